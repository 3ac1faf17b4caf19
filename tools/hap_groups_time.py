#!/usr/bin/env python3
"""What the gene-level haplotype counts cost (c3r_hap_group_counts / k_hap_group_counts), counted in LDS first and directly, beside
k_hap_region_counts on the same exons and on the per-gene spans.

    python tools/hap_groups_time.py [--commit ID] [--out profiles/hap_groups.txt] [--rounds 10] [--procs 3] [--only phased,stress]

The loads are tools/hap_expr_time.py's (`phased`: synthetic MAS-Seq chr20 ~30x; `stress`: loci at ~500x) with its annotation: the exons are
the merged M / D stretches of the reads, the genes the merged read spans, and every exon is named by the gene it lies in — the table of
c3r_hap_group_counts.  --procs fresh processes per load, one after the other; every process times all four launches on the same reads.

Per load, written to --out (appended):
    intervals, groups, rows; the counted (read, gene) pairs beside the (read, exon) pairs of the exon table
    k_hap_group_counts (LDS stage), k_hap_group_counts_direct, k_hap_region_counts on the exon table and on the per-gene spans
                                                                       ms per launch (profiling on; mean over the rounds), per process,
                                                                       then the mean and the spread (max - min) across the processes
    Engine.hap_group_counts wall time (both variants)                  ms, median and min .. max (profiling off), per process
and whether the aggregated variant beats the direct one by more than the direct one's spread."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_hap_group_counts", "k_hap_group_counts_direct", "k_hap_region_counts (exons)", "k_hap_region_counts (gene spans)"]


def time_load(name, rounds):
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import hap_expr_time
    import phase_time
    from clair3_rna_amd import capi, hap_expr, synth
    title, gen, L = phase_time.LOADS[name]
    gen = dict(gen)
    L = L or synth.CHR20_LEN
    ref, rs, _info = synth.generate_contig(contig_len=L, seed=synth.SEED + gen.pop("seed_off"), **gen)
    rs = capi.pinned_readset(rs)
    eng = capi.Engine(0)
    eng.set_params()
    eng.load_reads(rs)
    sites, what = phase_time.pass1_candidates(eng, ref, L)
    res = dict(head="-- %s (%s): %d reads, %d CIGAR ops; %s" % (name, title, len(rs.reads), len(rs.cigar), what))
    out, st = eng.phase_sites(sites) if len(sites) else (sites, dict(n_phased=0))
    if not st["n_phased"]:
        res["head"] += "; no phased sites: nothing to time"
        return res
    table = np.ascontiguousarray(out[out["ps"] >= 0])
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    exons, genes = hap_expr_time.annotation(rs)
    gene_start = np.array([g[0] for g in genes])
    groups = [(".", None, []) for _ in genes]
    for a, b in exons:
        groups[int(np.searchsorted(gene_start, a, "right")) - 1][2].append((a, b))
    assert all(g[2] for g in groups)
    gtab, goff, grow_ps = hap_expr.group_table(groups, table["pos"], table["ps"])
    etab, erow_ps, _ = hap_expr.region_table([(a, b, ".", None) for a, b in exons], table["pos"], table["ps"])
    stab, srow_ps, _ = hap_expr.region_table([(a, b, ".", None) for a, b in genes], table["pos"], table["ps"])
    got = {}
    for direct in (False, True):
        eng.set_hap_group_direct(direct)
        got[direct] = eng.hap_group_counts(gtab, len(groups), goff, grow_ps)      # (first use: buffers)
    assert all(got[False][k].tobytes() == got[True][k].tobytes() for k in (0, 1)), "the two variants differ"
    by_exon, by_span = eng.hap_region_counts(etab, erow_ps), eng.hap_region_counts(stab, srow_ps)
    res.update(intervals=len(gtab), groups=len(groups), rows=len(grow_ps), gene_pairs=int(got[False][0].sum()) + int(got[False][1].sum()),
               exon_pairs=int(by_exon[0].sum()) + int(by_exon[1].sum()), span_pairs=int(by_span[0].sum()) + int(by_span[1].sum()))
    eng.set_profiling(True)
    kern = {k: [] for k in KERNELS}

    def one(label, kernel, call):
        eng.reset_kernel_stats()
        call()
        v = eng.kernel_stats()[kernel]
        kern[label].append(v["total_ms"] / max(1, v["launches"]))

    for _ in range(rounds):
        for direct in (False, True):
            eng.set_hap_group_direct(direct)
            one(KERNELS[1 if direct else 0], "k_hap_group_counts_direct" if direct else "k_hap_group_counts", lambda: eng.hap_group_counts(gtab, len(groups), goff, grow_ps))
        one(KERNELS[2], "k_hap_region_counts", lambda: eng.hap_region_counts(etab, erow_ps))
        one(KERNELS[3], "k_hap_region_counts", lambda: eng.hap_region_counts(stab, srow_ps))
    eng.set_profiling(False)
    res["kernel_ms"] = {k: float(np.mean(v)) for k, v in kern.items()}
    wall = {"aggregated": [], "direct": []}
    for _ in range(rounds):
        for direct in (False, True):
            eng.set_hap_group_direct(direct)
            eng.synchronize()
            t0 = time.perf_counter()
            eng.hap_group_counts(gtab, len(groups), goff, grow_ps)
            wall["direct" if direct else "aggregated"].append(1e3 * (time.perf_counter() - t0))
    eng.close()
    res["wall"] = {k: phase_time.spread(v) for k, v in wall.items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_groups.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--only", default="phased,stress")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(time_load(a.child, a.rounds)), flush=True)
        return 0
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    emit(["== hap_groups_time: commit %s, %d rounds, %d fresh processes per load" % (a.commit or phase_time.commit_id(), a.rounds, a.procs)])
    for name in a.only.split(","):
        runs = []
        for p in range(a.procs):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(a.rounds)], stdout=subprocess.PIPE, text=True, timeout=400)
            hit = [l for l in r.stdout.split("\n") if l.startswith("RESULT ")]
            if r.returncode != 0 or not hit:
                emit(["-- %s: process %d ended with %d and no result: stopped" % (name, p, r.returncode)])
                return 1
            res = json.loads(hit[-1][7:])
            if "kernel_ms" not in res:
                emit([res["head"]])
                break
            if not runs:
                emit([res["head"],
                      "   %d exons in %d genes, %d rows; (read, gene) pairs %d; (read, exon) pairs of the exon table %d; (read, span) pairs of the per-gene spans %d"
                      % (res["intervals"], res["groups"], res["rows"], res["gene_pairs"], res["exon_pairs"], res["span_pairs"])])
            emit(["   process %d: kernels, ms per launch (profiling on, mean of %d): %s" % (p, a.rounds, "  ".join("%s %.4f" % (k, res["kernel_ms"][k]) for k in KERNELS)),
                  "   process %d: wall ms (profiling off): Engine.hap_group_counts %s | the same, direct %s" % (p, res["wall"]["aggregated"], res["wall"]["direct"])])
            runs.append(res)
        if not runs:
            continue
        stat = {}
        for k in KERNELS:
            v = [r["kernel_ms"][k] for r in runs]
            stat[k] = (float(np.mean(v)), max(v) - min(v))
            emit(["   %-36s mean of the processes %.4f ms, spread (max - min) %.4f" % (k, stat[k][0], stat[k][1])])
        gain = stat[KERNELS[1]][0] - stat[KERNELS[0]][0]
        emit(["   aggregated against direct: %.4f ms less, the direct variant's spread is %.4f: %s"
              % (gain, stat[KERNELS[1]][1], "the aggregation wins here" if gain > stat[KERNELS[1]][1] else "the aggregation does NOT win here")])
    return 0


if __name__ == "__main__":
    sys.exit(main())
