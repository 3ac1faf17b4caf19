#!/usr/bin/env python3
"""What the haplotype-resolved junction counts cost (c3r_hap_junction_counts / k_hap_junction_counts), counted in LDS first and directly,
beside the kernels that read the same records once.

    python tools/hap_junctions_time.py [--commit ID] [--out profiles/hap_junctions.txt] [--rounds 10] [--procs 3] [--only phased,stress]

The loads are tools/hapcount_time.py's (`phased`: MAS-Seq chr20 ~30x; `stress`: loci at ~500x), and so are the phase table (the chain's,
from pass 1's own heterozygous SNVs) and the query of k_hap_counts; the regions of k_hap_region_counts are tools/hap_expr_time.py's exons +
genes.  --procs fresh processes per load, one after the other; every process times both variants of the kernel on the same reads.

Per load, written to --out (appended):
    distinct junctions, rows, reads per junction (the adds that meet on one `reads` word without aggregation: mean and largest), and the
    launches one call takes at the default slots_hint (1: no grow-and-repeat round)
    k_hap_junction_counts (LDS stage) and k_hap_junction_counts_direct beside k_hap_region_counts, k_hap_counts and k_haplotag
                                                                       ms per launch (profiling on; mean over the rounds), per process,
                                                                       then the mean and the spread (max - min) across the processes
    Engine.hap_junction_counts wall time (both variants) beside Engine.load_reads   ms, median and min .. max (profiling off), per process"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_hap_junction_counts", "k_hap_junction_counts_direct", "k_hap_region_counts", "k_hap_counts", "k_haplotag"]


def time_load(name, rounds):
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import hap_expr_time
    import phase_time
    from clair3_rna_amd import capi, hap_expr, hap_vcf, synth
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
    table = np.ascontiguousarray(out[out["ps"] >= 0]) if st["n_phased"] else None
    if table is not None:
        eng.set_phase_sites(table)
        eng.load_reads(rs)
        query = hap_vcf.nearest_sets(sites, table)
        exons, genes = hap_expr_time.annotation(rs)
        tab, row_ps, _ = hap_expr.region_table([(a, b, ".", None) for a, b in exons + genes], table["pos"], table["ps"])
        eng.hap_counts(query)                                # (first use: buffers)
        eng.hap_region_counts(tab, row_ps)
    else:
        res["head"] += "; no phased sites: every read is untagged, k_hap_counts and k_hap_region_counts are not timed"
    got = {}
    for direct in (False, True):
        eng.set_hap_junction_direct(direct)
        got[direct] = eng.hap_junction_counts()              # (first use: buffers)
    assert all(got[False][k].tobytes() == got[True][k].tobytes() for k in (0, 1)), "the two variants differ"
    j, r = got[False]
    res.update(junctions=len(j), rows=len(r), reads_mean=float(j["reads"].mean()) if len(j) else 0.0, reads_max=int(j["reads"].max()) if len(j) else 0,
               untagged=int(j["untagged"].sum()), hp1=int(r["hp1"].sum()), hp2=int(r["hp2"].sum()))
    eng.set_profiling(True)
    kern, launches = {}, {}
    for _ in range(rounds):
        eng.reset_kernel_stats()
        eng.load_reads(rs)                                   # under the table: k_prep_count, k_haplotag, k_prep_write
        if table is not None:
            eng.hap_counts(query)
            eng.hap_region_counts(tab, row_ps)
        for direct in (False, True):
            eng.set_hap_junction_direct(direct)
            eng.hap_junction_counts()
        for k, v in eng.kernel_stats().items():
            kern.setdefault(k, []).append(v["total_ms"] / max(1, v["launches"]))
            launches[k] = v["launches"]
    eng.set_profiling(False)
    res["kernel_ms"] = {k: float(np.mean(kern[k])) for k in KERNELS if k in kern}
    res["launches_per_call"] = {k: launches[k] for k in KERNELS[:2]}
    wall = {"load_reads": [], "aggregated": [], "direct": []}
    for _ in range(rounds):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.load_reads(rs)
        eng.synchronize()
        wall["load_reads"].append(1e3 * (time.perf_counter() - t0))
        for direct in (False, True):
            eng.set_hap_junction_direct(direct)
            t0 = time.perf_counter()
            eng.hap_junction_counts()
            wall["direct" if direct else "aggregated"].append(1e3 * (time.perf_counter() - t0))
    eng.close()
    res["wall"] = {k: phase_time.spread(v) for k, v in wall.items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_junctions.txt"))
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
    emit(["== hap_junctions_time: commit %s, %d rounds, %d fresh processes per load" % (a.commit or phase_time.commit_id(), a.rounds, a.procs)])
    for name in a.only.split(","):
        runs = []
        for p in range(a.procs):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(a.rounds)], stdout=subprocess.PIPE, text=True, timeout=540)
            hit = [l for l in r.stdout.split("\n") if l.startswith("RESULT ")]
            if r.returncode != 0 or not hit:
                emit(["-- %s: process %d ended with %d and no result: stopped" % (name, p, r.returncode)])
                return 1
            res = json.loads(hit[-1][7:])
            if not runs:
                emit([res["head"],
                      "   %d distinct junctions, %d rows; reads per junction: mean %.1f, largest %d; untagged %d, hp1 %d, hp2 %d"
                      % (res["junctions"], res["rows"], res["reads_mean"], res["reads_max"], res["untagged"], res["hp1"], res["hp2"]),
                      "   launches per call at the default slots_hint: %s" % "  ".join("%s %d" % kv for kv in res["launches_per_call"].items())])
            emit(["   process %d: kernels, ms per launch (profiling on, mean of %d): %s" % (p, a.rounds, "  ".join("%s %.4f" % (k, res["kernel_ms"][k]) for k in KERNELS if k in res["kernel_ms"])),
                  "   process %d: wall ms (profiling off): Engine.load_reads %s | Engine.hap_junction_counts %s | the same, direct %s"
                  % (p, res["wall"]["load_reads"], res["wall"]["aggregated"], res["wall"]["direct"])])
            runs.append(res)
        for k in KERNELS:
            v = [r["kernel_ms"][k] for r in runs if k in r["kernel_ms"]]
            if v:
                emit(["   %-30s mean of the processes %.4f ms, spread (max - min) %.4f" % (k, float(np.mean(v)), max(v) - min(v))])
    return 0


if __name__ == "__main__":
    sys.exit(main())
