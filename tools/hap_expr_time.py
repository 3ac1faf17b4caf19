#!/usr/bin/env python3
"""What the haplotype-resolved region counts cost (c3r_hap_region_counts / k_hap_region_counts) beside the kernels that read the same records
once.

    python tools/hap_expr_time.py [--commit ID] [--out profiles/hap_expression.txt] [--rounds 10] [--only phased,stress]

The loads are tools/hapcount_time.py's (`phased`: MAS-Seq chr20 ~30x; `stress`: loci at ~500x), and so are the phase table (the chain's, from
pass 1's own heterozygous SNVs) and the query of k_hap_counts.  The generator hands out no annotation, so the BED is read back from what it
expressed: the exons are the merged stretches under the reads' M / = / X / D ops, the genes the merged spans of the reads, both without a
strand; a region's rows are hap_expr's (the distinct sets of the table's sites inside it).  One fresh process per load.

Per load, written to --out (appended):
    k_hap_region_counts on the exons + genes, on the exons alone and on the genes alone, beside k_hap_counts and k_haplotag of the same
    process                                                            ms per launch (profiling on; mean over the rounds)
    Engine.hap_region_counts wall time beside Engine.load_reads       ms, median and min .. max (profiling off)"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def merged(start, end):
    """Sorted disjoint intervals [(start, end)] covering the same positions as the given ones (touching ones are joined)."""
    order = np.argsort(start, kind="stable")
    s, e = start[order], np.maximum.accumulate(end[order])
    first = np.ones(len(s), bool)
    first[1:] = s[1:] > e[:-1]
    at = np.flatnonzero(first)
    return list(zip(s[at].tolist(), e[np.append(at[1:] - 1, len(s) - 1)].tolist()))


def annotation(rs):
    """(exons, genes) of a ReadSet: merged M / D stretches, merged read spans; 0-based half-open."""
    cig = np.asarray(rs.cigar)
    op, ln = (cig & 15).astype(np.int64), (cig >> 4).astype(np.int64)
    n_cig = rs.reads["n_cigar"].astype(np.int64)
    owner = np.repeat(np.arange(len(rs.reads)), n_cig)
    consumes = np.isin(op, (0, 2, 3, 7, 8))
    cr = np.cumsum(np.where(consumes, ln, 0))
    first = rs.reads["cigar_off"].astype(np.int64)
    base = np.where(first > 0, cr[np.maximum(first - 1, 0)], 0)
    op_end = rs.reads["pos"].astype(np.int64)[owner] + cr - base[owner]
    covers = np.isin(op, (0, 2, 7, 8)) & (ln > 0)
    exons = merged((op_end - ln)[covers], op_end[covers])
    last = first + n_cig - 1
    has = n_cig > 0
    genes = merged(rs.reads["pos"].astype(np.int64)[has], (rs.reads["pos"].astype(np.int64)[has] + cr[last[has]] - base[has]))
    return exons, genes


def time_load(name, rounds):
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
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
    lines = ["-- %s (%s): %d reads, %d CIGAR ops; %s" % (name, title, len(rs.reads), len(rs.cigar), what)]
    out, st = eng.phase_sites(sites) if len(sites) else (sites, dict(n_phased=0))
    if not st["n_phased"]:
        eng.close()
        return lines + ["   no phased sites: nothing to time"]
    table = np.ascontiguousarray(out[out["ps"] >= 0])
    query = hap_vcf.nearest_sets(sites, table)
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    exons, genes = annotation(rs)
    tables = {}
    for label, regs in (("exons + genes", exons + genes), ("exons", exons), ("genes", genes)):
        tab, row_ps, _ = hap_expr.region_table([(a, b, ".", None) for a, b in regs], table["pos"], table["ps"])
        tables[label] = (tab, row_ps)
        rc, wc = eng.hap_region_counts(tab, row_ps)          # (first use: buffers)
        lines.append("   %-13s: %d regions, %d rows, max_j (j - first_open[j]) = %d; counts: untagged %d, other set %d, hp1 %d, hp2 %d"
                     % (label, len(tab), len(row_ps), hap_expr.max_back(tab), rc[:, 0].sum(), rc[:, 1].sum(), wc[:, 0].sum(), wc[:, 1].sum()))
    eng.hap_counts(query)
    eng.set_profiling(True)
    kern = {}
    for label, (tab, row_ps) in tables.items():
        for _ in range(rounds):
            eng.reset_kernel_stats()
            if label == "exons + genes":
                eng.load_reads(rs)                           # under the table: k_prep_count, k_haplotag, k_prep_write
                eng.hap_counts(query)
            eng.hap_region_counts(tab, row_ps)
            for k, v in eng.kernel_stats().items():
                kern.setdefault(k if k != "k_hap_region_counts" else "k_hap_region_counts (%s)" % label, []).append(v["total_ms"] / max(1, v["launches"]))
    eng.set_profiling(False)
    lines.append("   kernels, ms per launch (profiling on, mean of %d; k_hap_counts on %d query sites): %s" % (
        rounds, len(query), "  ".join("%s %.4f" % (k, float(np.mean(kern[k]))) for k in
                                      ["k_hap_region_counts (%s)" % l for l in tables] + ["k_hap_counts", "k_haplotag", "k_prep_count", "k_prep_write"] if k in kern)))
    tab, row_ps = tables["exons + genes"]
    w_load, w_count = [], []
    for _ in range(rounds):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.load_reads(rs)
        eng.synchronize()
        w_load.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        eng.hap_region_counts(tab, row_ps)
        w_count.append(1e3 * (time.perf_counter() - t0))
    eng.close()
    lines.append("   Engine.load_reads          wall ms (profiling off, table set): %s" % phase_time.spread(w_load))
    lines.append("   Engine.hap_region_counts   wall ms (profiling off, exons + genes): %s" % phase_time.spread(w_count))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_expression.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", default="phased,stress")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("\n".join(time_load(a.child, a.rounds)), flush=True)
        return 0
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    emit(["== hap_expr_time: commit %s, %d rounds, one process per load" % (a.commit or phase_time.commit_id(), a.rounds)])
    for name in a.only.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(a.rounds)], stdout=subprocess.PIPE, text=True, timeout=540)
        emit([l for l in r.stdout.split("\n") if l.startswith(("--", "   "))] or ["-- %s: the child ended with %d and no line" % (name, r.returncode)])
        if r.returncode != 0:
            emit(["-- %s: the child ended with %d: stopped" % (name, r.returncode)])
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
