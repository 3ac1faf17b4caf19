#!/usr/bin/env python3
"""What the per-haplotype allele counts cost (c3r_hap_counts / k_hap_counts) beside the kernels that read the same records once, and what
the extra store of the read's phase set costs k_haplotag.

    python tools/hapcount_time.py [--commit ID] [--out profiles/hap_counts.txt] [--rounds 10] [--only phased,stress] [--parent_root DIR [--ab_loads phased,stress]]

The loads are tools/phase_time.py's (`phased`: BASELINE.json configs[3], MAS-Seq chr20 ~30x; `stress`: configs[4], loci at ~500x; `deep`:
loci at ~20,000x, not in the default list), and so are the candidates: pass 1's own heterozygous SNVs through synth.random_weights.  The
phase table is what the chain (Engine.phase_sites) makes of them; the query sites are ALL candidates, each with the set of the nearest
table site (hap_vcf.nearest_sets) — what hap_vcf asks.

Per load, written to --out (appended):
    k_hap_counts beside k_phase_links, k_haplotag and k_prep_count   ms per launch (profiling on; mean over the rounds), same reads, same run
    Engine.hap_counts wall time beside Engine.load_reads              ms, median and min .. max (profiling off)
--parent_root DIR: a built tree of the parent commit.  k_haplotag is then timed in child processes that alternate between this tree and
that one (three of each), every child on the same reads under the same table (saved by this process): the extra store against the
run-to-run spread."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def haplotag_child(root, name, table_fn, rounds):
    """One process: k_haplotag ms per launch over `rounds` loads of `name` under the saved table, with the package of `root`."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import phase_time                                        # (puts this tree first on the path: `root` goes before it afterwards)
    sys.path.insert(0, os.path.abspath(root))
    from clair3_rna_amd import capi, synth
    assert os.path.abspath(capi.__file__).startswith(os.path.abspath(root) + os.sep), capi.__file__
    _title, gen, L = phase_time.LOADS[name]
    gen = dict(gen)
    L = L or synth.CHR20_LEN
    _ref, rs, _info = synth.generate_contig(contig_len=L, seed=synth.SEED + gen.pop("seed_off"), **gen)
    rs = capi.pinned_readset(rs)
    eng = capi.Engine(0)
    eng.set_params()
    eng.set_phase_sites(np.load(table_fn))
    eng.load_reads(rs)                                       # (first use: buffers)
    eng.set_profiling(True)
    ms = []
    for _ in range(rounds):
        eng.reset_kernel_stats()
        eng.load_reads(rs)
        eng.synchronize()
        k = eng.kernel_stats()["k_haplotag"]
        ms.append(k["total_ms"] / k["launches"])
    eng.close()
    print("HAPLOTAG_MS %s" % " ".join("%.4f" % v for v in ms), flush=True)


def time_load(name, rounds, parent_root, scratch):
    """The lines of one load; parent_root None: no A/B of k_haplotag."""
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    from clair3_rna_amd import capi, hap_vcf, synth
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
    counts = eng.hap_counts(query)
    _, ast = capi.hap_assign(query, counts)
    lines.append("   table: %d sites in %d sets; %d query sites; observations by row (none, hp1, hp2): %s; hap_assign: %s"
                 % (len(table), len(set(table["ps"].tolist())), len(query), counts.sum(axis=(0, 2)).tolist(), ast))
    eng.set_profiling(True)
    kern = {}
    for _ in range(rounds):
        eng.reset_kernel_stats()
        eng.load_reads(rs)                                   # under the table: k_prep_count, k_haplotag, k_prep_write
        eng.phase_links(sites)
        eng.hap_counts(query)
        for k, v in eng.kernel_stats().items():
            kern.setdefault(k, []).append(v["total_ms"] / max(1, v["launches"]))
    eng.set_profiling(False)
    lines.append("   kernels, ms per launch (profiling on, mean of %d): %s" % (
        rounds, "  ".join("%s %.4f" % (k, float(np.mean(kern[k]))) for k in ("k_hap_counts", "k_phase_links", "k_haplotag", "k_prep_count", "k_prep_write") if k in kern)))
    w_load, w_count = [], []
    for _ in range(rounds):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.load_reads(rs)
        eng.synchronize()
        w_load.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        eng.hap_counts(query)
        w_count.append(1e3 * (time.perf_counter() - t0))
    eng.close()
    lines.append("   Engine.load_reads  wall ms (profiling off, table set): %s" % phase_time.spread(w_load))
    lines.append("   Engine.hap_counts  wall ms (profiling off): %s" % phase_time.spread(w_count))
    if parent_root:
        os.makedirs(scratch, exist_ok=True)
        table_fn = os.path.join(scratch, "hapcount_table_%s.npy" % name)
        np.save(table_fn, table)
        runs = {"this": [], "parent": []}
        for k in range(6):                                   # this, parent, this, parent, ...: fresh processes, one at a time
            who = "this" if k % 2 == 0 else "parent"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--haplotag_child", ROOT if who == "this" else parent_root, "--only", name,
                                "--table", table_fn, "--rounds", str(rounds)], stdout=subprocess.PIPE, text=True, timeout=300)
            got = [l for l in r.stdout.split("\n") if l.startswith("HAPLOTAG_MS ")]
            if r.returncode != 0 or not got:
                lines.append("   k_haplotag A/B: the %s child ended with %d: stopped" % (who, r.returncode))
                break
            runs[who].append(float(np.mean([float(v) for v in got[0].split()[1:]])))
        lines.append("   k_haplotag ms per launch, alternating processes (mean of %d loads each): this commit %s | parent commit %s" % (
            rounds, " ".join("%.4f" % v for v in runs["this"]), " ".join("%.4f" % v for v in runs["parent"])))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_counts.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", default="phased,stress")
    ap.add_argument("--parent_root", default=None, help="a built tree of the parent commit: k_haplotag there against here")
    ap.add_argument("--ab_loads", default="phased,stress", help="the loads on which k_haplotag is timed against --parent_root")
    ap.add_argument("--scratch", default=None, help="where the table of the A/B children is kept (default: a fresh temporary directory)")
    ap.add_argument("--haplotag_child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--table", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.haplotag_child:
        return haplotag_child(a.haplotag_child, a.only, a.table, a.rounds)
    if a.scratch is None:
        import tempfile
        a.scratch = tempfile.mkdtemp(prefix="hapcount_time_")
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    emit(["== hapcount_time: commit %s, %d rounds" % (a.commit or phase_time.commit_id(), a.rounds)])
    for name in a.only.split(","):
        emit(time_load(name, a.rounds, a.parent_root if name in a.ab_loads.split(",") else None, a.scratch))


if __name__ == "__main__":
    main()
