#!/usr/bin/env python3
"""What the built-in phasing costs (c3r_phase_links / k_phase_links, c3r_phase_resolve) beside the kernels that read the same records once,
and how often its greedy chain switches against the generator's truth.

    python tools/phase_time.py [--commit ID] [--out profiles/phase_links.txt] [--rounds 10] [--only phased,stress,deep,switch] [--merge_levels 4]

Three loads, the inputs of bench.py's additional figures:
    phased   BASELINE.json configs[3]: synthetic PacBio MAS-Seq chr20 ~30x
    stress   configs[4]: 16-Mb contig, expressed loci at ~500x
    deep     one 400-kb contig with loci at ~20,000x (mpileup's depth cap does not apply to the voters: every kept read adds)
Candidates: pass 1's own heterozygous SNVs — the contig goes through the 18-channel tensor build and the network (synth.random_weights: no
trained model is at hand, so which sites are called 0/1 is arbitrary; their number and spacing are what the timing depends on), and the rows
are read as phasing.candidates_from_vcf reads them.  Fewer than 100 of them: every biallelic SNV row instead, and the output says so.

Per load, written to --out (appended):
    k_phase_links beside k_haplotag and k_prep_count   ms (profiling on; mean over the rounds) — the two yardsticks read the same records once
    Engine.phase_sites wall time                       ms, median and min .. max (profiling off): upload, clear, kernel, read-back, resolve
    Engine.load_reads wall time                        ms, the same way: what `deep` is weighed against
    the block-merge stage (--merge_levels, default 4; 0 leaves it out), level by level until one joins nothing:
        units and units joined; walks per voting read, a histogram the host counts from unit_of (a read whose sites in range lie in P
        units walks its CIGAR once when P <= 1 and P + 1 times otherwise — an upper bound: a unit none of whose sites the read observes
        costs no walk); k_phase_unit_links ms per launch (profiling on) beside k_phase_links on the same reads in the same run, its
        yardstick; Engine.phase_unit_links wall ms (profiling off); and the kernel once more on the chain's table with every phased site
        made a unit of its own, the bound of the walks
and once:
    switch errors of phase_sites against tests/phaseref.gen_case(errors=True)'s truth, eight seeds."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOADS = {
    "phased": ("BASELINE.json configs[3]: MAS-Seq chr20 ~30x", dict(seed_off=3, depth=30.0, platform="hifi", phased=True), None),
    "stress": ("configs[4]: 16-Mb contig, loci at ~500x", dict(seed_off=4, depth=500.0), 16000000),
    "deep": ("400-kb contig, loci at ~20,000x", dict(seed_off=5, depth=20000.0, expressed_frac=0.01, intron_lo=100.0, intron_hi=800.0), 400000),
}


def commit_id():
    try:
        h = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "status", "--porcelain"], cwd=ROOT, stdout=subprocess.PIPE, text=True).stdout.strip()
        return h + ("+uncommitted changes" if dirty else "")
    except Exception:          # noqa: BLE001
        return "unknown"


def pass1_candidates(eng, ref, L):
    """(candidate table, what it holds) from the 18-channel pass over the loaded reads."""
    import bench
    from clair3_rna_amd import phasing, synth
    eng.set_reference(1, ref)
    eng.load_weights(synth.random_weights(18), 18)
    eng.begin_batch()
    eng.scan_regions(bench.chunk_list(L))
    eng.end_batch()
    eng.infer(fetch=False)
    text, _ = eng.call_rows_text("ctg", qual=None, show_ref=False)
    rows = text.decode().split("\n")
    per = phasing._parse(rows, "ctg")
    sites, skipped = phasing._table(*per["ctg"])
    what = "pass 1's heterozygous SNVs"
    if len(sites) < 100:
        relaxed = []
        for r in rows:
            f = r.split("\t")
            if len(f) >= 10 and len(f[3]) == 1 and len(f[4]) == 1:
                f[6], f[8], f[9] = "PASS", "GT", "0/1"
                relaxed.append("\t".join(f))
        sites, skipped = phasing._table(*phasing._parse(relaxed, "ctg")["ctg"])
        what = "every biallelic SNV row of pass 1 (it called fewer than 100 of them 0/1)"
    return sites, "%d candidates: %s" % (len(sites), what)


def spread(v):
    return "median %.3f  min %.3f  max %.3f" % (float(np.median(v)), min(v), max(v))


def time_load(name, rounds, merge_levels=0):
    from clair3_rna_amd import capi, synth
    title, gen, L = LOADS[name]
    gen = dict(gen)
    L = L or synth.CHR20_LEN
    ref, rs, info = synth.generate_contig(contig_len=L, seed=synth.SEED + gen.pop("seed_off"), **gen)
    rs = capi.pinned_readset(rs)
    eng = capi.Engine(0)
    eng.set_params()
    eng.load_reads(rs)
    sites, what = pass1_candidates(eng, ref, L)
    lines = ["-- %s (%s): %d reads, %d CIGAR ops; %s" % (name, title, len(rs.reads), len(rs.cigar), what)]
    if not len(sites):
        eng.close()
        return lines + ["   no candidates: nothing to time"]
    out, st = eng.phase_sites(sites)
    lines.append("   phase_sites: %s" % st)
    table = out[out["ps"] >= 0] if st["n_phased"] else None
    # kernels, profiling on: one load under the phased table (k_haplotag runs), one phase_links
    eng.set_profiling(True)
    kern = {}
    for _ in range(rounds):
        eng.reset_kernel_stats()
        eng.set_phase_sites(None)
        eng.load_reads(rs)
        if table is not None:
            eng.set_phase_sites(table)                       # (tags the loaded reads: k_haplotag once more, with the rebuild of the tables)
        eng.phase_links(sites)
        for k, v in eng.kernel_stats().items():
            kern.setdefault(k, []).append(v["total_ms"] / max(1, v["launches"]))
    eng.set_profiling(False)
    eng.set_phase_sites(None)
    lines.append("   kernels, ms per launch (profiling on, mean of %d): %s" % (
        rounds, "  ".join("%s %.4f" % (k, float(np.mean(kern[k]))) for k in ("k_phase_links", "k_haplotag", "k_prep_count", "k_prep_write") if k in kern)))
    w_load, w_phase = [], []
    for _ in range(rounds):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.load_reads(rs)
        eng.synchronize()
        w_load.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        eng.phase_sites(sites)
        w_phase.append(1e3 * (time.perf_counter() - t0))
    lines.append("   Engine.load_reads  wall ms (profiling off): %s" % spread(w_load))
    lines.append("   Engine.phase_sites wall ms (profiling off): %s" % spread(w_phase))
    if merge_levels > 0:
        lines += merge_cost(eng, rs, out, rounds, merge_levels, float(np.mean(kern["k_phase_links"])))
    eng.close()
    return lines


def walks_histogram(rs, table, prm):
    """{walks: voting reads} for one k_phase_unit_links launch over `table`, from the host's copy of the records: the sites in the read's
    span [pos, end) and their units."""
    pos = table["pos"].astype(np.int64)
    units = np.unique(table["ps"][table["ps"] >= 0])
    unit_of = np.where(table["ps"] >= 0, np.searchsorted(units, table["ps"]), -1)
    r = rs.reads
    flag = r["flag"].astype(np.int64)
    votes = ((flag & int(prm["excl_flags"])) == 0) & ((flag & 4) == 0) & (((flag & 1) == 0) | ((flag & 2) != 0)) & (r["mapq"] >= int(prm["min_mq"]))
    ref_len = np.zeros(len(r), np.int64)
    ops, lens = rs.cigar & 15, (rs.cigar >> 4).astype(np.int64)
    consumes = np.isin(ops, (0, 2, 3, 7, 8)) * lens
    csum = np.concatenate([[0], np.cumsum(consumes)])
    off = r["cigar_off"].astype(np.int64)
    ref_len = csum[off + r["n_cigar"].astype(np.int64)] - csum[off]
    lo = np.searchsorted(pos, r["pos"].astype(np.int64) + 1)
    hi = np.searchsorted(pos, r["pos"].astype(np.int64) + ref_len + 1)
    hist = {}
    for i in np.nonzero(votes)[0]:
        if hi[i] - lo[i] < 2:
            w = 0
        else:
            u = unit_of[lo[i]:hi[i]]
            p = len(np.unique(u[u >= 0]))
            w = 1 if p <= 1 else p + 1
        hist[w] = hist.get(w, 0) + 1
    return hist


def merge_cost(eng, rs, chain, rounds, merge_levels, links_ms):
    from clair3_rna_amd import capi
    lines, table = [], chain
    prm = dict(min_mq=eng.params.min_mq, excl_flags=eng.params.excl_flags)
    for level in range(1, merge_levels + 1):
        n_units = len(np.unique(table["ps"][table["ps"] >= 0]))
        hist = walks_histogram(rs, table, prm)
        eng.set_profiling(True)
        eng.reset_kernel_stats()
        for _ in range(rounds):
            ul = eng.phase_unit_links(table)
        k = eng.kernel_stats().get("k_phase_unit_links")
        eng.set_profiling(False)
        wall = []
        for _ in range(rounds):
            eng.synchronize()
            t0 = time.perf_counter()
            eng.phase_unit_links(table)
            wall.append(1e3 * (time.perf_counter() - t0))
        table, st, joined = capi.phase_merge(table, ul)
        lines.append("   merge level %d: %d units, %d joined -> %d blocks; walks per voting read (walks: reads): %s" % (
            level, n_units, joined, st["n_blocks"], "  ".join("%d: %d" % kv for kv in sorted(hist.items()))))
        lines.append("      k_phase_unit_links ms per launch (profiling on, mean of %d): %s   [k_phase_links, same reads, same run: %.4f]" % (
            rounds, "%.4f" % (k["total_ms"] / k["launches"]) if k else "not launched (fewer than two units)", links_ms))
        lines.append("      Engine.phase_unit_links wall ms (profiling off): %s" % spread(wall))
        if joined == 0:
            break
    # the bound of the P + 1 walks: the chain's phased sites, every one a unit of its own
    worst = chain.copy()
    worst["ps"] = np.where(chain["ps"] >= 0, chain["pos"], -1)
    if int((worst["ps"] >= 0).sum()) >= 2:
        hist = walks_histogram(rs, worst, prm)
        eng.set_profiling(True)
        eng.reset_kernel_stats()
        for _ in range(rounds):
            eng.phase_unit_links(worst)
        k = eng.kernel_stats()["k_phase_unit_links"]
        eng.set_profiling(False)
        reads = sum(hist.values())
        lines.append("   every phased site a unit of its own (%d units; the bound of the walks: mean %.1f, most %d per voting read): k_phase_unit_links %.4f ms per launch" % (
            int((worst["ps"] >= 0).sum()), sum(w * c for w, c in hist.items()) / max(1, reads), max(hist), k["total_ms"] / k["launches"]))
    return lines


def switch_errors():
    from clair3_rna_amd import capi
    from tests import phaseref
    eng = capi.Engine(0)
    eng.set_params()
    tot = dict(sites=0, phased=0, blocks=0, pairs=0, switches=0)
    for seed in range(8):
        _, rs, sites, truth, _ = phaseref.gen_case(seed, errors=True)
        eng.load_reads(rs)
        out, st = eng.phase_sites(sites)
        rel = out["h1"] ^ truth
        for ps in set(out["ps"].tolist()) - {-1}:
            m = np.nonzero(out["ps"] == ps)[0]
            tot["pairs"] += len(m) - 1
            tot["switches"] += int((rel[m][1:] != rel[m][:-1]).sum())
        tot["sites"] += st["n_sites"]
        tot["phased"] += st["n_phased"]
        tot["blocks"] += st["n_blocks"]
    eng.close()
    return ["-- switch errors against the generator's truth, tests/phaseref.gen_case(seed, errors=True), seeds 0-7 (5 % substitutions, 1 % N, indels):",
            "   %(sites)d sites, %(phased)d phased in %(blocks)d blocks; %(switches)d switches in %(pairs)d pairs of neighbours inside a block" % tot
            + (" = %.2f %%" % (100.0 * tot["switches"] / tot["pairs"]) if tot["pairs"] else "")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_links.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--only", default="phased,stress,deep,switch")
    ap.add_argument("--merge_levels", type=int, default=4, help="levels of the block-merge stage to time after the chain (0: none)")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    emit(["== phase_time: commit %s, %d rounds" % (a.commit or commit_id(), a.rounds)])
    for name in a.only.split(","):
        emit(switch_errors() if name == "switch" else time_load(name, a.rounds, a.merge_levels))


if __name__ == "__main__":
    main()
