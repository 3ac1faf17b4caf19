#!/usr/bin/env python3
"""What haplotagging on the device costs a c3r_load_reads, on the contig of BASELINE.json configs[3] (synthetic PacBio MAS-Seq chr20 ~30x,
phased — bench.py's phased_1gpu input).

    python tools/haplotag_time.py [--commit ID] [--out profiles/haplotag_time.txt] [--contig_len N] [--rounds 20]

Phase sites: one per kb over the contig, the reference base as `ref` (positions whose reference base is not A, C, G or T are left out), a
random `alt`, a random h1, phase sets in blocks of 20 sites.  After a warm-up, `rounds` load_reads calls with the table set and `rounds`
without, alternating, with profiling on (every kernel bracketed by events); the same again with profiling off for the wall time of a load
as a caller sees it.  Between the two modes an empty read set is loaded, so that switching the table rebuilds nothing.

Written to --out (a section of its own: the file may already hold the bench.py series of the path without sites):
    k_haplotag, k_prep_count, k_prep_write   ms per load (mean over the rounds), from kernel_stats()
    load_reads wall time                      ms, median and min .. max, both modes, profiling on and off
The kernel reads what k_prep<false> reads, once: the expectation is k_haplotag <= k_prep_count in the same run."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_sites(ref, seed=1, every=1000, block=20):
    from clair3_rna_amd.capi import PHASE_SITE_DTYPE
    rng = np.random.RandomState(seed)
    pos = np.arange(every // 2, len(ref), every, dtype=np.int64)                 # 1-based
    base = np.frombuffer(ref, dtype=np.uint8)[pos - 1] & 0xdf                    # upper case
    code = np.zeros(256, np.uint8)
    for ch, c in zip(b"ACGT", (1, 2, 4, 8)):
        code[ch] = c
    rc = code[base]
    keep = rc > 0
    pos, rc = pos[keep], rc[keep]
    shift = rng.randint(1, 4, size=len(pos))
    ac = np.array([1, 2, 4, 8], np.uint8)[(np.log2(rc).astype(np.int64) + shift) % 4]
    a = np.zeros(len(pos), dtype=PHASE_SITE_DTYPE)
    a["pos"], a["ref"], a["alt"], a["h1"] = pos, rc, ac, rng.randint(0, 2, size=len(pos))
    a["ps"] = pos[(np.arange(len(pos)) // block) * block]                         # a block's number: the position of its first site
    return a


def commit_id():
    try:
        h = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "status", "--porcelain"], cwd=ROOT, stdout=subprocess.PIPE, text=True).stdout.strip()
        return h + ("+uncommitted changes" if dirty else "")
    except Exception:          # noqa: BLE001
        return "unknown"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haplotag_time.txt"))
    ap.add_argument("--contig_len", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    from clair3_rna_amd import capi, synth
    from clair3_rna_amd.reads import ReadSet
    L = a.contig_len or synth.CHR20_LEN
    ref, rs, info = synth.generate_contig(contig_len=L, seed=synth.SEED + 3, depth=30.0, platform="hifi", phased=True)
    rs = capi.pinned_readset(rs)
    sites = make_sites(ref)
    empty = ReadSet.from_records([])
    eng = capi.Engine(0)
    eng.set_params(channels=30)

    def one(with_sites):
        eng.load_reads(empty)
        eng.set_phase_sites(sites if with_sites else None)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.load_reads(rs)
        eng.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(3):
        one(True), one(False)
    eng.set_phase_sites(sites)
    eng.load_reads(rs)
    st = eng.haplotags()[1]
    res = {}
    for prof in (True, False):
        eng.set_profiling(prof)
        wall = {True: [], False: []}
        kern = {True: {}, False: {}}
        for _ in range(a.rounds):
            for mode in (True, False):
                eng.reset_kernel_stats()
                wall[mode].append(one(mode))
                if prof:
                    for k, v in eng.kernel_stats().items():
                        kern[mode][k] = kern[mode].get(k, 0.0) + v["total_ms"]
        res[prof] = (wall, kern)
    eng.set_profiling(False)
    eng.close()

    def spread(v):
        return "median %.3f  min %.3f  max %.3f" % (float(np.median(v)), min(v), max(v))
    lines = ["== haplotag_time: commit %s" % (a.commit or commit_id()),
             "input: synth.generate_contig(contig_len=%d, seed=SEED+3, depth=30, platform=hifi, phased=True): %d reads, %d CIGAR ops, %.1f MB of bases" % (L, len(rs.reads), len(rs.cigar), len(rs.seq) / 1e6),
             "phase sites: %d (one per kb, phase sets of 20 sites); tags: %s" % (len(sites), st),
             "%d load_reads calls per mode, alternating, after 3 warm-up pairs" % a.rounds,
             "kernel times, ms per load (profiling on; mean of %d):" % a.rounds]
    wall, kern = res[True]
    for mode, name in ((True, "with sites"), (False, "without  ")):
        ks = kern[mode]
        lines.append("  %s  k_haplotag %s  k_prep_count %.4f  k_prep_write %.4f  k_prefmax_bins %.4f  k_bin_scan %.4f" % (
            name, "%.4f" % (ks["k_haplotag"] / a.rounds) if "k_haplotag" in ks else "  -   ", ks.get("k_prep_count", 0) / a.rounds, ks.get("k_prep_write", 0) / a.rounds,
            ks.get("k_prefmax_bins", 0) / a.rounds, ks.get("k_bin_scan", 0) / a.rounds))
    for prof in (True, False):
        wall = res[prof][0]
        lines.append("load_reads wall time, ms (profiling %s):" % ("on" if prof else "off"))
        lines.append("  with sites  %s" % spread(wall[True]))
        lines.append("  without     %s" % spread(wall[False]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
