#!/usr/bin/env python3
"""What the haplotagged-BAM step (clair3_rna_amd/haplotag_bam.py, call_sample --haplotagged_bam) costs per contig, on one MI355X, split
into its stages, on synthetic loads.

    python tools/haplotag_bam_time.py [--commit ID] [--out profiles/haplotag_bam.txt] [--rounds 3] [--only phased,stress] [--threads 1,16]
                                      [--contig_len N]

The loads are tools/phase_time.py's (`phased`: BASELINE.json configs[3], MAS-Seq chr20 ~30x; `stress`: configs[4], loci at ~500x), written
to an indexed BAM by the test writer (clair3_rna_amd/bam.py: no qualities worth the name, one short name per read — a real BAM carries
more bytes per record); the phase table is tools/haplotag_time.py's (one site per kb, sets of 20 sites).  Per load and per thread count
(--threads: BGZF inflate threads of the handle and deflate threads of the writer, both), `rounds` times after one warm-up:

    fetch        BamFile.fetch(ctg): the whole contig's read records
    load         Engine.set_phase_sites + Engine.load_reads + synchronize (k_haplotag runs here)
    read-back    Engine.haplotags() + Engine.read_phase_sets()
    write        BamFile.write_haplotagged -> <ctg>.bam       (inflate, strip / append aux fields, deflate)
    index        bamio.index_build -> <ctg>.bam.bai

and the input's compressed megabytes per second of the write alone and of the whole step.  Medians, with min .. max.  No target: this is
the first measurement.  Synthetic loads only — no real data, and no comparison with `whatshap haplotag` + `samtools index`."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STAGES = ("fetch", "load", "read-back", "write", "index")


def measure(name, threads_list, rounds, contig_len, tmp):
    from haplotag_time import make_sites
    from phase_time import LOADS
    from clair3_rna_amd import bam, bamio, capi, synth
    title, gen, L = LOADS[name]
    gen = dict(gen)
    L = contig_len or L or synth.CHR20_LEN
    t0 = time.perf_counter()
    ref, rs, _info = synth.generate_contig(contig_len=L, seed=synth.SEED + gen.pop("seed_off"), **gen)
    print("[%s] %d reads generated in %.0f s" % (name, len(rs), time.perf_counter() - t0), flush=True)
    bam_fn = os.path.join(tmp, name + ".bam")
    t0 = time.perf_counter()
    bam.write_bam(bam_fn, [("chr20", L)], {"chr20": rs})
    bamio.index_build(bam_fn)
    in_mb = os.path.getsize(bam_fn) / 1e6
    print("[%s] input BAM of %.1f MB written and indexed in %.0f s" % (name, in_mb, time.perf_counter() - t0), flush=True)
    sites = make_sites(ref)
    del ref, rs
    eng = capi.Engine(0)
    eng.set_params()
    out = os.path.join(tmp, name + ".tagged.bam")
    lines = ["load %s: %s; %d-base contig, input BAM %.1f MB compressed, %d phase sites" % (name, title, L, in_mb, len(sites))]
    try:
        for T in threads_list:
            t = {s: [] for s in STAGES}
            st = tags = None
            for r in range(rounds + 1):
                with bamio.BamFile(bam_fn, threads=T) as bf:
                    c0 = time.perf_counter()
                    reads = bf.fetch("chr20")
                    c1 = time.perf_counter()
                    eng.set_phase_sites(sites)
                    eng.load_reads(reads)
                    eng.synchronize()
                    c2 = time.perf_counter()
                    hp, tags = eng.haplotags()
                    ps = eng.read_phase_sets()
                    c3 = time.perf_counter()
                    st = bf.write_haplotagged("chr20", out, reads, hp, ps, pg_line="@PG\tID:c3r_haplotag\tPN:clair3_rna_amd", threads=T)
                    c4 = time.perf_counter()
                bamio.index_build(out)
                c5 = time.perf_counter()
                if r:                                            # (round 0 warms the page cache and the context's buffers)
                    for s, d in zip(STAGES, (c1 - c0, c2 - c1, c3 - c2, c4 - c3, c5 - c4)):
                        t[s].append(d)
                print("[%s] threads %d round %d: %.2f s" % (name, T, r, c5 - c0), flush=True)
            out_mb = os.path.getsize(out) / 1e6
            med = {s: float(np.median(t[s])) for s in STAGES}
            total = sum(med.values())
            lines.append("  threads %2d: %d records, %d HP1, %d HP2, %d untagged -> %.1f MB" % (T, st["records"], tags["n_hp1"], tags["n_hp2"], st["records"] - st["tagged"], out_mb))
            for s in STAGES:
                lines.append("    %-10s median %8.3f s   min %8.3f   max %8.3f" % (s, med[s], min(t[s]), max(t[s])))
            lines.append("    %-10s        %8.3f s   (sum of the medians)" % ("step", total))
            lines.append("    input compressed MB/s: write alone %.1f, whole step %.1f" % (in_mb / med["write"], in_mb / total))
    finally:
        eng.close()
        for fn in (bam_fn, bam_fn + ".bai", out, out + ".bai"):
            if os.path.exists(fn):
                os.remove(fn)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haplotag_bam.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="phased,stress")
    ap.add_argument("--threads", default="1,16", help="thread counts, comma-separated (given, never taken from the machine's CPU count)")
    ap.add_argument("--contig_len", type=int, default=0, help="shorter contigs for a trial run")
    a = ap.parse_args()
    from haplotag_time import commit_id
    threads = [int(x) for x in a.threads.split(",")]
    lines = ["== haplotag_bam_time: commit %s" % (a.commit or commit_id()),
             "stages of the haplotagged-BAM step per contig, seconds, %d rounds after one warm-up; synthetic loads, one MI355X; no real data, no comparison with whatshap" % a.rounds]
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.only.split(","):
            lines += measure(name, threads, a.rounds, a.contig_len, tmp)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
