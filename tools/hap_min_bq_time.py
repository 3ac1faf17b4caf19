#!/usr/bin/env python3
"""What --hap_min_bq costs (c3r_load_reads_q, c3r_set_hap_min_bq: the upload of the qualities and k_mask_low_bq), and that it costs nothing
switched off, on the two contigs of tools/left_align_time.py: `phased` (MAS-Seq chr20 ~30x) and `stress` (16-Mb contig, loci at ~500x),
with the table of that tool — pass 1's heterozygous SNVs phased by Engine.phase_sites, as an SNV table and, every third site turned into an
insertion or deletion of 2 (haplotag_alleles_time.planted), as an allele table.  The qualities are uniform in 0 .. 40 (a fixed seed): the
kernel's time does not depend on their values.

    python tools/hap_min_bq_time.py [--commit ID] [--out profiles/hap_min_bq.txt] [--parent_root TREE] [--rounds 10] [--repeats 3] [--only phased,stress,resources]

Per contig one process prepares the reads, the qualities and the table.  Then FRESH PROCESSES take turns, `repeats` times each:
    parent    the tree of --parent_root (built there), where neither the qualities nor the switch exist
    off       this tree, reads without qualities, threshold 0: what every run without the flag does
    on        this tree, reads with qualities, threshold 10
A process warms up with two loads, then runs `rounds` rounds with profiling on — per table kind one load and one call each of the counts,
the links and the unit links: ms per launch of every kernel from kernel_stats (the mean of `rounds` launches) — then `rounds` loads with
profiling off (Engine.load_reads wall time: the median).
GATED: every kernel that the parent runs, and Engine.load_reads, switched off — the median of the off processes does not lie above the
parent's own spread [min, max] of the same run, widened by 2 % of the parent's median for the timer (a median below the spread is said,
and is no cost).  RECORDED, not gated: k_mask_low_bq in ms and as
a fraction of the HBM peak (8 TB/s) on 2 bytes per base (1 of quality and 1/2 of sequence read, 1/2 written); Engine.load_reads with
qualities and threshold 10 against without (the upload of one byte per base is the expected bulk of the difference); the device bytes held.
`resources` (no GPU needed): tools/kernel_resources.py for k_mask_low_bq."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("parent", "off", "on")
HBM_PEAK = 8.0e12
Q_ON = 10


def prepare(name, path):
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    from clair3_rna_amd import capi, synth
    title, gen, L = phase_time.LOADS[name]
    gen = dict(gen)
    L = L or synth.CHR20_LEN
    ref, rs, _ = synth.generate_contig(contig_len=L, seed=synth.SEED + gen.pop("seed_off"), **gen)
    eng = capi.Engine(0)
    eng.set_params()
    eng.load_reads(rs)
    sites, what = phase_time.pass1_candidates(eng, ref, L)
    out, _ = eng.phase_sites(sites)
    eng.close()
    table = np.ascontiguousarray(out[out["ps"] >= 0])
    qual = np.random.default_rng(7).integers(0, 41, 2 * len(rs.seq), dtype=np.uint8)
    odd = rs.reads[(rs.reads["l_seq"] & 1) == 1]
    qual[2 * odd["seq_off"].astype(np.int64) + odd["l_seq"].astype(np.int64)] = 0xff
    np.savez(path, reads=rs.reads, cigar=rs.cigar, seq=rs.seq, qual=qual, table=table)
    print(json.dumps(dict(title=title, n_reads=len(rs.reads), n_ops=len(rs.cigar), n_bases=int(rs.reads["l_seq"].sum(dtype=np.int64)), n_seq_bytes=len(rs.seq), what=what,
                          n_sites=len(table))))


def child(variant, root, path, rounds):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import haplotag_alleles_time                             # (it puts this tree first on the path: `root` goes in front of it afterwards)
    sys.path.insert(0, root)
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    z = np.load(path)
    on = variant == "on"
    rs = capi.pinned_readset(ReadSet(z["reads"], z["cigar"], z["seq"], z["qual"]) if on else ReadSet(z["reads"], z["cigar"], z["seq"]))
    table = z["table"]
    q, h1, pool, nb = haplotag_alleles_time.planted(table)
    units = table.copy()
    units["ps"] = 1 + (np.arange(len(table)) // 10) * 10
    aunits = q.copy()
    aunits["ps"] = 1 + (np.arange(len(q)) // 10) * 10
    eng = capi.Engine(0)
    eng.set_params(channels=30)
    if on:
        eng.set_hap_min_bq(Q_ON)
    eng.set_phase_sites(table)
    for _ in range(2):
        eng.load_reads(rs)
    eng.synchronize()
    eng.set_profiling(True)
    eng.reset_kernel_stats()
    for _ in range(rounds):
        eng.set_phase_sites(table)
        eng.load_reads(rs)
        eng.hap_counts(table)
        eng.phase_links(table)
        eng.phase_unit_links(units)
        eng.set_phase_alleles(q, h1, pool, nb)
        eng.load_reads(rs)
        eng.hap_allele_counts(q, pool)
        eng.phase_allele_links(q, pool, nb)
        eng.phase_allele_unit_links(aunits, h1, pool, nb)
    eng.synchronize()
    ks = eng.kernel_stats()
    eng.set_profiling(False)
    eng.set_phase_sites(table)
    wall = []
    for _ in range(rounds):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.load_reads(rs)
        eng.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    masked = eng.hap_min_bq()[1] if on else 0
    eng.close()
    assert ("k_mask_low_bq" in ks) == on, sorted(ks)
    print(json.dumps(dict(kernels={k: v["total_ms"] / v["launches"] for k, v in ks.items() if v["launches"] and v["total_ms"] > 0}, wall_ms=float(np.median(wall)),
                          masked=int(masked))))


def run(args, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit, check=True).stdout
    return json.loads(out.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_min_bq.txt"))
    ap.add_argument("--parent_root", default=None, help="the parent commit's tree, built; without it only off and on are measured and nothing is gated")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="phased,stress,resources")
    ap.add_argument("--prepare", nargs=2, metavar=("NAME", "ARCHIVE"), help=argparse.SUPPRESS)
    ap.add_argument("--child", nargs=3, metavar=("VARIANT", "ROOT", "ARCHIVE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.prepare:
        return prepare(*a.prepare)
    if a.child:
        return child(a.child[0], a.child[1], a.child[2], a.rounds)
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")

    commit = a.commit or phase_time.commit_id()
    variants = [v for v in VARIANTS if v != "parent" or a.parent_root]
    only = [n for n in a.only.split(",") if n]
    broken = []
    if only != ["resources"]:
        emit(["== hap_min_bq_time: commit %s, %d rounds a process, %d fresh processes a variant, taking turns%s"
              % (commit, a.rounds, a.repeats, "" if a.parent_root else " (no --parent_root: the parent commit is not measured, nothing is gated)")])
    with tempfile.TemporaryDirectory() as tmp:
        for name in only:
            if name == "resources":
                table = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "mask_low_bq"], stdout=subprocess.PIPE, text=True, check=True).stdout
                emit(["== compiled, commit %s (tools/kernel_resources.py 'mask_low_bq': hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage)" % commit]
                     + ["   " + ln for ln in table.rstrip("\n").split("\n")])
                continue
            path = os.path.join(tmp, name + ".npz")
            info = run(["--prepare", name, path], 900)
            emit(["-- %s (%s): %d reads, %d CIGAR ops, %d bases in %d sequence bytes; table: %d sites (%s, phased by Engine.phase_sites; as an allele table every third an "
                  "insertion or deletion of 2)" % (name, info["title"], info["n_reads"], info["n_ops"], info["n_bases"], info["n_seq_bytes"], info["n_sites"], info["what"])])
            got = {v: [] for v in variants}
            for _ in range(a.repeats):
                for v in variants:
                    got[v].append(run(["--child", v, a.parent_root if v == "parent" else ROOT, path, "--rounds", str(a.rounds)], 600))
                    print("[%s: %s measured]" % (name, v), file=sys.stderr, flush=True)
            base = "parent" if a.parent_root else "off"
            rows = [(k, lambda g, k=k: g["kernels"].get(k)) for k in sorted(got[base][0]["kernels"])] + [("Engine.load_reads wall (median of %d)" % a.rounds, lambda g: g["wall_ms"])]
            for label, pick in rows:
                vals = {v: [pick(g) for g in got[v]] for v in variants}
                for v in variants:
                    if None not in vals[v]:
                        emit(["   %-7s %-44s ms: %s" % (v, label, " ".join("%.4f" % x for x in vals[v]))])
                if a.parent_root and None not in vals["off"]:
                    lo, hi, med = min(vals["parent"]), max(vals["parent"]), float(np.median(vals["parent"]))
                    off_med = float(np.median(vals["off"]))
                    ok = off_med <= hi + 0.02 * med
                    emit(["           %-44s off median %.4f against the parent's %.4f .. %.4f: %s" % (label, off_med, lo, hi, "ABOVE" if not ok else "below" if off_med < lo else "inside")])
                    if not ok:
                        broken.append((name, label))
            ms = [g["kernels"]["k_mask_low_bq"] for g in got["on"]]
            moved = 2.0 * info["n_bases"]
            emit(["   on      k_mask_low_bq: %s ms per launch; %d of %d bases masked at threshold %d; %.0f MB moved (2 bytes per base): %.1f %% of the HBM peak (8 TB/s) at the median"
                  % (" ".join("%.4f" % x for x in ms), got["on"][0]["masked"], info["n_bases"], Q_ON, moved / 1e6, 100.0 * moved / (1e-3 * float(np.median(ms))) / HBM_PEAK),
                  "   on      device bytes held beside the parent's: %d for the qualities, %d for the masked copy" % (2 * info["n_seq_bytes"] + 32, info["n_seq_bytes"] + 16),
                  "   on      Engine.load_reads with qualities and threshold %d: median %.3f ms against %.3f ms without (%d bytes of qualities uploaded)"
                  % (Q_ON, float(np.median([g["wall_ms"] for g in got["on"]])), float(np.median([g["wall_ms"] for g in got["off"]])), 2 * info["n_seq_bytes"])])
    if a.parent_root and only != ["resources"]:
        emit(["-- gate (switched off, every kernel the parent runs and Engine.load_reads not above the parent's spread): %s" % ("HOLDS" if not broken else "BROKEN for %s" % broken)])
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
