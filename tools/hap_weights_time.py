#!/usr/bin/env python3
"""What --hap_bq_weights costs (c3r_set_hap_bq_weights: the four _w tagging kernels), and that it costs nothing switched off, on the two
contigs and with the tables of tools/hap_min_bq_time.py and tools/realign_time.py: `phased` (MAS-Seq chr20 ~30x) and `stress` (16-Mb
contig, loci at ~500x); pass 1's heterozygous SNVs phased by Engine.phase_sites, as an SNV table and, every third site an insertion or
deletion of 2 (haplotag_alleles_time.planted), as an allele table; qualities uniform in 0 .. 40 (a fixed seed).

    python tools/hap_weights_time.py [--commit ID] [--out profiles/hap_weights.txt] [--parent_root TREE] [--rounds 10] [--repeats 3] [--overhang 10]
                                     [--only phased,stress,flagship]

Per contig one process prepares the reads, the qualities, the reference and the table.  Then FRESH PROCESSES take turns, `repeats` times
each, one per (tree, form):
    tree      parent   the tree of --parent_root (built there), where the switch does not exist
              off      this tree, reads without qualities, switch off: what every run without the flag does
              on       this tree, reads with qualities: per round the load under the switch AND the load without it, so that each _w kernel
                       stands beside its sibling in the same process
    form      plain    the SNV table (k_haplotag) and the allele table (k_haplotag_alleles)
              la       the allele table, left-aligned, under c3r_set_hap_left_align (k_haplotag_alleles_la)
              ra       the allele table under c3r_set_hap_realign(--overhang) (k_haplotag_alleles_ra)
A process warms up with two loads, then runs `rounds` rounds with profiling on — per table one load: ms per launch of every kernel from
kernel_stats (the mean of `rounds` launches) — then `rounds` loads with profiling off (Engine.load_reads wall time: the median).
GATED, per form: switched off, the tagging kernel, every other kernel of the load and Engine.load_reads — the median of the off processes
does not lie above the parent's maximum plus 2 % of its median.  RECORDED, not gated: each _w kernel beside its sibling, and
Engine.load_reads with qualities under the switch.
`flagship`: bench.py --gpus 1 --steps 10 --warmup 2 (it launches none of these kernels) of the parent's tree and of this tree, taking
turns, `repeats` times each: recorded."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = ("parent", "off", "on")
FORMS = ("plain", "la", "ra")
TAGGERS = dict(plain=("k_haplotag", "k_haplotag_alleles"), la=("k_haplotag_alleles_la",), ra=("k_haplotag_alleles_ra",))


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
    np.savez(path, reads=rs.reads, cigar=rs.cigar, seq=rs.seq, qual=qual, table=table, ref=np.frombuffer(ref.encode() if isinstance(ref, str) else bytes(ref), dtype=np.uint8))
    print(json.dumps(dict(title=title, n_reads=len(rs.reads), n_ops=len(rs.cigar), n_bases=int(rs.reads["l_seq"].sum(dtype=np.int64)), what=what, n_sites=len(table))))


def child(tree, form, root, path, rounds, overhang):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import haplotag_alleles_time                             # (it puts this tree first on the path: `root` goes in front of it afterwards)
    sys.path.insert(0, root)
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    z = np.load(path)
    on = tree == "on"
    rs = capi.pinned_readset(ReadSet(z["reads"], z["cigar"], z["seq"], z["qual"]) if on else ReadSet(z["reads"], z["cigar"], z["seq"]))
    table = z["table"]
    q, h1, pool, nb = haplotag_alleles_time.planted(table)
    eng = capi.Engine(0)
    eng.set_params(channels=30)
    if form != "plain":
        eng.set_reference(1, z["ref"])
    if form == "la":
        q, pool, nb, src, _ = capi.hap_left_align_sites(q, pool, 1, z["ref"], nb)
        h1 = np.ascontiguousarray(h1[src])
        eng.set_hap_left_align(True)
    if form == "ra":
        eng.set_hap_realign(overhang)

    def tables():                                            # each table of the form, set before its load
        if form == "plain":
            yield lambda: eng.set_phase_sites(table)
        yield lambda: eng.set_phase_alleles(q, h1, pool, nb)
    for set_table in tables():
        set_table()
    for _ in range(2):
        eng.load_reads(rs)
    eng.synchronize()
    eng.set_profiling(True)
    eng.reset_kernel_stats()
    for _ in range(rounds):
        for weights in ((False, True) if on else (False,)):
            if on:
                eng.set_hap_bq_weights(weights)
            for set_table in tables():
                set_table()
                eng.load_reads(rs)
    eng.synchronize()
    ks = eng.kernel_stats()
    eng.set_profiling(False)
    if on:
        eng.set_hap_bq_weights(True)
    wall = []
    for _ in range(rounds):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.load_reads(rs)
        eng.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    eng.close()
    for k in TAGGERS[form]:
        assert k in ks and ((k + "_w") in ks) == on, sorted(ks)
    print(json.dumps(dict(kernels={k: v["total_ms"] / v["launches"] for k, v in ks.items() if v["launches"] and v["total_ms"] > 0}, wall_ms=float(np.median(wall)))))


def run(args, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit, check=True).stdout
    return json.loads(out.strip().split("\n")[-1])


def bench(root):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True,
                         timeout=300, check=True).stdout
    d = json.loads(out.strip().split("\n")[-1])
    return d["value"], d["ms_per_step"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_weights.txt"))
    ap.add_argument("--parent_root", default=None, help="the parent commit's tree, built; without it only off and on are measured and nothing is gated")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--overhang", type=int, default=10)
    ap.add_argument("--only", default="phased,stress,flagship")
    ap.add_argument("--prepare", nargs=2, metavar=("NAME", "ARCHIVE"), help=argparse.SUPPRESS)
    ap.add_argument("--child", nargs=4, metavar=("TREE", "FORM", "ROOT", "ARCHIVE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.prepare:
        return prepare(*a.prepare)
    if a.child:
        return child(a.child[0], a.child[1], a.child[2], a.child[3], a.rounds, a.overhang)
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")

    commit = a.commit or phase_time.commit_id()
    parent_root = os.path.abspath(a.parent_root) if a.parent_root else None
    trees = [t for t in TREES if t != "parent" or parent_root]
    broken = []
    emit(["== hap_weights_time: commit %s, overhang %d, %d rounds a process, %d fresh processes a (tree, form), taking turns%s"
          % (commit, a.overhang, a.rounds, a.repeats, "" if parent_root else " (no --parent_root: the parent commit is not measured, nothing is gated)")])
    with tempfile.TemporaryDirectory() as tmp:
        for name in [n for n in a.only.split(",") if n]:
            if name == "flagship":
                roots = ([("parent", parent_root)] if parent_root else []) + [("this", ROOT)]
                got = {k: [] for k, _ in roots}
                for _ in range(a.repeats):
                    for k, root in roots:
                        got[k].append(bench(root))
                emit(["-- flagship (bench.py --gpus 1 --steps 10 --warmup 2, which launches none of these kernels; the trees taking turns, %d runs each)" % a.repeats]
                     + ["   %-7s sites/s: %s   ms per step: %s" % (k, " ".join("%.0f" % v for v, _ in got[k]), " ".join("%.3f" % m for _, m in got[k])) for k, _ in roots])
                continue
            path = os.path.join(tmp, name + ".npz")
            info = run(["--prepare", name, path], 900)
            emit(["-- %s (%s): %d reads, %d CIGAR ops, %d bases; table: %d sites (%s, phased by Engine.phase_sites; as an allele table every third an insertion or deletion of 2)"
                  % (name, info["title"], info["n_reads"], info["n_ops"], info["n_bases"], info["n_sites"], info["what"])])
            got = {(t, f): [] for t in trees for f in FORMS}
            for _ in range(a.repeats):
                for f in FORMS:
                    for t in trees:
                        got[(t, f)].append(run(["--child", t, f, parent_root if t == "parent" else ROOT, path, "--rounds", str(a.rounds), "--overhang", str(a.overhang)], 600))
                        print("[%s: %s %s measured]" % (name, t, f), file=sys.stderr, flush=True)
            for f in FORMS:
                base = "parent" if parent_root else "off"
                rows = [(k, lambda g, k=k: g["kernels"].get(k)) for k in sorted(got[(base, f)][0]["kernels"])] + [("Engine.load_reads wall (median of %d)" % a.rounds, lambda g: g["wall_ms"])]
                for label, pick in rows:
                    vals = {t: [pick(g) for g in got[(t, f)]] for t in trees}
                    for t in trees:
                        if None not in vals[t]:
                            emit(["   %-5s %-7s %-44s ms: %s" % (f, t, label, " ".join("%.4f" % x for x in vals[t]))])
                    if parent_root and None not in vals["off"]:
                        limit = max(vals["parent"]) + 0.02 * float(np.median(vals["parent"]))
                        off_med = float(np.median(vals["off"]))
                        ok = off_med <= limit
                        emit(["   %-5s gate    %-44s off median %.4f, parent max + 2 %% of its median %.4f: %s" % (f, label, off_med, limit, "not above" if ok else "ABOVE")])
                        if not ok:
                            broken.append((name, f, label))
                for sib in TAGGERS[f]:
                    ms_w, ms_s = [g["kernels"][sib + "_w"] for g in got[("on", f)]], [g["kernels"][sib] for g in got[("on", f)]]
                    emit(["   %-5s on      %-26s %s ms per launch beside %-24s %s in the same processes: %.2f x at the medians"
                          % (f, sib + "_w", " ".join("%.4f" % x for x in ms_w), sib, " ".join("%.4f" % x for x in ms_s), float(np.median(ms_w)) / float(np.median(ms_s)))])
                emit(["   %-5s on      Engine.load_reads with qualities under the switch: median %.3f ms against %.3f ms without qualities, switch off"
                      % (f, float(np.median([g["wall_ms"] for g in got[("on", f)]])), float(np.median([g["wall_ms"] for g in got[("off", f)]])))])
    if parent_root and set(a.only.split(",")) - {"flagship"}:
        emit(["-- gate (switched off, per form: every kernel of the load that the parent runs and Engine.load_reads not above the parent's maximum plus 2 %% of its median): %s"
              % ("HOLDS" if not broken else "BROKEN for %s" % broken)])
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())
