#!/usr/bin/env python3
"""What --hap_realign costs (c3r_set_hap_realign: the four _ra kernels beside the four they stand in for and beside their _la forms), by
the method of tools/left_align_time.py on its two contigs and its table: `phased` (MAS-Seq chr20 ~30x) and `stress` (16-Mb contig, loci at
~500x); pass 1's heterozygous SNVs phased by Engine.phase_sites, every third site turned into an insertion or deletion of 2 behind its
anchor (haplotag_alleles_time.planted).

    python tools/realign_time.py [--commit ID] [--out profiles/realign.txt] [--parent_root TREE] [--rounds 10] [--repeats 3] [--overhang 10] [--only phased,stress,resources]

Per contig one process prepares the reads, the reference and the table.  Then FRESH PROCESSES take turns, `repeats` times each:
    parent    the tree of --parent_root (built there), where the switch does not exist
    off       this tree, both switches off
    la        this tree, --left_align_indels' switch on (the table left-aligned)
    ra        this tree, --hap_realign's switch on with --overhang
A process warms up with two loads, then times `rounds` loads with profiling on — ms per launch of the tagging kernel — and one call each
of hap_allele_counts, phase_allele_links and phase_allele_unit_links per round (ms per launch from kernel_stats), then `rounds` loads with
profiling off (Engine.load_reads wall time: the median).  GATE, switched off: the median of the three processes of every kernel and of
Engine.load_reads must not lie above the parent's maximum plus 2 % of the parent's median of the same run (exit status 1 otherwise).  The
switched-on cost is recorded, not gated.  `resources` (no GPU needed): tools/kernel_resources.py for the twelve kernels."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("parent", "off", "la", "ra")
SUFFIX = dict(parent="", off="", la="_la", ra="_ra")
KERNELS = ("k_haplotag_alleles", "k_hap_allele_counts", "k_phase_allele_links", "k_phase_allele_unit_links")


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
    np.savez(path, reads=rs.reads, cigar=rs.cigar, seq=rs.seq, table=table, ref=np.frombuffer(ref.encode() if isinstance(ref, str) else bytes(ref), dtype=np.uint8))
    print(json.dumps(dict(title=title, n_reads=len(rs.reads), n_ops=len(rs.cigar), what=what, n_sites=len(table))))


def child(variant, root, path, rounds, overhang):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import haplotag_alleles_time                             # (it puts this tree first on the path: `root` goes in front of it afterwards)
    sys.path.insert(0, root)
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    z = np.load(path)
    rs = capi.pinned_readset(ReadSet(z["reads"], z["cigar"], z["seq"]))
    q, h1, pool, nb = haplotag_alleles_time.planted(z["table"])
    on = variant == "la"
    suffix = SUFFIX[variant]
    eng = capi.Engine(0)
    eng.set_params(channels=30)
    if on:
        eng.set_reference(1, z["ref"])
        q, pool, nb, src, _ = capi.hap_left_align_sites(q, pool, 1, z["ref"], nb)
        h1 = np.ascontiguousarray(h1[src])
        eng.set_hap_left_align(True)
    if variant == "ra":
        eng.set_reference(1, z["ref"])
        eng.set_hap_realign(overhang)
    eng.set_phase_alleles(q, h1, pool, nb)
    units = q.copy()
    units["ps"] = 1 + (np.arange(len(q)) // 10) * 10                            # (units of ten table sites, as tools/phase_allele_time.py cuts them)
    for _ in range(2):
        eng.load_reads(rs)
    eng.synchronize()
    eng.set_profiling(True)
    eng.reset_kernel_stats()
    for _ in range(rounds):
        eng.load_reads(rs)
        eng.hap_allele_counts(q, pool)
        eng.phase_allele_links(q, pool, nb)
        eng.phase_allele_unit_links(units, h1, pool, nb)
    eng.synchronize()
    ks = eng.kernel_stats()
    eng.set_profiling(False)
    wall = []
    for _ in range(rounds):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.load_reads(rs)
        eng.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    eng.close()
    assert not [k for k in KERNELS for x in ("", "_la", "_ra") if x != suffix and k + x in ks], sorted(ks)
    print(json.dumps(dict(kernels={k: ks[k + suffix]["total_ms"] / ks[k + suffix]["launches"] for k in KERNELS}, wall_ms=float(np.median(wall)), n_sites=len(q))))


def run(args, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit, check=True).stdout
    return json.loads(out.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "realign.txt"))
    ap.add_argument("--parent_root", default=None, help="the parent commit's tree, built; without it only off and on are measured")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--overhang", type=int, default=10)
    ap.add_argument("--only", default="phased,stress,resources")
    ap.add_argument("--prepare", nargs=2, metavar=("NAME", "ARCHIVE"), help=argparse.SUPPRESS)
    ap.add_argument("--child", nargs=3, metavar=("VARIANT", "ROOT", "ARCHIVE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.prepare:
        return prepare(*a.prepare)
    if a.child:
        return child(a.child[0], a.child[1], a.child[2], a.rounds, a.overhang)
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
    if only != ["resources"]:
        emit(["== realign_time: commit %s, overhang %d, %d rounds a process, %d fresh processes a variant, taking turns%s"
              % (commit, a.overhang, a.rounds, a.repeats, "" if a.parent_root else " (no --parent_root: the parent commit is not measured)")])
    failed = False
    with tempfile.TemporaryDirectory() as tmp:
        for name in only:
            if name == "resources":
                table = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "allele"], stdout=subprocess.PIPE, text=True, check=True).stdout
                emit(["== compiled, commit %s (tools/kernel_resources.py 'allele': hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage)" % commit]
                     + ["   " + ln for ln in table.rstrip("\n").split("\n")])
                continue
            path = os.path.join(tmp, name + ".npz")
            info = run(["--prepare", name, path], 900)
            emit(["-- %s (%s): %d reads, %d CIGAR ops; table: %d sites (%s, phased by Engine.phase_sites; every third an insertion or deletion of 2)"
                  % (name, info["title"], info["n_reads"], info["n_ops"], info["n_sites"], info["what"])])
            got = {v: [] for v in variants}
            for _ in range(a.repeats):
                for v in variants:
                    got[v].append(run(["--child", v, a.parent_root if v == "parent" else ROOT, path, "--rounds", str(a.rounds), "--overhang", str(a.overhang)], 600))
            for k in KERNELS:
                for v in variants:
                    emit(["   %-7s %-32s ms per launch: %s" % (v, k + SUFFIX[v], " ".join("%.4f" % g["kernels"][k] for g in got[v]))])
            for v in variants:
                emit(["   %-7s Engine.load_reads wall ms (median of %d): %s   (table: %d sites)"
                      % (v, a.rounds, " ".join("%.3f" % g["wall_ms"] for g in got[v]), got[v][0]["n_sites"])])
            if "parent" in got:                              # the gate: switched off against the parent's own spread of this run
                for what, pick in [(k, (lambda g, k=k: g["kernels"][k])) for k in KERNELS] + [("Engine.load_reads", lambda g: g["wall_ms"])]:
                    par, off = sorted(pick(g) for g in got["parent"]), sorted(pick(g) for g in got["off"])
                    limit = par[-1] + 0.02 * par[len(par) // 2]
                    ok = off[len(off) // 2] <= limit
                    failed = failed or not ok
                    emit(["   gate    %-32s off median %.4f, parent max + 2 %% of its median %.4f: %s" % (what, off[len(off) // 2], limit, "inside" if ok else "ABOVE")])
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
