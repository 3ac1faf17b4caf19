#!/usr/bin/env python3
"""What --hap_realign_spliced costs on top of --hap_realign (c3r_set_hap_realign_spliced: the five _rs kernels beside their _ra siblings),
on the two contigs and the table of tools/realign_time.py: `phased` (MAS-Seq chr20 ~30x) and `stress` (16-Mb contig, loci at ~500x); pass
1's heterozygous SNVs phased by Engine.phase_sites, every third site turned into an insertion or deletion of 2 behind its anchor.  The
loads carry the generator's own N ops: the reads are spliced as the generator splices them.

    python tools/realign_spliced_time.py [--commit ID] [--out profiles/realign_spliced.txt] [--parent_root TREE] [--rounds 10] [--repeats 3] [--overhang 10] [--only phased,stress,resources]

Per contig one process prepares the reads, the reference and the table.  Then `repeats` FRESH PROCESSES each measure BOTH forms, the _ra
kernels first and the _rs kernels behind them: a process warms up with two loads per form, then times `rounds` loads with profiling on —
ms per launch of the tagging kernel — and one call each of hap_allele_counts, phase_allele_links and phase_allele_unit_links per round (ms
per launch from kernel_stats); the _w tagger likewise under c3r_set_hap_bq_weights with a quality of 30 on every base.  Then `rounds`
loads per form with profiling off (Engine.load_reads wall time: the median).  The _rs figures are recorded, not gated: the switch is opt-in.
GATE, with --parent_root (the parent commit's tree, built, where the switch does not exist): fresh processes of that tree measure ITS _ra
kernels and its load by its own tools/realign_time.py, taking turns with this tree's processes, and the median of this tree's three
processes of every _ra kernel and of Engine.load_reads under the overhang must not lie above the parent's maximum plus 2 % of the parent's
median of the same run (exit status 1 otherwise); the gate on the paths with both switches off is tools/realign_time.py's.  `resources` (no GPU needed): tools/kernel_resources.py for the _ra and _rs kernels."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = (("ra", False), ("rs", True))
KERNELS = ("k_haplotag_alleles", "k_hap_allele_counts", "k_phase_allele_links", "k_phase_allele_unit_links")


def child(path, rounds, overhang):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import haplotag_alleles_time                             # (it puts this tree first on the path)
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    z = np.load(path)
    plain = ReadSet(z["reads"], z["cigar"], z["seq"])
    n_spliced = int(sum(1 for i in range(len(plain.reads)) if (plain.cigar[int(plain.reads[i]["cigar_off"]):int(plain.reads[i]["cigar_off"]) + int(plain.reads[i]["n_cigar"])] & 15 == 3).any()))
    rs = capi.pinned_readset(plain)
    rsq = capi.pinned_readset(ReadSet(z["reads"], z["cigar"], z["seq"], np.full(2 * len(z["seq"]), 30, np.uint8)))
    q, h1, pool, nb = haplotag_alleles_time.planted(z["table"])
    units = q.copy()
    units["ps"] = 1 + (np.arange(len(q)) // 10) * 10                            # (units of ten table sites, as tools/phase_allele_time.py cuts them)
    eng = capi.Engine(0)
    eng.set_params(channels=30)
    eng.set_reference(1, z["ref"])
    eng.set_hap_realign(overhang)
    eng.set_phase_alleles(q, h1, pool, nb)
    out = dict(n_sites=len(q), n_reads=len(plain.reads), n_spliced=n_spliced)
    for name, spliced in FORMS:
        suffix = "_" + name
        eng.set_hap_bq_weights(False)
        eng.set_hap_realign_spliced(spliced)
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
        assert not [k for k in KERNELS for x in ("", "_la", "_ra", "_rs") if x != suffix and k + x in ks], sorted(ks)
        got = {k + suffix: ks[k + suffix]["total_ms"] / ks[k + suffix]["launches"] for k in KERNELS}
        eng.set_profiling(False)
        wall = []
        for _ in range(rounds):
            eng.synchronize()
            t0 = time.perf_counter()
            eng.load_reads(rs)
            eng.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        # the _w tagger: the same reads with qualities
        eng.load_reads(rsq)
        eng.set_hap_bq_weights(True)
        for _ in range(2):
            eng.load_reads(rsq)
        eng.synchronize()
        eng.set_profiling(True)
        eng.reset_kernel_stats()
        for _ in range(rounds):
            eng.load_reads(rsq)
        eng.synchronize()
        ks = eng.kernel_stats()
        eng.set_profiling(False)
        k = "k_haplotag_alleles" + suffix + "_w"
        got[k] = ks[k]["total_ms"] / ks[k]["launches"]
        eng.set_hap_bq_weights(False)
        out[name] = dict(kernels=got, wall_ms=float(np.median(wall)))
    eng.close()
    print(json.dumps(out))


def run(args, limit):
    out = subprocess.run([sys.executable] + args, stdout=subprocess.PIPE, text=True, timeout=limit, check=True).stdout
    return json.loads(out.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "realign_spliced.txt"))
    ap.add_argument("--parent_root", default=None, help="the parent commit's tree, built; without it the _ra kernels are not gated")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--overhang", type=int, default=10)
    ap.add_argument("--only", default="phased,stress,resources")
    ap.add_argument("--child", metavar="ARCHIVE", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rounds, a.overhang)
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import phase_time
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")

    commit = a.commit or phase_time.commit_id()
    only = [n for n in a.only.split(",") if n]
    if only != ["resources"]:
        emit(["== realign_spliced_time: commit %s, overhang %d, %d rounds a form, %d fresh processes, each measuring the _ra kernels and then the _rs kernels%s"
              % (commit, a.overhang, a.rounds, a.repeats, ", taking turns with processes of the parent commit's tree" if a.parent_root else " (no --parent_root: the _ra kernels are not gated)")])
    failed = False
    with tempfile.TemporaryDirectory() as tmp:
        for name in only:
            if name == "resources":
                table = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "_r[as](_w)?$"], stdout=subprocess.PIPE, text=True, check=True).stdout
                emit(["== compiled, commit %s (tools/kernel_resources.py '_r[as](_w)?$': hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage)" % commit]
                     + ["   " + ln for ln in table.rstrip("\n").split("\n")])
                continue
            path = os.path.join(tmp, name + ".npz")
            info = run([os.path.join(ROOT, "tools", "realign_time.py"), "--prepare", name, path], 900)
            got, par = [], []
            for _ in range(a.repeats):
                if a.parent_root:
                    par.append(run([os.path.join(a.parent_root, "tools", "realign_time.py"), "--child", "ra", a.parent_root, path, "--rounds", str(a.rounds), "--overhang", str(a.overhang)], 900))
                got.append(run([os.path.abspath(__file__), "--child", path, "--rounds", str(a.rounds), "--overhang", str(a.overhang)], 900))
            emit(["-- %s (%s): %d reads, %d of them with an N op, %d CIGAR ops; table: %d sites (%s, phased by Engine.phase_sites; every third an insertion or deletion of 2)"
                  % (name, info["title"], info["n_reads"], got[0]["n_spliced"], info["n_ops"], got[0]["n_sites"], info["what"])])
            med = lambda xs: sorted(xs)[len(xs) // 2]
            for k in KERNELS + ("k_haplotag_alleles_w",):
                stem, w = (k[:-2], "_w") if k.endswith("_w") else (k, "")
                vals = {f: [g[f]["kernels"][stem + "_" + f + w] for g in got] for f, _ in FORMS}
                for f, _ in FORMS:
                    emit(["   %-34s ms per launch: %s" % (stem + "_" + f + w, " ".join("%.4f" % v for v in vals[f]))])
                emit(["   %-34s the _rs kernel takes %.2f times its _ra sibling's time (medians)" % ("", med(vals["rs"]) / med(vals["ra"]))])
            for f, _ in FORMS:
                emit(["   %-34s Engine.load_reads wall ms (median of %d): %s" % (f, a.rounds, " ".join("%.3f" % g[f]["wall_ms"] for g in got))])
            emit(["   %-34s Engine.load_reads under both switches takes %.2f times the load under the overhang alone (medians)"
                  % ("", med([g["rs"]["wall_ms"] for g in got]) / med([g["ra"]["wall_ms"] for g in got]))])
            if par:                                          # the gate: this tree's _ra kernels and load against the parent's own spread of this run
                for what, mine, theirs in [(k + "_ra", (lambda g, k=k: g["ra"]["kernels"][k + "_ra"]), (lambda g, k=k: g["kernels"][k])) for k in KERNELS] + [
                        ("Engine.load_reads (overhang)", lambda g: g["ra"]["wall_ms"], lambda g: g["wall_ms"])]:
                    p, m = sorted(theirs(g) for g in par), sorted(mine(g) for g in got)
                    limit = p[-1] + 0.02 * p[len(p) // 2]
                    ok = m[len(m) // 2] <= limit
                    failed = failed or not ok
                    emit(["   gate    %-32s parent: %s; this tree's median %.4f, parent max + 2 %% of its median %.4f: %s"
                          % (what, " ".join("%.4f" % v for v in p), m[len(m) // 2], limit, "inside" if ok else "ABOVE")])
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
