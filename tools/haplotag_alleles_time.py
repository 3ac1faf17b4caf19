#!/usr/bin/env python3
"""What k_haplotag_alleles (c3r_set_phase_alleles: a phase table with indels and two-ALT sites) costs beside k_haplotag (c3r_set_phase_sites),
on the two contigs of tools/phase_time.py: `phased` (BASELINE.json configs[3]: MAS-Seq chr20 ~30x) and `stress` (16-Mb contig, loci at ~500x).

    python tools/haplotag_alleles_time.py [--commit ID] [--out profiles/haplotag_alleles.txt] [--rounds 10] [--repeats 3] [--only phased,stress,resources]

Per contig one process prepares the input — the reads, and the table: pass 1's heterozygous SNVs phased by Engine.phase_sites — and leaves it
in a temporary archive.  Then FRESH PROCESSES take turns, `repeats` times each, one variant a process:
    snv       Engine.set_phase_sites(table)                                     -> k_haplotag
    alleles   Engine.set_phase_alleles(the same table as REF-and-one-SNV sites)  -> k_haplotag_alleles on an SNV-only table
    planted   the same with every third site turned into an insertion of 2 or a deletion of 2 behind its anchor (event_matters = 1: the walk
              reads the op behind every M op that ends on such a site; the reads do not carry these alleles, so they show allele A)
A process warms up with two loads, then times `rounds` loads with profiling on (ms per launch of the tagging kernel, from kernel_stats) and
`rounds` with profiling off (Engine.load_reads wall time as a caller sees it: the MEDIAN of the `rounds` wall times).  `resources` (needs
no GPU: `--only resources` appends it on a machine without one) is what tools/kernel_resources.py reports for the tagging and counting
kernels of this tree.  The parent commit's k_haplotag figure for the same contigs and table stands in profiles/hap_counts.txt
(hapcount_time); the tool does not read it."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

VARIANTS = ("snv", "alleles", "planted")
KERNEL = dict(snv="k_haplotag", alleles="k_haplotag_alleles", planted="k_haplotag_alleles")


def prepare(name, path):
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
    out, st = eng.phase_sites(sites)
    eng.close()
    table = np.ascontiguousarray(out[out["ps"] >= 0])
    np.savez(path, reads=rs.reads, cigar=rs.cigar, seq=rs.seq, table=table)
    print(json.dumps(dict(title=title, n_reads=len(rs.reads), n_ops=len(rs.cigar), what=what, n_sites=len(table), n_sets=len(set(table["ps"].tolist())))))


def planted(table):
    """(HAP_SITE_DTYPE sites, h1, packed pool, bases): every third site's allele B becomes an insertion of 2 (GT) or a deletion of 2 behind the
    site's REF base; allele A stays the REF base."""
    from clair3_rna_amd import capi
    q = capi.hap_sites_from_snvs(table)
    pool = []
    for k in range(0, len(q), 3):
        q["base_matters"][k], q["event_matters"][k], q["b_base"][k], q["b_len"][k] = 0, 1, q["a_base"][k], 2
        if (k // 3) % 2:
            q["b_kind"][k] = capi.HAP_EV_DEL
        else:
            q["b_kind"][k], q["b_ins_off"][k] = capi.HAP_EV_INS, len(pool)
            pool += [4, 8]
    return q, np.ascontiguousarray(table["h1"]), capi.pack_nibbles(pool), len(pool)


def child(variant, path, rounds):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    z = np.load(path)
    rs = capi.pinned_readset(ReadSet(z["reads"], z["cigar"], z["seq"]))
    table = z["table"]
    eng = capi.Engine(0)
    eng.set_params(channels=30)
    if variant == "snv":
        eng.set_phase_sites(table)
    elif variant == "alleles":
        eng.set_phase_alleles(capi.hap_sites_from_snvs(table), table["h1"])
    else:
        eng.set_phase_alleles(*planted(table))
    for _ in range(2):
        eng.load_reads(rs)
    eng.synchronize()
    st = eng.haplotags()[1]
    eng.set_profiling(True)
    eng.reset_kernel_stats()
    for _ in range(rounds):
        eng.load_reads(rs)
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
    k = ks[KERNEL[variant]]
    assert k["launches"] == rounds and not [n for n in ks if "haplotag" in n and n != KERNEL[variant]], ks
    print(json.dumps(dict(kernel_ms=k["total_ms"] / k["launches"], wall_ms=float(np.median(wall)), stats=st)))


def run(args, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit, check=True).stdout
    return json.loads(out.strip().split("\n")[-1])


def main():
    import phase_time
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haplotag_alleles.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="phased,stress,resources")
    ap.add_argument("--prepare", nargs=2, metavar=("NAME", "ARCHIVE"), help=argparse.SUPPRESS)
    ap.add_argument("--child", nargs=2, metavar=("VARIANT", "ARCHIVE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.prepare:
        return prepare(*a.prepare)
    if a.child:
        return child(a.child[0], a.child[1], a.rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")

    only = [n for n in a.only.split(",") if n]
    if only != ["resources"]:
        emit(["== haplotag_alleles_time: commit %s, %d loads a process, %d fresh processes a variant, taking turns" % (a.commit or phase_time.commit_id(), a.rounds, a.repeats)])
    with tempfile.TemporaryDirectory() as tmp:
        for name in only:
            if name == "resources":
                table = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_hap"], stdout=subprocess.PIPE, text=True, check=True).stdout
                emit(["== compiled, commit %s (tools/kernel_resources.py 'k_hap': hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage)"
                      % (a.commit or phase_time.commit_id())] + ["   " + ln for ln in table.rstrip("\n").split("\n")])
                continue
            path = os.path.join(tmp, name + ".npz")
            info = run(["--prepare", name, path], 900)
            emit(["-- %s (%s): %d reads, %d CIGAR ops; table: %d sites in %d sets (%s, phased by Engine.phase_sites)"
                  % (name, info["title"], info["n_reads"], info["n_ops"], info["n_sites"], info["n_sets"], info["what"])])
            got = {v: [] for v in VARIANTS}
            for _ in range(a.repeats):
                for v in VARIANTS:
                    got[v].append(run(["--child", v, path, "--rounds", str(a.rounds)], 600))
            for v in VARIANTS:
                st = got[v][0]["stats"]
                emit(["   %-8s %-19s ms per launch: %s | Engine.load_reads wall ms (median of %d): %s | tagged %d + %d, ties %d, votes %d"
                      % (v, KERNEL[v], " ".join("%.4f" % g["kernel_ms"] for g in got[v]), a.rounds, " ".join("%.3f" % g["wall_ms"] for g in got[v]),
                         st["n_hp1"], st["n_hp2"], st["n_tie"], st["n_votes"])])


if __name__ == "__main__":
    main()
