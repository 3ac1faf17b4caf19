#!/usr/bin/env python3
"""What k_phase_allele_links / k_phase_allele_unit_links (c3r_phase_allele_links, c3r_phase_allele_unit_links: the phasing between the passes
over a table with indels and two-ALT sites) cost beside k_phase_links / k_phase_unit_links, on the two contigs of tools/phase_time.py:
`phased` (BASELINE.json configs[3]: MAS-Seq chr20 ~30x) and `stress` (16-Mb contig, loci at ~500x).

    python tools/phase_allele_time.py [--commit ID] [--out profiles/phase_allele_links.txt] [--rounds 10] [--repeats 3] [--only phased,stress]
                                      [--parent_root DIR]

Per contig one process prepares the input — the reads, the candidates (pass 1's heterozygous SNVs) and the chain's table of them
(Engine.phase_sites) — and leaves it in a temporary archive.  Then FRESH PROCESSES take turns, `repeats` times each.  A process of this tree
measures, with profiling on (ms per launch from kernel_stats, mean of `rounds` launches after two warm-up calls):
    k_phase_links                          the candidates
    k_phase_allele_links, SNV table        the same candidates as REF-and-one-SNV sites
    k_phase_allele_links, planted          the same with every third site turned into an insertion of 2 or a deletion of 2 behind its anchor
                                           (event_matters = 1; the reads do not carry these alleles, so they show allele A)
    k_phase_unit_links                     the chain's table with every ten consecutive phased sites a unit (the chain's own blocks are few)
    k_phase_allele_unit_links, SNV table / planted   likewise
and with profiling off the wall time of Engine.phase_sites and of Engine.phase_allele_sites on the SNV table and on the planted one (median
of `rounds`).  --parent_root DIR: a built tree of the parent commit; its processes take turns with this tree's and measure the two kernels
it has — the yardstick for "k_phase_links did not move" is that commit's kernel and its run-to-run spread."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                     # (a child that measures another tree's library imports that tree's package)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))


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
    np.savez(path, reads=rs.reads, cigar=rs.cigar, seq=rs.seq, sites=sites, chain=out)
    print(json.dumps(dict(title=title, n_reads=len(rs.reads), n_ops=len(rs.cigar), what=what, n_sites=len(sites), n_phased=st["n_phased"], n_blocks=st["n_blocks"])))


def planted(sites):
    """(HAP_SITE_DTYPE sites, packed pool): every third site's allele B becomes an insertion of 2 (GT) or a deletion of 2 behind the site's REF
    base; allele A stays the REF base."""
    from clair3_rna_amd import capi
    q = capi.hap_sites_from_snvs(sites)
    pool = []
    for k in range(0, len(q), 3):
        q["base_matters"][k], q["event_matters"][k], q["b_base"][k], q["b_len"][k] = 0, 1, q["a_base"][k], 2
        if (k // 3) % 2:
            q["b_kind"][k] = capi.HAP_EV_DEL
        else:
            q["b_kind"][k], q["b_ins_off"][k] = capi.HAP_EV_INS, len(pool)
            pool += [4, 8]
    return q, capi.pack_nibbles(pool)


def child(path, rounds, old_only):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    z = np.load(path)
    rs = capi.pinned_readset(ReadSet(z["reads"], z["cigar"], z["seq"]))
    sites, chain = z["sites"], z["chain"].copy()
    idx = np.nonzero(chain["ps"] >= 0)[0]
    chain["ps"][idx] = chain["pos"][idx[(np.arange(len(idx)) // 10) * 10]]                # units of ten consecutive phased sites
    eng = capi.Engine(0)
    eng.set_params()
    eng.load_reads(rs)
    calls = [("k_phase_links", "k_phase_links", lambda: eng.phase_links(sites)),
             ("k_phase_unit_links", "k_phase_unit_links", lambda: eng.phase_unit_links(chain))]
    walls = [("Engine.phase_sites", lambda: eng.phase_sites(sites))]
    if not old_only:
        q, (p, pool), h1 = capi.hap_sites_from_snvs(sites), planted(sites), np.ascontiguousarray(chain["h1"])
        qc, pc = q.copy(), p.copy()
        qc["ps"], pc["ps"] = chain["ps"], chain["ps"]
        calls += [("k_phase_allele_links, SNV table", "k_phase_allele_links", lambda: eng.phase_allele_links(q)),
                  ("k_phase_allele_links, planted", "k_phase_allele_links", lambda: eng.phase_allele_links(p, pool)),
                  ("k_phase_allele_unit_links, SNV table", "k_phase_allele_unit_links", lambda: eng.phase_allele_unit_links(qc, h1)),
                  ("k_phase_allele_unit_links, planted", "k_phase_allele_unit_links", lambda: eng.phase_allele_unit_links(pc, h1, pool))]
        walls += [("Engine.phase_allele_sites, SNV table", lambda: eng.phase_allele_sites(q)),
                  ("Engine.phase_allele_sites, planted", lambda: eng.phase_allele_sites(p, pool))]
    res = {}
    for label, kernel, call in calls:
        call()
        call()
        eng.set_profiling(True)
        eng.reset_kernel_stats()
        for _ in range(rounds):
            call()
        k = eng.kernel_stats().get(kernel)
        eng.set_profiling(False)
        res[label] = k["total_ms"] / k["launches"] if k else None
    for label, call in walls:
        w = []
        for _ in range(rounds):
            eng.synchronize()
            t0 = time.perf_counter()
            call()
            w.append(1e3 * (time.perf_counter() - t0))
        res[label] = float(np.median(w))
    eng.close()
    print(json.dumps(res))


def run(args, limit, script=None):
    out = subprocess.run([sys.executable, script or os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit, check=True).stdout
    return json.loads(out.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_allele_links.txt"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="phased,stress")
    ap.add_argument("--parent_root", default=None, help="a built tree of the parent commit: its processes take turns with this tree's")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--prepare", nargs=2, metavar=("NAME", "ARCHIVE"), help=argparse.SUPPRESS)
    ap.add_argument("--child", nargs=1, metavar="ARCHIVE", help=argparse.SUPPRESS)
    ap.add_argument("--old_only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.prepare:
        return prepare(*a.prepare)
    if a.child:
        return child(a.child[0], a.rounds, a.old_only)
    import phase_time
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(lines):                                         # (section by section: a run cut short keeps what it measured)
        print("\n".join(lines), flush=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")

    emit(["== phase_allele_time: commit %s, %d launches a figure, %d fresh processes a tree, taking turns%s" % (
        a.commit or phase_time.commit_id(), a.rounds, a.repeats, "; `parent`: the parent commit's tree" if a.parent_root else "")])
    with tempfile.TemporaryDirectory() as tmp:
        for name in [n for n in a.only.split(",") if n]:
            path = os.path.join(tmp, name + ".npz")
            info = run(["--prepare", name, path], 900)
            emit(["-- %s (%s): %d reads, %d CIGAR ops; %s; the chain phases %d of them in %d blocks"
                  % (name, info["title"], info["n_reads"], info["n_ops"], info["what"], info["n_phased"], info["n_blocks"])])
            got = {"this": [], "parent": []}
            for _ in range(a.repeats):
                got["this"].append(run(["--child", path, "--rounds", str(a.rounds)], 600))
                if a.parent_root:
                    got["parent"].append(run(["--child", path, "--rounds", str(a.rounds), "--old_only", "--root", a.parent_root], 600))
            for label in got["this"][0]:
                unit = "wall ms, median of %d" % a.rounds if label.startswith("Engine") else "ms per launch"
                line = "   %-40s %s: this %s" % (label, unit, " ".join("-" if g[label] is None else "%.4f" % g[label] for g in got["this"]))
                if got["parent"] and label in got["parent"][0]:
                    line += " | parent %s" % " ".join("-" if g[label] is None else "%.4f" % g[label] for g in got["parent"])
                emit([line])


if __name__ == "__main__":
    main()
