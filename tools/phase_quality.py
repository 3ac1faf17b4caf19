#!/usr/bin/env python3
"""What the block-merge stage (include/c3r.h: c3r_phase_unit_links / c3r_phase_merge) does to the phasing of reads with runs of RNA-editing
sites, against the generator's truth: the chain alone beside the chain plus --levels levels of the merge.

    python tools/phase_quality.py [--gpu] [--levels 4] [--seeds 8] [--out profiles/phase_merge_quality.txt]

Input: tests/phasemergeref.gen_fragmented(seed, run) — phaseref.gen_case's ONT-like reads (5 % substitutions, 1 % N, indels) over ~120
heterozygous SNVs, plus two runs of `run` editing sites on which every read shows ALT with probability 0.3 whatever its haplotype — for runs
of 0, 6, 9 and 14 sites at 403 and at 83 reads, summed over the seeds.
Without --gpu the rule runs as its plain-Python restatement (tests/phaseref.py, tests/phasemergeref.py: no device needed); with --gpu through
Engine.phase_sites (k_phase_links, k_phase_unit_links).  Both give the same tables (tests/test_gpu_phasemerge.py), so the figures are the
same.

Per line: phased sites; blocks that hold a true SNV; switch errors / pairs of neighbouring true SNVs inside a block; editing sites inside a
block.  Agreement with whatshap is not measured here or anywhere."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpu", action="store_true", help="through Engine.phase_sites instead of the restatement")
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_merge_quality.txt"))
    a = ap.parse_args()
    from tests import phasemergeref as M
    from tests import phaseref as P
    eng = None
    if a.gpu:
        from clair3_rna_amd import capi
        eng = capi.Engine(0)
        eng.set_params()
    lines = ["== phase_quality: %s, seeds 0-%d of gen_fragmented, chain | chain + %d levels of the block merge"
             % ("Engine.phase_sites on the device" if a.gpu else "the plain-Python restatement, no device", a.seeds - 1, a.levels),
             "   reads  run  | phased sites | blocks among true SNVs | switch errors / pairs | editing sites in blocks | units joined, levels run"]
    keys = ("phased", "blocks", "err", "pairs", "editing")
    for n_reads in (403, 83):
        for run in (0, 6, 9, 14):
            tot = [dict.fromkeys(keys, 0), dict.fromkeys(keys, 0)]
            joined, levels = 0, []
            for seed in range(a.seeds):
                _, rs, sites, truth, editing = M.gen_fragmented(seed, run, n_reads=n_reads)
                if eng is not None:
                    eng.load_reads(rs)
                    chain, _ = eng.phase_sites(sites)
                    merged, st = eng.phase_sites(sites, merge_levels=a.levels)
                else:
                    lk = P.links(rs, sites)
                    chain, _ = P.resolve(sites, lk)
                    merged, st = M.phase(rs, sites, lk, a.levels)
                joined += st["merge_units_joined"]
                levels.append(st["merge_levels_run"])
                for t, table in zip(tot, (chain, merged)):
                    q = M.quality(table, truth, editing)
                    t["phased"] += q["phased"]
                    t["blocks"] += q["blocks"]
                    t["err"] += q["switches"][0]
                    t["pairs"] += q["switches"][1]
                    t["editing"] += q["editing"]
            c, m = tot
            lines.append("   %5d  %3d  | %5d -> %5d | %4d -> %4d | %d / %d -> %d / %d | %3d -> %3d | %d, %s"
                         % (len(rs), run, c["phased"], m["phased"], c["blocks"], m["blocks"], c["err"], c["pairs"], m["err"], m["pairs"],
                            c["editing"], m["editing"], joined, " ".join(str(v) for v in levels)))
    if eng is not None:
        eng.close()
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
