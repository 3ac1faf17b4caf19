#!/usr/bin/env python3
"""How often the per-haplotype majority rule (include/c3r.h: c3r_hap_counts / c3r_hap_assign) phases a heterozygous SNV that the phase table
does not hold, and how often it phases it right — against a GENERATOR's truth, not real data: it shows that the rule is sound, not how
good it is.  Plain Python (tests/hapcountref.py, the restatement of the rule): no GPU.

    python tools/hap_assign_quality.py [--commit ID] [--out profiles/hap_assign_quality.txt] [--min_reads 2] [--min_agree_pct 75]

tests/phaseref.gen_case(seed, errors=True), seeds 0-7 (5 % substitutions, 1 % N, indels; 12 % of the reads fail the filters).  Every third
true SNV (table indices 0, 3, 6, ...) is held out of the phase table; the reads are tagged from the rest; the held-out sites are counted
against the set of the nearest table site and assigned.
    row 1   the table is the truth: every other site with its true h1, all in one set
    row 2   the table is the chain's output (phaseref.phase) without the held-out sites; a block's orientation against the truth is that of
            the majority of its table sites, and a held-out site agrees when its own orientation is its block's"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))


def held_out(table, rs, sites, truth, min_reads, pct):
    """(held out, phased, agree, disagree) for one case."""
    from tests import hapcountref as HC
    held = np.arange(0, len(sites), 3)
    keep = table[~np.isin(table["pos"], sites["pos"][held])]
    if not len(keep):
        return len(held), 0, 0, 0
    truth_at = dict(zip(sites["pos"].tolist(), truth.tolist()))
    query = HC.nearest_sets(sites[held], keep)
    out, _ = HC.assign(query, HC.hap_counts(rs, keep, query), min_reads, pct)
    phased = agree = 0
    for s in out:
        if int(s["ps"]) < 0:
            continue
        block = keep[keep["ps"] == s["ps"]]
        flips = [int(b["h1"]) ^ truth_at[int(b["pos"])] for b in block]
        orient = 1 if 2 * sum(flips) > len(flips) else 0
        phased += 1
        agree += int((int(s["h1"]) ^ truth_at[int(s["pos"])]) == orient)
    return len(held), phased, agree, phased - agree


def main():
    import phase_time
    from clair3_rna_amd import phasing
    from tests import phaseref
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_assign_quality.txt"))
    ap.add_argument("--min_reads", type=int, default=2)
    ap.add_argument("--min_agree_pct", type=int, default=75)
    a = ap.parse_args()
    rows = {"truth": np.zeros(4, np.int64), "chain": np.zeros(4, np.int64)}
    for seed in range(8):
        _, rs, sites, truth, _ = phaseref.gen_case(seed, errors=True)
        true_table = sites.copy()
        true_table["ps"], true_table["h1"] = 1, truth
        rows["truth"] += held_out(true_table, rs, sites, truth, a.min_reads, a.min_agree_pct)
        rows["chain"] += held_out(phasing.phased_only(phaseref.phase(rs, sites)[0]), rs, sites, truth, a.min_reads, a.min_agree_pct)
    lines = ["== hap_assign_quality: commit %s; a GENERATOR's result (tests/phaseref.gen_case(seed, errors=True), seeds 0-7), thresholds %d / %d"
             % (a.commit or phase_time.commit_id(), a.min_reads, a.min_agree_pct),
             "   table            held out  phased  agree  disagree"]
    for name, label in (("truth", "the truth, one set"), ("chain", "the chain's blocks")):
        lines.append("   %-18s %6d  %6d  %5d  %8d" % ((label,) + tuple(int(v) for v in rows[name])))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
