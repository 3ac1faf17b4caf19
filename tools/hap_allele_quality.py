#!/usr/bin/env python3
"""How often the per-haplotype majority rule phases a heterozygous insertion, deletion or 1/2 site (include/c3r.h: c3r_hap_allele_counts /
c3r_hap_assign), and how often it phases it right — against a GENERATOR's truth, not real data: it shows that the rule is sound, not how
good it is.  Plain Python (tests/hapalleleref.py, the restatement of the rule): no GPU.

    python tools/hap_allele_quality.py [--commit ID] [--out profiles/hap_assign_quality.txt] [--min_reads 2] [--min_agree_pct 75]

tests/hapalleleref.gen_case(seed, errors=True), seeds 0-7: phaseref.gen_case's reads (5 % substitutions, 1 % N, an indel of 1-3 every ~60
bases; 12 % of the reads fail the filters) with heterozygous insertions and deletions of 1-6 bases and a few 1/2 sites planted on the two
haplotypes.  The phase table is every true SNV with its true h1, in one set; the reads are tagged from it; the planted sites are the
query.  A site agrees when the haplotype that the rule gives allele B is the one that carries it."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))


def main():
    import phase_time
    from tests import hapalleleref as HA
    from tests import hapref
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_assign_quality.txt"))
    ap.add_argument("--min_reads", type=int, default=2)
    ap.add_argument("--min_agree_pct", type=int, default=75)
    ap.add_argument("--show", action="store_true", help="print the count table of every site that disagrees")
    a = ap.parse_args()
    rows = {"ins": np.zeros(4, np.int64), "del": np.zeros(4, np.int64), "two": np.zeros(4, np.int64)}
    for seed in range(8):
        _, rs, snvs, truth, planted, _ = HA.gen_case(seed, errors=True)
        table = hapref.make_sites([(p, r, alt, int(t), 1) for (p, r, alt), t in zip(snvs, truth)])
        sites = [dict(s, ps=1) for s in HA.planted_sites(planted)]
        counts = HA.counts(rs, table, sites)
        for s, p, (ps, h1), t in zip(sites, planted, HA.assign(sites, counts, a.min_reads, a.min_agree_pct), counts):
            kind = "two" if p["gt"] == "1/2" else s["B"][1][0]
            ok = ps >= 0 and h1 == p["truth"]
            rows[kind] += (1, int(ps >= 0), int(ok), int(ps >= 0 and not ok))
            if a.show and ps >= 0 and not ok:
                print("seed %d pos %d %s>%s truth %d: %s" % (seed, s["pos"], s["ref"], s["alt"], p["truth"], t.tolist()))
    lines = ["== hap_allele_quality: commit %s; a GENERATOR's result (tests/hapalleleref.gen_case(seed, errors=True), seeds 0-7; the table is every "
             "true SNV, one set), thresholds %d / %d" % (a.commit or phase_time.commit_id(), a.min_reads, a.min_agree_pct),
             "   query              held out  phased  agree  disagree"]
    for name, label in (("ins", "insertions, 0/1"), ("del", "deletions, 0/1"), ("two", "1/2 sites")):
        lines.append("   %-18s %8d  %6d  %5d  %8d" % ((label,) + tuple(int(v) for v in rows[name])))
    lines.append("   %-18s %8d  %6d  %5d  %8d" % (("all",) + tuple(int(v) for v in sum(rows.values()))))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
