#!/usr/bin/env python3
"""What the indel and two-ALT sites of a phase table add to the haplotags (include/c3r.h: c3r_set_phase_alleles against
c3r_set_phase_sites) — against a GENERATOR's truth, not real data: it shows what the rule does with votes it used to discard, not how good
the tags of a real sample are.  Agreement with `whatshap haplotag` is NOT MEASURED (the tool is on none of our machines).  Plain Python
(tests/hapindelref.py, the restatement of the rule): no GPU.

    python tools/haplotag_indel_quality.py [--commit ID] [--out profiles/haplotag_indel_quality.txt]

tests/hapalleleref.gen_case(seed, errors=True), seeds 0-7: 403 reads over 6 kb — exons joined by N ops, 5 % substitutions, 1 % N, an indel
of 1-3 every ~60 bases — from two haplotypes that differ at 120 SNVs, 36 insertions and deletions of 1-6 bases and 10 two-ALT sites.  The
generator's truth is the table: the SNV rows alone (what c3r_set_phase_sites can hold) against all planted sites (c3r_set_phase_alleles),
one phase set.  `sparse`: the same with every fourth SNV only, which is nearer to short reads between distant SNVs.  Per seed: reads
tagged, reads tagged AGAINST the generator's haplotype, ties (votes, and c1 == c2)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))


def tables(seed, every):
    from tests import hapalleleref as HA
    from tests import hapindelref as HI
    _, rs, rows, truth, planted, hap = HA.gen_case(seed, errors=True)
    snvs = [HI.site(p, r, a, "1|0" if t else "0|1", 1) for (p, r, a), t in list(zip(rows, truth))[::every]]
    other = [dict(s, ps=1, h1=int(p["truth"])) for s, p in zip(HA.planted_sites(planted), planted)]
    return rs, hap, snvs, sorted(snvs + other, key=lambda s: s["pos"])


def measure(rs, hap, sites):
    from tests import hapindelref as HI
    hp, st, _ = HI.haplotag(rs, sites)
    tagged = hp > 0
    return int(tagged.sum()), int((hp != hap)[tagged].sum()), st["n_tie"], st["n_votes"]


def main():
    import phase_time
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haplotag_indel_quality.txt"))
    a = ap.parse_args()
    lines = ["== haplotag_indel_quality: commit %s; a GENERATOR's result (tests/hapalleleref.gen_case(seed, errors=True), 403 reads a seed; the table is "
             "the generator's truth, one set), by the restatement tests/hapindelref.py on the CPU.  Not real data; agreement with `whatshap haplotag`: NOT MEASURED"
             % (a.commit or phase_time.commit_id())]
    for label, every in (("every SNV", 1), ("sparse: every fourth SNV", 4)):
        lines.append("-- %s" % label)
        lines.append("   seed  sites snv/all   SNV-only table: tagged  wrong  ties   votes   full table: tagged  wrong  ties   votes")
        total = [0] * 8
        for seed in range(8):
            rs, hap, snvs, full = tables(seed, every)
            row = measure(rs, hap, snvs) + measure(rs, hap, full)
            total = [t + v for t, v in zip(total, row)]
            lines.append("   %4d  %5d / %-5d %22d  %5d  %4d  %6d  %19d  %5d  %4d  %6d" % ((seed, len(snvs), len(full)) + row))
        lines.append("   all                 %22d  %5d  %4d  %6d  %19d  %5d  %4d  %6d" % tuple(total))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
