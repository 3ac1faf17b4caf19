#!/usr/bin/env python3
"""What --hap_bq_weights changes (include/c3r.h: c3r_set_hap_bq_weights) beside --hap_min_bq — against a GENERATOR's truth, with
qualities that are informative BY CONSTRUCTION, not real data: it shows what the two rules do when wrong bases do carry lower qualities,
not how good the qualities of a real ONT run are, and no default is chosen from it.  Agreement with whatshap is NOT MEASURED (the tool is
on none of our machines).  Plain Python (tests/hapweightref.py and tests/qualref.py, the restatements of the rules): no GPU.

    python tools/hap_weights_quality.py [--commit ID] [--out profiles/hap_weights_quality.txt]

The reads, the table and the qualities are tools/hap_min_bq_quality.py's (tests/leftalignref.gen_repeats(seed, jitter=False, errors=True),
seeds 0-7; a wrong base draws its quality from ERR_Q, every other base from OK_Q).  Four variants side by side: unit weights, the
threshold Q = 10, weights, and weights with Q = 5.  Per seed and variant: reads tagged, reads tagged against the haplotype they were made
from, and reads whose phase set came to a tie."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

VARIANTS = (("unit", 0, False), ("Q=10", 10, False), ("weights", 0, True), ("weights+Q=5", 5, True))


def main():
    import hap_min_bq_quality as MQ
    import phase_time
    from tests import hapweightref as HW
    from tests import leftalignref as LA
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_weights_quality.txt"))
    a = ap.parse_args()
    lines = ["== hap_weights_quality: commit %s; a GENERATOR's result (tests/leftalignref.gen_repeats(seed, jitter=False, errors=True), 403 reads a seed), by the "
             "restatements tests/hapweightref.py and tests/qualref.py on the CPU.  The qualities are informative BY CONSTRUCTION: a wrong base (not what the "
             "read's haplotype carries there) draws uniformly from %d..%d, every other base from %d..%d.  Not real data; no default is chosen from these "
             "numbers; agreement with whatshap: NOT MEASURED" % ((a.commit or phase_time.commit_id(),) + MQ.ERR_Q + MQ.OK_Q)]
    lines.append("   seed  variant       reads tagged  against their haplotype  ties")
    total = {v[0]: [0, 0, 0] for v in VARIANTS}
    for seed in range(8):
        ref, rs, rows, truth, planted, hap = LA.gen_repeats(seed, False, errors=True)
        table, _ = LA.table_of_case(rows, truth, planted)
        rq, _ = MQ.with_qualities(rs, hap, table, ref, seed)
        for name, Q, weighted in VARIANTS:
            got = HW.haplotag(HW.masked_as_n(rq, Q) if Q else rq, table, weighted=weighted)
            tagged = got["hp"] > 0
            row = (int(tagged.sum()), int((tagged & (got["hp"] != hap)).sum()), got["st"]["n_tie"])
            total[name] = [t + v for t, v in zip(total[name], row)]
            lines.append("   %4d  %-12s  %12d  %23d  %4d" % ((seed, name) + row))
    for name, _, _ in VARIANTS:
        lines.append("   all   %-12s  %12d  %23d  %4d" % ((name,) + tuple(total[name])))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
