#!/usr/bin/env python3
"""What --hap_min_bq changes (include/c3r.h: c3r_set_hap_min_bq) — against a GENERATOR's truth, with qualities that are informative BY
CONSTRUCTION, not real data: it shows what the rule does when wrong bases do carry lower qualities, not how good the qualities of a real
ONT run are, and no default is chosen from it.  Agreement with whatshap is NOT MEASURED (the tool is on none of our machines).  Plain Python
(tests/qualref.py and tests/leftalignref.py, the restatements of the rules): no GPU.

    python tools/hap_min_bq_quality.py [--commit ID] [--out profiles/hap_min_bq_quality.txt]

Reads: tests/leftalignref.gen_repeats(seed, jitter=False, errors=True), seeds 0-7 — 403 reads over 6 kb from two haplotypes that differ at
100 SNVs and up to 36 insertions and deletions, with 5 % substitutions, 1 % N and an indel of 1-3 every ~60 bases.
Qualities (random.Random(1000 + seed)): a base under an M op is WRONG when it is not what the read's source haplotype carries on that
position (the allele of the table's site there, else the reference base); a wrong base draws its quality uniformly from ERR_Q, every
other base (inserted and clipped bases included) from OK_Q.
For Q in 0, 5, 10, 15, 20 the reads go through qualref.with_n(rs, Q) — the rule IS "the switched-off rule on reads whose masked bases are
N" — and then, per seed: the columns of tools/left_align_quality.py (switch off), and the reads whose phase set came to a tie."""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

ERR_Q = (2, 14)          # inclusive: wrong bases
OK_Q = (8, 40)           # inclusive: every other base
THRESHOLDS = (0, 5, 10, 15, 20)


def with_qualities(rs, hap, table, ref, seed):
    """The ReadSet with qualities by the model above, and the number of wrong bases."""
    import numpy as np
    from clair3_rna_amd.reads import ReadSet
    from tests import hapalleleref as HA
    rnd = random.Random(1000 + seed)
    by_pos = {s["pos"]: s for s in table}
    qual = np.full(2 * len(rs.seq), 0xff, np.uint8)
    wrong = 0
    for i, r in enumerate(rs.reads):
        o, L = 2 * int(r["seq_off"]), int(r["l_seq"])
        bad = set()
        x, y = int(r["pos"]), 0
        for k in range(int(r["n_cigar"])):
            c = int(rs.cigar[int(r["cigar_off"]) + k])
            op, ln = "MIDNSHP=X"[c & 15], c >> 4
            if op in "M=X":
                for d in range(ln):
                    s = by_pos.get(x + d + 1)
                    want = ref[x + d]
                    if s is not None:
                        want = (s["B"] if (s["h1"] == 1) == (int(hap[i]) == 1) else s["A"])[0]
                    if y + d < L and HA.LETTER.get(HA.code_at(rs, i, y + d)) != want:
                        bad.add(y + d)
                x += ln
                y += ln
            elif op in "DN":
                x += ln
            elif op in "IS":
                y += ln
        for j in range(L):
            qual[o + j] = rnd.randint(*(ERR_Q if j in bad else OK_Q))
        wrong += len(bad)
    return ReadSet(rs.reads, rs.cigar, rs.seq, qual), wrong


def main():
    import left_align_quality
    import phase_time
    from tests import hapalleleref as HA
    from tests import leftalignref as LA
    from tests import qualref as QR
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_min_bq_quality.txt"))
    a = ap.parse_args()
    lines = ["== hap_min_bq_quality: commit %s; a GENERATOR's result (tests/leftalignref.gen_repeats(seed, jitter=False, errors=True), 403 reads a seed), by the "
             "restatements tests/qualref.py and tests/leftalignref.py on the CPU.  The qualities are informative BY CONSTRUCTION: a wrong base (not what the "
             "read's haplotype carries there) draws uniformly from %d..%d, every other base from %d..%d.  Not real data; no default is chosen from these "
             "numbers; agreement with whatshap: NOT MEASURED" % ((a.commit or phase_time.commit_id(),) + ERR_Q + OK_Q)]
    lines.append("   seed   Q  masked bases  wrong bases  indel sites  phased  agree  SNV switch errors  reads tagged  wrong  ties")
    total = {Q: [0] * 9 for Q in THRESHOLDS}
    for seed in range(8):
        ref, rs, rows, truth, planted, hap = LA.gen_repeats(seed, False, errors=True)
        table, is_snv = LA.table_of_case(rows, truth, planted)
        rq, wrong = with_qualities(rs, hap, table, ref, seed)
        for Q in THRESHOLDS:
            rn = QR.with_n(rq, Q)
            m = left_align_quality.measure(rn, hap, table, is_snv, HA.observe)
            ties = LA.haplotag(rn, table, HA.observe)[1]["n_tie"]
            row = (QR.mask(rq, Q)[1], wrong) + m[:6] + (ties,)
            total[Q] = [t + v for t, v in zip(total[Q], row)]
            lines.append("   %4d  %2d  %12d  %11d  %11d  %6d  %5d  %17d  %12d  %5d  %4d" % ((seed, Q) + row))
    for Q in THRESHOLDS:
        lines.append("   all   %2d  %12d  %11d  %11d  %6d  %5d  %17d  %12d  %5d  %4d" % ((Q,) + tuple(total[Q])))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
