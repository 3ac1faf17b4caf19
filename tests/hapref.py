"""The haplotagging rule of include/c3r.h (c3r_set_phase_sites) restated in plain Python: one read at a time, one base at a time, a dict of
votes per read.  It shares nothing with csrc/haplotag_kernels.hpp — no searches of a sorted table, no folded or normalised CIGAR, no
lanes — and is what the GPU tests compare the kernel with.  Its own behaviour is pinned by the hand-derived cases of tests/test_hapref.py
(CASES below: the GPU tests run the same table through the engine).

gen_case(seed) builds the random two-haplotype read sets of the GPU tests."""
import random

import numpy as np

from clair3_rna_amd.capi import PHASE_SITE_DTYPE
from clair3_rna_amd.reads import ReadSet

CODE = {"A": 1, "C": 2, "G": 4, "T": 8}
STAT_KEYS = ("n_reads", "n_hp1", "n_hp2", "n_no_vote", "n_tie", "n_votes")


def make_sites(rows):
    """[(pos, ref letter, alt letter, h1, ps)] -> PHASE_SITE_DTYPE array (as given: the caller sorts)."""
    a = np.zeros(len(rows), dtype=PHASE_SITE_DTYPE)
    for k, (pos, ref, alt, h1, ps) in enumerate(rows):
        a[k] = (pos, ps, CODE[ref], CODE[alt], h1, 0)
    return a


def tag_read(rs, i, by_pos):
    """(hp, c1, c2, {ps: [c1, c2, position of the first voting site]}) of read i; by_pos: {1-based pos: site record}."""
    r = rs.reads[i]
    x, y = int(r["pos"]), 0                                  # 0-based reference cursor, query cursor
    tally = {}
    for k in range(int(r["n_cigar"])):
        c = int(rs.cigar[int(r["cigar_off"]) + k])
        op, ln = "MIDNSHP=X"[c & 15], c >> 4
        if op in "M=X":
            for d in range(ln):
                s = by_pos.get(x + d + 1)
                q = y + d
                if s is None or q >= int(r["l_seq"]):
                    continue
                byte = int(rs.seq[int(r["seq_off"]) + q // 2])
                b = byte & 15 if q % 2 else byte >> 4
                if b == int(s["ref"]):
                    allele = 0
                elif b == int(s["alt"]):
                    allele = 1
                else:
                    continue
                t = tally.setdefault(int(s["ps"]), [0, 0, int(s["pos"])])
                t[0 if allele == int(s["h1"]) else 1] += 1
            x += ln
            y += ln
        elif op in "DN":
            x += ln
        elif op in "IS":
            y += ln
    if not tally:
        return 0, 0, 0, tally
    c1, c2, _ = max(tally.values(), key=lambda t: (t[0] + t[1], -t[2]))
    return (1 if c1 > c2 else 2 if c2 > c1 else 0), c1, c2, tally


def haplotag(rs, sites):
    """(uint8[n] tags, stats dict like Engine.haplotags(), phase sets seen per read)."""
    by_pos = {int(s["pos"]): s for s in sites}
    hp = np.zeros(len(rs), np.uint8)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["n_reads"] = len(rs)
    n_ps = np.zeros(len(rs), np.int64)
    for i in range(len(rs)):
        hp[i], _, _, tally = tag_read(rs, i, by_pos)
        n_ps[i] = len(tally)
        st["n_votes"] += sum(t[0] + t[1] for t in tally.values())
        st["n_hp1" if hp[i] == 1 else "n_hp2" if hp[i] == 2 else "n_tie" if tally else "n_no_vote"] += 1
    return hp, st, n_ps


def with_hp(rs, hp):
    """A copy of the ReadSet whose records carry the tags `hp`."""
    reads = rs.reads.copy()
    reads["hp"] = hp
    return ReadSet(reads, rs.cigar.copy(), rs.seq.copy())


# ---- hand-derived known answers: (name, [(pos0, cigar, seq[, l_seq])], [(pos1, ref, alt, h1, ps)], [(hp, c1, c2) per read]).
# Reference positions are 1-based in the sites and 0-based in the reads; every expectation was worked out by hand from the rule.
CASES = [
    # read at 0-based 10 = 1-based 11..14; sites on its first and its last aligned base
    ("first_and_last_base", [(10, "4M", "ACGT")], [(11, "A", "C", 0, 7), (14, "T", "G", 0, 7)], [(1, 2, 0)]),
    ("just_outside_the_read", [(10, "4M", "ACGT")], [(10, "A", "C", 0, 7), (15, "T", "G", 0, 7)], [(0, 0, 0)]),
    ("site_at_position_1", [(0, "3M", "CAA")], [(1, "A", "C", 0, 1)], [(2, 0, 1)]),
    # 2M 2D 2M at 0: bases on 1-based 1, 2, 5, 6; 3 and 4 are deleted
    ("inside_a_deletion", [(0, "2M2D2M", "AAAA")], [(3, "A", "C", 0, 1), (4, "A", "C", 0, 1)], [(0, 0, 0)]),
    ("after_a_deletion", [(0, "2M2D2M", "AAGA")], [(5, "G", "C", 1, 1)], [(2, 0, 1)]),
    # 2M 10N 2M at 0: bases on 1, 2, 13, 14
    ("inside_a_ref_skip", [(0, "2M10N2M", "AAAA")], [(3, "A", "C", 0, 1), (12, "A", "C", 0, 1)], [(0, 0, 0)]),
    ("after_a_ref_skip", [(0, "2M10N2M", "AACA")], [(13, "A", "C", 0, 1)], [(2, 0, 1)]),
    # soft clips consume the query only: 2S 3M 2S at 0-based 5 covers 1-based 6..8 with query 2..4
    ("under_soft_clips", [(5, "2S3M2S", "CCAAACC")], [(4, "A", "C", 0, 1), (5, "A", "C", 0, 1), (9, "A", "C", 0, 1), (10, "A", "C", 0, 1)], [(0, 0, 0)]),
    ("between_soft_clips", [(5, "2S3M2S", "CCAGACC")], [(7, "G", "T", 0, 1)], [(1, 1, 0)]),
    # 2M 2I 2M at 0: query 0 1 | 2 3 inserted | 4 5; reference 1 2 | 3 4
    ("before_and_after_an_insertion", [(0, "2M2I2M", "ACTTGA")], [(2, "C", "T", 0, 1), (3, "G", "T", 0, 1)], [(1, 2, 0)]),
    ("inserted_bases_do_not_vote", [(0, "2M2I2M", "AATTAA")], [(2, "T", "A", 0, 1), (3, "T", "A", 0, 1)], [(2, 0, 2)]),
    ("eq_and_x_ops", [(0, "2=1X2=", "ACGTA")], [(2, "C", "T", 0, 1), (3, "A", "G", 0, 1), (5, "A", "T", 1, 1)], [(2, 1, 2)]),
    # a read base that is '=' (code 0), N, or a third base gives no vote
    ("base_eq_n_third", [(0, "4M", "=NGA")], [(1, "A", "C", 0, 1), (2, "A", "C", 0, 1), (3, "A", "C", 0, 1), (4, "A", "C", 0, 1)], [(1, 1, 0)]),
    ("iupac_base", [(0, "2M", "RM")], [(1, "A", "G", 0, 1), (2, "A", "C", 0, 1)], [(0, 0, 0)]),
    # the CIGAR claims 6 bases and l_seq says 3 (the fourth nibble holds a C that is not part of the read): query 3.. gives no vote
    ("l_seq_shorter_than_cigar", [(0, "6M", "AACC", 3)], [(3, "A", "C", 0, 1), (4, "A", "C", 1, 1), (6, "A", "C", 1, 1)], [(2, 0, 1)]),
    ("h1_0_ref", [(0, "1M", "A")], [(1, "A", "C", 0, 1)], [(1, 1, 0)]),
    ("h1_0_alt", [(0, "1M", "C")], [(1, "A", "C", 0, 1)], [(2, 0, 1)]),
    ("h1_1_ref", [(0, "1M", "A")], [(1, "A", "C", 1, 1)], [(2, 0, 1)]),
    ("h1_1_alt", [(0, "1M", "C")], [(1, "A", "C", 1, 1)], [(1, 1, 0)]),
    ("one_to_one_tie", [(0, "2M", "AC")], [(1, "A", "C", 0, 1), (2, "A", "C", 0, 1)], [(0, 1, 1)]),
    # two phase sets, two votes each: set 9 votes first (position 1), so it is the read's set although 3 is the smaller number
    # (set 9: A, A -> 2 : 0; set 3: C, C -> 0 : 2)
    ("equal_sets_earlier_first_site_wins", [(0, "4M", "ACAC")], [(1, "A", "C", 0, 9), (2, "A", "C", 0, 3), (3, "A", "C", 0, 9), (4, "A", "C", 0, 3)], [(1, 2, 0)]),
    # the same with the numbers swapped: neither the smaller nor the larger number decides
    ("equal_sets_earlier_first_site_wins_2", [(0, "4M", "ACAC")], [(1, "A", "C", 0, 3), (2, "A", "C", 0, 9), (3, "A", "C", 0, 3), (4, "A", "C", 0, 9)], [(1, 2, 0)]),
    # the later set has three votes to one
    ("later_set_with_more_votes_wins", [(0, "4M", "ACCC")], [(1, "A", "C", 0, 5), (2, "A", "C", 0, 6), (3, "A", "C", 0, 6), (4, "A", "C", 0, 6)], [(2, 0, 3)]),
    # interleaved: set 1 on 1, 3, 5 (two for haplotype 2, one for 1), set 2 on 2, 4
    ("interleaved_sets", [(0, "5M", "CACAA")], [(1, "A", "C", 0, 1), (2, "A", "C", 0, 2), (3, "A", "C", 0, 1), (4, "A", "C", 0, 2), (5, "A", "C", 0, 1)], [(2, 1, 2)]),
    # a no-vote site of another set earlier on the read does not make that set "first"
    ("first_VOTING_site_counts", [(0, "3M", "GAC")], [(1, "A", "C", 0, 4), (2, "A", "C", 0, 8), (3, "A", "C", 0, 4)], [(1, 1, 0)]),
    ("hard_clip_pad_and_empty_ops", [(0, "3H2M0I1P2M2H", "ACGT")], [(2, "C", "A", 1, 1), (3, "G", "A", 1, 1)], [(2, 0, 2)]),
    ("two_reads", [(0, "3M", "AAA"), (1, "3M", "CCC")], [(2, "A", "C", 0, 1), (3, "A", "C", 0, 1)], [(1, 2, 0), (2, 0, 2)]),
]


def case_inputs(case):
    """(ReadSet, site array) of one entry of CASES.  The reads keep the order of the table (they are given sorted by position)."""
    _, reads, sites, _ = case
    recs = [dict(pos=r[0], cigar=r[1], seq=r[2], flag=0, mapq=60, hp=0) for r in reads]
    rs = ReadSet.from_records(recs)
    for i, r in enumerate(reads):
        if len(r) > 3:
            rs.reads["l_seq"][i] = r[3]
    return rs, make_sites(sites)


# ---- random cases
def gen_case(seed, L=6000, n_reads=400, n_sites=120, n_ps=30):
    """(ref, ReadSet with hp = 0, site array, uint8 source haplotype per read): a random 6-kb reference, 120 sites with a random alt and h1,
    30 phase sets in consecutive blocks with 30 % of the sites moved to a random set, ~400 reads drawn from one of two haplotypes, each
    1-40 M runs of 1-60 (10 % written as = or X) separated by N 1-300, D 1-5 or I 1-5, an optional leading S, 5 % base errors, 1 % N, random
    strand."""
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    rows = []
    for k, p in enumerate(sorted(rng.sample(range(50, L - 50), n_sites))):
        rb = ref[p - 1]
        ab = rng.choice([b for b in "ACGT" if b != rb])
        ps = k * n_ps // n_sites
        if rng.random() < 0.3:
            ps = rng.randrange(n_ps)
        rows.append((p, rb, ab, rng.randint(0, 1), 1000 + ps))
    smap = {r[0]: r for r in rows}
    recs = []
    for _ in range(n_reads):
        hap = rng.randint(1, 2)
        p0 = rng.randrange(0, L - 400)
        x, cig, seq = p0, [], []
        if rng.random() < 0.3:
            n = rng.randint(1, 20)
            cig.append("%dS" % n)
            seq += [rng.choice("ACGT") for _ in range(n)]
        nops = rng.randint(1, 40)
        for o in range(nops):
            ln = rng.randint(1, 60)
            if x + ln >= L - 1:
                break
            for d in range(ln):
                p1 = x + d + 1
                b = ref[p1 - 1]
                if p1 in smap:
                    _, rb, ab, h1, _ = smap[p1]
                    b = ab if (h1 == 1) == (hap == 1) else rb          # haplotype 1 carries ALT where GT is 1|0
                u = rng.random()
                if u < 0.05:
                    b = rng.choice("ACGT")
                elif u < 0.06:
                    b = "N"
                seq.append(b)
            cig.append("%d%s" % (ln, rng.choice("=X") if rng.random() < 0.1 else "M"))
            x += ln
            if o + 1 < nops:
                u = rng.random()
                if u < 0.3:
                    n = rng.randint(1, 300)
                    cig.append("%dN" % n)
                    x += n
                elif u < 0.5:
                    n = rng.randint(1, 5)
                    cig.append("%dD" % n)
                    x += n
                elif u < 0.7:
                    n = rng.randint(1, 5)
                    cig.append("%dI" % n)
                    seq += [rng.choice("ACGT") for _ in range(n)]
        while cig and cig[-1][-1] in "ND":                    # (an alignment does not end on a deletion or a ref-skip)
            cig.pop()
        if not any(c[-1] in "M=X" for c in cig):
            continue
        recs.append(dict(pos=p0, cigar="".join(cig), seq="".join(seq), flag=16 * rng.randint(0, 1), mapq=60, hp=0, truth=hap))
    recs.sort(key=lambda r: r["pos"])
    return ref, ReadSet.from_records(recs), make_sites(rows), np.array([r["truth"] for r in recs], np.uint8)
