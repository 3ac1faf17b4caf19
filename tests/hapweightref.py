"""The quality-weighted haplotag decision of include/c3r.h (c3r_set_hap_bq_weights, the rule `bq_weights`) restated in plain Python.  The
observation is not restated here: it is an argument, obs(rs, i, site_at) -> {table index: column}, and the tests pass hapalleleref.observe
(an SNV table goes through hapindelref.from_snv_table), leftalignref.observer(ref) or realignref.observer(ref, W).  What is written here
is the rest of the rule: where the anchor base of an observation lies in the read (a walk of the raw CIGAR, one base at a time), its
weight, the sums per phase set, the choice of the set and the tag.  Nothing is shared with csrc/haplotag_kernels.hpp.

A site is hapindelref's dict (pos, ps, A, B, h1).  weighted=False gives every observation weight 1: the rule of c3r_set_phase_sites."""
import random

import numpy as np

from clair3_rna_amd.reads import ReadSet
from tests import hapalleleref as HA
from tests import hapref

STAT_KEYS = hapref.STAT_KEYS


def anchor_offsets(rs, i):
    """{1-based reference position: query offset} of every base of read i under an M, = or X op."""
    r = rs.reads[i]
    x, y, at = int(r["pos"]), 0, {}
    for op, n in HA.read_ops(rs, i):
        if op in "M=X":
            for d in range(n):
                at[x + d + 1] = y + d
            x, y = x + n, y + n
        elif op in "DN":
            x += n
        elif op in "IS":
            y += n
    return at


def weight(rs, i, q):
    """The weight of the base at query offset q of read i: its quality byte; 1 for 0xff and for a ReadSet without qualities."""
    if getattr(rs, "qual", None) is None:
        return 1
    b = int(rs.qual[2 * int(rs.reads[i]["seq_off"]) + q])
    return 1 if b == 0xff else b


def tag_read(rs, i, sites, site_at, obs=HA.observe, weighted=True):
    """dict(hp, ps (-1 when hp is 0), w1, w2 of the chosen set, n: observations on all sets) of read i."""
    votes = sorted((j, c) for j, c in obs(rs, i, site_at).items() if c in (0, 1))
    if not votes:
        return dict(hp=0, ps=-1, w1=0, w2=0, n=0)
    at = anchor_offsets(rs, i)
    sets = {}                                                 # ps -> [w1, w2, table index of the first voting site]
    for j, c in votes:
        s = sites[j]
        t = sets.setdefault(s["ps"], [0, 0, j])
        t[0 if c == s["h1"] else 1] += weight(rs, i, at[s["pos"]]) if weighted else 1
    ps, (w1, w2, _) = max(sets.items(), key=lambda kv: (kv[1][0] + kv[1][1], -kv[1][2]))
    hp = 1 if w1 > w2 else 2 if w2 > w1 else 0
    return dict(hp=hp, ps=ps if hp else -1, w1=w1, w2=w2, n=len(votes), chosen=ps)


def haplotag(rs, sites, obs=HA.observe, weighted=True):
    """dict(hp uint8[n], ps int32[n], w12 uint32[n][2], words uint32[n] (tag | n << 2), st: the statistics of Engine.haplotags(),
    chosen int64[n]: the set of the largest sum also where the tag is 0, -1 without an observation)."""
    site_at = {s["pos"]: (j, s) for j, s in enumerate(sites)}
    n = len(rs)
    out = dict(hp=np.zeros(n, np.uint8), ps=np.full(n, -1, np.int32), w12=np.zeros((n, 2), np.uint32), words=np.zeros(n, np.uint32),
               chosen=np.full(n, -1, np.int64), st=dict.fromkeys(STAT_KEYS, 0))
    st = out["st"]
    st["n_reads"] = n
    for i in range(n):
        t = tag_read(rs, i, sites, site_at, obs, weighted)
        out["hp"][i], out["ps"][i], out["w12"][i], out["words"][i], out["chosen"][i] = t["hp"], t["ps"], (t["w1"], t["w2"]), t["hp"] | t["n"] << 2, t.get("chosen", -1)
        st["n_votes"] += t["n"]
        st["n_hp1" if t["hp"] == 1 else "n_hp2" if t["hp"] == 2 else "n_tie" if t["n"] else "n_no_vote"] += 1
    return out


def pc_of(w12):
    """uint32[n]: |w1 - w2|, what the haplotagged BAM carries as PC."""
    w = np.asarray(w12, np.int64)
    return np.abs(w[:, 0] - w[:, 1]).astype(np.uint32)


def with_qual(rs, qual):
    """The ReadSet with another quality array (None: without one)."""
    return ReadSet(rs.reads.copy(), rs.cigar.copy(), rs.seq.copy(), None if qual is None else np.asarray(qual, np.uint8))


def masked_as_n(rs, Q):
    """The reads with the bases that c3r_set_hap_min_bq(Q) masks replaced by N, and their qualities as they were."""
    from tests import qualref
    return ReadSet(rs.reads.copy(), rs.cigar.copy(), qualref.mask(rs, Q)[0], rs.qual.copy())


# ---- hand cases: (name, [(pos0, cigar, seq, quals or None)], [(pos1, REF, ALT, GT, ps)], Q of c3r_set_hap_min_bq,
#                  [(hp, w1, w2, ps, n) per read under weights], [(hp, ps) per read under unit weights]).  Worked out by hand from the rule.
CASES = [
    # sites on 1, 2, 3, all 0|1: A (REF) is haplotype 1.  The read shows ALT, ALT, REF with Q5, Q5, Q30: 30 against 10
    ("q30_outvotes_two_q5", [(0, "3M", "CCA", [5, 5, 30])], [(1, "A", "C", "0|1", 4), (2, "A", "C", "0|1", 4), (3, "A", "C", "0|1", 4)], 0,
     [(1, 30, 10, 4, 3)], [(2, 4)]),
    # set 7 holds two observations of Q2 (sum 4), set 9 one of Q40: the set is chosen by weight
    ("set_by_weight_not_by_count", [(0, "3M", "AAC", [2, 2, 40])], [(1, "A", "C", "0|1", 7), (2, "A", "C", "0|1", 7), (3, "A", "C", "0|1", 9)], 0,
     [(2, 0, 40, 9, 3)], [(1, 7)]),
    # sets 9 and 3 weigh 20 each; set 9's first voting site comes first on the read (and 3 is the smaller number); by count set 3 wins
    ("equal_weight_first_site_wins", [(0, "3M", "ACC", [20, 10, 10])], [(1, "A", "C", "0|1", 9), (2, "A", "C", "0|1", 3), (3, "A", "C", "0|1", 3)], 0,
     [(1, 20, 0, 9, 3)], [(2, 3)]),
    # 10 + 20 for haplotype 1, 30 for haplotype 2: a tie where unit weights say 2 : 1
    ("w1_equals_w2_is_a_tie", [(0, "3M", "AAC", [10, 20, 30])], [(1, "A", "C", "0|1", 4), (2, "A", "C", "0|1", 4), (3, "A", "C", "0|1", 4)], 0,
     [(0, 30, 30, -1, 3)], [(1, 4)]),
    # a Q0 base is an observation and adds nothing: 1 : 1 under unit weights, 0 : 7 under weights, two observations in the tag word
    ("q0_counts_and_adds_nothing", [(0, "2M", "AC", [0, 7])], [(1, "A", "C", "0|1", 4), (2, "A", "C", "0|1", 4)], 0,
     [(2, 0, 7, 4, 2)], [(0, -1)]),
    # only Q0 observations: a tie of (0, 0) with one observation, not "no vote"
    ("only_q0", [(0, "1M", "A", [0])], [(1, "A", "C", "0|1", 4)], 0, [(0, 0, 0, -1, 1)], [(1, 4)]),
    # a record without qualities (0xff throughout) weighs 1 per vote: its unit-weight result
    ("no_qualities", [(0, "3M", "CCA", None)], [(1, "A", "C", "0|1", 4), (2, "A", "C", "0|1", 4), (3, "A", "C", "0|1", 4)], 0,
     [(2, 1, 2, 4, 3)], [(2, 4)]),
    # Q = 10 masks the two Q5 bases: they are N and no observation; the Q30 base is left alone with its own quality
    ("masked_bases_do_not_vote", [(0, "3M", "CCA", [5, 5, 30])], [(1, "A", "C", "0|1", 4), (2, "A", "C", "0|1", 4), (3, "A", "C", "0|1", 4)], 10,
     [(1, 30, 0, 4, 1)], [(1, 4)]),
    # 3M 2D 3M, GAA > G on 3 (B = the deletion, 1|0: B is haplotype 1) weighs the anchor's quality 33; the SNV on 1 (0|1, REF: haplotype 1
    # ... the read shows ALT C: haplotype 2) weighs 12, the SNV on 7 (ALT: haplotype 2) 20: 33 against 32
    ("indel_weighs_its_anchor", [(0, "3M2D3M", "CCGTTT", [12, 9, 33, 9, 20, 9])], [(1, "A", "C", "0|1", 5), (3, "GAA", "G", "1|0", 5), (7, "A", "T", "0|1", 5)], 0,
     [(1, 33, 32, 5, 3)], [(2, 5)]),
]


def case_inputs(case):
    """(ReadSet with qualities — 0xff where the case gives none —, sites, Q) of one entry of CASES."""
    from tests import hapindelref as HI
    _, reads, rows, Q, _, _ = case
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=0, mapq=60, hp=0, **({} if r[3] is None else dict(qual=r[3]))) for r in reads])
    if rs.qual is None:
        rs = with_qual(rs, np.full(2 * len(rs.seq), 0xff, np.uint8))
    return rs, [HI.site(*row) for row in rows], Q


# ---- the seeded fuzz of the CPU and GPU tests
FUZZ_SEED = 3


def gen_fuzz(seed=FUZZ_SEED, n_reads=300):
    """(reference (0, letters), table, ReadSet with qualities): realignref.gen_fuzz's reads — SNV, insertion, deletion and two-ALT sites
    every 15 bases, = / X ops and pads in every second read, soft clips — with the sites dealt to three interleaved phase sets, a third
    of them phased the other way round than the reads were made, and a
    quality of 0 .. 40 on every base (one in sixteen 0, a tenth of the reads without qualities)."""
    from tests import realignref as RR
    ref, table, rs = RR.gen_fuzz(seed, n_reads=n_reads, quals=True)
    rng = random.Random(seed + 500)
    for k, s in enumerate(table):
        s["ps"] = 21 + (k * 3 // len(table) if rng.random() < 0.6 else rng.randrange(3))
        if rng.random() < 0.35:                               # (a site phased the wrong way round: the reads' votes disagree, and weights decide)
            s["h1"] = 1 - s["h1"]
    qual = rs.qual.copy()
    for i, r in enumerate(rs.reads):
        o, L = 2 * int(r["seq_off"]), int(r["l_seq"])
        if i % 10 == 7:
            qual[o:o + L] = 0xff
        else:
            qual[o:o + L] = [0 if rng.random() < 1 / 16 else rng.choice((3, 5, 8, 12, 20, 30, 40)) for _ in range(L)]
    return ref, table, with_qual(rs, qual)


def snv_rows(table):
    """The sites of a table that are plain biallelic SNVs, as a PHASE_SITE_DTYPE array (c3r_set_phase_sites)."""
    rows = [(s["pos"], s["A"][0], s["B"][0], s["h1"], s["ps"]) for s in table if s["A"][1] == HA.NONE and s["B"][1] == HA.NONE]
    return hapref.make_sites(rows)


def fuzz_classes(weighted, unit):
    """How the reads move between the two rules: dict(tagged_unit, differ, flipped, set_changed, became_tie, left_tie)."""
    hw, hu, pw, pu = weighted["hp"], unit["hp"], weighted["ps"], unit["ps"]
    tagged = hu > 0
    return dict(tagged_unit=int(tagged.sum()), differ=int((tagged & ((hw != hu) | (pw != pu))).sum()),
                flipped=int((tagged & (hw > 0) & (hw != hu)).sum()), set_changed=int((tagged & (hw > 0) & (pw != pu)).sum()),
                became_tie=int((tagged & (hw == 0)).sum()),
                left_tie=int(((hu == 0) & ((unit["words"] >> 2) > 0) & (hw > 0)).sum()))
