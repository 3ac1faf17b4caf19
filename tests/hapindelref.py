"""The haplotagging rule of include/c3r.h for a table with indels and two-ALT sites (c3r_set_phase_alleles) restated in plain Python.  The
header states that rule as the join of two others, and so does this file: the observation is hapalleleref.observe (one read, one base at a
time, its own CIGAR normalisation), the tally and the decision are hapref.tag_read's.  The join itself is all that is written here: the
sites a read votes on, in table order, become a pseudo-read of one base each — A where the read shows allele A, C where it shows allele B —
over a pseudo-table of A>C sites that carry the real sites' h1 and ps, and hapref.tag_read / hapcountref.read_tag_and_set decide on that.
Nothing is shared with csrc/haplotag_kernels.hpp or phasedvcf.py.  Its own behaviour is pinned by the hand-derived CASES below
(tests/test_hapindel_ref.py; the GPU tests run the same table through the engine).

A site is hapalleleref's dict (pos, ps, A, B, ref, alt) with one more key, h1: 0 — allele A on haplotype 1 (GT 0|1, 1|2) —, 1 — allele B
(GT 1|0, 2|1)."""
import numpy as np

from clair3_rna_amd.reads import ReadSet
from tests import hapalleleref as HA
from tests import hapcountref as HC
from tests import hapref

STAT_KEYS = hapref.STAT_KEYS


# ---- sites
def site(pos, ref, alt, gt, ps):
    """The site of one phased row: gt is `0|1`, `1|0`, `1|2` or `2|1`."""
    s = HA.site_of_row(pos, ref, alt, {"0|1": "0/1", "1|0": "1/0", "1|2": "1/2", "2|1": "2/1"}[gt], ps)
    assert not isinstance(s, str), (pos, ref, alt, gt, s)
    return dict(s, h1=1 if gt in ("1|0", "2|1") else 0)


def from_snv_table(table):
    """A PHASE_SITE_DTYPE table (c3r_set_phase_sites) as sites of this module."""
    return [dict(s, h1=int(t["h1"])) for s, t in zip(HA.snv_sites(table), table)]


def to_engine(sites, lead=0):
    """(HAP_SITE_DTYPE array, uint8 h1, packed pool, bases in the pool): the arguments of Engine.set_phase_alleles.  `lead` bases go into the
    pool first, which moves every insertion's offset (and its parity)."""
    q, pool = HA.to_query(sites, lead)
    n = lead + sum(len(ev[1]) for s in sites for _, ev in (s["A"], s["B"]) if ev[0] == "ins")
    return q, np.array([s["h1"] for s in sites], dtype=np.uint8), pool, n


# ---- one read
def votes_of(rs, i, site_at):
    """[(table index, column 0 / 1)] of the sites read i votes on, in table order."""
    return sorted((j, c) for j, c in HA.observe(rs, i, site_at).items() if c in (0, 1))


def tag_read(rs, i, sites, site_at=None):
    """(hp, c1, c2 of the winning set, that set or -1 when hp is 0, votes on all sets) of read i."""
    if site_at is None:
        site_at = {s["pos"]: (j, s) for j, s in enumerate(sites)}
    votes = votes_of(rs, i, site_at)
    if not votes:
        return 0, 0, 0, -1, 0
    pseudo = ReadSet.from_records([dict(pos=0, cigar="%dM" % len(votes), seq="".join("AC"[c] for _, c in votes), flag=0, mapq=60, hp=0)])
    by_pos = {k + 1: dict(pos=k + 1, ref=1, alt=2, h1=sites[j]["h1"], ps=sites[j]["ps"]) for k, (j, _) in enumerate(votes)}
    hp, c1, c2, _ = hapref.tag_read(pseudo, 0, by_pos)
    hp2, ps = HC.read_tag_and_set(pseudo, 0, by_pos)
    assert hp2 == hp
    return hp, c1, c2, ps, len(votes)


def haplotag(rs, sites):
    """(uint8[n] tags, stats dict like Engine.haplotags(), int32[n] phase sets like Engine.read_phase_sets())."""
    site_at = {s["pos"]: (j, s) for j, s in enumerate(sites)}
    hp = np.zeros(len(rs), np.uint8)
    ps = np.full(len(rs), -1, np.int32)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["n_reads"] = len(rs)
    for i in range(len(rs)):
        hp[i], _, _, ps[i], n = tag_read(rs, i, sites, site_at)
        st["n_votes"] += n
        st["n_hp1" if hp[i] == 1 else "n_hp2" if hp[i] == 2 else "n_tie" if n else "n_no_vote"] += 1
    return hp, st, ps


def allele_counts(rs, hp, ps, query, params=HC.DEFAULT_PARAMS):
    """hapalleleref.counts with the reads' tags and sets given (uint32 (n, 3, 3)): what c3r_hap_allele_counts returns under these tags."""
    from tests import phaseref
    site_at = {s["pos"]: (j, s) for j, s in enumerate(query)}
    out = np.zeros((len(query), 3, 3), dtype=np.uint32)
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], params):
            continue
        for j, col in HA.observe(rs, i, site_at).items():
            out[j, int(hp[i]) if hp[i] and int(ps[i]) == query[j]["ps"] else 0, col] += 1
    return out


def snv_counts(rs, hp, ps, query, params=HC.DEFAULT_PARAMS):
    """hapcountref.hap_counts with the reads' tags and sets given: what c3r_hap_counts returns under these tags."""
    from tests import phaseref
    query_at = {int(s["pos"]): (j, s) for j, s in enumerate(query)}
    out = np.zeros((len(query), 3, 3), dtype=np.uint32)
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], params):
            continue
        for j, col in HC.observe(rs, i, query_at).items():
            out[j, int(hp[i]) if hp[i] and int(ps[i]) == int(query[j]["ps"]) else 0, col] += 1
    return out


# ---- hand-derived known answers: (name, [(pos0, cigar, seq[, l_seq])], [(pos1, REF, ALT, GT, ps)], [(hp, c1, c2, set) per read]).
# Reference positions are 1-based in the sites and 0-based in the reads; c1 / c2 are those of the winning set; every expectation was worked
# out by hand from the rule in include/c3r.h.
CASES = [
    # 3M 2D 3M at 0: bases on 1, 2, 3, 6, 7, 8.  GAA > G on 3: A = (G, none), B = (G, del 2); the read shows del 2 behind the anchor: B.
    ("deletion_only_0|1", [(0, "3M2D3M", "ACGTTT")], [(3, "GAA", "G", "0|1", 5)], [(2, 0, 1, 5)]),
    ("deletion_only_1|0", [(0, "3M2D3M", "ACGTTT")], [(3, "GAA", "G", "1|0", 5)], [(1, 1, 0, 5)]),
    # the same read beside an SNV it does not reach: with the SNV rows alone the read is untagged
    ("only_an_indel_on_the_read", [(0, "3M2D3M", "ACGTTT")], [(3, "GAA", "G", "1|0", 5), (50, "A", "C", "0|1", 5)], [(1, 1, 0, 5)]),
    # a deletion one base longer than the allele's is another allele; a read without the deletion shows A
    ("deletion_one_off", [(0, "3M3D3M", "ACGTTT")], [(3, "GAA", "G", "1|0", 5)], [(0, 0, 0, -1)]),
    ("no_deletion_is_allele_a", [(0, "6M", "ACGAAT")], [(3, "GAA", "G", "1|0", 5)], [(2, 0, 1, 5)]),
    # 2M 2I 2M at 0: query 0 1 | 2 3 inserted | 4 5.  C > CTT on 2; the read inserts TG: column 2
    ("insertion_one_base_off", [(0, "2M2I2M", "ACTGAA")], [(2, "C", "CTT", "0|1", 1)], [(0, 0, 0, -1)]),
    ("insertion_equal", [(0, "2M2I2M", "ACTTAA")], [(2, "C", "CTT", "0|1", 1)], [(2, 0, 1, 1)]),
    # an insertion directly followed by a deletion is the `+<ins>-<del>` column: no allele's event
    ("insertion_then_deletion", [(0, "2M2I1D2M", "ACTTAA")], [(2, "C", "CTT", "0|1", 1)], [(0, 0, 0, -1)]),
    # C > T,CGG on 2, GT 1|2: A = (T, none), B = (C, ins GG).  Read 0 shows T mid-op (A), read 1 C + GG (B), read 2 the reference (neither)
    ("two_alt_1|2", [(0, "3M", "ATA"), (0, "2M2I1M", "ACGGA"), (0, "3M", "ACA")], [(2, "C", "T,CGG", "1|2", 4)], [(1, 1, 0, 4), (2, 0, 1, 4), (0, 0, 0, -1)]),
    ("two_alt_2|1", [(0, "3M", "ATA"), (0, "2M2I1M", "ACGGA"), (0, "3M", "ACA")], [(2, "C", "T,CGG", "2|1", 4)], [(2, 0, 1, 4), (1, 1, 0, 4), (0, 0, 0, -1)]),
    # 4M 1D 3M at 0: bases on 1 .. 4 and 6 .. 8.  Two SNVs show REF (haplotype 1 under 0|1), TA > T on 4 shows B (haplotype 2): 2 : 1
    ("snvs_outvote_an_indel", [(0, "4M1D3M", "ACGTAAA")], [(1, "A", "C", "0|1", 7), (2, "C", "G", "0|1", 7), (4, "TA", "T", "0|1", 7)], [(1, 2, 1, 7)]),
    # the same three votes over two sets: set 7 holds two, set 3 one — the set is chosen by count, not by number
    ("two_sets_by_count", [(0, "4M1D3M", "ACGTAAA")], [(1, "A", "C", "0|1", 7), (2, "C", "G", "0|1", 7), (4, "TA", "T", "0|1", 3)], [(1, 2, 0, 7)]),
    # and with the indel's set holding two: set 9 wins by count and is tied 1 : 1 in itself
    ("two_sets_by_count_tied_winner", [(0, "4M1D3M", "ACGTAAA")], [(1, "A", "C", "0|1", 7), (2, "C", "G", "0|1", 9), (4, "TA", "T", "0|1", 9)], [(0, 1, 1, -1)]),
    # 2M 1I 3M at 0: one vote each in sets 9 and 3; set 9's (first) voting site is the insertion on 2, which comes first in the table
    ("equal_sets_first_site_is_an_indel", [(0, "2M1I3M", "ACGTTA")], [(2, "C", "CG", "1|0", 9), (3, "T", "A", "1|0", 3)], [(1, 1, 0, 9)]),
    ("equal_sets_first_site_is_an_snv", [(0, "2M1I3M", "ACGTTA")], [(1, "A", "G", "1|0", 3), (2, "C", "CG", "1|0", 9)], [(2, 0, 1, 3)]),
    # a site whose anchor lies under a D or an N op
    ("anchor_under_a_deletion", [(0, "2M2D2M", "AAAA")], [(3, "AT", "A", "0|1", 1)], [(0, 0, 0, -1)]),
    ("anchor_under_a_ref_skip", [(0, "2M10N2M", "AAAA")], [(5, "A", "AG", "0|1", 1)], [(0, 0, 0, -1)]),
    # 2M 3I 2M with l_seq 3: the insertion's bases do not all lie in SEQ — no observation where the event matters, a base vote where it does not
    ("insertion_cut_off_event_matters", [(0, "2M3I2M", "ACGT", 3)], [(2, "C", "CGTT", "0|1", 1)], [(0, 0, 0, -1)]),
    ("insertion_cut_off_snv_site", [(0, "2M3I2M", "ACGT", 3)], [(2, "C", "T", "0|1", 1)], [(1, 1, 0, 1)]),
]


def case_inputs(case):
    """(ReadSet, sites) of one entry of CASES.  The reads keep the order of the table (they are given sorted by position)."""
    _, reads, rows, _ = case
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=0, mapq=60, hp=0) for r in reads])
    for i, r in enumerate(reads):
        if len(r) > 3:
            rs.reads["l_seq"][i] = r[3]
    return rs, [site(*row) for row in rows]
