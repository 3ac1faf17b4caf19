"""The block-merge stage without a GPU: tests/phasemergeref.py pinned by hand-derived known answers, c3r_phase_merge (host code of
libc3r.so) against it, and what the stage does to the blocks the chain leaves on reads with runs of RNA-editing sites, against the truth."""
import random

import numpy as np
import pytest

from tests import phasemergeref as M
from tests import phaseref as P

K = P.K


def _readset(recs):
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=r[4] if len(r) > 4 else 60, hp=0) for r in recs])


def _table(rows):
    """[(pos, ps, h1)] -> a chain's table, every site REF A / ALT C."""
    t = P.make_sites([(r[0], "A", "C") for r in rows])
    t["ps"], t["h1"] = [r[1] for r in rows], [r[2] for r in rows]
    return t


def _ulinks(n_units, entries):
    """{(u, k): (same, different)} -> the (U, K, 2) table."""
    lk = np.zeros((n_units, K, 2), dtype=np.uint32)
    for (u, k), sd in entries.items():
        assert 1 <= k <= K and u - k >= 0
        lk[u, k - 1] = sd
    return lk


# ---- the known answer of include/c3r.h's rule: 12 sites REF A / ALT C on 11, 12, 21..28, 41, 42
KNOWN_SITES = [11, 12] + list(range(21, 29)) + [41, 42]
KNOWN_READS = [(10, "2M28N2M", "ACCC")] * 3 + [(10, "2M28N2M", "CAAA")] * 2 + [(20, "8M", "AAAAAAAA")]


def _known(extra=()):
    rs = _readset(KNOWN_READS + list(extra))
    sites = P.make_sites([(p, "A", "C") for p in KNOWN_SITES])
    chain, st = P.phase(rs, sites)
    return rs, chain, st


def test_known_answer_the_chain_leaves_two_blocks():
    _, chain, st = _known()
    # site 41's eight predecessors are the sites 21..28, which only the 8M read shows: the ninth, site 12, is out of the chain's reach
    assert chain["ps"].tolist() == [11, 11] + [-1] * 8 + [41, 41] and chain["h1"].tolist() == [0, 1] + [0] * 8 + [0, 0]
    assert st == dict(n_sites=12, n_phased=4, n_blocks=2, max_block=2)


def test_known_answer_one_level_joins_them():
    rs, chain, _ = _known()
    assert M.units_of(chain) == [11, 41]
    ul = M.unit_links(rs, chain)
    # ACCC: unit 0 shows A on 11 (allele 0 = h1) and C on 12 (allele 1 = h1): 2 : 0, haplotype 1; unit 1 shows C C against h1 0 0: 0 : 2,
    # haplotype 2.  CAAA: 0 : 2 and 2 : 0.  All five differ; the 8M read sees no unit
    assert ul.shape == (2, K, 2) and ul[1, 0].tolist() == [0, 5] and int(ul.sum()) == 5
    out, st, joined = M.merge(chain, ul)
    assert out["ps"].tolist() == [11, 11] + [-1] * 8 + [11, 11] and out["h1"].tolist() == [0, 1] + [0] * 8 + [1, 1] and joined == 1
    assert st == dict(n_sites=12, n_phased=4, n_blocks=1, max_block=4)
    assert out["pos"].tolist() == KNOWN_SITES and out["ref"].tolist() == [1] * 12 and out["alt"].tolist() == [2] * 12
    # a second level: one unit, nothing to join
    ul2 = M.unit_links(rs, out)
    assert ul2.shape == (1, K, 2) and int(ul2.sum()) == 0
    out2, st2, joined2 = M.merge(out, ul2)
    assert P.equal_sites(out2, out) and st2 == st and joined2 == 0
    assert M.merge_levels(rs, chain, 4)[2:] == (2, 1) and M.merge_levels(rs, chain, 1)[2:] == (1, 1)


def test_known_answer_sites_below_the_agreement_stay_alone():
    # four reads with 11 and 12 in cis against five in trans: 5 of 9 is below 75 %
    rs, chain, _ = _known([(10, "2M28N2M", "AACC")] * 4)
    assert chain["ps"].tolist() == [-1] * 10 + [41, 41] and chain["h1"].tolist() == [0] * 12
    ul = M.unit_links(rs, chain)
    assert ul.shape == (1, K, 2) and int(ul.sum()) == 0
    out, st, joined = M.merge(chain, ul)
    assert P.equal_sites(out, chain) and joined == 0 and st == dict(n_sites=12, n_phased=2, n_blocks=1, max_block=2)


# ---- further hand-derived cases
def test_a_whole_unit_is_flipped():
    # unit 0 (ps 100): sites 100 (h1 0), 110 (h1 1); unit 1 (ps 200): sites 200 (h1 1), 210 (h1 0), 220 (h1 1)
    chain = _table([(100, 100, 0), (110, 100, 1), (150, -1, 0), (200, 200, 1), (210, 200, 0), (220, 200, 1)])
    # reads over 100..220: A on 100 (c1), C on 110 (c1); on unit 1 A C A = alleles 0 1 0 against h1 1 0 1: 0 : 3, haplotype 2
    rs = _readset([(99, "121M", "A" + "G" * 9 + "C" + "G" * 39 + "C" + "G" * 49 + "A" + "G" * 9 + "C" + "G" * 9 + "A")] * 3)
    ul = M.unit_links(rs, chain)
    assert ul[1, 0].tolist() == [0, 3] and int(ul.sum()) == 3
    out, st, joined = M.merge(chain, ul)
    assert out["ps"].tolist() == [100, 100, -1, 100, 100, 100] and out["h1"].tolist() == [0, 1, 0, 0, 1, 0] and joined == 1
    assert st == dict(n_sites=6, n_phased=5, n_blocks=1, max_block=5)
    # with the same haplotype nothing is flipped
    out, _, joined = M.merge(chain, _ulinks(2, {(1, 1): (3, 0)}))
    assert out["ps"].tolist() == [100, 100, -1, 100, 100, 100] and out["h1"].tolist() == [0, 1, 0, 1, 0, 1] and joined == 1
    # ... and below the agreement nothing happens at all
    out, st, joined = M.merge(chain, _ulinks(2, {(1, 1): (2, 1)}))
    assert P.equal_sites(out, chain) and joined == 0 and st == dict(n_sites=6, n_phased=5, n_blocks=2, max_block=3)


def test_a_unit_eight_back_joins_and_one_nine_back_does_not():
    # ten units of one site each on 10, 20, .. 100; three reads show units 0 and 8, three show units 0 and 9
    chain = _table([(10 * (u + 1), 10 * (u + 1), 0) for u in range(10)])
    rs = _readset([(9, "1M79N1M", "AA")] * 3 + [(9, "1M89N1M", "AA")] * 3)
    ul = M.unit_links(rs, chain)
    assert ul.shape == (10, K, 2) and ul[8, 7].tolist() == [3, 0] and int(ul.sum()) == 3 and int(ul[9].sum()) == 0
    out, st, joined = M.merge(chain, ul)
    assert out["ps"].tolist() == [10, 20, 30, 40, 50, 60, 70, 80, 10, 100] and out["h1"].tolist() == [0] * 10 and joined == 1
    assert st == dict(n_sites=10, n_phased=10, n_blocks=9, max_block=2)


def test_interleaved_units_ties_and_bases_that_are_neither():
    # unit 0 (ps 100): sites 100, 120 (h1 0 0); unit 1 (ps 110): sites 110 (h1 0), 130 (h1 1); unit 2 (ps 140): site 140 (h1 0)
    chain = _table([(100, 100, 0), (110, 110, 0), (120, 100, 0), (130, 110, 1), (140, 140, 0)])

    def read(b100, b110, b120, b130, b140):
        return (99, "41M", b100 + "G" * 9 + b110 + "G" * 9 + b120 + "G" * 9 + b130 + "G" * 9 + b140)
    rs = _readset([read("A", "A", "A", "C", "A")] * 3      # 2 : 0 | 2 : 0 | 1 : 0 -> 1 1 1
                  + [read("A", "A", "A", "A", "C")] * 2    # 2 : 0 | 1 : 1 tied | 0 : 1 -> 1 - 2: unit 1 is not observed, units 0 and 2 are two apart
                  + [read("C", "G", "T", "A", "A")]        # 0 : 1 (T is neither) | 0 : 1 (G is neither) | 1 : 0 -> 2 2 1
                  + [read("A", "N", "C", "C", "N")]        # 1 : 1 tied | 1 : 0 | nothing -> - 1 -
                  + [read("A", "A", "A", "C", "A") + (256,)])      # a secondary alignment does not vote
    ul = M.unit_links(rs, chain)
    assert ul[1, 0].tolist() == [4, 0] and ul[2, 0].tolist() == [3, 1] and ul[2, 1].tolist() == [3, 3] and int(ul.sum()) == 14
    out, st, joined = M.merge(chain, ul)
    # unit 1 joins unit 0; unit 2 sees that block with 6 : 4 = 60 %: it stays
    assert out["ps"].tolist() == [100, 100, 100, 100, 140] and out["h1"].tolist() == [0, 0, 0, 1, 0] and joined == 1
    assert st == dict(n_sites=5, n_phased=5, n_blocks=2, max_block=4)
    loose = dict(min_mq=0, excl_flags=0)
    assert M.unit_links(rs, chain, loose)[1, 0].tolist() == [5, 0]


def test_levels_stop_early_and_a_second_level_joins_what_the_first_made_neighbours():
    # ten units of one site each; two reads link every unit to the one before it up to unit 8; two reads link unit 9 to unit 0 in trans
    chain = _table([(10 * (u + 1), 10 * (u + 1), 0) for u in range(10)])
    rs = _readset([(10 * (j + 1) - 1, "1M9N1M", "AA") for j in range(8) for _ in range(2)] + [(9, "1M89N1M", "AC")] * 2)
    ul = M.unit_links(rs, chain)
    assert [ul[u, 0].tolist() for u in range(10)] == [[0, 0]] + [[2, 0]] * 8 + [[0, 0]] and int(ul.sum()) == 16
    one, st1, run1, joined1 = M.merge_levels(rs, chain, 1)
    assert one["ps"].tolist() == [10] * 9 + [100] and (run1, joined1) == (1, 8) and st1 == dict(n_sites=10, n_phased=10, n_blocks=2, max_block=9)
    # second level: two units, one apart
    ul2 = M.unit_links(rs, one)
    assert ul2.shape == (2, K, 2) and ul2[1, 0].tolist() == [0, 2]
    two, st2, run2, joined2 = M.merge_levels(rs, chain, 2)
    assert two["ps"].tolist() == [10] * 10 and two["h1"].tolist() == [0] * 9 + [1] and (run2, joined2) == (2, 9)
    # a third joins nothing and a fourth does not run
    more, st4, run4, joined4 = M.merge_levels(rs, chain, 4)
    assert P.equal_sites(more, two) and (run4, joined4) == (3, 9) and st4 == st2 == dict(n_sites=10, n_phased=10, n_blocks=1, max_block=10)
    none, st0, run0, joined0 = M.merge_levels(rs, chain, 0)
    assert P.equal_sites(none, chain) and (run0, joined0) == (0, 0)


# ---- c3r_phase_merge against the restatement
def _same(got, want):
    assert P.equal_sites(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], (got, want)


def test_library_merge_on_the_known_answers():
    from clair3_rna_amd import capi
    for extra in ((), [(10, "2M28N2M", "AACC")] * 4):
        rs, chain, _ = _known(extra)
        table = chain
        for _ in range(2):
            ul = M.unit_links(rs, table)
            want = M.merge(table, ul)
            _same(capi.phase_merge(table, ul), want)
            table = want[0]
    out, st, joined = capi.phase_merge(_known()[1], _ulinks(2, {(1, 1): (0, 5)}))
    assert out["ps"].tolist() == [11, 11] + [-1] * 8 + [11, 11] and out["h1"].tolist() == [0, 1] + [0] * 8 + [1, 1] and joined == 1
    empty = capi.phase_merge(np.zeros(0, capi.PHASE_SITE_DTYPE), np.zeros((0, K, 2), np.uint32))
    assert len(empty[0]) == 0 and empty[1] == dict.fromkeys(P.STAT_KEYS, 0) and empty[2] == 0


def test_library_merge_on_two_hundred_random_tables():
    from clair3_rna_amd import capi
    rng = random.Random(77)
    total = 0
    for _ in range(200):
        n = rng.randint(1, 40)
        pos = sorted(rng.sample(range(1, 400), n))
        pool = rng.sample(range(1, 400), rng.randint(1, 14))
        rows = [(p, -1 if rng.random() < 0.25 else rng.choice(pool), rng.randint(0, 1)) for p in pos]
        table = _table(rows)
        U = len(M.units_of(table))
        ul = np.zeros((U, K, 2), np.uint32)
        for u in range(U):
            for k in range(1, min(K, u) + 1):
                if rng.random() < 0.5:
                    ul[u, k - 1] = rng.choice([(rng.randint(0, 9), rng.randint(0, 9)), (rng.randint(2, 30), 0), (0, rng.randint(2, 30)), (3, 1), (1, 1)])
        mr, pct = rng.choice([(2, 75), (2, 75), (1, 100), (0, 0), (5, 60)])
        want = M.merge(table, ul, mr, pct)
        _same(capi.phase_merge(table, ul, mr, pct), want)
        total += want[2]
    assert total > 200                                       # the comparison is about something


BAD = [
    ("ps_zero", dict(ps=(1, 0)), None),
    ("ps_below_minus_one", dict(ps=(1, -2)), None),
    ("h1_above_one", dict(h1=(0, 2)), None),
    ("positions_not_increasing", dict(pos=(2, 100)), None),
    ("one_row_too_few", {}, 1),
    ("one_row_too_many", {}, 3),
]


@pytest.mark.parametrize("name, patch, rows", BAD, ids=[b[0] for b in BAD])
def test_library_merge_refuses_bad_arguments(name, patch, rows):
    from clair3_rna_amd import capi
    table = _table([(100, 100, 0), (110, 100, 1), (120, -1, 0), (130, 130, 0)])
    for k, (j, v) in patch.items():
        table[k][j] = v
    with pytest.raises(capi.C3RError) as e:
        capi.phase_merge(table, np.zeros((rows or 2, K, 2), np.uint32))
    assert e.value.code == -1


def test_library_merge_refuses_bad_parameters_and_shapes():
    from clair3_rna_amd import capi
    table = _table([(100, 100, 0), (110, 100, 1), (120, -1, 0), (130, 130, 0)])
    ul = np.zeros((2, K, 2), np.uint32)
    assert capi.phase_merge(table, ul)[2] == 0
    for kw in (dict(min_reads=-1), dict(min_agree_pct=101), dict(min_agree_pct=-1)):
        with pytest.raises(capi.C3RError):
            capi.phase_merge(table, ul, **kw)
    with pytest.raises(ValueError):
        capi.phase_merge(table, np.zeros((2, K), np.uint32))
    with pytest.raises(TypeError):
        capi.phase_merge(np.zeros(4, np.int32), ul)


# ---- quality against the truth
@pytest.mark.parametrize("run", [9, 14])
def test_the_merge_repairs_what_editing_runs_cut(run):
    """Seeds 0-7 of gen_fragmented(run).  Measured when this was written, chain -> four levels, summed over the seeds: blocks among the true
    SNVs 20 -> 8 (run 9) and 22 -> 8 (run 14); switch errors 0 -> 0; editing sites in blocks 7 -> 7 and 32 -> 32."""
    chain_blocks = merged_blocks = 0
    for seed in range(8):
        _, rs, sites, truth, editing = M.gen_fragmented(seed, run)
        assert len(editing) == 2 * run and len(rs) == 403
        lk = P.links(rs, sites)
        chain, _ = P.resolve(sites, lk)
        merged, st = M.phase(rs, sites, lk, 4)
        qc, qm = M.quality(chain, truth, editing), M.quality(merged, truth, editing)
        print(run, seed, qc, qm, st)
        assert qc["blocks"] >= 2                             # there is something to merge
        assert not [j for j in editing if int(merged[j]["ps"]) >= 0 and int(chain[j]["ps"]) < 0]
        assert qm["editing"] == qc["editing"] and qm["phased"] == qc["phased"]
        assert qm["switches"][0] <= qc["switches"][0]
        chain_blocks += qc["blocks"]
        merged_blocks += qm["blocks"]
    assert chain_blocks >= 20 and 2 * merged_blocks <= chain_blocks


def test_without_editing_runs_the_merge_has_nothing_to_do():
    _, rs, sites, truth, editing = M.gen_fragmented(0, 0)
    assert not editing
    lk = P.links(rs, sites)
    chain, cst = P.resolve(sites, lk)
    merged, st = M.phase(rs, sites, lk, 4)
    assert P.equal_sites(merged, chain) and st["merge_units_joined"] == 0 and st["merge_levels_run"] == 1
    assert {k: st[k] for k in P.STAT_KEYS} == cst
