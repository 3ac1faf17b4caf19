"""Gene-level haplotype read counts on the device (c3r_hap_group_counts / k_hap_group_counts) against tests/hapgroupref.py, the plain-Python
restatement of the rule `hap_groups`: element for element, no tolerance; both CIGAR walks; the aggregated and the direct kernel; that the call
leaves tags, sets, count tables and scans alone; the validation paths through the C ABI; and the drivers (hap_expr --group_by_name,
call_sample --hap_expression_group_by_name)."""
import os

import numpy as np
import pytest

from clair3_rna_amd import hap_expr
from tests import hapgroupref as HG
from tests import hapref
from tests import hapregionref as HR
from tests import phaseref as P

pytestmark = pytest.mark.gpu

EINVAL = -1                                                   # C3R_EINVAL


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clean(request):
    """Every test of this module starts and leaves its engine without phase sites, with default parameters and the default kernel."""
    yield
    if "eng" in request.fixturenames:
        from clair3_rna_amd import capi
        e = request.getfixturevalue("eng")
        e.set_phase_sites(None)
        e.params = capi.default_params()
        e.set_params()
        e.set_hap_group_direct(False)


def _readset(recs):
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=r[4] if len(r) > 4 else 60, hp=0) for r in recs])


def _forced_serial(rs, every=1):
    """The same reads with an empty op (`0D`) behind the first op of every `every`-th read: an op the plain walk does not take, so those
    reads go through the serial walk, and one the rule does not see."""
    from clair3_rna_amd.reads import ReadSet
    cig, reads, off = [], rs.reads.copy(), 0
    for i, r in enumerate(rs.reads):
        c = rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])].tolist()
        if i % every == 0:
            c = c[:1] + [2] + c[1:]                              # (length 0 << 4 | D)
        reads[i]["cigar_off"], reads[i]["n_cigar"] = off, len(c)
        cig += c
        off += len(c)
    return ReadSet(reads, np.array(cig, dtype=np.uint32), rs.seq.copy())


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape
        assert np.array_equal(g, w), (np.argwhere(g != w)[:10], g[g != w][:10], w[g != w][:10])


def _check(eng, rs, table, tab, n_groups, off, row_ps, stranded=0, params=HG.DEFAULT_PARAMS, load=True, want=None):
    """The engine's two tables for (rs, table, intervals) under its current filters, from the aggregated and from the direct kernel, equal
    the restatement's under `params` (or `want`, the restatement's tables computed before); returns them."""
    want = HG.counts(rs, table, tab, n_groups, off, row_ps, stranded, params) if want is None else want
    if load:
        eng.set_phase_sites(table)
        eng.load_reads(rs)
    for direct in (False, True):
        eng.set_hap_group_direct(direct)
        assert eng.hap_group_direct() is direct
        _same(eng.hap_group_counts(tab, n_groups, off, row_ps, stranded), want)
    eng.set_hap_group_direct(False)
    return want


# ---- 1. against the restatement
@pytest.mark.parametrize("case", HG.HAND, ids=[c[0] for c in HG.HAND])
def test_the_hand_cases(eng, case):
    rs, table, tab, n_groups, off, row_ps, stranded, want_gc, want_wc = HG.hand_inputs(case)
    gc, wc = _check(eng, rs, table, tab, n_groups, off, row_ps, stranded)
    assert gc.tolist() == want_gc.tolist() and wc.tolist() == want_wc.tolist()
    gc, wc = _check(eng, _forced_serial(rs), table, tab, n_groups, off, row_ps, stranded)      # the same through the serial walk
    assert gc.tolist() == want_gc.tolist() and wc.tolist() == want_wc.tolist()


_fuzz = {}


def _fuzz_case(seed, grouping):
    """phaseref.gen_case(errors=True) with its truth as the phase table, in consecutive sets of ten sites; its exons grouped (HG.fuzz_table);
    the restatement's tables per `stranded`, computed once."""
    if (seed, grouping) not in _fuzz:
        ref, rs, sites, truth, _ = P.gen_case(seed, errors=True)
        table = sites.copy()
        table["h1"], table["ps"] = truth, 1000 + np.arange(len(table)) // 10
        n_groups, tab, off, row_ps = HG.fuzz_table(seed, grouping, table, len(ref))
        want = {0: HG.counts(rs, table, tab, n_groups, off, row_ps, 0)}
        # the pairs of the exons' groups alone (the five extra intervals are the last five groups, each met in its one interval)
        detail, n_genes = {}, n_groups - 5
        HG.counts(rs, table, tab[tab["group"] < n_genes], n_genes, np.zeros(n_genes, np.int32), np.zeros(0, np.int32), 0, detail=detail)
        _fuzz[(seed, grouping)] = dict(rs=rs, serial=_forced_serial(rs), table=table, tab=tab, n_groups=n_groups, off=off, row_ps=row_ps, want=want, detail=detail, ref=ref)
    return _fuzz[(seed, grouping)]


def _want(c, stranded):
    if stranded not in c["want"]:
        c["want"][stranded] = HG.counts(c["rs"], c["table"], c["tab"], c["n_groups"], c["off"], c["row_ps"], stranded)
    return c["want"][stranded]


@pytest.mark.parametrize("grouping", ["triples", "interleaved"])
@pytest.mark.parametrize("seed", range(4))
def test_generated_spliced_reads_over_grouped_exons(eng, seed, grouping):
    c = _fuzz_case(seed, grouping)
    d = c["detail"]
    print("seed %d %s: %d intervals in %d groups, %d rows; pairs %d, multi-interval %d, skipped-inside %d"
          % (seed, grouping, len(c["tab"]), c["n_groups"], len(c["row_ps"]), d["pairs"], d["multi_interval_pairs"], d["skipped_inside_pairs"]))
    if grouping == "triples":                                 # the fuzz is not empty: from the restatement alone (42-55 % of 511-559 pairs, and 9-18)
        assert d["multi_interval_pairs"] >= 0.3 * d["pairs"] and d["skipped_inside_pairs"] >= 5
    args = (c["table"], c["tab"], c["n_groups"], c["off"], c["row_ps"])
    gc, wc = _check(eng, c["rs"], *args, want=_want(c, 0))
    assert gc[:, 0].sum() > 0 and gc[:, 1].sum() > 0 and wc[:, 0].sum() > 50 and wc[:, 1].sum() > 50      # all four kinds of count occur
    _check(eng, c["serial"], *args, want=_want(c, 0))         # every read through the serial walk: the same tables
    stranded = 1 + seed % 2
    _check(eng, c["rs"], *args, stranded=stranded, want=_want(c, stranded))
    assert not np.array_equal(_want(c, stranded)[1], wc)      # (the genes carry strands: the switch shows)


@pytest.mark.parametrize("seed", range(2))
def test_singleton_groups_are_hap_region_counts(eng, seed):
    _, rs, table, _ = hapref.gen_case(seed)
    tab, row_ps = HR.gen_regions(seed, table)
    ivs, n_groups, off = HG.singletons(tab)
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    for stranded in (0, 1, 2):
        rc, wc = eng.hap_region_counts(tab, row_ps, stranded)
        assert rc.sum() > 1000 and wc.sum() > 500
        for direct in (False, True):
            eng.set_hap_group_direct(direct)
            gc, gw = eng.hap_group_counts(ivs, n_groups, off, row_ps, stranded)
            assert np.array_equal(gc, rc) and np.array_equal(gw, wc)


def test_more_count_words_than_lds_slots(eng):
    """One workgroup's 16 reads of 400 M bases at one start over 300 one-base groups, half of the reads untagged: 600 distinct count words,
    more than the workgroup's table holds, so some of them are added globally at once."""
    reads = [(1000, "400M", ("AA" + ("A" if k % 2 else "G") + "A" * 397), 16 * (k % 4 == 0)) for k in range(16)]
    rs = _readset(reads)
    table = hapref.make_sites([(1003, "A", "C", 0, 7)])
    tab, off, row_ps = HG.pack([(1000 + k, 1001 + k, k, 0) for k in range(300)], [[7]] * 300)
    gc, wc = _check(eng, rs, table, tab, 300, off, row_ps)
    assert gc.tolist() == [[8, 0]] * 300 and wc.tolist() == [[8, 0]] * 300
    _check(eng, _forced_serial(rs), table, tab, 300, off, row_ps)
    # the same words from two workgroups, and groups of two intervals each
    rs2 = _readset(reads + reads[:5])
    tab2, off2, row_ps2 = HG.pack([(1000 + k, 1001 + k, k % 150, 0) for k in range(300)], [[7]] * 150)
    gc, wc = _check(eng, rs2, table, tab2, 150, off2, row_ps2)
    assert gc.tolist() == [[11, 0]] * 150 and wc.tolist() == [[10, 0]] * 150


@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_read_counts_around_a_workgroup(eng, n):
    rs = _readset([(100 + k // 3, "4M20N4M", ("AAAAAAAA", "CCCCCCCC", "GGGGGGGG")[k % 3]) for k in range(n)])
    table = hapref.make_sites([(p, "A", "C", 0, 1) for p in (103, 104, 105, 106)])
    tab, off, row_ps = HG.pack([(0, 50, 0, 0), (100, 103, 1, 0), (101, 104, 2, 0), (104, 105, 3, 0), (124, 140, 1, 0), (126, 127, 3, 0)], [[], [1], [1], [2]])
    _check(eng, rs, table, tab, 4, off, row_ps)


# ---- 2. life cycle
def test_the_call_leaves_tags_sets_count_tables_and_a_scan_alone(eng):
    c = _fuzz_case(1, "triples")
    rs, table, ref = c["rs"], c["table"], c["ref"]
    args = (table, c["tab"], c["n_groups"], c["off"], c["row_ps"])
    regs = sorted((a, b, 0) for a, b in HR.phase_case_exons(1))
    rtab, rrow_ps = HR.pack(regs, HR.row_table(regs, table))
    query = table.copy()
    query["h1"] = 0
    eng.set_params(min_coverage=2)
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    eng.set_reference(1, ref)
    assert eng.params.channels == 18

    def scan():
        n = eng.scan(1, len(ref))
        return n, eng.tensors(rescaled=True).tobytes(), eng.tensors(rescaled=False).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()

    def regions():
        return tuple(x.tobytes() for x in eng.hap_region_counts(rtab, rrow_ps, 1))

    plain, tags, sets, counts, by_region = scan(), eng.haplotags(), eng.read_phase_sets().tolist(), eng.hap_counts(query).tobytes(), regions()
    assert plain[0] > 20 and tags[1]["n_hp1"] > 30 and tags[1]["n_hp2"] > 30
    eng.load_reads(rs)
    _check(eng, rs, *args, load=False, want=_want(c, 0))
    after = eng.haplotags()
    assert after[0].tolist() == tags[0].tolist() and after[1] == tags[1] and eng.read_phase_sets().tolist() == sets
    assert eng.hap_counts(query).tobytes() == counts and regions() == by_region
    assert scan() == plain
    _check(eng, rs, *args, stranded=2, load=False, want=_want(c, 2))      # after the scan: what it left is still there
    assert (eng.tensors(rescaled=True).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()) == (plain[1], plain[3], plain[4])
    assert scan() == plain and eng.hap_counts(query).tobytes() == counts and regions() == by_region
    # a second call with another table, and a call after a new load_reads
    other = _fuzz_case(1, "interleaved")
    _check(eng, rs, table, other["tab"], other["n_groups"], other["off"], other["row_ps"], load=False, want=_want(other, 0))
    c2 = _fuzz_case(0, "triples")
    eng.set_phase_sites(c2["table"])
    eng.load_reads(c2["rs"])
    _check(eng, c2["rs"], c2["table"], c2["tab"], c2["n_groups"], c2["off"], c2["row_ps"], load=False, want=_want(c2, 0))
    # the voters follow set_params: the reads already loaded are filtered anew
    eng.set_params(min_mq=30)
    gc, wc = _check(eng, c2["rs"], c2["table"], c2["tab"], c2["n_groups"], c2["off"], c2["row_ps"], params=dict(min_mq=30, excl_flags=2316), load=False)
    total = sum(int(x.sum()) for x in _want(c2, 0))
    assert 0 < int(gc.sum()) + int(wc.sum()) <= total
    eng.set_params(min_mq=0, excl_flags=0)
    gc, wc = _check(eng, c2["rs"], c2["table"], c2["tab"], c2["n_groups"], c2["off"], c2["row_ps"], params=dict(min_mq=0, excl_flags=0), load=False)
    assert int(gc.sum()) + int(wc.sum()) > total
    eng.set_params(min_mq=61)
    assert sum(int(x.sum()) for x in eng.hap_group_counts(c2["tab"], c2["n_groups"], c2["off"], c2["row_ps"])) == 0


def test_region_and_group_calls_alternate_on_their_shared_buffers(eng):
    """c3r_hap_region_counts and c3r_hap_group_counts upload into one set of device buffers.  On one engine and one loaded read set: a region
    call on table A, a group call on a smaller table B — behind which A's entries, first_open, rows and counts still lie —, then A again;
    each equals its restatement.  17 reads (a workgroup's 16 and one), every third through the serial walk."""
    rs = _forced_serial(_readset([(100 + 2 * k, "10M40N10M", "ACG"[k % 3] * 20, 16 * (k % 4 == 0)) for k in range(17)]), 3)
    table = hapref.make_sites([(105, "A", "C", 0, 1), (120, "A", "C", 1, 2), (158, "A", "C", 0, 3), (175, "A", "C", 0, 4), (186, "A", "C", 1, 5)])
    regs = [(90, 105, 0), (100, 112, 1), (104, 130, 2), (110, 111, 0), (118, 150, 0), (125, 190, 1), (140, 156, 0), (150, 165, 2), (155, 158, 0), (160, 180, 0),
            (170, 200, 1), (185, 186, 0)]
    a_tab, a_rows = HR.pack(regs, HR.row_table(regs, table))
    ivs = [(100, 110, 0, 1), (120, 135, 1, 2), (150, 160, 0, 1), (175, 192, 1, 2)]      # read 0 covers [100, 110) and [150, 160): both intervals of group 0
    b_tab, b_off, b_rows = HG.pack(ivs, HG.group_rows(ivs, 2, table))
    assert len(a_tab) == 12 and len(b_tab) < len(a_tab) and 0 < len(b_rows) < len(a_rows)
    detail = {}
    want_a = HR.counts(rs, table, a_tab, a_rows, 1)
    want_b = HG.counts(rs, table, b_tab, 2, b_off, b_rows, 1, detail=detail)
    assert detail["multi_interval_pairs"] >= 1 and all(int(w.sum()) > 0 for w in want_a + want_b)
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    for direct in (False, True):
        eng.set_hap_group_direct(direct)
        _same(eng.hap_region_counts(a_tab, a_rows, 1), want_a)
        _same(eng.hap_group_counts(b_tab, 2, b_off, b_rows, 1), want_b)
        _same(eng.hap_region_counts(a_tab, a_rows, 1), want_a)


def test_no_intervals_no_reads_and_no_table(eng):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    c = _fuzz_case(0, "triples")
    args = (c["tab"], c["n_groups"], c["off"], c["row_ps"])
    eng.load_reads(c["rs"])
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        eng.hap_group_counts(*args)
    _check(eng, c["rs"], c["table"], *args, want=_want(c, 0))      # the context is usable afterwards
    eng.set_profiling(True)
    try:
        eng.reset_kernel_stats()
        gc, wc = eng.hap_group_counts(None, 0, None, None)
        assert gc.shape == (0, 2) and wc.shape == (0, 2) and not [k for k in eng.kernel_stats() if k.startswith("k_hap_group_counts")]
        eng.hap_group_counts(*args)
        eng.set_hap_group_direct(True)
        eng.hap_group_counts(*args)
        eng.set_hap_group_direct(False)
        stats = eng.kernel_stats()
        assert stats["k_hap_group_counts"]["launches"] == 1 and stats["k_hap_group_counts_direct"]["launches"] == 1 and "k_hap_region_counts" not in stats
        eng.load_reads(ReadSet.from_records([]))
        eng.reset_kernel_stats()
        gc, wc = eng.hap_group_counts(*args)
        assert gc.shape == (c["n_groups"], 2) and wc.shape == (len(c["row_ps"]), 2) and gc.sum() == 0 and wc.sum() == 0
        assert not [k for k in eng.kernel_stats() if k.startswith("k_hap_group_counts")]
    finally:
        eng.set_profiling(False)
    # intervals far from every read, and a table without any row
    eng.load_reads(c["rs"])
    far = HG.pack([(7000, 7001, 0, 0), (2000000000, 2147483647, 0, 0)], [[1000]])
    gc, wc = eng.hap_group_counts(far[0], 1, far[1], far[2])
    assert gc.sum() == 0 and wc.sum() == 0
    none = np.zeros(c["n_groups"], np.int32)
    gc, wc = _check(eng, c["rs"], c["table"], c["tab"], c["n_groups"], none, np.zeros(0, np.int32), load=False)
    assert wc.shape == (0, 2) and gc[:, 1].sum() > 200
    eng.set_phase_sites(None)                                 # cleared: refused again
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        eng.hap_group_counts(*args)


# ---- 3. validation: (name, intervals [(start, end, group, strand)], n_groups, group_row_off, row_ps, stranded, the words that name the offender)
GOOD = ([(100, 110, 0, 1), (120, 130, 1, 0), (200, 300, 0, 1), (250, 260, 2, 2)], 3, [0, 1, 3], [1, 1, 2])
BAD = [
    ("unsorted", [(100, 110, 0, 1), (200, 300, 0, 1), (120, 130, 1, 0), (250, 260, 2, 2)], 3, [0, 1, 3], [1, 1, 2], 0, "interval 2:.*sorted"),
    ("unsorted_by_end", [(100, 110, 0, 1), (100, 105, 1, 0), (200, 300, 0, 1), (250, 260, 2, 2)], 3, [0, 1, 3], [1, 1, 2], 0, "interval 1:.*sorted"),
    ("start_not_below_end", [(100, 110, 0, 1), (120, 120, 1, 0), (200, 300, 0, 1), (250, 260, 2, 2)], 3, [0, 1, 3], [1, 1, 2], 0, r"interval 1: \[120, 120\)"),
    ("negative_start", [(-1, 110, 0, 1), (120, 130, 1, 0), (200, 300, 0, 1), (250, 260, 2, 2)], 3, [0, 1, 3], [1, 1, 2], 0, r"interval 0: \[-1, 110\)"),
    ("group_too_large", [(100, 110, 0, 1), (120, 130, 3, 0), (200, 300, 0, 1), (250, 260, 2, 2)], 3, [0, 1, 3], [1, 1, 2], 0, "interval 1: group 3 is not in"),
    ("group_negative", [(100, 110, 0, 1), (120, 130, 1, 0), (200, 300, 0, 1), (250, 260, -1, 2)], 3, [0, 1, 3], [1, 1, 2], 0, "interval 3: group -1 is not in"),
    ("group_without_an_interval", [(100, 110, 0, 1), (120, 130, 0, 1), (200, 300, 0, 1), (250, 260, 2, 2)], 3, [0, 1, 3], [1, 1, 2], 0, "group 1: no interval"),
    ("overlap_in_one_group", [(100, 110, 0, 1), (120, 130, 1, 0), (200, 300, 0, 1), (250, 260, 0, 1)], 2, [0, 1], [1, 1, 2], 0, "interval 3:.*overlaps interval 2"),
    ("two_strands_in_one_group", [(100, 110, 0, 1), (120, 130, 1, 0), (200, 300, 0, 2), (250, 260, 2, 2)], 3, [0, 1, 3], [1, 1, 2], 0, "interval 2: strand 2.*interval 0"),
    ("strand_3", [(100, 110, 0, 1), (120, 130, 1, 3), (200, 300, 0, 1), (250, 260, 2, 2)], 3, [0, 1, 3], [1, 1, 2], 0, "interval 1: strand must be"),
    ("row_off_not_0_at_group_0", GOOD[0], 3, [1, 1, 3], [1, 1, 2], 0, "group 0: group_row_off 1"),
    ("row_off_decreases", GOOD[0], 3, [0, 2, 1], [1, 2, 2], 0, "group 2: group_row_off 1"),
    ("row_off_above_n_rows", GOOD[0], 3, [0, 1, 4], [1, 1, 2], 0, "group 2: group_row_off 4"),
    ("negative_ps", GOOD[0], 3, [0, 1, 3], [1, -1, 2], 0, r"row 1 \(group 1\): phase set -1"),
    ("ps_not_increasing", GOOD[0], 3, [0, 1, 3], [1, 2, 2], 0, r"row 2 \(group 1\):.*strictly increasing"),
    ("stranded_3", GOOD[0], 3, [0, 1, 3], [1, 1, 2], 3, "stranded 3"),
    ("stranded_negative", GOOD[0], 3, [0, 1, 3], [1, 1, 2], -1, "stranded -1"),
]


def _table(intervals, off, row_ps):
    from clair3_rna_amd import capi
    tab = np.zeros(len(intervals), dtype=capi.HAP_INTERVAL_DTYPE)
    for j, e in enumerate(intervals):
        tab[j]["start"], tab[j]["end"], tab[j]["group"], tab[j]["strand"] = e
    return tab, np.array(off, dtype=np.int32), np.array(row_ps, dtype=np.int32)


@pytest.fixture()
def loaded(eng):
    eng.set_phase_sites(hapref.make_sites([(1, "A", "C", 0, 1)]))
    eng.load_reads(_readset([(90, "40M", "A" * 40)]))
    return eng


@pytest.mark.parametrize("name, intervals, n_groups, off, row_ps, stranded, words", BAD, ids=[b[0] for b in BAD])
def test_bad_tables_name_the_offender(loaded, name, intervals, n_groups, off, row_ps, stranded, words):
    from clair3_rna_amd import capi
    tab, off, row_ps = _table(intervals, off, row_ps)
    with pytest.raises(capi.C3RError, match=words) as e:
        loaded.hap_group_counts(tab, n_groups, off, row_ps, stranded)
    assert e.value.code == EINVAL
    tab, off, row_ps = _table(GOOD[0], GOOD[2], GOOD[3])      # the context is usable afterwards: the read covers [90, 130), untagged
    assert loaded.hap_group_counts(tab, GOOD[1], off, row_ps)[0].tolist() == [[1, 0], [1, 0], [0, 0]]


def test_the_other_refusals(loaded):
    from clair3_rna_amd import capi
    tab, off, row_ps = _table(GOOD[0], GOOD[2], GOOD[3])
    bad = tab.copy()
    bad["reserved"][2][1] = 1
    with pytest.raises(capi.C3RError, match="interval 2:.*reserved"):
        loaded.hap_group_counts(bad, 3, off, row_ps)
    # 2^24 rows in one group
    with pytest.raises(capi.C3RError, match="group 0: 16777216 rows"):
        loaded.hap_group_counts(tab[:1], 1, [0], np.arange(1 << 24, dtype=np.int32))
    # the bound of hap_regions on the interval table: one interval open over MAX_BACK + 1 later ones
    n = capi.HAP_REGION_MAX_BACK + 1
    over = _table([(0, 3 * n, 0, 0)] + [(10 + 2 * k, 11 + 2 * k, 1, 0) for k in range(n)], [0, 0], [])
    with pytest.raises(capi.C3RError, match="interval %d:.*C3R_HAP_REGION_MAX_BACK" % n):
        loaded.hap_group_counts(over[0], 2, over[1], over[2])
    under = _table([(0, 3 * n, 0, 0)] + [(10 + 2 * k, 11 + 2 * k, 1, 0) for k in range(n - 1)], [0, 0], [])
    assert loaded.hap_group_counts(under[0], 2, under[1], under[2])[0].tolist() == [[1, 0], [1, 0]]      # (the read covers [90, 130))
    # rows or groups and no interval; the switch; the wrapper's own checks
    with pytest.raises(capi.C3RError, match="no interval"):
        loaded.hap_group_counts(None, 1, [0], None)
    assert loaded.L.c3r_set_hap_group_direct(loaded.h, 2) == EINVAL and "c3r_set_hap_group_direct: 2" in loaded.L.c3r_last_error(loaded.h).decode()
    assert loaded.L.c3r_set_hap_group_direct(loaded.h, -1) == EINVAL and loaded.hap_group_direct() is False
    with pytest.raises(TypeError):
        loaded.hap_group_counts(np.zeros(2, np.int32), 1, [0], None)
    with pytest.raises(TypeError):
        loaded.hap_group_counts(tab, 3, off[:2], row_ps)
    loaded.set_phase_sites(None)
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        loaded.hap_group_counts(tab, 3, off, row_ps)


# ---- 4. drivers
def _gene_sample(d):
    s = HR.driver_sample(d)
    s["gene_bed_fn"] = os.path.join(d, "genes.bed")
    HG.write_gene_bed(s["gene_bed_fn"])
    return s


def test_hap_expr_group_by_name_writes_the_restatements_table(tmp_path):
    s = _gene_sample(str(tmp_path))
    out = str(tmp_path / "genes.tsv")
    msgs = []
    base = ["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["gene_bed_fn"], "--output_fn", out]
    done = hap_expr.Run(hap_expr.build_parser().parse_args(base + ["--group_by_name"]), log=msgs.append)
    got = open(out).read().split("\n")
    want = HG.predicted_lines(s, "chr1") + HG.uncounted_lines("chr2") + HG.uncounted_lines("chrEmpty")
    assert got[0] == hap_expr.GROUP_HEADER and got[-1] == "" and got[1:-1] == want
    assert sorted(done) == ["chr1", "chr2", "chrEmpty"] and done["chr1"]["launched"] and done["chr1"]["groups"] == 5
    assert len([m for m in msgs if m.startswith("[WARNING]")]) == 1 and len([m for m in msgs if m.startswith("[INFO]")]) == 3
    hap_expr.Run(hap_expr.build_parser().parse_args(base + ["--group_by_name", "--stranded", "same", "--ctg_name", "chr1"]), log=msgs.append)
    assert open(out).read().split("\n")[1:-1] == HG.predicted_lines(s, "chr1", stranded=1) != want[:len(HG.predicted_lines(s, "chr1"))]
    # without the flag the same BED still gives the lines the region restatement predicts
    hap_expr.Run(hap_expr.build_parser().parse_args(base), log=msgs.append)
    sr = dict(s, bed=HG.GENE_BED)
    got = open(out).read().split("\n")
    assert got[0] == hap_expr.HEADER and got[1:-1] == HR.predicted_lines(sr, "chr1") + HR.uncounted_lines(sr, "chr2") + HR.uncounted_lines(sr, "chrEmpty")


def test_call_sample_with_the_flag_equals_the_stand_alone_run(tmp_path):
    from clair3_rna_amd import bam, bamio, call_sample, io, synth
    tmp = str(tmp_path)
    ref, rs, _, _ = hapref.gen_case(11)
    fa, wfn, bed_fn, bam_fn = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model"), os.path.join(tmp, "genes.bed"), os.path.join(tmp, "plain.bam")
    io.write_fasta(fa, [("chr1", ref)])
    np.save(wfn + ".c3rw.npy", synth.random_weights(30, seed=5))
    np.save(wfn + "18.c3rw.npy", synth.random_weights(18, seed=5))
    bed = {"chr1": [(3000, 3400, "g1", "+"), (100, 900, "g2", "-"), (1500, 1501, ".", None), (3300, 3600, "g1", "+"), (4000, 4800, "g2", "-"), (4500, 5000, "g3", None)]}
    with open(bed_fn, "w") as f:
        for a, b, label, strand in bed["chr1"]:
            f.write("chr1\t%d\t%d\t%s\t0\t%s\n" % (a, b, label, strand or "."))
    bam.write_bam(bam_fn, [("chr1", len(ref))], {"chr1": rs})
    bamio.index_build(bam_fn)
    out = os.path.join(tmp, "out")
    argv = ["--bam_fn", bam_fn, "--ref_fn", fa, "--output_dir", out, "--pileup_model_path", wfn + "18", "--phased_pileup_model_path", wfn, "--chunk_num", "3",
            "--min_coverage", "2", "--enable_phasing_model", "--phasing", "builtin", "--hap_expression_bed", bed_fn, "--hap_expression_stranded", "reverse",
            "--hap_expression_group_by_name"]
    assert call_sample.Run(call_sample.build_parser().parse_args(argv), log=lambda m: None) == 0
    tsv = os.path.join(out, "output_enable_phasing_hap_expression_by_name.tsv")
    assert os.path.isfile(tsv) and not os.path.exists(os.path.join(out, "output_enable_phasing_hap_expression.tsv"))
    per = os.path.join(out, "tmp", "phased_output", "phased_vcf")
    by_hand = str(tmp_path / "by_hand.tsv")
    hap_expr.Run(hap_expr.build_parser().parse_args(["--bam_fn", bam_fn, "--phased_vcf_fn", per, "--regions_bed_fn", bed_fn, "--output_fn", by_hand, "--stranded", "reverse",
                                                     "--group_by_name"]), log=lambda m: None)
    assert open(tsv).read() == open(by_hand).read()
    # and the restatement's prediction from the phased VCF the built-in phasing left
    from clair3_rna_amd import phasedvcf
    table = phasedvcf.contig_sites(per, "chr1")
    want = HG.predicted_lines(dict(reads={"chr1": rs}, case={}), "chr1", bed, stranded=2, table=table)
    got = open(tsv).read().split("\n")
    assert got[0] == hap_expr.GROUP_HEADER and got[1:-1] == want
    tagged = sum(int(l.split("\t")[8]) + int(l.split("\t")[9]) for l in want if l.split("\t")[7] != ".")
    print("phased sites %d, reads counted on a haplotype %d" % (len(table), tagged))
    assert len(table) >= 2 and tagged >= 10                   # the comparison is about something
