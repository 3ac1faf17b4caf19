"""Phasing over an allele table on the device (c3r_phase_allele_links / k_phase_allele_links, c3r_phase_allele_unit_links /
k_phase_allele_unit_links) against tests/phaseindelref.py, the plain-Python restatement; that the calls leave a set table, the tags and the
scans alone; and the drivers (phase_vcf --indels, call_sample --phasing builtin --phasing_indels)."""
import gzip
import os
import random

import numpy as np
import pytest

from tests import hapalleleref as HA
from tests import hapindelref as HI
from tests import helpers as H
from tests import phaseindelref as PI
from tests import phasemergeref as PM
from tests import phaseref as P

pytestmark = pytest.mark.gpu

K = P.K
NONE = HA.NONE
_state = {}


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clean(request):
    """Every test of this module starts and leaves its engine without a phase table and with default parameters."""
    yield
    if "eng" in request.fixturenames:
        from clair3_rna_amd import capi
        e = request.getfixturevalue("eng")
        e.set_phase_sites(None)
        e.params = capi.default_params()
        e.set_params()


def _readset(recs):
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=r[4] if len(r) > 4 else 60, hp=0) for r in recs])


def _snv(pos, ref, alt):
    return dict(pos=pos, ps=0, A=(ref, NONE), B=(alt, NONE), ref=ref, alt=alt)


def _row(pos, ref, alt, gt="0/1"):
    s = HA.site_of_row(pos, ref, alt, gt)
    assert not isinstance(s, str), (pos, ref, alt, s)
    return s


def _check(eng, rs, sites, params=P.DEFAULT_PARAMS, lead=0, load=True):
    """The engine's link table for (rs, sites) under its current filters equals the restatement's under `params`; returns it."""
    exp = PI.links(rs, sites, params)
    if load:
        eng.load_reads(rs)
    q, pool = HA.to_query(sites, lead)
    got = eng.phase_allele_links(q, pool)
    assert got.shape == (len(sites), K, 2) and got.dtype == np.uint32
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    return exp


def _check_units(eng, rs, sites, ps, h1, params=P.DEFAULT_PARAMS, lead=0, load=True):
    exp = PI.unit_links(rs, sites, ps, h1, params)
    if load:
        eng.load_reads(rs)
    q, pool = HA.to_query(sites, lead)
    q["ps"] = ps
    got = eng.phase_allele_unit_links(q, np.array(h1, np.uint8), pool)
    assert got.shape == exp.shape and np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    return exp


def _split(sites, ps, every=6):
    """The chain's blocks cut into units of `every` consecutive table sites (the generated reads link nearly everything into one block, and
    one unit launches nothing)."""
    return [sites[(j // every) * every]["pos"] if ps[j] >= 0 else -1 for j in range(len(sites))]


def _gen(seed):
    """hapalleleref.gen_case(seed, errors=True) as one table of SNVs and planted sites, with the restatement's link table, computed once."""
    if seed not in _state:
        ref, rs, rows, truth, planted, _ = HA.gen_case(seed, errors=True)
        sites, tr, is_snv = PI.table_of_case(rows, truth, planted)
        _state[seed] = (ref, rs, sites, tr, is_snv, PI.links(rs, sites))
    return _state[seed]


# ---- 1. generated cases
@pytest.mark.parametrize("seed", range(4))
def test_generated_cases(eng, seed):
    _, rs, sites, _, is_snv, exp = _gen(seed)
    assert len(rs) == 403 and sum(is_snv) >= 100 and len(sites) - sum(is_snv) >= 40
    indel = [j for j, s in enumerate(sites) if not is_snv[j]]
    assert int(exp[indel].sum()) > 300 and int(exp[:, :, 1].sum()) > 100 and int(exp[:, K - 1].sum()) > 0
    eng.load_reads(rs)
    q, pool = HA.to_query(sites, seed % 2)                   # (odd seeds: every insertion's offset in the pool is odd)
    got = eng.phase_allele_links(q, pool)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    # the resolved table, and the unit links after the chain
    ps, h1, st = PI.resolve(sites, exp)
    gps, gh1, gst = eng.phase_allele_sites(q, pool)
    assert gps.tolist() == ps and gh1.tolist() == h1 and gst == st and st["n_phased"] > len(sites) // 2
    assert gps.dtype == np.int32 and gh1.dtype == np.uint8
    ul = _check_units(eng, rs, sites, ps, h1, lead=seed % 2, load=False)
    assert len(ul) == st["n_blocks"]
    flipped = [h ^ ((j // 6) % 2) for j, h in enumerate(h1)]                      # (every other unit turned over: its links become trans)
    cut = _check_units(eng, rs, sites, _split(sites, ps), flipped, lead=seed % 2, load=False)
    assert len(cut) >= 25 and int(cut.sum()) > 1000 and int(cut[:, :, 1].sum()) > 0 and int(cut[:, K - 1].sum()) > 0
    # and with merge levels
    wps, wh1, wst = PI.phase(rs, sites, 2)
    gps, gh1, gst = eng.phase_allele_sites(q, pool, merge_levels=2)
    assert gps.tolist() == wps and gh1.tolist() == wh1 and gst == wst and "merge_levels_run" in gst


# ---- 2. an SNV-only table gives the words of the SNV kernels
def test_an_snv_only_table_gives_the_words_of_phase_links(eng):
    from clair3_rna_amd import capi
    _, rs, sites, _, _ = P.gen_case(0)
    eng.load_reads(rs)
    old = eng.phase_links(sites)
    new = eng.phase_allele_links(capi.hap_sites_from_snvs(sites))
    assert np.array_equal(old, new) and int(old.sum()) > 1000
    out, st = eng.phase_sites(sites)
    ps, h1, st2 = eng.phase_allele_sites(capi.hap_sites_from_snvs(sites))
    assert ps.tolist() == out["ps"].tolist() and h1.tolist() == out["h1"].tolist() and st == st2
    # blocks of ten consecutive sites, oriented by the chain's h1: many units a read
    out["ps"] = sites["pos"][(np.arange(len(sites)) // 10) * 10]
    q = capi.hap_sites_from_snvs(out)
    uold = eng.phase_unit_links(out)
    unew = eng.phase_allele_unit_links(q, np.ascontiguousarray(out["h1"]))
    assert np.array_equal(uold, unew) and int(uold.sum()) > 100 and len(uold) == (len(sites) + 9) // 10


# ---- 3. the serial walk
def test_reads_that_take_the_serial_walk(eng):
    from clair3_rna_amd.reads import ReadSet
    from tests.test_gpu_phase import _takes_serial_walk
    seed = 4100
    ref, recs = H._case(seed, phased=False)
    rng = random.Random(9100 + seed)
    covered = set()
    for r in recs:
        covered.update(range(r["pos"] + 1, r["pos"] + H.cigar_ref_len(r["cigar"]) + 1))
    # every op's last base (an event can only show there) and a sample of the other covered positions
    import re
    last = set()
    for r in recs:
        x = r["pos"]
        for n, o in re.findall(r"(\d+)([MIDNSHP=X])", r["cigar"]):
            if o in "M=X" and int(n):
                last.add(x + int(n))
            if o in "MDN=X":
                x += int(n)
    pos = sorted(set(rng.sample(sorted(last), min(40, len(last)))) | set(rng.sample(sorted(covered), min(40, len(covered)))))
    sites = []
    for k, p in enumerate(pos):
        b = ref[p - 1].upper() if ref[p - 1].upper() in "ACGT" else "A"
        o = "ACGT"[("ACGT".index(b) + 1) % 4]
        kind = k % 4
        sites.append(_snv(p, b, o) if kind == 0 else _row(p, b, b + rng.choice("ACGT") * rng.randint(1, 2)) if kind == 1
                     else _row(p, b + "A" * rng.randint(1, 3), b) if kind == 2 else _row(p, b + "AA", o + "AA," + b, "1/2"))
    rs = ReadSet.from_records(recs)
    serial = [_takes_serial_walk(r["cigar"]) for r in recs]
    assert sum(serial) >= 5 and sum(serial) < len(recs)
    exp = _check(eng, rs, sites, lead=1)
    assert int(exp.sum()) > 50
    only = ReadSet.from_records([r for r, s in zip(recs, serial) if s])
    assert int(_check(eng, only, sites).sum()) > 0
    ps = [sites[(j // 4) * 4]["pos"] for j in range(len(sites))]
    h1 = [j % 2 for j in range(len(sites))]
    assert int(_check_units(eng, rs, sites, ps, h1).sum()) > 0


# ---- 4. hand-made events on an op's last base.  Every read starts on 0-based 100; an SNV A>C on 1-based 106 (the read shows A: allele 0) stands
# before the site on 1-based 111, so the site's column shows as cis (column 0) or trans (column 1) in links[1][0], or as nothing.
B11 = "TTTTTATTTTG"                                           # the read's first 11 bases: A on 106, G on 111
EVENTS = [
    ("matching_insertion", _row(111, "G", "GTT"), [("11M2I5M", B11 + "TT" + "CCCCC")], [0, 1]),
    ("one_base_differs", _row(111, "G", "GTT"), [("11M2I5M", B11 + "TA" + "CCCCC")], [0, 0]),
    ("no_event_is_ref", _row(111, "G", "GTT"), [("16M", B11 + "CCCCC")], [1, 0]),
    ("cut_off_by_l_seq", _row(111, "G", "GTT"), [("11M2I5M", B11 + "TT" + "CCCCC", 12)], [0, 0]),
    ("insertion_then_deletion", _row(111, "G", "GTT"), [("11M2I3D5M", B11 + "TT" + "CCCCC")], [0, 0]),
    ("deletion", _row(111, "GAC", "G"), [("11M2D5M", B11 + "CCCCC")], [0, 1]),
    ("deletion_of_the_wrong_length", _row(111, "GAC", "G"), [("11M3D5M", B11 + "CCCCC")], [0, 0]),
    ("3M2=_anchor_on_the_third_base", _row(111, "G", "GTT"), [("8X3M2=", B11 + "CC")], [1, 0]),
    ("3M2=_then_the_insertion", _row(113, "C", "CTT"), [("8X3M2=2I3M", B11 + "CC" + "TT" + "GGG")], [0, 1]),
    ("two_insertions_of_different_parity", _row(111, "G", "GT,GCA", "1/2"), [("11M1I5M", B11 + "T" + "CCCCC"), ("11M2I5M", B11 + "CA" + "CCCCC"),
                                                                              ("11M2I5M", B11 + "CT" + "CCCCC")], [1, 1]),
    ("anchor_under_a_deletion", _row(111, "G", "GTT"), [("9M3D5M", B11[:9] + "CCCCC")], [0, 0]),
    ("anchor_under_a_ref_skip", _row(111, "G", "GTT"), [("9M3N5M", B11[:9] + "CCCCC")], [0, 0]),
]


@pytest.mark.parametrize("name, site, reads, want", EVENTS, ids=[e[0] for e in EVENTS])
def test_hand_made_events(eng, name, site, reads, want):
    rs = _readset([(100, r[0], r[1]) for r in reads])
    for i, r in enumerate(reads):
        if len(r) > 2:
            rs.reads["l_seq"][i] = r[2]
    sites = [_snv(106, "A", "C"), site]
    for lead in (0, 1):
        exp = _check(eng, rs, sites, lead=lead)
        assert exp[1, 0].tolist() == want and int(exp.sum()) == sum(want)


# ---- 5. more than 256 sites in a read's range
def test_three_windows_per_read_with_pairs_across_the_seams(eng):
    rng = random.Random(15)
    L = 720
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    alt = ["ACGT"[("ACGT".index(b) + 1 + rng.randrange(3)) % 4] for b in ref]
    sites = [(_row(p + 1, ref[p:p + 2], ref[p]) if p % 5 == 0 else _snv(p + 1, ref[p], alt[p])) for p in range(L - 1)]
    recs = []
    for n in range(40):
        start = 0 if n == 0 else rng.randrange(0, 100)
        ops, x, left = [], start, 600
        while left > 0:                                       # M runs that end on a deletion site now and then, where the read then deletes one base
            run = min(left, rng.randrange(40, 200))
            end = x + run
            if n % 2 == 0:
                run = left
                end = x + run
            if n % 2 and left - run > 5:
                end -= (end - 1) % 5                          # the run's last base lies on 0-based p with p % 5 == 0
                run = end - x
                ops += [("M", run), ("D", 1)]
                x, left = end + 1, left - run
            else:
                ops.append(("M", run))
                x, left = end, left - run
        hap = n % 2
        seq, x = [], start
        for op, ln in ops:
            if op == "M":
                seq += [rng.choice("ACGT") if rng.random() < 0.05 else (alt[y] if (y * 7 + hap) % 3 == 0 and y % 5 else ref[y]) for y in range(x, x + ln)]
            x += ln
        assert x < L
        recs.append((start, "".join("%d%s" % (ln, op) for op, ln in ops), "".join(seq)))
    rs = _readset(recs)
    assert recs[0][1] == "600M"
    exp = _check(eng, rs, sites)
    dele = exp[[j for j in range(L - 1) if j % 5 == 0]]
    assert int(dele[:, :, 1].sum()) > 50                      # the deleting reads show allele B there: trans to their neighbours
    # the first read's seams lie at its sites 256 and 504 (windows advance by 256 - K): every k is counted on both sides
    alone = _check(eng, _readset(recs[:1]), sites)
    for j in list(range(247, 257)) + list(range(495, 505)) + [257, 263, 505, 511]:
        for k in range(K):
            pair_seen = all(PI.seen_of(_readset(recs[:1]), 0, {s["pos"]: (i, s) for i, s in enumerate(sites)}).get(t) is not None for t in (j, j - k - 1))
            assert int(alone[j, k].sum()) == int(pair_seen), (j, k)
    assert int(alone.sum()) > 500 * K * 0.8


# ---- 6. the group and workgroup edges of the barrier loop
@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_read_counts_at_the_group_edges(eng, n):
    from clair3_rna_amd.reads import ReadSet
    _, rs, sites, _, _, _ = _gen(0)
    idx = [i for i in range(len(rs)) if P.votes(rs.reads[i], P.DEFAULT_PARAMS)]
    recs = []
    for k in range(n):
        if k % 4 == 3:                                        # a read with no site in range, between the others
            recs.append(dict(pos=5990, cigar="8M", seq="ACGTACGT", flag=0, mapq=60, hp=0))
            continue
        i = idx[(k * 7) % len(idx)]
        r = rs.reads[i]
        recs.append(dict(pos=int(r["pos"]), cigar="".join("%d%s" % (ln, op) for op, ln in HA.read_ops(rs, i)),
                         seq="".join("=ACMGRSVTWYHKDBN"[HA.code_at(rs, i, t)] for t in range(int(r["l_seq"]))), flag=0, mapq=60, hp=0))
    recs.sort(key=lambda r: r["pos"])
    few = ReadSet.from_records(recs)
    exp = _check(eng, few, sites)
    assert int(exp.sum()) > 0
    ps, h1, _ = PI.resolve(sites, _gen(0)[5])
    assert int(_check_units(eng, few, sites, _split(sites, ps), h1, load=False).sum()) > 0


# ---- 7. one pair under many reads
def test_one_site_pair_under_five_thousand_reads(eng):
    recs = [(100, "2M2I3M", "AG" "TT" "CCC")] * 5000
    sites = [_snv(101, "A", "C"), _row(102, "G", "GTT")]
    exp = _check(eng, _readset(recs), sites)
    assert exp[1, 0].tolist() == [0, 5000] and int(exp.sum()) == 5000


# ---- 8. the filters
def test_the_filters_decide_who_votes(eng):
    _, rs, sites, _, _, exp = _gen(0)
    assert sum(1 for i in range(len(rs)) if not P.votes(rs.reads[i], P.DEFAULT_PARAMS)) >= 20
    q, pool = HA.to_query(sites)
    eng.load_reads(rs)
    assert np.array_equal(eng.phase_allele_links(q, pool), exp)
    eng.set_params(min_mq=0, excl_flags=0)                    # the reads already loaded are filtered anew
    loose = dict(min_mq=0, excl_flags=0)
    got = eng.phase_allele_links(q, pool)
    assert not np.array_equal(got, exp) and np.array_equal(got, PI.links(rs, sites, loose))
    ps, h1, _ = PI.resolve(sites, exp)
    ps = _split(sites, ps)
    _check_units(eng, rs, sites, ps, h1, loose, load=False)
    eng.set_params(min_mq=5, excl_flags=2316 | 16)            # the reverse strand drops out
    strict = dict(min_mq=5, excl_flags=2316 | 16)
    _check(eng, rs, sites, strict, load=False)
    _check_units(eng, rs, sites, ps, h1, strict, load=False)


# ---- 9. nothing to do
def test_no_sites_no_reads_and_sites_outside_every_read(eng):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    _, rs, sites, _, _, exp = _gen(0)
    q, pool = HA.to_query(sites)
    ps, h1, _ = PI.resolve(sites, exp)
    ps = _split(sites, ps)
    qq = q.copy()
    qq["ps"] = ps
    eng.load_reads(rs)
    eng.set_profiling(True)
    try:
        eng.reset_kernel_stats()
        none = eng.phase_allele_links(np.zeros(0, capi.HAP_SITE_DTYPE))
        assert none.shape == (0, K, 2)
        assert eng.phase_allele_unit_links(None, None).shape == (0, K, 2)
        gps, gh1, st = eng.phase_allele_sites(None)
        assert len(gps) == 0 and len(gh1) == 0 and st == dict.fromkeys(P.STAT_KEYS, 0)
        one = qq.copy()
        one["ps"] = np.where(np.array(ps) >= 0, 7, -1)        # a single unit: nothing to link, nothing launched
        assert eng.phase_allele_unit_links(one, np.array(h1, np.uint8), pool).tolist() == np.zeros((1, K, 2), int).tolist()
        assert not any(k.startswith("k_phase") for k in eng.kernel_stats())
        eng.phase_allele_links(q, pool)
        eng.phase_allele_unit_links(qq, np.array(h1, np.uint8), pool)
        stats = eng.kernel_stats()
        assert stats["k_phase_allele_links"]["launches"] == 1 and stats["k_phase_allele_unit_links"]["launches"] == 1
        assert "k_phase_links" not in stats and "k_phase_unit_links" not in stats and "k_haplotag_alleles" not in stats
    finally:
        eng.set_profiling(False)
    far = [_row(p, "A", "AT") for p in (7000, 7001, 7002, 9000, 2000000000)]
    assert _check(eng, rs, far).sum() == 0
    before = [_row(1, "A", "AT"), _snv(2, "A", "C"), _row(3, "AC", "A")]
    shifted = ReadSet(rs.reads.copy(), rs.cigar, rs.seq)
    shifted.reads["pos"] += 100
    assert _check(eng, shifted, before).sum() == 0
    eng.load_reads(ReadSet.from_records([]))
    assert eng.phase_allele_links(q, pool).sum() == 0 and eng.phase_allele_links(q, pool).shape == (len(sites), K, 2)
    ul = eng.phase_allele_unit_links(qq, np.array(h1, np.uint8), pool)
    assert ul.sum() == 0 and len(ul) == len({p for p in ps if p >= 0})


# ---- 10. bad tables
GOOD = [_snv(30, "A", "C"), _row(31, "A", "AGT"), _row(40, "C", "T,CGG", "1/2"), _row(50, "ACC", "A")]
BAD = [
    ("unsorted", 2, lambda q: q["pos"].__setitem__(2, 31)),
    ("pos_below_1", 0, lambda q: q["pos"].__setitem__(0, 0)),
    ("flag_not_0_1", 1, lambda q: q["event_matters"].__setitem__(1, 2)),
    ("bad_base_code", 3, lambda q: q["b_base"].__setitem__(3, 3)),
    ("unknown_kind", 1, lambda q: q["b_kind"].__setitem__(1, 3)),
    ("indel_of_length_0", 3, lambda q: q["b_len"].__setitem__(3, 0)),
    ("length_on_kind_none", 0, lambda q: q["a_len"].__setitem__(0, 1)),
    ("insertion_past_the_pool", 2, lambda q: q["b_ins_off"].__setitem__(2, 3)),
    ("same_alleles", 0, lambda q: q["b_base"].__setitem__(0, 1)),
]


@pytest.mark.parametrize("name, index, patch", BAD, ids=[b[0] for b in BAD])
def test_bad_tables_name_the_index(eng, name, index, patch):
    from clair3_rna_amd import capi
    q, pool = HA.to_query(GOOD)
    patch(q)
    h1 = np.zeros(len(q), np.uint8)
    eng.load_reads(_readset([(0, "60M", "A" * 60)]))
    with pytest.raises(capi.C3RError, match="candidate site %d:" % index):
        eng.phase_allele_links(q, pool)
    q["ps"] = 30
    with pytest.raises(capi.C3RError, match="unit site %d:" % index):
        eng.phase_allele_unit_links(q, h1, pool)


def test_bad_pool_ps_h1_and_capacity(eng):
    import ctypes as C
    from clair3_rna_amd import capi
    q, pool = HA.to_query(GOOD)
    eng.load_reads(_readset([(0, "60M", "A" * 60)] * 3))
    bad_pool = pool.copy()
    bad_pool[0] = 0x30 | (bad_pool[0] & 15)                   # the first inserted base of site 1 is no base code
    with pytest.raises(capi.C3RError, match="candidate site 1:"):
        eng.phase_allele_links(q, bad_pool)
    # ps is ignored by the site links: a negative one is accepted
    q["ps"] = [-7, -1, -2000000000, 5]
    got = eng.phase_allele_links(q, pool)
    assert got[1, 0].tolist() == [3, 0] and got[3, 2].tolist() == [3, 0]          # the reads copy the reference: allele A everywhere but on the 1/2 site
    # the unit links have a rule for ps and h1
    h1 = np.zeros(len(q), np.uint8)
    for ps, index in (([30, 0, 30, 30], 1), ([30, 30, -2, 30], 2)):
        q["ps"] = ps
        with pytest.raises(capi.C3RError, match="unit site %d: ps" % index):
            eng.phase_allele_unit_links(q, h1, pool)
    q["ps"] = [30, 30, 50, 50]
    h1[3] = 2
    with pytest.raises(capi.C3RError, match="unit site 3: h1"):
        eng.phase_allele_unit_links(q, h1, pool)
    h1[3] = 0
    assert eng.phase_allele_unit_links(q, h1, pool).shape == (2, K, 2)
    # cap_units too small, and the count-only call
    u, out = C.c_int64(0), np.zeros((1, K, 2), np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert eng.L.c3r_phase_allele_unit_links(eng.h, ptr(q), ptr(h1), len(q), ptr(pool), 2 * len(pool), None, 0, C.byref(u)) == 0 and u.value == 2
    rc = eng.L.c3r_phase_allele_unit_links(eng.h, ptr(q), ptr(h1), len(q), ptr(pool), 2 * len(pool), ptr(out), 1, C.byref(u))
    assert rc == -6 and b"2 units do not fit 1 slots" in eng.L.c3r_last_error(eng.h)
    with pytest.raises(TypeError):
        eng.phase_allele_unit_links(q, h1[:2], pool)


# ---- 11. the calls leave everything else alone
def _scan_bytes(eng, ref):
    n = eng.scan(1, len(ref))
    return n, eng.tensors(rescaled=True).tobytes(), eng.tensors(rescaled=False).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()


@pytest.mark.parametrize("table", ["set_phase_sites", "set_phase_alleles"])
def test_a_set_table_the_tags_and_the_scans_are_unchanged(eng, table):
    from clair3_rna_amd import capi
    ref, rs, sites, truth, is_snv, exp = _gen(1)
    if table == "set_phase_sites":
        t = P.make_sites([(s["pos"], s["ref"], s["alt"]) for s, v in zip(sites, is_snv) if v])
        t["ps"], t["h1"] = 1000 + np.arange(len(t)) // 10, [v for v, k in zip(truth, is_snv) if k]
        eng.set_phase_sites(t)
    else:
        tagged = [dict(s, ps=1000 + j // 10, h1=truth[j]) for j, s in enumerate(sites)]
        eng.set_phase_alleles(*HI.to_engine(tagged, 3))
    eng.load_reads(rs)
    eng.set_reference(1, ref)
    tags, sets = eng.haplotags(), eng.read_phase_sets().tolist()
    assert tags[1]["n_hp1"] > 50 and tags[1]["n_hp2"] > 50
    # a query under the set table, with a pool of its own
    query = [dict(s, ps=1000 + j // 10) for j, s in enumerate(sites) if not is_snv[j]]
    cq, cpool = HA.to_query(query, 1)
    counts = eng.hap_allele_counts(cq, cpool)
    assert counts[:, 1:, :2].sum() > 100
    scans = {}
    for channels in (18, 30):
        eng.set_params(channels=channels, min_coverage=2)
        scans[channels] = _scan_bytes(eng, ref)
        assert scans[channels][0] > 20
    # both new calls, on another table and another pool than any that is set
    other = sites[::2]
    q, pool = HA.to_query(other, 2)
    assert np.array_equal(eng.phase_allele_links(q, pool), PI.links(rs, other))
    ps, h1, _ = PI.phase(rs, other)
    assert int(_check_units(eng, rs, other, _split(other, ps), h1, lead=2, load=False).sum()) > 100
    after = eng.haplotags()
    assert after[0].tolist() == tags[0].tolist() and after[1] == tags[1] and eng.read_phase_sets().tolist() == sets
    assert np.array_equal(eng.hap_allele_counts(cq, cpool), counts)           # it still sees its own pool
    for channels in (18, 30):
        eng.set_params(channels=channels, min_coverage=2)
        assert _scan_bytes(eng, ref) == scans[channels]
    if table == "set_phase_alleles":                          # the tags rebuilt from the set table are the same ones: its buffers were not touched
        eng.load_reads(rs)
        assert eng.haplotags()[0].tolist() == tags[0].tolist()
    assert isinstance(eng, capi.Engine)


# ---- 12. unit links
def _long_reads(rng, L, n, sites_alt, ref):
    recs = []
    for k in range(n):
        start, hap = rng.randrange(0, L - 610), k % 2
        seq = [rng.choice("ACGT") if rng.random() < 0.05 else (sites_alt[y] if (y + hap) % 2 and y in sites_alt else ref[y]) for y in range(start, start + 600)]
        recs.append((start, "600M", "".join(seq)))
    recs.sort()
    return recs


def test_a_unit_every_five_sites_under_long_reads(eng):
    rng = random.Random(21)
    L = 900
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    alt = {p: "ACGT"[("ACGT".index(ref[p]) + 1) % 4] for p in range(0, L - 2, 3)}
    sites = [(_row(p + 1, ref[p:p + 2], ref[p]) if p % 4 == 0 else _snv(p + 1, ref[p], alt[p])) for p in sorted(alt)]
    rs = _readset(_long_reads(rng, L, 24, alt, ref))
    ps = [sites[(j // 5) * 5]["pos"] if j % 11 else -1 for j in range(len(sites))]         # a unit every 5 sites; every 11th site a singleton
    h1 = [rng.randint(0, 1) for _ in sites]
    exp = _check_units(eng, rs, sites, ps, h1)
    assert len(exp) >= 55 and int(exp.sum()) > 24 * 30 and int(exp[:, K - 1].sum()) > 0


def test_a_unit_the_read_sees_tied_and_interleaved_units(eng):
    # sites 101 .. 108 (SNVs A>C) and two deletion sites; the read shows A, C by hand
    sites = [_snv(p, "A", "C") for p in range(101, 109)] + [_row(110, "AT", "A"), _row(112, "AT", "A")]
    h1 = [0] * len(sites)
    #        101 102 103 104 105 106 107 108 | 110 (del) 112 (no del)
    rs = _readset([(100, "10M1D4M", "AC" "AA" "CA" "AA" "AA" "AAAA"),
                   (100, "10M1D4M", "AA" "AA" "AA" "AA" "AA" "AAAA")])
    # unit 101: sites 101, 102 — read 0 shows A (hap 1) and C (hap 2): tied, not observed; read 1: haplotype 1
    # unit 103: 103, 104 and 110 — read 0: A, A, deletion (B): 2 against 1: haplotype 1
    # unit 105: 105, 106, 112 — read 0: C, A, no deletion (A): haplotype 1
    ps = [101, 101, 103, 103, 105, 105, 107, 107, 103, 105]
    exp = _check_units(eng, rs, sites, ps, h1)
    assert exp[1, 0].tolist() == [1, 0]                       # read 1 links 103 to 101; read 0 does not (tied)
    assert exp[2, 0].tolist() == [2, 0] and exp[2, 1].tolist() == [1, 0] and exp[3, 2].tolist() == [1, 0]
    # interleaved: the sites of two units alternate
    ps2 = [101, 102, 101, 102, 101, 102, 107, 107, 101, 102]
    h2 = [0, 1, 0, 1, 0, 1, 0, 0, 1, 0]
    exp2 = _check_units(eng, rs, sites, ps2, h2, load=False)
    # unit 101 (101, 103, 105, 110 with B on haplotype 1): both reads haplotype 1; unit 102 (102, 104, 106, 112): read 0 tied 2 : 2, read 1
    # haplotype 2; unit 107: both haplotype 1
    assert len(exp2) == 3 and exp2[1, 0].tolist() == [0, 1] and exp2[2, 0].tolist() == [0, 1] and exp2[2, 1].tolist() == [2, 0]


def test_unit_links_on_the_fragmenting_input_with_indel_sites(eng):
    ref, rs, table, _, _ = PM.gen_fragmented(0)
    sites = HA.snv_sites(table)
    taken = {s["pos"] for s in sites}
    # the reads' own deletions and insertions of one base become sites where no SNV stands: anchors on the base before them
    seen = {}
    for i in range(len(rs)):
        x = int(rs.reads[i]["pos"])
        ops = HA.normalise(HA.read_ops(rs, i))
        for k, (op, n) in enumerate(ops):
            if op == "M" and k + 1 < len(ops) and ops[k + 1][0] == "D" and ops[k + 1][1] <= 2:
                seen.setdefault((x + n, ops[k + 1][1]), 0)
                seen[(x + n, ops[k + 1][1])] += 1
            if op in "MDN":
                x += n
    added = 0
    for (p, n), _ in sorted(seen.items()):
        if p not in taken and p + n < len(ref) and added < 40:
            sites.append(_row(p, ref[p - 1:p + n], ref[p - 1]))
            taken.add(p)
            added += 1
    assert added >= 20
    sites.sort(key=lambda s: s["pos"])
    lk = _check(eng, rs, sites)
    ps, h1, st = PI.resolve(sites, lk)
    assert st["n_blocks"] >= 3
    exp = _check_units(eng, rs, sites, ps, h1, load=False)
    assert int(exp.sum()) > 0
    want = PI.phase(rs, sites, 3)
    q, pool = HA.to_query(sites)
    gps, gh1, gst = eng.phase_allele_sites(q, pool, merge_levels=3)
    assert (gps.tolist(), gh1.tolist(), gst) == want


# ---- 13. drivers
HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """Two contigs of hapalleleref.gen_case's reads (SNVs, indels and 1/2 sites on two haplotypes) in an untagged BAM, the unphased pass on
    it, and `with`: a VCF that holds an unphased PASS row for every SNV and every planted site."""
    from clair3_rna_amd import bam, bamio, io, synth
    tmp = str(tmp_path_factory.mktemp("phase_indel_drivers"))
    contigs, reads, rows = [], {}, []
    for name, seed in (("chr1", 11), ("chr2", 12)):
        ref, rs, snvs, _, planted, _ = HA.gen_case(seed, errors=True)
        contigs.append((name, ref))
        reads[name] = rs
        both = [(p, r, a, "0/1") for p, r, a in snvs] + [(s["pos"], s["ref"], s["alt"], s["gt"]) for s in planted]
        rows += ["%s\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:GQ\t%s:30\n" % ((name,) + r) for r in sorted(both)]
    fa, w18, w30 = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model18"), os.path.join(tmp, "model30")
    io.write_fasta(fa, contigs)
    np.save(w18 + ".c3rw.npy", synth.random_weights(18, seed=5))
    np.save(w30 + ".c3rw.npy", synth.random_weights(30, seed=5))
    bam_fn = os.path.join(tmp, "plain.bam")
    bam.write_bam(bam_fn, [(n, len(r)) for n, r in contigs], reads)
    bamio.index_build(bam_fn)
    s = dict(tmp=tmp, fa=fa, w18=w18, w30=w30, bam=bam_fn, reads=reads, rows=rows)
    s["with"] = os.path.join(tmp, "with_indels.vcf")
    with open(s["with"], "w") as f:
        f.write(HEAD + "".join(rows))
    _call_sample(s, "hand", [])
    s["pass1"] = os.path.join(tmp, "hand", "output.vcf.gz")
    assert os.path.isfile(s["pass1"])
    return s


def _call_sample(s, out, extra, log=None):
    from clair3_rna_amd import call_sample
    argv = ["--bam_fn", s["bam"], "--ref_fn", s["fa"], "--output_dir", os.path.join(s["tmp"], out), "--pileup_model_path", s["w18"],
            "--phased_pileup_model_path", s["w30"], "--chunk_num", "3", "--min_coverage", "2"] + list(extra)
    assert call_sample.Run(call_sample.build_parser().parse_args(argv), log=log or (lambda m: None)) == 0


def _gz(fn):
    with gzip.open(fn, "rt") as f:
        return f.read()


@pytest.mark.parametrize("levels", [0, 2])
def test_phase_vcf_indels_writes_the_files_the_restatement_predicts(sample, tmp_path, levels):
    from clair3_rna_amd import phase_vcf
    out_dir, msgs = str(tmp_path / "phased_vcf"), []
    written = phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", sample["with"], "--output_dir", out_dir, "--indels",
                                                                 "--merge_levels", str(levels)]), log=msgs.append)
    assert len(written) == 2 and len(msgs) == 2 and all(m.startswith("[INFO] chr") and "with indels and two-ALT rows" in m for m in msgs)
    n_event = 0
    for ctg in ("chr1", "chr2"):
        lines = [ln for ln in sample["rows"] if ln.startswith(ctg + "\t")]
        cands, skipped = HA.candidates(lines, ctg)
        assert len(cands) == len(lines) and not any(skipped.values())
        ps, h1, _ = PI.phase(sample["reads"][ctg], cands, levels)
        exp = HEAD.replace("#CHROM", '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set identifier">\n#CHROM')
        exp += "".join(HA.rewritten(ln, s, (p, h)) if p >= 0 else ln for ln, s, p, h in zip(lines, cands, ps, h1))
        assert _gz(os.path.join(out_dir, "phased_%s.vcf.gz" % ctg)) == exp
        n_event += sum(1 for s, p in zip(cands, ps) if p >= 0 and HA.flags(s)[1])
    assert n_event >= 40                                      # the comparison is about indel and two-ALT rows


FLOWS = [("plain", []), ("merge", ["--phase_merge_levels", "2"]), ("outputs", ["--phase_output", "--phase_indels", "--haplotagged_bam"])]


@pytest.mark.parametrize("name, extra", FLOWS, ids=[f[0] for f in FLOWS])
def test_call_sample_with_phasing_indels_equals_the_three_steps_by_hand(sample, name, extra):
    from clair3_rna_amd import phase_vcf
    levels = "2" if name == "merge" else "0"
    # by hand: pass 1 is the fixture's; phase_vcf --indels on its VCF; pass 2 with --phased_vcf_fn DIR --haplotag_indels
    hand = "hand_" + name
    hand_dir = os.path.join(sample["tmp"], hand, "phased_vcf")
    phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", sample["pass1"], "--output_dir", hand_dir, "--indels", "--merge_levels", levels]),
                  log=lambda m: None)
    behind = [e for e in extra if not e.startswith("--phase_merge") and e != "2"]
    _call_sample(sample, hand, ["--enable_phasing_model", "--phased_vcf_fn", hand_dir, "--haplotag_indels"] + behind)
    one = "one_" + name
    msgs = []
    _call_sample(sample, one, ["--enable_phasing_model", "--phasing", "builtin", "--phasing_indels"] + extra, msgs.append)
    a, b = os.path.join(sample["tmp"], hand), os.path.join(sample["tmp"], one)
    assert _gz(os.path.join(b, "output.vcf.gz")) == _gz(sample["pass1"])
    one_dir = os.path.join(b, "tmp", "phased_output", "phased_vcf")
    for ctg in ("chr1", "chr2"):
        fa_, fb_ = os.path.join(hand_dir, "phased_%s.vcf.gz" % ctg), os.path.join(one_dir, "phased_%s.vcf.gz" % ctg)
        assert os.path.exists(fa_) == os.path.exists(fb_) and (not os.path.exists(fa_) or _gz(fa_) == _gz(fb_))
    names = ["output_enable_phasing.vcf.gz"]
    if name == "outputs":
        names += ["output_enable_phasing_phased.vcf.gz", "output_enable_phasing_hap_counts.tsv"] + [os.path.join("tmp", "phased_output", "phased_bam", c + e) for c in ("chr1", "chr2") for e in (".bam", ".bam.bai")]
    for fn in names:
        with open(os.path.join(a, fn), "rb") as f, open(os.path.join(b, fn), "rb") as g:
            assert f.read() == g.read(), fn
    assert any("--haplotag_indels" in m and "phased sites in the table" in m for m in msgs)          # pass 2 read the allele table
    if name == "plain":                                       # the phasing shows in the records: the comparison above can fail
        _call_sample(sample, "untagged", ["--enable_phasing_model"])
        assert _gz(os.path.join(sample["tmp"], "untagged", "output_enable_phasing.vcf.gz")) != _gz(os.path.join(b, "output_enable_phasing.vcf.gz"))


def test_the_bridge_through_the_device(eng, tmp_path):
    """SNV, deletion, SNV with no read over both SNVs: the SNV-only chain phases nothing, so no read is tagged; with the deletion in the
    table all three share a block and the reads that cover only the deletion are tagged, by the haplotype they were drawn from."""
    from clair3_rna_amd import bam, bamio, phase_vcf, phasedvcf
    rs, hap = PI.bridge_reads()
    bam_fn = str(tmp_path / "bridge.bam")
    bam.write_bam(bam_fn, [("chrB", len(PI.BRIDGE_REF))], {"chrB": rs})
    bamio.index_build(bam_fn)
    vcf = str(tmp_path / "bridge.vcf")
    with open(vcf, "w") as f:
        f.write(HEAD + "".join("chrB\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT\t0/1\n" % (s["pos"], s["ref"], s["alt"]) for s in PI.BRIDGE_SITES))
    # plain: the SNV chain leaves both SNVs unphased, nothing is written, nothing can tag a read
    plain = phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", bam_fn, "--vcf_fn", vcf, "--output_dir", str(tmp_path / "plain")]), log=lambda m: None)
    assert len(plain) == 1 and len(phasedvcf.contig_alleles(str(tmp_path / "plain"), "chrB")[0]) == 0 and "|" not in _gz(plain[0]).split("#CHROM")[1]
    # --indels: one block
    phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", bam_fn, "--vcf_fn", vcf, "--output_dir", str(tmp_path / "indels"), "--indels"]), log=lambda m: None)
    sites, h1, pool, pool_bases, _ = phasedvcf.contig_alleles(str(tmp_path / "indels"), "chrB")
    assert sites["pos"].tolist() == [21, 61, 101] and sites["ps"].tolist() == [21, 21, 21]
    assert [int(a) ^ b for a, b in zip(h1, PI.BRIDGE_TRUTH)] in ([0, 0, 0], [1, 1, 1])
    eng.set_phase_alleles(sites, h1, pool, pool_bases)
    eng.load_reads(rs)
    tags = eng.haplotags()[0].tolist()
    only_d = [i for i in range(len(rs)) if int(rs.reads[i]["pos"]) == 50 and H.cigar_ref_len("".join("%d%s" % (n, o) for o, n in HA.read_ops(rs, i))) == 30]
    assert len(only_d) == 4 and all(tags[i] in (1, 2) for i in only_d)
    flip = int(h1[0]) ^ PI.BRIDGE_TRUTH[0]
    assert all(tags[i] == (hap[i] if not flip else 3 - hap[i]) for i in range(len(rs)))
    want = HI.haplotag(rs, [dict(s, ps=21, h1=int(h)) for s, h in zip(PI.BRIDGE_SITES, h1)])[0]
    assert tags == want.tolist()
