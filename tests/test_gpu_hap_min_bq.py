"""The base-quality threshold on the device (c3r_load_reads_q, c3r_set_hap_min_bq, k_mask_low_bq): the kernel alone against
tests/qualref.py byte for byte; the invariance the feature stands for — every call that holds the reads against a site table gives with
(qualities, Q) what it gives with Q = 0 on reads whose masked bases are N — on hand-made reads, each of whose cases is shown to matter;
what must not move (the tensor build); the life cycle; and the drivers on one small BAM with qualities."""
import gzip
import os

import numpy as np
import pytest

from tests import hapalleleref as HA
from tests import hapref
from tests import qualref as QR

pytestmark = pytest.mark.gpu

Q10 = 10
_state = {}


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clean(request):
    """Every test of this module starts and leaves its engine without reads, with the threshold and the left-alignment off, without a phase
    table and with default parameters."""
    yield
    if "eng" in request.fixturenames:
        from clair3_rna_amd import capi
        from clair3_rna_amd.reads import ReadSet
        e = request.getfixturevalue("eng")
        e.load_reads(ReadSet.from_records([]))
        e.set_hap_min_bq(0)
        e.set_phase_sites(None)
        e.set_hap_left_align(False)
        e.params = capi.default_params()
        e.set_params()


# ---- 1. the kernel alone
def _flat_case(n, read_len, Q):
    """n packed bytes under reads of read_len bases; the qualities go round Q - 1, Q, 0, 93, 0xff (a period of five: each value meets both
    nibbles of a byte); the byte behind a read of odd length is 0xff."""
    seq = np.array([(37 * t + 11) & 0xff for t in range(n)], np.uint8)
    vals = [Q - 1, Q, 0, 93, 0xff]
    qual = np.array([vals[t % 5] for t in range(2 * n)], np.uint8)
    rs = QR.flat_readset(seq, qual, read_len)
    for r in rs.reads:
        if int(r["l_seq"]) & 1:
            rs.qual[2 * int(r["seq_off"]) + int(r["l_seq"])] = 0xff
    assert QR.layout_ok(rs)
    return rs


@pytest.mark.parametrize("Q", [1, 10, 93])
@pytest.mark.parametrize("read_len", [33, 32])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 8 * 255 + 3, 8 * 700 + 5])
def test_the_kernel_alone(eng, n, read_len, Q):
    rs = _flat_case(n, read_len, Q)
    want, n_masked = QR.mask(rs, Q)
    if n >= 7:
        assert 0 < n_masked < 2 * n and not np.array_equal(want, rs.seq)
    eng.set_hap_min_bq(Q)
    eng.load_reads(rs)
    got = eng.hap_seq()
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert eng.hap_min_bq() == (Q, n_masked)
    eng.set_hap_min_bq(0)                                    # off: the sequence itself
    assert np.array_equal(eng.hap_seq(), rs.seq) and eng.hap_min_bq() == (0, 0)
    eng.set_hap_min_bq(Q)                                    # and set after the load: the same copy
    assert np.array_equal(eng.hap_seq(), want) and eng.hap_min_bq() == (Q, n_masked)


def test_the_kernel_by_name(eng):
    rs = _flat_case(100, 33, Q10)
    eng.set_profiling(True)
    try:
        eng.reset_kernel_stats()
        eng.load_reads(rs)                                   # off: not launched, although the qualities are there
        assert "k_mask_low_bq" not in eng.kernel_stats()
        eng.set_hap_min_bq(Q10)
        eng.load_reads(rs)
        assert eng.kernel_stats()["k_mask_low_bq"]["launches"] == 2       # once by the setter, once inside the load
    finally:
        eng.set_profiling(False)


# ---- 2. hand-made reads: two haplotypes over a dozen sites in two phase sets
REF_LEFT = "GATCCGTACGTTAGCCATGCATTGCAGTCCGATGCTAGCTTGACCGTAGCATGCCT"
REF = ("TGCA" * 25 + REF_LEFT + "CAAAAAG" + "TCGATCGGCTTACGGATCCATGCAAGTCTGACGTCAGTACGATCGTTAGCAGCTAGGCTAACGGTACCTGATTCGA" + "ACTG" * 40)
OFF = 100                                                    # 0-based index of REF_LEFT[0]
HOMO = OFF + len(REF_LEFT)                                   # 0-based index of the C before AAAAA


def _other(b):
    return "ACGT"[("ACGT".index(b) + 1) % 4]


def _rows():
    """[(pos, REF, ALT, GT, ps)] of the allele table, sorted: SNVs, a pure deletion, an insertion, an insertion in the homopolymer (at its
    left-most place), a 1/2 row of an SNV and a deletion."""
    at = lambda p: REF[p - 1]
    rows = [(p, at(p), _other(at(p)), "0/1", 11) for p in (OFF + 5, OFF + 12, OFF + 20)]
    rows.append((OFF + 30, REF[OFF + 29:OFF + 32], at(OFF + 30), "0/1", 11))                       # DEL 2, pure
    rows.append((OFF + 40, at(OFF + 40), at(OFF + 40) + "GC", "0/1", 11))                          # INS GC
    rows.append((HOMO + 1, "C", "CA", "0/1", 11))                                                   # INS A before AAAAA
    rows += [(p, at(p), _other(at(p)), "0/1", 77) for p in (HOMO + 20, HOMO + 30, HOMO + 40)]
    p = HOMO + 50
    rows.append((p, REF[p - 1:p + 1], _other(at(p)) + at(p + 1) + "," + at(p), "1/2", 77))          # SNV | DEL 1
    rows += [(q, at(q), _other(at(q)), "0/1", 77) for q in (HOMO + 60, HOMO + 70)]
    return sorted(rows)


def _table():
    table = []
    for j, row in enumerate(_rows()):
        s = HA.site_of_row(*row)
        assert isinstance(s, dict), (row, s)
        table.append(dict(s, h1=j % 2))
    return table


def _read(hap, start, end, spelling, table):
    """(pos, CIGAR, SEQ) of a read of haplotype `hap` (1, 2) over the 0-based [start, end): at every site the allele of that haplotype —
    the homopolymer insertion placed at the RIGHT end of the tract.  spelling 0: plain; 1: the first M run as `3M2=...`; 2: a pad in the
    first M run (the serial walk)."""
    ops, seq, x = [], [], start
    def m(n):
        if n:
            ops.append([n, "M"])
    for s in table:
        p0 = s["pos"] - 1
        if p0 < start or p0 + 3 >= end:
            continue
        base, ev = s["B"] if (hap == 1) == (s["h1"] == 1) else s["A"]
        if s["pos"] == HOMO + 1 and ev != HA.NONE:                                  # C AAAAA then the inserted A
            seq += list(REF[x:p0 + 6]); m(p0 + 6 - x); x = p0 + 6
            seq += list(ev[1]); ops.append([len(ev[1]), "I"])
            continue
        seq += list(REF[x:p0]) + [base]; m(p0 + 1 - x); x = p0 + 1
        if ev[0] == "ins":
            seq += list(ev[1]); ops.append([len(ev[1]), "I"])
        elif ev[0] == "del":
            ops.append([ev[1], "D"]); x += ev[1]
    seq += list(REF[x:end]); m(end - x)
    merged = []
    for n, o in ops:
        if merged and merged[-1][1] == o:
            merged[-1][0] += n
        else:
            merged.append([n, o])
    assert merged[0][1] == "M" and merged[0][0] > 8
    first = merged[0][0]
    head = {0: "%dM" % first, 1: "3M2=%dM" % (first - 5), 2: "4M1P%dM" % (first - 4)}[spelling]
    return start, head + "".join("%d%s" % (n, o) for n, o in merged[1:]), "".join(seq)


def _query_offset(cigar, pos0, target0):
    """The query offset of the base a read shows on the 0-based reference position target0 (under an M-like op)."""
    import re
    x, y = pos0, 0
    for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar):
        n = int(n)
        if o in "M=X":
            if x <= target0 < x + n:
                return y + target0 - x
            x += n; y += n
        elif o in "DN":
            x += n
        elif o in "IS":
            y += n
    raise AssertionError("position not under an M op")


def _scenario():
    """The reads with their qualities, the tables, and the three directed reads: (a) a low-quality anchor on the pure deletion, (b) a
    low-quality base inside the matching insertion, (c) a low-quality inserted base that stops the left shift in the homopolymer."""
    if "sc" in _state:
        return _state["sc"]
    from clair3_rna_amd.reads import ReadSet
    table = _table()
    by_pos = {s["pos"]: j for j, s in enumerate(table)}
    j_del, j_ins, j_homo = by_pos[OFF + 30], by_pos[OFF + 40], by_pos[HOMO + 1]
    hap_of = lambda j, allele: 1 if (table[j]["h1"] == 1) == (allele == "B") else 2      # the haplotype that shows that allele at site j
    spans = [(OFF - 40, HOMO + 120), (OFF - 40, HOMO + 15), (OFF + 15, HOMO + 120), (OFF - 13, HOMO + 85), (HOMO + 9, HOMO + 121), (OFF - 7, HOMO + 58)]
    recs = []
    for i in range(30):
        start, end = spans[i % len(spans)]
        pos, cigar, seq = _read(1 + i % 2, start, end, (i // 2) % 3, table)
        qual = [40] * len(seq)
        snv = [s for s in table if HA.flags(s) == (True, False) and start <= s["pos"] - 1 < end - 3]
        if snv:                                              # one site below Q = 10 on every read, one at 0 on every third
            qual[_query_offset(cigar, pos, snv[i % len(snv)]["pos"] - 1)] = 5
            if i % 3 == 0:
                qual[_query_offset(cigar, pos, snv[(i + 3) % len(snv)]["pos"] - 1)] = 0
        if i % 5 == 0:                                       # the last unit of the unit links is not seen at all: its four sites at 0
            for s in table[8:]:
                if start <= s["pos"] - 1 < end - 3:
                    qual[_query_offset(cigar, pos, s["pos"] - 1)] = 0
        if i in (1, 13, 19):                                 # two wrong bases of low quality on three sites: they turn the tag unless they are masked
            seq = list(seq)
            for s in table[:2]:
                y = _query_offset(cigar, pos, s["pos"] - 1)
                seq[y], qual[y] = (s["alt"] if seq[y] == s["ref"] else s["ref"]), 5
            seq = "".join(seq)
        recs.append(dict(pos=pos, cigar=cigar, seq=seq, qual=qual, flag=16 * (i % 2), mapq=60, hp=0))
    recs[7]["qual"] = None                                   # a read without qualities: never masked
    directed = {}
    whole = (OFF - 40, HOMO + 120)
    for name, j, target in (("anchor", j_del, OFF + 29), ("in_ins", j_ins, None), ("shift", j_homo, None)):
        pos, cigar, seq = _read(hap_of(j, "B"), whole[0], whole[1] - len(directed), 0, table)
        qual = [40] * len(seq)
        if name == "anchor":
            qual[_query_offset(cigar, pos, target)] = 2
        elif name == "in_ins":
            qual[_query_offset(cigar, pos, OFF + 39) + 2] = 2                          # the second inserted base
        else:
            qual[_query_offset(cigar, pos, HOMO + 5) + 1] = 2                          # the A inserted behind the tract
        directed[name] = len(recs)
        recs.append(dict(pos=pos, cigar=cigar, seq=seq, qual=qual, flag=0, mapq=60, hp=0))
    order = sorted(range(len(recs)), key=lambda k: recs[k]["pos"])                     # from_records sorts (stable): where the directed reads land
    rs = ReadSet.from_records(recs)
    directed = {k: order.index(v) for k, v in directed.items()}
    assert QR.layout_ok(rs) and any(int(r["l_seq"]) & 1 for r in rs.reads) and any(not int(r["l_seq"]) & 1 for r in rs.reads)
    snv_rows = [(s["pos"], s["ref"], s["alt"], s["h1"], s["ps"]) for s in table if HA.flags(s) == (True, False)]
    sc = dict(rs=rs, table=table, snv=hapref.make_sites(snv_rows), directed=directed, j=dict(anchor=j_del, in_ins=j_ins, shift=j_homo))
    _state["sc"] = sc
    return sc


def _snv_results(eng, rs, sites):
    eng.load_reads(rs)
    eng.set_phase_sites(sites)
    hp, st = eng.haplotags()
    chain = sites.copy()
    chain["ps"] = [11 if k < 3 else 77 if k < 6 else 115 for k in range(len(sites))]
    return dict(hp=hp, st=st, ps=eng.read_phase_sets(), counts=eng.hap_counts(sites), links=eng.phase_links(sites), ulinks=eng.phase_unit_links(chain))


def _allele_results(eng, rs, table, la):
    from clair3_rna_amd import capi
    q, pool = HA.to_query(table)
    h1 = np.array([s["h1"] for s in table], np.uint8)
    if la:
        eng.set_reference(1, REF)
        q, pool, _, src, st = capi.hap_left_align_sites(q, pool, 1, REF)
        assert list(src) == list(range(len(table))) and st["n_moved"] == 0               # (the rows are written at their left-most places)
    eng.set_hap_left_align(la)
    eng.load_reads(rs)
    eng.set_phase_alleles(q, h1, pool)
    hp, st = eng.haplotags()
    chain = q.copy()
    chain["ps"] = [11 if k < 4 else 77 if k < 8 else 115 for k in range(len(q))]
    return dict(hp=hp, st=st, ps=eng.read_phase_sets(), counts=eng.hap_allele_counts(q, pool), links=eng.phase_allele_links(q, pool),
                ulinks=eng.phase_allele_unit_links(chain, h1, pool))


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("hp", "ps", "counts", "links", "ulinks")) and a["st"] == b["st"]


def _assert_same(got, exp):
    assert np.array_equal(got["hp"], exp["hp"]), np.nonzero(got["hp"] != exp["hp"])[0][:10]
    assert np.array_equal(got["ps"], exp["ps"]) and got["st"] == exp["st"]
    for key in ("counts", "links", "ulinks"):
        assert got[key].shape == exp[key].shape and np.array_equal(got[key], exp[key]), (key, np.argwhere(got[key] != exp[key])[:10])


def _no_quals(rs):
    from clair3_rna_amd.reads import ReadSet
    return ReadSet(rs.reads, rs.cigar, rs.seq)


@pytest.mark.parametrize("Q", [1, Q10, 93])
def test_invariance_snv_entry_points(eng, Q):
    """Tags and read phase sets of set_phase_sites, hap_counts, phase_links, phase_unit_links."""
    sc = _scenario()
    eng.set_hap_min_bq(Q)
    got = _snv_results(eng, sc["rs"], sc["snv"])
    assert eng.hap_min_bq() == (Q, QR.mask(sc["rs"], Q)[1])
    eng.set_hap_min_bq(0)
    exp = _snv_results(eng, QR.with_n(sc["rs"], Q), sc["snv"])
    _assert_same(got, exp)
    ignoring = _snv_results(eng, _no_quals(sc["rs"]), sc["snv"])
    for key in ("counts", "links", "ulinks"):                # it matters: a no-op implementation gives `ignoring`
        assert not np.array_equal(got[key], ignoring[key]), key
    assert got["st"]["n_votes"] < ignoring["st"]["n_votes"]
    if Q == 93:                                              # every base with a quality is masked: only the read without them votes
        assert got["st"]["n_no_vote"] == len(sc["rs"]) - 1
    # and the restatement of the tag rule on the reads with N
    hp, st, _ = hapref.haplotag(QR.with_n(sc["rs"], Q), sc["snv"])
    assert np.array_equal(got["hp"], hp) and got["st"] == st


@pytest.mark.parametrize("la", [False, True], ids=["plain", "left_aligned"])
@pytest.mark.parametrize("Q", [1, Q10, 93])
def test_invariance_allele_entry_points(eng, Q, la):
    """Tags and read phase sets of set_phase_alleles, hap_allele_counts, phase_allele_links, phase_allele_unit_links; and again under
    set_hap_left_align(1)."""
    sc = _scenario()
    eng.set_hap_min_bq(Q)
    got = _allele_results(eng, sc["rs"], sc["table"], la)
    eng.set_hap_min_bq(0)
    exp = _allele_results(eng, QR.with_n(sc["rs"], Q), sc["table"], la)
    _assert_same(got, exp)
    ignoring = _allele_results(eng, _no_quals(sc["rs"]), sc["table"], la)
    for key in ("counts", "links", "ulinks"):
        assert not np.array_equal(got[key], ignoring[key]), key
    if Q != Q10:
        return
    # the directed reads, in the count table (all rows of a site summed: whatever the read's tag): [A, B, another allele]
    col = lambda res, j: res["counts"][j].sum(axis=0).astype(int)
    j = sc["j"]
    # (a) a low-quality anchor on the pure deletion is still observed by its event: the site's columns do not move at all
    assert np.array_equal(col(got, j["anchor"]), col(ignoring, j["anchor"])) and col(got, j["anchor"])[1] >= 1
    # (b) a low-quality base inside the matching insertion: the read leaves column B for column 2
    assert np.array_equal(col(got, j["in_ins"]) - col(ignoring, j["in_ins"]), [0, -1, 1])
    # (c) the homopolymer: without left-alignment nobody shows the insertion on the row's place; with it every read of that haplotype
    # does — but for the one whose inserted A is below the threshold: its shift stops at once and it shows the reference there
    if la:
        assert np.array_equal(col(got, j["shift"]) - col(ignoring, j["shift"]), [1, -1, 0]) and col(ignoring, j["shift"])[1] >= 5
    else:
        assert col(got, j["shift"])[1] == 0 and col(ignoring, j["shift"])[1] == 0
    # the three reads' own tags are decided by many sites: they stay; the masked SNVs move other reads' votes
    assert got["st"]["n_votes"] < ignoring["st"]["n_votes"]


def test_both_walks_are_on_the_reads(eng):
    sc = _scenario()
    cig = lambda r: [int(c) & 15 for c in sc["rs"].cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]]
    assert any(cig(r)[:2] == [0, 7] for r in sc["rs"].reads) and any(6 in cig(r) for r in sc["rs"].reads)       # `3M2=` and a pad
    assert 30 <= len(sc["rs"]) <= 40 and len(sc["table"]) == 12 and sorted(set(s["ps"] for s in sc["table"])) == [11, 77]


# ---- 3. what must not move
def test_the_tensor_build_never_sees_the_threshold(eng):
    from clair3_rna_amd import synth
    sc = _scenario()
    rs = sc["rs"]
    w = synth.random_weights(18, seed=5)

    def scan18():
        eng.set_params(channels=18, min_coverage=2)
        eng.load_reads(rs)
        eng.set_reference(1, REF)
        n = eng.scan(1, len(REF))
        build = (n, eng.sites().tobytes(), eng.tokens().tobytes(), eng.tensors(rescaled=False).tobytes())
        eng.load_weights(w, 18)
        eng.infer(fetch=False)
        rows, _ = eng.call_rows_text("chr1", qual=0, show_ref=True)
        return build + (bytes(rows),)
    eng.set_phase_sites(sc["snv"])
    off = scan18()
    eng.set_hap_min_bq(Q10)
    on = scan18()
    assert off[0] >= 8 and on == off and len(off[4]) > 100
    # 30 channels: the scan under (table, Q) is the scan without a table of the same reads carrying the Q run's tags
    eng.set_params(channels=30, min_coverage=2)
    eng.load_reads(rs)
    tags = eng.haplotags()[0].copy()
    assert eng.hap_min_bq()[1] > 0 and set(tags.tolist()) >= {1, 2}
    eng.set_reference(1, REF)
    n = eng.scan(1, len(REF))
    with_table = (n, eng.sites().tobytes(), eng.tokens().tobytes(), eng.tensors(rescaled=False).tobytes())
    eng.set_hap_min_bq(0)
    untagged_differs = not np.array_equal(eng.haplotags()[0], tags)
    eng.set_phase_sites(None)
    eng.load_reads(hapref.with_hp(_no_quals(rs), tags))
    n2 = eng.scan(1, len(REF))
    assert (n2, eng.sites().tobytes(), eng.tokens().tobytes(), eng.tensors(rescaled=False).tobytes()) == with_table
    assert untagged_differs                                  # (the tags of the Q run are not the tags without the threshold)


# ---- 4. life cycle
def test_life_cycle():
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    sc = _scenario()
    rs, sites = sc["rs"], sc["snv"]
    want10, _, _ = hapref.haplotag(QR.with_n(rs, Q10), sites)
    want93, _, _ = hapref.haplotag(QR.with_n(rs, 93), sites)
    want0, _, _ = hapref.haplotag(rs, sites)
    assert not np.array_equal(want10, want0) and not np.array_equal(want93, want10)
    e = capi.Engine(0)
    try:
        assert e.hap_min_bq() == (0, 0)
        for bad in (94, -1):
            with pytest.raises(capi.C3RError) as err:
                e.set_hap_min_bq(bad)
            assert err.value.code == -1 and "c3r_set_hap_min_bq" in str(err.value) and e.hap_min_bq() == (0, 0)
        # before the load
        e.set_phase_sites(sites)
        e.set_hap_min_bq(Q10)
        e.load_reads(rs)
        assert np.array_equal(e.haplotags()[0], want10)
        # changed: tagged again; back to 0: the tags without it
        e.set_hap_min_bq(93)
        assert np.array_equal(e.haplotags()[0], want93)
        e.set_hap_min_bq(0)
        assert np.array_equal(e.haplotags()[0], want0) and np.array_equal(e.hap_seq(), rs.seq)
        # after the load: the same tags as before it
        e.set_hap_min_bq(Q10)
        assert np.array_equal(e.haplotags()[0], want10) and e.hap_min_bq() == (Q10, QR.mask(rs, Q10)[1])
        # new filters do not touch the copy
        e.set_params(min_mq=61)
        assert np.array_equal(e.hap_seq(), QR.mask(rs, Q10)[0]) and np.array_equal(e.haplotags()[0], want10)
        e.set_params(min_mq=5)
        # a second load of another size
        small = ReadSet.from_records([dict(pos=OFF, cigar="30M", seq=REF[OFF:OFF + 30], qual=[3] * 15 + [50] * 15)])
        e.load_reads(small)
        assert e.hap_min_bq() == (Q10, 15) and np.array_equal(e.hap_seq(), QR.mask(small, Q10)[0]) and len(e.haplotags()[0]) == 1
        e.load_reads(rs)
        assert np.array_equal(e.haplotags()[0], want10)
        # a load without qualities under Q > 0 is refused before anything is given up
        with pytest.raises(capi.C3RError) as err:
            e.load_reads(_no_quals(rs))
        assert err.value.code == -1 and "c3r_load_reads" in str(err.value) and "c3r_set_hap_min_bq" in str(err.value)
        assert np.array_equal(e.haplotags()[0], want10) and np.array_equal(e.hap_seq(), QR.mask(rs, Q10)[0])
        # n_reads = 0 is allowed, with and without an array
        e.load_reads(ReadSet.from_records([]))
        assert e.hap_min_bq() == (Q10, 0) and len(e.hap_seq()) == 0
        e.load_reads(ReadSet(rs.reads[:0], rs.cigar[:0], rs.seq[:0], rs.qual[:0]))
        assert e.hap_min_bq() == (Q10, 0)
        # Q > 0 set on reads that came without qualities is refused, and the context works on
        e.set_hap_min_bq(0)
        e.load_reads(_no_quals(rs))
        with pytest.raises(capi.C3RError) as err:
            e.set_hap_min_bq(Q10)
        assert err.value.code == -1 and "c3r_set_hap_min_bq" in str(err.value) and "without qualities" in str(err.value)
        assert e.hap_min_bq() == (0, 0) and np.array_equal(e.haplotags()[0], want0)
        # a wrong number of quality bytes
        L = capi.load_library()
        bad = np.zeros(2 * len(rs.seq) + 1, np.uint8)
        rc = L.c3r_load_reads_q(e.h, rs.reads.ctypes.data, len(rs.reads), rs.cigar.ctypes.data, len(rs.cigar), rs.seq.ctypes.data, len(rs.seq), bad.ctypes.data, len(bad))
        assert rc == -1 and np.array_equal(e.haplotags()[0], want0)
        # a buffer too small for the sequence
        out = np.zeros(4, np.uint8)
        assert L.c3r_get_hap_seq(e.h, out.ctypes.data, 4) == -6
    finally:
        e.close()


# ---- 5. the drivers on one small BAM with qualities
HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    from clair3_rna_amd import bam, bamio, io, synth
    tmp = str(tmp_path_factory.mktemp("hap_min_bq_drivers"))
    sc = _scenario()
    fa, w18, w30 = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model18"), os.path.join(tmp, "model30")
    io.write_fasta(fa, [("chr1", REF)])
    np.save(w18 + ".c3rw.npy", synth.random_weights(18, seed=5))
    np.save(w30 + ".c3rw.npy", synth.random_weights(30, seed=5))
    bam_fn = os.path.join(tmp, "quals.bam")
    bam.write_bam(bam_fn, [("chr1", len(REF))], {"chr1": sc["rs"]})
    bamio.index_build(bam_fn)
    phased = os.path.join(tmp, "phased.vcf")
    letter = {1: "A", 2: "C", 4: "G", 8: "T"}
    with open(phased, "w") as f:
        f.write(HEAD + "".join("chr1\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s:%d\n" % (int(s["pos"]), letter[int(s["ref"])], letter[int(s["alt"])], "1|0" if int(s["h1"]) else "0|1",
                                                                                   int(s["ps"])) for s in sc["snv"]))
    return dict(tmp=tmp, fa=fa, w18=w18, w30=w30, bam=bam_fn, phased=phased, sc=sc)


def test_haplotag_bam_writes_the_tags_of_the_reads_with_n(sample, tmp_path):
    from clair3_rna_amd import haplotag_bam
    from tests import bamref
    sc = sample["sc"]
    out = {}
    for q in (0, Q10):
        out_dir, msgs = str(tmp_path / ("q%d" % q)), []
        haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", sample["bam"], "--phased_vcf_fn", sample["phased"], "--output_dir", out_dir]
                                                                + (["--hap_min_bq", str(q)] if q else [])), log=msgs.append)
        recs = bamref.Bam(os.path.join(out_dir, "chr1.bam")).records
        out[q] = [((recs[i].tag("HP") or (None, 0))[1], (recs[i].tag("PS") or (None, -1))[1]) for i in range(len(recs))]
        info = [m for m in msgs if "--hap_min_bq" in m and m.startswith("[INFO]")]
        warn = [m for m in msgs if m.startswith("[WARNING]")]
        if q:
            total = int(sc["rs"].reads["l_seq"].sum())
            assert info == ["[INFO] chr1: --hap_min_bq %d: %d of %d bases masked for haplotagging, counts and phasing votes" % (q, QR.mask(sc["rs"], q)[1], total)]
            assert warn == ["[WARNING] chr1: 1 of %d reads carry no base qualities: --hap_min_bq masks none of their bases" % len(sc["rs"])]
        else:
            assert not info and not warn
    for q in (0, Q10):
        rs = QR.with_n(sc["rs"], q)
        by_pos = {int(s["pos"]): s for s in sc["snv"]}
        want = []
        for i in range(len(rs)):
            hp, _, _, tally = hapref.tag_read(rs, i, by_pos)
            ps = max(tally.items(), key=lambda kv: (kv[1][0] + kv[1][1], -kv[1][2]))[0] if hp else -1
            want.append((hp, ps))
        assert out[q] == want, q
    assert out[0] != out[Q10]


def test_call_sample_builtin_under_the_flag_reaches_the_end(sample):
    from clair3_rna_amd import call_sample

    def run(out, extra, log):
        argv = ["--bam_fn", sample["bam"], "--ref_fn", sample["fa"], "--output_dir", os.path.join(sample["tmp"], out), "--pileup_model_path", sample["w18"],
                "--phased_pileup_model_path", sample["w30"], "--chunk_num", "1", "--min_coverage", "2"] + extra
        assert call_sample.Run(call_sample.build_parser().parse_args(argv), log=log) == 0
    # The first pass of the flagged run is the unphased 18-channel pass, so the run without the flag is that pass alone.  The `##` lines of a
    # VCF name the command line and the output directory, which differ between the two runs by construction: every other line — #CHROM and
    # all records — must be the same bytes.
    msgs = []
    run("plain", [], lambda m: None)
    run("flag", ["--enable_phasing_model", "--phasing", "builtin", "--hap_min_bq", str(Q10), "--haplotagged_bam"], msgs.append)
    gz = lambda fn: gzip.open(fn, "rt").read()
    data = lambda text: [l for l in text.splitlines() if not l.startswith("##")]
    first = gz(os.path.join(sample["tmp"], "flag", "output.vcf.gz"))
    assert data(first) == data(gz(os.path.join(sample["tmp"], "plain", "output.vcf.gz"))) and len(data(first)) >= 1
    assert os.path.isfile(os.path.join(sample["tmp"], "flag", "output_enable_phasing.vcf.gz"))
    # every step behind the first pass that loaded reads said what the threshold masked.  How many steps load reads depends on what the
    # random weights call: phase_vcf and haplotag_bam load a contig only when it has candidates / phased sites; the 30-channel pass always does.
    said = [m for m in msgs if m.startswith("[INFO] chr1: --hap_min_bq %d: " % Q10)]
    assert len(said) >= 1 and all(" of %d bases masked" % int(sample["sc"]["rs"].reads["l_seq"].sum()) in m for m in said)
