"""Per-haplotype counts of SNV, insertion, deletion and two-ALT alleles on the device (c3r_hap_allele_counts / k_hap_allele_counts) against
tests/hapalleleref.py, the plain-Python restatement of the rule: element for element, no tolerance; that the call leaves tags and scans
alone; and the drivers (hap_vcf --indels, call_sample --phase_output --phase_indels)."""
import gzip
import os
import random
import re

import numpy as np
import pytest

from clair3_rna_amd import hap_vcf
from tests import hapalleleref as HA
from tests import hapcountref as HC
from tests import hapref
from tests import phaseref as P

pytestmark = pytest.mark.gpu

_state = {}


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clean(request):
    """Every test of this module starts and leaves its engine without phase sites and with default parameters."""
    yield
    if "eng" in request.fixturenames:
        from clair3_rna_amd import capi
        e = request.getfixturevalue("eng")
        e.set_phase_sites(None)
        e.params = capi.default_params()
        e.set_params()


def _readset(recs):
    """[(pos0, cigar, seq[, l_seq])], given sorted by pos -> ReadSet."""
    from clair3_rna_amd.reads import ReadSet
    assert [r[0] for r in recs] == sorted(r[0] for r in recs)
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=0, mapq=60, hp=0) for r in recs])
    for i, r in enumerate(recs):
        if len(r) > 3:
            rs.reads["l_seq"][i] = r[3]
    return rs


def _check(eng, rs, table, sites, params=HC.DEFAULT_PARAMS, load=True, lead=0):
    """The engine's count table for (rs, table, sites) under its current filters equals the restatement's under `params`; returns it."""
    exp = HA.counts(rs, table, sites, params)
    if load:
        eng.set_phase_sites(table)
        eng.load_reads(rs)
    query, pool = HA.to_query(sites, lead)
    got = eng.hap_allele_counts(query, pool)
    assert got.shape == (len(sites), 3, 3) and got.dtype == np.uint32
    assert np.array_equal(got, exp), [(int(j), sites[int(j)]["pos"], got[int(j)].tolist(), exp[int(j)].tolist()) for j in np.unique(np.argwhere(got != exp)[:, 0])[:5]]
    return exp


def _site(ref, pos, a, b=None, ps=1):
    """A site on 1-based `pos` of the reference string: a, b = ("snv", letter) / ("ins", letters) / ("del", n); b None: GT 0/1 with REF as A."""
    pair = [a] if b is None else [a, b]
    span = max([x[1] for x in pair if x[0] == "del"] + [0])
    alts = []
    for kind, v in pair:
        base = v if kind == "snv" else ref[pos - 1]
        alts.append(base + (v if kind == "ins" else "") + ref[pos + (v if kind == "del" else 0):pos + span])
    s = HA.site_of_row(pos, ref[pos - 1:pos + span], ",".join(alts), "0/1" if b is None else "1/2", ps)
    assert not isinstance(s, str), (s, pos, a, b)
    return s


def _other(b, k=1):
    return "ACGT"[("ACGT".index(b) + k) % 4]


REF = "".join(random.Random(99).choice("ACGT") for _ in range(700))
TABLE = hapref.make_sites([(p, REF[p - 1], _other(REF[p - 1]), (p // 5) % 2, 1 + (p // 10) % 2) for p in range(5, 700, 5)])


def _read(pos0, ops, edits=None, rng=None):
    """(pos0, cigar, seq) of a read that copies REF under its M ops; inserted and clipped bases are random (rng) or taken from `edits`
    ({op index: bases}); `edits` on an M op replaces its LAST base."""
    rng = rng or random.Random(pos0)
    x, seq = pos0, []
    for k, (op, n) in enumerate(ops):
        if op in "M=X":
            seq += list(REF[x:x + n])
            if edits and k in edits and n:
                seq[-1] = edits[k]
            x += n
        elif op in "DN":
            x += n
        elif op in "IS":
            seq += list(edits[k]) if edits and k in edits else [rng.choice("ACGT") for _ in range(n)]
    return (pos0, "".join("%d%s" % (n, op) for op, n in ops), "".join(seq))


# ---- 1. an SNV-only query is c3r_hap_counts
def _as_alleles(eng, rs, table, query):
    sites = HA.snv_sites(query)
    exp = _check(eng, rs, table, sites)
    old = eng.hap_counts(query)
    assert np.array_equal(old, exp) and np.array_equal(exp, HC.hap_counts(rs, table, query))
    return exp


@pytest.mark.parametrize("case", hapref.CASES, ids=[c[0] for c in hapref.CASES])
def test_snv_queries_equal_hap_counts_on_the_haplotagging_cases(eng, case):
    rs, table = hapref.case_inputs(case)
    query = table.copy()
    query["h1"] = 0
    _as_alleles(eng, rs, table, query)


@pytest.mark.parametrize("seed", range(4))
def test_snv_queries_equal_hap_counts_on_generated_reads(eng, seed):
    _, rs, table, _ = hapref.gen_case(seed)
    rng = random.Random(seed)
    query = table.copy()
    query["h1"] = 0
    query["ps"][::4] = [rng.choice(table["ps"].tolist()) for _ in query[::4]]
    exp = _as_alleles(eng, rs, table, query)
    assert exp[:, 1].sum() > 300 and exp[:, 2].sum() > 300 and exp[:, :, 2].sum() > 20


# ---- 2. generated insertions, deletions and 1/2 sites
def _gen(seed, errors):
    key = (seed, errors)
    if key not in _state:
        ref, rs, rows, truth, planted, _ = HA.gen_case(seed, errors=errors)
        # the true SNVs as the table, in interleaved phase sets: three sets take turns inside every stretch of 30 sites
        table = hapref.make_sites([(p, r, a, int(t), 100 + 3 * (k // 30) + k % 3) for k, ((p, r, a), t) in enumerate(zip(rows, truth))])
        sites = HA.planted_sites(planted) + HA.snv_sites(table[::5])
        sites = HA.nearest_sets(sorted(sites, key=lambda s: s["pos"]), table)
        _state[key] = (ref, rs, table, sites, planted)
    return _state[key]


@pytest.mark.parametrize("errors", [False, True], ids=["clean", "errors"])
@pytest.mark.parametrize("seed", range(4))
def test_generated_indel_and_two_alt_sites_over_interleaved_sets(eng, seed, errors):
    _, rs, table, sites, planted = _gen(seed, errors)
    assert len(planted) >= 30 and sum(p["gt"] == "1/2" for p in planted) >= 5 and len(rs) % 16 != 0 and len(set(table["ps"].tolist())) >= 9
    exp = _check(eng, rs, table, sites, lead=seed % 2)
    at = [j for j, s in enumerate(sites) if HA.flags(s)[1]]                       # the sites with an insertion or a deletion
    assert len(at) >= 30
    print("seed %d errors %d: event sites %d, A %d, B %d, other %d, untagged %d" % (seed, errors, len(at), exp[at, 1:, 0].sum(), exp[at, 1:, 1].sum(),
                                                                                  exp[at, :, 2].sum(), exp[at, 0].sum()))
    assert exp[at, 1:, 0].sum() > 200 and exp[at, 1:, 1].sum() > 200 and exp[at, 0].sum() > 0
    assert (exp[at, :, 2].sum() > 20) if errors else True


# ---- 3. sizes
@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_read_counts_around_a_workgroup(eng, n):
    ins = ["GG", "GG", "GT", "G", ""]
    recs = []
    for k in range(n):
        p0 = 20 + k // 3
        ops = [("M", 30 - p0), ("I", len(ins[k % 5])), ("M", 6)] if ins[k % 5] else [("M", 36 - p0)]
        recs.append(_read(p0, ops, {1: ins[k % 5]}))
    sites = [_site(REF, 30, ("ins", "GG"), ps=2), _site(REF, 31, ("snv", _other(REF[30])), ps=2)]
    exp = _check(eng, _readset(recs), TABLE, sites)
    assert int(exp.sum()) == 2 * n and int(exp[0, :, 1].sum()) == sum(1 for k in range(n) if k % 5 < 2)


@pytest.mark.parametrize("n_sites", [1, 2])
def test_one_and_two_query_sites(eng, n_sites):
    rs = _readset([_read(20, [("M", 10), ("D", 2), ("M", 8)]), _read(22, [("M", 8), ("I", 3), ("M", 8)], {1: "ACT"}), _read(24, [("M", 20)])])
    sites = [_site(REF, 30, ("del", 2), ("ins", "ACT")), _site(REF, 33, ("snv", _other(REF[32])), ("del", 1))][:n_sites]
    exp = _check(eng, rs, TABLE, sites)
    assert exp[0].sum(axis=0).tolist() == [1, 1, 1]


def test_six_hundred_sites_on_consecutive_positions(eng):
    """Sites of every kind on 600 consecutive positions, so that a deletion's anchor is followed by sites under the deletion, and reads
    whose indels sit on many of them."""
    rng = random.Random(5)
    recs = []
    for start in (0, 3, 21, 40, 57, 58):
        ops, x = [], start
        while x < 640:
            n = rng.randint(1, 12)
            ops.append(("M", n))
            x += n
            u = rng.random()
            if u < 0.4:
                ops.append(("I", rng.randint(1, 3)))
            elif u < 0.8:
                d = rng.randint(1, 3)
                ops.append(("D", d))
                x += d
            elif u < 0.9:
                ops.append(("N", 7))
                x += 7
        while ops[-1][0] != "M":
            ops.pop()
        recs.append(_read(start, ops, rng=rng))
    shown = {}                                               # what the reads show behind the last base of an M op, by 1-based position
    for rec in recs:
        x, y = rec[0], 0
        ops = [(o, int(n)) for n, o in re.findall(r"(\d+)([MIDN])", rec[1])]
        for k, (op, n) in enumerate(ops):
            if op == "M" and k + 1 < len(ops) and ops[k + 1][0] in "ID":
                shown.setdefault(x + n, ("ins", rec[2][y + n:y + n + ops[k + 1][1]]) if ops[k + 1][0] == "I" else ("del", ops[k + 1][1]))
            x += n if op in "MDN" else 0
            y += n if op in "MI" else 0
    kinds = []
    for p in range(41, 641):
        a = [("snv", _other(REF[p - 1], 1 + p % 3)), ("ins", "ACGT"[p % 4] * (1 + p % 2)), ("del", 1 + p % 3), ("ins", "ACGT"[p % 4] + "ACGT"[(p // 4) % 4])][p % 4]
        if p in shown and p % 3:
            a = shown[p]                                     # two thirds of the events that a read shows are an allele of their site
        b = None if p % 5 else [("snv", _other(REF[p - 1], 1 + (p + 1) % 3)), ("del", 1 + (p + 1) % 3), ("ins", "TG" + "ACGT"[p % 4])][p % 3]
        kinds.append(_site(REF, p, a, b if b != a else None, ps=1 + (p // 100) % 2))
    assert len(kinds) == 600
    exp = _check(eng, _readset(recs), TABLE, kinds, lead=1)
    assert int(exp.sum()) > 6 * 400 * 0.7 and exp[:, :, 1].sum() > 150 and exp[:, :, 2].sum() > 150 and exp[:, 1:].sum() > 500


# ---- 4. the walk's edges: 40 ops, indels on the op indices where the 16 lanes wrap
def _forty(shape):
    """(ops, indices of the indel ops) of a 40-op read."""
    if shape == "odd":                                       # M on the even indices; 15: I, 31: D
        ops = [("M", 3) if k % 2 == 0 else ("N", 5) for k in range(40)]
        ops[15], ops[31], ops[39] = ("I", 2), ("D", 2), ("S", 2)
        return ops, [15, 31]
    if shape == "even":                                      # a leading soft clip, M on the odd indices; 16: D, 32: I
        ops = [("M", 4) if k % 2 else ("N", 4) for k in range(40)]
        ops[0], ops[16], ops[32] = ("S", 1), ("D", 3), ("I", 1)
        return ops, [16, 32]
    # 15: I and 16: D at once behind it; 31: D and 32: I behind it (19: a D behind an N, which puts an M on 30)
    ops = [("M", 3) if k % 2 == 0 else ("N", 6) for k in range(40)]
    ops[15:20] = [("I", 2), ("D", 1), ("M", 3), ("N", 6), ("D", 1)]
    ops[31:34] = [("D", 2), ("I", 2), ("M", 2)]
    for k in range(34, 40):
        ops[k] = ("M", 3) if k % 2 else ("N", 6)
    return ops, [15, 16, 31, 32]


@pytest.mark.parametrize("serial", [False, True], ids=["plain", "serial"])
@pytest.mark.parametrize("shape", ["odd", "even", "both"])
def test_indels_where_the_lanes_wrap(eng, shape, serial):
    ops, at = _forty(shape)
    assert len(ops) == 40 and all(ops[k][0] in "ID" for k in at) and all(a[0] != b[0] for a, b in zip(ops, ops[1:]))
    rec = _read(10, ops + ([("P", 1)] if serial else []), rng=random.Random(3))
    rs = _readset([rec, _read(10, [("M", 200)])])
    # where every op starts
    x, y, start = 10, 0, []
    for op, n in ops:
        start.append((x, y))
        x += n if op in "MDN" else 0
        y += n if op in "MIS" else 0
    sites = {}
    for k in at:
        if ops[k - 1][0] != "M":
            continue
        p = start[k][0]                                      # 1-based position of the last base before the indel
        bases = rec[2][start[k][1]:start[k][1] + ops[k][1]]
        ev = ("ins", bases) if ops[k][0] == "I" else ("del", ops[k][1])
        sites[p] = _site(REF, p, ev)
        sites[p - 1] = _site(REF, p - 1, ev, ("snv", _other(REF[p - 2])))
    sites[x] = _site(REF, x, ("ins", "AC"))                  # the read's last base
    sites[x - 1] = _site(REF, x - 1, ("del", 1))
    sites = [sites[p] for p in sorted(sites)]
    exp = _check(eng, rs, TABLE, sites)
    hit = [int(exp[j, :, 1].sum()) for j, s in enumerate(sites) if s["pos"] in [start[k][0] for k in at]]
    print(shape, serial, hit)
    # the allele of every indel that follows an M is seen once — unless a D follows the I at once
    assert hit == {"odd": [1, 1], "even": [1, 1], "both": [0, 1]}[shape]


# ---- 5. insertion and deletion edges
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("m", [9, 10])
@pytest.mark.parametrize("ins", ["G", "GT", "GTA", "GTAC"])
def test_insertions_of_both_parities_at_both_parities(eng, ins, m, lead):
    """The inserted bases start at query offset m (odd, even); the pool offset of the allele is `lead` (+ what comes before it)."""
    wrong = ins[:-1] + _other(ins[-1])
    first = _other(ins[0]) + ins[1:]
    recs = [_read(20, [("M", m), ("I", len(ins)), ("M", 5)], {1: ins}),                # the allele
            _read(20, [("M", m), ("I", len(ins)), ("M", 5)], {1: wrong}),              # the last base differs
            _read(20, [("M", m), ("I", len(ins)), ("M", 5)], {1: first}),              # the first base differs
            _read(20, [("M", m), ("I", len(ins) + 1), ("M", 5)], {1: ins + "A"}),      # one longer
            _read(20, [("M", m), ("I", len(ins)), ("M", 5)], {1: ins[:-1] + "N"}),     # an inserted N
            _read(20, [("M", m), ("I", len(ins)), ("M", 5)], {1: ins}) + (m + len(ins) - 1,),      # SEQ ends inside the insertion
            _read(20, [("M", m), ("I", len(ins)), ("M", 5)], {1: ins}) + (m + len(ins),),          # SEQ ends right behind it
            _read(20, [("M", m + 6)])]
    if len(ins) > 1:
        recs.append(_read(20, [("M", m), ("I", len(ins) - 1), ("M", 5)], {1: ins[:-1]}))           # one shorter
    p = 20 + m
    sites = [_site(REF, p, ("ins", ins), ps=1 + (p // 10) % 2), _site(REF, p + 1, ("ins", "TT"), ("ins", ins), ps=1)]
    exp = _check(eng, _readset(recs), TABLE, sites, lead=lead)
    assert exp[0].sum(axis=0).tolist() == [1, 2, len(recs) - 4] and int(exp[1, :, :2].sum()) == 0


def test_deletions_of_the_alleles_length_and_one_off(eng):
    recs = [_read(20, [("M", 10), ("D", n), ("M", 6)]) for n in (1, 2, 3, 4)] + [_read(20, [("M", 20)]), _read(21, [("M", 9), ("D", 2), ("I", 1), ("M", 6)])]
    sites = [_site(REF, 30, ("del", 2)), _site(REF, 31, ("del", 1), ("del", 2)), _site(REF, 33, ("del", 3), ("snv", _other(REF[32])))]
    exp = _check(eng, _readset(recs), TABLE, sites)
    assert exp[0].sum(axis=0).tolist() == [1, 2, 3]


def test_an_snv_site_does_not_look_at_the_event(eng):
    """An SNV on the last base before an insertion that a short SEQ cuts off, and before an I with a D behind it: counted as c3r_hap_counts
    counts it."""
    recs = [_read(20, [("M", 10), ("I", 2), ("M", 6)]) + (11,), _read(20, [("M", 10), ("I", 2), ("D", 1), ("M", 6)]), _read(20, [("M", 10), ("D", 2), ("M", 6)])]
    query = HC.make_query([(30, REF[29], _other(REF[29]), 2)])
    exp = _as_alleles(eng, _readset(recs), TABLE, query)
    assert exp[0].sum(axis=0).tolist() == [3, 0, 0]


FORMS = [("10M2I1D6M", "other"), ("10M1P1D6M", "A"), ("10M1I1P1I6M", "B2"), ("4M0D6M2I6M", "B2"), ("2S1I10M2I6M", "B2"), ("10M1I1P1D6M", "other"),
         ("3H10M2I6M2H", "B2"), ("6=4X2I6M", "B2"), ("10M2I", "B2"), ("10M2I3S", "B2"), ("10M2I5N6M", "B2"), ("10M1P2I6M", "B2"), ("10M", "A"),
         ("10M1D6M", "B1"), ("10M1P1P1D6M", "A"), ("10M0I1D6M", "B1")]


@pytest.mark.parametrize("tail", ["", "0D", "1P"], ids=["as_it_is", "empty_op", "pad"])
@pytest.mark.parametrize("cigar, want", FORMS, ids=[f[0] for f in FORMS])
def test_cigar_forms_on_both_walks(eng, cigar, want, tail):
    """Every form as it is (the plain walk where the form allows it) and with an empty op or a pad behind it (the serial walk)."""
    ops = [(o, int(n)) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar + tail)]
    k_ins = [k for k, (o, n) in enumerate(ops) if o == "I" and k > 0 and n]
    if cigar.startswith("2S1I"):
        k_ins = k_ins[1:]
    rec = _read(20, ops, {k: "G" * 2 if len(k_ins) == 1 else "G" for k in k_ins} if len(k_ins) <= 2 else None)
    rs = _readset([rec, _read(20, [("M", 20)])])
    sites = [_site(REF, 29, ("ins", "GG"), ps=2), _site(REF, 30, ("del", 1), ("ins", "GG"), ps=2), _site(REF, 31, ("ins", "GG"), ps=2)]
    exp = _check(eng, rs, TABLE, sites)
    col = exp[1].sum(axis=0).tolist()                         # the site on the last base of the 10 M: the second read shows no event there
    assert col == {"other": [0, 0, 2], "A": [0, 0, 2], "B2": [0, 1, 1], "B1": [1, 0, 1]}[want], (cigar, col)


def test_a_mixed_site(eng):
    # ACC -> A,TCC in the reads' terms: A = (the reference base, DEL 2), B = (another base, no event)
    r, t = REF[29], _other(REF[29])
    recs = [_read(20, [("M", 20)]),                                            # the reference allele: other
            _read(20, [("M", 10), ("D", 2), ("M", 8)]),                        # allele A
            _read(20, [("M", 10), ("M", 10)], {0: t}),                         # allele B
            _read(20, [("M", 10), ("D", 2), ("M", 8)], {0: _other(r, 2)}),     # the deletion behind another base: other
            _read(20, [("M", 10), ("M", 10)], {0: _other(r, 2)}),              # a third base: other
            _read(20, [("M", 10), ("D", 2), ("M", 8)], {0: "N"}),              # N on the anchor: nothing
            _read(20, [("M", 10), ("D", 2), ("M", 8)], {0: t}),                # B's base with A's event: other
            _read(20, [("M", 10), ("D", 3), ("M", 7)]),                        # DEL 3: other
            _read(20, [("M", 10), ("I", 1), ("M", 7)])]                        # an insertion: other
    sites = [_site(REF, 30, ("del", 2), ("snv", t), ps=2)]
    assert sites[0]["A"] == (r, ("del", 2)) and sites[0]["B"] == (t, HA.NONE) and HA.flags(sites[0]) == (True, True)
    exp = _check(eng, _readset(recs), TABLE, sites)
    assert exp[0].sum(axis=0).tolist() == [1, 1, 6]


def test_five_thousand_reads_on_one_insertion_site(eng):
    recs = [_read(100, [("M", 4), ("I", 3), ("M", 2)], {1: "GAT"})] * 3000 + [_read(100, [("M", 6)])] * 1500 + [_read(100, [("M", 4), ("I", 3), ("M", 2)], {1: "GAA"})] * 500
    table = hapref.make_sites([(101, REF[100], _other(REF[100]), 0, 4)])
    exp = _check(eng, _readset(recs), table, [_site(REF, 104, ("ins", "GAT"), ps=4)])
    assert exp[0].tolist() == [[0, 0, 0], [1500, 3000, 500], [0, 0, 0]]


# ---- 6. filters, a replaced table, errors, side effects
def test_the_filters_change_the_counts_and_not_the_tags(eng):
    _, rs, table, sites, _ = _gen(0, True)
    failing = [i for i in range(len(rs)) if not P.votes(rs.reads[i], P.DEFAULT_PARAMS)]
    assert len(failing) >= 20
    exp = _check(eng, rs, table, sites)
    tags, sets = eng.haplotags(), eng.read_phase_sets().tolist()
    eng.set_params(min_mq=0, excl_flags=0)                    # the reads already loaded are filtered anew
    loose = _check(eng, rs, table, sites, dict(min_mq=0, excl_flags=0), load=False)
    assert int(loose.sum()) > int(exp.sum())
    after = eng.haplotags()
    assert after[0].tolist() == tags[0].tolist() and after[1] == tags[1] and eng.read_phase_sets().tolist() == sets
    eng.set_params(min_mq=61)
    assert eng.hap_allele_counts(*HA.to_query(sites)).sum() == 0 and eng.haplotags()[0].tolist() == tags[0].tolist()


def test_a_table_replaced_after_the_load_moves_tags_sets_and_counts_together(eng):
    _, rs, table, sites, _ = _gen(1, True)
    exp = _check(eng, rs, table, sites)
    tags, ps = eng.haplotags()[0], eng.read_phase_sets()
    other = table.copy()
    other["h1"] ^= 1
    other["ps"] += 100000
    moved = [dict(s, ps=s["ps"] + 100000) for s in sites]
    eng.set_phase_sites(other)                                # reads stay loaded
    exp2 = _check(eng, rs, other, moved, load=False)
    assert eng.read_phase_sets().tolist() == [p + 100000 if p >= 0 else -1 for p in ps.tolist()]
    assert eng.haplotags()[0].tolist() == [{0: 0, 1: 2, 2: 1}[t] for t in tags.tolist()]
    assert np.array_equal(exp2, exp[:, [0, 2, 1], :]) and not np.array_equal(exp2, exp)
    old = eng.hap_allele_counts(*HA.to_query(sites))          # against the old numbers every read is "tagged in another set"
    assert old[:, 1:].sum() == 0 and np.array_equal(old[:, 0], exp.sum(axis=1))


def _bad(name):
    from clair3_rna_amd import capi
    good = [_site(REF, 30, ("ins", "GG")), _site(REF, 31, ("del", 2)), _site(REF, 40, ("snv", _other(REF[39])), ("ins", "ACT"))]
    q, pool = HA.to_query(good)
    index = 1
    if name == "unsorted":
        q["pos"][2], index = 25, 2
    elif name == "repeated":
        q["pos"][1] = 30
    elif name == "pos_below_1":
        q["pos"][0], index = 0, 0
    elif name == "negative_ps":
        q["ps"][1] = -1
    elif name == "bad_base":
        q["b_base"][1] = 3
    elif name == "bad_anchor_base":
        q["a_base"][2], index = 0, 2
    elif name == "unknown_kind":
        q["a_kind"][1] = 3
    elif name == "deletion_of_length_0":
        q["b_len"][1] = 0
    elif name == "insertion_of_length_0":
        q["b_len"][0], index = 0, 0
    elif name == "length_without_an_event":
        q["a_len"][1] = 2
    elif name == "equal_alleles":
        q["a_kind"][1], q["a_len"][1] = capi.HAP_EV_DEL, 2
    elif name == "equal_insertions":
        q["a_kind"][0], q["a_len"][0], q["a_ins_off"][0], index = capi.HAP_EV_INS, 2, 0, 0
    elif name == "insertion_past_the_pool":
        q["b_ins_off"][2], index = 2 * len(pool) - 2, 2
    elif name == "bad_base_in_the_pool":
        pool, index = pool.copy(), 2
        pool[1] = 0xf0 | (pool[1] & 15)                       # the first base of ACT (pool offset 2)
    elif name == "bad_flag":
        q["event_matters"][1] = 2
    return q, pool, index


BAD = ["unsorted", "repeated", "pos_below_1", "negative_ps", "bad_base", "bad_anchor_base", "unknown_kind", "deletion_of_length_0", "insertion_of_length_0",
       "length_without_an_event", "equal_alleles", "equal_insertions", "insertion_past_the_pool", "bad_base_in_the_pool", "bad_flag"]


@pytest.mark.parametrize("name", BAD)
def test_bad_queries_name_the_index(eng, name):
    from clair3_rna_amd import capi
    eng.set_phase_sites(TABLE)
    eng.load_reads(_readset([_read(0, [("M", 100)])]))
    q, pool, index = _bad(name)
    with pytest.raises(capi.C3RError, match="query site %d:" % index):
        eng.hap_allele_counts(q, pool)
    q, pool, _ = _bad("none")                                 # the table the bad ones were made from is a good one: the read copies the
    got = eng.hap_allele_counts(q, pool)                      # reference, so it shows allele A (REF) on 30 and 31 and neither ALT of the 1/2 site on 40
    assert got.sum(axis=1).tolist() == [[1, 0, 0], [1, 0, 0], [0, 0, 1]]
    with pytest.raises(TypeError):
        eng.hap_allele_counts(TABLE, pool)


def test_no_table_is_refused_and_no_sites_and_no_reads_launch_nothing(eng):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    _, rs, table, sites, _ = _gen(0, False)
    q, pool = HA.to_query(sites)
    eng.load_reads(rs)
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        eng.hap_allele_counts(q, pool)
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        eng.hap_allele_counts(None)
    eng.set_phase_sites(table)
    eng.set_profiling(True)
    try:
        eng.reset_kernel_stats()
        assert eng.hap_allele_counts(None).shape == (0, 3, 3) and eng.hap_allele_counts(np.zeros(0, capi.HAP_SITE_DTYPE), pool).shape == (0, 3, 3)
        assert "k_hap_allele_counts" not in eng.kernel_stats()
        assert eng.hap_allele_counts(q, pool).sum() > 0
        stats = eng.kernel_stats()
        assert stats["k_hap_allele_counts"]["launches"] == 1 and "k_hap_counts" not in stats
        eng.load_reads(ReadSet.from_records([]))
        eng.reset_kernel_stats()
        got = eng.hap_allele_counts(q, pool)
        assert got.shape == (len(q), 3, 3) and got.sum() == 0 and "k_hap_allele_counts" not in eng.kernel_stats()
    finally:
        eng.set_profiling(False)
    eng.load_reads(rs)
    last = int(rs.reads["pos"].max()) + 100000               # sites that no read reaches, up to the largest position
    far = [dict(_site(REF, 30, ("ins", "AC")), pos=last), dict(_site(REF, 31, ("del", 2)), pos=last + 1), dict(_site(REF, 32, ("snv", _other(REF[31]))), pos=2000000000)]
    assert eng.hap_allele_counts(*HA.to_query(far)).sum() == 0


def test_tags_and_a_scan_are_the_same_with_and_without_the_call(eng):
    ref, rs, table, sites, _ = _gen(2, True)
    q, pool = HA.to_query(sites)
    eng.set_params(channels=30, min_coverage=2)
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    eng.set_reference(1, ref)

    def scan():
        n = eng.scan(1, len(ref))
        return n, eng.tensors(rescaled=True).tobytes(), eng.tensors(rescaled=False).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()

    plain, tags, sets = scan(), eng.haplotags(), eng.read_phase_sets().tolist()
    assert plain[0] > 20 and tags[1]["n_hp1"] > 30 and tags[1]["n_hp2"] > 30
    eng.load_reads(rs)
    assert eng.hap_allele_counts(q, pool).sum() > 0
    after = eng.haplotags()
    assert after[0].tolist() == tags[0].tolist() and after[1] == tags[1] and eng.read_phase_sets().tolist() == sets
    assert scan() == plain
    assert eng.hap_allele_counts(q[::2], pool).sum() > 0      # after the scan: what it left is still there
    assert (eng.tensors(rescaled=True).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()) == (plain[1], plain[3], plain[4])
    assert scan() == plain


# ---- 7. drivers, on the two-contig sample of the haplotagging tests' driver cases with indel and 1/2 rows added to the VCF
@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """Built the way the sample of tests/test_gpu_hapcount.py is: two contigs in an untagged BAM, the phased VCFs of two thirds of their true
    SNVs as a directory of phased_<ctg>.vcf.gz, and call_sample's phased pass on them WITHOUT --phase_output.  The reads are
    hapalleleref.gen_case's, so the two haplotypes carry insertions, deletions and 1/2 sites; `with` is that pass's VCF with a row added
    for each of them and for the SNVs held out of the phased VCFs."""
    from clair3_rna_amd import bam, bamio, io, synth
    tmp = str(tmp_path_factory.mktemp("hapallele_drivers"))
    contigs, reads, extra = [], {}, {}
    per = os.path.join(tmp, "phased_vcf")
    os.makedirs(per)
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    for name, seed in (("chr1", 11), ("chr2", 12)):
        ref, rs, snvs, truth, planted, _ = HA.gen_case(seed, errors=True)
        contigs.append((name, ref))
        reads[name] = rs
        with gzip.open(os.path.join(per, "phased_%s.vcf.gz" % name), "wt") as f:
            f.write(head + "".join("%s\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s:%d\n" % (name, p, r, a, "1|0" if t else "0|1", 1000 + k // 20)
                                   for k, ((p, r, a), t) in enumerate(zip(snvs, truth)) if k % 3))
        extra[name] = ["%s\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:GQ\t0/1:30\n" % (name, p, r, a) for p, r, a in snvs[::3]]
        extra[name] += ["%s\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:GQ\t%s:30\n" % (name, s["pos"], s["ref"], s["alt"], s["gt"]) for s in planted]
    fa, wfn = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model")
    io.write_fasta(fa, contigs)
    np.save(wfn + ".c3rw.npy", synth.random_weights(30, seed=7))
    bam_fn = os.path.join(tmp, "plain.bam")
    bam.write_bam(bam_fn, [(n, len(r)) for n, r in contigs], reads)
    bamio.index_build(bam_fn)
    s = dict(tmp=tmp, fa=fa, wfn=wfn, bam=bam_fn, per=per, reads=reads)
    _call_sample(s, "base", ["--phased_vcf_fn", per])
    s["final"] = os.path.join(tmp, "base", "output_enable_phasing.vcf.gz")
    assert os.path.isfile(s["final"])
    with gzip.open(s["final"], "rt") as f:
        lines = f.readlines()
    rows = []
    for c in ("chr1", "chr2"):
        own = [ln for ln in lines if ln.startswith(c + "\t")]
        # (where the pass called the position too, the added row comes first and is the candidate; the pass's row stays behind it)
        rows += sorted(extra[c] + own, key=lambda ln: int(ln.split("\t")[1]))
    s["added"] = extra["chr1"] + extra["chr2"]
    s["with"] = os.path.join(tmp, "with_indels.vcf")
    with open(s["with"], "w") as f:
        f.writelines([ln for ln in lines if ln.startswith("#")] + rows)
    return s


def _argv(s, out, extra):
    return ["--bam_fn", s["bam"], "--ref_fn", s["fa"], "--output_dir", os.path.join(s["tmp"], out), "--pileup_model_path", s["wfn"],
            "--phased_pileup_model_path", s["wfn"], "--chunk_num", "3", "--min_coverage", "2"] + list(extra)


def _call_sample(s, out, extra):
    from clair3_rna_amd import call_sample
    assert call_sample.Run(call_sample.build_parser().parse_args(_argv(s, out, ["--enable_phasing_model"] + list(extra))), log=lambda m: None) == 0


def _gz(fn):
    with gzip.open(fn, "rt") as f:
        return f.read()


def _by_hand(s, vcf, out_fn, tsv_fn, extra=(), log=None):
    return hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", s["bam"], "--vcf_fn", vcf, "--phased_vcf_fn", s["per"], "--output_fn", out_fn,
                                                           "--hap_counts_fn", tsv_fn] + list(extra)), log=log or (lambda m: None))


def test_hap_vcf_with_indels_writes_what_the_restatement_gives(sample, tmp_path):
    from clair3_rna_amd import phasedvcf
    out_fn, tsv_fn = str(tmp_path / "phased.vcf.gz"), str(tmp_path / "counts.tsv")
    msgs = []
    n = _by_hand(sample, sample["with"], out_fn, tsv_fn, ["--indels"], msgs.append)
    assert len(msgs) == 2 and all(m.startswith("[INFO] chr") for m in msgs)
    lines = open(sample["with"]).readlines()
    want_rows = {}
    tsv = ["\t".join(hap_vcf.COLUMNS + ("ALLELES",)) + "\n"]
    n_event = n_event_phased = n_two_phased = 0
    for ctg in ("chr1", "chr2"):
        table = phasedvcf.contig_sites(sample["per"], ctg)
        sites, _ = HA.candidates(lines, ctg)
        sites = HA.nearest_sets(sites, table)
        counts = HA.counts(sample["reads"][ctg], table, sites)
        decided = HA.assign(sites, counts)
        for s, d, t in zip(sites, decided, counts):
            tsv.append(HA.counts_line(ctg, s, d, t))
            n_event += int(HA.flags(s)[1])
            if d[0] >= 0:
                want_rows[(ctg, s["pos"])] = (s, d)
                n_event_phased += int(HA.flags(s)[1])
                n_two_phased += int("," in s["alt"])
    print("candidates with an event %d, of them phased %d; 1/2 rows phased %d; rows rewritten %d" % (n_event, n_event_phased, n_two_phased, n))
    assert n == len(want_rows) and n_event >= 60 and n_event_phased >= 40 and n_two_phased >= 8     # the comparison below is about something
    want, has_ps = [], False
    for ln in lines:
        if ln.startswith("#CHROM"):
            want.append('##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set identifier">\n')
        f = ln.split("\t")
        key = (f[0], int(f[1])) if not ln.startswith("#") else None
        if key in want_rows and (f[3], f[4]) == (want_rows[key][0]["ref"], want_rows[key][0]["alt"]):
            ln = HA.rewritten(ln, *want_rows.pop(key))
        want.append(ln)
    assert not want_rows and _gz(out_fn) == "".join(want) and os.path.isfile(out_fn + ".tbi")
    assert open(tsv_fn).read() == "".join(tsv)


def test_without_the_flag_the_added_rows_change_nothing(sample, tmp_path):
    """hap_vcf without --indels on the VCF with the added rows: what the SNV restatement and the SNV writer give, the added rows byte
    for byte, fifteen columns."""
    from clair3_rna_amd import phasedvcf, phasing
    out_fn, tsv_fn = str(tmp_path / "phased.vcf"), str(tmp_path / "counts.tsv")
    n = _by_hand(sample, sample["with"], out_fn, tsv_fn)
    assigned, lines = {}, ["\t".join(hap_vcf.COLUMNS) + "\n"]
    for ctg in ("chr1", "chr2"):
        table = phasedvcf.contig_sites(sample["per"], ctg)
        cands, _ = phasing.candidates_from_vcf(sample["with"], ctg)
        query = HC.nearest_sets(cands, table)
        counts = HC.hap_counts(sample["reads"][ctg], table, query)
        assigned[ctg], _ = HC.assign(query, counts)
        lines += hap_vcf.counts_lines(ctg, query, assigned[ctg], counts)
    exp_fn = str(tmp_path / "exp.vcf")
    assert hap_vcf.write_vcf(sample["with"], assigned, exp_fn) == n and n >= 40
    assert open(out_fn).read() == open(exp_fn).read() and open(tsv_fn).read() == "".join(lines)
    # and the rows of the pass's own VCF on positions without an added row come out of both files the same: the added rows change no other row
    own_fn, own_tsv = str(tmp_path / "own.vcf"), str(tmp_path / "own.tsv")
    _by_hand(sample, sample["final"], own_fn, own_tsv)
    with_rows = set(open(out_fn).readlines())
    added_at = set(tuple(ln.split("\t")[:2]) for ln in sample["added"])
    kept = [ln for ln in open(own_fn) if tuple(ln.split("\t")[:2]) not in added_at]
    assert len(kept) >= 10 and all(ln in with_rows for ln in kept)
    # the added insertion, deletion and 1/2 rows are there byte for byte
    added = [ln for ln in sample["added"] if len(ln.split("\t")[3]) > 1 or len(ln.split("\t")[4]) > 1]
    assert len(added) >= 60 and all(ln in with_rows for ln in added)


def test_call_sample_with_phase_indels_equals_hap_vcf_with_indels_by_hand(sample, tmp_path):
    out_fn, tsv_fn = str(tmp_path / "phased.vcf.gz"), str(tmp_path / "counts.tsv")
    _by_hand(sample, sample["final"], out_fn, tsv_fn, ["--indels"])
    _call_sample(sample, "indels", ["--phased_vcf_fn", sample["per"], "--phase_output", "--phase_indels"])
    out = os.path.join(sample["tmp"], "indels")
    assert open(os.path.join(out, "output_enable_phasing.vcf.gz"), "rb").read() == open(sample["final"], "rb").read()
    assert open(os.path.join(out, "output_enable_phasing_phased.vcf.gz"), "rb").read() == open(out_fn, "rb").read()
    assert open(os.path.join(out, "output_enable_phasing_hap_counts.tsv")).read() == open(tsv_fn).read()
    assert open(tsv_fn).readline().rstrip("\n").split("\t")[-1] == "ALLELES" and "|" in _gz(out_fn)
    # without --phase_indels: the unflagged hap_vcf's bytes, fifteen columns
    plain_fn, plain_tsv = str(tmp_path / "plain.vcf.gz"), str(tmp_path / "plain.tsv")
    _by_hand(sample, sample["final"], plain_fn, plain_tsv)
    _call_sample(sample, "plain", ["--phased_vcf_fn", sample["per"], "--phase_output"])
    out = os.path.join(sample["tmp"], "plain")
    assert open(os.path.join(out, "output_enable_phasing_phased.vcf.gz"), "rb").read() == open(plain_fn, "rb").read()
    assert open(os.path.join(out, "output_enable_phasing_hap_counts.tsv")).read() == open(plain_tsv).read()
    assert open(plain_tsv).readline().rstrip("\n").split("\t") == list(hap_vcf.COLUMNS)


def test_phase_indels_without_phase_output_is_refused(sample):
    from clair3_rna_amd import call_sample
    with pytest.raises(SystemExit) as e:
        call_sample.Run(call_sample.build_parser().parse_args(_argv(sample, "refused", ["--enable_phasing_model", "--phased_vcf_fn", sample["per"], "--phase_indels"])))
    assert str(e.value.code).startswith("[ERROR]") and "--phase_indels" in str(e.value.code) and "--phase_output" in str(e.value.code)
    assert not os.path.exists(os.path.join(sample["tmp"], "refused"))
