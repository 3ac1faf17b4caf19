"""Haplotags from a phase table with insertions, deletions and two-ALT sites on the device (c3r_set_phase_alleles / k_haplotag_alleles)
against tests/hapindelref.py, the plain-Python restatement: tags, the six statistics and the reads' phase sets, element for element, no
tolerance; the life cycle of the two tables; what reads the tags afterwards; and the drivers under --haplotag_indels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import hapalleleref as HA
from tests import hapcountref as HC
from tests import hapindelref as HI
from tests import hapref
from tests.test_gpu_hapallele import _gz, sample  # noqa: F401  (the driver tests' two-contig sample)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREP_READS = 16                                              # reads per workgroup of k_haplotag_alleles (csrc/reads_kernels.hpp)
_state = {}


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clean(request):
    """Every test of this module leaves its engine without a phase table and with default parameters."""
    yield
    if "eng" in request.fixturenames:
        from clair3_rna_amd import capi
        e = request.getfixturevalue("eng")
        e.set_phase_alleles(None, None)
        e.params = capi.default_params()
        e.set_params()


# ---- a reference that is a function of the position, so that reads and sites can stand anywhere below 2^31
def ref_at(x0):
    return "ACGT"[(x0 * 7 + x0 // 3 + x0 // 11) % 4]


def refstr(pos1, n=1):
    return "".join(ref_at(pos1 - 1 + k) for k in range(n))


def _other(b, k=1):
    return "ACGT"[("ACGT".index(b) + k) % 4]


def _read(pos0, ops, edits=None):
    """(pos0, cigar, seq) of a read that copies the reference under its M ops; inserted and clipped bases are T, or taken from `edits`
    ({op index: bases}); `edits` on an M op replaces its LAST base."""
    x, seq = pos0, []
    for k, (op, n) in enumerate(ops):
        if op in "M=X":
            seq += [ref_at(x + d) for d in range(n)]
            if edits and k in edits and n:
                seq[-1] = edits[k]
            x += n
        elif op in "DN":
            x += n
        elif op in "IS":
            seq += list(edits[k]) if edits and k in edits else ["T"] * n
    return (pos0, "".join("%d%s" % (n, op) for op, n in ops), "".join(seq))


def _ops(cigar):
    return [(o, int(n)) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def _readset(recs):
    from clair3_rna_amd.reads import ReadSet
    assert [r[0] for r in recs] == sorted(r[0] for r in recs)
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=0, mapq=60, hp=0) for r in recs])
    for i, r in enumerate(recs):
        if len(r) > 3:
            rs.reads["l_seq"][i] = r[3]
    return rs


def snv(pos, gt, ps, k=1):
    return HI.site(pos, refstr(pos), _other(refstr(pos), k), gt, ps)


def ins(pos, bases, gt, ps):
    return HI.site(pos, refstr(pos), refstr(pos) + bases, gt, ps)


def dele(pos, n, gt, ps):
    return HI.site(pos, refstr(pos, n + 1), refstr(pos), gt, ps)


def two(pos, a, b, gt, ps):
    """A two-ALT site: a, b = ("snv", letter) / ("ins", letters) / ("del", n)."""
    span = max([x[1] for x in (a, b) if x[0] == "del"] + [0])
    alts = [(v if kind == "snv" else refstr(pos)) + (v if kind == "ins" else "") + refstr(pos + 1 + (v if kind == "del" else 0), span - (v if kind == "del" else 0))
            for kind, v in (a, b)]
    return HI.site(pos, refstr(pos, span + 1), ",".join(alts), gt, ps)


def _check(eng, rs, sites, lead=0, load=True, table=True):
    """Tags, statistics and phase sets of the engine for (rs, sites) equal the restatement's; returns them."""
    hp, st, ps = HI.haplotag(rs, sites)
    if table:
        eng.set_phase_alleles(*HI.to_engine(sites, lead))
    if load:
        eng.load_reads(rs)
    got_hp, got_st = eng.haplotags()
    got_ps = eng.read_phase_sets()
    bad = np.flatnonzero((got_hp != hp) | (got_ps != ps))[:5]
    assert not len(bad), [(int(i), int(got_hp[i]), int(hp[i]), int(got_ps[i]), int(ps[i])) for i in bad]
    assert got_st == st and got_hp.dtype == np.uint8 and got_ps.dtype == np.int32
    return hp, st, ps


# ---- 1. on an SNV table the new call is the old one
def _snv_inputs():
    out = []
    for case in hapref.CASES:
        rs, table = hapref.case_inputs(case)
        out.append((case[0], rs, table))
    for seed in range(4):
        _, rs, table, _ = hapref.gen_case(seed)
        out.append(("gen%d" % seed, rs, table))
    return out


def test_an_snv_table_through_either_setter(eng):
    from clair3_rna_amd import capi
    n_tagged = 0
    for name, rs, table in _snv_inputs():
        eng.set_phase_sites(table)
        eng.load_reads(rs)
        old = (eng.haplotags(), eng.read_phase_sets())
        eng.set_phase_alleles(capi.hap_sites_from_snvs(table), table["h1"])
        new = (eng.haplotags(), eng.read_phase_sets())
        assert np.array_equal(old[0][0], new[0][0]) and old[0][1] == new[0][1] and np.array_equal(old[1], new[1]), name
        hp, st, ps = _check(eng, rs, HI.from_snv_table(table), table=False, load=False)
        assert np.array_equal(hp, hapref.haplotag(rs, table)[0]), name
        n_tagged += st["n_hp1"] + st["n_hp2"]
    assert n_tagged > 1000


# ---- 2. generated reads: every planted site and every SNV forms the table, in interleaved sets
def _gen(seed, errors):
    key = (seed, errors)
    if key not in _state:
        ref, rs, rows, truth, planted, hap = HA.gen_case(seed, errors=errors)
        sites = [dict(s, h1=int(p["truth"])) for s, p in zip(HA.planted_sites(planted), planted)]
        sites += [HI.site(p, r, a, "1|0" if t else "0|1", 0) for (p, r, a), t in zip(rows, truth)]
        sites.sort(key=lambda s: s["pos"])
        sites = [dict(s, ps=100 + 3 * (k // 30) + k % 3) for k, s in enumerate(sites)]
        _state[key] = (ref, rs, sites, hap)
    return _state[key]


@pytest.mark.parametrize("errors", [False, True], ids=["clean", "errors"])
@pytest.mark.parametrize("seed", range(4))
def test_generated_reads_over_interleaved_sets(eng, seed, errors):
    _, rs, sites, hap = _gen(seed, errors)
    assert len(rs) == 403 and sum(HA.flags(s)[1] for s in sites) >= 30 and sum("," in s["alt"] for s in sites) >= 5 and len(set(s["ps"] for s in sites)) >= 9
    hp, st, ps = _check(eng, rs, sites, lead=seed % 2)
    print("seed %d errors %d: %s; tags equal to the generator's haplotype %d of %d" % (seed, errors, st, int((hp == hap)[hp > 0].sum()), int((hp > 0).sum())))
    assert st["n_hp1"] > 100 and st["n_hp2"] > 100 and st["n_no_vote"] > 0 and len(set(ps.tolist())) > 5


# ---- 3. group and grid edges
@pytest.mark.parametrize("n", [1, PREP_READS - 1, PREP_READS, PREP_READS + 1])
def test_read_counts_around_a_workgroup(eng, n):
    shown = ["GG", "GG", "GT", "G", ""]
    recs = []
    for k in range(n):
        p0 = 20 + k // 3
        ops = [("M", 30 - p0), ("I", len(shown[k % 5])), ("M", 6)] if shown[k % 5] else [("M", 36 - p0)]
        recs.append(_read(p0, ops, {1: shown[k % 5]}))
    hp, st, _ = _check(eng, _readset(recs), [ins(30, "GG", "1|0", 2), snv(33, "0|1", 2)])
    # GG: two votes for haplotype 1; no insertion: one each, a tie; GT and G: the SNV's vote alone
    assert hp.tolist() == [[1, 1, 1, 1, 0][k % 5] for k in range(n)] and st["n_votes"] == sum([2, 2, 1, 1, 2][k % 5] for k in range(n))


@pytest.mark.parametrize("n_sites", [1, 2])
def test_tables_of_one_and_two_sites(eng, n_sites):
    rs = _readset([_read(20, [("M", 10), ("D", 2), ("M", 8)]), _read(22, [("M", 8), ("I", 3), ("M", 8)], {1: "ACT"}), _read(24, [("M", 20)])])
    sites = [two(30, ("del", 2), ("ins", "ACT"), "1|2", 7), two(33, ("snv", _other(refstr(33))), ("del", 1), "2|1", 7)][:n_sites]
    hp, _, _ = _check(eng, rs, sites)
    assert hp.tolist() == [1, 2, 0]


def test_six_hundred_sites_on_consecutive_positions(eng):
    """Sites of every kind on 600 consecutive positions — a deletion's anchor is followed by sites under the deletion — in five phase sets
    that take turns, and reads whose indels sit on many of them: the group search and the walk per set."""
    import random
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
        recs.append(_read(start, ops, {k: "".join(rng.choice("ACGT") for _ in range(n)) for k, (op, n) in enumerate(ops) if op == "I"}))
    shown = {}                                               # what the reads show behind the last base of an M op, by 1-based position
    for rec in recs:
        x, y = rec[0], 0
        ops = _ops(rec[1])
        for k, (op, n) in enumerate(ops):
            if op == "M" and k + 1 < len(ops) and ops[k + 1][0] in "ID":
                shown.setdefault(x + n, ("ins", rec[2][y + n:y + n + ops[k + 1][1]]) if ops[k + 1][0] == "I" else ("del", ops[k + 1][1]))
            x += n if op in "MDN" else 0
            y += n if op in "MI" else 0
    sites = []
    for p in range(41, 641):
        gt, ps = ("0|1", "1|0")[p % 2], 1 + (p // 7) % 5
        a = [("snv", _other(refstr(p), 1 + p % 3)), ("ins", "ACGT"[p % 4] * (1 + p % 2)), ("del", 1 + p % 3), ("ins", "ACGT"[p % 4] + "ACGT"[(p // 4) % 4])][p % 4]
        if p in shown and p % 3:
            a = shown[p]                                     # two thirds of the events that a read shows are an allele of their site
        b = None if p % 5 else [("snv", _other(refstr(p), 1 + (p + 1) % 3)), ("del", 1 + (p + 1) % 3), ("ins", "TG" + "ACGT"[p % 4])][p % 3]
        if b is None or b == a:
            sites.append({"snv": lambda: snv(p, gt, ps, 1 + p % 3), "ins": lambda: ins(p, a[1], gt, ps), "del": lambda: dele(p, a[1], gt, ps)}[a[0]]())
        else:
            sites.append(two(p, a, b, gt.replace("0", "2"), ps))
    assert len(sites) == 600 and [s["pos"] for s in sites] == list(range(41, 641))
    hp, st, ps = _check(eng, _readset(recs), sites, lead=1)
    assert st["n_votes"] > 1500 and st["n_no_vote"] == 0 and len(set(ps.tolist())) >= 2      # (the restatement alone: 2255 votes — the comparison is about something)


# ---- 4. insertions of both parities at both parities, on both walks
@pytest.mark.parametrize("m", [9, 10])
@pytest.mark.parametrize("bases", ["G", "GT", "GTA", "GTAC"])
def test_insertions_of_both_parities_at_both_parities(eng, bases, m):
    """The inserted bases start at query offset clip + m (odd, even); the allele's offset in the pool is `lead`; a trailing empty op sends
    the read down the serial walk."""
    n = len(bases)
    for clip in (0, 1):
        for tail in ([], [("D", 0)]):
            def rd(shown, k=n, l_seq=None, clip=clip, tail=tail):
                head = [("S", clip)] if clip else []
                r = _read(20, head + [("M", m), ("I", k), ("M", 5)] + tail, {len(head) + 1: shown})
                return r if l_seq is None else r + (l_seq,)
            recs = [rd(bases),                                                      # the allele: two votes for haplotype 1
                    rd(bases[:-1] + _other(bases[-1])),                             # the last base differs: the SNV's vote alone
                    rd(_other(bases[0]) + bases[1:]),                               # the first base differs
                    rd(bases + "A", n + 1),                                         # one longer
                    rd(bases[:-1] + "N"),                                           # an inserted N
                    rd(bases, l_seq=clip + m + n - 1),                              # SEQ ends inside the insertion: no observation, and no base behind it
                    rd(bases, l_seq=clip + m + n),                                  # SEQ ends right behind it: the insertion's vote alone
                    _read(20, ([("S", clip)] if clip else []) + [("M", m + 6)] + tail)]    # no insertion: allele A, a tie with the SNV's vote
            p = 20 + m
            sites = [ins(p, bases, "1|0", 3), snv(p + 2, "0|1", 3)]
            for lead in (0, 1):
                hp, st, _ = _check(eng, _readset(recs), sites, lead=lead)
                assert hp.tolist() == [1, 1, 1, 1, 1, 0, 1, 0] and st["n_votes"] == 2 + 1 + 1 + 1 + 1 + 0 + 1 + 2, (clip, tail, lead)


# ---- 5. CIGAR forms on both walks
# (CIGAR, the site on 30, what the read shows there: 0 — allele A —, 1 — allele B —, None — another allele or nothing, no vote).  The site is
# "mix": a deletion of one (A) and the insertion GG (B), GT 1|2; or "del2": REF (A) and a deletion of two (B), GT 0|1.
FORMS = [("10M2I1D6M", "mix", None),                         # I then D: the `+<ins>-<del>` column
         ("10M1D6M", "mix", 0), ("10M2D6M", "mix", None),     # a D of the allele's length, and one longer
         ("10M2D6M", "del2", 1), ("10M1D6M", "del2", None), ("10M3D6M", "del2", None), ("10M", "del2", 0),      # the same allele one shorter and one longer
         ("10M1P1D6M", "mix", None), ("10M1P2D6M", "del2", 0),                                                   # a pad before the D: no event
         ("10M5N6M", "mix", None), ("10M2I3S", "mix", 1), ("10M2I", "mix", 1), ("10M", "mix", None), ("8M2=2I6M", "mix", 1), ("7M3=", "mix", None),
         ("2S10M2I6M", "mix", 1), ("3H10M2I6M2H", "mix", 1), ("10M1P2I6M", "mix", 1)]


@pytest.mark.parametrize("tail", ["", "0D", "1P"], ids=["as_it_is", "empty_op", "pad"])
@pytest.mark.parametrize("cigar, kind, shown", FORMS, ids=["%s-%s" % f[:2] for f in FORMS])
def test_cigar_forms_on_both_walks(eng, cigar, kind, shown, tail):
    """Every form as it stands (the plain walk where the form allows it) and with an empty op or a pad behind it (the serial walk), against
    the site on 30, the last base of the ten M.  The site on 28 (`8M2=`: the first op's last base, inside the merged op) sees no event
    anywhere: allele A."""
    ops = _ops(cigar + tail)
    rec = _read(20, ops, {k: "GG" for k, (o, n) in enumerate(ops) if o == "I" and n == 2})
    rs = _readset([rec, _read(20, [("M", 20)])])
    on30 = two(30, ("del", 1), ("ins", "GG"), "1|2", 2) if kind == "mix" else dele(30, 2, "0|1", 2)
    sites = [ins(28, "GG", "1|0", 5), on30, ins(32, "GG", "0|1", 2)]
    _check(eng, rs, sites)
    votes = HI.votes_of(rs, 0, {s["pos"]: (j, s) for j, s in enumerate(sites)})
    assert (0, 0) in votes and ((1, 1) in votes) == (shown == 1) and ((1, 0) in votes) == (shown == 0), (cigar, kind, votes)


def test_an_insertion_cut_off_by_a_short_seq(eng):
    rec = _read(20, [("M", 10), ("I", 2), ("M", 6)], {1: "GG"})
    for tail in ("", "0D", "1P"):
        rs = _readset([(rec[0], rec[1] + tail, rec[2], 11), (rec[0], rec[1] + tail, rec[2], 12), (rec[0], rec[1] + tail, rec[2])])
        hp, _, _ = _check(eng, rs, [ins(30, "GG", "1|0", 1)])
        assert hp.tolist() == [0, 1, 1]
        hp, _, _ = _check(eng, rs, [snv(30, "0|1", 1)])      # the event does not matter there: the base votes
        assert hp.tolist() == [1, 1, 1]


# ---- 6. the hand-derived cases of the restatement
@pytest.mark.parametrize("case", HI.CASES, ids=[c[0] for c in HI.CASES])
def test_hand_derived_cases(eng, case):
    rs, sites = HI.case_inputs(case)
    hp, _, ps = _check(eng, rs, sites)
    assert hp.tolist() == [e[0] for e in case[3]] and ps.tolist() == [e[3] for e in case[3]]


def test_a_read_that_covers_only_an_indel_is_tagged_now(eng):
    """What the feature exists for: under the SNV rows alone the read has no vote; with the deletion in the table it is tagged."""
    case = [c for c in HI.CASES if c[0] == "only_an_indel_on_the_read"][0]
    rs, sites = HI.case_inputs(case)
    eng.set_phase_sites(hapref.make_sites([(50, "A", "C", 0, 5)]))
    eng.load_reads(rs)
    hp, st = eng.haplotags()
    assert hp.tolist() == [0] and st["n_no_vote"] == 1 and eng.read_phase_sets().tolist() == [-1]
    eng.set_phase_alleles(*HI.to_engine(sites))
    hp, st = eng.haplotags()
    assert hp.tolist() == [1] and st["n_hp1"] == 1 and st["n_votes"] == 1 and eng.read_phase_sets().tolist() == [5]


# ---- 7. several sets
def test_three_interleaved_sets_where_an_indel_vote_decides(eng):
    # 12M 1D 12M at 100: bases on 101 .. 112 and 114 .. 125.  Sets 8, 4 and 6 take turns; 8 and 4 hold two SNV votes each, the deletion behind 112 is 4's third
    rs = _readset([_read(100, [("M", 12), ("D", 1), ("M", 12)])])
    snvs = [snv(102, "0|1", 8), snv(104, "1|0", 4), snv(106, "0|1", 6), snv(108, "0|1", 8), snv(110, "1|0", 4)]
    hp, st, ps = _check(eng, rs, snvs)
    assert (hp.tolist(), ps.tolist(), st["n_votes"]) == ([1], [8], 5)           # without the indel: 8 and 4 are equal and 8 votes first
    hp, st, ps = _check(eng, rs, snvs + [dele(112, 1, "1|0", 4)])
    assert (hp.tolist(), ps.tolist(), st["n_votes"]) == ([2], [4], 6)           # 4 holds three: REF, REF under 1|0 and the deletion under 1|0 — 1 : 2
    # equal again, and the first voting site decides: the insertion-site on 101 is set 6's and comes first in the table
    hp, st, ps = _check(eng, rs, [ins(101, "T", "1|0", 6)] + snvs[:4])
    assert (hp.tolist(), ps.tolist(), st["n_votes"]) == ([0], [-1], 5)          # 6: no insertion under 1|0 and REF under 0|1 — 1 : 1, the winner is tied
    hp, st, ps = _check(eng, rs, [ins(101, "T", "0|1", 6)] + snvs[:4])
    assert (hp.tolist(), ps.tolist()) == ([1], [6])


# ---- 8. chromosome-scale coordinates
@pytest.mark.parametrize("end", [248000000, 2 ** 31 - 1], ids=["248M", "int32_max"])
def test_positions_of_a_chromosome_and_the_last_one_the_load_accepts(eng, end):
    """Reads whose last base lies on 1-based `end` (INT32_MAX: the last the load accepts, include/c3r.h "coordinates"), a deletion and an
    insertion before it and an SNV on it."""
    p0 = end - 40
    recs = [_read(p0, [("M", 10), ("D", 3), ("M", 10), ("I", 2), ("M", 17)], {3: "CA"}), _read(p0, [("M", 40)]), _read(p0 + 25, [("M", 15)], {0: _other(refstr(end))})]
    sites = [snv(p0 + 2, "0|1", p0), dele(p0 + 10, 3, "1|0", p0), ins(p0 + 23, "CA", "1|0", p0), snv(end, "1|0", end)]
    assert sites[-1]["pos"] == end and all(r[0] + sum(n for o, n in _ops(r[1]) if o in "MDN") == end for r in recs)
    hp, st, ps = _check(eng, _readset(recs), sites)
    # read 0: REF, deletion, insertion, REF on the last base: 3 : 0 in set p0; read 1: 1 : 2 in set p0; read 2: the ALT on the last base alone
    assert hp.tolist() == [1, 2, 1] and ps.tolist() == [p0, p0, end] and st["n_votes"] == 4 + 4 + 1


# ---- 9. life cycle
def test_a_table_set_after_the_load_moves_tags_and_sets_together(eng):
    _, rs, sites, _ = _gen(1, True)
    eng.load_reads(rs)
    hp, _, ps = _check(eng, rs, sites, load=False)
    moved = [dict(s, h1=1 - s["h1"], ps=s["ps"] + 100000) for s in sites]
    hp2, _, ps2 = _check(eng, rs, moved, load=False)
    assert hp2.tolist() == [{0: 0, 1: 2, 2: 1}[t] for t in hp.tolist()] and ps2.tolist() == [p + 100000 if p >= 0 else -1 for p in ps.tolist()]


def test_each_setter_replaces_the_others_table(eng):
    from clair3_rna_amd import capi
    _, rs, sites, _ = _gen(0, True)
    table = hapref.make_sites([(s["pos"], s["ref"], s["alt"], 1 - s["h1"], 7) for s in sites if len(s["ref"]) == 1 and len(s["alt"]) == 1])
    assert len(table) >= 100
    eng.set_profiling(True)
    try:
        hp, _, _ = _check(eng, rs, sites)
        eng.reset_kernel_stats()
        eng.set_phase_sites(table)                           # the SNV table after the allele table
        old = eng.haplotags()[0]
        assert np.array_equal(old, hapref.haplotag(rs, table)[0]) and not np.array_equal(old, hp)
        assert np.array_equal(eng.read_phase_sets(), HC.read_phase_sets(rs, table))
        ks = eng.kernel_stats()
        assert ks["k_haplotag"]["launches"] == 1 and "k_haplotag_alleles" not in ks
        eng.reset_kernel_stats()
        eng.load_reads(rs)                                   # and it stays for the next load
        assert np.array_equal(eng.haplotags()[0], old) and "k_haplotag_alleles" not in eng.kernel_stats()
        eng.reset_kernel_stats()
        _check(eng, rs, sites, load=False)                   # the allele table after the SNV table
        ks = eng.kernel_stats()
        assert ks["k_haplotag_alleles"]["launches"] == 1 and "k_haplotag" not in ks
        eng.reset_kernel_stats()
        _check(eng, rs, sites, table=False)
        ks = eng.kernel_stats()
        assert ks["k_haplotag_alleles"]["launches"] == 1 and "k_haplotag" not in ks
    finally:
        eng.set_profiling(False)
    with pytest.raises(TypeError):
        eng.set_phase_alleles(table, table["h1"])
    with pytest.raises(TypeError):
        eng.set_phase_alleles(capi.hap_sites_from_snvs(table), table["h1"][:-1])


@pytest.mark.parametrize("clear", ["alleles", "sites"])
def test_an_empty_table_through_either_setter_brings_back_the_records_own_tags(eng, clear):
    from clair3_rna_amd import capi
    ref, rs, sites, hap = _gen(2, True)
    own = hapref.with_hp(rs, hap)                            # records that carry tags of their own

    def scan(e):
        n = e.scan(1, len(ref))
        return n, e.tensors(rescaled=True).tobytes(), e.tensors(rescaled=False).tobytes(), e.sites().tobytes(), e.tokens().tobytes()

    fresh = capi.Engine(0)                                   # a context that never held a table
    try:
        fresh.set_params(channels=30, min_coverage=2)
        fresh.load_reads(own)
        fresh.set_reference(1, ref)
        want = scan(fresh)
    finally:
        fresh.close()
    eng.set_params(channels=30, min_coverage=2)
    eng.set_phase_alleles(*HI.to_engine(sites))
    eng.load_reads(own)
    eng.set_reference(1, ref)
    tagged = scan(eng)
    assert want[0] > 20 and tagged[1] != want[1]
    if clear == "alleles":
        eng.set_phase_alleles(None, None)
    else:
        eng.set_phase_sites(None)
    with pytest.raises(capi.C3RError, match="no phase sites"):
        eng.haplotags()
    with pytest.raises(capi.C3RError, match="no phase sites"):
        eng.read_phase_sets()
    assert scan(eng) == want
    eng.load_reads(own)
    assert scan(eng) == want


def test_no_reads_and_no_sites_launch_nothing(eng):
    from clair3_rna_amd.reads import ReadSet
    _, rs, sites, _ = _gen(0, False)
    eng.set_profiling(True)
    try:
        eng.load_reads(ReadSet.from_records([]))
        eng.reset_kernel_stats()
        eng.set_phase_alleles(*HI.to_engine(sites))          # no reads loaded
        hp, st = eng.haplotags()
        assert len(hp) == 0 and st["n_reads"] == 0 and len(eng.read_phase_sets()) == 0
        eng.set_phase_alleles(None, None)                    # n = 0
        eng.set_phase_alleles(None, None)
        eng.load_reads(rs)
        assert not [k for k in eng.kernel_stats() if "haplotag" in k], eng.kernel_stats()
        eng.set_phase_alleles(*HI.to_engine(sites))
        assert eng.kernel_stats()["k_haplotag_alleles"]["launches"] == 1
        eng.reset_kernel_stats()
        eng.set_phase_alleles(None, None)
        assert not [k for k in eng.kernel_stats() if "haplotag" in k]
    finally:
        eng.set_profiling(False)


# ---- 10. bad tables
def _bad(name):
    from clair3_rna_amd import capi
    good = [ins(30, "GG", "0|1", 1), dele(31, 2, "1|0", 1), two(40, ("snv", _other(refstr(40))), ("ins", "ACT"), "1|2", 2)]
    q, h1, pool, n = HI.to_engine(good)
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
    elif name == "unknown_kind":
        q["a_kind"][1] = 3
    elif name == "deletion_of_length_0":
        q["b_len"][1] = 0
    elif name == "length_without_an_event":
        q["a_len"][1] = 2
    elif name == "equal_alleles":
        q["a_kind"][1], q["a_len"][1] = capi.HAP_EV_DEL, 2
    elif name == "insertion_past_the_pool":
        q["b_ins_off"][2], index = n - 2, 2
    elif name == "bad_base_in_the_pool":
        pool, index = pool.copy(), 2
        pool[1] = 0xf0 | (pool[1] & 15)                       # the first base of ACT (pool offset 2)
    elif name == "bad_flag":
        q["event_matters"][1] = 2
    elif name == "h1_above_1":
        h1[2], index = 2, 2
    return q, h1, pool, n, index


BAD = ["unsorted", "repeated", "pos_below_1", "negative_ps", "bad_base", "unknown_kind", "deletion_of_length_0", "length_without_an_event", "equal_alleles",
       "insertion_past_the_pool", "bad_base_in_the_pool", "bad_flag", "h1_above_1"]


@pytest.mark.parametrize("name", BAD)
def test_bad_tables_name_the_index_and_leave_the_table_in_force(eng, name):
    from clair3_rna_amd import capi
    rs = _readset([_read(0, [("M", 28), ("D", 2), ("M", 20)])])
    eng.set_phase_alleles(*HI.to_engine([dele(28, 2, "1|0", 9)]))
    eng.load_reads(rs)
    assert eng.haplotags()[0].tolist() == [1]
    q, h1, pool, n, index = _bad(name)
    with pytest.raises(capi.C3RError, match="phase allele site %d:" % index) as e:
        eng.set_phase_alleles(q, h1, pool, n)
    assert e.value.code == -1                                # C3R_EINVAL
    assert eng.haplotags()[0].tolist() == [1] and eng.read_phase_sets().tolist() == [9]
    q, h1, pool, n, _ = _bad("none")                         # the table the bad ones were made from is a good one
    eng.set_phase_alleles(q, h1, pool, n)
    # 30 lies under the read's D: nothing; 31 is the first base behind it and shows no deletion: A under 1|0, haplotype 2; 40 shows neither ALT
    assert eng.haplotags()[0].tolist() == [2] and eng.read_phase_sets().tolist() == [1]


# ---- 11. what reads the tags afterwards
def test_the_counts_follow_the_new_tags(eng):
    _, rs, sites, _ = _gen(3, True)
    hp, _, ps = _check(eng, rs, sites)
    query = [dict(s) for s in sites[::3]]
    q, pool = HA.to_query(query, 1)
    assert np.array_equal(eng.hap_allele_counts(q, pool), HI.allele_counts(rs, hp, ps, query))
    snvs = hapref.make_sites([(s["pos"], s["ref"], s["alt"], 0, s["ps"]) for s in sites if len(s["ref"]) == 1 and len(s["alt"]) == 1])
    got = eng.hap_counts(snvs)
    assert np.array_equal(got, HI.snv_counts(rs, hp, ps, snvs)) and got[:, 1:].sum() > 500
    after = eng.haplotags()[0]
    assert np.array_equal(after, hp) and np.array_equal(eng.read_phase_sets(), ps)


def test_the_thirty_channel_tensors_are_those_of_records_that_carry_the_tags(eng):
    from clair3_rna_amd import capi
    ref, rs, sites, _ = _gen(2, True)
    hp, _, _ = HI.haplotag(rs, sites)

    def scan(e):
        n = e.scan(1, len(ref))
        return n, e.tensors(rescaled=True).tobytes(), e.tensors(rescaled=False).tobytes(), e.sites().tobytes(), e.tokens().tobytes()

    eng.set_params(channels=30, min_coverage=2)
    eng.set_phase_alleles(*HI.to_engine(sites))
    eng.load_reads(rs)
    eng.set_reference(1, ref)
    got = scan(eng)
    other = capi.Engine(0)
    try:
        other.set_params(channels=30, min_coverage=2)
        other.load_reads(hapref.with_hp(rs, hp))
        other.set_reference(1, ref)
        want = scan(other)
        other.load_reads(rs)
        assert scan(other)[1] != want[1]                     # the tags show in the tensors: the comparison below can fail
    finally:
        other.close()
    assert got[0] > 20 and got == want


# ---- 12. drivers
def _phased_table(lines, ctg):
    """The restatement's own reading of a phased VCF: the first row of a position whose GT is one of the four and whose alleles reduce."""
    sites, seen = [], set()
    for ln in lines:
        f = ln.rstrip("\n").split("\t")
        if ln.startswith("#") or f[0] != ctg:
            continue
        fmt = dict(zip(f[8].split(":"), f[9].split(":")))
        if fmt.get("GT") not in ("0|1", "1|0", "1|2", "2|1"):
            continue
        s = HA.site_of_row(int(f[1]), f[3], f[4], fmt["GT"].replace("|", "/"), int(fmt.get("PS", 0)))
        if isinstance(s, str) or s["pos"] in seen:
            continue
        seen.add(s["pos"])
        sites.append(dict(s, h1=1 if fmt["GT"] in ("1|0", "2|1") else 0))
    return sorted(sites, key=lambda s: s["pos"])


@pytest.fixture(scope="module")
def phased(sample):
    """Step 1 of the recipe on the sample: the VCF with indel and two-ALT rows, phased by hap_vcf --indels from the SNV-only phased VCFs
    (what call_sample --phase_output --phase_indels runs); the restatement's table, tags and sets per contig; a BAM that carries those tags."""
    from clair3_rna_amd import bam, bamio, hap_vcf, io
    s = dict(sample)
    s["x"] = os.path.join(s["tmp"], "with_indels_phased.vcf.gz")
    hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", s["bam"], "--vcf_fn", s["with"], "--phased_vcf_fn", s["per"], "--output_fn", s["x"], "--indels"]),
                log=lambda m: None)
    lines = _gz(s["x"]).splitlines(True)
    s["table"], s["tags"], s["sets"], tagged = {}, {}, {}, {}
    for ctg in ("chr1", "chr2"):
        s["table"][ctg] = _phased_table(lines, ctg)
        s["tags"][ctg], _, s["sets"][ctg] = HI.haplotag(s["reads"][ctg], s["table"][ctg])
        tagged[ctg] = hapref.with_hp(s["reads"][ctg], s["tags"][ctg])
    both = s["table"]["chr1"] + s["table"]["chr2"]
    n_event = sum(HA.flags(t)[1] for t in both)
    assert n_event >= 40 and sum("," in t["alt"] for t in both) >= 8 and len(both) - n_event >= 40       # (hap_vcf --indels phases that many on this sample)
    s["tagged_bam"] = os.path.join(s["tmp"], "tagged_by_the_restatement.bam")
    contigs = [(row[0], row[1]) for row in io.read_fai(s["fa"])]
    bam.write_bam(s["tagged_bam"], contigs, tagged)
    bamio.index_build(s["tagged_bam"])
    return s


def _pass(s, out, bam_fn, extra, log=None):
    from clair3_rna_amd import call_sample
    argv = ["--bam_fn", bam_fn, "--ref_fn", s["fa"], "--output_dir", os.path.join(s["tmp"], out), "--pileup_model_path", s["wfn"], "--phased_pileup_model_path", s["wfn"],
            "--chunk_num", "3", "--min_coverage", "2", "--enable_phasing_model"] + list(extra)
    assert call_sample.Run(call_sample.build_parser().parse_args(argv), log=log or (lambda m: None)) == 0
    return open(os.path.join(s["tmp"], out, "output_enable_phasing.vcf.gz"), "rb").read()


def test_call_sample_with_the_flag_writes_the_bytes_of_the_tagged_bam(phased):
    msgs = []
    want = _pass(phased, "hi_tagged", phased["tagged_bam"], [])
    got = _pass(phased, "hi_flag", phased["bam"], ["--phased_vcf_fn", phased["x"], "--haplotag_indels"], msgs.append)
    assert got == want
    assert _pass(phased, "hi_snv", phased["bam"], ["--phased_vcf_fn", phased["x"]]) != want      # the SNV rows alone tag differently: the comparison can fail
    for ctg in ("chr1", "chr2"):
        t = phased["table"][ctg]
        line = "[INFO] %s: %d phased sites in the table of --haplotag_indels, %d with an insertion or deletion, %d with two ALTs" % (
            ctg, len(t), sum(HA.flags(x)[1] for x in t), sum("," in x["alt"] for x in t))
        assert line in msgs, (line, msgs)


def test_call_var_bam_with_the_flag_writes_the_bytes_of_the_tagged_bam(phased, tmp_path):
    from clair3_rna_amd import call_var_bam

    def chunk(out, bam_fn, extra):
        fn = str(tmp_path / out)
        argv = ["--chkpnt_fn", phased["wfn"], "--bam_fn", bam_fn, "--ref_fn", phased["fa"], "--ctgName", "chr1", "--pileup", "--enable_phasing_model", "True",
                "--minCoverage", "2", "--call_fn", fn] + extra
        call_var_bam.Run(call_var_bam.build_parser().parse_args(argv))
        return open(fn).read()

    want = chunk("tagged.vcf", phased["tagged_bam"], [])
    assert chunk("flag.vcf", phased["bam"], ["--phased_vcf_fn", phased["x"], "--haplotag_indels"]) == want and want.count("\n") > 10
    assert chunk("snv.vcf", phased["bam"], ["--phased_vcf_fn", phased["x"]]) != want


def test_haplotag_bam_with_the_flag_writes_the_restatements_tags(phased, tmp_path):
    from clair3_rna_amd import haplotag_bam
    from tests import bamref
    out = str(tmp_path / "bams")
    msgs = []
    haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", phased["bam"], "--phased_vcf_fn", phased["x"], "--output_dir", out, "--haplotag_indels"]), log=msgs.append)
    for ctg in ("chr1", "chr2"):
        got = bamref.Bam(os.path.join(out, ctg + ".bam"))
        assert [r.tag("HP")[1] if r.tag("HP") else 0 for r in got.records] == phased["tags"][ctg].tolist()
        assert [r.tag("PS")[1] if r.tag("PS") else -1 for r in got.records] == phased["sets"][ctg].tolist()
        t = phased["table"][ctg]
        assert any(m.startswith("[INFO] %s:" % ctg) and "%d phased sites (--haplotag_indels: %d with an insertion or deletion, %d with two ALTs)"
                   % (len(t), sum(HA.flags(x)[1] for x in t), sum("," in x["alt"] for x in t)) in m for m in msgs), msgs


def test_hap_vcf_with_both_flags_counts_under_the_new_tags(phased, tmp_path):
    from clair3_rna_amd import hap_vcf
    out_fn, tsv_fn = str(tmp_path / "p.vcf"), str(tmp_path / "c.tsv")
    hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", phased["bam"], "--vcf_fn", phased["with"], "--phased_vcf_fn", phased["x"], "--output_fn", out_fn,
                                                   "--hap_counts_fn", tsv_fn, "--indels", "--haplotag_indels"]), log=lambda m: None)
    lines = open(phased["with"]).readlines()
    tsv = ["\t".join(hap_vcf.COLUMNS + ("ALLELES",)) + "\n"]
    n_phased = 0
    for ctg in ("chr1", "chr2"):
        cands, _ = HA.candidates(lines, ctg)
        cands = HA.nearest_sets(cands, phased["table"][ctg])
        counts = HI.allele_counts(phased["reads"][ctg], phased["tags"][ctg], phased["sets"][ctg], cands)
        decided = HA.assign(cands, counts)
        n_phased += sum(d[0] >= 0 for d in decided)
        tsv += [HA.counts_line(ctg, s, d, t) for s, d, t in zip(cands, decided, counts)]
    assert open(tsv_fn).read() == "".join(tsv) and n_phased >= 40
    assert sum("|" in ln.split("\t")[9] for ln in open(out_fn) if not ln.startswith("#")) == n_phased


def _closes(s, x, out):
    """Step 2 on the file `x` of step 1: the pass accepts it and its [INFO] lines count the rows step 1 phased.  -> (sites, with an indel, with two ALTs)."""
    msgs = []
    _pass(s, out, s["bam"], ["--phased_vcf_fn", x, "--haplotag_indels"], msgs.append)
    lines = _gz(x).splitlines(True)
    total = [0, 0, 0]
    for ctg in ("chr1", "chr2"):
        t = _phased_table(lines, ctg)
        n = (len(t), sum(HA.flags(site)[1] for site in t), sum("," in site["alt"] for site in t))
        line = "[INFO] %s: %d phased sites in the table of --haplotag_indels, %d with an insertion or deletion, %d with two ALTs" % ((ctg,) + n)
        assert line in msgs, (line, msgs)
        total = [a + b for a, b in zip(total, n)]
    return total


def test_the_two_step_recipe_closes(phased):
    """Step 1: --phase_output --phase_indels writes <prefix>_enable_phasing_phased.vcf.gz.  Step 2 takes that file as --phased_vcf_fn with
    --haplotag_indels: its table holds every indel and two-ALT row step 1 phased.  The pass's own VCF comes from random weights and need
    not hold a heterozygous indel, so the same is done with the file step 1's command (hap_vcf --indels, what --phase_output --phase_indels
    runs) makes of the VCF with the planted indel and 1/2 rows: there the indel and two-ALT rows are many, and they come back."""
    _pass(phased, "step1", phased["bam"], ["--phased_vcf_fn", phased["per"], "--phase_output", "--phase_indels"])
    own = _closes(phased, os.path.join(phased["tmp"], "step1", "output_enable_phasing_phased.vcf.gz"), "step2")
    planted = _closes(phased, phased["x"], "step2_planted")
    print("rows step 1 phased (sites, with an indel, with two ALTs): the pass's own VCF %s, the VCF with planted rows %s" % (own, planted))
    assert own[0] > 0 and planted[1] >= 40 and planted[2] >= 8          # (the floors the `phased` fixture holds for the restatement's reading)


# ---- the C ABI alone
def test_the_stand_alone_check_program(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to build tests/c/phase_alleles_check.c"
    lib = os.path.join(ROOT, "clair3_rna_amd")
    exe = str(tmp_path / "phase_alleles_check")
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "phase_alleles_check.c"),
                           "-L", lib, "-lc3r", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "phase_alleles_check: ok" in out.stdout, out.stdout + out.stderr
