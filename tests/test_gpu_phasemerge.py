"""The block-merge stage on the device (c3r_phase_unit_links / k_phase_unit_links, c3r_phase_merge) against tests/phasemergeref.py, the
plain-Python restatement of the rule; that the call leaves scans and haplotags alone; and the drivers (phase_vcf --merge_levels,
call_sample --phasing builtin --phase_merge_levels)."""
import gzip
import os
import random
import re

import numpy as np
import pytest

from tests import hapref
from tests import helpers as H
from tests import phasemergeref as M
from tests import phaseref as P

pytestmark = pytest.mark.gpu

K = P.K
_state = {}

KNOWN_SITES = [11, 12] + list(range(21, 29)) + [41, 42]
KNOWN_READS = [(10, "2M28N2M", "ACCC")] * 3 + [(10, "2M28N2M", "CAAA")] * 2 + [(20, "8M", "AAAAAAAA")]


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
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=r[4] if len(r) > 4 else 60, hp=0) for r in recs])


def _check(eng, rs, table, params=P.DEFAULT_PARAMS):
    """The engine's unit link table for (rs, table) under the engine's current filters equals the restatement's under `params`; returns it."""
    exp = M.unit_links(rs, table, params)
    eng.load_reads(rs)
    got = eng.phase_unit_links(table)
    assert got.shape == (len(M.units_of(table)), K, 2) and got.dtype == np.uint32
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    return exp


def _gen(seed):
    """gen_fragmented(seed, 9), its site link table and the chain's table, computed once."""
    if seed not in _state:
        case = M.gen_fragmented(seed, 9)
        lk = P.links(case[1], case[2])
        _state[seed] = case + (lk, P.resolve(case[2], lk)[0])
    return _state[seed]


def _hand_table(sites, rng, singles=0.25):
    """A hand-set table over `sites`: a quarter of the sites without a block; the others in runs of 1-5 sites, two runs at a time shuffled
    into each other (interleaved units); ps = the pos of the unit's first site; random h1."""
    t = sites.copy()
    t["ps"], t["h1"] = -1, 0
    rest = [j for j in range(len(t)) if rng.random() >= singles]
    k = 0
    while k < len(rest):
        a, b = rng.randint(1, 5), rng.randint(1, 5)
        both = rest[k:k + a + b]
        k += a + b
        first = set(rng.sample(both, min(a, len(both))))
        for group in ([j for j in both if j in first], [j for j in both if j not in first]):
            for j in group:
                t["ps"][j], t["h1"][j] = int(t["pos"][group[0]]), rng.randint(0, 1)
    return t


def _takes_serial_walk(cigar):
    """What csrc/reads_kernels.hpp calls a CIGAR that is not plain: a zero-length op, a pad, a hard clip inside, equal neighbours other than
    M-like ones."""
    ops = [(int(n), o) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    fold = ["M" if o in "=X" else o for _, o in ops]
    return (any(n == 0 or o == "P" for n, o in ops) or any(o == "H" and 0 < k < len(ops) - 1 for k, (_, o) in enumerate(ops))
            or any(fold[k] == fold[k - 1] != "M" for k in range(1, len(ops))))


# ---- 1. Engine.phase_unit_links against phasemergeref.unit_links
def test_known_answer(eng):
    rs = _readset(KNOWN_READS)
    sites = P.make_sites([(p, "A", "C") for p in KNOWN_SITES])
    eng.load_reads(rs)
    chain, _ = eng.phase_sites(sites)
    assert chain["ps"].tolist() == [11, 11] + [-1] * 8 + [41, 41] and chain["h1"].tolist() == [0, 1] + [0] * 8 + [0, 0]
    exp = _check(eng, rs, chain)
    assert exp[1, 0].tolist() == [0, 5] and int(exp.sum()) == 5
    out, st = eng.phase_sites(sites, merge_levels=4)
    assert out["ps"].tolist() == [11, 11] + [-1] * 8 + [11, 11] and out["h1"].tolist() == [0, 1] + [0] * 8 + [1, 1]
    assert st == dict(n_sites=12, n_phased=4, n_blocks=1, max_block=4, merge_levels_run=2, merge_units_joined=1)
    # with four reads that show 11 and 12 in cis those two stay alone: one unit, nothing launched, the chain's values kept
    rs2 = _readset(KNOWN_READS + [(10, "2M28N2M", "AACC")] * 4)
    eng.load_reads(rs2)
    chain2, cst2 = eng.phase_sites(sites)
    assert chain2["ps"].tolist() == [-1] * 10 + [41, 41]
    assert _check(eng, rs2, chain2).shape == (1, K, 2)
    out2, st2 = eng.phase_sites(sites, merge_levels=4)
    assert P.equal_sites(out2, chain2) and st2 == dict(cst2, merge_levels_run=1, merge_units_joined=0)


@pytest.mark.parametrize("seed", range(4))
def test_generated_cases_after_the_chain(eng, seed):
    _, rs, sites, _, editing, _, chain = _gen(seed)
    assert 380 <= len(rs) <= 420 and len(rs) % 16 != 0 and 130 <= len(sites) <= 150 and len(editing) == 18
    exp = _check(eng, rs, chain)
    assert len(exp) >= 2 and int(exp.sum()) > 0


@pytest.mark.parametrize("seed", range(4))
def test_generated_reads_under_hand_set_tables(eng, seed):
    _, rs, sites, _, _, _, _ = _gen(seed)
    rng = random.Random(300 + seed)
    table = _hand_table(sites, rng)
    ps = table["ps"].tolist()
    units = M.units_of(table)
    assert 20 <= ps.count(-1) <= 55 and len(units) >= 25
    # interleaved: some unit has a site of another unit between two of its own
    assert any(ps[j] != ps[j + 1] and ps[j] in ps[j + 2:j + 9] for j in range(len(ps) - 2) if ps[j] >= 0 and ps[j + 1] >= 0)
    exp = _check(eng, rs, table)
    assert int(exp[:, 0].sum()) > 300 and int(exp[:, K - 1].sum()) > 0 and int(exp[:, :, 1].sum()) > 50


def test_more_than_a_hundred_units_on_a_read(eng):
    """600-base reads over a table with a site on every position and a unit every five sites: every read walks its CIGAR once per unit, and
    the units kept from the walks before turn over a dozen times."""
    rng = random.Random(5)
    L = 720
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    alt = ["ACGT"[("ACGT".index(b) + 1 + rng.randrange(3)) % 4] for b in ref]
    table = P.make_sites([(p + 1, ref[p], alt[p]) for p in range(L)])
    table["ps"] = [5 * (p // 5) + 1 for p in range(L)]
    table["h1"] = [rng.randint(0, 1) for _ in range(L)]
    recs = []
    for start, cigar in ((0, "600M"), (3, "600M"), (57, "300M2D298M"), (97, "250=100X250M"), (110, "100M9N500M"), (119, "592M")):
        seq, x, hap = [], start, rng.randint(0, 1)
        for n, op in re.findall(r"(\d+)([MDN=X])", cigar):
            for _ in range(int(n)):
                if op in "M=X":
                    # the read's haplotype as the table's h1 spells it, 30 % of the bases the other allele (ties and flips), 5 % anything
                    a = int(table["h1"][x]) ^ hap ^ (rng.random() < 0.3)
                    seq.append(rng.choice("ACGT") if rng.random() < 0.05 else (alt[x] if a else ref[x]))
                x += 1
        assert x < L
        recs.append((start, cigar, "".join(seq)))
    rs = _readset(recs)
    assert len(M.units_of(table)) == 144
    exp = _check(eng, rs, table)
    assert all(int(exp[:, k].sum()) > 300 for k in range(K))     # (~118 units a read, most of them observed, K links each)
    assert int(exp[:, :, 0].sum()) > 500 and int(exp[:, :, 1].sum()) > 500
    ties = sum(1 for u in range(30, 100) if int(exp[u, 0].sum()) < 6)
    assert ties > 5                                               # (a unit of five sites ties or goes unobserved now and then)


@pytest.mark.parametrize("seed", [4100, 4101, 4102])
def test_reads_that_take_the_serial_walk(eng, seed):
    from clair3_rna_amd.reads import ReadSet
    ref, recs = H._case(seed, phased=False)
    rng = random.Random(9000 + seed)
    covered = set()
    for r in recs:
        covered.update(range(r["pos"] + 1, r["pos"] + H.cigar_ref_len(r["cigar"]) + 1))
    rows = []
    for p in sorted(rng.sample(sorted(covered), min(60, len(covered)))):
        a, b = rng.sample("ACGT", 2)
        rows.append((p, a, b))
    table = _hand_table(P.make_sites(rows), rng, singles=0.1)
    serial = [_takes_serial_walk(r["cigar"]) for r in recs]
    assert sum(serial) >= 5 and sum(serial) < len(recs)
    exp = _check(eng, ReadSet.from_records(recs), table)
    assert int(exp.sum()) > 20
    # ... and the serial reads alone say something
    only = ReadSet.from_records([r for r, s in zip(recs, serial) if s])
    assert int(_check(eng, only, table).sum()) > 0


@pytest.mark.parametrize("cigar", ["8M", "4M0D4M"], ids=["plain_walk", "serial_walk"])
def test_a_query_offset_at_or_beyond_l_seq(eng, cigar):
    """SEQ shorter than the CIGAR claims: two units of two sites each under one 8M op, one read per haplotype pattern, whole (l_seq 8), cut
    so that the second unit's sites lie at (l_seq 5) or beyond (4) the end of SEQ, and cut between the second unit's two sites (6), where
    the nibble left behind the end says the opposite of the site before it: counted, it would tie the unit and take the link away."""
    assert _takes_serial_walk(cigar) == (cigar != "8M")
    table = P.make_sites([(p, "A", "C") for p in (2, 3, 6, 7)])
    table["ps"], table["h1"] = [2, 2, 6, 6], [0, 0, 1, 1]
    patterns = ["AAAAAAAA", "ACCAAAAA", "AAAAACCA", "ACCAACCA"]
    whole, cut, between = [(s, 8) for s in patterns], [(s, n) for n in (5, 4) for s in patterns], [("AAAAAACA", 6), ("AAAAACAA", 6)]

    def rs_of(rows):
        rs = _readset([(0, cigar, s) for s, _ in rows])
        rs.reads["l_seq"][:] = [n for _, n in rows]          # (the nibbles behind the end stay where they are)
        return rs
    # the restatement alone: the whole reads link the two units, the cut ones link nothing
    assert M.unit_links(rs_of(whole), table)[1, 0].tolist() == [2, 2] and int(M.unit_links(rs_of(cut), table).sum()) == 0
    assert M.unit_links(rs_of(between), table)[1, 0].tolist() == [1, 1]
    exp = _check(eng, rs_of(whole + cut + between), table)
    assert exp[1, 0].tolist() == [3, 3] and int(exp.sum()) == 6


def test_one_unit_pair_under_five_thousand_reads(eng):
    rng = random.Random(6)
    recs = [(100, "2M", rng.choice(["AG", "AG", "CT", "CT", "AT", "CG", "NG", "AA"])) for _ in range(5000)]
    table = P.make_sites([(101, "A", "C"), (102, "G", "T")])
    table["ps"], table["h1"] = [101, 102], [0, 1]
    exp = _check(eng, _readset(recs), table)
    assert int(exp[1, 0, 1]) > 2000 and int(exp[1, 0, 0]) > 1000 and int(exp.sum()) < 5000


def test_the_filters_decide_who_votes(eng):
    _, rs, sites, _, _, _, chain = _gen(0)
    exp = M.unit_links(rs, chain)
    eng.load_reads(rs)
    assert np.array_equal(eng.phase_unit_links(chain), exp)
    eng.set_params(min_mq=0, excl_flags=0)                    # the reads already loaded are filtered anew
    loose = dict(min_mq=0, excl_flags=0)
    got = eng.phase_unit_links(chain)
    assert not np.array_equal(got, exp) and np.array_equal(got, M.unit_links(rs, chain, loose))
    eng.set_params(min_mq=5, excl_flags=2316 | 16)            # the reverse strand drops out
    strict = dict(min_mq=5, excl_flags=2316 | 16)
    assert not np.array_equal(_check(eng, rs, chain, strict), exp)


def test_fewer_than_two_units_no_reads_and_sites_outside_every_read(eng):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    _, rs, sites, _, _, _, chain = _gen(0)
    eng.load_reads(rs)
    eng.set_profiling(True)
    try:
        eng.reset_kernel_stats()
        none = eng.phase_unit_links(np.zeros(0, capi.PHASE_SITE_DTYPE))
        assert none.shape == (0, K, 2)
        alone = chain.copy()
        alone["ps"], alone["h1"] = -1, 0
        assert eng.phase_unit_links(alone).shape == (0, K, 2)
        one = chain.copy()
        one["ps"] = int(chain["pos"][0])
        got = eng.phase_unit_links(one)
        assert got.shape == (1, K, 2) and got.sum() == 0
        assert "k_phase_unit_links" not in eng.kernel_stats()
        out, st = eng.phase_sites(None, merge_levels=4)
        assert len(out) == 0 and st == dict(dict.fromkeys(P.STAT_KEYS, 0), merge_levels_run=1, merge_units_joined=0)
        assert "k_phase_unit_links" not in eng.kernel_stats()
        eng.phase_unit_links(chain)
        assert eng.kernel_stats()["k_phase_unit_links"]["launches"] == 1
    finally:
        eng.set_profiling(False)
    # the C entry point: ulinks = NULL asks for the count, too few slots are refused before anything is written
    import ctypes as C
    n_units, U = C.c_int64(-1), len(M.units_of(chain))
    table = np.ascontiguousarray(chain)
    assert eng.L.c3r_phase_unit_links(eng.h, table.ctypes.data_as(C.c_void_p), len(table), None, 0, C.byref(n_units)) == 0 and n_units.value == U
    small = np.full((U - 1, K, 2), 7, np.uint32)
    assert eng.L.c3r_phase_unit_links(eng.h, table.ctypes.data_as(C.c_void_p), len(table), small.ctypes.data_as(C.c_void_p), U - 1, C.byref(n_units)) == -6
    assert (small == 7).all() and n_units.value == U
    far = P.make_sites([(p, "A", "C") for p in (7000, 7001, 7002, 9000, 2000000000)])
    far["ps"], far["h1"] = [7000, 7000, 7002, 7002, 2000000000], [0, 1, 0, 1, 1]
    assert _check(eng, rs, far).sum() == 0 and len(M.units_of(far)) == 3
    before = P.make_sites([(1, "A", "C"), (2, "A", "C"), (3, "A", "C")])
    before["ps"] = [1, 2, 3]
    shifted = ReadSet(rs.reads.copy(), rs.cigar, rs.seq)
    shifted.reads["pos"] += 100
    assert _check(eng, shifted, before).sum() == 0
    eng.load_reads(ReadSet.from_records([]))
    got = eng.phase_unit_links(chain)
    assert got.sum() == 0 and got.shape == (len(M.units_of(chain)), K, 2)


BAD_TABLES = [
    ("unsorted", dict(pos=(2, 15)), 2),
    ("pos_below_1", dict(pos=(0, 0)), 0),
    ("bad_alt_code", dict(alt=(1, 3)), 1),
    ("ref_equals_alt", dict(alt=(3, 1)), 3),
    ("ps_zero", dict(ps=(2, 0)), 2),
    ("ps_below_minus_one", dict(ps=(1, -7)), 1),
    ("h1_above_one", dict(h1=(3, 2)), 3),
]


@pytest.mark.parametrize("name, patch, index", BAD_TABLES, ids=[b[0] for b in BAD_TABLES])
def test_bad_tables_name_the_index(eng, name, patch, index):
    from clair3_rna_amd import capi
    table = P.make_sites([(10, "A", "C"), (20, "A", "C"), (30, "A", "C"), (40, "A", "C")])
    table["ps"], table["h1"] = [10, 10, -1, 40], [0, 0, 0, 1]
    eng.load_reads(_readset([(0, "60M", "A" * 60)] * 2))
    assert eng.phase_unit_links(table)[1, 0].tolist() == [0, 2]
    for k, (j, v) in patch.items():
        table[k][j] = v
    with pytest.raises(capi.C3RError, match="unit site %d:" % index):
        eng.phase_unit_links(table)
    with pytest.raises(ValueError):
        eng.phase_sites(table, merge_levels=-1)


# ---- 2. the call leaves everything else alone
def _scan_bytes(eng, ref):
    n = eng.scan(1, len(ref))
    return n, eng.tensors(rescaled=True).tobytes(), eng.tensors(rescaled=False).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()


@pytest.mark.parametrize("channels", [18, 30])
def test_a_scan_is_the_same_with_and_without_the_call(eng, channels):
    ref, rs, sites, _, _, _, chain = _gen(1)
    tagged = hapref.with_hp(rs, (np.arange(len(rs)) % 3).astype(np.uint8))
    eng.set_params(channels=channels, min_coverage=2)
    eng.load_reads(tagged)
    eng.set_reference(1, ref)
    plain = _scan_bytes(eng, ref)
    assert plain[0] > 20
    eng.load_reads(tagged)
    assert eng.phase_unit_links(chain).sum() > 0
    assert _scan_bytes(eng, ref) == plain
    assert eng.phase_unit_links(chain).sum() > 0              # after the scan: what it left is still there
    assert (eng.tensors(rescaled=True).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()) == (plain[1], plain[3], plain[4])
    assert _scan_bytes(eng, ref) == plain


def test_haplotags_under_a_set_table_are_unchanged(eng):
    _, rs, sites, truth, _, _, chain = _gen(2)
    table = sites.copy()
    table["ps"], table["h1"] = 1000 + np.arange(len(sites)) // 10, truth
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    before = eng.haplotags()
    assert before[1]["n_hp1"] > 50 and before[1]["n_hp2"] > 50
    assert eng.phase_unit_links(chain).sum() > 0              # another table than the one that is set
    merged, _ = eng.phase_sites(sites, merge_levels=4)
    after = eng.haplotags()
    assert after[0].tolist() == before[0].tolist() and after[1] == before[1]
    assert before[0].tolist() == hapref.haplotag(rs, table)[0].tolist()


# ---- 3. the entry points agree
@pytest.mark.parametrize("seed", [0, 3])
def test_phase_sites_with_levels_equals_the_restatement(eng, seed):
    _, rs, sites, _, _, lk, chain = _gen(seed)
    eng.load_reads(rs)
    want, wst = M.phase(rs, sites, lk, 4)
    out, st = eng.phase_sites(sites, merge_levels=4)
    assert P.equal_sites(out, want) and st == wst and st["merge_units_joined"] >= 1 and not P.equal_sites(out, chain)
    out1, st1 = eng.phase_sites(sites, merge_levels=1)
    want1, wst1 = M.phase(rs, sites, lk, 1)
    assert P.equal_sites(out1, want1) and st1 == wst1 and st1["merge_levels_run"] == 1
    outm, stm = eng.phase_sites(sites, 1, 100, merge_levels=4)
    wantm, wstm = M.phase(rs, sites, P.links(rs, sites), 4, min_reads=1, min_agree_pct=100)
    assert P.equal_sites(outm, wantm) and stm == wstm
    # merge_levels = 0 is the phase_sites of before: the chain and its four statistics
    cst = P.resolve(sites, lk)[1]
    for got in (eng.phase_sites(sites), eng.phase_sites(sites, merge_levels=0), eng.phase_sites(sites, 2, 75, 0)):
        assert P.equal_sites(got[0], chain) and got[1] == cst and sorted(got[1]) == sorted(P.STAT_KEYS)


# ---- 4. drivers, on a BAM written from gen_fragmented
@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    from clair3_rna_amd import bam, bamio, io, synth
    tmp = str(tmp_path_factory.mktemp("phasemerge_drivers"))
    ref, rs, sites, _, _, lk, chain = _gen(0)
    fa, w18, w30 = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model18"), os.path.join(tmp, "model30")
    io.write_fasta(fa, [("chr1", ref)])
    np.save(w18 + ".c3rw.npy", synth.random_weights(18, seed=5))
    np.save(w30 + ".c3rw.npy", synth.random_weights(30, seed=5))
    bam_fn = os.path.join(tmp, "plain.bam")
    bam.write_bam(bam_fn, [("chr1", len(ref))], {"chr1": rs})
    bamio.index_build(bam_fn)
    # a pass-1 VCF written by hand: every site of the table a PASS 0/1 row
    vcf = os.path.join(tmp, "pass1.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n" % len(ref))
        for s in sites:
            f.write("chr1\t%d\t.\t%s\t%s\t20\tPASS\t.\tGT:GQ\t0/1:20\n" % (int(s["pos"]), "ACGT"[(1, 2, 4, 8).index(int(s["ref"]))], "ACGT"[(1, 2, 4, 8).index(int(s["alt"]))]))
    return dict(tmp=tmp, fa=fa, w18=w18, w30=w30, bam=bam_fn, vcf=vcf)


def _gz_text(fn):
    with gzip.open(fn, "rt") as f:
        return f.read()


def _phase_vcf(s, out, extra, msgs=None):
    from clair3_rna_amd import phase_vcf
    out_dir = os.path.join(s["tmp"], out)
    log = msgs.append if msgs is not None else (lambda m: None)
    phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", s["bam"], "--vcf_fn", s["vcf"], "--output_dir", out_dir] + list(extra)), log=log)
    return os.path.join(out_dir, "phased_chr1.vcf.gz")


def test_phase_vcf_with_merge_levels_writes_the_file_the_restatement_predicts(sample, tmp_path):
    from clair3_rna_amd import io, phasing
    _, _, sites, _, _, _, _ = _gen(0)
    cands, _ = phasing.candidates_from_vcf(sample["vcf"], "chr1")
    assert P.equal_sites(cands, sites)
    rs = io.load_reads(sample["bam"], "chr1")                 # the voters as the driver sees them
    lk = P.links(rs, cands)
    msgs4, msgs0 = [], []
    got4, got0 = _phase_vcf(sample, "merge4", ["--merge_levels", "4"], msgs4), _phase_vcf(sample, "merge0", ["--merge_levels", "0"], msgs0)
    today = _phase_vcf(sample, "default", [])
    want4, st4 = M.phase(rs, cands, lk, 4)
    want0, _ = P.resolve(cands, lk)
    exp4, exp0 = str(tmp_path / "exp4.vcf.gz"), str(tmp_path / "exp0.vcf.gz")
    phasing.write_phased_vcf(sample["vcf"], "chr1", want4, exp4)
    phasing.write_phased_vcf(sample["vcf"], "chr1", want0, exp0)
    assert _gz_text(got4) == _gz_text(exp4) and _gz_text(got0) == _gz_text(exp0) == _gz_text(today)
    assert _gz_text(got4) != _gz_text(got0) and st4["merge_units_joined"] >= 1
    assert len(msgs4) == 1 and len(msgs0) == 1 and msgs4[0].startswith("[INFO] chr1:")
    assert "block merge: %d units joined in %d levels" % (st4["merge_units_joined"], st4["merge_levels_run"]) in msgs4[0]
    assert "block merge" not in msgs0[0]
    from clair3_rna_amd import phase_vcf
    with pytest.raises(SystemExit) as e:
        phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", sample["vcf"], "--output_dir", str(tmp_path / "neg"), "--merge_levels", "-1"]))
    assert str(e.value.code).startswith("[ERROR]") and "--merge_levels" in str(e.value.code) and not os.path.exists(str(tmp_path / "neg"))


def _argv(s, out, extra):
    return ["--bam_fn", s["bam"], "--ref_fn", s["fa"], "--output_dir", os.path.join(s["tmp"], out), "--pileup_model_path", s["w18"],
            "--chunk_num", "3", "--min_coverage", "2"] + list(extra)


def _call_sample(s, out, extra, compress=False):
    from clair3_rna_amd import call_sample
    assert call_sample.Run(call_sample.build_parser().parse_args(_argv(s, out, extra) + ([] if compress else ["--no_compress"])), log=lambda m: None) == 0


def test_call_sample_with_merge_levels_equals_the_three_steps_by_hand(sample):
    from clair3_rna_amd import phase_vcf
    phased = ["--phased_pileup_model_path", sample["w30"], "--enable_phasing_model"]
    _call_sample(sample, "hand", [])
    pass1 = os.path.join(sample["tmp"], "hand", "output.vcf")
    phased_dir = os.path.join(sample["tmp"], "hand", "tmp", "phased_output", "phased_vcf")
    phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", pass1, "--output_dir", phased_dir, "--merge_levels", "4"]), log=lambda m: None)
    _call_sample(sample, "hand", phased + ["--phased_vcf_fn", phased_dir])
    hand1, hand2 = open(pass1).read(), open(os.path.join(sample["tmp"], "hand", "output_enable_phasing.vcf")).read()
    _call_sample(sample, "builtin", phased + ["--phasing", "builtin", "--phase_merge_levels", "4"])
    out = os.path.join(sample["tmp"], "builtin")
    assert open(os.path.join(out, "output.vcf")).read() == hand1
    assert open(os.path.join(out, "output_enable_phasing.vcf")).read() == hand2
    a, b = (os.path.join(d, "phased_chr1.vcf.gz") for d in (phased_dir, os.path.join(out, "tmp", "phased_output", "phased_vcf")))
    assert os.path.exists(a) == os.path.exists(b) and (not os.path.exists(a) or _gz_text(a) == _gz_text(b))


def test_the_flag_is_refused_where_it_means_nothing(sample):
    from clair3_rna_amd import call_sample

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:
            call_sample.Run(call_sample.build_parser().parse_args(_argv(sample, "refused", extra)))
        assert str(e.value.code).startswith("[ERROR]") and all(w in str(e.value.code) for w in words), e.value.code

    refused(["--phase_merge_levels", "4"], "--phase_merge_levels", "--phasing builtin")
    refused(["--phase_merge_levels", "4", "--phased_pileup_model_path", sample["w30"], "--enable_phasing_model", "--phased_vcf_fn", sample["vcf"]],
            "--phase_merge_levels", "--phasing builtin")
    refused(["--phasing", "builtin", "--phased_pileup_model_path", sample["w30"], "--enable_phasing_model", "--phase_merge_levels", "-2"], "--phase_merge_levels")
    assert not os.path.exists(os.path.join(sample["tmp"], "refused"))
