"""Allele realignment on the device (c3r_set_hap_realign: k_haplotag_alleles_ra, k_hap_allele_counts_ra, k_phase_allele_links_ra,
k_phase_allele_unit_links_ra) against tests/realignref.py, the plain-Python restatement: the seeded fuzz through both walks, the hand cases,
the invariance the feature stands for — where inside the window the CIGAR places its indels does not matter —, the fallbacks, the
composition with the base-quality threshold, the scans that must not move, and the switch's life cycle."""
import numpy as np
import pytest

from tests import hapalleleref as HA
from tests import leftalignref as LA
from tests import phaseref as P
from tests import qualref as QR
from tests import realignref as RR

pytestmark = pytest.mark.gpu

FUZZ_SEED = 1
_state = {}


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clean(request):
    """Every test of this module starts and leaves its engine with the switches off, without a phase table and with default parameters."""
    yield
    if "eng" in request.fixturenames:
        from clair3_rna_amd import capi
        e = request.getfixturevalue("eng")
        e.set_phase_sites(None)
        e.set_hap_realign(0)
        e.set_hap_left_align(False)
        e.set_hap_min_bq(0)
        e.params = capi.default_params()
        e.set_params()


def _units(table):
    """Units of three table sites, every seventh site in none, oriented by the sites' h1."""
    return [-1 if j % 7 == 5 else 1 + j // 3 for j in range(len(table))], [s["h1"] for s in table]


def _memo(obs):
    """An observation computed once per read (the four tables of the restatement each ask for it)."""
    seen = {}

    def once(rs, i, site_at):
        if i not in seen:
            seen[i] = obs(rs, i, site_at)
        return seen[i]
    return once


def _expected(rs, table, obs):
    obs = _memo(obs)
    hp, st, ps = LA.haplotag(rs, table, obs)
    ups, uh1 = _units(table)
    return dict(hp=hp, st=st, ps=ps, counts=LA.allele_counts(rs, hp, ps, table, obs), links=LA.links(rs, table, obs),
                ulinks=LA.unit_links(rs, table, ups, uh1, obs))


def _device(eng, rs, table, ref, W, load=True):
    """The engine's four tables under overhang W; ref = (first 0-based position, letters)."""
    q, pool = HA.to_query(table)
    h1 = np.array([s["h1"] for s in table], np.uint8)
    eng.set_reference(ref[0] + 1, ref[1])
    eng.set_hap_realign(W)
    if load:
        eng.load_reads(rs)
    eng.set_phase_alleles(q, h1, pool)
    hp, st = eng.haplotags()
    ups, uh1 = _units(table)
    qu = q.copy()
    qu["ps"] = ups
    return dict(hp=hp, st=st, ps=eng.read_phase_sets(), counts=eng.hap_allele_counts(q, pool), links=eng.phase_allele_links(q, pool),
                ulinks=eng.phase_allele_unit_links(qu, np.array(uh1, np.uint8), pool))


def _assert_same(got, exp):
    assert np.array_equal(got["hp"], exp["hp"]), np.argwhere(got["hp"] != exp["hp"])[:10]
    assert np.array_equal(got["ps"], exp["ps"]) and got["st"] == exp["st"]
    for key in ("counts", "links", "ulinks"):
        assert got[key].shape == exp[key].shape and np.array_equal(got[key], exp[key]), (key, np.argwhere(got[key] != exp[key])[:10])


def _differ(a, b):
    return not np.array_equal(a["counts"], b["counts"]) and not np.array_equal(a["links"], b["links"])


def _fuzz():
    if "fuzz" not in _state:
        _state["fuzz"] = RR.gen_fuzz(FUZZ_SEED, quals=True)
    return _state["fuzz"]


def _no_quals(rs):
    from clair3_rna_amd.reads import ReadSet
    return ReadSet(rs.reads, rs.cigar, rs.seq)


# ---- 1. the fuzz of the CPU test, through both walks, for each of the four entry points
@pytest.mark.parametrize("W", [1, 10, 16])
def test_fuzz_against_the_restatement(eng, W):
    ref, table, rs = _fuzz()
    cig = lambda r: [int(c) & 15 for c in rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]]
    kinds = [cig(r) for r in rs.reads]
    assert sum(1 for k in kinds if 7 in k or 8 in k) >= 40 and sum(1 for k in kinds if 6 in k) >= 40 and sum(1 for k in kinds if set(k) <= {0, 1, 2, 4}) >= 80
    exp = _expected(rs, table, RR.observer(ref, W))
    assert int(exp["counts"][:, 1:, :2].sum()) > 500 and int(exp["links"].sum()) > 5000 and len(exp["ulinks"]) >= 6 and int(exp["ulinks"].sum()) > 500
    got = _device(eng, _no_quals(rs), table, ref, W)
    _assert_same(got, exp)
    if W == 10:                                              # and the switch is what does it
        off = _device(eng, _no_quals(rs), table, ref, 0)
        _assert_same(off, _expected(rs, table, HA.observe))
        assert _differ(got, off)


# ---- 2. the hand cases of tests/test_realign_ref.py: one read, its column from the count table
def _column(eng, site):
    """The column of the ONE loaded read at one site (3: no observation), from the count table."""
    q, pool = HA.to_query([site])
    q["ps"] = 7
    counts = eng.hap_allele_counts(q, pool)
    assert int(counts.sum()) <= 1
    return int(np.argmax(counts[0].sum(axis=0))) if counts.sum() else 3          # (whatever the read's tag: all rows of the site)


def _load_one(eng, ref, rs, W):
    eng.set_reference(ref[0] + 1, ref[1])
    eng.set_hap_realign(W)
    eng.load_reads(rs)
    far = np.zeros(1, dtype=HA.to_query([])[0].dtype)        # a table must be set for the counts: one far SNV that the read does not reach
    far[0]["pos"], far[0]["base_matters"], far[0]["a_base"], far[0]["b_base"] = 5000, 1, 1, 2
    eng.set_phase_alleles(far, np.zeros(1, np.uint8))


@pytest.mark.parametrize("case", RR.HAND, ids=[c[0] for c in RR.HAND])
def test_hand_made_reads(eng, case):
    _, ref, row, W, read, want, want_off = case
    rs, site = RR.one_read(read), RR.site_of(row)
    _load_one(eng, ref, rs, W)
    assert _column(eng, site) == want[0]
    # the other three entry points on the same read — links, unit links and the tag — from a table of this site and a clean SNV before
    # it, whichever slice the case sets: fallbacks included
    table = [dict(RR.site_of((8, "G", "A", "0/1")), h1=0, ps=7), dict(site, h1=1, ps=7)]
    q, pool = HA.to_query(table)
    obs = RR.observer(ref, W)
    assert np.array_equal(eng.phase_allele_links(q, pool), LA.links(rs, table, obs))
    qu = q.copy()
    qu["ps"] = [1, 50]
    assert np.array_equal(eng.phase_allele_unit_links(qu, np.array([0, 1], np.uint8), pool), LA.unit_links(rs, table, [1, 50], [0, 1], obs))
    eng.set_phase_alleles(q, np.array([0, 1], np.uint8), pool)
    hp, st, ps = LA.haplotag(rs, table, obs)
    assert np.array_equal(eng.haplotags()[0], hp) and eng.haplotags()[1] == st and np.array_equal(eng.read_phase_sets(), ps)
    if not want[1]:                                          # a fallback: the three equal the switch-off results too
        assert np.array_equal(LA.links(rs, table, obs), LA.links(rs, table, HA.observe)) and np.array_equal(hp, LA.haplotag(rs, table, HA.observe)[0])
    # switched off, and as a fallback, the column is the one of today's rule
    eng.set_hap_realign(0)
    assert _column(eng, site) == want_off
    if not want[1]:
        assert want[0] == want_off


def test_the_two_limits_of_64_on_the_device(eng):
    p0, W, ref = 60, 16, (0, RR.LONG)
    ins11, ins12 = "GATTACAGATT", "GATTACAGATTA"
    dele = RR.LONG[p0:p0 + 21]
    fits = RR.site_of((p0 + 1, dele, RR.LONG[p0] + ins11 + dele[1:] + "," + RR.LONG[p0], "1/2"))
    over = RR.site_of((p0 + 1, dele, RR.LONG[p0] + ins12 + dele[1:] + "," + RR.LONG[p0], "1/2"))
    # m = 64 (realigned), m = 65 (the CIGAR's column), 2W + 1 + D + I = 65 (never realigned) and 63: the read shows the insertion, allele A
    for site, read, w in ((fits, RR.long_read(p0, ins11), W), (fits, RR.long_read(p0, ins11, extra_at=70), W), (over, RR.long_read(p0, ins12), W), (over, RR.long_read(p0, ins12), W - 1)):
        rs = RR.one_read(read)
        _load_one(eng, ref, rs, w)
        assert _column(eng, site) == RR.column_of(rs, 0, site, ref, w)[0] == 0


# ---- 3. the invariance the feature stands for
#   a homopolymer (CAAAAAG on 40 .. 46: one A deleted), a 2-base repeat (GACACACT on 80 .. 87: AC inserted) and an SNV on 120 whose ALT the
#   aligner may write as 1D1M1I or 1I1M1D; clean SNVs on 20 and 145.  Every read spans [5, 160).
def _inv_ref():
    text = list("".join("ACGT"[(k * 7 + k // 4 + k // 16) % 4] for k in range(170)))
    text[40:47] = "CAAAAAG"
    text[80:88] = "GACACACT"
    return "".join(text)


INV_REF = _inv_ref()
INV_ROWS = [(21, INV_REF[20], "ACGT"[("ACGT".index(INV_REF[20]) + 1) % 4], "0/1"), (41, "CA", "C", "0/1"), (81, "G", "GAC", "0/1"),
            (121, INV_REF[120], "ACGT"[("ACGT".index(INV_REF[120]) + 2) % 4], "0/1"), (146, INV_REF[145], "ACGT"[("ACGT".index(INV_REF[145]) + 1) % 4], "0/1")]


def _inv_read(k_del, k_ins, form):
    """A read of the ALT haplotype with its deleted A written k_del places right of the left-most one, its inserted AC k_ins places right,
    and the SNV on 120 written plainly (0), as 1D1M1I (1) or as 1I1M1D (2).  The sequence is the same for all."""
    r = INV_REF
    seq = r[5:20] + INV_ROWS[0][2] + r[21:41] + r[42:81] + "AC" + r[81:120] + INV_ROWS[3][2] + r[121:145] + INV_ROWS[4][2] + r[146:160]
    ops = [("M", 40 + k_del - 5 + 1), ("D", 1), ("M", 80 + k_ins - (42 + k_del) + 1), ("I", 2)]
    if form == 0:
        ops += [("M", 160 - (81 + k_ins))]
    elif form == 1:
        ops += [("M", 119 - (81 + k_ins)), ("D", 1), ("M", 1), ("I", 1), ("M", 160 - 121)]
    else:
        ops += [("M", 120 - (81 + k_ins)), ("I", 1), ("M", 1), ("D", 1), ("M", 160 - 122)]
    assert sum(n for op, n in ops if op in "MI") == len(seq) and sum(n for op, n in ops if op in "MD") == 155
    return dict(pos=5, cigar="".join("%d%s" % (n, op) for op, n in ops), seq=seq, flag=0, mapq=60, hp=0)


def _inv_sets():
    from clair3_rna_amd.reads import ReadSet
    ref_read = dict(pos=5, cigar="155M", seq=INV_REF[5:160], flag=0, mapq=60, hp=0)
    placed = [_inv_read(i % 5, i % 7, i % 3) for i in range(35)]
    assert {(i % 5) for i in range(35)} == set(range(5)) and len({r["cigar"] for r in placed}) == 35
    clean = [_inv_read(0, 0, 0) for _ in range(35)]
    return ReadSet.from_records(placed + [ref_read] * 30), ReadSet.from_records(clean + [ref_read] * 30)


def _inv_table():
    return [dict(RR.site_of(row), h1=j % 2, ps=21) for j, row in enumerate(INV_ROWS)]


def test_placement_inside_the_window_does_not_matter(eng):
    table = _inv_table()
    ref, W = (0, INV_REF), 10
    placed, clean = _inv_sets()
    on_placed, on_clean = _device(eng, placed, table, ref, W), _device(eng, clean, table, ref, W)
    _assert_same(on_placed, on_clean)
    _assert_same(on_placed, _expected(placed, table, RR.observer(ref, W)))
    # error-free reads with left-most indels: exactly the switch-off results
    off_clean = _device(eng, clean, table, ref, 0)
    _assert_same(on_clean, off_clean)
    _assert_same(off_clean, _expected(clean, table, HA.observe))
    # and each placement set differs from its run with the switch off
    off_placed = _device(eng, placed, table, ref, 0)
    assert _differ(on_placed, off_placed) and not np.array_equal(on_placed["hp"], off_placed["hp"])
    _assert_same(off_placed, _expected(placed, table, HA.observe))
    assert int(on_placed["counts"][1:4, :, 1].sum()) == 3 * 35 and int(off_placed["counts"][1:4, :, 1].sum()) == 7 + 5 + 12
    # the three kinds one at a time: only the deletion moves, only the insertion, only the SNV's spelling
    from clair3_rna_amd.reads import ReadSet
    for name, reads in (("homopolymer", [_inv_read(k, 0, 0) for k in range(5)]), ("2-base repeat", [_inv_read(0, k, 0) for k in range(7)]),
                        ("1D1I", [_inv_read(0, 0, f) for f in range(3)])):
        rs, base = ReadSet.from_records(reads), ReadSet.from_records([_inv_read(0, 0, 0)] * len(reads))
        on = _device(eng, rs, table, ref, W)
        _assert_same(on, _device(eng, base, table, ref, W))
        assert _differ(on, _device(eng, rs, table, ref, 0)), name


# ---- 4. composition with the base-quality threshold: (qualities, Q) equals Q = 0 on the reads with N, with the switch on
@pytest.mark.parametrize("Q", [10, 25])
def test_composition_with_hap_min_bq(eng, Q):
    ref, table, rs = _fuzz()
    W = 10
    eng.load_reads(rs)                                       # (the threshold is refused while reads without qualities are loaded)
    eng.set_hap_min_bq(Q)
    got = _device(eng, rs, table, ref, W)
    assert eng.hap_min_bq() == (Q, QR.mask(rs, Q)[1]) and eng.hap_realign() == W
    eng.set_hap_min_bq(0)
    with_n = QR.with_n(rs, Q)
    exp = _device(eng, with_n, table, ref, W)
    _assert_same(got, exp)
    assert _differ(got, _device(eng, _no_quals(rs), table, ref, W))
    if Q == 10:
        _assert_same(got, _expected(with_n, table, RR.observer(ref, W)))


# ---- 5. what must not move: the 18- and 30-channel scans
def test_the_scans_never_see_the_switch(eng):
    from tests import hapref
    ref, table, rs = (0, INV_REF), _inv_table(), _inv_sets()[0]              # (the placed reads: their tags move with the switch)
    q, pool = HA.to_query(table)
    h1 = np.array([s["h1"] for s in table], np.uint8)

    def scan(channels, W, reads=rs, tagged=True):
        eng.set_params(channels=channels, min_coverage=2)
        eng.set_reference(1, ref[1])
        eng.set_hap_realign(W)
        if tagged:
            eng.set_phase_alleles(q, h1, pool)
        else:
            eng.set_phase_sites(None)
        eng.load_reads(reads)
        n = eng.scan(1, len(ref[1]))
        return n, eng.sites().tobytes(), eng.tokens().tobytes(), eng.tensors(rescaled=False).tobytes()
    off = scan(18, 0)
    assert off[0] >= 3 and scan(18, 10) == off
    # 30 channels: the scan under (table, W) is the scan without a table of the same reads carrying the W run's tags
    with_table = scan(30, 10)
    tags = eng.haplotags()[0].copy()
    eng.set_hap_realign(0)
    assert not np.array_equal(eng.haplotags()[0], tags) and set(tags.tolist()) >= {1, 2}
    assert scan(30, 0, hapref.with_hp(rs, tags), tagged=False) == with_table


# ---- 6. the life cycle of the switch
def test_life_cycle():
    from clair3_rna_amd import capi
    ref, table, rs = (0, INV_REF), _inv_table(), _inv_sets()[0]              # (the placed reads: their tags move with the switch)
    q, pool = HA.to_query(table)
    h1 = np.array([s["h1"] for s in table], np.uint8)
    ups, uh1 = _units(table)
    qu = q.copy()
    qu["ps"] = ups
    on_tags, _, on_ps = LA.haplotag(rs, table, _memo(RR.observer(ref, 10)))
    e = capi.Engine(0)
    try:
        assert e.hap_realign() == 0
        for bad in (17, -1, 64):
            with pytest.raises(capi.C3RError) as err:
                e.set_hap_realign(bad)
            assert err.value.code == -1 and "outside 0 .. 16" in str(err.value) and e.hap_realign() == 0
        # no reference: the switch itself is accepted, the four calls are refused, and nothing is lost by the refusals
        e.load_reads(rs)
        e.set_hap_realign(10)
        for call in (lambda: e.set_phase_alleles(q, h1, pool), lambda: e.phase_allele_links(q, pool),
                     lambda: e.phase_allele_unit_links(qu, np.array(uh1, np.uint8), pool)):
            with pytest.raises(capi.C3RError) as err:
                call()
            assert err.value.code == -1 and "no reference is set" in str(err.value)
        e.set_phase_alleles(None, None)                      # n = 0 still clears
        e.set_hap_realign(0)
        e.set_phase_alleles(q, h1, pool)
        off_tags = e.haplotags()[0].copy()
        with pytest.raises(capi.C3RError) as err:            # a table and reads are there: the toggle would tag again
            e.set_hap_realign(10)
        assert err.value.code == -1 and e.hap_realign() == 0 and np.array_equal(e.haplotags()[0], off_tags)
        # with a reference the toggle tags again, both ways, and so does a change of the overhang
        e.set_reference(1, ref[1])
        e.set_hap_realign(10)
        assert np.array_equal(e.haplotags()[0], on_tags) and np.array_equal(e.read_phase_sets(), on_ps) and not np.array_equal(off_tags, on_tags)
        e.set_hap_realign(1)
        assert np.array_equal(e.haplotags()[0], LA.haplotag(rs, table, _memo(RR.observer(ref, 1)))[0])
        e.set_hap_realign(0)
        assert np.array_equal(e.haplotags()[0], off_tags)
        # the exclusion, in both orders; a refused call changes nothing
        e.set_hap_realign(10)
        with pytest.raises(capi.C3RError) as err:
            e.set_hap_left_align(True)
        assert err.value.code == -1 and "exclude each other" in str(err.value) and np.array_equal(e.haplotags()[0], on_tags)
        e.set_hap_realign(0)
        e.set_hap_left_align(True)
        left_tags = e.haplotags()[0].copy()
        with pytest.raises(capi.C3RError) as err:
            e.set_hap_realign(10)
        assert err.value.code == -1 and "exclude each other" in str(err.value) and e.hap_realign() == 0 and np.array_equal(e.haplotags()[0], left_tags)
        e.set_hap_left_align(False)
        e.set_hap_realign(10)
        # a load under the switch tags with it; a later set_reference does not tag again
        e.load_reads(rs)
        assert np.array_equal(e.haplotags()[0], on_tags)
        e.set_reference(1, "N" * len(ref[1]))
        assert np.array_equal(e.haplotags()[0], on_tags)
        e.set_reference(1, ref[1])
        # the SNV table of set_phase_sites never looks at the switch
        snv = P.make_sites([(s["pos"], s["ref"], s["alt"]) for s in table if s["A"][1] == HA.NONE and s["B"][1] == HA.NONE and "," not in s["alt"]])
        snv["ps"] = 0
        e.set_phase_sites(snv)
        snv_tags = e.haplotags()[0].copy()
        e.set_hap_realign(0)
        assert np.array_equal(e.haplotags()[0], snv_tags)
    finally:
        e.close()


def test_kernels_by_name(eng):
    """Switched on, each call launches its _ra kernel once and neither of its siblings — and switched off, the plain one alone."""
    ref, table, rs = _fuzz()
    eng.set_profiling(True)
    try:
        for W, want in ((10, "_ra"), (0, "")):
            eng.reset_kernel_stats()
            _device(eng, _no_quals(rs), table, ref, W)
            stats = eng.kernel_stats()
            for k in ("k_haplotag_alleles", "k_hap_allele_counts", "k_phase_allele_links", "k_phase_allele_unit_links"):
                assert stats[k + want]["launches"] >= 1, (W, k, sorted(stats))
                assert not [s for s in ("", "_la", "_ra") if s != want and k + s in stats], (W, k, sorted(stats))
    finally:
        eng.set_profiling(False)


# ---- 7. the drivers that carry the flag: one tiny BAM (the placed reads of the invariance) through phase_vcf and haplotag_bam
HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
PS_LINE = '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set identifier">\n'


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    import os
    from clair3_rna_amd import bam, bamio, io
    tmp = str(tmp_path_factory.mktemp("realign_drivers"))
    rs = _inv_sets()[0]
    rows = ["chr1\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:GQ\t%s:30\n" % r for r in INV_ROWS]
    fa, bam_fn, vcf = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "plain.bam"), os.path.join(tmp, "calls.vcf")
    io.write_fasta(fa, [("chr1", INV_REF)])
    bam.write_bam(bam_fn, [("chr1", len(INV_REF))], {"chr1": rs})
    bamio.index_build(bam_fn)
    with open(vcf, "w") as f:
        f.write(HEAD + "".join(rows))
    return dict(tmp=tmp, fa=fa, bam=bam_fn, vcf=vcf, rows=rows, rs=rs)


def _gz(fn):
    import gzip
    with gzip.open(fn, "rt") as f:
        return f.read()


def _phase_vcf(sample, out_dir, extra):
    from clair3_rna_amd import phase_vcf
    argv = ["--bam_fn", sample["bam"], "--vcf_fn", sample["vcf"], "--output_dir", out_dir] + extra
    assert len(phase_vcf.Run(phase_vcf.build_parser().parse_args(argv), log=lambda m: None)) == 1
    import os
    return _gz(os.path.join(out_dir, "phased_chr1.vcf.gz"))


def _predicted_vcf(sample, cands, obs):
    from tests import phaseindelref as PI
    ps, h1, _ = PI.resolve(cands, LA.links(sample["rs"], cands, _memo(obs)))
    keep = {c["pos"]: (p, h) for c, p, h in zip(cands, ps, h1)}
    by_pos = {c["pos"]: c for c in cands}
    out = HEAD.replace("#CHROM", PS_LINE + "#CHROM")
    for ln in sample["rows"]:
        pos = int(ln.split("\t")[1])
        out += HA.rewritten(ln, by_pos[pos], keep[pos]) if pos in keep and keep[pos][0] >= 0 else ln
    return out


def test_phase_vcf_with_and_without_the_flag(sample, tmp_path):
    ref = (0, INV_REF)
    cands, skipped = HA.candidates(sample["rows"], "chr1")
    assert len(cands) == 5 and not any(skipped.values())
    snvs = [c for c in cands if HA.flags(c) == (True, False)]
    ra = ["--hap_realign", "--ref_fn", sample["fa"]]
    got = {name: _phase_vcf(sample, str(tmp_path / name), extra) for name, extra in
           (("indels", ["--indels"]), ("indels_ra", ["--indels"] + ra), ("snv", []), ("snv_ra", ra))}
    assert got["indels"] == _predicted_vcf(sample, cands, HA.observe) and got["snv"] == _predicted_vcf(sample, snvs, HA.observe)
    assert got["indels_ra"] == _predicted_vcf(sample, cands, RR.observer(ref, 10)) and got["snv_ra"] == _predicted_vcf(sample, snvs, RR.observer(ref, 10))
    assert got["indels_ra"] != got["indels"]
    assert sum("|" in l.split("\t")[9] for l in got["indels_ra"].splitlines() if not l.startswith("#")) == 5


@pytest.mark.parametrize("tag_indels", [True, False], ids=["haplotag_indels", "snv_table"])
def test_haplotag_bam_with_and_without_the_flag(sample, tmp_path, tag_indels):
    import os
    from clair3_rna_amd import haplotag_bam, io
    ref = (0, INV_REF)
    phased_dir = str(tmp_path / "phased_vcf")
    text = _phase_vcf(sample, phased_dir, ["--indels", "--hap_realign", "--ref_fn", sample["fa"]])
    sites = []
    for f in (l.split("\t") for l in text.splitlines() if not l.startswith("#")):
        gt, ps = f[9].split(":")[0], f[9].split(":")[-1]
        if "|" in gt:
            sites.append(dict(HA.site_of_row(int(f[1]), f[3], f[4], gt.replace("|", "/"), int(ps)), h1=1 if gt in ("1|0", "2|1") else 0))
    if not tag_indels:
        sites = [s for s in sites if HA.flags(s) == (True, False)]
    assert len(sites) == (5 if tag_indels else 3)
    hp = {}
    for flag in (True, False):
        out_dir = str(tmp_path / ("bam_%d" % flag))
        argv = ["--bam_fn", sample["bam"], "--phased_vcf_fn", phased_dir, "--output_dir", out_dir] + (["--haplotag_indels"] if tag_indels else []) + (
            ["--hap_realign", "10", "--ref_fn", sample["fa"]] if flag else [])
        haplotag_bam.Run(haplotag_bam.build_parser().parse_args(argv), log=lambda m: None)
        hp[flag] = io.load_reads(os.path.join(out_dir, "chr1.bam"), "chr1").reads["hp"].copy()
    assert np.array_equal(hp[True], LA.haplotag(sample["rs"], sites, _memo(RR.observer(ref, 10)))[0])
    assert np.array_equal(hp[False], LA.haplotag(sample["rs"], sites, HA.observe)[0])
    assert int((hp[True] != 0).sum()) == len(sample["rs"])
    if tag_indels:                                           # (the clean SNVs alone decide every tag alike)
        assert not np.array_equal(hp[True], hp[False])


def _hap_vcf(sample, bam, phased_dir, out, extra):
    from clair3_rna_amd import hap_vcf
    argv = ["--bam_fn", bam, "--vcf_fn", sample["vcf"], "--phased_vcf_fn", phased_dir, "--output_fn", out + ".vcf", "--hap_counts_fn", out + ".tsv", "--min_mq", "5"] + extra
    hap_vcf.Run(hap_vcf.build_parser().parse_args(argv), log=lambda m: None)
    return open(out + ".vcf").read(), open(out + ".tsv").read()


@pytest.mark.parametrize("indels", [True, False], ids=["indels", "snv_table"])
def test_hap_vcf_with_and_without_the_flag(sample, tmp_path, indels):
    """The placed reads under the flag give the files that the cleanly written reads give without it (whose device results the invariance
    test holds to the restatement), and other files without the flag."""
    import os
    from clair3_rna_amd import bam, bamio
    clean_bam = str(tmp_path / "clean.bam")
    bam.write_bam(clean_bam, [("chr1", len(INV_REF))], {"chr1": _inv_sets()[1]})
    bamio.index_build(clean_bam)
    phased_dir = str(tmp_path / "phased_vcf")
    _phase_vcf(sample, phased_dir, ["--indels", "--hap_realign", "--ref_fn", sample["fa"]])
    kind = ["--indels", "--haplotag_indels"] if indels else []
    ra = ["--hap_realign", "10", "--ref_fn", sample["fa"]]
    on_placed = _hap_vcf(sample, sample["bam"], phased_dir, str(tmp_path / "on_placed"), kind + ra)
    off_clean = _hap_vcf(sample, clean_bam, phased_dir, str(tmp_path / "off_clean"), kind)
    on_clean = _hap_vcf(sample, clean_bam, phased_dir, str(tmp_path / "on_clean"), kind + ra)
    off_placed = _hap_vcf(sample, sample["bam"], phased_dir, str(tmp_path / "off_placed"), kind)
    assert on_placed == off_clean == on_clean
    assert on_placed[1].count("\n") == 1 + (5 if indels else 3) and sum("|" in l.split("\t")[9] for l in on_placed[0].splitlines() if not l.startswith("#")) >= 3
    assert off_placed[1] != on_placed[1]                     # (also on the SNV table: the SNV on 121 is written 1D1M1I / 1I1M1D in two reads of three)


@pytest.fixture(scope="module")
def big_sample(tmp_path_factory):
    """The sample of tests/test_gpu_left_align.py (6 kb, 403 reads, SNVs and indels at random equivalent placements in repeats) and its
    unphased pass: enough heterozygous calls for the built-in phasing to phase."""
    import os
    from tests import test_gpu_left_align as GL
    tmp = str(tmp_path_factory.mktemp("realign_call_sample"))
    s = GL.write_sample(tmp)
    GL._call_sample(s, "pass1", [])
    s["pass1"] = os.path.join(tmp, "pass1", "output.vcf.gz")
    return s


def test_call_sample_builtin_with_the_flag_equals_the_steps_by_hand(big_sample):
    """call_sample --phasing builtin --phasing_indels --hap_realign in one command writes what the steps write one by one under the flag;
    the unphased pass never gets the flag."""
    import os
    from clair3_rna_amd import hap_vcf, haplotag_bam, io, phase_vcf
    from tests.test_gpu_left_align import _call_sample as run
    s = big_sample
    ra = ["--hap_realign", "10", "--ref_fn", s["fa"]]
    flags = ["--enable_phasing_model", "--phasing", "builtin", "--phasing_indels", "--phase_output", "--phase_indels", "--haplotagged_bam"]
    run(s, "one", flags + ["--hap_realign"])
    run(s, "plain", flags)
    one, plain, hand = (os.path.join(s["tmp"], d) for d in ("one", "plain", "hand"))
    assert _gz(os.path.join(one, "output.vcf.gz")) == _gz(s["pass1"]) == _gz(os.path.join(plain, "output.vcf.gz"))
    hand_dir = os.path.join(hand, "phased_vcf")
    phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", s["bam"], "--vcf_fn", s["pass1"], "--output_dir", hand_dir, "--indels"] + ra), log=lambda m: None)
    assert _gz(os.path.join(one, "tmp", "phased_output", "phased_vcf", "phased_chr1.vcf.gz")) == _gz(os.path.join(hand_dir, "phased_chr1.vcf.gz"))
    run(s, "hand", ["--enable_phasing_model", "--phased_vcf_fn", hand_dir, "--haplotag_indels", "--hap_realign"])
    stem = os.path.join(hand, "output_enable_phasing")
    hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", s["bam"], "--vcf_fn", stem + ".vcf.gz", "--phased_vcf_fn", hand_dir, "--output_fn", stem + "_phased.vcf.gz",
                                                   "--hap_counts_fn", stem + "_hap_counts.tsv", "--min_mq", "5", "--indels", "--haplotag_indels"] + ra), log=lambda m: None)
    for fn in ("output_enable_phasing.vcf.gz", "output_enable_phasing_phased.vcf.gz", "output_enable_phasing_hap_counts.tsv"):
        assert open(os.path.join(one, fn), "rb").read() == open(os.path.join(hand, fn), "rb").read(), fn
    bam_dir = os.path.join(hand, "tmp", "phased_output", "phased_bam")
    haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", hand_dir, "--output_dir", bam_dir, "--haplotag_indels", "--ctg_name", "chr1"] + ra),
                     log=lambda m: None)
    tags = lambda d: io.load_reads(os.path.join(d, "tmp", "phased_output", "phased_bam", "chr1.bam"), "chr1").reads
    a, b = tags(one), io.load_reads(os.path.join(bam_dir, "chr1.bam"), "chr1").reads
    assert a.tobytes() == b.tobytes() and int((a["hp"] != 0).sum()) > 100
    # (that the flag changes results is shown step by step: phase_vcf, hap_vcf, haplotag_bam and call_var_bam differ with it; this sample's
    # random-weight network calls one heterozygous row in the final VCF, whose counts do not move)


def test_call_var_bam_tags_with_the_realigned_observation(sample, tmp_path):
    """The per-chunk driver under the flag: the whole contig as the slice, the switch on the engine, and the tags its pass used are the
    restatement's for the phased table; without the flag the engine is never switched."""
    import os
    from clair3_rna_amd import call_var_bam, capi, synth
    ref = (0, INV_REF)
    phased_dir = str(tmp_path / "phased_vcf")
    text = _phase_vcf(sample, phased_dir, ["--indels", "--hap_realign", "--ref_fn", sample["fa"]])
    sites = []
    for f in (l.split("\t") for l in text.splitlines() if not l.startswith("#")):
        gt, ps = f[9].split(":")[0], f[9].split(":")[-1]
        if "|" in gt:
            sites.append(dict(HA.site_of_row(int(f[1]), f[3], f[4], gt.replace("|", "/"), int(ps)), h1=1 if gt in ("1|0", "2|1") else 0))
    w30 = str(tmp_path / "model30")
    np.save(w30 + ".c3rw.npy", synth.random_weights(30, seed=5))
    tags = {}
    for flag in (True, False):
        e = capi.Engine(0)
        try:
            argv = ["--chkpnt_fn", w30, "--bam_fn", sample["bam"], "--ref_fn", sample["fa"], "--call_fn", str(tmp_path / ("chunk_%d.vcf" % flag)), "--ctgName", "chr1", "--pileup",
                    "--chunk_id", "1", "--chunk_num", "1", "--minCoverage", "2", "--enable_phasing_model", "True", "--phased_vcf_fn", phased_dir, "--haplotag_indels"] + (
                        ["--hap_realign"] if flag else [])
            call_var_bam.Run(call_var_bam.build_parser().parse_args(argv), engine=e)
            assert e.hap_realign() == (10 if flag else 0)
            tags[flag] = e.haplotags()[0].copy()
        finally:
            e.close()
    assert np.array_equal(tags[True], LA.haplotag(sample["rs"], sites, _memo(RR.observer(ref, 10)))[0])
    assert np.array_equal(tags[False], LA.haplotag(sample["rs"], sites, HA.observe)[0]) and not np.array_equal(tags[True], tags[False])
