"""Allele realignment across splice junctions on the device (c3r_set_hap_realign_spliced: k_haplotag_alleles_rs and its _w sibling,
k_hap_allele_counts_rs, k_phase_allele_links_rs, k_phase_allele_unit_links_rs) against tests/realignspliceref.py, the plain-Python
restatement: the seeded fuzz with planted introns through both walks, the hand cases, the splice invariance the feature stands for — the
introns' lengths and letters do not matter —, the equality with the _ra kernels where no read holds an N, the composition with the
base-quality threshold, the scans that must not move, the switch's life cycle and the two drivers that write what the kernels decide."""
import os

import numpy as np
import pytest

from tests import hapalleleref as HA
from tests import hapweightref as HW
from tests import leftalignref as LA
from tests import qualref as QR
from tests import realignref as RR
from tests import realignspliceref as RS
from tests import test_gpu_realign as GR

pytestmark = pytest.mark.gpu

W = 10
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
        e.set_hap_bq_weights(False)
        e.set_hap_realign(0)
        e.set_hap_realign_spliced(False)
        e.set_hap_min_bq(0)
        e.params = capi.default_params()
        e.set_params()


def _fuzz(seed):
    """(the fuzz of tests/realignref.py with qualities, the same with an intron planted every 60 bases)."""
    if seed not in _state:
        plain = RR.gen_fuzz(seed, quals=True)
        _state[seed] = (plain, RS.plant(*plain, cuts=RS.CUTS, seed=seed))
    return _state[seed]


def _sparse_fuzz():
    """A planted fuzz whose TAGS move with the switch: six sites 60 bases apart and an intron 8 bases behind each — a read holds two or three
    sites, so that single observations move tags (four reads' tags differ between `realign` and the rule here)."""
    if "sparse" not in _state:
        plain = RR.gen_fuzz(2, step=60)
        ref, table, rs = RS.plant(*plain, cuts=[s["pos"] - 1 + 8 for s in plain[1]], seed=2)
        a, b = (LA.haplotag(rs, table, GR._memo(obs))[0] for obs in (RS.observer(ref, W), RR.observer(ref, W)))
        assert int((a != b).sum()) >= 3 and set(a.tolist()) >= {1, 2} and len(table) == 6
        _state["sparse"] = (ref, table, rs)
    return _state["sparse"]


def _junction_set():
    """Thirty reads on realignspliceref.REF whose TAGS move with each switch, and their table (W = 3): the ALT read of the hand case
    `1D1I_beside_a_junction`, the same read without the intron, and a clean REF read, ten times each.  Allele A lies on haplotype 2 at
    both sites, so the CIGAR's column at the site on 14 (another allele: no vote) leaves every read on haplotype 2, and a realigned ALT
    read ties: tags 2 / 2 / 2 with both switches off, 2 / 0 / 2 under the overhang alone, 0 / 0 / 2 under both."""
    from clair3_rna_amd.reads import ReadSet
    R = RS.REF
    reads = [(5, "7M1D1M1I1M5N5M", R[5:13] + "C" + R[14] + R[20:25])] * 10 + [(5, "7M1D1M1I11M", R[5:13] + "C" + R[14:25])] * 10 + [(5, "20M", R[5:25])] * 10
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=0, mapq=60, hp=0) for r in reads])
    table = [dict(RR.site_of((8, "G", "A", "0/1")), h1=1, ps=7), dict(RR.site_of(RS.SNV), h1=1, ps=7)]
    tags = {name: LA.haplotag(rs, table, obs) for name, obs in (("rs", RS.observer((0, R), 3)), ("ra", RR.observer((0, R), 3)), ("off", HA.observe))}
    assert [tags[k][0].tolist() for k in ("off", "ra", "rs")] == [[2] * 30, [2] * 10 + [0] * 10 + [2] * 10, [0] * 20 + [2] * 10]
    return (0, R), table, rs, tags


def _device(eng, rs, table, ref, w, spliced, load=True):
    """The engine's four tables under overhang w and the switch; ref = (first 0-based position, letters)."""
    q, pool = HA.to_query(table)
    h1 = np.array([s["h1"] for s in table], np.uint8)
    eng.set_reference(ref[0] + 1, ref[1])
    eng.set_hap_realign_spliced(spliced)
    eng.set_hap_realign(w)
    if load:
        eng.load_reads(rs)
    eng.set_phase_alleles(q, h1, pool)
    hp, st = eng.haplotags()
    ups, uh1 = GR._units(table)
    qu = q.copy()
    qu["ps"] = ups
    return dict(hp=hp, st=st, ps=eng.read_phase_sets(), words=eng.haplotag_words(), counts=eng.hap_allele_counts(q, pool), links=eng.phase_allele_links(q, pool),
                ulinks=eng.phase_allele_unit_links(qu, np.array(uh1, np.uint8), pool))


def _same(got, exp):
    GR._assert_same(got, exp)
    if "words" in exp:
        assert np.array_equal(got["words"], exp["words"])


# ---- 1. the planted fuzz against the restatement: the four entry points, both walks (every second read takes the serial one)
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_planted_fuzz_against_the_restatement(eng, seed):
    _, (ref, table, rs) = _fuzz(seed)
    cig = lambda r: [int(c) & 15 for c in rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]]
    kinds = [cig(r) for r in rs.reads]
    with_n = [k for k in kinds if 3 in k]
    assert len(with_n) >= 150 and sum(1 for k in with_n if 7 in k or 8 in k) >= 30 and sum(1 for k in with_n if 6 in k) >= 30 and sum(1 for k in with_n if set(k) <= {0, 1, 2, 3, 4}) >= 60
    obs = GR._memo(RS.observer(ref, W))
    exp = GR._expected(rs, table, obs)
    exp["words"] = HW.haplotag(rs, table, obs, weighted=False)["words"]
    assert not np.array_equal(exp["words"], HW.haplotag(rs, table, GR._memo(RR.observer(ref, W)), weighted=False)["words"])
    assert int(exp["counts"][:, 1:, :2].sum()) > 500 and int(exp["links"].sum()) > 5000 and len(exp["ulinks"]) >= 6 and int(exp["ulinks"].sum()) > 500
    got = _device(eng, GR._no_quals(rs), table, ref, W, True)
    _same(got, exp)
    if seed == 0:                                            # and the switch is what does it: without it, plain `realign`'s tables — other ones
        plain = _device(eng, GR._no_quals(rs), table, ref, W, False)
        GR._assert_same(plain, GR._expected(rs, table, RR.observer(ref, W)))
        assert GR._differ(got, plain) and not np.array_equal(got["ulinks"], plain["ulinks"])


def test_the_weighted_tagger_against_the_restatement(eng):
    """k_haplotag_alleles_rs_w: tags, sets, tag words and the weight pairs."""
    _, (ref, table, rs) = _fuzz(1)
    exp = HW.haplotag(rs, table, GR._memo(RS.observer(ref, W)), weighted=True)
    q, pool = HA.to_query(table)
    eng.set_reference(1, ref[1])
    eng.set_hap_realign_spliced(True)
    eng.set_hap_realign(W)
    eng.load_reads(rs)                                       # (the weights are refused while reads without qualities are loaded)
    eng.set_hap_bq_weights(True)
    eng.set_phase_alleles(q, np.array([s["h1"] for s in table], np.uint8), pool)
    hp, st = eng.haplotags()
    assert np.array_equal(hp, exp["hp"]) and st == exp["st"] and np.array_equal(eng.read_phase_sets(), exp["ps"])
    assert np.array_equal(eng.haplotag_words(), exp["words"]) and np.array_equal(eng.haplotag_weights(), exp["w12"])
    assert int(exp["w12"].sum()) > 10000 and not np.array_equal(exp["w12"], HW.haplotag(rs, table, GR._memo(RR.observer(ref, W)), weighted=True)["w12"])


# ---- 2. the hand cases of tests/realignspliceref.py: one read, its column from the count table, and the other three entry points
@pytest.mark.parametrize("case", RS.HAND, ids=[c[0] for c in RS.HAND])
def test_hand_made_reads(eng, case):
    _, ref, row, w, read, want, want_plain, want_off, _ = case
    rs, site = RR.one_read(read), RR.site_of(row)
    eng.set_hap_realign_spliced(True)
    GR._load_one(eng, ref, rs, w)
    assert GR._column(eng, site) == want[0]
    table = [dict(RR.site_of((8, "G", "A", "0/1")), h1=0, ps=7), dict(site, h1=1, ps=7)]
    q, pool = HA.to_query(table)
    obs = RS.observer(ref, w)
    assert np.array_equal(eng.phase_allele_links(q, pool), LA.links(rs, table, obs))
    qu = q.copy()
    qu["ps"] = [1, 50]
    assert np.array_equal(eng.phase_allele_unit_links(qu, np.array([0, 1], np.uint8), pool), LA.unit_links(rs, table, [1, 50], [0, 1], obs))
    eng.set_phase_alleles(q, np.array([0, 1], np.uint8), pool)
    hp, st, ps = LA.haplotag(rs, table, obs)
    assert np.array_equal(eng.haplotags()[0], hp) and eng.haplotags()[1] == st and np.array_equal(eng.read_phase_sets(), ps)
    # without the switch the column is plain `realign`'s, without the overhang today's — whatever the switch says
    eng.set_hap_realign_spliced(False)
    assert GR._column(eng, site) == want_plain[0]
    eng.set_hap_realign_spliced(True)
    eng.set_hap_realign(0)
    assert GR._column(eng, site) == want_off


def test_the_two_limits_of_64_on_the_device(eng):
    p0, w = 60, 16
    ins11, ins12 = "GATTACAGATT", "GATTACAGATTA"
    dele = RR.LONG[p0:p0 + 21]
    fits = (p0 + 1, dele, RR.LONG[p0] + ins11 + dele[1:] + "," + RR.LONG[p0], "1/2")
    over = (p0 + 1, dele, RR.LONG[p0] + ins12 + dele[1:] + "," + RR.LONG[p0], "1/2")
    # m = 64 (realigned), m = 65 (the CIGAR's column), 2W + 1 + D + I = 65 (never realigned) and 63, with an intron in the tail
    for row, read, ww, realigned in ((fits, RR.long_read(p0, ins11), w, True), (fits, RR.long_read(p0, ins11, extra_at=70), w, False), (over, RR.long_read(p0, ins12), w, False),
                                     (over, RR.long_read(p0, ins12), w - 1, True)):
        ref, table, rs = RS.plant((0, RR.LONG), [RR.site_of(row)], RR.one_read(read), cuts=(90,), seed=3)
        assert RS.column_of(rs, 0, table[0], ref, ww) == (0, realigned) and RR.column_of(rs, 0, table[0], ref, ww) == (0, False)
        eng.set_hap_realign_spliced(True)
        GR._load_one(eng, ref, rs, ww)
        assert GR._column(eng, table[0]) == 0


# ---- 3. the two properties on the device
@pytest.mark.parametrize("seed", [2, 3])
def test_splice_invariance_on_the_device(eng, seed):
    """(b) With the switch on, the planted set's tables are the _ra kernels' tables on the set without introns: reads and sites keep their indices."""
    (ref, table, rs), (pref, ptable, prs) = _fuzz(seed)
    on_planted = _device(eng, GR._no_quals(prs), ptable, pref, W, True)
    base = _device(eng, GR._no_quals(rs), table, ref, W, False)
    _same(on_planted, base)
    assert int(base["links"].sum()) > 5000
    # and it is the switch that does it
    assert GR._differ(_device(eng, GR._no_quals(prs), ptable, pref, W, False), base)


def test_without_an_n_the_rs_kernels_give_the_ra_kernels_tables(eng):
    """(a) On the fuzz without introns the _rs kernels' output is the _ra kernels', for every overhang's extremes too."""
    (ref, table, rs), _ = _fuzz(1)
    assert RS.n_ops(rs) == 0
    for w in (1, 10, 16):
        on, off = _device(eng, GR._no_quals(rs), table, ref, w, True), _device(eng, GR._no_quals(rs), table, ref, w, False)
        _same(on, off)
        assert int(on["counts"].sum()) > 500


# ---- 4. composition with the base-quality threshold: a masked base inside a window that spans a junction
def test_composition_with_hap_min_bq(eng):
    _, (ref, table, rs) = _fuzz(0)
    Q = 10
    # the case exists: (read, site) pairs realigned only under the switch whose window holds a masked base
    spanning = 0
    for i in range(len(rs)):
        for j, s in enumerate(table):
            w = RS.spliced_window(rs, i, ref, s, W)
            if w is not None and RR.realigned_window(rs, i, ref, s, W) is None:
                spanning += any(QR.masked(QR.qual_at(rs, i, k), Q) for k in range(w[0], w[1]))
    assert spanning >= 50
    eng.load_reads(rs)                                       # (the threshold is refused while reads without qualities are loaded)
    eng.set_hap_min_bq(Q)
    got = _device(eng, rs, table, ref, W, True)
    assert eng.hap_min_bq() == (Q, QR.mask(rs, Q)[1]) and eng.hap_realign() == W and eng.hap_realign_spliced() is True
    eng.set_hap_min_bq(0)
    with_n = QR.with_n(rs, Q)
    _same(got, _device(eng, with_n, table, ref, W, True))
    assert GR._differ(got, _device(eng, GR._no_quals(rs), table, ref, W, True))
    GR._assert_same(got, GR._expected(with_n, table, RS.observer(ref, W)))


# ---- 5. what must not move: the 18- and 30-channel scans
def test_the_scans_never_see_the_switch(eng):
    from tests import hapref
    ref, table, rs = _sparse_fuzz()                          # (its tags move with the switch)
    q, pool = HA.to_query(table)
    h1 = np.array([s["h1"] for s in table], np.uint8)

    def scan(channels, w, spliced, reads=rs, tagged=True):
        eng.set_params(channels=channels, min_coverage=2)
        eng.set_reference(1, ref[1])
        eng.set_hap_realign_spliced(spliced)
        eng.set_hap_realign(w)
        if tagged:
            eng.set_phase_alleles(q, h1, pool)
        else:
            eng.set_phase_sites(None)
        eng.load_reads(reads)
        n = eng.scan(1, len(ref[1]))
        return n, eng.sites().tobytes(), eng.tokens().tobytes(), eng.tensors(rescaled=False).tobytes()
    off = scan(18, 0, False)
    assert off[0] >= 3 and scan(18, W, True) == off and scan(18, 0, True) == off
    # 30 channels: the scan under (table, W, switch) is the scan without a table of the same reads carrying that run's tags
    with_table = scan(30, W, True)
    tags = eng.haplotags()[0].copy()
    eng.set_hap_realign_spliced(False)
    assert not np.array_equal(eng.haplotags()[0], tags) and set(tags.tolist()) >= {1, 2}
    assert scan(30, 0, False, hapref.with_hp(rs, tags), tagged=False) == with_table


# ---- 6. the life cycle of the switch
def test_life_cycle():
    from clair3_rna_amd import capi
    ref, table, rs, tags = _junction_set()                   # (three different tag vectors: both off, the overhang alone, both on)
    W = 3
    q, pool = HA.to_query(table)
    h1 = np.array([s["h1"] for s in table], np.uint8)
    rs_tags, _, rs_ps = tags["rs"]
    ra_tags, off_tags = tags["ra"][0], tags["off"][0]
    L = capi.load_library()
    e = capi.Engine(0)
    try:
        assert e.hap_realign_spliced() is False
        for bad in (2, -1, 64):
            with pytest.raises(capi.C3RError) as err:
                e.set_hap_realign_spliced(bad)
            assert err.value.code == -1 and "neither 0 nor 1" in str(err.value) and e.hap_realign_spliced() is False
        # the switch before the overhang: accepted at any time, without a reference too, and without effect while the overhang is 0
        e.set_reference(1, ref[1])
        e.load_reads(rs)
        e.set_phase_alleles(q, h1, pool)
        assert np.array_equal(e.haplotags()[0], off_tags)
        e.set_hap_realign_spliced(True)
        assert e.hap_realign_spliced() is True and np.array_equal(e.haplotags()[0], off_tags)
        e.set_hap_realign(W)
        assert np.array_equal(e.haplotags()[0], rs_tags) and np.array_equal(e.read_phase_sets(), rs_ps)
        # the switch after the overhang: a flip re-tags, both ways
        e.set_hap_realign_spliced(False)
        assert np.array_equal(e.haplotags()[0], ra_tags)
        e.set_hap_realign_spliced(True)
        assert np.array_equal(e.haplotags()[0], rs_tags)
        # a refused flip leaves tags and value as they were
        assert L.c3r_set_hap_realign_spliced(e.h, 2) == -1 and e.hap_realign_spliced() is True and np.array_equal(e.haplotags()[0], rs_tags)
        e.set_hap_realign_spliced(False)
        assert L.c3r_set_hap_realign_spliced(e.h, -1) == -1 and e.hap_realign_spliced() is False and np.array_equal(e.haplotags()[0], ra_tags)
        # left-align keeps excluding realign, whatever this switch says, and a refusal changes nothing
        e.set_hap_realign_spliced(True)
        with pytest.raises(capi.C3RError) as err:
            e.set_hap_left_align(True)
        assert err.value.code == -1 and "exclude each other" in str(err.value) and np.array_equal(e.haplotags()[0], rs_tags)
        # a load under both switches tags with them; the overhang back to 0 gives today's tags with the switch still on
        e.load_reads(rs)
        assert np.array_equal(e.haplotags()[0], rs_tags)
        e.set_hap_realign(0)
        assert e.hap_realign_spliced() is True and np.array_equal(e.haplotags()[0], off_tags)
        e.set_hap_realign(W)
        # set_phase_alleles with n = 0 still clears, and a new table is tagged under the switch
        e.set_phase_alleles(None, None)
        with pytest.raises(capi.C3RError):
            e.haplotags()                                    # (no table: there are no tags)
        e.set_phase_alleles(q, h1, pool)
        assert np.array_equal(e.haplotags()[0], rs_tags)
        # no reference: the switch itself is accepted where no re-tagging is due, and n = 0 still clears
        e2 = capi.Engine(0)
        try:
            e2.load_reads(rs)
            e2.set_hap_realign(W)
            e2.set_hap_realign_spliced(True)
            with pytest.raises(capi.C3RError) as err:
                e2.set_phase_alleles(q, h1, pool)
            assert err.value.code == -1 and "no reference is set" in str(err.value) and e2.hap_realign_spliced() is True
            e2.set_phase_alleles(None, None)
        finally:
            e2.close()
    finally:
        e.close()


def test_kernels_by_name(eng):
    """Both switches on, each call launches its _rs kernel once and none of its siblings; the switch alone launches the plain ones, the
    overhang alone the _ra ones; under the weights the tagger is k_haplotag_alleles_rs_w."""
    _, (ref, table, rs) = _fuzz(0)
    names = ("k_haplotag_alleles", "k_hap_allele_counts", "k_phase_allele_links", "k_phase_allele_unit_links")
    eng.set_profiling(True)
    try:
        for w, spliced, want in ((W, True, "_rs"), (0, True, ""), (W, False, "_ra")):
            eng.reset_kernel_stats()
            _device(eng, GR._no_quals(rs), table, ref, w, spliced)
            stats = eng.kernel_stats()
            for k in names:
                assert stats[k + want]["launches"] >= 1, (w, spliced, k, sorted(stats))
                assert not [s for s in ("", "_la", "_ra", "_rs") if s != want and k + s in stats], (w, spliced, k, sorted(stats))
        eng.load_reads(rs)                                   # (with qualities: the weights are refused without)
        eng.set_hap_bq_weights(True)
        eng.reset_kernel_stats()
        _device(eng, rs, table, ref, W, True)
        stats = eng.kernel_stats()
        assert stats["k_haplotag_alleles_rs_w"]["launches"] >= 1 and not [k for k in stats if k.startswith("k_haplotag") and k != "k_haplotag_alleles_rs_w"], sorted(stats)
    finally:
        eng.set_profiling(False)


# ---- 7. the drivers that write what the kernels decide: the planted fuzz as a BAM through phase_vcf and haplotag_bam
@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    from clair3_rna_amd import bam, bamio, io
    tmp = str(tmp_path_factory.mktemp("realign_spliced_drivers"))
    ref, table, rs = _sparse_fuzz()
    rows = ["chr1\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:GQ\t%s:30\n" % (s["pos"], s["ref"], s["alt"], "1/2" if "," in s["alt"] else "0/1") for s in table]
    fa, bam_fn, vcf = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "plain.bam"), os.path.join(tmp, "calls.vcf")
    io.write_fasta(fa, [("chr1", ref[1])])
    bam.write_bam(bam_fn, [("chr1", len(ref[1]))], {"chr1": rs})
    bamio.index_build(bam_fn)
    with open(vcf, "w") as f:
        f.write(GR.HEAD + "".join(rows))
    return dict(tmp=tmp, fa=fa, bam=bam_fn, vcf=vcf, rows=rows, rs=rs, ref=ref)


def test_phase_vcf_with_the_flag(sample, tmp_path):
    ref = sample["ref"]
    cands, skipped = HA.candidates(sample["rows"], "chr1")
    assert len(cands) == 6 and not any(skipped.values())
    snvs = [c for c in cands if HA.flags(c) == (True, False)]
    ra = ["--hap_realign", "--ref_fn", sample["fa"]]
    got = {name: GR._phase_vcf(sample, str(tmp_path / name), extra) for name, extra in
           (("indels_ra", ["--indels"] + ra), ("indels_rs", ["--indels", "--hap_realign_spliced"] + ra), ("snv_rs", ra + ["--hap_realign_spliced"]))}
    assert got["indels_rs"] == GR._predicted_vcf(sample, cands, RS.observer(ref, 10)) and got["snv_rs"] == GR._predicted_vcf(sample, snvs, RS.observer(ref, 10))
    assert got["indels_ra"] == GR._predicted_vcf(sample, cands, RR.observer(ref, 10))
    assert sum("|" in l.split("\t")[9] for l in got["indels_rs"].splitlines() if not l.startswith("#")) == 6


def test_haplotag_bam_with_the_flag(sample, tmp_path):
    from clair3_rna_amd import haplotag_bam, io
    ref = sample["ref"]
    phased_dir = str(tmp_path / "phased_vcf")
    text = GR._phase_vcf(sample, phased_dir, ["--indels", "--hap_realign", "--hap_realign_spliced", "--ref_fn", sample["fa"]])
    sites = []
    for f in (l.split("\t") for l in text.splitlines() if not l.startswith("#")):
        gt, ps = f[9].split(":")[0], f[9].split(":")[-1]
        if "|" in gt:
            sites.append(dict(HA.site_of_row(int(f[1]), f[3], f[4], gt.replace("|", "/"), int(ps)), h1=1 if gt in ("1|0", "2|1") else 0))
    assert len(sites) == 6
    hp = {}
    for name, extra in (("rs", ["--hap_realign", "10", "--hap_realign_spliced"]), ("ra", ["--hap_realign", "10"])):
        out_dir = str(tmp_path / ("bam_" + name))
        argv = ["--bam_fn", sample["bam"], "--phased_vcf_fn", phased_dir, "--output_dir", out_dir, "--haplotag_indels", "--ref_fn", sample["fa"]] + extra
        haplotag_bam.Run(haplotag_bam.build_parser().parse_args(argv), log=lambda m: None)
        hp[name] = io.load_reads(os.path.join(out_dir, "chr1.bam"), "chr1").reads["hp"].copy()
    assert np.array_equal(hp["rs"], LA.haplotag(sample["rs"], sites, GR._memo(RS.observer(ref, 10)))[0])
    assert np.array_equal(hp["ra"], LA.haplotag(sample["rs"], sites, GR._memo(RR.observer(ref, 10)))[0])
    assert int((hp["rs"] != 0).sum()) >= 150 and not np.array_equal(hp["rs"], hp["ra"])
