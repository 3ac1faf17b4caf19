"""Quality-weighted haplotag votes on the device (c3r_set_hap_bq_weights: k_haplotag_w, k_haplotag_alleles_w, k_haplotag_alleles_la_w,
k_haplotag_alleles_ra_w) against tests/hapweightref.py, the plain-Python restatement: the hand cases and the seeded fuzz through the four
kernels and both walks, the invariances (equal qualities, no qualities), the composition with the threshold, what must not move (counts,
links, scans), the switch's life cycle and the drivers."""
import os

import numpy as np
import pytest

from tests import hapalleleref as HA
from tests import hapindelref as HI
from tests import hapref
from tests import hapweightref as HW
from tests import leftalignref as LA
from tests import qualref as QR
from tests import realignref as RR

pytestmark = pytest.mark.gpu

FORMS = ("snv", "alleles", "la", "ra")
RA_W = 10
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
        e.set_hap_left_align(False)
        e.set_hap_min_bq(0)
        e.params = capi.default_params()
        e.set_params()


def _fuzz():
    if "fuzz" not in _state:
        _state["fuzz"] = HW.gen_fuzz()
    return _state["fuzz"]


def _form(form, table, ref):
    """(the table as the restatement holds it under this form, its observation); ref = (first 0-based position, letters)."""
    if form == "snv":
        return HI.from_snv_table(HW.snv_rows(table)), HA.observe
    if form == "alleles":
        return table, HA.observe
    if form == "la":
        return LA.align_sites(table, (ref[1], ref[0]))[0], LA.observer((ref[1], ref[0]))
    return table, RR.observer(ref, RA_W)


def _expected(form, rs, table, ref, weighted=True):
    key = (form, id(rs), id(table), weighted)
    if key not in _state:
        t, obs = _form(form, table, ref)
        _state[key] = HW.haplotag(rs, t, obs, weighted)
    return _state[key]


def _device(eng, form, rs, table, ref, weights, load=True):
    """The engine's tags under this form: dict(hp, ps, words, st, w12 (None with the switch off))."""
    t, _ = _form(form, table, ref)
    if form in ("la", "ra"):
        eng.set_reference(ref[0] + 1, ref[1])
    eng.set_hap_left_align(form == "la")
    eng.set_hap_realign(RA_W if form == "ra" else 0)
    eng.set_hap_bq_weights(weights)
    if load:
        eng.load_reads(rs)
    if form == "snv":
        eng.set_phase_sites(HW.snv_rows(table))
    else:
        q, h1, pool, n = HI.to_engine(t)
        eng.set_phase_alleles(q, h1, pool, n)
    hp, st = eng.haplotags()
    return dict(hp=hp, st=st, ps=eng.read_phase_sets(), words=eng.haplotag_words(), w12=eng.haplotag_weights() if weights else None)


def _assert_same(got, exp, pairs=True):
    assert np.array_equal(got["hp"], exp["hp"]), np.argwhere(got["hp"] != exp["hp"])[:10].ravel()
    assert np.array_equal(got["ps"], exp["ps"]), np.argwhere(got["ps"] != exp["ps"])[:10].ravel()
    assert got["words"].dtype == np.uint32 and np.array_equal(got["words"], exp["words"]), np.argwhere(got["words"] != exp["words"])[:10].ravel()
    assert got["st"] == exp["st"]
    if pairs:
        assert got["w12"].dtype == np.uint32 and got["w12"].shape == exp["w12"].shape and np.array_equal(got["w12"], exp["w12"]), np.argwhere(got["w12"] != exp["w12"])[:10]


# ---- 1. the four kernels against the restatement
@pytest.mark.parametrize("case", HW.CASES, ids=[c[0] for c in HW.CASES])
def test_hand_cases(eng, case):
    rs, sites, Q = HW.case_inputs(case)
    q, h1, pool, n = HI.to_engine(sites)
    eng.set_hap_min_bq(Q)
    eng.set_hap_bq_weights(True)
    eng.load_reads(rs)
    eng.set_phase_alleles(q, h1, pool, n)
    hp, st = eng.haplotags()
    ps, w, words = eng.read_phase_sets(), eng.haplotag_weights(), eng.haplotag_words()
    for i, (ehp, w1, w2, eps, n_obs) in enumerate(case[4]):
        assert (int(hp[i]), int(w[i][0]), int(w[i][1]), int(ps[i]), int(words[i])) == (ehp, w1, w2, eps, ehp | n_obs << 2), (case[0], i)
    assert st["n_votes"] == sum(c[4] for c in case[4]) and st["n_tie"] == sum(1 for c in case[4] if c[0] == 0 and c[4]) and st["n_no_vote"] == sum(1 for c in case[4] if not c[4])
    # and the switch is what does it: off, the tags are the unit-weight ones, which differ wherever the case says so
    eng.set_hap_bq_weights(False)
    off = [(int(a), int(b)) for a, b in zip(eng.haplotags()[0], eng.read_phase_sets())]
    assert off == case[5]
    on = [(c[0], c[3]) for c in case[4]]
    if case[0] not in ("no_qualities", "masked_bases_do_not_vote"):          # (the two cases whose point is that nothing moves)
        assert on != off
    else:
        assert on == off
    # an SNV-only case also goes through k_haplotag_w
    if all(s["A"][1] == HA.NONE and s["B"][1] == HA.NONE for s in sites):
        eng.set_hap_bq_weights(True)
        eng.set_phase_sites(HW.snv_rows(sites))
        assert [tuple(int(x) for x in r) for r in eng.haplotag_weights()] == [(c[1], c[2]) for c in case[4]] and eng.haplotags()[0].tolist() == [c[0] for c in case[4]]
        assert eng.haplotag_words().tolist() == [c[0] | c[4] << 2 for c in case[4]]


@pytest.mark.parametrize("form", FORMS)
def test_fuzz_against_the_restatement(eng, form):
    ref, table, rs = _fuzz()
    exp, unit = _expected(form, rs, table, ref), _expected(form, rs, table, ref, False)
    c = HW.fuzz_classes(exp, unit)
    assert c["tagged_unit"] >= 100 and c["differ"] * 20 >= c["tagged_unit"], c             # (the old rule would fail the comparison below)
    got = _device(eng, form, rs, table, ref, True)
    _assert_same(got, exp)
    off = _device(eng, form, rs, table, ref, False)
    _assert_same(off, unit, pairs=False)
    assert not np.array_equal(off["hp"], got["hp"])


def test_twenty_interleaved_sets_and_an_odd_cigar(eng):
    """One read over 60 sites of 20 interleaved phase sets (a further walk per set), and one whose CIGAR is `3M2=1X1P4M`, hard clips around it."""
    import random
    from clair3_rna_amd.reads import ReadSet
    rng = random.Random(11)
    L = 60
    rows = [(p + 1, "A", "C", "0|1" if rng.random() < 0.5 else "1|0", 100 + (p * 7) % 20) for p in range(L)]
    sites = [HI.site(*r) for r in rows]
    seq = "".join(rng.choice("AC") for _ in range(L))
    recs = [dict(pos=0, cigar="%dM" % L, seq=seq, flag=0, mapq=60, hp=0, qual=[rng.choice((0, 2, 9, 17, 33, 41)) for _ in range(L)]),
            dict(pos=3, cigar="2H3M2=1X1P4M3H", seq=seq[3:13], flag=0, mapq=60, hp=0, qual=[rng.randint(0, 60) for _ in range(10)])]
    rs = ReadSet.from_records(recs)
    exp = HW.haplotag(rs, sites)
    assert len(set(s["ps"] for s in sites)) == 20 and exp["st"]["n_votes"] == 70
    for snv in (False, True):
        eng.set_hap_bq_weights(True)
        eng.load_reads(rs)
        if snv:
            eng.set_phase_sites(HW.snv_rows(sites))
        else:
            eng.set_phase_alleles(*HI.to_engine(sites))
        hp, st = eng.haplotags()
        _assert_same(dict(hp=hp, st=st, ps=eng.read_phase_sets(), words=eng.haplotag_words(), w12=eng.haplotag_weights()), exp)


# ---- 2. the invariances
@pytest.mark.parametrize("form", FORMS)
def test_equal_qualities_and_no_qualities_give_the_switched_off_run(eng, form):
    ref, table, rs = _fuzz()
    off = _device(eng, form, rs, table, ref, False)
    unit = _expected(form, rs, table, ref, False)
    for k in (23, 0xff):                                        # every base Q23; every base without a quality, which weighs 1
        on = _device(eng, form, HW.with_qual(rs, np.full(len(rs.qual), k, np.uint8)), table, ref, True)
        _assert_same(on, off, pairs=False)
        assert np.array_equal(on["w12"], unit["w12"] * (1 if k == 0xff else k)), k


# ---- 3. composition with the threshold
@pytest.mark.parametrize("form", ("snv", "alleles"))
def test_composition_with_hap_min_bq(eng, form):
    ref, table, rs = _fuzz()
    Q = 8
    with_n = HW.masked_as_n(rs, Q)
    eng.set_hap_min_bq(Q)
    got = _device(eng, form, rs, table, ref, True)
    assert eng.hap_min_bq()[1] == QR.mask(rs, Q)[1] > 100
    t, obs = _form(form, table, ref)
    exp = HW.haplotag(with_n, t, obs)
    _assert_same(got, exp)
    eng.set_hap_min_bq(0)
    assert not np.array_equal(eng.haplotag_weights(), got["w12"])
    on_n = _device(eng, form, with_n, table, ref, True)          # the host's N in the place of the device's mask
    _assert_same(on_n, exp)


# ---- 4. what must not move
def test_counts_and_links_do_not_look_at_the_switch(eng):
    """The count and link tables under the switch are the restatement's for the WEIGHTED tags (counts) and the unweighted links."""
    ref, table, rs = _fuzz()
    q, h1, pool, n = HI.to_engine(table)
    snv = HW.snv_rows(table)
    units = snv.copy()
    units["ps"] = 1 + np.arange(len(snv)) // 3               # (units of three SNV sites, oriented by the sites' h1)
    out = {}
    for on in (False, True):
        got = _device(eng, "alleles", rs, table, ref, on)
        out[on] = dict(tags=got, counts=eng.hap_allele_counts(q, pool), links=eng.phase_allele_links(q, pool),
                       ulinks=eng.phase_allele_unit_links(q, h1, pool), snv_links=eng.phase_links(snv), snv_ulinks=eng.phase_unit_links(units),
                       snv_counts=eng.hap_counts(snv))
    # the four link calls hold reads against sites, not against tags: bit for bit the same
    for key in ("links", "ulinks", "snv_links", "snv_ulinks"):
        assert np.array_equal(out[True][key], out[False][key]) and int(out[True][key].sum()) > 100, key
    # counts are split by the tags: they are the unweighted count of reads under the weighted tags, and so are the SNV counts
    exp = _expected("alleles", rs, table, ref)
    assert np.array_equal(out[True]["counts"], HI.allele_counts(rs, exp["hp"], exp["ps"], table))
    assert np.array_equal(out[True]["snv_counts"], HI.snv_counts(rs, exp["hp"], exp["ps"], snv))
    unit = _expected("alleles", rs, table, ref, False)
    assert np.array_equal(out[False]["counts"], HI.allele_counts(rs, unit["hp"], unit["ps"], table))
    assert out[True]["counts"].sum() == out[False]["counts"].sum() and not np.array_equal(out[True]["counts"], out[False]["counts"])


def test_the_scans_change_only_through_the_tags(eng):
    from clair3_rna_amd import synth
    from clair3_rna_amd.reads import ReadSet
    ref, table, rs = _fuzz()
    snv = HW.snv_rows(table)

    def scan(channels):
        eng.set_params(channels=channels, min_coverage=2)
        eng.load_reads(rs)
        eng.set_reference(ref[0] + 1, ref[1])
        n = eng.scan(1, len(ref[1]))
        return (n, eng.sites().tobytes(), eng.tokens().tobytes(), eng.tensors(rescaled=False).tobytes())
    eng.set_phase_sites(snv)
    off18 = scan(18)
    off30 = scan(30)
    eng.set_hap_bq_weights(True)
    on18 = scan(18)
    on30 = scan(30)
    tags = eng.haplotags()[0].copy()
    assert off18[0] >= 8 and on18 == off18 and on30 != off30
    eng.set_hap_bq_weights(False)
    eng.set_phase_sites(None)
    eng.set_params(channels=30, min_coverage=2)
    eng.load_reads(hapref.with_hp(ReadSet(rs.reads, rs.cigar, rs.seq), tags))
    eng.set_reference(ref[0] + 1, ref[1])
    n = eng.scan(1, len(ref[1]))
    assert (n, eng.sites().tobytes(), eng.tokens().tobytes(), eng.tensors(rescaled=False).tobytes()) == on30


# ---- 5. life cycle
def test_life_cycle():
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    ref, table, rs = _fuzz()
    snv = HW.snv_rows(table)
    sn = HI.from_snv_table(snv)
    want_on, want_off = HW.haplotag(rs, sn), HW.haplotag(rs, sn, weighted=False)
    want_alleles = _expected("alleles", rs, table, ref)
    no_quals = ReadSet(rs.reads, rs.cigar, rs.seq)
    e = capi.Engine(0)
    try:
        same = lambda want: np.array_equal(e.haplotags()[0], want["hp"]) and np.array_equal(e.read_phase_sets(), want["ps"])
        assert e.hap_bq_weights() is False
        for bad in (2, -1):
            assert capi.load_library().c3r_set_hap_bq_weights(e.h, bad) == -1 and e.hap_bq_weights() is False
        # the getter is refused without a table and with the switch off
        with pytest.raises(capi.C3RError):
            e.haplotag_weights()
        e.set_phase_sites(snv)
        e.load_reads(rs)
        with pytest.raises(capi.C3RError) as err:
            e.haplotag_weights()
        assert err.value.code == -1 and "c3r_set_hap_bq_weights is off" in str(err.value) and same(want_off)
        assert np.array_equal(e.haplotag_words(), want_off["words"])       # (the words are there with the switch off too)
        # after the load: tagged again on the device
        e.set_hap_bq_weights(True)
        assert e.hap_bq_weights() is True and same(want_on) and np.array_equal(e.haplotag_weights(), want_on["w12"])
        # on -> off -> on
        e.set_hap_bq_weights(False)
        assert same(want_off)
        with pytest.raises(capi.C3RError):
            e.haplotag_weights()
        e.set_hap_bq_weights(True)
        assert same(want_on) and np.array_equal(e.haplotag_weights(), want_on["w12"])
        # before the load: the same result
        e.load_reads(rs)
        assert same(want_on) and np.array_equal(e.haplotag_weights(), want_on["w12"])
        # a table replaced under the switch, and the SNV table back
        e.set_phase_alleles(*HI.to_engine(table))
        assert same(want_alleles) and np.array_equal(e.haplotag_weights(), want_alleles["w12"])
        e.set_phase_sites(snv)
        assert same(want_on)
        # new filters rebuild the tables: the same tags and pairs
        e.set_params(min_mq=61)
        assert same(want_on) and np.array_equal(e.haplotag_weights(), want_on["w12"])
        e.set_params(min_mq=5)
        # a small cap
        out = np.zeros((2, 2), np.uint32)
        assert capi.load_library().c3r_get_haplotag_weights(e.h, out.ctypes.data, 2) == -6 and capi.load_library().c3r_get_haplotag_words(e.h, out.ctypes.data, 2) == -6
        assert np.array_equal(e.haplotag_words(), want_on["words"])
        # a load without qualities under the switch is refused before anything is given up
        with pytest.raises(capi.C3RError) as err:
            e.load_reads(no_quals)
        assert err.value.code == -1 and "c3r_set_hap_bq_weights" in str(err.value) and same(want_on) and np.array_equal(e.haplotag_weights(), want_on["w12"])
        # n_reads = 0 is allowed
        e.load_reads(ReadSet.from_records([]))
        assert e.haplotag_weights().shape == (0, 2)
        # the switch set on reads that came without qualities is refused, and the context works on
        e.set_hap_bq_weights(False)
        e.load_reads(no_quals)
        with pytest.raises(capi.C3RError) as err:
            e.set_hap_bq_weights(True)
        assert err.value.code == -1 and "without qualities" in str(err.value) and e.hap_bq_weights() is False and same(want_off)
        e.load_reads(rs)
        e.set_hap_bq_weights(True)
        assert same(want_on)
    finally:
        e.close()


# ---- 6. the drivers on one small BAM with qualities
HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    from clair3_rna_amd import bam, bamio, io, synth
    tmp = str(tmp_path_factory.mktemp("hap_bq_weights_drivers"))
    ref, table, rs = _fuzz()
    snv = HW.snv_rows(table)
    fa, w30 = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model30")
    io.write_fasta(fa, [("chr1", ref[1])])
    np.save(w30 + ".c3rw.npy", synth.random_weights(30, seed=5))
    bam_fn = os.path.join(tmp, "quals.bam")
    bam.write_bam(bam_fn, [("chr1", len(ref[1]))], {"chr1": rs})
    bamio.index_build(bam_fn)
    phased = os.path.join(tmp, "phased.vcf")
    letter = {1: "A", 2: "C", 4: "G", 8: "T"}
    with open(phased, "w") as f:
        f.write(HEAD + "".join("chr1\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s:%d\n" % (int(s["pos"]), letter[int(s["ref"])], letter[int(s["alt"])], "1|0" if int(s["h1"]) else "0|1",
                                                                                   int(s["ps"])) for s in snv))
    sn = HI.from_snv_table(snv)
    return dict(tmp=tmp, fa=fa, w30=w30, bam=bam_fn, phased=phased, rs=rs, on=HW.haplotag(rs, sn), off=HW.haplotag(rs, sn, weighted=False))


def test_haplotag_bam_writes_the_weighted_tags_and_pc(sample, tmp_path):
    from clair3_rna_amd import haplotag_bam
    from tests import bamref
    out, raw = {}, {}
    for flag in (False, True):
        out_dir = str(tmp_path / ("w%d" % flag))
        haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", sample["bam"], "--phased_vcf_fn", sample["phased"], "--output_dir", out_dir]
                                                                + (["--hap_bq_weights"] if flag else [])), log=lambda m: None)
        recs = bamref.Bam(os.path.join(out_dir, "chr1.bam")).records
        out[flag] = [((r.tag("HP") or (None, 0))[1], (r.tag("PS") or (None, -1))[1], (r.tag("PC") or (None, None))[1]) for r in recs]
        raw[flag] = recs
    pc = HW.pc_of(sample["on"]["w12"])
    want_on = [(int(h), int(p), int(c) if h else None) for h, p, c in zip(sample["on"]["hp"], sample["on"]["ps"], pc)]
    assert out[True] == want_on and sum(1 for w in want_on if w[2] is not None) > 100
    assert all(r.tag("PC")[0] == ("C" if r.tag("PC")[1] < 256 else "S" if r.tag("PC")[1] < 65536 else "I") for r in raw[True] if r.tag("PC"))      # (the smallest type)
    assert out[False] == [(int(h), int(p), None) for h, p in zip(sample["off"]["hp"], sample["off"]["ps"])]
    # without the flag the file is the one the writer's old entry point makes from the engine's tags
    from clair3_rna_amd import bamio, capi
    e = capi.Engine(0)
    try:
        e.set_phase_sites(HW.snv_rows(_fuzz()[1]))
        with bamio.BamFile(sample["bam"]) as bf:
            rs = bf.fetch("chr1")
            e.load_reads(rs)
            line = haplotag_bam.pg_line(bf.header_text(), haplotag_bam._version(), "x")
            plain = str(tmp_path / "plain.bam")
            bf.write_haplotagged("chr1", plain, rs, e.haplotags()[0], e.read_phase_sets(), pg_line=line)
    finally:
        e.close()
    records = lambda path: [bytes(r.raw) for r in bamref.Bam(path).records]          # (the headers differ by the command in @PG)
    assert records(plain) == records(os.path.join(str(tmp_path / "w0"), "chr1.bam"))


def test_call_var_bam_under_the_flag_equals_a_run_on_a_bam_with_the_weighted_tags(sample, tmp_path):
    from clair3_rna_amd import bam, bamio, call_var_bam, capi
    from clair3_rna_amd.reads import ReadSet
    rs = sample["rs"]
    tagged_bam = str(tmp_path / "tagged.bam")
    bam.write_bam(tagged_bam, [("chr1", len(_fuzz()[0][1]))], {"chr1": hapref.with_hp(ReadSet(rs.reads, rs.cigar, rs.seq), sample["on"]["hp"])})
    bamio.index_build(tagged_bam)
    base = ["--chkpnt_fn", sample["w30"], "--ref_fn", sample["fa"], "--ctgName", "chr1", "--pileup", "--chunk_id", "1", "--chunk_num", "1", "--minCoverage", "2",
            "--enable_phasing_model", "True"]
    runs = {"weights": ["--bam_fn", sample["bam"], "--phased_vcf_fn", sample["phased"], "--hap_bq_weights"],
            "unit": ["--bam_fn", sample["bam"], "--phased_vcf_fn", sample["phased"]],
            "tagged": ["--bam_fn", tagged_bam]}
    text, tags = {}, {}
    for name, extra in runs.items():
        e = capi.Engine(0)
        try:
            fn = str(tmp_path / (name + ".vcf"))
            call_var_bam.Run(call_var_bam.build_parser().parse_args(base + extra + ["--call_fn", fn]), engine=e)
            text[name] = open(fn).read() if os.path.exists(fn) else ""
            assert e.hap_bq_weights() is (name == "weights")
            if name != "tagged":
                tags[name] = e.haplotags()[0].copy()
        finally:
            e.close()
    assert np.array_equal(tags["weights"], sample["on"]["hp"]) and np.array_equal(tags["unit"], sample["off"]["hp"])
    assert text["weights"] == text["tagged"] and text["weights"].count("\n") > 5
