"""Left-alignment of the reads' indels on the device (c3r_set_hap_left_align: k_hap_allele_counts_la, k_haplotag_alleles_la,
k_phase_allele_links_la, k_phase_allele_unit_links_la) against tests/leftalignref.py, the plain-Python restatement: random repeat cases,
hand-made reads where the kernel can go wrong, the invariance the feature stands for, the switched-off calls against hapalleleref, and the
switch's life cycle; and the five drivers under --left_align_indels."""
import gzip
import os

import numpy as np
import pytest

from tests import hapalleleref as HA
from tests import hapindelref as HI
from tests import leftalignref as LA
from tests import phaseindelref as PI
from tests import phaseref as P

pytestmark = pytest.mark.gpu

K = P.K
_state = {}


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clean(request):
    """Every test of this module starts and leaves its engine with the switch off, without a phase table and with default parameters."""
    yield
    if "eng" in request.fixturenames:
        from clair3_rna_amd import capi
        e = request.getfixturevalue("eng")
        e.set_phase_sites(None)
        e.set_hap_left_align(False)
        e.params = capi.default_params()
        e.set_params()


def _units(sites):
    """Units of six table sites, every eleventh site in none, oriented by the sites' h1 (the chain leaves one block on these cases)."""
    return [-1 if j % 11 == 5 else 1 + j // 6 for j in range(len(sites))], [s["h1"] for s in sites]


def _expected(rs, table, obs):
    """The restatement's four tables of (reads, table) under an observation."""
    hp, st, ps = LA.haplotag(rs, table, obs)
    ups, uh1 = _units(table)
    return dict(hp=hp, st=st, ps=ps, counts=LA.allele_counts(rs, hp, ps, table, obs), links=LA.links(rs, table, obs),
                ulinks=LA.unit_links(rs, table, ups, uh1, obs))


def _device(eng, rs, table, ref, on, lo=0, load=True):
    """The engine's four tables; `table` as the restatement holds it (align_sites' output when the switch is on)."""
    q, pool = HA.to_query(table)
    h1 = np.array([s["h1"] for s in table], np.uint8)
    if on:
        eng.set_reference(lo + 1, ref)
    eng.set_hap_left_align(on)
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


def _case(seed):
    """gen_repeats(seed, False / True) with their tables and the restatement's answers, computed once."""
    if seed not in _state:
        plain, jit = LA.gen_repeats(seed, False), LA.gen_repeats(seed, True)
        ref = (plain[0], 0)
        t_off, _ = LA.table_of_case(plain[2], plain[3], plain[4])
        t_jit, _ = LA.table_of_case(jit[2], jit[3], jit[4])
        t_on, _, skipped, moved = LA.align_sites(t_jit, ref)
        assert moved > 10 and not any(skipped.values())
        _state[seed] = dict(ref=plain[0], rs_off=plain[1], rs_jit=jit[1], t_off=t_off, t_jit=t_jit, t_on=t_on,
                            exp_on=_expected(jit[1], t_on, LA.observer(ref)), exp_off=_expected(plain[1], t_off, HA.observe))
    return _state[seed]


# ---- 1. the four entry points, switch on, on reads and rows that place their indels anywhere in a repeat
@pytest.mark.parametrize("seed", range(3))
def test_generated_repeats(eng, seed):
    from clair3_rna_amd import capi
    c = _case(seed)
    assert len(c["rs_jit"]) <= 403 and len(c["ref"]) == 6000
    # the table the host function makes of the jittered rows is the restatement's
    qj, pj = HA.to_query(c["t_jit"])
    q, pool, _, src, st = capi.hap_left_align_sites(qj, pj, 1, c["ref"])
    eq, epool = HA.to_query(c["t_on"])
    assert q.tobytes() == eq.tobytes() and pool.tobytes() == epool[:len(pool)].tobytes() and list(src) == list(range(len(qj))) and st["n_moved"] > 10
    exp = c["exp_on"]
    assert int(exp["counts"][:, 1:, 1].sum()) > 100 and int(exp["links"].sum()) > 1000 and len(exp["ulinks"]) > 10 and int(exp["ulinks"].sum()) > 100
    _assert_same(_device(eng, c["rs_jit"], c["t_on"], c["ref"], True), exp)


# ---- 2. the invariance, on the device: (jitter, switch on) == (no jitter, switch off), and the switch is what does it
@pytest.mark.parametrize("seed", range(3))
def test_invariance_on_the_device(eng, seed):
    c = _case(seed)
    on = _device(eng, c["rs_jit"], c["t_on"], c["ref"], True)
    off = _device(eng, c["rs_off"], c["t_off"], c["ref"], False)
    _assert_same(on, off)
    _assert_same(off, c["exp_off"])
    unaligned = _device(eng, c["rs_jit"], c["t_jit"], c["ref"], False)
    assert not np.array_equal(unaligned["links"], off["links"]) and not np.array_equal(unaligned["counts"], off["counts"])


# ---- 3. switched off, the four calls are what they were: hapalleleref's observation on its own cases (random sequence, read errors)
@pytest.mark.parametrize("seed", range(2))
def test_switch_off_is_todays_output(eng, seed):
    ref, rs, rows, truth, planted, _ = HA.gen_case(seed, errors=True)
    sites, tr, _ = PI.table_of_case(rows, truth, planted)
    table = [dict(s, h1=t) for s, t in zip(sites, tr)]
    got = _device(eng, rs, table, ref, False)
    hp, st, ps = HI.haplotag(rs, table)
    ups, uh1 = _units(table)
    assert np.array_equal(got["hp"], hp) and np.array_equal(got["ps"], ps) and got["st"] == st
    assert np.array_equal(got["counts"], HI.allele_counts(rs, hp, ps, table))
    assert np.array_equal(got["links"], PI.links(rs, table)) and np.array_equal(got["ulinks"], PI.unit_links(rs, table, ups, uh1))
    # and a reference that is set, or the switch having been on before, changes nothing of it
    eng.set_reference(1, ref)
    eng.set_hap_left_align(True)
    eng.set_hap_left_align(False)
    again = _device(eng, rs, table, ref, False, load=False)
    _assert_same(again, got)


# ---- 4. hand-made reads
def _columns(eng, rs, table, ref, lo):
    """{table index: column} of the ONE loaded read, from the count table (row 0: the read carries no tag of the query's set)."""
    q, pool = HA.to_query(table)
    q["ps"] = 7
    counts = eng.hap_allele_counts(q, pool)
    assert int(counts.sum()) == int(counts[:, 0].sum()) and int(counts.max(initial=0)) <= 1
    return {int(j): int(c) for j, c in zip(*np.nonzero(counts[:, 0]))}


@pytest.mark.parametrize("case", LA.HAND_READS, ids=[c[0] for c in LA.HAND_READS])
def test_hand_made_reads(eng, case):
    name, (text, lo), read, want = case
    table = [dict(s, h1=0) for s in LA.hand_table()]
    rs = LA.hand_readset(read)
    eng.set_reference(lo + 1, text)
    eng.set_hap_left_align(True)
    eng.load_reads(rs)
    # a table must be set for the counts: one far SNV that the read does not reach
    far = np.zeros(1, dtype=HA.to_query(table)[0].dtype)
    far[0]["pos"], far[0]["base_matters"], far[0]["a_base"], far[0]["b_base"] = 5000, 1, 1, 2
    eng.set_phase_alleles(far, np.zeros(1, np.uint8))
    assert _columns(eng, rs, table, text, lo) == want
    # the links of the same read: every pair of sites it shows an allele of (columns 0 / 1)
    q, pool = HA.to_query(table)
    assert np.array_equal(eng.phase_allele_links(q, pool), LA.links(rs, table, LA.observer((text, lo))))
    # and its tag from this table
    eng.set_phase_alleles(q, np.zeros(len(q), np.uint8), pool)
    hp, st, ps = LA.haplotag(rs, table, LA.observer((text, lo)))
    ghp, gst = eng.haplotags()
    assert np.array_equal(ghp, hp) and gst == st and np.array_equal(eng.read_phase_sets(), ps)


def test_plain_and_serial_walk_agree(eng):
    """The two spellings of a read — plain, and with an empty op that sends it down the serial walk — in ONE load give one answer twice."""
    from clair3_rna_amd.reads import ReadSet
    by = {c[0]: c for c in LA.HAND_READS}
    table = [dict(s, h1=0) for s in LA.hand_table()]
    for a, b in (("m_like_run_plain", "m_like_run_serial"), ("ins_rotated_plain", "ins_rotated_serial")):
        assert by[a][3] == by[b][3] and by[a][2][0] == by[b][2][0]
        rs = ReadSet.from_records([dict(pos=by[n][2][0], cigar=by[n][2][1], seq=by[n][2][2], flag=0, mapq=60, hp=0) for n in (a, b)])
        got = _device(eng, rs, table, LA.HAND_REF, True)
        _assert_same(got, _expected(rs, table, LA.observer((LA.HAND_REF, 0))))
        want = np.zeros((len(table), 3), np.uint32)
        for j, col in by[a][3].items():
            want[j, col] = 2
        assert np.array_equal(got["counts"].sum(axis=1), want)


def test_reads_on_the_lane_boundary(eng):
    from clair3_rna_amd.reads import ReadSet
    ref, reads, rows = LA.boundary_reads()
    table = []
    for row in rows:
        table.append(dict(HA.site_of_row(*row), h1=0))
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=0, mapq=60, hp=0) for _, r in reads])
    assert [int(n) for n in rs.reads["n_cigar"]] == [17, 32, 33]
    obs = LA.observer((ref, 0))
    site_at = {s["pos"]: (j, s) for j, s in enumerate(table)}
    for i in range(3):                                       # the deleted A shows on its left-most place, not where the CIGAR has it
        assert LA.observe(rs, i, site_at, (ref, 0)) == {2 * i: 1, 2 * i + 1: 0}
    got = _device(eng, rs, table, ref, True)
    _assert_same(got, _expected(rs, table, obs))
    assert int(got["counts"][:, :, 1].sum()) == 3


# ---- 5. the life cycle of the switch
def test_life_cycle(eng):
    from clair3_rna_amd import capi
    c = _case(0)
    rs, table = c["rs_jit"], c["t_on"]
    q, pool = HA.to_query(table)
    h1 = np.array([s["h1"] for s in table], np.uint8)
    ups, uh1 = _units(table)
    qu = q.copy()
    qu["ps"] = ups
    e = capi.Engine(0)
    try:
        # no reference: the switch itself is accepted, the four calls are refused, and nothing is lost by the refusals
        e.load_reads(rs)
        e.set_hap_left_align(True)
        for call in (lambda: e.set_phase_alleles(q, h1, pool), lambda: e.phase_allele_links(q, pool),
                     lambda: e.phase_allele_unit_links(qu, np.array(uh1, np.uint8), pool)):
            with pytest.raises(capi.C3RError) as err:
                call()
            assert err.value.code == -1 and "no reference is set" in str(err.value)
        e.set_hap_left_align(False)
        e.set_phase_alleles(q, h1, pool)
        off_tags = e.haplotags()[0].copy()
        with pytest.raises(capi.C3RError) as err:            # a table and reads are there: the toggle would tag again
            e.set_hap_left_align(True)
        assert err.value.code == -1 and np.array_equal(e.haplotags()[0], off_tags)
        assert np.array_equal(e.hap_allele_counts(q, pool), LA.allele_counts(rs, *_tags(rs, table, HA.observe), table))      # (still off)
        # with a reference the toggle tags again, both ways
        e.set_reference(1, c["ref"])
        e.set_hap_left_align(True)
        assert np.array_equal(e.haplotags()[0], c["exp_on"]["hp"]) and np.array_equal(e.read_phase_sets(), c["exp_on"]["ps"])
        assert not np.array_equal(off_tags, c["exp_on"]["hp"])
        e.set_hap_left_align(False)
        assert np.array_equal(e.haplotags()[0], off_tags)
        e.set_hap_left_align(True)
        # a load under the switch tags with it; hap_allele_counts without a reference is refused once the slice is gone
        e.load_reads(rs)
        assert np.array_equal(e.haplotags()[0], c["exp_on"]["hp"])
        # n = 0 clears, switch on or not
        e.set_phase_alleles(None, None)
        with pytest.raises(capi.C3RError):
            e.haplotags()
        # the SNV table of set_phase_sites never looks at the switch
        snv = P.make_sites([(s["pos"], s["ref"], s["alt"]) for s in table if s["A"][1] == HA.NONE and s["B"][1] == HA.NONE])
        snv["ps"] = 0
        snv["h1"] = [s["h1"] for s in table if s["A"][1] == HA.NONE and s["B"][1] == HA.NONE]
        e.set_phase_sites(snv)
        on_tags = e.haplotags()[0].copy()
        e.set_hap_left_align(False)
        assert np.array_equal(e.haplotags()[0], on_tags)
    finally:
        e.close()


def _tags(rs, table, obs):
    hp, _, ps = LA.haplotag(rs, table, obs)
    return hp, ps


def test_kernels_by_name(eng):
    """Switched on, each call launches its _la kernel once and the switched-off kernel not at all — and the other way round."""
    c = _case(0)
    eng.set_profiling(True)
    try:
        for on, want, never in ((True, "_la", ""), (False, "", "_la")):
            eng.reset_kernel_stats()
            _device(eng, c["rs_jit"], c["t_on"], c["ref"], on)
            stats = eng.kernel_stats()
            for k in ("k_haplotag_alleles", "k_hap_allele_counts", "k_phase_allele_links", "k_phase_allele_unit_links"):
                assert stats[k + want]["launches"] >= 1 and k + never not in stats, (on, k, sorted(stats))
    finally:
        eng.set_profiling(False)


# ---- 6. the drivers
HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
PS_LINE = '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set identifier">\n'


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """One contig of gen_repeats' jittered reads in an untagged BAM, the unphased pass on it, and `with`: a VCF with an unphased PASS row
    for every SNV and every planted row (at its jittered placement)."""
    tmp = str(tmp_path_factory.mktemp("left_align_drivers"))
    s = write_sample(tmp)
    _call_sample(s, "pass1", [])
    s["pass1"] = os.path.join(tmp, "pass1", "output.vcf.gz")
    assert os.path.isfile(s["pass1"])
    return s


def write_sample(tmp):
    """The sample's input files in `tmp` (ref.fa, plain.bam, with_indels.vcf, model18, model30) and what the tests need beside them."""
    from clair3_rna_amd import bam, bamio, io, synth
    ref, rs, snvs, _, planted, _ = LA.gen_repeats(11, True)
    both = [(p, r, a, "0/1") for p, r, a in snvs] + [(s["pos"], s["ref"], s["alt"], s["gt"]) for s in planted]
    rows = ["chr1\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:GQ\t%s:30\n" % r for r in sorted(both)]
    fa, w18, w30 = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model18"), os.path.join(tmp, "model30")
    io.write_fasta(fa, [("chr1", ref)])
    np.save(w18 + ".c3rw.npy", synth.random_weights(18, seed=5))
    np.save(w30 + ".c3rw.npy", synth.random_weights(30, seed=5))
    bam_fn = os.path.join(tmp, "plain.bam")
    bam.write_bam(bam_fn, [("chr1", len(ref))], {"chr1": rs})
    bamio.index_build(bam_fn)
    s = dict(tmp=tmp, fa=fa, w18=w18, w30=w30, bam=bam_fn, rs=rs, ref=ref, rows=rows, with_=os.path.join(tmp, "with_indels.vcf"))
    with open(s["with_"], "w") as f:
        f.write(HEAD + "".join(rows))
    return s


def _call_sample(s, out, extra, log=None):
    from clair3_rna_amd import call_sample
    argv = ["--bam_fn", s["bam"], "--ref_fn", s["fa"], "--output_dir", os.path.join(s["tmp"], out), "--pileup_model_path", s["w18"],
            "--phased_pileup_model_path", s["w30"], "--chunk_num", "3", "--min_coverage", "2"] + list(extra)
    assert call_sample.Run(call_sample.build_parser().parse_args(argv), log=log or (lambda m: None)) == 0


def _gz(fn):
    with gzip.open(fn, "rt") as f:
        return f.read()


def _bytes(fn):
    with open(fn, "rb") as f:
        return f.read()


def test_phase_vcf_with_the_flag_writes_what_the_restatement_predicts(sample, tmp_path):
    from clair3_rna_amd import phase_vcf
    out = {}
    for flag in (True, False):
        out_dir, msgs = str(tmp_path / ("la" if flag else "plain")), []
        argv = ["--bam_fn", sample["bam"], "--vcf_fn", sample["with_"], "--output_dir", out_dir, "--indels"] + (["--left_align_indels", "--ref_fn", sample["fa"]] if flag else [])
        assert len(phase_vcf.Run(phase_vcf.build_parser().parse_args(argv), log=msgs.append)) == 1 and len(msgs) == 1
        out[flag] = _gz(os.path.join(out_dir, "phased_chr1.vcf.gz"))
        assert ("left-aligned" in msgs[0]) == flag
    cands, skipped = HA.candidates(sample["rows"], "chr1")
    assert len(cands) == len(sample["rows"]) and not any(skipped.values())
    ref = (sample["ref"], 0)
    table, src, dropped, moved = LA.align_sites(cands, ref)
    assert moved > 10 and not any(dropped.values())
    ps, h1, _ = PI.resolve(table, LA.links(sample["rs"], table, LA.observer(ref)))
    decided = {j: (p, h) for j, p, h in zip(src, ps, h1)}
    exp = HEAD.replace("#CHROM", PS_LINE + "#CHROM")
    exp += "".join(HA.rewritten(ln, cands[j], decided[j]) if decided[j][0] >= 0 else ln for j, ln in enumerate(sample["rows"]))
    assert out[True] == exp
    # the rows keep POS, REF and ALT, and more indel rows are phased than without the flag
    event = [j for j, s in enumerate(cands) if HA.flags(s)[1]]
    phased = lambda text: sum(1 for j, ln in enumerate([l for l in text.splitlines() if not l.startswith("#")]) if j in event and "|" in ln.split("\t")[9])
    assert [l.split("\t")[:5] for l in out[True].splitlines() if not l.startswith("#")] == [l.split("\t")[:5] for l in sample["rows"]]
    assert out[True] != out[False] and phased(out[True]) >= 20 and phased(out[True]) > phased(out[False])


def test_call_sample_with_the_flag_equals_the_steps_by_hand(sample):
    from clair3_rna_amd import hap_vcf, haplotag_bam, phase_vcf
    la = ["--left_align_indels", "--ref_fn", sample["fa"]]
    hand = os.path.join(sample["tmp"], "hand")
    hand_dir = os.path.join(hand, "phased_vcf")
    phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", sample["pass1"], "--output_dir", hand_dir, "--indels"] + la), log=lambda m: None)
    msgs = []
    _call_sample(sample, "hand", ["--enable_phasing_model", "--phased_vcf_fn", hand_dir, "--haplotag_indels", "--left_align_indels"], msgs.append)
    assert any("--left_align_indels:" in m and "left-aligned" in m for m in msgs)
    stem = os.path.join(hand, "output_enable_phasing")
    hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", stem + ".vcf.gz", "--phased_vcf_fn", hand_dir, "--output_fn", stem + "_phased.vcf.gz",
                                                   "--hap_counts_fn", stem + "_hap_counts.tsv", "--min_mq", "5", "--indels", "--haplotag_indels"] + la), log=lambda m: None)
    bam_dir = os.path.join(hand, "tmp", "phased_output", "phased_bam")
    haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", sample["bam"], "--phased_vcf_fn", hand_dir, "--output_dir", bam_dir, "--haplotag_indels",
                                                             "--ctg_name", "chr1"] + la), log=lambda m: None)
    _call_sample(sample, "one", ["--enable_phasing_model", "--phasing", "builtin", "--phasing_indels", "--left_align_indels", "--phase_output", "--phase_indels",
                                 "--haplotagged_bam"])
    one = os.path.join(sample["tmp"], "one")
    assert _gz(os.path.join(one, "output.vcf.gz")) == _gz(sample["pass1"])
    assert _gz(os.path.join(one, "tmp", "phased_output", "phased_vcf", "phased_chr1.vcf.gz")) == _gz(os.path.join(hand_dir, "phased_chr1.vcf.gz"))
    for fn in ("output_enable_phasing.vcf.gz", "output_enable_phasing_phased.vcf.gz", "output_enable_phasing_hap_counts.tsv"):
        assert _bytes(os.path.join(one, fn)) == _bytes(os.path.join(hand, fn)), fn
    # (the BAM's @PG line names the command that wrote it: the records and the index are compared)
    from clair3_rna_amd import io
    a, b = io.load_reads(os.path.join(one, "tmp", "phased_output", "phased_bam", "chr1.bam"), "chr1"), io.load_reads(os.path.join(bam_dir, "chr1.bam"), "chr1")
    assert a.reads.tobytes() == b.reads.tobytes() and int((a.reads["hp"] != 0).sum()) > 100


def test_haplotag_bam_with_the_flag_tags_by_the_left_aligned_table(sample, tmp_path):
    """A phased VCF whose indel rows sit anywhere in their repeats (phase_vcf --indels --left_align_indels on the VCF with the planted rows):
    haplotag_bam under the flag writes the tags the restatement gives for the left-aligned table, and other tags without it."""
    from clair3_rna_amd import haplotag_bam, io, phase_vcf, phasedvcf
    la = ["--left_align_indels", "--ref_fn", sample["fa"]]
    phased_dir = str(tmp_path / "phased_vcf")
    phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", sample["with_"], "--output_dir", phased_dir, "--indels"] + la), log=lambda m: None)
    hp = {}
    for flag in (True, False):
        out_dir, msgs = str(tmp_path / ("bam_%d" % flag)), []
        haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", sample["bam"], "--phased_vcf_fn", phased_dir, "--output_dir", out_dir, "--haplotag_indels"]
                                                                + (la if flag else [])), log=msgs.append)
        hp[flag] = io.load_reads(os.path.join(out_dir, "chr1.bam"), "chr1").reads["hp"].copy()
        assert ("--left_align_indels:" in msgs[-1]) == flag
    # the restatement: the phased rows as sites (h1 and ps from GT and PS), left-aligned, under the left-aligned observation
    rows = [l.split("\t") for l in _gz(os.path.join(phased_dir, "phased_chr1.vcf.gz")).splitlines() if not l.startswith("#")]
    sites = []
    for f in rows:
        gt, ps = f[9].split(":")[0], f[9].split(":")[-1]
        if "|" in gt:
            sites.append(dict(HA.site_of_row(int(f[1]), f[3], f[4], gt.replace("|", "/"), int(ps)), h1=1 if gt in ("1|0", "2|1") else 0))
    ref = (sample["ref"], 0)
    table, _, dropped, moved = LA.align_sites(sites, ref)
    assert moved > 10 and not any(dropped.values())
    want, _, _ = LA.haplotag(sample["rs"], table, LA.observer(ref))
    assert np.array_equal(hp[True], want) and not np.array_equal(hp[False], want) and int((want != 0).sum()) > 100
    t = phasedvcf.PhaseSource(phased_dir, True, None, io.contig_reference(sample["fa"])).table("chr1")
    assert list(t.pos) == [s["pos"] for s in table]


def test_without_the_flag_every_driver_writes_the_parent_commits_bytes(sample, tmp_path):
    """tests/golden/left_align_parent_bytes.json: the hashes tests/support/driver_bytes.py gave with the PARENT commit's package on these
    input files (the files are made by this tree's generator, which is all of this commit that took part)."""
    import json
    from tests.support import driver_bytes
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "left_align_parent_bytes.json")) as f:
        want = json.load(f)
    got = driver_bytes.hashes(sample["tmp"], str(tmp_path))
    assert sorted(got) == sorted(want["hashes"]) and len(got) == 11
    assert got == want["hashes"], [k for k in got if got[k] != want["hashes"][k]]


def test_call_var_bam_under_the_flag_scans_the_same_bytes(sample, tmp_path):
    """A table without indels, with and without the flag: the reference is fetched for the whole contig under it, and the chunk's VCF is
    the same file."""
    from clair3_rna_amd import call_var_bam, phase_vcf
    snv_dir = str(tmp_path / "snv_only")
    phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", sample["pass1"], "--output_dir", snv_dir]), log=lambda m: None)
    got = {}
    for flag in (False, True):
        fn = str(tmp_path / ("chunk_%d.vcf" % flag))
        argv = ["--chkpnt_fn", sample["w30"], "--bam_fn", sample["bam"], "--ref_fn", sample["fa"], "--call_fn", fn, "--ctgName", "chr1", "--pileup", "--chunk_id", "2",
                "--chunk_num", "3", "--minCoverage", "2", "--enable_phasing_model", "True", "--phased_vcf_fn", snv_dir, "--haplotag_indels"] + (["--left_align_indels"] if flag else [])
        call_var_bam.Run(call_var_bam.build_parser().parse_args(argv))
        got[flag] = _bytes(fn)
    assert got[True] == got[False] and got[True].count(b"\nchr1\t") > 5
