"""Haplotagging on the device (c3r_set_phase_sites / k_haplotag) against tests/hapref.py, the plain-Python restatement of the rule, and
— for what the tags are for — the 30-channel tensor build against the oracle run on records that carry hapref's tags."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hapref
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=60, hp=0) for r in recs])


def _check(eng, rs, sites):
    """The engine's tags and statistics for (rs, sites) equal hapref's; returns (tags, stats, phase sets per read)."""
    exp, st, n_ps = hapref.haplotag(rs, sites)
    eng.set_phase_sites(sites)
    eng.load_reads(rs)
    got, gst = eng.haplotags()
    assert got.tolist() == exp.tolist(), np.nonzero(got != exp)[0][:10]
    assert gst == st
    return exp, st, n_ps


# ---- 1. known answers
@pytest.mark.parametrize("case", hapref.CASES, ids=[c[0] for c in hapref.CASES])
def test_known_answers(eng, case):
    rs, sites = hapref.case_inputs(case)
    eng.set_phase_sites(sites)
    eng.load_reads(rs)
    hp, st = eng.haplotags()
    assert hp.tolist() == [e[0] for e in case[3]]
    assert st["n_reads"] == len(rs) and st["n_hp1"] == sum(e[0] == 1 for e in case[3]) and st["n_hp2"] == sum(e[0] == 2 for e in case[3])
    assert st["n_tie"] == sum(e[0] == 0 and e[1] + e[2] > 0 for e in case[3]) and st["n_no_vote"] == sum(e[1] + e[2] == 0 for e in case[3])


@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_read_counts_around_a_workgroup(eng, n):
    """16 reads make a workgroup: the last read of one, the first of the next, and a lone read, each with an answer of its own."""
    seqs = ["AAAA", "CCCC", "ACAC", "GGGG", "AACA"]             # 1, 2, tie, no vote, 1
    rs = _readset([(k // 3, "4M", seqs[k % 5]) for k in range(n)])
    sites = hapref.make_sites([(p, "A", "C", 0, 1) for p in (3, 4, 5, 6, 7, 8)])
    exp, st, _ = _check(eng, rs, sites)
    if n >= 15:
        assert st["n_hp1"] and st["n_hp2"] and st["n_tie"] and st["n_no_vote"]


def test_forty_ops_with_sites_where_the_lane_round_changes(eng):
    """Ops 0-15 are the first round of the 16 lanes, 16-31 the second: sites in ops 15, 16 and 17 (and nowhere else), every op M-like so that
    the CIGAR takes the parallel walk; then the same with insertions, deletions and ref-skips between the runs."""
    for sep in (None, ["2I", "3D", "7N"]):
        ops, starts, x, seq = [], [], 100, []
        for k in range(40):
            ln = 2 + k % 3
            ops.append("%d%s" % (ln, "M=X"[k % 3]))
            starts.append((k, x, len(seq)))
            seq += ["ACGT"[(k + j) % 4] for j in range(ln)]
            x += ln
            if sep and k < 39:
                s = sep[k % 3]
                ops.append(s)
                if s[-1] == "I":
                    seq += ["T"] * int(s[:-1])
                else:
                    x += int(s[:-1])
        step = 2 if sep else 1                                   # (with separators the M runs are the even ops: runs 15, 16, 17 = ops 30, 32, 34;
        want = [15, 16, 17] if not sep else [7, 8, 9]            #  there the lane round changes between M runs 7 and 8 = ops 14 and 16)
        rows = []
        for k, x0, q0 in starts:
            if k in want:
                b = seq[q0]
                rows.append((x0 + 1, b, "ACGT"[("ACGT".index(b) + 1) % 4], k % 2, 3))
        assert len(ops) == (40 if not sep else 79) and all(o * step < len(ops) for o in want)
        rs = _readset([(100, "".join(ops), "".join(seq))])
        exp, st, _ = _check(eng, rs, hapref.make_sites(rows))
        assert st["n_votes"] == 3 and exp[0] in (1, 2)


@pytest.mark.parametrize("cigar", ["4M1P4M", "4M0D4M", "4M2H4M", "2S3M0I2M1P1D2M", "8M0M"])
def test_cigars_that_take_the_serial_walk(eng, cigar):
    seq = "ACGTACGTAC"
    rows = [(p, "ACGT"[(p - 11) % 4], "ACGT"[(p - 10) % 4], p % 2, 1 + p % 2) for p in range(9, 22)]
    rs = _readset([(10, cigar, seq), (10, "8M", seq), (12, cigar, seq, 16)])
    exp, st, _ = _check(eng, rs, hapref.make_sites(rows))
    assert st["n_votes"] >= 6


@pytest.mark.parametrize("n_sets", [9, 20])
def test_a_read_that_sees_many_phase_sets(eng, n_sets):
    """Set k (numbered so that neither the order of the numbers nor the order of the sites is the order of the votes) holds 1 + (k * 7) % 5 sites;
    the sets interleave along the read.  A second read sees the same sets through the serial walk."""
    import random
    rng = random.Random(n_sets)
    owners = [k for k in range(n_sets) for _ in range(1 + (k * 7) % 5)]
    rng.shuffle(owners)
    number = rng.sample(range(100, 100000), n_sets)
    seq = "".join(rng.choice("ACGT") for _ in range(2 * len(owners) + 4))
    rows = []
    for j, k in enumerate(owners):
        b = seq[2 * j + 1]
        rows.append((50 + 2 * j + 2, b, "ACGT"[("ACGT".index(b) + 1 + j % 3) % 4], rng.randint(0, 1), number[k]))
    half = len(seq) // 2
    rs = _readset([(50, "%dM" % len(seq), seq), (50, "%dM0I%dM" % (half, len(seq) - half), seq)])
    exp, st, n_ps = _check(eng, rs, hapref.make_sites(rows))
    assert n_ps.tolist() == [n_sets, n_sets] and st["n_votes"] == 2 * len(owners)


def test_no_site_in_the_span_and_an_empty_read_set(eng):
    rs = _readset([(100, "50M", "A" * 50), (100, "20M1000N30M", "A" * 50), (400, "5M", "AAAAA")])
    sites = hapref.make_sites([(50, "A", "C", 0, 1), (100, "A", "C", 0, 1), (600, "A", "C", 0, 1), (1171, "A", "C", 0, 1)])
    exp, st, _ = _check(eng, rs, sites)
    assert exp.tolist() == [0, 0, 0] and st["n_no_vote"] == 3 and st["n_votes"] == 0
    from clair3_rna_amd.reads import ReadSet
    eng.load_reads(ReadSet.from_records([]))
    hp, st = eng.haplotags()
    assert len(hp) == 0 and st == dict.fromkeys(hapref.STAT_KEYS, 0)


# ---- 2. generated cases
def _gen(seed):
    if ("gen", seed) not in _state:
        ref, rs, sites, truth = hapref.gen_case(seed)
        _state[("gen", seed)] = (ref, rs, sites, truth) + hapref.haplotag(rs, sites)
    return _state[("gen", seed)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_generated_cases(eng, seed):
    ref, rs, sites, truth, exp, st, n_ps = _gen(seed)
    assert st["n_hp1"] >= 100 and st["n_hp2"] >= 100 and st["n_no_vote"] >= 5 and st["n_tie"] >= 1 and int((n_ps >= 9).sum()) >= 1, st
    _check(eng, rs, sites)


# ---- 3. ordering and clearing
def test_sites_before_or_after_the_reads_and_new_filters_keep_the_tags(eng):
    ref, rs, sites, truth, exp, st, _ = _gen(1)
    rs = hapref.with_hp(rs, 0)
    rs.reads["mapq"][1::2] = 10                                  # (every read votes, whatever its mapping quality)
    eng.set_phase_sites(sites)
    eng.load_reads(rs)
    before = eng.haplotags()
    eng.set_phase_sites(None)
    eng.load_reads(rs)
    eng.set_phase_sites(sites)
    after = eng.haplotags()
    assert before[0].tolist() == after[0].tolist() == exp.tolist() and before[1] == after[1] == st
    eng.set_params(min_mq=20, excl_flags=16)                     # most reads fail the filters now: the tags are the same
    again = eng.haplotags()
    assert again[0].tolist() == exp.tolist() and again[1] == st
    eng.load_reads(rs)                                           # the table stays for later loads
    assert eng.haplotags()[0].tolist() == exp.tolist()


def _phased_case(seed, n_sites=40):
    """helpers._case(seed, phased=True): (ref, ReadSet with the records' own hp, the same with hp = 0, 40 random sites on covered positions)."""
    import random
    from clair3_rna_amd.reads import ReadSet
    key = ("case", seed)
    if key not in _state:
        ref, recs = H._case(seed, phased=True)
        rs = ReadSet.from_records(recs)
        rng = random.Random(77000 + seed)
        covered = set()
        for r in recs:
            covered.update(range(r["pos"] + 1, r["pos"] + H.cigar_ref_len(r["cigar"]) + 1))
        rows = []
        for p in sorted(rng.sample(sorted(covered), min(n_sites, len(covered)))):
            a, b = rng.sample("ACGT", 2)
            rows.append((p, a, b, rng.randint(0, 1), rng.choice([5, 5, 5, 9, 2])))
        _state[key] = (ref, rs, hapref.with_hp(rs, 0), hapref.make_sites(rows))
    return _state[key]


def _oracle30(rs, ref, **kw):
    return H.oracle_chunk(rs, ref, 1, 1, len(ref), channels=30, min_coverage=2, **kw)


def test_clearing_the_sites_brings_back_the_records_own_tags(eng):
    ref, rs_own, _, sites = _phased_case(4100)
    tags, _, _ = hapref.haplotag(rs_own, sites)
    assert set(rs_own.reads["hp"].tolist()) == {0, 1, 2} and (tags != rs_own.reads["hp"]).sum() > 5
    eng.set_params(channels=30, min_coverage=2)
    eng.set_phase_sites(sites)
    got = H.engine_chunk(eng, rs_own, ref, 1, 1, len(ref))
    exp = _oracle30(hapref.with_hp(rs_own, tags), ref)
    own = _oracle30(rs_own, ref)
    assert exp["lines"] != own["lines"] and len(own["lines"]) > 20
    assert got["lines"] == exp["lines"], H.first_diff(got["lines"], exp["lines"])
    eng.set_phase_sites(None)                                    # the loaded reads are rebuilt with their records' hp
    n = eng.scan(1, len(ref))
    from clair3_rna_amd import altinfo
    lines = altinfo.format_lines(H.CTG, eng.sites(), eng.tensors(rescaled=False), eng.tokens(), rs_own, ref.upper(), 1, padins=eng.pad_insertions())
    assert n == len(own["lines"]) and lines == own["lines"], H.first_diff(lines, own["lines"])
    got = H.engine_chunk(eng, rs_own, ref, 1, 1, len(ref))       # and so is a fresh load
    assert got["lines"] == own["lines"]


def test_nothing_runs_without_sites(eng):
    from clair3_rna_amd import capi
    ref, rs, sites, *_ = _gen(0)
    eng.set_profiling(True)
    try:
        eng.reset_kernel_stats()
        eng.load_reads(rs)
        ks = eng.kernel_stats()
        assert "k_prep_count" in ks and not [k for k in ks if "haplotag" in k], ks
        with pytest.raises(capi.C3RError, match="no phase sites"):
            eng.haplotags()
        eng.set_phase_sites(sites)
        assert eng.kernel_stats()["k_haplotag"]["launches"] == 1
        eng.set_phase_sites(None)
        eng.reset_kernel_stats()
        eng.load_reads(rs)
        assert not [k for k in eng.kernel_stats() if "haplotag" in k]
        with pytest.raises(capi.C3RError, match="no phase sites"):
            eng.haplotags()
    finally:
        eng.set_profiling(False)


BAD_SITES = [
    ("unsorted", [(10, "A", "C", 0, 1), (30, "A", "C", 0, 1), (20, "A", "C", 0, 1)], {}, 2),
    ("duplicate", [(10, "A", "C", 0, 1), (10, "A", "G", 0, 1)], {}, 1),
    ("pos_below_1", [(0, "A", "C", 0, 1)], {}, 0),
    ("bad_ref_code", [(5, "A", "C", 0, 1), (6, "A", "C", 0, 1)], dict(ref=3), 1),
    ("bad_alt_code", [(5, "A", "C", 0, 1), (6, "A", "C", 0, 1), (7, "A", "C", 0, 1), (8, "A", "C", 0, 1)], dict(alt=15), 3),
    ("zero_code", [(5, "A", "C", 0, 1)], dict(alt=0), 0),
    ("ref_is_alt", [(5, "A", "C", 0, 1), (6, "G", "G", 0, 1)], {}, 1),
    ("h1_above_1", [(5, "A", "C", 0, 1), (6, "A", "C", 0, 1), (7, "A", "C", 2, 1)], {}, 2),
]


@pytest.mark.parametrize("name, rows, patch, index", BAD_SITES, ids=[b[0] for b in BAD_SITES])
def test_bad_site_tables_name_the_index(eng, name, rows, patch, index):
    from clair3_rna_amd import capi
    good = hapref.make_sites([(3, "A", "C", 0, 1)])
    rs = _readset([(0, "4M", "AAAA")])
    eng.set_phase_sites(good)
    eng.load_reads(rs)
    a = hapref.make_sites(rows)
    for k, v in patch.items():
        a[k][index] = v
    with pytest.raises(capi.C3RError, match=r"phase site %d\b.*EINVAL" % index):
        eng.set_phase_sites(a)
    assert eng.haplotags()[0].tolist() == [1]                    # the table that was there is still in force


def test_records_out_of_range_fail_as_before(eng):
    from clair3_rna_amd import capi
    ref, rs, sites, *_ = _gen(2)
    bad = hapref.with_hp(rs, 0)
    bad.reads["cigar_off"][37] = len(bad.cigar) + 5
    eng.set_phase_sites(sites)
    with pytest.raises(capi.C3RError, match="cigar range of read 37 out of bounds"):
        eng.load_reads(bad)
    bad = hapref.with_hp(rs, 0)
    bad.reads["seq_off"][5] = len(bad.seq)
    with pytest.raises(capi.C3RError, match="seq range of read 5 out of bounds"):
        eng.load_reads(bad)
    _check(eng, rs, sites)                                       # and the context goes on


# ---- 4. tensor parity, 30 channels
PARITY = [dict(), dict(mpileup_compat=1), dict(head_tail=1, splice_padding=1)]


@pytest.mark.parametrize("kw", PARITY, ids=["compat0", "compat1", "head_tail_splice_padding"])
def test_thirty_channel_lines_equal_the_oracle_on_tagged_records(eng, kw):
    """Pile records (PileRec::w), DevRead and — on the columns whose haplotype channels depend on the reads' order — the legacy tables of the
    ordered recompute all take the tag the kernel wrote."""
    n_lines = n_tagged = 0
    for seed in range(4200, 4212):
        ref, _, rs0, sites = _phased_case(seed)
        tags, st, _ = hapref.haplotag(rs0, sites)
        okw = {k: bool(v) if k != "mpileup_compat" else v for k, v in kw.items()}
        exp = _oracle30(hapref.with_hp(rs0, tags), ref, **okw)
        eng.set_params(channels=30, min_coverage=2, **kw)
        eng.set_phase_sites(sites)
        try:
            got = H.engine_chunk(eng, rs0, ref, 1, 1, len(ref))
        except Exception as e:                                   # (the pad table's documented limit, as in helpers.fuzz_samtools_1_11)
            assert kw.get("mpileup_compat") and "more than 64 characters" in str(e), (seed, e)
            continue
        assert eng.haplotags()[0].tolist() == tags.tolist()
        assert got["lines"] == exp["lines"], (seed, H.first_diff(got["lines"], exp["lines"]))
        assert np.array_equal(got["X"], exp["X"])
        if st["n_hp1"] + st["n_hp2"] > 0:
            assert exp["lines"] != _oracle30(rs0, ref, **okw)["lines"], seed          # the tags show in the lines
        n_lines += len(exp["lines"])
        n_tagged += st["n_hp1"] + st["n_hp2"]
    assert n_lines > 800 and n_tagged > 150, (n_lines, n_tagged)


def test_a_deep_locus(eng):
    """2,100 reads over three sites: the span goes to the deep-span kernel, whose records carry the tags like any other.  The reads are 70M
    from 0-based 165..173, so that every site's 33-column window (1-based 189 .. 232) is covered and each site gives a candidate line."""
    import random
    from clair3_rna_amd.reads import ReadSet
    rng = random.Random(5)
    ref = "".join(rng.choice("ACGT") for _ in range(500))
    rows = [(p, ref[p - 1], "ACGT"[("ACGT".index(ref[p - 1]) + 1) % 4], h1, 4) for p, h1 in ((205, 0), (210, 1), (216, 0))]
    recs = []
    for k in range(2100):
        hap = rng.randint(1, 2)
        p0 = 165 + rng.randint(0, 8)
        seq = list(ref[p0:p0 + 70])
        for p, rb, ab, h1, _ in rows:
            if (h1 == 1) == (hap == 1):
                seq[p - 1 - p0] = ab
        for j in range(len(seq)):
            if rng.random() < 0.03:
                seq[j] = rng.choice("ACGT")
        recs.append(dict(pos=p0, cigar="70M", seq="".join(seq), flag=16 * rng.randint(0, 1), mapq=60, hp=0))
    rs = ReadSet.from_records(recs)
    sites = hapref.make_sites(rows)
    tags, st, _ = hapref.haplotag(rs, sites)
    assert st["n_hp1"] > 900 and st["n_hp2"] > 900
    exp = _oracle30(hapref.with_hp(rs, tags), ref)
    eng.set_params(channels=30, min_coverage=2)
    eng.set_phase_sites(sites)
    got = H.engine_chunk(eng, rs, ref, 1, 1, len(ref))
    c = eng.scan_counts()
    assert c["deep"] >= 1, c
    assert eng.haplotags()[1] == st
    assert got["lines"] == exp["lines"] and len(exp["lines"]) >= 3, H.first_diff(got["lines"], exp["lines"])
    assert np.array_equal(got["X"], exp["X"])


# ---- 5. drivers: the untagged BAM plus the phased VCF equals the BAM tagged by hapref
@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """Two contigs of gen_case reads, written twice — untagged, and tagged by hapref — with the phased VCF (one file, and a directory of
    phased_<ctg>.vcf.gz); and what call_sample makes of the TAGGED BAM without any VCF."""
    import gzip
    from clair3_rna_amd import bam, bamio, call_sample, io, synth
    from clair3_rna_amd.reads import NT16
    tmp = str(tmp_path_factory.mktemp("haplotag_drivers"))
    contigs, plain, tagged, vcf_rows = [], {}, {}, {}
    for name, seed in (("chr1", 11), ("chr2", 12)):
        ref, rs, sites, _ = hapref.gen_case(seed)
        tags, st, _ = hapref.haplotag(rs, sites)
        assert st["n_hp1"] > 100 and st["n_hp2"] > 100
        contigs.append((name, ref))
        plain[name], tagged[name] = rs, hapref.with_hp(rs, tags)
        vcf_rows[name] = ["%s\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s:%d" % (name, s["pos"], NT16[s["ref"]], NT16[s["alt"]], "1|0" if s["h1"] else "0|1", s["ps"])
                          for s in sites]
    fa, wfn = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model")
    io.write_fasta(fa, contigs)
    np.save(wfn + ".c3rw.npy", synth.random_weights(30, seed=5))
    bams = {}
    for kind, reads in (("plain", plain), ("tagged", tagged)):
        bams[kind] = os.path.join(tmp, kind + ".bam")
        bam.write_bam(bams[kind], [(n, len(r)) for n, r in contigs], reads)
        bamio.index_build(bams[kind])
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    one = os.path.join(tmp, "phased.vcf")
    with open(one, "w") as f:
        f.write(head + "".join(r + "\n" for n, _ in contigs for r in vcf_rows[n]))
    per = os.path.join(tmp, "phased_vcf")
    os.makedirs(per)
    for n, _ in contigs:
        with gzip.open(os.path.join(per, "phased_%s.vcf.gz" % n), "wt") as f:
            f.write(head + "".join(r + "\n" for r in vcf_rows[n]))
    s = dict(tmp=tmp, fa=fa, wfn=wfn, bams=bams, one=one, per=per)
    s["tagged_out"] = open(_call_sample(s, "tagged_out", "tagged")).read()
    recs = [r for r in s["tagged_out"].split("\n") if r and r[0] != "#"]
    assert len(recs) > 30 and {r.split("\t")[0] for r in recs} == {"chr1", "chr2"}
    return s


def _call_sample(s, out, kind, extra=()):
    from clair3_rna_amd import call_sample
    argv = ["--bam_fn", s["bams"][kind], "--ref_fn", s["fa"], "--output_dir", os.path.join(s["tmp"], out), "--pileup_model_path", s["wfn"],
            "--phased_pileup_model_path", s["wfn"], "--enable_phasing_model", "--chunk_num", "3", "--no_compress", "--min_coverage", "2"] + list(extra)
    assert call_sample.Run(call_sample.build_parser().parse_args(argv)) == 0
    return os.path.join(s["tmp"], out, "output_enable_phasing.vcf")


def test_call_sample_with_a_phased_vcf_equals_the_tagged_bam(sample):
    got = open(_call_sample(sample, "vcf_out", "plain", ["--phased_vcf_fn", sample["one"]])).read()
    assert got == sample["tagged_out"]
    untagged = open(_call_sample(sample, "untagged_out", "plain")).read()
    assert untagged != sample["tagged_out"]                      # the tags show in the records: the comparison above can fail


def test_call_sample_with_a_directory_of_phased_vcfs(sample):
    got = open(_call_sample(sample, "dir_out", "plain", ["--phased_vcf_fn", sample["per"], "--contexts", "1", "--fetch_threads", "2"])).read()
    assert got == sample["tagged_out"]


def test_per_chunk_calls_with_the_whole_contigs_sites(sample):
    """call_var_bam per CHUNK_LIST row (three chunks per contig) + sort_vcf: a chunk's reads are tagged from the whole contig's sites, so a
    read that reaches across a chunk border carries the same tag in both chunks."""
    from tests.test_gpu_sample import _reference_flow
    flow = os.path.join(sample["tmp"], "flow")
    os.makedirs(flow)
    exp = _reference_flow(flow, sample["fa"], sample["bams"]["plain"], sample["wfn"], os.path.join(sample["tmp"], "tagged_out"),
                          extra_chunk=["--phased_vcf_fn", sample["one"], "--minCoverage", "2"], phased=True)
    assert open(exp).read() == sample["tagged_out"]
    rows = [r.split() for r in open(os.path.join(sample["tmp"], "tagged_out", "tmp", "CHUNK_LIST"))]
    assert rows == [[c, str(k), "3"] for c in ("chr1", "chr2") for k in (1, 2, 3)]


def test_a_phased_vcf_without_the_phasing_model_is_refused(sample, tmp_path):
    from clair3_rna_amd import call_sample, call_var_bam
    argv = ["--bam_fn", sample["bams"]["plain"], "--ref_fn", sample["fa"], "--output_dir", str(tmp_path), "--pileup_model_path", sample["wfn"],
            "--phased_vcf_fn", sample["one"]]
    with pytest.raises(SystemExit) as e:
        call_sample.Run(call_sample.build_parser().parse_args(argv))
    assert "[ERROR]" in str(e.value.code) and "--enable_phasing_model" in str(e.value.code)
    argv = ["--chkpnt_fn", sample["wfn"], "--bam_fn", sample["bams"]["plain"], "--ref_fn", sample["fa"], "--ctgName", "chr1", "--pileup",
            "--phased_vcf_fn", sample["one"]]
    with pytest.raises(SystemExit) as e:
        call_var_bam.Run(call_var_bam.build_parser().parse_args(argv))
    assert "[ERROR]" in str(e.value.code) and "--enable_phasing_model" in str(e.value.code)
    # as a command: a non-zero exit status and the line on stderr
    r = subprocess.run([sys.executable, "-m", "clair3_rna_amd.call_var_bam"] + argv, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "[ERROR] --phased_vcf_fn" in r.stderr
