"""--hap_min_bq without a GPU: the qualities' way from a BAM file into a ReadSet (csrc/bamio.cpp: c3r_bam_want_quals / c3r_bam_copy_quals, and
the pure-Python reader) and back (bam.write_bam), the plain-Python restatement tests/qualref.py on hand cases, the bytes of a BAM written
without qualities against the parent commit's, and the flag's way through the five drivers with a logging fake engine."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest

from clair3_rna_amd import bam, bamio, call_sample, call_var_bam, capi, hap_vcf, haplotag_bam, io, phase_vcf, phasing
from clair3_rna_amd.reads import ReadSet, pack_seq
from tests import qualref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 2, 15, 16, 17, 33)


def _records():
    """One read per length of LENGTHS with qualities, one without, one whose qualities are a phred+33 string."""
    recs = []
    for k, L in enumerate(LENGTHS):
        seq = "".join("ACGT"[(k + j) % 4] for j in range(L))
        recs.append(dict(pos=10 * k, cigar="%dM" % L if L else "3D", seq=seq, qual=[(7 * j + k) % 94 for j in range(L)]))
    recs.append(dict(pos=200, cigar="9M", seq="ACGTACGTA"))                                # no qualities: 0xff throughout
    recs.append(dict(pos=210, cigar="4M", seq="ACGT", qual="!+5I"))                        # phred+33: 0, 10, 20, 40
    return recs


def _exit_text(fn, *a, **kw):
    with pytest.raises(SystemExit) as e:
        fn(*a, **kw)
    return str(e.value)


# ---- the container
def test_from_records_lays_the_qualities_out():
    rs = ReadSet.from_records(_records())
    assert QR.layout_ok(rs) and len(rs.qual) == 2 * len(rs.seq)
    for i, L in enumerate(LENGTHS):
        assert [QR.qual_at(rs, i, j) for j in range(L)] == [(7 * j + i) % 94 for j in range(L)]
    assert [QR.qual_at(rs, 7, j) for j in range(9)] == [0xff] * 9 and [QR.qual_at(rs, 8, j) for j in range(4)] == [0, 10, 20, 40]
    assert ReadSet.from_records([dict(pos=0, cigar="2M", seq="AC")]).qual is None          # no record has any: absent
    with pytest.raises(ValueError):
        ReadSet.from_records([dict(pos=0, cigar="2M", seq="AC", qual=[1])])
    with pytest.raises(ValueError):
        ReadSet(rs.reads, rs.cigar, rs.seq, rs.qual[:-1])


def test_the_restatement_on_hand_cases():
    # bases A C G T A, qualities 9 10 0 93 0xff: under Q = 10 the first and the third are masked, under Q = 93 all but T and the last
    rs = ReadSet.from_records([dict(pos=0, cigar="5M", seq="ACGTA", qual=[9, 10, 0, 93, 0xff])])
    m, n = QR.mask(rs, 0)
    assert n == 0 and list(m) == [0x12, 0x48, 0x10]
    m, n = QR.mask(rs, 10)
    assert n == 2 and list(m) == [0xf2, 0xf8, 0x10]
    m, n = QR.mask(rs, 93)
    assert n == 3 and list(m) == [0xff, 0xf8, 0x10]
    m, n = QR.mask(rs, 1)
    assert n == 1 and list(m) == [0x12, 0xf8, 0x10]
    wn = QR.with_n(rs, 10)
    assert wn.qual is None and wn.read_bases(0, 0, 5) == "NCNTA" and wn.reads.tobytes() == rs.reads.tobytes()
    assert list(rs.seq) == list(pack_seq("ACGTA"))                                       # the input is left alone


# ---- BAM -> ReadSet -> BAM
@pytest.fixture(scope="module")
def qual_bam(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("hap_min_bq_bam"))
    rs = ReadSet.from_records(_records())
    fn = os.path.join(tmp, "q.bam")
    bam.write_bam(fn, [("chr1", 1000)], {"chr1": rs})
    return types.SimpleNamespace(tmp=tmp, fn=fn, rs=rs)


def _same(a, b):
    return a.reads.tobytes() == b.reads.tobytes() and a.cigar.tobytes() == b.cigar.tobytes() and a.seq.tobytes() == b.seq.tobytes()


@pytest.mark.parametrize("indexed", [False, True])
def test_qual_round_trip(qual_bam, indexed, tmp_path):
    fn = str(tmp_path / "q.bam")
    shutil.copy(qual_bam.fn, fn)
    if indexed:
        bamio.index_build(fn)
    with bamio.BamFile(fn) as bf:
        plain = bf.fetch("chr1")
        got = bf.fetch("chr1", want_quals=True)
        part = bf.fetch("chr1", 195, 1000, want_quals=True)
    assert plain.qual is None and _same(plain, qual_bam.rs) and _same(got, qual_bam.rs)
    assert QR.layout_ok(got) and got.qual.tobytes() == qual_bam.rs.qual.tobytes()
    assert list(part.reads["pos"]) == [200, 210] and QR.layout_ok(part) and [QR.qual_at(part, 1, j) for j in range(4)] == [0, 10, 20, 40]
    py = bam.read_contig(fn, "chr1", want_quals=True)
    assert bam.read_contig(fn, "chr1").qual is None and _same(py, qual_bam.rs) and py.qual.tobytes() == qual_bam.rs.qual.tobytes()
    assert io.load_reads(fn, "chr1").qual is None and io.load_reads(fn, "chr1", want_quals=True).qual.tobytes() == got.qual.tobytes()
    # and a second trip writes the same file
    again = str(tmp_path / "again.bam")
    bam.write_bam(again, [("chr1", 1000)], {"chr1": got})
    with open(again, "rb") as f, open(qual_bam.fn, "rb") as g:
        assert f.read() == g.read()


def test_copy_quals_without_want_quals_is_refused(qual_bam):
    L = bamio.load_library()
    with bamio.BamFile(qual_bam.fn) as bf:
        n, nc, ns = C.c_int64(), C.c_int64(), C.c_int64()
        assert L.c3r_bam_fetch(bf.h, b"chr1", 0, 0, C.byref(n), C.byref(nc), C.byref(ns)) == 0
        buf = np.zeros(2 * ns.value + 1, np.uint8)
        assert L.c3r_bam_copy_quals(bf.h, buf.ctypes.data) == -1 and b"c3r_bam_want_quals" in L.c3r_bam_last_error(bf.h) and not buf.any()
        assert L.c3r_bam_want_quals(bf.h, 1) == 0 and L.c3r_bam_copy_quals(bf.h, buf.ctypes.data) == -1        # still the old fetch
        assert L.c3r_bam_fetch(bf.h, b"chr1", 0, 0, C.byref(n), C.byref(nc), C.byref(ns)) == 0
        assert L.c3r_bam_copy_quals(bf.h, buf.ctypes.data) == 0 and buf[:-1].tobytes() == qual_bam.rs.qual.tobytes() and buf[-1] == 0


def test_long_cigar_record_keeps_its_qualities(tmp_path):
    """A CG:B,I record (the real CIGAR behind the placeholder), an odd record before it and an even one behind."""
    M, I, N, S = 0, 1, 3, 4
    op = lambda ln, o: (ln << 4) | o
    real = [op(3, M), op(1, I), op(2, M), op(50, N), op(5, M)]

    def rec(pos, cig, L, aux, k):
        codes = [(1, 2, 4, 8)[(j + k) % 4] for j in range(L)]
        packed = bytearray((L + 1) // 2)
        for j, c in enumerate(codes):
            packed[j >> 1] |= c << (0 if j & 1 else 4)
        body = struct.pack("<iiBBHHHiiii", 0, pos, 2, 60, 0, len(cig), 0, L, -1, -1, 0) + b"q\x00" + np.asarray(cig, "<u4").tobytes() + bytes(packed) \
            + bytes((11 * j + k) % 94 for j in range(L)) + aux
        return struct.pack("<i", len(body)) + body
    text = "@HD\tVN:1.6\tSO:coordinate\n"
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", 3) + b"c1\x00" + struct.pack("<i", 100000)
    out += rec(100, [op(7, M)], 7, b"", 0)
    out += rec(150, [op(11, S), op(60, N)], 11, b"CGBI" + struct.pack("<I", len(real)) + np.asarray(real, "<u4").tobytes() + b"HPC\x01", 1)
    out += rec(160, [op(8, M)], 8, b"", 2)
    fn = str(tmp_path / "cg.bam")
    with open(fn, "wb") as f:
        bam._bgzf_write(f, out)
        f.write(bam._BGZF_EOF)
    with bamio.BamFile(fn) as bf:
        got = bf.fetch("c1", want_quals=True)
    assert list(got.reads["n_cigar"]) == [1, 5, 1] and list(got.reads["l_seq"]) == [7, 11, 8] and QR.layout_ok(got)
    for i, L in enumerate((7, 11, 8)):
        assert [QR.qual_at(got, i, j) for j in range(L)] == [(11 * j + i) % 94 for j in range(L)]
    py = bam.read_contig(fn, "c1", want_quals=True)
    assert py.qual.tobytes() == got.qual.tobytes() and _same(py, got)


def test_a_bam_without_qualities_has_the_parent_commits_bytes(tmp_path):
    """tests/golden/hap_min_bq_parent_bytes.json: what tests/support/bam_bytes.py gave with the PARENT commit's package."""
    from tests.support import bam_bytes
    with open(os.path.join(ROOT, "tests", "golden", "hap_min_bq_parent_bytes.json")) as f:
        want = json.load(f)["hashes"]
    assert bam_bytes.bam_hash(str(tmp_path)) == want["write_bam/no_quals.bam"]
    # and the run of 0xff is what stands in the file
    rs = ReadSet.from_records(bam_bytes.records())
    fn = str(tmp_path / "x.bam")
    bam.write_bam(fn, [("chr1", 5000)], {"chr1": rs})
    back = bam.read_contig(fn, "chr1", want_quals=True)
    assert rs.qual is None and back.qual is not None and bool((back.qual == 0xff).all())


def test_the_stand_alone_check_program(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/c/bam_quals_check.cpp"
    csrc = os.path.join(ROOT, "clair3_rna_amd", "csrc")
    exe = str(tmp_path / "bam_quals_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-pthread", os.path.join(ROOT, "tests", "c", "bam_quals_check.cpp"),
                           os.path.join(csrc, "bamio.cpp"), os.path.join(csrc, "vcfio.cpp"), "-lz", "-o", exe])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "bam_quals_check: ok" in out.stdout, out.stdout + out.stderr
    assert os.listdir(str(tmp_path)) == ["bam_quals_check"]                              # it removes what it wrote


def test_the_engine_binding_declares_the_new_calls():
    for name in ("c3r_load_reads_q", "c3r_set_hap_min_bq", "c3r_get_hap_min_bq", "c3r_get_hap_seq"):
        assert name in capi.EXPORTS
    for name in ("c3r_bam_want_quals", "c3r_bam_copy_quals"):
        assert name in bamio.EXPORTS
    with open(os.path.join(ROOT, "include", "c3r.h")) as f:
        header = f.read()
    for name in ("c3r_load_reads_q", "c3r_set_hap_min_bq", "c3r_get_hap_min_bq", "c3r_get_hap_seq"):
        assert "int %s(" % name in header


# ---- the drivers, with an engine that only writes down what it is asked
class _Engine(object):
    log = []

    def __init__(self, device=0): self.q = 0
    def close(self): pass
    def set_params(self, **kw): pass
    def set_phase_sites(self, sites): _Engine.log.append(("table", 0 if sites is None else len(sites)))
    def set_hap_min_bq(self, q): self.q = q; _Engine.log.append(("min_bq", q))
    def hap_min_bq(self): return self.q, 5
    def load_reads(self, rs): _Engine.log.append(("reads", len(rs), rs.qual is not None))
    def haplotags(self): return np.zeros(2, np.uint8), {}
    def read_phase_sets(self): return np.full(2, -1, np.int32)

    def phase_sites(self, sites, min_reads, min_agree_pct, merge_levels):
        _Engine.log.append(("phase", len(sites)))
        n = len(sites)
        out = sites.copy()
        out["ps"] = 3
        return out, dict(n_sites=n, n_phased=n, n_blocks=1, max_block=n)

    def hap_counts(self, query):
        _Engine.log.append(("counts", len(query)))
        return np.zeros((len(query), 3, 3), np.uint32)


HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"


@pytest.fixture()
def files(tmp_path):
    ref = "ACGTTGCAACGGTCA" * 4
    fa = str(tmp_path / "ref.fa")
    io.write_fasta(fa, [("ctg", ref)])
    plain, phased = str(tmp_path / "calls.vcf"), str(tmp_path / "phased.vcf")
    rows = [(3, "G", "T"), (9, "A", "C")]
    with open(plain, "w") as f:
        f.write(HEAD + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT\t0/1\n" % r for r in rows))
    with open(phased, "w") as f:
        f.write(HEAD + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT:PS\t0|1:3\n" % r for r in rows))
    # two reads, one of them without qualities
    rs = ReadSet.from_records([dict(pos=0, cigar="12M", seq=ref[:12], qual=[30] * 12), dict(pos=2, cigar="11M", seq=ref[2:13])])
    bam_fn = str(tmp_path / "in.bam")
    bam.write_bam(bam_fn, [("ctg", len(ref))], {"ctg": rs})
    return types.SimpleNamespace(ref=ref, fa=fa, vcf=plain, phased=phased, bam=bam_fn, out=str(tmp_path / "out"))


def test_the_one_function_that_applies_it():
    rs = ReadSet.from_records([dict(pos=0, cigar="3M", seq="ACG", qual=[1, 2, 3]), dict(pos=1, cigar="2M", seq="AC"), dict(pos=2, cigar="3D", seq="")])
    assert phasing.reads_without_quals(rs) == 1                                          # (the read without bases is not one of them)
    _Engine.log, lines = [], []
    e = _Engine()
    phasing.load_reads_min_bq(e, rs, 0, "ctg", lines.append)
    assert _Engine.log == [("reads", 3, True)] and lines == []                            # off: the plain load and not a word
    _Engine.log = []
    phasing.load_reads_min_bq(e, rs, 7, "ctg", lines.append)
    assert _Engine.log == [("min_bq", 7), ("reads", 3, True)]                             # the threshold before the reads
    assert lines == ["[INFO] ctg: --hap_min_bq 7: 5 of 5 bases masked for haplotagging, counts and phasing votes",
                     "[WARNING] ctg: 1 of 3 reads carry no base qualities: --hap_min_bq masks none of their bases"]
    with pytest.raises(ValueError):
        phasing.load_reads_min_bq(e, ReadSet.from_records([dict(pos=0, cigar="3M", seq="ACG")]), 7, "ctg", lines.append)
    ns = lambda **kw: types.SimpleNamespace(**kw)
    assert phasing.hap_min_bq_arg(ns(), False, "x") == 0 and phasing.hap_min_bq_arg(ns(hap_min_bq=0), False, "x") == 0
    assert phasing.hap_min_bq_arg(ns(hap_min_bq=93), True, "x") == 93
    for bad in (94, -1):
        assert _exit_text(phasing.hap_min_bq_arg, ns(hap_min_bq=bad), True, "x") == "[ERROR] --hap_min_bq must lie between 0 and 93 (phred; 0: off)"
    assert _exit_text(phasing.hap_min_bq_arg, ns(hap_min_bq=5), False, "--y").startswith("[ERROR] --hap_min_bq needs --y (")


def test_refusals(files):
    cv = ["--chkpnt_fn", "w", "--bam_fn", files.bam, "--ref_fn", files.fa, "--call_fn", files.out + ".vcf", "--ctgName", "ctg", "--pileup"]
    assert _exit_text(call_var_bam.Run, call_var_bam.build_parser().parse_args(cv + ["--hap_min_bq", "10"])).startswith("[ERROR] --hap_min_bq needs --phased_vcf_fn")
    assert _exit_text(call_var_bam.Run, call_var_bam.build_parser().parse_args(cv + ["--enable_phasing_model", "True", "--phased_vcf_fn", files.phased, "--hap_min_bq", "94"])) \
        == "[ERROR] --hap_min_bq must lie between 0 and 93 (phred; 0: off)"
    for mod, argv in ((phase_vcf, ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--output_dir", files.out]),
                      (hap_vcf, ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--phased_vcf_fn", files.phased, "--output_fn", files.out + ".vcf"]),
                      (haplotag_bam, ["--bam_fn", files.bam, "--phased_vcf_fn", files.phased, "--output_dir", files.out])):
        assert _exit_text(mod.Run, mod.build_parser().parse_args(argv + ["--hap_min_bq", "-3"])) == "[ERROR] --hap_min_bq must lie between 0 and 93 (phred; 0: off)"
    assert not os.path.exists(files.out)


def _plan(files, extra):
    argv = ["--bam_fn", files.bam, "--ref_fn", files.fa, "--output_dir", files.out, "--pileup_model_path", "m"] + extra
    return call_sample._plan(call_sample.build_parser().parse_args(argv))


def test_call_sample_hands_the_flag_to_every_step_with_a_site_table(files, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "1")
    phased = ["--enable_phasing_model", "--phased_pileup_model_path", "m30"]
    want = "[ERROR] --hap_min_bq needs --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin"
    assert _exit_text(_plan, files, ["--hap_min_bq", "10"]).startswith(want)
    assert _exit_text(_plan, files, phased + ["--hap_min_bq", "10"]).startswith(want)
    assert _exit_text(_plan, files, phased + ["--phasing", "builtin", "--hap_min_bq", "200"]) == "[ERROR] --hap_min_bq must lie between 0 and 93 (phred; 0: off)"
    has = lambda handed: [handed[k:k + 2] for k in range(len(handed)) if handed[k] == "--hap_min_bq"]
    steps = _plan(files, phased + ["--phasing", "builtin", "--phase_output", "--haplotagged_bam", "--hap_min_bq", "10"])
    assert [s.name for s in steps] == ["pass", "clear", "phase_vcf", "pass", "hap_vcf", "clear", "haplotag_bam"]
    for s in steps:
        if s.name in ("phase_vcf", "hap_vcf", "haplotag_bam"):
            assert has(s.handed) == [["--hap_min_bq", "10"]], s
    # the unphased pass holds its reads against no table; the 30-channel pass tags its reads under the threshold
    assert steps[0].handed.hap_min_bq == 0 and steps[3].handed.hap_min_bq == 10 and steps[3].handed.phased_vcf_fn
    # with a phased VCF handed in: the pass and the steps behind it
    steps = _plan(files, phased + ["--phased_vcf_fn", files.phased, "--phase_output", "--haplotagged_bam", "--hap_min_bq", "10"])
    assert steps[0].handed.hap_min_bq == 10 and [bool(has(s.handed)) for s in steps if s.name in ("hap_vcf", "haplotag_bam")] == [True, True]
    # and without the flag no step's arguments change
    without = _plan(files, phased + ["--phased_vcf_fn", files.phased, "--phase_output", "--haplotagged_bam"])
    for a, b in zip(steps, without):
        if a.name in ("hap_vcf", "haplotag_bam"):
            assert [x for k, x in enumerate(a.handed) if x != "--hap_min_bq" and (k == 0 or a.handed[k - 1] != "--hap_min_bq")] == b.handed and not has(b.handed)


def test_the_fetcher_carries_the_qualities_through_parts_and_join(files):
    f = call_sample._Fetcher(files.bam, files.fa, want_quals=True)
    try:
        whole = f.part("ctg", 0, None)
        tail = f.part("ctg", 1, None)                                                    # the reads that start at 1 or later: the second one
        assert whole.qual is not None and len(whole.reads) == 2 and len(tail.reads) == 1 and len(tail.qual) == 2 * len(tail.seq)
        head = ReadSet(whole.reads[:1], whole.cigar[:1], whole.seq[:6], whole.qual[:12])
        joined = f.join([head, tail])
        assert _same(joined, whole) and joined.qual.tobytes() == whole.qual.tobytes() and QR.layout_ok(joined)
        assert call_sample._Fetcher(files.bam, files.fa).part("ctg", 0, None).qual is None
    finally:
        f.close()


def test_drivers_fetch_set_and_say(files, monkeypatch):
    monkeypatch.setattr(capi, "Engine", _Engine)
    for q in (0, 10):
        flag = ["--hap_min_bq", str(q)] if q else []
        want_reads = [("min_bq", 10), ("reads", 2, True)] if q else [("reads", 2, False)]
        # phase_vcf
        _Engine.log, lines = [], []
        phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--output_dir", files.out] + flag), log=lines.append)
        assert _Engine.log == want_reads + [("phase", 2)]
        info, warn = [m for m in lines if "--hap_min_bq" in m and m.startswith("[INFO]")], [m for m in lines if m.startswith("[WARNING]")]
        assert (info, warn) == ((["[INFO] ctg: --hap_min_bq 10: 5 of 23 bases masked for haplotagging, counts and phasing votes"],
                                 ["[WARNING] ctg: 1 of 2 reads carry no base qualities: --hap_min_bq masks none of their bases"]) if q else ([], []))
        # hap_vcf: the table first, then the threshold and the reads
        _Engine.log, lines = [], []
        hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--phased_vcf_fn", files.phased, "--output_fn", files.out + ".vcf"] + flag),
                    log=lines.append)
        assert _Engine.log == [("table", 2)] + want_reads + [("counts", 2)]
        assert len([m for m in lines if "--hap_min_bq" in m]) == (2 if q else 0)
        # haplotag_bam
        _Engine.log, lines = [], []
        haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", files.bam, "--phased_vcf_fn", files.phased, "--output_dir", files.out + "_bam"] + flag),
                         log=lines.append)
        assert _Engine.log == [("table", 2)] + want_reads
        assert len([m for m in lines if "--hap_min_bq" in m]) == (2 if q else 0)
