"""Quality-weighted haplotag votes (c3r_set_hap_bq_weights, --hap_bq_weights) without a GPU: the restatement tests/hapweightref.py held to
hand-derived answers, the condition on the seeded fuzz that the GPU tests reuse, PC in the haplotagged BAM through tests/bamref.py, the
stand-alone check of the writer's new entry point, the bindings, and the drivers' refusals and plumbing with a logging fake engine."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from clair3_rna_amd import bam, bamio, capi, haplotag_bam, io, phasing
from tests import bamref
from tests import hapalleleref as HA
from tests import hapindelref as HI
from tests import hapweightref as HW
from tests import qualref as QR
from tests.support import fake_engine_realign as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule by hand
@pytest.mark.parametrize("case", HW.CASES, ids=[c[0] for c in HW.CASES])
def test_rule_by_hand(case):
    rs, sites, Q = HW.case_inputs(case)
    seen = HW.masked_as_n(rs, Q) if Q else rs
    got = HW.haplotag(seen, sites)
    unit = HW.haplotag(seen, sites, weighted=False)
    for i, (hp, w1, w2, ps, n) in enumerate(case[4]):
        assert (int(got["hp"][i]), int(got["w12"][i][0]), int(got["w12"][i][1]), int(got["ps"][i]), int(got["words"][i]) >> 2) == (hp, w1, w2, ps, n), (case[0], i)
        assert int(got["words"][i]) & 3 == hp
    assert [(int(h), int(p)) for h, p in zip(unit["hp"], unit["ps"])] == case[5]
    # unit weights through this module are the rule of c3r_set_phase_alleles as tests/hapindelref.py states it
    hp, st, ps = HI.haplotag(seen, sites)
    assert np.array_equal(hp, unit["hp"]) and np.array_equal(ps, unit["ps"]) and st == unit["st"]


def test_statistics_by_hand():
    by_name = {c[0]: c for c in HW.CASES}
    rs, sites, _ = HW.case_inputs(by_name["w1_equals_w2_is_a_tie"])
    assert HW.haplotag(rs, sites)["st"] == dict(n_reads=1, n_hp1=0, n_hp2=0, n_no_vote=0, n_tie=1, n_votes=3)
    rs, sites, _ = HW.case_inputs(by_name["only_q0"])
    assert HW.haplotag(rs, sites)["st"] == dict(n_reads=1, n_hp1=0, n_hp2=0, n_no_vote=0, n_tie=1, n_votes=1)
    assert HW.haplotag(rs, [HI.site(50, "A", "C", "0|1", 4)])["st"] == dict(n_reads=1, n_hp1=0, n_hp2=0, n_no_vote=1, n_tie=0, n_votes=0)
    # a read without a quality array and a read whose bytes are 0xff are the same read
    rs, sites, _ = HW.case_inputs(by_name["q30_outvotes_two_q5"])
    a, b = HW.haplotag(HW.with_qual(rs, None), sites), HW.haplotag(HW.with_qual(rs, np.full(len(rs.qual), 0xff, np.uint8)), sites)
    assert np.array_equal(a["w12"], b["w12"]) and a["w12"].tolist() == [[1, 2]] and a["hp"].tolist() == [2]
    assert HW.pc_of([[30, 10], [0, 7], [5, 5]]).tolist() == [20, 7, 0]


# ---- the fuzz that tests/test_gpu_hap_bq_weights.py runs on the device: it cannot pass by agreeing with the old rule
def test_fuzz_precondition():
    ref, table, rs = HW.gen_fuzz()
    assert QR.layout_ok(rs) and 200 <= len(rs) <= 400 and int(rs.reads["l_seq"].max()) <= 200
    w, u = HW.haplotag(rs, table), HW.haplotag(rs, table, weighted=False)
    c = HW.fuzz_classes(w, u)
    assert c["tagged_unit"] >= 100 and c["differ"] * 20 >= c["tagged_unit"], c
    assert min(c["flipped"], c["set_changed"], c["became_tie"], c["left_tie"]) >= 1, c
    assert np.array_equal(w["words"] >> 2, u["words"] >> 2)                     # the observations are the same: only their weights differ
    # and the SNV rows alone (k_haplotag_w's table) move reads as well
    snv = HI.from_snv_table(HW.snv_rows(table))
    c = HW.fuzz_classes(HW.haplotag(rs, snv), HW.haplotag(rs, snv, weighted=False))
    assert c["differ"] * 20 >= c["tagged_unit"] >= 100 and c["flipped"] >= 1, c
    kinds = [[int(x) & 15 for x in rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]] for r in rs.reads]
    assert sum(1 for k in kinds if 7 in k or 8 in k) >= 20 and sum(1 for k in kinds if 6 in k) >= 20      # = / X runs and pads: the serial walk


# ---- PC in the BAM
def _tagged_bam(tmp_path, pcs):
    recs = [dict(pos=10 * k, cigar="8M", seq="ACGTACGT", flag=0, mapq=60, hp=0) for k in range(len(pcs))]
    from clair3_rna_amd.reads import ReadSet
    rs = ReadSet.from_records(recs)
    fn = str(tmp_path / "in.bam")
    bam.write_bam(fn, [("chr1", 5000)], {"chr1": rs})
    return fn


def test_pc_in_all_three_widths_and_absent_for_untagged_reads(tmp_path):
    pcs = np.array([0, 255, 256, 65535, 65536, 4000000000, 7, 9], np.uint32)
    hp = np.array([1, 2, 1, 2, 1, 2, 0, 0], np.uint8)
    ps = np.array([5, 5, 300, 5, 70000, 5, -1, -1], np.int32)
    fn = _tagged_bam(tmp_path, pcs)
    out = {k: str(tmp_path / (k + ".bam")) for k in ("pc", "none", "old")}
    with bamio.BamFile(fn) as bf:
        rs = bf.fetch("chr1")
        st = bf.write_haplotagged("chr1", out["pc"], rs, hp, ps, pc=pcs)
        assert st == dict(records=8, tagged=6, stripped=0, unpaired=0)
        bf.write_haplotagged("chr1", out["none"], rs, hp, ps, pc=None)
        L = bamio.load_library()                                               # the old entry point itself
        reads = np.ascontiguousarray(rs.reads)
        import ctypes as C
        counts = (C.c_int64 * 4)()
        assert L.c3r_bam_write_haplotagged(bf.h, b"chr1", reads.ctypes.data, hp.ctypes.data, ps.ctypes.data, 8, os.fsencode(out["old"]), None, 0, counts) == 0
        with pytest.raises(ValueError):
            bf.write_haplotagged("chr1", out["pc"] + ".x", rs, hp, ps, pc=pcs[:3])
        with pytest.raises(ValueError):
            bf.write_haplotagged("chr1", out["pc"] + ".x", None, None, None, pc=pcs)
    assert open(out["none"], "rb").read() == open(out["old"], "rb").read()
    recs = list(bamref.Bam(out["pc"]).records)
    assert len(recs) == 8
    want_type = ["C", "C", "S", "S", "I", "I"]
    for k, r in enumerate(recs):
        tags = {t: (ty, v) for t, ty, v in r.aux}
        if hp[k]:
            assert [t for t, _, _ in r.aux][-3:] == ["HP", "PS", "PC"] and tags["PC"] == (want_type[k], int(pcs[k])) and tags["HP"] == ("C", int(hp[k]))
        else:
            assert not {"HP", "PS", "PC"} & set(tags)
    assert all("PC" not in {t for t, _, _ in r.aux} for r in bamref.Bam(out["old"]).records)


def test_the_stand_alone_check_program(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/c/hapbam_pc_check.cpp"
    csrc = os.path.join(ROOT, "clair3_rna_amd", "csrc")
    exe = str(tmp_path / "hapbam_pc_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-pthread", os.path.join(ROOT, "tests", "c", "hapbam_pc_check.cpp"),
                           os.path.join(csrc, "bamio.cpp"), os.path.join(csrc, "vcfio.cpp"), "-lz", "-o", exe])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "hapbam_pc_check: ok" in out.stdout, out.stdout + out.stderr
    assert os.listdir(str(tmp_path)) == ["hapbam_pc_check"]                               # it removes what it wrote


def test_the_bindings_declare_the_new_calls():
    for name in ("c3r_set_hap_bq_weights", "c3r_get_hap_bq_weights", "c3r_get_haplotag_weights", "c3r_get_haplotag_words"):
        assert name in capi.EXPORTS
    assert "c3r_bam_write_haplotagged_pc" in bamio.EXPORTS
    with open(os.path.join(ROOT, "include", "c3r.h")) as f:
        text = f.read()
    for name in ("int c3r_set_hap_bq_weights(c3r_ctx *ctx, int on);", "int c3r_get_hap_bq_weights(c3r_ctx *ctx, int *on);",
                 "int c3r_get_haplotag_weights(c3r_ctx *ctx, uint32_t *w12, int64_t cap);", "int c3r_get_haplotag_words(c3r_ctx *ctx, uint32_t *words, int64_t cap);"):
        assert name in text
    lib = os.path.join(ROOT, "clair3_rna_amd", "libc3r.so")
    if os.path.exists(lib):
        import ctypes as C
        L = C.CDLL(lib)
        for name in ("c3r_set_hap_bq_weights", "c3r_get_hap_bq_weights", "c3r_get_haplotag_weights", "c3r_get_haplotag_words"):
            assert hasattr(L, name)
    assert hasattr(bamio.load_library(), "c3r_bam_write_haplotagged_pc")


# ---- the drivers: refusals and plumbing, with the logging fake engine
class Eng(FE.Engine):
    def set_hap_bq_weights(self, on):
        FE.Engine.log.append(("bq_weights", bool(on)))

    def hap_min_bq(self):
        return 0, 0

    def haplotag_weights(self):
        FE.Engine.log.append(("weights",))
        return np.array([[30, 10]], np.uint32)

    def haplotags(self):
        return np.array([1], np.uint8), {}

    def read_phase_sets(self):
        return np.array([3], np.int32)


def _exit_text(fn, *a):
    with pytest.raises(SystemExit) as e:
        fn(*a)
    return str(e.value)


@pytest.fixture()
def files(tmp_path):
    ref = "ACGTTGCAGGCTAACGTAGCTAGGATCCAGT" * 2
    fa = str(tmp_path / "ref.fa")
    io.write_fasta(fa, [("ctg", ref)])
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
    rows = [(8, ref[7], "A" if ref[7] != "A" else "C", "0/1", "0|1"), (14, ref[13], "C" if ref[13] != "C" else "G", "0/1", "1|0")]
    plain, phased = str(tmp_path / "calls.vcf"), str(tmp_path / "phased.vcf")
    with open(plain, "w") as f:
        f.write(head + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT\t%s\n" % r[:4] for r in rows))
    with open(phased, "w") as f:
        f.write(head + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT:PS\t%s:3\n" % (r[0], r[1], r[2], r[4]) for r in rows))
    from clair3_rna_amd.reads import ReadSet
    rs = ReadSet.from_records([dict(pos=2, cigar="20M", seq=ref[2:22], flag=0, mapq=60, hp=0, qual=list(range(10, 30)))])
    bam_fn = str(tmp_path / "in.bam")
    bam.write_bam(bam_fn, [("ctg", len(ref))], {"ctg": rs})
    return types.SimpleNamespace(ref=ref, fa=fa, vcf=plain, phased=phased, bam=bam_fn, out=str(tmp_path / "out"), rs=rs)


def _plan(files, extra, phasing_model=True):
    from clair3_rna_amd import call_sample
    argv = ["--bam_fn", files.bam, "--ref_fn", files.fa, "--output_dir", files.out, "--pileup_model_path", "m"] + (
        ["--enable_phasing_model", "--phased_pileup_model_path", "m30"] if phasing_model else []) + extra
    return call_sample._plan(call_sample.build_parser().parse_args(argv))


def test_driver_refusals(files, monkeypatch):
    from clair3_rna_amd import call_var_bam
    run = lambda mod, argv: _exit_text(mod.Run, mod.build_parser().parse_args(argv))
    cv = ["--chkpnt_fn", "w", "--bam_fn", files.bam, "--ref_fn", files.fa, "--call_fn", files.out + ".vcf", "--ctgName", "ctg", "--pileup"]
    why = " (it weighs the votes of the step that haplotags the reads from a site table)"
    assert run(call_var_bam, cv + ["--hap_bq_weights"]) == "[ERROR] --hap_bq_weights needs --phased_vcf_fn: without a phase table no step haplotags the reads" + why
    assert call_var_bam.build_parser().parse_args(cv).hap_bq_weights is False
    monkeypatch.setenv("WORLD_SIZE", "1")
    source = "[ERROR] --hap_bq_weights needs --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin: without a phase table no step haplotags the reads" + why
    assert _exit_text(_plan, files, ["--hap_bq_weights"], False) == source
    assert _exit_text(_plan, files, ["--hap_bq_weights"]) == source
    assert phasing.hap_bq_weights_arg(types.SimpleNamespace()) is False                      # a parser without the flag
    # reads fetched without qualities are refused where the engine is met, before the switch
    eng = Eng()
    FE.Engine.log = []
    with pytest.raises(ValueError):
        phasing.load_reads_min_bq(eng, HW.with_qual(files.rs, None), 0, "ctg", lambda m: None, weights=True)
    assert FE.Engine.log == []


def test_call_sample_hands_the_flag_to_the_steps_that_tag(files, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "1")
    steps = _plan(files, ["--hap_bq_weights", "--phasing", "builtin", "--phase_output", "--haplotagged_bam"])
    assert [s.name for s in steps] == ["pass", "clear", "phase_vcf", "pass", "hap_vcf", "clear", "haplotag_bam"]
    assert "--hap_bq_weights" not in steps[2].handed                           # phase_vcf: its links stay unweighted
    assert "--hap_bq_weights" in steps[4].handed and "--hap_bq_weights" in steps[6].handed
    assert steps[0].handed.hap_bq_weights is False and steps[3].handed.hap_bq_weights is True and steps[3].handed.phased_vcf_fn
    with_flag = _plan(files, ["--hap_bq_weights", "--phased_vcf_fn", files.phased, "--phase_output", "--haplotagged_bam"])
    without = _plan(files, ["--phased_vcf_fn", files.phased, "--phase_output", "--haplotagged_bam"])
    for a, b in zip(with_flag, without):
        if a.name in ("hap_vcf", "haplotag_bam"):
            assert [x for x in a.handed if x != "--hap_bq_weights"] == b.handed and "--hap_bq_weights" not in b.handed
    assert without[0].handed.hap_bq_weights is False and with_flag[0].handed.hap_bq_weights is True


def test_haplotag_bam_plumbing(files, monkeypatch):
    monkeypatch.setattr(capi, "Engine", Eng)
    base = ["--bam_fn", files.bam, "--phased_vcf_fn", files.phased, "--output_dir", files.out]
    got = {}
    for name, extra in (("off", []), ("on", ["--hap_bq_weights"]), ("on_bq", ["--hap_bq_weights", "--hap_min_bq", "12"])):
        FE.Engine.log = []
        logged = []
        haplotag_bam.Run(haplotag_bam.build_parser().parse_args(base + extra), log=logged.append)
        recs = list(bamref.Bam(os.path.join(files.out, "ctg.bam")).records)
        got[name] = (list(FE.Engine.log), [(t, v) for t, _, v in recs[0].aux if t in ("HP", "PS", "PC")])
    assert got["off"] == ([("snv_table", 2), ("reads", 1)], [("HP", 1), ("PS", 3)])
    # the switch comes before the reads, the qualities come with them, and PC = |30 - 10| follows PS
    assert got["on"] == ([("snv_table", 2), ("bq_weights", True), ("reads", 1), ("weights",)], [("HP", 1), ("PS", 3), ("PC", 20)])
    assert got["on_bq"][0] == [("snv_table", 2), ("bq_weights", True), ("min_bq", 12), ("reads", 1), ("weights",)]


def test_hap_vcf_and_call_var_bam_ask_for_the_qualities(files, monkeypatch):
    from clair3_rna_amd import hap_vcf

    class E2(Eng):
        def hap_counts(self, query):
            return np.zeros((len(query), 3, 3), np.uint32)
    asked = []
    monkeypatch.setattr(capi, "Engine", E2)
    monkeypatch.setattr(io, "load_reads", lambda bam_fn, ctg, **kw: (asked.append(kw), files.rs if kw.get("want_quals") else HW.with_qual(files.rs, None))[1])
    base = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--phased_vcf_fn", files.phased, "--output_fn", files.out + ".vcf", "--hap_counts_fn", files.out + ".tsv"]
    FE.Engine.log = []
    hap_vcf.Run(hap_vcf.build_parser().parse_args(base), log=lambda m: None)
    assert asked == [{}] and FE.Engine.log == [("snv_table", 2), ("reads", 1)]
    FE.Engine.log = []
    hap_vcf.Run(hap_vcf.build_parser().parse_args(base + ["--hap_bq_weights"]), log=lambda m: None)
    assert asked[1] == dict(want_quals=True) and FE.Engine.log == [("snv_table", 2), ("bq_weights", True), ("reads", 1)]
