"""Allele realignment (include/c3r.h: c3r_set_hap_realign, c3r_hap_realign_column) without a GPU: the rule by hand on the restatement
(tests/realignref.py) and on the library's host entry — which is compiled from the header the kernels use —, the two against each other on
the hand cases and on a seeded fuzz, and the C ABI alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from clair3_rna_amd import capi
from clair3_rna_amd.reads import ReadSet
from tests import hapalleleref as HA
from tests import realignref as RR

REF, SNV, DEL, NO, HAND, LONG = RR.REF, RR.SNV, RR.DEL, RR.NO, RR.HAND, RR.LONG
one_read, site_of, long_read = RR.one_read, RR.site_of, RR.long_read


def library_column(rs, i, site, ref, W):
    q, pool = HA.to_query([site])
    return capi.hap_realign_column(q[0], pool, ref[0] + 1, ref[1], rs.reads[i], rs.cigar, rs.seq, W)


def test_distances_on_paper():
    """Pins the RESTATEMENT to paper (strings and distances); the library is held to the same paper by test_rule_by_hand below."""
    assert RR.haplotype((0, REF), site_of(SNV), "A", 3) == "CGATCGG" and RR.haplotype((0, REF), site_of(SNV), "B", 3) == "CGACCGG"
    assert RR.haplotype((0, REF), site_of(DEL), "A", 3) == "CGATCGGA" and RR.haplotype((0, REF), site_of(DEL), "B", 3) == "CGATGGA"
    ins = site_of((14, "T", "TAA", "0/1"))
    assert RR.window(ins, 3) == (13, 0, 2, 10, 17) and RR.haplotype((0, REF), ins, "B", 3) == "CGATAACGG"
    d = RR.levenshtein
    assert (d("CGATCGG", "CGATCGG"), d("CGATCGG", "CGACCGG")) == (0, 1)
    assert (d("CAACCGG", "CGATCGG"), d("CAACCGG", "CGACCGG")) == (2, 1)
    assert (d("CGATAGGA", "CGATCGGA"), d("CGATAGGA", "CGATGGA")) == (1, 1)
    assert (d("CGATCGGTT", "CGATCGG"), d("CGATCGGTT", "CGACCGG")) == (2, 3)
    assert (d("GATCGG", "CGATCGG"), d("GATCGG", "CGACCGG")) == (1, 2)
    assert (d(list("CGA") + [None] + list("CGG"), "CGATCGG"), d("", "ACG"), d("ACG", "")) == (1, 3, 3)
    assert d("kitten", "sitting") == 3


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_rule_by_hand(case):
    _, ref, row, W, read, want, want_off = case
    rs, site = one_read(read), site_of(row)
    assert RR.column_of(rs, 0, site, ref, W) == want
    assert RR.column_of(rs, 0, site, ref, 0) == (want_off, False) == (HA.observe(rs, 0, {site["pos"]: (0, site)}).get(0, NO), False)
    assert library_column(rs, 0, site, ref, W) == want
    assert library_column(rs, 0, site, ref, 0) == (want_off, False)


def test_the_two_limits_of_64():
    p0, W = 60, 16
    ins11, ins12 = "GATTACAGATT", "GATTACAGATTA"
    dele = LONG[p0:p0 + 21]
    fits = site_of((p0 + 1, dele, LONG[p0] + ins11 + dele[1:] + "," + LONG[p0], "1/2"))      # INS 11 / DEL 20: 2W + 1 + D + I = 64
    over = site_of((p0 + 1, dele, LONG[p0] + ins12 + dele[1:] + "," + LONG[p0], "1/2"))      # INS 12 / DEL 20: 65
    assert fits["A"][1] == ("ins", ins11) and fits["B"][1] == ("del", 20) and over["A"][1] == ("ins", ins12)
    assert RR.window(fits, W) == (60, 20, 11, 44, 97) and RR.realignable((0, LONG), fits, W) and not RR.realignable((0, LONG), over, W)
    # a clean read with the insertion: m = 53 + 11 = 64, the window is haplotype A itself
    rs = one_read(long_read(p0, ins11))
    assert RR.realigned_window(rs, 0, (0, LONG), fits, W) == (14, 78)
    assert RR.column_of(rs, 0, fits, (0, LONG), W) == (0, True) == library_column(rs, 0, fits, (0, LONG), W)
    # one more inserted base inside the window: m = 65, the column is the CIGAR's (the insertion behind the anchor is allele A's)
    rs = one_read(long_read(p0, ins11, extra_at=70))
    assert RR.realigned_window(rs, 0, (0, LONG), fits, W) is None
    assert RR.column_of(rs, 0, fits, (0, LONG), W) == (0, False) == library_column(rs, 0, fits, (0, LONG), W)
    # ... and outside the window it does not count
    rs = one_read(long_read(p0, ins11, extra_at=100))
    assert RR.column_of(rs, 0, fits, (0, LONG), W) == (0, True) == library_column(rs, 0, fits, (0, LONG), W)
    # 65: never realigned; one less overhang and it is
    rs = one_read(long_read(p0, ins12))
    assert RR.column_of(rs, 0, over, (0, LONG), W) == (0, False) == library_column(rs, 0, over, (0, LONG), W)
    assert RR.column_of(rs, 0, over, (0, LONG), W - 1) == (0, True) == library_column(rs, 0, over, (0, LONG), W - 1)


# ---- the host entry against the restatement
FUZZ_SEED = 1


@pytest.fixture(scope="module")
def fuzz():
    return RR.gen_fuzz(FUZZ_SEED)


@pytest.mark.parametrize("W", [1, 10, 16])
def test_host_entry_equals_the_restatement_on_the_fuzz(fuzz, W):
    ref, table, rs = fuzz
    assert len(ref[1]) == 400 and len(rs) == 200
    n, n_ra, n_diff = RR.fuzz_profile(ref, table, rs, W)
    print("W = %d: %d observations, %d realigned, %d columns differ from the switch-off rule" % (W, n, n_ra, n_diff))
    assert 2 * n_ra >= n and n_diff >= 10                                  # (a fuzz that falls back everywhere must not pass)
    q, pool = HA.to_query(table)
    for i in range(len(rs)):
        for j, site in enumerate(table):
            want = RR.column_of(rs, i, site, ref, W)
            assert capi.hap_realign_column(q[j], pool, 1, ref[1], rs.reads[i], rs.cigar, rs.seq, W) == want, (i, j)


def test_host_entry_refusals():
    rs, site = one_read(HAND[0][4]), site_of(SNV)
    q, pool = HA.to_query([site])
    ok = lambda **kw: capi.hap_realign_column(kw.get("q", q[0]), pool, kw.get("start", 1), REF, rs.reads[0], kw.get("cigar", rs.cigar), rs.seq, kw.get("W", 3))
    assert ok() == (0, True)
    for bad in (dict(W=17), dict(W=-1), dict(start=0)):
        with pytest.raises(capi.C3RError):
            ok(**bad)
    bad_site = q.copy()
    bad_site[0]["b_kind"] = 2                                               # a deletion without a length
    with pytest.raises(capi.C3RError):
        ok(q=bad_site[0])
    with pytest.raises(capi.C3RError):
        ok(cigar=rs.cigar | 15)                                             # an op code that no CIGAR has


# ---- the C ABI alone (host code: the program needs no device)
def test_the_stand_alone_check_program(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/c/realign_check.cpp"
    lib = os.path.join(root, "clair3_rna_amd")
    exe = str(tmp_path / "realign_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "realign_check.cpp"),
                           "-L", lib, "-lc3r", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "realign_check: ok" in out.stdout, out.stdout + out.stderr


# ---- the drivers: refusals and plumbing, with a logging fake engine
import gzip
import types

from clair3_rna_amd import haplotag_bam, io, phase_vcf, phasedvcf, phasing
from tests.support import fake_engine_realign as FE


def _exit_text(fn, *a):
    with pytest.raises(SystemExit) as e:
        fn(*a)
    return str(e.value)


@pytest.fixture()
def files(tmp_path):
    ref = REF
    fa = str(tmp_path / "ref.fa")
    io.write_fasta(fa, [("ctg", ref)])
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
    rows = [(8, "G", "A", "0/1", "0|1"), (14, "T", "C", "0/1", "1|0")]
    plain, phased = str(tmp_path / "calls.vcf"), str(tmp_path / "phased.vcf")
    with open(plain, "w") as f:
        f.write(head + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT\t%s\n" % r[:4] for r in rows))
    with open(phased, "w") as f:
        f.write(head + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT:PS\t%s:3\n" % (r[0], r[1], r[2], r[4]) for r in rows))
    bam = str(tmp_path / "in.bam")
    open(bam, "w").close()
    return types.SimpleNamespace(ref=ref, fa=fa, vcf=plain, phased=phased, bam=bam, out=str(tmp_path / "out"))


def test_driver_refusals(files):
    base = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--output_dir", files.out]
    run = lambda mod, argv: _exit_text(mod.Run, mod.build_parser().parse_args(argv))
    assert phase_vcf.build_parser().parse_args(base + ["--hap_realign"]).hap_realign == 10 == phasing.HAP_REALIGN_DEFAULT
    assert phase_vcf.build_parser().parse_args(base + ["--hap_realign", "4"]).hap_realign == 4 and phase_vcf.build_parser().parse_args(base).hap_realign == 0
    assert run(phase_vcf, base + ["--hap_realign"]) == "[ERROR] --hap_realign needs --ref_fn"
    assert run(phase_vcf, base + ["--hap_realign", "--ref_fn", files.fa + ".no"]) == "[ERROR] file %s.no not found" % files.fa
    for bad in ("17", "-1"):
        assert run(phase_vcf, base + ["--hap_realign", bad, "--ref_fn", files.fa]).startswith("[ERROR] --hap_realign must lie between 1 and 16")
    assert run(phase_vcf, base + ["--hap_realign", "--indels", "--left_align_indels", "--ref_fn", files.fa]) == (
        "[ERROR] --hap_realign and --left_align_indels exclude each other (include/c3r.h: c3r_set_hap_realign)")
    hb = ["--bam_fn", files.bam, "--phased_vcf_fn", files.phased, "--output_dir", files.out]
    assert run(haplotag_bam, hb + ["--hap_realign"]) == "[ERROR] --hap_realign needs --ref_fn"
    assert run(haplotag_bam, hb + ["--hap_realign", "--haplotag_indels", "--left_align_indels", "--ref_fn", files.fa]).startswith("[ERROR] --hap_realign and --left_align_indels exclude")
    assert phasing.hap_realign_arg(types.SimpleNamespace()) == (0, None)                        # a parser without the flag
    assert _exit_text(phasing.hap_realign_arg, types.SimpleNamespace(hap_realign=10, ref_fn=files.fa), False, "--phased_vcf_fn") == (
        "[ERROR] --hap_realign needs --phased_vcf_fn (it realigns reads for the steps that hold them against a site table)")


def test_phase_vcf_plumbing(files, monkeypatch):
    monkeypatch.setattr(capi, "Engine", FE.Engine)
    monkeypatch.setattr(io, "load_reads", lambda bam, ctg: one_read(HAND[0][4]))
    base = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--output_dir", files.out]
    out = {}
    for name, extra in (("off", []), ("on", ["--hap_realign", "--ref_fn", files.fa]), ("on_indels", ["--hap_realign", "3", "--indels", "--ref_fn", files.fa])):
        FE.Engine.log = []
        phase_vcf.Run(phase_vcf.build_parser().parse_args(base + extra), log=lambda m: None)
        out[name] = (list(FE.Engine.log), gzip.open(files.out + "/phased_ctg.vcf.gz", "rt").read())
    # without the flag: no reference, no switch, the SNV call
    assert out["off"][0] == [("reads", 1), ("phase_snv", [8, 14])]
    # with it: the reference and the switch come before the reads, and the SNV table goes through the allele call (A = REF, B = ALT, base_matters)
    assert out["on"][0] == [("reference", 1, len(files.ref)), ("realign", 10), ("reads", 1), ("phase_alleles", [8, 14], [(4, 1, 1, 0), (8, 2, 1, 0)])]
    assert out["on_indels"][0][:3] == [("reference", 1, len(files.ref)), ("realign", 3), ("reads", 1)] and out["on_indels"][0][3][0] == "phase_alleles"
    assert out["on"][1] == out["off"][1] and "0|1:3" in out["on"][1]                           # (the fake phases alike: the writer is the same)


def test_phase_source_hands_an_snv_table_to_the_allele_call(files):
    t = phasedvcf.PhaseSource(files.phased, False, realign=10).table("ctg")
    FE.Engine.log = []
    phasedvcf.PhaseSource(files.phased, False, realign=10).apply(FE.Engine(), t)
    assert FE.Engine.log == [("allele_table", 2, [1, 1], [0, 1])]
    FE.Engine.log = []
    phasedvcf.PhaseSource(files.phased, False).apply(FE.Engine(), t)
    assert FE.Engine.log == [("snv_table", 2)]
    sites, h1 = phasing.snv_sites_as_alleles(t.sites)
    assert list(sites["pos"]) == [8, 14] and list(sites["ps"]) == [3, 3] and list(h1) == [0, 1] and not sites["event_matters"].any()
    calls = []
    eng = types.SimpleNamespace(set_reference=lambda s, r: calls.append(("reference", s)), set_hap_realign=lambda w: calls.append(("realign", w)))
    phasing.apply_hap_realign(eng, 0, None)
    phasing.apply_hap_realign(eng, 7, (1, "ACGT"))
    assert calls == [("reference", 1), ("realign", 7)]


def test_refusals_of_the_other_drivers(files, monkeypatch):
    from clair3_rna_amd import call_sample, call_var_bam, hap_vcf
    run = lambda mod, argv: _exit_text(mod.Run, mod.build_parser().parse_args(argv))
    hv = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--phased_vcf_fn", files.phased, "--output_fn", files.out + ".vcf"]
    assert run(hap_vcf, hv + ["--hap_realign"]) == "[ERROR] --hap_realign needs --ref_fn"
    assert run(hap_vcf, hv + ["--hap_realign", "20", "--ref_fn", files.fa]).startswith("[ERROR] --hap_realign must lie between 1 and 16")
    assert run(hap_vcf, hv + ["--hap_realign", "--indels", "--left_align_indels", "--ref_fn", files.fa]).startswith("[ERROR] --hap_realign and --left_align_indels exclude")
    cv = ["--chkpnt_fn", "w", "--bam_fn", files.bam, "--ref_fn", files.fa, "--call_fn", files.out + ".vcf", "--ctgName", "ctg", "--pileup"]
    needs = "without a phase table no step holds the reads against one (it realigns reads for the steps that hold them against a site table)"
    assert run(call_var_bam, cv + ["--hap_realign"]) == "[ERROR] --hap_realign needs --phased_vcf_fn: " + needs
    assert run(call_var_bam, cv + ["--enable_phasing_model", "True", "--phased_vcf_fn", files.phased, "--haplotag_indels", "--left_align_indels", "--hap_realign"]).startswith(
        "[ERROR] --hap_realign and --left_align_indels exclude")
    assert call_var_bam.build_parser().parse_args(cv + ["--hap_realign"]).hap_realign == 10 and call_var_bam.build_parser().parse_args(cv).hap_realign == 0
    # call_sample: without a step that holds reads against a table; beside --left_align_indels; several ranks under the built-in phasing
    monkeypatch.setenv("WORLD_SIZE", "1")
    source = "[ERROR] --hap_realign needs --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin: " + needs
    assert _exit_text(_plan, files, ["--hap_realign"], False) == source
    assert _exit_text(_plan, files, ["--hap_realign"]) == source                                 # (the phasing model without a phasing source)
    assert _exit_text(_plan, files, ["--hap_realign", "--phased_vcf_fn", files.phased, "--haplotag_indels", "--left_align_indels"]).startswith(
        "[ERROR] --hap_realign and --left_align_indels exclude")
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert _exit_text(_plan, files, ["--hap_realign", "--phasing", "builtin"]).startswith("[ERROR] --phasing builtin runs in one process")
    assert _exit_text(_plan, files, ["--hap_realign", "--phasing", "builtin", "--phasing_indels"]).startswith("[ERROR] --phasing builtin runs in one process")


def _plan(files, extra, phasing_model=True):
    from clair3_rna_amd import call_sample
    argv = ["--bam_fn", files.bam, "--ref_fn", files.fa, "--output_dir", files.out, "--pileup_model_path", "m"] + (
        ["--enable_phasing_model", "--phased_pileup_model_path", "m30"] if phasing_model else []) + extra
    return call_sample._plan(call_sample.build_parser().parse_args(argv))


def test_call_sample_hands_the_flag_to_every_step_that_holds_reads_against_a_table(files, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "1")
    ra = ["--hap_realign", "10", "--ref_fn", files.fa]
    has = lambda handed: [handed[k:k + 4] for k in range(len(handed)) if handed[k] == "--hap_realign"]
    steps = _plan(files, ["--hap_realign", "--phasing", "builtin", "--phase_output", "--haplotagged_bam"])
    assert [s.name for s in steps] == ["pass", "clear", "phase_vcf", "pass", "hap_vcf", "clear", "haplotag_bam"]
    for s in steps:
        if s.name in ("phase_vcf", "hap_vcf", "haplotag_bam"):
            assert has(s.handed) == [ra], s
    # the unphased pass holds its reads against no table: it does not get the flag; the 30-channel pass does
    assert steps[0].handed.hap_realign == 0 and steps[3].handed.hap_realign == 10 and steps[3].handed.phased_vcf_fn
    steps = _plan(files, ["--hap_realign", "4", "--phased_vcf_fn", files.phased, "--phase_output", "--phase_indels", "--haplotagged_bam"])
    assert [s.name for s in steps] == ["pass", "hap_vcf", "clear", "haplotag_bam"] and steps[0].handed.hap_realign == 4
    assert [s.handed[s.handed.index("--hap_realign") + 1] for s in steps if s.name in ("hap_vcf", "haplotag_bam")] == ["4", "4"]
    # and without the flag no step's arguments change
    with_flag = _plan(files, ["--hap_realign", "--phased_vcf_fn", files.phased, "--phase_output", "--haplotagged_bam"])
    without = _plan(files, ["--phased_vcf_fn", files.phased, "--phase_output", "--haplotagged_bam"])
    for a, b in zip(with_flag, without):
        if a.name in ("hap_vcf", "haplotag_bam"):
            k = a.handed.index("--hap_realign")
            assert a.handed[:k] + a.handed[k + 4:] == b.handed and "--hap_realign" not in b.handed
    assert without[0].handed.hap_realign == 0


def test_hap_vcf_plumbing(files, monkeypatch):
    from clair3_rna_amd import hap_vcf

    class Eng(FE.Engine):
        def hap_counts(self, query):
            FE.Engine.log.append(("counts_snv", len(query)))
            return np.zeros((len(query), 3, 3), np.uint32)

        def hap_allele_counts(self, query, pool=None):
            FE.Engine.log.append(("counts_alleles", [int(b) for b in query["base_matters"]], [int(p) for p in query["ps"]]))
            return np.zeros((len(query), 3, 3), np.uint32)
    monkeypatch.setattr(capi, "Engine", Eng)
    monkeypatch.setattr(io, "load_reads", lambda bam, ctg: one_read(HAND[0][4]))
    base = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--phased_vcf_fn", files.phased, "--output_fn", files.out + ".vcf", "--hap_counts_fn", files.out + ".tsv"]
    got = {}
    for name, extra in (("off", []), ("on", ["--hap_realign", "--ref_fn", files.fa])):
        FE.Engine.log = []
        hap_vcf.Run(hap_vcf.build_parser().parse_args(base + extra), log=lambda m: None)
        got[name] = (list(FE.Engine.log), open(files.out + ".vcf").read(), open(files.out + ".tsv").read())
    assert got["off"][0] == [("snv_table", 2), ("reads", 1), ("counts_snv", 2)]
    assert got["on"][0] == [("reference", 1, len(files.ref)), ("realign", 10), ("allele_table", 2, [1, 1], [0, 1]), ("reads", 1), ("counts_alleles", [1, 1], [3, 3])]
    assert got["on"][1:] == got["off"][1:] and got["on"][2].count("\n") == 3                    # (the same writers, the counts file with its two rows)
