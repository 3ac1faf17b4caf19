"""Haplotagging from phased indels and two-ALT sites, without a device: the restatement (tests/hapindelref.py) against its hand-derived
cases and against hapref on SNV tables, the reader of the table (phasedvcf.read_phase_alleles), and the drivers' refusals."""
import gzip
import os

import numpy as np
import pytest

from clair3_rna_amd import capi, phasedvcf
from tests import hapcountref as HC
from tests import hapindelref as HI
from tests import hapref


@pytest.mark.parametrize("case", HI.CASES, ids=[c[0] for c in HI.CASES])
def test_hand_derived_cases(case):
    rs, sites = HI.case_inputs(case)
    got = [HI.tag_read(rs, i, sites)[:4] for i in range(len(rs))]
    assert got == case[3]
    hp, st, ps = HI.haplotag(rs, sites)
    assert hp.tolist() == [e[0] for e in case[3]] and ps.tolist() == [e[3] for e in case[3]]
    assert st["n_reads"] == len(rs) == st["n_hp1"] + st["n_hp2"] + st["n_no_vote"] + st["n_tie"]


def test_the_cases_cover_what_the_rule_names():
    names = " ".join(c[0] for c in HI.CASES)
    for word in ("deletion_only", "one_base_off", "insertion_then_deletion", "two_alt_1|2", "two_alt_2|1", "outvote", "by_count", "first_site_is_an_indel",
                 "under_a_deletion", "under_a_ref_skip", "cut_off_event_matters", "cut_off_snv_site"):
        assert word in names, word


def _snv_inputs():
    for case in hapref.CASES:
        rs, table = hapref.case_inputs(case)
        yield case[0], rs, table[np.argsort(table["pos"], kind="stable")]
    for seed in range(4):
        _, rs, table, _ = hapref.gen_case(seed)
        yield "gen%d" % seed, rs, table


def test_on_snv_tables_the_restatement_is_haprefs():
    for name, rs, table in _snv_inputs():
        hp0, st0, _ = hapref.haplotag(rs, table)
        ps0 = HC.read_phase_sets(rs, table)
        hp, st, ps = HI.haplotag(rs, HI.from_snv_table(table))
        assert np.array_equal(hp, hp0) and np.array_equal(ps, ps0) and st == st0, name
        # and the engine's form of the converted table is the one capi makes of the SNV table
        q, h1, pool, n = HI.to_engine(HI.from_snv_table(table))
        assert np.array_equal(q, capi.hap_sites_from_snvs(table)) and np.array_equal(h1, table["h1"]) and n == 0 and len(pool) == 0, name


# ---- the reader
HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
ROWS = [
    ("chr1", 10, "A", "C", "PASS", "GT:PS", "0|1:10"),            # kept: SNV
    ("chr1", 20, "c", "cag", "LowQual", "GT:PS", "1|0:10"),       # kept: insertion, FILTER ignored, lower case
    ("chr1", 30, "GTT", "G", "PASS", "GT:GQ:PS", "0|1:9:30"),     # kept: deletion
    ("chr1", 40, "C", "T,CGG", "PASS", "GT:PS", "1|2:30"),        # kept: two ALTs
    ("chr1", 50, "ACC", "A,TCC", "PASS", "GT:PS", "2|1:30"),      # kept: two ALTs, suffix stripped: A = (A, del 2), B = (T, none)
    ("chr1", 55, "A", "AT", "PASS", "GT", "0|1"),                 # kept: no PS -> 0
    ("chr1", 60, "A", "C", "PASS", "GT:PS", "0/1:10"),            # not_phased_het
    ("chr1", 61, "A", "C", "PASS", "GT:PS", "1|1:10"),            # not_phased_het
    ("chr1", 62, "A", "C", "PASS", "GT:PS", "1|2:10"),            # not_phased_het (1|2 with one ALT)
    ("chr1", 63, "A", "C,G", "PASS", "GT:PS", "0|1:10"),          # multi_alt
    ("chr1", 64, "A", "C,G,T", "PASS", "GT:PS", "1|2:10"),        # multi_alt
    ("chr1", 65, "AT", "GC", "PASS", "GT:PS", "0|1:10"),          # complex_allele
    ("chr1", 66, "A", "<DEL>", "PASS", "GT:PS", "0|1:10"),        # complex_allele
    ("chr1", 67, "AT", "ACT,ACT", "PASS", "GT:PS", "1|2:10"),     # same_alleles
    ("chr1", 68, "A", "C", "PASS", "GT:PS", "0|1:x"),             # malformed (PS)
    ("chr1", 20, "C", "T", "PASS", "GT:PS", "0|1:99"),            # duplicate_pos: the first row on 20 stays
    ("chr2", 5, "A", "AGG", "PASS", "GT:PS", "1|0:5"),            # other_contig for chr1
]


def _write(path, rows, gz=False):
    text = HEAD + "".join("%s\t%d\t.\t%s\t%s\t30\t%s\t.\t%s\t%s\n" % r for r in rows) + "chr1\tx\n"
    with (gzip.open(path, "wt") if gz else open(path, "w")) as f:
        f.write(text)
    return str(path)


def _as_rows(sites, h1, pool):
    """The table back as readable rows: (pos, ps, h1, base_matters, event_matters, A, B) with an allele as (letter, kind, length, inserted letters)."""
    letter = {1: "A", 2: "C", 4: "G", 8: "T"}
    codes = [c for byte in pool.tolist() for c in (byte >> 4, byte & 15)]
    out = []
    for s, h in zip(sites, h1):
        al = []
        for n in "ab":
            ins = "".join(letter[c] for c in codes[int(s[n + "_ins_off"]):int(s[n + "_ins_off"]) + int(s[n + "_len"])]) if s[n + "_kind"] == capi.HAP_EV_INS else ""
            al.append((letter[int(s[n + "_base"])], int(s[n + "_kind"]), int(s[n + "_len"]), ins))
        out.append((int(s["pos"]), int(s["ps"]), int(h), int(s["base_matters"]), int(s["event_matters"]), al[0], al[1]))
    return out


def test_the_reader_keeps_and_skips_by_the_rule(tmp_path):
    fn = _write(tmp_path / "p.vcf", ROWS)
    sites, h1, pool, pool_bases, skipped = phasedvcf.read_phase_alleles(fn, "chr1")
    N, I, D = capi.HAP_EV_NONE, capi.HAP_EV_INS, capi.HAP_EV_DEL
    assert _as_rows(sites, h1, pool) == [
        (10, 10, 0, 1, 0, ("A", N, 0, ""), ("C", N, 0, "")),
        (20, 10, 1, 0, 1, ("C", N, 0, ""), ("C", I, 2, "AG")),
        (30, 30, 0, 0, 1, ("G", N, 0, ""), ("G", D, 2, "")),
        (40, 30, 0, 1, 1, ("T", N, 0, ""), ("C", I, 2, "GG")),
        (50, 30, 1, 1, 1, ("A", D, 2, ""), ("T", N, 0, "")),
        (55, 0, 0, 0, 1, ("A", N, 0, ""), ("A", I, 1, "T")),
    ]
    assert pool_bases == 5 and len(pool) == 3 and sites.dtype == capi.HAP_SITE_DTYPE and h1.dtype == np.uint8
    assert skipped == dict(other_contig=1, malformed=2, not_snv=0, not_phased_het=3, duplicate_pos=1, multi_alt=2, complex_allele=2, same_alleles=1)
    assert tuple(skipped) == phasedvcf.ALLELE_SKIP_REASONS and skipped.kept == dict(indel=5, two_alt=2)
    # every contig in one pass; gzipped
    per = phasedvcf.read_all_phase_alleles(_write(tmp_path / "p.vcf.gz", ROWS, gz=True))
    assert sorted(per) == ["chr1", "chr2"] and np.array_equal(per["chr1"][0], sites) and np.array_equal(per["chr1"][1], h1)
    assert _as_rows(*per["chr2"][:3]) == [(5, 5, 1, 0, 1, ("A", N, 0, ""), ("A", I, 2, "GG"))] and per["chr2"][3] == 2
    assert per["chr1"][4]["other_contig"] == 0 and per["chr1"][4]["malformed"] == 2
    # the restatement reads the same alleles from the same rows
    for row, got in zip(ROWS[:6], _as_rows(sites, h1, pool)):
        s = HI.site(row[1], row[2], row[3], row[6].split(":")[0], got[1])
        q, hh, pl, n = HI.to_engine([s])
        assert _as_rows(q, hh, pl) == [got], row


def test_an_snv_only_file_reads_as_read_phase_sites_does(tmp_path):
    rows = [("chr1", 10, "A", "C", "PASS", "GT:PS", "0|1:10"), ("chr1", 12, "g", "t", "q10", "GT:PS", "1|0:10"), ("chr1", 9, "T", "A", "PASS", "GT", "1|0"),
            ("chr1", 12, "G", "A", "PASS", "GT:PS", "0|1:7"), ("chr1", 30, "C", "G", "PASS", "GT:PS", "0/1:10"), ("chr1", 31, "C", "G", "PASS", "GT:PS", "0|1:.")]
    fn = _write(tmp_path / "s.vcf", rows)
    old, old_skipped = phasedvcf.read_phase_sites(fn, "chr1")
    sites, h1, pool, pool_bases, skipped = phasedvcf.read_phase_alleles(fn, "chr1")
    assert np.array_equal(sites["pos"], old["pos"]) and np.array_equal(sites["ps"], old["ps"]) and np.array_equal(h1, old["h1"]) and len(old) == 4
    assert np.array_equal(sites, _with_ps(capi.hap_sites_from_snvs(old), old["ps"])) and pool_bases == 0 and len(pool) == 0
    assert {k: skipped[k] for k in old_skipped} == old_skipped and skipped.kept == dict(indel=0, two_alt=0)


def _with_ps(q, ps):
    q = q.copy()
    q["ps"] = ps
    return q


def test_a_directory_of_per_contig_files(tmp_path):
    d = tmp_path / "phased_vcf"
    d.mkdir()
    _write(d / "phased_chr1.vcf.gz", ROWS, gz=True)
    sites, h1, pool, pool_bases, skipped = phasedvcf.contig_alleles(str(d), "chr1")
    one = phasedvcf.read_phase_alleles(_write(tmp_path / "p.vcf", ROWS), "chr1")
    assert np.array_equal(sites, one[0]) and np.array_equal(h1, one[1]) and np.array_equal(pool, one[2]) and pool_bases == one[3] and skipped == one[4]
    sites, h1, pool, pool_bases, skipped = phasedvcf.contig_alleles(str(d), "chr7")           # no file: nothing phased there
    assert len(sites) == 0 and sites.dtype == capi.HAP_SITE_DTYPE and len(h1) == 0 and pool_bases == 0 and not any(skipped.values())
    with pytest.raises(SystemExit):
        phasedvcf.contig_alleles(str(tmp_path / "nowhere"), "chr1")


# ---- the drivers refuse the flag where it means nothing, before a context exists
def _no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(capi, "Engine", boom)


def test_the_flag_without_a_phased_vcf_is_refused(tmp_path, monkeypatch):
    from clair3_rna_amd import call_sample, call_var_bam
    _no_engine(monkeypatch)
    out = str(tmp_path / "out")
    argv = ["--bam_fn", str(tmp_path / "x.bam"), "--ref_fn", str(tmp_path / "x.fa"), "--output_dir", out, "--pileup_model_path", "m", "--phased_pileup_model_path", "m",
            "--enable_phasing_model", "--haplotag_indels"]
    with pytest.raises(SystemExit) as e:
        call_sample.Run(call_sample.build_parser().parse_args(argv))
    assert str(e.value.code).startswith("[ERROR]") and "--haplotag_indels" in str(e.value.code) and "--phased_vcf_fn" in str(e.value.code)
    assert not os.path.exists(out)
    argv = ["--chkpnt_fn", "m", "--bam_fn", str(tmp_path / "x.bam"), "--ref_fn", str(tmp_path / "x.fa"), "--ctgName", "chr1", "--pileup", "--enable_phasing_model", "True",
            "--haplotag_indels"]
    with pytest.raises(SystemExit) as e:
        call_var_bam.Run(call_var_bam.build_parser().parse_args(argv))
    assert str(e.value.code).startswith("[ERROR]") and "--haplotag_indels" in str(e.value.code) and "--phased_vcf_fn" in str(e.value.code)


def test_the_flag_with_the_builtin_phasing_is_refused_and_names_the_two_steps(tmp_path, monkeypatch):
    from clair3_rna_amd import call_sample
    _no_engine(monkeypatch)
    out = str(tmp_path / "out")
    argv = ["--bam_fn", str(tmp_path / "x.bam"), "--ref_fn", str(tmp_path / "x.fa"), "--output_dir", out, "--pileup_model_path", "m", "--phased_pileup_model_path", "m",
            "--enable_phasing_model", "--phasing", "builtin", "--haplotag_indels"]
    for extra in ([], ["--phase_output", "--phase_indels"]):
        with pytest.raises(SystemExit) as e:
            call_sample.Run(call_sample.build_parser().parse_args(argv + extra))
        msg = str(e.value.code)
        assert msg.startswith("[ERROR]") and "--phasing builtin" in msg and "SNV-only" in msg
        assert "--phase_output --phase_indels" in msg and "--phased_vcf_fn <prefix>_enable_phasing_phased.vcf.gz --haplotag_indels" in msg
        assert not os.path.exists(out)


def test_the_flag_is_off_by_default_everywhere():
    from clair3_rna_amd import call_sample, call_var_bam, hap_vcf, haplotag_bam
    assert call_sample.build_parser().parse_args(["-b", "b", "-f", "r", "-o", "o", "--pileup_model_path", "m"]).haplotag_indels is False
    assert call_var_bam.build_parser().parse_args(["--bam_fn", "b", "--chkpnt_fn", "c", "--ref_fn", "r"]).haplotag_indels is False
    assert hap_vcf.build_parser().parse_args(["-b", "b", "--vcf_fn", "v", "--phased_vcf_fn", "p", "-o", "o"]).haplotag_indels is False
    assert haplotag_bam.build_parser().parse_args(["-b", "b", "--phased_vcf_fn", "p", "-o", "o"]).haplotag_indels is False
    for mod, argv in ((hap_vcf, ["-b", "b", "--vcf_fn", "v", "-o", "o", "--haplotag_indels"]), (haplotag_bam, ["-b", "b", "-o", "o", "--haplotag_indels"])):
        with pytest.raises(SystemExit):                      # (--phased_vcf_fn is a required argument of the two)
            mod.build_parser().parse_args(argv)
