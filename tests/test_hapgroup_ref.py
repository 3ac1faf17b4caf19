"""The rule `hap_groups` (include/c3r.h: c3r_hap_group_counts) on the CPU: the restatement of tests/hapgroupref.py against answers worked out by
hand, the grouping, merging and mixed-strand resolution of hap_expr --group_by_name, the driver with the engine replaced by a stub that logs
its calls and answers from the restatement, and the two drivers' refusals.  tests/test_gpu_hapgroup.py runs the same tables on the device."""
import os

import numpy as np
import pytest

from clair3_rna_amd import capi, hap_expr
from tests import hapgroupref as HG
from tests import hapref, hapregionref
from tests.test_hapregion_ref import LogEngine


# ---- the rule by hand
@pytest.mark.parametrize("case", HG.HAND, ids=[c[0] for c in HG.HAND])
def test_the_restatement_gives_the_hand_derived_answer(case):
    rs, table, tab, n_groups, off, row_ps, stranded, want_gc, want_wc = HG.hand_inputs(case)
    # the inputs are what the rule allows: sorted, a group's intervals disjoint and of one strand, every group present
    ivs = [(int(e["start"]), int(e["end"])) for e in tab]
    assert ivs == sorted(ivs) and sorted(set(tab["group"].tolist())) == list(range(n_groups))
    for g in range(n_groups):
        mine = [e for e in tab if int(e["group"]) == g]
        assert len({int(e["strand"]) for e in mine}) == 1 and all(int(a["end"]) <= int(b["start"]) for a, b in zip(mine, mine[1:]))
    gc, wc = HG.counts(rs, table, tab, n_groups, off, row_ps, stranded)
    assert gc.tolist() == want_gc.tolist() and wc.tolist() == want_wc.tolist()


def test_the_hand_cases_cover_what_they_are_for():
    names = {c[0] for c in HG.HAND}
    assert len(names) == len(HG.HAND) >= 20 and {c[4] for c in HG.HAND} == {0, 1, 2}
    by = {c[0]: HG.hand_inputs(c) for c in HG.HAND}
    rs = by["forty_m_ops_over_forty_exons"][0]
    assert int(rs.reads[0]["n_cigar"]) == 79 and hapregionref.covered(rs, 0) == [(100 + 8 * k, 103 + 8 * k) for k in range(40)]
    d = {}
    rs, table, tab, n_groups, off, row_ps = by["exon_1_and_3_and_exon_2_in_the_intron"][:6]
    HG.counts(rs, table, tab, n_groups, off, row_ps, detail=d)
    assert d == dict(pairs=1, multi_interval_pairs=1, skipped_inside_pairs=1)
    rs, table, tab, n_groups, off, row_ps = by["two_genes_with_alternating_exons"][:6]
    HG.counts(rs, table, tab, n_groups, off, row_ps, detail=d)
    assert d == dict(pairs=2, multi_interval_pairs=2, skipped_inside_pairs=0)


def test_singleton_groups_are_the_region_rule():
    _, rs, table, _ = hapref.gen_case(2, n_reads=60)
    tab, row_ps = hapregionref.gen_regions(2, table)
    ivs, n_groups, off = HG.singletons(tab)
    for stranded in (0, 1, 2):
        rc, wc = hapregionref.counts(rs, table, tab, row_ps, stranded)
        gc, gw = HG.counts(rs, table, ivs, n_groups, off, row_ps, stranded)
        assert np.array_equal(rc, gc) and np.array_equal(wc, gw) and rc.sum() + wc.sum() > 100


# ---- the driver's grouping
def test_grouping_merging_and_mixed_strands():
    lines = HG.GENE_BED["chr1"]
    groups, n_mixed = hap_expr.group_by_name(lines)
    assert groups == [("geneA", "+", [(100, 900), (2000, 2600)]), ("geneB", "-", [(3000, 3300), (4000, 4500)]), (".", None, [(500, 501)]),
                      ("geneMixed", None, [(1000, 1200), (1500, 1800)]), (".", "+", [(600, 650)])] and n_mixed == 1
    assert [tuple(g) for g in HG.grouped(lines)] == groups     # the test's own grouping says the same
    assert hap_expr.group_by_name([]) == ([], 0)
    # nested lines of one name, and abutting ones
    assert hap_expr.group_by_name([(10, 100, "g", None), (20, 30, "g", None), (100, 110, "g", None), (111, 120, "g", None)])[0] == [("g", None, [(10, 110), (111, 120)])]
    # a strand against no strand is mixed as well
    assert hap_expr.group_by_name([(10, 20, "g", "+"), (30, 40, "g", None)]) == ([("g", None, [(10, 20), (30, 40)])], 1)
    # the table: sorted by (start, end), groups numbered by first appearance, rows = the distinct ps inside any merged interval
    pos, ps = np.array([150, 600, 900, 901, 2500, 3100, 4100]), np.array([1, 2, 1, 9, 2, 5, 4])
    tab, off, row_ps = hap_expr.group_table(groups, pos, ps)
    assert tab.dtype == capi.HAP_INTERVAL_DTYPE
    assert [(int(e["start"]), int(e["end"]), int(e["group"]), int(e["strand"])) for e in tab] == [
        (100, 900, 0, 1), (500, 501, 2, 0), (600, 650, 4, 1), (1000, 1200, 3, 0), (1500, 1800, 3, 0), (2000, 2600, 0, 1), (3000, 3300, 1, 2), (4000, 4500, 1, 2)]
    # geneA: sites 150 (1), 600 (2), 900 (1; pos <= end), 2500 (2) -> [1, 2]; 901 lies outside; geneB: 5 and 4 -> [4, 5]; (600, 650): 600 is not > start
    assert off.tolist() == [0, 2, 4, 4, 4] and row_ps.tolist() == [1, 2, 4, 5]
    assert tab["reserved"].sum() == 0


class GroupEngine(LogEngine):
    def hap_group_counts(self, intervals, n_groups, group_row_off, row_ps, stranded=0):
        LogEngine.log.append(("hap_group_counts", len(intervals), n_groups, len(row_ps), stranded))
        assert len(group_row_off) == n_groups
        return HG.counts(self.rs, self.table, intervals, n_groups, group_row_off, row_ps, stranded, self.params)


def _sample(d, **kw):
    s = hapregionref.driver_sample(d, **kw)
    s["gene_bed_fn"] = os.path.join(d, "genes.bed")
    HG.write_gene_bed(s["gene_bed_fn"])
    return s


def test_the_driver_writes_the_restatements_gene_table(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "Engine", GroupEngine)
    s = _sample(str(tmp_path))
    out = str(tmp_path / "out" / "genes.tsv")
    LogEngine.log, msgs = [], []
    base = ["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["gene_bed_fn"], "--output_fn", out]
    done = hap_expr.Run(hap_expr.build_parser().parse_args(base + ["--group_by_name"]), log=msgs.append)
    got = open(out).read().split("\n")
    assert got[0] == "#CHROM\tSTART\tEND\tNAME\tSTRAND\tINTERVALS\tLENGTH\tPS\tHP1\tHP2\tUNTAGGED\tOTHER_SET" == hap_expr.GROUP_HEADER and got[-1] == ""
    want1 = HG.predicted_lines(s, "chr1")
    assert got[1:-1] == want1 + HG.uncounted_lines("chr2") + HG.uncounted_lines("chrEmpty")
    # lines worked out by hand: the span, the merged intervals and their summed length; groups in order of first appearance
    heads = [l.split("\t")[:7] for l in want1 if l.split("\t")[7] == "."]
    assert heads == [["chr1", "100", "2600", "geneA", "+", "2", "1400"], ["chr1", "3000", "4500", "geneB", "-", "2", "800"], ["chr1", "500", "501", ".", ".", "1", "1"],
                     ["chr1", "1000", "1800", "geneMixed", ".", "2", "500"], ["chr1", "600", "650", ".", "+", "1", "50"]]
    assert HG.uncounted_lines("chr2") == ["chr2\t10\t1100\tg2\t+\t2\t990\t.\t.\t.\t.\t."]
    body = [l.split("\t") for l in want1]
    assert sum(int(l[8]) + int(l[9]) for l in body if l[7] != ".") >= 30          # of 83 reads, each once per gene at most: the comparison is about something
    n1 = len(s["reads"]["chr1"])
    assert LogEngine.log == [("engine", 0), ("set_params", dict(min_mq=5)), ("set_phase_sites", len(s["case"]["chr1"])), ("load_reads", n1),
                             ("hap_group_counts", 8, 5, len(body) - 5, 0), ("close",)]
    assert sorted(done) == ["chr1", "chr2", "chrEmpty"] and done["chr1"]["launched"] and not done["chr2"]["launched"]
    assert done["chr1"]["groups"] == 5 and done["chr1"]["regions"] == 10 and done["chr1"]["skipped"] == 1 and done["chr1"]["rows"] == len(body) - 5
    warnings = [m for m in msgs if m.startswith("[WARNING]")]
    assert warnings == ["[WARNING] chr1: 1 groups have BED lines of more than one strand: they are counted without a strand"]
    infos = [m for m in msgs if m.startswith("[INFO]")]
    assert len(infos) == 3 and infos[0].startswith("[INFO] chr1: 5 groups of 10 regions (1 BED lines with end <= start skipped), %d phase-set rows, %d reads, " % (len(body) - 5, n1))
    assert infos[1].startswith("[INFO] chr2: 1 groups of 2 regions") and "nothing counted" in infos[1] and infos[2].startswith("[INFO] chrEmpty: 1 groups of 1 regions")
    assert os.listdir(os.path.dirname(out)) == ["genes.tsv"]
    # --stranded and --min_mq reach the engine and the table
    LogEngine.log = []
    hap_expr.Run(hap_expr.build_parser().parse_args(base + ["--group_by_name", "--stranded", "same", "--min_mq", "30", "--ctg_name", "chr1"]), log=msgs.append)
    assert ("hap_group_counts", 8, 5, len(body) - 5, 1) in LogEngine.log and ("set_params", dict(min_mq=30)) in LogEngine.log
    got2 = open(out).read().split("\n")
    assert got2[1:-1] == HG.predicted_lines(s, "chr1", stranded=1, params=dict(min_mq=30, excl_flags=2316)) != want1
    # without the flag: the same BED gives the file the region restatement predicts, through hap_region_counts alone
    LogEngine.log = []
    hap_expr.Run(hap_expr.build_parser().parse_args(base), log=msgs.append)
    s_regions = dict(s, bed=HG.GENE_BED)
    got3 = open(out).read().split("\n")
    assert got3[0] == hap_expr.HEADER and got3[1:-1] == (hapregionref.predicted_lines(s_regions, "chr1") + hapregionref.uncounted_lines(s_regions, "chr2")
                                                         + hapregionref.uncounted_lines(s_regions, "chrEmpty"))
    assert [c[0] for c in LogEngine.log] == ["engine", "set_params", "set_phase_sites", "load_reads", "hap_region_counts", "close"]


def test_a_failed_contig_leaves_no_file(tmp_path, monkeypatch):
    class Failing(GroupEngine):
        def hap_group_counts(self, *a, **kw):
            raise capi.C3RError(-1, "interval 3: refused")

    monkeypatch.setattr(capi, "Engine", Failing)
    s = _sample(str(tmp_path), n_reads=20)
    out = str(tmp_path / "o" / "genes.tsv")
    LogEngine.log = []
    with pytest.raises(capi.C3RError, match="interval 3: refused"):
        hap_expr.Run(hap_expr.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["gene_bed_fn"], "--output_fn", out,
                                                         "--group_by_name"]), log=lambda m: None)
    assert os.listdir(os.path.dirname(out)) == [] and LogEngine.log[-1] == ("close",)


def test_the_help_states_what_the_flag_does_and_does_not():
    text = " ".join(hap_expr.build_parser().format_help().split())
    for words in ("--group_by_name", "counts once per group", "No GTF reader", "no fractional assignment", "no statistics"):
        assert words in text, words


# ---- the two drivers' refusals
def test_hap_expr_refusals_leave_no_file(tmp_path):
    s = _sample(str(tmp_path), n_reads=20)
    out = str(tmp_path / "refused.tsv")
    base = ["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["gene_bed_fn"], "--output_fn", out, "--group_by_name"]
    for extra, words in ((["--left_align_indels"], "--haplotag_indels"), (["--hap_realign"], "--ref_fn"), (["--hap_min_bq", "200"], "--hap_min_bq")):
        with pytest.raises(SystemExit) as e:
            hap_expr.Run(hap_expr.build_parser().parse_args(base + extra), log=lambda m: None)
        assert "[ERROR]" in str(e.value.code) and words in str(e.value.code), e.value.code
    argv = list(base)
    argv[argv.index("--regions_bed_fn") + 1] = str(tmp_path / "nope.bed")
    with pytest.raises(SystemExit) as e:
        hap_expr.Run(hap_expr.build_parser().parse_args(argv), log=lambda m: None)
    assert "not found" in str(e.value.code)
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")


def test_call_sample_refuses_the_flag_without_its_bed_and_hands_it_to_the_step(tmp_path):
    from clair3_rna_amd import call_sample
    bed = str(tmp_path / "exons.bed")
    open(bed, "w").write("chr1\t1\t2\tg\n")
    phased = str(tmp_path / "p.vcf")
    open(phased, "w").close()
    out = str(tmp_path / "out")
    base = ["--bam_fn", str(tmp_path / "x.bam"), "--ref_fn", str(tmp_path / "x.fa"), "--output_dir", out, "--pileup_model_path", "w18",
            "--phased_pileup_model_path", "w30"]
    with pytest.raises(SystemExit) as e:
        call_sample.Run(call_sample.build_parser().parse_args(base + ["--hap_expression_group_by_name", "--enable_phasing_model", "--phased_vcf_fn", phased]))
    msg = str(e.value.code)
    assert msg.startswith("[ERROR] --hap_expression_group_by_name") and "--hap_expression_bed" in msg and "\n" not in msg
    with pytest.raises(SystemExit) as e:                      # the BED's own conditions come first
        call_sample.Run(call_sample.build_parser().parse_args(base + ["--hap_expression_bed", bed, "--hap_expression_group_by_name"]))
    assert str(e.value.code).startswith("[ERROR] --hap_expression_bed") and "--enable_phasing_model" in str(e.value.code)
    assert not os.path.exists(out)
    stem = os.path.join(out, "output_enable_phasing")
    flags = ["--hap_expression_bed", bed, "--enable_phasing_model", "--phased_vcf_fn", phased, "--hap_expression_stranded", "reverse", "--hap_min_bq", "7", "--gpu_id", "2"]
    plan = call_sample._plan(call_sample.build_parser().parse_args(base + flags + ["--hap_expression_group_by_name"]))
    assert [st.name for st in plan] == ["pass", "hap_expr"]
    assert plan[-1].handed == ["--phased_vcf_fn", phased, "--regions_bed_fn", bed, "--output_fn", stem + "_hap_expression_by_name.tsv", "--min_mq", "5", "--stranded", "reverse",
                               "--group_by_name", "--hap_min_bq", "7", "--gpu_id", "2"]
    assert hap_expr.build_parser().parse_args(["--bam_fn", "x"] + plan[-1].handed).group_by_name
    # without it: the step of the parent
    plain = call_sample._plan(call_sample.build_parser().parse_args(base + flags))
    assert plain[-1].handed == ["--phased_vcf_fn", phased, "--regions_bed_fn", bed, "--output_fn", stem + "_hap_expression.tsv", "--min_mq", "5", "--stranded", "reverse",
                                "--hap_min_bq", "7", "--gpu_id", "2"]
    assert not hap_expr.build_parser().parse_args(["--bam_fn", "x"] + plain[-1].handed).group_by_name
    assert not os.path.exists(out)
