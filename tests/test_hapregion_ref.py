"""The rule `hap_regions` (include/c3r.h: c3r_hap_region_counts) on the CPU: the restatement of tests/hapregionref.py against answers worked out
by hand, first_open and the bound, io.read_bed_regions, the hap_expr driver with the engine replaced by a stub that logs its calls and answers
from the restatement, and call_sample's rules for --hap_expression_bed.  tests/test_gpu_hapregion.py runs the same tables on the device."""
import gzip
import os

import pytest

from clair3_rna_amd import capi, hap_expr, io
from clair3_rna_amd.reads import NT16, ReadSet
from tests import hapref, hapregionref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule by hand
@pytest.mark.parametrize("case", hapregionref.HAND, ids=[c[0] for c in hapregionref.HAND])
def test_the_restatement_gives_the_hand_derived_answer(case):
    rs, table, tab, row_ps, stranded, want_rc, want_wc = hapregionref.hand_inputs(case)
    rc, wc = hapregionref.counts(rs, table, tab, row_ps, stranded)
    assert rc.tolist() == want_rc.tolist() and wc.tolist() == want_wc.tolist()


def test_the_hand_cases_cover_what_they_are_for():
    names = {c[0] for c in hapregionref.HAND}
    assert len(names) == len(hapregionref.HAND) >= 20
    assert {c[3] for c in hapregionref.HAND} == {0, 1, 2}
    # the covered stretches of the spliced read and of the one with every odd op
    rs = ReadSet.from_records([dict(pos=100, cigar="10M50N10M", seq="A" * 20, flag=0, mapq=60, hp=0), dict(pos=100, cigar="2H4=0D1X1P5M50N10M3H", seq="A" * 20, flag=0, mapq=60, hp=0),
                               dict(pos=100, cigar="5M3D5M", seq="A" * 10, flag=0, mapq=60, hp=0)])
    assert hapregionref.covered(rs, 0) == [(100, 110), (160, 170)] == hapregionref.covered(rs, 1)
    assert hapregionref.covered(rs, 2) == [(100, 105), (105, 108), (108, 113)]


def test_a_new_min_mq_changes_the_voters():
    rs, table, tab, row_ps, _, _, _ = hapregionref.hand_inputs(("x", [(100, "10M", "A" * 10, 0, 20), (100, "10M", "A" * 10, 0, 40)], [(100, 110, 0, [7])], 0, [], []))
    for min_mq, n in ((5, 2), (30, 1), (41, 0)):
        assert hapregionref.counts(rs, table, tab, row_ps, 0, dict(min_mq=min_mq, excl_flags=2316))[1].tolist() == [[n, 0]]


# ---- first_open and the bound
def nested_table(n_short, long_at=0):
    """One region over everything at index long_at = 0 (it starts first) and n_short regions of 10 bases, 20 apart, behind its start."""
    regs = [(0, 20 * n_short + 100, 0)] + [(10 + 20 * k, 20 + 20 * k, 0) for k in range(n_short)]
    return hapregionref.pack(regs, [[] for _ in regs])[0]


def test_first_open_and_the_bound_on_a_nested_table():
    tab = hapregionref.pack([(0, 10, 0), (5, 100, 0), (20, 30, 0), (20, 30, 0), (40, 50, 0), (100, 110, 0), (105, 106, 0)], [[]] * 7)[0]
    # region 1 stays open under 2, 3, 4; it ends at 100, where 5 starts
    assert hapregionref.first_open(tab) == [0, 0, 1, 1, 1, 5, 5]
    assert hapregionref.max_back(tab) == 3 == hap_expr.max_back(tab)
    for n in (1, 50, 300):
        t = nested_table(n)
        assert hapregionref.max_back(t) == n == hap_expr.max_back(t)
    assert capi.HAP_REGION_MAX_BACK == hapregionref.MAX_BACK == 4096
    disjoint = hapregionref.pack([(10 * k, 10 * k + 10, 0) for k in range(100)], [[]] * 100)[0]
    assert hap_expr.max_back(disjoint) == 0 and hap_expr.max_back(disjoint[:0]) == 0


class LogEngine(object):
    """What hap_expr asks of capi.Engine, logged, and answered by the restatements."""
    log = []

    def __init__(self, device=0):
        LogEngine.log.append(("engine", device))

    def set_params(self, **kw):
        self.params = dict(hapregionref.DEFAULT_PARAMS, **kw)
        LogEngine.log.append(("set_params", kw))

    def set_phase_sites(self, table):
        self.table = table
        LogEngine.log.append(("set_phase_sites", len(table)))

    def set_phase_alleles(self, sites, *rest):
        LogEngine.log.append(("set_phase_alleles", len(sites)))
        self.table = hapref.make_sites([(int(s["pos"]), NT16[int(s["a_base"])], NT16[int(s["b_base"])], int(h), int(s["ps"])) for s, h in zip(sites, rest[0])])

    def load_reads(self, rs):
        self.rs = rs
        LogEngine.log.append(("load_reads", len(rs)))

    def hap_region_counts(self, regions, row_ps, stranded=0):
        LogEngine.log.append(("hap_region_counts", len(regions), len(row_ps), stranded))
        if hapregionref.max_back(regions) > hapregionref.MAX_BACK:
            raise capi.C3RError(-1, "region over C3R_HAP_REGION_MAX_BACK")
        return hapregionref.counts(self.rs, self.table, regions, row_ps, stranded, self.params)

    def close(self):
        LogEngine.log.append(("close",))


def test_the_split_at_the_median_length_and_its_refusal():
    ref, rs, sites, _ = hapref.gen_case(0, n_reads=40)
    eng = LogEngine()
    eng.set_params()
    eng.set_phase_sites(sites)
    eng.load_reads(rs)
    n = hapregionref.MAX_BACK + 4
    # one gene over n short exons: over the bound as one table, under it as two
    regions = [(0, 5900, "gene", None)] + [(10 + k, 11 + k, "e%d" % k, None) for k in range(n)]
    LogEngine.log = []
    got = hap_expr.count_regions(eng, regions, sites["pos"], sites["ps"])
    calls = [c for c in LogEngine.log if c[0] == "hap_region_counts"]
    assert len(calls) == 2 and sorted(c[1] for c in calls) == [1, n]
    tab, row_ps, order = hap_expr.region_table(regions[:40], sites["pos"], sites["ps"])
    rc, wc = hapregionref.counts(rs, sites, tab, row_ps)
    for k, o in enumerate(order):
        assert got[o][0] == tuple(rc[k].tolist())
    assert len(got[0][1]) == len(set(sites["ps"][sites["pos"] <= 5900].tolist())) and sum(h1 + h2 for _, h1, h2 in got[0][1]) > 10
    # equal regions by the thousand lie over each other whatever the cut: no split helps, the one call is refused with the library's message
    regions = [(0, 5900, "g%d" % k, None) for k in range(n)] + [(0, 5900, "h", None)]
    LogEngine.log = []
    with pytest.raises(capi.C3RError, match="C3R_HAP_REGION_MAX_BACK"):
        hap_expr.count_regions(eng, regions, sites["pos"], sites["ps"])
    assert [c[1] for c in LogEngine.log] == [n + 1]


# ---- io.read_bed_regions
def test_read_bed_regions(tmp_path):
    text = ("# a comment\ntrack name=x\nbrowser position chr1:1-2\n\n"
            "chr1\t100\t200\tgeneA\t0\t+\n"
            "chr2\t5\t9\tother\t0\t-\n"
            "chr1\t50\t60\n"
            "chr1\t300\t300\tempty\t0\t+\n"
            "chr1\t400\t390\tbackwards\n"
            "chr1\t100\t200\tgene B\t.\t-\textra\n"
            "chr1\t7\t8\t\t0\t.\n"
            "chr1 20 30 spaced 0 +\n")
    fn = str(tmp_path / "r.bed")
    open(fn, "w").write(text)
    got = io.read_bed_regions(fn, "chr1")
    assert list(got) == [(100, 200, "geneA", "+"), (50, 60, ".", None), (100, 200, "gene B", "-"), (7, 8, ".", None), (20, 30, "spaced", "+")]
    assert got.n_skipped == 2
    assert list(io.read_bed_regions(fn, "chr2")) == [(5, 9, "other", "-")] and io.read_bed_regions(fn, "chr2").n_skipped == 0
    assert list(io.read_bed_regions(fn, "chr3")) == []
    gz = str(tmp_path / "r.bed.gz")
    with gzip.open(gz, "wt") as f:
        f.write(text)
    assert list(io.read_bed_regions(gz, "chr1")) == list(got)
    assert hap_expr.bed_contigs(fn) == ["chr1", "chr2"]
    # io.read_bed is what it was: it widens start == end and refuses end < start
    open(str(tmp_path / "r2.bed"), "w").write("chr1\t5\t5\nchr1\t9\t12\n")
    assert io.read_bed(str(tmp_path / "r2.bed"), "chr1") == ([(5, 6), (9, 12)], 5, 12)


# ---- the driver
sample, predicted_lines, uncounted_lines = hapregionref.driver_sample, hapregionref.predicted_lines, hapregionref.uncounted_lines


def test_the_driver_writes_the_restatements_table(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "Engine", LogEngine)
    s = sample(str(tmp_path))
    out = str(tmp_path / "out" / "expr.tsv")
    LogEngine.log, msgs = [], []
    done = hap_expr.Run(hap_expr.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["bed_fn"], "--output_fn", out, "--gpu_id", "3"]),
                        log=msgs.append)
    got = open(out).read().split("\n")
    assert got[0] == "#CHROM\tSTART\tEND\tNAME\tSTRAND\tPS\tHP1\tHP2\tUNTAGGED\tOTHER_SET" == hap_expr.HEADER and got[-1] == ""
    # contigs in the header's order (chr1 before chr2, whatever the BED says), regions in BED order; a contig without a phased site or without
    # a read: summary lines with `.`; a BED contig the BAM does not know and a BAM contig the BED does not name: nothing
    want = predicted_lines(s, "chr1") + uncounted_lines(s, "chr2") + uncounted_lines(s, "chrEmpty")
    assert got[1:-1] == want
    body = [l.split("\t") for l in predicted_lines(s, "chr1")]
    assert sum(l[5] != "." for l in body) >= 10 and sum(int(l[6]) + int(l[7]) for l in body if l[5] != ".") >= 50 and sum(int(l[9]) for l in body if l[5] == ".") >= 20
    assert sorted(done) == ["chr1", "chr2", "chrEmpty"] and done["chr1"]["launched"] and not done["chr2"]["launched"] and done["chr1"]["skipped"] == 1
    assert done["chr1"]["regions"] == 5 and done["chr1"]["rows"] == len(body) - 5
    n1 = len(s["reads"]["chr1"])
    assert LogEngine.log == [("engine", 3), ("set_params", dict(min_mq=5)), ("set_phase_sites", len(s["case"]["chr1"])), ("load_reads", n1),
                             ("hap_region_counts", 5, len(body) - 5, 0), ("close",)]
    assert len(msgs) == 3 and msgs[0].startswith("[INFO] chr1: 5 regions (1 BED lines with end <= start skipped), %d phase-set rows, %d reads, " % (len(body) - 5, n1))
    assert "nothing counted" in msgs[1] and msgs[1].startswith("[INFO] chr2: 1 regions") and "nothing counted" in msgs[2]
    assert os.listdir(os.path.dirname(out)) == ["expr.tsv"]
    # --stranded, --min_mq and --ctg_name reach the engine and the table
    LogEngine.log = []
    hap_expr.Run(hap_expr.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["bed_fn"], "--output_fn", out, "--stranded", "reverse",
                                                     "--min_mq", "30", "--ctg_name", "chr1,chrNope"]), log=msgs.append)
    assert ("set_params", dict(min_mq=30)) in LogEngine.log and ("hap_region_counts", 5, len(body) - 5, 2) in LogEngine.log and LogEngine.log[0] == ("engine", 0)
    got2 = open(out).read().split("\n")
    assert got2[1:-1] == predicted_lines(s, "chr1", 2, dict(min_mq=30, excl_flags=2316)) and got2[1:-1] != want[:len(got2) - 2]


def test_the_tagging_flags_go_through_the_helpers_of_haplotag_bam(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "Engine", LogEngine)
    s = sample(str(tmp_path), n_reads=30)
    out = str(tmp_path / "expr.tsv")
    LogEngine.log = []
    hap_expr.Run(hap_expr.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["bed_fn"], "--output_fn", out, "--haplotag_indels"]),
                 log=lambda m: None)
    assert [c[0] for c in LogEngine.log] == ["engine", "set_params", "set_phase_alleles", "load_reads", "hap_region_counts", "close"]
    assert open(out).read().split("\n")[1:-1] == predicted_lines(s, "chr1") + uncounted_lines(s, "chr2") + uncounted_lines(s, "chrEmpty")
    # the flags haplotag_bam takes, with its defaults and its refusals
    from clair3_rna_amd import haplotag_bam
    mine = {a.dest: a for a in hap_expr.build_parser()._actions}
    for a in haplotag_bam.build_parser()._actions:
        if a.dest in ("haplotag_indels", "left_align_indels", "ref_fn", "hap_realign", "hap_realign_spliced", "hap_min_bq", "hap_bq_weights", "gpu_id", "threads"):
            assert a.dest in mine and mine[a.dest].default == a.default and mine[a.dest].option_strings == a.option_strings and mine[a.dest].nargs == a.nargs, a.dest
    assert mine["min_mq"].default == 5 and mine["stranded"].default == "no" and sorted(mine["stranded"].choices) == ["no", "reverse", "same"]
    base = ["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["bed_fn"], "--output_fn", str(tmp_path / "refused.tsv")]
    for extra, words in ((["--left_align_indels"], "--haplotag_indels"), (["--hap_realign"], "--ref_fn"), (["--hap_min_bq", "200"], "--hap_min_bq")):
        with pytest.raises(SystemExit) as e:
            hap_expr.Run(hap_expr.build_parser().parse_args(base + extra), log=lambda m: None)
        assert "[ERROR]" in str(e.value.code) and words in str(e.value.code), e.value.code
    for missing in ("--bam_fn", "--regions_bed_fn", "--phased_vcf_fn"):
        argv = list(base)
        argv[argv.index(missing) + 1] = str(tmp_path / "nope")
        with pytest.raises(SystemExit) as e:
            hap_expr.Run(hap_expr.build_parser().parse_args(argv), log=lambda m: None)
        assert "not found" in str(e.value.code)
    assert not os.path.exists(str(tmp_path / "refused.tsv")) and not os.path.exists(str(tmp_path / "refused.tsv.tmp"))


def test_a_failed_contig_leaves_no_file(tmp_path, monkeypatch):
    class Failing(LogEngine):
        def hap_region_counts(self, regions, row_ps, stranded=0):
            raise capi.C3RError(-1, "region 3: refused")

    monkeypatch.setattr(capi, "Engine", Failing)
    s = sample(str(tmp_path), n_reads=20)
    out = str(tmp_path / "o" / "expr.tsv")
    LogEngine.log = []
    with pytest.raises(capi.C3RError, match="region 3: refused"):
        hap_expr.Run(hap_expr.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["bed_fn"], "--output_fn", out]), log=lambda m: None)
    assert os.listdir(os.path.dirname(out)) == [] and LogEngine.log[-1] == ("close",)


def test_the_help_states_the_limits():
    text = " ".join(hap_expr.build_parser().format_help().split())
    for words in ("counts once in every region", "no gene-level union", "no fractional assignment", "no statistics", "has not been measured"):
        assert words in text, words


# ---- call_sample
def test_call_sample_refuses_the_flag_where_it_cannot_work_and_hands_the_step_its_argv(tmp_path, monkeypatch):
    from clair3_rna_amd import call_sample
    bed = str(tmp_path / "exons.bed")
    open(bed, "w").write("chr1\t1\t2\n")
    phased = str(tmp_path / "p.vcf")
    open(phased, "w").close()
    out = str(tmp_path / "out")
    base = ["--bam_fn", str(tmp_path / "x.bam"), "--ref_fn", str(tmp_path / "x.fa"), "--output_dir", out, "--pileup_model_path", "w18",
            "--phased_pileup_model_path", "w30"]

    def refused(extra, *words, **kw):
        with pytest.raises(SystemExit) as e:
            call_sample.Run(call_sample.build_parser().parse_args(base + extra))
        assert str(e.value.code).startswith("[ERROR] " + kw.get("head", "--hap_expression_bed")) and all(w in str(e.value.code) for w in words), e.value.code

    flag = ["--hap_expression_bed", bed]
    refused(flag, "--enable_phasing_model")
    refused(flag + ["--phasing", "builtin"], "--enable_phasing_model")
    refused(flag + ["--enable_phasing_model"], "--phased_vcf_fn", "--phasing builtin")
    refused(["--hap_expression_bed", str(tmp_path / "nope.bed"), "--enable_phasing_model", "--phased_vcf_fn", phased], "not found", head="file")
    refused(["--hap_expression_stranded", "same", "--enable_phasing_model", "--phased_vcf_fn", phased], "--hap_expression_bed", head="--hap_expression_stranded")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(flag + ["--enable_phasing_model", "--phased_vcf_fn", phased], "WORLD_SIZE", "python -m clair3_rna_amd.hap_expr")
    refused(flag + ["--enable_phasing_model", "--phasing", "builtin"], "WORLD_SIZE", "python -m clair3_rna_amd.hap_expr")
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert not os.path.exists(out)
    # the plan: one more step behind the others, with the tagging flags haplotag_bam gets
    stem = os.path.join(out, "output_enable_phasing")
    plan = call_sample._plan(call_sample.build_parser().parse_args(base + flag + ["--enable_phasing_model", "--phased_vcf_fn", phased, "--haplotagged_bam", "--phase_output",
                                                                                   "--haplotag_indels", "--hap_min_bq", "7", "--hap_expression_stranded", "reverse", "--gpu_id", "2"]))
    assert [st.name for st in plan] == ["pass", "hap_vcf", "clear", "haplotag_bam", "hap_expr"]
    step, tagger = plan[-1], plan[-2]
    assert step.needs == stem + ".vcf.gz" == tagger.needs
    assert step.handed == ["--phased_vcf_fn", phased, "--regions_bed_fn", bed, "--output_fn", stem + "_hap_expression.tsv", "--min_mq", "5", "--stranded", "reverse",
                           "--haplotag_indels", "--hap_min_bq", "7", "--gpu_id", "2"]
    assert step.handed[10:] == tagger.handed[4:]                # what follows haplotag_bam's --phased_vcf_fn / --output_dir
    hap_expr.build_parser().parse_args(["--bam_fn", "x"] + step.handed)
    builtin = call_sample._plan(call_sample.build_parser().parse_args(base + flag + ["--enable_phasing_model", "--phasing", "builtin", "--phasing_indels"]))
    assert [st.name for st in builtin] == ["pass", "clear", "phase_vcf", "pass", "hap_expr"]
    assert builtin[-1].handed[:2] == ["--phased_vcf_fn", os.path.join(out, "tmp", "phased_output", "phased_vcf")] and "--haplotag_indels" in builtin[-1].handed
    # without the flag: the plan of the parent
    plain = call_sample._plan(call_sample.build_parser().parse_args(base + ["--enable_phasing_model", "--phased_vcf_fn", phased, "--haplotagged_bam"]))
    assert [st.name for st in plain] == ["pass", "clear", "haplotag_bam"]
    assert not os.path.exists(out)
