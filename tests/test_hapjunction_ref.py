"""The rule `hap_junctions` (include/c3r.h: c3r_hap_junction_counts) on the CPU: the restatement of tests/hapjunctionref.py against answers
worked out by hand, the TSV lines and the motif / strand table, the hap_junctions driver with the engine replaced by a stub that logs its
calls and answers from the restatement, and call_sample's rules for --hap_junctions.  tests/test_gpu_hap_junctions.py runs the same cases
on the device."""
import os

import numpy as np
import pytest

from clair3_rna_amd import capi, hap_junctions
from clair3_rna_amd.reads import NT16
from tests import hapjunctionref as HJ
from tests import hapref


# ---- the rule by hand
@pytest.mark.parametrize("case", HJ.HAND, ids=[c[0] for c in HJ.HAND])
def test_the_restatement_gives_the_hand_derived_answer(case):
    rs, table, want = HJ.hand_inputs(case)
    got = HJ.counts(rs, table)
    assert got == want and HJ.invariant(got)
    # without a table: the same junctions, every read untagged, no rows
    bare = HJ.counts(rs, None)
    assert {k: (e["reads"], e["reverse"]) for k, e in bare.items()} == {k: (e["reads"], e["reverse"]) for k, e in want.items()}
    assert all(e["untagged"] == e["reads"] and not e["rows"] for e in bare.values())


def test_the_hand_cases_cover_what_they_are_for():
    names = {c[0] for c in HJ.HAND}
    assert len(names) == len(HJ.HAND) >= 15
    rs = HJ.readset([(100, "2H4=0D1X1P5M50N1P4=6X3H", HJ.A20), (100, "10M20N1P0I30N10M", HJ.A20), (100, "5M3I10N5M", "A" * 13), (100, "10M0N10M", HJ.A20)])
    assert HJ.normalised(rs, 0) == [("M", 10), ("N", 50), ("M", 10)] == HJ.normalised(rs, 1)
    assert HJ.normalised(rs, 2) == [("M", 5), ("I", 3), ("N", 10), ("M", 5)] and HJ.read_junctions(rs, 2) == [(105, 115)]
    assert HJ.normalised(rs, 3) == [("M", 20)] and HJ.read_junctions(rs, 3) == []
    ends = [k[1] for c in HJ.HAND for k in c[2]]
    assert max(ends) == 2 ** 31 - 1 and min(k[0] for c in HJ.HAND for k in c[2]) == 0
    assert any(v[1] for c in HJ.HAND for v in c[2].values()) and any(v[3].get(7, (0, 0))[1] for c in HJ.HAND for v in c[2].values())


def test_the_arrays_are_sorted_and_their_rows_follow_row_off():
    rs, table, _ = HJ.hand_inputs(("x", [(100, "10M60N10M", HJ.C20), (100, "10M50N10M", HJ.A20), (100, "5M10N5M20N10M", HJ.A20)], {}))
    j, r = HJ.arrays(HJ.counts(rs, table))
    assert j.dtype == capi.HAP_JUNCTION_DTYPE and r.dtype == capi.HAP_JUNCTION_ROW_DTYPE and j.itemsize == 24 and r.itemsize == 12
    assert [(int(e["start"]), int(e["end"])) for e in j] == [(105, 115), (110, 160), (110, 170), (120, 140)]
    assert j["row_off"].tolist() == [0, 1, 2, 3] and len(r) == 4
    assert all(int(e["reads"]) == 1 and int(e["untagged"]) == 0 for e in j)
    assert [(int(x["ps"]), int(x["hp1"]), int(x["hp2"])) for x in r] == [(7, 1, 0), (7, 1, 0), (7, 0, 1), (7, 1, 0)]


def test_a_new_min_mq_changes_the_counted_reads():
    rs = HJ.readset([(100, "10M50N10M", HJ.A20, 0, 20), (100, "10M50N10M", HJ.A20, 16, 40), (100, "10M50N10M", HJ.A20, 4, 60), (100, "10M50N10M", HJ.A20, 1, 60),
                     (100, "10M50N10M", HJ.A20, 3, 60)])
    for min_mq, n, rev in ((5, 3, 1), (30, 2, 1), (41, 1, 0), (61, 0, 0)):
        got = HJ.counts(rs, None, dict(min_mq=min_mq, excl_flags=2316))
        assert (got[(110, 160)]["reads"], got[(110, 160)]["reverse"]) == (n, rev) if n else got == {}


def test_the_generated_cases_hold_what_the_gpu_tests_need():
    untagged = 0
    for seed in range(4):
        rs, table = HJ.shared_case(seed)
        found = HJ.counts(rs, table)
        assert HJ.invariant(found)
        assert len(found) >= 10 and max(e["reads"] for e in found.values()) >= 50 and sum(len(e["rows"]) >= 2 for e in found.values()) >= 5
        untagged += sum(e["untagged"] > 0 for e in found.values())
    assert untagged >= 1
    rs, table = HJ.distinct_case(0)
    found = HJ.counts(rs, table)
    assert HJ.invariant(found) and len(found) >= 1500 and len(rs) <= 400


# ---- the TSV and the motif table
def test_motif_and_strand():
    #      0         1         2
    #      0123456789012345678901234
    seq = "AAGTCCCCAGAActccacTTgcAAG"
    assert HJ.motif(seq, 2, 10) == ("GT-AG", "+") == hap_junctions.motif(seq, 2, 10)
    assert HJ.motif(seq, 12, 18) == ("CT-AC", "-") == hap_junctions.motif(seq, 12, 18)            # lower case in the file
    assert HJ.motif(seq, 20, 25) == ("GC-AG", "+") == hap_junctions.motif(seq, 20, 25)            # ends with the sequence
    assert HJ.motif(seq, 20, 26) == (".", ".") == hap_junctions.motif(seq, 20, 26)                # one past it
    assert HJ.motif(seq, 24, 30) == (".", ".") == hap_junctions.motif(seq, 24, 30)                # starts on the last base
    assert HJ.motif(seq, 0, 4) == ("AA-GT", ".") == hap_junctions.motif(seq, 0, 4)
    assert HJ.motif(seq, 2, 3) == ("GT-AG", "+") == hap_junctions.motif(seq, 2, 3)                # an intron of one base: the pairs overlap
    assert HJ.motif(seq, 0, 1) == (".", ".") == hap_junctions.motif(seq, 0, 1)                    # no two bases before its end
    assert HJ.motif(None, 2, 10) == (".", ".") == hap_junctions.motif(None, 2, 10)
    for m, strand in (("GT-AG", "+"), ("GC-AG", "+"), ("AT-AC", "+"), ("CT-AC", "-"), ("CT-GC", "-"), ("GT-AT", "-"), ("AA-AA", "."), ("NN-AG", ".")):
        s = m[:2].lower() + "TTTT" + m[3:]
        assert HJ.motif(s, 0, 8) == (m, strand) == hap_junctions.motif(s, 0, 8)
    assert hap_junctions.MOTIF_STRAND == dict([(m, "+") for m in HJ.PLUS] + [(m, "-") for m in HJ.MINUS])


def test_the_lines_byte_for_byte():
    found = {(110, 160): dict(reads=5, reverse=2, untagged=1, rows={1002: [0, 1], 7: [3, 0]}), (2, 10): dict(reads=1, reverse=0, untagged=1, rows={})}
    seq = "AAGTCCCCAGAA"
    want = ["chrX\t2\t10\tGT-AG\t+\t1\t0\t.\t.\t.\t1",
            "chrX\t110\t160\t.\t.\t5\t2\t.\t.\t.\t1",
            "chrX\t110\t160\t.\t.\t.\t.\t7\t3\t0\t.",
            "chrX\t110\t160\t.\t.\t.\t.\t1002\t0\t1\t."]
    assert HJ.lines("chrX", found, seq) == want == hap_junctions.junction_lines("chrX", *HJ.arrays(found), seq=seq)
    assert HJ.lines("chrX", found, None, 2) == [l.replace("GT-AG\t+", ".\t.") for l in want[1:]] == hap_junctions.junction_lines("chrX", *HJ.arrays(found), min_reads=2)
    assert HJ.lines("chrX", {}) == [] == hap_junctions.junction_lines("chrX", *HJ.arrays({}))
    assert hap_junctions.HEADER == HJ.HEADER == "#CHROM\tSTART\tEND\tMOTIF\tSTRAND\tREADS\tREVERSE\tPS\tHP1\tHP2\tUNTAGGED"


# ---- the driver
class LogEngine(object):
    """What hap_junctions asks of capi.Engine, logged, and answered by the restatements."""
    log = []

    def __init__(self, device=0):
        self.table = None
        LogEngine.log.append(("engine", device))

    def set_params(self, **kw):
        self.params = dict(HJ.DEFAULT_PARAMS, **kw)
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

    def hap_junction_counts(self, slots_hint=0):
        LogEngine.log.append(("hap_junction_counts", slots_hint))
        return HJ.arrays(HJ.counts(self.rs, self.table, self.params))

    def close(self):
        LogEngine.log.append(("close",))


def _run(argv, log=None):
    return hap_junctions.Run(hap_junctions.build_parser().parse_args(argv), log=log or (lambda m: None))


def test_the_driver_writes_the_restatements_table(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "Engine", LogEngine)
    s = HJ.driver_sample(str(tmp_path))
    out = str(tmp_path / "out" / "junctions.tsv")
    LogEngine.log, msgs = [], []
    done = _run(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--output_fn", out, "--gpu_id", "3"], msgs.append)
    got = open(out).read().split("\n")
    assert got[0] == HJ.HEADER and got[-1] == ""
    # contigs in the header's order; chr2 has no phased site and is counted all the same, every read untagged; chrEmpty has no read
    want1, want2 = HJ.predicted_lines(s, "chr1"), HJ.predicted_lines(s, "chr2")
    assert got[1:-1] == want1 + want2
    body = [l.split("\t") for l in want1]
    assert sum(l[7] != "." for l in body) >= 20 and sum(int(l[8]) + int(l[9]) for l in body if l[7] != ".") >= 100 and sum(int(l[10]) for l in body if l[7] == ".") >= 1
    assert all(l.split("\t")[7] == "." and l.split("\t")[5] == l.split("\t")[10] for l in want2) and len(want2) >= 100
    assert sorted(done) == ["chr1", "chr2", "chrEmpty"] and done["chrEmpty"] == dict(junctions=0, written=0, rows=0, reads=0, sites=0)
    assert done["chr1"]["rows"] == sum(l[7] != "." for l in body) and done["chr1"]["junctions"] == done["chr1"]["written"] == len(body) - done["chr1"]["rows"]
    n1, n2 = len(s["reads"]["chr1"]), len(s["reads"]["chr2"])
    assert LogEngine.log == [("engine", 3), ("set_params", dict(min_mq=5)), ("set_phase_sites", len(s["case"]["chr1"])), ("load_reads", n1), ("hap_junction_counts", 0),
                             ("set_phase_sites", 0), ("load_reads", n2), ("hap_junction_counts", 0), ("close",)]
    assert len(msgs) == 3 and msgs[0].startswith("[INFO] chr1: %d junctions (%d with at least 1 reads written), %d phase-set rows, %d reads, " % (
        done["chr1"]["junctions"], done["chr1"]["junctions"], done["chr1"]["rows"], n1))
    assert "every read is untagged" in msgs[1] and "every read is untagged" not in msgs[0] and msgs[2].startswith("[INFO] chrEmpty: 0 junctions")
    assert os.listdir(os.path.dirname(out)) == ["junctions.tsv"]
    # --ref_fn, --min_reads, --min_mq and --ctg_name
    LogEngine.log = []
    _run(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--output_fn", out, "--ref_fn", s["fa"], "--min_reads", "2", "--min_mq", "30", "--ctg_name", "chr1,chrNope"])
    got2 = open(out).read().split("\n")[1:-1]
    assert got2 == HJ.predicted_lines(s, "chr1", True, 2, dict(min_mq=30, excl_flags=2316)) and ("set_params", dict(min_mq=30)) in LogEngine.log and LogEngine.log[0] == ("engine", 0)
    assert 0 < len(got2) < len(want1) and all(l.split("\t")[3] != "." for l in got2) and all(int(l.split("\t")[5]) >= 2 for l in got2 if l.split("\t")[7] == ".")
    # without a phased VCF: a plain junction counter, no table is ever set
    LogEngine.log = []
    _run(["--bam_fn", s["bam"], "--output_fn", out, "--ctg_name", "chr1"])
    assert open(out).read().split("\n")[1:-1] == HJ.predicted_lines(s, "chr1", phased=False)
    assert [c[0] for c in LogEngine.log] == ["engine", "set_params", "load_reads", "hap_junction_counts", "close"]


def test_the_tagging_flags_go_through_the_helpers_of_haplotag_bam(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "Engine", LogEngine)
    s = HJ.driver_sample(str(tmp_path), n_reads=30)
    out = str(tmp_path / "j.tsv")
    LogEngine.log = []
    _run(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--output_fn", out, "--haplotag_indels", "--ctg_name", "chr1"])
    assert [c[0] for c in LogEngine.log] == ["engine", "set_params", "set_phase_alleles", "load_reads", "hap_junction_counts", "close"]
    assert open(out).read().split("\n")[1:-1] == HJ.predicted_lines(s, "chr1")
    from clair3_rna_amd import haplotag_bam
    mine = {a.dest: a for a in hap_junctions.build_parser()._actions}
    for a in haplotag_bam.build_parser()._actions:
        if a.dest in ("haplotag_indels", "left_align_indels", "hap_realign", "hap_realign_spliced", "hap_min_bq", "hap_bq_weights", "gpu_id", "threads"):
            assert a.dest in mine and mine[a.dest].default == a.default and mine[a.dest].option_strings == a.option_strings and mine[a.dest].nargs == a.nargs, a.dest
    assert mine["min_mq"].default == 5 and mine["min_reads"].default == 1 and mine["phased_vcf_fn"].default is None and mine["ref_fn"].default is None
    base = ["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--output_fn", str(tmp_path / "refused.tsv")]
    for extra, words in ((["--left_align_indels"], "--haplotag_indels"), (["--hap_realign"], "--ref_fn"), (["--hap_min_bq", "200"], "--hap_min_bq"), (["--min_reads", "0"], "--min_reads"),
                         (["--ref_fn", str(tmp_path / "nope.fa")], "not found")):
        with pytest.raises(SystemExit) as e:
            _run(base + extra)
        assert "[ERROR]" in str(e.value.code) and words in str(e.value.code), e.value.code
    for flag in (["--haplotag_indels"], ["--hap_realign", "4"], ["--hap_min_bq", "7"], ["--hap_bq_weights"]):
        with pytest.raises(SystemExit) as e:
            _run(["--bam_fn", s["bam"], "--output_fn", str(tmp_path / "refused.tsv")] + flag)
        assert "needs --phased_vcf_fn" in str(e.value.code), e.value.code
    for missing in ("--bam_fn", "--phased_vcf_fn"):
        argv = list(base)
        argv[argv.index(missing) + 1] = str(tmp_path / "nope")
        with pytest.raises(SystemExit) as e:
            _run(argv)
        assert "not found" in str(e.value.code)
    assert not os.path.exists(str(tmp_path / "refused.tsv")) and not os.path.exists(str(tmp_path / "refused.tsv.tmp"))


def test_a_failed_contig_leaves_no_file(tmp_path, monkeypatch):
    class Failing(LogEngine):
        def hap_junction_counts(self, slots_hint=0):
            raise capi.C3RError(-6, "the tables still had no place")

    monkeypatch.setattr(capi, "Engine", Failing)
    s = HJ.driver_sample(str(tmp_path), n_reads=20)
    out = str(tmp_path / "o" / "j.tsv")
    LogEngine.log = []
    with pytest.raises(capi.C3RError, match="no place"):
        _run(["--bam_fn", s["bam"], "--output_fn", out])
    assert os.listdir(os.path.dirname(out)) == [] and LogEngine.log[-1] == ("close",)


def test_the_help_states_the_limits():
    text = " ".join(hap_junctions.build_parser().format_help().split())
    for words in ("no minimum intron length", "anchor length", "no annotation", "no statistics", "has not been measured"):
        assert words in text, words


# ---- call_sample
def test_call_sample_refuses_the_flag_where_it_cannot_work_and_hands_the_step_its_argv(tmp_path, monkeypatch):
    from clair3_rna_amd import call_sample
    bed = str(tmp_path / "exons.bed")
    open(bed, "w").write("chr1\t1\t2\n")
    phased = str(tmp_path / "p.vcf")
    open(phased, "w").close()
    out = str(tmp_path / "out")
    fa = str(tmp_path / "x.fa")
    base = ["--bam_fn", str(tmp_path / "x.bam"), "--ref_fn", fa, "--output_dir", out, "--pileup_model_path", "w18", "--phased_pileup_model_path", "w30"]

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:
            call_sample.Run(call_sample.build_parser().parse_args(base + extra))
        assert str(e.value.code).startswith("[ERROR] --hap_junctions") and all(w in str(e.value.code) for w in words), e.value.code

    flag = ["--hap_junctions"]
    refused(flag, "--enable_phasing_model")
    refused(flag + ["--phasing", "builtin"], "--enable_phasing_model")
    refused(flag + ["--enable_phasing_model"], "--phased_vcf_fn", "--phasing builtin")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(flag + ["--enable_phasing_model", "--phased_vcf_fn", phased], "WORLD_SIZE", "python -m clair3_rna_amd.hap_junctions")
    refused(flag + ["--enable_phasing_model", "--phasing", "builtin"], "WORLD_SIZE", "python -m clair3_rna_amd.hap_junctions")
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert not os.path.exists(out)
    # the plan: one more step behind all the others, with the tagging flags hap_expr gets and --ref_fn
    stem = os.path.join(out, "output_enable_phasing")
    plan = call_sample._plan(call_sample.build_parser().parse_args(base + flag + ["--enable_phasing_model", "--phased_vcf_fn", phased, "--haplotagged_bam", "--phase_output",
                                                                                   "--hap_expression_bed", bed, "--haplotag_indels", "--hap_min_bq", "7", "--gpu_id", "2"]))
    assert [st.name for st in plan] == ["pass", "hap_vcf", "clear", "haplotag_bam", "hap_expr", "hap_junctions"]
    step, expr = plan[-1], plan[-2]
    assert step.needs == stem + ".vcf.gz" == expr.needs
    assert step.handed == ["--phased_vcf_fn", phased, "--output_fn", stem + "_hap_junctions.tsv", "--min_mq", "5", "--ref_fn", fa, "--haplotag_indels", "--hap_min_bq", "7", "--gpu_id", "2"]
    assert step.handed[8:] == expr.handed[10:]                  # what follows hap_expr's own flags
    hap_junctions.build_parser().parse_args(["--bam_fn", "x"] + step.handed)
    open(fa, "w").close()                                       # (--hap_realign looks for its reference)
    builtin = call_sample._plan(call_sample.build_parser().parse_args(base + flag + ["--enable_phasing_model", "--phasing", "builtin", "--phasing_indels", "--hap_realign", "5"]))
    assert [st.name for st in builtin] == ["pass", "clear", "phase_vcf", "pass", "hap_junctions"]
    handed = builtin[-1].handed
    assert handed[:2] == ["--phased_vcf_fn", os.path.join(out, "tmp", "phased_output", "phased_vcf")] and "--haplotag_indels" in handed and "--hap_realign" in handed
    assert hap_junctions.build_parser().parse_args(["--bam_fn", "x"] + handed).ref_fn == fa      # (named twice: once for MOTIF, once by --hap_realign)
    # without the flag: the plan of the parent
    plain = call_sample._plan(call_sample.build_parser().parse_args(base + ["--enable_phasing_model", "--phased_vcf_fn", phased, "--haplotagged_bam"]))
    assert [st.name for st in plain] == ["pass", "clear", "haplotag_bam"]
    assert not os.path.exists(out)
