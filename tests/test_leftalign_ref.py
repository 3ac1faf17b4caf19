"""Left-alignment of indels (include/c3r.h: c3r_set_hap_left_align, c3r_hap_left_align_sites) without a GPU: the rule by hand on the
restatement (tests/leftalignref.py) and on the library's host function, the two against each other on random repeat cases, and the
invariance the feature stands for — reads and rows that place their indels anywhere in a repeat, seen with the switch on, give the tables
that left-most reads and rows give with the switch off."""
import gzip
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from clair3_rna_amd import call_sample, call_var_bam, capi, hap_vcf, haplotag_bam, io, phase_vcf, phasedvcf, phasing
from tests import hapalleleref as HA
from tests import leftalignref as LA

SEEDS = list(range(8))


# ---- the table, by hand.  Positions in the comments are 0-based; rows are 1-based.
#        01234567
HOMO = "GCAAAATC"             # AAAA on 2 .. 5 behind a C
#         0123456789
DINUC = "TGACACACGT"          # (AC)3 on 2 .. 7 behind a G
WITH_N = "GCAANAATC"          # the tract is cut by an N on 4
# (name, (slice, its first 0-based position), rows (pos, REF, ALT, GT), [(pos, A, B) of the sites that stay], their input index, moved, skipped)
TABLE_CASES = [
    # AA > A on 5: anchor 4.  A=A on 4|5, 3|4, 2|3, then C on 1: three shifts, the anchor is the C on 1
    ("homopolymer_del", (HOMO, 0), [(5, "AA", "A", "0/1")], [(2, ("C", HA.NONE), ("C", ("del", 1)))], [0], 1, (0, 0)),
    # A > ACA on 5 (anchor 4, INS CA): A = last(CA) -> AC; C = C -> CA; A = A -> AC; then G on 1: three shifts, INS AC behind the G
    ("dinucleotide_ins_rotated", (DINUC, 0), [(5, "A", "ACA", "0/1")], [(2, ("G", HA.NONE), ("G", ("ins", "AC")))], [0], 1, (0, 0)),
    # AAA > AA,A on 4 (anchor 3): DEL 1 and DEL 2 both shift twice (3|4 and 3|5, 2|3 and 2|4, then the C)
    ("two_deletions_1/2", (HOMO, 0), [(4, "AAA", "AA,A", "1/2")], [(2, ("C", ("del", 1)), ("C", ("del", 2)))], [0], 1, (0, 0)),
    # AA > TA,A on 4: an SNV and a deletion that would shift twice: the SNV pins the anchor
    ("snv_and_indel_in_a_tract", (HOMO, 0), [(4, "AA", "TA,A", "1/2")], [], [], 0, (1, 0)),
    # the same deleted A written on 4 and on 5: both land on 2, the first row stays
    ("collision", (HOMO, 0), [(4, "AA", "A", "0/1"), (5, "AA", "A", "0/1")], [(2, ("C", HA.NONE), ("C", ("del", 1)))], [0], 2, (0, 1)),
    # the slice starts on 2: 4|5 and 3|4 shift, 2|3 would move the anchor to 1, outside: two shifts, the anchor is the A on 2
    ("tract_at_slice_edge", (HOMO[2:], 2), [(5, "AA", "A", "0/1")], [(3, ("A", HA.NONE), ("A", ("del", 1)))], [0], 1, (0, 0)),
    # A > AA on 7 (anchor 6): A = A with an A on 5: one shift; then the anchor would move onto the N: the A on 5 it is
    ("n_inside_a_tract", (WITH_N, 0), [(7, "A", "AA", "0/1")], [(6, ("A", HA.NONE), ("A", ("ins", "A")))], [0], 1, (0, 0)),
    # nothing to do: an SNV, and a deletion behind a base that differs from the deleted one
    ("already_left_most", (HOMO, 0), [(2, "CA", "C", "0/1"), (7, "T", "G", "0/1")],
     [(2, ("C", HA.NONE), ("C", ("del", 1))), (7, ("T", HA.NONE), ("G", HA.NONE))], [0, 1], 0, (0, 0)),
]


def rows_to_sites(rows):
    out = []
    for row in rows:
        s = HA.site_of_row(*row)
        assert not isinstance(s, str), (row, s)
        out.append(s)
    return out


def library_table(sites, ref):
    """c3r_hap_left_align_sites on a list of sites: (HAP_SITE_DTYPE array, pool, bases, src, stats)."""
    q, pool = HA.to_query(sites)
    return capi.hap_left_align_sites(q, pool, ref[1] + 1, ref[0])


def assert_same_table(sites, ref):
    """The library's table equals the restatement's, element for element."""
    exp, src, skipped, moved = LA.align_sites(sites, ref)
    eq, epool = HA.to_query(exp)
    q, pool, nb, gsrc, st = library_table(sites, ref)
    assert q.tobytes() == eq.tobytes()
    assert nb == sum(len(ev[1]) for s in exp for _, ev in (s["A"], s["B"]) if ev[0] == "ins")
    assert pool.tobytes() == epool[:(nb + 1) // 2].tobytes()
    assert list(gsrc) == src
    assert st == dict(n_in=len(sites), n_out=len(exp), n_moved=moved, n_not_left_alignable=skipped["not_left_alignable"],
                      n_same_pos_after_left_align=skipped["same_pos_after_left_align"])
    return exp, st


@pytest.mark.parametrize("case", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_table_by_hand(case):
    _, ref, rows, want, want_src, want_moved, (n_not, n_same) = case
    sites = rows_to_sites(rows)
    got, src, skipped, moved = LA.align_sites(sites, ref)
    assert [(s["pos"], s["A"], s["B"]) for s in got] == want
    assert src == want_src and moved == want_moved
    assert (skipped["not_left_alignable"], skipped["same_pos_after_left_align"]) == (n_not, n_same)
    assert_same_table(sites, ref)


def test_left_align_counts_by_hand():
    assert LA.left_align((HOMO, 0), 4, "del", 1) == (3, "")
    assert LA.left_align((HOMO, 0), 1, "del", 1) == (0, "")
    assert LA.left_align((DINUC, 0), 5, "ins", 2, "AC") == (4, "AC")
    assert LA.left_align((DINUC, 0), 4, "ins", 2, "CA") == (3, "AC")
    assert LA.left_align((DINUC.lower(), 0), 4, "ins", 2, "ca") == (3, "AC")
    assert LA.left_align((HOMO, 0), 40, "del", 1) == (0, "")                       # an anchor outside the slice


def test_library_refuses_bad_tables():
    q, pool = HA.to_query(rows_to_sites([(5, "A", "ACA", "0/1")]))
    for field, value in (("pos", 0), ("b_kind", 3), ("b_len", 0), ("b_ins_off", 1), ("base_matters", 2)):
        bad = q.copy()
        bad[0][field] = value
        with pytest.raises(capi.C3RError):
            capi.hap_left_align_sites(bad, pool, 1, DINUC, pool_bases=2)
    out, _, nb, src, st = capi.hap_left_align_sites(q[:0], None, 1, DINUC)
    assert len(out) == 0 and nb == 0 and len(src) == 0 and st["n_in"] == 0


# ---- the reads, by hand
@pytest.mark.parametrize("case", LA.HAND_READS, ids=[c[0] for c in LA.HAND_READS])
def test_reads_by_hand(case):
    _, ref, read, want = case
    table = LA.hand_table()
    assert LA.observe(LA.hand_readset(read), 0, {s["pos"]: (j, s) for j, s in enumerate(table)}, ref) == want


# ---- random repeat cases
@pytest.fixture(scope="module", params=SEEDS)
def pair(request):
    """(seed, gen_repeats(seed, False), gen_repeats(seed, True))"""
    return request.param, LA.gen_repeats(request.param, False), LA.gen_repeats(request.param, True)


def test_generator_keeps_its_promises(pair):
    _, plain, jit = pair
    assert plain[0] == jit[0] and np.array_equal(plain[1].seq, jit[1].seq) and np.array_equal(plain[1].reads["pos"], jit[1].reads["pos"])
    assert len(plain[1]) <= 403 and len(plain[0]) == 6000
    ref = (plain[0], 0)
    for p, j in zip(plain[4], jit[4]):
        assert p["pos"] == p["left"] == j["left"] and j["pos"] >= j["left"]
    table, _ = LA.table_of_case(plain[2], plain[3], plain[4])
    _, _, skipped, moved = LA.align_sites(table, ref)
    assert moved == 0 and not any(skipped.values())
    table, _ = LA.table_of_case(jit[2], jit[3], jit[4])
    _, _, skipped, moved = LA.align_sites(table, ref)
    assert moved > 0 and not any(skipped.values())
    assert sum(1 for i in range(len(jit[1])) if HA.read_ops(jit[1], i) != HA.read_ops(plain[1], i)) > 20


def test_library_table_equals_restatement(pair):
    _, plain, jit = pair
    for case in (plain, jit):
        table, _ = LA.table_of_case(case[2], case[3], case[4])
        assert_same_table(table, (case[0], 0))
        # and on a slice that cuts the contig: tracts at its edges
        assert_same_table(table, (case[0][1500:4200], 1500))


def test_invariance(pair):
    """(jitter, switch on) == (no jitter, switch off): tags and phase sets, count tables, link words, unit link words."""
    _, plain, jit = pair
    ref = (plain[0], 0)
    t_off, _ = LA.table_of_case(plain[2], plain[3], plain[4])
    t_jit, _ = LA.table_of_case(jit[2], jit[3], jit[4])
    t_on, src, _, _ = LA.align_sites(t_jit, ref)
    assert [s["pos"] for s in t_on] == [s["pos"] for s in t_off] and src == list(range(len(t_jit)))
    on = LA.observer(ref)
    hp0, st0, ps0 = LA.haplotag(plain[1], t_off)
    hp1, st1, ps1 = LA.haplotag(jit[1], t_on, on)
    assert np.array_equal(hp0, hp1) and np.array_equal(ps0, ps1) and st0 == st1
    assert np.array_equal(LA.allele_counts(plain[1], hp0, ps0, t_off), LA.allele_counts(jit[1], hp1, ps1, t_on, on))
    lk0, lk1 = LA.links(plain[1], t_off), LA.links(jit[1], t_on, on)
    assert np.array_equal(lk0, lk1)
    # units of six table sites (every eleventh site in none), oriented by the truth: the chain itself leaves one block here
    ps, h1 = [-1 if j % 11 == 5 else 1 + j // 6 for j in range(len(t_off))], [s["h1"] for s in t_off]
    ul0, ul1 = LA.unit_links(plain[1], t_off, ps, h1), LA.unit_links(jit[1], t_on, ps, h1, on)
    assert len(ul0) > 1 and np.array_equal(ul0, ul1)
    # and the switch is what does it: without it the jittered reads give other tables
    assert not np.array_equal(lk0, LA.links(jit[1], t_jit))


# ---- the drivers without a GPU: refusals, what call_sample hands down, the readers' tables and the [INFO] counts


def _exit_text(fn, *a, **k):
    with pytest.raises(SystemExit) as e:
        fn(*a, **k)
    return str(e.value.code)


@pytest.fixture()
def files(tmp_path):
    """A contig with the tracts of the hand cases, its FASTA, and an unphased and a phased VCF with rows on right-hand placements."""
    ref = "G" + HOMO + "TTGCA" + DINUC + "ACGGT"              # HOMO on 1 .. 8, DINUC on 14 .. 23 (0-based)
    fa = str(tmp_path / "ref.fa")
    io.write_fasta(fa, [("ctg", ref)])
    rows = [(3, "C", "T", "0/1", "0|1"),                     # an SNV
            (6, "AA", "A", "0/1", "1|0"),                    # AAAA on 3 .. 6: moves to 3 (the C on 0-based 2)
            (7, "A", "G", "0/1", "0|1"),                     # an SNV inside the tract: it stays
            (19, "A", "ACA", "0/1", "0|1"),                  # (AC)3 on 16 .. 21, anchor 18: moves to 16 (the G on 0-based 15), INS AC
            (5, "AA", "TA,A", "1/2", "1|2"),                 # an SNV and a deletion in the tract: not_left_alignable
            (5, "AA", "A", "0/1", "0|1")]                    # dropped before left-alignment: duplicate_pos
    rows.sort(key=lambda r: r[0])
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
    plain, phased = str(tmp_path / "calls.vcf"), str(tmp_path / "phased.vcf")
    with open(plain, "w") as f:
        f.write(head + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT\t%s\n" % r[:4] for r in rows))
    with open(phased, "w") as f:
        f.write(head + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT:PS\t%s:3\n" % (r[0], r[1], r[2], r[4]) for r in rows))
    bam = str(tmp_path / "in.bam")
    open(bam, "w").close()
    return types.SimpleNamespace(ref=ref, fa=fa, vcf=plain, phased=phased, bam=bam, out=str(tmp_path / "out"))


def test_candidates_are_left_aligned_in_one_place(files):
    ref_of = io.contig_reference(files.fa)
    assert ref_of("ctg") == (1, files.ref.encode())
    off = phasing.allele_candidates_from_vcf(files.vcf, "ctg")
    assert list(off[0]["pos"]) == [3, 5, 6, 7, 19] and off[3]["duplicate_pos"] == 1 and not isinstance(off[3], phasing.LeftAligned)
    assert all(len(s) == 2 for s in off[2])
    sites, pool, strings, skipped = phasing.allele_candidates_from_vcf(files.vcf, "ctg", ref_of)
    # 6 -> 3 collides with the SNV on 3, which comes first in the table: dropped; 19 -> 16; the 1/2 row cannot move
    assert list(sites["pos"]) == [3, 7, 16] and strings == [("C", "T", 3), ("A", "G", 7), ("A", "ACA", 19)]
    assert skipped["not_left_alignable"] == 1 and skipped["same_pos_after_left_align"] == 1 and skipped["duplicate_pos"] == 1 and skipped.moved == 2
    assert phasing.left_align_note(skipped) == ", 2 left-aligned" and phasing.left_align_note(off[3]) == ""
    assert (int(sites[2]["b_kind"]), int(sites[2]["b_len"]), int(sites[2]["a_base"]), int(sites[2]["b_base"])) == (1, 2, 4, 4)
    assert [int(pool[0]) >> 4, int(pool[0]) & 15] == [1, 2]                      # AC, rotated from CA
    both = phasing.allele_candidates_from_vcf(files.vcf, None, ref_of)
    assert both["ctg"][0].tobytes() == sites.tobytes() and both["ctg"][2] == strings
    # the rows that are rewritten are the rows the sites came from
    out = os.path.join(os.path.dirname(files.vcf), "w.vcf.gz")
    n = phasing.write_allele_phased_vcf(files.vcf, "ctg", sites, strings, [3, -1, 3], [0, 0, 1], out)
    body = [l.split("\t") for l in gzip.open(out, "rt") if not l.startswith("#")]
    assert n == 2 and [(r[1], r[3], r[4], r[9].strip()) for r in body if "|" in r[9]] == [("3", "C", "T", "0|1:3"), ("19", "A", "ACA", "1|0:3")]


def test_phase_source_left_aligns_its_allele_table(files):
    ref_of = io.contig_reference(files.fa)
    off = phasedvcf.PhaseSource(files.phased, True).table("ctg")
    assert list(off.pos) == [3, 5, 6, 7, 19] and off.skipped.moved is None
    assert "left-aligned" not in phasedvcf.PhaseSource(files.phased, True).indel_note(off, "x: ")
    for only in (None, "ctg"):
        src = phasedvcf.PhaseSource(files.phased, True, only, ref_of)
        t = src.table("ctg")
        assert list(t.pos) == [3, 7, 16] and list(t._rest[0]) == [0, 0, 0] and t._rest[2] == 2 and list(t.ps) == [3, 3, 3]
        assert t.kept == dict(indel=1, two_alt=0) and t.skipped.moved == 2
        assert src.indel_note(t, "x: ") == ("x: 1 with an insertion or deletion, 0 with two ALTs, --left_align_indels: 2 left-aligned, "
                                            "1 not_left_alignable, 1 same_pos_after_left_align")
    calls = []
    eng = types.SimpleNamespace(set_hap_left_align=lambda on: calls.append(("switch", on)), set_phase_alleles=lambda s, *r: calls.append(("table", len(s))))
    src.apply(eng, t)
    assert calls == [("switch", True), ("table", 3)]
    calls.clear()
    phasedvcf.PhaseSource(files.phased, True).apply(eng, off)                    # without the flag the switch is never touched
    assert calls == [("table", 5)]
    assert _exit_text(phasedvcf.PhaseSource, files.phased, False, None, ref_of) == "[ERROR] --left_align_indels needs --haplotag_indels"


def test_refusals(files):
    base = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--output_dir", files.out]
    run = lambda mod, argv: _exit_text(mod.Run, mod.build_parser().parse_args(argv))
    assert run(phase_vcf, base + ["--left_align_indels"]) == "[ERROR] --left_align_indels needs --indels"
    assert run(phase_vcf, base + ["--left_align_indels", "--indels"]) == "[ERROR] --left_align_indels needs --ref_fn"
    assert run(phase_vcf, base + ["--left_align_indels", "--indels", "--ref_fn", files.fa + ".no"]) == "[ERROR] file %s.no not found" % files.fa
    hv = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--phased_vcf_fn", files.phased, "--output_fn", files.out + ".vcf"]
    assert run(hap_vcf, hv + ["--left_align_indels"]) == "[ERROR] --left_align_indels needs --indels"
    assert run(hap_vcf, hv + ["--left_align_indels", "--indels"]) == "[ERROR] --left_align_indels needs --ref_fn"
    hb = ["--bam_fn", files.bam, "--phased_vcf_fn", files.phased, "--output_dir", files.out]
    assert run(haplotag_bam, hb + ["--left_align_indels", "--ref_fn", files.fa]) == "[ERROR] --left_align_indels needs --haplotag_indels"
    assert run(haplotag_bam, hb + ["--left_align_indels", "--haplotag_indels"]) == "[ERROR] --left_align_indels needs --ref_fn"
    cv = ["--chkpnt_fn", "w", "--bam_fn", files.bam, "--ref_fn", files.fa, "--call_fn", files.out + ".vcf", "--ctgName", "ctg", "--pileup",
          "--enable_phasing_model", "True", "--phased_vcf_fn", files.phased]
    assert _exit_text(call_var_bam.Run, call_var_bam.build_parser().parse_args(cv + ["--left_align_indels"])) == (
        "[ERROR] --left_align_indels needs --haplotag_indels (it left-aligns the indels the reads are haplotagged from)")
    assert not os.path.exists(files.out)


def _plan(files, extra):
    argv = ["--bam_fn", files.bam, "--ref_fn", files.fa, "--output_dir", files.out, "--pileup_model_path", "m", "--enable_phasing_model",
            "--phased_pileup_model_path", "m30"] + extra
    return call_sample._plan(call_sample.build_parser().parse_args(argv))


def test_call_sample_hands_the_flag_down(files, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "1")
    want = "[ERROR] --left_align_indels needs one of --phase_indels, --haplotag_indels, --phasing_indels (it left-aligns the indels those steps read)"
    assert _exit_text(_plan, files, ["--left_align_indels"]) == want
    assert _exit_text(_plan, files, ["--left_align_indels", "--phasing", "builtin", "--phase_output", "--haplotagged_bam"]) == want
    # an older rule that is broken as well still speaks first
    assert _exit_text(_plan, files, ["--left_align_indels", "--phase_indels"]).startswith("[ERROR] --phase_indels belongs to --phase_output")
    la = ["--left_align_indels", "--ref_fn", files.fa]
    has = lambda handed: [handed[k:k + 3] for k in range(len(handed)) if handed[k] == "--left_align_indels"]
    steps = _plan(files, ["--left_align_indels", "--phasing", "builtin", "--phasing_indels", "--phase_output", "--phase_indels", "--haplotagged_bam"])
    assert [s.name for s in steps] == ["pass", "clear", "phase_vcf", "pass", "hap_vcf", "clear", "haplotag_bam"]
    for s in steps:
        if s.name in ("phase_vcf", "hap_vcf", "haplotag_bam"):
            assert has(s.handed) == [la], s
    assert steps[3].handed.left_align_indels and steps[3].handed.haplotag_indels
    # only the steps that read indels get it
    steps = _plan(files, ["--left_align_indels", "--phasing", "builtin", "--phase_output", "--phase_indels", "--haplotagged_bam"])
    assert [bool(has(s.handed)) for s in steps if s.name in ("phase_vcf", "hap_vcf", "haplotag_bam")] == [False, True, False]
    # and without the flag no step's arguments change
    with_flag = _plan(files, ["--left_align_indels", "--phased_vcf_fn", files.phased, "--haplotag_indels", "--phase_output", "--haplotagged_bam"])
    without = _plan(files, ["--phased_vcf_fn", files.phased, "--haplotag_indels", "--phase_output", "--haplotagged_bam"])
    for a, b in zip(with_flag, without):
        if a.name in ("hap_vcf", "haplotag_bam"):
            assert has(a.handed) == [la] and [x for x in a.handed if x not in la] == b.handed


class _Engine(object):
    """What phase_vcf asks of an engine, recorded."""
    log = []

    def __init__(self, device=0): pass
    def close(self): pass
    def set_params(self, **kw): pass
    def set_reference(self, start, seq): _Engine.log.append(("reference", start, len(seq)))
    def set_hap_left_align(self, on): _Engine.log.append(("switch", on))
    def load_reads(self, rs): _Engine.log.append(("reads", len(rs)))

    def phase_allele_sites(self, sites, pool, min_reads, min_agree_pct, merge_levels):
        _Engine.log.append(("phase", [int(p) for p in sites["pos"]]))
        n = len(sites)
        return np.full(n, 3, np.int32), np.zeros(n, np.uint8), dict(n_sites=n, n_phased=n, n_blocks=1, max_block=n)


def test_phase_vcf_info_line_counts(files, monkeypatch):
    from clair3_rna_amd.reads import ReadSet
    monkeypatch.setattr(capi, "Engine", _Engine)
    monkeypatch.setattr(io, "load_reads", lambda bam, ctg: ReadSet.from_records([dict(pos=0, cigar="9M", seq="GGCAAAATC", flag=0, mapq=60, hp=0)]))
    for la in (True, False):
        _Engine.log, lines = [], []
        argv = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--output_dir", files.out, "--indels"] + (["--left_align_indels", "--ref_fn", files.fa] if la else [])
        phase_vcf.Run(phase_vcf.build_parser().parse_args(argv), log=lines.append)
        assert len(lines) == 1
        if la:
            # the reference and the switch come before the reads
            assert _Engine.log == [("reference", 1, len(files.ref)), ("switch", True), ("reads", 1), ("phase", [3, 7, 16])]
            assert "3 candidate sites with indels and two-ALT rows, 2 left-aligned (duplicate_pos 1, not_left_alignable 1, same_pos_after_left_align 1)" in lines[0]
        else:
            assert _Engine.log == [("reads", 1), ("phase", [3, 5, 6, 7, 19])]
            assert "5 candidate sites with indels and two-ALT rows (duplicate_pos 1)" in lines[0]


# ---- the C ABI alone (host code: the program needs no device)
def test_the_stand_alone_check_program(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to build tests/c/left_align_check.c"
    lib = os.path.join(root, "clair3_rna_amd")
    exe = str(tmp_path / "left_align_check")
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "left_align_check.c"),
                           "-L", lib, "-lc3r", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "left_align_check: ok" in out.stdout, out.stdout + out.stderr
