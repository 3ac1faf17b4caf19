"""Allele realignment across splice junctions (include/c3r.h: c3r_set_hap_realign_spliced, c3r_hap_realign_column_spliced) without a GPU:
the rule by hand on the restatement (tests/realignspliceref.py) and on the library's host entry — which is compiled from the header the
kernels use —, the two against each other on the hand cases and on four seeded fuzzes with planted introns, the three properties the rule
stands for, the C ABI alone, and the drivers' refusals and plumbing."""
import gzip
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from clair3_rna_amd import capi, haplotag_bam, io, phase_vcf, phasing
from tests import hapalleleref as HA
from tests import realignref as RR
from tests import realignspliceref as RS
from tests.support import fake_engine_realign as FE

REF, SNV, DEL, NO, HAND, LONG = RS.REF, RS.SNV, RS.DEL, RS.NO, RS.HAND, RR.LONG
one_read, site_of = RR.one_read, RR.site_of
W_FUZZ = 10
SEEDS = (0, 1, 2, 3)


def library_column(rs, i, site, ref, W, spliced=True):
    q, pool = HA.to_query([site])
    return capi.hap_realign_column(q[0], pool, ref[0] + 1, ref[1], rs.reads[i], rs.cigar, rs.seq, W, spliced=spliced)


# ---- the hand cases
def test_strings_on_paper():
    """Pins the RESTATEMENT's map to paper: the spliced positions, the window's indices and offsets of the two cases the rule was written for."""
    rs, site = one_read((5, "12M5N3M", REF[5:17] + REF[22:25])), site_of(SNV)
    xs, cov = RS.spliced(rs, 0)
    assert xs == list(range(5, 17)) + [22, 23, 24] and cov[17] == ("N", 12) and cov[22] == ("M", 12)
    qs, qt, _, k0 = RS.spliced_window(rs, 0, (0, REF), site, 3)
    assert (qs, qt, k0, xs[k0 - 3], xs[k0 + 4]) == (5, 12, 8, 10, 22)
    rs = one_read((5, "7M1D1M1I1M5N5M", REF[5:13] + "C" + REF[14] + REF[20:25]))
    xs, _ = RS.spliced(rs, 0)
    assert xs == list(range(5, 15)) + list(range(20, 25))
    qs, qt, _, k0 = RS.spliced_window(rs, 0, (0, REF), site, 3)
    assert (qs, qt, k0, [xs[k] for k in range(k0 + 1, k0 + 4)]) == (5, 12, 8, [14, 20, 21])
    d = RR.levenshtein
    assert (d("CGACCCT", "CGATCCT"), d("CGACCCT", "CGACCCT")) == (1, 0)
    assert (d("CGATCGGTT", "CGATCGG"), d("CGATCGGTT", "CGACCGG")) == (2, 3)
    assert (d("CGATCG", "CGATCGG"), d("CGATCG", "CGACCGG")) == (1, 2)


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_rule_by_hand(case):
    _, ref, row, W, read, want, want_plain, want_off, strings = case
    rs, site = one_read(read), site_of(row)
    assert RS.column_of(rs, 0, site, ref, W) == want
    if want[1]:
        assert RS.strings_of(rs, 0, site, ref, W) == strings
    else:
        assert strings is None and RS.spliced_window(rs, 0, ref, site, W) is None and want[0] == want_off
    # plain `realign` and both switches off, on the restatements
    assert RR.column_of(rs, 0, site, ref, W) == want_plain
    assert RS.column_of(rs, 0, site, ref, 0) == (want_off, False) == (HA.observe(rs, 0, {site["pos"]: (0, site)}).get(0, NO), False)
    # the host entry: the new one under the switch, without it (the old entry's result) and with overhang 0
    assert library_column(rs, 0, site, ref, W) == want
    assert library_column(rs, 0, site, ref, W, spliced=False) == want_plain
    assert library_column(rs, 0, site, ref, 0) == (want_off, False)


def test_the_cases_of_plain_realign_that_hold_an_n():
    """tests/realignref.py's own hand cases under the switch: those with an N op become realigned, every other one keeps its result."""
    changed = {}
    for name, ref, row, W, read, want, _ in RR.HAND:
        rs, site = one_read(read), site_of(row)
        got = RS.column_of(rs, 0, site, ref, W)
        assert library_column(rs, 0, site, ref, W) == got, name
        if got != want:
            changed[name] = got
        else:
            assert "N" not in read[1] or want[1], name
    assert changed == {"N_on_t": (0, True), "N_on_s": (0, True)}


def _planted_long(read, cut, site_row):
    """A read of realignref.long_read with an intron planted before `cut`: (reference, site, ReadSet)."""
    ref, table, rs = RS.plant((0, LONG), [site_of(site_row)], one_read(read), cuts=(cut,), seed=3)
    assert RS.n_ops(rs) == 1 and len(ref[1]) >= len(LONG) + 40
    return ref, table[0], rs


def test_the_two_limits_of_64_across_a_junction():
    p0, W = 60, 16
    ins11, ins12 = "GATTACAGATT", "GATTACAGATTA"
    dele = LONG[p0:p0 + 21]
    fits = (p0 + 1, dele, LONG[p0] + ins11 + dele[1:] + "," + LONG[p0], "1/2")            # INS 11 / DEL 20: 2W + 1 + D + I = 64
    over = (p0 + 1, dele, LONG[p0] + ins12 + dele[1:] + "," + LONG[p0], "1/2")            # INS 12 / DEL 20: 65
    for cut in (50, 90):                                                                    # inside the left flank [44, 60), inside the tail [81, 97)
        # m = 53 + 11 = 64: realigned, the window is haplotype A itself
        ref, site, rs = _planted_long(RR.long_read(p0, ins11), cut, fits)
        qs, qt, _, _ = RS.spliced_window(rs, 0, ref, site, W)
        assert qt - qs == 64 and RR.realigned_window(rs, 0, ref, site, W) is None
        assert RS.column_of(rs, 0, site, ref, W) == (0, True) == library_column(rs, 0, site, ref, W)
        # m = 65: one more inserted base inside the window — the CIGAR's column (the insertion behind the anchor is allele A's)
        ref, site, rs = _planted_long(RR.long_read(p0, ins11, extra_at=70), cut, fits)
        assert RS.spliced_window(rs, 0, ref, site, W) is None
        assert RS.column_of(rs, 0, site, ref, W) == (0, False) == library_column(rs, 0, site, ref, W)
        # 2W + 1 + D + I = 65: never realigned; one less overhang and it is
        ref, site, rs = _planted_long(RR.long_read(p0, ins12), cut, over)
        assert RS.column_of(rs, 0, site, ref, W) == (0, False) == library_column(rs, 0, site, ref, W)
        assert RS.column_of(rs, 0, site, ref, W - 1) == (0, True) == library_column(rs, 0, site, ref, W - 1)


# ---- the fuzz: realignref.gen_fuzz with an intron planted every 60 bases
_memo = {}


def fuzz(seed):
    """(plain fuzz, planted fuzz, {(read, site): column of plain `realign` on the plain fuzz}, {(read, site): (column, realigned) of the rule
    on the planted fuzz}, {(read, site): the same of plain `realign` on the planted fuzz}) — the restatements', computed once."""
    if seed not in _memo:
        plain = RR.gen_fuzz(seed)
        planted = RS.plant(*plain, cuts=RS.CUTS, seed=seed)
        pairs = [(i, j) for i in range(len(plain[2])) for j in range(len(plain[1]))]
        base = {(i, j): RR.column_of(plain[2], i, plain[1][j], plain[0], W_FUZZ) for i, j in pairs}
        on = {(i, j): RS.column_of(planted[2], i, planted[1][j], planted[0], W_FUZZ) for i, j in pairs}
        off = {(i, j): RR.column_of(planted[2], i, planted[1][j], planted[0], W_FUZZ) for i, j in pairs}
        _memo[seed] = (plain, planted, base, on, off)
    return _memo[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_the_planter(seed):
    plain, planted, _, _, _ = fuzz(seed)
    (ref, table, rs), (pref, ptable, prs) = plain, planted
    assert len(ref[1]) == 400 and len(rs) == 200 == len(prs) and len(table) == 24 == len(ptable)
    assert RS.n_ops(rs) == 0 and RS.n_ops(prs) >= 300
    assert 400 + 6 * 40 <= len(pref[1]) <= 400 + 6 * 300
    assert np.array_equal(rs.seq, prs.seq) and np.array_equal(rs.reads["l_seq"], prs.reads["l_seq"]) and (np.diff(prs.reads["pos"].astype(np.int64)) >= 0).all()
    # every site keeps its anchor's letter and its alleles, and cutting the introns out of a read's spliced positions gives the read's old positions
    for s, t in zip(table, ptable):
        assert pref[1][t["pos"] - 1] == ref[1][s["pos"] - 1] and (s["A"], s["B"]) == (t["A"], t["B"])
    for i in range(0, len(rs), 7):
        xs, cov = RS.spliced(rs, i)
        pxs, pcov = RS.spliced(prs, i)
        assert len(xs) == len(pxs) and [ref[1][x] for x in xs] == [pref[1][x] for x in pxs]
        assert [cov[x] for x in xs] == [pcov[x] for x in pxs]
    # both orders of an N and an adjacent I occur, = / X and pad reads got their introns too
    text = ["".join("%d%s" % (n, op) for op, n in HA.read_ops(prs, i)) for i in range(len(prs))]
    import re
    assert any(re.search(r"\dI\d+N", t) for t in text) and any(re.search(r"\dN\d+I", t) for t in text)
    assert sum(1 for t in text if "N" in t and ("=" in t or "X" in t)) >= 20 and sum(1 for t in text if "N" in t and "P" in t) >= 20


@pytest.mark.parametrize("seed", SEEDS)
def test_host_entry_equals_the_restatement_on_the_planted_fuzz(seed):
    _, (pref, ptable, prs), _, on, off = fuzz(seed)
    q, pool = HA.to_query(ptable)
    for (i, j), want in on.items():
        assert capi.hap_realign_column(q[j], pool, 1, pref[1], prs.reads[i], prs.cigar, prs.seq, W_FUZZ, spliced=True) == want, (i, j)
    for (i, j), want in list(off.items())[::5]:                           # (and the old rule through the new entry)
        assert capi.hap_realign_column(q[j], pool, 1, pref[1], prs.reads[i], prs.cigar, prs.seq, W_FUZZ, spliced=False) == want, (i, j)


@pytest.mark.parametrize("seed", SEEDS)
def test_a_without_introns_the_switch_changes_nothing(seed):
    (ref, table, rs), _, base, _, _ = fuzz(seed)
    q, pool = HA.to_query(table)
    for (i, j), want in base.items():
        assert RS.column_of(rs, i, table[j], ref, W_FUZZ) == want, (i, j)
        assert capi.hap_realign_column(q[j], pool, 1, ref[1], rs.reads[i], rs.cigar, rs.seq, W_FUZZ, spliced=True) == want, (i, j)


@pytest.mark.parametrize("seed", SEEDS)
def test_b_splice_invariance(seed):
    """With the switch on, the planted set's columns are plain `realign`'s columns on the set without introns, for every (read, site) pair
    — and so is whether the read was realigned."""
    _, _, base, on, _ = fuzz(seed)
    differing = [k for k in base if base[k] != on[k]]
    assert differing == []


@pytest.mark.parametrize("seed", SEEDS)
def test_c_the_invariance_is_not_empty(seed):
    """On the restatement alone: at least 30 % of the anchored pairs are realigned only under the switch (the first restatement the rule was
    proposed with gave 41 - 42 %), and at least 15 columns differ from plain `realign` on the same planted set (it gave 22 - 36)."""
    _, (pref, ptable, prs), _, _, _ = fuzz(seed)
    n, n_plain, n_spliced, n_diff = RS.profile(pref, ptable, prs, W_FUZZ)
    print("seed %d: %d anchored pairs, %d realigned today, %d under the switch, %d columns differ" % (seed, n, n_plain, n_spliced, n_diff))
    assert n >= 1500 and n_spliced - n_plain >= 0.30 * n and n_diff >= 15


def test_host_entry_refusals():
    rs, site = one_read(HAND[0][4]), site_of(SNV)
    q, pool = HA.to_query([site])
    L = capi.load_library()
    import ctypes as C
    col, ra = C.c_int32(7), C.c_int32(7)
    args = lambda spliced: (q.ctypes.data, None, 1, REF.encode(), len(REF), rs.reads.ctypes.data, rs.cigar.ctypes.data, rs.seq.ctypes.data, 3, spliced, C.byref(col), C.byref(ra))
    assert L.c3r_hap_realign_column_spliced(*args(1)) == 0 and (col.value, ra.value) == (0, 1)
    assert L.c3r_hap_realign_column_spliced(*args(0)) == 0 and (col.value, ra.value) == (0, 0)
    for bad in (2, -1, 256):
        assert L.c3r_hap_realign_column_spliced(*args(bad)) == -1
    for kw in (dict(W=17), dict(W=-1), dict(start=0)):
        with pytest.raises(capi.C3RError):
            capi.hap_realign_column(q[0], pool, kw.get("start", 1), REF, rs.reads[0], rs.cigar, rs.seq, kw.get("W", 3), spliced=True)
    with pytest.raises(capi.C3RError):
        capi.hap_realign_column(q[0], pool, 1, REF, rs.reads[0], rs.cigar | 15, rs.seq, 3, spliced=True)      # an op code that no CIGAR has


# ---- the C ABI alone (host code: the program needs no device)
def test_the_stand_alone_check_program(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/c/realign_spliced_check.cpp"
    lib = os.path.join(root, "clair3_rna_amd")
    exe = str(tmp_path / "realign_spliced_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "realign_spliced_check.cpp"),
                           "-L", lib, "-lc3r", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "realign_spliced_check: ok" in out.stdout, out.stdout + out.stderr


# ---- the drivers: refusals and plumbing, with the logging fake engine
class Engine(FE.Engine):
    def set_hap_realign_spliced(self, on):
        FE.Engine.log.append(("realign_spliced", on))


def _exit_text(fn, *a):
    with pytest.raises(SystemExit) as e:
        fn(*a)
    return str(e.value)


@pytest.fixture()
def files(tmp_path):
    fa = str(tmp_path / "ref.fa")
    io.write_fasta(fa, [("ctg", REF)])
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
    rows = [(8, "G", "A", "0/1", "0|1"), (14, "T", "C", "0/1", "1|0")]
    plain, phased = str(tmp_path / "calls.vcf"), str(tmp_path / "phased.vcf")
    with open(plain, "w") as f:
        f.write(head + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT\t%s\n" % r[:4] for r in rows))
    with open(phased, "w") as f:
        f.write(head + "".join("ctg\t%d\t.\t%s\t%s\t9\tPASS\t.\tGT:PS\t%s:3\n" % (r[0], r[1], r[2], r[4]) for r in rows))
    bam = str(tmp_path / "in.bam")
    open(bam, "w").close()
    return types.SimpleNamespace(ref=REF, fa=fa, vcf=plain, phased=phased, bam=bam, out=str(tmp_path / "out"))


NEEDS = "[ERROR] --hap_realign_spliced needs --hap_realign (it says how the window of --hap_realign is counted)"


def test_driver_refusals(files, monkeypatch):
    from clair3_rna_amd import call_sample, call_var_bam, hap_vcf
    run = lambda mod, argv: _exit_text(mod.Run, mod.build_parser().parse_args(argv))
    pv = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--output_dir", files.out]
    hb = ["--bam_fn", files.bam, "--phased_vcf_fn", files.phased, "--output_dir", files.out]
    hv = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--phased_vcf_fn", files.phased, "--output_fn", files.out + ".vcf"]
    cv = ["--chkpnt_fn", "w", "--bam_fn", files.bam, "--ref_fn", files.fa, "--call_fn", files.out + ".vcf", "--ctgName", "ctg", "--pileup", "--enable_phasing_model", "True",
          "--phased_vcf_fn", files.phased]
    for mod, base in ((phase_vcf, pv), (haplotag_bam, hb), (hap_vcf, hv), (call_var_bam, cv)):
        p = mod.build_parser()
        assert p.parse_args(base).hap_realign_spliced is False and p.parse_args(base + ["--hap_realign_spliced"]).hap_realign_spliced is True
        assert run(mod, base + ["--hap_realign_spliced"]) == NEEDS
        assert run(mod, base + ["--hap_realign_spliced", "--ref_fn", files.fa]) == NEEDS
        # beside --hap_realign the flag changes none of --hap_realign's own refusals
        assert run(mod, base + ["--hap_realign", "17", "--hap_realign_spliced", "--ref_fn", files.fa]).startswith("[ERROR] --hap_realign must lie between 1 and 16")
    assert run(phase_vcf, pv + ["--hap_realign", "--hap_realign_spliced"]) == "[ERROR] --hap_realign needs --ref_fn"
    assert not os.path.exists(files.out) and not os.path.exists(files.out + ".vcf")             # (before any file exists)
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert _exit_text(_plan, files, ["--hap_realign_spliced"]) == NEEDS
    assert _exit_text(_plan, files, ["--hap_realign_spliced", "--phasing", "builtin"]) == NEEDS
    assert _exit_text(_plan, files, ["--hap_realign_spliced", "--phased_vcf_fn", files.phased], False) == NEEDS
    assert phasing.hap_realign_spliced_arg(types.SimpleNamespace()) is False and phasing.hap_realign_arg(types.SimpleNamespace()) == (0, None)
    assert _exit_text(phasing.hap_realign_arg, types.SimpleNamespace(hap_realign_spliced=True)) == NEEDS
    assert not os.path.exists(files.out)


def _plan(files, extra, phasing_model=True):
    from clair3_rna_amd import call_sample
    argv = ["--bam_fn", files.bam, "--ref_fn", files.fa, "--output_dir", files.out, "--pileup_model_path", "m"] + (
        ["--enable_phasing_model", "--phased_pileup_model_path", "m30"] if phasing_model else []) + extra
    return call_sample._plan(call_sample.build_parser().parse_args(argv))


def test_apply_is_the_one_place():
    calls = []
    eng = types.SimpleNamespace(set_reference=lambda s, r, **how: calls.append(("reference", s, how)), set_hap_realign=lambda w: calls.append(("realign", w)),
                                set_hap_realign_spliced=lambda on: calls.append(("realign_spliced", on)))
    phasing.apply_hap_realign(eng, 0, None, True)                                               # (no overhang: nothing is touched)
    phasing.apply_hap_realign(eng, 7, (1, "ACGT"))
    phasing.apply_hap_realign(eng, 7, (1, "ACGT"), False)
    assert calls == [("reference", 1, {}), ("realign", 7)] * 2
    del calls[:]
    phasing.apply_hap_realign(eng, 7, (1, "ACGT"), True, upper_view=True)
    assert calls == [("reference", 1, dict(upper_view=True)), ("realign_spliced", True), ("realign", 7)]
    # the drivers name the engine's switch nowhere else
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("phase_vcf", "hap_vcf", "haplotag_bam", "call_var_bam", "call_sample", "phasedvcf"):
        assert ".set_hap_realign_spliced(" not in open(os.path.join(root, "clair3_rna_amd", name + ".py")).read(), name


def test_phase_vcf_and_haplotag_bam_plumbing(files, monkeypatch):
    monkeypatch.setattr(capi, "Engine", Engine)
    monkeypatch.setattr(io, "load_reads", lambda bam, ctg: one_read(HAND[0][4]))
    base = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--output_dir", files.out]
    out = {}
    for name, extra in (("on", ["--hap_realign", "--ref_fn", files.fa]), ("spliced", ["--hap_realign", "4", "--hap_realign_spliced", "--ref_fn", files.fa])):
        FE.Engine.log = []
        phase_vcf.Run(phase_vcf.build_parser().parse_args(base + extra), log=lambda m: None)
        out[name] = (list(FE.Engine.log), gzip.open(files.out + "/phased_ctg.vcf.gz", "rt").read())
    # without the new flag the engine's second switch is never touched; with it: reference, the switch, the overhang, then the reads
    assert out["on"][0][:3] == [("reference", 1, len(REF)), ("realign", 10), ("reads", 1)] and not [c for c in out["on"][0] if c[0] == "realign_spliced"]
    assert out["spliced"][0][:4] == [("reference", 1, len(REF)), ("realign_spliced", True), ("realign", 4), ("reads", 1)] and out["spliced"][0][4][0] == "phase_alleles"
    assert out["on"][1] == out["spliced"][1]                                                    # (the fake phases alike: the writer is the same)


def test_hap_vcf_plumbing(files, monkeypatch):
    from clair3_rna_amd import hap_vcf

    class Eng(Engine):
        def hap_allele_counts(self, query, pool=None):
            FE.Engine.log.append(("counts_alleles", len(query)))
            return np.zeros((len(query), 3, 3), np.uint32)
    monkeypatch.setattr(capi, "Engine", Eng)
    monkeypatch.setattr(io, "load_reads", lambda bam, ctg: one_read(HAND[0][4]))
    base = ["--bam_fn", files.bam, "--vcf_fn", files.vcf, "--phased_vcf_fn", files.phased, "--output_fn", files.out + ".vcf", "--hap_counts_fn", files.out + ".tsv"]
    FE.Engine.log = []
    hap_vcf.Run(hap_vcf.build_parser().parse_args(base + ["--hap_realign", "--hap_realign_spliced", "--ref_fn", files.fa]), log=lambda m: None)
    assert FE.Engine.log == [("reference", 1, len(REF)), ("realign_spliced", True), ("realign", 10), ("allele_table", 2, [1, 1], [0, 1]), ("reads", 1), ("counts_alleles", 2)]


def test_call_sample_hands_the_flag_to_exactly_the_steps_that_get_hap_realign(files, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "1")
    both = ["--hap_realign", "10", "--ref_fn", files.fa, "--hap_realign_spliced"]
    has = lambda handed: [handed[k:k + 5] for k in range(len(handed)) if handed[k] == "--hap_realign"]
    steps = _plan(files, ["--hap_realign", "--hap_realign_spliced", "--phasing", "builtin", "--phase_output", "--haplotagged_bam"])
    assert [s.name for s in steps] == ["pass", "clear", "phase_vcf", "pass", "hap_vcf", "clear", "haplotag_bam"]
    for s in steps:
        if s.name in ("phase_vcf", "hap_vcf", "haplotag_bam"):
            assert has(s.handed) == [both] and s.handed.count("--hap_realign_spliced") == 1, s
    # the unphased pass gets neither flag; the 30-channel pass gets both
    assert (steps[0].handed.hap_realign, steps[0].handed.hap_realign_spliced) == (0, False)
    assert (steps[3].handed.hap_realign, steps[3].handed.hap_realign_spliced) == (10, True) and steps[3].handed.phased_vcf_fn
    steps = _plan(files, ["--hap_realign", "4", "--hap_realign_spliced", "--phased_vcf_fn", files.phased, "--phase_output", "--haplotagged_bam"])
    assert [s.name for s in steps] == ["pass", "hap_vcf", "clear", "haplotag_bam"] and steps[0].handed.hap_realign_spliced is True
    # and without the new flag no step's arguments change
    for s in _plan(files, ["--hap_realign", "--phased_vcf_fn", files.phased, "--phase_output", "--haplotagged_bam"]):
        if s.name in ("hap_vcf", "haplotag_bam"):
            assert "--hap_realign_spliced" not in s.handed and "--hap_realign" in s.handed
        elif s.name == "pass":
            assert s.handed.hap_realign_spliced is False
