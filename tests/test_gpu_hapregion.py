"""Haplotype-resolved read counts per interval on the device (c3r_hap_region_counts / k_hap_region_counts) against tests/hapregionref.py, the
plain-Python restatement of the rule `hap_regions`: element for element, no tolerance; both CIGAR walks; that the call leaves tags, sets,
count tables and scans alone; the validation paths through the C ABI; and the drivers (hap_expr, call_sample --hap_expression_bed)."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from clair3_rna_amd import hap_expr
from tests import hapref
from tests import hapregionref as HR
from tests import phaseref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=r[4] if len(r) > 4 else 60, hp=0) for r in recs])


def _check(eng, rs, table, tab, row_ps, stranded=0, params=HR.DEFAULT_PARAMS, load=True, detail=None):
    """The engine's two tables for (rs, table, regions) under its current filters equal the restatement's under `params`; returns them."""
    exp_rc, exp_wc = HR.counts(rs, table, tab, row_ps, stranded, params, detail)
    if load:
        eng.set_phase_sites(table)
        eng.load_reads(rs)
    rc, wc = eng.hap_region_counts(tab, row_ps, stranded)
    assert rc.dtype == np.uint32 and wc.dtype == np.uint32 and rc.shape == (len(tab), 2) and wc.shape == (len(row_ps), 2)
    assert np.array_equal(rc, exp_rc), (np.argwhere(rc != exp_rc)[:10], rc[rc != exp_rc][:10], exp_rc[rc != exp_rc][:10])
    assert np.array_equal(wc, exp_wc), (np.argwhere(wc != exp_wc)[:10], wc[wc != exp_wc][:10], exp_wc[wc != exp_wc][:10])
    return exp_rc, exp_wc


def _forced_serial(rs, every=1):
    """The same reads with an empty op (`0D`) behind the first op of every `every`-th read: an op the plain walk does not take, so those
    reads go through the serial walk, and one the rule does not see."""
    from clair3_rna_amd.reads import ReadSet
    cig, reads, off = [], rs.reads.copy(), 0
    for i, r in enumerate(rs.reads):
        c = rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])].tolist()
        if i % every == 0:
            c = c[:1] + [2] + c[1:]                              # (length 0 << 4 | D)
        reads[i]["cigar_off"], reads[i]["n_cigar"] = off, len(c)
        cig += c
        off += len(c)
    return ReadSet(reads, np.array(cig, dtype=np.uint32), rs.seq.copy())


# ---- 1. against the restatement
@pytest.mark.parametrize("case", HR.HAND, ids=[c[0] for c in HR.HAND])
def test_the_hand_cases(eng, case):
    rs, table, tab, row_ps, stranded, want_rc, want_wc = HR.hand_inputs(case)
    rc, wc = _check(eng, rs, table, tab, row_ps, stranded)
    assert rc.tolist() == want_rc.tolist() and wc.tolist() == want_wc.tolist()
    rc, wc = _check(eng, _forced_serial(rs), table, tab, row_ps, stranded)      # the same through the serial walk
    assert rc.tolist() == want_rc.tolist() and wc.tolist() == want_wc.tolist()


_fuzz = {}


def _fuzz_case(seed):
    if seed not in _fuzz:
        _, rs, table, _ = hapref.gen_case(seed)
        _fuzz[seed] = (rs, table) + HR.gen_regions(seed, table)
    return _fuzz[seed]


@pytest.mark.parametrize("stranded", [0, 1, 2])
@pytest.mark.parametrize("seed", range(4))
def test_generated_reads_and_regions(eng, seed, stranded):
    rs, table, tab, row_ps = _fuzz_case(seed)
    assert 350 <= len(rs) <= 400 and len(tab) == 50 and HR.max_back(tab) >= 10
    detail = {}
    rc, wc = _check(eng, rs, table, tab, row_ps, stranded, detail=detail)
    offs = tab["row_off"].tolist() + [len(row_ps)]
    no_row = sum(offs[j + 1] == offs[j] for j in range(len(tab)))
    empty = sum(int(rc[j].sum()) + int(wc[offs[j]:offs[j + 1]].sum()) == 0 for j in range(len(tab)))
    print("seed %d stranded %d: UNTAGGED %d OTHER_SET %d HP1 %d HP2 %d multi-op pairs %d regions without a row %d empty regions %d"
          % (seed, stranded, rc[:, 0].sum(), rc[:, 1].sum(), wc[:, 0].sum(), wc[:, 1].sum(), detail["multi_op_pairs"], no_row, empty))
    # the fuzz is not empty
    assert rc[:, 0].sum() >= 30 and rc[:, 1].sum() >= 1000 and wc[:, 0].sum() >= 400 and wc[:, 1].sum() >= 400
    assert detail["multi_op_pairs"] >= 2000 and no_row >= 10 and empty == 0
    # every third read through the serial walk: the same table
    _check(eng, _forced_serial(rs, 3), table, tab, row_ps, stranded)


_spliced = {}


def _spliced_case(seed):
    """phaseref.gen_case(errors=True) with its truth as the phase table, in sets of ten sites; regions: its exons and two spans over all."""
    if seed not in _spliced:
        ref, rs, sites, truth, _ = P.gen_case(seed, errors=True)
        table = sites.copy()
        table["h1"], table["ps"] = truth, 1000 + np.arange(len(table)) // 10
        exons = HR.phase_case_exons(seed)
        regs = sorted([(a, b, (0, 1, 2)[k % 3]) for k, (a, b) in enumerate(exons)] + [(exons[0][0], exons[-1][1], 0), (0, len(ref), 1)], key=lambda r: (r[0], r[1]))
        _spliced[seed] = (rs, table) + HR.pack(regs, HR.row_table(regs, table))
    return _spliced[seed]


@pytest.mark.parametrize("seed", range(2))
def test_spliced_reads_over_their_exons_and_the_filters(eng, seed):
    rs, table, tab, row_ps = _spliced_case(seed)
    failing = [i for i in range(len(rs)) if not P.votes(rs.reads[i], P.DEFAULT_PARAMS)]
    assert len(rs) == 403 and len(failing) >= 20 and len(tab) >= 10
    # every read starts inside an exon: the exons found again are the generator's
    assert all(any(a <= int(r["pos"]) < b for a, b in HR.phase_case_exons(seed)) for r in rs.reads)
    rc, wc = _check(eng, rs, table, tab, row_ps, 1)
    assert wc[:, 0].sum() > 200 and wc[:, 1].sum() > 200 and rc[:, 0].sum() > 20 and rc[:, 1].sum() > 100      # all four kinds of count occur
    tags = eng.haplotags()
    total = int(rc.sum()) + int(wc.sum())
    # the voters follow set_params: the reads already loaded are filtered anew, the tags stay
    eng.set_params(min_mq=30)
    rc2, wc2 = _check(eng, rs, table, tab, row_ps, 1, dict(min_mq=30, excl_flags=2316), load=False)
    eng.set_params(min_mq=0, excl_flags=0)
    rc3, wc3 = _check(eng, rs, table, tab, row_ps, 1, dict(min_mq=0, excl_flags=0), load=False)
    assert int(rc2.sum()) + int(wc2.sum()) <= total < int(rc3.sum()) + int(wc3.sum())
    after = eng.haplotags()
    assert after[0].tolist() == tags[0].tolist() and after[1] == tags[1]
    eng.set_params(min_mq=61)
    assert sum(int(x.sum()) for x in eng.hap_region_counts(tab, row_ps, 0)) == 0


def _long_read(n_ops, lead_clip):
    """(cigar ops [(length, letter)], [(op index, first, past the last)] of its M / D ops) of a read at 0-based 1000: M ops on every other
    op, between them N 7, I 2 and D 2 in turn; lead_clip: a soft clip first, which moves the M ops to the odd indices."""
    ops = [(2, "S")] if lead_clip else []
    between = [(7, "N"), (2, "I"), (2, "D")]
    while len(ops) < n_ops:
        ops.append((3 + len(ops) % 4, "M"))
        if len(ops) < n_ops:
            ops.append(between[(len(ops) // 2) % 3])
    assert len(ops) == n_ops and ops[-1][1] == "M"
    x, cov = 1000, []
    for k, (ln, op) in enumerate(ops):
        if op in "MD":
            cov.append((k, x, x + ln))
        if op in "MDN":
            x += ln
    return ops, cov


@pytest.mark.parametrize("n_ops, lead_clip", [(17, False), (33, False), (40, True)], ids=["17_ops", "33_ops", "40_ops"])
def test_regions_over_ops_of_two_rounds_count_once_in_both_walks(eng, n_ops, lead_clip):
    ops, cov = _long_read(n_ops, lead_clip)
    regs = [(1000, cov[-1][2], 0), (999, 1000, 0), (cov[-1][2], cov[-1][2] + 1, 0), (cov[-1][2] - 1, cov[-1][2], 0)]
    for edge in range(16, n_ops, 16):                        # ops edge - 1 and edge lie in different rounds of 16
        near = [c for c in cov if edge - 4 <= c[0] < edge + 4]
        before, behind = [c for c in near if c[0] < edge], [c for c in near if c[0] >= edge]
        assert before and behind
        regs += [(before[0][1], behind[-1][2], 0), (before[-1][2] - 1, behind[0][1] + 1, 0), (before[-1][1], behind[0][2], 0), (behind[0][1], behind[0][1] + 1, 0)]
    regs = sorted(set(regs), key=lambda r: (r[0], r[1]))
    table = hapref.make_sites([(1002, "A", "C", 0, 5)])
    tab, row_ps = HR.pack(regs, [[5] if k % 2 else [] for k in range(len(regs))])
    n_seq = sum(ln for ln, op in ops if op in "MIS")
    forms = {"plain": "".join("%d%s" % o for o in ops)}
    k_m = [k for k, o in enumerate(ops) if o[1] == "M" and o[0] >= 3][0]
    forms["eq_beside_m"] = "".join("%d%s" % o if k != k_m else "2=%dM" % (o[0] - 2) for k, o in enumerate(ops))
    forms["empty_op"] = "".join(("%d%s" % o) + ("0I" if k == 1 else "") for k, o in enumerate(ops))      # no plain CIGAR: the serial walk
    forms["pad"] = "".join(("%d%s" % o) + ("1P" if k == n_ops - 2 else "") for k, o in enumerate(ops))
    got = {}
    for name, cigar in forms.items():
        rs = _readset([(1000, cigar, "A" * n_seq)])
        assert HR.covered(rs, 0)[0][0] == 1000 and HR.covered(rs, 0)[-1][1] == cov[-1][2]
        rc, wc = _check(eng, rs, table, tab, row_ps)
        got[name] = (rc.tolist(), wc.tolist())
        # one read: every region that a covered base lies in holds exactly one count, the others none
        offs = tab["row_off"].tolist() + [len(row_ps)]
        for j, (a, b, _) in enumerate(regs):
            hit = any(x0 < b and x1 > a for _, x0, x1 in cov)
            assert int(rc[j].sum()) + int(wc[offs[j]:offs[j + 1]].sum()) == (1 if hit else 0), (name, j, regs[j])
    assert all(g == got["plain"] for g in got.values())
    assert sum(1 for a, b, _ in regs if sum(1 for _, x0, x1 in cov if x0 < b and x1 > a) >= 2) >= 3 * ((n_ops - 1) // 16)


def test_two_thousand_identical_reads_on_one_region(eng):
    rs = _readset([(100, "10M50N10M", "A" * 20, 16 * (k % 2)) for k in range(2000)])
    table = hapref.make_sites(HR.HAND_SITES)
    tab, row_ps = HR.pack([(90, 200, 1), (90, 200, 0), (105, 165, 2)], [[7], [], [6, 7, 8]])
    rc, wc = _check(eng, rs, table, tab, row_ps)
    assert rc.tolist() == [[0, 0], [0, 2000], [0, 0]] and wc.tolist() == [[2000, 0], [0, 0], [2000, 0], [0, 0]]
    rc, wc = _check(eng, rs, table, tab, row_ps, 1, load=False)
    assert rc.tolist() == [[0, 0], [0, 2000], [0, 0]] and wc.tolist() == [[1000, 0], [0, 0], [1000, 0], [0, 0]]


@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_read_counts_around_a_workgroup(eng, n):
    rs = _readset([(100 + k // 3, "4M", ("AAAA", "CCCC", "GGGG")[k % 3]) for k in range(n)])
    table = hapref.make_sites([(p, "A", "C", 0, 1) for p in (103, 104, 105, 106)])
    tab, row_ps = HR.pack([(0, 50, 0), (100, 103, 0), (101, 120, 0), (104, 105, 0)], [[], [1], [1], [2]])
    _check(eng, rs, table, tab, row_ps)


# ---- 2. life cycle
def test_the_call_leaves_tags_sets_count_tables_and_a_scan_alone(eng):
    rs, table, tab, row_ps = _spliced_case(1)
    ref = P.gen_case(1, errors=True)[0]
    query = table.copy()
    query["h1"] = 0
    eng.set_params(min_coverage=2)
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    eng.set_reference(1, ref)
    assert eng.params.channels == 18

    def scan():
        n = eng.scan(1, len(ref))
        return n, eng.tensors(rescaled=True).tobytes(), eng.tensors(rescaled=False).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()

    plain, tags, sets, counts = scan(), eng.haplotags(), eng.read_phase_sets().tolist(), eng.hap_counts(query).tobytes()
    assert plain[0] > 20 and tags[1]["n_hp1"] > 30 and tags[1]["n_hp2"] > 30
    eng.load_reads(rs)
    _check(eng, rs, table, tab, row_ps, load=False)
    after = eng.haplotags()
    assert after[0].tolist() == tags[0].tolist() and after[1] == tags[1] and eng.read_phase_sets().tolist() == sets
    assert eng.hap_counts(query).tobytes() == counts
    assert scan() == plain
    _check(eng, rs, table, tab, row_ps, 2, load=False)        # after the scan: what it left is still there
    assert (eng.tensors(rescaled=True).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()) == (plain[1], plain[3], plain[4])
    assert scan() == plain and eng.hap_counts(query).tobytes() == counts


def test_a_new_phase_table_changes_the_counts_as_the_restatement_says(eng):
    rs, table, tab, row_ps = _fuzz_case(1)
    rc, wc = _check(eng, rs, table, tab, row_ps)
    other = table.copy()
    other["h1"] ^= 1
    eng.set_phase_sites(other)                                # reads stay loaded: tagged again
    rc2, wc2 = _check(eng, rs, other, tab, row_ps, load=False)
    assert np.array_equal(rc2, rc) and np.array_equal(wc2, wc[:, ::-1]) and not np.array_equal(wc2, wc)
    moved = table.copy()
    moved["ps"] += 100000                                     # against the old numbers every tagged read is "tagged in another set"
    eng.set_phase_sites(moved)
    rc3, wc3 = _check(eng, rs, moved, tab, row_ps, load=False)
    offs = tab["row_off"].tolist() + [len(row_ps)]
    assert wc3.sum() == 0 and rc3[:, 0].tolist() == rc[:, 0].tolist()
    assert rc3[:, 1].tolist() == [int(rc[j, 1]) + int(wc[offs[j]:offs[j + 1]].sum()) for j in range(len(tab))]


def test_no_regions_no_reads_and_no_table(eng):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    rs, table, tab, row_ps = _fuzz_case(0)
    eng.load_reads(rs)
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        eng.hap_region_counts(tab, row_ps)
    _check(eng, rs, table, tab, row_ps)                       # the context is usable afterwards
    eng.set_profiling(True)
    try:
        eng.reset_kernel_stats()
        rc, wc = eng.hap_region_counts(None, None)
        assert rc.shape == (0, 2) and wc.shape == (0, 2) and "k_hap_region_counts" not in eng.kernel_stats()
        eng.hap_region_counts(tab, row_ps, 1)
        assert eng.kernel_stats()["k_hap_region_counts"]["launches"] == 1
        eng.load_reads(ReadSet.from_records([]))
        eng.reset_kernel_stats()
        rc, wc = eng.hap_region_counts(tab, row_ps)
        assert rc.shape == (50, 2) and wc.shape == (len(row_ps), 2) and rc.sum() == 0 and wc.sum() == 0 and "k_hap_region_counts" not in eng.kernel_stats()
    finally:
        eng.set_profiling(False)
    # regions far from every read, and a table without any row
    eng.load_reads(rs)
    far, none = HR.pack([(7000, 7001, 0), (2000000000, 2147483647, 0)], [[1000], []])
    rc, wc = eng.hap_region_counts(far, none)
    assert rc.sum() == 0 and wc.sum() == 0
    bare = tab.copy()
    bare["row_off"] = 0
    rc, wc = _check(eng, rs, table, bare, np.zeros(0, np.int32), load=False)
    assert wc.shape == (0, 2) and rc[:, 1].sum() > 3000
    eng.set_phase_sites(None)                                 # cleared: refused again
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        eng.hap_region_counts(tab, row_ps)


BAD_TABLES = [
    ("unsorted", dict(start=(2, 5)), "region 2:"),
    ("start_not_below_end", dict(end=(1, 200)), "region 1:"),
    ("row_off_decreases", dict(row_off=(2, 0)), "region 2:"),
    ("strand_3", dict(strand=(0, 3)), "region 0:"),
]


@pytest.mark.parametrize("name, patch, words", BAD_TABLES, ids=[b[0] for b in BAD_TABLES])
def test_bad_tables_name_the_region_through_the_engine(eng, name, patch, words):
    from clair3_rna_amd import capi
    tab, row_ps = HR.pack([(100, 110, 0), (200, 300, 0), (250, 260, 0)], [[1], [1, 2], []])
    for k, (j, v) in patch.items():
        tab[k][j] = v
    eng.set_phase_sites(hapref.make_sites([(1, "A", "C", 0, 1)]))
    eng.load_reads(_readset([(90, "40M", "A" * 40)]))
    with pytest.raises(capi.C3RError, match=words):
        eng.hap_region_counts(tab, row_ps)
    with pytest.raises(capi.C3RError, match="stranded 3"):
        eng.hap_region_counts(HR.pack([(100, 110, 0)], [[]])[0], None, 3)
    with pytest.raises(TypeError):
        eng.hap_region_counts(np.zeros(2, np.int32), None)
    good = HR.pack([(100, 110, 0), (200, 300, 0), (250, 260, 0)], [[1], [1, 2], []])
    assert eng.hap_region_counts(*good)[0][:, 0].tolist() == [1, 0, 0]


# ---- 3. the C ABI alone
def test_the_stand_alone_check_program(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to build tests/c/hap_regions_check.c"
    lib = os.path.join(ROOT, "clair3_rna_amd")
    exe = str(tmp_path / "hap_regions_check")
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "hap_regions_check.c"),
                           "-L", lib, "-lc3r", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "hap_regions_check: ok" in out.stdout, out.stdout + out.stderr


# ---- 4. drivers
@pytest.mark.parametrize("indels", [False, True], ids=["snv_table", "haplotag_indels"])
def test_hap_expr_writes_the_restatements_table(tmp_path, indels):
    s = HR.driver_sample(str(tmp_path))
    out = str(tmp_path / "expr.tsv")
    msgs = []
    done = hap_expr.Run(hap_expr.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["bed_fn"], "--output_fn", out]
                                                           + (["--haplotag_indels"] if indels else [])), log=msgs.append)
    got = open(out).read().split("\n")
    want = HR.predicted_lines(s, "chr1") + HR.uncounted_lines(s, "chr2") + HR.uncounted_lines(s, "chrEmpty")
    assert got[0] == hap_expr.HEADER and got[-1] == "" and got[1:-1] == want
    assert sorted(done) == ["chr1", "chr2", "chrEmpty"] and len(msgs) == 3 and done["chr1"]["launched"]
    body = [l.split("\t") for l in HR.predicted_lines(s, "chr1")]
    assert sum(int(l[6]) + int(l[7]) for l in body if l[5] != ".") >= 50 and sum(int(l[9]) for l in body if l[5] == ".") >= 20
    hap_expr.Run(hap_expr.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--regions_bed_fn", s["bed_fn"], "--output_fn", out, "--stranded", "same",
                                                     "--ctg_name", "chr1"] + (["--haplotag_indels"] if indels else [])), log=msgs.append)
    assert open(out).read().split("\n")[1:-1] == HR.predicted_lines(s, "chr1", 1) != want[:len(HR.predicted_lines(s, "chr1"))]


@pytest.fixture(scope="module")
def called(tmp_path_factory):
    """Two contigs of hapref.gen_case reads, a BED over both, and call_sample --phasing builtin on them without and with --hap_expression_bed."""
    from clair3_rna_amd import bam, bamio, call_sample, io, synth
    tmp = str(tmp_path_factory.mktemp("hapregion_drivers"))
    contigs, reads, bed = [], {}, {}
    for name, seed in (("chr1", 11), ("chr2", 12)):
        ref, rs, _, _ = hapref.gen_case(seed)
        contigs.append((name, ref))
        reads[name] = rs
        bed[name] = [(a, b, "%s_r%d" % (name, k), (None, "+", "-")[k % 3]) for k, (a, b) in enumerate([(3000, 3400), (100, 5000), (1500, 1501), (3000, 3400), (4000, 4800)])]
    fa, wfn, bed_fn = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model"), os.path.join(tmp, "exons.bed")
    io.write_fasta(fa, contigs)
    np.save(wfn + ".c3rw.npy", synth.random_weights(30, seed=5))    # (the sample of tests/test_gpu_haplotag_bam.py's driver case: the built-in phasing tags reads of both haplotypes here)
    np.save(wfn + "18.c3rw.npy", synth.random_weights(18, seed=5))
    with open(bed_fn, "w") as f:
        for name in ("chr2", "chr1"):
            for a, b, label, strand in bed[name]:
                f.write("%s\t%d\t%d\t%s\t0\t%s\n" % (name, a, b, label, strand or "."))
    bam_fn = os.path.join(tmp, "plain.bam")
    bam.write_bam(bam_fn, [(n, len(r)) for n, r in contigs], reads)
    bamio.index_build(bam_fn)
    s = dict(tmp=tmp, bam=bam_fn, bed_fn=bed_fn, bed=bed, reads=reads)
    for out, extra in (("base", []), ("flag", ["--hap_expression_bed", bed_fn, "--hap_expression_stranded", "reverse"])):
        argv = ["--bam_fn", bam_fn, "--ref_fn", fa, "--output_dir", os.path.join(tmp, out), "--pileup_model_path", wfn + "18", "--phased_pileup_model_path", wfn,
                "--chunk_num", "3", "--min_coverage", "2", "--enable_phasing_model", "--phasing", "builtin"] + extra
        assert call_sample.Run(call_sample.build_parser().parse_args(argv), log=lambda m: None) == 0
    return s


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_call_sample_with_the_flag_equals_the_steps_by_hand_and_the_restatement(called, tmp_path):
    from clair3_rna_amd import phasedvcf
    base, flag = os.path.join(called["tmp"], "base"), os.path.join(called["tmp"], "flag")
    tsv = os.path.join(flag, "output_enable_phasing_hap_expression.tsv")
    # without the flag: the file set of the parent; with it: one file more and no byte different
    assert not [f for f in _files(base) if "hap_expression" in f]
    assert _files(flag) == sorted(_files(base) + ["output_enable_phasing_hap_expression.tsv"])
    for f in _files(base):
        if f.endswith((".vcf.gz", ".tbi")):
            # (phase_vcf's per-contig files go through Python's gzip, which stamps the time into the header: those are compared inflated)
            both = [(gzip.open if f.startswith("tmp") and f.endswith(".gz") else open)(os.path.join(d, f), "rb").read() for d in (base, flag)]
            assert both[0] == both[1], f
    # the step by hand, on the directory the built-in phasing left
    per = os.path.join(base, "tmp", "phased_output", "phased_vcf")
    by_hand = str(tmp_path / "by_hand.tsv")
    hap_expr.Run(hap_expr.build_parser().parse_args(["--bam_fn", called["bam"], "--phased_vcf_fn", per, "--regions_bed_fn", called["bed_fn"], "--output_fn", by_hand,
                                                     "--stranded", "reverse"]), log=lambda m: None)
    assert open(tsv).read() == open(by_hand).read()
    # the restatement's prediction from the phased VCFs
    want, n_sites = [], 0
    for ctg in ("chr1", "chr2"):
        table = phasedvcf.contig_sites(per, ctg)
        n_sites += len(table)
        want += HR.predicted_lines(dict(bed=called["bed"], reads=called["reads"], case={}), ctg, 2, table=table) if len(table) else HR.uncounted_lines(called, ctg)
    got = open(tsv).read().split("\n")
    assert got[0] == hap_expr.HEADER and got[1:-1] == want
    tagged = sum(int(l.split("\t")[6]) + int(l.split("\t")[7]) for l in want if l.split("\t")[5] != ".")
    print("phased sites %d, reads counted on a haplotype %d" % (n_sites, tagged))
    assert n_sites >= 4 and tagged >= 20                      # the comparison is about something
