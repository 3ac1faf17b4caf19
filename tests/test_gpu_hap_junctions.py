"""Haplotype-resolved splice-junction counts on the device (c3r_hap_junction_counts / k_hap_junction_counts) against tests/hapjunctionref.py,
the plain-Python restatement of the rule `hap_junctions`: element for element, no tolerance; both CIGAR walks; both kernel variants (counted
in LDS first, and directly); growth of the hash tables from the smallest size; that the call leaves tags, sets, count tables and scans
alone; and the drivers (hap_junctions, call_sample --hap_junctions)."""
import gzip
import os

import numpy as np
import pytest

from clair3_rna_amd import hap_junctions
from tests import hapjunctionref as HJ
from tests import hapref

pytestmark = pytest.mark.gpu

VARIANTS = [False, True]                                      # c3r_set_hap_junction_direct
KERNEL = {False: "k_hap_junction_counts", True: "k_hap_junction_counts_direct"}


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clean(request):
    """Every test of this module starts and leaves its engine without phase sites, with default parameters and the aggregated kernel."""
    yield
    if "eng" in request.fixturenames:
        from clair3_rna_amd import capi
        e = request.getfixturevalue("eng")
        e.set_phase_sites(None)
        e.set_hap_junction_direct(False)
        e.set_profiling(False)
        e.params = capi.default_params()
        e.set_params()


def _same(got, want):
    j, r = got
    ej, er = want
    assert j.dtype == ej.dtype and r.dtype == er.dtype
    assert len(j) == len(ej), (len(j), len(ej))
    for f in ("start", "end", "reads", "reverse", "untagged", "row_off"):
        assert np.array_equal(j[f], ej[f]), (f, np.argwhere(j[f] != ej[f])[:10].ravel(), j[f][j[f] != ej[f]][:10], ej[f][j[f] != ej[f]][:10])
    assert len(r) == len(er), (len(r), len(er))
    for f in ("ps", "hp1", "hp2"):
        assert np.array_equal(r[f], er[f]), (f, np.argwhere(r[f] != er[f])[:10].ravel())
    assert j.tobytes() == ej.tobytes() and r.tobytes() == er.tobytes()


def _check(eng, rs, table, params=HJ.DEFAULT_PARAMS, load=True, hints=(0,), found=None):
    """The engine's arrays for (rs, table) under its current filters equal the restatement's under `params`, with both kernel variants and
    every slots_hint of `hints`; returns the restatement's dict."""
    found = HJ.counts(rs, table, params) if found is None else found
    assert HJ.invariant(found)
    want = HJ.arrays(found)
    if load:
        eng.set_phase_sites(table)
        eng.load_reads(rs)
    for direct in VARIANTS:
        eng.set_hap_junction_direct(direct)
        for hint in hints:
            _same(eng.hap_junction_counts(hint), want)
    eng.set_hap_junction_direct(False)
    return found


# ---- 1. against the restatement
@pytest.mark.parametrize("case", HJ.HAND, ids=[c[0] for c in HJ.HAND])
def test_the_hand_cases(eng, case):
    rs, table, want = HJ.hand_inputs(case)
    assert _check(eng, rs, table) == want
    assert _check(eng, HJ.forced_serial(rs), table) == want            # the same through the serial walk
    # without a table: a plain junction counter
    eng.set_phase_sites(None)
    bare = _check(eng, rs, None, load=False)
    assert sorted(bare) == sorted(want) and all(e["untagged"] == e["reads"] and not e["rows"] for e in bare.values())


@pytest.mark.parametrize("name", ["both_haplotypes_and_an_untagged_read_on_one_junction", "same_start_other_end", "forward_and_reverse"])
def test_hand_cases_under_an_allele_table(eng, name):
    """The tags of c3r_set_phase_alleles (--haplotag_indels) count like those of c3r_set_phase_sites: the same table as REF-and-one-SNV
    allele sites gives the hand answers, and a generated case the restatement's."""
    from clair3_rna_amd import phasing
    rs, table, want = HJ.hand_inputs([c for c in HJ.HAND if c[0] == name][0])
    assert any(e["rows"] for e in want.values())
    eng.set_phase_alleles(*phasing.snv_sites_as_alleles(table))
    eng.load_reads(rs)
    assert _check(eng, rs, table, load=False) == want
    rs, table = HJ.shared_case(3)
    eng.load_reads(rs)                                        # (tagged under the hand table: other counts)
    eng.set_phase_alleles(*phasing.snv_sites_as_alleles(table))      # reads stay loaded: tagged again
    found = _check(eng, rs, table, load=False, hints=(0, 1))
    assert sum(len(e["rows"]) for e in found.values()) >= 20
    eng.set_phase_alleles(None, None)


_cases = {}


def _case(kind, seed):
    if (kind, seed) not in _cases:
        rs, table = (HJ.shared_case if kind == "shared" else HJ.distinct_case)(seed)
        _cases[(kind, seed)] = (rs, table, HJ.counts(rs, table))
    return _cases[(kind, seed)]


@pytest.mark.parametrize("seed", range(4))
def test_shared_junctions(eng, seed):
    rs, table, found = _case("shared", seed)
    n_untagged = sum(e["untagged"] > 0 for e in found.values())
    print("seed %d: %d junctions, most reads on one %d, %d with two or more rows, %d with both haplotypes, %d with untagged reads"
          % (seed, len(found), max(e["reads"] for e in found.values()), sum(len(e["rows"]) >= 2 for e in found.values()),
             sum(any(a and b for a, b in e["rows"].values()) for e in found.values()), n_untagged))
    assert len(found) >= 10 and max(e["reads"] for e in found.values()) >= 50 and sum(len(e["rows"]) >= 2 for e in found.values()) >= 5
    _check(eng, rs, table, found=found, hints=(0, 1))
    _check(eng, HJ.forced_serial(rs, 3), table, found=found)          # every third read through the serial walk: the same table


def test_shared_junctions_hold_untagged_reads_somewhere():
    assert sum(sum(e["untagged"] > 0 for e in _case("shared", seed)[2].values()) for seed in range(4)) >= 1


@pytest.mark.parametrize("seed", range(4))
def test_many_distinct_junctions_and_the_growth_of_the_tables(eng, seed):
    rs, table, found = _case("distinct", seed)
    per_read = max(len(HJ.read_junctions(rs, i)) for i in range(len(rs)))
    print("seed %d: %d junctions from %d reads, up to %d on one read, %d rows" % (seed, len(found), len(rs), per_read, sum(len(e["rows"]) for e in found.values())))
    assert len(found) >= 1500 and per_read >= 10 and len(rs) <= 400
    _check(eng, rs, table, found=found, hints=(1, 0, 1 << 16))
    # the smallest tables grow round by round, the default ones not at all
    eng.set_profiling(True)
    for direct in VARIANTS:
        eng.set_hap_junction_direct(direct)
        eng.reset_kernel_stats()
        eng.hap_junction_counts(1)
        grown = eng.kernel_stats()[KERNEL[direct]]["launches"]
        eng.reset_kernel_stats()
        eng.hap_junction_counts()
        assert grown >= 8 and eng.kernel_stats()[KERNEL[direct]]["launches"] == 1 and KERNEL[not direct] not in eng.kernel_stats()


def test_four_thousand_reads_on_one_junction(eng):
    rs = HJ.readset([(100, "10M50N10M", HJ.A20, 16 * (k % 2)) for k in range(2000)] + [(100, "10M50N10M", HJ.C20) for _ in range(2000)])
    found = _check(eng, rs, hapref.make_sites(HJ.HAND_SITES), hints=(0, 1))
    assert found == {(110, 160): dict(reads=4000, reverse=1000, untagged=0, rows={7: [2000, 2000]})}


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_read_counts_around_a_workgroup(eng, n):
    rs = HJ.readset([(100 + k // 3, "4M%dN4M" % (5 + k % 4), ("AAAAAAAA", "CCCCCCCC", "GGGGGGGG")[k % 3]) for k in range(n)])
    _check(eng, rs, hapref.make_sites([(p, "A", "C", 0, 1 + p % 2) for p in (103, 104, 105, 106)]))


def test_a_read_with_junctions_in_several_rounds_of_lanes(eng):
    # 40 introns on one read: ops 0 .. 80, five rounds of the plain walk's 16 lanes; the same with an empty op, through the serial walk
    cigar = "".join("3M%dN" % (7 + k) for k in range(40)) + "3M"
    rs = HJ.readset([(1000, cigar, "A" * 123), (1000, cigar.replace("3M7N", "3M0I7N", 1), "A" * 123, 16)])
    found = _check(eng, rs, hapref.make_sites([(1002, "A", "C", 0, 5)]))
    assert len(found) == 40 and all(e == dict(reads=2, reverse=1, untagged=0, rows={5: [2, 0]}) for e in found.values())


def _introns(r, n=40):
    """A CIGAR of n introns between 3-base M ops whose lengths, and so whose positions, depend on r; and its number of bases."""
    return "".join("3M%dN" % (7 + k + 41 * r) for k in range(n)) + "3M", 3 * n + 3


def test_more_junctions_in_a_workgroup_than_its_lds_table_holds(eng):
    # 20 reads at one position, 40 introns each, no two reads share one: a workgroup's 16 reads bring 640 keys to the 256 slots of its
    # table in LDS, so most of them go straight to the global tables
    recs = []
    for r in range(20):
        cigar, n = _introns(r)
        recs.append((1000, cigar, ("AAA" if r % 2 else "ACA") + "A" * (n - 3), 16 * (r % 3 == 0)))
    found = _check(eng, HJ.readset(recs), hapref.make_sites([(1002, "A", "C", 0, 5)]), hints=(0, 1))
    assert len(found) == 800 and all(e["reads"] == 1 and e["rows"] in ({5: [1, 0]}, {5: [0, 1]}) for e in found.values())
    assert sum(e["rows"][5][1] for e in found.values()) == 400 and sum(e["reverse"] for e in found.values()) == 280


def test_more_phase_sets_on_a_workgroups_junctions_than_its_lds_table_holds(eng):
    # 20 reads share 40 introns and each is tagged in a set of its own: the first base of its r-th M op is the only base of the read that
    # shows an allele of a site (the other reads show T there, neither allele).  A workgroup's 16 reads bring 40 junctions and 640
    # (junction, set) pairs to the 256 slots of each LDS table: the junctions all fit, most of their rows go to the global table directly
    cigar, n = _introns(0)
    starts, x = [], 1000
    for k in range(40):
        starts.append(x)
        x += 3 + 7 + k
    recs, sites = [], []
    for r in range(20):
        seq = ["T"] * n
        seq[3 * r] = "AC"[r % 2]
        recs.append((1000, cigar, "".join(seq)))
        sites.append((starts[r] + 1, "A", "C", 0, 100 + r))
    found = _check(eng, HJ.readset(recs), hapref.make_sites(sites), hints=(0, 1))
    assert len(found) == 40 and all(e["reads"] == 20 and e["untagged"] == 0 and sorted(e["rows"]) == list(range(100, 120)) for e in found.values())
    assert all(e["rows"][100 + r] == ([1, 0], [0, 1])[r % 2] for e in found.values() for r in range(20))


# ---- 2. no table, no reads, life cycle
def test_no_phase_table_and_no_reads(eng):
    from clair3_rna_amd.reads import ReadSet
    rs, table, found = _case("shared", 1)
    bare = _check(eng, rs, None)
    assert sorted(bare) == sorted(found) and all(e["untagged"] == e["reads"] and not e["rows"] for e in bare.values())
    assert len(eng.hap_junction_counts()[1]) == 0
    eng.set_profiling(True)
    eng.load_reads(ReadSet.from_records([]))
    for direct in VARIANTS:
        eng.set_hap_junction_direct(direct)
        eng.reset_kernel_stats()
        j, r = eng.hap_junction_counts()
        assert len(j) == 0 and len(r) == 0 and j.dtype.itemsize == 24 and r.dtype.itemsize == 12 and not [k for k in eng.kernel_stats() if "junction" in k]
    # reads without any junction
    eng.set_hap_junction_direct(False)
    eng.load_reads(HJ.readset([(100, "20M", HJ.A20), (105, "5M2D5M3I7M", HJ.A20)]))
    eng.reset_kernel_stats()
    j, r = eng.hap_junction_counts()
    assert len(j) == 0 and len(r) == 0 and eng.kernel_stats()["k_hap_junction_counts"]["launches"] == 1


def test_the_call_leaves_tags_sets_count_tables_and_scans_alone(eng):
    from tests import hapregionref, phaseref
    rs, table, found = _case("shared", 1)
    ref = phaseref.gen_case(1)[0]
    query = table.copy()
    query["h1"] = 0
    regions = hapregionref.pack([(0, len(ref), 0), (1000, 3000, 1)], [[1000, 1001, 1002], [1001]])

    def scan():
        n = eng.scan(1, len(ref))
        return n, eng.tensors(rescaled=True).tobytes(), eng.tensors(rescaled=False).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()

    for channels in (18, 30):
        eng.set_params(channels=channels, min_coverage=2)
        eng.set_phase_sites(table)
        eng.load_reads(rs)
        eng.set_reference(1, ref)
        assert eng.params.channels == channels
        before = (scan(), eng.haplotags()[0].tolist(), eng.haplotags()[1], eng.read_phase_sets().tolist(), eng.hap_counts(query).tobytes(),
                  [x.tobytes() for x in eng.hap_region_counts(*regions)])
        assert before[0][0] > 20 and before[2]["n_hp1"] > 30 and before[2]["n_hp2"] > 30
        eng.load_reads(rs)
        _check(eng, rs, table, found=found, load=False, hints=(1, 0))
        after = (scan(), eng.haplotags()[0].tolist(), eng.haplotags()[1], eng.read_phase_sets().tolist(), eng.hap_counts(query).tobytes(),
                 [x.tobytes() for x in eng.hap_region_counts(*regions)])
        assert after == before
        _check(eng, rs, table, found=found, load=False)             # after the scan: what it left is still there
        assert scan() == before[0]


def test_the_filters_a_new_table_and_a_second_load(eng):
    from clair3_rna_amd import capi
    rs, table, found = _case("shared", 2)
    _check(eng, rs, table, found=found)
    # the counted reads follow set_params: the reads already loaded are filtered anew
    eng.set_params(min_mq=30)
    strict = _check(eng, rs, table, dict(min_mq=30, excl_flags=2316), load=False)
    eng.set_params(min_mq=0, excl_flags=0)
    loose = _check(eng, rs, table, dict(min_mq=0, excl_flags=0), load=False)
    total = lambda f: sum(e["reads"] for e in f.values())
    assert total(strict) <= total(found) <= total(loose) and total(strict) < total(loose)
    eng.set_params(min_mq=61)
    assert len(eng.hap_junction_counts()[0]) == 0
    eng.set_params(min_mq=5, excl_flags=2316)
    # a new table with the reads loaded: tagged again, the haplotypes swap
    other = table.copy()
    other["h1"] ^= 1
    eng.set_phase_sites(other)
    swapped = _check(eng, rs, other, load=False)
    assert all(swapped[k]["rows"] == {ps: c[::-1] for ps, c in found[k]["rows"].items()} for k in found) and swapped != found
    # the getter: its capacities, and a second load forgets the result
    nj, nr = len(found), sum(len(e["rows"]) for e in found.values())
    j, r = np.zeros(nj, capi.HAP_JUNCTION_DTYPE), np.zeros(nr, capi.HAP_JUNCTION_ROW_DTYPE)
    get = lambda cj, cr: eng.L.c3r_get_hap_junctions(eng.h, j.ctypes.data, cj, r.ctypes.data, cr)
    assert get(nj, nr) == 0 and get(nj + 5, nr + 5) == 0 and j.tobytes() == HJ.arrays(swapped)[0].tobytes()
    EINVAL = -1
    assert capi.C3R_ERRORS[EINVAL] == "EINVAL" and get(-1, nr) == EINVAL and nj >= 10 and nr >= 10
    assert get(nj, nr - 1) == EINVAL and get(nj - 1, nr) == EINVAL and "do not fit" in eng.L.c3r_last_error(eng.h).decode()
    eng.load_reads(rs)
    assert get(nj, nr) == EINVAL and "nothing has been counted" in eng.L.c3r_last_error(eng.h).decode()
    with pytest.raises(capi.C3RError, match="negative"):
        eng.hap_junction_counts(-1)
    with pytest.raises(capi.C3RError, match="neither 0 nor 1"):
        eng._chk(eng.L.c3r_set_hap_junction_direct(eng.h, 2))
    _check(eng, rs, other, load=False, found=swapped)               # the context is usable afterwards


# ---- 3. the C ABI alone
def test_the_stand_alone_check_program(tmp_path):
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to build tests/c/hap_junctions_check.c"
    lib = os.path.join(root, "clair3_rna_amd")
    exe = str(tmp_path / "hap_junctions_check")
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "hap_junctions_check.c"),
                           "-L", lib, "-lc3r", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "hap_junctions_check: ok" in out.stdout, out.stdout + out.stderr


# ---- 4. drivers
def test_hap_junctions_writes_the_restatements_table(tmp_path):
    s = HJ.driver_sample(str(tmp_path))
    out = str(tmp_path / "junctions.tsv")
    msgs = []
    run = lambda extra: hap_junctions.Run(hap_junctions.build_parser().parse_args(["--bam_fn", s["bam"], "--output_fn", out] + extra), log=msgs.append)
    done = run(["--phased_vcf_fn", s["per"]])
    got = open(out).read().split("\n")
    want1 = HJ.predicted_lines(s, "chr1")
    assert got[0] == hap_junctions.HEADER and got[-1] == "" and got[1:-1] == want1 + HJ.predicted_lines(s, "chr2")
    assert sorted(done) == ["chr1", "chr2", "chrEmpty"] and len(msgs) == 3 and done["chr1"]["rows"] >= 20 and done["chr2"]["rows"] == 0 and done["chr2"]["junctions"] >= 100
    run(["--phased_vcf_fn", s["per"], "--ref_fn", s["fa"]])
    with_ref = open(out).read().split("\n")[1:-1]
    assert with_ref == HJ.predicted_lines(s, "chr1", True) + HJ.predicted_lines(s, "chr2", True)
    assert all(l.split("\t")[3] != "." for l in with_ref) and [l.split("\t")[:3] + l.split("\t")[5:] for l in with_ref] == [l.split("\t")[:3] + l.split("\t")[5:] for l in got[1:-1]]
    run(["--phased_vcf_fn", s["per"], "--min_reads", "2", "--ctg_name", "chr1"])
    few = open(out).read().split("\n")[1:-1]
    assert few == HJ.predicted_lines(s, "chr1", min_reads=2) and 0 < len(few) < len(want1)
    run(["--ctg_name", "chr1"])                               # no phased VCF: a plain junction counter
    assert open(out).read().split("\n")[1:-1] == HJ.predicted_lines(s, "chr1", phased=False)


@pytest.fixture(scope="module")
def called(tmp_path_factory):
    """Two contigs of hapref.gen_case reads and call_sample --phasing builtin on them without and with --hap_junctions."""
    from clair3_rna_amd import bam, bamio, call_sample, io, synth
    tmp = str(tmp_path_factory.mktemp("hapjunction_drivers"))
    contigs, reads, refs = [], {}, {}
    for name, seed in (("chr1", 11), ("chr2", 12)):
        ref, rs, _, _ = hapref.gen_case(seed)
        contigs.append((name, ref))
        reads[name], refs[name] = rs, ref
    fa, wfn = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model")
    io.write_fasta(fa, contigs)
    np.save(wfn + ".c3rw.npy", synth.random_weights(30, seed=5))    # (the sample of tests/test_gpu_haplotag_bam.py's driver case: the built-in phasing tags reads of both haplotypes here)
    np.save(wfn + "18.c3rw.npy", synth.random_weights(18, seed=5))
    bam_fn = os.path.join(tmp, "plain.bam")
    bam.write_bam(bam_fn, [(n, len(r)) for n, r in contigs], reads)
    bamio.index_build(bam_fn)
    for out, extra in (("base", []), ("flag", ["--hap_junctions"])):
        argv = ["--bam_fn", bam_fn, "--ref_fn", fa, "--output_dir", os.path.join(tmp, out), "--pileup_model_path", wfn + "18", "--phased_pileup_model_path", wfn,
                "--chunk_num", "3", "--min_coverage", "2", "--enable_phasing_model", "--phasing", "builtin"] + extra
        assert call_sample.Run(call_sample.build_parser().parse_args(argv), log=lambda m: None) == 0
    return dict(tmp=tmp, bam=bam_fn, fa=fa, reads=reads, refs=refs)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_call_sample_with_the_flag_equals_the_step_by_hand_and_the_restatement(called, tmp_path):
    from clair3_rna_amd import phasedvcf
    base, flag = os.path.join(called["tmp"], "base"), os.path.join(called["tmp"], "flag")
    tsv = os.path.join(flag, "output_enable_phasing_hap_junctions.tsv")
    # without the flag: the file set of the parent; with it: one file more and no byte different
    assert not [f for f in _files(base) if "hap_junctions" in f]
    assert _files(flag) == sorted(_files(base) + ["output_enable_phasing_hap_junctions.tsv"])
    for f in _files(base):
        if f.endswith((".vcf.gz", ".tbi")):
            # (phase_vcf's per-contig files go through Python's gzip, which stamps the time into the header: those are compared inflated)
            both = [(gzip.open if f.startswith("tmp") and f.endswith(".gz") else open)(os.path.join(d, f), "rb").read() for d in (base, flag)]
            assert both[0] == both[1], f
    # the step by hand, on the directory the built-in phasing left
    per = os.path.join(base, "tmp", "phased_output", "phased_vcf")
    by_hand = str(tmp_path / "by_hand.tsv")
    hap_junctions.Run(hap_junctions.build_parser().parse_args(["--bam_fn", called["bam"], "--phased_vcf_fn", per, "--ref_fn", called["fa"], "--output_fn", by_hand]), log=lambda m: None)
    assert open(tsv).read() == open(by_hand).read()
    # the restatement's prediction from the phased VCFs
    want, n_sites = [], 0
    for ctg in ("chr1", "chr2"):
        table = phasedvcf.contig_sites(per, ctg)
        n_sites += len(table)
        want += HJ.lines(ctg, HJ.counts(called["reads"][ctg], table), called["refs"][ctg])
    got = open(tsv).read().split("\n")
    assert got[0] == hap_junctions.HEADER and got[1:-1] == want
    tagged = sum(int(l.split("\t")[8]) + int(l.split("\t")[9]) for l in want if l.split("\t")[7] != ".")
    print("phased sites %d, junction reads counted on a haplotype %d" % (n_sites, tagged))
    assert n_sites >= 4 and tagged >= 20                      # the comparison is about something
