"""c3r_load_reads at the limits of its own machinery (csrc/reads_kernels.hpp: k_prep<false>, k_prefmax_bins, k_bin_scan, k_prep<true>;
c3r_lib.hip: prepare_tables).  The parity and fuzz suites enter through the load with 25-90 reads on a few hundred bases, or with realistic
contigs whose reads are short and dense; these read sets are sized for the branches that such inputs never reach:

  * more distinct bins in one workgroup than its LDS hash has slots (HB = 1024, HB_PROBES = 16): records counted and placed through the
    global counter directly, in both passes;
  * a read that ends beyond the bin table's first guess (the last read's start plus 2 Mb): the first pass runs twice, on counters that the
    clamped first attempt left behind; the far region's first read is found through prefix maxima carried across blocks of 1024 reads;
  * reads that end on the edge of a 256-position coarse bin — the device's, counted from the first read's bin, and the host's, absolute —
    where LoadStats::max_cover decides whether mpileup's depth cap is looked at at all.

All of these are integer tables: the oracle restates none of the bin, hash or look-back machinery, and every comparison is bit-exact.  Which
branch a case reaches is asserted before the engine runs, from the reads' positions (tests/helpers.py; tests/test_load_edges_ref.py holds
the same conditions without a GPU; tests/c/layout_check.hip ties each number to its constant), and after it through the profiler's
statistics where the library counts (launches of k_prep_count; k_prep_recount_workgroups).  The recount path of the second pass WITHOUT hash
exhaustion is tests/test_gpu_load.py::test_long_reads_far_apart_take_the_recount_path_of_the_second_pass."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


def _reset(eng, **prm):
    from clair3_rna_amd import capi
    eng.params = capi.default_params()
    eng.set_bed(0, None); eng.set_bed(1, None)
    eng.set_params(**prm)


def _readset(recs):
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records(recs)


def _scanned(eng, rs, ref):
    """dict(lines, X, sites, tokens) of the candidates the context holds (one scan, or one scan_regions of a batch), reference from 1."""
    from clair3_rna_amd import altinfo
    raw, X = eng.tensors(rescaled=False), eng.tensors(rescaled=True)
    sites, toks = eng.sites(), eng.tokens()
    return dict(lines=altinfo.format_lines(H.CTG, sites, raw, toks, rs, ref, 1), X=X, sites=sites, tokens=toks)


def _same(got, exp, what):
    assert got["lines"] == exp["lines"], (what, H.first_diff(got["lines"], exp["lines"]))
    assert np.array_equal(got["X"], exp["X"]), what


def _loaded_with_stats(eng, rs):
    """load_reads under the profiler: the launches of the load's kernels, by name."""
    eng.set_profiling(True); eng.reset_kernel_stats()
    try:
        eng.load_reads(rs)
        ks = eng.kernel_stats()
    finally:
        eng.set_profiling(False)
    return {k: v["launches"] for k, v in ks.items()}


_small = {}


def _nothing_leaked(eng):
    """Right after a case, in the same context: a small ordinary contig gives, byte for byte, the sites, tokens and tensors of a fresh context.
    The load leaves its counters "all zero" and never clears them again: a count left behind by the case before would show here."""
    from clair3_rna_amd import capi, synth
    if not _small:
        ref, rs, _ = synth.small_case(seed=11, ref_len=60000, n_genes=10, depth=25)
        fresh = capi.Engine(0)
        try:
            fresh.set_params()
            fresh.load_reads(rs); fresh.set_reference(1, ref)
            n = fresh.scan(1, len(ref))
            _small.update(ref=ref, rs=rs, want=(n, fresh.sites().tobytes(), fresh.tokens().tobytes(), fresh.tensors().tobytes()))
        finally:
            fresh.close()
        assert _small["want"][0] > 50
    _reset(eng)
    eng.load_reads(_small["rs"]); eng.set_reference(1, _small["ref"])
    n = eng.scan(1, len(_small["ref"]))
    assert (n, eng.sites().tobytes(), eng.tokens().tobytes(), eng.tensors().tobytes()) == _small["want"]


# ---- 1. hash exhaustion -------------------------------------------------------------------------------------------------------------
_hash = {}


def _hash_case():
    if not _hash:
        ref, recs = H.hash_exhaustion_case()
        _hash.update(ref=ref, recs=recs, rs=_readset(recs))
    return _hash["ref"], _hash["recs"], _hash["rs"]


def _hash_conditions(recs):
    """From positions alone: in every workgroup of 16 reads, more bins lie wholly inside a read than the hash has slots.  Records are cut every
    30 positions, so each of those bins holds a record start: they cannot all find a slot (there is no counter for the direct path, and none
    is wanted: this is the proof that it ran)."""
    whole = H.workgroup_whole_bins(recs)
    assert len(whole) == 3 and all(w > H.HB for w in whole), whole          # 1368 per workgroup
    return len(whole)


@pytest.mark.parametrize("channels", [18, 30])
def test_more_bins_in_a_workgroup_than_hash_slots(eng, channels):
    ref, recs, rs = _hash_case()
    n_wg = _hash_conditions(recs)
    exp = H.oracle_chunk(rs, ref, 1, 1, len(ref), channels=channels, min_coverage=2)
    assert len(exp["lines"]) > 1200 and all(H.reads_with_a_line(recs, exp["lines"]))          # oracle: 1368 lines, in every read of every workgroup
    _reset(eng, channels=channels, min_coverage=2)
    ks = _loaded_with_stats(eng, rs)
    assert ks.get("k_prep_count") == 1 and ks.get("k_prep_write") == 1, ks
    assert ks.get("k_prep_recount_workgroups") == n_wg, ks                  # every workgroup overflows its slab as well
    eng.set_reference(1, ref)
    assert eng.scan(1, len(ref)) == len(exp["lines"])
    _same(_scanned(eng, rs, ref), exp, channels)
    _nothing_leaked(eng)


def test_more_bins_than_hash_slots_scanned_in_regions_that_cut_through_loci(eng):
    ref, recs, rs = _hash_case()
    _hash_conditions(recs)
    regions = H.hash_exhaustion_regions(len(ref))
    exps = [H.oracle_chunk(rs, ref, 1, a, b, min_coverage=2) for a, b in regions]
    assert all(len(e["lines"]) > 50 for e in exps)                          # oracle: 1368 lines in all, 86 in the last region
    _reset(eng, min_coverage=2)
    eng.load_reads(rs); eng.set_reference(1, ref)
    eng.begin_batch()
    n = eng.scan_regions(regions)
    eng.end_batch()
    assert n == sum(len(e["lines"]) for e in exps)
    got = _scanned(eng, rs, ref)
    _same(got, dict(lines=[l for e in exps for l in e["lines"]], X=np.concatenate([e["X"] for e in exps])), regions)
    tok = got["tokens"].tobytes()
    eng.begin_batch()                                                       # the same as successive scans
    for a, b in regions:
        eng.scan(a, b)
    eng.end_batch()
    assert np.array_equal(got["X"], eng.tensors()) and got["sites"].tobytes() == eng.sites().tobytes() and tok == eng.tokens().tobytes()
    _reset(eng)


# ---- 3. regrowth of the bin table ---------------------------------------------------------------------------------------------------
_regrow = {}


def _regrow_case():
    if not _regrow:
        ref, recs, near, far = H.regrowth_case()
        rs = _readset(recs)
        assert H.readset_end(rs) > recs[-1]["pos"] + H.BIN_END_GUESS and len(recs) - 4 > 2 * H.PM_BLK          # from positions alone, before the engine runs
        _regrow.update(ref=ref, recs=recs, rs=rs, near=near, far=far)
    return _regrow


def _regrow_oracle(name, **kw):
    c = _regrow_case()
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _regrow:
        a, b = c[name]
        _regrow[key] = H.oracle_chunk(c["rs"], c["ref"], 1, a, b, min_coverage=2, head_tail=True, **kw)
    return _regrow[key]


def _regrow_scan(eng, name, **kw):
    c = _regrow_case()
    exp = _regrow_oracle(name, **kw)
    a, b = c[name]
    assert eng.scan(a, b) == len(exp["lines"]), (name, kw)
    _same(_scanned(eng, c["rs"], c["ref"]), exp, (name, kw))
    return exp


def test_a_read_beyond_the_first_guess_regrows_the_bin_table(eng):
    c = _regrow_case()
    _reset(eng, min_coverage=2, head_tail=1)
    ks = _loaded_with_stats(eng, c["rs"])
    assert ks.get("k_prep_count") == 2 and ks.get("k_prep_write") == 1, ks   # the regrowth: the first pass ran twice
    eng.set_reference(1, c["ref"])
    assert len(_regrow_scan(eng, "near")["lines"]) > 1400                   # oracle: 1625 lines
    far = _regrow_scan(eng, "far")
    assert len(far["lines"]) >= 4                                           # oracle: 4 lines, all owed to the bridging reads
    # under a cap of 2 the second bridging read on position 1020 is discarded; the region's first read and the cap's entry list are both
    # upper bounds into prefix maxima that the bridging reads hold across three blocks of k_prefmax_bins
    eng.set_params(max_depth=2)
    capped = _regrow_scan(eng, "far", max_depth=2)
    assert capped["lines"] != far["lines"] and len(capped["lines"]) >= 4
    _regrow_scan(eng, "near", max_depth=2)
    _nothing_leaked(eng)


def test_new_filters_drop_and_bring_back_the_regrowth(eng):
    """The bridging reads have mapq 7.  min_mq = 10 re-derives the tables without them — one first pass, no line in the far region; min_mq = 5
    brings the regrowth back."""
    c = _regrow_case()
    _reset(eng, min_coverage=2, head_tail=1)
    eng.load_reads(c["rs"]); eng.set_reference(1, c["ref"])
    _regrow_scan(eng, "far")
    for min_mq, first_passes in ((10, 1), (5, 2), (10, 1)):
        eng.set_profiling(True); eng.reset_kernel_stats()
        try:
            eng.set_params(min_mq=min_mq)
            ks = {k: v["launches"] for k, v in eng.kernel_stats().items()}
        finally:
            eng.set_profiling(False)
        assert ks.get("k_prep_count") == first_passes and ks.get("k_prep_write") == 1, (min_mq, ks)
        kw = dict(min_mq=10) if min_mq == 10 else {}
        far = _regrow_scan(eng, "far", **kw)
        assert (len(far["lines"]) == 0) == (min_mq == 10)
        assert len(_regrow_scan(eng, "near", **kw)["lines"]) > 1400          # oracle: 1621 lines without the bridging reads, 1625 with them
    _nothing_leaked(eng)


# ---- 4. the depth cap's gate on coarse-bin edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("far", [False, True], ids=["near", "with_far_read"])
@pytest.mark.parametrize("kind", H.GATE_EDGES)
@pytest.mark.parametrize("first", H.GATE_FIRSTS)
def test_depth_cap_gate_with_reads_that_end_on_a_coarse_bin_edge(eng, first, kind, far):
    """K = 30 reads end on (one before, one past) the position on which M = 10 reads start, and that position is the edge of a coarse bin.  The
    cap K + 2 bites exactly when the enders are still in htslib's read list (tests/test_load_edges_ref.py); a max_cover that left them out
    would be 11, below the cap, and the engine would return the uncapped lines."""
    for d in H.GATE_DS:
        ref, recs, last = H.gate_case(first, kind, d, far)
        rs = _readset(recs)
        exps = [H.oracle_chunk(rs, ref, 1, 1, last, min_coverage=2, max_depth=cap) for cap in H.GATE_CAPS]
        assert (exps[0]["lines"] != exps[2]["lines"]) == (d >= 0) and exps[1]["lines"] == exps[2]["lines"] and len(exps[2]["lines"]) >= 2
        for cap, exp in zip(H.GATE_CAPS, exps):
            _reset(eng, min_coverage=2, max_depth=cap)
            got = H.engine_chunk(eng, rs, ref, 1, 1, last)
            _same(got, exp, (first, kind, d, cap, far))
    _nothing_leaked(eng)
