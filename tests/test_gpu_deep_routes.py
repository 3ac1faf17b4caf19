"""The adversarial-CIGAR parity tests through the deep-span kernels.

Which kernel builds a span depends only on the records in its range: k_fused_tiles below 2048 (DEEP_MIN_RECORDS), k_fused_deep from there,
k_deep_walk / k_deep_alleles ahead of it from 8192 (SPLIT_MIN_RECORDS) once the context has its pool.  How a span's indel alleles are counted
(I1 / i1 / D1 / d1) depends on its events: the LDS store up to 3072 (DEEP_EV_LDS), the same scheme in global buckets up to 9216, a CAS hash
table beyond, the table of k_deep_alleles for a giant span; the events come from the workgroup's arrival-order buffer up to 49152
(DEEP_EVG_CAP) and from a second walk otherwise.  k_fused_tiles keeps 192 events in LDS (18 channels), counts all pairs in global scratch up
to 1024 (EV_HASH_MIN) and hashes beyond.  tests/c/layout_check.hip ties every one of these numbers to its constant.

The random-CIGAR cases are 25-90 reads, so in tests/test_gpu_fuzz.py they meet k_fused_tiles alone.  Here
  * the same generator runs with every span FORCED through one deep route (environment variables that the library reads at every scan), and
  * "allele zoo" read sets (tests/helpers.py) sized for each bracket above run at the natural thresholds and on the forced routes,
and every test asserts through Engine.scan_counts() that the scan took the route it names: a mis-spelt variable fails, it does not pass quietly.
All cases of one test run one after the other in one context: nothing of a scan may leak into the next (the giant spans' allele table must be
all-zero between scans; the event pool and the per-workgroup buffers are never cleared)."""
import pytest

import numpy as np

from tests import helpers as H

pytestmark = pytest.mark.gpu

ROUTES, ROUTE_VARS, _set_route, route_check, _most_aligned = H.ROUTES, H.ROUTE_VARS, H._set_route, H.route_check, H._most_aligned          # shared with tests/test_gpu_coords.py (tests/helpers.py)
FORCED = ["deep_walk_twice", "deep_event_buffer", "giant_slices"]
SLICE, MAX_SLICES, SLOTS = H.SLICE, H.MAX_SLICES, H.SLOTS         # C3R_SPLIT_SLICE of the route; GIANT_MAX_HELP; GIANT_SLOTS

_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.fixture
def routed(monkeypatch):
    """routed(route) -> the route's engine: a context of its own, created after the route's variables are set, closed at the end of the module."""
    return H.routed_get(monkeypatch, _engines)


def _swept(route, seen):
    """The sweep as a whole went where it says (scan by scan is asserted in route_check)."""
    assert seen["scans"] >= 40 and seen["listed"] >= 40, seen
    if route == "giant_slices":
        assert seen["slices"] > seen["giant"] > 0, seen        # some case of the sweep has a span above 64 records


# ---- the fuzz sweep per route: 40 seeds each, seed bases (600000 ..) that neither tests/test_gpu_fuzz.py, its soaks nor tests/golden/diff_tensor.py draw.  The floors are conditions, not
# measurements: beside each stands what the ORACLE alone gives for these seeds (computed without a GPU).
SEEDS = range(40)


@pytest.mark.parametrize("k, kw", enumerate([dict(), dict(channels=30), dict(snp_min_af=0.0), dict(min_mq=0, min_coverage=1)]), ids=["plain", "ch30", "af0", "mq0_cov1"])
@pytest.mark.parametrize("route", FORCED)
def test_random_cigars_match_the_oracle(routed, route, k, kw):
    eng, seen = routed(route), {}
    n_cases, n_lines = H.fuzz_match_oracle(eng, SEEDS, kw, case_base=600000 + 1000 * k, on_scan=route_check(route, seen))
    assert n_cases == 40 and n_lines > 4000, n_lines          # oracle: 5901, 5957, 6235, 6828 lines
    _swept(route, seen)


@pytest.mark.parametrize("kw", [dict(), dict(channels=30)], ids=["plain", "ch30"])
@pytest.mark.parametrize("route", FORCED)
def test_random_cigars_with_the_samtools_1_11_printer(routed, route, kw):
    eng, seen = routed(route), {}
    n_lines, n_both, n_padded, n_refused = H.fuzz_samtools_1_11(eng, SEEDS, kw, case_base=610000 + 1000 * len(kw), on_scan=route_check(route, seen))
    # oracle: 5900 / 5905 lines, 98 / 99 columns with an insertion and a deletion, 49 / 36 padded alleles; no case of these seed bases has a run of
    # I and P ops above 64 characters (counted from the CIGAR strings), so the pad table's cap of 5 % of the cases + 1 leaves room
    assert n_lines > 4000 and n_both > 70 and n_padded > 25 and n_refused <= 0.05 * 40 + 1, (n_lines, n_both, n_padded, n_refused)
    _swept(route, seen)


@pytest.mark.parametrize("mode", ["lbed", "cbed", "both_beds", "subregion", "deep"])
@pytest.mark.parametrize("route", FORCED)
def test_random_cigars_with_filters_and_regions(routed, route, mode):
    eng, seen = routed(route), {}
    n_lines = H.fuzz_filters_and_regions(eng, SEEDS, mode, case_base=620000, rng_base=621000, head_tail=0, on_scan=route_check(route, seen))
    floor = dict(lbed=350, cbed=800, both_beds=100, subregion=2000, deep=4500)[mode]          # oracle: 1262, 1766, 250, 3013, 6608 lines
    assert n_lines > floor, (mode, n_lines)
    _swept(route, seen)


@pytest.mark.parametrize("compat", [0, 1])
@pytest.mark.parametrize("route", FORCED)
def test_random_cigars_decode_rows_cpp_equals_python_and_regions(routed, route, compat):
    eng, seen = routed(route), {}
    n_rows, kinds = H.fuzz_decode_rows_and_regions(eng, SEEDS, compat, case_base=630000, rng_base=631000, on_scan=route_check(route, seen))
    # oracle (its own forward pass and the Python decoder): 5869 rows with either printer, genotypes 0/0, 0/1, 1/1 and 1/2
    assert n_rows > 4000 and {"0/0", "0/1", "1/1"} <= kinds, (n_rows, kinds)
    _swept(route, seen)


@pytest.mark.parametrize("channels", [18, 30])
@pytest.mark.parametrize("route", FORCED)
def test_mpileup_depth_cap(routed, route, channels):
    eng, seen = routed(route), {}
    n_dropped_cases = H.fuzz_depth_cap(eng, SEEDS, channels, case_base=640000, rng_base=641000, splice_padding=0, head_tail=0,
                                       on_scan=route_check(route, seen))
    assert n_dropped_cases > 18, n_dropped_cases             # oracle: the cap changes the lines of 25 (18 channels) and 26 of the 40 cases
    _swept(route, seen)


# ---- threshold cases: the forced sweep has tiny spans (a median of 35 indel events per case), so it never leaves the LDS store and rarely
# reaches 32 slices.  One allele-zoo read set per bracket; before the engine runs, the oracle's columns and the CIGARs say that the case lies
# in its bracket (H.span_bounds: what the largest span must and may hold).
DEEP, GIANT, EV_LDS, LEAD_CAP, EVG_CAP, TILE_LDS, HASH_MIN = 2048, 8192, 3072, 9216, 49152, 192, 1024
#        reads, events per read, share of random-CIGAR reads
CASES = dict(a=(1500, 1, 0.10),          # deep, not giant; the LDS store
             b=(580, 6, 0.03),           # deep, not giant; the global buckets with first-of-allele slots
             c=(10500, 1, 0.10),         # the CAS hash table (giant by its records at the natural thresholds)
             d=(9000, 6, 0.02),          # beyond the arrival-order buffer
             h1=(600, 1, 0.10))          # k_fused_tiles: beyond its LDS store, all pairs in global scratch  (h2: case a with the deep kernel off)


def in_bracket(name, b):
    if name == "a":
        return DEEP <= b["rec_lo"] and b["rec_hi"] < GIANT and 0 < b["ev_lo"] and b["ev_hi"] <= EV_LDS
    if name == "f":
        return SLICE * MAX_SLICES < b["rec_lo"]
    if name == "h2":
        return HASH_MIN < b["ev_lo"]
    if name == "b":
        return DEEP <= b["rec_lo"] and b["rec_hi"] < GIANT and EV_LDS < b["ev_lo"] and b["ev_hi"] <= LEAD_CAP
    if name in ("c", "e"):
        return GIANT <= b["rec_lo"] and LEAD_CAP < b["ev_lo"] and b["ev_hi"] <= EVG_CAP
    if name == "d":
        return GIANT <= b["rec_lo"] and EVG_CAP < b["ev_lo"]
    if name == "h1":
        return b["rec_hi"] < DEEP and TILE_LDS < b["ev_lo"] and b["ev_hi"] <= HASH_MIN
    raise KeyError(name)


_zoo = {}


def zoo_case(name, channels, compat):
    """(ref, ReadSet, oracle result with the depth cap off, span bounds) of a bracket's case — built once, shared by the routes, never changed."""
    from clair3_rna_amd.reads import ReadSet
    reads = dict(f="a", e="c", h2="a").get(name, name)
    if (reads, compat) not in _zoo:
        n, k, share = CASES[reads]
        ref, recs = H.allele_zoo(n, 1000 + ord(reads[0]), compat=compat, events_per_read=k, random_share=share)
        rs = ReadSet.from_records(recs)
        plain = H.oracle_chunk(rs, ref, 1, 1, len(ref), channels=18, min_coverage=2, max_depth=0, mpileup_compat=compat)
        _zoo[(reads, compat)] = (ref, recs, rs, H.span_bounds(recs, plain["rows"], ref))
    ref, recs, rs, bounds = _zoo[(reads, compat)]
    if (reads, compat, channels) not in _zoo:
        _zoo[(reads, compat, channels)] = H.oracle_chunk(rs, ref, 1, 1, len(ref), channels=channels, min_coverage=2, max_depth=0, mpileup_compat=compat)
    return ref, recs, rs, _zoo[(reads, compat, channels)], bounds


def _multiplicities(raw, channels):
    idx = [5, 7, 14, 16]           # I1, D1, i1, d1 (include/c3r_types.h; the haplotype channels lie behind the first 18)
    return int(raw[:, :, idx].max()) if len(raw) else 0


def run_zoo(eng, route, name, channels, compat, check=None):
    from clair3_rna_amd import capi
    ref, recs, rs, exp, bounds = zoo_case(name, channels, compat)
    assert in_bracket(name, bounds), (name, bounds)          # from the oracle and the CIGARs, before the engine runs
    assert H.long_insertions_tell(recs), name                # and a comparison that stops at the 16 bases of the key would show in I1 / i1
    eng.params = capi.default_params()
    eng.set_bed(0, None); eng.set_bed(1, None)
    eng.set_params(channels=channels, min_coverage=2, max_depth=0, mpileup_compat=compat)
    got = H.engine_chunk(eng, rs, ref, 1, 1, len(ref))
    route_check(route)(eng, exp)
    c = eng.scan_counts()
    if check is not None:
        check(c, bounds)
    assert got["lines"] == exp["lines"] and len(exp["lines"]) > 20, (route, name, c, H.first_diff(got["lines"], exp["lines"]))
    assert np.array_equal(got["X"], exp["X"]), (route, name, c)
    assert _multiplicities(got["raw"], channels) > 1, (route, name)          # the multiplicities these routes exist to compute are in play
    eng.params = capi.default_params()
    eng.set_params()
    return c, got, exp


def _default_counts(name):
    def check(c, b):
        if name in ("a", "b"):
            assert c["deep"] >= 1 and c["giant"] == 0, (name, c)
        else:
            assert c["deep"] >= 1 and c["giant"] >= 1, (name, c)
    return check


@pytest.mark.parametrize("compat", [0, 1])
@pytest.mark.parametrize("channels", [18, 30])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
@pytest.mark.parametrize("route", ["default", "deep_walk_twice", "deep_event_buffer"])
def test_event_brackets_of_the_deep_kernel(routed, route, name, channels, compat):
    """(a) at most 3072 events, (b) 3073-9216, (c) above 9216, (d) above 49152 in one span: at the natural thresholds (a, b: deep, not giant; c, d:
    giant by their records) and with k_fused_deep forced to count them itself, without and with the arrival-order buffer."""
    run_zoo(routed(route), route, name, channels, compat, check=_default_counts(name) if route == "default" else None)


@pytest.mark.parametrize("compat", [0, 1])
@pytest.mark.parametrize("channels", [18, 30])
@pytest.mark.parametrize("name", ["c", "d", "f"])
def test_event_brackets_through_the_slices(routed, name, channels, compat):
    """(c), (d): the hash-table brackets with the alleles from k_deep_alleles' table; (f): a span above 32 x 64 records — the slices are capped at
    32 and grow instead."""
    def check(c, b):
        assert c["giant"] <= SLOTS and c["giant"] < c["slices"] <= MAX_SLICES * c["giant"], c
        assert c["slices"] >= MAX_SLICES, c                  # (the largest span alone has more than 32 x 64 records)
    run_zoo(routed("giant_slices"), "giant_slices", name, channels, compat, check=check)


@pytest.mark.parametrize("compat", [0, 1])
@pytest.mark.parametrize("channels", [18, 30])
def test_a_giant_span_at_the_natural_thresholds_scanned_twice(routed, channels, compat):
    """(e) a fresh context meets its first giant span without a pool — k_fused_deep walks it — and allocates one; the second scan of the same
    reads lists slices of 4096 records for k_deep_walk.  Both equal the oracle."""
    eng = routed("default", fresh=True)
    try:
        c1, g1, exp = run_zoo(eng, "default", "e", channels, compat)
        assert c1["giant"] >= 1 and c1["slices"] == 0, c1
        c2, g2, _ = run_zoo(eng, "default", "e", channels, compat)
        assert c2["giant"] == c1["giant"] and c2["slices"] > c2["giant"], (c1, c2)
        assert np.array_equal(g1["raw"], g2["raw"]) and g1["tokens"].tobytes() == g2["tokens"].tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("compat", [0, 1])
@pytest.mark.parametrize("channels", [18, 30])
def test_more_giant_spans_than_slots(routed, channels, compat):
    """(g) one small case at 300 offsets 1000 bp apart, every span giant: the first 256 take the slots and are cut into slices, the others are
    walked by their own workgroup."""
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    key = ("g", compat)
    if key not in _zoo:
        # 30 zoo reads and three plain ones that give the locus its 33 contiguous rows: more than 64 and at most 128 records per copy
        ref0, one = H.allele_zoo(30, 77, compat=compat, random_share=0.0)
        one = sorted(one + [dict(pos=265, cigar="70M", seq=ref0[265:335], flag=16 * (q % 2), mapq=60, hp=q) for q in range(3)], key=lambda r: r["pos"])
        unit = -(-len(ref0) // 1000) * 1000
        ref1 = ref0 + ref0[:unit - len(ref0)]
        recs = [dict(r, pos=r["pos"] + k * unit) for k in range(300) for r in one]
        rs = ReadSet.from_records(recs)
        per_copy = H.span_bounds(one, H.oracle_chunk(ReadSet.from_records(one), ref0, 1, 1, len(ref0), min_coverage=2, max_depth=0, mpileup_compat=compat)["rows"], ref0)
        _zoo[key] = (ref1 * 300, rs, per_copy, unit)
    ref, rs, per_copy, unit = _zoo[key]
    if (key, channels) not in _zoo:
        _zoo[(key, channels)] = H.oracle_chunk(rs, ref, 1, 1, len(ref), channels=channels, min_coverage=2, max_depth=0, mpileup_compat=compat)
    exp = _zoo[(key, channels)]
    # every copy has lines of its own, and no span (224 positions) reaches from one copy into the next: more than 256 spans are listed
    assert len(set((int(l.split("\t")[1]) - 1) // unit for l in exp["lines"])) == 300 and SLICE < per_copy["rec_lo"] and per_copy["rec_hi"] <= 2 * SLICE, per_copy
    eng = routed("giant_slices")
    eng.params = capi.default_params()
    eng.set_params(channels=channels, min_coverage=2, max_depth=0, mpileup_compat=compat)
    got = H.engine_chunk(eng, rs, ref, 1, 1, len(ref))
    c = eng.scan_counts()
    assert c["listed"] >= 300 and c["giant"] == c["listed"] == c["deep"], c
    # the first 256 only: a sliced span has one or two slices (at most 128 records per copy); had all been sliced, each of the 300 copies' main
    # spans (more than 64 records) would have brought two
    assert SLOTS <= c["slices"] <= 2 * SLOTS < 2 * 300, (c, per_copy)
    assert got["lines"] == exp["lines"], (c, H.first_diff(got["lines"], exp["lines"]))
    assert np.array_equal(got["X"], exp["X"])
    assert _multiplicities(got["raw"], channels) > 1
    eng.params = capi.default_params()
    eng.set_params()


@pytest.mark.parametrize("compat", [0, 1])
@pytest.mark.parametrize("channels", [18, 30])
@pytest.mark.parametrize("name", ["h1", "h2"])
def test_event_brackets_of_the_tile_kernel(routed, name, channels, compat):
    """(h) k_fused_tiles with the deep kernel off: 193-1024 events (beyond its LDS store of 192 at 18 channels, which 30 channels do not have:
    global scratch, all pairs) and above 1024 (the hash table)."""
    route = "default" if name == "h1" else "tiles_only"          # (h1 stays below 2048 records by itself)

    def check(c, b):
        assert c["listed"] >= 1 and c["deep"] == 0 and c["giant"] == 0, c
    run_zoo(routed(route), route, name, channels, compat, check=check)


@pytest.mark.parametrize("channels", [18, 30])
@pytest.mark.parametrize("route", ["default", "deep_walk_twice", "deep_event_buffer", "giant_slices"])
def test_hash_table_bracket_under_a_depth_cap_in_two_regions(routed, route, channels):
    """(c) with mpileup's cap at 150 and two regions that overlap on the hot locus: one scan of both equals two successive scans equals the
    oracle region by region (a read may survive in one region and not in the other; the masks are per region)."""
    from clair3_rna_amd import capi
    ref, recs, rs, _, bounds = zoo_case("c", channels, 0)
    assert in_bracket("c", bounds), bounds
    regions = [(150, 320), (290, 470)]
    key = ("c-capped", channels)
    if key not in _zoo:
        _zoo[key] = [H.oracle_chunk(rs, ref, 1, a, b, channels=channels, min_coverage=2, max_depth=150) for a, b in regions]
        _zoo[key + ("off",)] = [H.oracle_chunk(rs, ref, 1, a, b, channels=channels, min_coverage=2, max_depth=0) for a, b in regions]
    e1, e2 = _zoo[key]
    assert len(e1["lines"]) > 20 and len(e2["lines"]) > 20 and e1["lines"] != _zoo[key + ("off",)][0]["lines"] and e2["lines"] != _zoo[key + ("off",)][1]["lines"]          # the cap bites in both regions
    eng = routed(route)
    check = route_check(route)
    eng.params = capi.default_params()
    eng.set_bed(0, None); eng.set_bed(1, None)
    eng.set_params(channels=channels, min_coverage=2, max_depth=150)
    eng.load_reads(rs)
    eng.set_reference(1, ref)
    eng.begin_batch()
    eng.scan(*regions[0]); check(eng, e1)
    eng.scan(*regions[1]); check(eng, e2)
    eng.end_batch()
    X1, S1, T1 = eng.tensors(), eng.sites(), eng.tokens()
    eng.begin_batch(); eng.scan_regions(regions); eng.end_batch()
    check(eng, [e1, e2])
    assert np.array_equal(X1, eng.tensors()) and S1.tobytes() == eng.sites().tobytes() and T1.tobytes() == eng.tokens().tobytes()
    assert [int(l.split("\t")[1]) for l in e1["lines"] + e2["lines"]] == S1["pos"].tolist()
    assert np.array_equal(X1, np.concatenate([e1["X"], e2["X"]]))
    eng.params = capi.default_params()
    eng.set_params()
