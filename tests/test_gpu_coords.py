"""Parity at chromosome-scale coordinates and at the end of the accepted domain (include/c3r.h, "coordinates").

Every other parity test scans contigs of a few hundred bases from position 1: the first tile starts at p0 = 0, on a bin edge and on a coarse-bin
edge at once, and no position exceeds a few thousand.  Here the same random-CIGAR cases, hand-made reads and phasing cases are TRANSLATED
(tests/helpers.py: place, shift_readset, shift_sites) to
  * K_CHR1  — the case's last reference base on the last base of GRCh38 chr1 (248,956,422),
  * K_2_28  — the centre of its pile on 2^28,
  * K_TOP   — its scan ending on the last accepted ctg_end (C3R_CTG_END_MAX), and, for the phasing kernels, its last read END on INT32_MAX,
and, at K_LOW = 1000 and K_CHR1, swept through the phases of reads against bins (shift + 0, 1, 31) and of tile starts against reads, bins and
coarse bins (`front` 0, 1, 223, 255 uncovered positions before the case).  Engine and oracle always get the same inputs; tests/test_coords_ref.py
shows on the CPU, for exactly these seeds and translations, that the oracle and the phasing restatements do not depend on the translation, so
engine(K) == oracle(K) == shift(oracle(0)), and the last term is the one pinned to the golden vectors.

The specs below (seed bases, parameters, seeds) are plain data that tests/test_coords_ref.py imports.  The seed bases (900000 ..) are drawn
neither by tests/test_gpu_fuzz.py, tests/test_gpu_deep_routes.py, their soaks (bases below 140000) nor by tests/golden/diff_tensor.py (300000 ..).
The floors are conditions, not measurements: beside each stands what the ORACLE alone gives for these seeds (tests/test_coords_ref.py asserts it)."""
import random

import numpy as np
import pytest

from tests import helpers as H
from tests import hapalleleref as HA
from tests import hapcountref as HC
from tests import hapref
from tests import phasemergeref as M
from tests import phaseref as P

pytestmark = pytest.mark.gpu

INT32_MAX, CTG_END_MAX = H.INT32_MAX, H.CTG_END_MAX
SEEDS = range(24)
MAGNITUDES = dict(chr1=H.K_CHR1, p2_28=H.K_2_28, top=H.K_TOP)

# ---- the tensor build, every scan path: (helper, its argument, seed base, floor on the lines, the oracle's lines).  No case of these seed bases has a
# run of I and P ops above 64 characters (counted from the CIGAR strings: tests/test_coords_ref.py), so the samtools 1.11 printer refuses none.
BUILD = dict(
    plain=("match", dict(), 900000, 2400, 3553),
    ch30=("match", dict(channels=30), 901000, 2300, 3416),
    head_tail=("match", dict(head_tail=1), 902000, 2600, 3766),          # (the column store)
    splice=("match", dict(splice_padding=1), 903000, 2600, 3756),        # (the column store)
    samtools=("samtools", dict(), 904000, 2300, 3399),
    both_beds=("filters", "both_beds", 905000, 130, 196),
    sites=("filters", "sites", 905000, 110, 160),                        # (genotyping mode: the column store)
    deep=("filters", "deep", 905000, 2900, 4207),
)
RNG_BASE = 906000
# ---- the same through the deep routes: (parameters, seed base, floor, oracle)
ROUTES = ["default", "deep_walk_twice", "deep_event_buffer", "giant_slices"]
ROUTED = dict(plain=(dict(), 910000, 2600, 3747), ch30=(dict(channels=30), 911000, 2300, 3311))
# ---- the phase sweep: 12 combinations of (phi, front), four cases each, 48 different cases per test
SWEEP = dict(fused=(dict(), None, 920000, 4600, 6678), column_store=(dict(head_tail=1), None, 921000, 5000, 7226),
             deep_event_buffer=(dict(), "deep_event_buffer", 922000, 5100, 7326))
SWEEP_K = dict(low=H.K_LOW, chr1=H.K_CHR1)
GRID = [(phi, front) for phi in H.PHIS for front in H.FRONTS]
# ---- rows: (seed base, rng base, floor on the rows, oracle)
ROWS = (930000, 931000, 2400, 3468)

_engines = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.fixture
def routed(monkeypatch):
    """routed(route) -> the route's engine, one per route for the module (tests/helpers.py: routed_get)."""
    return H.routed_get(monkeypatch, _engines)


def run_build(eng, name, shift, seeds=SEEDS, front=0, on_scan=None):
    """One BUILD spec through the engine; returns the lines seen."""
    kind, arg, base, _, _ = BUILD[name]
    if kind == "match":
        n_cases, n_lines = H.fuzz_match_oracle(eng, seeds, arg, case_base=base, on_scan=on_scan, shift=shift, front=front)
        assert n_cases == len(seeds)
        return n_lines
    if kind == "samtools":
        n_lines, n_both, n_padded, n_refused = H.fuzz_samtools_1_11(eng, seeds, arg, case_base=base, on_scan=on_scan, shift=shift, front=front)
        assert n_both > 45 and n_padded > 28 and n_refused <= 0.05 * len(seeds) + 1, (n_both, n_padded, n_refused)          # oracle: 68 columns with an insertion and a deletion, 43 padded alleles
        return n_lines
    return H.fuzz_filters_and_regions(eng, seeds, arg, case_base=base, rng_base=RNG_BASE, on_scan=on_scan, shift=shift, front=front)


# ---- 1. the tensor build at every magnitude
@pytest.mark.parametrize("where", list(MAGNITUDES))
@pytest.mark.parametrize("name", list(BUILD))
def test_tensor_build_at_chromosome_scale(routed, name, where):
    n_lines = run_build(routed("default"), name, MAGNITUDES[where])
    assert n_lines > BUILD[name][3], (name, where, n_lines)


# ---- 2. the same through the deep routes
@pytest.mark.parametrize("where", ["chr1", "top"])
@pytest.mark.parametrize("name", list(ROUTED))
@pytest.mark.parametrize("route", ROUTES)
def test_deep_routes_at_chromosome_scale(routed, route, name, where):
    kw, base, floor, _ = ROUTED[name]
    seen = {}
    n_cases, n_lines = H.fuzz_match_oracle(routed(route), SEEDS, kw, case_base=base, on_scan=H.route_check(route, seen), shift=MAGNITUDES[where])
    assert n_cases == len(SEEDS) and n_lines > floor, n_lines
    assert seen["scans"] >= len(SEEDS) and seen["listed"] >= len(SEEDS), seen
    if route == "giant_slices":
        assert seen["slices"] > seen["giant"] > 0, seen


# ---- 3. the phases of reads against bins and of tile starts against reads, bins and coarse bins
def sweep_cases(name, K):
    """[(seeds, shift, front)] of one sweep test: combination i takes the seeds 4 i .. 4 i + 3."""
    return [(range(4 * i, 4 * i + 4), H.k_plus(K, phi), front) for i, (phi, front) in enumerate(GRID)]


@pytest.mark.parametrize("where", list(SWEEP_K))
@pytest.mark.parametrize("name", list(SWEEP))
def test_phases_of_reads_and_tiles_against_bins(routed, name, where):
    kw, route, base, floor, _ = SWEEP[name]
    eng = routed(route or "default")
    n_lines = 0
    for seeds, shift, front in sweep_cases(name, SWEEP_K[where]):
        n_lines += H.fuzz_match_oracle(eng, seeds, kw, case_base=base, on_scan=H.route_check(route) if route else None, shift=shift, front=front)[1]
    assert n_lines > floor, (name, where, n_lines)


# ---- 4. the very top, by hand
TOP_REF_LEN, TOP_REGION = 1500, 400


def top_case(channels):
    """(ReadSet, reference slice, its 1-based first position, ctg_start, ctg_end): 16 reads that END on 0-based INT32_MAX — the last position a read
    may end on — and eight shorter ones, both strands, three haplotype tags, over a slice whose last base is 1-based INT32_MAX; the reads carry an
    SNP on ctg_end - 5, a deletion of two behind ctg_end - 13 and an insertion of three behind ctg_end - 21, ctg_end = C3R_CTG_END_MAX: all within
    the last 33 positions of the region, whose rows (to ctg_end + 33) and windows the reads cover."""
    from clair3_rna_amd.reads import ReadSet
    rng = random.Random(41)
    L = TOP_REF_LEN
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    first = INT32_MAX - L + 1                       # 1-based position of ref[0]; 0-based position first - 1
    end = CTG_END_MAX - first                       # index in ref of ctg_end's base
    snp, dl, ins = end - 5, end - 13, end - 21
    alt = "A" if ref[snp] != "A" else "C"
    recs = []
    for k in range(24):
        s = 60 + 9 * k                              # the read's first base (index in ref)
        stop = L if k < 16 else L - 40 - 11 * k     # (exclusive)
        body = list(ref)
        if k % 2 == 0:
            body[snp] = alt
        ops, seq, x = [], [], s

        def aligned(to):
            return "".join(body[x:to])
        if k % 3 == 0:                              # insertion behind `ins`
            ops.append("%dM3I" % (ins + 1 - x)); seq.append(aligned(ins + 1) + "GAT"); x = ins + 1
        if k % 4 == 1:                              # deletion behind `dl`
            ops.append("%dM2D" % (dl + 1 - x)); seq.append(aligned(dl + 1)); x = dl + 3
        ops.append("%dM" % (stop - x)); seq.append(aligned(stop))
        recs.append(dict(pos=first - 1 + s, cigar="".join(ops), seq="".join(seq), flag=16 * (k % 2 == (k // 2) % 2), mapq=60, hp=(k % 3) if channels == 30 else 0))
    rs = ReadSet.from_records(recs)
    assert H.readset_end(rs) == INT32_MAX
    return rs, ref, first, CTG_END_MAX - TOP_REGION, CTG_END_MAX


def top_oracle(channels, head_tail, ctg_end=CTG_END_MAX):
    rs, ref, first, a, _ = top_case(channels)
    return H.oracle_chunk(rs, ref, first, a, ctg_end, channels=channels, min_coverage=2, head_tail=bool(head_tail))


def _scan_top(eng, channels, head_tail, route=None):
    from clair3_rna_amd import capi
    rs, ref, first, a, b = top_case(channels)
    exp = top_oracle(channels, head_tail)
    eng.params = capi.default_params()
    eng.set_bed(0, None); eng.set_bed(1, None)
    eng.set_params(channels=channels, min_coverage=2, head_tail=head_tail)
    got = H.engine_chunk(eng, rs, ref, first, a, b)
    if route is not None and not head_tail:
        H.route_check(route)(eng, exp)
    assert got["lines"] == exp["lines"], H.first_diff(got["lines"], exp["lines"])
    assert np.array_equal(got["X"], exp["X"])
    pos = [int(l.split("\t")[1]) for l in exp["lines"]]
    assert sum(b - 33 <= p <= b for p in pos) >= 3 and len(pos) >= 3, pos          # the SNP, the deletion and the insertion: the comparison is about the edge
    eng.params = capi.default_params()
    eng.set_params()
    return exp


@pytest.mark.parametrize("head_tail", [0, 1])
@pytest.mark.parametrize("route", ROUTES)
def test_reads_that_end_on_int32_max_in_the_last_accepted_region(routed, route, head_tail):
    eng = routed(route)
    _scan_top(eng, 18, head_tail, route)
    _scan_top(eng, 30, head_tail, route)


# ---- 5. one past the top
def test_the_first_refused_region_end_and_the_scan_after_it(routed):
    from clair3_rna_amd import capi
    eng = routed("default")
    rs, ref, first, a, b = top_case(18)
    eng.params = capi.default_params()
    eng.set_params(min_coverage=2)
    eng.load_reads(rs)
    eng.set_reference(first, ref)
    with pytest.raises(capi.C3RError, match=r"region 0 ends beyond C3R_CTG_END_MAX = 2147482590"):
        eng.scan(a, b + 1)
    with pytest.raises(capi.C3RError, match=r"region 1 ends beyond C3R_CTG_END_MAX"):
        eng.scan_regions([(a, b - 100), (b - 99, b + 1)])
    with pytest.raises(capi.C3RError, match=r"reference slice ends beyond 2\^31"):
        eng.set_reference(first + 1, ref)
    eng.set_reference(first, ref)
    assert eng.scan(a, b) == len(top_oracle(18, 0)["lines"]) > 0
    _scan_top(eng, 18, 0)


# ---- 6. several regions, the last one ending on the last accepted position
REGIONS_SEEDS = range(6)


def regions_case(seed):
    """(ReadSet, slice, first, three regions that tile the case at K_TOP)"""
    rs, ref, first, last, _ = H.placed_case(940000 + seed, False, H.K_TOP)
    n = last - first + 1
    return rs, ref, first, [(first, first + n // 3), (first + n // 3 + 1, first + 2 * n // 3), (first + 2 * n // 3 + 1, last)]


def test_three_regions_the_last_ending_on_the_last_accepted_position(routed):
    from clair3_rna_amd import capi
    eng = routed("default")
    n_lines = 0
    for seed in REGIONS_SEEDS:
        rs, ref, first, regions = regions_case(seed)
        assert regions[-1][1] == CTG_END_MAX
        exps = [H.oracle_chunk(rs, ref, first, a, b, min_coverage=2) for a, b in regions]
        eng.params = capi.default_params()
        eng.set_params(min_coverage=2)
        eng.load_reads(rs)
        eng.set_reference(first, ref)
        eng.begin_batch()
        for a, b in regions:
            eng.scan(a, b)
        eng.end_batch()
        X1, S1, T1 = eng.tensors(), eng.sites(), eng.tokens()
        eng.begin_batch(); eng.scan_regions(regions); eng.end_batch()
        assert np.array_equal(X1, eng.tensors()) and S1.tobytes() == eng.sites().tobytes() and T1.tobytes() == eng.tokens().tobytes(), seed
        assert [int(l.split("\t")[1]) for e in exps for l in e["lines"]] == S1["pos"].tolist(), seed
        assert np.array_equal(X1, np.concatenate([e["X"] for e in exps])) if len(S1) else True
        n_lines += len(S1)
    assert n_lines > 770, n_lines                   # oracle: 1106 lines over the three regions of the six cases
    eng.params = capi.default_params()
    eng.set_params()


# ---- 7. rows: POS of nine and of ten digits
@pytest.mark.parametrize("where", ["chr1", "top"])
@pytest.mark.parametrize("compat", [0, 1])
def test_rows_cpp_equals_python_with_nine_and_ten_digit_positions(routed, compat, where):
    base, rng_base, floor, _ = ROWS
    n_rows, kinds = H.fuzz_decode_rows_and_regions(routed("default"), SEEDS, compat, case_base=base, rng_base=rng_base, shift=MAGNITUDES[where])
    assert n_rows > floor and {"0/0", "0/1", "1/1"} <= kinds, (n_rows, kinds)
    assert len(str(H.K_CHR1(777, 0) + 1)) == 9 and len(str(H.K_TOP(777, 0) + 1)) == 10


# ---- 8. the phasing kernels
PHASING = ["hap", "links", "merge", "allele"]
PHASING_SEEDS = [0, 1]
_phasing = {}


def _other(rng, b):
    return rng.choice([c for c in "ACGT" if c != b])


def phasing_case(kind, seed):
    """The generated case of a kind, untranslated, with one more site on the last base of the read that ends last (`end`: the largest 0-based exclusive
    read end = that base's 1-based position): dict(rs, end, L, table, ...).  Built once, never changed."""
    if (kind, seed) in _phasing:
        return _phasing[(kind, seed)]
    rng = random.Random(5150 + seed)
    if kind == "hap":
        ref, rs, table, _ = hapref.gen_case(seed)
        end = H.readset_end(rs)
        assert end > int(table["pos"][-1])
        table = np.concatenate([table, hapref.make_sites([(end, ref[end - 1], _other(rng, ref[end - 1]), 1, int(table["ps"][-1]))])])
        query = table.copy()
        query["h1"] = 0
        query["ps"][::4] = [rng.choice(table["ps"].tolist()) for _ in query[::4]]          # a quarter counted against some other set
        c = dict(rs=rs, table=table, query=query)
    elif kind in ("links", "merge"):
        if kind == "links":
            ref, rs, sites, _, _ = P.gen_case(seed, errors=True)
        else:
            ref, rs, sites, _, _ = M.gen_fragmented(seed, 9)
        end = H.readset_end(rs)
        assert end > int(sites["pos"][-1])
        sites = np.concatenate([sites, P.make_sites([(end, ref[end - 1], _other(rng, ref[end - 1]))])])
        c = dict(rs=rs, table=sites)
    else:
        ref, rs, rows, truth, planted, _ = HA.gen_case(seed, errors=True)
        end = H.readset_end(rs)
        table = hapref.make_sites([(p, r, a, int(t), 100 + 3 * (k // 30) + k % 3) for k, ((p, r, a), t) in enumerate(zip(rows, truth))])
        assert end > int(table["pos"][-1]) and end > max(p["pos"] for p in planted) + 8
        table = np.concatenate([table, hapref.make_sites([(end, ref[end - 1], _other(rng, ref[end - 1]), 1, int(table["ps"][-1]))])])
        sites = HA.planted_sites(planted) + HA.snv_sites(table[::5]) + (HA.snv_sites(table[-1:]) if (len(table) - 1) % 5 else [])
        c = dict(rs=rs, table=table, sites=HA.nearest_sets(sorted(sites, key=lambda s: s["pos"]), table))
    c.update(end=end, L=len(ref))
    _phasing[(kind, seed)] = c
    return c


def phasing_shift(kind, seed, where):
    c = phasing_case(kind, seed)
    return H.CHR1_LEN - c["L"] if where == "chr1" else INT32_MAX - c["end"]


def phasing_expected(kind, seed, K):
    """The restatements' answers for the case translated by K (ps values as they are): a dict of arrays."""
    c = phasing_case(kind, seed)
    rs, table = H.shift_readset(c["rs"], K), H.shift_sites(c["table"], K)
    out = dict(rs=rs, table=table)
    if kind == "hap":
        out["query"] = H.shift_sites(c["query"], K)
        out["hp"], out["stats"], _ = hapref.haplotag(rs, table)
        out["ps"] = HC.read_phase_sets(rs, table)
        out["counts"] = HC.hap_counts(rs, table, out["query"])
    elif kind in ("links", "merge"):
        out["links"] = P.links(rs, table)
        out["chain"] = P.resolve(table, out["links"])[0]
        out["ulinks"] = M.unit_links(rs, out["chain"])
    else:
        out["sites"] = [dict(s, pos=s["pos"] + K) for s in c["sites"]]
        out["counts"] = HA.counts(rs, table, out["sites"])
    return out


def phasing_floors(kind, e):
    """The tables are not empty (from the restatement alone), and the site on the last read's last base is seen."""
    if kind == "hap":
        n = e["counts"]
        assert e["stats"]["n_hp1"] >= 100 and e["stats"]["n_hp2"] >= 100 and len(set(e["ps"].tolist())) >= 20, e["stats"]
        assert n[:, 1].sum() > 300 and n[:, 2].sum() > 300 and n[:, 0].sum() > 100 and n[-1].sum() >= 1, n[-1]
    elif kind in ("links", "merge"):
        assert int(e["links"].sum()) > 3000 and int(e["links"][-1].sum()) >= 1 and len(e["ulinks"]) >= (2 if kind == "merge" else 1), (int(e["links"].sum()), len(e["ulinks"]))
        if kind == "merge":
            assert int(e["ulinks"].sum()) > 50, int(e["ulinks"].sum())
    else:
        n = e["counts"]
        at = [j for j, s in enumerate(e["sites"]) if HA.flags(s)[1]]
        assert len(at) >= 30 and n[at, 1:, 0].sum() > 200 and n[at, 1:, 1].sum() > 200 and n[-1].sum() >= 1, n[-1]


@pytest.mark.parametrize("where", ["chr1", "end"])
@pytest.mark.parametrize("seed", PHASING_SEEDS)
@pytest.mark.parametrize("kind", PHASING)
def test_phasing_kernels_at_chromosome_scale_and_on_int32_max(routed, kind, seed, where):
    from clair3_rna_amd import capi
    eng = routed("default")
    K = phasing_shift(kind, seed, where)
    e = phasing_expected(kind, seed, K)
    if where == "end":
        assert H.readset_end(e["rs"]) == INT32_MAX and int(e["table"]["pos"][-1]) == INT32_MAX
    phasing_floors(kind, e)
    eng.params = capi.default_params()
    eng.set_params()
    try:
        if kind == "hap":
            eng.set_phase_sites(e["table"])
            eng.load_reads(e["rs"])
            hp, st = eng.haplotags()
            assert hp.tolist() == e["hp"].tolist() and st == e["stats"]
            assert eng.read_phase_sets().tolist() == e["ps"].tolist()
            got = eng.hap_counts(e["query"])
            assert np.array_equal(got, e["counts"]), np.argwhere(got != e["counts"])[:10]
        elif kind in ("links", "merge"):
            eng.set_phase_sites(None)
            eng.load_reads(e["rs"])
            got = eng.phase_links(e["table"])
            assert np.array_equal(got, e["links"]), np.argwhere(got != e["links"])[:10]
            got = eng.phase_unit_links(e["chain"])
            assert got.shape == e["ulinks"].shape and np.array_equal(got, e["ulinks"]), np.argwhere(got != e["ulinks"])[:10]
        else:
            eng.set_phase_sites(e["table"])
            eng.load_reads(e["rs"])
            query, pool = HA.to_query(e["sites"], seed % 2)
            got = eng.hap_allele_counts(query, pool)
            assert np.array_equal(got, e["counts"]), np.argwhere(got != e["counts"])[:10]
    finally:
        eng.set_phase_sites(None)
