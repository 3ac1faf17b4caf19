"""The fused scan's output allocators (c3r_lib.hip, scan_fused; pileup_kernels.hpp, fused_span / k_order_spans / k_finalize_sites).

A scan of fewer than 4096 tiles has one allocator and dense rows.  From 4096 tiles — 917 kb, every real contig — sixteen sub-allocators own
equal slices of the row and token space, sized from what the context's previous sharded scan needed; a span that does not fit its shard
makes the whole scan grow its buffers and run again, the output has holes between the shards' runs that every consumer must step over
through win_idx / tok_off, and later scans of a batch append behind the whole padded space.

The tile count depends only on the region, so ~130 reads within 9 kb of a 918-kb region are a sharded scan that the oracle answers in 0.1 s.
Repeats are FORCED by pigeonhole, never hoped for: a sharded scan of a region without reads leaves 64 rows and 2048 token slots per shard,
and the inputs hold more than 16 x 64 candidates or 16 x 2048 tokens (tests/test_scan_shards_ref.py asserts that with the oracle alone).
They are PROVEN by the launches of k_fused_tiles under the profiler, read right after the scan (the raw re-run launches it again).  The
profiler serialises the deep kernels, so every sequence runs on two fresh contexts: profiled for the counts, unprofiled for the results in
the production two-stream order.  Hint state is per context: every case makes its own and closes it.

The inputs are also shaped so that the third attempt ALWAYS fits.  A regrowth sizes the shards by 1.25 x the fullest shard of the attempt
that failed, and the scan gives up after two regrowths — so three or more equally heavy spans that land one, then two, then three in one
shard would end a scan with "output buffers still too small after growing".  An earlier form of the token-only case (three piles of 18000
slots each) was seen taking all three attempts on the deep route; with two piles, and with a burst whose 41 spans would all have to meet in
one shard, the chain cannot reach a fourth.  The library's policy is left as it is: this is a note for whoever changes it.

On an MI355X: burst (1376 candidates; 5911 tokens at 18 channels, 591 at 30) 2 attempts after each prime on every route; piles (56
candidates, 50400 / 131040 tokens) 2 attempts, 3 once on giant_slices; the wide pile on a fresh context (468 candidates, 2611440 tokens) 2;
IUPAC burst 3 of k_fused_tiles and 1 of k_legacy_tables; the batch's sharded scans (1432 and 56 candidates) 2 each, its dense and empty
scans 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEAT_ROUTES = ["tiles_only", "deep_event_buffer", "giant_slices"]
WHOLE = [(1, H.SHARD_END)]
RAW_REFUSED = "raw tensors are only available for a single (non-batched) scan"

_cases, _oracle = {}, {}


@pytest.fixture
def routed(monkeypatch):
    """routed(route) -> a fresh context made with the route's variables set; the caller closes it."""
    get = H.routed_get(monkeypatch, {})
    return lambda route: get(route, fresh=True)


def _case(name, channels=18):
    if (name, channels) not in _cases:
        _cases[(name, channels)] = H.shard_case(name, channels)
    return _cases[(name, channels)]


def _exp(name, channels=18, regions=WHOLE):
    """The oracle's answer, computed once per input and region list and never changed."""
    key = (name, channels, tuple(regions))
    if key not in _oracle:
        c = _case(name, channels)
        _oracle[key] = H.oracle_regions(c["rs"], c["ref"], list(regions), **c["okw"])
    return _oracle[key]


def _load(eng, c, profiled=None):
    from clair3_rna_amd import capi
    eng.params = capi.default_params()
    eng.set_params(**c["kw"])
    eng.load_reads(c["rs"])
    eng.set_reference(1, c["ref"])
    if profiled is not None:
        eng.set_profiling(profiled)


def _launches(eng, kernel="k_fused_tiles"):
    return eng.kernel_stats().get(kernel, dict(launches=0))["launches"]


def _prime(eng, profiled):
    """A sharded scan that finds nothing: the next one starts from H.PRIMED_ROWS rows and H.PRIMED_TOKS token slots per shard."""
    if profiled:
        eng.reset_kernel_stats()
    assert eng.scan(*H.PRIME_REGION) == 0
    if profiled:
        assert _launches(eng) == 1


def _scan(eng, regions, profiled, on_scan=None, exp=None):
    """One scan -> dict(n, launches, tables, X, raw, S, T).  The launches are read before anything else runs; the raw re-run is made twice:
    it repeats its own bytes and leaves the rescaled tensors, the sites and the tokens as they were."""
    if profiled:
        eng.reset_kernel_stats()
    n = eng.scan(*regions[0]) if len(regions) == 1 else eng.scan_regions(regions)
    launches, tables = (_launches(eng), _launches(eng, "k_legacy_tables")) if profiled else (None, None)
    if on_scan is not None:
        on_scan(eng, exp)
    X, S, T = eng.tensors(), eng.sites(), eng.tokens()
    raw = eng.tensors(rescaled=False)
    assert raw.tobytes() == eng.tensors(rescaled=False).tobytes()
    assert X.tobytes() == eng.tensors().tobytes() and S.tobytes() == eng.sites().tobytes() and T.tobytes() == eng.tokens().tobytes()
    return dict(n=n, launches=launches, tables=tables, X=X, raw=raw, S=S, T=T)


def _equals_oracle(eng, c, got, exp):
    """Sites, alt-info lines (which hold the un-rescaled windows and are built from the tokens) and rescaled tensors."""
    from clair3_rna_amd import altinfo
    assert got["n"] == len(got["S"]) == len(exp["lines"]), (got["n"], len(exp["lines"]))
    assert got["S"]["pos"].tolist() == H.line_positions(exp["lines"])
    lines = altinfo.format_lines(H.CTG, got["S"], got["raw"], got["T"], c["rs"], c["ref"].upper(), 1, padins=eng.pad_insertions())
    assert lines == exp["lines"], H.first_diff(lines, exp["lines"])
    assert np.array_equal(got["X"], exp["X"])
    assert len(got["T"]) == int(got["S"]["n_tok"].sum()) >= H.alt_tokens(exp["lines"])      # (a token per alt_info count, and per `*` inside a deletion)


def _same(a, b):
    for k in ("X", "raw", "S", "T"):
        assert a[k].tobytes() == b[k].tobytes(), k


def _one_shard(eng, monkeypatch, regions, profiled):
    """The same scan with one allocator and dense rows (the library reads the variable at every scan; hints are left alone)."""
    monkeypatch.setenv("C3R_ONE_SHARD", "1")
    try:
        return _scan(eng, regions, profiled)
    finally:
        monkeypatch.delenv("C3R_ONE_SHARD")


def _report(what, **kw):
    print("[scan shards] %s: %s" % (what, ", ".join("%s=%s" % kv for kv in sorted(kw.items()))))


# ---- 1. the edge --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profiled", [True, False], ids=["profiled", "two_streams"])
def test_4095_tiles_take_one_allocator_and_4096_take_sixteen(routed, monkeypatch, profiled):
    """The burst scanned to ctg_end 917247 (4095 tiles) and 917248 (4096), and through 64 regions of 63 x 64 + 63 and 64 x 64 tiles: the same
    bytes, the oracle's; on a primed context the dense scan runs once and the sharded one has to repeat.  A fresh context's first sharded
    scan runs once (4096 rows per shard hold the burst): it is the priming that forces the repeat."""
    eng = routed("default")
    try:
        c, exp = _case("burst"), _exp("burst")
        _load(eng, c, profiled)
        fresh = _scan(eng, WHOLE, profiled)
        _equals_oracle(eng, c, fresh, exp)
        ref = _one_shard(eng, monkeypatch, WHOLE, profiled)          # (its buffers stay: the dense scans below find room at once)
        _same(fresh, ref)
        _prime(eng, profiled)
        dense = _scan(eng, [(1, H.DENSE_END)], profiled)
        sharded = _scan(eng, WHOLE, profiled)
        _same(ref, dense)
        _same(ref, sharded)
        _prime(eng, profiled)
        dense64 = _scan(eng, H.edge_regions(63), profiled)
        sharded64 = _scan(eng, H.edge_regions(64), profiled)
        _same(ref, dense64)
        _same(ref, sharded64)
        _same(ref, _one_shard(eng, monkeypatch, H.edge_regions(64), profiled))
        if profiled:
            _report("edge", candidates=fresh["n"], fresh=fresh["launches"], dense=dense["launches"], sharded=sharded["launches"],
                    dense_regions=dense64["launches"], sharded_regions=sharded64["launches"])
            assert fresh["launches"] == 1
            assert dense["launches"] == 1 and sharded["launches"] >= 2
            assert dense64["launches"] == 1 and sharded64["launches"] >= 2
    finally:
        eng.close()


# ---- 2. repeats are exact -----------------------------------------------------------------------------------------------------------------
def _repeat_sequence(eng, monkeypatch, route, channels, profiled):
    on = H.route_check(route)
    c, exp = _case("burst", channels), _exp("burst", channels)
    _load(eng, c, profiled)
    _prime(eng, profiled)
    a = _scan(eng, WHOLE, profiled, on, exp)
    _equals_oracle(eng, c, a, exp)
    _prime(eng, profiled)
    b = _scan(eng, WHOLE, profiled, on, exp)
    _same(a, b)
    c2, exp2 = _case("burst2", channels), _exp("burst2", channels)
    _load(eng, c2)
    moved = _scan(eng, WHOLE, profiled, on, exp2)
    _equals_oracle(eng, c2, moved, exp2)
    _load(eng, c)
    again = [_scan(eng, WHOLE, profiled, on, exp) for _ in range(3)]      # which shard a span lands in differs from run to run: the output may not
    for g in again:
        _same(a, g)
    _same(a, _one_shard(eng, monkeypatch, WHOLE, profiled))
    if profiled:
        _report("repeat %s %d" % (route, channels), candidates=a["n"], tokens=len(a["T"]), after_prime=(a["launches"], b["launches"]), moved=moved["launches"],
                again=[g["launches"] for g in again])
        assert a["launches"] >= 2 and b["launches"] >= 2


@pytest.mark.parametrize("channels", [18, 30])
@pytest.mark.parametrize("route", REPEAT_ROUTES)
def test_repeat_is_exact(routed, monkeypatch, route, channels):
    """prime, burst, prime, burst, the burst at another offset, the first burst three more times, through the tile kernel and the deep
    kernels (whose shard is blockIdx % 16 with one workgroup per CU): the oracle's output every time, byte for byte the one-allocator scan's,
    and at least two attempts on each burst that follows a prime."""
    for profiled in (True, False):
        eng = routed(route)
        try:
            _repeat_sequence(eng, monkeypatch, route, channels, profiled)
        finally:
            eng.close()


# ---- 3. an overflow of tokens alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route, piles", [("default", "piles_tile"), ("default", "piles_deep"), ("tiles_only", "piles_deep"),
                                          ("deep_event_buffer", "piles_tile"), ("giant_slices", "piles_tile")])
def test_token_only_overflow_then_a_row_overflow(routed, monkeypatch, route, piles):
    """56 candidates fit any shard, their 50400 / 131040 tokens do not fit sixteen primed ones: the scan repeats for tokens alone and
    loses no candidate.  The burst behind it meets hints sized for the piles (at most 1.25 x 56 + 64 rows a shard, fewer than one of its
    spans holds): it repeats for rows."""
    for profiled in (True, False):
        eng = routed(route)
        try:
            on = H.route_check(route)
            c, exp = _case(piles), _exp(piles)
            _load(eng, c, profiled)
            _prime(eng, profiled)
            got = _scan(eng, WHOLE, profiled, on, exp)
            counts = eng.scan_counts()
            _equals_oracle(eng, c, got, exp)
            assert got["n"] == len(exp["lines"]) <= H.PRIMED_ROWS and len(got["T"]) > H.ALLOC_SHARDS * H.PRIMED_TOKS
            if route == "default":
                assert (counts["deep"] > 0) == (piles == "piles_deep") and counts["giant"] == 0, counts
            _same(got, _one_shard(eng, monkeypatch, WHOLE, profiled))
            cb, expb = _case("burst"), _exp("burst")
            _load(eng, cb)
            burst = _scan(eng, WHOLE, profiled, on, expb)
            _equals_oracle(eng, cb, burst, expb)
            _same(burst, _one_shard(eng, monkeypatch, WHOLE, profiled))
            if profiled:
                _report("tokens only %s %s" % (route, piles), candidates=got["n"], tokens=len(got["T"]), piles=got["launches"], burst=burst["launches"], deep_spans=counts["deep"])
                assert got["launches"] >= 2 and burst["launches"] >= 2
        finally:
            eng.close()


def test_a_fresh_context_outgrows_its_first_hints_on_tokens(routed, monkeypatch):
    """No priming: 468 candidates with 2.6 M tokens against the 16 x 131072 slots a context starts with (4096 rows a shard are plenty)."""
    seen = []
    for profiled in (True, False):
        eng = routed("default")
        try:
            c, exp = _case("wide"), _exp("wide")
            _load(eng, c, profiled)
            got = _scan(eng, WHOLE, profiled)
            assert got["n"] == len(exp["lines"]) and np.array_equal(got["X"], exp["X"]) and len(got["T"]) > H.ALLOC_SHARDS * H.FRESH_TOKS
            seen.append(got)
            if profiled:
                _report("fresh context", candidates=got["n"], tokens=len(got["T"]), k_fused_tiles=got["launches"])
                assert got["launches"] >= 2
            else:
                _equals_oracle(eng, c, got, exp)
                _same(got, _one_shard(eng, monkeypatch, WHOLE, profiled))
        finally:
            eng.close()
    _same(*seen)


# ---- 4. two reasons to repeat at once -----------------------------------------------------------------------------------------------------
def test_order_tables_and_a_shard_overflow_in_one_scan(routed, monkeypatch):
    """30 channels, a fresh context (no op / segment tables yet), primed, the burst with an IUPAC base on a covered column: one attempt finds
    the flagged column, the next — with the tables — a full shard, the third fits."""
    for profiled in (True, False):
        eng = routed("default")
        try:
            c, exp = _case("burst_iupac", 30), _exp("burst_iupac", 30)
            _load(eng, c, profiled)
            _prime(eng, profiled)
            if profiled:
                assert "k_legacy_tables" not in eng.kernel_stats()
            got = _scan(eng, WHOLE, profiled)
            _equals_oracle(eng, c, got, exp)
            _same(got, _one_shard(eng, monkeypatch, WHOLE, profiled))
            if profiled:
                _report("two reasons", candidates=got["n"], tokens=len(got["T"]), k_fused_tiles=got["launches"], k_legacy_tables=got["tables"])
                assert got["tables"] >= 1 and got["launches"] >= 3
        finally:
            eng.close()


# ---- 5. batches ---------------------------------------------------------------------------------------------------------------------------
def _batch(eng, profiled):
    """H.BATCH_SCANS as one batch -> (dict(X, S, T, P, rows, text), per scan (kind, candidates, launches))."""
    from clair3_rna_amd import capi
    eng.begin_batch()
    per = []
    for region, kind in H.BATCH_SCANS:
        if profiled:
            eng.reset_kernel_stats()
        n = eng.scan(*region)
        per.append((kind, n, _launches(eng) if profiled else None))
    eng.end_batch()
    out = dict(X=eng.tensors(), S=eng.sites(), T=eng.tokens(), P=eng.infer())
    out["rows"] = eng.call_rows(H.CTG)
    out["text"] = eng.rows_begin(drop_ref_calls=True).decode(H.CTG, qual=2, show_ref=False)[0]
    with pytest.raises(capi.C3RError, match=RAW_REFUSED.replace("(", r"\(").replace(")", r"\)")):
        eng.tensors(rescaled=False)
    assert out["X"].tobytes() == eng.tensors().tobytes() and out["T"].tobytes() == eng.tokens().tobytes()
    return out, per


@pytest.mark.parametrize("profiled", [True, False], ids=["profiled", "two_streams"])
def test_batch_with_regrowths_keeps_every_scan(routed, monkeypatch, profiled):
    """dense, (prime,) sharded burst and piles, dense, (prime,) sharded piles, dense in ONE batch: both sharded scans grow the batch's buffers
    and repeat while earlier scans are resident.  Sites, tokens, tensors, probabilities and row text equal the column-store path's, byte for
    byte; every scan's slice of the batch equals that scan alone, which equals the oracle."""
    from clair3_rna_amd import synth
    eng = routed("default")
    try:
        c = _case("batch")
        _load(eng, c, profiled)
        eng.load_weights(synth.random_weights(18, seed=9), 18)
        eng.set_precision("f16x3")
        fused, per = _batch(eng, profiled)
        again, _per = _batch(eng, profiled)                          # (hints have settled: no repeat now, other shards, the same bytes)
        monkeypatch.setenv("C3R_NO_FUSE", "1")
        store, _p = _batch(eng, False)
        monkeypatch.delenv("C3R_NO_FUSE")
        for k in ("S", "T", "X", "P"):
            assert fused[k].tobytes() == store[k].tobytes(), k
            assert fused[k].tobytes() == again[k].tobytes(), k
        assert fused["rows"] == store["rows"] == again["rows"] and fused["text"] == store["text"] == again["text"] and len(fused["text"]) > 0
        assert np.isfinite(fused["P"]).all()
        # slice by slice: the scan alone, and the oracle
        row, tok = 0, 0
        for (region, kind), (_k, n, _l) in zip(H.BATCH_SCANS, per):
            exp = _exp("batch", 18, [region])
            assert n == len(exp["lines"]), (region, kind)
            if kind == "prime":
                continue
            alone = _scan(eng, [region], False)
            _equals_oracle(eng, c, alone, exp)
            nt = len(alone["T"])
            S = alone["S"].copy()
            S["tok_off"] += tok
            assert fused["S"][row:row + n].tobytes() == S.tobytes(), (region, kind)
            assert fused["X"][row:row + n].tobytes() == alone["X"].tobytes(), (region, kind)
            assert fused["T"][tok:tok + nt].tobytes() == alone["T"].tobytes(), (region, kind)
            row, tok = row + n, tok + nt
        assert row == len(fused["S"]) and tok == len(fused["T"])
        if profiled:
            _report("batch", scans=per, candidates=row, tokens=tok)
            assert all(l >= 2 for k, _n, l in per if k == "sharded") and all(l == 1 for k, _n, l in per if k == "prime")
    finally:
        eng.close()


# ---- 7. the holes between the shards are never read ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [1, 255])
def test_repeats_and_batches_pass_with_poisoned_allocations(byte):
    """Tests 2 and 5 again with every fresh device allocation filled with `byte` (tests/test_gpu_poison.py): a consumer that reads a row or a
    token slot between the shards' runs sees the fill."""
    if os.environ.get("C3R_POISON"):
        pytest.skip("already inside a poisoned run")
    env = dict(os.environ, C3R_POISON=str(byte))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_scan_shards.py",
                        "-k", "test_repeat_is_exact or test_batch_with_regrowths_keeps_every_scan"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "\n8 passed" in r.stdout, r.stdout[-500:]
