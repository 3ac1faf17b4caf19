"""The network on counts that one f16 cannot hold.  The A5 rescale divides a window by the depth of its CENTRE position only
(clair3_rna/utils.py:88-92): a candidate of 12 reads beside an exon covered by thousands keeps those thousands in its flank.  f16 holds
integers exactly up to 2048 and ends at 65504; mpileup's cap is 8000 reads, and without it the tensor build goes on to int32 windows.
Whatever int32 count a caller or the tensor build delivers, every precision must stay within the project's 1e-4 of the fp32 oracle.

The CPU part (no marker) proves that the inputs have teeth: rounding their counts to one f16 moves the float64 reference's own
probabilities by more than 1e-4 on most windows of every set with D >= 8000."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import netref

WEIGHTS = {18: 1234, 30: 99}
DEPTHS = (2048, 4096, 8000, 32767, 65504, 70000, 2 ** 20)     # 8000: mpileup's cap; 32767: the int16 windows' limit; 65504: the last f16
N_PER_SET = 200
TOL = 1e-4                                                    # the project's tolerance (README, include/c3r.h)


@functools.lru_cache(maxsize=None)
def _sets(C):
    """[(name, X, fp32 oracle, float64 reference, windows moved by more than TOL when the counts are rounded to one f16)]"""
    from clair3_rna_amd import synth
    from oracle import oracle as orc
    w = synth.random_weights(C, seed=WEIGHTS[C])
    out = []
    for name, X in [("D=%d" % D, H.deep_flank_windows(N_PER_SET, C, D, 1000 + C)) for D in DEPTHS] + [("edge entries", H.edge_count_windows(C, 50 + C))]:
        p64 = netref.forward(w, X)
        d = np.abs(netref.forward(w, X, input_cast=netref.f16_round) - p64).max(axis=1)
        out.append((name, X, orc.forward(w, X), p64, int((~(d <= TOL)).sum())))          # (a NaN counts as moved)
    return w, out


@pytest.mark.parametrize("C", [18, 30])
def test_the_deep_flank_windows_have_teeth(C):
    """Measured (windows of 200 moved by more than 1e-4, C = 18 / C = 30): D = 2048: 0 / 0 (every count is below 2048: nothing to round),
    4096: 80 / 75, 8000: 184 / 175, 32767: 190 / 187, 65504: 180 / 177, 70000: 181 / 176, 2^20: 200 / 200 (counts beyond 65504 become
    inf and the probabilities NaN).  The counts must be of both parities: with a 1:1 strand split a depth of 7012 is two even numbers
    that one f16 still holds."""
    _w, sets = _sets(C)
    for name, X, _po, _p64, moved in sets:
        print("C=%d %-12s max |x| %7d, odd counts %5.1f %%, f16 rounding moves %3d of %d windows by more than %.0e" %
              (C, name, np.abs(X).max(), 100.0 * (X[np.abs(X) > 2048] % 2 != 0).mean() if (np.abs(X) > 2048).any() else 0.0, moved, len(X), TOL))
        if name.startswith("D=") and int(name[2:]) >= 8000:
            assert 2 * moved > len(X), (C, name, moved)
            big = X[np.abs(X) > 2048]
            assert 0.3 < (big % 2 != 0).mean() < 0.7, (C, name)
        if name == "D=2048":
            assert moved == 0 and np.abs(X).max() <= 2048


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16+f8", "auto"])
@pytest.mark.parametrize("C", [18, 30])
def test_host_batches_with_counts_beyond_f16(eng, C, precision):
    """Every probability finite and within 1e-4 of the oracle, for each depth of the flank and for the single large entries, in the
    precision the engine reports ('auto' takes 'f16+f8' for these weights, as test_precision_f16_f8_opt_in_and_auto_guard asserts).

    With one f16 per count (the kernel before it split them), max |P - oracle| per set, measured on an MI355X — C = 18 / C = 30:
        f16x3   D = 2048: 3.6e-6 / 2.5e-6   4096: 1.9e-3 / 1.7e-3   8000: 3.7e-3 / 3.2e-3   32767: 6.7e-3 / 6.8e-3   65504: 6.5e-3 / 1.0e-2
                70000: 1.0e-2 / 5.1e-3   2^20: 0.90 / 0.93 (finite — the gates saturate on the infinities — and all 200 windows wrong)
                edge entries: 1.9e-5 / 2.3e-5
        f16+f8  the same figures to two digits from D = 4096 on (the counts never pass through fp8); edge entries 3.6e-5 / 2.9e-5
        f32     2.0e-6 .. 4.8e-6 everywhere (it converts the counts to fp32)
    With the counts split exactly: f16x3 1.8e-6 .. 4.6e-6 up to D = 70000 and 2.3e-5 / 4.4e-6 at 2^20 (where the oracle itself is 7.3e-6 /
    2.9e-6 from float64), f16+f8 1.5e-5 .. 2.5e-5 (its usual distance), f32 unchanged."""
    w, sets = _sets(C)
    try:
        eng.set_precision("f16x3")
        eng.load_weights(w, C)
        eng.set_precision(precision)
        mode = eng.precision()[0]
        assert mode == ("f16+f8" if precision == "auto" else precision) and not eng.precision_guard()["fell_back"], (mode, eng.precision_guard())
        worst = {}
        for name, X, po, p64, _moved in sets:
            p = eng.infer(tensors=X)
            err = np.abs(p - po).max(axis=1)
            worst[name] = (bool(np.isfinite(p).all()), float(np.nanmax(err)) if np.isfinite(err).any() else float("nan"))
            print("C=%d %-7s %-12s max |x| %7d   finite %s   max |P - oracle| %.2e (windows above 1e-4 or NaN: %d)   |P - fp64| %.2e   |oracle - fp64| %.2e" %
                  (C, mode, name, np.abs(X).max(), worst[name][0], worst[name][1], int((~(err < TOL)).sum()), float(np.nanmax(np.abs(p - p64))), float(np.abs(po - p64).max())))
        for name, (finite, err) in worst.items():
            assert finite, (C, mode, name, worst)
            assert err < TOL, (C, mode, name, worst)
    finally:
        eng.set_precision("f16x3")


def _scan_and_check(e, rs, ref, C, max_depth):
    e.set_params(channels=C, max_depth=max_depth)
    got = H.engine_chunk(e, rs, ref, 1, 1, len(ref))
    exp = H.oracle_chunk(rs, ref, 1, 1, len(ref), channels=C, max_depth=max_depth)
    assert got["lines"] == exp["lines"], H.first_diff(got["lines"], exp["lines"])
    assert np.array_equal(got["X"], exp["X"]) and np.array_equal(got["raw"], exp["X"])          # (centre depth 12: no rescale)
    return got, exp


@pytest.mark.gpu
@pytest.mark.parametrize("C", [18, 30])
def test_resident_int16_windows_with_a_flank_count_above_2048(C):
    """5003 reads 60M (a third of them on the reverse strand) end where 12 reads with a SNP begin: inside mpileup's cap, int16 windows,
    one candidate of depth 12 whose window holds counts of 3341.  Lines and tensors bit-exact, probabilities within 1e-4 in every
    precision, and the resident windows give the very bits a host batch of the same tensors gives.
    (One f16 per count, measured: |P - oracle| 4.3e-4 at C = 18, 1.2e-4 at C = 30 for f16x3; split exactly: 1.3e-6 / 1.9e-6.)"""
    from clair3_rna_amd import capi, synth
    from oracle import oracle as orc
    ref, rs = H.shallow_locus_beside_a_deep_one(n_deep=5003)
    w = synth.random_weights(C, seed=WEIGHTS[C])
    e = capi.Engine(0)
    try:
        got, exp = _scan_and_check(e, rs, ref, C, 8000)
        X = exp["X"]
        assert got["n"] == 1 and int(got["sites"]["depth"][0]) == 12 and 2048 < np.abs(X).max() <= 32767, (got["n"], np.abs(X).max())
        d = np.abs(netref.forward(w, X, input_cast=netref.f16_round) - netref.forward(w, X)).max()
        assert d > TOL, d                                                                       # teeth: one f16 per count is not enough here
        po = orc.forward(w, X)
        e.load_weights(w, C)
        for precision in ("f32", "f16x3", "f16+f8"):
            e.set_precision(precision)
            assert e.precision()[0] == precision
            p = e.infer()
            err = float(np.abs(p - po).max())
            print("C=%d %-7s resident int16 windows, max |x| %d: max |P - oracle| %.2e" % (C, precision, np.abs(X).max(), err))
            assert np.isfinite(p).all() and err < TOL, (C, precision, err)
            assert np.array_equal(p, e.infer(tensors=X)), (C, precision)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("C", [18, 30])
def test_resident_int32_windows_with_a_flank_count_above_65504(C):
    """Without the cap: 65,700 forward reads 12M end where the 12 reads begin.  More than 32,767 reads cover a position, so the scan
    takes int32 windows; the candidate (depth 12) has the deep pile beside it, not under it, and one channel of its flank holds
    -65,706: beyond the last f16.  (One f16 per count, measured: |P - oracle| 0.49 at C = 18, 0.57 at C = 30 for f16x3; split exactly: 6.0e-7 / 5.4e-7.)"""
    from clair3_rna_amd import capi, synth
    from oracle import oracle as orc
    ref, rs = H.shallow_locus_beside_a_deep_one(n_deep=65700, deep_len=12, fwd_every=0)
    w = synth.random_weights(C, seed=WEIGHTS[C])
    e = capi.Engine(0)
    try:
        got, exp = _scan_and_check(e, rs, ref, C, 0)
        X = exp["X"]
        assert got["n"] == 1 and int(got["sites"]["depth"][0]) == 12 and np.abs(X).max() > 65504, (got["n"], np.abs(X).max())
        po = orc.forward(w, X)
        e.load_weights(w, C)
        for precision in ("f32", "f16x3", "f16+f8"):
            e.set_precision(precision)
            assert e.precision()[0] == precision
            p = e.infer()
            err = float(np.abs(p - po).max())
            print("C=%d %-7s resident int32 windows, max |x| %d: max |P - oracle| %.2e" % (C, precision, np.abs(X).max(), err))
            assert np.isfinite(p).all() and err < TOL, (C, precision, err)
            assert np.array_equal(p, e.infer(tensors=X)), (C, precision)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "f16+f8"])
@pytest.mark.parametrize("C", [18, 30])
def test_a_sites_result_does_not_depend_on_its_neighbours_counts(eng, C, precision):
    """Layer 1 multiplies the counts' extra f16 parts for a whole workgroup of 64 sites, from the first time step on at which one of the 64
    needs them.  Ordinary windows interleaved one by one with deep-flank ones (D = 8000: level 1; D = 2^20: level 2; flanks at either
    end of the window, so the two directions change loops at different steps) must give the very bits they give in a batch of their own,
    and so must the deep ones."""
    w, sets = _sets(C)
    by_name = {name: X for name, X, _po, _p64, _moved in sets}
    shallow = H.pileup_like(96, C, 77 + C)
    try:
        eng.set_precision("f16x3")
        eng.load_weights(w, C)
        eng.set_precision(precision)
        alone = eng.infer(tensors=shallow).copy()
        for name in ("D=8000", "D=1048576"):
            deep = by_name[name][:96]
            deep_alone = eng.infer(tensors=deep).copy()
            mixed = np.empty((192,) + shallow.shape[1:], np.int32)
            mixed[0::2], mixed[1::2] = shallow, deep
            p = eng.infer(tensors=mixed)
            assert np.array_equal(p[0::2], alone), (C, precision, name, float(np.abs(p[0::2] - alone).max()))
            assert np.array_equal(p[1::2], deep_alone), (C, precision, name, float(np.abs(p[1::2] - deep_alone).max()))
    finally:
        eng.set_precision("f16x3")
