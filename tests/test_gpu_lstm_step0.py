"""Step 0 of the layer-2 LSTM (k_lstm2_w16, precision "f16x3") runs without its recurrent part: h_{-1} = 0, so those products are exact
zeros and the kernel skips them.  What that must not change: windows whose whole signal sits in the step that is step 0 of the forward
(t = 0) or of the backward (t = 32) workgroup, windows with no signal at all, ragged batches at both channel counts, weights that run
on a run-time scale, and — nothing may depend on LDS that a skipped step no longer writes — the bits of a batch that is run again after
another one, or shifted to other lanes, blocks and workgroups.  Every case against the fp32 oracle, with the tolerances of
tests/test_gpu_lstm2_w16.py."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    e.set_precision("f16x3")
    yield e
    e.close()


_W = {}


def _weights(C):
    from clair3_rna_amd import synth
    if C not in _W:
        _W[C] = synth.random_weights(C, seed=500 + C)
    return _W[C]


def _windows(n, C, seed):
    """Pileup-shaped windows (negative reference channels, small alt counts, mixed depths) and a share of plain random ones."""
    r = np.random.RandomState(seed)
    X = r.randint(-40, 41, size=(n, 33, C)).astype(np.int32)
    depth = r.choice([6, 20, 90, 216], size=(n, 1, 1))
    X[::2] = np.minimum(np.abs(X[::2]), 8)
    X[::2, :, :C // 2] = -depth[::2]
    return X


def _err(eng, w, X):
    from oracle import oracle as orc
    p = eng.infer(tensors=X)
    assert p.shape == (len(X), 24) and np.isfinite(p).all()
    return float(np.abs(p - orc.forward(w, X)).max())


@pytest.mark.parametrize("t", [0, 32])
def test_signal_only_in_an_end_column(eng, t):
    """t = 0 is step 0 of the forward workgroups, t = 32 of the backward ones: everything the window says enters in the shortened step."""
    C = 18
    w = _weights(C)
    eng.load_weights(w, C)
    X = np.zeros((70, 33, C), np.int32)
    X[:, t, :] = _windows(70, C, 7 + t)[:, t, :]
    err = _err(eng, w, X)
    assert err <= 1e-5, err


def test_all_zero_windows(eng):
    """Every step is bias only; sites beyond one workgroup."""
    C = 18
    w = _weights(C)
    eng.load_weights(w, C)
    err = _err(eng, w, np.zeros((65, 33, C), np.int32))
    assert err <= 1e-5, err


@pytest.mark.parametrize("C", [18, 30])
@pytest.mark.parametrize("n", [1, 17, 64, 65, 130])
def test_ragged_batches(eng, n, C):
    w = _weights(C)
    eng.load_weights(w, C)
    err = _err(eng, w, _windows(n, C, 1000 * C + n))
    assert err <= 1e-5, err


def test_run_time_scale(eng):
    """The weights of test_w16_run_time_scale_matches_oracle: layer 2 and L4 on scales below 2^12, the RTS instantiation of the kernel."""
    from clair3_rna_amd import synth
    C = 18
    o = H.blob_offsets(C)
    w = synth.random_weights(C, seed=1234)
    w[o["l2_bias0"] + 3] = 30.0
    w[o["l2"] + 11] = 9.0
    w[o["l4"] + 99] = 100.0
    eng.load_weights(w, C)
    g = eng.precision_guard()
    try:
        assert g["scale_log2"][1] < 12 and g["scale_log2"][2] < 12 and not g["fell_back"] and eng.precision()[0] == "f16x3", g
        err = _err(eng, w, _windows(65, C, 9))
        assert err < 1e-4, err
    finally:
        eng.set_precision("f16x3")


def test_repeat_and_shift_keep_every_bit(eng):
    """Two calls on one engine with different batches, then the first batch again; the batch shifted by 16 sites (another block) and by 48
    (another quarter of the workgroup, the tail in another workgroup)."""
    C = 18
    w = _weights(C)
    eng.load_weights(w, C)
    X = _windows(200, C, 21)
    X[::7] //= 8                                   # small activations -> small h -> subnormal lo halves
    Y = _windows(130, C, 22) * 3
    base = eng.infer(tensors=X).copy()
    other = eng.infer(tensors=Y).copy()
    assert np.array_equal(eng.infer(tensors=X), base)
    assert np.array_equal(eng.infer(tensors=Y), other)
    for k in (16, 48):
        assert np.array_equal(eng.infer(tensors=X[k:]), base[k:]), k
    from oracle import oracle as orc
    err = float(np.abs(base - orc.forward(w, X)).max())
    assert err <= 1e-5, err
