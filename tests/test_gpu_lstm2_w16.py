"""Layer 2 on v_mfma_f32_16x16x32_f16 (k_lstm2_w16, precision "f16x3"): against the fp32 oracle at both channel counts, with weights that
need a run-time scale, on ragged batches, and bit for bit wherever a site sits inside the 16-site MFMA blocks."""
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


def _windows(n, C, seed):
    """Pileup-shaped windows (negative reference channels, small alt counts, mixed depths) and a share of plain random ones."""
    r = np.random.RandomState(seed)
    X = r.randint(-40, 41, size=(n, 33, C)).astype(np.int32)
    depth = r.choice([6, 20, 90, 216], size=(n, 1, 1))
    X[::2] = np.minimum(np.abs(X[::2]), 8)
    X[::2, :, :C // 2] = -depth[::2]
    return X


@pytest.mark.parametrize("C", [18, 30])
def test_w16_matches_oracle(eng, C):
    from clair3_rna_amd import synth
    from oracle import oracle as orc
    w = synth.random_weights(C, seed=300 + C)
    eng.load_weights(w, C)
    assert eng.precision()[0] == "f16x3" and eng.precision_guard()["scale_log2"] == [12, 12, 12]
    X = _windows(500, C, C)
    err = float(np.abs(eng.infer(tensors=X) - orc.forward(w, X)).max())
    assert err <= 1e-5, err


def test_w16_run_time_scale_matches_oracle(eng):
    """A layer-2 bias of 30 and an L4 weight of 100: layer 2 and L4 run on scales below 2^12 (the RTS instantiation)."""
    from clair3_rna_amd import synth
    from oracle import oracle as orc
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
        X = _windows(300, C, 9)
        err = float(np.abs(eng.infer(tensors=X) - orc.forward(w, X)).max())
        assert err < 1e-4, err
    finally:
        eng.set_precision("f16x3")


@pytest.mark.parametrize("n", [1, 15, 17, 63, 65])
def test_w16_ragged_batches(eng, n):
    from clair3_rna_amd import synth
    from oracle import oracle as orc
    w = synth.random_weights(18, seed=41)
    eng.load_weights(w, 18)
    X = _windows(n, 18, 100 + n)
    p = eng.infer(tensors=X)
    assert p.shape == (n, 24) and np.isfinite(p).all()
    assert float(np.abs(p - orc.forward(w, X)).max()) <= 1e-5


def test_w16_result_does_not_depend_on_position_in_the_site_blocks(eng):
    """Offsets 8, 16 and 48 move every site to another lane of its 16-site block, to another block, and to another quarter of the workgroup."""
    from clair3_rna_amd import synth
    w = synth.random_weights(18, seed=77)
    eng.load_weights(w, 18)
    X = _windows(400, 18, 17)
    X[::7] //= 8                                   # small activations -> small h -> subnormal lo halves
    base = eng.infer(tensors=X).copy()
    for k in (8, 16, 48):
        assert np.array_equal(eng.infer(tensors=X[k:]), base[k:]), k
