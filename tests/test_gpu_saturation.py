"""Saturated gates.  The cell updates clamp the exp2 values of g, tanh(c) and i; the o and f gates' exp2 may overflow to inf and must
come out as an exact 0, never as a NaN.  Weights and windows here drive layer-1 and layer-2 pre-activations of i, f, g and o far beyond
both ends — below -89, where exp2 of the sigmoid argument is inf in fp32, and above +52, where tanh's exp2 underflows to 0 — at some
units, among them cells with i at the low end and g at the high end at once (inf * 0: why i keeps its clamp), while the rest of the
network stays the usual random one.  Checked at both channel counts, on the split-f16 kernels with the fixed 2^12 scale,
on their run-time-scale instantiations (biases of +-60) and on the fp32 MFMA path: no NaN, and the oracle's probabilities within the
suite's 1e-4.  That the inputs do saturate is asserted on a float64 evaluation of the pre-activations, not assumed."""
import numpy as np
import pytest

from tests import helpers as H
from tests import netref

pytestmark = pytest.mark.gpu

H1, H2, T = netref.H1, netref.H2, netref.T
BIG = 7.5            # below the 8 that the fixed 2^12 split-f16 scale allows a weight
DRIVEN = range(8, 24)        # layer-1 units (both directions) held at h ~ +1: layer 2's large inputs


def _views(w, C):
    """Writable (K, R, b) views of the two LSTM layers' directions inside the flat blob: dict(l1=[fwd, bwd], l2=[fwd, bwd])."""
    out, pos = {}, 0
    for name, cin, Hn in (("l1", C, H1), ("l2", 2 * H1, H2)):
        out[name] = []
        for _ in range(2):
            K = w[pos:pos + cin * 4 * Hn].reshape(cin, 4 * Hn); pos += K.size
            R = w[pos:pos + Hn * 4 * Hn].reshape(Hn, 4 * Hn); pos += R.size
            b = w[pos:pos + 4 * Hn]; pos += b.size
            out[name].append((K, R, b))
    return out


def _weights(C, rts, seed):
    """synth.random_weights with a few saturating units.  Gate columns are i | f | g | o blocks of H."""
    from clair3_rna_amd import synth
    w = synth.random_weights(C, seed=seed)
    v = _views(w, C)
    for d in range(2):
        K, R, b = v["l1"][d]
        # the last channel carries counts of both signs (see _windows): one weight row reaches both ends of a gate
        for u, gate in ((0, 0), (1, 3), (2, 2), (3, 1), (4, 0), (4, 2), (5, 3), (5, 0)):
            K[C - 1, gate * H1 + u] = BIG if (u + d) % 2 == 0 else -BIG
        K[C - 1, 0 * H1 + 6], K[C - 1, 2 * H1 + 6] = BIG, -BIG          # unit 6: i and g at opposite ends
        K[C - 1, 3 * H1 + 7], K[C - 1, 2 * H1 + 7] = -BIG, BIG          # unit 7: o and g at opposite ends
        # units held near h = +1 by their biases alone (i, f, o open, g at +1: c grows by one a step)
        for u in DRIVEN:
            K[:, [g * H1 + u for g in range(4)]] = 0.0
            R[:, [g * H1 + u for g in range(4)]] = 0.0
            for g in range(4):
                b[g * H1 + u] = BIG
        K2, R2, b2 = v["l2"][d]
        # layer-2 units 0 .. 7: each gate driven to about +-16 * 7.5 * h by the sixteen held units of layer 1's forward half
        for u, gate, sign in ((0, 0, 1), (1, 0, -1), (2, 3, 1), (3, 3, -1), (4, 2, 1), (5, 2, -1), (6, 1, 1), (7, 1, -1),
                              (8, 0, -1), (8, 2, 1), (9, 3, -1), (9, 2, 1), (9, 0, 1)):
            for k in DRIVEN:
                K2[k, gate * H2 + u] = sign * BIG
        if rts:
            for u, gate, val in ((30, 0, -60.0), (31, 0, 60.0), (32, 3, -60.0), (33, 3, 60.0), (34, 2, -60.0), (35, 2, 60.0)):
                b[gate * H1 + u] = val
                b2[gate * H2 + u] = val
    return w


def _windows(n, C, seed):
    r = np.random.RandomState(seed)
    X = H.pileup_like(n, C, seed)
    X[:, :, C - 1] = r.randint(-30, 31, size=(n, T))
    X[::5, :, C - 1] = 0
    return X


def _preact_range(w, X):
    """float64 min / max of every gate's pre-activation in both layers, {(layer, gate): (min, max)}, and under (layer, "i-g+") the
    number of cells with i below -89 and g above +52 at once."""
    C = X.shape[2]
    W = netref.split_blob(w, C)
    out = {}

    def run(x, K, R, b, reverse, layer):
        n, Hn = x.shape[0], R.shape[0]
        zx = x @ K + b
        h, c = np.zeros((n, Hn)), np.zeros((n, Hn))
        y = np.empty((n, T, Hn))
        for s in range(T):
            t = T - 1 - s if reverse else s
            z = zx[:, t] + h @ R
            for g in range(4):
                zg = z[:, g * Hn:(g + 1) * Hn]
                lo, hi = out.get((layer, g), (np.inf, -np.inf))
                out[(layer, g)] = (min(lo, float(zg.min())), max(hi, float(zg.max())))
            out[(layer, "i-g+")] = out.get((layer, "i-g+"), 0) + int(((z[:, :Hn] < -89.0) & (z[:, 2 * Hn:3 * Hn] > 52.0)).sum())
            c = netref._sigm(z[:, Hn:2 * Hn]) * c + netref._sigm(z[:, :Hn]) * np.tanh(z[:, 2 * Hn:3 * Hn])
            h = netref._sigm(z[:, 3 * Hn:]) * np.tanh(c)
            y[:, t] = h
        return y

    x = np.asarray(X, dtype=np.float64)
    y1 = np.concatenate([run(x, *W["l1"][d], bool(d), 1) for d in range(2)], axis=2)
    for d in range(2):
        run(y1, *W["l2"][d], bool(d), 2)
    return out


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("rts", [False, True], ids=["fixed_scale", "run_time_scale"])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("C", [18, 30])
def test_saturated_gates_match_oracle(eng, C, precision, rts):
    from oracle import oracle as orc
    w = _weights(C, rts, seed=500 + C)
    X = _windows(256, C, 60 + C)
    rng = _preact_range(w, X)
    for layer in (1, 2):
        for gate in (0, 3):                     # i, o: gate_frac's a arguments — exp2 overflows below -88.7
            assert rng[(layer, gate)][0] < -89.0 and rng[(layer, gate)][1] > 45.0, (layer, gate, rng[(layer, gate)])
        for gate in (1, 2):                     # f, g
            assert rng[(layer, gate)][0] < -52.0 and rng[(layer, gate)][1] > 52.0, (layer, gate, rng[(layer, gate)])
        assert rng[(layer, "i-g+")] > 100, (layer, rng[(layer, "i-g+")])
    eng.set_precision(precision)
    try:
        eng.load_weights(w, C)
        g = eng.precision_guard()
        assert eng.precision()[0] == precision and not g["fell_back"], (eng.precision(), g)
        if precision == "f16x3":
            assert (g["scale_log2"][0] < 12 and g["scale_log2"][1] < 12) if rts else g["scale_log2"] == [12, 12, 12], g
        p = eng.infer(tensors=X)
        assert p.shape == (len(X), 24) and np.isfinite(p).all(), int((~np.isfinite(p)).sum())
        err = float(np.abs(p - orc.forward(w, X)).max())
        print("saturation C=%d %s rts=%d: max |dP| = %.3g, pre-activation ranges %s" % (C, precision, rts, err, {k: (tuple(round(x) for x in v) if isinstance(v, tuple) else v) for k, v in rng.items()}))
        assert err < 1e-4, err
    finally:
        eng.set_precision("f16x3")
