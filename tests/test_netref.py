"""The fp32 CPU oracle against the float64 reference of tests/netref.py (no GPU): probabilities and both LSTM layers' outputs, at both
channel counts, on the suite's usual windows and on windows whose flank reaches into a deep locus (tests/helpers.py)."""
import numpy as np
import pytest

from tests import helpers as H
from tests import netref

WEIGHTS = {18: 1234, 30: 99}

# Twice the largest |oracle - float64| measured over the cases below (both channel counts; the values are in the test's docstring).
BOUND = {"ordinary": dict(P=8.2e-6, y1=6.8e-5, y2=3.7e-6), "beyond f16": dict(P=1.5e-5, y1=5.0e-4, y2=2.8e-5)}


def _usual(C):
    rng = np.random.RandomState(11 + C)
    return np.concatenate([H.pileup_like(150, C, 7 + C), rng.randint(-216, 217, size=(40, 33, C)).astype(np.int32),
                           rng.randint(-20, 21, size=(60, 33, C)).astype(np.int32), np.zeros((3, 33, C), np.int32)])


def _cases(C):
    return [("ordinary", "usual windows, |x| <= 216", _usual(C)),
            ("ordinary", "deep flank, D = 8000", H.deep_flank_windows(120, C, 8000, 1000 + C)),
            ("ordinary", "deep flank, D = 32767", H.deep_flank_windows(120, C, 32767, 1000 + C)),
            ("beyond f16", "deep flank, D = 2^20", H.deep_flank_windows(120, C, 2 ** 20, 1000 + C)),
            ("ordinary", "single entries of +-2047 .. +-65505", H.edge_count_windows(C, 50 + C))]


@pytest.mark.parametrize("C", [18, 30])
def test_oracle_agrees_with_the_float64_reference(C):
    """max |oracle - float64| as measured when the bounds were set (probabilities / layer-1 output / layer-2 output):

        C = 18   usual windows           3.57e-06 / 5.46e-06 / 4.27e-07        C = 30   2.34e-06 / 1.00e-05 / 5.63e-07
                 deep flank D = 8000     2.25e-06 / 7.04e-06 / 5.30e-07                 2.33e-06 / 2.35e-05 / 9.97e-07
                 deep flank D = 32767    3.07e-06 / 2.90e-05 / 1.82e-06                 4.08e-06 / 3.40e-05 / 1.23e-06
                 single large entries    1.71e-06 / 1.22e-06 / 3.55e-07                 2.03e-06 / 7.49e-07 / 3.19e-07
                 deep flank D = 2^20     7.33e-06 / 2.49e-04 / 1.40e-05                 2.86e-06 / 1.67e-04 / 7.20e-06

    The hidden states are compared as they are (|h| < 1).  Counts of 10^5 .. 10^6 put pre-activations of 10^4 .. 10^5 into fp32 sums, whose
    last bit is then 10^-3 .. 10^-2: the oracle's layer-1 output is worse there, its probabilities hardly are."""
    from clair3_rna_amd import synth
    from oracle import oracle as orc
    w = synth.random_weights(C, seed=WEIGHTS[C])
    assert netref.weight_count(C) == w.size
    for kind, name, X in _cases(C):
        p, y1, y2, a4 = netref.forward(w, X, return_hidden=True)
        po, o1, o2 = orc.forward(w, X, return_hidden=True)
        assert p.dtype == np.float64 and p.shape == (len(X), 24) and y1.shape == o1.shape and y2.shape == o2.shape and a4.shape == (len(X), 128)
        assert np.isfinite(p).all() and np.allclose(p[:, :21].sum(1), 1, atol=1e-12) and np.allclose(p[:, 21:].sum(1), 1, atol=1e-12)
        got = dict(P=float(np.abs(po - p).max()), y1=float(np.abs(o1 - y1).max()), y2=float(np.abs(o2 - y2).max()))
        print("C=%d %-38s max |x| %7d   |oracle - fp64|: P %.2e  y1 %.2e  y2 %.2e" % (C, name, np.abs(X).max(), got["P"], got["y1"], got["y2"]))
        for k, v in got.items():
            assert v <= BOUND[kind][k], (C, name, k, v, BOUND[kind][k])


def test_the_input_cast_hook_sees_the_integer_windows():
    """input_cast is applied to the windows before layer 1 and to nothing else: the identity changes nothing, rounding to one f16 changes
    nothing while every count is at most 2048, and moves the result as soon as one is not."""
    from clair3_rna_amd import synth
    w = synth.random_weights(18, seed=1234)
    X = H.pileup_like(20, 18, 3)
    p = netref.forward(w, X)
    assert np.array_equal(netref.forward(w, X, input_cast=lambda x: x), p)
    assert np.array_equal(netref.forward(w, X, input_cast=netref.f16_round), p)
    X[:, 3, 0] = -2049
    X[:, 3, 9] = -4097
    assert np.abs(netref.forward(w, X, input_cast=netref.f16_round) - netref.forward(w, X)).max() > 1e-6
    Y = X.copy()
    Y[:, 5, 0], Y[:, 5, 9] = 70000, -70000
    assert np.isnan(netref.forward(w, Y, input_cast=netref.f16_round)).any() and np.isfinite(netref.forward(w, Y)).all()
