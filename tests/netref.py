"""A float64 evaluation of the network (CPU, numpy only), vectorised over sites: the yardstick that tells the GPU's own error from the
fp32 oracle's.  Written from the Keras LSTM equations and the weight blob layout of include/c3r.h (c3r_load_weights):

    per LSTM layer (128 then 160 units) and direction (forward, backward): K[in, 4H], R[H, 4H], b[4H], gate columns i | f | c | o
        z_t = x_t K + h_{t-1} R + b;  c_t = sigm(z_f) c_{t-1} + sigm(z_i) tanh(z_c);  h_t = sigm(z_o) tanh(c_t)
        the backward direction walks t = 32 .. 0 and writes h_t at position t; a layer's output is [forward | backward] per position
    L4: selu(flatten(y2)[33 * 320] W + b) -> 128;  L5_1, L5_2: selu(a4 W + b) -> 128 each
    Y_gt21 = softmax(selu(a5_1 W + b)) (21 classes), Y_genotype = softmax(selu(a5_2 W + b)) (3 classes)
"""
import numpy as np

H1, H2, T, L4 = 128, 160, 33, 128
SELU_SCALE, SELU_ALPHA = 1.0507009873554805, 1.6732632423543772


def weight_count(C):
    n = 2 * (C * 4 * H1 + H1 * 4 * H1 + 4 * H1) + 2 * (2 * H1 * 4 * H2 + H2 * 4 * H2 + 4 * H2)
    return n + T * 2 * H2 * L4 + L4 + 2 * (L4 * L4 + L4) + L4 * 21 + 21 + L4 * 3 + 3


def split_blob(w, C):
    """The flat fp32 blob as float64 arrays: dict(l1=[(K, R, b) fwd, bwd], l2=[...], l4=(W, b), l51, l52, gt21, gt)."""
    w = np.asarray(w, dtype=np.float64)
    assert w.ndim == 1 and w.size == weight_count(C), (w.shape, weight_count(C))
    pos = [0]

    def take(*shape):
        n = int(np.prod(shape))
        a = w[pos[0]:pos[0] + n].reshape(shape)
        pos[0] += n
        return a

    out = {}
    for name, cin, H in (("l1", C, H1), ("l2", 2 * H1, H2)):
        out[name] = [(take(cin, 4 * H), take(H, 4 * H), take(4 * H)) for _ in range(2)]
    for name, cin, cout in (("l4", T * 2 * H2, L4), ("l51", L4, L4), ("l52", L4, L4), ("gt21", L4, 21), ("gt", L4, 3)):
        out[name] = (take(cin, cout), take(cout))
    assert pos[0] == w.size
    return out


def _sigm(z):
    # 1 / (1 + exp(-z)) without overflow warnings at the deep counts' pre-activations (exp(-z) = inf gives the correct 0)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def _selu(x):
    return np.where(x > 0, SELU_SCALE * x, SELU_SCALE * SELU_ALPHA * np.expm1(np.minimum(x, 0.0)))


def _softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _lstm_dir(x, K, R, b, reverse):
    n, H = x.shape[0], R.shape[0]
    zx = x @ K + b                                   # [n, T, 4H]
    h, c = np.zeros((n, H)), np.zeros((n, H))
    y = np.empty((n, T, H))
    for s in range(T):
        t = T - 1 - s if reverse else s
        z = zx[:, t] + h @ R
        c = _sigm(z[:, H:2 * H]) * c + _sigm(z[:, :H]) * np.tanh(z[:, 2 * H:3 * H])
        h = _sigm(z[:, 3 * H:]) * np.tanh(c)
        y[:, t] = h
    return y


def forward(weights, X, input_cast=None, return_hidden=False):
    """Probabilities [n, 24] in float64 for integer windows X [n, 33, C].  input_cast: applied to the integer windows before layer 1
    (e.g. `lambda X: X.astype(np.float16)`: what a kernel that rounds its counts to one f16 would see).  return_hidden: also the layer
    outputs, (probs, y1 [n, 33, 256], y2 [n, 33, 320], a4 [n, 128])."""
    X = np.asarray(X)
    assert X.ndim == 3 and X.shape[1] == T and np.issubdtype(X.dtype, np.integer), (X.shape, X.dtype)
    C = X.shape[2]
    W = split_blob(weights, C)
    with np.errstate(over="ignore", invalid="ignore"):           # (a cast to f16 may overflow to inf, and inf - inf is NaN: that is the point)
        x = np.asarray(X if input_cast is None else input_cast(X), dtype=np.float64)
        assert x.shape == X.shape
        y1 = np.concatenate([_lstm_dir(x, *W["l1"][d], reverse=bool(d)) for d in range(2)], axis=2)
        y2 = np.concatenate([_lstm_dir(y1, *W["l2"][d], reverse=bool(d)) for d in range(2)], axis=2)
        a4 = _selu(y2.reshape(len(X), T * 2 * H2) @ W["l4"][0] + W["l4"][1])
        a51 = _selu(a4 @ W["l51"][0] + W["l51"][1])
        a52 = _selu(a4 @ W["l52"][0] + W["l52"][1])
        probs = np.concatenate([_softmax(_selu(a51 @ W["gt21"][0] + W["gt21"][1])), _softmax(_selu(a52 @ W["gt"][0] + W["gt"][1]))], axis=1)
    return (probs, y1, y2, a4) if return_hidden else probs


def f16_round(X):
    """The conversion of a kernel that keeps one f16 per count: exact up to 2048, a multiple of 2 / 4 / ... above, inf beyond 65504."""
    with np.errstate(over="ignore"):
        return np.asarray(X, dtype=np.float64).astype(np.float16)
