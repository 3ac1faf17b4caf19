"""Every launch of net_forward_slice (csrc/net_host.hpp), once: arithmetic variant x channel count x kind of input.

    variant      layer 1                                    layer 2 (+ L4)               reached by
    f32          k_lstm<32, C, 128, true>                   k_lstm<256, 256, 160, false>, k_fc4     set_precision("f32")
    f16x3        k_lstm1_rs<C, false, false>                k_lstm2_w16<0, false>        set_precision("f16x3"), ordinary weights (scales 12 12 12)
    f16x3-rts    k_lstm1_rs<C, false, true>                 k_lstm2_w16<0, true>         set_precision("f16x3"), weights that need a run-time scale
    f16+f8       k_lstm1_rs<C, true, false>                 k_lstm2_mx                   set_precision("f16+f8"), ordinary weights
    (k_heads_mfma closes all of them)                       C = 18 and C = 30: the two instantiations of each layer-1 kernel

    input        host        c3r_infer(tensors): int32 rows in batch order            (x16 = 0, row_idx = null)
                 resident16  the scan's int16 windows through row_idx                  (x16 = 1)
                 resident32  the int32 windows a context keeps after one scan of a position covered by more than 32,767 reads (x16 = 0, row_idx)

Which variant ran is checked through the public API: precision(), the guard's scale_log2 (other than 12 12 12 <=> the RTS kernels) and
fell_back.  That a context is on int32 windows has no accessor: include/c3r.h (c3r_pileup_scan) promises that it stays on them."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import netref

pytestmark = pytest.mark.gpu

WEIGHTS = {18: 1234, 30: 99}
VARIANTS = ("f32", "f16x3", "f16x3-rts", "f16+f8")
INPUTS = ("host", "resident16", "resident32")
RAGGED = (1, 63, 65, 129)


@functools.lru_cache(maxsize=None)
def _case(C):
    from clair3_rna_amd import synth
    ref, rs, _ = synth.small_case(seed=3, ref_len=30000, n_genes=6, depth=20, phased=(C == 30))
    return ref, rs, H.oracle_chunk(rs, ref, 1, 1, len(ref), channels=C)


@functools.lru_cache(maxsize=None)
def _weights(C, variant):
    from clair3_rna_amd import synth
    return H.scaled_weights(C, seed=WEIGHTS[C]) if variant == "f16x3-rts" else synth.random_weights(C, seed=WEIGHTS[C])


@functools.lru_cache(maxsize=None)
def _expected(C, variant):
    from oracle import oracle as orc
    X, w = _case(C)[2]["X"], _weights(C, variant)
    return orc.forward(w, X), netref.forward(w, X)


@pytest.fixture(scope="module")
def engines():
    """'16': a fresh context (int16 resident windows); '32': a context after one scan of 33,000 reads over one position, without the cap."""
    from clair3_rna_amd import capi
    e16, e32 = capi.Engine(0), capi.Engine(0)
    ref, rs = H.shallow_locus_beside_a_deep_one(n_deep=33000, deep_len=12, fwd_every=2)
    e32.set_params(max_depth=0)
    got = H.engine_chunk(e32, rs, ref, 1, 1, len(ref))
    assert got["n"] == 1 and got["raw"].min() < -16000
    e32.set_params(max_depth=8000)
    yield {"16": e16, "32": e32}
    e16.close()
    e32.close()


def _select(eng, C, variant):
    w = _weights(C, variant)
    eng.set_precision("f16x3")
    eng.load_weights(w, C)
    eng.set_precision(variant.split("-")[0])
    g, mode = eng.precision_guard(), eng.precision()[0]
    assert mode == variant.split("-")[0] and not g["fell_back"], (variant, mode, g)
    assert (g["scale_log2"] != [12, 12, 12]) == (variant == "f16x3-rts"), (variant, g)
    return w


def _bound(variant):
    return 1e-5 if variant == "f16x3" else 1e-4         # (what the existing tests assert for f16x3 with ordinary weights; the project's 1e-4 elsewhere)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("C", [18, 30])
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_launch_variant_of_the_network(engines, variant, C, kind):
    """Within 1e-4 of the oracle (1e-5 for f16x3 with ordinary weights), and the resident windows give the very bits a host batch of the
    same tensors gives — in every cell: the kernels convert int16 and int32 rows to the same numbers and no result depends on the row
    order."""
    eng = engines["32" if kind == "resident32" else "16"]
    ref, rs, exp = _case(C)
    try:
        eng.set_params(channels=C)
        got = H.engine_chunk(eng, rs, ref, 1, 1, len(ref))
        assert got["n"] > 100 and np.array_equal(got["X"], exp["X"])
        _select(eng, C, variant)
        po, p64 = _expected(C, variant)
        p_res, p_host = eng.infer(), eng.infer(tensors=exp["X"])
        p = p_host if kind == "host" else p_res
        err = float(np.abs(p - po).max())
        print("%-9s C=%d %-10s n=%d  max |P - oracle| %.2e   |P - fp64| %.2e   |oracle - fp64| %.2e" %
              (variant, C, kind, len(p), err, float(np.abs(p - p64).max()), float(np.abs(po - p64).max())))
        assert np.isfinite(p).all() and err < _bound(variant), (variant, C, kind, err)
        assert np.array_equal(p_res, p_host), (variant, C, kind, float(np.abs(p_res - p_host).max()))
    finally:
        eng.set_precision("f16x3")


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_host_batches_run_time_scale_30_channels(engines, n):
    """k_lstm1_rs<30, false, true> on partial site blocks and partial workgroups."""
    C, variant = 30, "f16x3-rts"
    eng = engines["16"]
    X = _case(C)[2]["X"][5:5 + n]
    try:
        _select(eng, C, variant)
        p = eng.infer(tensors=X)
        err = float(np.abs(p - _expected(C, variant)[0][5:5 + n]).max())
        assert p.shape == (n, 24) and np.isfinite(p).all() and err < _bound(variant), (n, err)
    finally:
        eng.set_precision("f16x3")


@pytest.mark.parametrize("n", RAGGED)
@pytest.mark.parametrize("C", [18, 30])
def test_ragged_resident_batches_fp32(engines, C, n):
    """The fp32 kernels on n resident windows: the first n candidates of the case, scanned again as a genotyping-mode site list."""
    from clair3_rna_amd import capi
    from oracle import oracle as orc
    eng = engines["16"]
    ref, rs, exp = _case(C)
    pos = [int(l.split("\t")[1]) for l in exp["lines"][:n]]
    try:
        eng.set_params(channels=C, genotyping_mode=1)
        eng.set_sites(pos)
        eng.load_reads(rs)
        eng.set_reference(1, ref)
        assert eng.scan(1, len(ref)) == n
        X = eng.tensors(rescaled=True)
        w = _select(eng, C, "f32")
        p = eng.infer()
        err = float(np.abs(p - orc.forward(w, X)).max())
        assert p.shape == (n, 24) and np.isfinite(p).all() and err < 1e-4, (C, n, err)
        assert np.array_equal(p, eng.infer(tensors=X))
    finally:
        eng.set_precision("f16x3")
        eng.params = capi.default_params()
        eng.set_params()
