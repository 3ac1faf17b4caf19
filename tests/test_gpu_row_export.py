"""Row export on the device: k_row_keep, the exclusive scan, k_pack_rows / k_pack_tokens, k_export_tokens.
tests/c/row_export_check.hip drives the kernels themselves on hand-made arrays against serial host code; the engine tests below reach the same
kernels through c3r_rows_begin[_ex] where the existing row tests do not: sites of more than 64 tokens whose alleles tie (the later rounds of
site_tok_rank and the carried indel rank decide the row), keep counts of zero and of everything, and the kept count against the rule itself."""
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import keepref

pytestmark = pytest.mark.gpu


def test_row_export_kernels_against_the_host_reference(tmp_path):
    """Build tests/c/row_export_check.hip and run it once: k_row_keep on 102,468 cases (every centre letter, 0.5 and P(ref) ties to the ulp,
    the 1e-30 guard), the scan at 17 lengths on both routes, the packers and the exporter on sites of 0 .. 4097 tokens and on 33,003 sites,
    every output word compared, canaries around every output buffer.  (A few seconds to build, under two to run.)"""
    exe = H.build_row_export_check(str(tmp_path / "row_export_check"), timeout=90)
    assert exe is not None, "hipcc not found: the kernels cannot be checked"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=45)
    lines = out.stdout.strip().split("\n")
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert [l.split(":")[0] for l in lines] == ["A host", "A k_row_keep", "B scan", "C pack and export"] and all(l.endswith(": ok") for l in lines), out.stdout


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


def _text(rows):
    return "".join(r + "\n" for r in rows).encode()


_deep = {}


def _deep_case(compat):
    if compat not in _deep:
        ref, rs, cols = H.deep_tie_loci()
        _deep[compat] = (ref, rs, cols, H.oracle_chunk(rs, ref, 1, 1, len(ref), min_coverage=2, mpileup_compat=compat))
    return _deep[compat]


# weight seeds chosen on the CPU (orc.forward on the oracle's tensors, output layers sharpened x6): the reference decoder alone prints at the six
# deep loci  14: SNV + insertion pairs (`G>T,GCAG`)   17: insertions, deletions, two deletions (`CGCC>C,CCC`)   7: insertion + deletion (`GT>G,GCAGT`)
DEEP_WEIGHT_SEEDS = (14, 17, 7)


def _deep_weights(seed):
    from clair3_rna_amd import synth
    w = synth.random_weights(18, seed=seed)
    w[-24 * 129:] *= 6.0
    return w


@pytest.mark.parametrize("compat", [0, 1])
def test_deep_loci_with_tied_alleles_decode_like_the_reference(eng, compat):
    """Six loci of 63, 64, 65, 128, 129 and 200 tokens (tests/helpers.py deep_tie_loci): at each, two mismatching bases, two insertion alleles
    and two deletion lengths with EQUAL read counts, carriers interleaved in BAM order on both strands.  The decoder breaks every tie by first
    appearance, so a token (or an indel record) out of BAM order changes REF / ALT.  Reference: the oracle's alt_info lines through the Python
    decoder with the probabilities the device returned.  Every way rows leave the device must equal it byte for byte."""
    from clair3_rna_amd import capi, decode
    from oracle import oracle as orc
    ref, rs, cols, exp = _deep_case(compat)
    eng.params = capi.default_params()
    eng.set_bed(0, None); eng.set_bed(1, None)
    eng.set_params(min_coverage=2, mpileup_compat=compat)
    got = H.engine_chunk(eng, rs, ref, 1, 1, len(ref))
    assert got["lines"] == exp["lines"], H.first_diff(got["lines"], exp["lines"])
    sites = got["sites"]
    at = {int(s["pos"]): int(s["n_tok"]) for s in sites}
    assert tuple(at[c] for c in cols) == H.DEEP_TIE_TOKENS, at
    assert int((got["tokens"]["indel"] != 0).sum()) > 250
    f = [l.split("\t") for l in exp["lines"]]
    seen_indel = seen_snv = 0
    for seed in DEEP_WEIGHT_SEEDS:
        w = _deep_weights(seed)
        eng.load_weights(w, 18)
        eng.set_precision("f16x3")
        probs = eng.infer()
        assert np.abs(probs - orc.forward(w, exp["X"])).max() < 1e-4
        for show_ref in (True, False):
            py = decode.vcf_rows("chr20", [int(x[1]) for x in f], [x[2] for x in f], [x[4] for x in f], probs, show_ref=show_ref)
            want = _text(py)
            if not show_ref:
                deep = [r.split("\t") for r in py if int(r.split("\t")[1]) in cols]
                seen_indel += sum(1 for r in deep if any(len(a) != len(r[3]) for a in r[4].split(",")))
                seen_snv += sum(1 for r in deep if any(len(a) == 1 and len(r[3]) == 1 for a in r[4].split(",")))
            assert eng.call_rows_text("chr20", qual=2, show_ref=show_ref)[0] == want, (seed, show_ref)
            assert eng.rows_begin(host_reads=False).decode("chr20", qual=2, show_ref=show_ref)[0] == want, (seed, show_ref)
            assert eng.rows_begin(host_reads=True).decode("chr20", qual=2, show_ref=show_ref)[0] == want, (seed, show_ref)
        assert eng.rows_begin(drop_ref_calls=True).decode("chr20", qual=2, show_ref=False)[0] == want, seed
    assert seen_indel >= 6 and seen_snv >= 3, (seen_indel, seen_snv)       # (the reference alone prints indel and SNV ALTs at the deep loci)


_small = {}


def _small_case():
    from clair3_rna_amd import synth
    if not _small:
        _small["c"] = synth.small_case(seed=77, ref_len=60000, n_genes=12, depth=25)[:2]
    return _small["c"]


def _scan_small(eng):
    from clair3_rna_amd import capi
    ref, rs = _small_case()
    eng.params = capi.default_params()
    eng.set_bed(0, None); eng.set_bed(1, None)
    eng.set_params(min_coverage=2)
    eng.load_reads(rs); eng.set_reference(1, ref)
    n = eng.scan(1, len(ref))
    assert n > 500
    return n


def _snapshots(eng):
    """-> (rows of the full snapshot without show_ref, rows of the snapshot that drops RefCalls on the device, info of both)"""
    full_snap = eng.rows_begin(host_reads=False)
    info_full = full_snap.info()
    full, n_full = full_snap.decode("chr20", qual=2, show_ref=False)
    snap = eng.rows_begin(drop_ref_calls=True)
    info = snap.info()
    filt, n_filt = snap.decode("chr20", qual=2, show_ref=False)
    assert n_full == full.count(b"\n") and n_filt == filt.count(b"\n")
    return full, filt, info_full, info


def _biased_weights(which):
    """"bias X": synth.random_weights(seed 9) with ref_bias X.  "z0 underflow": +200 on the bias of the zygosity head's second class instead.  (The
    heads apply selu BEFORE the softmax, so no logit goes below -1.76: a negative ref_bias, however large, leaves P(0/0) near 0.04 and cannot make
    it underflow; a large logit of another class can.)"""
    from clair3_rna_amd import synth
    if which == "z0 underflow":
        w = synth.random_weights(18, seed=9)
        w[-2] += 200.0
        return w
    return synth.random_weights(18, seed=9, ref_bias=float(which.split()[1]))


def test_keep_counts_at_both_extremes_and_the_snapshot_after_an_empty_one(eng):
    """ref_bias +60: P(0/0) is 1 to the last bit and every class product of the other zygosities is below 1e-24, so every site is a RefCall before
    alt_info is looked at: nothing leaves the device, the snapshot is empty and equal to the full one's (empty) text.  A normal snapshot taken
    right after the empty one, in the same context, is correct (the staging blocks and the counters of the empty return are reused).
    ref_bias -200: the selu in front of the softmax holds the 0/0 logit at its floor, P(0/0) < P(1/1) at every site, so P(1/1) * P(ref ref) beats
    the reference product and every site is kept.  "z0 underflow": P(0/0) == 0 exactly, the `p_ref >= 1e-30f` side of the rule: every site kept."""
    n = _scan_small(eng)
    eng.set_precision("f16x3")
    eng.load_weights(_biased_weights("bias +60"), 18)
    eng.infer(fetch=False)
    p = eng.fetch_probs(n)
    assert (p[:, 21] == 1.0).all()
    full, filt, info_full, info = _snapshots(eng)
    assert full == filt == b"" and info == (0, 0, 0) and info_full[0] == n
    # right afterwards, same context: a normal weight set
    eng.load_weights(_biased_weights("bias 4"), 18)
    eng.infer(fetch=False)
    full, filt, info_full, info = _snapshots(eng)
    assert filt == full and 0 < info[0] < n and full != b""          # (some sites dropped, some kept, rows printed)
    for which in ("bias -200", "z0 underflow"):
        eng.load_weights(_biased_weights(which), 18)
        eng.infer(fetch=False)
        p = eng.fetch_probs(n)
        assert (p[:, 21] == 0.0).all() if which == "z0 underflow" else (p[:, 21] < p[:, 22]).all(), which
        full, filt, info_full, info = _snapshots(eng)
        assert filt == full and info[0] == n == info_full[0] and full.count(b"\n") > 100, which
        assert info[1:] == (len(eng.tokens()), info_full[2])       # every site kept: all its tokens, the same indel records


@pytest.mark.parametrize("which", ["bias 0", "bias 4", "bias +60", "bias -200", "z0 underflow", "deep ties"])
def test_kept_count_equals_the_rule(eng, which):
    """c3r_rows_info: the sites of a drop_ref_calls snapshot are exactly those tests/keepref.py keeps, given the device's own probabilities and
    the sites' centre letters; the full snapshot holds every site and one indel record per token with an indel."""
    from clair3_rna_amd import capi
    if which == "deep ties":
        ref, rs, cols, exp = _deep_case(0)
        eng.params = capi.default_params()
        eng.set_bed(0, None); eng.set_bed(1, None)
        eng.set_params(min_coverage=2)
        eng.load_reads(rs); eng.set_reference(1, ref)
        n = eng.scan(1, len(ref))
        w = _deep_weights(DEEP_WEIGHT_SEEDS[0])
    else:
        n = _scan_small(eng)
        w = _biased_weights(which)
    eng.set_precision("f16x3")
    eng.load_weights(w, 18)
    eng.infer(fetch=False)
    probs = eng.fetch_probs(n)
    sites, toks = eng.sites(), eng.tokens()
    centres = [chr(bytes(s)[16]) for s in sites["ref33"]]
    kept = keepref.keep(probs, centres)
    full = eng.rows_begin(host_reads=False)
    n_sites, n_bytes, n_recs = full.info()
    full.free()
    assert n_sites == n and n_recs == int((toks["indel"] != 0).sum()) and n_bytes >= len(toks)
    snap = eng.rows_begin(drop_ref_calls=True)
    k_sites, k_bytes, k_recs = snap.info()
    snap.free()
    assert k_sites == int(kept.sum()), (k_sites, int(kept.sum()), n)
    # (site order = token order of eng.tokens(): the kept sites' tokens and indel records are countable from the same arrays)
    owner = np.repeat(np.arange(n), sites["n_tok"])
    assert k_bytes == int(sites["n_tok"][kept].sum()) and k_recs == int(((toks["indel"] != 0) & kept[owner]).sum())


def test_tokens_and_both_snapshot_kinds_interleaved_on_one_context(eng):
    """The token export's scan total, the kept count and the two pack counters are words of one control block.  tokens(), a snapshot that drops
    RefCalls, tokens(), a full snapshot and another dropping one, in that order on one context: each call leaves the others' results as they were."""
    n = _scan_small(eng)
    eng.set_precision("f16x3")
    eng.load_weights(_biased_weights("bias 4"), 18)
    eng.infer(fetch=False)
    toks_a = eng.tokens()
    drop_a = eng.rows_begin(drop_ref_calls=True)
    info_a = drop_a.info()
    text_a = drop_a.decode("chr20", qual=2, show_ref=False)[0]
    toks_b = eng.tokens()
    full = eng.rows_begin(host_reads=False)
    info_full = full.info()
    text_full = full.decode("chr20", qual=2, show_ref=False)[0]
    drop_b = eng.rows_begin(drop_ref_calls=True)
    info_b = drop_b.info()
    text_b = drop_b.decode("chr20", qual=2, show_ref=False)[0]
    assert toks_a.tobytes() == toks_b.tobytes() and len(toks_a) > 0
    assert info_a == info_b and 0 < info_a[0] < n == info_full[0]
    assert text_a == text_b == text_full and text_a != b""
