"""What tests/test_gpu_coords.py compares the engine with does not depend on the coordinates (CPU only).

For exactly the seeds, parameters and translations of that file: the oracle's mpileup rows and create_tensor lines at K equal those at K = 0 with
the position field rewritten, and its tensors are identical; the phasing restatements give equal tags, sets and tables; the Python decoder's rows
agree after POS is rewritten.  The oracle carries positions as int64 and the restatements are plain Python, so this is what lets the GPU file
trust them at 2^31 — engine(K) == oracle(K) == shift(oracle(0)), the last term being the one the golden vectors pin.  The file also holds the
oracle's own line counts for those seeds: the floors of the GPU tests are at most 70 % of them."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_gpu_coords as G

_zero = {}


def _at_zero(key, make):
    if key not in _zero:
        _zero[key] = make()
    return _zero[key]


def _same(e0, eK, K, what, front=None):
    """eK is e0 moved by K.  front = (slice, first, front bases): head/tail calling prints the reference under a window that begins before the
    case's first base — the front bases, where the slice at K = 0 has none and shows 'A'; that field then equals the slice's own text."""
    assert H.shift_lines(e0["rows"], K) == eK["rows"], what
    if front is None or not front[2]:
        assert H.shift_lines(e0["lines"], K) == eK["lines"], what
    else:
        ref, first, d = front[0].upper(), front[1], front[2]
        assert len(e0["lines"]) == len(eK["lines"]), what
        for x, y in zip(H.shift_lines(e0["lines"], K), eK["lines"]):
            fx, fy = x.split("\t"), y.split("\t")
            pos = int(fy[1])
            assert fx[:2] == fy[:2] and fx[3:] == fy[3:], (what, pos)
            assert fy[2] == "".join(ref[p - first] if 0 <= p - first < len(ref) else "A" for p in range(pos - 16, pos + 17)), (what, pos)
            assert fx[2] == fy[2] or pos - 16 < first + d, (what, pos)
    assert np.array_equal(e0["X"], eK["X"]) and np.array_equal(e0["depth"], eK["depth"]), what
    return len(eK["lines"])


def _match_oracle(kw, compat, seed, shift, front):
    """(oracle result, K) for one case of fuzz_match_oracle / fuzz_samtools_1_11 / fuzz_decode_rows_and_regions."""
    channels = kw.get("channels", 18)
    okw = {k: bool(v) for k, v in kw.items() if k != "channels"}
    rs, ref, first, last, recs = H.placed_case(seed, channels == 30, shift, front)
    return H.oracle_chunk(rs, ref, first, first, last, channels=channels, min_coverage=2, mpileup_compat=compat, **okw), first + front - 1, (ref, first, front)


def _build_oracle(name, seed, shift, front):
    kind, arg, base, _, _ = G.BUILD[name]
    if kind in ("match", "samtools"):
        return _match_oracle(arg, int(kind == "samtools"), base + seed, shift, front)[:2]
    c0 = H.filters_case(seed, arg, base, G.RNG_BASE)
    c = H.filters_case(seed, arg, base, G.RNG_BASE, shift=shift, front=front)
    K = c["b"] - c0["b"]
    assert c["a"] == c0["a"] + K - front and c["ref_start"] == c0["ref_start"] + K - front and c["ht"] == c0["ht"]
    return H.filters_oracle(c), K


def _floor_ok(floor, figure):
    assert 0 < floor <= 0.7 * figure, (floor, figure)


@pytest.mark.parametrize("where", list(G.MAGNITUDES))
@pytest.mark.parametrize("name", list(G.BUILD))
def test_tensor_build_references(name, where):
    import re
    n, n_both, n_padded = 0, 0, 0
    for seed in G.SEEDS:
        e0, _ = _at_zero(("build", name, seed), lambda: _build_oracle(name, seed, 0, 0))
        eK, K = _build_oracle(name, seed, G.MAGNITUDES[where], 0)
        assert K > 2 ** 27
        n += _same(e0, eK, K, (name, where, seed))
        n_both += sum(1 for r in eK["rows"] if re.search(r"[+][0-9]+[ACGTNacgtn=RYry*#]+-[0-9]+[Nn]", r.split("\t")[4]))
        n_padded += sum(1 for l in eK["lines"] if re.search(r" I[ACGT][A-Z=]*[*#]", l.split("\t")[4]))
    assert n == G.BUILD[name][4], (name, n)
    _floor_ok(G.BUILD[name][3], n)
    if name == "samtools":
        assert (n_both, n_padded) == (68, 43), (n_both, n_padded)          # (run_build's floors: 45 and 28)


def test_no_case_of_the_1_11_printer_exceeds_the_pad_table():
    """Runs of I and P ops above 64 characters, counted from the CIGAR strings: none on the seeds that run with mpileup_compat = 1."""
    n = 0
    for base in (G.BUILD["samtools"][2], G.ROWS[0]):
        for seed in G.SEEDS:
            _, recs = H._case(base + seed, phased=False)
            n += sum(H._ip_run_chars(r["cigar"]) > 64 for r in recs)
    assert n == 0


@pytest.mark.parametrize("where", ["chr1", "top"])
@pytest.mark.parametrize("name", list(G.ROUTED))
def test_deep_route_references(name, where):
    kw, base, floor, figure = G.ROUTED[name]
    n = 0
    for seed in G.SEEDS:
        e0 = _at_zero(("routed", name, seed), lambda: _match_oracle(kw, 0, base + seed, 0, 0)[0])
        eK, K, _ = _match_oracle(kw, 0, base + seed, G.MAGNITUDES[where], 0)
        n += _same(e0, eK, K, (name, where, seed))
    assert n == figure, n
    _floor_ok(floor, n)


@pytest.mark.parametrize("where", list(G.SWEEP_K))
@pytest.mark.parametrize("name", list(G.SWEEP))
def test_phase_sweep_references(name, where):
    kw, _, base, floor, figure = G.SWEEP[name]
    n, moved = 0, set()
    for seeds, shift, front in G.sweep_cases(name, G.SWEEP_K[where]):
        for seed in seeds:
            e0 = _at_zero(("sweep", name, seed), lambda: _match_oracle(kw, 0, base + seed, 0, 0)[0])
            eK, K, placed = _match_oracle(kw, 0, base + seed, shift, front)
            n += _same(e0, eK, K, (name, where, seed, front), placed)
            moved.add(((K - front - 33) % 32, (K - front - 33) % 256, K % 32))          # p0 against bins and coarse bins; reads against bins
    assert n == figure and len(moved) >= 12, (n, moved)
    _floor_ok(floor, n)


@pytest.mark.parametrize("where", ["chr1", "top"])
@pytest.mark.parametrize("compat", [0, 1])
def test_row_references(compat, where):
    """The Python decoder on the oracle's lines and the oracle's forward pass: the rows at K are the rows at 0 with POS rewritten."""
    from clair3_rna_amd import decode, synth
    from oracle import oracle as orc
    base, _, floor, figure = G.ROWS
    w = synth.random_weights(18, seed=4242)
    w[-24 * 129:] *= 6.0
    n = 0

    def rows(e):
        f = [l.split("\t") for l in e["lines"]]
        return decode.vcf_rows("chr20", [int(x[1]) for x in f], [x[2] for x in f], [x[4] for x in f], e["probs"]) if f else []
    for seed in G.SEEDS:
        def zero():
            e = _match_oracle(dict(), compat, base + seed, 0, 0)[0]
            e["probs"] = orc.forward(w, e["X"]) if e["lines"] else None
            e["vcf"] = rows(e)
            return e
        e0 = _at_zero(("rows", compat, seed), zero)
        eK, K, _ = _match_oracle(dict(), compat, base + seed, G.MAGNITUDES[where], 0)
        _same(e0, eK, K, (compat, where, seed))
        eK["probs"] = e0["probs"]                       # (the tensors are identical)
        assert rows(eK) == H.shift_lines(e0["vcf"], K), (compat, where, seed)
        n += len(e0["vcf"])
    assert n == figure, n
    _floor_ok(floor, n)


@pytest.mark.parametrize("head_tail", [0, 1])
@pytest.mark.parametrize("channels", [18, 30])
def test_top_case_reference(channels, head_tail):
    """The hand-made reads that end on INT32_MAX, and the same reads 2,147,482,000 positions lower."""
    rs, ref, first, a, b = G.top_case(channels)
    D = 2147482000
    eK = G.top_oracle(channels, head_tail)
    e0 = H.oracle_chunk(H.shift_readset(rs, -D), ref, first - D, a - D, b - D, channels=channels, min_coverage=2, head_tail=bool(head_tail))
    assert _same(e0, eK, D, (channels, head_tail)) >= 3
    pos = [int(l.split("\t")[1]) for l in eK["lines"]]
    assert {b - 5, b - 13, b - 21} <= set(pos), pos                      # the SNP, the deletion and the insertion


def test_regions_reference():
    n = 0
    for seed in G.REGIONS_SEEDS:
        rs, ref, first, regions = G.regions_case(seed)
        K = first - 1
        for a, b in regions:
            eK = H.oracle_chunk(rs, ref, first, a, b, min_coverage=2)
            e0 = H.oracle_chunk(H.shift_readset(rs, -K), ref, 1, a - K, b - K, min_coverage=2)
            n += _same(e0, eK, K, (seed, a, b))
    assert n == 1106, n
    _floor_ok(770, n)


@pytest.mark.parametrize("where", ["chr1", "end"])
@pytest.mark.parametrize("seed", G.PHASING_SEEDS)
@pytest.mark.parametrize("kind", G.PHASING)
def test_phasing_references(kind, seed, where):
    K = G.phasing_shift(kind, seed, where)
    assert K > 2 ** 27
    e0 = _at_zero(("phasing", kind, seed), lambda: G.phasing_expected(kind, seed, 0))
    eK = G.phasing_expected(kind, seed, K)
    G.phasing_floors(kind, eK)
    for k in e0:
        if k in ("rs", "sites"):
            continue
        if k in ("table", "query", "chain"):
            assert eK[k].tobytes() == H.shift_sites(e0[k], K, ps=(k == "chain")).tobytes(), (kind, k)
        elif k == "stats":
            assert eK[k] == e0[k]
        else:
            assert eK[k].dtype == e0[k].dtype and np.array_equal(eK[k], e0[k]), (kind, k)


def test_the_limit_is_stated_once():
    """include/c3r.h, the Python binding and the tests' helpers name the same last accepted ctg_end: INT32_MAX - 33 (the rows of a region reach
    ctg_end + 33) - 1024 (headroom of the kernels' 32-bit position arithmetic: two tiles of 256 and a flank of 16 are what they add)."""
    import os
    import re
    from clair3_rna_amd import capi
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "c3r.h")).read()
    m = re.search(r"#define C3R_CTG_END_MAX (\d+)LL", text)
    assert m and int(m.group(1)) == capi.CTG_END_MAX == H.CTG_END_MAX == H.INT32_MAX - 33 - 1024
    assert 2 * 256 + 16 < 1024
