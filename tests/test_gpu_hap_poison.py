"""Uninitialised and stale device memory under the haplotype kernels and row export.  C3R_POISON=<byte> fills every FRESH allocation of
libc3r (tests/test_gpu_poison.py); a buffer that a larger earlier call filled is neither fresh nor poisoned — it holds that call's data, and
the drivers work exactly so: one context, contig after contig, large then small.  Both are covered here by one tour (tests/haptour.py)
through the mask, every tagger and its _w sibling, the count tables, the link tables in their four observation forms, region, gene and junction
counts (the tables grown from their smallest size) and row export, walked by a child process (tests/support/hap_tour_worker.py) per fill
byte: context 1 runs set A, then the smaller set B; context 2 runs B alone.

Every array of all three walks is compared with the plain-Python restatements under tests/*ref.py — dtype, shape and bytes, no tolerance:
they are integers and text —, B after A with B in a fresh context, and the three children's files with each other.  Each stop names the
kernel labels it must have reached (haptour.STOPS); a mis-wired stop fails.  The row texts are compared with decode.vcf_rows fed with the
engine's own probabilities, sites and alt_info, the candidates with the CPU oracle's, the kept count with tests/keepref.py.

A child runs under timeout=300: a cap that ends a hang, not a measurement.  Measured on the MI355X: the unpoisoned child takes
1.4 s of wall time, the poisoned ones 1.3 s each (process start, library load and the first allocations are
most of it).

The tour found no mismatch: on the commit that added it all four cases pass with the library as it stands.  That it can fail was tried once
with a library whose counter_table clears half of each table: all four cases fail — unpoisoned, 1A/allele_counts_la/counts holds the counts
of the stop before on top of its own (from index 492: 34, 17, 5 where 18, 10, 4 are due), and under fill 1 1A/counts/counts holds
0x01010101 plus the count from index 540 on."""
import os
import re
import signal
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import haptour as T
from tests import keepref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = [None, 1, 255]
WALKS = (("1A", "A"), ("1B", "B"), ("2B", "B"))
DEAD_STATUS = (134, 139, 124, 137)

_dead = []                                                    # the fill of a child that died: no later case starts anything on the GPU
_files = {}                                                   # fill -> its .npz, for the cross-child case


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("hap_poison"))


def _child(fill, out_dir):
    """Run one child (never two at a time: subprocess.run waits) and return its arrays."""
    if os.environ.get("C3R_POISON"):
        pytest.skip("already inside a poisoned run")
    if _dead:
        pytest.fail("not started: an earlier child died (fill %r)" % (_dead[0],))
    path = os.path.join(out_dir, "tour_%s.npz" % ("unset" if fill is None else fill))
    env = dict(os.environ) if fill is None else dict(os.environ, C3R_POISON=str(fill))
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, "-m", "tests.support.hap_tour_worker", path], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _dead.append(fill)
        pytest.fail("the child did not end within its time limit: %s" % str(e.output)[-2000:])
    print("fill %r: the child took %.1f s" % (fill, time.time() - t0))
    if r.returncode < 0 or r.returncode in DEAD_STATUS or "illegal memory access" in r.stdout:
        _dead.append(fill)
        what = signal.Signals(-r.returncode).name if r.returncode < 0 else "status %d" % r.returncode
        pytest.fail("the child died (%s): %s" % (what, r.stdout[-3000:]))
    assert r.returncode == 0, r.stdout[-3000:]
    _files[fill] = path
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _family(label):
    """A kernel label without the suffixes of its siblings: k_haplotag_alleles_rs_w -> k_haplotag_alleles."""
    return re.sub(r"(_la|_ra|_rs)?(_w)?(_direct)?$", "", label)


def _same(key, got, want):
    assert got.dtype == want.dtype, (key, got.dtype, want.dtype)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        flat = np.flatnonzero(got.reshape(-1) != want.reshape(-1)) if got.dtype.names is None else np.flatnonzero(got != want)
        raise AssertionError("%s: %d elements differ, first at %s: got %s, expected %s" % (key, len(flat), flat[:8].tolist(), got.reshape(-1)[flat[:8]].tolist(),
                                                                                       want.reshape(-1)[flat[:8]].tolist()))


def _check_rows(walk, which, got):
    """The rows stop: the candidates are the oracle's; every way rows leave the device gives decode.vcf_rows' text on the engine's own arrays."""
    g = lambda k: got["%s/rows/%s" % (walk, k)]
    sites, toks, probs = g("sites"), g("tokens"), g("probs")
    from clair3_rna_amd import altinfo
    snv = T.inputs(which)["snv"]
    lines = altinfo.format_lines(T.CTG, sites, g("raw"), toks, snv["rs_plain"], snv["ref"], 1)
    assert lines == T.oracle_rows(which)[0], (walk, "candidate lines differ from the oracle's")
    rows_all, rows_noref = T.rows_from(which, sites, g("raw"), toks, probs)
    assert len(rows_noref) < len(rows_all), (walk, "no RefCall row: drop_ref_calls drops nothing")
    for k in ("snap_all", "call_rows"):
        assert g(k).tobytes() == T.text(rows_all).tobytes(), (walk, k)
    for k in ("snap_all_noref", "snap_drop", "snap_device_reads", "call_rows_noref"):
        assert g(k).tobytes() == T.text(rows_noref).tobytes(), (walk, k)
    kept = keepref.keep(probs, [chr(bytes(s)[16]) for s in sites["ref33"]])
    owner = np.repeat(np.arange(len(sites)), sites["n_tok"])
    assert g("snap_drop_info").tolist() == [int(kept.sum()), int(sites["n_tok"][kept].sum()), int(((toks["indel"] != 0) & kept[owner]).sum())], walk
    assert g("snap_all_info")[0] == len(sites) and g("snap_all_info")[2] == int((toks["indel"] != 0).sum()), walk


@pytest.mark.parametrize("fill", FILLS, ids=["unset", "fill1", "fill255"])
def test_the_tour_equals_the_restatements_on_fresh_poisoned_and_reused_buffers(fill, out_dir):
    got = _child(fill, out_dir)
    row_fields = sorted(k.split("/", 2)[2] for k in got if k.startswith("1A/rows/"))
    for walk, which in WALKS:
        want = dict(T.expected(which))
        names = [name for name, _ in T.STOPS]
        # every stop ran, reached the kernels it names and wrote exactly the restatement's arrays
        assert sorted({k.split("/")[1] for k in got if k.startswith(walk + "/")}) == sorted(names), walk
        for name, kernels in T.STOPS:
            seen = got["%s/%s/kernels" % (walk, name)].tolist()
            assert set(kernels) <= set(seen), (walk, name, kernels, seen)
            others = [k for k in seen if k not in kernels and _family(k) in {_family(x) for x in kernels}]
            assert not others, (walk, name, "the stop also ran a sibling of its kernel", others)
        fields = sorted(k[len(walk) + 1:] for k in got if k.startswith(walk + "/") and not k.endswith("/kernels") and k.split("/")[1] != "rows")
        assert fields == sorted(want), (walk, sorted(set(fields) ^ set(want)))
        for key in fields:
            _same("%s/%s" % (walk, key), got["%s/%s" % (walk, key)], want[key])
        assert sorted(k.split("/", 2)[2] for k in got if k.startswith(walk + "/rows/")) == row_fields
        _check_rows(walk, which, got)
    # B after A is B in a fresh context, byte for byte (the row stop's arrays and the labels too)
    after = sorted(k[3:] for k in got if k.startswith("1B/"))
    assert after == sorted(k[3:] for k in got if k.startswith("2B/"))
    for key in after:
        _same("1B against 2B: " + key, got["1B/" + key], got["2B/" + key])


def test_the_three_children_wrote_the_same_arrays(out_dir):
    """Unpoisoned, filled with 0x01 and filled with 0xff: no array of any walk depends on what a fresh allocation holds."""
    if os.environ.get("C3R_POISON"):
        pytest.skip("already inside a poisoned run")
    if _dead:
        pytest.fail("not started: an earlier child died (fill %r)" % (_dead[0],))
    assert sorted(_files, key=str) == sorted(FILLS, key=str), "a child of the cases above left no file: %s" % sorted(_files, key=str)
    base = np.load(_files[None])
    for fill in FILLS[1:]:
        other = np.load(_files[fill])
        assert sorted(base.files) == sorted(other.files)
        for key in base.files:
            _same("fill %d against unset: %s" % (fill, key), other[key], base[key])
