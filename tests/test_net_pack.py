import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "net_pack_hashes.json")

# buffers the fixture's commit packed and uploaded but no kernel read: they are gone, and only they may be missing from the output
DROPPED = {"w4h", "w5", "wo", "w1q", "w1s"}


def parse(text):
    """The check program's lines -> {case: {"wlog2": [..], "buffers": {name: [bytes, fnv1a64 hex]}} | {"refused": rc, "message": ..}}"""
    cases = {}
    for line in text.splitlines():
        f = line.split()
        if len(f) < 3:
            continue
        c = cases.setdefault(f[0], {})
        if f[1] == "wlog2":
            c["wlog2"] = [int(v) for v in f[2:5]]
        elif f[1] == "buf":
            c.setdefault("buffers", {})[f[2]] = [int(f[3]), f[4]]
        elif f[1] == "refused":
            c["refused"] = int(f[2])
            c["message"] = " ".join(f[3:])
    return cases


def test_net_pack_bytes_match_the_recorded_hashes(tmp_path):
    """net_pack (csrc/net_pack.hpp) on blobs from a fixed seed — 18 and 30 channels, weights that force three different split-f16 scales,
    magnitudes from 2^-24 to 2^2 with exact zeros (f16 subnormals and rounding, the e4m3 edges), and a NaN that must be refused with
    C3R_EINVAL and its index: every buffer has the size and the FNV-1a hash that tests/golden/net_pack_hashes.json records from the
    packers of the commit named there.  Plain g++ (-Wall -Wextra -Werror: the header has to stay free of ROCm headers), no GPU."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "net_pack_check")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "c", "net_pack_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = parse(out.stdout)
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    assert sorted(got) == sorted(want) == ["c18", "c18_nan", "c18_scales", "c18_wide", "c30"]
    assert got["c18_nan"] == want["c18_nan"] == {"refused": -1, "message": "weight blob holds a non-finite value (index 424242)"}
    s = got["c18_scales"]["wlog2"]
    assert len(set(s) | {12}) == 4, s
    for case, w in want.items():
        if case == "c18_nan":
            continue
        g = got[case]
        assert g["wlog2"] == w["wlog2"], case
        missing = set(w["buffers"]) - set(g["buffers"])
        assert missing <= DROPPED, (case, sorted(missing))
        assert not set(g["buffers"]) & DROPPED, case
        assert set(g["buffers"]) <= set(w["buffers"]), (case, "buffers the fixture does not know", sorted(set(g["buffers"]) - set(w["buffers"])))
        for name, (nbytes, fnv) in g["buffers"].items():
            assert [nbytes, fnv] == w["buffers"][name], (case, name)
