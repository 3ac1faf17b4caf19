"""The references of the row-export tests, checked without a GPU: the keep rule of tests/keepref.py never drops a site the Python decoder
prints, and tests/c/row_export_check.hip --host-only (the same rule in C++ against decode.hpp, the generators of its device sections)."""
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import keepref


def test_row_export_check_host_only(tmp_path):
    """The program's host side: its restated keep rule gives the answers the hand-made cases were built for, a case it drops prints no row
    through decode.hpp's vcf_row without show_ref for four alt dictionaries (empty, SNVs, indels, everything tied), and the reference orders
    of its packer section are sorted permutations.  No HIP call is made."""
    exe = H.build_row_export_check(str(tmp_path / "row_export_check"))
    if exe is None:
        pytest.skip("no hipcc")
    out = subprocess.run([exe, "--host-only"], capture_output=True, text=True)
    lines = out.stdout.strip().split("\n")
    assert out.returncode == 0 and len(lines) == 2 and lines[0].startswith("A host:") and all(l.endswith(": ok") for l in lines), out.stdout + out.stderr


def test_keep_rule_gives_the_answers_its_edge_cases_were_built_for():
    centres, probs, expect = keepref.edge_cases()
    got = keepref.keep(probs, centres)
    assert len(got) == 16 * 4 + 4 * 18 + 4 * 23 * 3 + 40
    bad = np.nonzero(got != expect)[0]
    assert len(bad) == 0, [(int(i), centres[i], probs[i].tolist()) for i in bad[:3]]
    assert got.any() and not got.all()


def test_keep_rule_never_drops_a_site_the_decoder_prints():
    """Safety of the rule against the Python decoder: whatever alt_info holds, a site with keep == False prints nothing without show_ref.
    (The converse cannot hold: whether a kept site prints depends on its alt_info.)"""
    from clair3_rna_amd import decode
    c1, p1, _ = keepref.edge_cases()
    c2, p2 = keepref.softmax_cases(6000)
    centres, probs = list(c1) + list(c2), np.concatenate([p1, p2])
    kept = keepref.keep(probs, centres)
    dropped = np.nonzero(~kept)[0]
    assert len(dropped) > 1500 and kept.sum() > 1500, (len(dropped), int(kept.sum()))
    printed_kept = 0
    for i in range(len(centres)):
        ref33 = "A" * 16 + centres[i] + "A" * 16
        for ai in keepref.ALT_INFOS:
            row = decode.vcf_row("chr20", 1000 + i, ref33, ai, probs[i], 2, show_ref=False)
            if not kept[i]:
                assert row is None, (i, centres[i], ai, probs[i].tolist(), row)
            else:
                printed_kept += row is not None
    assert printed_kept > 1000            # (the dictionaries do let kept sites print: the property above is not vacuous)
