"""Cache policy of the LSTM kernels' global memory traffic, read from the gfx950 assembly of c3r_lib.hip as tests/test_lstm_isa.py does
(no GPU needed; skipped without hipcc).  y1 is written once by layer 1 and read once by layer 2, 6.8 GB per chr20 pass against an L2 of
4 MB per XCD that layer 2's weights nearly fill: the single-use streams carry the non-temporal bit, the weights must not."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
L1 = "_ZN3c3r10k_lstm1_rsILi18ELb0ELb0EE"          # k_lstm1_rs<18, false, false>
L2 = "_ZN3c3r11k_lstm2_w16ILi0ELb0EE"              # k_lstm2_w16<0, false>


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa_streams") / "c3r_lib.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Wno-unused-function",
                           os.path.join(ROOT, "clair3_rna_amd", "csrc", "c3r_lib.hip"), "-o", out])
    lines = open(out).read().split("\n")

    def get(prefix):
        start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(":")[0].startswith(prefix) and ":" in l)
        end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
        return [l.split(";")[0].strip() for l in lines[start + 1:end] if l.strip() and not l.strip().startswith(";")]

    return get


def _nt(line):
    return re.search(r"\bnt\b", line) is not None


def test_layer2_streams_y1_past_l2_and_keeps_its_weights(body):
    b = body(L2)
    dma = [l for l in b if l.startswith("global_load_lds_dwordx4")]
    # the prologue's 8 rows per wavefront and the time loop's 16 rows per DMA wavefront
    assert len(dma) == 24 and all(_nt(l) for l in dma), [l for l in dma if not _nt(l)]
    weights = [l for l in b if l.startswith("global_load_dwordx4")]
    assert len(weights) >= 250 and not any(_nt(l) for l in weights), [l for l in weights if _nt(l)]
    a4 = [l for l in b if l.startswith("global_store_dwordx4")]
    assert len(a4) == 8 and all(_nt(l) for l in a4), a4                           # a4part: 2 subtiles x 4 site blocks


def test_layer1_y1_stores_are_non_temporal(body):
    b = body(L1)
    y1 = [l for l in b if l.startswith("global_store_dwordx2")]
    # hi and lo plane x 2 site blocks x the two time loops
    assert len(y1) == 8 and all(_nt(l) for l in y1), y1
    weights = [l for l in b if l.startswith("global_load_dwordx4")]
    assert len(weights) == 20 and not any(_nt(l) for l in weights), weights      # 10 k-groups x (hi, lo), once, before the time loop
