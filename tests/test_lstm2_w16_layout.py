import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lstm2_w16_packing_feeds_each_weight_to_its_gate_row(tmp_path):
    """k_lstm2_w16's layer-2 and fused-L4 packing (csrc/net_pack.hpp: pack_lstm2_w16, pack_l4_w16) and its bias rows (csrc/net_kernels.hpp: w16_bias_row): every Keras weight,
    read at the address the kernel loads it from, sits in the lane and element that v_mfma_f32_16x16x32_f16 multiplies into the
    accumulator row the kernel reads as that weight's gate and unit (or L4 output), exactly once, in both directions.  Host-side (hipcc, no GPU)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "w16_layout_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-function",
                           os.path.join(ROOT, "tests", "c", "w16_layout_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "layer 2 ok" in out.stdout and "L4 ok" in out.stdout, out.stdout + out.stderr
