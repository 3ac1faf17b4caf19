"""What the compiler makes of the two headline LSTM kernels, read from the gfx950 assembly of c3r_lib.hip (no GPU needed; skipped
without hipcc).  The source can say "double-buffered" or "never v_fma_mixlo_f16" and the binary can disagree — it did — so the
properties that the kernels' speed rests on are asserted on the instruction stream itself.  Every threshold is the shipped binary's
count; the value of the build before this guard existed stands beside it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
L1 = "_ZN3c3r10k_lstm1_rsILi18ELb0ELb0EE"          # k_lstm1_rs<18, false, false>
L2 = "_ZN3c3r11k_lstm2_w16ILi0ELb0EE"              # k_lstm2_w16<0, false>


@pytest.fixture(scope="session")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa") / "c3r_lib.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Wno-unused-function",
                           os.path.join(ROOT, "clair3_rna_amd", "csrc", "c3r_lib.hip"), "-o", out])
    text = open(out).read()
    lines = text.split("\n")

    def body(prefix):
        start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(":")[0].startswith(prefix) and ":" in l)
        end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
        return [l.strip() for l in lines[start + 1:end] if l.strip() and not l.strip().startswith(";")]

    def meta(prefix, key):
        m = re.search(r"\.name:\s+%s\S*\n(?:\s+\.\w+:.*\n)*?\s+\.%s:\s+(\d+)" % (re.escape(prefix), key), text)
        assert m, (prefix, key)
        return int(m.group(1))

    return body, meta


def _count(body, pattern):
    rx = re.compile(pattern)
    return sum(1 for l in body if rx.match(l))


def _l1_blocks(body):
    """The K loops of the ordinary time loop's two 32-site blocks: from the MFMA that starts an accumulator (C = 0) to the block's last
    MFMA, 28 MFMAs each (the loop for counts beyond one f16 has more per block and is left out)."""
    blocks, i = [], 0
    while i < len(body):
        if body[i].startswith("v_mfma") and body[i].endswith(", 0"):
            j = i
            while j < len(body) and not body[j].startswith("v_exp_f32"):
                j += 1
            last = max(k for k in range(i, j) if body[k].startswith("v_mfma"))
            blk = body[i:last + 1]
            if _count(blk, r"v_mfma") == 28:
                blocks.append(blk)
            i = j
        else:
            i += 1
    return blocks


def test_layer1_k_loop_waits(isa):
    body, _ = isa
    blocks = _l1_blocks(body(L1))
    assert len(blocks) == 2, len(blocks)
    for b in blocks:
        reads = _count(b, r"ds_read_b(128|64) ")
        assert reads >= 17, reads                                              # shipped: 17 — the block's 18 B fragments are read inside it, the first sits above
        assert _count(b, r"s_waitcnt .*lgkmcnt\(0\)") == 0                      # before: 18 per block, one full LDS round trip in front of every MFMA group
        # waits that leave the next group's two reads in flight, alone or sharing an instruction with the first block's vmcnt chain for
        # the weights (that chain, 19 waits, stays: one wait before the time loop instead of it was measured and did not pay)
        assert _count(b, r"s_waitcnt (vmcnt\(\d+\) )?lgkmcnt\([23]\)") >= 14    # shipped: 15 in each block


def test_layer2_weight_addresses_are_scalar(isa):
    body, _ = isa
    b = body(L2)
    assert _count(b, r"v_mov_b64") == 0                                         # before: 64
    assert _count(b, r"v_add_co_u32") == 0 and _count(b, r"v_addc_co_u32") == 0  # before: 97 + 97
    loads = [l for l in b if l.startswith("global_load_dwordx4")]
    vector_base = [l for l in loads if not re.search(r", s\[\d+:\d+\]", l)]
    # SGPR base + one lane-offset VGPR in the time loops; the four that remain belong to the last step's L4 contribution after them
    assert len(loads) >= 250 and len(vector_base) <= 4, (len(loads), len(vector_base))        # before: all 284 on 64-bit VGPR addresses


@pytest.mark.parametrize("kernel,cells", [(L1, 16), (L2, 40)], ids=["k_lstm1_rs", "k_lstm2_w16"])
def test_cell_update_instructions(isa, kernel, cells):
    """cells: cell updates in the kernel's text (layer 1: 4 cells x 2 blocks x 2 time loops; layer 2: 8 cells x (3 + 2) tiles, one body per
    wavefront kind)."""
    body, _ = isa
    b = body(kernel)
    assert _count(b, r"v_pk_fma_f32") == 0 and _count(b, r"v_pk_add_f32") == 0  # before: 16 (layer 1) and 40 (layer 2) v_pk_fma_f32
    assert _count(b, r"v_fma_mix(lo|hi)_f16") == 0                              # before: 24 and 60 — h evaluated three times
    assert _count(b, r"v_fma_mix_f32") == cells                                 # h - f16(h): one per cell, reading the packed half directly
    assert _count(b, r"v_rcp_f32") == 3 * cells and _count(b, r"v_exp_f32") == 5 * cells
    assert _count(b, r"v_min_f32") == 3 * cells                                 # before: 4 per cell


def test_no_scratch_and_register_budget(isa):
    _, meta = isa
    assert meta(L1, "private_segment_fixed_size") == 0 and meta(L2, "private_segment_fixed_size") == 0
    assert meta(L1, "vgpr_count") <= 128                                        # four wavefronts per SIMD
    assert meta(L2, "vgpr_count") <= 256
