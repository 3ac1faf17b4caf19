"""The read sets of tests/test_gpu_load_edges.py (and the recount case of tests/test_gpu_load.py) held in their brackets without a GPU: every
generator of tests/helpers.py is rebuilt here and the conditions that make it reach its branch of c3r_load_reads are asserted from the reads'
positions and against the oracle alone — the pigeonhole counts against k_prep's hash and slab, the far end beyond the bin table's first guess,
the pattern in which mpileup's depth cap bites on a coarse-bin edge, and the floors on lines (beside each: what the oracle gave).  A generator
that drifts out of its bracket fails here, not silently on the device."""
import numpy as np
import pytest

from tests import helpers as H


def _rs(recs):
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records(recs)


def test_constants_are_the_ones_the_cases_are_sized_by():
    """(tests/c/layout_check.hip ties the same numbers to the kernels' constants)"""
    assert (H.PREP_READS, H.HB, H.HB_PROBES, H.WG_TAB_PAIRS, H.PM_BLK, H.BS_BLK, H.BIN_END_GUESS, H.OP_CHOP) == (16, 1024, 16, 510, 1024, 4096, 1 << 21, 30)
    assert H.LOAD_CBIN == 8 * H.LOAD_BIN == 256


def test_hash_exhaustion_case_has_more_bins_than_slots_in_every_workgroup():
    ref, recs = H.hash_exhaustion_case()
    assert len(recs) == 2 * H.HASH_LOCI == 3 * H.PREP_READS and [r["pos"] for r in recs] == sorted(r["pos"] for r in recs)
    assert sum(1 for r in recs if "0D" in r["cigar"]) == 2 * (H.HASH_LOCI // 3)               # every third locus takes the serial walk
    whole, starts = H.workgroup_whole_bins(recs), H.workgroup_bins(recs)
    assert whole == [1368, 1368, 1368] and all(w > H.HB for w in whole)                       # the pigeonhole: more bins with a record start than slots
    assert all(s >= w for s, w in zip(starts, whole)) and all(s > H.WG_TAB_PAIRS for s in starts)        # (1384 bins hold a record start; the slab overflows too)
    rs = _rs(recs)
    for channels in (18, 30):
        exp = H.oracle_chunk(rs, ref, 1, 1, len(ref), channels=channels, min_coverage=2)
        assert len(exp["lines"]) > 1200                                                       # oracle: 1368 lines at 18 and at 30 channels
        assert all(H.reads_with_a_line(recs, exp["lines"]))                                   # every read of every workgroup is looked at
        assert set((p - 501) // H.HASH_PITCH for p in H.line_positions(exp["lines"])) == set(range(H.HASH_LOCI))
        if channels == 30:
            assert np.any(exp["X"][:, :, 18:])                                                # (the haplotype channels are in play)
    # the regions of the sub-region scan cut through loci, and every region has lines
    regions = H.hash_exhaustion_regions(len(ref))
    cut = [b for _a, b in regions[:-1] if any(r["pos"] + 100 < b < r["pos"] + H.HASH_RLEN - 100 for r in recs)]
    assert len(regions) == 10 and len(cut) >= 5
    n = [len(H.oracle_chunk(rs, ref, 1, a, b, min_coverage=2)["lines"]) for a, b in regions]
    assert min(n) > 50 and sum(n) > 1200                                                      # oracle: 1368 lines in all, 86 in the last region


def test_slab_overflow_case_compares_every_record_of_the_recounting_workgroups():
    """16 x 41 = 656 bins: above the slab's 510 pairs (the second pass counts again), below the hash's 1024 slots (no exhaustion: that is
    hash_exhaustion_case).  Every record that a recounting workgroup places holds a position inside a compared window."""
    ref, recs = H.slab_overflow_case()
    bins = H.workgroup_bins(recs)
    assert bins == [167, 168, 168, 290, 656, 656, 492]
    recount = [k for k, b in enumerate(bins) if b > H.WG_TAB_PAIRS]
    assert recount == [4, 5] and all(bins[k] < H.HB for k in recount)
    exp = H.oracle_chunk(_rs(recs), ref, 1, 1, len(ref), min_coverage=1)
    assert len(exp["lines"]) > 1800                                                           # oracle: 2124 lines
    seen = np.zeros(len(ref) + 64, bool)
    for p in H.line_positions(exp["lines"]):
        seen[p - 1 - 16:p - 1 + 17] = True                                                    # the 33 positions of the candidate's window
    for k in recount:
        for r in recs[k * H.PREP_READS:(k + 1) * H.PREP_READS]:
            n = H.cigar_ref_len(r["cigar"])
            assert all(seen[r["pos"] + q:r["pos"] + min(q + H.OP_CHOP, n)].any() for q in range(0, n, H.OP_CHOP)), r["pos"]


@pytest.fixture(scope="module")
def regrow():
    ref, recs, near, far = H.regrowth_case()
    return ref, recs, _rs(recs), near, far


def test_regrowth_case_reaches_beyond_the_first_guess(regrow):
    ref, recs, rs, near, far = regrow
    assert len(ref) == 2300000 and len(recs) == 3004 and H.REGROW_SHORT > 2 * H.PM_BLK          # three blocks of k_prefmax_bins
    bridges = [r for r in recs if "N" in r["cigar"]]
    assert recs[:4] == bridges and len(set(r["pos"] for r in bridges)) == 3 and all(r["mapq"] == 7 for r in bridges)
    end = H.readset_end(rs)
    assert end > recs[-1]["pos"] + H.BIN_END_GUESS and end == max(r["pos"] + H.cigar_ref_len(r["cigar"]) for r in bridges)       # 2201140 against 2159132
    assert max(r["pos"] + 50 for r in recs[4:]) <= recs[-1]["pos"] + H.BIN_END_GUESS            # (without the bridging reads, i.e. with min_mq = 10, the guess holds)
    assert (end >> 5) - (recs[0]["pos"] >> 5) > 8 * H.BS_BLK                                     # more than one block of k_bin_scan's coarse chain
    assert far[0] < min(r["pos"] for r in bridges) + 60 + H.BRIDGE_SKIP and far[1] > end and far[1] - far[0] == 600


def test_regrowth_case_lines_near_and_far(regrow):
    ref, recs, rs, near, far = regrow
    kw = dict(min_coverage=2, head_tail=True)
    near_all = H.oracle_chunk(rs, ref, 1, near[0], near[1], **kw)
    assert len(near_all["lines"]) > 1400                                                      # oracle: 1625 lines
    far_all = H.oracle_chunk(rs, ref, 1, far[0], far[1], **kw)
    far_pos = H.line_positions(far_all["lines"])
    assert len(far_pos) >= 4 and all(far[0] <= p <= far[1] for p in far_pos)                  # oracle: 4 lines, all owed to the bridging reads:
    assert H.oracle_chunk(rs, ref, 1, far[0], far[1], min_mq=10, **kw)["lines"] == []         # without them the far region is empty
    near_mq10 = H.oracle_chunk(rs, ref, 1, near[0], near[1], min_mq=10, **kw)
    assert len(near_mq10["lines"]) == len(near_all["lines"]) - 4                              # oracle: 1621 lines
    # the cap of 2 discards the second bridging read on position 1020, in both regions
    far_cap = H.oracle_chunk(rs, ref, 1, far[0], far[1], max_depth=2, **kw)
    assert len(far_cap["lines"]) >= 4 and far_cap["lines"] != far_all["lines"]
    assert H.oracle_chunk(rs, ref, 1, near[0], near[1], max_depth=2, **kw)["lines"] != near_all["lines"]


@pytest.mark.parametrize("far", [False, True], ids=["near", "with_far_read"])
@pytest.mark.parametrize("kind", H.GATE_EDGES)
@pytest.mark.parametrize("first", H.GATE_FIRSTS)
def test_depth_cap_bites_exactly_when_the_enders_reach_the_starters(first, kind, far):
    """The cap K + 2 changes the oracle's lines when the K enders' exclusive end is at or past the M starters' position, and not one position
    before; the cap K + M + 1 never does.  An engine whose max_cover misses the enders on the edge (11 <= 32) would skip the cap where it bites."""
    edge = H.gate_edge(first, kind)
    assert edge % 256 == 0 if kind == "host" else (edge - ((first >> 5) << 5)) % 256 == 0
    for d in H.GATE_DS:
        ref, recs, last = H.gate_case(first, kind, d, far)
        assert len(recs) == 2 + H.GATE_K + H.GATE_M + int(far) and recs[0]["pos"] == first and [r["pos"] for r in recs] == sorted(r["pos"] for r in recs)
        assert sum(1 for r in recs if r["pos"] + H.cigar_ref_len(r["cigar"]) == edge + d) == H.GATE_K and sum(1 for r in recs if r["pos"] == edge) == H.GATE_M
        rs = _rs(recs)
        lines = [H.oracle_chunk(rs, ref, 1, 1, last, min_coverage=2, max_depth=cap)["lines"] for cap in H.GATE_CAPS]
        assert len(lines[2]) >= 2                                              # oracle: 2 / 4 / 4 lines for d = -1 / 0 / +1 (7 with the far read)
        assert (lines[0] != lines[2]) == (d >= 0), (first, kind, d)
        assert lines[1] == lines[2], (first, kind, d)
        if far:
            assert (H.readset_end(rs) >> 8) - (first >> 8) > H.BS_BLK
