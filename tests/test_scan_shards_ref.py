"""The inputs of tests/test_gpu_scan_shards.py held on their floors without a GPU.  Those tests force the fused scan's sharded allocator to
grow and repeat by pigeonhole: after a sharded scan that found nothing a shard owns PRIMED_ROWS rows and PRIMED_TOKS token slots, so a scan of
more than 16 x 64 candidates, or of more than 16 x 2048 tokens, cannot fit whichever workgroup takes which span.  Here the tile counts of
their regions and the oracle's candidate and token counts of their read sets are asserted (beside each: what the oracle gave); an input that
drifts below its floor fails here, not silently on the device."""
import numpy as np
import pytest

from tests import helpers as H


def _exp(case, regions):
    c = H.shard_case(*case) if isinstance(case, tuple) else H.shard_case(case)
    return c, H.oracle_regions(c["rs"], c["ref"], regions, **c["okw"])


def test_tile_counts_on_either_side_of_the_switch():
    assert (H.SPAN, H.SHARD_TILES, H.ALLOC_SHARDS) == (224, 4096, 16)
    assert H.scan_tiles([(1, H.DENSE_END)]) == H.SHARD_TILES - 1 and H.scan_tiles([(1, H.SHARD_END)]) == H.SHARD_TILES
    assert H.scan_tiles([H.PRIME_REGION]) >= H.SHARD_TILES and H.PRIME_REGION[1] + 33 <= H.SHARD_REF_LEN
    for n_last, total in ((63, H.SHARD_TILES - 1), (64, H.SHARD_TILES)):
        regs = H.edge_regions(n_last)
        assert len(regs) == 64 and H.scan_tiles(regs) == total and [H.scan_tiles([r]) for r in regs[:-1]] == [64] * 63
        assert all(regs[k][1] + 1 == regs[k + 1][0] for k in range(63))
        assert regs[0][0] <= H.BURST_AT2 and H.BURST_AT + 9000 < regs[-1][0]                  # both bursts lie in regions that the two lists share
    assert all(H.scan_tiles([r]) >= H.SHARD_TILES if kind != "dense" else H.scan_tiles([r]) < 64 for r, kind in H.BATCH_SCANS)


@pytest.mark.parametrize("channels", [18, 30])
@pytest.mark.parametrize("name", ["burst", "burst2"])
def test_burst_has_more_candidates_than_sixteen_primed_shards_hold(name, channels):
    c, exp = _exp((name, channels), [(1, H.SHARD_END)])
    off = H.BURST_AT2 if name == "burst2" else H.BURST_AT
    pos = H.line_positions(exp["lines"])
    assert len(c["rs"].reads) < 200 and off < min(pos) and max(pos) <= off + 9000
    assert len(exp["lines"]) >= 1200 > H.ALLOC_SHARDS * H.PRIMED_ROWS                           # oracle: 1376 candidates at 18 and at 30 channels
    assert H.alt_tokens(exp["lines"]) > (3000 if channels == 18 else 400)                     # oracle: 3706 tokens (18 channels, ONT errors), 464 (30, HiFi)
    # one span of the burst alone is more than a shard holds after a scan of the piles (at most 1.25 x 56 + 64 rows): the second half of the
    # token-only test repeats for rows whatever the tickets do
    assert H.max_span_candidates(exp["lines"]) > 56 + 56 // 4 + 64                             # oracle: 224 (burst) / 209 (burst2) candidates in one span
    # the regions of the edge test cut the burst, and the same candidates come out of them
    if channels == 18:
        per = H.oracle_regions(c["rs"], c["ref"], H.edge_regions(64), **c["okw"])
        assert per["lines"] == exp["lines"] and np.array_equal(per["X"], exp["X"])
        assert per["lines"] == H.oracle_regions(c["rs"], c["ref"], H.edge_regions(63), **c["okw"])["lines"]
        assert exp["lines"] == H.oracle_regions(c["rs"], c["ref"], [(1, H.DENSE_END)], **c["okw"])["lines"]


def test_iupac_base_changes_a_candidate_of_the_phased_burst():
    c, exp = _exp(("burst_iupac", 30), [(1, H.SHARD_END)])
    _c, plain = _exp(("burst", 30), [(1, H.SHARD_END)])
    assert len(exp["lines"]) >= 1200 and len(exp["lines"]) == len(plain["lines"]) and not np.array_equal(exp["X"], plain["X"])


@pytest.mark.parametrize("name, depth, n_piles", [("piles_tile", 1000, 2), ("piles_deep", 2600, 2)])
def test_piles_are_few_candidates_and_many_tokens(name, depth, n_piles):
    c, exp = _exp(name, [(1, H.SHARD_END)])
    assert len(c["rs"].reads) == depth * n_piles
    assert len(exp["lines"]) == n_piles * H.DEEP_PILE_COLS <= H.PRIMED_ROWS                   # 56 candidates: they fit ANY one shard
    assert H.alt_tokens(exp["lines"]) == n_piles * H.DEEP_PILE_COLS * (depth - depth // 10) > 40000 > H.ALLOC_SHARDS * H.PRIMED_TOKS     # 50400 / 131040 tokens
    assert exp["depth"].min() == depth > 216                                                  # (every window is rescaled)
    # records of a span: two per read, one pile per span at most
    assert (2 * depth < 2048) == (name == "piles_tile") and 2 * depth < 8192


def test_wide_pile_outgrows_a_fresh_context():
    c, exp = _exp("wide", [(1, H.SHARD_END)])
    n = H.WIDE_RLEN - 32
    assert len(c["rs"].reads) == H.WIDE_DEPTH and len(exp["lines"]) == n <= H.FRESH_ROWS      # 468 candidates: rows never overflow
    tokens = H.alt_tokens(exp["lines"])
    assert tokens == n * (H.WIDE_DEPTH - H.WIDE_DEPTH // 10) and 10 * tokens >= 12 * H.ALLOC_SHARDS * H.FRESH_TOKS       # 2611440 tokens against 2097152 slots
    per_span = sorted(np.bincount([(p - 1) // H.SPAN for p in H.line_positions(exp["lines"])]).tolist())[-3:]
    assert per_span == [20, 224, 224] and 224 * (H.WIDE_DEPTH - H.WIDE_DEPTH // 10) > H.FRESH_TOKS       # one span overflows a fresh shard wherever it lands
    assert 5 * (per_span[1] + per_span[2]) // 4 >= n                                           # after two such spans met in one shard, everything fits one


def test_batch_scans_hold_what_their_kinds_say():
    c = H.shard_case("batch")
    n = {}
    for region, kind in H.BATCH_SCANS:
        exp = H.oracle_regions(c["rs"], c["ref"], [region], **c["okw"])
        n.setdefault(kind, []).append((len(exp["lines"]), H.alt_tokens(exp["lines"])))
    assert n["prime"] == [(0, 0), (0, 0)]
    assert all(k > 100 for k, _t in n["dense"][:2]) and n["dense"][2] == (H.DEEP_PILE_COLS, H.DEEP_PILE_COLS * 2340)      # oracle: 600 and 776 candidates, then one pile
    assert n["sharded"][0][0] >= 1200 + 2 * H.DEEP_PILE_COLS and n["sharded"][0][1] > 131040    # burst and piles: 1432 candidates
    assert n["sharded"][1] == (2 * H.DEEP_PILE_COLS, 131040)                                   # the piles alone: tokens only
