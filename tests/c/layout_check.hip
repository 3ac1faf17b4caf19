// Host-side checks of K0's counter layout (clair3_rna_amd/csrc/reads_kernels.hpp, cnt_at) and of the giant spans' slice arithmetic
// (pileup_kernels.hpp, giant_slices / giant_slice): compiled by hipcc, runs without a GPU.
//   * a permutation of every block of 1024 bins (no two bins share a counter, none leaves its block: the host sizes the array in whole blocks)
//   * a group of four bins stays four consecutive, 16-byte-aligned words in bin order (k_bin_scan reads it with one load per thread)
//   * neighbouring groups lie at least a cache line (128 bytes) apart — the point of the layout: the bins of one locus are neighbours
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../clair3_rna_amd/csrc/reads_kernels.hpp"
#include "../../clair3_rna_amd/csrc/export_kernels.hpp"

// The thresholds that tests/test_gpu_deep_routes.py sizes its cases by: which kernel builds a span, and how its indel alleles are counted
#define ROUTE_CONST(expr, what) static_assert(expr, what " changed: update tests/test_gpu_deep_routes.py (its brackets and case sizes)")
ROUTE_CONST(c3r::DEEP_MIN_RECORDS == 2048, "DEEP_MIN_RECORDS, the records from which a span is k_fused_deep's,");
ROUTE_CONST(c3r::SPLIT_MIN_RECORDS == 8192, "SPLIT_MIN_RECORDS, the records from which a span is giant,");
ROUTE_CONST(c3r::DEEP_EV_LDS == 3072, "DEEP_EV_LDS, the events of k_fused_deep's LDS store,");
ROUTE_CONST(c3r::DEEP_EV_LDS * sizeof(c3r::EvRec) / 8 == 9216, "LEAD_CAP (tile_columns: sizeof(M.ev) / 8), the events counted by first-of-allele slots in global buckets,");
ROUTE_CONST(sizeof(c3r::TileMem<C3R_CH, c3r::DEEP_EV_LDS>::ev) / 8 == 9216, "LEAD_CAP (tile_columns: sizeof(M.ev) / 8)");
ROUTE_CONST(c3r::EV_HASH_MIN == 1024, "EV_HASH_MIN, the events from which k_fused_tiles hashes,");
ROUTE_CONST(c3r::DEEP_EVG_CAP == 49152, "DEEP_EVG_CAP, the events of a workgroup's arrival-order buffer,");
ROUTE_CONST(c3r::TileMem<C3R_CH>::EV_LDS == 192 && c3r::TileMem<C3R_CH_PHASED>::EV_LDS == 0, "TileMem::EV_LDS, the events of k_fused_tiles' LDS store,");
ROUTE_CONST(c3r::GIANT_SLICE == 4096, "GIANT_SLICE, the records of a slice at the natural thresholds (the tests force 64),");
ROUTE_CONST(c3r::GIANT_MAX_HELP == 32, "GIANT_MAX_HELP, the slices of one span,");
ROUTE_CONST(c3r::GIANT_SLOTS == 256, "GIANT_SLOTS, the giant spans of a scan that are sliced,");
ROUTE_CONST(c3r::FUSE_IN == 224 && c3r::TILE == 256 && C3R_FLANK == 16, "FUSE_IN / TILE / C3R_FLANK, the positions of a span,");
ROUTE_CONST(c3r::OP_CHOP == 30, "OP_CHOP, the positions of one record,");

// The limits of c3r_load_reads that tests/test_gpu_load_edges.py and tests/test_load_edges_ref.py size their cases by (tests/helpers.py holds the same numbers)
#define LOAD_CONST(expr, what) static_assert(expr, what " changed: update tests/helpers.py (the load-edge generators), tests/test_load_edges_ref.py and tests/test_gpu_load_edges.py")
LOAD_CONST(c3r::HB == 1024 && c3r::HB_LOG == 10, "HB, the slots of k_prep's LDS hash,");
LOAD_CONST(c3r::HB_PROBES == 16, "HB_PROBES, the places a bin may take in that hash,");
LOAD_CONST(c3r::WG_TAB_PAIRS == 510 && c3r::WG_TAB_WORDS * 4 == 4096, "WG_TAB_PAIRS, the bins of a workgroup's slab (above it the second pass counts again),");
LOAD_CONST(c3r::PREP_READS == 16 && c3r::PREP_THREADS == 256 && c3r::PREP_GRP == 16, "PREP_READS, the reads of a k_prep workgroup,");
LOAD_CONST(c3r::PM_BLK == 1024, "PM_BLK, the reads of a k_prefmax_bins block,");
LOAD_CONST(c3r::BS_BLK == 4096, "BS_BLK, the bins of a k_bin_scan block,");
LOAD_CONST(c3r::BIN_END_GUESS == (1 << 21), "BIN_END_GUESS, how far beyond the last read's start the bin table is sized before the ends are known,");
LOAD_CONST(c3r::BIN_SHIFT == 5 && c3r::CBIN_SHIFT == 3, "BIN_SHIFT / CBIN_SHIFT, the positions of a bin (32) and the bins of a coarse bin (8),");

// The scans' control blocks (pileup_kernels.hpp: ScanCtl + ScanCtlLayout for c3r_ctx::d_lb, ColCtl for ::d_small).  The kernels take pointers to single
// words and the host reads the blocks back by field: every field stays on the byte it had when the host addressed it by number.
#define CTL_AT(S, field, off) static_assert(offsetof(c3r::S, field) == off, #S "::" #field " has moved")
static_assert(sizeof(c3r::ScanCtl) == 64 && sizeof(c3r::ColCtl) == 64, "the control blocks' heads are 64 bytes");
CTL_AT(ScanCtl, ticket_ranges, 0);  CTL_AT(ScanCtl, ticket_alleles, 4); CTL_AT(ScanCtl, n_cand, 8);        CTL_AT(ScanCtl, n_tok, 12);
CTL_AT(ScanCtl, overflow, 16);      CTL_AT(ScanCtl, n_listed, 20);      CTL_AT(ScanCtl, ev_cursor, 24);    CTL_AT(ScanCtl, ev_overflow, 32);
CTL_AT(ScanCtl, rows_out, 36);      CTL_AT(ScanCtl, ticket_order, 40);  CTL_AT(ScanCtl, n_deep, 44);       CTL_AT(ScanCtl, ticket_deep, 48);
CTL_AT(ScanCtl, n_giant, 52);       CTL_AT(ScanCtl, n_help, 56);        CTL_AT(ScanCtl, ticket_walk, 60);
CTL_AT(ColCtl, ev_cursor, 0);       CTL_AT(ColCtl, ev_overflow, 8);     CTL_AT(ColCtl, n_cand, 12);        CTL_AT(ColCtl, n_tok, 16);
CTL_AT(ColCtl, n_tile_list, 20);    CTL_AT(ColCtl, n_tile_list2, 24);   CTL_AT(ColCtl, tok_written, 28);   CTL_AT(ColCtl, tok_lost, 32);
CTL_AT(ColCtl, unused, 36);
// Row export's control block (export_kernels.hpp: RowCtl for c3r_ctx::d_rowctl and its host mirror); the packers take &n_recs as counters[0], [1]
static_assert(sizeof(c3r::RowCtl) == 64, "the row-export control block is 64 bytes");
CTL_AT(RowCtl, n_recs, 0);          CTL_AT(RowCtl, n_bytes, 8);         CTL_AT(RowCtl, n_keep, 16);        CTL_AT(RowCtl, export_toks, 20);
// (k_order_spans and k_tile_tokens write totals[0] and totals[1] through one pointer)
static_assert(offsetof(c3r::ScanCtl, n_tok) == offsetof(c3r::ScanCtl, n_cand) + 4 && offsetof(c3r::ColCtl, tok_lost) == offsetof(c3r::ColCtl, tok_written) + 4, "totals[0], [1]");
static_assert(c3r::EV_OVF_SCRATCH == 1 && c3r::EV_OVF_DEPTH16 == 2, "EvOverflow bits");
static_assert(c3r::FUSED_OVF_SHARD == 1 && c3r::FUSED_OVF_ORDER_TABLES == 4 && c3r::FUSED_OVF_TOKEN_LOST == 8, "FusedOverflow bits");
static_assert(c3r::TICKET_Q == 16 && c3r::TICKET_STRIDE == 64 && c3r::ALLOC_SHARDS == 16 && c3r::ALLOC_STRIDE == 32, "ticket / allocator words, 256 bytes apart");
constexpr bool scan_ctl_layout_ok(int nblk) {
    const c3r::ScanCtlLayout L(nblk);
    const size_t alloc = 64 + (size_t)c3r::TICKET_Q * c3r::TICKET_STRIDE * 4, head = alloc + (size_t)c3r::ALLOC_SHARDS * c3r::ALLOC_STRIDE * 8;
    return L.ticket == 64 && L.alloc == alloc && L.lb_ranges == head && L.lb_order == head + (size_t)nblk * 8 && L.lb_runs == head + (size_t)nblk * 16 &&
           L.bytes == 64 + (size_t)c3r::TICKET_Q * c3r::TICKET_STRIDE * 4 + (size_t)c3r::ALLOC_SHARDS * c3r::ALLOC_STRIDE * 8 + (size_t)nblk * 24;
}
static_assert(scan_ctl_layout_ok(1) && scan_ctl_layout_ok(2) && scan_ctl_layout_ok(257) && scan_ctl_layout_ok(8191), "ScanCtlLayout");

int main() {
    const uint32_t N = 8 * 1024;
    std::vector<int> seen(N, 0);
    for (uint32_t b = 0; b < N; ++b) {
        const uint32_t i = c3r::cnt_at(b);
        if (i >= N || (i & ~1023u) != (b & ~1023u)) { printf("bin %u leaves its block: %u\n", b, i); return 1; }
        if (seen[i]++) { printf("two bins on counter %u\n", i); return 1; }
        if ((i & 3u) != (b & 3u) || c3r::cnt_at(b & ~3u) + (b & 3u) != i) { printf("group of bin %u is not contiguous\n", b); return 1; }
    }
    if (C3R_CNT_SWZ)
        for (uint32_t b = 0; b + 4 < N; b += 4) {
            if ((b & 1023u) == 1020u) continue;                       // (the next group opens the next block)
            const long d = (long)c3r::cnt_at(b + 4) - (long)c3r::cnt_at(b);
            if ((d < 0 ? -d : d) * 4 < 128) { printf("groups %u and %u share a cache line\n", b / 4, b / 4 + 1); return 1; }
        }
    // the slices of a giant span's records (k_deep_walk) and events (k_deep_alleles): 1 .. GIANT_MAX_HELP of them, a partition of [0, n) in order
    const int ns[] = {1, 2, 63, 64, 65, 4095, 4096, 4097, 8192, 131071, 131072, 131073, 264960, 655904, 12582912, 2147483000, 2147483646};
    const int slices[] = {1, 64, 4096, 16384};
    for (int n : ns)
        for (int sl : slices) {
            const int G = c3r::giant_slices(n, sl);
            if (G < 1 || G > c3r::GIANT_MAX_HELP || (G < c3r::GIANT_MAX_HELP && (long long)G * sl < n)) { printf("n %d slice %d: %d slices\n", n, sl, G); return 1; }
            int at = 0;
            for (int k = 0; k < G; ++k) {
                int lo, hi;
                c3r::giant_slice(n, k, G, lo, hi);
                if (lo < hi) { if (lo != at) { printf("n %d G %d: slice %d starts at %d, not %d\n", n, G, k, lo, at); return 1; } at = hi; }
                else if (lo < at) { printf("n %d G %d: empty slice %d before the end\n", n, G, k); return 1; }
            }
            if (at != n) { printf("n %d G %d: the slices end at %d\n", n, G, at); return 1; }
        }
    printf("cnt_at ok (swizzle %d), giant slices ok, scan control blocks ok\n", (int)C3R_CNT_SWZ);
    return 0;
}
