// hapregion_kernels.hpp — k_hap_region_counts: reads by haplotype and phase set per interval of a sorted interval table (c3r_hap_region_counts:
// the exons or genes of a BED file), from the reads, tags and phase sets that c3r_load_reads left on the device.  Included by c3r_lib.hip only.
//
// What it is for: allele-specific expression — how many reads of each haplotype a gene or an exon is expressed from — without writing the
// haplotagged BAM and reading it again.  The rule (`hap_regions`) is stated in include/c3r.h and restated, independently of this file, by
// tests/hapregionref.py.
//
// The shape of k_hap_counts: 16 lanes per read, no LDS, no workgroup barrier, whole groups leave early — past n_reads, a read that read
// preparation does not keep (read_kept), or no region that can overlap the read's span.  One walk (walk_plain_ops / walk_serial_ops) whose
// callback takes the M and D ops.  For an op [x, x + len) of the lane:
//   hi = the first region with start >= x + len, k = the last region with start <= x, and the candidates are [first_open[k], hi) — [0, hi)
//   when no region starts at or before x —, filtered by end > x.  first_open[j] (the host computes it) is the smallest i <= j with
//   end_i > start_j, so a region below first_open[k] ends at or before start_k <= x: the candidates hold every region the op overlaps.
// A (read, region) pair is counted by the op that holds the read's first covered position inside the region: the region overlaps the op and
// starts at or behind the end of the read's nearest earlier M / D op (there is none for the first one).  The plain walk's lane finds that end by
// stepping back over the I / S / N ops before its own; the serial walk's one lane carries it.  One relaxed, agent-scope add per pair: integer
// sums, arrival order never shows.  Nothing is reduced across lanes: no shuffle follows the walk.
//
// The table on the device is the caller's with one change: c3r_hap_region_counts puts the number of the region's rows into reserved[0 .. 2] of
// its copy, so that a candidate is one 16-byte load.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "haplotag_kernels.hpp"

namespace c3r {

// a region as the kernel loads it: c3r_hap_region_t with the count of its rows above the strand byte
struct DevHapRegion { int32_t start, end, row_off; uint32_t strand_rows; };
static_assert(sizeof(DevHapRegion) == 16 && sizeof(c3r_hap_region_t) == 16, "region layout");

struct HapRegionArgs : ReadArgs {
    const uint32_t *tags;                     // [n_reads] k_haplotag's: tag in the low two bits
    const int32_t *read_ps;                   // [n_reads] k_haplotag's: the set the tag was decided in, -1 when the tag is 0
    int32_t min_mq, excl_flags;               // the voters: read_kept
    const DevHapRegion *regions; int32_t n_regions;       // sorted by (start, end)
    const int32_t *first_open;                // [n_regions] smallest i <= j with end_i > start_j
    const int32_t *row_ps;                    // the regions' phase sets: region j's at [row_off, row_off + rows), strictly increasing
    int32_t stranded;                         // 0 off, 1 same, 2 reverse
    uint32_t *region_counts;                  // [n_regions][2] untagged, tagged in another set; zero on entry
    uint32_t *row_counts;                     // [n_rows][2] haplotype 1, 2; zero on entry
};

// first region of [lo, hi) with start >= p (hi: none)
__device__ __forceinline__ int region_lower(const DevHapRegion *regions, int lo, int hi, long long p) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)regions[mid].start < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

constexpr long long HAP_REGION_NO_END = INT64_MIN;         // no earlier covering op

__global__ __launch_bounds__(PREP_THREADS) void k_hap_region_counts(const HapRegionArgs a) {
    const GroupAt g;
    const int gl = g.gl, i = g.i;
    if (i >= a.n_reads) return;
    const DevRead d = a.reads[i];
    if (!read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags) || d.end <= d.pos) return;
    // the regions that can overlap [pos, end): those below the first that starts at or behind `end`, from the first one open at the last start <= pos
    const int r_hi = region_lower(a.regions, 0, a.n_regions, (long long)d.end);
    const int r_k = region_lower(a.regions, 0, r_hi, (long long)d.pos + 1) - 1;
    if ((r_k >= 0 ? a.first_open[r_k] : 0) >= r_hi) return;
    const bool serial = a.serial[i] != 0;
    const ReadInfo R(d, i, a.cigars, 0);
    const uint32_t tag = a.tags[i] & 3u;
    const int32_t set = tag ? a.read_ps[i] : -1;
    const uint32_t own = (d.flag & 16u) ? 2u : 1u, want = a.stranded == 1 ? own : 3u - own;      // the region strand that counts this read
    // every region that [x, x + len) overlaps and that starts at or behind prev_end
    auto count_op = [&](long long x, uint32_t len, long long prev_end) __attribute__((always_inline)) {
        const int hi = region_lower(a.regions, r_k < 0 ? 0 : r_k, r_hi, x + (long long)len);
        const int k = region_lower(a.regions, r_k < 0 ? 0 : r_k, hi, x + 1) - 1;
        for (int j = k >= 0 ? a.first_open[k] : 0; j < hi; ++j) {
            const DevHapRegion e = a.regions[j];
            if ((long long)e.end <= x || (long long)e.start < prev_end) continue;
            const uint32_t strand = e.strand_rows & 255u;
            if (a.stranded != 0 && strand != 0u && strand != want) continue;
            uint32_t *word = a.region_counts + 2 * (size_t)j;          // untagged
            if (tag) {
                word += 1;                                             // tagged in a set that is none of the region's rows
                int lo = e.row_off, top = e.row_off + (int)(e.strand_rows >> 8);
                while (lo < top) {
                    const int mid = (lo + top) >> 1;
                    const int32_t p = a.row_ps[mid];
                    if (p == set) { word = a.row_counts + 2 * (size_t)mid + (tag - 1u); break; }
                    if (p < set) lo = mid + 1; else top = mid;
                }
            }
            __hip_atomic_fetch_add(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (!serial) {
        uint32_t k_op = (uint32_t)gl;                                  // the raw index of the op the callback holds: gl, gl + 16, ... in the walk's order
        walk_plain_ops(R, gl, [&](uint32_t op, uint32_t len, long long x, uint32_t, const OpCtx &) __attribute__((always_inline)) {
            const uint32_t k = k_op;
            k_op += PREP_GRP;
            if (op != C3R_CIG_M && op != C3R_CIG_D) return;
            // the end of the nearest earlier M / D op: x less the introns between (I, S and H consume no reference)
            long long prev_end = HAP_REGION_NO_END, gap = 0;
            for (uint32_t b = k; b > 0; --b) {
                const uint32_t c = R.cig[b - 1], o = fold_op(c);
                if (o == C3R_CIG_M || o == C3R_CIG_D) { prev_end = x - gap; break; }
                if (o == C3R_CIG_N) gap += (long long)(c >> 4);
            }
            count_op(x, len, prev_end);
        });
    } else if (gl == 0) {
        long long prev_end = HAP_REGION_NO_END;
        (void)walk_serial_ops(R, [&](uint32_t op, uint32_t len, long long x, uint32_t, const OpCtx &) __attribute__((always_inline)) {
            if (op != C3R_CIG_M && op != C3R_CIG_D) return;
            count_op(x, len, prev_end);
            prev_end = x + (long long)len;
        });
    }
}

}  // namespace c3r
