// hapgroup_kernels.hpp — k_hap_group_counts: reads by haplotype and phase set per GROUP of intervals of a sorted interval table
// (c3r_hap_group_counts: the genes of a BED file, each the group of its exons), from the reads, tags and phase sets that c3r_load_reads left
// on the device.  Included by c3r_lib.hip only.
//
// What it is for: allele-specific expression per gene — a read over three exons of one gene is one read of that gene, and a read that lies
// only in the gene's introns is none.  The rule (`hap_groups`) is stated in include/c3r.h and restated, independently of this file, by
// tests/hapgroupref.py.
//
// The shape of k_hap_region_counts: 16 lanes per read, the two CIGAR walks whose callback takes the M and D ops, the candidate intervals of
// an op from first_open and the two searches, and the pair (read, interval) found by the op that holds the read's first covered position
// inside the interval (the prev_end test).  Two things are new.
//
// Exactly one count per (read, group), with no per-read table.  The op that found (read, interval j) counts for j's group only if the read
// covers no position of an EARLIER interval of that group: then j is the first interval of the group that the read covers, and there is
// exactly one such interval.  A group's intervals are disjoint and the table is sorted, so they lie in table order along the reference; the
// host gives every interval `prev`, the previous interval of its group in table order (-1: none).  hg_earlier_hit follows that chain
// backwards while end > read.pos and, beside it, steps backwards over the read's raw ops from the op that found the pair: both sequences
// decrease, so it is one merge — an op that starts at or behind the chain interval's end is dropped for good, an op that ends behind the
// chain interval's start is a hit, else the chain moves on.  Bounded by the chain intervals inside the read's span plus the raw ops; for the
// usual read — the previous M op in the previous exon — the first step answers.  It reads the RAW ops (empty ops cover nothing, = and X
// fold into M, H and P consume nothing), so the serial walk uses it as well, from the read's last op.  One strand per group: a chain
// interval that does not admit the read never occurs.
//
// Aggregation (AGG = true), as k_hap_junction_counts has it.  The count words are one dense table — [n_groups][2], then [n_rows][2] — so
// the LDS stage is one table keyed by the word's index: PREP_THREADS slots (a slot per thread for the clearing and the flush), claimed with
// hj_claim_lds, counted with LDS adds.  After the workgroup's barrier every thread flushes its slot with one relaxed global add if it is
// non-zero.  A word that finds no slot among its HJ_LDS_PROBES is added globally at once.  Every thread reaches every barrier: a group of
// lanes without a read to walk skips the walk, not the kernel.  AGG = false is the same body without LDS and barrier
// (c3r_set_hap_group_direct); the sums are integers, so the tables are identical.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "hapjunction_kernels.hpp"
#include "hapregion_kernels.hpp"

namespace c3r {

// an interval as the kernel loads it: c3r_hap_interval_t with the chain in place of the padding
struct DevHapInterval { int32_t start, end, prev; uint32_t group_strand; };       // group << 2 | strand
static_assert(sizeof(DevHapInterval) == 16 && sizeof(c3r_hap_interval_t) == 16, "interval layout");

struct HapGroupArgs : ReadArgs {
    const uint32_t *tags;                     // [n_reads] k_haplotag's: tag in the low two bits
    const int32_t *read_ps;                   // [n_reads] k_haplotag's: the set the tag was decided in, -1 when the tag is 0
    int32_t min_mq, excl_flags;               // the voters: read_kept
    const DevHapInterval *intervals; int32_t n_intervals;     // sorted by (start, end)
    const int32_t *first_open;                // [n_intervals] smallest i <= j with end_i > start_j
    const int32_t *group_row_off;             // [n_groups + 1] group g's rows: [group_row_off[g], group_row_off[g + 1])
    const int32_t *row_ps;                    // strictly increasing inside a group
    int32_t n_groups, stranded;               // stranded: 0 off, 1 same, 2 reverse
    uint32_t *counts;                         // [2 n_groups + 2 n_rows]: per group untagged, tagged in another set; then per row haplotype 1, 2; zero on entry
};

struct HapGroupLds { unsigned long long key[HJ_LDS]; uint32_t cnt[HJ_LDS]; };     // key: the index of the count word
struct HapGroupNoLds {};

// first interval of [lo, hi) with start >= p (hi: none)
__device__ __forceinline__ int interval_lower(const DevHapInterval *v, int lo, int hi, long long p) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)v[mid].start < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Does the read cover a position of the chain interval `c` or of one before it in the chain?  The raw ops [0, b) lie before reference
// position p (op b - 1 ends there).
__device__ __forceinline__ bool hg_earlier_hit(const DevHapInterval *intervals, const ReadInfo &R, int c, uint32_t b, long long p) {
    long long o_lo = 0, o_hi = 0;             // the M / D op the merge holds
    bool have = false;
    while (c >= 0) {
        const DevHapInterval ce = intervals[c];
        if ((long long)ce.end <= (long long)R.pos) return false;       // this one and every earlier one of the chain end before the read begins
        while (!have || o_lo >= (long long)ce.end) {                   // on to the nearest op that starts before the interval's end
            if (b == 0) return false;
            const uint32_t cg = R.cig[--b], o = fold_op(cg), len = cg >> 4;
            have = false;
            if (o == C3R_CIG_M || o == C3R_CIG_D) { o_hi = p; p -= (long long)len; o_lo = p; have = len != 0u; }
            else if (o == C3R_CIG_N) p -= (long long)len;
        }
        if (o_hi > (long long)ce.start) return true;
        c = ce.prev;                                                   // the op lies before this interval: it may still meet an earlier one
    }
    return false;
}

template <bool AGG>
__global__ __launch_bounds__(PREP_THREADS) void k_hap_group_counts(const HapGroupArgs a) {
    __shared__ typename std::conditional<AGG, HapGroupLds, HapGroupNoLds>::type T;
    const GroupAt g;
    const int gl = g.gl, i = g.i, tid = (int)threadIdx.x;
    if constexpr (AGG) {
        T.key[tid] = HJ_EMPTY; T.cnt[tid] = 0;
        __syncthreads();
    }
    bool walk = i < a.n_reads;
    DevRead d;
    int r_hi = 0, r_k = -1;
    if (walk) {
        d = a.reads[i];
        walk = read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags) && d.end > d.pos;
    }
    if (walk) {
        // the intervals that can overlap [pos, end): those below the first that starts at or behind `end`, from the first one open at the last start <= pos
        r_hi = interval_lower(a.intervals, 0, a.n_intervals, (long long)d.end);
        r_k = interval_lower(a.intervals, 0, r_hi, (long long)d.pos + 1) - 1;
        walk = (r_k >= 0 ? a.first_open[r_k] : 0) < r_hi;
    }
    if constexpr (!AGG) { if (!walk) return; }
    if (walk) {
        const bool serial = a.serial[i] != 0;
        const ReadInfo R(d, i, a.cigars, 0);
        const uint32_t tag = a.tags[i] & 3u;
        const int32_t set = tag ? a.read_ps[i] : -1;
        const uint32_t own = (d.flag & 16u) ? 2u : 1u, want = a.stranded == 1 ? own : 3u - own;      // the interval strand that counts this read
        // every interval that [x, x + len) overlaps and that starts at or behind prev_end, unless the read met its group before; (b, p):
        // where hg_earlier_hit starts from
        auto count_op = [&](long long x, uint32_t len, long long prev_end, uint32_t b, long long p) __attribute__((always_inline)) {
            const int hi = interval_lower(a.intervals, r_k < 0 ? 0 : r_k, r_hi, x + (long long)len);
            const int k = interval_lower(a.intervals, r_k < 0 ? 0 : r_k, hi, x + 1) - 1;
            for (int j = k >= 0 ? a.first_open[k] : 0; j < hi; ++j) {
                const DevHapInterval e = a.intervals[j];
                if ((long long)e.end <= x || (long long)e.start < prev_end) continue;
                const uint32_t strand = e.group_strand & 3u, grp = e.group_strand >> 2;
                if (a.stranded != 0 && strand != 0u && strand != want) continue;
                if (hg_earlier_hit(a.intervals, R, e.prev, b, p)) continue;
                uint32_t word = 2u * grp;                                  // untagged
                if (tag) {
                    word += 1u;                                            // tagged in a set that is none of the group's rows
                    int lo = a.group_row_off[grp], top = a.group_row_off[grp + 1u];
                    while (lo < top) {
                        const int mid = (lo + top) >> 1;
                        const int32_t q = a.row_ps[mid];
                        if (q == set) { word = 2u * (uint32_t)a.n_groups + 2u * (uint32_t)mid + (tag - 1u); break; }
                        if (q < set) lo = mid + 1; else top = mid;
                    }
                }
                if constexpr (AGG) {
                    const int s = hj_claim_lds(T.key, (unsigned long long)word);
                    if (s >= 0) { atomicAdd(&T.cnt[s], 1u); continue; }
                }
                hj_add(a.counts + word, 1u);
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
                count_op(x, len, prev_end, k + 1u, x + (long long)len);
            });
        } else if (gl == 0) {
            // the serial walk delivers normalised ops without their raw index: the merge starts from the read's last raw op
            long long rend = (long long)R.pos;
            for (uint32_t b = 0; b < R.n_cig; ++b) { const uint32_t c = R.cig[b]; if (op_ref(fold_op(c))) rend += (long long)(c >> 4); }
            long long prev_end = HAP_REGION_NO_END;
            (void)walk_serial_ops(R, [&](uint32_t op, uint32_t len, long long x, uint32_t, const OpCtx &) __attribute__((always_inline)) {
                if (op != C3R_CIG_M && op != C3R_CIG_D) return;
                count_op(x, len, prev_end, R.n_cig, rend);
                prev_end = x + (long long)len;
            });
        }
    }
    if constexpr (AGG) {
        __syncthreads();
        const unsigned long long key = T.key[tid];
        const uint32_t v = T.cnt[tid];
        if (key != HJ_EMPTY && v) hj_add(a.counts + (size_t)key, v);
    }
}

}  // namespace c3r
