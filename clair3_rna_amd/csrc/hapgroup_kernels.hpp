// hapgroup_kernels.hpp — k_hap_group_counts: reads by haplotype and phase set per GROUP of intervals of a sorted interval table
// (c3r_hap_group_counts: the genes of a BED file, each the group of its exons), from the reads, tags and phase sets that c3r_load_reads left
// on the device.  Included by c3r_lib.hip only.
//
// What it is for: allele-specific expression per gene — a read over three exons of one gene is one read of that gene, and a read that lies
// only in the gene's introns is none.  The rule (`hap_groups`) is stated in include/c3r.h and restated, independently of this file, by
// tests/hapgroupref.py.
//
// Built from the pieces of hapregion_kernels.hpp — 16 lanes per read, the two CIGAR walks whose M and D ops find the pair (read, interval)
// at the read's first covered position inside the interval — under the policy HapGroupTable.  Two things are its own.
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

struct HapGroupArgs : HapIntervalArgs<DevHapInterval> {
    const int32_t *group_row_off;             // [n_groups + 1] group g's rows: [group_row_off[g], group_row_off[g + 1])
};

struct HapGroupLds { unsigned long long key[HJ_LDS]; uint32_t cnt[HJ_LDS]; };     // key: the index of the count word
struct HapGroupNoLds {};

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

struct HapGroupTable {
    using Entry = DevHapInterval;
    using Args = HapGroupArgs;
    static constexpr bool RAW_END = true;
    static __device__ __forceinline__ uint32_t strand(const Entry &e) { return e.group_strand & 3u; }
    // the interval is the first of its group that the read covers
    static __device__ __forceinline__ bool counts_here(const Args &a, const ReadInfo &R, const Entry &e, uint32_t b, long long p) { return !hg_earlier_hit(a.entries, R, e.prev, b, p); }
    static __device__ __forceinline__ uint32_t owner(int, const Entry &e) { return e.group_strand >> 2; }
    static __device__ __forceinline__ void rows(const Args &a, const Entry &e, int &lo, int &top) { const uint32_t grp = e.group_strand >> 2; lo = a.group_row_off[grp]; top = a.group_row_off[grp + 1u]; }
};

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
    HapSpan r;
    if (walk) {
        d = a.reads[i];
        walk = hap_read_span(a, d, r);
    }
    if constexpr (!AGG) { if (!walk) return; }
    if (walk)
        hap_count_read<HapGroupTable>(a, d, i, gl, r, [&](uint32_t word) __attribute__((always_inline)) {
            if constexpr (AGG) {
                const int s = hj_claim_lds(T.key, (unsigned long long)word);
                if (s >= 0) { atomicAdd(&T.cnt[s], 1u); return; }
            }
            hj_add(a.counts + word, 1u);
        });
    if constexpr (AGG) {
        __syncthreads();
        const unsigned long long key = T.key[tid];
        const uint32_t v = T.cnt[tid];
        if (key != HJ_EMPTY && v) hj_add(a.counts + (size_t)key, v);
    }
}

}  // namespace c3r
