// hapjunction_kernels.hpp — k_hap_junction_counts: reads by haplotype and phase set per splice junction (c3r_hap_junction_counts), from the
// reads, tags and phase sets that c3r_load_reads left on the device.  Included by c3r_lib.hip only.
//
// What it is for: allele-specific splicing — which haplotype uses which intron — without writing the haplotagged BAM and counting its N ops
// again.  The rule (`hap_junctions`) is stated in include/c3r.h and restated, independently of this file, by tests/hapjunctionref.py.
//
// The shape of k_hap_region_counts: 16 lanes per read, the two CIGAR walks (walk_plain_ops / walk_serial_ops) with a callback that takes
// the N ops; a read that read preparation does not keep (read_kept) or that lies past n_reads is never walked.  The junctions are
// discovered, not given, so the counts go into two insert-only open-addressing tables in global memory:
//   junctions  key (start << 32) | end            counters reads, reverse, untagged
//   rows       key (junction slot << 32) | ps     counters hp1, hp2
// A key is claimed with a 64-bit compare-and-swap against the empty key (all ones: a start is >= 0 and a slot is below 2^28, so no key
// equals it); a lane that finds its key there uses that slot; nothing ever waits for another lane.  A slot's key changes once, from empty to
// its key, so the plain look before the swap can only err towards `empty`, and then the swap answers.  Every probe loop is bounded by the
// table's size and by HJ_MAX_PROBES = 256: a lane that finds no place within that raises the table's bit of the overflow word and gives up,
// and the host doubles that table, clears both and launches again (c3r_lib.hip) — the counts are sums, so the repeat is exact.  The cap
// makes a table grow before linear probing degenerates (a run of 256 occupied slots means a load factor near 0.9 or above; growing early
// is harmless), and once any bit of the overflow word is set — this launch's counts are thrown away — a claim that has not found its place
// within 16 probes looks at the word and leaves.
//
// Aggregation (AGG = true).  Dozens to thousands of reads hold one junction, and a workgroup's 16 reads are neighbours in the sorted input:
// they mostly share their junctions.  One global add per (read, junction) would serialise on the junction's words as the per-gene counts of
// k_hap_region_counts did.  So the counts go first into two tables of the same form in LDS (BinHash / hb_find of reads_kernels.hpp: the key,
// the counters beside it, an LDS compare-and-swap to claim, LDS adds), and after the workgroup's barrier every thread flushes one slot of
// each: one global claim and one add per non-zero counter.  The LDS tables have PREP_THREADS = 256 slots each — a slot per thread for the
// clearing and the flush, and room for 16 distinct junctions per read of the workgroup before anything spills — in 10 KB.  A key that
// finds no place among its HJ_LDS_PROBES slots goes straight to the global tables, like a bin that hb_find refuses.  The row table's LDS key
// names the junction's LDS slot; the flush of the junctions leaves each slot's global slot in LDS, a second barrier, and the rows follow.
// Every thread reaches every barrier: a group without a read to walk skips the walk, not the kernel.
// AGG = false is the same body without the LDS stage (no LDS, no barrier, whole groups leave early): c3r_set_hap_junction_direct picks it
// at run time, so that tools/hap_junctions_time.py can say what the aggregation buys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "haplotag_kernels.hpp"

namespace c3r {

constexpr unsigned long long HJ_EMPTY = ~0ull;                      // no key
constexpr uint32_t HJ_OVER_JUNCTIONS = 1u, HJ_OVER_ROWS = 2u;       // bits of the overflow word: the table that had no place for a key
constexpr int HJ_MIN_LOG = 4, HJ_MAX_LOG = 28;                       // a global table has 2^4 .. 2^28 slots
constexpr uint32_t HJ_MAX_PROBES = 256u, HJ_LOOK_AT = 16u;            // a claim's probes at most; the probe at which it looks at the overflow word
constexpr int HJ_LDS_LOG = 8, HJ_LDS = 1 << HJ_LDS_LOG, HJ_LDS_PROBES = 16;
static_assert(HJ_LDS == PREP_THREADS, "a thread clears and flushes one slot of each LDS table");
static_assert(sizeof(c3r_hap_junction_t) == 24 && sizeof(c3r_hap_junction_row_t) == 12, "junction layout");

struct HapJunctionArgs : ReadArgs {
    const uint32_t *tags;                     // [n_reads] k_haplotag's: tag in the low two bits; null: no phase table, every read is untagged
    const int32_t *read_ps;                   // [n_reads] k_haplotag's: the set the tag was decided in
    int32_t min_mq, excl_flags;               // the counted reads: read_kept
    unsigned long long *jkeys; uint32_t *jcounts; uint32_t jlog;      // 2^jlog junction slots: keys all ones, [slots][3] counters zero on entry
    unsigned long long *rkeys; uint32_t *rcounts; uint32_t rlog;      // 2^rlog row slots: keys all ones, [slots][2] counters zero on entry
    uint32_t *overflow;                       // zero on entry
};

// the workgroup's tables (AGG)
struct HapJunctionLds {
    unsigned long long jkey[HJ_LDS], rkey[HJ_LDS];        // rkey: (slot in jkey << 32) | ps
    uint32_t jcnt[HJ_LDS][3], rcnt[HJ_LDS][2];
    int32_t jslot[HJ_LDS];                                 // the flush: the junction's slot in the global table, -1: none
};
struct HapJunctionNoLds {};

__device__ __forceinline__ uint32_t hj_hash(unsigned long long key, uint32_t log) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64u - log)); }

__device__ __forceinline__ void hj_overflow(const HapJunctionArgs &a, uint32_t bit) {
    if (!(__hip_atomic_load(a.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) __hip_atomic_fetch_or(a.overflow, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// slot of `key` in a global table of 2^log slots, claimed if it was not there; -1: none — no place within min(2^log, HJ_MAX_PROBES) probes,
// and then `bit` of the overflow word is raised, or the launch is being repeated anyway (see above)
__device__ __forceinline__ int hj_claim(const HapJunctionArgs &a, unsigned long long *keys, uint32_t log, unsigned long long key, uint32_t bit) {
    const uint32_t mask = (1u << log) - 1u, last = min(mask, HJ_MAX_PROBES - 1u);
    uint32_t h = hj_hash(key, log);
    for (uint32_t p = 0; p <= last; ++p, h = (h + 1u) & mask) {
        if (p == HJ_LOOK_AT && __hip_atomic_load(a.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return -1;
        unsigned long long k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == HJ_EMPTY) {
            k = HJ_EMPTY;
            if (__hip_atomic_compare_exchange_strong(&keys[h], &k, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return (int)h;
        }
        if (k == key) return (int)h;
    }
    hj_overflow(a, bit);
    return -1;
}
// the same in an LDS table of HJ_LDS slots, HJ_LDS_PROBES probes; no bit: the key goes to the global tables
__device__ __forceinline__ int hj_claim_lds(unsigned long long *keys, unsigned long long key) {
    uint32_t h = hj_hash(key, HJ_LDS_LOG);
    for (int p = 0; p < HJ_LDS_PROBES; ++p, h = (h + 1u) & (HJ_LDS - 1)) {
        // a plain look beside other lanes' swaps: a slot changes once, from empty to its key, and an aligned 64-bit LDS load does not tear,
        // so the look can only err towards `empty`, and then the swap answers
        unsigned long long k = keys[h];
        if (k == HJ_EMPTY) k = atomicCAS(&keys[h], HJ_EMPTY, key);
        if (k == HJ_EMPTY || k == key) return (int)h;
    }
    return -1;
}
__device__ __forceinline__ void hj_add(uint32_t *word, uint32_t n) { __hip_atomic_fetch_add(word, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// n more reads of haplotype `tag` (1, 2) in set `ps` at the junction of global slot g
__device__ __forceinline__ void hj_row_add(const HapJunctionArgs &a, int g, int32_t ps, uint32_t tag, uint32_t n) {
    const int r = hj_claim(a, a.rkeys, a.rlog, ((unsigned long long)(uint32_t)g << 32) | (unsigned long long)(uint32_t)ps, HJ_OVER_ROWS);
    if (r >= 0) hj_add(a.rcounts + 2 * (size_t)r + (tag - 1u), n);
}

template <bool AGG>
__global__ __launch_bounds__(PREP_THREADS) void k_hap_junction_counts(const HapJunctionArgs a) {
    __shared__ typename std::conditional<AGG, HapJunctionLds, HapJunctionNoLds>::type T;
    const GroupAt g;
    const int gl = g.gl, i = g.i, tid = (int)threadIdx.x;
    if constexpr (AGG) {
        T.jkey[tid] = HJ_EMPTY; T.rkey[tid] = HJ_EMPTY; T.jslot[tid] = -1;
        T.jcnt[tid][0] = 0; T.jcnt[tid][1] = 0; T.jcnt[tid][2] = 0; T.rcnt[tid][0] = 0; T.rcnt[tid][1] = 0;
        __syncthreads();
    }
    bool walk = i < a.n_reads;
    DevRead d;
    if (walk) {
        d = a.reads[i];
        walk = read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags) && d.end > d.pos;
    }
    if constexpr (!AGG) { if (!walk) return; }
    if (walk) {
        const bool serial = a.serial[i] != 0;
        const ReadInfo R(d, i, a.cigars, 0);
        const uint32_t tag = a.tags ? a.tags[i] & 3u : 0u;
        const int32_t set = tag ? a.read_ps[i] : -1;
        const bool reverse = (d.flag & 16u) != 0;
        auto on_op = [&](uint32_t op, uint32_t len, long long x, uint32_t, const OpCtx &) __attribute__((always_inline)) {
            if (op != C3R_CIG_N || len == 0u) return;
            const unsigned long long key = ((unsigned long long)(uint32_t)x << 32) | (unsigned long long)(uint32_t)(x + (long long)len);
            if constexpr (AGG) {
                const int s = hj_claim_lds(T.jkey, key);
                if (s >= 0) {
                    atomicAdd(&T.jcnt[s][0], 1u);
                    if (reverse) atomicAdd(&T.jcnt[s][1], 1u);
                    if (!tag) { atomicAdd(&T.jcnt[s][2], 1u); return; }
                    const int r = hj_claim_lds(T.rkey, ((unsigned long long)(uint32_t)s << 32) | (unsigned long long)(uint32_t)set);
                    if (r >= 0) { atomicAdd(&T.rcnt[r][tag - 1u], 1u); return; }
                    // the junction counts in LDS, the row finds no place there: the junction's global slot now (the flush finds it again)
                    const int gs = hj_claim(a, a.jkeys, a.jlog, key, HJ_OVER_JUNCTIONS);
                    if (gs >= 0) hj_row_add(a, gs, set, tag, 1u);
                    return;
                }
            }
            const int gs = hj_claim(a, a.jkeys, a.jlog, key, HJ_OVER_JUNCTIONS);
            if (gs < 0) return;
            uint32_t *const c = a.jcounts + 3 * (size_t)gs;
            hj_add(c, 1u);
            if (reverse) hj_add(c + 1, 1u);
            if (!tag) hj_add(c + 2, 1u); else hj_row_add(a, gs, set, tag, 1u);
        };
        if (!serial) walk_plain_ops(R, gl, on_op);
        else if (gl == 0) (void)walk_serial_ops(R, on_op);
    }
    if constexpr (AGG) {
        __syncthreads();
        const unsigned long long key = T.jkey[tid];
        if (key != HJ_EMPTY) {
            const int gs = hj_claim(a, a.jkeys, a.jlog, key, HJ_OVER_JUNCTIONS);
            if (gs >= 0) {
                uint32_t *const c = a.jcounts + 3 * (size_t)gs;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const uint32_t v = T.jcnt[tid][k]; if (v) hj_add(c + k, v); }
                T.jslot[tid] = gs;
            }
        }
        __syncthreads();
        const unsigned long long rk = T.rkey[tid];
        if (rk != HJ_EMPTY) {
            const int gs = T.jslot[(uint32_t)(rk >> 32)];
            if (gs >= 0) {
#pragma unroll
                for (uint32_t t = 1; t <= 2; ++t) { const uint32_t v = T.rcnt[tid][t - 1u]; if (v) hj_row_add(a, gs, (int32_t)(uint32_t)rk, t, v); }
            }
        }
    }
}

}  // namespace c3r
