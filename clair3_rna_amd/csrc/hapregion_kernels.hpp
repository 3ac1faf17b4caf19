// hapregion_kernels.hpp — reads by haplotype and phase set over a sorted interval table, from the reads, tags and phase sets that
// c3r_load_reads left on the device: the pieces that k_hap_region_counts (here: one count per read and interval, c3r_hap_region_counts — the
// exons or genes of a BED file) and k_hap_group_counts (hapgroup_kernels.hpp: one count per read and GROUP of intervals) are both made of,
// and the first of the two kernels.  Included by c3r_lib.hip only.
//
// What it is for: allele-specific expression — how many reads of each haplotype a gene or an exon is expressed from — without writing the
// haplotagged BAM and reading it again.  The rule (`hap_regions`) is stated in include/c3r.h and restated, independently of this file, by
// tests/hapregionref.py.
//
// Each rule stands once, at its code:
//   interval_lower, hap_span       the table entries that can overlap a stretch of the reference, from the host's first_open
//   walk_covering_ops              the M / D ops of a read through either CIGAR walk, each with the end of the nearest earlier one
//   hap_entry, hap_op_candidates   the entries an op counts for, one 16-byte load each: overlap, first covered position (prev_end), strand
//   hap_row_of, hap_count_word     the count word of a (read, owner) pair in the dense table
//   hap_count_read                 the four above for one read; what differs between the two tables is a policy (HapRegionTable here,
//                                  HapGroupTable there), what is done with a count word is the kernel's
// One add per pair: integer sums, arrival order never shows.  Nothing is reduced across lanes: no shuffle follows the walk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "haplotag_kernels.hpp"

namespace c3r {

// What both kernels take: the table's entries (16 bytes each, beginning with start, end), sorted by (start, end), and the count words as
// one dense table — two per owner (a region, or a group), then two per row.
template <class Entry>
struct HapIntervalArgs : ReadArgs {
    const uint32_t *tags;                     // [n_reads] k_haplotag's: tag in the low two bits
    const int32_t *read_ps;                   // [n_reads] k_haplotag's: the set the tag was decided in, -1 when the tag is 0
    int32_t min_mq, excl_flags;               // the voters: read_kept
    const Entry *entries; int32_t n_entries;  // sorted by (start, end)
    const int32_t *first_open;                // [n_entries] smallest i <= j with end_i > start_j
    const int32_t *row_ps;                    // the owners' phase sets, owner by owner, strictly increasing inside an owner
    int32_t n_owners, stranded;               // stranded: 0 off, 1 same, 2 reverse
    uint32_t *counts;                         // [2 n_owners + 2 n_rows]: per owner untagged, tagged in another set; then per row haplotype 1, 2; zero on entry
};

// first entry of [lo, hi) with start >= p (hi: none)
template <class Entry>
__device__ __forceinline__ int interval_lower(const Entry *v, int lo, int hi, long long p) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)v[mid].start < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The entries that can overlap [from, to): [first, hi).  hi is the first entry that starts at or behind `to`, k the last one that starts at
// or before `from` (-1: none), and first = first_open[k] — 0 when k is -1.  first_open[j] (the host computes it) is the smallest i <= j with
// end_i > start_j, so an entry below first_open[k] ends at or before start_k <= from: [first, hi) holds every entry the stretch overlaps.
struct HapSpan {
    int k, first, hi;
    __device__ __forceinline__ bool empty() const { return first >= hi; }
};
// ... searched in [lo, top) only: a read's span in the whole table, an op's in the read's — from the read's k (the read begins at or before
// the op) to the read's hi
template <class Entry>
__device__ __forceinline__ HapSpan hap_span(const Entry *v, const int32_t *first_open, int lo, int top, long long from, long long to) {
    HapSpan s;
    s.hi = interval_lower(v, lo, top, to);
    s.k = interval_lower(v, lo, s.hi, from + 1) - 1;
    s.first = s.k >= 0 ? first_open[s.k] : 0;
    return s;
}
// Is the read a voter with a span that some entry can overlap?  `r`: that span.
template <class Args>
__device__ __forceinline__ bool hap_read_span(const Args &a, const DevRead &d, HapSpan &r) {
    if (!read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags) || d.end <= d.pos) return false;
    r = hap_span(a.entries, a.first_open, 0, a.n_entries, (long long)d.pos, (long long)d.end);
    return !r.empty();
}

constexpr long long HAP_REGION_NO_END = INT64_MIN;         // no earlier covering op

// on_op(x, len, prev_end, b, p) for every M / D op [x, x + len) of the read, by the lane that holds it.  prev_end is the end of the read's
// nearest earlier M / D op (HAP_REGION_NO_END for the first one): the plain walk's lane finds it by stepping back over the I / S / N ops
// before its own, the serial walk's one lane carries it.  (b, p), under RAW_END only: the raw ops [0, b) lie before reference position p,
// where op b - 1 ends — in the plain walk the op itself, in the serial walk, which delivers normalised ops without their raw index, the
// read's last op.
template <bool RAW_END, class OnOp>
__device__ __forceinline__ void walk_covering_ops(const ReadInfo &R, int gl, bool serial, OnOp &&on_op) {
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
            on_op(x, len, prev_end, k + 1u, x + (long long)len);
        });
    } else if (gl == 0) {
        long long rend = (long long)R.pos;
        if constexpr (RAW_END)
            for (uint32_t b = 0; b < R.n_cig; ++b) { const uint32_t c = R.cig[b]; if (op_ref(fold_op(c))) rend += (long long)(c >> 4); }
        long long prev_end = HAP_REGION_NO_END;
        (void)walk_serial_ops(R, [&](uint32_t op, uint32_t len, long long x, uint32_t, const OpCtx &) __attribute__((always_inline)) {
            if (op != C3R_CIG_M && op != C3R_CIG_D) return;
            on_op(x, len, prev_end, R.n_cig, rend);
            prev_end = x + (long long)len;
        });
    }
}

// A candidate is one 16-byte load, whichever fields the tests behind it read and in whichever order (left to itself the compiler fetches
// a field where it is first used: three dependent loads per candidate of the interval table).
template <class Entry>
__device__ __forceinline__ Entry hap_entry(const Entry *p) {
    static_assert(sizeof(Entry) == 16 && alignof(int4) == 16, "an entry is one 16-byte load");
    const int4 raw = *reinterpret_cast<const int4 *>(p);
    Entry e;
    __builtin_memcpy(&e, &raw, sizeof e);
    return e;
}

// on_entry(j, entry) for every entry that the op [x, x + len) of a read with span `r` counts for: it overlaps the op, it starts at or behind
// prev_end — so the op holds the read's first covered position inside it, and a (read, entry) pair is found exactly once — and its strand
// admits the read (`want`: the entry strand that does, under stranded 1 or 2).
template <class Table, class OnEntry>
__device__ __forceinline__ void hap_op_candidates(const typename Table::Entry *v, const int32_t *first_open, const HapSpan &r, long long x, uint32_t len,
                                                  long long prev_end, int32_t stranded, uint32_t want, OnEntry &&on_entry) {
    const HapSpan s = hap_span(v, first_open, r.k < 0 ? 0 : r.k, r.hi, x, x + (long long)len);
    for (int j = s.first; j < s.hi; ++j) {
        const typename Table::Entry e = hap_entry(v + j);
        if ((long long)e.end <= x || (long long)e.start < prev_end) continue;
        const uint32_t strand = Table::strand(e);
        if (stranded != 0 && strand != 0u && strand != want) continue;
        on_entry(j, e);
    }
}

// the row of [lo, top) whose phase set is `set` (-1: none)
__device__ __forceinline__ int hap_row_of(const int32_t *row_ps, int lo, int top, int32_t set) {
    while (lo < top) {
        const int mid = (lo + top) >> 1;
        const int32_t p = row_ps[mid];
        if (p == set) return mid;
        if (p < set) lo = mid + 1; else top = mid;
    }
    return -1;
}

// The index of the word that counts a read with `tag` and `set` for `owner`: the owner's first word for an untagged read, the row's word
// of the tag when the set is one of the owner's rows (Table::rows), else the owner's second word.
template <class Table>
__device__ __forceinline__ uint32_t hap_count_word(const typename Table::Args &a, uint32_t owner, const typename Table::Entry &e, uint32_t tag, int32_t set) {
    if (!tag) return 2u * owner;
    int lo, top;
    Table::rows(a, e, lo, top);
    const int row = hap_row_of(a.row_ps, lo, top, set);
    return row < 0 ? 2u * owner + 1u : 2u * (uint32_t)a.n_owners + 2u * (uint32_t)row + (tag - 1u);
}

// add(word index) for every count of read i (`d`, span `r`), by the lane that finds it.  Table names what the two tables differ in: Entry
// and Args; strand(e); RAW_END and counts_here(a, R, e, b, p), the last word on whether the op that found (read, e) counts for e's owner;
// owner(j, e); rows(a, e, lo, top).
template <class Table, class Add>
__device__ __forceinline__ void hap_count_read(const typename Table::Args &a, const DevRead &d, int i, int gl, const HapSpan &r, Add &&add) {
    const bool serial = a.serial[i] != 0;
    const ReadInfo R(d, i, a.cigars, 0);
    const uint32_t tag = a.tags[i] & 3u;
    const int32_t set = tag ? a.read_ps[i] : -1;
    const uint32_t own = (d.flag & 16u) ? 2u : 1u, want = a.stranded == 1 ? own : 3u - own;      // the entry strand that counts this read
    walk_covering_ops<Table::RAW_END>(R, gl, serial, [&](long long x, uint32_t len, long long prev_end, uint32_t b, long long p) __attribute__((always_inline)) {
        hap_op_candidates<Table>(a.entries, a.first_open, r, x, len, prev_end, a.stranded, want, [&](int j, const typename Table::Entry &e) __attribute__((always_inline)) {
            if (Table::counts_here(a, R, e, b, p)) add(hap_count_word<Table>(a, Table::owner(j, e), e, tag, set));
        });
    });
}

// ---- k_hap_region_counts: every entry is its own owner
// a region as the kernel loads it: c3r_hap_region_t with the count of its rows above the strand byte (c3r_hap_region_counts puts it into
// reserved[0 .. 2] of its copy, so that a candidate is one 16-byte load)
struct DevHapRegion { int32_t start, end, row_off; uint32_t strand_rows; };
static_assert(sizeof(DevHapRegion) == 16 && sizeof(c3r_hap_region_t) == 16, "region layout");

struct HapRegionArgs : HapIntervalArgs<DevHapRegion> {};

struct HapRegionTable {
    using Entry = DevHapRegion;
    using Args = HapRegionArgs;
    static constexpr bool RAW_END = false;
    static __device__ __forceinline__ uint32_t strand(const Entry &e) { return e.strand_rows & 255u; }
    static __device__ __forceinline__ bool counts_here(const Args &, const ReadInfo &, const Entry &, uint32_t, long long) { return true; }
    static __device__ __forceinline__ uint32_t owner(int j, const Entry &) { return (uint32_t)j; }
    static __device__ __forceinline__ void rows(const Args &, const Entry &e, int &lo, int &top) { lo = e.row_off; top = e.row_off + (int)(e.strand_rows >> 8); }
};

// The shape of k_hap_counts: 16 lanes per read, no LDS, no workgroup barrier, whole groups leave early — past n_reads, a read that read
// preparation does not keep, or no region that can overlap the read's span.  One relaxed, agent-scope add per pair.
__global__ __launch_bounds__(PREP_THREADS) void k_hap_region_counts(const HapRegionArgs a) {
    const GroupAt g;
    if (g.i >= a.n_reads) return;
    const DevRead d = a.reads[g.i];
    HapSpan r;
    if (!hap_read_span(a, d, r)) return;
    hap_count_read<HapRegionTable>(a, d, g.i, g.gl, r, [&](uint32_t word) __attribute__((always_inline)) {
        __hip_atomic_fetch_add(a.counts + word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
}

}  // namespace c3r
