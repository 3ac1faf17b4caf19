// phase_kernels.hpp — k_phase_links: pairwise linkage counts between the contig's heterozygous SNVs from the loaded reads (c3r_phase_links),
// the device half of the project's own phasing; and k_phase_unit_links, the same between the blocks the chain left (c3r_phase_unit_links,
// the block-merge stage; at the end of the file); k_phase_allele_links and k_phase_allele_unit_links: the two over a table that also holds
// insertions, deletions and two-ALT sites (c3r_phase_allele_links, c3r_phase_allele_unit_links).  Included by c3r_lib.hip only.
//
// What it replaces: the read pass of `whatshap phase` / `longphase phase` between the two passes of the reference flow
// (run_clair3_rna:729-767).  The rule — a greedy linkage chain, not wMEC — is stated in include/c3r.h and restated, independently of this
// file, by tests/phaseref.py.  The chain itself is resolved on the host (c3r_phase_resolve): n dependent steps of K terms.
//
// 16 lanes per read and the launch shape of k_haplotag, the same two group searches for the read's sites [lo, hi) and the same two walks.
// Only the reads that read preparation keeps vote (read_kept); fewer than two sites in range and the CIGAR is never read.  Per window of
// PHASE_WIN table sites:
//   1. the walk stores one observation byte per site (0 none, 1 allele 0, 2 allele 1) in the read's slab in LDS (256 B x PREP_READS);
//   2. the group's lanes stride over the window's observed sites s and add one to links[s][k - 1][cis | trans] for every observed s - k,
//      k <= K, s - k >= lo (relaxed, agent scope: integer sums, arrival order never shows).
// Successive windows overlap by K sites and window w > 0 counts from its K-th site on, so every pair is counted in exactly one window; a
// read with more than PHASE_WIN sites in range walks its CIGAR once per window (the trade of k_haplotag's P + 1 walks: no global scratch).
// A slab is written by the lanes that hold the ops and read by the lanes that hold the sites, so the three steps of a window are separated
// by workgroup barriers: the window loop runs as often as the workgroup's longest read needs, every thread of the workgroup reaches every
// barrier (no early return for the groups past n_reads), and a read with fewer windows idles at them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "haplotag_kernels.hpp"

namespace c3r {

constexpr int PHASE_K = C3R_PHASE_LINKS, PHASE_WIN = 256, PHASE_STEP = PHASE_WIN - PHASE_K;
static_assert(PHASE_WIN == 16 * PREP_GRP, "a group clears its slab with one 16-byte store per lane");
static_assert(PHASE_K >= 1 && PHASE_K < PHASE_WIN, "windows overlap by K sites");

struct LinkArgs : ReadArgs {
    const c3r_phase_site_t *sites; int32_t n_sites;       // candidate sites (ps and h1 are not read)
    int32_t min_mq, excl_flags;               // the voters: read_kept
    uint32_t *links;                          // [n_sites][PHASE_K][2] cis / trans, zero on entry
};

// The body of k_phase_links and k_phase_allele_links: the window loop above with column(site, R, the read's bases, walk_sites' arguments)
// -> the allele index the read shows, 0 or 1, or 2 for nothing (the slab byte is the index + 1).  compat_plain: ReadInfo::compat of a read of the plain walk.  Every thread of the
// workgroup comes here and reaches every barrier.
template <bool LA = false, class Args, class Column>
__device__ __forceinline__ void phase_links_read(const Args &a, bool compat_plain, Column &&column) {
    __shared__ uint4 s_obs4[PREP_READS][PHASE_WIN / 16];
    __shared__ int s_nwin;
    const GroupAt g;
    const int gl = g.gl, slot = g.slot, i = g.i;
    uint8_t *const obs = reinterpret_cast<uint8_t *>(s_obs4[slot]);
    if (threadIdx.x == 0) s_nwin = 0;
    __syncthreads();
    SiteRange r = {0, 0};
    int nwin = 0;
    bool serial = false;
    ReadInfo R(DevRead{}, i, a.cigars, 0);                             // (an empty read until the group's own is known to vote)
    if (i < a.n_reads) {                                               // (whole groups take the branch: the ballots and shuffles below stay inside a group)
        const DevRead d = a.reads[i];
        if (read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags)) {
            r = read_sites(a.sites, a.n_sites, d, gl);
            const int m = r.hi - r.lo;
            nwin = m < 2 ? 0 : m <= PHASE_WIN ? 1 : 1 + (m - PHASE_WIN + PHASE_STEP - 1) / PHASE_STEP;
            R = ReadInfo(d, i, a.cigars, 0);
            serial = a.serial[i] != 0 || (LA && cigar_has_m_neighbours(R, gl));
            if (compat_plain && !serial) R.compat = 1;
        }
    }
    const int lo = r.lo, hi = r.hi;
    const uint8_t *rseq = a.seq + R.seq_off;
    if (gl == 0 && nwin > 0) atomicMax(&s_nwin, nwin);
    __syncthreads();
    const int nwin_wg = s_nwin;
    for (int w = 0; w < nwin_wg; ++w) {
        const bool mine = w < nwin;
        const int ws = lo + w * PHASE_STEP, we = min(ws + PHASE_WIN, hi);                 // the window's sites
        if (mine) s_obs4[slot][gl] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        if (mine) {
            walk_sites(R, gl, serial, a.sites, ws, we, [&](int s, const auto &e, unsigned long long q, bool first, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
                const uint32_t al = column(e, R, rseq, q, first, last, iq, cx);
                if (al != 2u) obs[s - ws] = (uint8_t)(al + 1u);
            });
        }
        __syncthreads();
        if (mine) {
            // window 0 counts from its first site (predecessors down to lo), a later one from its K-th (the sites before belong to the window before)
            for (int s = (w ? ws + PHASE_K : ws) + gl; s < we; s += PREP_GRP) {
                const uint32_t o = obs[s - ws];
                if (!o) continue;
#pragma unroll
                for (int k = 1; k <= PHASE_K; ++k) {
                    if (s - k < ws) break;
                    const uint32_t p = obs[s - k - ws];
                    if (p) __hip_atomic_fetch_add(&a.links[((size_t)s * PHASE_K + (size_t)(k - 1)) * 2 + (o != p ? 1 : 0)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        __syncthreads();                                                       // (the next window clears the slab)
    }
}

__global__ __launch_bounds__(PREP_THREADS) void k_phase_links(const LinkArgs a) {
    phase_links_read(a, false, [&](const c3r_phase_site_t &e, const ReadInfo &, const uint8_t *rseq, unsigned long long q, bool, bool, unsigned long long, const OpCtx &) __attribute__((always_inline)) {
        return snv_column(e, hap_nibble(rseq, q));
    });
}

// ---- k_phase_allele_links: the same link table over a table whose sites may be SNVs, insertions, deletions and two-ALT sites
// (c3r_phase_allele_links; the rule is in include/c3r.h, restated by tests/phaseindelref.py).  k_phase_links' body with hap_observe
// (haplotag_kernels.hpp) in the place of the nibble compare: columns 0 / 1 are the slab bytes 1 / 2, column 2 and no observation are 0.
// As in k_haplotag_alleles the reads of the plain walk get ReadInfo::compat = 1 so that OpCtx::n2op is filled (an I with a D behind it).
struct AlleleLinkArgs : ReadArgs {
    const c3r_hap_site_t *sites; int32_t n_sites;         // candidate sites (ps and reserved are not read)
    const uint8_t *pool;                      // the alleles' inserted bases, 4-bit packed like seq (never read when no allele is an insertion)
    int32_t min_mq, excl_flags;               // the voters: read_kept
    uint32_t *links;                          // [n_sites][PHASE_K][2] cis / trans, zero on entry
};

__global__ __launch_bounds__(PREP_THREADS) void k_phase_allele_links(const AlleleLinkArgs a) {
    phase_links_read(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = hap_observe(e, rseq, R.l_seq, a.pool, q, last, iq, cx);
        return al < 2u ? al : 2u;                                       // (another allele and no observation are both nothing here)
    });
}

// The same with the left-aligned observation (c3r_set_hap_left_align): hap_observe_la against the reference slice.
struct AlleleLinkLaArgs : AlleleLinkArgs { HapRef ref; };

__global__ __launch_bounds__(PREP_THREADS) void k_phase_allele_links_la(const AlleleLinkLaArgs a) {
    phase_links_read<true>(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool first, bool, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = hap_observe_la(e, rseq, R.l_seq, a.pool, a.ref, q, first, iq, cx);
        return al < 2u ? al : 2u;
    });
}

// The same with the realigned observation (c3r_set_hap_realign): hap_observe_ra against the reference slice, with the switch's overhang.
struct AlleleLinkRaArgs : AlleleLinkLaArgs { uint32_t overhang; };

__global__ __launch_bounds__(PREP_THREADS) void k_phase_allele_links_ra(const AlleleLinkRaArgs a) {
    phase_links_read(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = hap_observe_ra(e, R, rseq, a.pool, a.ref, a.overhang, q, last, iq, cx);
        return al < 2u ? al : 2u;
    });
}

// The same across splice junctions (c3r_set_hap_realign_spliced): hap_observe_rs, the _ra kernel's arguments.
__global__ __launch_bounds__(PREP_THREADS) void k_phase_allele_links_rs(const AlleleLinkRaArgs a) {
    phase_links_read(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = hap_observe_rs(e, R, rseq, a.pool, a.ref, a.overhang, q, last, iq, cx);
        return al < 2u ? al : 2u;
    });
}

// ---- k_phase_unit_links: the link table of the block-merge stage (c3r_phase_unit_links; the rule is in include/c3r.h, restated by
// tests/phasemergeref.py).  The units are the blocks the chain left (unit_of[s]: the unit of table site s, -1 for a singleton), and a read
// observes a unit with the majority of its sites' votes there: haplotype 1 / 2, nothing on a tie.
//
// The shape of k_haplotag: 16 lanes per read, no LDS, no workgroup barrier, whole groups leave early, and every loop count is a reduced
// value, the same in all lanes of a group.  A first walk finds the lowest and the highest unit the read observes; one unit (the common
// case after the chain) or none and the read is done without a global write.  Otherwise one walk per unit in increasing unit number,
// each of which counts that unit's votes and finds the next unit above it (the P + 1 walks of k_haplotag).  What the read has seen of
// the K units before the current one is two bit masks in registers — bit k: unit u - k was observed (not tied) / with haplotype 2 —
// shifted by the distance to the next unit, so a tied unit or one the read does not touch leaves a hole and no link spans more than K
// unit numbers.  Lane k - 1 of the group adds the link to unit u - k (relaxed, agent scope: integer sums, arrival order never shows).
struct UnitLinkArgs : ReadArgs {
    const c3r_phase_site_t *sites; int32_t n_sites;       // the chain's table: ref, alt and h1 are read, ps never (it holds -1)
    const int32_t *unit_of;                   // [n_sites] unit of every site, -1: singleton
    int32_t n_units;
    int32_t min_mq, excl_flags;               // the voters: read_kept
    uint32_t *ulinks;                         // [n_units][PHASE_K][2] same / different haplotype, zero on entry
};
static_assert(PHASE_K <= PREP_GRP && PHASE_K < 31, "one lane per predecessor unit, one mask bit per unit");

constexpr int32_t UNIT_NONE = 0x7fffffff;     // no unit (a unit number is below n_units <= n_sites < 2^31 - 1)

struct UnitTally {
    uint32_t c1, c2;          // votes for haplotype 1 / 2 in unit `cur` (cur < 0: not counted)
    int32_t u_min, u_max;     // smallest / largest observed unit above `cur` (u_min UNIT_NONE: none)
    __device__ __forceinline__ void reduce() {
#pragma unroll
        for (int off = PREP_GRP / 2; off > 0; off >>= 1) {
            c1 += __shfl_xor(c1, off, PREP_GRP);
            c2 += __shfl_xor(c2, off, PREP_GRP);
            u_min = min(u_min, (int32_t)__shfl_xor(u_min, off, PREP_GRP));
            u_max = max(u_max, (int32_t)__shfl_xor(u_max, off, PREP_GRP));
        }
    }
};

// One walk over the sites [lo, hi) that the read's M ops cover; singleton sites are skipped before anything else.  column(site, R, the
// read's bases, walk_sites' arguments) -> the allele index the read shows, 0 or 1, or 2 for nothing; h1_of(site) -> the index that lies on
// haplotype 1.  All lanes of the group come here together.
template <class Args, class Column, class H1Of>
__device__ __forceinline__ UnitTally unit_walk(const ReadInfo &R, int gl, bool serial, const Args &a, int lo, int hi, int32_t cur, Column &&column, H1Of &&h1_of) {
    UnitTally t;
    t.c1 = 0; t.c2 = 0; t.u_min = UNIT_NONE; t.u_max = -1;
    const uint8_t *rseq = a.seq + R.seq_off;
    walk_sites(R, gl, serial, a.sites, lo, hi, [&](int s, const auto &e, unsigned long long q, bool first, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const int32_t u = a.unit_of[s];
        if (u < 0 || u < cur) return;
        const uint32_t al = column(e, R, rseq, q, first, last, iq, cx);
        if (al == 2u) return;
        if (u > cur) { t.u_min = min(t.u_min, u); t.u_max = max(t.u_max, u); return; }
        if (al == h1_of(e)) t.c1 += 1; else t.c2 += 1;                 // (u == cur)
    });
    t.reduce();
    return t;
}

// The body of k_phase_unit_links and k_phase_allele_unit_links.  compat_plain: ReadInfo::compat of a read of the plain walk.  All lanes of
// a group take the same way through it (whole groups leave: the shuffles stay inside a group).
template <bool LA = false, class Args, class Column, class H1Of>
__device__ __forceinline__ void phase_unit_links_read(const Args &a, bool compat_plain, Column &&column, H1Of &&h1_of) {
    const GroupAt g;
    const int gl = g.gl, i = g.i;
    if (i >= a.n_reads) return;                                        // (whole groups leave: the shuffles below stay inside a group)
    const DevRead d = a.reads[i];
    if (!read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags)) return;
    const SiteRange r = read_sites(a.sites, a.n_sites, d, gl);
    const int lo = r.lo, hi = r.hi;
    if (hi - lo < 2) return;                                           // (two units take two sites)
    ReadInfo R(d, i, a.cigars, 0);
    const bool serial = a.serial[i] != 0 || (LA && cigar_has_m_neighbours(R, gl));
    if (compat_plain && !serial) R.compat = 1;
    const UnitTally all = unit_walk(R, gl, serial, a, lo, hi, -1, column, h1_of);
    if (all.u_min >= all.u_max) return;                                // no unit observed (UNIT_NONE, -1) or one
    uint32_t seen = 0, hap2 = 0;                                       // bit k: unit `last` - k was observed / with haplotype 2
    int32_t last = all.u_min;
    for (int32_t u = all.u_min; u != UNIT_NONE;) {
        const UnitTally t = unit_walk(R, gl, serial, a, lo, hi, u, column, h1_of);
        const int32_t dist = u - last;
        seen = dist < 32 ? seen << dist : 0u;                          // now bit k: unit u - k
        hap2 = dist < 32 ? hap2 << dist : 0u;
        last = u;
        if (t.c1 != t.c2) {                                            // (a tie is no observation: it links nothing and is not kept)
            const uint32_t h = t.c2 > t.c1 ? 1u : 0u;
            const int k = gl + 1;
            if (k <= PHASE_K && ((seen >> k) & 1u) && u < a.n_units)
                __hip_atomic_fetch_add(&a.ulinks[((size_t)u * PHASE_K + (size_t)(k - 1)) * 2 + ((((hap2 >> k) & 1u) != h) ? 1 : 0)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            seen |= 1u;
            hap2 |= h;
        }
        u = t.u_min;
    }
}

__global__ __launch_bounds__(PREP_THREADS) void k_phase_unit_links(const UnitLinkArgs a) {
    phase_unit_links_read(a, false, [&](const c3r_phase_site_t &e, const ReadInfo &, const uint8_t *rseq, unsigned long long q, bool, bool, unsigned long long, const OpCtx &) __attribute__((always_inline)) {
        return snv_column(e, hap_nibble(rseq, q));
    }, [](const c3r_phase_site_t &e) __attribute__((always_inline)) { return (uint32_t)e.h1; });
}

// ---- k_phase_allele_unit_links: the unit link table over the allele table (c3r_phase_allele_unit_links) -- k_phase_unit_links' body with
// hap_observe in the place of the nibble compare.  The device's copy of the table holds h1 in reserved[0] of every site, as the copy of
// c3r_set_phase_alleles does, so that a site is one 32-byte load.
struct AlleleUnitLinkArgs : ReadArgs {
    const c3r_hap_site_t *sites; int32_t n_sites;         // the chain's table: reserved[0] holds h1; ps is not read
    const uint8_t *pool;                      // the alleles' inserted bases, 4-bit packed like seq
    const int32_t *unit_of;                   // [n_sites] unit of every site, -1: singleton
    int32_t n_units;
    int32_t min_mq, excl_flags;               // the voters: read_kept
    uint32_t *ulinks;                         // [n_units][PHASE_K][2] same / different haplotype, zero on entry
};

__global__ __launch_bounds__(PREP_THREADS) void k_phase_allele_unit_links(const AlleleUnitLinkArgs a) {
    phase_unit_links_read(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = hap_observe(e, rseq, R.l_seq, a.pool, q, last, iq, cx);
        return al < 2u ? al : 2u;
    }, [](const c3r_hap_site_t &e) __attribute__((always_inline)) { return (uint32_t)e.reserved[0]; });
}

// The same with the left-aligned observation (c3r_set_hap_left_align): hap_observe_la against the reference slice.
struct AlleleUnitLinkLaArgs : AlleleUnitLinkArgs { HapRef ref; };

__global__ __launch_bounds__(PREP_THREADS) void k_phase_allele_unit_links_la(const AlleleUnitLinkLaArgs a) {
    phase_unit_links_read<true>(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool first, bool, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = hap_observe_la(e, rseq, R.l_seq, a.pool, a.ref, q, first, iq, cx);
        return al < 2u ? al : 2u;
    }, [](const c3r_hap_site_t &e) __attribute__((always_inline)) { return (uint32_t)e.reserved[0]; });
}

// The same with the realigned observation (c3r_set_hap_realign).
struct AlleleUnitLinkRaArgs : AlleleUnitLinkLaArgs { uint32_t overhang; };

__global__ __launch_bounds__(PREP_THREADS) void k_phase_allele_unit_links_ra(const AlleleUnitLinkRaArgs a) {
    phase_unit_links_read(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = hap_observe_ra(e, R, rseq, a.pool, a.ref, a.overhang, q, last, iq, cx);
        return al < 2u ? al : 2u;
    }, [](const c3r_hap_site_t &e) __attribute__((always_inline)) { return (uint32_t)e.reserved[0]; });
}

// The same across splice junctions (c3r_set_hap_realign_spliced).
__global__ __launch_bounds__(PREP_THREADS) void k_phase_allele_unit_links_rs(const AlleleUnitLinkRaArgs a) {
    phase_unit_links_read(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = hap_observe_rs(e, R, rseq, a.pool, a.ref, a.overhang, q, last, iq, cx);
        return al < 2u ? al : 2u;
    }, [](const c3r_hap_site_t &e) __attribute__((always_inline)) { return (uint32_t)e.reserved[0]; });
}

}  // namespace c3r
