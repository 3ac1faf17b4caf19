// hapcount_kernels.hpp — k_hap_counts, k_hap_allele_counts: reads by (haplotype of the read) x (allele the read shows) at a list of called sites
// (c3r_hap_counts: biallelic SNVs; c3r_hap_allele_counts: SNVs, insertions, deletions and two-ALT sites), from the reads, tags and phase sets that c3r_load_reads left on the device.  Included by c3r_lib.hip only.
//
// What it is for: the phase of the FINAL VCF's heterozygous SNVs (c3r_hap_assign reads the table on the host) and the per-site haplotype
// support that the reference flow leaves as a haplotagged BAM per contig (run_clair3_rna:769-801).  The rule is stated in include/c3r.h
// and restated, independently of this file, by tests/hapcountref.py.
//
// The shape of k_haplotag: 16 lanes per read, no LDS, no workgroup barrier, whole groups leave early — past n_reads, a read that read
// preparation does not keep (read_kept: the voters of k_phase_links), or no query site on the read's span after the two group searches.
// One walk (walk_plain_ops / walk_serial_ops): every M op searches its own stretch of the read's sites once, reads one nibble per site
// and adds one to counts[site][row][allele] (relaxed, agent scope: integer sums, arrival order never shows).  A reference position lies
// under at most one op of a read, so a read adds to a site at most once.  The row is the read's tag where the read's phase set is the
// site's, else 0.  Nothing is reduced across lanes: no shuffle follows the walk.
//
// At a very deep locus every read adds to the same nine words; the adds are not aggregated in LDS (DESIGN.md section 4 says what has been measured and what has not).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "haplotag_kernels.hpp"

namespace c3r {

// What the two counting kernels take beside their table.
struct HapTableArgs : ReadArgs {
    const uint32_t *tags;                     // [n_reads] k_haplotag's: tag in the low two bits
    const int32_t *read_ps;                   // [n_reads] k_haplotag's: the set the tag was decided in, -1 when the tag is 0
    int32_t min_mq, excl_flags;               // the voters: read_kept
    uint32_t *counts;                         // [n_sites][3][3] row (0, haplotype 1, 2) x column (ref / A, alt / B, other), zero on entry
};

// The body of k_hap_counts and k_hap_allele_counts: one walk of the group's read, one add per site where
// column(site, R, the read's bases, walk_sites' arguments) gives 0, 1 or 2 (more: nothing).  compat_plain: ReadInfo::compat of a read of
// the plain walk.  All lanes of a group take the same way through it (whole groups leave: the ballots of the searches stay inside a group).
template <bool LA = false, class Args, class Column>
__device__ __forceinline__ void hap_count_read(const Args &a, bool compat_plain, Column &&column) {
    const GroupAt g;
    const int gl = g.gl, i = g.i;
    if (i >= a.n_reads) return;
    const DevRead d = a.reads[i];
    if (!read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags)) return;
    const SiteRange r = read_sites(a.sites, a.n_sites, d, gl);
    if (r.lo >= r.hi) return;
    const bool serial = a.serial[i] != 0 || (LA && cigar_has_m_neighbours(ReadInfo(d, i, a.cigars, 0), gl));
    const ReadInfo R(d, i, a.cigars, compat_plain && !serial ? 1 : 0);
    const uint8_t *rseq = a.seq + R.seq_off;
    const uint32_t tag = a.tags[i] & 3u;
    const int32_t set = tag ? a.read_ps[i] : -1;
    walk_sites(R, gl, serial, a.sites, r.lo, r.hi, [&](int s, const auto &e, unsigned long long q, bool first, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = column(e, R, rseq, q, first, last, iq, cx);
        if (al > 2u) return;
        const uint32_t row = e.ps == set ? tag : 0u;                   // (set = -1 equals no query ps: they are >= 0)
        __hip_atomic_fetch_add(&a.counts[(size_t)s * 9 + row * 3 + al], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
}

struct HapCountArgs : HapTableArgs {
    const c3r_phase_site_t *sites; int32_t n_sites;       // query sites (h1 is not read)
};

__global__ __launch_bounds__(PREP_THREADS) void k_hap_counts(const HapCountArgs a) {
    hap_count_read(a, false, [&](const c3r_phase_site_t &e, const ReadInfo &, const uint8_t *rseq, unsigned long long q, bool, bool, unsigned long long, const OpCtx &) __attribute__((always_inline)) {
        const uint32_t b = hap_nibble(rseq, q);
        return hap_is_acgt(b) ? snv_column(e, b) : HAP_NOTHING;
    });
}

// ---- k_hap_allele_counts: the same table for sites whose two alleles may be SNVs, insertions or deletions (c3r_hap_allele_counts) ----------
// The rule is stated in include/c3r.h and restated, independently of this file, by tests/hapalleleref.py.  k_hap_counts' shape: 16 lanes per
// read, the two group searches, one walk, one relaxed add per observation, no LDS, no barrier, nothing reduced across lanes.  The column is
// hap_observe's (haplotag_kernels.hpp, where k_haplotag_alleles takes the same observation).
struct HapAlleleArgs : HapTableArgs {
    const c3r_hap_site_t *sites; int32_t n_sites;
    const uint8_t *pool;                      // the alleles' inserted bases, 4-bit packed like seq (never read when no allele is an insertion)
};

__global__ __launch_bounds__(PREP_THREADS) void k_hap_allele_counts(const HapAlleleArgs a) {
    hap_count_read(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        return hap_observe(e, rseq, R.l_seq, a.pool, q, last, iq, cx);
    });
}

// The same with the left-aligned observation (c3r_set_hap_left_align): hap_observe_la against the reference slice.
struct HapAlleleLaArgs : HapAlleleArgs { HapRef ref; };

__global__ __launch_bounds__(PREP_THREADS) void k_hap_allele_counts_la(const HapAlleleLaArgs a) {
    hap_count_read<true>(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool first, bool, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        return hap_observe_la(e, rseq, R.l_seq, a.pool, a.ref, q, first, iq, cx);
    });
}

// The same with the realigned observation (c3r_set_hap_realign): hap_observe_ra against the reference slice, with the switch's overhang.
struct HapAlleleRaArgs : HapAlleleLaArgs { uint32_t overhang; };

__global__ __launch_bounds__(PREP_THREADS) void k_hap_allele_counts_ra(const HapAlleleRaArgs a) {
    hap_count_read(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        return hap_observe_ra(e, R, rseq, a.pool, a.ref, a.overhang, q, last, iq, cx);
    });
}

// The same across splice junctions (c3r_set_hap_realign_spliced): hap_observe_rs, the _ra kernel's arguments.
__global__ __launch_bounds__(PREP_THREADS) void k_hap_allele_counts_rs(const HapAlleleRaArgs a) {
    hap_count_read(a, true, [&](const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        return hap_observe_rs(e, R, rseq, a.pool, a.ref, a.overhang, q, last, iq, cx);
    });
}

}  // namespace c3r
