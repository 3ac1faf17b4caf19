// haplotag_kernels.hpp — k_haplotag: every loaded read's haplotype from the contig's phased heterozygous SNVs (c3r_set_phase_sites), on the
// device, as part of read preparation; k_haplotag_alleles (at the end of this file): the same from a table that also holds phased insertions,
// deletions and two-ALT sites (c3r_set_phase_alleles).  Included by c3r_lib.hip only.
//
// What it replaces: the "Haplotag the BAM" step of the reference flow (run_clair3_rna:769-801: `whatshap haplotag` / `longphase haplotag` per
// contig, then `samtools index`), which rewrites the whole BAM to add one byte per read.  The rule is stated in include/c3r.h and restated,
// independently of this file, by tests/hapref.py.
//
// Where it runs: between the host wait of c3r_load_reads and k_prep<true>, so the records have passed k_prep<false>'s range checks (a load
// that fails them never gets here) and DevRead / `serial` are there.  It overwrites DevRead::hp — the one field all three consumers of a
// read's haplotype take it from (k_prep<true>: PileRec::w; the ordered recompute; k_legacy_write: DevSeg::hp) — and leaves the caller's
// records (d_rawreads) alone: without a table k_prep<false> copies their hp as before.
//
// 16 lanes per read, like k_prep, and the same two walks (walk_plain_ops / walk_serial_ops).  Per read:
//   1. two searches of the table for the read's span [pos, end), by the 16 lanes together (hap_lower_group): no site there (most reads of a
//      sample whose phased SNVs are a kilobase apart) and the CIGAR is never touched;
//   2. the walk: every M op searches its own stretch of the read's sites once and reads one nibble per site;
//   3. the lanes' votes meet by shuffles.  When all votes of the read lie in one phase set (the common case) that is all.  Otherwise the
//      phase sets are taken one at a time in the order of their numbers: each further walk counts the votes of one set and finds the next
//      number above it, so any number of sets — interleaved as they may be — is exact in P + 1 walks with no storage.
// The set the tag was decided in is kept beside the tag (read_ps): k_hap_counts (hapcount_kernels.hpp) counts a read on a haplotype only at
// the sites of that set.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reads_kernels.hpp"

namespace c3r {

struct HapArgs {
    DevRead *reads; int32_t n_reads;          // headers of k_prep<false>; hp is overwritten
    const uint8_t *serial;                    // [n_reads] != 0: the read takes the serial walk
    const uint32_t *cigars;
    const uint8_t *seq;                       // 4-bit packed bases
    const c3r_phase_site_t *sites; int32_t n_sites;
    uint32_t *tags;                           // [n_reads] tag | votes of the read on all phase sets << 2
    int32_t *read_ps;                         // [n_reads] the phase set the tag was decided in, -1 when the tag is 0
};

// first site of [lo, hi) with pos >= p (hi: none).  Site: any record with a `pos` (c3r_phase_site_t; c3r_hap_site_t in hapcount_kernels.hpp)
template <class Site>
__device__ __forceinline__ int hap_lower(const Site *sites, int lo, int hi, long long p) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)sites[mid].pos < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The same search by the 16 lanes of a read together: sixteen probes a round and a seventeenth of the candidates left after it (64 k sites:
// four dependent loads where hap_lower takes sixteen).  All lanes of the group call it, with the same arguments, and all return the index.
template <class Site>
__device__ __forceinline__ int hap_lower_group(const Site *sites, int lo, int hi, long long p, int gl) {
    const int shift = (int)(threadIdx.x & 63u) & ~(PREP_GRP - 1);              // where the group's lanes lie in the wavefront's ballot
    while (lo < hi) {
        const long long span = hi - lo;                                         // pivot g = lo + (g + 1) * span / 17: in [lo, hi), never decreasing with g
        const bool below = (long long)sites[lo + (int)(((long long)gl + 1) * span / (PREP_GRP + 1))].pos < p;
        const int c = __popc((uint32_t)(__ballot(below) >> shift) & ((1u << PREP_GRP) - 1u));          // pivots 0 .. c - 1 lie below p
        const int nlo = c > 0 ? lo + (int)((long long)c * span / (PREP_GRP + 1)) + 1 : lo;
        const int nhi = c < PREP_GRP ? lo + (int)(((long long)c + 1) * span / (PREP_GRP + 1)) : hi;
        lo = nlo; hi = nhi;
    }
    return lo;
}

constexpr uint32_t HAP_NONE = 0xffffffffu;    // no phase set (ps is an int32 >= 0)

// What one walk over a read gathers in one lane, and in all lanes of the group after reduce().
struct HapTally {
    uint32_t c1, c2;          // votes for haplotype 1 / 2 in the phase set `cur` (HAP_NONE: in all sets)
    uint32_t first;           // table index of the first voting site of those (HAP_NONE: none)
    uint32_t ps_min, ps_max;  // smallest / largest phase set above `cur` that holds a vote (ps_min HAP_NONE: none)
    __device__ __forceinline__ void clear() { c1 = 0; c2 = 0; first = HAP_NONE; ps_min = HAP_NONE; ps_max = 0; }
    __device__ __forceinline__ void reduce() {
#pragma unroll
        for (int off = PREP_GRP / 2; off > 0; off >>= 1) {
            c1 += __shfl_xor(c1, off, PREP_GRP);
            c2 += __shfl_xor(c2, off, PREP_GRP);
            first = min(first, (uint32_t)__shfl_xor(first, off, PREP_GRP));
            ps_min = min(ps_min, (uint32_t)__shfl_xor(ps_min, off, PREP_GRP));
            ps_max = max(ps_max, (uint32_t)__shfl_xor(ps_max, off, PREP_GRP));
        }
    }
};

// One walk: the votes of the sites [lo, hi) that the read's M ops cover.  cur = HAP_NONE: every vote counts and ps_min / ps_max span all
// sets; else only the votes of set `cur` count and ps_min is the next set above it.  All lanes of the group come here together.
__device__ __forceinline__ HapTally hap_walk(const ReadInfo &R, int gl, bool serial, const HapArgs &a, int lo, int hi, uint32_t cur) {
    HapTally t;
    t.clear();
    auto on_op = [&](uint32_t op, uint32_t len, long long x, uint32_t y, const OpCtx &) __attribute__((always_inline)) {
        if (op != C3R_CIG_M) return;
        for (int s = hap_lower(a.sites, lo, hi, x + 1); s < hi; ++s) {
            const c3r_phase_site_t e = a.sites[s];
            const long long d = (long long)e.pos - 1 - x;
            if (d >= (long long)len) break;
            const unsigned long long q = (unsigned long long)y + (unsigned long long)d;
            if (q >= R.l_seq) break;                                   // (the later sites of this op lie further out still)
            const uint32_t byte = a.seq[R.seq_off + (q >> 1)], b = (q & 1) ? (byte & 15u) : (byte >> 4);
            if (b != e.ref && b != e.alt) continue;
            const uint32_t ps = (uint32_t)e.ps;
            if (cur == HAP_NONE) { t.ps_min = min(t.ps_min, ps); t.ps_max = max(t.ps_max, ps); }
            else {
                if (ps > cur) t.ps_min = min(t.ps_min, ps);
                if (ps != cur) continue;
            }
            const uint32_t allele = b == e.alt ? 1u : 0u;
            if (allele == e.h1) t.c1 += 1; else t.c2 += 1;
            t.first = min(t.first, (uint32_t)s);
        }
    };
    if (!serial) walk_plain_ops(R, gl, on_op);
    else if (gl == 0) (void)walk_serial_ops(R, on_op);
    t.reduce();
    return t;
}

__global__ __launch_bounds__(PREP_THREADS) void k_haplotag(const HapArgs a) {
    const int tid = (int)threadIdx.x, gl = tid & (PREP_GRP - 1);
    const int i = (int)(blockIdx.x * PREP_READS + (tid / PREP_GRP));
    if (i >= a.n_reads) return;                                        // (whole groups leave: the shuffles below stay inside a group)
    const DevRead d = a.reads[i];
    // the sites a base of the read can lie on: 0-based pos - 1 in [d.pos, d.end)
    const int lo = hap_lower_group(a.sites, 0, a.n_sites, (long long)d.pos + 1, gl), hi = hap_lower_group(a.sites, lo, a.n_sites, (long long)d.end + 1, gl);
    uint32_t tag = 0, votes = 0, set = HAP_NONE;
    if (lo < hi) {
        ReadInfo R;
        R.cig = a.cigars + d.cig_off; R.pos = d.pos; R.n_cig = d.n_cig; R.l_seq = d.l_seq; R.read_idx = (uint32_t)i; R.wbits = 0; R.seq_off = d.seq_off;
        R.compat = 0; R.padbit = 0;
        const bool serial = a.serial[i] != 0;
        HapTally t = hap_walk(R, gl, serial, a, lo, hi, HAP_NONE);
        votes = t.c1 + t.c2;
        set = t.ps_min;                                                // (one set, or no vote: HAP_NONE)
        if (votes && t.ps_min != t.ps_max) {
            // several phase sets: one walk each, in the order of their numbers; the set with the most votes wins, the earlier first site among equals
            uint32_t best_n = 0, best_first = HAP_NONE, b1 = 0, b2 = 0;
            for (uint32_t cur = t.ps_min; cur != HAP_NONE;) {
                const HapTally u = hap_walk(R, gl, serial, a, lo, hi, cur);
                const uint32_t n = u.c1 + u.c2;
                if (n > best_n || (n == best_n && u.first < best_first)) { best_n = n; best_first = u.first; b1 = u.c1; b2 = u.c2; set = cur; }
                cur = u.ps_min;
            }
            t.c1 = b1; t.c2 = b2;
        }
        tag = t.c1 > t.c2 ? 1u : t.c2 > t.c1 ? 2u : 0u;
    }
    if (gl == 0) {
        a.reads[i].hp = (uint8_t)tag;
        a.tags[i] = tag | (votes << 2);
        a.read_ps[i] = tag ? (int32_t)set : -1;
    }
}

// ---- k_haplotag_alleles: the same tags from a table whose sites may be SNVs, insertions, deletions and two-ALT sites (c3r_set_phase_alleles) --
// The rule is stated in include/c3r.h and restated, independently of this file, by tests/hapindelref.py.  k_haplotag's shape — 16 lanes per
// read, the two group searches, the walks folded through HapTally, one further walk per phase set in the order of the sets' numbers, no LDS,
// no barrier, no atomics — with k_hap_allele_counts' observation (hapcount_kernels.hpp) in the place of the nibble compare: the lane that
// holds an M op decides, the event behind the anchor is read from OpCtx on the op's last base only, compat = 1 on the plain walk so that
// n2op is filled and 0 on the serial walk, insertions compared nibble by nibble against the pool.  Columns A and B vote — for haplotype 1
// when the column equals the site's h1 —, column 2 and no observation do not.  The observation is written out here a second time and not
// shared with k_hap_allele_counts: that kernel's text, and with it its registers, stay as they were.
// The table on the device is the caller's with one change: c3r_set_phase_alleles puts h1 into reserved[0] of its copy of every site, so
// that a site is one 32-byte load.
constexpr uint32_t HAP_EV_OTHER = 3u;         // an insertion with a deletion at once behind it: equals no allele's kind

__device__ __forceinline__ uint32_t hap_nibble(const uint8_t *p, unsigned long long q) {
    const uint32_t byte = p[q >> 1];
    return (q & 1) ? (byte & 15u) : (byte >> 4);
}

struct HapAlleleTagArgs {
    DevRead *reads; int32_t n_reads;          // headers of k_prep<false>; hp is overwritten
    const uint8_t *serial;                    // [n_reads] != 0: the read takes the serial walk
    const uint32_t *cigars;
    const uint8_t *seq;                       // 4-bit packed bases
    const c3r_hap_site_t *sites; int32_t n_sites;         // reserved[0] holds h1
    const uint8_t *pool;                      // the alleles' inserted bases, 4-bit packed like seq (never read when no allele is an insertion)
    uint32_t *tags;                           // [n_reads] tag | votes of the read on all phase sets << 2
    int32_t *read_ps;                         // [n_reads] the phase set the tag was decided in, -1 when the tag is 0
};

// hap_walk for the allele table; R.compat is set by the caller (1: plain walk, 0: serial walk).
__device__ __forceinline__ HapTally hap_walk_alleles(const ReadInfo &R, int gl, bool serial, const HapAlleleTagArgs &a, int lo, int hi, uint32_t cur) {
    HapTally t;
    t.clear();
    const uint8_t *rseq = a.seq + R.seq_off;
    auto on_op = [&](uint32_t op, uint32_t len, long long x, uint32_t y, const OpCtx &cx) __attribute__((always_inline)) {
        if (op != C3R_CIG_M) return;
        for (int s = hap_lower(a.sites, lo, hi, x + 1); s < hi; ++s) {
            const c3r_hap_site_t e = a.sites[s];
            const long long dd = (long long)e.pos - 1 - x;
            if (dd >= (long long)len) break;
            const unsigned long long q = (unsigned long long)y + (unsigned long long)dd;
            if (q >= R.l_seq) break;                                   // (the later sites of this op lie further out still)
            const uint32_t b = hap_nibble(rseq, q);
            if (e.base_matters && b != 1u && b != 2u && b != 4u && b != 8u) continue;      // (=, N, IUPAC: nothing)
            uint32_t ek = C3R_HAP_EV_NONE, en = 0;
            const unsigned long long iq = (unsigned long long)y + len;              // query offset of the bases of an insertion behind this op
            if (e.event_matters && dd == (long long)len - 1) {
                if (cx.nop == C3R_CIG_I) {
                    if (cx.n2op == C3R_CIG_D) ek = HAP_EV_OTHER;
                    else if (iq + cx.nlen > R.l_seq) continue;         // (SEQ ends inside the insertion: nothing)
                    else { ek = C3R_HAP_EV_INS; en = cx.nlen; }
                } else if (cx.nop == C3R_CIG_D) { ek = C3R_HAP_EV_DEL; en = cx.nlen; }
            }
            auto shows = [&](const c3r_hap_allele_t &al) __attribute__((always_inline)) {
                if (e.base_matters && b != al.base) return false;
                if (!e.event_matters) return true;
                if (ek != al.kind || en != al.len) return false;       // (NONE: both lengths are 0)
                if (ek != C3R_HAP_EV_INS) return true;
                for (uint32_t j = 0; j < en; ++j)
                    if (hap_nibble(rseq, iq + j) != hap_nibble(a.pool, (unsigned long long)al.ins_off + j)) return false;
                return true;
            };
            const uint32_t allele = shows(e.a) ? 0u : shows(e.b) ? 1u : 2u;
            if (allele == 2u) continue;                                // (another allele: no vote)
            const uint32_t ps = (uint32_t)e.ps;
            if (cur == HAP_NONE) { t.ps_min = min(t.ps_min, ps); t.ps_max = max(t.ps_max, ps); }
            else {
                if (ps > cur) t.ps_min = min(t.ps_min, ps);
                if (ps != cur) continue;
            }
            if (allele == e.reserved[0]) t.c1 += 1; else t.c2 += 1;
            t.first = min(t.first, (uint32_t)s);
        }
    };
    if (!serial) walk_plain_ops(R, gl, on_op);
    else if (gl == 0) (void)walk_serial_ops(R, on_op);
    t.reduce();
    return t;
}

__global__ __launch_bounds__(PREP_THREADS) void k_haplotag_alleles(const HapAlleleTagArgs a) {
    const int tid = (int)threadIdx.x, gl = tid & (PREP_GRP - 1);
    const int i = (int)(blockIdx.x * PREP_READS + (tid / PREP_GRP));
    if (i >= a.n_reads) return;                                        // (whole groups leave: the shuffles below stay inside a group)
    const DevRead d = a.reads[i];
    const int lo = hap_lower_group(a.sites, 0, a.n_sites, (long long)d.pos + 1, gl), hi = hap_lower_group(a.sites, lo, a.n_sites, (long long)d.end + 1, gl);
    uint32_t tag = 0, votes = 0, set = HAP_NONE;
    if (lo < hi) {
        const bool serial = a.serial[i] != 0;
        ReadInfo R;
        R.cig = a.cigars + d.cig_off; R.pos = d.pos; R.n_cig = d.n_cig; R.l_seq = d.l_seq; R.read_idx = (uint32_t)i; R.wbits = 0; R.seq_off = d.seq_off;
        R.compat = serial ? 0 : 1; R.padbit = 0;                       // (compat: n2op in the plain walk, as in k_hap_allele_counts)
        HapTally t = hap_walk_alleles(R, gl, serial, a, lo, hi, HAP_NONE);
        votes = t.c1 + t.c2;
        set = t.ps_min;                                                // (one set, or no vote: HAP_NONE)
        if (votes && t.ps_min != t.ps_max) {
            // several phase sets: k_haplotag's loop — one walk each, in the order of their numbers; most votes, the earlier first site among equals
            uint32_t best_n = 0, best_first = HAP_NONE, b1 = 0, b2 = 0;
            for (uint32_t cur = t.ps_min; cur != HAP_NONE;) {
                const HapTally u = hap_walk_alleles(R, gl, serial, a, lo, hi, cur);
                const uint32_t n = u.c1 + u.c2;
                if (n > best_n || (n == best_n && u.first < best_first)) { best_n = n; best_first = u.first; b1 = u.c1; b2 = u.c2; set = cur; }
                cur = u.ps_min;
            }
            t.c1 = b1; t.c2 = b2;
        }
        tag = t.c1 > t.c2 ? 1u : t.c2 > t.c1 ? 2u : 0u;
    }
    if (gl == 0) {
        a.reads[i].hp = (uint8_t)tag;
        a.tags[i] = tag | (votes << 2);
        a.read_ps[i] = tag ? (int32_t)set : -1;
    }
}

}  // namespace c3r
