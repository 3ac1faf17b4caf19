// realign.hpp — the rule `realign` of include/c3r.h (c3r_set_hap_realign) as code that compiles for the host and for gfx950: the map from a
// reference position to a query offset of a read, the two haplotype strings of a site, and the global unit-cost edit distance of the read's
// window to each.  Included by haplotag_kernels.hpp (hap_observe_ra: the four _ra kernels) and, through it, by c3r_lib.hip
// (c3r_hap_realign_column: the same functions on the host, no context and no device).  tests/realignref.py restates the rule on its own:
// a textbook DP and a CIGAR map of its own.  At the end of the file: the rule `realign_spliced` (c3r_set_hap_realign_spliced), whose window
// crosses an N op — new functions beside the old ones (hap_observe_rs: the five _rs kernels; c3r_hap_realign_column_spliced), which keep
// their code; tests/realignspliceref.py restates it.
//
// What it replaces: the realignment of a read's local window against the two alleles that stands behind `whatshap phase` and `whatshap
// haplotag` in the reference flow (run_clair3_rna:749-794) — here with unit costs, no quality weights and no affine gaps.
//
// The distance is Myers' bit-vector algorithm in Hyyrö's formulation for the GLOBAL distance (the horizontal delta of row 0 is +1): both
// strings are at most 64 long, so the vertical deltas of one column are two 64-bit words, a text character costs about a dozen 64-bit
// operations for each haplotype, and there is no table in LDS or in scratch.  A haplotype is held as the four match masks of its letters —
// named members picked by selects, never an array indexed at run time, which would live in scratch.  Nothing here is an array.
#pragma once
#include <stdint.h>

#include "../../include/c3r_types.h"

#if defined(__HIPCC__)
#define C3R_RA_FN __host__ __device__ __forceinline__
#else
#define C3R_RA_FN inline
#endif

namespace c3r {

constexpr uint32_t RA_MAX_W = 16;             // c3r_set_hap_realign: overhang 0 (off), 1 .. 16
constexpr uint32_t RA_MAX_LEN = 64;           // of a haplotype string and of a read window: one 64-bit word
constexpr uint32_t RA_NOTHING = 3u;           // no observation (hap_observe's HAP_NOTHING)

C3R_RA_FN uint32_t ra_nibble(const uint8_t *p, unsigned long long q) {
    const uint32_t byte = p[q >> 1];
    return (q & 1) ? (byte & 15u) : (byte >> 4);
}

// ---- the reference-to-query map -------------------------------------------------------------------------------------------------------
// q(s) and q(t) of the read whose CIGAR is cig[0 .. n_cig) and whose first reference base is pos, on the RAW CIGAR: an op of length 0, H and
// P consume nothing, = and X are M, S counts in the query offset.  ok: pos <= s, t lies under an M or a D of the read (t < the read's end),
// and no N op holds a position of [s, t].  An op code above X consumes nothing (a load refuses such a read before any kernel gets here).
struct RaSpan { unsigned long long qs, qt; bool ok; };
C3R_RA_FN RaSpan ra_query_span(const uint32_t *cig, uint32_t n_cig, long long pos, long long s, long long t) {
    RaSpan r;
    r.qs = 0; r.qt = 0; r.ok = false;
    if (pos > s) return r;
    long long x = pos;
    unsigned long long y = 0;
    bool have_s = false;
    for (uint32_t k = 0; k < n_cig; ++k) {
        const uint32_t c = cig[k], raw = c & 15u, len = c >> 4;
        const uint32_t op = (raw == C3R_CIG_EQ || raw == C3R_CIG_X) ? (uint32_t)C3R_CIG_M : raw;
        if (len == 0) continue;
        if (op == C3R_CIG_N) {
            if (x <= t && x + (long long)len > s) return r;            // an N op touches [s, t]
            x += len;
        } else if (op == C3R_CIG_M || op == C3R_CIG_D) {
            const long long xe = x + (long long)len;
            if (!have_s && s < xe) { r.qs = op == C3R_CIG_M ? y + (unsigned long long)(s - x) : y; have_s = true; }
            if (t < xe) { r.qt = op == C3R_CIG_M ? y + (unsigned long long)(t - x) : y; r.ok = true; return r; }
            x = xe;
            if (op == C3R_CIG_M) y += len;
        } else if (op == C3R_CIG_I || op == C3R_CIG_S) y += len;
    }
    return r;                                                           // the read ends at or before t
}

// ---- the two haplotype strings, packed ------------------------------------------------------------------------------------------------
// A string of n <= 64 letters as the match masks of A, C, G, T: bit j of ma is set when letter j is an A.  A letter that is none of the
// four (never pushed: the site is realignable) would match nothing.
struct RaHap {
    uint64_t ma, mc, mg, mt;
    uint32_t n;
    C3R_RA_FN void clear() { ma = 0; mc = 0; mg = 0; mt = 0; n = 0; }
    C3R_RA_FN void push(uint32_t code) {
        const uint64_t bit = 1ull << (n & 63u);
        ma |= code == 1u ? bit : 0ull; mc |= code == 2u ? bit : 0ull; mg |= code == 4u ? bit : 0ull; mt |= code == 8u ? bit : 0ull;
        ++n;
    }
    // the match mask of a read code: N, a masked base and every IUPAC code equal no letter
    C3R_RA_FN uint64_t eq(uint32_t code) const { return code == 1u ? ma : code == 2u ? mc : code == 4u ? mg : code == 8u ? mt : 0ull; }
};

// The window of a site: D and I (the larger DEL / INS length of its two alleles) and whether 2W + 1 + D + I <= 64.
struct RaWindow { uint32_t D, I; bool fits; };
C3R_RA_FN RaWindow ra_window(const c3r_hap_site_t &e, uint32_t W) {
    RaWindow w;
    const uint32_t da = e.a.kind == C3R_HAP_EV_DEL ? e.a.len : 0u, db = e.b.kind == C3R_HAP_EV_DEL ? e.b.len : 0u;
    const uint32_t ia = e.a.kind == C3R_HAP_EV_INS ? e.a.len : 0u, ib = e.b.kind == C3R_HAP_EV_INS ? e.b.len : 0u;
    w.D = da > db ? da : db; w.I = ia > ib ? ia : ib;
    w.fits = 2u * W + 1u + w.D + w.I <= RA_MAX_LEN;
    return w;
}
// Is every reference base of [s, t) an A, C, G or T of the slice?  Ref: code(p) -> 1, 2, 4, 8, or 0 outside the slice and for any other letter.
template <class Ref>
C3R_RA_FN bool ra_ref_ok(const Ref &ref, long long s, long long t) {
    bool ok = true;
    for (long long p = s; p < t; ++p) ok = ok && ref.code(p) != 0u;
    return ok;
}
// ref[s, p0) + X.base + X.ins + ref[p0 + 1 + X.del, t) of a realignable site
template <class Ref>
C3R_RA_FN RaHap ra_haplotype(const Ref &ref, const c3r_hap_allele_t &al, const uint8_t *pool, long long s, long long p0, long long t) {
    RaHap h;
    h.clear();
    for (long long p = s; p < p0; ++p) h.push(ref.code(p));
    h.push(al.base);
    if (al.kind == C3R_HAP_EV_INS)
        for (uint32_t j = 0; j < al.len; ++j) h.push(ra_nibble(pool, (unsigned long long)al.ins_off + j));
    for (long long p = p0 + 1 + (al.kind == C3R_HAP_EV_DEL ? (long long)al.len : 0ll); p < t; ++p) h.push(ref.code(p));
    return h;
}

// ---- the edit distance ----------------------------------------------------------------------------------------------------------------
// One text character into the column of one haplotype (1 <= h.n <= 64): pv / mv are the vertical deltas +1 / -1 of the column, d the
// distance in its last row.  Start: pv = ~0, mv = 0, d = h.n (the distance of the empty text).
C3R_RA_FN void ra_myers_step(const RaHap &h, uint32_t code, uint64_t &pv, uint64_t &mv, uint32_t &d) {
    const uint64_t eq = h.eq(code), top = 1ull << ((h.n - 1u) & 63u);
    const uint64_t xv = eq | mv;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv), mh = pv & xh;
    d += (ph & top) ? 1u : 0u;
    d -= (mh & top) ? 1u : 0u;
    ph = (ph << 1) | 1ull;                                              // (global: row 0 grows by one per text character)
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}
// dA, dB: the global unit-cost edit distances of the m <= 64 codes at q0 .. q0 + m - 1 of rseq to the two haplotype strings.
C3R_RA_FN void ra_distances(const RaHap &ha, const RaHap &hb, const uint8_t *rseq, unsigned long long q0, uint32_t m, uint32_t &dA, uint32_t &dB) {
    uint64_t pva = ~0ull, mva = 0, pvb = ~0ull, mvb = 0;
    uint32_t da = ha.n, db = hb.n;
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t code = ra_nibble(rseq, q0 + j);
        ra_myers_step(ha, code, pva, mva, da);
        ra_myers_step(hb, code, pvb, mvb, db);
    }
    dA = da; dB = db;
}

// ---- the observation ------------------------------------------------------------------------------------------------------------------
// The realigned column of one read at one site whose anchor the caller found under an M op: 0 (dA < dB), 1 (dB < dA), RA_NOTHING (a tie).
// realigned = false: the read is not realigned at the site and the return value means nothing — the caller takes hap_observe's column.
// The cheap tests come first: the window's size, then the scan of the CIGAR, then the reference bases.
template <class Ref>
C3R_RA_FN uint32_t ra_column(const c3r_hap_site_t &e, const uint8_t *pool, const Ref &ref, const uint32_t *cig, uint32_t n_cig, long long read_pos, uint32_t l_seq,
                             const uint8_t *rseq, uint32_t W, bool &realigned) {
    realigned = false;
    const RaWindow w = ra_window(e, W);
    if (W == 0u || !w.fits) return RA_NOTHING;
    const long long p0 = (long long)e.pos - 1, s = p0 - (long long)W, t = p0 + 1 + (long long)w.D + (long long)W;
    const RaSpan sp = ra_query_span(cig, n_cig, read_pos, s, t);
    if (!sp.ok || sp.qt > (unsigned long long)l_seq || sp.qt - sp.qs > (unsigned long long)RA_MAX_LEN) return RA_NOTHING;
    if (!ra_ref_ok(ref, s, t)) return RA_NOTHING;
    realigned = true;
    const RaHap ha = ra_haplotype(ref, e.a, pool, s, p0, t), hb = ra_haplotype(ref, e.b, pool, s, p0, t);
    uint32_t dA, dB;
    ra_distances(ha, hb, rseq, sp.qs, (uint32_t)(sp.qt - sp.qs), dA, dB);
    return dA < dB ? 0u : dB < dA ? 1u : RA_NOTHING;
}

// ---- the same across splice junctions (the rule `realign_spliced` of include/c3r.h; c3r_set_hap_realign_spliced) -------------------------
// The window is counted in the read's SPLICED positions x_0 < x_1 < ... — the reference positions under its M-like and D ops, never those
// under an N — and not in reference positions: ks = k0 - W and kt = k0 + 1 + D + W around the anchor's index k0.  An N consumes no query
// base, so the read's window stays one stretch of SEQ; only the reference side follows the read's own splicing, for both strings alike.
// tests/realignspliceref.py restates the rule on its own.  The simple form: two forward scans of the raw CIGAR in the lane that holds the
// M op — the first for k0, the read's number of spliced positions and the core test, the second for q(x_ks), q(x_kt) and the flank letters.

// Scan 1.  k0: the spliced index of p0; n: the spliced positions of the whole read; ok: p0 lies under an M or a D and no N op holds a
// position of the core [p0, p0 + D] (what the read has of it: that it reaches p0 + D is kt < n's to say).
struct RaAnchor { unsigned long long k0, n; bool ok; };
C3R_RA_FN RaAnchor ra_spliced_anchor(const uint32_t *cig, uint32_t n_cig, long long pos, long long p0, uint32_t D) {
    RaAnchor r;
    r.k0 = 0; r.n = 0; r.ok = false;
    if (pos > p0) return r;
    long long x = pos;
    unsigned long long c = 0;
    bool have = false, cut = false;
    for (uint32_t k = 0; k < n_cig; ++k) {
        const uint32_t w = cig[k], raw = w & 15u, len = w >> 4;
        if (len == 0) continue;
        if (raw == C3R_CIG_N) {
            cut = cut || (x <= p0 + (long long)D && x + (long long)len > p0);      // an N op touches the core
            x += len;
        } else if (raw == C3R_CIG_M || raw == C3R_CIG_D || raw == C3R_CIG_EQ || raw == C3R_CIG_X) {
            const long long xe = x + (long long)len;
            if (!have && p0 < xe) { r.k0 = c + (unsigned long long)(p0 - x); have = true; }
            x = xe;
            c += len;
        }
    }
    r.n = c;
    r.ok = have && !cut;
    return r;
}

// Scan 2.  q(x_ks) and q(x_kt), the letters of the left flank x_ks .. x_(k0-1) and of the tail x_kd .. x_(kt-1) (kd = k0 + 1 + D: what both
// strings share behind the core), and whether all those letters are A, C, G or T of the slice.  Introns are never read.  ks < k0 < kd <= kt
// and kt is an index of the read (the caller has tested it), so both offsets are found.
struct RaFlanks { RaHap left, tail; unsigned long long qs, qt; bool ref_ok; };
template <class Ref>
C3R_RA_FN RaFlanks ra_spliced_flanks(const Ref &ref, const uint32_t *cig, uint32_t n_cig, long long pos, unsigned long long ks, unsigned long long k0, unsigned long long kd,
                                     unsigned long long kt) {
    RaFlanks f;
    f.left.clear(); f.tail.clear(); f.qs = 0; f.qt = 0; f.ref_ok = true;
    long long x = pos;
    unsigned long long y = 0, c = 0;
    for (uint32_t k = 0; k < n_cig; ++k) {
        const uint32_t w = cig[k], raw = w & 15u, len = w >> 4;
        const bool m = raw == C3R_CIG_M || raw == C3R_CIG_EQ || raw == C3R_CIG_X;
        if (len == 0) continue;
        if (raw == C3R_CIG_N) x += len;
        else if (m || raw == C3R_CIG_D) {
            const unsigned long long ce = c + len;
            if (ks >= c && ks < ce) f.qs = m ? y + (ks - c) : y;
            for (unsigned long long i = ks > c ? ks : c; i < (k0 < ce ? k0 : ce); ++i) {
                const uint32_t code = ref.code(x + (long long)(i - c));
                f.ref_ok = f.ref_ok && code != 0u;
                f.left.push(code);
            }
            for (unsigned long long i = kd > c ? kd : c; i < (kt < ce ? kt : ce); ++i) {
                const uint32_t code = ref.code(x + (long long)(i - c));
                f.ref_ok = f.ref_ok && code != 0u;
                f.tail.push(code);
            }
            if (kt < ce) { f.qt = m ? y + (kt - c) : y; return f; }
            x += len;
            c = ce;
            if (m) y += len;
        } else if (raw == C3R_CIG_I || raw == C3R_CIG_S) y += len;
    }
    return f;
}

// left + X.base + X.ins + ref[p0 + 1 + X.del, p0 + 1 + D) + tail: the core holds no N, so its positions are consecutive
template <class Ref>
C3R_RA_FN RaHap ra_haplotype_spliced(const Ref &ref, const c3r_hap_allele_t &al, const uint8_t *pool, const RaHap &left, const RaHap &tail, long long p0, uint32_t D) {
    RaHap h = left;
    h.push(al.base);
    if (al.kind == C3R_HAP_EV_INS)
        for (uint32_t j = 0; j < al.len; ++j) h.push(ra_nibble(pool, (unsigned long long)al.ins_off + j));
    for (long long p = p0 + 1 + (al.kind == C3R_HAP_EV_DEL ? (long long)al.len : 0ll); p < p0 + 1 + (long long)D; ++p) h.push(ref.code(p));
    const uint32_t sh = h.n & 63u;                                      // (tail.n = W >= 1 and the whole fits: h.n <= 63 here)
    h.ma |= tail.ma << sh; h.mc |= tail.mc << sh; h.mg |= tail.mg << sh; h.mt |= tail.mt << sh;
    h.n += tail.n;
    return h;
}

// ra_column under realign_spliced: the same three results.
template <class Ref>
C3R_RA_FN uint32_t ra_column_spliced(const c3r_hap_site_t &e, const uint8_t *pool, const Ref &ref, const uint32_t *cig, uint32_t n_cig, long long read_pos, uint32_t l_seq,
                                     const uint8_t *rseq, uint32_t W, bool &realigned) {
    realigned = false;
    const RaWindow w = ra_window(e, W);
    if (W == 0u || !w.fits) return RA_NOTHING;
    const long long p0 = (long long)e.pos - 1;
    const RaAnchor an = ra_spliced_anchor(cig, n_cig, read_pos, p0, w.D);
    const unsigned long long kd = an.k0 + 1ull + w.D, kt = kd + W;
    if (!an.ok || an.k0 < (unsigned long long)W || kt >= an.n) return RA_NOTHING;
    if (!ra_ref_ok(ref, p0, p0 + 1 + (long long)w.D)) return RA_NOTHING;
    const RaFlanks f = ra_spliced_flanks(ref, cig, n_cig, read_pos, an.k0 - W, an.k0, kd, kt);
    if (!f.ref_ok || f.qt > (unsigned long long)l_seq || f.qt - f.qs > (unsigned long long)RA_MAX_LEN) return RA_NOTHING;
    realigned = true;
    const RaHap ha = ra_haplotype_spliced(ref, e.a, pool, f.left, f.tail, p0, w.D), hb = ra_haplotype_spliced(ref, e.b, pool, f.left, f.tail, p0, w.D);
    uint32_t dA, dB;
    ra_distances(ha, hb, rseq, f.qs, (uint32_t)(f.qt - f.qs), dA, dB);
    return dA < dB ? 0u : dB < dA ? 1u : RA_NOTHING;
}

}  // namespace c3r
