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
// Each tagging kernel has a _w sibling (c3r_set_hap_bq_weights): the same body with HapTallyW, which weighs a vote by the quality byte of
// the read's base on the site and stores the chosen set's (w1, w2) per read.
//
// The pieces that every kernel which holds reads against a sorted site table shares are here as well (hapcount_kernels.hpp and
// phase_kernels.hpp include this file): ReadArgs, GroupAt, read_sites, walk_sites, hap_nibble, snv_column, hap_observe, hap_observe_la,
// hap_observe_ra, hap_observe_rs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "reads_kernels.hpp"
#include "realign.hpp"

namespace c3r {

// ---- shared by the six per-read kernels over a site table (this file, hapcount_kernels.hpp, phase_kernels.hpp) -------------------------------
// What c3r_load_reads left on the device: the base of every such kernel's arguments (c3r_lib.hip: read_args fills it).
struct ReadArgs {
    const DevRead *reads; int32_t n_reads;    // headers of k_prep<false>
    const uint8_t *serial;                    // [n_reads] != 0: the read takes the serial walk
    const uint32_t *cigars;
    const uint8_t *seq;                       // 4-bit packed bases
};

// Where a thread stands: its lane in the 16-lane group, the group's slot in the workgroup and the group's read (may lie past n_reads).
struct GroupAt {
    int gl, slot, i;
    __device__ __forceinline__ GroupAt() : gl((int)threadIdx.x & (PREP_GRP - 1)), slot((int)threadIdx.x / PREP_GRP), i((int)(blockIdx.x * PREP_READS) + slot) {}
};

// first site of [lo, hi) with pos >= p (hi: none).  Site: any record with a `pos` (c3r_phase_site_t, c3r_hap_site_t)
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

// The sites [lo, hi) a base of read d can lie on: 0-based pos - 1 in [d.pos, d.end).  Every kernel calls it once per read; all lanes of the
// group call it together, with the same arguments, and all get the range (nothing here leaves the kernel: k_phase_links' threads stay).
struct SiteRange { int lo, hi; };
template <class Site>
__device__ __forceinline__ SiteRange read_sites(const Site *sites, int n_sites, const DevRead &d, int gl) {
    SiteRange r;
    r.lo = hap_lower_group(sites, 0, n_sites, (long long)d.pos + 1, gl);
    r.hi = hap_lower_group(sites, r.lo, n_sites, (long long)d.end + 1, gl);
    return r;
}

__host__ __device__ __forceinline__ uint32_t hap_nibble(const uint8_t *p, unsigned long long q) { return ra_nibble(p, q); }      // (realign.hpp owns it)

// One walk of a read over the sites [lo, hi) (k_phase_links: a window of them) that its M ops cover: every M op searches its own stretch once.
// on_site(site index, site, query offset of the read's base there, is it the op's first base, is it the op's last base, query offset behind
// the op — where an insertion's bases start —, the op's neighbours) runs in the lane that holds the op.  Every kernel's walk; all lanes of the group come here together.
template <class Site, class OnSite>
__device__ __forceinline__ void walk_sites(const ReadInfo &R, int gl, bool serial, const Site *sites, int lo, int hi, OnSite &&on_site) {
    auto on_op = [&](uint32_t op, uint32_t len, long long x, uint32_t y, const OpCtx &cx) __attribute__((always_inline)) {
        if (op != C3R_CIG_M) return;
        for (int s = hap_lower(sites, lo, hi, x + 1); s < hi; ++s) {
            const Site e = sites[s];
            const long long dd = (long long)e.pos - 1 - x;
            if (dd >= (long long)len) break;
            const unsigned long long q = (unsigned long long)y + (unsigned long long)dd;
            if (q >= R.l_seq) break;                                   // (the later sites of this op lie further out still)
            on_site(s, e, q, dd == 0, dd == (long long)len - 1, (unsigned long long)y + len, cx);
        }
    };
    if (!serial) walk_plain_ops(R, gl, on_op);
    else if (gl == 0) (void)walk_serial_ops(R, on_op);
}

// The column of a biallelic SNV that base b shows: 0 ref, 1 alt, 2 neither (k_hap_counts: `other` for A, C, G, T; the others: nothing).
__device__ __forceinline__ uint32_t snv_column(const c3r_phase_site_t &e, uint32_t b) { return b == e.ref ? 0u : b == e.alt ? 1u : 2u; }
__host__ __device__ __forceinline__ bool hap_is_acgt(uint32_t b) { return b == 1u || b == 2u || b == 4u || b == 8u; }      // (not =, N, IUPAC)

// The column of an allele site (SNV, insertion, deletion, two-ALT; the rule of include/c3r.h) that the read shows: 0 allele A, 1 allele B,
// 2 another allele, HAP_NOTHING no observation.  The lane that holds the M op decides: the read's base on the anchor and — on the op's LAST
// base only — the event behind it from the op's neighbours: an I (its bases start at query offset iq of the same read), a D, or an I with
// a D at once behind it (n2op), which is the `+<ins>-<del>` column and matches no allele.  A pad kept before a D, an N, an S and the read's
// end are no event.  Adjacent M-like ops of a plain CIGAR (`3M2=`) are one op of the normalised form: the first one's last base sees
// nop = M, no event, which is what the merged op says.  Insertions are compared nibble by nibble: the read's offset and the pool's have
// independent parity.  walk_sites' arguments; called by k_hap_allele_counts (2 is a column) and k_haplotag_alleles (2 is no vote).
// n2op: walk_serial_ops always fills it; walk_plain_ops fills it only with ReadInfo::compat set, so both kernels set compat = 1 for the
// reads of the plain walk (there it costs the loads of two more neighbours next to an insertion and nothing else) and leave it 0 for
// the serial walk, where compat would also run mpileup_compat's scan of the pads inside insertions, which this rule does not know.
constexpr uint32_t HAP_EV_OTHER = 3u;         // an insertion with a deletion at once behind it: equals no allele's kind
constexpr uint32_t HAP_NOTHING = RA_NOTHING;  // no observation (realign.hpp owns the value)
__host__ __device__ __forceinline__ uint32_t hap_observe(const c3r_hap_site_t &e, const uint8_t *rseq, uint32_t l_seq, const uint8_t *pool, unsigned long long q, bool last,
                                                unsigned long long iq, const OpCtx &cx) {
    const uint32_t b = hap_nibble(rseq, q);
    if (e.base_matters && !hap_is_acgt(b)) return HAP_NOTHING;
    uint32_t ek = C3R_HAP_EV_NONE, en = 0;
    if (e.event_matters && last) {
        if (cx.nop == C3R_CIG_I) {
            if (cx.n2op == C3R_CIG_D) ek = HAP_EV_OTHER;
            else if (iq + cx.nlen > l_seq) return HAP_NOTHING;         // (SEQ ends inside the insertion)
            else { ek = C3R_HAP_EV_INS; en = cx.nlen; }
        } else if (cx.nop == C3R_CIG_D) { ek = C3R_HAP_EV_DEL; en = cx.nlen; }
    }
    auto shows = [&](const c3r_hap_allele_t &al) __attribute__((always_inline)) {
        if (e.base_matters && b != al.base) return false;
        if (!e.event_matters) return true;
        if (ek != al.kind || en != al.len) return false;               // (NONE: both lengths are 0)
        if (ek != C3R_HAP_EV_INS) return true;
        for (uint32_t j = 0; j < en; ++j)
            if (hap_nibble(rseq, iq + j) != hap_nibble(pool, (unsigned long long)al.ins_off + j)) return false;
        return true;
    };
    return shows(e.a) ? 0u : shows(e.b) ? 1u : 2u;
}

// ---- the left-aligned observation (c3r_set_hap_left_align; the rule `left_align` of include/c3r.h, restated by tests/leftalignref.py) ----------
// The reference slice of c3r_set_reference as the four allele kernels read it: upper-case ASCII, 0-based position p at ref[p - beg0].
struct HapRef {
    const uint8_t *ref; int32_t beg0, len;
    // base code 1, 2, 4, 8 of position p; 0: outside the slice, or not A, C, G, T (either stops a shift)
    __device__ __forceinline__ uint32_t code(long long p) const {
        const long long o = p - beg0;
        if (o < 0 || o >= (long long)len) return 0u;
        const uint32_t c = ref[o];
        return c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 4u : c == 'T' ? 8u : 0u;
    }
};

// Does the read's CIGAR hold two M-like ops in a row (`3M2=`)?  The plain walk hands them out as two ops, and the left-aligned observation
// needs the whole run — its first base and its distance to the event —, so with the switch on such a read takes the serial walk, which
// hands out the normalised form.  By the 16 lanes together; all return the group's answer.
__device__ __forceinline__ bool cigar_has_m_neighbours(const ReadInfo &R, int gl) {
    int o = 0;
    for (uint32_t k0 = 0; k0 < R.n_cig; k0 += PREP_GRP) {
        const uint32_t k = k0 + (uint32_t)gl;
        if (k > 0 && k < R.n_cig && fold_op(R.cig[k]) == C3R_CIG_M && fold_op(R.cig[k - 1]) == C3R_CIG_M) o = 1;
    }
#pragma unroll
    for (int off = PREP_GRP / 2; off > 0; off >>= 1) o |= __shfl_xor(o, off, PREP_GRP);
    return o != 0;
}
// hap_observe with the read's event brought to its left-most form inside its M run.  The op at hand is the whole run (see above): the site
// lies `tail` = iq - 1 - q bases before its last base, whose reference position is a = pos - 1 + tail, and the event E behind the run shows
// at this site when left_align shifts it by exactly `tail` — or by more, when this is the run's first base (the cap).  Every other site of the
// run sees no event.  Not shifted, and seen on the run's last base only: an I with a D at once behind it (OTHER) and an insertion that SEQ
// cuts off (no observation).  A run whose last base lies past SEQ carries no event.  The loop ends at the first step that fails: a read
// pays the length of the repeat it sits in, not of its run.  The shifted insertion s' is ref[pos .. pos + k) followed by the first n - k
// inserted bases of the read.
__device__ __forceinline__ uint32_t hap_observe_la(const c3r_hap_site_t &e, const uint8_t *rseq, uint32_t l_seq, const uint8_t *pool, const HapRef &ref, unsigned long long q,
                                                   bool first, unsigned long long iq, const OpCtx &cx) {
    const uint32_t b = hap_nibble(rseq, q);
    if (e.base_matters && !hap_is_acgt(b)) return HAP_NOTHING;
    uint32_t ek = C3R_HAP_EV_NONE, en = 0, k = 0;
    if (e.event_matters && iq - 1 < l_seq) {
        const unsigned long long tail = iq - 1 - q;
        if (cx.nop == C3R_CIG_I && (cx.n2op == C3R_CIG_D || iq + cx.nlen > l_seq)) {
            if (tail == 0) {
                if (cx.n2op != C3R_CIG_D) return HAP_NOTHING;
                ek = HAP_EV_OTHER;
            }
        } else if (cx.nop == C3R_CIG_I || cx.nop == C3R_CIG_D) {
            const bool ins = cx.nop == C3R_CIG_I;
            const uint32_t n = cx.nlen;
            const long long a = (long long)e.pos - 1 + (long long)tail;
            // step j: the anchor moves from a - j to a - j - 1 (an A, C, G, T of the slice too) when ref[a - j] equals the event's last base
            auto step = [&](unsigned long long j) __attribute__((always_inline)) {
                const uint32_t r = ref.code(a - (long long)j);
                if (r == 0u || ref.code(a - (long long)j - 1) == 0u) return false;
                const uint32_t t = (ins && j < n) ? hap_nibble(rseq, iq + n - 1 - j) : ref.code(a - (long long)j + n);
                return r == t;
            };
            unsigned long long j = 0;
            while (j < tail && step(j)) ++j;
            if (j == tail && (first || !step(tail))) { ek = ins ? C3R_HAP_EV_INS : C3R_HAP_EV_DEL; en = n; k = (uint32_t)min(tail, (unsigned long long)n); }
        }
    }
    auto shows = [&](const c3r_hap_allele_t &al) __attribute__((always_inline)) {
        if (e.base_matters && b != al.base) return false;
        if (!e.event_matters) return true;
        if (ek != al.kind || en != al.len) return false;               // (NONE: both lengths are 0)
        if (ek != C3R_HAP_EV_INS) return true;
        for (uint32_t j = 0; j < en; ++j) {
            const uint32_t s = j < k ? ref.code((long long)e.pos + j) : hap_nibble(rseq, iq + j - k);
            if (s != hap_nibble(pool, (unsigned long long)al.ins_off + j)) return false;
        }
        return true;
    };
    return shows(e.a) ? 0u : shows(e.b) ? 1u : 2u;
}

// ---- the realigned observation (c3r_set_hap_realign; the rule `realign` of include/c3r.h, restated by tests/realignref.py) --------------------
// hap_observe where the read is not realigned at the site, else the column of the smaller edit distance of the read's window to the two
// haplotype strings (realign.hpp: ra_column; a tie is no observation).  In the lane that holds the M op, like its two siblings; q(s) and q(t)
// lie under other ops, so that lane scans the read's raw CIGAR from its first op (ra_query_span) — the simple form: a read pays its ops
// once per site it covers.  Nothing of the walk is looked at before the fallback, so the result does not depend on the walk, and reads
// with adjacent M-like ops keep the plain walk.  __host__ too: c3r_hap_realign_column (c3r_lib.hip) is this function behind the serial walk.
template <class Ref>
__host__ __device__ __forceinline__ uint32_t hap_observe_ra(const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, const uint8_t *pool, const Ref &ref, uint32_t overhang,
                                                            unsigned long long q, bool last, unsigned long long iq, const OpCtx &cx, bool *realigned = nullptr) {
    bool ra;
    const uint32_t col = ra_column(e, pool, ref, R.cig, R.n_cig, (long long)R.pos, R.l_seq, rseq, overhang, ra);
    if (realigned) *realigned = ra;
    return ra ? col : hap_observe(e, rseq, R.l_seq, pool, q, last, iq, cx);
}
// The same across splice junctions (c3r_set_hap_realign_spliced; the rule `realign_spliced` of include/c3r.h, restated by
// tests/realignspliceref.py): ra_column_spliced in ra_column's place — two scans of the raw CIGAR per site in the place of one.
template <class Ref>
__host__ __device__ __forceinline__ uint32_t hap_observe_rs(const c3r_hap_site_t &e, const ReadInfo &R, const uint8_t *rseq, const uint8_t *pool, const Ref &ref, uint32_t overhang,
                                                            unsigned long long q, bool last, unsigned long long iq, const OpCtx &cx, bool *realigned = nullptr) {
    bool ra;
    const uint32_t col = ra_column_spliced(e, pool, ref, R.cig, R.n_cig, (long long)R.pos, R.l_seq, rseq, overhang, ra);
    if (realigned) *realigned = ra;
    return ra ? col : hap_observe(e, rseq, R.l_seq, pool, q, last, iq, cx);
}

// ---- the tags ---------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t HAP_NONE = 0xffffffffu;    // no phase set (ps is an int32 >= 0)

// What one walk over a read gathers in one lane, and in all lanes of the group after reduce().
struct HapTally {
    uint32_t c1, c2;          // votes for haplotype 1 / 2 in the phase set `cur` (HAP_NONE: in all sets)
    uint32_t first;           // table index of the first voting site of those (HAP_NONE: none)
    uint32_t ps_min, ps_max;  // smallest / largest phase set above `cur` that holds a vote (ps_min HAP_NONE: none)
    __device__ __forceinline__ void clear() { c1 = 0; c2 = 0; first = HAP_NONE; ps_min = HAP_NONE; ps_max = 0; }
    // one vote of site s, phase set ps.  cur = HAP_NONE: every vote counts and ps_min / ps_max span all sets; else only the votes of set
    // `cur` count and ps_min is the next set above it.  (hap_walk, hap_walk_alleles)
    __device__ __forceinline__ void vote(uint32_t cur, uint32_t ps, bool hap1, int s) {
        if (cur == HAP_NONE) { ps_min = min(ps_min, ps); ps_max = max(ps_max, ps); }
        else {
            if (ps > cur) ps_min = min(ps_min, ps);
            if (ps != cur) return;
        }
        if (hap1) c1 += 1; else c2 += 1;
        first = min(first, (uint32_t)s);
    }
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

// The tally of quality-weighted votes (c3r_set_hap_bq_weights; the rule `bq_weights` of include/c3r.h, restated by tests/hapweightref.py):
// c1 / c2 are sums of the quality bytes of the read's bases on the voting sites, n counts the observations (a Q0 base is one and adds
// nothing), and everything else — the sets, the first site, the shuffles — is HapTally's.
struct HapTallyW : HapTally {
    uint32_t n;               // observations that counted (a read's sum fits: l_seq x 254)
    __device__ __forceinline__ void clear() { HapTally::clear(); n = 0; }
    // HapTally::vote with the weight in the place of 1; qual[at] = 0xff — a record without qualities — weighs 1
    __device__ __forceinline__ void vote(uint32_t cur, uint32_t ps, bool hap1, int s, const uint8_t *qual, unsigned long long at) {
        if (cur == HAP_NONE) { ps_min = min(ps_min, ps); ps_max = max(ps_max, ps); }
        else {
            if (ps > cur) ps_min = min(ps_min, ps);
            if (ps != cur) return;
        }
        const uint32_t b = qual[at], w = b == 0xffu ? 1u : b;
        if (hap1) c1 += w; else c2 += w;
        n += 1;
        first = min(first, (uint32_t)s);
    }
    __device__ __forceinline__ void reduce() {
        HapTally::reduce();
#pragma unroll
        for (int off = PREP_GRP / 2; off > 0; off >>= 1) n += __shfl_xor(n, off, PREP_GRP);
    }
};

// What the two tagging kernels take beside their table.
struct HapTagArgs : ReadArgs {
    DevRead *hp_reads;                        // the same headers as `reads`, to write: hp is overwritten
    uint32_t *tags;                           // [n_reads] tag | votes of the read on all phase sets << 2
    int32_t *read_ps;                         // [n_reads] the phase set the tag was decided in, -1 when the tag is 0
};
// What a _w kernel takes beside its sibling's arguments.
template <class Base>
struct HapWeighted : Base {
    const uint8_t *qual;                      // one quality byte per base of `seq`: the base at query offset q of a read is qual[2 * seq_off + q]
    uint32_t *w12;                            // [n_reads][2] the weight sums (w1, w2) of the set the tag was decided in; a tie's pair when the tag is 0
};
// A tagging kernel and its _w sibling (HapWeighted<ARGS>) from one body, which names its arguments `a`, its tally `Tally` and the quality
// bytes `qual` (null in the unit form, which never reads them): the one place where the two forms part.  The body stands in the kernel
// itself: behind a function template of its own the compiler schedules the four kernels that were there before the weights differently
// (tools/device_asm_diff.py), and they are held to their code byte for byte.
#define C3R_HAPLOTAG_KERNELS(NAME, ARGS, ...)                                                                                            \
    __global__ __launch_bounds__(PREP_THREADS) void NAME(const ARGS a) { using Tally = HapTally; const uint8_t *const qual = nullptr; __VA_ARGS__ }      \
    __global__ __launch_bounds__(PREP_THREADS) void NAME##_w(const HapWeighted<ARGS> a) { using Tally = HapTallyW; const uint8_t *const qual = a.qual; __VA_ARGS__ }

// The tag of the group's read from walk(R, gl, serial, lo, hi, cur) -> HapTally, the reduced votes of one walk (steps 1 to 3 above), and
// lane 0's three stores.  compat_plain: ReadInfo::compat of a read of the plain walk.  LA: the left-aligned observation (cigar_has_m_neighbours).  The body of k_haplotag and k_haplotag_alleles; all
// lanes of a group take the same way through it (whole groups leave: the shuffles stay inside a group).
// With Tally = HapTallyW (the _w kernels, whose Args are HapWeighted) the sets are compared by weight, the tag word still holds the observations, and lane 0 stores the
// chosen set's (w1, w2) as well.
template <class Tally, bool LA = false, class Args, class Walk>
__device__ __forceinline__ void hap_tag_read(const Args &a, bool compat_plain, Walk &&walk) {
    constexpr bool weighted = !std::is_same<Tally, HapTally>::value;
    const GroupAt g;
    const int gl = g.gl, i = g.i;
    if (i >= a.n_reads) return;
    const DevRead d = a.reads[i];
    const SiteRange r = read_sites(a.sites, a.n_sites, d, gl);
    uint32_t tag = 0, votes = 0, set = HAP_NONE;
    if (r.lo < r.hi) {
        const bool serial = a.serial[i] != 0 || (LA && cigar_has_m_neighbours(ReadInfo(d, i, a.cigars, 0), gl));
        const ReadInfo R(d, i, a.cigars, compat_plain && !serial ? 1 : 0);
        Tally t = walk(R, gl, serial, r.lo, r.hi, HAP_NONE);
        if constexpr (weighted) votes = t.n; else votes = t.c1 + t.c2;        // (the observations behind c1 / c2)
        set = t.ps_min;                                                // (one set, or no vote: HAP_NONE)
        if (votes && t.ps_min != t.ps_max) {
            // several phase sets: one walk each, in the order of their numbers; the set with the most votes wins, the earlier first site among equals
            uint32_t best_n = 0, best_first = HAP_NONE, b1 = 0, b2 = 0;
            for (uint32_t cur = t.ps_min; cur != HAP_NONE;) {
                const Tally u = walk(R, gl, serial, r.lo, r.hi, cur);
                const uint32_t n = u.c1 + u.c2;
                if (n > best_n || (n == best_n && u.first < best_first)) { best_n = n; best_first = u.first; b1 = u.c1; b2 = u.c2; set = cur; }
                cur = u.ps_min;
            }
            t.c1 = b1; t.c2 = b2;
        }
        tag = t.c1 > t.c2 ? 1u : t.c2 > t.c1 ? 2u : 0u;
        if constexpr (weighted) { if (gl == 0) *(uint2 *)(a.w12 + 2 * (size_t)i) = make_uint2(t.c1, t.c2); }      // (a tie's pair too)
    } else if constexpr (weighted) {
        if (gl == 0) *(uint2 *)(a.w12 + 2 * (size_t)i) = make_uint2(0u, 0u);
    }
    if (gl == 0) {
        a.hp_reads[i].hp = (uint8_t)tag;
        a.tags[i] = tag | (votes << 2);
        a.read_ps[i] = tag ? (int32_t)set : -1;
    }
}

struct HapArgs : HapTagArgs {
    const c3r_phase_site_t *sites; int32_t n_sites;
};

// One walk: the votes of the sites [lo, hi) that the read's M ops cover.  All lanes of the group come here together.
// qual: the quality bytes of HapWeighted, read by HapTallyW only.
template <class Tally>
__device__ __forceinline__ Tally hap_walk(const ReadInfo &R, int gl, bool serial, const HapArgs &a, int lo, int hi, uint32_t cur, const uint8_t *qual) {
    Tally t;
    t.clear();
    const uint8_t *rseq = a.seq + R.seq_off;
    walk_sites(R, gl, serial, a.sites, lo, hi, [&](int s, const c3r_phase_site_t &e, unsigned long long q, bool, bool, unsigned long long, const OpCtx &) __attribute__((always_inline)) {
        const uint32_t al = snv_column(e, hap_nibble(rseq, q));
        if (al != 2u) {
            if constexpr (std::is_same<Tally, HapTally>::value) t.vote(cur, (uint32_t)e.ps, al == e.h1, s);
            else t.vote(cur, (uint32_t)e.ps, al == e.h1, s, qual, 2ull * R.seq_off + q);
        }
    });
    t.reduce();
    return t;
}

C3R_HAPLOTAG_KERNELS(k_haplotag, HapArgs,
    hap_tag_read<Tally>(a, false, [&](const ReadInfo &R, int gl, bool serial, int lo, int hi, uint32_t cur) __attribute__((always_inline)) { return hap_walk<Tally>(R, gl, serial, a, lo, hi, cur, qual); });
)

// ---- k_haplotag_alleles: the same tags from a table whose sites may be SNVs, insertions, deletions and two-ALT sites (c3r_set_phase_alleles) --
// The rule is stated in include/c3r.h and restated, independently of this file, by tests/hapindelref.py.  k_haplotag's shape — 16 lanes per
// read, the two group searches, the walks folded through HapTally, one further walk per phase set in the order of the sets' numbers, no LDS,
// no barrier, no atomics — with hap_observe in the place of the nibble compare.  Columns A and B vote — for haplotype 1 when the column
// equals the site's h1 —, column 2 and no observation do not.
// The table on the device is the caller's with one change: c3r_set_phase_alleles puts h1 into reserved[0] of its copy of every site, so
// that a site is one 32-byte load.
struct HapAlleleTagArgs : HapTagArgs {
    const c3r_hap_site_t *sites; int32_t n_sites;         // reserved[0] holds h1
    const uint8_t *pool;                      // the alleles' inserted bases, 4-bit packed like seq (never read when no allele is an insertion)
};

// hap_walk for the allele table; observe(site, walk_sites' arguments) -> hap_observe's column
template <class Tally, class Observe>
__device__ __forceinline__ Tally hap_walk_alleles(const ReadInfo &R, int gl, bool serial, const HapAlleleTagArgs &a, int lo, int hi, uint32_t cur, const uint8_t *qual, Observe &&observe) {
    Tally t;
    t.clear();
    walk_sites(R, gl, serial, a.sites, lo, hi, [&](int s, const c3r_hap_site_t &e, unsigned long long q, bool first, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
        const uint32_t al = observe(e, q, first, last, iq, cx);
        if (al < 2u) {
            if constexpr (std::is_same<Tally, HapTally>::value) t.vote(cur, (uint32_t)e.ps, al == e.reserved[0], s);
            else t.vote(cur, (uint32_t)e.ps, al == e.reserved[0], s, qual, 2ull * R.seq_off + q);
        }
    });
    t.reduce();
    return t;
}

C3R_HAPLOTAG_KERNELS(k_haplotag_alleles, HapAlleleTagArgs,
    hap_tag_read<Tally>(a, true, [&](const ReadInfo &R, int gl, bool serial, int lo, int hi, uint32_t cur) __attribute__((always_inline)) {
        const uint8_t *rseq = a.seq + R.seq_off;
        return hap_walk_alleles<Tally>(R, gl, serial, a, lo, hi, cur, qual, [&](const c3r_hap_site_t &e, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
            return hap_observe(e, rseq, R.l_seq, a.pool, q, last, iq, cx);
        });
    });
)

// The same with the left-aligned observation (c3r_set_hap_left_align): hap_observe_la against the reference slice.
struct HapAlleleTagLaArgs : HapAlleleTagArgs { HapRef ref; };

C3R_HAPLOTAG_KERNELS(k_haplotag_alleles_la, HapAlleleTagLaArgs,
    hap_tag_read<Tally, true>(a, true, [&](const ReadInfo &R, int gl, bool serial, int lo, int hi, uint32_t cur) __attribute__((always_inline)) {
        const uint8_t *rseq = a.seq + R.seq_off;
        return hap_walk_alleles<Tally>(R, gl, serial, a, lo, hi, cur, qual, [&](const c3r_hap_site_t &e, unsigned long long q, bool first, bool, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
            return hap_observe_la(e, rseq, R.l_seq, a.pool, a.ref, q, first, iq, cx);
        });
    });
)

// The same with the realigned observation (c3r_set_hap_realign): hap_observe_ra against the reference slice, with the switch's overhang.
struct HapAlleleTagRaArgs : HapAlleleTagLaArgs { uint32_t overhang; };

C3R_HAPLOTAG_KERNELS(k_haplotag_alleles_ra, HapAlleleTagRaArgs,
    hap_tag_read<Tally>(a, true, [&](const ReadInfo &R, int gl, bool serial, int lo, int hi, uint32_t cur) __attribute__((always_inline)) {
        const uint8_t *rseq = a.seq + R.seq_off;
        return hap_walk_alleles<Tally>(R, gl, serial, a, lo, hi, cur, qual, [&](const c3r_hap_site_t &e, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
            return hap_observe_ra(e, R, rseq, a.pool, a.ref, a.overhang, q, last, iq, cx);
        });
    });
)

// The same across splice junctions (c3r_set_hap_realign_spliced): hap_observe_rs, the _ra kernels' arguments.
C3R_HAPLOTAG_KERNELS(k_haplotag_alleles_rs, HapAlleleTagRaArgs,
    hap_tag_read<Tally>(a, true, [&](const ReadInfo &R, int gl, bool serial, int lo, int hi, uint32_t cur) __attribute__((always_inline)) {
        const uint8_t *rseq = a.seq + R.seq_off;
        return hap_walk_alleles<Tally>(R, gl, serial, a, lo, hi, cur, qual, [&](const c3r_hap_site_t &e, unsigned long long q, bool, bool last, unsigned long long iq, const OpCtx &cx) __attribute__((always_inline)) {
            return hap_observe_rs(e, R, rseq, a.pool, a.ref, a.overhang, q, last, iq, cx);
        });
    });
)
#undef C3R_HAPLOTAG_KERNELS

}  // namespace c3r
