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

struct HapCountArgs {
    const DevRead *reads; int32_t n_reads;    // headers of k_prep<false>; read only
    const uint8_t *serial;                    // [n_reads] != 0: the read takes the serial walk
    const uint32_t *cigars;
    const uint8_t *seq;                       // 4-bit packed bases
    const c3r_phase_site_t *sites; int32_t n_sites;       // query sites (h1 is not read)
    const uint32_t *tags;                     // [n_reads] k_haplotag's: tag in the low two bits
    const int32_t *read_ps;                   // [n_reads] k_haplotag's: the set the tag was decided in, -1 when the tag is 0
    int32_t min_mq, excl_flags;               // the voters: read_kept
    uint32_t *counts;                         // [n_sites][3][3] row (0, haplotype 1, 2) x allele (ref, alt, other), zero on entry
};

__global__ __launch_bounds__(PREP_THREADS) void k_hap_counts(const HapCountArgs a) {
    const int tid = (int)threadIdx.x, gl = tid & (PREP_GRP - 1);
    const int i = (int)(blockIdx.x * PREP_READS + (tid / PREP_GRP));
    if (i >= a.n_reads) return;                                        // (whole groups leave: the ballots of the searches stay inside a group)
    const DevRead d = a.reads[i];
    if (!read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags)) return;
    // the sites a base of the read can lie on: 0-based pos - 1 in [d.pos, d.end)
    const int lo = hap_lower_group(a.sites, 0, a.n_sites, (long long)d.pos + 1, gl), hi = hap_lower_group(a.sites, lo, a.n_sites, (long long)d.end + 1, gl);
    if (lo >= hi) return;
    ReadInfo R;
    R.cig = a.cigars + d.cig_off; R.pos = d.pos; R.n_cig = d.n_cig; R.l_seq = d.l_seq; R.read_idx = (uint32_t)i; R.wbits = 0; R.seq_off = d.seq_off;
    R.compat = 0; R.padbit = 0;
    const uint32_t tag = a.tags[i] & 3u;
    const int32_t set = tag ? a.read_ps[i] : -1;
    auto on_op = [&](uint32_t op, uint32_t len, long long x, uint32_t y, const OpCtx &) __attribute__((always_inline)) {
        if (op != C3R_CIG_M) return;
        for (int s = hap_lower(a.sites, lo, hi, x + 1); s < hi; ++s) {
            const c3r_phase_site_t e = a.sites[s];
            const long long dd = (long long)e.pos - 1 - x;
            if (dd >= (long long)len) break;
            const unsigned long long q = (unsigned long long)y + (unsigned long long)dd;
            if (q >= R.l_seq) break;                                   // (the later sites of this op lie further out still)
            const uint32_t byte = a.seq[R.seq_off + (q >> 1)], b = (q & 1) ? (byte & 15u) : (byte >> 4);
            if (b != 1u && b != 2u && b != 4u && b != 8u) continue;    // (=, N, IUPAC: nothing)
            const uint32_t al = b == e.ref ? 0u : b == e.alt ? 1u : 2u;
            const uint32_t row = e.ps == set ? tag : 0u;               // (set = -1 equals no query ps: they are >= 0)
            __hip_atomic_fetch_add(&a.counts[(size_t)s * 9 + row * 3 + al], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (a.serial[i] == 0) walk_plain_ops(R, gl, on_op);
    else if (gl == 0) (void)walk_serial_ops(R, on_op);
}

// ---- k_hap_allele_counts: the same table for sites whose two alleles may be SNVs, insertions or deletions (c3r_hap_allele_counts) ----------
// The rule is stated in include/c3r.h and restated, independently of this file, by tests/hapalleleref.py.  k_hap_counts' shape: 16 lanes per
// read, the two group searches, one walk, one relaxed add per observation, no LDS, no barrier, nothing reduced across lanes.  The lane that
// holds an M op decides everything for the sites under it: the read's base on the anchor, and — on the op's LAST base only — the event
// behind it from the op's neighbours (OpCtx): an I (nop; its bases start at query offset y + len of the same read), a D, or an I with a D
// at once behind it (n2op), which is the `+<ins>-<del>` column and matches no allele.  A pad kept before a D, an N, an S and the read's end
// are no event.  Adjacent M-like ops of a plain CIGAR (`3M2=`) are one op of the normalised form: the first one's last base sees nop = M,
// no event, which is what the merged op says.
// n2op: walk_serial_ops always fills it; walk_plain_ops fills it only with ReadInfo::compat set, so the kernel sets compat = 1 for the
// reads of the plain walk (there it costs the loads of two more neighbours next to an insertion and nothing else) and leaves it 0 for
// the serial walk, where compat would also run mpileup_compat's scan of the pads inside insertions, which this rule does not know.
// Insertions are compared nibble by nibble: the read's offset and the pool's have independent parity.
struct HapAlleleArgs {
    const DevRead *reads; int32_t n_reads;    // headers of k_prep<false>; read only
    const uint8_t *serial;                    // [n_reads] != 0: the read takes the serial walk
    const uint32_t *cigars;
    const uint8_t *seq;                       // 4-bit packed bases
    const c3r_hap_site_t *sites; int32_t n_sites;
    const uint8_t *pool;                      // the alleles' inserted bases, 4-bit packed like seq (never read when no allele is an insertion)
    const uint32_t *tags;                     // [n_reads] k_haplotag's: tag in the low two bits
    const int32_t *read_ps;                   // [n_reads] k_haplotag's: the set the tag was decided in, -1 when the tag is 0
    int32_t min_mq, excl_flags;               // the voters: read_kept
    uint32_t *counts;                         // [n_sites][3][3] row (0, haplotype 1, 2) x allele (A, B, other), zero on entry
};

// (HAP_EV_OTHER and hap_nibble: haplotag_kernels.hpp, where k_haplotag_alleles takes the same observation)
__global__ __launch_bounds__(PREP_THREADS) void k_hap_allele_counts(const HapAlleleArgs a) {
    const int tid = (int)threadIdx.x, gl = tid & (PREP_GRP - 1);
    const int i = (int)(blockIdx.x * PREP_READS + (tid / PREP_GRP));
    if (i >= a.n_reads) return;                                        // (whole groups leave: the ballots of the searches stay inside a group)
    const DevRead d = a.reads[i];
    if (!read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags)) return;
    const int lo = hap_lower_group(a.sites, 0, a.n_sites, (long long)d.pos + 1, gl), hi = hap_lower_group(a.sites, lo, a.n_sites, (long long)d.end + 1, gl);
    if (lo >= hi) return;
    const bool serial = a.serial[i] != 0;
    ReadInfo R;
    R.cig = a.cigars + d.cig_off; R.pos = d.pos; R.n_cig = d.n_cig; R.l_seq = d.l_seq; R.read_idx = (uint32_t)i; R.wbits = 0; R.seq_off = d.seq_off;
    R.compat = serial ? 0 : 1; R.padbit = 0;                           // (compat: n2op in the plain walk, see above)
    const uint8_t *rseq = a.seq + R.seq_off;
    const uint32_t tag = a.tags[i] & 3u;
    const int32_t set = tag ? a.read_ps[i] : -1;
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
            const uint32_t al = shows(e.a) ? 0u : shows(e.b) ? 1u : 2u;
            const uint32_t row = e.ps == set ? tag : 0u;               // (set = -1 equals no query ps: they are >= 0)
            __hip_atomic_fetch_add(&a.counts[(size_t)s * 9 + row * 3 + al], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (!serial) walk_plain_ops(R, gl, on_op);
    else if (gl == 0) (void)walk_serial_ops(R, on_op);
}

}  // namespace c3r
