// phase_kernels.hpp — k_phase_links: pairwise linkage counts between the contig's heterozygous SNVs from the loaded reads (c3r_phase_links),
// the device half of the project's own phasing.  Included by c3r_lib.hip only.
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

struct LinkArgs {
    const DevRead *reads; int32_t n_reads;    // headers of k_prep<false>; read only
    const uint8_t *serial;                    // [n_reads] != 0: the read takes the serial walk
    const uint32_t *cigars;
    const uint8_t *seq;                       // 4-bit packed bases
    const c3r_phase_site_t *sites; int32_t n_sites;       // candidate sites (ps and h1 are not read)
    int32_t min_mq, excl_flags;               // the voters: read_kept
    uint32_t *links;                          // [n_sites][PHASE_K][2] cis / trans, zero on entry
};

__global__ __launch_bounds__(PREP_THREADS) void k_phase_links(const LinkArgs a) {
    __shared__ uint4 s_obs4[PREP_READS][PHASE_WIN / 16];
    __shared__ int s_nwin;
    const int tid = (int)threadIdx.x, gl = tid & (PREP_GRP - 1), slot = tid / PREP_GRP;
    const int i = (int)(blockIdx.x * PREP_READS) + slot;
    uint8_t *const obs = reinterpret_cast<uint8_t *>(s_obs4[slot]);
    if (tid == 0) s_nwin = 0;
    __syncthreads();
    int lo = 0, hi = 0, nwin = 0;
    bool serial = false;
    ReadInfo R;
    R.cig = a.cigars; R.pos = 0; R.n_cig = 0; R.l_seq = 0; R.read_idx = (uint32_t)i; R.wbits = 0; R.seq_off = 0; R.compat = 0; R.padbit = 0;
    if (i < a.n_reads) {                                               // (whole groups take the branch: the ballots and shuffles below stay inside a group)
        const DevRead d = a.reads[i];
        if (read_kept(d.flag, d.mapq, a.min_mq, a.excl_flags)) {
            // the sites a base of the read can lie on: 0-based pos - 1 in [d.pos, d.end)
            lo = hap_lower_group(a.sites, 0, a.n_sites, (long long)d.pos + 1, gl);
            hi = hap_lower_group(a.sites, lo, a.n_sites, (long long)d.end + 1, gl);
            const int m = hi - lo;
            nwin = m < 2 ? 0 : m <= PHASE_WIN ? 1 : 1 + (m - PHASE_WIN + PHASE_STEP - 1) / PHASE_STEP;
            R.cig = a.cigars + d.cig_off; R.pos = d.pos; R.n_cig = d.n_cig; R.l_seq = d.l_seq; R.seq_off = d.seq_off;
            serial = a.serial[i] != 0;
        }
    }
    if (gl == 0 && nwin > 0) atomicMax(&s_nwin, nwin);
    __syncthreads();
    const int nwin_wg = s_nwin;
    for (int w = 0; w < nwin_wg; ++w) {
        const bool mine = w < nwin;
        const int ws = lo + w * PHASE_STEP, we = min(ws + PHASE_WIN, hi);                 // the window's sites
        if (mine) s_obs4[slot][gl] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        if (mine) {
            auto on_op = [&](uint32_t op, uint32_t len, long long x, uint32_t y, const OpCtx &) __attribute__((always_inline)) {
                if (op != C3R_CIG_M) return;
                for (int s = hap_lower(a.sites, ws, we, x + 1); s < we; ++s) {
                    const c3r_phase_site_t e = a.sites[s];
                    const long long d = (long long)e.pos - 1 - x;
                    if (d >= (long long)len) break;
                    const unsigned long long q = (unsigned long long)y + (unsigned long long)d;
                    if (q >= R.l_seq) break;                                   // (the later sites of this op lie further out still)
                    const uint32_t byte = a.seq[R.seq_off + (q >> 1)], b = (q & 1) ? (byte & 15u) : (byte >> 4);
                    if (b == e.ref) obs[s - ws] = 1; else if (b == e.alt) obs[s - ws] = 2;
                }
            };
            if (!serial) walk_plain_ops(R, gl, on_op);
            else if (gl == 0) (void)walk_serial_ops(R, on_op);
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

}  // namespace c3r
