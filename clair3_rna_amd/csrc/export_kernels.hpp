// export_kernels.hpp — gfx950 kernels that take a batch's results off the device in the order and the form their host readers want (c3r_get_tensors,
// c3r_get_tokens, c3r_rows_begin[_ex]).  Included after pileup_kernels.hpp, which keeps the scans that number the kept rows and the exported tokens
// (launch_excl_scan: the column store uses them too), by c3r_lib.hip and tests/c/row_export_check.hip.
#pragma once
#include "pileup_kernels.hpp"

namespace c3r {

// The control words of row export (c3r_ctx::d_rowctl, mirrored in page-locked host memory): the packers' counters[0], [1] and two targets of device_excl_scan.
struct RowCtl {
    unsigned long long n_recs;    // k_pack_tokens / k_pack_rows: indel records handed out
    unsigned long long n_bytes;   // k_pack_rows: token bytes handed out (the kept sites' bytes lie back to back)
    int32_t n_keep;               // c3r_rows_begin_ex(drop_ref_calls): the rows kept
    int32_t export_toks;          // c3r_get_tokens: the tokens of all sites
    int32_t unused[10];
};
static_assert(sizeof(RowCtl) == 64 && offsetof(RowCtl, n_recs) == 0 && offsetof(RowCtl, n_bytes) == 8 && offsetof(RowCtl, n_keep) == 16 && offsetof(RowCtl, export_toks) == 20, "RowCtl layout");

// rows of a [n][row_ints] int32 table through an index (c3r_get_tensors: windows in position order)
// (x16: the source rows are int16 — the resident windows; idx null: row i)
__global__ __launch_bounds__(256) void k_gather_rows(const void *src, const int32_t *idx, int n, int row_ints, int32_t *dst, int x16) {
    const int lane = (int)(threadIdx.x & 63), nw = (int)(gridDim.x * (blockDim.x >> 6));
    for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < n; i += nw) {
        const size_t row = idx ? (size_t)idx[i] : (size_t)i;
        int32_t *d_ = dst + (size_t)i * row_ints;
        if (x16) {
            const int16_t *s_ = (const int16_t *)src + row * row_ints;
            for (int k = lane; k < row_ints; k += 64) d_[k] = (int32_t)s_[k];
        } else {
            const int32_t *s_ = (const int32_t *)src + row * row_ints;
            for (int k = lane; k < row_ints; k += 64) d_[k] = s_[k];
        }
    }
}
// c3r_get_tokens: the tokens of site 0, then of site 1, ... (the fused path writes a span's tokens where they arrive); n_tok per site first
__global__ __launch_bounds__(256) void k_site_ntok(const c3r_site_t *sites, int n, int32_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sites[i].n_tok;
    else if (i == n) out[i] = 0;
}
// A site's tokens lie in the order they arrived (tile_tokens); whoever takes them out puts them into BAM order = by read index (a read has
// at most one token per site).  One wavefront per site: rank of token k0 + lane among the site's n tokens, and among those that carry an
// indel (the packed form keeps the indel records apart).  Sites hold two or three tokens; a deep site's thousands cost n^2 / 64 steps.
__device__ __forceinline__ void site_tok_rank(const c3r_token_t *s_, int n, uint32_t my_read, int my_k, int lane, int &rank, int &rank_ind) {
    rank = 0; rank_ind = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        uint32_t oi = 0xffffffffu; int oind = 0;
        if (j < n) { oi = s_[j].read_idx; oind = s_[j].indel != 0 ? 1 : 0; }
        const int m = min(64, n - j0);
        for (int l = 0; l < m; ++l) {
            const uint32_t x = (uint32_t)__shfl((int)oi, l, 64);
            const int xi = __shfl(oind, l, 64);
            // (equal read indices cannot occur — one token per read and site — but a rank must be a permutation whatever the input)
            if (x < my_read || (x == my_read && j0 + l < my_k)) { ++rank; rank_ind += xi; }
        }
    }
}
__global__ __launch_bounds__(256) void k_export_tokens(const c3r_site_t *sites, const int32_t *dst_off, int n, const c3r_token_t *tok, c3r_token_t *out) {
    const int lane = (int)(threadIdx.x & 63), nw = (int)(gridDim.x * (blockDim.x >> 6));
    for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < n; i += nw) {
        const c3r_token_t *s_ = tok + sites[i].tok_off;
        int4 *d_ = reinterpret_cast<int4 *>(out + dst_off[i]);
        const int nt = sites[i].n_tok;
        for (int k0 = 0; k0 < nt; k0 += 64) {
            const int k = k0 + lane;
            int4 v = make_int4(0, 0, 0, 0);
            if (k < nt) v = reinterpret_cast<const int4 *>(s_)[k];
            int rank, rind;
            site_tok_rank(s_, nt, k < nt ? (uint32_t)v.x : 0xffffffffu, k, lane, rank, rind);
            if (k < nt) d_[rank] = v;
        }
    }
}


// ---- tokens for the row decoder, packed.  A token is 16 bytes (c3r_token_t) but the decoder reads the read index, the indel length
// and the query offset only of the few tokens that carry an indel; of all others it needs the base code.  One wavefront per site
// turns its tokens into one byte each (base code | 0x20 on the reverse strand | 0x80 when an indel record follows) and appends the indel records (TokRec, 16 bytes,
// token order kept by a ballot prefix) to a contiguous range it draws from one counter: a 250-Mb contig copies out ~60 MB instead
// of 760 MB.
struct TokRec { uint32_t read_idx; int32_t indel; uint32_t qpos; uint32_t del_after; };
static_assert(sizeof(TokRec) == 16, "TokRec must be 16 bytes");

// The work of one wavefront on one site: count the site's n_tok tokens (from tok[off]) that carry an indel, draw that many records from `counter`, write one byte per
// token to bytes[boff + rank in BAM order] and one TokRec per indel.  Lane 0 leaves the base it drew in *rec_slot at once (behind the loop the store's address costs registers).
__device__ __forceinline__ void pack_site(const c3r_token_t *__restrict__ tok, uint32_t off, int n_tok, int lane, uint8_t *__restrict__ bytes, uint32_t boff,
                                          TokRec *__restrict__ recs, uint32_t *__restrict__ rec_slot, unsigned long long *__restrict__ counter) {
    int cnt = 0;
    for (int i = lane; i < n_tok; i += 64) cnt += tok[off + i].indel != 0;
    for (int d = 32; d; d >>= 1) cnt += __shfl_xor(cnt, d);
    uint32_t base = 0;
    if (lane == 0) {
        base = cnt ? (uint32_t)atomicAdd(counter, (unsigned long long)cnt) : 0u;
        *rec_slot = base;
    }
    base = __shfl(base, 0);
    for (int i0 = 0; i0 < n_tok; i0 += 64) {
        const int i = i0 + lane;
        const bool valid = i < n_tok;
        c3r_token_t t{};
        if (valid) t = tok[off + i];
        int rank, rind;
        site_tok_rank(tok + off, n_tok, valid ? t.read_idx : 0xffffffffu, i, lane, rank, rind);     // BAM order
        const bool f = valid && t.indel != 0;
        if (valid) bytes[boff + rank] = (uint8_t)((t.base & 31) | (t.rev ? 0x20 : 0) | (f ? 0x80 : 0));
        if (f) recs[base + (uint32_t)rind] = TokRec{t.read_idx, t.indel, t.qpos, t.del_after};
    }
}

__global__ __launch_bounds__(256) void k_pack_tokens(const c3r_site_t *__restrict__ sites, const c3r_token_t *__restrict__ tok, int64_t n_sites,
                                                      uint8_t *__restrict__ bytes, TokRec *__restrict__ recs, uint32_t *__restrict__ rec_off,
                                                      unsigned long long *__restrict__ counter) {
    const int lane = threadIdx.x & 63;
    const int64_t site = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (site >= n_sites) return;
    const uint32_t off = sites[site].tok_off;
    pack_site(tok, off, sites[site].n_tok, lane, bytes, off, recs, rec_off + site, counter);
}

// ---- row snapshots without the sites the decoder prints nothing for.  Without --show_ref a site whose probabilities take the early
// RefCall exit of the decoder (clair3_rna/call_variants.py:540-542: P(0/0) >= 0.5 and P(gt21 = ref ref) >= 0.5, decode.hpp call_site) leaves
// no row, whatever its alt_info says, and so does a site whose reference class wins the first round of the decoder's arg-max — together 97 %
// of the candidates of a trained model.  k_row_keep applies those very tests, an exclusive scan turns the flags into row numbers, and k_pack_rows moves only the kept sites: site record,
// probabilities, packed tokens.  keep[n] is the scan's sentinel.
__global__ __launch_bounds__(256) void k_row_keep(const c3r_site_t *__restrict__ sites, const float *__restrict__ probs, int n, int32_t *__restrict__ keep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { keep[i] = 0; return; }
    const char c = sites[i].ref33[C3R_FLANK];
    // iupac2acgt (decode.hpp): ACGTURYSWKMBDHVN -> ACGTTACCAGACAAAA, anything else A; then gt21 of the homozygous reference genotype
    int rr = 0;                                                               // AA
    if (c == 'C' || c == 'Y' || c == 'S' || c == 'B') rr = 4;                 // CC
    else if (c == 'G' || c == 'K') rr = 7;                                    // GG
    else if (c == 'T' || c == 'U') rr = 9;                                    // TT
    const float *p = probs + (size_t)i * C3R_NPROB;
    const float z0 = p[21], z1 = p[22], z2 = p[23];
    bool ref_call = z0 >= 0.5f && p[rr] >= 0.5f;
    // ... and the first round of the decoder's arg-max (call_site: `top == p_ref`): when no class product exceeds P(0/0) * P(gt21 = ref ref)
    // the site is a RefCall before alt_info is looked at.  The same float32 products (one IEEE multiply each); p_ref must be a normal
    // number so that a flushed denormal on either side cannot turn the comparison.
    if (!ref_call) {
        const float p_ref = z0 * p[rr];
        float top = 0.f;
        const int homo[4] = {0, 4, 7, 9}, het[6] = {1, 2, 3, 5, 6, 8};
#pragma unroll
        for (int k = 0; k < 4; ++k) top = fmaxf(top, z1 * p[homo[k]]);
#pragma unroll
        for (int k = 0; k < 6; ++k) top = fmaxf(top, z2 * p[het[k]]);
        top = fmaxf(top, fmaxf(z1 * p[15], z2 * p[15]));                      // InsIns
        top = fmaxf(top, fmaxf(z1 * p[10], z2 * p[10]));                      // DelDel
#pragma unroll
        for (int k = 0; k < 4; ++k) top = fmaxf(top, fmaxf(p[16 + k] * z2, p[11 + k] * z2));      // base + Ins, base + Del
        top = fmaxf(top, z2 * p[20]);                                         // InsDel
        ref_call = p_ref >= 1e-30f && p_ref >= top;
    }
    keep[i] = ref_call ? 0 : 1;
}
// idx: the exclusive scan of the keep flags ([n + 1]); counters: [0] indel records, [1] token bytes handed out
__global__ __launch_bounds__(256) void k_pack_rows(const c3r_site_t *__restrict__ sites, const c3r_token_t *__restrict__ tok, const float *__restrict__ probs,
                                                    const int32_t *__restrict__ idx, int64_t n_sites, c3r_site_t *__restrict__ sites_c, float *__restrict__ probs_c,
                                                    uint8_t *__restrict__ bytes, TokRec *__restrict__ recs, uint32_t *__restrict__ rec_off,
                                                    unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const int64_t site = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (site >= n_sites) return;
    const int j = idx[site];
    if (idx[site + 1] == j) return;                                           // not kept
    const uint32_t off = sites[site].tok_off;
    const int n_tok = sites[site].n_tok;
    uint32_t bbase = 0;
    if (lane == 0) bbase = (uint32_t)atomicAdd(&counters[1], (unsigned long long)n_tok);
    bbase = __shfl(bbase, 0);
    static_assert(sizeof(c3r_site_t) == 52 && offsetof(c3r_site_t, tok_off) == 48, "c3r_site_t layout");
    if (lane < 13) reinterpret_cast<uint32_t *>(&sites_c[j])[lane] = lane == 12 ? bbase : reinterpret_cast<const uint32_t *>(&sites[site])[lane];
    if (lane < C3R_NPROB) probs_c[(size_t)j * C3R_NPROB + lane] = probs[(size_t)site * C3R_NPROB + lane];
    pack_site(tok, off, n_tok, lane, bytes, bbase, recs, rec_off + j, &counters[0]);
}

}  // namespace c3r
