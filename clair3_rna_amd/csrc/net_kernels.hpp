// net_kernels.hpp — gfx950 kernels for the Clair3-RNA pileup network (K2-K5).  Their operands are packed on the host by net_pack.hpp
// (which also defines the network's dimensions and the split-f16 scale); net_host.hpp uploads them and launches the kernels.
//
// What it replaces: clair3_rna/model.py:126-216 (Clair3_P: BiLSTM(128) -> BiLSTM(160) -> flatten ->
// Dense128 selu -> {Dense128 selu -> Dense21 selu -> softmax ; Dense128 selu -> Dense3 selu -> softmax})
// as run by m.predict_on_batch (clair3_rna/call_variants.py:1505).  Keras LSTM conventions: gates
// i,f,c,o; one bias; zero initial state; backward outputs stored at their original time index.
//
// Design.  fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32 (exact f32; the
// 1e-4 probability tolerance rules out plain bf16).  One workgroup = 32 candidate sites x one
// direction, persistent over the 33 time steps.  Per step it computes Z^T = W^T [4H x K] * act^T
// [K x 32 sites] with K = input||hidden, so input projection and recurrence are ONE fused GEMM and
// nothing but the layer output ever goes to HBM:
//   * MFMA rows  = gate columns, permuted at pack time so that each lane's 16 accumulator rows of a
//     32-row block are {4 gates} x {4 consecutive hidden units}  -> the LSTM cell update is lane-local
//     (no cross-lane / LDS exchange of gates), cell state c stays in registers for all 33 steps;
//   * MFMA cols  = sites; the B operand (activations) is one ds_read_b128 per lane per 8 k's from an
//     LDS tile act[32][K+4] (row stride chosen conflict-free for b128 reads);
//   * the A operand (weights) streams from L2 as one fully coalesced global_load_dwordx4 per lane per
//     8 k's from a layout pre-packed on the host in exact fragment order;
//   * 4 wavefronts split the 4H/32 row blocks evenly (H=128: 4 each, H=160: 5 each).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>

#include "../../include/c3r.h"
#include "net_pack.hpp"       // NET_H1, NET_H2, NET_T, NET_FLAT, NET_L4, WSCALE_LOG2, WSCALE, WUNSCALE

namespace c3r {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int NET_SITES = 32;              // sites per MFMA column block
constexpr int LSTM_SB = 2;                 // column blocks per wavefront in k_lstm
constexpr int LSTM_SITES = NET_SITES * LSTM_SB;
// The split-f16 kernels (k_lstm1_rs, k_lstm2_w16, k_lstm2_mx) run on the grid (2, groups): blockIdx.x is the direction, so the two
// directions of a site group are dispatched back to back.  (The alternatives that were measured and closed: DESIGN.md §kernels.)
// y1 (6.8 GB per chr20 pass) and a4part are written once and read once, and layer 2's hot set — a direction's weights and its W4p time
// slices, 3.8 MB — is nearly the whole of an XCD's 4 MB L2: the single-use streams carry the non-temporal policy (layer 2's LDS-DMA of
// y1, k_lstm1_rs's y1 stores, layer 2's a4part stores), the weights do not.
constexpr int Y1_NT_AUX = 2;      // __builtin_amdgcn_global_load_lds's cache policy: bit 1 = nt
template <class V, class P>
__device__ __forceinline__ void y1_store(V v, P p) {
    __builtin_nontemporal_store(v, p);
}

// sigmoid / tanh on the hardware transcendentals: v_exp_f32 + v_rcp_f32 (about 1 ulp each), no IEEE division
// sequence.  exp2 overflow -> inf -> rcp 0; underflow -> 0 -> rcp(1) = 1, so both saturate correctly.
__device__ __forceinline__ float fast_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float fast_tanh(float x) {
    return fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.8853900817779268f * x)), -1.0f);
}
// (1 - b) / ((1 + a)(1 + b)) with a, b = exp2 values: sigmoid(i) * tanh(g) and sigmoid(o) * tanh(c) of the cell update.
// Written with explicit FMAs — t = 1 + a, d = t * b + t, r = 1 / d, r - b * r — 3 VALU operations + 1 rcp instead of 5 + 1.
// b is always clamped (fminf(.., 1e18f) at the call sites): b = inf would give r - inf * 0 = NaN.  a = inf gives d = inf, r = 0 and
// the result 0 — the limit of sigmoid — but only while b > 0: with b = 0, t * b + t is inf * 0 + inf = NaN.  So a keeps its clamp in
// i * g, where g's exp2 underflows to 0 from a pre-activation of +52 on, and goes without it in o * tanh(c), where |c| <= 33 (it grows
// by at most one a step) keeps b above 2^-96.
__device__ __forceinline__ float gate_frac(float a, float b) {
    const float t = 1.0f + a;
    const float r = __builtin_amdgcn_rcpf(fmaf(t, b, t));
    return fmaf(-b, r, r);
}
// Value barrier of the cell updates: the value passes through one VGPR as it is.  Put on the results of the two FMA groups of a cell
// update (i*g, f*c + i*g) it keeps the SLP vectoriser from pairing neighbouring cells into v_pk_fma_f32, which is slower than the two
// v_fma_f32 it replaces beside MFMAs (measured in both layers: profiles/lstm_issue_stream_ab.txt); no instruction is emitted for it.
__device__ __forceinline__ float cell_fence(float x) {
    asm("" : "+v"(x));
    return x;
}
// The split of two cells' h into f16 pairs, hi = f16(h) and lo = f16(h - hi) (both round-to-nearest-even), in four instructions:
// v_cvt_pk_f16_f32 of the two h, one v_fma_mix_f32 per cell that reads its f16 half of the packed register directly (-hi * 1 + h,
// exact in fp32), v_cvt_pk_f16_f32 of the two differences.  h enters through a value barrier, so it is evaluated once, in fp32
// (without it the compiler forms it three times: v_fma_f32, v_fma_mixlo_f16 and v_fma_mixhi_f16 of the same operands).
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_h2(float h0, float h1, half2v &hi, half2v &lo, float &d0, float &d1) {
    asm("" : "+v"(h0));
    asm("" : "+v"(h1));
    const float2v h = {h0, h1};
    hi = __builtin_convertvector(h, half2v);
    // (the compiler has no pattern that reaches v_fma_mix_f32 from h - (float)hi: it converts first, then subtracts)
    // -hi * 1.0 + h: the f16 half negated by its source modifier; the inline constant 1.0 in an f16-selected source reads as f16 1.0
    // (outputs bit-identical to the constant in an SGPR and to the plain conversions on a fenced h: profiles/lstm_issue_stream_ab.txt)
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel_hi:[1,1,0]" : "=v"(d0) : "v"(hi), "v"(h0));
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "=v"(d1) : "v"(hi), "v"(h1));
    const float2v d = {d0, d1};
    lo = __builtin_convertvector(d, half2v);
}
// The LSTM cell update of the split-f16 kernels (k_lstm1_rs, k_lstm2_w16, k_lstm2_mx) for a lane's N cells: zi, zf, zg, zo are the gate
// pre-activations as they leave the accumulators (still times the weight scale), K1 = -log2(e) / scale for the sigmoids, K2 = 2 K1 for
// tanh; c is updated in place, h receives o * tanh(c).  Nine stages, each over all N cells before the next begins: the transcendentals of
// one stage are independent and fill each other's latency.  tests/test_lstm_isa.py guards the instruction stream this compiles to.
template <int N>
__device__ __forceinline__ void lstm_cell_update(const float (&zi)[N], const float (&zf)[N], const float (&zg)[N], const float (&zo)[N],
                                                 float (&c)[N], float (&h)[N], const float K1, const float K2) {
    float ei[N], ef[N], eg[N], eo[N];
#pragma unroll
    for (int u = 0; u < N; ++u) ei[u] = fminf(__builtin_amdgcn_exp2f(K1 * zi[u]), 1e18f);
#pragma unroll
    for (int u = 0; u < N; ++u) ef[u] = __builtin_amdgcn_exp2f(K1 * zf[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) eg[u] = fminf(__builtin_amdgcn_exp2f(K2 * zg[u]), 1e18f);
#pragma unroll
    for (int u = 0; u < N; ++u) eo[u] = __builtin_amdgcn_exp2f(K1 * zo[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) ei[u] = cell_fence(gate_frac(ei[u], eg[u]));                                  // sigmoid(i) * tanh(g)
#pragma unroll
    for (int u = 0; u < N; ++u) ef[u] = __builtin_amdgcn_rcpf(1.0f + ef[u]);                                  // sigmoid(f)
#pragma unroll
    for (int u = 0; u < N; ++u) c[u] = cell_fence(fmaf(ef[u], c[u], ei[u]));
#pragma unroll
    for (int u = 0; u < N; ++u) eg[u] = fminf(__builtin_amdgcn_exp2f(-2.8853900817779268f * c[u]), 1e18f);
#pragma unroll
    for (int u = 0; u < N; ++u) h[u] = gate_frac(eo[u], eg[u]);                                               // sigmoid(o) * tanh(c)
}
__device__ __forceinline__ float selu(float x) {
    const float scale = 1.0507009873554805f, alpha = 1.6732632423543772f;
    return x > 0.f ? scale * x : scale * alpha * (__expf(x) - 1.0f);
}

// ------------------------------------------------------------------------------------------------
// Fused bidirectional LSTM layer.  grid = (ceil(n/32), 2 directions), block = 256.
//   INP   : input width padded to a multiple of 8 (zero columns / zero weight rows)
//   CIN   : real input width in memory
//   H     : hidden units
//   INT_IN: input is int32 (the pileup tensor) instead of float
// Wp: packed weights [dir][wave][g][tile][64 lanes] float4, bp: packed bias [dir][blk][32 rows]
// ABL: timing-only ablation bits for tools/lstm_probe.hip (0 in the product): 1 weights from one L1-hot group,
// 2 no gate math, 4 no y store, 8 no barrier, 16 constant x operand.
// SB : 32-site blocks per wavefront.  Every weight fragment fetched from L2 feeds SB MFMAs; the probe showed the
//      L2 weight stream, not the matrix pipe, limits SB = 1 (66 % of peak; 81 % with L1-hot weights).
template <int INP, int CIN, int H, bool INT_IN, int SB = 2, int ABL = 0>
__global__ __launch_bounds__(256, (SB == 1 ? 2 : 1)) void k_lstm(const void *__restrict__ xin, const float4 *__restrict__ Wp,
                                                                  const float *__restrict__ bp, float *__restrict__ y, int n,
                                                                  const int32_t *__restrict__ row_idx = nullptr /* INT_IN: row of site i in xin (null: i) */,
                                                                  int x16 = 0 /* INT_IN: the rows are int16 (the tensor build's windows), not int32 */) {
    constexpr int NGX = INP / 8;           // k-groups fed from the layer input (global memory)
    constexpr int NGH = H / 8;             // k-groups fed from h_{t-1} (LDS)
    constexpr int NG = NGX + NGH;
    constexpr int HP = H + 4;              // LDS row stride: conflict-free for ds_read_b128 (H=128: 132, H=160: 164)
    constexpr int NBLK = 4 * H / 32;
    constexpr int NT = NBLK / 4;           // 32-row blocks per wave
    constexpr int WG_SITES = 32 * SB;
    static_assert(INP % 16 == 0 && H % 32 == 0, "shape: even k-group counts for the ping-pong pipeline");
    __shared__ __attribute__((aligned(16))) float hbuf[2][WG_SITES][HP];   // h double buffer: one barrier per step

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, hh = lane >> 5;
    const int dir = blockIdx.y;
    const int site0 = blockIdx.x * WG_SITES;

    // weights of this wave: [g][tt][lane] float4, contiguous per k-group -> one base pointer + immediate offsets
    const float4 *wl = Wp + ((size_t)(dir * 4 + wave) * NG) * NT * 64 + lane;
    // bias enters through one extra MFMA per tile and step: A = bias column (k=0 half of the wave), B = 1
    float bias_a[NT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) bias_a[tt] = hh == 0 ? bp[((size_t)dir * NBLK + wave * NT + tt) * 32 + j] : 0.f;

    float cst[NT][SB][4];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int sb = 0; sb < SB; ++sb)
#pragma unroll
            for (int q = 0; q < 4; ++q) cst[tt][sb][q] = 0.f;

    for (int i = tid; i < WG_SITES * HP; i += 256) (&hbuf[0][0][0])[i] = 0.f;   // h_{-1} = 0
    __syncthreads();

    size_t xoff[SB];
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
        int sj = site0 + 32 * sb + j;
        if (sj >= n) sj = n - 1;
        if (INT_IN && row_idx) sj = row_idx[sj];
        xoff[sb] = (size_t)sj * NET_T * CIN;
    }

    for (int step = 0; step < NET_T; ++step) {
        const int t = dir ? NET_T - 1 - step : step;
        const int cur = step & 1, nxt = cur ^ 1;

        // B operand for k-group g of the input part: x_t[site][8g+4hh..+3] straight from global (rows stay in L1/L2
        // across the K loop); of the recurrent part: h_{t-1} from LDS.  Two separate loaders so every load site has
        // a static address space (a merged pointer select degrades to flat_load + vmcnt(0)).
        auto ldx = [&](int g, float4 (&b)[SB]) {
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) {
                if (ABL & 16) { b[sb] = make_float4(1.f, 0.5f, 0.25f, (float)g); continue; }
                if (INT_IN) {
                    const int k0 = 8 * g + 4 * hh;
                    if (x16) {
                        const int16_t *xp = (const int16_t *)xin + xoff[sb] + (size_t)t * CIN;
                        b[sb].x = (k0 + 0 < CIN) ? (float)xp[k0 + 0] : 0.f;
                        b[sb].y = (k0 + 1 < CIN) ? (float)xp[k0 + 1] : 0.f;
                        b[sb].z = (k0 + 2 < CIN) ? (float)xp[k0 + 2] : 0.f;
                        b[sb].w = (k0 + 3 < CIN) ? (float)xp[k0 + 3] : 0.f;
                    } else {
                        const int32_t *xp = (const int32_t *)xin + xoff[sb] + (size_t)t * CIN;
                        b[sb].x = (k0 + 0 < CIN) ? (float)xp[k0 + 0] : 0.f;
                        b[sb].y = (k0 + 1 < CIN) ? (float)xp[k0 + 1] : 0.f;
                        b[sb].z = (k0 + 2 < CIN) ? (float)xp[k0 + 2] : 0.f;
                        b[sb].w = (k0 + 3 < CIN) ? (float)xp[k0 + 3] : 0.f;
                    }
                } else {
                    b[sb] = *(const float4 *)((const float *)xin + xoff[sb] + (size_t)t * CIN + 8 * g + 4 * hh);
                }
            }
        };
        auto ldh = [&](int g, float4 (&b)[SB]) {
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) b[sb] = *(const float4 *)&hbuf[cur][32 * sb + j][8 * g + 4 * hh];
        };
        auto ldw = [&](int g, float4 (&a)[NT]) {
            const float4 *wg = wl + (size_t)((ABL & 1) ? 0 : g) * NT * 64;
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) a[tt] = wg[tt * 64];
        };

        floatx16 acc[NT][SB];
        {
            floatx16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = 0.f;
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                for (int sb = 0; sb < SB; ++sb) acc[tt][sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(bias_a[tt], 1.0f, z, 0, 0, 0);
        }
#define C3R_MMA_K(comp)                                                                                              \
    _Pragma("unroll") for (int tt = 0; tt < NT; ++tt) _Pragma("unroll") for (int sb = 0; sb < SB; ++sb)             \
        acc[tt][sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tt].comp, b[sb].comp, acc[tt][sb], 0, 0, 0);
        auto mma = [&](const float4 (&a)[NT], const float4 (&b)[SB]) {
            C3R_MMA_K(x) C3R_MMA_K(y) C3R_MMA_K(z) C3R_MMA_K(w)
        };
#undef C3R_MMA_K
        // Software-pipelined K loop with ping-pong registers: the operands of group g+1 are in flight while group g is
        // on the matrix pipe.  (h_{-1} = 0 is a zero-filled LDS buffer: straight-line loops keep hipcc's register
        // allocation sane; skipping the recurrent part at step 0 would save 1.2 % of the MFMAs.)
        // sched_barrier(0): hipcc's scheduler otherwise clusters the ping and pong loads at the loop top and the
        // waitcnt pass then has to drain everything (vmcnt(0)) before the first MFMA of each half.
        float4 a0[NT], a1[NT], b0[SB], b1[SB];
#define C3R_FENCE() __builtin_amdgcn_sched_barrier(0)
        ldw(0, a0);
        ldx(0, b0);
#pragma unroll 1
        for (int g = 0; g + 2 < NGX; g += 2) {
            C3R_FENCE(); ldw(g + 1, a1); ldx(g + 1, b1); C3R_FENCE();
            mma(a0, b0);
            C3R_FENCE(); ldw(g + 2, a0); ldx(g + 2, b0); C3R_FENCE();
            mma(a1, b1);
        }
        C3R_FENCE(); ldw(NGX - 1, a1); ldx(NGX - 1, b1); C3R_FENCE();
        mma(a0, b0);
        C3R_FENCE(); ldw(NGX, a0); ldh(0, b0); C3R_FENCE();
        mma(a1, b1);
#pragma unroll 1
        for (int g = 0; g + 2 < NGH; g += 2) {
            C3R_FENCE(); ldw(NGX + g + 1, a1); ldh(g + 1, b1); C3R_FENCE();
            mma(a0, b0);
            C3R_FENCE(); ldw(NGX + g + 2, a0); ldh(g + 2, b0); C3R_FENCE();
            mma(a1, b1);
        }
        C3R_FENCE(); ldw(NG - 1, a1); ldh(NGH - 1, b1); C3R_FENCE();
        mma(a0, b0);
        mma(a1, b1);
        C3R_FENCE();
#undef C3R_FENCE
        // ---- lane-local cell update: acc row 4q+m <-> gate m (i,f,g,o) of unit 8*blk + 4*hh + q
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) {
                float hq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (ABL & 2) { hq[q] = acc[tt][sb][4 * q] + acc[tt][sb][4 * q + 1] + acc[tt][sb][4 * q + 2] + acc[tt][sb][4 * q + 3]; continue; }
                    const float ig = fast_sigmoid(acc[tt][sb][4 * q + 0]);
                    const float fg = fast_sigmoid(acc[tt][sb][4 * q + 1]);
                    const float gg = fast_tanh(acc[tt][sb][4 * q + 2]);
                    const float og = fast_sigmoid(acc[tt][sb][4 * q + 3]);
                    const float c = fg * cst[tt][sb][q] + ig * gg;
                    cst[tt][sb][q] = c;
                    hq[q] = og * fast_tanh(c);
                }
                *(float4 *)&hbuf[nxt][32 * sb + j][8 * (wave * NT + tt) + 4 * hh] = make_float4(hq[0], hq[1], hq[2], hq[3]);
            }
        }
        if (!(ABL & 8)) __syncthreads();   // h_t complete; everyone is done reading h_{t-1}
        // ---- layer output y[site][t][dir*H + u]: coalesced 16-byte stores from the LDS copy of h_t
        constexpr int HV = H / 4;
        if (!(ABL & 4))
        for (int f = tid; f < WG_SITES * HV; f += 256) {
            const int row = f / HV, c4 = f % HV;
            const int s = site0 + row;
            if (s < n) {
                const float4 v = *(const float4 *)&hbuf[nxt][row][4 * c4];
                *(float4 *)(y + ((size_t)s * NET_T + t) * (2 * H) + dir * H + 4 * c4) = v;
            }
        }
    }
}

// ================================================================================================
// Split-f16 path ("f16x3"): fp32-equivalent GEMMs on the f16 matrix pipe (16x the f32 MFMA rate).
// Every fp32 operand v is carried as two halves v = hi + lo (hi = f16(v), lo = f16(v - hi): 22 significand bits)
// and every product is evaluated as  w_hi*x_hi + w_hi*x_lo + w_lo*x_hi  with fp32 accumulation inside
// v_mfma_f32_32x32x16_f16; the dropped lo*lo term is 2^-22 relative.  Weights are pre-scaled by 2^12 at pack time so
// that their lo halves stay normal f16 numbers; the scale is undone for free inside the gate math.  3 MFMAs of 32
// cycles replace 8 MFMAs of 64 cycles per 16 k's: 5.3x less matrix-pipe time at the same 1e-4 probability bar
// (tests/test_gpu_parity.py compares both paths with the fp32 oracle).
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float sigmoid_scaled(float acc) {   // sigmoid(acc * 2^-12)
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((-1.4426950408889634f * WUNSCALE) * acc));
}
__device__ __forceinline__ float tanh_scaled(float acc) {      // tanh(acc * 2^-12)
    return fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((-2.8853900817779268f * WUNSCALE) * acc)), -1.0f);
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

// Interleave plan for one scheduling region: NM MFMAs with NV global loads and ND LDS reads spread evenly between them
// (sched_group_barrier masks: 0x008 MFMA, 0x020 VMEM read, 0x100 DS read).  One wavefront per SIMD issues everything:
// a burst of 14 wave-wide 16-byte loads holds the issue port for a few hundred cycles and drains the matrix pipe's
// short queue, whereas one load every second MFMA hides completely (<= 5 fillers fit into a 32-cycle MFMA).
template <int NM, int NV, int ND>
__device__ __forceinline__ void sched_interleave() {
    constexpr int K = (NM / (NV + ND + 1)) > 0 ? (NM / (NV + ND + 1)) : 1;
    if constexpr (NV > 0 && NM >= K) {
        __builtin_amdgcn_sched_group_barrier(0x008, K, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        sched_interleave<NM - K, NV - 1, ND>();
    } else if constexpr (ND > 0 && NM >= K) {
        __builtin_amdgcn_sched_group_barrier(0x008, K, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        sched_interleave<NM - K, NV, ND - 1>();
    } else if constexpr (NM > 0) {
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
    }
}

// Operand layouts of the split-f16 kernels (32-row gate blocks permuted for a lane-local cell update, see k_lstm):
//   Wp  : [dir][quarter(4)][g][tile][hi|lo][64 lanes] half8  (k-groups of 16; lane half hh owns k = 16g + 8hh + 0..7; x 2^12)
//   xin : layer 1: int32 [n][33][CIN] (staged as up to four f16 integers that sum to the count exactly, k_lstm1_rs); layer 2: hi plane then lo plane, each f16 [33][CIN/8][nstride][8]
//   y   : hi plane then lo plane, each f16 [33][2H/8][nstride][8]
//   W4p : the flatten + Dense(128) layer L4, fused into layer 2: [dir][t][blk(4)][g(H/16)][hi|lo][64 lanes] half8, x 2^12; after every
//         step the fresh h_t is multiplied by the [160 x 128] slice of W4 that belongs to (t, direction) and accumulated in
//         registers; y2 is never written.  a4part: fp32 [n][2][128] partial pre-activations, one per direction (k_heads_mfma adds them)
//   ldw : the weight loader launders its base pointer through an empty asm (with literal k-group numbers hipcc precomputes every
//         load address: 520 registers -> scratch) and re-types it address_space(1) (a laundered GENERIC pointer becomes flat_load,
//         which returns out of order and forces vmcnt(0) lgkmcnt(0) drains)

// ------------------------------------------------------------------------------------------------
// Layer 2 (+ fused L4) with TWO wavefronts per SIMD: 512 threads, 64 sites x one direction per workgroup (k_lstm2_w16, k_lstm2_mx).
//
// Round 1's kernel ran one wavefront per SIMD (its 160 accumulator registers + the L4 accumulators + the prefetch ring need the
// whole 512-register file).  A wavefront issues in order, so everything that is not an MFMA — the weight and operand
// loads the ring cannot cover, the cell update (5 exp2 + 3 rcp per unit), the L4 pass with its unprefetched loads, two
// barriers — is time the matrix pipe sits out: 57 % busy.  Here the 20 gate-row tiles of a direction are dealt 3 + 2 to the
// two wavefronts of each SIMD (waves w and w+4 share a SIMD): a wavefront's accumulators shrink to 96 / 64 registers, the
// cell state returns to registers, and whenever one wavefront waits (loads, transcendental latency, barrier) its partner
// keeps the matrix pipe fed.  Weight traffic is unchanged (each wavefront streams only its own rows); the B operands are
// read from LDS by eight wavefronts instead of four (852 KB per step, a quarter of the LDS read rate).
//   * the 2-tile wavefronts also own the fused L4 rows: W4[t-1, dir] x h_{t-1} rides in the recurrent part of step t as a
//     third tile on the very same B fragments (h_{t-1} hi/lo) — no separate pass, its weights join the prefetch ring; in the
//     recurrent part both wavefronts of a SIMD therefore carry three tiles each;
//   * no workgroup barriers inside the time loop: the wavefronts meet through three LDS counters (x_t read by all / x_{t+1} landed /
//     h_t written by all), so that one wavefront's cell update runs under its SIMD partner's MFMAs.  x_t is dead after the input
//     part: the four 3-tile wavefronts issue the LDS-DMA of x_{t+1} after their recurrent part, and it lands under the cell update; h is
//     double-buffered because a wavefront's cell update now runs while others still read h_{t-1}.  LDS: 2 x 42 KB (h hi/lo) + 64 KB (x tile) = 148 KB.
//   Wp / W4p / bp / a4part: see "Operand layouts" above (the "quarter" sq = wave & 3 indexes them).
// Counters in LDS that only grow: arrive = release + one increment per wavefront, wait = spin until the count is reached, then acquire.
__device__ __forceinline__ void lds_arrive(int *c) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if ((threadIdx.x & 63) == 0) atomicAdd(c, 1);
}
// A wait that gives up (2^24 polls, over a second, against real waits of microseconds) raises the CONTEXT's time-out word (NetState::d_tmo,
// a kernel argument) instead of hanging the GPU: the host checks the word whenever it fetches probabilities and fails the call (c3r_infer /
// c3r_get_probs / c3r_rows_begin) rather than hand out numbers computed from a half-written h_t or x_t.  The word is cleared when the next
// c3r_infer of that context starts: only the faulty batch fails, and no other context of the process is touched.
__device__ __forceinline__ void lds_wait(int *c, int target, int *tmo) {
    for (int it = 0; __atomic_load_n(c, __ATOMIC_RELAXED) < target; ++it) {
        if (it >= (1 << 24)) { if ((threadIdx.x & 63) == 0 && tmo) atomicOr(tmo, 1); break; }
        __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// LDS-DMA of layer 2's input of time slice tt_ (both planes: 2 KC rows of 1 KiB — 64 sites x 16 bytes) into the x tile, the rows dealt
// evenly to NW wavefronts of which the caller is number w; lane l fetches site xsite's 16 bytes of each of its wavefront's rows.
// Non-temporal: y1 is read once.  The caller waits (vmcnt) before anyone reads the tile.
template <int NW, int KC, int WG_SITES>
__device__ __forceinline__ void dma_x_rows(_Float16 (&xs)[2][KC][WG_SITES][8], const _Float16 *xin, size_t plane_in, int ns, int xsite, int w, int tt_) {
    typedef const _Float16 __attribute__((address_space(1))) *gp_t;
    typedef _Float16 __attribute__((address_space(3))) *lp_t;
#pragma unroll
    for (int r = 0; r < 2 * KC / NW; ++r) {
        const int row = w * (2 * KC / NW) + r, pl = row / KC, kc = row % KC;
        const _Float16 *src = xin + (size_t)pl * plane_in + (((size_t)tt_ * KC + kc) * ns + xsite) * 8;
        __builtin_amdgcn_global_load_lds((gp_t)src, (lp_t)&xs[pl][kc][0][0], 16, 0, Y1_NT_AUX);
    }
}

// RTS ("run-time scale"): the weights were packed with a power-of-two scale below 2^12 because some |w| would not fit f16 at 2^12
// (net_load, NetState::wlog2); the scale (layer 2: wsc = 2^s, wun = 2^-s; fused L4: wun4) then comes in as kernel arguments.  With RTS
// = false — every set of weights seen so far — the constants fold exactly as before.
// ------------------------------------------------------------------------------------------------
// Layer 2 (+ fused L4) on v_mfma_f32_16x16x32_f16: k_lstm2_w16.  The decomposition above (512 threads, 64 sites x one direction per
// workgroup, tiles dealt 3 + 2 (+ L4) to the two wavefronts of a SIMD, x_t by LDS-DMA one step ahead, the three LDS counters, h
// double-buffered in LDS) with the smaller MFMA shape: under the chip's power limit the matrix pipe holds a higher clock on 16x16x32 than
// on 32x32x16 at equal cycles per flop (profiles/lstm2_mfma_shape_probe.txt: the same kernel with every 32x32x16 as two 16x16x32 ran in
// 0.944x the time).
//   * a 32-row gate tile is two 16-row subtiles st, the 64 sites four 16-site blocks sb; a k-group is 32 k wide.  A lane holds rows
//     4q + m (q = lane / 16) of column lane % 16: with the rows of subtile st of tile T packed as  row 4q + m <-> gate m of unit
//     8T + 2q + st  (pack_lstm2_w16) the four gates of a unit stay in one lane, and a lane's two subtiles are two consecutive units (its
//     h_t writes are 4-byte stores);
//   * the pipeline runs over (k-group G, subtile st) units — 26 of them, A operands of the same size as the 16-k groups of the
//     32x32x16 layout, so the same two-slot ring; the B operands (four site blocks, hi and lo) are read once per k-group, one unit ahead, and serve both subtiles;
//   * the accumulators start from the fp32 bias x 2^s (exact; kept in LDS) instead of a bias MFMA;
//   * the fused L4's 32 rows of a quarter are two subtiles as well: a lane's 4 rows are 4 consecutive L4 outputs (float4 stores);
//   * step 0 is the x part alone (h_{-1} = 0: ten of its 26 units and the L4 tile are exact zeros); y1 comes in and a4part goes out with
//     the non-temporal policy.
//   ABL : timing-only ablation bits for tools/lstm_probe_w8.hip (0 in the product): 1 weights from one L1-hot unit, 2 no gate math,
//         16 weights loaded for unit 0 only, 32 B operands read for k-group 0 only.
//   Wp  : [dir][quarter(4)][u = 2G + st (26)][tile(5)][hi|lo][64 lanes] half8 — lane l: row l % 16 of subtile st, k = 32G + 8 (l / 16) + 0..7
//   W4p : [dir][t][quarter(4)][u = 2G + st (10)][hi|lo][64 lanes] half8 — row l % 16 <-> L4 output 32 quarter + 16 st + l % 16
//   bp  : pack_lstm_dir's fp32 bias layout (pack_lstm_dir: [dir][tile][r = 8q + 4hh + m] <-> gate m of unit 8 tile + 4 hh + q)
// Row of pack_lstm_dir's bias tile (r = 8q' + 4hh + m <-> gate m of unit 8 tile + 4hh + q') that holds the bias of k_lstm2_w16's accumulator
// row 4q + m of subtile st (gate m of unit 8 tile + 2q + st)
__host__ __device__ constexpr int w16_bias_row(int st, int q, int m) { return 8 * ((2 * q + st) & 3) + 4 * ((2 * q + st) >> 2) + m; }
template <int ABL = 0, bool RTS = false>
__global__ __launch_bounds__(512, 2) void k_lstm2_w16(const _Float16 *__restrict__ xin, const half8 *__restrict__ Wp,
                                                       const float *__restrict__ bp, int n, const half8 *__restrict__ W4p,
                                                       float *__restrict__ a4part, int nstride, float wsc_arg = WSCALE, float wun_arg = WUNSCALE, float wun4_arg = WUNSCALE,
                                                       int *tmo = nullptr /* the context's time-out word (lds_wait) */) {
    const float wsc = RTS ? wsc_arg : WSCALE, wun = RTS ? wun_arg : WUNSCALE, wun4 = RTS ? wun4_arg : WUNSCALE;
    constexpr int INP = 2 * NET_H1, H = NET_H2, NGX = INP / 32, NGH = H / 32, NG = NGX + NGH, NU = 2 * NG, HP = H + 8, NBLK = 4 * H / 32, NTQ = NBLK / 4;
    constexpr int SB = 4, WG_SITES = 16 * SB, KC = INP / 8;
    static_assert(NTQ == 5 && NU == 26, "3 + 2 tile split of a quarter, 26 (k-group, subtile) units (the operand ring holds one unit of prefetch)");
    __shared__ __attribute__((aligned(16))) _Float16 hb_hi[2][WG_SITES][HP];
    __shared__ __attribute__((aligned(16))) _Float16 hb_lo[2][WG_SITES][HP];
    __shared__ __attribute__((aligned(16))) _Float16 xs[2][KC][WG_SITES][8];      // [plane][k/8][site][8]
    __shared__ __attribute__((aligned(16))) float s_bias[NBLK][2][16];          // 2^s b: [tile][st][4q + m]
    __shared__ int s_ctr[4];        // the LDS counters: [0] done reading x_t, [1] x DMAs landed, [2] done writing h_t

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // in an SGPR: the weight addresses below are scalar arithmetic plus one lane offset
    const int c16 = lane & 15, q4 = lane >> 4;
    const int sq = wave & 3;                     // quarter of the gate rows
    const bool heavy3 = wave < 4;                // the 3-tile wavefront of its SIMD pair (waves w and w + 4 share a SIMD: round-robin placement)
    const int dir = blockIdx.x;
    const int site0 = blockIdx.y * WG_SITES;
    const int ns = nstride ? nstride : n;
    const size_t plane_in = (size_t)ns * NET_T * INP;

    for (int i = tid; i < WG_SITES * HP; i += 512) { (&hb_hi[0][0][0])[i] = (_Float16)0.f; (&hb_lo[0][0][0])[i] = (_Float16)0.f; }
    for (int i = tid; i < NBLK * 32; i += 512) {
        const int T = i >> 5, st = (i >> 4) & 1, q = (i >> 2) & 3, m = i & 3;
        s_bias[T][st][4 * q + m] = wsc * bp[((size_t)dir * NBLK + T) * 32 + w16_bias_row(st, q, m)];
    }
    if (tid < 4) s_ctr[tid] = 0;

    int xsite = site0 + lane;
    if (xsite >= n) xsite = n - 1;
    auto dma_x = [&](int tt_) { dma_x_rows<8>(xs, xin, plane_in, ns, xsite, wave, tt_); };            // before the time loop: eight rows per wavefront
    auto dma_x16 = [&](int tt_) { dma_x_rows<4>(xs, xin, plane_in, ns, xsite, wave & 3, tt_); };      // inside it: all 64 rows from the four 3-tile wavefronts
    dma_x(dir ? NET_T - 1 : 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    auto body = [&](auto ntc, auto toffc, auto l4c) {
        constexpr int NT = decltype(ntc)::value, TOFF = decltype(toffc)::value;
        constexpr bool L4T = decltype(l4c)::value;
        constexpr int NTH = NT + (L4T ? 1 : 0);
        const half8 *wl = Wp + ((size_t)(dir * 4 + sq) * NU) * NTQ * 2 * 64 + (size_t)TOFF * 2 * 64;      // uniform; the lane's fragment: + lane
        float cst[NT][2 * SB];          // [tile][4 st + sb]
#pragma unroll
        for (int tt = 0; tt < NT; ++tt)
#pragma unroll
            for (int u = 0; u < 2 * SB; ++u) cst[tt][u] = 0.f;
        floatx4 facc[L4T ? 2 : 1][L4T ? SB : 1];
#pragma unroll
        for (int st = 0; st < (L4T ? 2 : 1); ++st)
#pragma unroll
            for (int sb = 0; sb < (L4T ? SB : 1); ++sb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // (every zero a value of its own: facc now enters the loop past the step-0 branch, and zeros the compiler knows to be
                    // one value are set up before the loop as 16 v_mov_b64 copies of a register pair — harmless, but tests/test_lstm_isa.py
                    // takes any v_mov_b64 in this kernel for a weight address rebuilt in vector registers)
                    float z = 0.f;
                    if constexpr (L4T) asm volatile("" : "+v"(z));
                    facc[st][sb][r] = z;
                }
            }

        typedef const half8 __attribute__((address_space(1))) *gptr_t;
        const uint32_t wlane = (uint32_t)lane;
        for (int step = 0; step < NET_T; ++step) {
            const int t = dir ? NET_T - 1 - step : step;
            const int tprev = step ? (dir ? t + 1 : t - 1) : t;      // step 0: any valid slice (unit 2 NGX's is still requested, never multiplied)
            const int cur = step & 1, nxt = cur ^ 1;

            auto ldx = [&](int g, half8 (&bh)[SB], half8 (&bl)[SB]) {
#pragma unroll
                for (int sb = 0; sb < SB; ++sb) {
                    if ((ABL & 32) && g > 0) continue;
                    bh[sb] = *(const half8 *)&xs[0][4 * g + q4][16 * sb + c16][0];
                    bl[sb] = *(const half8 *)&xs[1][4 * g + q4][16 * sb + c16][0];
                }
            };
            auto ldh = [&](int g, half8 (&bh)[SB], half8 (&bl)[SB]) {
#pragma unroll
                for (int sb = 0; sb < SB; ++sb) {
                    if (ABL & 32) continue;
                    bh[sb] = *(const half8 *)&hb_hi[cur][16 * sb + c16][32 * g + 8 * q4];
                    bl[sb] = *(const half8 *)&hb_lo[cur][16 * sb + c16][32 * g + 8 * q4];
                }
            };
            auto ldw = [&](int u, half8 (&ah)[NTH], half8 (&al)[NTH]) {
                // address laundering, address_space(1): see "Operand layouts", ldw.  The unit's base is uniform: it is advanced by scalar
                // adds and laundered in an SGPR pair; the loads take it as their scalar base with the lane offset in one VGPR
                gptr_t wg = (gptr_t)wl + (size_t)((ABL & 1) ? 0 : u) * NTQ * 2 * 64;
                asm volatile("" : "+s"(wg));
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) {
                    if ((ABL & 16) && u > 0) continue;
                    ah[tt] = wg[(tt * 2 + 0) * 64 + wlane]; al[tt] = wg[(tt * 2 + 1) * 64 + wlane];
                }
                if constexpr (L4T) {
                    if (u >= 2 * NGX && !((ABL & 16) && u > 2 * NGX)) {
                        gptr_t w4 = (gptr_t)(W4p + (((size_t)(dir * NET_T + tprev) * 4 + sq) * 2 * NGH) * 2 * 64) + (size_t)(u - 2 * NGX) * 2 * 64;
                        asm volatile("" : "+s"(w4));
                        ah[NT] = w4[wlane]; al[NT] = w4[64 + wlane];
                    }
                }
            };

            if (step > 0) lds_wait(&s_ctr[1], 4 * step, tmo);      // x_t has landed (four DMA wavefronts per step)
            floatx4 acc[NT][2][SB];
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const floatx4 b4 = *(const floatx4 *)&s_bias[sq * NTQ + TOFF + tt][st][4 * q4];
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) acc[tt][st][sb] = b4;
                }
            // one (k-group, subtile) unit: hi x hi, hi x lo, lo x hi
            auto mma = [&](const half8 (&ah)[NTH], const half8 (&al)[NTH], const half8 (&bh)[SB], const half8 (&bl)[SB], auto stc, bool hpart) {
                constexpr int st = decltype(stc)::value;
#pragma unroll
                for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) acc[tt][st][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[tt], bh[sb], acc[tt][st][sb], 0, 0, 0);
                if (L4T && hpart) {
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) facc[L4T ? st : 0][L4T ? sb : 0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[L4T ? NT : 0], bh[sb], facc[L4T ? st : 0][L4T ? sb : 0], 0, 0, 0);
                }
#pragma unroll
                for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) acc[tt][st][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[tt], bl[sb], acc[tt][st][sb], 0, 0, 0);
                if (L4T && hpart) {
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) facc[L4T ? st : 0][L4T ? sb : 0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[L4T ? NT : 0], bl[sb], facc[L4T ? st : 0][L4T ? sb : 0], 0, 0, 0);
                }
#pragma unroll
                for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) acc[tt][st][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[tt], bh[sb], acc[tt][st][sb], 0, 0, 0);
                if (L4T && hpart) {
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) facc[L4T ? st : 0][L4T ? sb : 0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[L4T ? NT : 0], bh[sb], facc[L4T ? st : 0][L4T ? sb : 0], 0, 0, 0);
                }
            };
            half8 ah[2][NTH], al[2][NTH], bh[2][SB], bl[2][SB];
#define C3R_FENCE() __builtin_amdgcn_sched_barrier(0)
            // unit U = 2G + st: A of unit U in slot U % 2; B of k-group G in slot G % 2, read with the A of unit 2G (one unit ahead)
#define C3R_LOAD(U) do { ldw((U), ah[(U) % 2], al[(U) % 2]);                                                       \
                         if constexpr (((U) & 1) == 0) {                                                          \
                             if constexpr ((U) / 2 < NGX) ldx((U) / 2, bh[((U) / 2) % 2], bl[((U) / 2) % 2]);      \
                             else ldh((U) / 2 - NGX, bh[((U) / 2) % 2], bl[((U) / 2) % 2]); } } while (0)
#define C3R_STEP(U)                                                                                              \
    if constexpr ((U) < NU) {                                                                                     \
        C3R_FENCE();                                                                                              \
        if constexpr ((U) + 1 == 2 * NGX) { lds_wait(&s_ctr[2], 8 * step, tmo); C3R_FENCE(); }   /* h_{t-1} is complete */ \
        if constexpr ((U) + 1 < NU) { C3R_LOAD((U) + 1); }                                                        \
        mma(ah[(U) % 2], al[(U) % 2], bh[((U) / 2) % 2], bl[((U) / 2) % 2], std::integral_constant<int, (U) & 1>{}, (U) >= 2 * NGX); \
        if constexpr ((U) + 1 < NU) {                                                                             \
            constexpr int NMM = ((U) >= 2 * NGX ? NTH : NT) * SB * 3;                                             \
            sched_interleave<NMM, ((U) + 1 >= 2 * NGX ? NTH : NT) * 2, (((U) & 1) ? SB * 2 : 0)>();                \
        }                                                                                                         \
        if constexpr ((U) == 2 * NGX - 1) {                                                                       \
            C3R_FENCE();                                                                                          \
            lds_arrive(&s_ctr[0]);                                                    /* done with x_t */           \
        }                                                                                                         \
    }
            // Step 0 ends with the x part: h_{-1} = 0, so the recurrent units U >= 2 NGX (their weight stream, their reads of a zeroed hb,
            // their MFMAs, the fused L4 tile) add exact zeros.  One uniform branch, no second copy of the body; the counters see the
            // same arrivals (s_ctr[0] after unit 2 NGX - 1, s_ctr[2] and s_ctr[1] after the cell update).  The operands of unit 2 NGX are
            // still requested at step 0, under the MFMAs of the unit before it as at every step: with that request inside the branch
            // too, its loads no longer share registers with the operands that die under those MFMAs, and 12 registers spill.
            static_assert(2 * NGX == 16, "the unit lists below: the x part ends with unit 15");
            C3R_LOAD(0);
            C3R_STEP(0) C3R_STEP(1) C3R_STEP(2) C3R_STEP(3) C3R_STEP(4) C3R_STEP(5) C3R_STEP(6) C3R_STEP(7) C3R_STEP(8) C3R_STEP(9)
            C3R_STEP(10) C3R_STEP(11) C3R_STEP(12) C3R_STEP(13) C3R_STEP(14) C3R_STEP(15)
            if (step) {
                C3R_STEP(16) C3R_STEP(17) C3R_STEP(18)
                C3R_STEP(19) C3R_STEP(20) C3R_STEP(21) C3R_STEP(22) C3R_STEP(23) C3R_STEP(24) C3R_STEP(25)
            }
            C3R_FENCE();
#undef C3R_STEP
#undef C3R_LOAD
#undef C3R_FENCE
            // x_{t+1}: once all eight wavefronts are done with x_t, the four 3-tile wavefronts fetch it; it lands during the cell update
            if (!L4T && step + 1 < NET_T) { lds_wait(&s_ctr[0], 8 * (step + 1), tmo); dma_x16(dir ? NET_T - 2 - step : step + 1); }
            // ---- lane-local cell update, one tile at a time: cell u = 4 st + sb is unit 8T + 2 q4 + st at site 16 sb + c16
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
                __builtin_amdgcn_sched_barrier(0);
                constexpr int NC = 2 * SB;
                const float K1 = -1.4426950408889634f * wun, K2 = -2.8853900817779268f * wun;
                float zi[NC], zf[NC], zg[NC], zo[NC], hval[NC];
#pragma unroll
                for (int u = 0; u < NC; ++u) { zi[u] = acc[tt][u / SB][u % SB][0]; zf[u] = acc[tt][u / SB][u % SB][1]; zg[u] = acc[tt][u / SB][u % SB][2]; zo[u] = acc[tt][u / SB][u % SB][3]; }
                if (ABL & 2) {
#pragma unroll
                    for (int u = 0; u < NC; ++u) hval[u] = zi[u] + zf[u] + zg[u] + zo[u];
                } else lstm_cell_update(zi, zf, zg, zo, cst[tt], hval, K1, K2);
#pragma unroll
                for (int sb = 0; sb < SB; ++sb) {
                    half2v vh, vl;
                    float d0, d1;
                    split_h2(hval[sb], hval[SB + sb], vh, vl, d0, d1);
                    *(half2v *)&hb_hi[nxt][16 * sb + c16][8 * (sq * NTQ + TOFF + tt) + 2 * q4] = vh;
                    *(half2v *)&hb_lo[nxt][16 * sb + c16][8 * (sq * NTQ + TOFF + tt) + 2 * q4] = vl;
                }
            }
            lds_arrive(&s_ctr[2]);
            if (!L4T && step + 1 < NET_T) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); lds_arrive(&s_ctr[1]); }      // (LDS-DMA is tracked by vmcnt)
        }
        if constexpr (L4T) {
            lds_wait(&s_ctr[2], 8 * NET_T, tmo);
            // ---- the last step's h (buffer NET_T & 1) still owes its L4 contribution
            const int tl = dir ? 0 : NET_T - 1, hbuf = NET_T & 1;
            const half8 *w4 = W4p + (((size_t)(dir * NET_T + tl) * 4 + sq) * 2 * NGH) * 2 * 64 + lane;
#pragma unroll 1
            for (int g = 0; g < NGH; ++g) {
                half8 b_h[SB], b_l[SB];
#pragma unroll
                for (int sb = 0; sb < SB; ++sb) {
                    b_h[sb] = *(const half8 *)&hb_hi[hbuf][16 * sb + c16][32 * g + 8 * q4];
                    b_l[sb] = *(const half8 *)&hb_lo[hbuf][16 * sb + c16][32 * g + 8 * q4];
                }
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const half8 a_h = w4[(size_t)((2 * g + st) * 2 + 0) * 64], a_l = w4[(size_t)((2 * g + st) * 2 + 1) * 64];
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) facc[st][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h, b_h[sb], facc[st][sb], 0, 0, 0);
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) facc[st][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h, b_l[sb], facc[st][sb], 0, 0, 0);
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) facc[st][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_l, b_h[sb], facc[st][sb], 0, 0, 0);
                }
            }
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) {
                const int sidx = site0 + 16 * sb + c16;
                if (sidx < n) {
#pragma unroll
                    for (int st = 0; st < 2; ++st) {
                        const floatx4 v = {facc[st][sb][0] * wun4, facc[st][sb][1] * wun4, facc[st][sb][2] * wun4, facc[st][sb][3] * wun4};
                        y1_store(v, (floatx4 *)(a4part + ((size_t)sidx * 2 + dir) * NET_L4 + 32 * sq + 16 * st + 4 * q4));
                    }
                }
            }
        }
    };
    if (heavy3) body(std::integral_constant<int, 3>{}, std::integral_constant<int, 0>{}, std::false_type{});
    else body(std::integral_constant<int, 2>{}, std::integral_constant<int, 3>{}, std::true_type{});
}

// ------------------------------------------------------------------------------------------------
// Precision 2: layer 2 (+ fused L4) with both correction terms on the block-scaled fp8 pipe — k_lstm2_mx.
// the split-f16 layer 2's decomposition (512 threads, 64 sites x one direction, tiles dealt 3 + 2 (+ L4) to the two wavefronts of a SIMD, x_t by
// LDS-DMA, h double-buffered).  Per block of 32 k's the three f16 products of the split-f16 path,
//        w_hi x_hi + w_hi x_lo + w_lo x_hi        (6 MFMAs of 32 cycles per tile and site block),
// become two f16 MFMAs for w_hi x_hi and ONE v_mfma_scale_f32_32x32x64_f8f6f4 (64 cycles) whose K = 64 is the concatenation
//        [ fp8(w) | fp8(w - f16(w)) ]  x  [ fp8(x - f16(x)) ; fp8(x) ]
// (a lane's bytes 0-15 belong to the instruction's first scale block, its bytes 16-31 to the second — tools/mx_scale_probe.hip — so
// every lane carries 16 k's of each term; lanes 0-31 supply the first term's scales, lanes 32-63 the second's).
// Weights carry one power-of-two scale per (gate row, block, term), folded with the 2^12 of the f16 operands; activations are in
// (-1, 1), so FIXED scales do: x 2^6 and (x - f16(x)) 2^18.  The corrections are then good to ~2^-5 of themselves, i.e. the
// pre-activations to ~2^-16 instead of f16x3's 2^-22: max |dP| 2-3e-5 on random weights (tolerance 1e-4), and NOT robust to
// weights of 2-3x the norm (tools/precision_probe.py, scheme f16+2f8k) — which is why c3r_load_weights measures it (precision
// "auto") before this path is used.
//   xin: plane 0 = f16(x) [t][k/8][site][8 halves]; plane 1, same geometry, rows (kb, term, part) = kb * 4 + term * 2 + part of 16 bytes
//        per site: fp8 of k = 32 kb + 16 part + 0..15, term 0 = (x - f16(x)) 2^18, term 1 = x 2^6   (written by k_lstm1_rs<.., YQ>)
//   Wp / W4p: the 32x32x16 split-f16 fragments of pack_lstm_dir_h / net_load's w4f (only the hi halves are read); Wq / Wsc, W4q / W4sc: pack_mx
__global__ __launch_bounds__(512, 2) void k_lstm2_mx(const _Float16 *__restrict__ xin, const half8 *__restrict__ Wp, const uint32_t *__restrict__ Wq,
                                                      const uint32_t *__restrict__ Wsc, const float *__restrict__ bp, int n,
                                                      const half8 *__restrict__ W4p, const uint32_t *__restrict__ W4q,
                                                      const uint32_t *__restrict__ W4sc, float *__restrict__ a4part, int nstride, int *tmo = nullptr) {
    constexpr int INP = 2 * NET_H1, H = NET_H2, NGX = INP / 16, NGH = H / 16, NG = NGX + NGH, HP = H + 8, NBLK = 4 * H / 32, NTQ = NBLK / 4;
    constexpr int SB = 2, WG_SITES = 32 * SB, KC = INP / 8;
    constexpr int NKB = NG / 2, NKBX = NGX / 2, NKBH = NGH / 2, NK4 = (NKB + 3) / 4, NK4L = (NKBH + 3) / 4;
    static_assert(NTQ == 5 && NG == 26 && NGX % 2 == 0 && NGH % 2 == 0, "3 + 2 tile split of a quarter, whole 32-k blocks");
    typedef int intx8 __attribute__((ext_vector_type(8)));
    typedef int intx4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) _Float16 hb_hi[2][WG_SITES][HP];
    __shared__ __attribute__((aligned(16))) intx4 hq[2][NKBH][2][2][WG_SITES];     // fp8 of h: [buffer][kb][term][part][site] 16 bytes
    __shared__ __attribute__((aligned(16))) _Float16 xs[2][KC][WG_SITES][8];      // [plane][row][site][16 bytes]
    __shared__ int s_ctr[4];        // the LDS counters: [0] done reading x_t, [1] x DMAs landed, [2] done writing h_t

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, hh = lane >> 5;
    const int sq = wave & 3;                     // quarter of the gate rows
    const bool heavy3 = wave < 4;                // the 3-tile wavefront of its SIMD pair (waves w and w + 4 share a SIMD)
    const int dir = blockIdx.x;
    const int site0 = blockIdx.y * WG_SITES;
    const int ns = nstride ? nstride : n;
    const size_t plane_in = (size_t)ns * NET_T * INP;

    for (int i = tid; i < WG_SITES * HP; i += 512) (&hb_hi[0][0][0])[i] = (_Float16)0.f;
    for (int i = tid; i < NKBH * 2 * 2 * WG_SITES; i += 512) (&hq[0][0][0][0][0])[i] = intx4{0, 0, 0, 0};
    if (tid < 4) s_ctr[tid] = 0;

    int xsite = site0 + lane;
    if (xsite >= n) xsite = n - 1;
    auto dma_x = [&](int tt_) { dma_x_rows<8>(xs, xin, plane_in, ns, xsite, wave, tt_); };            // before the time loop: eight rows per wavefront
    auto dma_x16 = [&](int tt_) { dma_x_rows<4>(xs, xin, plane_in, ns, xsite, wave & 3, tt_); };      // inside it: all 64 rows from the four 3-tile wavefronts
    dma_x(dir ? NET_T - 1 : 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    auto body = [&](auto ntc, auto toffc, auto l4c) {
        constexpr int NT = decltype(ntc)::value, TOFF = decltype(toffc)::value;
        constexpr bool L4T = decltype(l4c)::value;
        constexpr int NTH = NT + (L4T ? 1 : 0);
        const half8 *wl = Wp + ((size_t)(dir * 4 + sq) * NG) * NTQ * 2 * 64 + (size_t)TOFF * 2 * 64 + lane;
        const intx8 *wq = reinterpret_cast<const intx8 *>(Wq) + ((size_t)(dir * 4 + sq) * NKB * NTQ + TOFF) * 64 + lane;
        const uint32_t *wsc = Wsc + ((size_t)(dir * 4 + sq) * NK4 * NTQ + TOFF) * 64 + lane;
        typedef _Float16 half2v __attribute__((ext_vector_type(2)));
        unsigned bias_hl[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            const float bv = WSCALE * bp[((size_t)dir * NBLK + sq * NTQ + TOFF + tt) * 32 + j];
            half2v hl;
            hl[0] = (_Float16)bv;
            hl[1] = (_Float16)(bv - (float)hl[0]);
            bias_hl[tt] = hh == 0 ? __builtin_bit_cast(unsigned, hl) : 0u;
        }
        const half2v one2 = {(_Float16)1.f, (_Float16)1.f};
        const unsigned ones_b = hh == 0 ? __builtin_bit_cast(unsigned, one2) : 0u;
        const int sbc = hh ? 121 : 109;          // E8M0 scales of the activation bytes: x 2^6 (lanes 32-63), (x - f16(x)) 2^18 (lanes 0-31)
        float cst[NT][SB][4];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt)
#pragma unroll
            for (int sb = 0; sb < SB; ++sb)
#pragma unroll
                for (int q = 0; q < 4; ++q) cst[tt][sb][q] = 0.f;
        floatx16 facc[L4T ? SB : 1];
#pragma unroll
        for (int sb = 0; sb < (L4T ? SB : 1); ++sb)
#pragma unroll
            for (int r = 0; r < 16; ++r) facc[sb][r] = 0.f;

        typedef const half8 __attribute__((address_space(1))) *gptr_t;
        typedef const intx8 __attribute__((address_space(1))) *g8_t;
        typedef const uint32_t __attribute__((address_space(1))) *gs_t;
        // a lane's 32 operand bytes: `p` counts 32-byte units per lane as if they were contiguous; in memory the two 16-byte halves of the
        // 64 lanes are separate 1 KiB runs ([term][lane][16 B]): base of the set = p - lane, halves at + lane and + 64 + lane (in 16-byte units)
        auto ld_q = [&](g8_t p) {
            typedef const intx4 __attribute__((address_space(1))) *g4_t;
            const g4_t h = (g4_t)(p - lane) + lane;
            const intx4 lo = h[0], hi4 = h[64];
            return intx8{lo[0], lo[1], lo[2], lo[3], hi4[0], hi4[1], hi4[2], hi4[3]};
        };
        for (int step = 0; step < NET_T; ++step) {
            const int t = dir ? NET_T - 1 - step : step;
            const int tprev = step ? (dir ? t + 1 : t - 1) : t;
            const int cur = step & 1, nxt = cur ^ 1;

            if (step > 0) lds_wait(&s_ctr[1], 4 * step, tmo);      // x_t has landed
            half8 ah[2][NTH], bh[2][SB];          // two-slot ring: group G in slot G % 2, requested one group ahead
            intx8 a8[NTH], b8[SB];
            int sc[NTH];
            // operands of k-group G: the f16 hi fragments; with an odd G also the fp8 fragments (and every fourth block the scale words) of
            // the 32-k block G / 2, consumed by the block-scaled MFMA that follows group G's f16 MFMAs
            auto load = [&](auto gc, half8 (&ahr)[NTH], half8 (&bhr)[SB]) {
                constexpr int G = decltype(gc)::value;
                uintptr_t wbase = (uintptr_t)wl;                 // (address laundering, address_space(1): see "Operand layouts", ldw)
                asm volatile("" : "+v"(wbase));
                const gptr_t wg = (gptr_t)wbase + (size_t)G * NTQ * 2 * 64;
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) ahr[tt] = wg[(tt * 2 + 0) * 64];
                if constexpr (L4T && G >= NGX) {
                    uintptr_t w4base = (uintptr_t)(W4p + (((size_t)(dir * NET_T + tprev) * 4 + sq) * NGH) * 2 * 64 + lane);
                    asm volatile("" : "+v"(w4base));
                    ahr[NT] = ((gptr_t)w4base)[(size_t)(G - NGX) * 2 * 64];
                }
#pragma unroll
                for (int sb = 0; sb < SB; ++sb) {
                    if constexpr (G < NGX) bhr[sb] = *(const half8 *)&xs[0][2 * G + hh][32 * sb + j][0];
                    else bhr[sb] = *(const half8 *)&hb_hi[cur][32 * sb + j][16 * (G - NGX) + 8 * hh];
                }
                if constexpr ((G & 1) != 0) {
                    constexpr int KB = G / 2;
                    uintptr_t qbase = (uintptr_t)wq;
                    asm volatile("" : "+v"(qbase));
                    const g8_t qg = (g8_t)qbase + (size_t)KB * NTQ * 64;
#pragma unroll
                    for (int tt = 0; tt < NT; ++tt) a8[tt] = ld_q(qg + (size_t)tt * 64);
                    if constexpr (KB % 4 == 0) {
                        uintptr_t sbase = (uintptr_t)wsc;
                        asm volatile("" : "+v"(sbase));
                        const gs_t sg = (gs_t)sbase + (size_t)(KB / 4) * NTQ * 64;
#pragma unroll
                        for (int tt = 0; tt < NT; ++tt) sc[tt] = (int)sg[tt * 64];
                    }
                    if constexpr (L4T && KB >= NKBX) {
                        constexpr int KL = KB - NKBX;
                        uintptr_t q4 = (uintptr_t)(reinterpret_cast<const intx8 *>(W4q) + ((size_t)(dir * NET_T + tprev) * 4 + sq) * NKBH * 64 + lane);
                        asm volatile("" : "+v"(q4));
                        a8[L4T ? NT : 0] = ld_q((g8_t)q4 + (size_t)KL * 64);
                        if constexpr (KL % 4 == 0) {
                            uintptr_t s4 = (uintptr_t)(W4sc + ((size_t)(dir * NET_T + tprev) * 4 + sq) * NK4L * 64 + lane);
                            asm volatile("" : "+v"(s4));
                            sc[L4T ? NT : 0] = (int)((gs_t)s4)[(size_t)(KL / 4) * 64];
                        }
                    }
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) {
                        intx4 p0, p1;
                        if constexpr (KB < NKBX) {
                            p0 = *(const intx4 *)&xs[1][KB * 4 + 0 + hh][32 * sb + j][0];      // term 0, k = 16 hh + 0..15 of the block
                            p1 = *(const intx4 *)&xs[1][KB * 4 + 2 + hh][32 * sb + j][0];      // term 1, the same k's
                        } else {
                            p0 = hq[cur][KB - NKBX][0][hh][32 * sb + j];
                            p1 = hq[cur][KB - NKBX][1][hh][32 * sb + j];
                        }
                        b8[sb] = intx8{p0[0], p0[1], p0[2], p0[3], p1[0], p1[1], p1[2], p1[3]};
                    }
                }
            };

            floatx16 acc[NT][SB];
            {   // bias: one f16 MFMA per (tile, site block), A = {hi, lo} of 2^12 b on k-slots 0 and 1, B = {1, 1}
                floatx16 z;
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = 0.f;
                typedef unsigned uint4v __attribute__((ext_vector_type(4)));
                const uint4v bb = {ones_b, 0u, 0u, 0u};
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) {
                    const uint4v ba = {bias_hl[tt], 0u, 0u, 0u};
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb)
                        acc[tt][sb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, ba), __builtin_bit_cast(half8, bb), z, 0, 0, 0);
                }
            }
            auto mma = [&](auto gc, const half8 (&ahr)[NTH], const half8 (&bhr)[SB]) {
                constexpr int G = decltype(gc)::value;
#pragma unroll
                for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) acc[tt][sb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahr[tt], bhr[sb], acc[tt][sb], 0, 0, 0);
                if constexpr (L4T && G >= NGX) {
#pragma unroll
                    for (int sb = 0; sb < SB; ++sb) facc[L4T ? sb : 0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahr[L4T ? NT : 0], bhr[sb], facc[L4T ? sb : 0], 0, 0, 0);
                }
                if constexpr ((G & 1) != 0) {
                    constexpr int KB = G / 2;
#pragma unroll
                    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                        for (int sb = 0; sb < SB; ++sb)
                            acc[tt][sb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8[tt], b8[sb], acc[tt][sb], 0, 0, KB % 4, sc[tt], 0, sbc);
                    if constexpr (L4T && KB >= NKBX) {
#pragma unroll
                        for (int sb = 0; sb < SB; ++sb)
                            facc[L4T ? sb : 0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8[L4T ? NT : 0], b8[sb], facc[L4T ? sb : 0], 0, 0, (KB - NKBX) % 4,
                                                                                                 sc[L4T ? NT : 0], 0, sbc);
                    }
                }
            };
#define C3R_FENCE() __builtin_amdgcn_sched_barrier(0)
#define C3R_STEP(G)                                                                                              \
    if constexpr ((G) < NG) {                                                                                     \
        C3R_FENCE();                                                                                              \
        if constexpr ((G) + 1 == NGX) { lds_wait(&s_ctr[2], 8 * step, tmo); C3R_FENCE(); }   /* h_{t-1} is complete */ \
        if constexpr ((G) + 1 < NG) { load(std::integral_constant<int, (G) + 1>{}, ah[((G) + 1) % 2], bh[((G) + 1) % 2]); } \
        mma(std::integral_constant<int, (G)>{}, ah[(G) % 2], bh[(G) % 2]);                                        \
        if constexpr ((G) + 1 < NG) {                                                                             \
            constexpr int NMM = ((G) >= NGX ? NTH : NT) * SB * (((G) & 1) ? 2 : 1);                               \
            constexpr int NTL = ((G) + 1 >= NGX ? NTH : NT);                                                      \
            sched_interleave<NMM, NTL * ((((G) + 1) & 1) ? 3 : 1), SB * ((((G) + 1) & 1) ? 3 : 1)>();             \
        }                                                                                                         \
        if constexpr ((G) == NGX - 1) {                                                                           \
            C3R_FENCE();                                                                                          \
            lds_arrive(&s_ctr[0]);                                                       /* done with x_t */        \
        }                                                                                                         \
    }
            load(std::integral_constant<int, 0>{}, ah[0], bh[0]);
            C3R_STEP(0) C3R_STEP(1) C3R_STEP(2) C3R_STEP(3) C3R_STEP(4) C3R_STEP(5) C3R_STEP(6) C3R_STEP(7) C3R_STEP(8) C3R_STEP(9)
            C3R_STEP(10) C3R_STEP(11) C3R_STEP(12) C3R_STEP(13) C3R_STEP(14) C3R_STEP(15) C3R_STEP(16) C3R_STEP(17) C3R_STEP(18)
            C3R_STEP(19) C3R_STEP(20) C3R_STEP(21) C3R_STEP(22) C3R_STEP(23) C3R_STEP(24) C3R_STEP(25)
            C3R_FENCE();
#undef C3R_STEP
#undef C3R_FENCE
            if (!L4T && step + 1 < NET_T) { lds_wait(&s_ctr[0], 8 * (step + 1), tmo); dma_x16(dir ? NET_T - 2 - step : step + 1); }      // lands during the cell update
            // ---- lane-local cell update (k_lstm2_w16's), h_t to LDS as f16 plus the two fp8 bytes per unit
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
                __builtin_amdgcn_sched_barrier(0);
                constexpr int NU = 4 * SB;
                constexpr float K1 = -1.4426950408889634f * WUNSCALE, K2 = -2.8853900817779268f * WUNSCALE;
                float zi[NU], zf[NU], zg[NU], zo[NU], cq[NU], hval[NU];
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    cq[u] = cst[tt][u >> 2][u & 3];
                    zi[u] = acc[tt][u >> 2][4 * (u & 3) + 0]; zf[u] = acc[tt][u >> 2][4 * (u & 3) + 1];
                    zg[u] = acc[tt][u >> 2][4 * (u & 3) + 2]; zo[u] = acc[tt][u >> 2][4 * (u & 3) + 3];
                }
                lstm_cell_update(zi, zf, zg, zo, cq, hval, K1, K2);
                const int T = sq * NTQ + TOFF + tt;          // tile of the direction: units 8 T + 4 hh + q
#pragma unroll
                for (int sb = 0; sb < SB; ++sb) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) cst[tt][sb][q] = cq[4 * sb + q];
                    typedef _Float16 half4 __attribute__((ext_vector_type(4)));
                    half2v vh01, vh23, vl01, vl23;
                    float lo[4];
                    split_h2(hval[4 * sb + 0], hval[4 * sb + 1], vh01, vl01, lo[0], lo[1]);
                    split_h2(hval[4 * sb + 2], hval[4 * sb + 3], vh23, vl23, lo[2], lo[3]);
                    const half4 vh = __builtin_shufflevector(vh01, vh23, 0, 1, 2, 3);
#pragma unroll
                    for (int q = 0; q < 4; ++q) lo[q] *= 262144.f;
                    *(half4 *)&hb_hi[nxt][32 * sb + j][8 * T + 4 * hh] = vh;
                    int w_lo = __builtin_amdgcn_cvt_pk_fp8_f32(lo[0], lo[1], 0, false);
                    w_lo = __builtin_amdgcn_cvt_pk_fp8_f32(lo[2], lo[3], w_lo, true);
                    int w_hi = __builtin_amdgcn_cvt_pk_fp8_f32(hval[4 * sb + 0] * 64.f, hval[4 * sb + 1] * 64.f, 0, false);
                    w_hi = __builtin_amdgcn_cvt_pk_fp8_f32(hval[4 * sb + 2] * 64.f, hval[4 * sb + 3] * 64.f, w_hi, true);
                    // k = 8 T + 4 hh + q of the direction's 160: block T / 4, 16-byte part (T % 4) / 2, bytes 8 (T % 2) + 4 hh + q
                    {
                    reinterpret_cast<int *>(&hq[nxt][T >> 2][0][(T & 3) >> 1][32 * sb + j])[2 * (T & 1) + hh] = w_lo;
                    reinterpret_cast<int *>(&hq[nxt][T >> 2][1][(T & 3) >> 1][32 * sb + j])[2 * (T & 1) + hh] = w_hi;
                    }
                }
            }
            lds_arrive(&s_ctr[2]);
            if (!L4T && step + 1 < NET_T) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); lds_arrive(&s_ctr[1]); }      // (LDS-DMA is tracked by vmcnt)
        }
        if constexpr (L4T) {
            lds_wait(&s_ctr[2], 8 * NET_T, tmo);
            // ---- the last step's h (buffer NET_T & 1) still owes its L4 contribution
            const int tl = dir ? 0 : NET_T - 1, hbuf = NET_T & 1;
            const half8 *w4 = W4p + (((size_t)(dir * NET_T + tl) * 4 + sq) * NGH) * 2 * 64 + lane;
            const intx8 *q4 = reinterpret_cast<const intx8 *>(W4q) + ((size_t)(dir * NET_T + tl) * 4 + sq) * NKBH * 64 + lane;
            const uint32_t *s4 = W4sc + ((size_t)(dir * NET_T + tl) * 4 + sq) * NK4L * 64 + lane;
            static_for<0, NKBH>([&](auto pc) {
                constexpr int P = decltype(pc)::value;
                const half8 a0 = w4[(size_t)((2 * P) * 2) * 64], a1 = w4[(size_t)((2 * P + 1) * 2) * 64];
                const intx8 aq = ld_q((g8_t)(q4 + (size_t)P * 64));
                const int scl = (int)s4[(size_t)(P / 4) * 64];
#pragma unroll
                for (int sb = 0; sb < SB; ++sb) {
                    const half8 b0 = *(const half8 *)&hb_hi[hbuf][32 * sb + j][16 * (2 * P) + 8 * hh];
                    const half8 b1 = *(const half8 *)&hb_hi[hbuf][32 * sb + j][16 * (2 * P + 1) + 8 * hh];
                    const intx4 p0 = hq[hbuf][P][0][hh][32 * sb + j], p1 = hq[hbuf][P][1][hh][32 * sb + j];
                    const intx8 bq = {p0[0], p0[1], p0[2], p0[3], p1[0], p1[1], p1[2], p1[3]};
                    facc[sb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, facc[sb], 0, 0, 0);
                    facc[sb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, facc[sb], 0, 0, 0);
                    facc[sb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(aq, bq, facc[sb], 0, 0, P % 4, scl, 0, sbc);
                }
            });
#pragma unroll
            for (int sb = 0; sb < SB; ++sb) {
                const int sidx = site0 + 32 * sb + j;
                if (sidx < n) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const floatx4 v = {facc[sb][4 * q] * WUNSCALE, facc[sb][4 * q + 1] * WUNSCALE, facc[sb][4 * q + 2] * WUNSCALE,
                                           facc[sb][4 * q + 3] * WUNSCALE};
                        y1_store(v, (floatx4 *)(a4part + ((size_t)sidx * 2 + dir) * NET_L4 + 32 * sq + 8 * q + 4 * hh));
                    }
                }
            }
        }
    };
    if (heavy3) body(std::integral_constant<int, 3>{}, std::integral_constant<int, 0>{}, std::false_type{});
    else body(std::integral_constant<int, 2>{}, std::integral_constant<int, 3>{}, std::true_type{});
}

// ------------------------------------------------------------------------------------------------
// Layer 1 with REGISTER-STATIONARY weights: k_lstm1_rs, 1024 threads = 16 wavefronts (four per SIMD, 128 registers), 64 sites x one
// direction per workgroup, one workgroup per CU.  Layer 1 is small enough for it: a wavefront owns ONE gate-row tile and loads that
// tile's split-f16 weights — 10 k-groups x (hi, lo) = 80 registers — once, before the time loop; there is no weight stream at all.
// Round 2's streaming kernel (k_lstm1_w8, in git history) had no registers for a prefetch ring at 128 registers, so each of its k-groups
// was "load, wait an L2 round trip, use": 13-16 k of a step's 21.7 k clocks.  The price: the workgroup's two 32-site blocks go through one
// accumulator one after the other (no registers for two), and every B fragment is read from LDS by sixteen wavefronts.
// Wp: [dir][quarter][g][tile(4)][hi|lo][lane] (tile blk = 4 quarter + tile); the bias rides on input slot CIN (x = 1 there).
// The counts: f16 holds integers exactly only up to 2048 and ends at 65504, and a window's flank is not bounded by the A5 rescale (it
// divides by the depth of the centre position alone).  Every int32 count is therefore staged as FOUR f16 integers,
//   x = 65536 T + r,  T = round(x / 65536) = th + tl,  r = rh + rl      (|T|, |r| <= 32768: an f16 and a remainder of at most 8 each),
// exactly.  rh is what the K loop always multiplies (for |x| <= 2048 it is x itself and the other three are zero); the others are
// multiplied only from the first step on at which one of them is non-zero at one of the workgroup's 64 sites — s_xlvl[step], set while
// the counts are staged: 1 = some rl, 2 = some T (never with int16 windows): the workgroup leaves the ordinary time loop for one that
// multiplies them before the K loop, the (wh + wl)(th + tl) sum scaled by 65536 in the accumulator.  A site's result does not depend
// on whether its neighbours raised the level: the extra products of its own zeros are zeros.
template <int CIN, bool YQ = false, bool RTS = false>
__global__ __launch_bounds__(1024) void k_lstm1_rs(const void *__restrict__ xin_v, const half8 *__restrict__ Wp, _Float16 *__restrict__ y, int n, int nstride,
                                                   const int32_t *__restrict__ row_idx /* row of site i in xin (the tensor build writes windows as they arrive); null: i */,
                                                   float wun_arg = WUNSCALE /* RTS: 2^-s of the layer's weight scale (k_lstm2_w16) */,
                                                   int x16 = 0 /* the rows are int16 (the tensor build's windows), not int32 (a caller's batch) */) {
    const float wun = RTS ? wun_arg : WUNSCALE;
    constexpr int H = NET_H1, NGX = 2, NGH = H / 16, NG = NGX + NGH, HP = H + 8, NTQ = 4, WG_SITES = 64, HV = H / 8, XP = 40;
    constexpr int NPC = (CIN + 1) / 2;
    static_assert(CIN % 2 == 0 && CIN < 32 && WG_SITES * NPC <= 1024, "even channel count, one free slot for the bias, one x piece per thread");
    typedef _Float16 half4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) _Float16 hb[2][2][WG_SITES][HP];      // h_t: [step parity][hi | lo] — a lane's hi and lo fragments of a block: one address, constant offsets
    __shared__ __attribute__((aligned(16))) _Float16 xs[4][2][WG_SITES][XP];      // the counts' parts rh, rl, th, tl (one array: one address, four offsets)
    __shared__ int s_xlvl[NET_T];              // per step: 0 = the 64 sites' counts are rh alone, 1 = some rl, 2 = some T
    // the cell state lives in LDS (one float4 per lane, block and wavefront: 32 KB; with the counts' four parts the workgroup holds 140 of the CU's 160 KB): its 8 registers
    // pay for the second B-operand buffer below
    __shared__ __attribute__((aligned(16))) float4 s_c[16][2][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int blk = __builtin_amdgcn_readfirstlane(tid >> 6);          // the wavefront's tile of the direction (units 8 blk .. 8 blk + 7); in an SGPR: what depends on it and the step alone is scalar arithmetic
    const int j = lane & 31, hh = lane >> 5;
    const int dir = blockIdx.x;
    const int site0 = blockIdx.y * WG_SITES;
    const size_t plane_out = (size_t)nstride * NET_T * 2 * H;

    for (int i = tid; i < 2 * WG_SITES * HP; i += 1024) (&hb[0][0][0][0])[i] = (_Float16)0.f;
    for (int i = tid; i < 2 * WG_SITES * XP; i += 1024) {
        (&xs[0][0][0][0])[i] = ((i % XP) == CIN) ? (_Float16)1.f : (_Float16)0.f;
        (&xs[1][0][0][0])[i] = (_Float16)0.f; (&xs[2][0][0][0])[i] = (_Float16)0.f; (&xs[3][0][0][0])[i] = (_Float16)0.f;
    }
    if (tid < NET_T) s_xlvl[tid] = 0;

    half8 wh[NG], wl[NG];
    {
        const half8 *wb = Wp + (((size_t)(dir * 4 + (blk >> 2)) * NG) * NTQ + (blk & 3)) * 2 * 64 + lane;
#pragma unroll
        for (int g = 0; g < NG; ++g) { wh[g] = wb[((size_t)g * NTQ * 2 + 0) * 64]; wl[g] = wb[((size_t)g * NTQ * 2 + 1) * 64]; }
    }
    s_c[blk][0][lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    s_c[blk][1][lane] = make_float4(0.f, 0.f, 0.f, 0.f);

    // x staging: one 8-byte piece (two int32 counts of row (site, t)) per thread
    typedef int int2v __attribute__((ext_vector_type(2)));
    int2v xr = {0, 0};
    const bool xmine = tid < WG_SITES * NPC;
    uint32_t xrow = 0;          // (element index: n * 33 * CIN < 2^32 — the host checks)
    if (xmine) {
        int sj = site0 + tid / NPC;
        if (sj >= n) sj = n - 1;
        if (row_idx) sj = row_idx[sj];
        xrow = (uint32_t)sj * (uint32_t)(NET_T * CIN) + 2u * (uint32_t)(tid % NPC);
    }
    // (the address: uniform base + 32-bit index x element size, the size a run-time scalar — one v_mad_u64_u32 and no 64-bit index held in registers)
    uint32_t xesz = x16 ? 2u : 4u;
    asm volatile("" : "+s"(xesz));       // (opaque: a known power of two becomes a 64-bit vector shift and a zero register kept for it)
    auto x_fetch = [&](int tt_) {
        if (xmine) {
            const char *xa = (const char *)xin_v + (uint64_t)(xrow + (uint32_t)(tt_ * CIN)) * xesz;
            if (x16) { const int pr = *(const int *)xa; xr[0] = (int)(int16_t)(pr & 0xffff); xr[1] = pr >> 16; }
            else xr = *(const int2v *)xa;
        }
    };
    auto x_store = [&](int buf, int step_) {
        if (xmine) {
            typedef _Float16 half2v __attribute__((ext_vector_type(2)));
            half2v vrh, vrl;
            int r[2] = {xr[0], xr[1]}, any_t = 0;
            const int site = tid / NPC, slot = 2 * (tid % NPC);
            if (!x16) {                                                                       // (int16 rows: T = 0, as initialised)
                half2v vth, vtl;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int T = (r[e] >> 16) + ((r[e] >> 15) & 1);                          // round(x / 65536), |T| <= 32768
                    r[e] = (int)((uint32_t)r[e] - ((uint32_t)T << 16));                       // -32768 .. 32767 (for |x| <= 32767: x itself)
                    vth[e] = (_Float16)(float)T;
                    vtl[e] = (_Float16)(float)(T - (int)(float)vth[e]);
                    any_t |= T;
                }
                *(half2v *)&xs[2][buf][site][slot] = vth; *(half2v *)&xs[3][buf][site][slot] = vtl;
            }
            vrh[0] = (_Float16)(float)r[0]; vrh[1] = (_Float16)(float)r[1];
            const int rl0 = r[0] - (int)(float)vrh[0], rl1 = r[1] - (int)(float)vrh[1];
            vrl[0] = (_Float16)(float)rl0; vrl[1] = (_Float16)(float)rl1;
            const int any_rl = rl0 | rl1;
            *(half2v *)&xs[0][buf][site][slot] = vrh;
            *(half2v *)&xs[1][buf][site][slot] = vrl;
            if (any_rl | any_t) atomicMax(&s_xlvl[step_], any_t ? 2 : 1);
        }
    };
    __syncthreads();
    x_fetch(dir ? NET_T - 1 : 0);
    x_store(0, 0);
    __syncthreads();
    // The lane's LDS addresses: four registers for the whole loop.  Each is the address of the lane's first access of its kind, the
    // step's parity included (moved by one buffer at the end of every step); blocks, groups, the hi | lo planes and the counts' parts
    // are constant offsets of the instructions.  (Left to the compiler: ten registers of addresses that differ by constants.)
    typedef const char __attribute__((address_space(3))) *lds_t;
    typedef char __attribute__((address_space(3))) *ldsw_t;
    typedef const half8 __attribute__((address_space(3))) *lds_h8;
    constexpr int XBUF = WG_SITES * XP * 2, HBUF = 2 * WG_SITES * HP * 2, HLO = WG_SITES * HP * 2, XPARTB = 2 * XBUF;      // bytes
    lds_t xrd = (lds_t)&xs[0][0][j][8 * hh];                  // B fragments of x_t, parity 0 first
    lds_t hrd = (lds_t)&hb[0][0][j][8 * hh];                  // B fragments of h_{t-1}
    ldsw_t hwr = (ldsw_t)&hb[1][0][j][8 * blk + 4 * hh];      // the lane's four units of h_t
    const ldsw_t scp = (ldsw_t)&s_c[blk][0][lane];
    asm volatile("" : "+v"(xrd), "+v"(hrd), "+v"(hwr));

    // One time step.  DEEP = false is the loop every ordinary window runs; DEEP = true multiplies the counts' other parts as well and
    // loads its B fragments in place (no second buffer: its registers go to those parts, and the path is rare)
    auto one_step = [&](const int step, auto deep_c) {
        constexpr bool DEEP = decltype(deep_c)::value;
        const int t = dir ? NET_T - 1 - step : step;
        const int cur = step & 1, nxt = cur ^ 1;
        // y1 rows of the step: a uniform base (SGPRs) and one 32-bit lane offset
        typedef _Float16 __attribute__((address_space(1))) *gh_t;
        typedef half4 __attribute__((address_space(1))) *gh4_t;
        gh_t yrow = (gh_t)(y + ((size_t)t * (2 * HV) + dir * HV + blk) * nstride * 8 + (size_t)site0 * 8);
        asm volatile("" : "+s"(yrow));       // (stays a scalar base: otherwise the lane offset is folded into a 64-bit vector pointer outside the loop)
        const uint32_t ylane = (uint32_t)(j * 8 + 4 * hh);
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            const lds_t xb = xrd + 32 * sb * XP * 2;      // the lane's B fragment of group 0, part rh: the others at constant offsets
            const lds_t hb_r = hrd + 32 * sb * HP * 2;
            // x_{t+1}: requested when the second block starts — it lands under that block's K loop, and its two registers are not alive under the first
            if (sb == 1 && step + 1 < NET_T) x_fetch(dir ? NET_T - 2 - step : step + 1);
            floatx16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            // counts beyond one f16 somewhere in the workgroup (see the header): their other parts first.  Full K = 16 products also for the
            // second group (its unused slots are zeros on both sides); the level is uniform over the workgroup
            if constexpr (DEEP) {
                if (__builtin_amdgcn_readfirstlane(s_xlvl[step]) == 2) {
#pragma unroll
                    for (int g = 0; g < NGX; ++g) {
                        const half8 th = *(lds_h8)(xb + 2 * XPARTB + 32 * g), tl = *(lds_h8)(xb + 3 * XPARTB + 32 * g);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[g], th, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[g], th, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[g], tl, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[g], tl, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] *= 65536.f;
                }
#pragma unroll
                for (int g = 0; g < NGX; ++g) {
                    const half8 rl = *(lds_h8)(xb + XPARTB + 32 * g);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[g], rl, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[g], rl, acc, 0, 0, 0);
                }
            }
            // B operands double-buffered: group g + 1's fragments (hi and lo together) are requested before group g's MFMAs are issued.
            // The fences hold the compiler to it: left alone it sinks every read to its first use, one register quad, a full
            // lgkmcnt(0) round trip in front of each MFMA pair
            half8 bh[2], bl[2];
            auto ldb = [&](auto gc, half8 &h, half8 &l) {
                constexpr int G = decltype(gc)::value;
                if constexpr (G < NGX) h = *(lds_h8)(xb + 32 * G);
                else { h = *(lds_h8)(hb_r + 32 * (G - NGX)); l = *(lds_h8)(hb_r + HLO + 32 * (G - NGX)); }
            };
            if constexpr (!DEEP) ldb(std::integral_constant<int, 0>{}, bh[0], bl[0]);
            static_for<0, NG>([&](auto gc) {
                constexpr int G = decltype(gc)::value;
                if constexpr (DEEP) ldb(std::integral_constant<int, G>{}, bh[G & 1], bl[G & 1]);
                else {
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (G + 1 < NG) ldb(std::integral_constant<int, G + 1>{}, bh[(G + 1) & 1], bl[(G + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (G == NGX - 1 && CIN + 1 <= 16 + 4) {
                    // 18 channels: the second input group holds channels 16 .. CIN - 1 and the bias slot CIN, zeros after them: a K = 8 product covers it
                    // (lane half hh takes k = 4 hh .. 4 hh + 3 of the group: for hh = 0 the first half of the lane's K = 16 fragment, for
                    // hh = 1 zeros — as is the first half of ITS fragment, k = 8 .. 11 of the group)
                    const half4 a_h = __builtin_shufflevector(wh[G], wh[G], 0, 1, 2, 3), a_l = __builtin_shufflevector(wl[G], wl[G], 0, 1, 2, 3);
                    const half4 b_h = __builtin_shufflevector(bh[G & 1], bh[G & 1], 0, 1, 2, 3);
                    acc = __builtin_amdgcn_mfma_f32_32x32x8f16(a_h, b_h, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x8f16(a_l, b_h, acc, 0, 0, 0);
                } else {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[G], bh[G & 1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[G], bh[G & 1], acc, 0, 0, 0);
                    if constexpr (G >= NGX) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[G], bl[G & 1], acc, 0, 0, 0);      // (the counts' other parts: before the loop)
                }
            });
            // ---- lane-local cell update of the block (four units per lane)
            const float K1 = -1.4426950408889634f * wun, K2 = -2.8853900817779268f * wun;
            float zi[4], zf[4], zg[4], zo[4], cq[4], hval[4];
            {
                const floatx4 c4 = *(floatx4 __attribute__((address_space(3))) *)(scp + sb * 64 * 16);
                cq[0] = c4[0]; cq[1] = c4[1]; cq[2] = c4[2]; cq[3] = c4[3];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { zi[u] = acc[4 * u + 0]; zf[u] = acc[4 * u + 1]; zg[u] = acc[4 * u + 2]; zo[u] = acc[4 * u + 3]; }
            lstm_cell_update(zi, zf, zg, zo, cq, hval, K1, K2);
            *(floatx4 __attribute__((address_space(3))) *)(scp + sb * 64 * 16) = floatx4{cq[0], cq[1], cq[2], cq[3]};
            half2v vh01, vh23, vl01, vl23;
            float lo[4];
            split_h2(hval[0], hval[1], vh01, vl01, lo[0], lo[1]);
            split_h2(hval[2], hval[3], vh23, vl23, lo[2], lo[3]);
            const half4 vh = __builtin_shufflevector(vh01, vh23, 0, 1, 2, 3), vl = __builtin_shufflevector(vl01, vl23, 0, 1, 2, 3);
#pragma unroll
            for (int q = 0; q < 4; ++q) lo[q] *= 262144.f;
            *(half4 __attribute__((address_space(3))) *)(hwr + 32 * sb * HP * 2) = vh;
            *(half4 __attribute__((address_space(3))) *)(hwr + 32 * sb * HP * 2 + HLO) = vl;
            const gh_t yp = yrow + (size_t)(ylane + 32 * sb * 8);
            y1_store(vh, (gh4_t)yp);
            if constexpr (!YQ) {
                y1_store(vl, (gh4_t)(yrow + plane_out + (size_t)(ylane + 32 * sb * 8)));
            } else {                                     // the fp8 plane precision 2's layer 2 reads (k_lstm2_mx's x layout)
                int w_lo = __builtin_amdgcn_cvt_pk_fp8_f32(lo[0], lo[1], 0, false);
                w_lo = __builtin_amdgcn_cvt_pk_fp8_f32(lo[2], lo[3], w_lo, true);
                int w_hi = __builtin_amdgcn_cvt_pk_fp8_f32(hval[0] * 64.f, hval[1] * 64.f, 0, false);
                w_hi = __builtin_amdgcn_cvt_pk_fp8_f32(hval[2] * 64.f, hval[3] * 64.f, w_hi, true);
                const int row0 = (dir * 4 + (blk >> 2)) * 4 + ((blk & 3) >> 1);
                gh_t qrow = (gh_t)(y + plane_out + ((size_t)t * (2 * HV) + row0) * nstride * 8 + (size_t)site0 * 8 + 4 * (blk & 1));
                asm volatile("" : "+s"(qrow));
                typedef int __attribute__((address_space(1))) *gi_t;
                const uint32_t qlane = (uint32_t)(j * 8 + 2 * hh + 32 * sb * 8);
                y1_store(w_lo, (gi_t)(qrow + (size_t)qlane));
                y1_store(w_hi, (gi_t)(qrow + (size_t)2 * nstride * 8 + (size_t)qlane));
            }
        }
        if (step + 1 < NET_T) x_store(nxt, step + 1);
        {                                                      // the other parity for the next step
            const int sg = cur ? -1 : 1;
            xrd += sg * XBUF; hrd += sg * HBUF; hwr -= sg * HBUF;
            asm volatile("" : "+v"(xrd), "+v"(hrd), "+v"(hwr));
        }
        __syncthreads();                                       // h_t and x_{t+1} complete; everyone is done with h_{t-1} and x_t (LDS counters
                                                               // instead of this barrier, as in layer 2, measured slower: 6.3 against 5.8 ms)
    };
    // the ordinary loop runs until a step's counts need more than one f16 each; the workgroup does the rest of its steps in the other one
    int step = 0;
    for (; step < NET_T; ++step) {
        if (__builtin_amdgcn_readfirstlane(s_xlvl[step])) break;
        one_step(step, std::false_type{});
    }
    for (; step < NET_T; ++step) one_step(step, std::true_type{});
}

// ------------------------------------------------------------------------------------------------
// L4: a4[n][128] = selu(y2[n][10560] * W4 + b4).  grid = ceil(n/32), block = 256 (wave = 32-row block
// of output units).  Same transposed MFMA scheme; B operand straight from global (each site row is
// streamed sequentially, 16 B per lane).
__global__ __launch_bounds__(256) void k_fc4(const float *__restrict__ y2, const float4 *__restrict__ Wp,
                                             const float *__restrict__ bias, float *__restrict__ a4, int n) {
    constexpr int NG = NET_FLAT / 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, hh = lane >> 5;
    const int site0 = blockIdx.x * NET_SITES;
    int s = site0 + j; if (s >= n) s = n - 1;
    const float *xrow = y2 + (size_t)s * NET_FLAT + 4 * hh;
    const float4 *wl = Wp + (size_t)wave * NG * 64 + lane;
    floatx16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll 4
    for (int g = 0; g < NG; g += 2) {
        const float4 b0 = *(const float4 *)(xrow + 8 * g);
        const float4 b1 = *(const float4 *)(xrow + 8 * g + 8);
        const float4 a0 = wl[(size_t)g * 64];
        const float4 a1 = wl[(size_t)(g + 1) * 64];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b1.w, acc1, 0, 0, 0);
    }
    if (site0 + j < n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = 32 * wave + 8 * q + 4 * hh;   // acc row 4q+m <-> output unit 32*wave + 8q + 4hh + m
            float4 v;
            v.x = selu(acc0[4 * q + 0] + acc1[4 * q + 0] + bias[u + 0]);
            v.y = selu(acc0[4 * q + 1] + acc1[4 * q + 1] + bias[u + 1]);
            v.z = selu(acc0[4 * q + 2] + acc1[4 * q + 2] + bias[u + 2]);
            v.w = selu(acc0[4 * q + 3] + acc1[4 * q + 3] + bias[u + 3]);
            *(float4 *)(a4 + (size_t)(site0 + j) * NET_L4 + u) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Heads on the fp32 matrix pipe (k_heads_mfma): L4's selu, the two 128->128 selu branches, 21 + 3
// logits with selu THEN softmax — as exact-f32 MFMAs (v_mfma_f32_32x32x2_f32 == an fmaf chain), 32 sites per workgroup.  A VALU version
// spent 0.39 ms of a chr20 pass on 14 GFLOP of scalar fmaf; the transposed scheme of k_fc4 (rows = output units, cols = sites)
// does it at the f32 MFMA rate.  The 24 logits are ONE 32-row tile over K = 256: rows 0..20 read the L5_1 half of a5, rows 21..23
// the L5_2 half (zero weights elsewhere); its K range is split over the four wavefronts and summed through LDS.
//   W5p: [blk(8)][g(16)][lane] float4 = W5[8g + 4kh + s][32 blk + r];   Wcp: [g(32)][lane] float4, rows >= 24 zero
__global__ __launch_bounds__(256) void k_heads_mfma(const float *__restrict__ a4, int parts, const float *__restrict__ b4,
                                                    const float4 *__restrict__ W5p, const float *__restrict__ b5,
                                                    const float4 *__restrict__ Wcp, const float *__restrict__ bo,
                                                    float *__restrict__ probs, int n) {
    constexpr int S = 32, P4 = 128 + 4, P5 = 256 + 4;
    __shared__ __attribute__((aligned(16))) float s_a4[S][P4];      // later: the four K-slices' partial logits [4][32 rows][33]
    __shared__ __attribute__((aligned(16))) float s_a5[S][P5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, hh = lane >> 5;
    const int site0 = blockIdx.x * S;
    for (int i = tid; i < S * 128; i += 256) {
        const int sl = i >> 7, u = i & 127, sg = site0 + sl;
        float v = 0.f;
        if (sg < n) v = parts == 2 ? selu(a4[((size_t)sg * 2) * 128 + u] + a4[((size_t)sg * 2 + 1) * 128 + u] + b4[u]) : a4[(size_t)sg * 128 + u];
        s_a4[sl][u] = v;
    }
    __syncthreads();
    {   // L5_1 | L5_2: 256 output rows = 8 tiles, two per wavefront, K = 128
        floatx16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
        const float4 *w0 = W5p + (size_t)(2 * wave) * 16 * 64 + lane, *w1 = w0 + 16 * 64;
#pragma unroll 4
        for (int g = 0; g < 16; ++g) {
            const float4 b = *(const float4 *)&s_a4[j][8 * g + 4 * hh];
            const float4 a0 = w0[g * 64], a1 = w1[g * 64];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b.w, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;      // C/D layout of the 32x32 tiles
            const int u0 = 64 * wave + row, u1 = u0 + 32;
            s_a5[j][u0] = selu(acc0[r] + b5[u0]);
            s_a5[j][u1] = selu(acc1[r] + b5[u1]);
        }
    }
    __syncthreads();
    float(*s_part)[32][33] = (float(*)[32][33]) & s_a4[0][0];       // 4 x 32 x 33 floats = 16.9 KB: fits the a4 tile's space
    {   // 24 logits as one tile, K = 256 split over the wavefronts
        floatx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float4 *wc = Wcp + (size_t)(8 * wave) * 64 + lane;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const float4 b = *(const float4 *)&s_a5[j][8 * (8 * wave + g) + 4 * hh];
            const float4 a = wc[g * 64];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) s_part[wave][(r & 3) + 8 * (r >> 2) + 4 * hh][j] = acc[r];
    }
    __syncthreads();
    if (tid < S * 2) {
        const int sl = tid >> 1, part = tid & 1;
        const int o0 = part ? 21 : 0, o1 = part ? 24 : 21;
        if (site0 + sl < n) {
            float lg[21];
            float m = -1e30f;
            for (int o = o0; o < o1; ++o) {
                const float v = selu(((s_part[0][o][sl] + s_part[1][o][sl]) + (s_part[2][o][sl] + s_part[3][o][sl])) + bo[o]);
                lg[o - o0] = v;
                m = fmaxf(m, v);
            }
            float sum = 0.f;
            for (int o = o0; o < o1; ++o) sum += __expf(lg[o - o0] - m);
            for (int o = o0; o < o1; ++o) probs[(size_t)(site0 + sl) * C3R_NPROB + o] = __expf(lg[o - o0] - m) / sum;
        }
    }
}

}  // namespace c3r
