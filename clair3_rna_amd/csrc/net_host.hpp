// net_host.hpp — host driver of the pileup network: the per-context device state, the weight upload (net_pack.hpp packs, this file
// copies), the activation buffers and the launches of the kernels of net_kernels.hpp.  The kernels have no build-time variants: what
// this file launches is the one form of each (fp32: grid (groups, 2); split-f16 and fp8-corrected: grid (2, groups)).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cmath>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/c3r.h"
#include "net_kernels.hpp"
#include "net_pack.hpp"

namespace c3r {

struct NetState {
    bool loaded = false;
    int channels = 0;
    // the weights, one pointer per PackedNet vector (net_each_weight_buffer pairs them; PackedNet says what each holds)
    float4 *d_w1 = nullptr; float *d_b1 = nullptr;     // packed LSTM1 (both dirs)
    float4 *d_w2 = nullptr; float *d_b2 = nullptr;     // packed LSTM2
    float4 *d_w4 = nullptr; float *d_b4 = nullptr;     // packed L4
    float *d_b5 = nullptr, *d_bo = nullptr;            // the heads' biases
    float4 *d_w5p = nullptr, *d_wcp = nullptr;         // heads in MFMA fragment order (k_heads_mfma)
    half8 *d_w2w = nullptr, *d_w4w = nullptr;          // k_lstm2_w16's layer-2 and fused-L4 fragments (pack_lstm2_w16, pack_l4_w16)
    half8 *d_w1h = nullptr, *d_w2h = nullptr;          // split-f16 packed weights (hi/lo, x 2^s) of the 32-row kernels
    half8 *d_w4f = nullptr;                            // L4 packed per (dir, t) for k_lstm2_mx's fused epilogue
    uint32_t *d_w2q = nullptr, *d_w2s = nullptr, *d_w4q = nullptr, *d_w4s = nullptr;   // precision 2: fp8 fragments and block scales of layer 2 / fused L4
    // log2 of the power-of-two scale the split-f16 weights of layer 1 / layer 2 / L4 were packed with (PackedNet::wlog2, chosen by
    // net_pack); below 12 the run-time-scale variants of the kernels run
    int wlog2[3] = {12, 12, 12};
    int precision = 1;            // 0 = fp32 MFMA, 1 = split-f16 (f16x3, fp32-equivalent), 2 = f16 main term + both corrections on the MX fp8 pipe
    float *d_y1 = nullptr, *d_y2 = nullptr, *d_a4 = nullptr, *d_probs = nullptr;
    int32_t *d_tmo = nullptr;        // the context's time-out word of the layer-2 rendezvous (lds_wait); allocated with the weights
    int64_t cap_probs = 0;           // sites d_probs holds (the whole batch); cap_sites bounds one network slice
    int64_t cap_sites = 0;
};

// The one list of weight buffers: f(NetState's device pointer, PackedNet's host vector) for each.  net_load uploads along it, net_free
// frees along it: a new buffer is a member on either side and one line here.
template <class F>
inline void net_each_weight_buffer(F &&f) {
    f(&NetState::d_w1, &PackedNet::w1);   f(&NetState::d_b1, &PackedNet::b1);   f(&NetState::d_w2, &PackedNet::w2);   f(&NetState::d_b2, &PackedNet::b2);
    f(&NetState::d_w4, &PackedNet::w4);   f(&NetState::d_b4, &PackedNet::b4);   f(&NetState::d_b5, &PackedNet::b5);   f(&NetState::d_bo, &PackedNet::bo);
    f(&NetState::d_w5p, &PackedNet::w5p); f(&NetState::d_wcp, &PackedNet::wcp);
    f(&NetState::d_w1h, &PackedNet::w1h); f(&NetState::d_w2h, &PackedNet::w2h); f(&NetState::d_w4f, &PackedNet::w4f);
    f(&NetState::d_w2w, &PackedNet::w2w); f(&NetState::d_w4w, &PackedNet::w4w);
    f(&NetState::d_w2q, &PackedNet::w2q); f(&NetState::d_w2s, &PackedNet::w2s); f(&NetState::d_w4q, &PackedNet::w4q); f(&NetState::d_w4s, &PackedNet::w4s);
}

// The layer-1 output of a full slice is one 8.9-GB allocation.  A process that destroys a context and creates another (a second
// sample, a test suite) would hand it back to the driver and ask for it again: the driver clears freed memory before it is
// reused, and that hipMalloc then takes 0.8 s instead of 0.3 ms.  Up to two such blocks per process are kept for the next context
// of the same device (C3R_NO_BLOCK_CACHE=1, or C3R_POISON — which wants fresh memory — turns this off).
struct BigBlock { int dev; size_t bytes; void *p; };
inline std::mutex &big_mu() { static std::mutex m; return m; }
inline std::vector<BigBlock> &big_cache() { static std::vector<BigBlock> v; return v; }
inline bool big_cache_on() {
    static const bool on = [] { const char *a = getenv("C3R_NO_BLOCK_CACHE"), *b = getenv("C3R_POISON"); return !(a && *a == '1') && !(b && *b); }();
    return on;
}
inline void *big_take(size_t bytes) {
    if (!big_cache_on()) return nullptr;
    int dev = 0; (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(big_mu());
    auto &c = big_cache();
    for (size_t k = 0; k < c.size(); ++k) if (c[k].dev == dev && c[k].bytes == bytes) { void *p = c[k].p; c.erase(c.begin() + (long)k); return p; }
    return nullptr;
}
inline void big_give(void *p, size_t bytes) {
    if (!p) return;
    if (big_cache_on() && bytes >= ((size_t)1 << 30)) {
        int dev = 0; (void)hipGetDevice(&dev);
        void *evict = nullptr;
        {
            std::lock_guard<std::mutex> g(big_mu());
            auto &c = big_cache();
            if (c.size() >= 2) { evict = c.front().p; c.erase(c.begin()); }      // the older of the two goes: sizes nobody asks for again do not stay
            c.push_back(BigBlock{dev, bytes, p});
        }
        if (evict) (void)hipFree(evict);
        return;
    }
    (void)hipFree(p);
}

// every cached block back to the driver (c3r_trim): a host application that destroys its contexts to give HBM back gets all of it
inline size_t big_trim() {
    std::vector<BigBlock> all;
    {
        std::lock_guard<std::mutex> g(big_mu());
        all.swap(big_cache());
    }
    size_t bytes = 0;
    int cur = 0; (void)hipGetDevice(&cur);
    for (auto &b : all) { (void)hipSetDevice(b.dev); (void)hipFree(b.p); bytes += b.bytes; }
    (void)hipSetDevice(cur);
    return bytes;
}

inline void net_free(NetState &s) {
    net_each_weight_buffer([&](auto dp, auto) { if (s.*dp) (void)hipFree(s.*dp); });
    void *ptrs[] = {s.d_y2, s.d_a4, s.d_probs, s.d_tmo};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    big_give(s.d_y1, (size_t)s.cap_sites * NET_T * 2 * NET_H1 * sizeof(float));
    s = NetState();
}

#define NET_HIP(call)                                                                   \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) { err = std::string(#call) + ": " + hipGetErrorString(e_); return C3R_EHIP; } \
    } while (0)

// a fresh device buffer with src's bytes; the copy is only queued: src has to live until the stream is synchronised
template <class D, class T>
inline int net_upload(D *&dst, const std::vector<T> &src, hipStream_t st, std::string &err) {
    if (dst) { (void)hipFree(dst); dst = nullptr; }
    NET_HIP(hipMalloc((void **)&dst, src.size() * sizeof(T)));
    NET_HIP(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return C3R_OK;
}

inline int net_load(NetState &s, const float *blob, int C, hipStream_t st, std::string &err) {
    PackedNet p;
    int rc = net_pack(blob, C, p, err);
    if (rc) return rc;
    for (int l = 0; l < 3; ++l) s.wlog2[l] = p.wlog2[l];
    net_each_weight_buffer([&](auto dp, auto hv) { if (!rc) rc = net_upload(s.*dp, p.*hv, st, err); });
    const hipError_t sync = hipStreamSynchronize(st);               // (also after a failed upload: p's vectors go away on return)
    if (rc) return rc;
    if (sync != hipSuccess) { err = std::string("hipStreamSynchronize(st): ") + hipGetErrorString(sync); return C3R_EHIP; }
    if (!s.d_tmo) {
        if (hipMalloc((void **)&s.d_tmo, 64) != hipSuccess) { err = "hipMalloc(64) failed"; return C3R_ENOMEM; }
        if (hipMemsetAsync(s.d_tmo, 0, 64, st) != hipSuccess) { err = "hipMemsetAsync failed"; return C3R_EHIP; }
    }
    s.channels = C; s.loaded = true;
    return C3R_OK;
}

// The network runs over the batch in slices of at most NET_SLICE sites: the layer-1 output is 33.8 KB per site (a 0.8 M-site
// contig would take 27 GB, and sizing that buffer cost 1.2 s), a slice of 2^18 sites is 1024 workgroup rounds of layer 2 —
// far beyond what the launch needs to fill the chip — and BASELINE's chr20 batch (201,945 sites) is still one slice.
constexpr int64_t NET_SLICE = 262144;

inline int net_reserve(NetState &s, int64_t n_total, hipStream_t st, std::string &err) {
    const int64_t n = std::min(n_total, NET_SLICE);
    const int64_t need = (n + 127) / 128 * 128;    // the y1 planes are stored with the site stride rounded up to 128
    const bool want_y2 = s.precision == 0;         // split-f16 fuses L4 into layer 2: y2 (42 KB per site) is never materialised
    if (n_total > s.cap_probs) {
        NET_HIP(hipStreamSynchronize(st));
        if (s.d_probs) { (void)hipFree(s.d_probs); s.d_probs = nullptr; }
        const int64_t cap = n_total + n_total / 4 + 256;
        NET_HIP(hipMalloc((void **)&s.d_probs, (size_t)cap * C3R_NPROB * sizeof(float)));
        if (const char *e = getenv("C3R_POISON")) if (*e) { NET_HIP(hipMemsetAsync(s.d_probs, atoi(e) & 0xff, (size_t)cap * C3R_NPROB * sizeof(float), st)); NET_HIP(hipStreamSynchronize(st)); }
        s.cap_probs = cap;
    }
    if (need <= s.cap_sites && (!want_y2 || s.d_y2)) return C3R_OK;
    const bool grow = need > s.cap_sites;
    const int64_t cap = grow ? std::min((need + need / 4 + 256 + 127) / 128 * 128, NET_SLICE) : s.cap_sites;
    const auto t0_ = std::chrono::steady_clock::now();
    NET_HIP(hipStreamSynchronize(st));
    float **bufs[] = {&s.d_y1, &s.d_y2, &s.d_a4};
    const size_t sizes[] = {(size_t)cap * NET_T * 2 * NET_H1, (size_t)cap * NET_T * 2 * NET_H2, (size_t)cap * NET_L4 * 2};
    for (int i = 0; i < 3; ++i) {
        const bool is_y2 = i == 1;
        if (!grow && !is_y2) continue;                                   // only y2 is missing (precision switched to fp32)
        if (*bufs[i]) { if (i == 0) big_give(*bufs[i], (size_t)s.cap_sites * NET_T * 2 * NET_H1 * sizeof(float)); else (void)hipFree(*bufs[i]); *bufs[i] = nullptr; }
        if (is_y2 && !want_y2) continue;
        if (i == 0 && (*bufs[i] = (float *)big_take(sizes[i] * sizeof(float)))) continue;
        NET_HIP(hipMalloc((void **)bufs[i], sizes[i] * sizeof(float)));
        if (const char *e = getenv("C3R_POISON")) if (*e) { NET_HIP(hipMemsetAsync(*bufs[i], atoi(e) & 0xff, sizes[i] * sizeof(float), st)); NET_HIP(hipStreamSynchronize(st)); }
    }
    s.cap_sites = cap;
    if (getenv("C3R_TIMING")) fprintf(stderr, "[net_reserve] %lld sites per slice: %.1f ms\n", (long long)cap, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count());
    return C3R_OK;
}

// Layer 1 of the split-f16 paths: k_lstm1_rs<C3R_CH | C3R_CH_PHASED, YQ, RTS> by the context's channel count, on the (2, groups) grid.
// YQ and RTS never come together (net_forward_slice).  The six instantiations are named in the order they have always been named in:
// it decides where each lands in the code object.
inline void launch_lstm1_rs(const NetState &s, bool yq, bool rts, dim3 grid, hipStream_t st, const void *d_x, _Float16 *y1h, int n, int ns,
                            const int32_t *row_idx, float wun, int xi) {
    using kern_t = void (*)(const void *, const half8 *, _Float16 *, int, int, const int32_t *, float, int);
    const bool c18 = s.channels == C3R_CH;
    const kern_t kern = rts ? (c18 ? k_lstm1_rs<C3R_CH, false, true> : k_lstm1_rs<C3R_CH_PHASED, false, true>)
                      : c18 ? (yq ? k_lstm1_rs<C3R_CH, true> : k_lstm1_rs<C3R_CH, false>)
                            : (yq ? k_lstm1_rs<C3R_CH_PHASED, true> : k_lstm1_rs<C3R_CH_PHASED, false>);
    hipLaunchKernelGGL(kern, grid, dim3(1024), 0, st, d_x, (const half8 *)s.d_w1h, y1h, n, ns, row_idx, wun, xi);
}

// d_x: device int32 [n][33][C].  prof(name, 0|1) brackets each kernel for optional event timing.
inline int net_forward_slice(NetState &s, const void *d_x, const int32_t *row_idx, int64_t n, float *d_probs, hipStream_t st,
                             const std::function<void(const char *, int)> &prof, std::string &err, bool x16) {
    const int xi = x16 ? 1 : 0;
    const int nb = (int)((n + NET_SITES - 1) / NET_SITES);
    const dim3 grid((unsigned)((n + LSTM_SITES - 1) / LSTM_SITES), 2), block(256);
    int heads_parts = 1;
    if (s.precision == 1 || s.precision == 2) {
        // split-f16 path: y1 holds a hi and a lo f16 plane (same bytes as one fp32 plane), stored with the site stride rounded up to 128
        // so that layer 1 needs no bounds guard.  Precision 2 (f16 main term + both corrections on the block-scaled fp8 pipe,
        // k_lstm2_mx): y1 = f16 plane + fp8 plane of the same geometry.  Layer 2 has the L4 dense layer fused in: y2 is never materialised.
        _Float16 *y1h = (_Float16 *)s.d_y1;
        const int ns = (int)((n + 127) / 128 * 128);
        const dim3 g2(2, grid.x);          // the split-f16 kernels read the direction from blockIdx.x, the site group from blockIdx.y
        const bool mx = s.precision == 2;
        const bool rts = s.wlog2[0] != 12 || s.wlog2[1] != 12 || s.wlog2[2] != 12;      // (never with precision 2: c3r_lib refuses that pairing)
        if (mx && rts) { err = "the fp8-corrected path (precision 2) needs weights that fit the 2^12 split-f16 scale"; return C3R_EINVAL; }
        const float wun1 = std::ldexp(1.f, -s.wlog2[0]), wsc2 = std::ldexp(1.f, s.wlog2[1]), wun2 = std::ldexp(1.f, -s.wlog2[1]), wun4 = std::ldexp(1.f, -s.wlog2[2]);
        prof("k_lstm1", 0);
        launch_lstm1_rs(s, mx, rts, g2, st, d_x, y1h, (int)n, ns, row_idx, rts ? wun1 : WUNSCALE, xi);
        prof("k_lstm1", 1);
        prof("k_lstm2", 0);
        if (rts)
            hipLaunchKernelGGL((k_lstm2_w16<0, true>), g2, dim3(512), 0, st, (const _Float16 *)y1h, (const half8 *)s.d_w2w, (const float *)s.d_b2, (int)n,
                               (const half8 *)s.d_w4w, s.d_a4, ns, wsc2, wun2, wun4, s.d_tmo);
        else if (mx)
            hipLaunchKernelGGL(k_lstm2_mx, g2, dim3(512), 0, st, (const _Float16 *)y1h, (const half8 *)s.d_w2h, (const uint32_t *)s.d_w2q, (const uint32_t *)s.d_w2s,
                               (const float *)s.d_b2, (int)n, (const half8 *)s.d_w4f, (const uint32_t *)s.d_w4q, (const uint32_t *)s.d_w4s, s.d_a4, ns, s.d_tmo);
        else
            hipLaunchKernelGGL((k_lstm2_w16<0, false>), g2, dim3(512), 0, st, (const _Float16 *)y1h, (const half8 *)s.d_w2w, (const float *)s.d_b2, (int)n,
                               (const half8 *)s.d_w4w, s.d_a4, ns, WSCALE, WUNSCALE, WUNSCALE, s.d_tmo);
        prof("k_lstm2", 1);
        heads_parts = 2;
    } else {
        prof("k_lstm1", 0);
        if (s.channels == C3R_CH)
            hipLaunchKernelGGL((k_lstm<NET_INP1, C3R_CH, NET_H1, true, LSTM_SB>), grid, block, 0, st, (const void *)d_x,
                               (const float4 *)s.d_w1, (const float *)s.d_b1, s.d_y1, (int)n, row_idx, xi);
        else
            hipLaunchKernelGGL((k_lstm<NET_INP1, C3R_CH_PHASED, NET_H1, true, LSTM_SB>), grid, block, 0, st, (const void *)d_x,
                               (const float4 *)s.d_w1, (const float *)s.d_b1, s.d_y1, (int)n, row_idx, xi);
        prof("k_lstm1", 1);
        prof("k_lstm2", 0);
        hipLaunchKernelGGL((k_lstm<2 * NET_H1, 2 * NET_H1, NET_H2, false, LSTM_SB>), grid, block, 0, st, (const void *)s.d_y1,
                           (const float4 *)s.d_w2, (const float *)s.d_b2, s.d_y2, (int)n);
        prof("k_lstm2", 1);
        prof("k_fc4", 0);
        hipLaunchKernelGGL(k_fc4, dim3(nb), block, 0, st, (const float *)s.d_y2, (const float4 *)s.d_w4, (const float *)s.d_b4, s.d_a4, (int)n);
        prof("k_fc4", 1);
    }
    prof("k_heads", 0);
    hipLaunchKernelGGL(k_heads_mfma, dim3((unsigned)((n + 31) / 32)), block, 0, st, (const float *)s.d_a4, heads_parts, (const float *)s.d_b4,
                       (const float4 *)s.d_w5p, (const float *)s.d_b5, (const float4 *)s.d_wcp, (const float *)s.d_bo, d_probs, (int)n);
    prof("k_heads", 1);
    NET_HIP(hipGetLastError());
    return C3R_OK;
}

// d_x: device int32 [rows][33][C]; site i of the batch reads row row_idx[i] (row_idx == nullptr: row i)
// x16: the rows are int16 (the tensor build's windows) instead of int32 (a caller's batch, the calibration windows)
inline int net_forward(NetState &s, const void *d_x, const int32_t *row_idx, int64_t n, hipStream_t st,
                       const std::function<void(const char *, int)> &prof, std::string &err, bool x16 = false) {
    int rc = net_reserve(s, n, st, err);
    if (rc) return rc;
    const int64_t step = std::min(n, NET_SLICE);
    for (int64_t off = 0; off < n; off += step) {
        const int64_t m = std::min(step, n - off);
        const void *x = row_idx ? d_x : (const void *)((const char *)d_x + (size_t)off * NET_T * s.channels * (x16 ? 2 : 4));
        if ((rc = net_forward_slice(s, x, row_idx ? row_idx + off : nullptr, m, s.d_probs + (size_t)off * C3R_NPROB, st, prof, err, x16))) return rc;
    }
    return C3R_OK;
}

}  // namespace c3r
