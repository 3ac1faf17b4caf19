// net_pack.hpp — the network's dimensions and the host-side packing of its weights into the layouts the kernels of net_kernels.hpp load.
//
// Host-only and free of ROCm headers (plain g++ compiles it: tests/c/net_pack_check.cpp).  net_pack turns a weight blob (the Keras
// arrays in model order, c3r_load_weights) into one std::vector per device buffer; net_host.hpp uploads them as they are.  The layout
// comments above the packers are the specification of what the kernels load.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/c3r.h"

namespace c3r {

constexpr int NET_H1 = 128;
constexpr int NET_H2 = 160;
constexpr int NET_T = C3R_WINDOW;          // 33 time steps
constexpr int NET_FLAT = NET_T * 2 * NET_H2;   // 10560
constexpr int NET_L4 = 128;
// the split-f16 scale of ordinary weights (see "Split-f16 path" in net_kernels.hpp)
constexpr float WSCALE_LOG2 = 12.0f;
constexpr float WSCALE = 4096.0f;
constexpr float WUNSCALE = 1.0f / 4096.0f;

inline int64_t net_weight_count(int C) {
    int64_t n = 0;
    n += 2 * ((int64_t)C * 4 * NET_H1 + (int64_t)NET_H1 * 4 * NET_H1 + 4 * NET_H1);
    n += 2 * ((int64_t)2 * NET_H1 * 4 * NET_H2 + (int64_t)NET_H2 * 4 * NET_H2 + 4 * NET_H2);
    n += (int64_t)NET_FLAT * NET_L4 + NET_L4;
    n += 2 * (128 * 128 + 128);
    n += 128 * 21 + 21 + 128 * 3 + 3;
    return n;
}

// float -> IEEE binary16 (round to nearest even) and back, host side
inline uint16_t f2h(float f) {
    uint32_t x; memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    const int32_t e = (int32_t)((x >> 23) & 0xff) - 127 + 15;
    uint32_t m = x & 0x7fffffu;
    if (((x >> 23) & 0xff) == 0xff) return (uint16_t)(sign | 0x7c00u | (m ? 0x200u : 0));
    if (e >= 31) return (uint16_t)(sign | 0x7c00u);
    if (e <= 0) {
        if (e < -10) return (uint16_t)sign;
        m |= 0x800000u;
        const int shift = 14 - e;
        uint32_t hm = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (hm & 1u))) ++hm;
        return (uint16_t)(sign | hm);
    }
    uint32_t h = (uint32_t)(e << 10) | (m >> 13);
    const uint32_t rem = m & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
    return (uint16_t)(sign | h);
}
inline float h2f(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 0x1f, m = h & 0x3ffu, x;
    if (e == 0) {
        if (m == 0) x = sign;
        else { int sh = 0; while (!(m & 0x400u)) { m <<= 1; ++sh; } m &= 0x3ffu; x = sign | ((uint32_t)(127 - 15 - sh + 1) << 23) | (m << 13); }
    } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
    else x = sign | ((e - 15 + 127) << 23) | (m << 13);
    float f; memcpy(&f, &x, 4); return f;
}
inline void split_h(float v, uint16_t &hi, uint16_t &lo) { hi = f2h(v); lo = f2h(v - h2f(hi)); }

// ---- the one fragment writer.  A fragment is what the 64 lanes of a wavefront load as the A operand of one (row tile, k-group): lane l
// holds row l % R of the tile and k-chunk l / R, the E consecutive k = KG g + E (l / R) + 0..E-1 of k-group g (KG = 64 / R * E k wide).
//   R = 32, E = 4: two steps of v_mfma_f32_32x32x2_f32 per lane half (f32);  R = 32, E = 8: v_mfma_f32_32x32x16_f16;
//   R = 16, E = 8: v_mfma_f32_16x16x32_f16
// SPLIT = false stores the weight as f32.  SPLIT = true stores scale * weight as two f16 planes, hi = f16(v) and lo = f16(v - hi), the lo
// fragment 64 lanes after the hi fragment.
//   at(tile, g)   : where the fragment lives in `out`, as the index of its lane 0 in units of lanes (E elements each)
//   w(tile, r, k) : the weight of row r of the tile at k
// `out` is sized (and zeroed) by the caller.
template <int R, int E, bool SPLIT, class T, class AT, class WT>
inline void pack_frags(std::vector<T> &out, int ntiles, int ngroups, float scale, AT &&at, WT &&w) {
    static_assert((R == 32 || R == 16) && (E == 4 || E == 8), "rows per tile: 32 or 16; elements per lane: 4 or 8");
    static_assert(sizeof(T) == (SPLIT ? 2 : 4), "f32 fragments are floats, split-f16 fragments are f16 bit patterns");
    constexpr int KG = 64 / R * E;
    for (int tile = 0; tile < ntiles; ++tile)
        for (int g = 0; g < ngroups; ++g) {
            T *f = out.data() + (size_t)at(tile, g) * E;
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < E; ++e) {
                    const float v = w(tile, l % R, KG * g + E * (l / R) + e);
                    if constexpr (SPLIT) split_h(scale * v, f[l * E + e], f[(64 + l) * E + e]);
                    else f[l * E + e] = v;
                }
        }
}

// Gate rows.  The rows of a gate tile are permuted so that a lane's accumulator rows are the four gates (Keras columns i|f|c|o, H apart)
// of whole units — the cell update is lane-local.  One rule per tile shape:
//   32-row tile `tile`: row r = 8q + 4hh + m <-> gate m of unit 8 tile + 4hh + q   (k_lstm, k_lstm1_rs, k_lstm2_mx; the bias layout)
inline int gate_col32(int tile, int r, int H) {
    const int q = r >> 3, hh = (r >> 2) & 1, m = r & 3;
    return m * H + 8 * tile + 4 * hh + q;
}
//   16-row tile t16 = 2T + st (subtile st of the 32-row tile T): row r = 4q + m <-> gate m of unit 8T + 2q + st   (k_lstm2_w16)
inline int gate_col16(int t16, int r, int H) {
    const int T = t16 >> 1, st = t16 & 1, q = r >> 2, m = r & 3;
    return m * H + 8 * T + 2 * q + st;
}

// Wcat = [K_in (cin rows, padded with zero rows to inp) ; R] of one LSTM direction, [inp + H][4H] (Keras: [in][4H], gate-major columns
// i|f|c|o).  bias_slot != nullptr: that vector rides on the first padded input slot (k = cin).
struct LstmW {
    const float *Kin; int cin, inp; const float *R; int H; const float *bias_slot;
    float operator()(int k, int col) const {
        if (k < inp) return k < cin ? Kin[(size_t)k * 4 * H + col] : (bias_slot && k == cin ? bias_slot[col] : 0.f);
        return R[(size_t)(k - inp) * 4 * H + col];
    }
};
// flatten row of h index k of direction d at time t, dt = d * NET_T + t: the flatten order is [t][fwd 160 | bwd 160]
inline size_t l4_row(int dt, int k) { return (size_t)(dt % NET_T) * 2 * NET_H2 + (size_t)(dt / NET_T) * NET_H2 + k; }

// Pack one LSTM direction: Wcat into MFMA fragment order [quarter(4)][g][tile][64 lanes][4] (k-groups of 8; lane half kh owns
// k = 8g + 4kh + 0..3) and the bias into [blk][r = 8q + 4hh + m] (gate_col32).
inline void pack_lstm_dir(const float *Kin, int cin, int inp, const float *R, const float *b, int H,
                          std::vector<float> &wp, std::vector<float> &bpk) {
    const int K = inp + H, NG = K / 8, NBLK = 4 * H / 32, NT = NBLK / 4;
    const LstmW wcat{Kin, cin, inp, R, H, nullptr};
    wp.assign((size_t)NBLK * NG * 64 * 4, 0.f);
    pack_frags<32, 4, false>(wp, NBLK, NG, 1.f, [&](int blk, int g) { return (((size_t)(blk / NT) * NG + g) * NT + (blk % NT)) * 64; },
                             [&](int blk, int r, int k) { return wcat(k, gate_col32(blk, r, H)); });
    bpk.assign((size_t)NBLK * 32, 0.f);
    for (int blk = 0; blk < NBLK; ++blk)
        for (int r = 0; r < 32; ++r) bpk[(size_t)blk * 32 + r] = b[gate_col32(blk, r, H)];
}

// Split-f16 packing of one LSTM direction: [quarter(4)][g16][tile][hi|lo][64 lanes][8 halves], weights x 2^s (k-groups of 16; lane half kh
// owns k = 16g + 8kh + 0..7).  bias_slot != nullptr (layer 1): the bias rides on the first padded input slot (k = cin).
inline void pack_lstm_dir_h(const float *Kin, int cin, int inp, const float *R, int H, std::vector<uint16_t> &wp, const float *bias_slot = nullptr, float wscale = WSCALE) {
    const int K = inp + H, NG = K / 16, NBLK = 4 * H / 32, NT = NBLK / 4;
    const LstmW wcat{Kin, cin, inp, R, H, bias_slot};
    wp.assign((size_t)NBLK * NG * 2 * 64 * 8, 0);
    pack_frags<32, 8, true>(wp, NBLK, NG, wscale, [&](int blk, int g) { return ((((size_t)(blk / NT) * NG + g) * NT + (blk % NT)) * 2) * 64; },
                            [&](int blk, int r, int k) { return wcat(k, gate_col32(blk, r, H)); });
}

// k_lstm2_w16's layer-2 fragments of one direction: [quarter(4)][u = 2G + st (26)][tile(5)][hi|lo][64 lanes][8 halves], weights x 2^s.
// Lane l of unit (G, st) of tile T holds row l % 16 of subtile st = gate m of unit 8T + 2q + st (l % 16 = 4q + m), k = 32G + 8 (l / 16) + 0..7
// (v_mfma_f32_16x16x32_f16: A[row l % 16][k = 8 (l / 16) + i]; its accumulator gives lane l rows 4 (l / 16) + 0..3).
inline void pack_lstm2_w16(const float *Kin, int inp, const float *R, int H, std::vector<uint16_t> &wp, float wscale) {
    const int K = inp + H, NG = K / 32, NU = 2 * NG, NBLK = 4 * H / 32, NT = NBLK / 4;
    const LstmW wcat{Kin, inp, inp, R, H, nullptr};
    wp.assign((size_t)NBLK * NU * 2 * 64 * 8, 0);
    pack_frags<16, 8, true>(wp, 2 * NBLK, NG, wscale,
                            [&](int t16, int g) { const int T = t16 >> 1, st = t16 & 1; return ((((size_t)(T / NT) * NU + 2 * g + st) * NT + (T % NT)) * 2) * 64; },
                            [&](int t16, int r, int k) { return wcat(k, gate_col16(t16, r, H)); });
}
// k_lstm2_w16's fused L4 fragments: [dir][t][quarter(4)][u = 2G + st (H / 16)][hi|lo][64 lanes][8]; lane l: L4 output 32 quarter + 16 st + l % 16,
// h index k = 32G + 8 (l / 16) + 0..7 of direction d at time t (flatten row t * 2H + d * H + k)
inline void pack_l4_w16(const float *W4, float wscale, std::vector<uint16_t> &w4p) {
    const int NU4 = NET_H2 / 16;
    w4p.assign((size_t)2 * NET_T * 4 * NU4 * 2 * 64 * 8, 0);
    // tile = (dt, 16-row tile t16 = 2 quarter + st): 8 tiles per (direction, time)
    pack_frags<16, 8, true>(w4p, 2 * NET_T * 8, NET_H2 / 32, wscale,
                            [&](int tile, int g) { const int dt = tile >> 3, sq = (tile >> 1) & 3, st = tile & 1; return ((((size_t)dt * 4 + sq) * NU4 + 2 * g + st) * 2) * 64; },
                            [&](int tile, int r, int k) { return W4[l4_row(tile >> 3, k) * NET_L4 + 16 * (tile & 7) + r]; });
}

// ---- precision 2: the two correction terms on the block-scaled fp8 pipe (v_mfma_scale_f32_32x32x64_f8f6f4, K = 64 = two terms x 32 k).
// float -> OCP e4m3fn, round to nearest even, saturating (|v| < 256 by construction here)
inline uint8_t f2e4m3(float v) {
    const uint8_t sign = std::signbit(v) ? 0x80 : 0;
    float a = std::fabs(v);
    if (!(a == a)) return 0x7f;
    if (a >= 464.f) return (uint8_t)(sign | 0x7e);
    if (a < 0.015625f) {                                   // subnormal: multiples of 2^-9
        const int q = (int)std::nearbyint(a * 512.f);
        return (uint8_t)(sign | q);                        // q == 8 is the smallest normal (0x08)
    }
    int e;
    const float fr = std::frexp(a, &e);                    // a = fr * 2^e, fr in [0.5, 1)
    int q = (int)std::nearbyint((fr * 2.f - 1.f) * 8.f), ex = e - 1;
    if (q == 8) { q = 0; ++ex; }
    int code = ((ex + 7) << 3) | q;
    if (code > 0x7e) code = 0x7e;
    return (uint8_t)(sign | code);
}
// One fragment set: rows = NBLK tiles of 32 gate rows (row r of tile blk <-> column col(blk, r) of W), k = k0 .. k0 + 32 * nkb.
// K order of the instruction (tools/mx_scale_probe.hip): a lane (r, g = lane / 32) holds k = 16 g + 0..15 of the FIRST scale block
// in its bytes 0-15 and k = 32 + 16 g + 0..15, the second scale block, in its bytes 16-31; the scale byte of lane r covers the first
// block of row r, that of lane 32 + r the second.  First block = term 0 (w), second = term 1 (w - f16(w)):
//   q: [quarter][kb][tile][term][64 lanes][16 bytes]   lane = 32 g + r: k = k0 + 32 kb + 16 g + 0..15; a lane's operand = its term-0 bytes then its term-1 bytes
//   sc: [quarter][kb / 4][tile][64 lanes] u32    lane = 32 term + r, byte kb % 4 = E8M0 scale: 2^(sc - 127) * byte = 2^12 * value
template <class WF>
inline void pack_mx(WF &&w /* (k, blk, r) -> weight */, int NBLK, int NT, int k0, int nkb, std::vector<uint32_t> &q, std::vector<uint32_t> &sc) {
    const int nk4 = (nkb + 3) / 4;
    q.assign((size_t)NBLK * nkb * 64 * 8, 0u);
    sc.assign((size_t)NBLK * nk4 * 64, 0x7f7f7f7fu);
    uint8_t *qb = reinterpret_cast<uint8_t *>(q.data());
    uint8_t *sb = reinterpret_cast<uint8_t *>(sc.data());
    for (int blk = 0; blk < NBLK; ++blk)
        for (int r = 0; r < 32; ++r)
            for (int kb = 0; kb < nkb; ++kb)
                for (int term = 0; term < 2; ++term) {
                    float v[32], m = 0.f;
                    for (int b = 0; b < 32; ++b) {
                        const float x = w(k0 + 32 * kb + b, blk, r);
                        v[b] = term ? x - h2f(f2h(WSCALE * x)) * WUNSCALE : x;       // (the f16 main term carries f16(2^12 w))
                        m = std::max(m, std::fabs(v[b]));
                    }
                    int e = 0;                                                   // block scale 2^e: the block's maximum lands in [128, 256)
                    if (m > 0.f) { int ex; (void)std::frexp(m, &ex); e = 8 - ex; }
                    e = std::min(e, 139);                                        // (E8M0 byte = 139 - e >= 0)
                    const size_t fo = (((size_t)(blk / NT) * nkb + kb) * NT + (blk % NT)) * 64;
                    // (each 16-byte half of a lane's 32 bytes is stored as its own 1 KiB run of the 64 lanes: two fully coalesced loads)
                    for (int b = 0; b < 32; ++b) qb[((fo * 2 + (size_t)term * 64) + 32 * (b / 16) + r) * 16 + (b % 16)] = f2e4m3(std::ldexp(v[b], e));
                    const size_t so = ((((size_t)(blk / NT) * nk4 + kb / 4) * NT + (blk % NT)) * 64 + 32 * term + r) * 4 + (kb % 4);
                    sb[so] = (uint8_t)std::max(0, 127 + (int)WSCALE_LOG2 - e);
                }
}

// What net_pack makes of a weight blob: one vector per device buffer (net_host.hpp pairs each with its NetState pointer).
struct PackedNet {
    std::vector<float> w1, b1, w2, b2;          // fp32 path: packed LSTM1 / LSTM2, both directions (pack_lstm_dir)
    std::vector<float> w4, b4;                  // fp32 path: packed L4 (k_fc4); b4 also feeds k_heads_mfma
    std::vector<float> b5, bo, w5p, wcp;        // heads: biases, and the weights in MFMA fragment order (k_heads_mfma)
    std::vector<uint16_t> w1h, w2h;             // split-f16 LSTM1 (k_lstm1_rs) / LSTM2 (k_lstm2_mx's main term), pack_lstm_dir_h
    std::vector<uint16_t> w4f;                  // split-f16 L4 per (dir, t), 32-row tiles (k_lstm2_mx's fused epilogue)
    std::vector<uint16_t> w2w, w4w;             // k_lstm2_w16's layer-2 and fused-L4 fragments (pack_lstm2_w16, pack_l4_w16)
    // precision 2 (MX corrections): fp8 (e4m3) fragments of w (lanes 0-31) and w - f16(w) (lanes 32-63) per block of 32 k, 32 bytes per
    // lane, and their E8M0 block scales, four blocks per dword: layer 2, fused L4
    std::vector<uint32_t> w2q, w2s, w4q, w4s;
    // log2 of the power-of-two scale the split-f16 weights of layer 1 / layer 2 / L4 were packed with: 12 unless some |w| (or a bias that
    // travels with the weights) would overflow f16 at 2^12; below 12 the run-time-scale variants of the kernels run
    int wlog2[3] = {12, 12, 12};
};

constexpr int NET_INP1 = 32;   // layer 1's input width, padded to an even number of 8-wide k-groups

template <class T>
inline void append(std::vector<T> &to, const std::vector<T> &from) { to.insert(to.end(), from.begin(), from.end()); }

// blob: net_weight_count(C) floats, the Keras arrays in model order.  C3R_EINVAL for a blob that holds a non-finite value.
inline int net_pack(const float *blob, int C, PackedNet &out, std::string &err) {
    out = PackedNet();
    const float *q = blob;
    std::vector<float> tw, tb;
    std::vector<uint16_t> th;
    std::vector<uint32_t> tq, ts;
    // ---- the split-f16 scale of each layer.  2^12 keeps the lo halves of ordinary weights normal f16 numbers, but f16 ends at 65504: a
    // weight (or a bias: layer 1's rides on an input slot, layer 2's is multiplied by the same scale) of 16 or more would become inf and
    // the probabilities NaN.  So the scale is the largest power of two <= 2^12 that keeps 2^s max|w| <= 2^15 (a factor two of headroom);
    // nothing in clair3_rna/model.py:126-172 bounds the weights.  Non-finite values are refused.
    {
        const int64_t nw = net_weight_count(C);
        for (int64_t i = 0; i < nw; ++i) if (!std::isfinite(blob[i])) { err = "weight blob holds a non-finite value (index " + std::to_string(i) + ")"; return C3R_EINVAL; }
        auto amax = [](const float *p, size_t n) { float m = 0.f; for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(p[i])); return m; };
        const size_t n1 = (size_t)C * 4 * NET_H1 + (size_t)NET_H1 * 4 * NET_H1 + 4 * NET_H1, n2 = (size_t)2 * NET_H1 * 4 * NET_H2 + (size_t)NET_H2 * 4 * NET_H2 + 4 * NET_H2;
        const float m[3] = {amax(blob, 2 * n1), amax(blob + 2 * n1, 2 * n2), amax(blob + 2 * n1 + 2 * n2, (size_t)NET_FLAT * NET_L4)};
        for (int l = 0; l < 3; ++l) {
            int sl = 12;
            while (sl > -24 && std::ldexp(m[l], sl) > 32768.f) --sl;
            out.wlog2[l] = sl;
        }
    }
    const float wsc1 = std::ldexp(1.f, out.wlog2[0]), wsc2 = std::ldexp(1.f, out.wlog2[1]), wsc4 = std::ldexp(1.f, out.wlog2[2]);
    // (layer 1 has no fp8 fragments: the integer pileup counts go through the f16 pipe, split exactly (k_lstm1_rs), never through fp8)
    for (int d = 0; d < 2; ++d) {
        const float *Kin = q; q += (size_t)C * 4 * NET_H1;
        const float *R = q; q += (size_t)NET_H1 * 4 * NET_H1;
        const float *b = q; q += 4 * NET_H1;
        pack_lstm_dir(Kin, C, NET_INP1, R, b, NET_H1, tw, tb);
        append(out.w1, tw); append(out.b1, tb);
        pack_lstm_dir_h(Kin, C, NET_INP1, R, NET_H1, th, b, wsc1);
        append(out.w1h, th);
    }
    for (int d = 0; d < 2; ++d) {
        const float *Kin = q; q += (size_t)2 * NET_H1 * 4 * NET_H2;
        const float *R = q; q += (size_t)NET_H2 * 4 * NET_H2;
        const float *b = q; q += 4 * NET_H2;
        pack_lstm_dir(Kin, 2 * NET_H1, 2 * NET_H1, R, b, NET_H2, tw, tb);
        append(out.w2, tw); append(out.b2, tb);
        pack_lstm_dir_h(Kin, 2 * NET_H1, 2 * NET_H1, R, NET_H2, th, nullptr, wsc2);
        append(out.w2h, th);
        pack_lstm2_w16(Kin, 2 * NET_H1, R, NET_H2, th, wsc2);
        append(out.w2w, th);
        const LstmW wcat{Kin, 2 * NET_H1, 2 * NET_H1, R, NET_H2, nullptr};
        pack_mx([&](int k, int blk, int r) { return wcat(k, gate_col32(blk, r, NET_H2)); }, 4 * NET_H2 / 32, 4 * NET_H2 / 128, 0, (2 * NET_H1 + NET_H2) / 32, tq, ts);
        append(out.w2q, tq); append(out.w2s, ts);
    }
    const float *W4 = q; q += (size_t)NET_FLAT * NET_L4;
    const float *b4 = q; q += NET_L4;
    const float *W51 = q; q += 128 * 128; const float *b51 = q; q += 128;
    const float *W52 = q; q += 128 * 128; const float *b52 = q; q += 128;
    const float *Wg = q; q += 128 * 21; const float *bg = q; q += 21;
    const float *Wz = q; q += 128 * 3; const float *bz = q; q += 3;
    // L4 packed [blk(4)][g][lane][s]: row r of block blk <-> output unit 32*blk + r
    const int NG4 = NET_FLAT / 8;
    out.w4.assign((size_t)4 * NG4 * 64 * 4, 0.f);
    pack_frags<32, 4, false>(out.w4, 4, NG4, 1.f, [&](int blk, int g) { return ((size_t)blk * NG4 + g) * 64; },
                             [&](int blk, int r, int k) { return W4[(size_t)k * NET_L4 + 32 * blk + r]; });
    // L4 for the fused LSTM2 epilogue: [dir][t][blk(4)][g(10)][hi|lo][lane][8]; flatten order is [t][fwd 160 | bwd 160]
    const int NGF = NET_H2 / 16;
    out.w4f.assign((size_t)2 * NET_T * 4 * NGF * 2 * 64 * 8, 0);
    pack_frags<32, 8, true>(out.w4f, 2 * NET_T * 4, NGF, wsc4, [&](int tile, int g) { return (((size_t)tile * NGF + g) * 2) * 64; },      // tile = (dt, blk)
                            [&](int tile, int r, int k) { return W4[l4_row(tile >> 2, k) * NET_L4 + 32 * (tile & 3) + r]; });
    pack_l4_w16(W4, wsc4, out.w4w);
    // fused L4 on the MX pipe: per (dir, t) one fragment set [quarter(4)][kb(5)][lane][32 B] (one tile per quarter)
    for (int dt = 0; dt < 2 * NET_T; ++dt) {
        pack_mx([&](int k, int blk, int r) { return W4[l4_row(dt, k) * NET_L4 + 32 * blk + r]; }, 4, 1, 0, NET_H2 / 32, tq, ts);
        append(out.w4q, tq); append(out.w4s, ts);
    }
    out.b4.assign(b4, b4 + NET_L4);
    // heads: W5 = [L5_1 | L5_2], [128][256], and the 24 logits Wo = [21 genotype | 3 zygosity], [128][24], each with its bias
    std::vector<float> w5((size_t)128 * 256), wo((size_t)128 * 24);
    out.b5.resize(256); out.bo.resize(24);
    for (int k = 0; k < 128; ++k)
        for (int o = 0; o < 128; ++o) { w5[(size_t)k * 256 + o] = W51[k * 128 + o]; w5[(size_t)k * 256 + 128 + o] = W52[k * 128 + o]; }
    for (int o = 0; o < 128; ++o) { out.b5[o] = b51[o]; out.b5[128 + o] = b52[o]; }
    for (int k = 0; k < 128; ++k) {
        for (int o = 0; o < 21; ++o) wo[(size_t)k * 24 + o] = Wg[k * 21 + o];
        for (int o = 0; o < 3; ++o) wo[(size_t)k * 24 + 21 + o] = Wz[k * 3 + o];
    }
    for (int o = 0; o < 21; ++o) out.bo[o] = bg[o];
    for (int o = 0; o < 3; ++o) out.bo[21 + o] = bz[o];
    // heads for k_heads_mfma: W5 as 8 row tiles [blk(8)][g(16)][lane][s]; the 24 logits as one tile over K = 256 = a5 = [L5_1 | L5_2]
    // (block structure: rows 0-20 read the first half, rows 21-23 the second), [g(32)][lane][s]
    out.w5p.assign((size_t)8 * 16 * 64 * 4, 0.f);
    pack_frags<32, 4, false>(out.w5p, 8, 16, 1.f, [&](int blk, int g) { return ((size_t)blk * 16 + g) * 64; },
                             [&](int blk, int r, int k) { return w5[(size_t)k * 256 + 32 * blk + r]; });
    out.wcp.assign((size_t)32 * 64 * 4, 0.f);
    pack_frags<32, 4, false>(out.wcp, 1, 32, 1.f, [&](int, int g) { return (size_t)g * 64; },
                             [&](int, int r, int k) { return r < 21 && k < 128 ? wo[(size_t)k * 24 + r] : r >= 21 && r < 24 && k >= 128 ? wo[(size_t)(k - 128) * 24 + r] : 0.f; });
    return C3R_OK;
}

}  // namespace c3r
