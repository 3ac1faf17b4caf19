// Host-side check of k_lstm2_w16's operand packing (clair3_rna_amd/csrc/net_pack.hpp: pack_lstm2_w16, pack_l4_w16; net_kernels.hpp: w16_bias_row):
// compiled by hipcc, runs without a GPU.  Every weight is packed with a value that names its Keras position, read back at the address the
// kernel loads it from (ldw: unit u = 2G + st, tile, hi|lo, lane), and compared with what v_mfma_f32_16x16x32_f16 makes of it:
//   A lane l, element e  = A[row l % 16][k = 8 (l / 16) + e] of k-group G   (the B operand of lane l holds the same k of column l % 16)
//   accumulator lane l'  = rows 4 (l' / 16) + 0..3 of column l' % 16        (the kernel reads row 4q + m as gate m of unit 8T + 2q + st)
// so the weight in lane l, element e must be W[k = 32G + 8 (l / 16) + e][gate (l % 4) of unit 8T + 2 ((l % 16) / 4) + st], and every Keras
// (k, gate, unit) must appear exactly once.  Both directions, and the fused L4 (row l % 16 <-> output 32 quarter + 16 st + l % 16).
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../clair3_rna_amd/csrc/net_kernels.hpp"   // w16_bias_row
#include "../../clair3_rna_amd/csrc/net_pack.hpp"      // the packers
using namespace c3r;

static int check_layer2() {
    const int INP = 2 * NET_H1, H = NET_H2, K = INP + H, NG = K / 32, NU = 2 * NG, NBLK = 4 * H / 32, NTQ = NBLK / 4;
    // W[k][col] = (k * 4H + col + 1) / 16: below 2^15, and hi + lo holds it exactly (22 significant bits)
    std::vector<float> Kin((size_t)INP * 4 * H), R((size_t)H * 4 * H), b(4 * H);
    for (int k = 0; k < K; ++k)
        for (int c = 0; c < 4 * H; ++c) (k < INP ? Kin[(size_t)k * 4 * H + c] : R[(size_t)(k - INP) * 4 * H + c]) = (float)((size_t)k * 4 * H + c + 1);
    for (int c = 0; c < 4 * H; ++c) b[c] = (float)(c + 1);
    std::vector<uint16_t> wp, one;
    std::vector<float> wf, bpk;
    for (int d = 0; d < 2; ++d) {          // a direction is one pack call; the kernel offsets by dir * 4 quarters (checked as such)
        pack_lstm2_w16(Kin.data(), INP, R.data(), H, one, 1.f / 16.f);
        wp.insert(wp.end(), one.begin(), one.end());
    }
    std::vector<int> seen((size_t)2 * K * 4 * H, 0);
    for (int d = 0; d < 2; ++d)
        for (int sq = 0; sq < 4; ++sq)
            for (int u = 0; u < NU; ++u)
                for (int tile = 0; tile < NTQ; ++tile)
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 8; ++e) {
                            // the kernel's address: wl = Wp + ((dir * 4 + sq) * NU) * NTQ * 2 * 64 + TOFF * 2 * 64 + lane, + u * NTQ * 2 * 64 + (tt * 2 + hl) * 64
                            const size_t a = (((size_t)(d * 4 + sq) * NU + u) * NTQ * 2 + tile * 2) * 64 + l;
                            const double v = ((double)h2f(wp[a * 8 + e]) + (double)h2f(wp[(a + 64) * 8 + e])) * 16.0;
                            const int G = u >> 1, st = u & 1, T = sq * NTQ + tile, r = l & 15;
                            const int k = 32 * G + 8 * (l >> 4) + e, unit = 8 * T + 2 * (r >> 2) + st, m = r & 3;
                            const double want = (double)((size_t)k * 4 * H + m * H + unit + 1);
                            if (v != want) {
                                printf("layer 2: dir %d quarter %d unit-step %d tile %d lane %d e %d holds %.1f, want k %d gate %d unit %d (%.1f)\n", d, sq, u, tile, l, e, v, k, m, unit, want);
                                return 1;
                            }
                            ++seen[((size_t)d * K + k) * 4 * H + m * H + unit];
                        }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) { printf("layer 2: Keras weight %zu packed %d times\n", i, seen[i]); return 1; }
    // bias: the kernel reads pack_lstm_dir's tile row w16_bias_row(st, q, m) for accumulator row 4q + m of subtile st
    pack_lstm_dir(Kin.data(), INP, INP, R.data(), b.data(), H, wf, bpk);
    for (int T = 0; T < NBLK; ++T)
        for (int st = 0; st < 2; ++st)
            for (int q = 0; q < 4; ++q)
                for (int m = 0; m < 4; ++m)
                    if (bpk[(size_t)T * 32 + w16_bias_row(st, q, m)] != b[m * H + 8 * T + 2 * q + st]) {
                        printf("bias: tile %d st %d row %d is not gate %d of unit %d\n", T, st, 4 * q + m, m, 8 * T + 2 * q + st);
                        return 1;
                    }
    printf("layer 2 ok: %d k x %d gate rows per direction, both directions, bias rows\n", K, 4 * H);
    return 0;
}

static int check_l4() {
    const int H = NET_H2, NU4 = H / 16;
    std::vector<float> W4((size_t)NET_FLAT * NET_L4);
    for (size_t i = 0; i < W4.size(); ++i) W4[i] = (float)(i + 1);          // (row * 128 + o + 1) / 128 < 2^14
    std::vector<uint16_t> w4p;
    pack_l4_w16(W4.data(), 1.f / 128.f, w4p);
    std::vector<int> seen(W4.size(), 0);
    for (int d = 0; d < 2; ++d)
        for (int t = 0; t < NET_T; ++t)
            for (int sq = 0; sq < 4; ++sq)
                for (int u = 0; u < NU4; ++u)
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 8; ++e) {
                            // the kernel's address: W4p + (((dir * NET_T + t) * 4 + sq) * 2 * NGH) * 2 * 64 + lane, + u * 2 * 64 (+ 64 for lo)
                            const size_t a = ((((size_t)(d * NET_T + t) * 4 + sq) * NU4 + u) * 2) * 64 + l;
                            const double v = ((double)h2f(w4p[a * 8 + e]) + (double)h2f(w4p[(a + 64) * 8 + e])) * 128.0;
                            const int k = 32 * (u >> 1) + 8 * (l >> 4) + e, o = 32 * sq + 16 * (u & 1) + (l & 15);
                            const size_t row = (size_t)t * 2 * H + (size_t)d * H + k;
                            if (v != (double)(row * NET_L4 + o + 1)) {
                                printf("L4: dir %d t %d quarter %d unit-step %d lane %d e %d holds %.1f, want row %zu output %d\n", d, t, sq, u, l, e, v, row, o);
                                return 1;
                            }
                            ++seen[row * NET_L4 + o];
                        }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) { printf("L4: weight %zu packed %d times\n", i, seen[i]); return 1; }
    printf("L4 ok: %d x %d\n", NET_FLAT, NET_L4);
    return 0;
}

int main() {
    if (check_layer2() || check_l4()) return 1;
    printf("w16 layout ok\n");
    return 0;
}
