// Host-side record of what net_pack (clair3_rna_amd/csrc/net_pack.hpp) makes of a weight blob: plain g++, no GPU, no ROCm header.
// Blobs come from a fixed xorshift64 seed; for every PackedNet buffer the program prints its name, its byte count and the 64-bit FNV-1a
// hash of its bytes, plus the three split-f16 scale exponents.  tests/test_net_pack.py compares the output with
// tests/golden/net_pack_hashes.json, recorded from the packers as they stood before they moved into net_pack.hpp.
//   net_pack_check          the five cases
//   net_pack_check --time   median of five timings of net_pack for 18 channels, in milliseconds
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "../../clair3_rna_amd/csrc/net_pack.hpp"
using namespace c3r;

static uint64_t rng_state;
static uint64_t rng() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static float uniform(float a) { return a * (float)((double)(rng() >> 11) * (2.0 / 9007199254740992.0) - 1.0); }   // [-a, a)

// float count of the blob's parts: the two directions of layer 1, the two of layer 2 (kernel, recurrent kernel, bias each), then W4
static size_t n_l1(int C) { return (size_t)C * 4 * NET_H1 + (size_t)NET_H1 * 4 * NET_H1 + 4 * NET_H1; }
static size_t n_l2() { return (size_t)2 * NET_H1 * 4 * NET_H2 + (size_t)NET_H2 * 4 * NET_H2 + 4 * NET_H2; }

static std::vector<float> ordinary_blob(int C, uint64_t seed) {
    rng_state = seed;
    std::vector<float> w((size_t)net_weight_count(C));
    for (float &v : w) v = uniform(0.25f);
    return w;
}
// magnitudes 2^-24 .. 2^2 (log-uniform exponent, random mantissa and sign), every 17th value an exact zero, every 19th a power of two
static std::vector<float> wide_blob(int C, uint64_t seed) {
    rng_state = seed;
    std::vector<float> w((size_t)net_weight_count(C));
    for (size_t i = 0; i < w.size(); ++i) {
        const int e = -24 + (int)(rng() % 26);                              // 2^e <= |v| < 2^(e + 1), e = -24 .. 1
        const float m = i % 19 == 0 ? 1.0f : 1.0f + 0.5f * (uniform(1.0f) + 1.0f);
        const float v = std::ldexp(std::min(m, 1.99999988f), e);
        w[i] = i % 17 == 0 ? 0.0f : (rng() & 1 ? -v : v);
    }
    return w;
}

static uint64_t fnv1a(const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
template <class T>
static void report(const char *name, const char *buf, const std::vector<T> &v) {
    printf("%s buf %s %zu %016llx\n", name, buf, v.size() * sizeof(T), (unsigned long long)fnv1a(v.data(), v.size() * sizeof(T)));
}

static int run_case(const char *name, const std::vector<float> &blob, int C) {
    PackedNet p;
    std::string err;
    const int rc = net_pack(blob.data(), C, p, err);
    if (rc) {
        printf("%s refused %d %s\n", name, rc, err.c_str());
        return 0;
    }
    printf("%s wlog2 %d %d %d\n", name, p.wlog2[0], p.wlog2[1], p.wlog2[2]);
#define BUF(x) report(name, #x, p.x)
    BUF(w1); BUF(b1); BUF(w2); BUF(b2); BUF(w4); BUF(b4); BUF(b5); BUF(bo); BUF(w5p); BUF(wcp);
    BUF(w1h); BUF(w2h); BUF(w4f); BUF(w2w); BUF(w4w);
    BUF(w2q); BUF(w2s); BUF(w4q); BUF(w4s);
#undef BUF
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--time")) {
        const std::vector<float> blob = ordinary_blob(18, 0x9e3779b97f4a7c15ull);
        double ms[5];
        for (double &m : ms) {
            PackedNet p;
            std::string err;
            const auto t0 = std::chrono::steady_clock::now();
            if (net_pack(blob.data(), 18, p, err)) { printf("net_pack failed: %s\n", err.c_str()); return 1; }
            m = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        std::sort(ms, ms + 5);
        printf("net_pack c18 median of 5: %.1f ms (min %.1f, max %.1f)\n", ms[2], ms[0], ms[4]);
        return 0;
    }
    run_case("c18", ordinary_blob(18, 0x9e3779b97f4a7c15ull), 18);
    run_case("c30", ordinary_blob(30, 0xd1b54a32d192ed03ull), 30);
    {
        // one large value per scaled layer: 2^s |w| <= 2^15 gives s = 9 for 40, s = 6 for 300, s = 2 for 5000
        std::vector<float> blob = ordinary_blob(18, 0x2545f4914f6cdd1dull);
        const size_t l1 = n_l1(18), l2 = n_l2();
        blob[1234] = 40.0f;                                                 // a layer-1 input weight, forward direction
        blob[2 * l1 + l2 - 7] = -300.0f;                                    // a layer-2 bias, forward direction
        blob[2 * l1 + 2 * l2 + 777777] = 5000.0f;                           // an L4 weight
        run_case("c18_scales", blob, 18);
    }
    run_case("c18_wide", wide_blob(18, 0x853c49e6748fea9bull), 18);
    {
        std::vector<float> blob = ordinary_blob(18, 0x9e3779b97f4a7c15ull);
        blob[424242] = std::numeric_limits<float>::quiet_NaN();
        run_case("c18_nan", blob, 18);
    }
    return 0;
}
