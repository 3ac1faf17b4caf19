// The row-export kernels (clair3_rna_amd/csrc/export_kernels.hpp; the scan: pileup_kernels.hpp) against plain serial host code, on hand-made arrays:
//   A  k_row_keep                                  the two RefCall rules of the decoder, restated here in float32
//   B  launch_excl_scan                            (k_excl_scan, or k_scan_local + k_excl_scan + k_scan_add) against an int64 sum
//   C  k_pack_tokens, k_pack_rows, k_export_tokens a stable sort of every site's tokens by (read_idx, arrival index); k_gather_rows beside them
// Every comparison is exact.  Every device output buffer has a canary margin on both sides, read back and checked after each kernel; inputs are
// always well-formed (no offset leaves its buffer).  The first HIP error or mismatch prints the case and ends the program with status 1.
//   row_export_check              all sections on device 0; one line per section, ending in "ok"
//   row_export_check --host-only  no HIP call: the generators, the hand-derived expectations of A and A's safety property against the real decoder
//                                 (decode.hpp, vcf_row): a case the rule drops prints no row without show_ref, whatever its alt dictionary holds
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../clair3_rna_amd/csrc/pileup_kernels.hpp"
#include "../../clair3_rna_amd/csrc/export_kernels.hpp"
#include "../../clair3_rna_amd/csrc/decode.hpp"

using namespace c3r;

static std::string g_case = "start";
[[noreturn]] static void fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stdout, "FAILED [%s]: ", g_case.c_str());
    vfprintf(stdout, fmt, ap);
    fprintf(stdout, "\n");
    va_end(ap);
    fflush(stdout);
    exit(1);
}
static std::string fmt(const char *f, ...) {
    char b[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}
#define HIP(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) fail("%s: %s", #x, hipGetErrorString(e_)); } while (0)
static void sync_check() { HIP(hipGetLastError()); HIP(hipDeviceSynchronize()); }

struct Rng {
    uint64_t s;
    uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    uint32_t u32() { return (uint32_t)(next() >> 32); }
    uint32_t below(uint32_t n) { return n ? u32() % n : 0; }
    double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

// ---- a device buffer of n items between two canary margins
constexpr size_t MARGIN = 256;
constexpr unsigned char CANARY = 0xA5;
template <typename T> struct Guarded {
    char *raw = nullptr; size_t n = 0; const char *name = "";
    Guarded(size_t n_, const char *name_) : n(n_), name(name_) {
        HIP(hipMalloc((void **)&raw, bytes() + 2 * MARGIN));
        HIP(hipMemset(raw, CANARY, bytes() + 2 * MARGIN));
    }
    Guarded(const Guarded &) = delete;
    ~Guarded() { if (raw) (void)hipFree(raw); }
    size_t bytes() const { return n * sizeof(T); }
    T *p() { return (T *)(raw + MARGIN); }
    void fill(int byte) { if (n) HIP(hipMemset(raw + MARGIN, byte, bytes())); }
    void put(const std::vector<T> &h) { if (h.size() != n) fail("%s: upload of %zu items into %zu", name, h.size(), n); if (n) HIP(hipMemcpy(p(), h.data(), bytes(), hipMemcpyHostToDevice)); }
    // the contents, after the canaries on both sides were found whole
    std::vector<T> get() {
        std::vector<unsigned char> all(bytes() + 2 * MARGIN);
        HIP(hipMemcpy(all.data(), raw, all.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < MARGIN; ++i) {
            if (all[i] != CANARY) fail("%s: canary byte %zu BEFORE the buffer was overwritten", name, MARGIN - i);
            if (all[MARGIN + bytes() + i] != CANARY) fail("%s: canary byte %zu AFTER the buffer's %zu items was overwritten", name, i, n);
        }
        std::vector<T> out(n);
        if (n) memcpy(out.data(), all.data() + MARGIN, bytes());
        return out;
    }
};

// =====================================================================================================================================
// A. k_row_keep
struct KeepCase { char c; float p[C3R_NPROB]; int expect; /* what the case was built to give; -1: whatever the rule says */ };

// The rule as the decoder states it (decode.hpp call_site = clair3_rna/call_variants.py:540-542 and the first round of the arg-max), one float32
// multiply per class product; the reference class must also be a normal number (the 1e-30f guard that k_row_keep documents).  1: the site is kept.
static int keep_rule(char c, const float *p) {
    static const char from[] = "ACGTURYSWKMBDHVN", to[] = "ACGTTACCAGACAAAA";
    char a = 'A';
    if (c) { const char *q = strchr(from, c); if (q) a = to[q - from]; }
    const int rr = a == 'A' ? 0 : a == 'C' ? 4 : a == 'G' ? 7 : 9;          // gt21 of AA, CC, GG, TT
    const float *g = p, z0 = p[21], z1 = p[22], z2 = p[23];
    if (z0 >= 0.5f && g[rr] >= 0.5f) return 0;
    const float p_ref = z0 * g[rr];
    float prod[23]; int k = 0;
    static const int homo[4] = {0, 4, 7, 9}, het[6] = {1, 2, 3, 5, 6, 8};
    for (int i = 0; i < 4; ++i) prod[k++] = z1 * g[homo[i]];
    for (int i = 0; i < 6; ++i) prod[k++] = z2 * g[het[i]];
    prod[k++] = z1 * g[15]; prod[k++] = z2 * g[15];
    prod[k++] = z1 * g[10]; prod[k++] = z2 * g[10];
    for (int i = 0; i < 4; ++i) prod[k++] = g[16 + i] * z2;
    for (int i = 0; i < 4; ++i) prod[k++] = g[11 + i] * z2;
    prod[k++] = z2 * g[20];
    float top = prod[0];
    for (int i = 1; i < 23; ++i) if (prod[i] > top) top = prod[i];
    return (p_ref >= 1e-30f && p_ref >= top) ? 0 : 1;
}

static const char CENTRES[] = {'A', 'C', 'G', 'T', 'U', 'R', 'Y', 'S', 'W', 'K', 'M', 'B', 'D', 'H', 'V', 'N', 'a', 'X', '*', '\0'};
struct Slot { int z, g; };
static const Slot SLOTS[23] = {{1, 0}, {1, 4}, {1, 7}, {1, 9}, {1, 15}, {1, 10}, {2, 1}, {2, 2}, {2, 3}, {2, 5}, {2, 6}, {2, 8}, {2, 15}, {2, 10},
                               {2, 16}, {2, 17}, {2, 18}, {2, 19}, {2, 11}, {2, 12}, {2, 13}, {2, 14}, {2, 20}};
static int n_edge_cases = 0;

static std::vector<KeepCase> gen_keep_cases() {
    std::vector<KeepCase> v;
    auto blank = [](char c, int expect) { KeepCase k; k.c = c; k.expect = expect; for (float &x : k.p) x = 0.f; return k; };
    static const int homo[4] = {0, 4, 7, 9};
    static const char to[] = "ACGTTACCAGACAAAAAAAA";                          // what CENTRES map to
    // every centre: one homozygous class at 0.75 with P(0/0) = 0.75 is the early exit exactly when it is the centre's own class
    for (int ci = 0; ci < 20; ++ci)
        for (int h = 0; h < 4; ++h) {
            const int rr = to[ci] == 'A' ? 0 : to[ci] == 'C' ? 4 : to[ci] == 'G' ? 7 : 9;
            KeepCase k = blank(CENTRES[ci], homo[h] == rr ? 0 : 1);
            k.p[homo[h]] = 0.75f; k.p[21] = 0.75f; k.p[22] = 0.25f;
            for (int o = 0; o < 4; ++o) if (o != h) k.p[homo[o]] = 0.0625f;
            v.push_back(k);
        }
    // z0 and g[rr] around 0.5, independently; a competitor above P(ref) so that only the early exit can drop the site, and without one
    const float half[3] = {nextafterf(0.5f, 0.f), 0.5f, nextafterf(0.5f, 1.f)};
    for (int ci = 0; ci < 4; ++ci)
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                for (int comp = 0; comp < 2; ++comp) {
                    const int rr = homo[ci], other = homo[(ci + 1) & 3];
                    KeepCase k = blank(CENTRES[ci], comp ? ((a >= 1 && b >= 1) ? 0 : 1) : 0);
                    k.p[21] = half[a]; k.p[rr] = half[b];
                    if (comp) { k.p[22] = 0.5f; k.p[other] = 0.75f; }         // 0.375 > 0.25 + 2 ulp
                    v.push_back(k);
                }
    // each of the 23 class products one ulp below P(ref), equal to it and one ulp above it, every other product lower.  P(ref) = 0.1875 exactly
    // (0.75 * 0.25, or 0.375 * 0.5 when the competitor is the centre's own homozygous class); the competitor is (0.375 -/+ 1 ulp) * 0.5, exact.
    const float zk[3] = {nextafterf(0.375f, 0.f), 0.375f, nextafterf(0.375f, 1.f)};
    for (int ci = 0; ci < 4; ++ci)
        for (int s = 0; s < 23; ++s)
            for (int rel = 0; rel < 3; ++rel) {
                const int rr = homo[ci];
                KeepCase k = blank(CENTRES[ci], rel == 2 ? 1 : 0);
                if (SLOTS[s].z == 1 && SLOTS[s].g == rr) { k.p[21] = 0.375f; k.p[rr] = 0.5f; k.p[22] = zk[rel]; }
                else { k.p[21] = 0.75f; k.p[rr] = 0.25f; k.p[SLOTS[s].g] = 0.5f; k.p[21 + SLOTS[s].z] = zk[rel]; }
                v.push_back(k);
            }
    // P(ref) at 1e-30f and its neighbours, zero and denormal, the best competitor below it (or zero) and above it
    const float tiny[5] = {nextafterf(1e-30f, 0.f), 1e-30f, nextafterf(1e-30f, 1.f), 0.f, 1e-40f};
    for (int t = 0; t < 5; ++t)
        for (int above = 0; above < 2; ++above)
            for (int ci = 0; ci < 4; ++ci) {
                const int rr = homo[ci], other = homo[(ci + 2) & 3];
                KeepCase k = blank(CENTRES[ci], (above || tiny[t] < 1e-30f) ? 1 : 0);
                k.p[21] = tiny[t]; k.p[rr] = 1.f; k.p[other] = 1.f; k.p[22] = above ? 0.25f : tiny[t] * 0.5f;
                v.push_back(k);
            }
    n_edge_cases = (int)v.size();
    // seeded softmax vectors at three sharpnesses
    Rng r{20240607};
    const double sharp[3] = {1.0, 4.0, 16.0};
    for (int s = 0; s < 3; ++s)
        for (int i = 0; i < 34000; ++i) {
            KeepCase k = blank(r.below(4) ? CENTRES[r.below(4)] : CENTRES[r.below(20)], -1);
            // (every other vector leans towards the centre's own class and 0/0, as a model's output does: both outcomes of both rules get their share)
            const char *q = k.c ? strchr("ACGTURYSWKMBDHVN", k.c) : nullptr;
            const char a = q ? "ACGTTACCAGACAAAA"[q - "ACGTURYSWKMBDHVN"] : 'A';
            const int lean = (i & 1) ? -1 : (a == 'A' ? 0 : a == 'C' ? 4 : a == 'G' ? 7 : 9);
            auto softmax = [&](float *out, int n, int fav) {
                double l[21], m = -1e300, sum = 0;
                for (int j = 0; j < n; ++j) { l[j] = sharp[s] * (r.unit() + r.unit() + r.unit() + r.unit() - 2.0) + (j == fav ? 0.7 * sharp[s] : 0.0); m = std::max(m, l[j]); }
                for (int j = 0; j < n; ++j) { l[j] = exp(l[j] - m); sum += l[j]; }
                for (int j = 0; j < n; ++j) out[j] = (float)(l[j] / sum);
            };
            softmax(k.p, 21, lean); softmax(k.p + 21, 3, lean < 0 ? -1 : 0);
            v.push_back(k);
        }
    return v;
}

static void site_of_case(const KeepCase &k, c3r_site_t &s, int i) {
    memset(&s, 0, sizeof s);
    s.pos = 1000 + i; s.depth = 30;
    memset(s.ref33, 'A', C3R_WINDOW);
    s.ref33[C3R_FLANK] = k.c;
}

static void section_a_host(const std::vector<KeepCase> &cases, std::vector<int32_t> &flags) {
    flags.resize(cases.size());
    int kept = 0, built = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        g_case = fmt("A host, case %zu (centre 0x%02x)", i, (unsigned char)cases[i].c);
        flags[i] = keep_rule(cases[i].c, cases[i].p);
        if (cases[i].expect >= 0) { ++built; if (flags[i] != cases[i].expect) fail("the restated rule gives %d where the case was built to give %d", flags[i], cases[i].expect); }
        kept += flags[i];
    }
    // safety against the real decoder: a dropped case prints nothing without show_ref, whatever alt_info holds
    const AltDict dicts[4] = {
        {},
        {{"XC", 7}, {"XG", 3}, {"XT", 2}, {"XA", 4}, {"RA", 14}},
        {{"IAC", 5}, {"IACG", 3}, {"DC", 4}, {"DCG", 2}, {"RA", 16}},
        {{"XA", 3}, {"XC", 3}, {"XG", 3}, {"XT", 3}, {"IAT", 3}, {"IATT", 3}, {"DC", 3}, {"DCG", 3}, {"RA", 3}},
    };
    int64_t checked = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        if (flags[i]) continue;
        c3r_site_t s; site_of_case(cases[i], s, (int)i);
        for (int d = 0; d < 4; ++d) {
            g_case = fmt("A host, case %zu (centre 0x%02x), alt dictionary %d", i, (unsigned char)cases[i].c, d);
            std::string out;
            const bool printed = vcf_row("ctg", s.pos, s.ref33, s.depth, dicts[d], cases[i].p, 2, false, out);
            if (printed || !out.empty()) fail("dropped by the rule, but the decoder prints: %s", out.c_str());
            ++checked;
        }
    }
    g_case = "A host";
    if (kept == 0 || kept == (int)cases.size()) fail("the cases do not exercise both outcomes (%d kept of %zu)", kept, cases.size());
    printf("A host: %zu cases (%d built by hand to a known answer), %d kept; %lld decodes of dropped cases print nothing: ok\n", cases.size(), built, kept, (long long)checked);
}

static void section_a_gpu(const std::vector<KeepCase> &cases, const std::vector<int32_t> &flags) {
    std::vector<c3r_site_t> sites(cases.size());
    std::vector<float> probs(cases.size() * C3R_NPROB);
    for (size_t i = 0; i < cases.size(); ++i) { site_of_case(cases[i], sites[i], (int)i); memcpy(&probs[i * C3R_NPROB], cases[i].p, sizeof cases[i].p); }
    c3r_site_t *d_sites; float *d_probs;
    HIP(hipMalloc((void **)&d_sites, sites.size() * sizeof(c3r_site_t))); HIP(hipMalloc((void **)&d_probs, probs.size() * 4));
    HIP(hipMemcpy(d_sites, sites.data(), sites.size() * sizeof(c3r_site_t), hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_probs, probs.data(), probs.size() * 4, hipMemcpyHostToDevice));
    const int ns[7] = {0, 1, 255, 256, 257, 1000, (int)cases.size()};
    for (int n : ns) {
        g_case = fmt("A k_row_keep, n = %d", n);
        Guarded<int32_t> keep((size_t)n + 1, "keep");
        keep.fill(0x77);
        hipLaunchKernelGGL(k_row_keep, dim3((unsigned)(n / 256 + 1)), dim3(256), 0, 0, (const c3r_site_t *)d_sites, (const float *)d_probs, n, keep.p());
        sync_check();
        const std::vector<int32_t> got = keep.get();
        for (int i = 0; i < n; ++i)
            if (got[i] != flags[i]) {
                std::string ps;
                for (int j = 0; j < C3R_NPROB; ++j) ps += fmt(" %a", cases[i].p[j]);
                fail("case %d (centre 0x%02x): keep = %d, the rule says %d; probabilities%s", i, (unsigned char)cases[i].c, got[i], flags[i], ps.c_str());
            }
        if (got[n] != 0) fail("keep[n] = %d, not 0", got[n]);
    }
    HIP(hipFree(d_sites)); HIP(hipFree(d_probs));
    g_case = "A";
    printf("A k_row_keep: %zu cases exact at n = 0, 1, 255, 256, 257, 1000 and all: ok\n", cases.size());
}

// =====================================================================================================================================
// B. the scan
static void scan_on_device(Guarded<int32_t> &data, int n, Guarded<int32_t> &total, Guarded<int32_t> &tops) {
    if ((size_t)n > data.n || (size_t)excl_scan_tops(n) > tops.n) fail("scan buffers too small");
    launch_excl_scan(0, data.p(), n, total.p(), tops.p());
    sync_check();
}
// data[0 .. n) scanned on the device against the serial sum of `in`; returns the total
static int32_t scan_and_check(const std::vector<int32_t> &in) {
    const int n = (int)in.size();
    Guarded<int32_t> data((size_t)n, "scan data"), total(1, "scan total"), tops((size_t)std::max(1, excl_scan_tops(n)), "scan block sums");
    data.put(in); total.fill(0x5A);
    scan_on_device(data, n, total, tops);
    const std::vector<int32_t> got = data.get(), tot = total.get();
    (void)tops.get();
    int64_t run = 0;
    for (int i = 0; i < n; ++i) {
        if ((int64_t)got[i] != run) fail("element %d of %d is %d, the serial sum says %lld", i, n, got[i], (long long)run);
        run += in[i];
    }
    if (run >= (1ll << 31)) fail("test input sums to %lld", (long long)run);
    if ((int64_t)tot[0] != run) fail("total of %d items is %d, the serial sum says %lld", n, tot[0], (long long)run);
    return tot[0];
}
static void section_b() {
    const int lens[17] = {1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 32767, 32768, 32769, 40961, 65537, 300001};
    Rng r{77};
    int runs = 0;
    for (int n : lens) {
        std::vector<int32_t> v((size_t)n);
        g_case = fmt("B scan, n = %d, all zero", n); std::fill(v.begin(), v.end(), 0); scan_and_check(v); ++runs;
        g_case = fmt("B scan, n = %d, all one", n); std::fill(v.begin(), v.end(), 1); scan_and_check(v); ++runs;
        g_case = fmt("B scan, n = %d, 0/1 flags", n); for (auto &x : v) x = (int32_t)r.below(2); scan_and_check(v); ++runs;
        g_case = fmt("B scan, n = %d, sparse 0/1 flags", n); for (auto &x : v) x = r.below(33) == 0; scan_and_check(v); ++runs;
        g_case = fmt("B scan, n = %d, token counts", n);           // mostly 0 .. 5, one item in a thousand up to 40000 (at most 301 of them: below 2^31)
        for (auto &x : v) x = (int32_t)r.below(6);
        for (int k = 0; k < n / 1000 + 1; ++k) v[r.below((uint32_t)n)] = (int32_t)(r.below(40000) + 1);
        v[(size_t)n - 1] = 40000;
        scan_and_check(v); ++runs;
        const int at[8] = {0, n - 1, SCAN_BLK - 1, SCAN_BLK, 4 * SCAN_BLK - 1, 4 * SCAN_BLK, 511, 512};
        for (int k = 0; k < 8; ++k) {
            if (at[k] < 0 || at[k] >= n || (k >= 1 && at[k] == 0) || (k >= 2 && at[k] == n - 1)) continue;
            g_case = fmt("B scan, n = %d, a single item at %d", n, at[k]);
            std::fill(v.begin(), v.end(), 0); v[(size_t)at[k]] = 12345; scan_and_check(v); ++runs;
        }
    }
    g_case = "B";
    printf("B scan: %d inputs at 17 lengths on both routes, every element, the total and the canaries: ok\n", runs);
}

// =====================================================================================================================================
// C. the packers and the exporter
enum { IND_NONE = 0, IND_ALL, IND_ALT, IND_RANDOM };
struct Layout {
    std::vector<c3r_site_t> sites;
    std::vector<c3r_token_t> tok;                    // the whole slot space, gaps filled with tokens that belong to nobody
    std::vector<float> probs;
    std::vector<std::vector<int>> order;             // per site: arrival indices in reference order (read_idx, then arrival)
    std::vector<int> n_ind;                          // per site: tokens with an indel
};
static uint8_t tok_byte(const c3r_token_t &t) { return (uint8_t)((t.base & 31) | (t.rev ? 0x20 : 0) | (t.indel != 0 ? 0x80 : 0)); }
static bool rec_is(const TokRec &q, const c3r_token_t &t) { return q.read_idx == t.read_idx && q.indel == t.indel && q.qpos == t.qpos && q.del_after == (uint32_t)t.del_after; }

static Layout make_layout(const std::vector<int> &ntok, int indel_mode, uint64_t seed) {
    Rng r{seed};
    Layout L;
    const size_t n = ntok.size();
    L.sites.resize(n); L.probs.resize(n * C3R_NPROB); L.order.resize(n); L.n_ind.assign(n, 0);
    for (auto &x : L.probs) x = (float)r.unit();
    static const uint8_t bases[8] = {1, 2, 4, 8, 16, 17, 15, 1};
    auto token = [&](uint32_t read, int indel_on) {
        c3r_token_t t;
        t.read_idx = read; t.qpos = r.u32(); t.base = bases[r.below(8)]; t.rev = (uint8_t)r.below(2); t.del_after = 0;
        t.indel = indel_on ? (r.below(2) ? (int32_t)(r.below(50) + 1) : -(int32_t)(r.below(50) + 1)) : 0;
        if (t.indel > 0 && r.below(2)) t.del_after = (uint16_t)(r.below(65535) + 1);
        return t;
    };
    // the slots: sites in a shuffled order, gaps of 0 .. 3 slots between them
    std::vector<uint32_t> perm(n);
    for (size_t i = 0; i < n; ++i) perm[i] = (uint32_t)i;
    for (size_t i = n; i > 1; --i) std::swap(perm[i - 1], perm[r.below((uint32_t)i)]);
    uint32_t cursor = r.below(4);
    for (size_t k = 0; k < n; ++k) { const uint32_t s = perm[k]; L.sites[s].tok_off = cursor; cursor += (uint32_t)ntok[s] + r.below(4); }
    L.tok.resize((size_t)cursor + 4);
    for (auto &t : L.tok) t = token(r.below(16), 1);
    for (size_t s = 0; s < n; ++s) {
        c3r_site_t &S = L.sites[s];
        S.pos = (int32_t)(r.below(1u << 30) + 1); S.depth = (int32_t)r.below(9000); S.n_tok = ntok[s];
        for (int j = 0; j < C3R_WINDOW; ++j) S.ref33[j] = "ACGTN"[r.below(5)];
        S.ref33[33] = S.ref33[34] = S.ref33[35] = 0;
        // read indices over the whole range (a quarter above 2^31, a quarter small), one in eight a copy of an earlier token's; arrival order random
        c3r_token_t *T = L.tok.data() + S.tok_off;
        for (int i = 0; i < ntok[s]; ++i) {
            uint32_t read;
            const uint32_t kind = r.below(8);
            if (kind == 0 && i > 0) read = T[r.below((uint32_t)i)].read_idx;
            else if (kind <= 2) read = 0x80000000u + r.below(0x7fffffffu);
            else if (kind <= 4) read = r.below(5000);
            else if (kind == 5) read = r.below(2) ? 0xfffffffeu : 0u;
            else read = r.u32() % 0xffffffffu;
            const int on = indel_mode == IND_ALL ? 1 : indel_mode == IND_ALT ? (i & 1) : indel_mode == IND_RANDOM ? (int)(r.below(3) == 0) : 0;
            T[i] = token(read, on);
            L.n_ind[s] += T[i].indel != 0;
        }
        std::vector<int> &o = L.order[s];
        o.resize((size_t)ntok[s]);
        for (int i = 0; i < ntok[s]; ++i) o[(size_t)i] = i;
        std::stable_sort(o.begin(), o.end(), [T](int a, int b) { return T[a].read_idx < T[b].read_idx; });
    }
    return L;
}
// the reference order is a permutation that is sorted by (read_idx, arrival): a property of the generator and the sort, checked without a GPU
static void check_layout(const Layout &L) {
    for (size_t s = 0; s < L.sites.size(); ++s) {
        const c3r_token_t *T = L.tok.data() + L.sites[s].tok_off;
        const std::vector<int> &o = L.order[s];
        std::vector<char> seen(o.size(), 0);
        if (L.sites[s].tok_off + (size_t)L.sites[s].n_tok > L.tok.size()) fail("site %zu leaves the slot space", s);
        for (size_t k = 0; k < o.size(); ++k) {
            if (seen[(size_t)o[k]]++) fail("site %zu: the reference order is no permutation", s);
            if (k && !(T[o[k - 1]].read_idx < T[o[k]].read_idx || (T[o[k - 1]].read_idx == T[o[k]].read_idx && o[k - 1] < o[k]))) fail("site %zu: the reference order is not sorted", s);
        }
    }
}
// do the ranges (start, length > 0) tile [0, total) ?
static void check_partition(std::vector<std::pair<uint64_t, uint64_t>> ranges, uint64_t total, const char *what) {
    std::sort(ranges.begin(), ranges.end());
    uint64_t at = 0;
    for (auto &x : ranges) { if (x.first != at) fail("%s: a range starts at %llu where %llu is the next free place", what, (unsigned long long)x.first, (unsigned long long)at); at += x.second; }
    if (at != total) fail("%s: the ranges end at %llu, the counter says %llu", what, (unsigned long long)at, (unsigned long long)total);
}

struct DevLayout {
    Guarded<c3r_site_t> sites; Guarded<c3r_token_t> tok; Guarded<float> probs;
    explicit DevLayout(const Layout &L) : sites(L.sites.size(), "sites"), tok(L.tok.size(), "token slots"), probs(L.probs.size(), "probabilities") {
        sites.put(L.sites); tok.put(L.tok); probs.put(L.probs);
    }
};

static void check_pack_tokens(const Layout &L, DevLayout &D) {
    const size_t n = L.sites.size();
    int64_t total_ind = 0;
    for (int x : L.n_ind) total_ind += x;
    Guarded<uint8_t> bytes(L.tok.size(), "token bytes");
    Guarded<TokRec> recs((size_t)std::max<int64_t>(1, total_ind), "indel records");
    Guarded<uint32_t> rec_off(n, "rec_off");
    Guarded<unsigned long long> counter(2, "counters");
    bytes.fill(0xEE); recs.fill(0xEE); rec_off.fill(0xEE);
    HIP(hipMemset(counter.p(), 0, 16));
    hipLaunchKernelGGL(k_pack_tokens, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, 0, (const c3r_site_t *)D.sites.p(), (const c3r_token_t *)D.tok.p(), (int64_t)n, bytes.p(), recs.p(),
                       rec_off.p(), counter.p());
    sync_check();
    const std::vector<uint8_t> gb = bytes.get();
    const std::vector<TokRec> gr = recs.get();
    const std::vector<uint32_t> go = rec_off.get();
    const std::vector<unsigned long long> gc = counter.get();
    (void)D.sites.get(); (void)D.tok.get();
    if ((int64_t)gc[0] != total_ind || gc[1] != 0) fail("counters %llu, %llu; the tokens with an indel are %lld", gc[0], gc[1], (long long)total_ind);
    std::vector<uint8_t> eb(L.tok.size(), 0xEE);
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    for (size_t s = 0; s < n; ++s) {
        const c3r_token_t *T = L.tok.data() + L.sites[s].tok_off;
        if (L.n_ind[s] == 0) { if (go[s] != 0) fail("site %zu has no indel, rec_off = %u", s, go[s]); }
        else {
            if ((uint64_t)go[s] + (uint64_t)L.n_ind[s] > (uint64_t)total_ind) fail("site %zu: rec_off %u + %d records leave the %lld handed out", s, go[s], L.n_ind[s], (long long)total_ind);
            ranges.push_back({go[s], (uint64_t)L.n_ind[s]});
        }
        int ri = 0;
        for (size_t k = 0; k < L.order[s].size(); ++k) {
            const c3r_token_t &t = T[L.order[s][k]];
            eb[L.sites[s].tok_off + k] = tok_byte(t);
            if (t.indel != 0) {
                if (!rec_is(gr[go[s] + (size_t)ri], t)) fail("site %zu (%d tokens): indel record %d is not that of the token at rank %zu (arrival %d, read %u)", s, L.sites[s].n_tok, ri, k, L.order[s][k], t.read_idx);
                ++ri;
            }
        }
    }
    for (size_t i = 0; i < eb.size(); ++i)
        if (gb[i] != eb[i]) {
            size_t s = 0;
            for (size_t q = 0; q < n; ++q) if (i >= L.sites[q].tok_off && i < L.sites[q].tok_off + (size_t)L.sites[q].n_tok) s = q + 1;
            fail("token byte %zu is 0x%02x, expected 0x%02x (%s %zu, %d tokens)", i, gb[i], eb[i], s ? "rank in site" : "a slot between sites", s ? i - L.sites[s - 1].tok_off : 0, s ? L.sites[s - 1].n_tok : 0);
        }
    check_partition(ranges, gc[0], "k_pack_tokens indel records");
}

static void check_pack_rows(const Layout &L, DevLayout &D, const std::vector<int32_t> &flags) {
    const size_t n = L.sites.size();
    // flags -> row numbers, through the scan of B (checked against the serial sum there as well)
    std::vector<int32_t> fl(flags); fl.push_back(0);
    Guarded<int32_t> idx(n + 1, "keep"), total(1, "n_keep"), tops((size_t)std::max(1, excl_scan_tops((int)n + 1)), "scan block sums");
    idx.put(fl); total.fill(0x5A);
    scan_on_device(idx, (int)n + 1, total, tops);
    const std::vector<int32_t> gi = idx.get(), gt = total.get();
    (void)tops.get();
    std::vector<int> kept;
    int64_t n_bytes = 0, n_ind = 0;
    for (size_t s = 0; s < n; ++s) {
        if (gi[s] != (int32_t)kept.size()) fail("scan of the keep flags: element %zu is %d, not %zu", s, gi[s], kept.size());
        if (flags[s]) { kept.push_back((int)s); n_bytes += L.sites[s].n_tok; n_ind += L.n_ind[s]; }
    }
    if (gi[n] != (int32_t)kept.size() || gt[0] != (int32_t)kept.size()) fail("scan of the keep flags: last element %d, total %d, kept %zu", gi[n], gt[0], kept.size());
    const size_t nk = kept.size();
    Guarded<c3r_site_t> sites_c(std::max<size_t>(1, nk), "compacted sites");
    Guarded<float> probs_c(std::max<size_t>(1, nk) * C3R_NPROB, "compacted probabilities");
    Guarded<uint8_t> bytes((size_t)std::max<int64_t>(1, n_bytes), "token bytes");
    Guarded<TokRec> recs((size_t)std::max<int64_t>(1, n_ind), "indel records");
    Guarded<uint32_t> rec_off(std::max<size_t>(1, nk), "rec_off");
    Guarded<unsigned long long> counter(2, "counters");
    sites_c.fill(0xEE); probs_c.fill(0xEE); bytes.fill(0xEE); recs.fill(0xEE); rec_off.fill(0xEE);
    HIP(hipMemset(counter.p(), 0, 16));
    hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, 0, (const c3r_site_t *)D.sites.p(), (const c3r_token_t *)D.tok.p(), (const float *)D.probs.p(),
                       (const int32_t *)idx.p(), (int64_t)n, sites_c.p(), probs_c.p(), bytes.p(), recs.p(), rec_off.p(), counter.p());
    sync_check();
    const std::vector<c3r_site_t> gs = sites_c.get();
    const std::vector<float> gp = probs_c.get();
    const std::vector<uint8_t> gb = bytes.get();
    const std::vector<TokRec> gr = recs.get();
    const std::vector<uint32_t> go = rec_off.get();
    const std::vector<unsigned long long> gc = counter.get();
    (void)idx.get(); (void)D.sites.get(); (void)D.tok.get(); (void)D.probs.get();
    if ((int64_t)gc[0] != n_ind || (int64_t)gc[1] != n_bytes) fail("counters %llu records, %llu bytes; the kept sites hold %lld and %lld", gc[0], gc[1], (long long)n_ind, (long long)n_bytes);
    if (nk == 0) {               // nothing kept: nothing written
        const unsigned char *a = (const unsigned char *)gs.data();
        for (size_t i = 0; i < sizeof(c3r_site_t); ++i) if (a[i] != 0xEE) fail("no site kept, yet a site record was written");
        if (gb[0] != 0xEE || go[0] != 0xEEEEEEEEu) fail("no site kept, yet bytes or rec_off were written");
        return;
    }
    std::vector<std::pair<uint64_t, uint64_t>> rr, br;
    for (size_t j = 0; j < nk; ++j) {
        const size_t s = (size_t)kept[j];
        const c3r_token_t *T = L.tok.data() + L.sites[s].tok_off;
        if (memcmp(&gs[j], &L.sites[s], 48) != 0) fail("kept site %zu (site %zu): the 12 copied words of the record differ", j, s);
        const uint64_t bb = gs[j].tok_off;
        if (bb + (uint64_t)L.sites[s].n_tok > (uint64_t)n_bytes) fail("kept site %zu (site %zu): byte base %llu + %d tokens leave the %lld bytes", j, s, (unsigned long long)bb, L.sites[s].n_tok, (long long)n_bytes);
        if (L.sites[s].n_tok) br.push_back({bb, (uint64_t)L.sites[s].n_tok});
        if (memcmp(&gp[j * C3R_NPROB], &L.probs[s * C3R_NPROB], C3R_NPROB * 4) != 0) fail("kept site %zu (site %zu): probabilities differ", j, s);
        if (L.n_ind[s] == 0) { if (go[j] != 0) fail("kept site %zu (site %zu) has no indel, rec_off = %u", j, s, go[j]); }
        else {
            if ((uint64_t)go[j] + (uint64_t)L.n_ind[s] > (uint64_t)n_ind) fail("kept site %zu (site %zu): rec_off %u + %d records leave the %lld", j, s, go[j], L.n_ind[s], (long long)n_ind);
            rr.push_back({go[j], (uint64_t)L.n_ind[s]});
        }
        int ri = 0;
        for (size_t k = 0; k < L.order[s].size(); ++k) {
            const c3r_token_t &t = T[L.order[s][k]];
            if (gb[bb + k] != tok_byte(t)) fail("kept site %zu (site %zu, %d tokens): byte at rank %zu is 0x%02x, expected 0x%02x (arrival %d, read %u)", j, s, L.sites[s].n_tok, k, gb[bb + k], tok_byte(t), L.order[s][k], t.read_idx);
            if (t.indel != 0) {
                if (!rec_is(gr[go[j] + (size_t)ri], t)) fail("kept site %zu (site %zu, %d tokens): indel record %d is not that of the token at rank %zu (arrival %d, read %u)", j, s, L.sites[s].n_tok, ri, k, L.order[s][k], t.read_idx);
                ++ri;
            }
        }
    }
    check_partition(br, gc[1], "k_pack_rows token bytes");
    check_partition(rr, gc[0], "k_pack_rows indel records");
}

static void check_export_tokens(const Layout &L, DevLayout &D) {
    const size_t n = L.sites.size();
    std::vector<int32_t> nt(n + 1, 0);
    int64_t total = 0;
    for (size_t s = 0; s < n; ++s) { nt[s] = L.sites[s].n_tok; total += nt[s]; }
    Guarded<int32_t> off(n + 1, "export offsets"), tot(1, "export total"), tops((size_t)std::max(1, excl_scan_tops((int)n + 1)), "scan block sums");
    off.put(nt); tot.fill(0x5A);
    scan_on_device(off, (int)n + 1, tot, tops);
    const std::vector<int32_t> go = off.get(), gt = tot.get();
    (void)tops.get();
    if (gt[0] != (int32_t)total) fail("scan of n_tok: total %d, not %lld", gt[0], (long long)total);
    Guarded<c3r_token_t> out((size_t)std::max<int64_t>(1, total), "exported tokens");
    out.fill(0xEE);
    hipLaunchKernelGGL(k_export_tokens, dim3((unsigned)std::min<int64_t>(((int64_t)n + 3) / 4, 8192)), dim3(256), 0, 0, (const c3r_site_t *)D.sites.p(), (const int32_t *)off.p(), (int)n,
                       (const c3r_token_t *)D.tok.p(), out.p());
    sync_check();
    const std::vector<c3r_token_t> g = out.get();
    (void)off.get(); (void)D.sites.get(); (void)D.tok.get();
    int64_t at = 0;
    for (size_t s = 0; s < n; ++s) {
        if (go[s] != (int32_t)at) fail("scan of n_tok: element %zu is %d, not %lld", s, go[s], (long long)at);
        const c3r_token_t *T = L.tok.data() + L.sites[s].tok_off;
        for (size_t k = 0; k < L.order[s].size(); ++k)
            if (memcmp(&g[(size_t)at + k], &T[L.order[s][k]], sizeof(c3r_token_t)) != 0)
                fail("site %zu (%d tokens): exported token %zu is not arrival %d (read %u); got read %u", s, L.sites[s].n_tok, k, L.order[s][k], T[L.order[s][k]].read_idx, g[(size_t)at + k].read_idx);
        at += L.sites[s].n_tok;
    }
}

static void check_gather_rows(int n, int row_ints) {
    Rng r{4242};
    std::vector<int32_t> src32((size_t)n * row_ints), idx((size_t)n);
    std::vector<int16_t> src16((size_t)n * row_ints);
    for (auto &x : src32) x = (int32_t)r.u32();
    for (auto &x : src16) x = (int16_t)r.u32();
    for (auto &x : idx) x = (int32_t)r.below((uint32_t)n);
    Guarded<int32_t> d32(src32.size(), "gather source"), didx(idx.size(), "gather index");
    Guarded<int16_t> d16(src16.size(), "gather source, 16 bit");
    d32.put(src32); d16.put(src16); didx.put(idx);
    for (int x16 = 0; x16 < 2; ++x16)
        for (int with_idx = 0; with_idx < 2; ++with_idx) {
            g_case = fmt("C k_gather_rows, %d rows of %d ints, x16 = %d, idx %s", n, row_ints, x16, with_idx ? "given" : "null");
            Guarded<int32_t> dst((size_t)n * row_ints, "gathered rows");
            dst.fill(0xEE);
            hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)std::min<int64_t>(((int64_t)n + 3) / 4, 8192)), dim3(256), 0, 0, x16 ? (const void *)d16.p() : (const void *)d32.p(),
                               with_idx ? (const int32_t *)didx.p() : (const int32_t *)nullptr, n, row_ints, dst.p(), x16);
            sync_check();
            const std::vector<int32_t> g = dst.get();
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < row_ints; ++k) {
                    const size_t row = with_idx ? (size_t)idx[(size_t)i] : (size_t)i;
                    const int32_t e = x16 ? (int32_t)src16[row * row_ints + k] : src32[row * row_ints + k];
                    if (g[(size_t)i * row_ints + k] != e) fail("row %d, int %d: %d, expected %d", i, k, g[(size_t)i * row_ints + k], e);
                }
        }
}

static const char *IND_NAME[4] = {"no indels", "all indels", "alternating indels", "random indels"};
static std::vector<int> deep_counts() {           // the token counts the issue names, then small ones: 23 sites, not a multiple of 4
    std::vector<int> v = {0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097};
    Rng r{5};
    while (v.size() < 23) v.push_back((int)r.below(7));
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[r.below((uint32_t)i)]);
    return v;
}
static std::vector<int> many_counts() {           // more than 32768 sites (k_export_tokens' second grid-stride trip, the scan's three launches), not a multiple of 4
    std::vector<int> v(33003);
    Rng r{6};
    for (auto &x : v) x = r.below(200) == 0 ? (int)(60 + r.below(12)) : (int)r.below(6);
    return v;
}
static void section_c_host() {
    g_case = "C host";
    for (int m = 0; m < 4; ++m) check_layout(make_layout(deep_counts(), m, 100 + (uint64_t)m));
    check_layout(make_layout(many_counts(), IND_RANDOM, 200));
}
static void section_c() {
    int packs = 0;
    auto keep_patterns = [&](const Layout &L, DevLayout &D, const char *what) {
        const size_t n = L.sites.size();
        Rng r{9};
        static const char *names[6] = {"none kept", "all kept", "alternating", "only the first", "only the last", "3 % at random"};
        for (int pat = 0; pat < 6; ++pat) {
            std::vector<int32_t> f(n);
            for (size_t s = 0; s < n; ++s) f[s] = pat == 0 ? 0 : pat == 1 ? 1 : pat == 2 ? (int)(s & 1) : pat == 3 ? s == 0 : pat == 4 ? s == n - 1 : r.below(100) < 3;
            g_case = fmt("C k_pack_rows, %s, %s", what, names[pat]);
            check_pack_rows(L, D, f); ++packs;
        }
    };
    for (int m = 0; m < 4; ++m) {
        const Layout L = make_layout(deep_counts(), m, 100 + (uint64_t)m);
        check_layout(L);
        DevLayout D(L);
        const std::string what = fmt("23 sites of 0 .. 4097 tokens, %s", IND_NAME[m]);
        g_case = "C k_pack_tokens, " + what; check_pack_tokens(L, D);
        g_case = "C k_export_tokens, " + what; check_export_tokens(L, D);
        keep_patterns(L, D, what.c_str());
        if (m == IND_RANDOM) {     // the deepest site kept together with its neighbours in a pattern of its own
            std::vector<int32_t> f(L.sites.size());
            for (size_t s = 0; s < f.size(); ++s) f[s] = L.sites[s].n_tok >= 63;
            g_case = "C k_pack_rows, " + what + ", the sites of 63 tokens and more";
            check_pack_rows(L, D, f); ++packs;
        }
    }
    {
        const Layout L = make_layout(many_counts(), IND_RANDOM, 200);
        check_layout(L);
        DevLayout D(L);
        const std::string what = "33003 small sites, random indels";
        g_case = "C k_pack_tokens, " + what; check_pack_tokens(L, D);
        g_case = "C k_export_tokens, " + what; check_export_tokens(L, D);
        keep_patterns(L, D, what.c_str());
    }
    check_gather_rows(33003, 5);
    g_case = "C";
    printf("C pack and export: k_pack_tokens and k_export_tokens on 5 layouts, k_pack_rows on %d keep patterns, k_gather_rows 4 ways at 33003 rows: ok\n", packs);
}

int main(int argc, char **argv) {
    const bool host_only = argc > 1 && !strcmp(argv[1], "--host-only");
    if (argc > 1 && !host_only) { fprintf(stderr, "usage: %s [--host-only]\n", argv[0]); return 2; }
    const std::vector<KeepCase> cases = gen_keep_cases();
    std::vector<int32_t> flags;
    section_a_host(cases, flags);
    section_c_host();
    if (host_only) { printf("host-only: the reference orders of C are sorted permutations: ok\n"); return 0; }
    HIP(hipSetDevice(0));
    section_a_gpu(cases, flags);
    section_b();
    section_c();
    return 0;
}
