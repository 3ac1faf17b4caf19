// realign_check.cpp — c3r_hap_realign_column through the C ABI alone: hand-derived cases of tests/test_realign_ref.py (a clean read, `1D1I`
// in the place of a substitution, a tie, the insertion-at-the-boundary convention, an N on t, the read's end, a non-ACGT reference base,
// the fallback), the refusals, and random reads without indels whose column is checked against a textbook edit distance written here.
// Host code only: no context, no device.  Built against include/c3r.h and libc3r.so:
//   c++ -std=c++17 -Wall -Iinclude tests/c/realign_check.cpp -Lclair3_rna_amd -lc3r -Wl,-rpath,<dir of libc3r.so> -o realign_check
// Prints "realign_check: ok" and exits 0, or says what differed and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "c3r.h"

static int failures = 0;
static void check(const char *name, bool ok) {
    if (!ok) { printf("realign_check: %s FAILED\n", name); failures += 1; }
}

static uint8_t code_of(char c) { return c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 4 : c == 'T' ? 8 : 15; }
static std::vector<uint8_t> pack(const std::string &s) {
    std::vector<uint8_t> out((s.size() + 1) / 2 + 1, 0);
    for (size_t k = 0; k < s.size(); ++k) out[k >> 1] |= (uint8_t)((k & 1) ? code_of(s[k]) : code_of(s[k]) << 4);
    return out;
}
static std::vector<uint32_t> cigar(const char *text) {
    std::vector<uint32_t> out;
    uint32_t n = 0;
    for (const char *p = text; *p; ++p) {
        if (*p >= '0' && *p <= '9') { n = n * 10 + (uint32_t)(*p - '0'); continue; }
        out.push_back(n << 4 | (uint32_t)(strchr("MIDNSHP=X", *p) - "MIDNSHP=X"));
        n = 0;
    }
    return out;
}
static c3r_hap_allele_t allele(char base, uint8_t kind, uint16_t len, uint32_t off) {
    c3r_hap_allele_t a;
    a.base = code_of(base); a.kind = kind; a.len = len; a.ins_off = off;
    return a;
}
static c3r_hap_site_t site(int32_t pos, c3r_hap_allele_t a, c3r_hap_allele_t b) {
    c3r_hap_site_t s;
    memset(&s, 0, sizeof s);
    s.pos = pos; s.ps = 7; s.a = a; s.b = b;
    s.base_matters = a.base != b.base;
    s.event_matters = a.kind != C3R_HAP_EV_NONE || b.kind != C3R_HAP_EV_NONE;
    return s;
}

struct Result { int rc, column, realigned; };
static Result run(const c3r_hap_site_t &s, const std::string &ref, int64_t ref_start, int32_t pos, const char *cig, const std::string &seq, int W,
                  const uint8_t *pool = nullptr) {
    const std::vector<uint32_t> c = cigar(cig);
    const std::vector<uint8_t> q = pack(seq);
    c3r_read_t r;
    memset(&r, 0, sizeof r);
    r.pos = pos; r.n_cigar = (uint32_t)c.size(); r.l_seq = (uint32_t)seq.size(); r.mapq = 60;
    Result out = {0, -1, -1};
    out.rc = c3r_hap_realign_column(&s, pool, ref_start, ref.data(), (int64_t)ref.size(), &r, c.data(), q.data(), W, &out.column, &out.realigned);
    return out;
}
static bool is(const Result &r, int column, int realigned) { return r.rc == C3R_OK && r.column == column && r.realigned == realigned; }

static int levenshtein(const std::string &a, const std::string &b) {
    std::vector<int> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); ++j) prev[j] = (int)j;
    for (size_t i = 1; i <= a.size(); ++i) {
        cur[0] = (int)i;
        for (size_t j = 1; j <= b.size(); ++j) {
            const bool same = a[i - 1] == b[j - 1] && a[i - 1] != 'N';
            cur[j] = std::min(std::min(prev[j] + 1, cur[j - 1] + 1), prev[j - 1] + (same ? 0 : 1));
        }
        prev.swap(cur);
    }
    return prev[b.size()];
}

int main() {
    //                       0         1         2
    //                       012345678901234567890123456789
    const std::string ref = "GATTACAGCTCGATCGGATCCTAGCATGCA";
    const c3r_hap_site_t snv = site(14, allele('T', C3R_HAP_EV_NONE, 0, 0), allele('C', C3R_HAP_EV_NONE, 0, 0));   // W = 3: [10, 17) = CGATCGG
    const c3r_hap_site_t del = site(14, allele('T', C3R_HAP_EV_NONE, 0, 0), allele('T', C3R_HAP_EV_DEL, 1, 0));
    const int NO = 3;

    check("clean_read", is(run(snv, ref, 1, 5, "20M", ref.substr(5, 20), 3), 0, 1));
    check("switch_off", is(run(snv, ref, 1, 5, "20M", ref.substr(5, 20), 0), 0, 0));
    // the read carries C on 13; the aligner deleted 12 and inserted behind 13
    const std::string alt = ref.substr(5, 8) + "C" + ref.substr(14, 11);
    check("1D1I_on", is(run(snv, ref, 1, 5, "7M1D1M1I11M", alt, 3), 1, 1));
    check("1D1I_off", is(run(snv, ref, 1, 5, "7M1D1M1I11M", alt, 0), 2, 0));
    // a wrong base on 14 written 1D1I behind the anchor of a deletion site: one edit from both haplotypes
    const std::string sub = ref.substr(5, 9) + "A" + ref.substr(15, 10);
    check("tie_on", is(run(del, ref, 1, 5, "9M1D1I10M", sub, 3), NO, 1));
    check("tie_off", is(run(del, ref, 1, 5, "9M1D1I10M", sub, 0), 1, 0));
    check("insertion_before_s", is(run(snv, ref, 1, 5, "5M2I15M", ref.substr(5, 5) + "TT" + ref.substr(10, 15), 3), 0, 1));
    check("insertion_before_t", is(run(snv, ref, 1, 5, "12M2I8M", ref.substr(5, 12) + "TT" + ref.substr(17, 8), 3), 0, 1));
    check("N_on_t", is(run(snv, ref, 1, 5, "12M5N3M", ref.substr(5, 12) + ref.substr(22, 3), 3), 0, 0));
    check("N_behind_t", is(run(snv, ref, 1, 5, "13M4N3M", ref.substr(5, 13) + ref.substr(22, 3), 3), 0, 1));
    check("read_ends_at_t", is(run(snv, ref, 1, 5, "12M", ref.substr(5, 12), 3), 0, 0));
    check("read_ends_behind_t", is(run(snv, ref, 1, 5, "13M", ref.substr(5, 13), 3), 0, 1));
    std::string with_n = ref;
    with_n[16] = 'N';
    check("n_in_the_reference", is(run(snv, with_n, 1, 5, "20M", ref.substr(5, 20), 3), 0, 0));
    check("slice_is_the_window", is(run(snv, "cgatcgg", 11, 5, "20M", ref.substr(5, 20), 3), 0, 1));
    check("slice_one_short", is(run(snv, "cgatcg", 11, 5, "20M", ref.substr(5, 20), 3), 0, 0));
    check("anchor_under_D", is(run(snv, ref, 1, 5, "8M1D11M", ref.substr(5, 8) + ref.substr(14, 11), 3), NO, 0));
    // an insertion allele read from the pool: T > TAA behind 13, pool = (pad) A A; the read carries it
    const uint8_t pool[2] = {0x11, 0x10};
    const c3r_hap_site_t ins = site(14, allele('T', C3R_HAP_EV_NONE, 0, 0), allele('T', C3R_HAP_EV_INS, 2, 1));
    const std::string carries = ref.substr(5, 9) + "AA" + ref.substr(14, 11);
    check("ins_at_the_anchor", is(run(ins, ref, 1, 5, "9M2I11M", carries, 3, pool), 1, 1));
    // ... written one base to the right the window CGATCAAGG is two edits from both CGATCGG and CGATAACGG
    check("ins_one_to_the_right_on", is(run(ins, ref, 1, 5, "10M2I10M", ref.substr(5, 10) + "AA" + ref.substr(15, 10), 3, pool), NO, 1));
    check("ins_one_to_the_right_off", is(run(ins, ref, 1, 5, "10M2I10M", ref.substr(5, 10) + "AA" + ref.substr(15, 10), 0, pool), 0, 0));

    // refusals
    check("overhang_17", run(snv, ref, 1, 5, "20M", ref.substr(5, 20), 17).rc == C3R_EINVAL);
    check("overhang_negative", run(snv, ref, 1, 5, "20M", ref.substr(5, 20), -1).rc == C3R_EINVAL);
    check("ref_start_0", run(snv, ref, 0, 5, "20M", ref.substr(5, 20), 3).rc == C3R_EINVAL);
    c3r_hap_site_t bad = del;
    bad.b.len = 0;
    check("deletion_without_length", run(bad, ref, 1, 5, "20M", ref.substr(5, 20), 3).rc == C3R_EINVAL);
    check("insertion_without_pool", run(ins, ref, 1, 5, "20M", ref.substr(5, 20), 3, nullptr).rc == C3R_EINVAL);
    int column = -1;
    check("null_site", c3r_hap_realign_column(nullptr, nullptr, 1, ref.data(), 30, nullptr, nullptr, nullptr, 3, &column, nullptr) == C3R_EINVAL);

    // random reads without indels over random references, every overhang: the column is the one of the smaller textbook distance
    uint64_t state = 0x9e3779b97f4a7c15ull;
    auto rnd = [&](uint32_t n) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((state >> 33) % n); };
    int n_bad = 0, n_tie = 0, n_ra = 0;
    for (int it = 0; it < 400; ++it) {
        std::string r(120, 'A'), seq;
        for (char &c : r) c = "ACGT"[rnd(4)];
        const int p0 = 40 + (int)rnd(30), W = 1 + (int)rnd(16);
        const uint16_t dlen = (uint16_t)(1 + rnd(6));
        char other = "ACGT"[rnd(4)];
        if (other == r[(size_t)p0]) other = r[(size_t)p0] == 'A' ? 'C' : 'A';
        const c3r_hap_site_t s = rnd(2) ? site(p0 + 1, allele(r[(size_t)p0], C3R_HAP_EV_NONE, 0, 0), allele(other, C3R_HAP_EV_NONE, 0, 0))
                                        : site(p0 + 1, allele(other, C3R_HAP_EV_NONE, 0, 0), allele(r[(size_t)p0], C3R_HAP_EV_DEL, dlen, 0));
        const int D = s.b.kind == C3R_HAP_EV_DEL ? dlen : 0, lo = p0 - W, hi = p0 + 1 + D + W;
        seq = r.substr(10, 100);
        for (char &c : seq) if (rnd(100) < 8) c = "ACGTN"[rnd(5)];
        const Result got = run(s, r, 1, 10, "100M", seq, W);
        const std::string win = seq.substr((size_t)(lo - 10), (size_t)(hi - lo));
        const std::string ha = r.substr((size_t)lo, (size_t)W) + (s.a.base == 1 ? "A" : s.a.base == 2 ? "C" : s.a.base == 4 ? "G" : "T") + r.substr((size_t)p0 + 1, (size_t)(D + W));
        const std::string hb = r.substr((size_t)lo, (size_t)W) + (s.b.base == 1 ? "A" : s.b.base == 2 ? "C" : s.b.base == 4 ? "G" : "T") + r.substr((size_t)(p0 + 1 + D), (size_t)W);
        const int da = levenshtein(win, ha), db = levenshtein(win, hb), want = da < db ? 0 : db < da ? 1 : 3;
        n_tie += want == 3;
        n_ra += got.realigned == 1;
        if (!is(got, want, 1)) { if (n_bad++ < 5) printf("realign_check: random case %d: got %d / %d, want %d (dA %d, dB %d)\n", it, got.column, got.realigned, want, da, db); }
    }
    check("random_cases", n_bad == 0 && n_ra == 400 && n_tie < 400);

    if (failures) return 1;
    printf("realign_check: ok\n");
    return 0;
}
