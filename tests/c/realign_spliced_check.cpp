// realign_spliced_check.cpp — c3r_hap_realign_column_spliced through the C ABI alone: hand-derived cases of tests/realignspliceref.py (an N
// on t, `1D1I` beside a junction, an N in the left flank, a micro-exon, an N in a deletion's core, the read's ends, an insertion on either
// side of an N, a D beside an N, the slice's edge), the old entry as the new one with spliced = 0, the refusals, and random reads whose
// window crosses a planted intron: the column must be the one of the smaller textbook edit distance on the reference WITHOUT the intron.
// Host code only: no context, no device.  Built against include/c3r.h and libc3r.so:
//   c++ -std=c++17 -Wall -Iinclude tests/c/realign_spliced_check.cpp -Lclair3_rna_amd -lc3r -Wl,-rpath,<dir of libc3r.so> -o realign_spliced_check
// Prints "realign_spliced_check: ok" and exits 0, or says what differed and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "c3r.h"

static int failures = 0;
static void check(const char *name, bool ok) {
    if (!ok) { printf("realign_spliced_check: %s FAILED\n", name); failures += 1; }
}

static uint8_t code_of(char c) { return c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 4 : c == 'T' ? 8 : 15; }
static std::vector<uint8_t> pack(const std::string &s) {
    std::vector<uint8_t> out((s.size() + 1) / 2 + 1, 0);
    for (size_t k = 0; k < s.size(); ++k) out[k >> 1] |= (uint8_t)((k & 1) ? code_of(s[k]) : code_of(s[k]) << 4);
    return out;
}
static std::vector<uint32_t> cigar(const std::string &text) {
    std::vector<uint32_t> out;
    uint32_t n = 0;
    for (const char *p = text.c_str(); *p; ++p) {
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
// spliced < 0: the old entry
static Result run(const c3r_hap_site_t &s, const std::string &ref, int64_t ref_start, int32_t pos, const std::string &cig, const std::string &seq, int W, int spliced) {
    const std::vector<uint32_t> c = cigar(cig);
    const std::vector<uint8_t> q = pack(seq);
    c3r_read_t r;
    memset(&r, 0, sizeof r);
    r.pos = pos; r.n_cigar = (uint32_t)c.size(); r.l_seq = (uint32_t)seq.size(); r.mapq = 60;
    Result out = {0, -1, -1};
    out.rc = spliced < 0 ? c3r_hap_realign_column(&s, nullptr, ref_start, ref.data(), (int64_t)ref.size(), &r, c.data(), q.data(), W, &out.column, &out.realigned)
                         : c3r_hap_realign_column_spliced(&s, nullptr, ref_start, ref.data(), (int64_t)ref.size(), &r, c.data(), q.data(), W, spliced, &out.column, &out.realigned);
    return out;
}
static bool is(const Result &r, int column, int realigned) { return r.rc == C3R_OK && r.column == column && r.realigned == realigned; }
static bool same(const Result &a, const Result &b) { return a.rc == b.rc && a.column == b.column && a.realigned == b.realigned; }

static int levenshtein(const std::string &a, const std::string &b) {
    std::vector<int> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); ++j) prev[j] = (int)j;
    for (size_t i = 1; i <= a.size(); ++i) {
        cur[0] = (int)i;
        for (size_t j = 1; j <= b.size(); ++j) {
            const bool eq = a[i - 1] == b[j - 1] && a[i - 1] != 'N';
            cur[j] = std::min(std::min(prev[j] + 1, cur[j - 1] + 1), prev[j - 1] + (eq ? 0 : 1));
        }
        prev.swap(cur);
    }
    return prev[b.size()];
}

int main() {
    //                       0         1         2
    //                       012345678901234567890123456789
    const std::string ref = "GATTACAGCTCGATCGGATCCTAGCATGCA";
    const c3r_hap_site_t snv = site(14, allele('T', C3R_HAP_EV_NONE, 0, 0), allele('C', C3R_HAP_EV_NONE, 0, 0));   // W = 3: CGATCGG / CGACCGG without an N
    const c3r_hap_site_t del = site(14, allele('T', C3R_HAP_EV_NONE, 0, 0), allele('T', C3R_HAP_EV_DEL, 1, 0));
    auto R = [&](size_t a, size_t b) { return ref.substr(a, b - a); };

    struct Case { const char *name; const c3r_hap_site_t *s; std::string ref; int32_t pos; const char *cig; std::string seq; int col_on, ra_on, col_plain, ra_plain, col_off; };
    const std::vector<Case> cases = {
        {"N_on_t", &snv, ref, 5, "12M5N3M", R(5, 17) + R(22, 25), 0, 1, 0, 0, 0},
        {"1D1I_beside_a_junction", &snv, ref, 5, "7M1D1M1I1M5N5M", R(5, 13) + "C" + R(14, 15) + R(20, 25), 1, 1, 2, 0, 2},
        {"N_inside_the_left_flank", &snv, ref, 2, "5M4N13M", R(2, 7) + R(11, 13) + "C" + R(14, 24), 1, 1, 1, 0, 1},
        {"two_N_ops_in_one_window", &snv, ref, 5, "10M3N2M3N5M", R(5, 15) + R(18, 20) + R(23, 28), 0, 1, 0, 0, 0},
        {"N_inside_the_core_of_a_deletion", &del, ref, 5, "9M4N8M", R(5, 14) + R(18, 26), 0, 0, 0, 0, 0},
        {"N_directly_behind_the_anchor", &snv, ref, 5, "9M4N8M", R(5, 14) + R(18, 26), 0, 1, 0, 0, 0},
        {"two_positions_before_the_anchor", &snv, ref, 4, "1M7N12M", R(4, 5) + R(12, 24), 0, 0, 0, 0, 0},
        {"three_positions_before_the_anchor", &snv, ref, 4, "2M6N12M", R(4, 6) + R(12, 24), 0, 1, 0, 0, 0},
        {"kt_behind_the_last_position", &snv, ref, 5, "9M4N3M", R(5, 14) + R(18, 21), 0, 0, 0, 0, 0},
        {"kt_on_the_last_position", &snv, ref, 5, "9M4N4M", R(5, 14) + R(18, 22), 0, 1, 0, 0, 0},
        {"insertion_before_the_N_before_x_kt", &snv, ref, 5, "12M2I5N3M", R(5, 17) + "TT" + R(22, 25), 0, 1, 0, 0, 0},
        {"insertion_behind_the_N_before_x_kt", &snv, ref, 5, "12M5N2I3M", R(5, 17) + "TT" + R(22, 25), 0, 1, 0, 0, 0},
        {"insertion_before_the_N_before_x_ks", &snv, ref, 3, "3M2I4N14M", R(3, 6) + "TT" + R(10, 24), 0, 1, 0, 1, 0},
        {"insertion_behind_the_N_before_x_ks", &snv, ref, 3, "3M4N2I14M", R(3, 6) + "TT" + R(10, 24), 0, 1, 0, 1, 0},
        {"D_before_an_N", &snv, ref, 5, "11M1D5N3M", R(5, 16) + R(22, 25), 0, 1, 0, 0, 0},
        {"D_behind_an_N", &snv, ref, 5, "12M5N1D2M", R(5, 17) + R(23, 25), 0, 1, 0, 0, 0},
        {"intron_outside_the_slice", &snv, ref.substr(0, 17), 5, "12M5N3M", R(5, 17) + R(22, 25), 0, 1, 0, 0, 0},
        {"flank_outside_the_slice", &snv, ref.substr(0, 16), 5, "12M5N3M", R(5, 17) + R(22, 25), 0, 0, 0, 0, 0},
        {"n_in_the_intron", &snv, ref.substr(0, 18) + "NN" + ref.substr(20), 5, "12M5N3M", R(5, 17) + R(22, 25), 0, 1, 0, 0, 0},
        {"no_N_at_all", &snv, ref, 5, "7M1D1M1I11M", R(5, 13) + "C" + R(14, 25), 1, 1, 1, 1, 2},
    };
    for (const Case &c : cases) {
        const Result on = run(*c.s, c.ref, 1, c.pos, c.cig, c.seq, 3, 1), plain = run(*c.s, c.ref, 1, c.pos, c.cig, c.seq, 3, 0), old = run(*c.s, c.ref, 1, c.pos, c.cig, c.seq, 3, -1);
        if (!is(on, c.col_on, c.ra_on) || !is(plain, c.col_plain, c.ra_plain) || !same(plain, old) || !is(run(*c.s, c.ref, 1, c.pos, c.cig, c.seq, 0, 1), c.col_off, 0) ||
            !is(run(*c.s, c.ref, 1, c.pos, c.cig, c.seq, 0, -1), c.col_off, 0)) {
            printf("realign_spliced_check: %s: spliced %d / %d, plain %d / %d, old entry %d / %d\n", c.name, on.column, on.realigned, plain.column, plain.realigned, old.column, old.realigned);
            check(c.name, false);
        }
    }

    // refusals: `spliced` is 0 or 1; the rest as the old entry refuses it
    check("spliced_2", run(snv, ref, 1, 5, "20M", R(5, 25), 3, 2).rc == C3R_EINVAL);
    check("spliced_negative", c3r_hap_realign_column_spliced(&snv, nullptr, 1, ref.data(), 30, nullptr, nullptr, nullptr, 3, -1, nullptr, nullptr) == C3R_EINVAL);
    check("overhang_17", run(snv, ref, 1, 5, "20M", R(5, 25), 17, 1).rc == C3R_EINVAL);
    check("ref_start_0", run(snv, ref, 0, 5, "20M", R(5, 25), 3, 1).rc == C3R_EINVAL);
    c3r_hap_site_t bad = del;
    bad.b.len = 0;
    check("deletion_without_length", run(bad, ref, 1, 5, "20M", R(5, 25), 3, 1).rc == C3R_EINVAL);
    int column = -1;
    check("null_site", c3r_hap_realign_column_spliced(nullptr, nullptr, 1, ref.data(), 30, nullptr, nullptr, nullptr, 3, 1, &column, nullptr) == C3R_EINVAL);

    // random reads over random references with one intron planted inside the window but outside the core, every overhang: the column is the
    // one of the smaller textbook distance on the reference without the intron, and the plain rule falls back
    uint64_t state = 0x9e3779b97f4a7c15ull;
    auto rnd = [&](uint32_t n) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((state >> 33) % n); };
    int n_bad = 0, n_tie = 0, n_ra = 0, n_plain_ra = 0;
    for (int it = 0; it < 400; ++it) {
        std::string r(120, 'A');
        for (char &c : r) c = "ACGT"[rnd(4)];
        const int p0 = 40 + (int)rnd(30), W = 1 + (int)rnd(16);
        const uint16_t dlen = (uint16_t)(1 + rnd(6));
        char other = "ACGT"[rnd(4)];
        if (other == r[(size_t)p0]) other = r[(size_t)p0] == 'A' ? 'C' : 'A';
        const bool is_del = rnd(2) == 0;
        const int D = is_del ? dlen : 0, lo = p0 - W, hi = p0 + 1 + D + W;
        std::string seq = r.substr(10, 100);
        for (char &c : seq) if (rnd(100) < 8) c = "ACGTN"[rnd(5)];
        // the cut: before a position of (lo, p0] or of (p0 + D, hi]: bases of the window on both of its sides, none of the core between them
        const int cut = rnd(2) ? lo + 1 + (int)rnd((uint32_t)W) : p0 + D + 1 + (int)rnd((uint32_t)W);
        const int L = 1 + (int)rnd(200);
        std::string junk((size_t)L, 'A');
        for (char &c : junk) c = "ACGTN"[rnd(5)];
        const std::string planted = r.substr(0, (size_t)cut) + junk + r.substr((size_t)cut);
        const int moved = cut <= p0 ? p0 + L : p0;
        const c3r_hap_site_t s = is_del ? site(moved + 1, allele(other, C3R_HAP_EV_NONE, 0, 0), allele(r[(size_t)p0], C3R_HAP_EV_DEL, dlen, 0))
                                        : site(moved + 1, allele(r[(size_t)p0], C3R_HAP_EV_NONE, 0, 0), allele(other, C3R_HAP_EV_NONE, 0, 0));
        const std::string cig = std::to_string(cut - 10) + "M" + std::to_string(L) + "N" + std::to_string(110 - cut) + "M";
        const Result got = run(s, planted, 1, 10, cig, seq, W, 1);
        n_plain_ra += run(s, planted, 1, 10, cig, seq, W, 0).realigned == 1;
        const std::string win = seq.substr((size_t)(lo - 10), (size_t)(hi - lo));
        const std::string letter_a(1, "?A" "C?G???T"[s.a.base]), letter_b(1, "?A" "C?G???T"[s.b.base]);
        const std::string ha = r.substr((size_t)lo, (size_t)W) + letter_a + r.substr((size_t)p0 + 1, (size_t)(D + W));
        const std::string hb = r.substr((size_t)lo, (size_t)W) + letter_b + r.substr((size_t)(p0 + 1 + D), (size_t)W);
        const int da = levenshtein(win, ha), db = levenshtein(win, hb), want = da < db ? 0 : db < da ? 1 : 3;
        n_tie += want == 3;
        n_ra += got.realigned == 1;
        if (!is(got, want, 1)) { if (n_bad++ < 5) printf("realign_spliced_check: random case %d: got %d / %d, want %d (dA %d, dB %d)\n", it, got.column, got.realigned, want, da, db); }
    }
    check("random_cases", n_bad == 0 && n_ra == 400 && n_plain_ra == 0 && n_tie < 400);

    if (failures) return 1;
    printf("realign_spliced_check: ok\n");
    return 0;
}
