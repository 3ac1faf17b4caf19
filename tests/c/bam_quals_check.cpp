// bam_quals_check.cpp — c3r_bam_want_quals / c3r_bam_copy_quals (include/c3r_io.h) through the C ABI alone, from a program with its own
// main: it writes a BAM whose records have l_seq 0, 1, 2, 15, 16, 17 and 33, one record without qualities (0xff throughout), a CG:B,I
// long-CIGAR record, a placed record without CIGAR (skipped by the fetch) and a record of another contig, fetches it with and without an
// index, on one thread and on several, and holds the layout against the bytes it wrote: the quality of base j of read i is byte
// 2 * seq_off_i + j, the byte behind a read of odd length is 0xff.  Linked with csrc/bamio.cpp and csrc/vcfio.cpp; built plainly by
// tests/test_hap_min_bq_ref.py, and with -fsanitize=address,undefined by hand.
//
//   bam_quals_check <scratch directory>      prints "bam_quals_check: ok" and exits 0; every file it wrote is removed
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/c3r.h"
#include "../../include/c3r_io.h"

typedef std::vector<uint8_t> Bytes;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "bam_quals_check: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

static void p16(Bytes &v, uint32_t x) { v.push_back((uint8_t)x); v.push_back((uint8_t)(x >> 8)); }
static void p32(Bytes &v, uint32_t x) { p16(v, x & 0xffff); p16(v, x >> 16); }
static uint32_t op(uint32_t len, uint32_t o) { return (len << 4) | o; }

static uint8_t qual_of(int k, uint32_t i) { return (uint8_t)((i * 7 + (uint32_t)k * 3) % 94); }

// one alignment with its block_size in front; no_qual: the QUAL column is 0xff throughout
static Bytes rec(int32_t tid, int32_t pos, const std::vector<uint32_t> &cig, uint32_t l_seq, const Bytes &aux, int k, bool no_qual) {
    Bytes b;
    char name[16];
    const int ln = snprintf(name, sizeof name, "r%d", k) + 1;
    p32(b, (uint32_t)tid); p32(b, (uint32_t)pos);
    b.push_back((uint8_t)ln); b.push_back(60); p16(b, 4680); p16(b, (uint32_t)cig.size()); p16(b, 0); p32(b, l_seq);
    p32(b, 0xffffffffu); p32(b, 0xffffffffu); p32(b, 0);
    b.insert(b.end(), name, name + ln);
    for (uint32_t c : cig) p32(b, c);
    for (uint32_t i = 0; i < (l_seq + 1) / 2; ++i) b.push_back((uint8_t)(0x12 + 0x11 * ((i + (uint32_t)k) % 3)));
    for (uint32_t i = 0; i < l_seq; ++i) b.push_back(no_qual ? 0xff : qual_of(k, i));
    b.insert(b.end(), aux.begin(), aux.end());
    Bytes out;
    p32(out, (uint32_t)b.size());
    out.insert(out.end(), b.begin(), b.end());
    return out;
}

static void write_bgzf(const std::string &path, const Bytes &data, size_t block) {
    FILE *f = fopen(path.c_str(), "wb");
    CHECK(f);
    for (size_t o = 0; o < data.size(); o += block) {
        const size_t n = std::min<size_t>(block, data.size() - o);
        z_stream zs; memset(&zs, 0, sizeof zs);
        CHECK(deflateInit2(&zs, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK);
        Bytes body(deflateBound(&zs, (uLong)n) + 16);
        zs.next_in = const_cast<Bytef *>(data.data() + o); zs.avail_in = (uInt)n;
        zs.next_out = body.data(); zs.avail_out = (uInt)body.size();
        CHECK(deflate(&zs, Z_FINISH) == Z_STREAM_END);
        const size_t clen = body.size() - zs.avail_out;
        deflateEnd(&zs);
        Bytes h = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        p16(h, (uint32_t)(clen + 25));
        h.insert(h.end(), body.begin(), body.begin() + (long)clen);
        p32(h, (uint32_t)crc32(crc32(0L, Z_NULL, 0), data.data() + o, (uInt)n)); p32(h, (uint32_t)n);
        CHECK(fwrite(h.data(), 1, h.size(), f) == h.size());
    }
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(fwrite(eof, 1, 28, f) == 28);
    CHECK(fclose(f) == 0);
}

struct Want { uint32_t l_seq; int k; bool no_qual; };

// one fetch of chr1 held against what was written
static void check_fetch(c3r_bam *b, const std::vector<Want> &want, int64_t beg0, int64_t end0, size_t first) {
    int64_t n = 0, nc = 0, ns = 0;
    CHECK(c3r_bam_fetch(b, "chr1", beg0, end0, &n, &nc, &ns) == C3R_OK);
    CHECK((size_t)n == want.size() - first);
    std::vector<c3r_read_t> reads((size_t)n + 1);
    std::vector<uint32_t> cig((size_t)nc + 1);
    Bytes seq((size_t)ns + 1), qual(2 * (size_t)ns + 1, 0x55);
    CHECK(c3r_bam_copy(b, reads.data(), cig.data(), seq.data()) == C3R_OK);
    CHECK(c3r_bam_copy_quals(b, qual.data()) == C3R_OK);
    CHECK(qual[2 * (size_t)ns] == 0x55);                                    // nothing behind the array is written
    Bytes seen(2 * (size_t)ns, 0);
    uint64_t off = 0;
    for (size_t i = 0; i < (size_t)n; ++i) {
        const Want &w = want[first + i];
        CHECK(reads[i].l_seq == w.l_seq && reads[i].seq_off == off);
        for (uint32_t j = 0; j < w.l_seq; ++j) {
            CHECK(qual[2 * off + j] == (w.no_qual ? 0xff : qual_of(w.k, j)));
            seen[2 * off + j] = 1;
        }
        if (w.l_seq & 1) { CHECK(qual[2 * off + w.l_seq] == 0xff); seen[2 * off + w.l_seq] = 1; }
        off += (w.l_seq + 1) / 2;
    }
    CHECK(off == (uint64_t)ns);
    for (uint8_t s : seen) CHECK(s == 1);                                   // every byte of the array belongs to a base or is a padding byte
}

int main(int argc, char **argv) {
    CHECK(argc == 2);
    const std::string dir = argv[1], path = dir + "/quals.bam", bai = path + ".bai";
    Bytes d;
    const char *text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr0\tLN:1000\n@SQ\tSN:chr1\tLN:200000\n";
    d.insert(d.end(), {'B', 'A', 'M', 1});
    p32(d, (uint32_t)strlen(text)); d.insert(d.end(), text, text + strlen(text));
    p32(d, 2);
    p32(d, 5); d.insert(d.end(), {'c', 'h', 'r', '0', 0}); p32(d, 1000);
    p32(d, 5); d.insert(d.end(), {'c', 'h', 'r', '1', 0}); p32(d, 200000);
    std::vector<Want> want;
    int k = 0;
    auto add = [&](int32_t tid, int32_t pos, const std::vector<uint32_t> &cig, uint32_t l_seq, const Bytes &aux, bool no_qual, bool kept) {
        const Bytes r = rec(tid, pos, cig, l_seq, aux, k, no_qual);
        d.insert(d.end(), r.begin(), r.end());
        if (kept) want.push_back(Want{l_seq, k, no_qual});
        ++k;
    };
    add(0, 5, {op(9, 0)}, 9, {}, false, false);                             // another contig
    add(1, 10, {op(3, 2)}, 0, {}, false, true);                             // l_seq 0 (a deletion only)
    const uint32_t lens[] = {1, 2, 15, 16, 17, 33};
    for (uint32_t L : lens) add(1, 20 + (int32_t)L, {op(L, 0)}, L, {}, false, true);
    add(1, 60, {op(7, 0)}, 7, {}, true, true);                              // no qualities
    add(1, 61, {}, 5, {}, false, false);                                    // no CIGAR: the fetch skips it
    {                                                                       // the real CIGAR in CG:B,I behind the placeholder 21S9N
        Bytes aux = {'C', 'G', 'B', 'I'};
        p32(aux, 3); p32(aux, op(10, 0)); p32(aux, op(1, 1)); p32(aux, op(10, 0));
        add(1, 70, {op(21, 4), op(21, 3)}, 21, aux, false, true);
    }
    const size_t first_far = want.size();
    for (int i = 0; i < 3000; ++i) add(1, 100000 + i, {op(31, 0)}, 31, {}, (i % 97) == 0, true);    // enough records for the threaded parse
    write_bgzf(path, d, 0x4000);

    c3r_bam *b = nullptr;
    for (int indexed = 0; indexed < 2; ++indexed) {
        for (int threads = 1; threads <= 4; threads += 3) {
            if (indexed) CHECK(c3r_bam_index_build(path.c_str(), bai.c_str()) == C3R_OK);
            CHECK(c3r_bam_open(path.c_str(), threads, &b) == C3R_OK);
            CHECK(c3r_bam_has_index(b) == indexed);
            int64_t n = 0, nc = 0, ns = 0;
            // off by default: the fetch collects nothing, and the copy is refused with a message
            CHECK(c3r_bam_fetch(b, "chr1", 0, 0, &n, &nc, &ns) == C3R_OK && (size_t)n == want.size());
            uint8_t one = 0;
            CHECK(c3r_bam_copy_quals(b, &one) == C3R_EINVAL && strstr(c3r_bam_last_error(b), "c3r_bam_want_quals"));
            CHECK(c3r_bam_want_quals(b, 1) == C3R_OK);
            CHECK(c3r_bam_copy_quals(b, &one) == C3R_EINVAL);               // (still the fetch from before)
            setenv("C3R_IO_PARSE_MIN", "64", 1);                            // threads on a small file
            setenv("C3R_IO_PAR_MIN", "1", 1);
            check_fetch(b, want, 0, 0, 0);
            check_fetch(b, want, 100000, 0, first_far);                      // a region: only the far records
            check_fetch(b, want, 0, 0, 0);                                   // and the whole contig again on the same handle
            CHECK(c3r_bam_fetch(b, "chr0", 0, 0, &n, &nc, &ns) == C3R_OK && n == 1 && ns == 5);
            CHECK(c3r_bam_fetch(b, "nope", 0, 0, &n, &nc, &ns) == C3R_OK && n == 0 && ns == 0);
            CHECK(c3r_bam_copy_quals(b, nullptr) == C3R_OK);                // an empty fetch with qualities: nothing to copy
            CHECK(c3r_bam_want_quals(b, 0) == C3R_OK);
            CHECK(c3r_bam_fetch(b, "chr1", 0, 0, &n, &nc, &ns) == C3R_OK);
            CHECK(c3r_bam_copy_quals(b, &one) == C3R_EINVAL);
            CHECK(c3r_bam_want_quals(nullptr, 1) == C3R_EINVAL && c3r_bam_copy_quals(nullptr, &one) == C3R_EINVAL);
            c3r_bam_close(b);
        }
    }
    remove(path.c_str());
    remove(bai.c_str());
    printf("bam_quals_check: ok\n");
    return 0;
}
