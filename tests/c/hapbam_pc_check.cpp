// hapbam_pc_check.cpp — c3r_bam_write_haplotagged_pc (include/c3r_io.h) through the C ABI alone, from a program with its own main: it
// writes a BAM of eight read records (one with stale HP / PS / PC fields, one with another aux field) and a record of another contig,
// fetches the contig, writes it back with tags and PC values of all three widths, inflates the output and holds every record's aux
// bytes against what the header file says: HP, PS and then PC in the smallest unsigned type behind the fields that stay, nothing for an
// untagged read, and with pc = NULL the bytes of c3r_bam_write_haplotagged.  Linked with csrc/bamio.cpp and csrc/vcfio.cpp; built
// plainly by tests/test_hap_bq_weights_ref.py, and with -fsanitize=address,undefined by hand.
//
//   hapbam_pc_check <scratch directory>      prints "hapbam_pc_check: ok" and exits 0; every file it wrote is removed
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

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "hapbam_pc_check: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

static void p16(Bytes &v, uint32_t x) { v.push_back((uint8_t)x); v.push_back((uint8_t)(x >> 8)); }
static void p32(Bytes &v, uint32_t x) { p16(v, x & 0xffff); p16(v, x >> 16); }
static uint32_t g32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// one alignment of l_seq bases under one M op, with its block_size in front
static Bytes rec(int32_t tid, int32_t pos, uint32_t l_seq, const Bytes &aux, int k) {
    Bytes b;
    char name[16];
    const int ln = snprintf(name, sizeof name, "r%d", k) + 1;
    p32(b, (uint32_t)tid); p32(b, (uint32_t)pos);
    b.push_back((uint8_t)ln); b.push_back(60); p16(b, 4680); p16(b, 1); p16(b, 0); p32(b, l_seq);
    p32(b, 0xffffffffu); p32(b, 0xffffffffu); p32(b, 0);
    b.insert(b.end(), name, name + ln);
    p32(b, l_seq << 4);
    for (uint32_t i = 0; i < (l_seq + 1) / 2; ++i) b.push_back(0x12);
    for (uint32_t i = 0; i < l_seq; ++i) b.push_back((uint8_t)(10 + i));
    b.insert(b.end(), aux.begin(), aux.end());
    Bytes out;
    p32(out, (uint32_t)b.size());
    out.insert(out.end(), b.begin(), b.end());
    return out;
}

static void write_bgzf(const std::string &path, const Bytes &data) {
    FILE *f = fopen(path.c_str(), "wb");
    CHECK(f);
    z_stream zs; memset(&zs, 0, sizeof zs);
    CHECK(deflateInit2(&zs, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK);
    Bytes body(deflateBound(&zs, (uLong)data.size()) + 16);
    zs.next_in = const_cast<Bytef *>(data.data()); zs.avail_in = (uInt)data.size();
    zs.next_out = body.data(); zs.avail_out = (uInt)body.size();
    CHECK(deflate(&zs, Z_FINISH) == Z_STREAM_END);
    const size_t clen = body.size() - zs.avail_out;
    deflateEnd(&zs);
    Bytes h = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    p16(h, (uint32_t)(clen + 25));
    h.insert(h.end(), body.begin(), body.begin() + (long)clen);
    p32(h, (uint32_t)crc32(crc32(0L, Z_NULL, 0), data.data(), (uInt)data.size())); p32(h, (uint32_t)data.size());
    CHECK(fwrite(h.data(), 1, h.size(), f) == h.size());
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(fwrite(eof, 1, 28, f) == 28);
    CHECK(fclose(f) == 0);
}

static Bytes slurp(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    CHECK(f);
    Bytes all;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + n);
    fclose(f);
    return all;
}

// the uncompressed stream of a BGZF file
static Bytes inflate_bgzf(const Bytes &gz) {
    Bytes out;
    for (size_t o = 0; o + 18 <= gz.size();) {
        const size_t bsize = ((size_t)gz[o + 16] | (size_t)gz[o + 17] << 8) + 1;
        CHECK(o + bsize <= gz.size());
        const uint32_t isize = g32(gz.data() + o + bsize - 4);
        const size_t at = out.size();
        out.resize(at + isize);
        if (isize) {
            z_stream zs; memset(&zs, 0, sizeof zs);
            CHECK(inflateInit2(&zs, -15) == Z_OK);
            zs.next_in = const_cast<Bytef *>(gz.data() + o + 18); zs.avail_in = (uInt)(bsize - 26);
            zs.next_out = out.data() + at; zs.avail_out = isize;
            CHECK(inflate(&zs, Z_FINISH) == Z_STREAM_END);
            inflateEnd(&zs);
        }
        o += bsize;
    }
    return out;
}

// the aux bytes of every record of an uncompressed BAM stream
static std::vector<Bytes> aux_of_records(const Bytes &d) {
    CHECK(d.size() >= 12 && memcmp(d.data(), "BAM\1", 4) == 0);
    size_t p = 8 + g32(d.data() + 4);
    const uint32_t n_ref = g32(d.data() + p);
    p += 4;
    for (uint32_t i = 0; i < n_ref; ++i) p += 8 + g32(d.data() + p);
    std::vector<Bytes> out;
    while (p + 4 <= d.size()) {
        const uint32_t bs = g32(d.data() + p);
        const uint8_t *r = d.data() + p + 4;
        CHECK(p + 4 + bs <= d.size() && bs >= 32);
        const uint32_t l_seq = g32(r + 16);
        const size_t a0 = 32 + r[8] + 4 * ((size_t)r[12] | (size_t)r[13] << 8) + (l_seq + 1) / 2 + l_seq;
        CHECK(a0 <= bs);
        out.push_back(Bytes(r + a0, r + bs));
        p += 4 + bs;
    }
    CHECK(p == d.size());
    return out;
}

int main(int argc, char **argv) {
    CHECK(argc == 2);
    const std::string dir = argv[1], path = dir + "/in.bam", out_pc = dir + "/out_pc.bam", out_null = dir + "/out_null.bam", out_old = dir + "/out_old.bam";
    Bytes d;
    const char *text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr0\tLN:1000\n@SQ\tSN:chr1\tLN:200000\n";
    d.insert(d.end(), {'B', 'A', 'M', 1});
    p32(d, (uint32_t)strlen(text)); d.insert(d.end(), text, text + strlen(text));
    p32(d, 2);
    p32(d, 5); d.insert(d.end(), {'c', 'h', 'r', '0', 0}); p32(d, 1000);
    p32(d, 5); d.insert(d.end(), {'c', 'h', 'r', '1', 0}); p32(d, 200000);
    const Bytes nm = {'N', 'M', 'C', 3};
    Bytes stale = {'H', 'P', 'C', 2, 'N', 'M', 'C', 3, 'P', 'S', 'I'};
    p32(stale, 77); stale.insert(stale.end(), {'P', 'C', 'S'}); p16(stale, 999);
    const int n = 8;
    { const Bytes r = rec(0, 5, 9, {}, 100); d.insert(d.end(), r.begin(), r.end()); }
    for (int k = 0; k < n; ++k) {
        const Bytes r = rec(1, 10 + 3 * k, 5 + (uint32_t)k, k == 1 ? stale : k == 2 ? nm : Bytes(), k);
        d.insert(d.end(), r.begin(), r.end());
    }
    write_bgzf(path, d);

    c3r_bam *b = nullptr;
    CHECK(c3r_bam_open(path.c_str(), 1, &b) == C3R_OK);
    int64_t nr = 0, nc = 0, ns = 0;
    CHECK(c3r_bam_fetch(b, "chr1", 0, 0, &nr, &nc, &ns) == C3R_OK && nr == n);
    std::vector<c3r_read_t> reads((size_t)nr);
    std::vector<uint32_t> cig((size_t)nc + 1);
    Bytes seq((size_t)ns + 1);
    CHECK(c3r_bam_copy(b, reads.data(), cig.data(), seq.data()) == C3R_OK);
    //                         untagged  C          stale, S    NM, I          C edge   S edge   I edge    untagged with a pc
    const uint8_t hp[n] =     {0,        1,         2,          1,             2,       1,       2,        0};
    const int32_t ps[n] =     {-1,       5,         300,        70000,         5,       5,       5,        -1};
    const uint32_t pc[n] =    {9,        0,         256,        4000000000u,   255,     65535,   65536,    12};
    int64_t counts[4] = {0, 0, 0, 0};
    CHECK(c3r_bam_write_haplotagged_pc(b, "chr1", reads.data(), hp, ps, pc, n, out_pc.c_str(), nullptr, 1, counts) == C3R_OK);
    CHECK(counts[0] == n && counts[1] == 6 && counts[2] == 1 && counts[3] == 0);
    CHECK(c3r_bam_write_haplotagged_pc(b, "chr1", reads.data(), hp, ps, nullptr, n, out_null.c_str(), nullptr, 1, counts) == C3R_OK);
    CHECK(counts[0] == n && counts[1] == 6 && counts[2] == 1);
    CHECK(c3r_bam_write_haplotagged(b, "chr1", reads.data(), hp, ps, n, out_old.c_str(), nullptr, 1, counts) == C3R_OK);
    CHECK(slurp(out_null) == slurp(out_old));                               // pc = NULL: the old entry point's file, byte for byte

    const std::vector<Bytes> with_pc = aux_of_records(inflate_bgzf(slurp(out_pc))), without = aux_of_records(inflate_bgzf(slurp(out_old)));
    CHECK(with_pc.size() == (size_t)n && without.size() == (size_t)n);
    for (int k = 0; k < n; ++k) {
        Bytes want = k == 1 || k == 2 ? nm : Bytes();                       // (the stale HP / PS / PC are gone, NM stays)
        if (hp[k]) {
            want.insert(want.end(), {'H', 'P', 'C', hp[k], 'P', 'S'});
            const uint32_t s = (uint32_t)ps[k];
            if (s < 256) { want.push_back('C'); want.push_back((uint8_t)s); } else if (s < 65536) { want.push_back('S'); p16(want, s); } else { want.push_back('I'); p32(want, s); }
        }
        CHECK(without[(size_t)k] == want);
        if (hp[k]) {
            want.insert(want.end(), {'P', 'C'});
            if (pc[k] < 256) { want.push_back('C'); want.push_back((uint8_t)pc[k]); } else if (pc[k] < 65536) { want.push_back('S'); p16(want, pc[k]); } else { want.push_back('I'); p32(want, pc[k]); }
        }
        CHECK(with_pc[(size_t)k] == want);                                  // (an untagged read gets no PC whatever pc[k] says)
    }
    // the refusals are the old entry point's: a haplotype without a phase set, too few reads handed in — and no file is left
    const int32_t bad_ps[n] = {-1, -1, 300, 70000, 5, 5, 5, -1};
    CHECK(c3r_bam_write_haplotagged_pc(b, "chr1", reads.data(), hp, bad_ps, pc, n, out_pc.c_str(), nullptr, 1, counts) == C3R_EINVAL);
    CHECK(c3r_bam_write_haplotagged_pc(b, "chr1", reads.data(), hp, ps, pc, n - 1, out_pc.c_str(), nullptr, 1, counts) == C3R_EINVAL);
    FILE *gone = fopen(out_pc.c_str(), "rb");
    CHECK(!gone);
    CHECK(c3r_bam_write_haplotagged_pc(nullptr, "chr1", reads.data(), hp, ps, pc, n, out_pc.c_str(), nullptr, 1, counts) == C3R_EINVAL);
    c3r_bam_close(b);
    remove(path.c_str()); remove(out_null.c_str()); remove(out_old.c_str());
    printf("hapbam_pc_check: ok\n");
    return 0;
}
