// hapbam_check.cpp — c3r_bam_write_haplotagged (include/c3r_io.h) through the C ABI alone, from a program with its own main: it writes a
// BAM that holds the writer's edge cases (stale HP / PS / PC fields of several types between others, a placed record without CIGAR between
// two read records, a CG:B,I long-CIGAR record, a 70,000-base record that straddles three blocks, records of other contigs before and
// behind), tags it, reads the result back with a BGZF / BAM reader of its own and with c3r_bam_fetch, and goes through the error cases.
// Linked with csrc/bamio.cpp and csrc/vcfio.cpp; built plainly by tests/test_haplotag_bam.py, and with -fsanitize=address,undefined by hand.
//
//   hapbam_check <scratch directory>      prints "hapbam_check: ok" and exits 0; every file it wrote is removed
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/c3r.h"
#include "../../include/c3r_io.h"

typedef std::vector<uint8_t> Bytes;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "hapbam_check: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

static void p16(Bytes &v, uint32_t x) { v.push_back((uint8_t)x); v.push_back((uint8_t)(x >> 8)); }
static void p32(Bytes &v, uint32_t x) { p16(v, x & 0xffff); p16(v, x >> 16); }
static void pstr(Bytes &v, const char *s, size_t n) { v.insert(v.end(), s, s + n); }
static uint32_t g32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint32_t op(uint32_t len, uint32_t o) { return (len << 4) | o; }

// one alignment with its block_size in front
static Bytes rec(int32_t tid, int32_t pos, const std::vector<uint32_t> &cig, uint32_t l_seq, const Bytes &aux, uint32_t flag, int k) {
    Bytes b;
    char name[16];
    const int ln = snprintf(name, sizeof name, "r%d", k) + 1;
    p32(b, (uint32_t)tid); p32(b, (uint32_t)pos);
    b.push_back((uint8_t)ln); b.push_back(60); p16(b, 4680); p16(b, (uint32_t)cig.size()); p16(b, flag); p32(b, l_seq);
    p32(b, 0xffffffffu); p32(b, 0xffffffffu); p32(b, 0);
    pstr(b, name, (size_t)ln);
    for (uint32_t c : cig) p32(b, c);
    for (uint32_t i = 0; i < (l_seq + 1) / 2; ++i) b.push_back((uint8_t)(0x12 + 0x11 * ((i + (uint32_t)k) % 3)));
    for (uint32_t i = 0; i < l_seq; ++i) b.push_back((uint8_t)((i * 7 + (uint32_t)k) % 40));
    b.insert(b.end(), aux.begin(), aux.end());
    Bytes out;
    p32(out, (uint32_t)b.size());
    out.insert(out.end(), b.begin(), b.end());
    return out;
}

static Bytes aux_of(const char *s, size_t n) { return Bytes(s, s + n); }
#define AUX(lit) aux_of(lit, sizeof(lit) - 1)

static void write_bgzf(const std::string &path, const Bytes &data) {
    FILE *f = fopen(path.c_str(), "wb");
    CHECK(f);
    for (size_t o = 0; o < data.size(); o += 0xff00) {
        const size_t n = std::min<size_t>(0xff00, data.size() - o);
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

// the whole uncompressed stream of a BGZF file; *n_blocks = blocks, the EOF block included
static Bytes read_bgzf(const std::string &path, size_t *n_blocks) {
    FILE *f = fopen(path.c_str(), "rb");
    CHECK(f);
    Bytes file, out;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + n);
    fclose(f);
    *n_blocks = 0;
    for (size_t o = 0; o < file.size();) {
        CHECK(o + 18 <= file.size() && file[o] == 0x1f && file[o + 1] == 0x8b && file[o + 12] == 'B' && file[o + 13] == 'C');
        const size_t bs = (size_t)(file[o + 16] | (file[o + 17] << 8)) + 1;
        CHECK(o + bs <= file.size());
        const uint32_t isize = g32(&file[o + bs - 4]);
        const size_t at = out.size();
        out.resize(at + isize);
        z_stream zs; memset(&zs, 0, sizeof zs);
        CHECK(inflateInit2(&zs, -15) == Z_OK);
        zs.next_in = &file[o + 18]; zs.avail_in = (uInt)(bs - 26);
        zs.next_out = isize ? &out[at] : buf; zs.avail_out = isize;
        CHECK(inflate(&zs, Z_FINISH) == Z_STREAM_END && zs.avail_out == 0);
        inflateEnd(&zs);
        CHECK(g32(&file[o + bs - 8]) == (uint32_t)crc32(crc32(0L, Z_NULL, 0), isize ? &out[at] : buf, isize));
        if (o + bs == file.size()) CHECK(isize == 0 && bs == 28);                  // the EOF block ends the file
        else CHECK(isize == 0xff00 || o + bs + 28 == file.size());                 // cut every 0xff00 bytes, but for the last data block
        o += bs; ++*n_blocks;
    }
    return out;
}

// value of the integer aux field `tag` of the record at r[0, n) (behind block_size); -1 absent.  *type receives its type letter.
static int64_t aux_int(const uint8_t *r, size_t n, const char *tag, char *type, int *n_fields) {
    const uint32_t l_seq = g32(r + 16);
    size_t p = 32 + r[8] + 4 * (size_t)(r[12] | (r[13] << 8)) + (l_seq + 1) / 2 + l_seq;
    int64_t v = -1;
    *n_fields = 0;
    while (p < n) {
        CHECK(p + 3 <= n);
        const uint8_t t0 = r[p], t1 = r[p + 1], ty = r[p + 2];
        p += 3; ++*n_fields;
        size_t sz = 0;
        if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1; else if (ty == 's' || ty == 'S') sz = 2; else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
        else if (ty == 'Z' || ty == 'H') { while (r[p]) { ++p; CHECK(p < n); } sz = 1; }
        else { CHECK(ty == 'B'); const uint8_t sub = r[p]; sz = 5 + (size_t)g32(r + p + 1) * ((sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4); }
        CHECK(p + sz <= n);
        if (t0 == (uint8_t)tag[0] && t1 == (uint8_t)tag[1]) {
            CHECK(v == -1);
            *type = (char)ty;
            v = ty == 'C' ? r[p] : ty == 'S' ? (r[p] | (r[p + 1] << 8)) : ty == 'I' ? (int64_t)g32(r + p) : -2;
        }
        p += sz;
    }
    CHECK(p == n);
    return v;
}

static int refused(c3r_bam *b, const char *ctg, const c3r_read_t *reads, const uint8_t *hp, const int32_t *ps, int64_t n, const std::string &out, const char *word) {
    int64_t counts[4];
    const int rc = c3r_bam_write_haplotagged(b, ctg, reads, hp, ps, n, out.c_str(), nullptr, 2, counts);
    FILE *f = fopen(out.c_str(), "rb");
    if (f) fclose(f);
    if (rc != C3R_EINVAL || f || !strstr(c3r_bam_last_error(b), word)) {
        fprintf(stderr, "hapbam_check: expected C3R_EINVAL with '%s' and no file, got %d, '%s', file %s\n", word, rc, c3r_bam_last_error(b), f ? "left" : "absent");
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    CHECK(argc == 2);
    const std::string dir = argv[1], in = dir + "/hapbam_in.bam", out = dir + "/hapbam_out.bam", out2 = dir + "/hapbam_out2.bam", bai = out + ".bai";
    const std::string text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:1000\n@SQ\tSN:b\tLN:500000\n@SQ\tSN:c\tLN:1000\n@SQ\tSN:d\tLN:1000\n";
    const char *names[4] = {"a", "b", "c", "d"};
    const int32_t lens[4] = {1000, 500000, 1000, 1000};
    Bytes s;
    pstr(s, "BAM\1", 4); p32(s, (uint32_t)text.size()); pstr(s, text.data(), text.size()); p32(s, 4);
    for (int i = 0; i < 4; ++i) { p32(s, 2); pstr(s, names[i], 2); p32(s, (uint32_t)lens[i]); }
    std::vector<uint32_t> real = {op(3, 0), op(1, 1), op(2, 0), op(50, 3), op(4, 0)};
    Bytes cg = AUX("XXi\1\0\0\0CGBI\5\0\0\0");
    for (uint32_t c : real) p32(cg, c);
    pstr(cg, "HPC\2", 4);
    std::vector<Bytes> recs = {
        rec(0, 5, {op(10, 0)}, 10, AUX("HPC\1"), 0, 0),
        rec(1, 100, {op(10, 0)}, 10, AUX("NMi\3\0\0\0HPi\2\0\0\0RGZgrp\0PSi\5\0\0\0XFf\0\0\x20\x40PCi\x3c\0\0\0ZBBs\2\0\0\0\1\0\2\0"), 0, 1),
        rec(1, 105, {op(10, 0)}, 10, AUX("RGZgrp\0XHH1AE3\0PSZold\0HPAx"), 16, 2),
        rec(1, 120, {}, 10, AUX("HPC\1XXi\7\0\0\0"), 4, 3),                        // placed, no CIGAR: not a read record
        rec(1, 130, {op(10, 0)}, 10, Bytes(), 1024, 4),
        rec(1, 140, {op(20000, 0)}, 20000, AUX("NMi\4\0\0\0"), 0, 5),              // moves the next but one to where it spans three blocks
        rec(1, 150, {op(10, 4), op(59, 3)}, 10, cg, 0, 6),
        rec(1, 160, {op(70000, 0)}, 70000, AUX("HPs\1\0NMi\x09\0\0\0"), 0, 7),
        rec(1, 170, {op(10, 0)}, 0, AUX("XXi\2\0\0\0"), 0, 8),
        rec(3, 7, {op(10, 0)}, 10, AUX("HPC\2"), 0, 9),
        rec(-1, -1, {}, 10, AUX("HPC\1"), 4, 10),
    };
    for (const Bytes &r : recs) s.insert(s.end(), r.begin(), r.end());
    write_bgzf(in, s);

    c3r_bam *b = nullptr;
    CHECK(c3r_bam_open(in.c_str(), 2, &b) == C3R_OK);
    int64_t n = 0, nc = 0, ns = 0;
    CHECK(c3r_bam_fetch(b, "b", 0, 0, &n, &nc, &ns) == C3R_OK && n == 7);
    std::vector<c3r_read_t> reads((size_t)n);
    std::vector<uint32_t> cigar((size_t)nc);
    Bytes seq((size_t)ns);
    CHECK(c3r_bam_copy(b, reads.data(), cigar.data(), seq.data()) == C3R_OK);
    const uint8_t hp[7] = {1, 2, 0, 2, 1, 2, 1};
    const int32_t ps[7] = {100, 40000, -1, 70000, 255, 256, 65536};
    const char want_type[7] = {'C', 'S', 0, 'I', 'C', 'S', 'I'};
    const char *pg = "@PG\tID:c3r_haplotag\tPN:clair3_rna_amd\tVN:check\tCL:hapbam_check";
    int64_t counts[4] = {-1, -1, -1, -1}, counts1[4];
    CHECK(c3r_bam_write_haplotagged(b, "b", reads.data(), hp, ps, n, out.c_str(), pg, 4, counts) == C3R_OK);
    CHECK(counts[0] == 8 && counts[1] == 6 && counts[2] == 5 && counts[3] == 1);
    CHECK(c3r_bam_write_haplotagged(b, "b", reads.data(), hp, ps, n, out2.c_str(), pg, 1, counts1) == C3R_OK && memcmp(counts, counts1, sizeof counts) == 0);

    // read back: header, records, tags
    size_t n_blocks = 0, n_blocks1 = 0;
    const Bytes got = read_bgzf(out, &n_blocks);
    CHECK(got == read_bgzf(out2, &n_blocks1) && n_blocks == n_blocks1 && n_blocks >= 4);       // the bytes do not depend on the threads
    const std::string want_text = text + pg + "\n";
    CHECK(got.size() > 12 + want_text.size() && memcmp(got.data(), "BAM\1", 4) == 0 && g32(&got[4]) == want_text.size());
    CHECK(memcmp(&got[8], want_text.data(), want_text.size()) == 0);
    size_t p = 8 + want_text.size();
    CHECK(g32(&got[p]) == 4);
    p += 4 + 4 * (4 + 2 + 4);
    int k = 0, n_rec = 0;
    size_t big_start = 0, big_end = 0;
    for (size_t i = 1; i <= 8; ++i, ++n_rec) {
        CHECK(p + 4 <= got.size());
        const size_t bs = g32(&got[p]);
        const uint8_t *r = &got[p + 4], *src = recs[i].data() + 4;
        CHECK(p + 4 + bs <= got.size() && bs >= 32 && g32(r) == 1);
        const size_t fixed = 32 + src[8] + 4 * (size_t)(src[12] | (src[13] << 8)) + (g32(src + 16) + 1) / 2 + g32(src + 16);
        CHECK(memcmp(r, src, fixed) == 0);                                        // everything before the aux area is the input's
        if (i == 7) { big_start = p; big_end = p + 4 + bs - 1; }
        char ty = 0, ty2 = 0;
        int nf = 0;
        const int64_t h = aux_int(r, bs, "HP", &ty, &nf), set = aux_int(r, bs, "PS", &ty2, &nf);
        int dummy;
        CHECK(aux_int(r, bs, "PC", &ty, &dummy) == -1);
        if (i == 3) { CHECK(h == -1 && set == -1 && nf == 1); }                   // the record without CIGAR: stripped, never tagged
        else {
            if (hp[k]) CHECK(h == hp[k] && set == ps[k] && ty2 == want_type[k]); else CHECK(h == -1 && set == -1);
            ++k;
        }
        if (i == 1) CHECK(nf == 6);                                               // NM RG XF ZB + HP PS
        if (i == 2) CHECK(nf == 4);                                               // RG XH + HP PS: the stale PS:Z and HP:A went
        p += 4 + bs;
    }
    CHECK(p == got.size() && k == 7 && n_rec == 8);
    CHECK(big_end / 0xff00 - big_start / 0xff00 == 2);                            // the 70,000-base record lies in three blocks

    // the product's reader and indexer on the result
    c3r_bam *o = nullptr;
    CHECK(c3r_bam_index_build(out.c_str(), bai.c_str()) == C3R_OK);
    CHECK(c3r_bam_open(out.c_str(), 3, &o) == C3R_OK && c3r_bam_has_index(o) == 1);
    int64_t m = 0, mc = 0, ms = 0;
    CHECK(c3r_bam_fetch(o, "b", 0, 0, &m, &mc, &ms) == C3R_OK && m == n && mc == nc && ms == ns);
    std::vector<c3r_read_t> back((size_t)m);
    std::vector<uint32_t> cigar2((size_t)mc);
    Bytes seq2((size_t)ms);
    CHECK(c3r_bam_copy(o, back.data(), cigar2.data(), seq2.data()) == C3R_OK && cigar2 == cigar && seq2 == seq);
    for (int64_t i = 0; i < m; ++i) CHECK(back[(size_t)i].hp == hp[i] && back[(size_t)i].pos == reads[(size_t)i].pos && back[(size_t)i].flag == reads[(size_t)i].flag);
    CHECK(c3r_bam_fetch(o, "b", 70100, 70101, &m, nullptr, nullptr) == C3R_OK && m == 1);
    CHECK(c3r_bam_fetch(o, "a", 0, 0, &m, nullptr, nullptr) == C3R_OK && m == 0);
    // through the new index the writer gives the same file again but for the second @PG line; an empty contig is header + EOF
    CHECK(c3r_bam_write_haplotagged(o, "b", reads.data(), hp, ps, n, out2.c_str(), nullptr, 2, counts1) == C3R_OK && counts1[0] == 8 && counts1[2] == 6);
    CHECK(read_bgzf(out2, &n_blocks1) == got);
    CHECK(c3r_bam_write_haplotagged(o, "c", nullptr, nullptr, nullptr, 0, out2.c_str(), nullptr, 2, counts1) == C3R_OK && counts1[0] == 0);
    CHECK(read_bgzf(out2, &n_blocks1).size() == 8 + want_text.size() + 4 + 40 && n_blocks1 == 2);
    c3r_bam_close(o);
    remove(out2.c_str());

    // the refusals: C3R_EINVAL, a message that names the index, no file
    int bad = 0;
    bad += refused(b, "b", reads.data(), hp, ps, n - 1, out2, "more read records than the 6 handed in");
    std::vector<c3r_read_t> longer(reads);
    longer.push_back(reads.back());
    const uint8_t hp8[8] = {1, 2, 0, 2, 1, 2, 1, 0};
    const int32_t ps8[8] = {100, 40000, -1, 70000, 255, 256, 65536, -1};
    bad += refused(b, "b", longer.data(), hp8, ps8, 8, out2, "reads[7] has no record");
    std::vector<c3r_read_t> swapped(reads);
    std::swap(swapped[1].flag, swapped[2].flag);
    bad += refused(b, "b", swapped.data(), hp, ps, n, out2, "reads[1]");
    uint8_t hp3[7]; memcpy(hp3, hp, 7); hp3[5] = 3;
    bad += refused(b, "b", reads.data(), hp3, ps, n, out2, "hp[5] = 3");
    int32_t psm[7]; memcpy(psm, ps, sizeof ps); psm[4] = -1;
    bad += refused(b, "b", reads.data(), hp, psm, n, out2, "hp[4] = 1 without a phase set");
    bad += refused(b, "nope", reads.data(), hp, ps, n, out2, "no contig nope");
    c3r_bam_close(b);
    // a truncated aux area
    Bytes t(s.begin(), s.begin() + (long)(8 + text.size() + 4 + 40));
    const Bytes cut = rec(1, 100, {op(10, 0)}, 10, AUX("NMi\1\2"), 0, 1), fine = rec(1, 90, {op(10, 0)}, 10, AUX("NMi\1\0\0\0"), 0, 0);
    t.insert(t.end(), fine.begin(), fine.end());
    t.insert(t.end(), cut.begin(), cut.end());
    write_bgzf(in, t);
    CHECK(c3r_bam_open(in.c_str(), 1, &b) == C3R_OK);
    bad += refused(b, "b", nullptr, nullptr, nullptr, 0, out2, "malformed alignment record at position 101");
    c3r_bam_close(b);
    remove(in.c_str()); remove(out.c_str()); remove(bai.c_str());
    if (bad) return 1;
    printf("hapbam_check: ok\n");
    return 0;
}
