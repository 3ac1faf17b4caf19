"""A BAM reader in plain Python for the tests of the haplotagged writer: SAM specification v1 sections 4.1 (BGZF) and 4.2 (BAM) read off
the page — zlib block by block, struct field by field.  It shares nothing with csrc/bamio.cpp or clair3_rna_amd/bam.py (no import of
either), checks what a reader may check (block sizes, CRC, ISIZE, the EOF block, that every aux field ends inside its record) and hands
out every record three ways: its raw bytes, its core fields, and the ordered list of its aux fields with type and value."""
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_FIXED = {"A": "<c", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


def blocks(path):
    """[(file offset, compressed size, payload bytes)] of every BGZF block, the EOF block included; asserts on every header field."""
    data = open(path, "rb").read()
    out, off = [], 0
    while off < len(data):
        id1, id2, cm, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<BBBBIBBH", data, off)
        assert (id1, id2, cm, flg) == (31, 139, 8, 4), "not a BGZF block at %d" % off
        extra, bsize, q = data[off + 12:off + 12 + xlen], None, 0
        while q < len(extra):
            si1, si2, slen = struct.unpack_from("<BBH", extra, q)
            if (si1, si2) == (66, 67):
                assert slen == 2
                bsize = struct.unpack_from("<H", extra, q + 4)[0] + 1
            q += 4 + slen
        assert bsize is not None and off + bsize <= len(data), "block at %d without size / past the file" % off
        crc, isize = struct.unpack_from("<II", data, off + bsize - 8)
        payload = zlib.decompressobj(-15).decompress(data[off + 12 + xlen:off + bsize - 8])
        assert len(payload) == isize and isize <= 65536 and (zlib.crc32(payload) & 0xffffffff) == crc, "block at %d: wrong ISIZE / CRC" % off
        out.append((off, bsize, payload))
        off += bsize
    assert off == len(data)
    return out


def parse_aux(raw, p):
    """[(tag, type, value)] of raw[p:]: value is a number, a 1-character str (A), bytes (Z, H: without the NUL) or (subtype, tuple) for B.
    Asserts that the last field ends exactly where the record does."""
    out = []
    while p < len(raw):
        assert p + 3 <= len(raw), "aux field cut short"
        tag, ty = raw[p:p + 2].decode("latin-1"), chr(raw[p + 2])
        p += 3
        if ty in _FIXED:
            n = struct.calcsize(_FIXED[ty])
            assert p + n <= len(raw), "aux value cut short"
            v = struct.unpack_from(_FIXED[ty], raw, p)[0]
            out.append((tag, ty, v.decode("latin-1") if ty == "A" else v))
            p += n
        elif ty in "ZH":
            q = raw.index(b"\x00", p)
            out.append((tag, ty, bytes(raw[p:q])))
            p = q + 1
        elif ty == "B":
            sub, cnt = chr(raw[p]), struct.unpack_from("<I", raw, p + 1)[0]
            fmt = "<%d%s" % (cnt, _FIXED[sub][1])
            assert p + 5 + struct.calcsize(fmt) <= len(raw), "B array cut short"
            out.append((tag, ty, (sub, struct.unpack_from(fmt, raw, p + 5))))
            p += 5 + struct.calcsize(fmt)
        else:
            raise AssertionError("aux type %r" % ty)
    assert p == len(raw)
    return out


class Record(object):
    """One alignment: raw (the block_size bytes after the length field), the core fields, and aux = [(tag, type, value)] in file order."""

    def __init__(self, raw):
        self.raw = raw
        (self.ref_id, self.pos, l_name, self.mapq, self.bin, self.n_cigar, self.flag, self.l_seq, self.next_ref_id, self.next_pos,
         self.tlen) = struct.unpack_from("<iiBBHHHiiii", raw, 0)
        p = 32
        self.name = raw[p:p + l_name - 1].decode("latin-1")
        assert raw[p + l_name - 1] == 0
        p += l_name
        self.cigar = list(struct.unpack_from("<%dI" % self.n_cigar, raw, p))
        p += 4 * self.n_cigar
        self.seq = raw[p:p + (self.l_seq + 1) // 2]
        p += (self.l_seq + 1) // 2
        self.qual = raw[p:p + self.l_seq]
        p += self.l_seq
        assert p <= len(raw)
        self.aux_off = p
        self.aux = parse_aux(raw, p)

    def tag(self, name):
        """(type, value) of the aux field `name`; None when absent; asserts that it occurs once."""
        hits = [(ty, v) for t, ty, v in self.aux if t == name]
        assert len(hits) <= 1, "%s occurs %d times" % (name, len(hits))
        return hits[0] if hits else None

    def without(self, names):
        """The record's bytes with the aux fields `names` cut out (what is left of the input's record in the output, and the reverse)."""
        out, p = bytearray(self.raw[:self.aux_off]), self.aux_off
        for t, ty, v in self.aux:
            if ty in _FIXED:
                n = 3 + struct.calcsize(_FIXED[ty])
            elif ty in "ZH":
                n = 3 + len(v) + 1
            else:
                n = 3 + 5 + struct.calcsize("<%d%s" % (len(v[1]), _FIXED[v[0]][1]))
            if t not in names:
                out += self.raw[p:p + n]
            p += n
        assert p == len(self.raw)
        return bytes(out)


class Bam(object):
    """text (header text, bytes), refs [(name, length)], records [Record] in file order, blocks (see blocks())."""

    def __init__(self, path):
        self.blocks = blocks(path)
        assert self.blocks and self.blocks[-1][2] == b"" and open(path, "rb").read()[-28:] == EOF_BLOCK, "no BGZF EOF block at the end"
        buf = b"".join(b[2] for b in self.blocks)
        assert buf[:4] == b"BAM\x01"
        l_text = struct.unpack_from("<i", buf, 4)[0]
        self.text = buf[8:8 + l_text]
        p = 8 + l_text
        n_ref = struct.unpack_from("<i", buf, p)[0]
        p += 4
        self.refs = []
        for _ in range(n_ref):
            l_name = struct.unpack_from("<i", buf, p)[0]
            name = buf[p + 4:p + 4 + l_name]
            assert name[-1] == 0
            self.refs.append((name[:-1].decode(), struct.unpack_from("<i", buf, p + 4 + l_name)[0]))
            p += 8 + l_name
        self.records = []
        while p < len(buf):
            bs = struct.unpack_from("<i", buf, p)[0]
            assert bs >= 32 and p + 4 + bs <= len(buf), "record at %d runs past the data" % p
            self.records.append(Record(buf[p + 4:p + 4 + bs]))
            p += 4 + bs
        assert p == len(buf)
