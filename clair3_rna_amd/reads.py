"""Flat read records: the host-side container handed to libc3r (include/c3r_types.h: c3r_read_t).

One ReadSet = the alignments of one contig in BAM order, i.e. what `samtools mpileup <bam> -r ctg:...`
would stream in the reference (src/create_tensor_pileup.py:446-451).
"""
import numpy as np

READ_DTYPE = np.dtype([("pos", "<i4"), ("cigar_off", "<u4"), ("n_cigar", "<u4"), ("l_seq", "<u4"),
                       ("seq_off", "<u8"), ("flag", "<u2"), ("mapq", "u1"), ("hp", "u1"), ("reserved", "<u4")],
                      align=True)
assert READ_DTYPE.itemsize == 32

CIGAR_OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"
_NT16_CODE = {c: i for i, c in enumerate(NT16)}
_NT16_CODE.update({c.lower(): i for i, c in enumerate(NT16)})


def parse_cigar(s):
    """'10M2I5N3M' -> uint32 array of BAM-encoded ops (len << 4 | op)."""
    out, num = [], 0
    for ch in s:
        if ch.isdigit():
            num = num * 10 + ord(ch) - 48
        else:
            out.append((num << 4) | CIGAR_OPS.index(ch))
            num = 0
    return np.asarray(out, dtype=np.uint32)


def pack_seq(seq):
    """ASCII bases -> BAM 4-bit packed bytes (first base in the high nibble)."""
    codes = np.fromiter((_NT16_CODE.get(c, 15) for c in seq), dtype=np.uint8, count=len(seq))
    if len(codes) & 1:
        codes = np.append(codes, np.uint8(0))
    return ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8)


def qual_bytes(q, l_seq):
    """One record's qualities -> l_seq phred bytes: a list of ints, a phred+33 string, or None (absent: 0xff throughout, as BAM
    stores it)."""
    if q is None:
        return np.full(l_seq, 0xff, np.uint8)
    a = np.frombuffer(q.encode("ascii"), np.uint8).astype(np.int64) - 33 if isinstance(q, str) else np.asarray(q, dtype=np.int64).reshape(-1)
    if len(a) != l_seq:
        raise ValueError("%d qualities for %d bases" % (len(a), l_seq))
    if len(a) and (a.min() < 0 or a.max() > 255):
        raise ValueError("quality outside 0..255")
    return a.astype(np.uint8)


class ReadSet(object):
    """reads (READ_DTYPE[n]), cigar (uint32[]), seq (uint8[] 4-bit packed), sorted by pos.  qual: None (absent) or uint8[2 * len(seq)],
    the base qualities in the layout of include/c3r_io.h: the quality of base j of read i is byte 2 * seq_off_i + j, the padding byte
    behind a read of odd length is 0xff."""

    qual = None         # (also for a set put together without __init__)

    def __init__(self, reads, cigar, seq, qual=None):
        self.reads = np.ascontiguousarray(reads, dtype=READ_DTYPE)
        self.cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.qual = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
        if self.qual is not None and self.qual.size != 2 * self.seq.size:
            raise ValueError("%d quality bytes for %d sequence bytes (2 per byte)" % (self.qual.size, self.seq.size))

    def __len__(self):
        return len(self.reads)

    @classmethod
    def from_records(cls, records):
        """records: iterable of dicts/tuples (pos0, cigar_str, seq_str, flag, mapq, hp); sorted by pos (stable).  A dict may hold
        "qual" (a list of ints or a phred+33 string); when one record does, the set carries qualities (0xff for the others)."""
        recs = [r if isinstance(r, dict) else dict(zip(("pos", "cigar", "seq", "flag", "mapq", "hp"), r)) for r in records]
        recs.sort(key=lambda r: r["pos"])
        reads = np.zeros(len(recs), dtype=READ_DTYPE)
        cig, seqs, quals = [], [], []
        want_q = any(r.get("qual") is not None for r in recs)
        coff = soff = 0
        for i, r in enumerate(recs):
            c = parse_cigar(r["cigar"]) if isinstance(r["cigar"], str) else np.asarray(r["cigar"], dtype=np.uint32)
            s = pack_seq(r["seq"])
            reads[i] = (r["pos"], coff, len(c), len(r["seq"]), soff, r.get("flag", 0), r.get("mapq", 60), r.get("hp", 0), 0)
            cig.append(c)
            seqs.append(s)
            if want_q:
                q = np.full(2 * len(s), 0xff, np.uint8)
                q[:len(r["seq"])] = qual_bytes(r.get("qual"), len(r["seq"]))
                quals.append(q)
            coff += len(c)
            soff += len(s)
        cigar = np.concatenate(cig) if cig else np.zeros(0, np.uint32)
        seq = np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)
        return cls(reads, cigar, seq, (np.concatenate(quals) if quals else np.zeros(0, np.uint8)) if want_q else None)

    def read_bases(self, i, q0, n):
        """Decode n bases of read i starting at query offset q0 (upper-case ASCII)."""
        r = self.reads[i]
        out = []
        for q in range(q0, q0 + n):
            if q >= r["l_seq"]:
                out.append("N")
                continue
            b = int(self.seq[int(r["seq_off"]) + (q >> 1)])
            out.append(NT16[(b & 15) if (q & 1) else (b >> 4)])
        return "".join(out)
