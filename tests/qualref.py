"""The base-quality threshold of include/c3r.h (c3r_set_hap_min_bq) in plain Python, base by base: the layout of the qualities, the masked
copy of the packed sequence that the site-table kernels read, and the reads with their masked bases replaced by N — the input on which the
switched-off engine must give what the switched-on engine gives on the real reads.  Shares nothing with csrc/qual_kernels.hpp; of the
package it imports reads.py's record types only.

Layout: the quality of base j of read i is byte 2 * seq_off_i + j of an array of 2 * len(seq) bytes; the byte behind a read of odd
length is 0xff.  Rule: with Q > 0 a base is masked iff its quality q satisfies q < Q and q != 0xff; Q = 0 masks nothing."""
import numpy as np

from clair3_rna_amd.reads import READ_DTYPE, ReadSet

N = 15


def qual_at(rs, i, j):
    """The quality byte of base j of read i."""
    return int(rs.qual[2 * int(rs.reads[i]["seq_off"]) + j])


def masked(q, Q):
    return Q > 0 and q < Q and q != 0xff


def layout_ok(rs):
    """Every byte of rs.qual is the quality of one base or a padding byte of 0xff, and the array has two bytes per sequence byte."""
    if rs.qual is None or len(rs.qual) != 2 * len(rs.seq):
        return False
    owner = np.zeros(len(rs.qual), np.int32)
    for r in rs.reads:
        o, L = 2 * int(r["seq_off"]), int(r["l_seq"])
        owner[o:o + L] += 1
        if L & 1:
            if rs.qual[o + L] != 0xff:
                return False
            owner[o + L] += 1
    return bool((owner == 1).all())


def mask(rs, Q):
    """(the packed sequence with every masked base as code 15, the number of masked bases)."""
    out = rs.seq.copy()
    n = 0
    for i, r in enumerate(rs.reads):
        s0 = int(r["seq_off"])
        for j in range(int(r["l_seq"])):
            if masked(qual_at(rs, i, j), Q):
                k = s0 + (j >> 1)
                out[k] = (out[k] | 0xf0) if (j & 1) == 0 else (out[k] | 0x0f)
                n += 1
    return out, n


def with_n(rs, Q):
    """A ReadSet without qualities whose masked bases are N: the same records and CIGARs over mask(rs, Q)'s sequence."""
    return ReadSet(rs.reads.copy(), rs.cigar.copy(), mask(rs, Q)[0])


def flat_readset(seq_bytes, quals, read_len):
    """Reads of `read_len` bases (the last one shorter) laid over n = len(seq_bytes) packed bytes, each `<l>M` at its own position, so that
    the flat arrays are exactly `seq_bytes` and `quals` (2 n bytes; the caller keeps the padding bytes at 0xff): what the kernel tests load."""
    n = len(seq_bytes)
    per = (read_len + 1) // 2
    recs = []
    for k, s0 in enumerate(range(0, n, per)):
        nb = min(per, n - s0)
        L = read_len if nb == per else 2 * nb
        recs.append((100 * k, k, 1, L, s0, 0, 60, 0, 0))
    reads = np.array(recs, dtype=READ_DTYPE) if recs else np.zeros(0, READ_DTYPE)
    cigar = np.array([(int(r["l_seq"]) << 4) for r in reads], np.uint32)
    return ReadSet(reads, cigar, np.asarray(seq_bytes, np.uint8), np.asarray(quals, np.uint8))
