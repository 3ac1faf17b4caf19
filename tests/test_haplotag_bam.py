"""The haplotagged BAM writer (include/c3r_io.h: c3r_bam_write_haplotagged; clair3_rna_amd/haplotag_bam.py; call_sample --haplotagged_bam)
on the CPU: tag arrays given by hand, the output read back by tests/bamref.py — a BAM reader that shares nothing with the writer — and by
the product's own reader.  The drivers run with the engine replaced by a stub that returns tests/hapref.py's tags (the GPU tests of
tests/test_gpu_haplotag_bam.py run them on the device)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from clair3_rna_amd import bam, bamio
from tests import bamref, hapcountref, hapref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, N, S = 0, 1, 2, 3, 4
PHASE = ("HP", "PS", "PC")
CONTIGS = (("c0", 50000), ("c1", 400000), ("c2", 9000), ("c3", 7000))
HEADER = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS) + "@PG\tID:aligner\tPN:aligner\n"
PG = "@PG\tID:c3r_haplotag\tPN:clair3_rna_amd\tVN:test\tPP:aligner\tCL:by hand"


def op(ln, o):
    return (ln << 4) | o


def reg2bin(beg, end):
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


def rec(tid, pos, cig, l_seq, aux=b"", flag=0, mapq=60, name=b"read", k=0):
    """One alignment's bytes with its block_size in front: bases, qualities and the name vary with k."""
    qn = name + b"%d" % k + b"\x00"
    ref_len = sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8))
    seq = bytes(((1, 2, 4, 8)[(i + k) % 4] << 4) | (1, 2, 4, 8)[(i + 1 + k) % 4] for i in range((l_seq + 1) // 2))
    qual = bytes((7 * i + k) % 41 for i in range(l_seq))
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qn), mapq, reg2bin(max(pos, 0), max(pos, 0) + max(1, ref_len)), len(cig), flag, l_seq, -1, -1, 0) + qn + \
        np.asarray(cig, "<u4").tobytes() + seq + qual + aux
    return struct.pack("<i", len(body)) + body


def write_raw(path, records, text=HEADER):
    out = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(CONTIGS)))
    for name, ln in CONTIGS:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\x00" + struct.pack("<i", ln)
    out += b"".join(records)
    with open(path, "wb") as f:
        bam._bgzf_write(f, bytes(out))
        f.write(bam._BGZF_EOF)


I32 = lambda v: struct.pack("<i", v)
LONG = [op(3, M), op(1, I), op(2, M), op(50, N), op(4, M)]                        # the real CIGAR of the CG:B,I record: 10 bases, 59 on the reference
OTHERS = b"RGZgrp1\x00" + b"XHH1AE301\x00" + b"ZBBs" + struct.pack("<Ihhh", 3, 1, -2, 3) + b"XFf" + struct.pack("<f", 1.5) + b"XAAq"


def edge_records():
    """(records of the file in order, per c1 record: is it a read record of the fetch).  c1 holds what can go wrong; c0 and c3 lie before
    and behind it, the unplaced tail at the end."""
    c1 = [
        # a record of the contig without a position: sorts first, never a read record
        (rec(1, -1, [], 10, b"HPC\x02", flag=4, k=1), False),
        # old HP / PS / PC between other aux fields: they go, the order of the others stays
        (rec(1, 100, [op(10, M)], 10, b"NMi" + I32(3) + b"HPi" + I32(2) + b"RGZgrp1\x00" + b"PSi" + I32(5) + b"XFf" + struct.pack("<f", 2.5) + b"PCi" + I32(60)
             + b"ZBBC" + struct.pack("<IBB", 2, 7, 9), k=2), True),
        (rec(1, 105, [op(10, M)], 10, OTHERS, flag=16, k=3), True),                 # tagged, with Z, H, B, f and A fields
        (rec(1, 110, [op(4, S), op(6, M)], 10, OTHERS + b"PSZold\x00" + b"HPAx" + b"PCBc" + struct.pack("<Ib", 1, -1), k=4), True),   # untagged; stale tags of odd types
        (rec(1, 120, [], 10, b"HPC\x01" + b"XXi" + I32(7), flag=4, mapq=0, k=5), False),     # flag 4, placed, no CIGAR: passes through between two kept ones
        (rec(1, 130, [op(10, M)], 10, b"", flag=1024, k=6), True),                  # no aux field at all
        (rec(1, 140, [op(20000, M)], 20000, b"NMi" + I32(4), k=10), True),           # 30 kb: moves the 70,000-base record to where it spans three blocks
        (rec(1, 150, [op(10, S), op(59, N)], 10, b"XXi" + I32(1) + b"CGBI" + struct.pack("<I", len(LONG)) + np.asarray(LONG, "<u4").tobytes() + b"HPC\x02", k=7), True),
        (rec(1, 160, [op(70000, M)], 70000, b"HPs" + struct.pack("<h", 1) + b"NMi" + I32(9), k=8), True),           # 70,000 bases, 105 kb: straddles three blocks
        (rec(1, 170, [op(10, M)], 0, b"XXi" + I32(2), k=9), True),                  # l_seq = 0
    ]
    for k in range(30):                                                             # filler, some of it with stale tags
        aux = (b"HPC\x01" if k % 3 == 0 else b"") + b"NMi" + I32(k) + (b"PSI" + struct.pack("<I", 99) if k % 5 == 0 else b"")
        c1.append((rec(1, 80000 + 700 * k, [op(20 + k, M), op(100 * k + 1, N), op(5, M)], 25 + k, aux, flag=16 * (k & 1), mapq=60 - k, k=100 + k), True))
    before = [rec(0, 10 + 5 * k, [op(10, M)], 10, b"HPC\x01", k=200 + k) for k in range(3)]
    after = [rec(3, 20 + 5 * k, [op(10, M)], 10, b"HPC\x02", k=300 + k) for k in range(3)] + [rec(-1, -1, [], 10, b"HPC\x01", flag=4, k=400)]
    return before + [r for r, _ in c1] + after, [kept for _, kept in c1]


def hand_tags(n):
    """hp / ps by hand for the n read records of c1: all three classes, phase sets of 100, 40,000 and 70,000 (types C, S, I), 0 and 255 / 256 /
    65535 / 65536 on the type borders; -1 where the tag is 0."""
    hp = np.array([(1, 2, 0, 2, 1, 2, 0)[k % 7] for k in range(n)], np.uint8)
    sets = (100, 40000, 70000, 0, 255, 256, 65535, 65536, 2 ** 31 - 1)
    ps = np.array([sets[k % len(sets)] if hp[k] else -1 for k in range(n)], np.int32)
    return hp, ps


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("hapbam"))
    records, kept = edge_records()
    src = os.path.join(d, "in.bam")
    write_raw(src, records)
    indexed = os.path.join(d, "indexed.bam")
    shutil.copy(src, indexed)
    bamio.index_build(indexed)
    with bamio.BamFile(src) as bf:
        rs = bf.fetch("c1")
    assert len(rs) == sum(kept) == 38
    hp, ps = hand_tags(len(rs))
    assert {0, 1, 2} == set(hp.tolist()) and hp[0] == 1 and ps[0] == 100 and hp[2] == 0
    out = os.path.join(d, "out.bam")
    with bamio.BamFile(src, threads=2) as bf:
        counts = bf.write_haplotagged("c1", out, rs, hp, ps, pg_line=PG, threads=1)
    return dict(d=d, src=src, indexed=indexed, rs=rs, hp=hp, ps=ps, out=out, counts=counts, kept=kept, inp=bamref.Bam(src), got=bamref.Bam(out))


def test_every_record_of_the_contig_and_no_other(edge):
    inp, got = edge["inp"], edge["got"]
    mine = [r for r in inp.records if r.ref_id == 1]
    assert len(mine) == len(edge["kept"]) == 40 and len(inp.records) == 40 + 7
    assert len(got.records) == len(mine) and all(r.ref_id == 1 for r in got.records)
    for a, b in zip(mine, got.records):
        # the record with HP / PS / PC removed equals the input record with HP / PS / PC removed, byte for byte
        assert b.without(PHASE) == a.without(PHASE), a.name
        assert (b.name, b.pos, b.bin, b.flag, b.mapq, b.cigar, b.seq, b.qual) == (a.name, a.pos, a.bin, a.flag, a.mapq, a.cigar, a.seq, a.qual)
        assert [x for x in b.aux if x[0] not in PHASE] == [x for x in a.aux if x[0] not in PHASE]
        assert not any(t == "PC" for t, _, _ in b.aux)
    long_rec = got.records[7]                                   # the placeholder CIGAR and its CG array are the input's
    assert long_rec.cigar == [op(10, S), op(59, N)] and long_rec.tag("CG") == ("B", ("I", tuple(LONG)))
    assert [t for t, _, _ in got.records[1].aux] == ["NM", "RG", "XF", "ZB", "HP", "PS"]       # the old fields went, the order stayed, the new ones are last


def test_the_tags_are_the_arrays(edge):
    got, hp, ps = edge["got"], edge["hp"], edge["ps"]
    k = 0
    for r, kept in zip(got.records, edge["kept"]):
        if not kept or hp[k] == 0:
            assert r.tag("HP") is None and r.tag("PS") is None, r.name
        else:
            want_ty = "C" if ps[k] < 256 else "S" if ps[k] < 65536 else "I"
            assert r.tag("HP") == ("C", int(hp[k])) and r.tag("PS") == (want_ty, int(ps[k])), (r.name, k)
            assert [t for t, _, _ in r.aux][-2:] == ["HP", "PS"]
        k += int(kept)
    assert k == len(hp)
    seen = {r.tag("PS") for r in got.records if r.tag("PS")}
    assert {("C", 100), ("S", 40000), ("I", 70000), ("C", 0), ("C", 255), ("S", 256), ("S", 65535), ("I", 65536), ("I", 2 ** 31 - 1)} <= seen
    # the product's reader sees the array
    with bamio.BamFile(edge["out"]) as bf:
        back = bf.fetch("c1")
    assert back.reads["hp"].tolist() == hp.tolist()
    for f in ("pos", "flag", "mapq", "l_seq", "n_cigar"):
        assert np.array_equal(back.reads[f], edge["rs"].reads[f]), f
    assert np.array_equal(back.cigar, edge["rs"].cigar) and np.array_equal(back.seq, edge["rs"].seq)


def test_counts_header_and_blocks(edge):
    hp = edge["hp"]
    stale = sum(1 for r in edge["inp"].records if r.ref_id == 1 and any(t in PHASE for t, _, _ in r.aux))
    assert edge["counts"] == dict(records=40, tagged=int((hp > 0).sum()), stripped=stale, unpaired=2) and stale >= 15
    inp, got = edge["inp"], edge["got"]
    assert got.text == inp.text + PG.encode() + b"\n" and got.refs == inp.refs == list(CONTIGS)
    # the payload is cut every 0xff00 bytes wherever that falls; the 70,000-base record spans three blocks
    sizes = [len(p) for _, _, p in got.blocks]
    assert sizes[-1] == 0 and all(s == 0xff00 for s in sizes[:-2]) and 0 < sizes[-2] <= 0xff00 and len(sizes) >= 4
    start = sum(len(struct.pack("<i", 0)) + len(r.raw) for r in got.records[:8]) + 8 + len(got.text) + 4 + sum(8 + len(n) + 1 for n, _ in got.refs)
    assert (start + 4 + len(got.records[8].raw) - 1) // 0xff00 - start // 0xff00 == 2
    with bamio.BamFile(edge["out"]) as bf:
        assert bf.header_text() == got.text and bf.contigs() == list(CONTIGS)


def test_the_bytes_do_not_depend_on_threads_or_on_the_index(edge, tmp_path):
    want = open(edge["out"], "rb").read()
    for src, handle_threads, threads in ((edge["src"], 1, 4), (edge["indexed"], 3, 4), (edge["indexed"], 1, 1), (edge["src"], 4, 0)):
        out = str(tmp_path / "t.bam")
        with bamio.BamFile(src, threads=handle_threads) as bf:
            assert bf.has_index == (src == edge["indexed"])
            assert bf.write_haplotagged("c1", out, edge["rs"], edge["hp"], edge["ps"], pg_line=PG, threads=threads) == edge["counts"]
        assert open(out, "rb").read() == want, (src, threads)


def test_records_across_inflate_rounds(edge, tmp_path, monkeypatch):
    monkeypatch.setenv("C3R_IO_BATCH", "1")                     # one block per round: the 70,000-base record is carried over several rounds
    out = str(tmp_path / "b.bam")
    for src in (edge["src"], edge["indexed"]):
        with bamio.BamFile(src, threads=2) as bf:
            bf.write_haplotagged("c1", out, edge["rs"], edge["hp"], edge["ps"], pg_line=PG, threads=2)
        assert open(out, "rb").read() == open(edge["out"], "rb").read()


def test_the_new_index_finds_what_the_input_holds(edge, tmp_path):
    out = str(tmp_path / "c1.bam")
    shutil.copy(edge["out"], out)
    bai = bamio.index_build(out)
    assert os.path.getsize(bai) > 8
    regions = [(0, 0), (100, 101), (109, 111), (125, 135), (150, 151), (180, 181), (160, 70160), (70159, 70160), (80000, 90000), (99999, 100001), (300000, 400000)]
    with bamio.BamFile(out) as new, bamio.BamFile(edge["indexed"]) as old:
        assert new.has_index and old.has_index
        for a, b in regions:
            x, y = new.fetch("c1", a, b), old.fetch("c1", a, b)
            for f in ("pos", "flag", "mapq", "l_seq", "n_cigar", "cigar_off", "seq_off"):
                assert np.array_equal(x.reads[f], y.reads[f]), (a, b, f)
            assert np.array_equal(x.cigar, y.cigar) and np.array_equal(x.seq, y.seq)
        assert len(new.fetch("c1", 180, 181)) == 3 and len(new.fetch("c1", 125, 135)) == 1
        assert len(new.fetch("c0")) == 0 and len(new.fetch("c3")) == 0
        # and a second round: the output is an input like any other (its @PG gets a successor, its tags are replaced)
        again = str(tmp_path / "again.bam")
        rs = new.fetch("c1")
        swapped = np.array([0, 2, 1], np.uint8)[edge["hp"]]
        new.write_haplotagged("c1", again, rs, swapped, edge["ps"], pg_line=PG.replace("ID:c3r_haplotag", "ID:c3r_haplotag.1"), threads=2)
    with bamio.BamFile(again) as bf:
        assert bf.fetch("c1").reads["hp"].tolist() == swapped.tolist()
    assert all(len([t for t, _, _ in r.aux if t in PHASE]) in (0, 2) for r in bamref.Bam(again).records)


def test_a_contig_without_records_gives_a_valid_empty_bam(edge, tmp_path):
    for src in (edge["src"], edge["indexed"]):
        out = str(tmp_path / "empty.bam")
        with bamio.BamFile(src) as bf:
            assert bf.write_haplotagged("c2", out, pg_line=PG) == dict(records=0, tagged=0, stripped=0, unpaired=0)
            empty = np.zeros(0, np.uint8)
            assert bf.write_haplotagged("c2", out + "2", bf.fetch("c2"), empty, empty.astype(np.int32), pg_line=PG)["records"] == 0
        got = bamref.Bam(out)
        assert got.records == [] and got.refs == list(CONTIGS) and got.text == edge["inp"].text + PG.encode() + b"\n"
        assert open(out, "rb").read() == open(out + "2", "rb").read()
        bamio.index_build(out)
        with bamio.BamFile(out) as bf:
            assert bf.has_index and len(bf.fetch("c2")) == 0 and len(bf.fetch("c1")) == 0


def test_no_arrays_means_untagged_and_stripped_and_no_pg_line_means_the_input_header(edge, tmp_path):
    out = str(tmp_path / "plain.bam")
    with bamio.BamFile(edge["indexed"]) as bf:
        st = bf.write_haplotagged("c1", out)
    assert st == dict(records=40, tagged=0, stripped=edge["counts"]["stripped"], unpaired=2)
    got = bamref.Bam(out)
    assert got.text == edge["inp"].text
    mine = [r for r in edge["inp"].records if r.ref_id == 1]
    assert [r.raw for r in got.records] == [r.without(PHASE) for r in mine]
    with bamio.BamFile(out) as bf:
        assert not bf.fetch("c1").reads["hp"].any()


def _refused(src, d, match, rs, hp, ps, contig="c1"):
    out = os.path.join(d, "refused.bam")
    with bamio.BamFile(src) as bf:
        with pytest.raises(IOError, match=match):
            bf.write_haplotagged(contig, out, rs, hp, ps, pg_line=PG)
    assert not os.path.exists(out)


def test_arrays_that_do_not_fit_are_refused_and_leave_no_file(edge, tmp_path):
    from clair3_rna_amd.reads import ReadSet
    rs, hp, ps, d = edge["rs"], edge["hp"], edge["ps"], str(tmp_path)
    cut = lambda n: ReadSet(rs.reads[:n].copy(), rs.cigar, rs.seq)
    for src in (edge["src"], edge["indexed"]):
        _refused(src, d, "more read records than the 37 handed in", cut(37), hp[:37], ps[:37])              # one short
        longer = ReadSet(np.concatenate([rs.reads, rs.reads[-1:]]), rs.cigar, rs.seq)
        _refused(src, d, r"holds 38 read records, 39 were handed in \(reads\[38\]", longer, np.append(hp, 0).astype(np.uint8), np.append(ps, -1).astype(np.int32))
        swapped = cut(38)
        assert swapped.reads["flag"][1] == 16 and swapped.reads["flag"][2] == 0
        swapped.reads["flag"][[1, 2]] = swapped.reads["flag"][[2, 1]]
        _refused(src, d, r"reads\[1\] .* is not record 1 of c1", swapped, hp, ps)
        for field, value in (("pos", 7), ("mapq", 3), ("l_seq", 11)):
            off = cut(38)
            off.reads[field][20] = value
            _refused(src, d, r"reads\[20\]", off, hp, ps)
        bad = hp.copy()
        bad[5] = 3
        _refused(src, d, r"hp\[5\] = 3", rs, bad, ps)
        bad = ps.copy()
        assert hp[4] == 1
        bad[4] = -1
        _refused(src, d, r"hp\[4\] = 1 without a phase set", rs, hp, bad)
        _refused(src, d, "no contig nope", rs, hp, ps, contig="nope")
    with bamio.BamFile(edge["src"]) as bf:
        with pytest.raises(IOError, match="one @PG line"):
            bf.write_haplotagged("c1", os.path.join(d, "x.bam"), rs, hp, ps, pg_line="@CO\tnot a program line")
        with pytest.raises(ValueError):
            bf.write_haplotagged("c1", os.path.join(d, "x.bam"), rs, hp[:5], ps)
    assert os.listdir(d) == []


@pytest.mark.parametrize("aux,why", [(b"NMi\x01\x02", "cut short"), (b"NMi" + I32(1) + b"XY", "cut short"), (b"RGZnever ends", "unterminated"),
                                     (b"XQ?" + I32(0), "unknown type"), (b"ZBBs" + struct.pack("<I", 5000) + b"\x00" * 4, "B-array")])
def test_an_aux_area_that_cannot_be_walked_is_an_error_not_a_pass_through(tmp_path, aux, why):
    good = [rec(1, 100 + 5 * k, [op(10, M)], 10, b"NMi" + I32(k), k=k) for k in range(4)]
    # once on a read record, once on a record the fetch skips (no CIGAR): it is copied too, so it is walked too
    for bad in (rec(1, 118, [op(10, M)], 10, aux, k=9), rec(1, 118, [], 10, aux, flag=4, k=9)):
        src = str(tmp_path / "bad.bam")
        write_raw(src, good + [bad])
        out = str(tmp_path / "out.bam")
        with bamio.BamFile(src) as bf:
            with pytest.raises(IOError, match="malformed alignment record at position 119 .*" + why):
                bf.write_haplotagged("c1", out)
        assert not os.path.exists(out)


def test_the_pg_line():
    from clair3_rna_amd import haplotag_bam as hb
    assert hb.pg_line(b"@HD\tVN:1.6\n", "c3r 0.1", "a  b\tc\n") == "@PG\tID:c3r_haplotag\tPN:clair3_rna_amd\tVN:c3r 0.1\tCL:a b c"
    text = HEADER + "@PG\tPN:x\tID:c3r_haplotag\tPP:aligner\n@PG\tID:c3r_haplotag.1\tPP:c3r_haplotag\n@PG\tID:last\n"
    assert hb.pg_line(text.encode() + b"\x00\x00", "v", "cmd") == "@PG\tID:c3r_haplotag.2\tPN:clair3_rna_amd\tVN:v\tPP:last\tCL:cmd"


# ---- the drivers, with the engine replaced by the restatement
class StubEngine(object):
    """What haplotag_bam asks of capi.Engine, answered by tests/hapref.py and tests/hapcountref.py."""
    loads = []

    def __init__(self, device=0):
        pass

    def set_params(self, **kw):
        assert not kw

    def set_phase_sites(self, table):
        self.table = table

    def load_reads(self, rs):
        self.rs = rs
        StubEngine.loads.append(len(rs))

    def haplotags(self):
        tags, st, _ = hapref.haplotag(self.rs, self.table)
        return tags, st

    def read_phase_sets(self):
        return hapcountref.read_phase_sets(self.rs, self.table)

    def close(self):
        pass


def two_contig_sample(d, tag_input=False):
    """chr1 (phased: a directory with phased_chr1.vcf.gz), chr2 (nothing phased), chrEmpty (no record) of gen_case reads, indexed."""
    import gzip
    from clair3_rna_amd.reads import NT16
    contigs, reads, case = [], {}, {}
    for name, seed in (("chr1", 0), ("chr2", 1)):
        ref, rs, sites, _ = hapref.gen_case(seed, n_reads=83)
        if tag_input:                                         # wrong tags in the input: every read of both contigs says haplotype 2
            rs = hapref.with_hp(rs, 2)
        contigs.append((name, len(ref)))
        reads[name], case[name] = rs, (ref, sites)
    bam_fn = os.path.join(d, "plain.bam")
    bam.write_bam(bam_fn, contigs + [("chrEmpty", 5000)], reads)
    bamio.index_build(bam_fn)
    per = os.path.join(d, "phased_vcf")
    os.makedirs(per)
    with gzip.open(os.path.join(per, "phased_chr1.vcf.gz"), "wt") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")
        for s in case["chr1"][1]:
            f.write("chr1\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s:%d\n" % (s["pos"], NT16[s["ref"]], NT16[s["alt"]], "1|0" if s["h1"] else "0|1", s["ps"]))
    return dict(bam=bam_fn, per=per, reads=reads, case=case, contigs=contigs)


def check_tagged_files(s, out_dir, contigs=("chr1", "chr2")):
    """<out_dir>/<ctg>.bam + .bai for `contigs` and nothing else; chr1's HP / PS are the restatement's tags and sets, all three classes present;
    chr2 is untagged."""
    assert sorted(os.listdir(out_dir)) == sorted([c + ".bam" for c in contigs] + [c + ".bam.bai" for c in contigs])
    for ctg in contigs:
        got = bamref.Bam(os.path.join(out_dir, ctg + ".bam"))
        rs = s["reads"][ctg]
        assert len(got.records) == len(rs) and [r.pos for r in got.records] == rs.reads["pos"].tolist()
        assert got.text.count(b"@PG\tID:c3r_haplotag\tPN:clair3_rna_amd\tVN:c3r ") == 1 and b"\tCL:" in got.text
        if ctg == "chr1":
            tags, st, _ = hapref.haplotag(rs, s["case"][ctg][1])
            sets = hapcountref.read_phase_sets(rs, s["case"][ctg][1])
            assert 1 <= st["n_no_vote"] + st["n_tie"] <= 5 and 35 <= st["n_hp1"] <= 43 and 38 <= st["n_hp2"] <= 44
            assert [r.tag("HP")[1] if r.tag("HP") else 0 for r in got.records] == tags.tolist()
            assert [r.tag("PS")[1] if r.tag("PS") else -1 for r in got.records] == sets.tolist()
            assert all(r.tag("HP") is None or r.tag("HP")[0] == "C" for r in got.records)
        else:
            assert not any(t in PHASE for r in got.records for t, _, _ in r.aux)
        with bamio.BamFile(os.path.join(out_dir, ctg + ".bam")) as bf:
            assert bf.has_index and len(bf.fetch(ctg, 1000, 3000)) == int(((rs.reads["pos"] < 3000) & (_ends(rs) > 1000)).sum())


def _ends(rs):
    end = np.zeros(len(rs), np.int64)
    for i, r in enumerate(rs.reads):
        c = rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]
        end[i] = int(r["pos"]) + max(1, int((c >> 4)[np.isin(c & 15, (0, 2, 3, 7, 8))].sum()))
    return end


@pytest.mark.parametrize("tag_input", [False, True], ids=["untagged_input", "wrongly_tagged_input"])
def test_the_driver_writes_one_indexed_file_per_contig_with_records(tmp_path, monkeypatch, tag_input):
    from clair3_rna_amd import capi, haplotag_bam
    monkeypatch.setattr(capi, "Engine", StubEngine)
    StubEngine.loads = []
    s = two_contig_sample(str(tmp_path), tag_input)
    out_dir = str(tmp_path / "tagged")
    msgs = []
    done = haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--output_dir", out_dir, "--threads", "2"]),
                            log=msgs.append)
    assert sorted(done) == ["chr1", "chr2"] and StubEngine.loads == [len(s["reads"]["chr1"])]       # nothing is loaded for the contig without a phased site
    check_tagged_files(s, out_dir)
    assert done["chr1"]["stripped"] == (len(s["reads"]["chr1"]) if tag_input else 0) and done["chr2"]["tagged"] == 0
    assert len(msgs) == 3 and msgs[0].startswith("[INFO] chr1: %d records, %d HP1, %d HP2, " % (done["chr1"]["records"], done["chr1"]["hp1"], done["chr1"]["hp2"]))
    assert "every read untagged" in msgs[1] and msgs[2].startswith("[INFO] chrEmpty: no record")
    # --ctg_name: a listed contig without records gets no file; one VCF for all contigs is read like the directory
    import gzip
    one = str(tmp_path / "phased.vcf")
    with open(one, "w") as f:
        f.write(gzip.open(os.path.join(s["per"], "phased_chr1.vcf.gz"), "rt").read())
    listed = str(tmp_path / "listed")
    done = haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", one, "--output_dir", listed,
                                                                    "--ctg_name", "chrEmpty,chr1,chrNope"]), log=msgs.append)
    assert sorted(done) == ["chr1"]
    check_tagged_files(s, listed, ("chr1",))
    assert open(os.path.join(listed, "chr1.bam"), "rb").read() == open(os.path.join(out_dir, "chr1.bam"), "rb").read()


def test_a_failed_contig_leaves_no_partial_file(tmp_path, monkeypatch):
    from clair3_rna_amd import capi, haplotag_bam

    class Short(StubEngine):
        def haplotags(self):
            tags, st = StubEngine.haplotags(self)
            tags[3] = 7
            return tags, st

    monkeypatch.setattr(capi, "Engine", Short)
    s = two_contig_sample(str(tmp_path))
    out_dir = str(tmp_path / "tagged")
    with pytest.raises(IOError, match=r"hp\[3\] = 7"):
        haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--output_dir", out_dir]), log=lambda m: None)
    assert os.listdir(out_dir) == []


def test_call_sample_refuses_the_flag_where_it_cannot_work(tmp_path, monkeypatch):
    from clair3_rna_amd import call_sample
    base = ["--bam_fn", str(tmp_path / "x.bam"), "--ref_fn", str(tmp_path / "x.fa"), "--output_dir", str(tmp_path / "out"), "--pileup_model_path", "w18",
            "--phased_pileup_model_path", "w30", "--haplotagged_bam"]

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:
            call_sample.Run(call_sample.build_parser().parse_args(base + extra))
        assert str(e.value.code).startswith("[ERROR] --haplotagged_bam") and all(w in str(e.value.code) for w in words), e.value.code

    refused([], "--enable_phasing_model")
    refused(["--phasing", "builtin"], "--enable_phasing_model")
    refused(["--enable_phasing_model"], "--phased_vcf_fn", "--phasing builtin")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(["--enable_phasing_model", "--phased_vcf_fn", "p.vcf"], "WORLD_SIZE", "python -m clair3_rna_amd.haplotag_bam")
    refused(["--enable_phasing_model", "--phasing", "builtin"], "WORLD_SIZE", "python -m clair3_rna_amd.haplotag_bam")
    assert not os.path.exists(str(tmp_path / "out"))


def test_the_help_states_the_rule():
    from clair3_rna_amd import haplotag_bam
    text = " ".join(haplotag_bam.build_parser().format_help().split())
    for words in ("all loaded reads are tagged", "unit-weight", "CIGAR-position", "no realignment", "no base qualities", "has not been measured"):
        assert words in text, words


# ---- the same edge cases through the C ABI alone, from a stand-alone program (the one a sanitizer build runs)
def test_the_stand_alone_check_program(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/c/hapbam_check.cpp"
    csrc = os.path.join(ROOT, "clair3_rna_amd", "csrc")
    exe = str(tmp_path / "hapbam_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-pthread", os.path.join(ROOT, "tests", "c", "hapbam_check.cpp"),
                           os.path.join(csrc, "bamio.cpp"), os.path.join(csrc, "vcfio.cpp"), "-o", exe, "-lz"])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "hapbam_check: ok" in out.stdout, out.stdout + out.stderr
    assert os.listdir(str(tmp_path)) == ["hapbam_check"]                         # it removes what it wrote
