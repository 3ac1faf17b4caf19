"""tests/hapalleleref.py — the plain-Python restatement of the allele rule of include/c3r.h (c3r_hap_allele_counts) — pinned by hand-derived
known answers; phasing.allele_candidates_from_vcf / allele_phased_row against it and against answers written out by hand; and hap_vcf
--indels with a stand-in engine.  The GPU tests (tests/test_gpu_hapallele.py) compare the kernel with the same restatement."""
import gzip

import numpy as np
import pytest

from clair3_rna_amd import capi, hap_vcf, phasing
from clair3_rna_amd.reads import ReadSet
from tests import hapalleleref as HA
from tests import hapref

NONE = HA.NONE


def _rs(recs):
    """[(pos0, cigar, seq[, l_seq])] -> ReadSet (flag 0, MAPQ 60)."""
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=0, mapq=60, hp=0) for r in recs])
    for i, r in enumerate(recs):
        if len(r) > 3:
            rs.reads["l_seq"][i] = r[3]
    return rs


# ---- 1. allele reduction
@pytest.mark.parametrize("ref, alt, want", [
    ("ACC", "A", ("A", ("del", 2))), ("ACC", "TCC", ("T", NONE)),
    ("GG", "G", ("G", ("del", 1))), ("GG", "CG", ("C", NONE)),
    ("T", "TT", ("T", ("ins", "T"))), ("T", "TCAC", ("T", ("ins", "CAC"))),
    ("G", "GAA", ("G", ("ins", "AA"))), ("G", "GC", ("G", ("ins", "C"))),
    ("C", "T", ("T", NONE)), ("C", "CGG", ("C", ("ins", "GG"))),
    ("ACGT", "AT", ("A", ("del", 2))),                         # the suffix T goes: ACG / A
    ("ATT", "ATTT", ("A", ("ins", "T"))),                      # AT T / AT TT -> A / AT: only suffixes, the anchor stays POS
    ("acc", "a", ("A", ("del", 2))), ("g", "Gaa", ("G", ("ins", "AA"))), ("c", "t", ("T", NONE)),
    ("GTA", "GTAAA", None),                                    # an insertion behind the third base: not anchored on POS
    ("AC", "GT", None), ("ACC", "TC", None), ("A", "CAA", None), ("ACG", "C", None), ("A", "A", None), ("AC", "AC", None),
    ("A", "N", None), ("AN", "A", None), ("A", "<DEL>", None), ("A", "*", None), ("A", "AR", None), ("A", "", None),
])
def test_allele_reduction(ref, alt, want):
    assert HA.reduce(ref, alt) == want
    got = phasing.reduce_allele(ref, alt)
    if want is None:
        assert got is None
    else:
        kind = {"none": capi.HAP_EV_NONE, "ins": capi.HAP_EV_INS, "del": capi.HAP_EV_DEL}[want[1][0]]
        ins = want[1][1] if kind == capi.HAP_EV_INS else ""
        n = len(ins) if kind == capi.HAP_EV_INS else want[1][1] if kind == capi.HAP_EV_DEL else 0
        assert got == (want[0], kind, n, ins)


def test_the_alleles_and_flags_of_rows():
    s = HA.site_of_row(7, "ACC", "A,TCC", "1/2")
    assert (s["A"], s["B"], HA.flags(s)) == (("A", ("del", 2)), ("T", NONE), (True, True))
    s = HA.site_of_row(7, "GG", "G,CG", "2/1")
    assert (s["A"], s["B"], HA.flags(s)) == (("G", ("del", 1)), ("C", NONE), (True, True))
    s = HA.site_of_row(7, "T", "TT,TCAC", "1/2")
    assert (s["A"], s["B"], HA.flags(s)) == (("T", ("ins", "T")), ("T", ("ins", "CAC")), (False, True))
    s = HA.site_of_row(7, "G", "GAA,GC", "1/2")
    assert (s["A"], s["B"], HA.flags(s)) == (("G", ("ins", "AA")), ("G", ("ins", "C")), (False, True))
    s = HA.site_of_row(7, "C", "T,G", "1/2")
    assert (s["A"], s["B"], HA.flags(s)) == (("T", NONE), ("G", NONE), (True, False))
    s = HA.site_of_row(7, "c", "cgg", "0/1")
    assert (s["A"], s["B"], HA.flags(s)) == (("C", NONE), ("C", ("ins", "GG")), (False, True))
    s = HA.site_of_row(7, "C", "T", "1/0")
    assert (s["A"], s["B"], HA.flags(s)) == (("C", NONE), ("T", NONE), (True, False))
    assert HA.site_of_row(7, "AC", "A,GT", "1/2") == "complex_allele" and HA.site_of_row(7, "A", "AN", "0/1") == "complex_allele"
    assert HA.site_of_row(7, "A", "C,G", "0/1") == "multi_alt" and HA.site_of_row(7, "A", "C,G,T", "1/2") == "multi_alt"
    assert HA.site_of_row(7, "A", "C", "1/2") == "not_het" and HA.site_of_row(7, "A", "C", "1/1") == "not_het"
    assert HA.site_of_row(7, "ATT", "AT,ATT", "1/2") == "complex_allele" and HA.site_of_row(7, "AT", "A,A", "1/2") == "same_alleles"


# ---- 2. the normalised CIGAR
@pytest.mark.parametrize("cigar, want", [
    ("3H2M0I1P2M2H", "4M"), ("4M1P1D3M", "4M1P1D3M"), ("4M1I1P1I3M", "4M2I3M"), ("4M1I1P1D3M", "4M1I1D3M"), ("4M0D4M", "8M"),
    ("2S1I4M", "2S1I4M"), ("2=2X1M", "5M"), ("4M1P3P2D1M", "4M2P2D1M"), ("4M2P4M", "8M"), ("4M1I0M1P1D2M", "4M1I1D2M"), ("4M1P0M2H1D2M", "4M1P1D2M"),
])
def test_the_normalised_form(cigar, want):
    import re
    ops = [(o, int(n)) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    assert "".join("%d%s" % (n, o) for o, n in HA.normalise(ops)) == want


# ---- 3. counts, worked out by hand.  Reference (1-based 1..40): ACGT ten times; the table is one SNV, 3 G>C with GT 0|1 in set 5, so a read
# with G on position 3 is haplotype 1, with C haplotype 2, with T untagged.  All reads start on position 1.
H1, H2, H0 = "ACGTACGTAC", "ACCTACGTAC", "ACTTACGTAC"         # the first ten bases of a read of haplotype 1 / 2 / neither
TABLE = hapref.make_sites([(3, "G", "C", 0, 5)])


def test_an_insertion_site():
    site = HA.site_of_row(10, "C", "CTT", "0/1", ps=5)
    rs = _rs([(0, "10M2I5M", H1 + "TT" + "GTACG"),            # the insertion: B on haplotype 1
              (0, "15M", H2 + "GTACG"),                       # nothing behind the anchor: A on haplotype 2
              (0, "10M2I5M", H1 + "TA" + "GTACG"),            # one base differs: other, haplotype 1
              (0, "10M3I5M", H2 + "TTT" + "GTACG"),           # one base longer: other, haplotype 2
              (0, "10M2I5M", H0 + "TT" + "GTACG"),            # B, untagged
              (0, "10M2I1D4M", H1 + "TT" + "TACG"),           # an insertion with a deletion at once behind it: other, haplotype 1
              (0, "8M3D5M", H1[:8] + "TACGT"),                # the anchor lies under a deletion: nothing
              (0, "10M2D4M", H2 + "ACGT"),                    # a deletion: other, haplotype 2
              (0, "10M", H1),                                 # the read ends on the anchor: A, haplotype 1
              (0, "10M5N5M", H2 + "ACGTA"),                   # a ref-skip: A, haplotype 2
              (0, "10M2I5M", H1 + "TT" + "GTACG", 11),        # SEQ ends inside the insertion: nothing
              (0, "10M2I5M", H1[:9] + "N" + "TT" + "GTACG"),  # the anchor base does not matter here: B, haplotype 1
              (0, "10M1I1P1I5M", H2 + "TT" + "GTACG"),        # a run with a pad is one insertion of two: B, haplotype 2
              (0, "10M1I5M", H2 + "T" + "GTACG")])            # one base shorter: other, haplotype 2
    assert HA.counts(rs, TABLE, [site]).tolist() == [[[0, 1, 0], [1, 2, 2], [2, 1, 3]]]
    # against a phase set the reads are not tagged in, every read lands in row 0
    assert HA.counts(rs, TABLE, [dict(site, ps=6)]).tolist() == [[[3, 4, 5], [0, 0, 0], [0, 0, 0]]]


def test_a_deletion_site_and_the_sites_under_it():
    sites = [HA.site_of_row(10, "CGT", "C", "0/1", ps=5), HA.site_of_row(11, "G", "A", "0/1", ps=5), HA.site_of_row(12, "TA", "T", "0/1", ps=5)]
    rs = _rs([(0, "10M2D3M", H1 + "ACG"),                     # DEL 2: B; 11 and 12 lie under it: nothing
              (0, "10M1D4M", H2 + "TACG"),                    # DEL 1: other; 11 under it; 12 (T, then A): A
              (0, "10M3D2M", H1 + "CG"),                      # DEL 3: other; 11, 12 under it
              (0, "15M", H2 + "ATACG"),                       # no event: A; 11 shows A: B; 12: A
              (0, "10M1P2D3M", H1 + "ACG"),                   # a pad before the D: no event, A; 11, 12 under the deletion
              (0, "12M1D2M", H2 + "GT" + "CG"),               # 10: A; 11 G: A; 12 DEL 1: B
              (0, "11M1I4M", H1 + "C" + "T" + "TACG")])       # 10: A; 11 shows C behind it an insertion: other (a third base); 12: A
    assert HA.counts(rs, TABLE, sites).tolist() == [[[0, 0, 0], [2, 1, 1], [2, 0, 1]],
                                                    [[0, 0, 0], [0, 0, 1], [1, 1, 0]],
                                                    [[0, 0, 0], [1, 0, 0], [2, 1, 0]]]


def test_a_mixed_site():
    site = HA.site_of_row(9, "ACG", "A,TCG", "1/2", ps=5)    # A = (A, DEL 2), B = (T, no event)
    rs = _rs([(0, "15M", H1 + "GTACG"),                       # the reference allele: other, haplotype 1
              (0, "9M2D4M", H1[:9] + "TACG"),                 # A, then DEL 2: allele A, haplotype 1
              (0, "15M", H2[:8] + "TC" + "GTACG"),            # T, no event: allele B, haplotype 2
              (0, "9M2D4M", H2[:8] + "G" + "TACG"),           # DEL 2 behind a G: other, haplotype 2
              (0, "15M", H1[:8] + "CC" + "GTACG"),            # C, no event: other, haplotype 1
              (0, "9M2D4M", H1[:8] + "N" + "TACG"),           # N on the anchor of a site whose base matters: nothing
              (0, "9M3D3M", H2[:9] + "ACG"),                  # DEL 3: other, haplotype 2
              (0, "9M1D5M", H2[:9] + "GTACG"),                # DEL 1: other, haplotype 2
              (0, "9M2D4M", H1[:8] + "T" + "TACG")])          # T with DEL 2: neither, haplotype 1
    assert HA.counts(rs, TABLE, [site]).tolist() == [[[0, 0, 0], [1, 0, 3], [0, 1, 3]]]


def test_odd_cigar_forms_and_short_reads():
    site = HA.site_of_row(8, "T", "TG", "0/1", ps=5)
    rs = _rs([(0, "4M0D4M1I2M", H1[:8] + "G" + "AC"),         # 4M0D4M is 8M: B
              (0, "3H4=4X1I2M2H", H2[:8] + "G" + "AC"),        # = and X fold into one M: B
              (0, "8M1I", H1[:8] + "G"),                      # the insertion ends the read: B
              (0, "8M1I2S", H2[:8] + "G" + "TT"),             # ... before a soft clip: B
              (0, "7M1I1M", H1[:7] + "G" + "T"),              # the insertion sits one base earlier: A
              (0, "8M1I2M", H1[:8] + "G" + "AC", 8),          # l_seq 8: the anchor is the last base, the insertion is cut off: nothing
              (0, "8M1I2M", H1[:8] + "G" + "AC", 7),          # l_seq 7: the anchor base itself is missing: nothing
              (5, "2S1I3M1I2M", "TTG" + "CGT" + "G" + "AC")])  # a leading 2S1I: the first M starts on position 6; B, untagged
    assert HA.counts(rs, TABLE, [site]).tolist() == [[[0, 1, 0], [1, 2, 0], [0, 2, 0]]]


def test_an_snv_only_site_is_todays_rule():
    from tests import hapcountref as HC
    # an SNV on the last base before an insertion that a short SEQ cuts off: today's rule counts the base, and so does this one —
    # while an insertion site on the same position sees nothing
    rs = _rs([(0, "8M2I2M", H1[:8] + "GG" + "AC", 9)])
    query = HC.make_query([(8, "T", "G", 5)])
    assert HC.hap_counts(rs, TABLE, query).tolist() == [[[0, 0, 0], [1, 0, 0], [0, 0, 0]]]
    assert HA.counts(rs, TABLE, HA.snv_sites(query)).tolist() == [[[0, 0, 0], [1, 0, 0], [0, 0, 0]]]
    assert HA.counts(rs, TABLE, [HA.site_of_row(8, "T", "TGG", "0/1", ps=5)]).sum() == 0
    for seed in range(2):
        _, rs, table, _ = hapref.gen_case(seed, n_reads=120)
        query = table.copy()
        query["h1"] = 0
        assert np.array_equal(HA.counts(rs, table, HA.snv_sites(query)), HC.hap_counts(rs, table, query))


# ---- 4. candidates, the row rewrite, hap_vcf's writer
HEADER = ["##fileformat=VCFv4.2\n", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"]
ROWS = ["chr1\t10\t.\tC\tCTT\t20\tPASS\tF\tGT:GQ\t0/1:20\n",             # 0 insertion
        "chr1\t20\t.\tACC\tA,TCC\t20\tPASS\tF\tGT:GQ\t1/2:20\n",          # 1 two ALTs
        "chr1\t30\t.\tg\tt\t20\tPASS\tF\tGQ:GT\t20:1/0\n",               # 2 a lower-case SNV, GT second
        "chr1\t40\t.\tGA\tG\t20\tPASS\tF\tGT:GQ\t1/1:20\n",              # 3 homozygous
        "chr1\t50\t.\tC\tT\t3\tLowQual\tF\tGT:GQ\t0/1:3\n",              # 4 not PASS
        "chr1\t60\t.\tAC\tGT\t20\tPASS\tF\tGT:GQ\t0/1:20\n",             # 5 complex
        "chr1\t70\t.\tA\tC,G,T\t20\tPASS\tF\tGT:GQ\t1/2:20\n",           # 6 three ALTs
        "chr1\t80\t.\tT\tTT,TCAC\t20\tPASS\tF\tGT:GQ\t2/1:20\n",         # 7 two insertions
        "chr1\t80\t.\tT\tG\t20\tPASS\tF\tGT:GQ\t0/1:20\n",               # 8 a second row on 80
        "chr1\t90\t.\tA\tAN\t20\tPASS\tF\tGT:GQ\t0/1:20\n",              # 9 a letter outside ACGT
        "chr1\t95\t.\tCGT\tC\t20\tPASS\tF\tGT:GQ\t0/1:20\n",             # 10 deletion
        "chr1\t97\t.\tAT\tA,A\t20\tPASS\tF\tGT:GQ\t1/2:20\n",            # 11 two equal ALTs
        "chr1\tx\t.\tA\tC\t20\tPASS\tF\tGT:GQ\t0/1:20\n",                # 12 malformed
        "chr2\t15\t.\tG\tGAA,GC\t20\tPASS\tF\tGT:GQ\t1/2:20\n",          # 13
        "chr2\t5\t.\tGG\tG,CG\t20\tPASS\tF\tGT:GQ\t1/2:20\n"]            # 14 out of order: sorted by pos


def _vcf(tmp_path, gz=False):
    fn = str(tmp_path / ("in.vcf.gz" if gz else "in.vcf"))
    with (gzip.open(fn, "wt") if gz else open(fn, "w")) as f:
        f.writelines(HEADER + ROWS)
    return fn


def _query_as_sites(query, pool, strings):
    """A HAP_SITE_DTYPE array and its packed pool back as the restatement's sites."""
    out = []
    for s, (ref, alt) in zip(query, strings):
        d = dict(pos=int(s["pos"]), ps=int(s["ps"]), ref=ref, alt=alt)
        for name in "ab":
            kind, n, off = int(s[name + "_kind"]), int(s[name + "_len"]), int(s[name + "_ins_off"])
            codes = [(int(pool[(off + k) // 2]) >> (0 if (off + k) % 2 else 4)) & 15 for k in range(n)] if kind == capi.HAP_EV_INS else []
            ev = NONE if kind == capi.HAP_EV_NONE else ("ins", "".join(HA.LETTER[c] for c in codes)) if kind == capi.HAP_EV_INS else ("del", n)
            d[name.upper()] = (HA.LETTER[int(s[name + "_base"])], ev)
        assert (int(s["base_matters"]), int(s["event_matters"])) == tuple(int(v) for v in HA.flags(d)) and not s["reserved"].any()
        out.append(d)
    return out


def test_candidate_selection(tmp_path):
    fn = _vcf(tmp_path)
    sites, skipped = HA.candidates(HEADER + ROWS, "chr1")
    assert [s["pos"] for s in sites] == [10, 20, 30, 80, 95]
    assert skipped == dict(other_contig=2, malformed=1, not_pass=1, not_snv=0, not_het=1, duplicate_pos=1, multi_alt=1, complex_allele=2, same_alleles=1)
    assert sites[3]["A"] == ("T", ("ins", "T")) and sites[3]["B"] == ("T", ("ins", "CAC")) and sites[2]["B"] == ("T", NONE)
    query, pool, strings, got_skipped = phasing.allele_candidates_from_vcf(fn, "chr1")
    assert query.dtype == capi.HAP_SITE_DTYPE and pool.dtype == np.uint8 and got_skipped == skipped and (query["ps"] == 0).all()
    assert strings == [("C", "CTT"), ("ACC", "A,TCC"), ("g", "t"), ("T", "TT,TCAC"), ("CGT", "C")]
    assert _query_as_sites(query, pool, strings) == sites
    assert query["a_ins_off"].tolist() == [0, 0, 0, 2, 0] and query["b_ins_off"].tolist() == [0, 0, 0, 3, 0] and len(pool) == 3     # TT | T | CAC
    # every contig in one pass, a gzipped file, a contig the file does not have
    per = phasing.allele_candidates_from_vcf(_vcf(tmp_path, gz=True), None)
    assert sorted(per) == ["chr1", "chr2"] and per["chr1"][0].tobytes() == query.tobytes() and per["chr1"][3] == dict(skipped, other_contig=0)
    chr2, _ = HA.candidates(HEADER + ROWS, "chr2")
    assert [s["pos"] for s in chr2] == [5, 15] and _query_as_sites(*per["chr2"][:3]) == chr2 and per["chr2"][2] == [("GG", "G,CG"), ("G", "GAA,GC")]
    none = phasing.allele_candidates_from_vcf(fn, "chr9")
    assert len(none[0]) == 0 and len(none[1]) == 0 and none[2] == [] and none[3]["other_contig"] == 15
    # the SNV-only parser keeps its output
    old, old_skipped = phasing.candidates_from_vcf(fn, "chr1")
    assert old["pos"].tolist() == [30, 80] and sorted(old_skipped) == sorted(phasing.SKIP_REASONS) and old_skipped["not_snv"] == 9


@pytest.mark.parametrize("row, gt, h1, want", [(0, "0/1", 0, "0|1"), (0, "1/0", 1, "1|0"), (1, "1/2", 0, "1|2"), (1, "2/1", 1, "2|1"),
                                               (0, "1/0", 0, "0|1"), (1, "2/1", 0, "1|2"), (2, "1/0", 1, "1|0")])
def test_the_row_rewrite(row, gt, h1, want):
    f = ROWS[row].rstrip("\n").split("\t")
    keys, vals = f[8].split(":"), f[9].split(":")
    vals[keys.index("GT")] = gt
    f[9] = ":".join(vals)
    line = "\t".join(f) + "\n"
    site = HA.site_of_row(int(f[1]), f[3], f[4], gt)
    table = {int(f[1]): (f[3], f[4], 77, h1)}
    text, done = phasing.allele_phased_row(line, f, table)
    assert done and text == HA.rewritten(line, site, (77, h1)) and not table
    out = text.rstrip("\n").split("\t")
    assert out[:8] == f[:8] and out[8] == f[8] + ":PS" and out[9] == f[9].replace(gt, want) + ":77"
    assert phasing.allele_phased_row(line, f, table) == (line, False)              # the site has left the table


def test_rows_the_rewrite_leaves_alone():
    for k, (line, entry) in enumerate([(ROWS[0], ("C", "CT", 7, 0)), (ROWS[0], ("c", "CTT", 7, 0)), (ROWS[1], ("ACC", "A", 7, 0)),
                                       (ROWS[3], ("GA", "G", 7, 0)), (ROWS[4], ("C", "T", 7, 0)), (ROWS[1].replace("1/2", "0/1"), ("ACC", "A,TCC", 7, 0)),
                                       (ROWS[0].replace("0/1", "1/2"), ("C", "CTT", 7, 0)), (ROWS[0].replace("0/1", "0|1"), ("C", "CTT", 7, 0)),
                                       (ROWS[0].replace("GT:GQ\t0/1:20", "GT:PS\t0/1:3"), ("C", "CTT", 7, 0)), (ROWS[12], ("A", "C", 7, 0)),
                                       (ROWS[0].replace("\n", "\r\n").replace("\tPASS", "\tq10"), ("C", "CTT", 7, 0))]):
        f = line.rstrip("\r\n").split("\t")
        table = {int(f[1]) if f[1].isdigit() else 0: entry}
        assert phasing.allele_phased_row(line, f, dict(table)) == (line, False), k
    line = ROWS[0].replace("\n", "\r\n")
    assert phasing.allele_phased_row(line, line.rstrip("\r\n").split("\t"), {10: ("C", "CTT", 7, 1)})[0] == "chr1\t10\t.\tC\tCTT\t20\tPASS\tF\tGT:GQ:PS\t1|0:20:7\r\n"


def test_the_writer_and_the_counts_lines(tmp_path):
    fn, out = _vcf(tmp_path), str(tmp_path / "out.vcf")
    query, pool, strings, _ = phasing.allele_candidates_from_vcf(fn, "chr1")
    assigned = capi.hap_site_keys(query)
    assigned["ps"], assigned["h1"] = [4, 4, -1, 9, 9], [1, 0, 0, 1, 0]
    assert hap_vcf.write_vcf(fn, {"chr1": assigned}, out, {"chr1": strings}) == 4
    want = list(ROWS)
    want[0] = "chr1\t10\t.\tC\tCTT\t20\tPASS\tF\tGT:GQ:PS\t1|0:20:4\n"
    want[1] = "chr1\t20\t.\tACC\tA,TCC\t20\tPASS\tF\tGT:GQ:PS\t1|2:20:4\n"
    want[7] = "chr1\t80\t.\tT\tTT,TCAC\t20\tPASS\tF\tGT:GQ:PS\t2|1:20:9\n"
    want[10] = "chr1\t95\t.\tCGT\tC\t20\tPASS\tF\tGT:GQ:PS\t0|1:20:9\n"
    assert open(out).read() == HEADER[0] + phasing.PS_HEADER + HEADER[1] + "".join(want)
    q = query.copy()
    q["ps"] = [4, 4, 4, 9, 9]
    c = np.arange(45, dtype=np.uint32).reshape(5, 3, 3)
    lines = hap_vcf.allele_counts_lines("chr1", q, strings, assigned, c)
    assert lines[0] == "chr1\t10\tC\tCTT\t4\t1|0\t3\t4\t5\t6\t7\t8\t0\t1\t2\t0,1\n"
    assert lines[1] == "chr1\t20\tACC\tA,TCC\t4\t1|2\t12\t13\t14\t15\t16\t17\t9\t10\t11\t1,2\n"
    assert lines[2] == "chr1\t30\tg\tt\t4\t0/1\t21\t22\t23\t24\t25\t26\t18\t19\t20\t0,1\n"
    assert lines[3].split("\t")[5] == "2|1" and lines[3].endswith("\t1,2\n")
    sites = HA.nearest_sets(HA.candidates(HEADER + ROWS, "chr1")[0], np.array([(1, 4), (85, 9)], dtype=[("pos", "i4"), ("ps", "i4")]))
    decided = [(int(a["ps"]), int(a["h1"])) for a in assigned]
    assert lines == [HA.counts_line("chr1", s, d, t) for s, d, t in zip(sites, decided, c)]
    assert hap_vcf.ALLELE_COLUMNS == hap_vcf.COLUMNS + ("ALLELES",)


def test_nearest_sets_takes_both_kinds_of_candidates():
    table = hapref.make_sites([(12, "A", "C", 0, 3), (40, "A", "C", 0, 8)])
    q = np.zeros(3, capi.HAP_SITE_DTYPE)
    q["pos"] = [1, 26, 27]
    assert hap_vcf.nearest_sets(q, table)["ps"].tolist() == [3, 3, 8]


# ---- 5. hap_vcf --indels from end to end with a stand-in engine that counts by the restatement
class _Engine(object):
    """Stands in for capi.Engine: what hap_vcf.Run calls, the counts computed by tests/hapalleleref.py from the query it is handed."""
    strings = None

    def __init__(self, device=0):
        self.calls = []

    def set_params(self, **kw):
        self.kw = kw

    def set_phase_sites(self, table):
        self.table = table

    def load_reads(self, rs):
        self.rs = rs

    def hap_allele_counts(self, query, pool):
        self.calls.append("alleles")
        return HA.counts(self.rs, self.table, _query_as_sites(query, pool, _Engine.strings))

    def hap_counts(self, query):
        from tests import hapcountref as HC
        self.calls.append("snvs")
        return HC.hap_counts(self.rs, self.table, query)

    def close(self):
        pass


def test_hap_vcf_with_and_without_indels_on_a_stand_in_engine(tmp_path, monkeypatch):
    from clair3_rna_amd import io
    h1t = H1[:5] + "T" + H1[6:]                              # haplotype 1 carries T on position 6
    rs = _rs([(0, "10M2I5M", h1t + "TT" + "GTACG"), (0, "10M2I5M", h1t + "TT" + "GTACG"), (0, "15M", H2 + "GTACG"), (0, "15M", H2 + "GTACG"),
              (0, "15M", h1t + "GTACG"), (0, "15M", h1t + "GTACG"), (0, "10M2I5M", H2 + "TT" + "GTACG")])
    rows = ["chr1\t6\t.\tC\tT\t20\tPASS\tF\tGT\t0/1\n", "chr1\t10\t.\tC\tCTT\t20\tPASS\tF\tGT\t0/1\n", "chr1\t12\t.\tT\tA,C\t20\tPASS\tF\tGT\t1/2\n",
            "chr7\t3\t.\tA\tAT\t20\tPASS\tF\tGT\t0/1\n"]
    vcf, tab = str(tmp_path / "in.vcf"), str(tmp_path / "phased.vcf")
    with open(vcf, "w") as f:
        f.writelines(HEADER + rows)
    with open(tab, "w") as f:
        f.writelines(HEADER + ["chr1\t3\t.\tG\tC\t20\tPASS\tF\tGT:PS\t0|1:5\n"])
    monkeypatch.setattr(capi, "Engine", _Engine)
    monkeypatch.setattr(io, "load_reads", lambda bam, ctg: rs)
    out = {}
    for name, extra in (("plain", []), ("indels", ["--indels"])):
        _Engine.strings = phasing.allele_candidates_from_vcf(vcf, "chr1")[2]
        msgs = []
        o, t = str(tmp_path / (name + ".vcf")), str(tmp_path / (name + ".tsv"))
        n = hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", vcf, "--vcf_fn", vcf, "--phased_vcf_fn", tab, "--output_fn", o, "--hap_counts_fn", t] + extra),
                        log=msgs.append)
        out[name] = (n, open(o).read(), open(t).read(), msgs)
    # without the flag: the SNV on 6 alone (the four reads of haplotype 1 show T, the three of haplotype 2 C: 1|0), 15 columns
    n, text, tsv, msgs = out["plain"]
    assert n == 1 and "chr1\t6\t.\tC\tT\t20\tPASS\tF\tGT:PS\t1|0:5\n" in text and rows[1] in text and rows[2] in text and rows[3] in text
    assert tsv == "\t".join(hap_vcf.COLUMNS) + "\n" + "chr1\t6\tC\tT\t5\t1|0\t0\t4\t0\t3\t0\t0\t0\t0\t0\n"
    assert len(msgs) == 2 and "not_snv 2" in msgs[0] and "SNV candidates: rows copied unchanged" in msgs[1]
    # with it: the insertion on 10 (haplotype 1: two with it and two without, haplotype 2: two without, one with — 3 : 4, no agreement) stays,
    # 12 (every read shows the reference's T: other) has no tagged observation of A or B and stays
    n, text, tsv, msgs = out["indels"]
    assert n == 1 and text == out["plain"][1]
    assert tsv == ("\t".join(hap_vcf.ALLELE_COLUMNS) + "\n" + "chr1\t6\tC\tT\t5\t1|0\t0\t4\t0\t3\t0\t0\t0\t0\t0\t0,1\n"
                   + "chr1\t10\tC\tCTT\t5\t0/1\t2\t2\t0\t2\t1\t0\t0\t0\t0\t0,1\n" + "chr1\t12\tT\tA,C\t5\t1/2\t0\t0\t4\t0\t0\t3\t0\t0\t0\t1,2\n")
    assert len(msgs) == 2 and "3 candidate sites (none skipped)" in msgs[0] and "1 without agreement" in msgs[0] and "1 with too few tagged reads" in msgs[0]
    assert "SNV / indel / two-ALT candidates: rows copied unchanged" in msgs[1]


def test_an_insertion_and_a_two_alt_row_the_tagged_reads_agree_on_are_written_phased(tmp_path, monkeypatch):
    from clair3_rna_amd import io
    # 10 C>CTT: the insertion on two reads of haplotype 2, none on two of haplotype 1 and one of haplotype 2: 4 : 1, B on haplotype 2: 0|1.
    # 11 GTA>G,GAATA (A = DEL 2, B = an insertion of AA behind 11): A on a read of haplotype 1, B on one of haplotype 2: A|B = 1|2
    rs = _rs([(0, "10M2I5M", H2 + "TT" + "GTACG"), (0, "10M2I5M", H2 + "TT" + "GTACG"), (0, "15M", H1 + "GTACG"), (0, "11M2D2M", H1 + "G" + "CG"),
              (0, "11M2I4M", H2 + "G" + "AA" + "TACG")])
    rows = ["chr1\t10\t.\tC\tCTT\t20\tPASS\tF\tGT\t0/1\n", "chr1\t11\t.\tGTA\tG,GAATA\t20\tPASS\tF\tGT:DP\t2/1:5\n"]
    vcf, tab = str(tmp_path / "in.vcf"), str(tmp_path / "phased.vcf")
    with open(vcf, "w") as f:
        f.writelines(HEADER + rows)
    with open(tab, "w") as f:
        f.writelines(HEADER + ["chr1\t3\t.\tG\tC\t20\tPASS\tF\tGT:PS\t0|1:5\n"])
    monkeypatch.setattr(capi, "Engine", _Engine)
    monkeypatch.setattr(io, "load_reads", lambda bam, ctg: rs)
    _Engine.strings = phasing.allele_candidates_from_vcf(vcf, "chr1")[2]
    o, t = str(tmp_path / "out.vcf"), str(tmp_path / "out.tsv")
    assert hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", vcf, "--vcf_fn", vcf, "--phased_vcf_fn", tab, "--output_fn", o, "--hap_counts_fn", t, "--indels"]),
                       log=lambda m: None) == 2
    assert open(o).read() == (HEADER[0] + phasing.PS_HEADER + HEADER[1] + "chr1\t10\t.\tC\tCTT\t20\tPASS\tF\tGT:PS\t0|1:5\n"
                              + "chr1\t11\t.\tGTA\tG,GAATA\t20\tPASS\tF\tGT:DP:PS\t1|2:5:5\n")
    assert open(t).read() == ("\t".join(hap_vcf.ALLELE_COLUMNS) + "\n" + "chr1\t10\tC\tCTT\t5\t0|1\t2\t0\t0\t1\t2\t0\t0\t0\t0\t0,1\n"
                              + "chr1\t11\tGTA\tG,GAATA\t5\t1|2\t1\t0\t1\t0\t1\t2\t0\t0\t0\t1,2\n")
