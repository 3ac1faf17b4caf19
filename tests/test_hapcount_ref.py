"""tests/hapcountref.py — the plain-Python restatement of the per-haplotype allele counts (include/c3r.h: c3r_get_read_phase_sets,
c3r_hap_counts, c3r_hap_assign) — pinned by hand-derived known answers; c3r_hap_assign (host code, no GPU) and hap_vcf's nearest-set rule
against it; and the writers of hap_vcf.  The GPU tests (tests/test_gpu_hapcount.py) compare the kernels with the same restatement."""
import ctypes as C
import gzip
import os
import random

import numpy as np
import pytest

from clair3_rna_amd import capi, hap_vcf, phasedvcf, phasing
from clair3_rna_amd.reads import ReadSet
from tests import hapcountref as HC
from tests import hapref


def _rs(recs):
    """[(pos0, cigar, seq[, flag[, mapq[, l_seq]]])] -> ReadSet."""
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=r[4] if len(r) > 4 else 60, hp=0) for r in recs])
    for i, r in enumerate(recs):
        if len(r) > 5:
            rs.reads["l_seq"][i] = r[5]
    return rs


def _rows(counts):
    """{site index: {(row, column): count}} of the non-zero entries."""
    out = {}
    for j, t, a in np.argwhere(counts):
        out.setdefault(int(j), {})[(int(t), int(a))] = int(counts[j, t, a])
    return out


# ---- 1. known answers, worked out by hand from the rule
def test_every_base_class_and_the_first_and_last_base():
    # 0-based 10, 8M: 1-based 11..18 carry A C G = N R T A.  Table: 11 A>C 0|1 in set 7 — the read shows REF there: haplotype 1, set 7
    rs = _rs([(10, "8M", "ACG=NRTA")])
    table = hapref.make_sites([(11, "A", "C", 0, 7)])
    assert HC.read_phase_sets(rs, table).tolist() == [7]
    query = HC.make_query([(10, "A", "C", 7), (11, "A", "C", 7), (12, "C", "T", 7), (13, "A", "G", 7), (14, "A", "C", 7), (15, "A", "C", 7),
                           (16, "A", "G", 7), (17, "A", "C", 7), (18, "C", "G", 7), (19, "A", "C", 7)])
    got = _rows(HC.hap_counts(rs, table, query))
    # 10 and 19 lie just outside; 14 (=), 15 (N) and 16 (R: IUPAC) show nothing; 17 (T) and 18 (A) show a third base
    assert got == {1: {(1, 0): 1}, 2: {(1, 0): 1}, 3: {(1, 1): 1}, 7: {(1, 2): 1}, 8: {(1, 2): 1}}


def test_deletions_ref_skips_insertions_and_soft_clips():
    # 0-based 10: 2S | 2M 11 12 "AC" | 2D 13 14 | 2M 15 16 "GT" | 2I "AA" | 2M 17 18 "CA" | 10N 19..28 | 2M 29 30 "GG"
    rs = _rs([(10, "2S2M2D2M2I2M10N2M", "TT" "AC" "GT" "AA" "CA" "GG")])
    table = hapref.make_sites([(11, "A", "C", 1, 3)])          # REF under GT 1|0: haplotype 2
    assert HC.read_phase_sets(rs, table).tolist() == [3]
    query = HC.make_query([(9, "T", "A", 3), (10, "T", "A", 3), (11, "A", "C", 3), (12, "C", "A", 3), (13, "A", "C", 3), (14, "A", "C", 3),
                           (15, "A", "G", 3), (16, "T", "A", 3), (17, "A", "G", 3), (18, "A", "C", 3), (19, "A", "C", 3), (28, "A", "C", 3),
                           (29, "G", "A", 3), (30, "A", "G", 3), (31, "G", "A", 3)])
    got = _rows(HC.hap_counts(rs, table, query))
    # soft clips (9, 10), the deletion (13, 14), the skip (19, 28) and 31 show nothing; 17 is the C after the insertion, not an inserted A
    assert got == {2: {(2, 0): 1}, 3: {(2, 0): 1}, 6: {(2, 1): 1}, 7: {(2, 0): 1}, 8: {(2, 2): 1}, 9: {(2, 0): 1}, 12: {(2, 0): 1}, 13: {(2, 1): 1}}


def test_l_seq_shorter_than_the_cigar():
    rs = _rs([(0, "6M", "AACC", 0, 60, 3)])                     # the fourth nibble holds a C that is not part of the read
    table = hapref.make_sites([(1, "A", "C", 0, 1)])
    query = HC.make_query([(p, "A", "C", 1) for p in range(1, 7)])
    assert _rows(HC.hap_counts(rs, table, query)) == {0: {(1, 0): 1}, 1: {(1, 0): 1}, 2: {(1, 1): 1}}


def test_a_read_tagged_in_another_set_and_a_tied_read_land_in_row_0():
    # set 9 on 1 and 3 (A, A: 2 : 0), set 3 on 2 (C: 0 : 1): the read is haplotype 1 of set 9
    rs = _rs([(0, "4M", "ACAC")])
    table = hapref.make_sites([(1, "A", "C", 0, 9), (2, "A", "C", 0, 3), (3, "A", "C", 0, 9)])
    assert HC.read_phase_sets(rs, table).tolist() == [9]
    assert _rows(HC.hap_counts(rs, table, HC.make_query([(4, "C", "A", 3)]))) == {0: {(0, 0): 1}}
    assert _rows(HC.hap_counts(rs, table, HC.make_query([(4, "C", "A", 9)]))) == {0: {(1, 0): 1}}
    # 1 : 1 in its only set: tag 0, no set
    tied = _rs([(0, "3M", "ACA")])
    table = hapref.make_sites([(1, "A", "C", 0, 1), (2, "A", "C", 0, 1)])
    assert HC.read_phase_sets(tied, table).tolist() == [-1]
    assert _rows(HC.hap_counts(tied, table, HC.make_query([(3, "A", "G", 1)]))) == {0: {(0, 0): 1}}
    # no vote at all
    none = _rs([(0, "3M", "GGA")])
    assert HC.read_phase_sets(none, table).tolist() == [-1]
    assert _rows(HC.hap_counts(none, table, HC.make_query([(3, "A", "G", 1)]))) == {0: {(0, 0): 1}}


def test_a_filtered_read_is_tagged_and_not_counted():
    recs = [(0, "2M", "AC"), (0, "2M", "AC", 0, 0), (0, "2M", "AC", 256), (0, "2M", "AC", 2048), (0, "2M", "AC", 4), (0, "2M", "AC", 1), (0, "2M", "CC", 16)]
    rs = _rs(recs)
    table = hapref.make_sites([(1, "A", "C", 0, 5)])
    assert HC.read_phase_sets(rs, table).tolist() == [5] * 7                      # (every loaded read is tagged, whatever the filters say)
    query = HC.make_query([(2, "C", "G", 5)])
    assert _rows(HC.hap_counts(rs, table, query)) == {0: {(1, 0): 1, (2, 0): 1}}  # the first and the last read
    assert _rows(HC.hap_counts(rs, table, query, dict(min_mq=0, excl_flags=0))) == {0: {(1, 0): 4, (2, 0): 1}}   # (unmapped and the anomalous pair never)


SETS = {"equal_sets_earlier_first_site_wins": [9], "equal_sets_earlier_first_site_wins_2": [3], "later_set_with_more_votes_wins": [6],
        "interleaved_sets": [1], "first_VOTING_site_counts": [8], "one_to_one_tie": [-1], "just_outside_the_read": [-1], "iupac_base": [-1],
        "two_reads": [1, 1], "first_and_last_base": [7]}


@pytest.mark.parametrize("name", sorted(SETS))
def test_read_phase_sets_of_the_haplotagging_cases(name):
    case = [c for c in hapref.CASES if c[0] == name][0]
    rs, table = hapref.case_inputs(case)
    assert HC.read_phase_sets(rs, table).tolist() == SETS[name]


def test_every_haplotagging_case_has_a_set_exactly_when_it_has_a_tag():
    for case in hapref.CASES:
        rs, table = hapref.case_inputs(case)
        ps = HC.read_phase_sets(rs, table)
        assert [p >= 0 for p in ps.tolist()] == [e[0] != 0 for e in case[3]], case[0]
        assert all(p < 0 or p in table["ps"].tolist() for p in ps.tolist())


# ---- 2. c3r_hap_assign against the restatement
def _table(rows):
    """[(hp1_ref, hp1_alt, hp2_ref, hp2_alt)] -> (query, counts)."""
    q = HC.make_query([(10 + 3 * k, "A", "C", 100 + k % 3) for k in range(len(rows))])
    c = np.zeros((len(rows), 3, 3), dtype=np.uint32)
    for k, r in enumerate(rows):
        c[k, 1, 0], c[k, 1, 1], c[k, 2, 0], c[k, 2, 1] = r
    return q, c


def test_assignment_known_answers():
    M = 0xffffffff
    q, c = _table([(0, 1, 0, 0), (1, 3, 0, 0), (1, 2, 0, 0), (2, 2, 0, 0), (0, 0, 1, 1), (1, 0, 0, 2), (0, 1, 1, 0), (M, M, M, 0), (0, 0, 0, 0)])
    want = [(-1, 0), (101, 1), (-1, 0), (-1, 0), (-1, 0), (102, 0), (100, 1), (-1, 0), (-1, 0)]
    stats = dict(n_sites=9, n_phased=3, n_few_reads=2, n_disagree=4)
    for fn in (HC.assign, capi.hap_assign):
        out, st = fn(q, c)
        assert list(zip(out["ps"].tolist(), out["h1"].tolist())) == want and st == stats, fn
        assert out["pos"].tolist() == q["pos"].tolist() and out["ref"].tolist() == q["ref"].tolist() and out["alt"].tolist() == q["alt"].tolist()
        # near 2^32: v1 = 2^33 - 2 against v0 = 2^32 - 1 is 66.7 % — and ALT on haplotype 1 only in sums that do not wrap
        out, st = fn(q[7:8], c[7:8], 2, 66)
        assert (int(out["ps"][0]), int(out["h1"][0])) == (101, 1) and st["n_phased"] == 1, fn
        out, st = fn(q[7:8], c[7:8], 2, 67)
        assert int(out["ps"][0]) == -1 and st["n_disagree"] == 1, fn
        # 3 : 1 is exactly 75 %; min_reads 5 turns it away for too few reads, 0 lets the empty site fail on v0 == v1
        assert fn(q[1:2], c[1:2], 5, 75)[1]["n_few_reads"] == 1 and fn(q[8:9], c[8:9], 0, 0)[1]["n_disagree"] == 1


def test_the_unphased_row_and_the_third_base_column_never_decide():
    q, c = _table([(0, 3, 1, 0), (2, 0, 0, 2), (1, 1, 0, 0)])
    plain = capi.hap_assign(q, c)
    c[:, 0, :] = 1000
    c[:, :, 2] = 4000000000
    noisy = capi.hap_assign(q, c)
    assert plain[1] == noisy[1] == HC.assign(q, c)[1] and plain[0].tobytes() == noisy[0].tobytes() == HC.assign(q, c)[0].tobytes()
    assert plain[0]["ps"].tolist() == [100, 101, -1] and plain[0]["h1"].tolist() == [1, 0, 0]


@pytest.mark.parametrize("seed, min_reads, pct", [(0, 2, 75), (1, 1, 100), (2, 4, 60), (3, 0, 0), (4, 3, 51)])
def test_assignment_of_random_tables(seed, min_reads, pct):
    rng = random.Random(seed)
    n = 2000
    q = HC.make_query([(5 + 2 * k, "A", "G", rng.randrange(1, 50)) for k in range(n)])
    c = np.zeros((n, 3, 3), dtype=np.uint32)
    for k in range(n):
        top = rng.choice([1, 2, 3, 6, 40, 0xffffffff])
        for t in range(3):
            for a in range(3):
                c[k, t, a] = rng.randint(0, top) if rng.random() < 0.7 else 0
    out, st = capi.hap_assign(q, c, min_reads, pct)
    want, wst = HC.assign(q, c, min_reads, pct)
    assert st == wst and out.tobytes() == want.tobytes()
    assert min(st["n_phased"], st["n_disagree"]) > 30 and (st["n_few_reads"] > 10 or min_reads == 0)


def test_null_parameters_in_place_and_empty():
    L = capi.load_library()
    q, c = _table([(1, 3, 0, 0), (1, 2, 0, 0), (0, 0, 4, 0)])
    want, wst = HC.assign(q, c)
    buf, st = q.copy(), capi.HapAssignStats()
    assert L.c3r_hap_assign(buf.ctypes.data_as(C.c_void_p), len(buf), c.ctypes.data_as(C.c_void_p), None, buf.ctypes.data_as(C.c_void_p), C.byref(st)) == 0
    assert buf.tobytes() == want.tobytes() and {k: int(getattr(st, k)) for k in HC.STAT_KEYS} == wst
    buf = q.copy()
    assert L.c3r_hap_assign(buf.ctypes.data_as(C.c_void_p), len(buf), c.ctypes.data_as(C.c_void_p), None, buf.ctypes.data_as(C.c_void_p), None) == 0
    assert buf.tobytes() == want.tobytes()
    assert L.c3r_hap_assign(None, 0, None, None, None, C.byref(st)) == 0 and st.n_sites == 0 and st.n_phased == 0
    out, st0 = capi.hap_assign(None, np.zeros((0, 3, 3), np.uint32))
    assert len(out) == 0 and st0 == dict.fromkeys(HC.STAT_KEYS, 0)
    for bad in ((-1, 75), (2, 101), (2, -1)):
        with pytest.raises(capi.C3RError):
            capi.hap_assign(q, c, *bad)
    with pytest.raises(ValueError):
        capi.hap_assign(q, c[:2])


# ---- 3. the nearest-set rule
def test_nearest_set_known_answers():
    table = hapref.make_sites([(100, "A", "C", 0, 1), (110, "A", "C", 1, 2), (111, "A", "C", 0, 3), (200, "A", "C", 0, 2)])
    cands = HC.make_query([(p, "G", "T", 0) for p in (1, 99, 100, 104, 105, 106, 110, 111, 155, 156, 200, 9000)])
    # 105 lies between 100 and 110 at equal distance: the site before; 155 / 156 between 111 and 200 (44 : 45, 45 : 44)
    want = [1, 1, 1, 1, 1, 2, 2, 3, 3, 2, 2, 2]
    for fn in (HC.nearest_sets, hap_vcf.nearest_sets):
        out = fn(cands, table)
        assert out["ps"].tolist() == want and out["pos"].tolist() == cands["pos"].tolist() and not out["h1"].any(), fn
    one = table[1:2]
    assert hap_vcf.nearest_sets(cands, one)["ps"].tolist() == [2] * len(cands) == HC.nearest_sets(cands, one)["ps"].tolist()


@pytest.mark.parametrize("seed", range(4))
def test_nearest_set_of_random_tables(seed):
    rng = random.Random(seed)
    table = hapref.make_sites([(p, "A", "C", rng.randint(0, 1), rng.randrange(5)) for p in sorted(rng.sample(range(1, 400), 40))])
    cands = HC.make_query([(p, "G", "T", 0) for p in sorted(rng.sample(range(1, 420), 150))])
    assert hap_vcf.nearest_sets(cands, table).tobytes() == HC.nearest_sets(cands, table).tobytes()


# ---- 4. the writers
HEADER = ["##fileformat=VCFv4.2\n", '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"]
ROWS = ["chr1\t10\t.\tA\tC\t20\tPASS\tF\tGT:GQ:DP\t0/1:20:9\n",
        "chr1\t20\t.\tG\tT\t20\tPASS\tF\tGT:GQ:DP\t1/0:20:9\n",
        "chr1\t30\t.\tG\tT\t20\tPASS\tF\tGT:GQ:DP\t1/1:20:9\n",
        "chr1\t40\t.\tGA\tG\t20\tPASS\tF\tGT:GQ:DP\t0/1:20:9\n",
        "chr1\t50\t.\tC\tT\t3\tLowQual\tF\tGT:GQ:DP\t0/1:3:9\n",
        "chr1\t60\t.\tC\tT\t20\tPASS\tF\tGT:GQ:DP\t0/1:20:9\n",
        "chr2\t10\t.\tA\tC\t20\tPASS\tF\tGT:GQ:DP\t0/1:20:9\n",
        "chr2\t15\t.\tA\tG\t20\tPASS\tF\tGT:GQ:DP\t0/1:20:9\n",
        "chr3\t7\t.\tT\tG\t20\tPASS\tF\tGT:GQ:DP\t0/1:20:9\n"]


def _assigned():
    a = hapref.make_sites([(10, "A", "C", 1, 10), (20, "G", "T", 0, 10), (30, "G", "T", 1, 10), (50, "C", "T", 1, 10), (60, "C", "T", 0, -1)])
    b = hapref.make_sites([(10, "A", "G", 1, 5), (15, "A", "G", 0, 5)])         # 10: another ALT than the row's
    return {"chr1": a, "chr2": b}


WANT = list(ROWS)
WANT[0] = "chr1\t10\t.\tA\tC\t20\tPASS\tF\tGT:GQ:DP:PS\t1|0:20:9:10\n"
WANT[1] = "chr1\t20\t.\tG\tT\t20\tPASS\tF\tGT:GQ:DP:PS\t0|1:20:9:10\n"
WANT[7] = "chr2\t15\t.\tA\tG\t20\tPASS\tF\tGT:GQ:DP:PS\t0|1:20:9:5\n"


def test_the_writer_rewrites_the_assigned_rows_and_no_others(tmp_path):
    src, out = str(tmp_path / "in.vcf"), str(tmp_path / "out.vcf")
    with open(src, "w") as f:
        f.writelines(HEADER + ROWS)
    assert hap_vcf.write_vcf(src, _assigned(), out) == 3
    got = open(out).read()
    assert got == "".join(HEADER[:2]) + phasing.PS_HEADER + HEADER[2] + "".join(WANT)
    # a header that has the PS line keeps it, once; a gzipped input gives the same
    with gzip.open(src + ".gz", "wt") as f:
        f.writelines(HEADER[:2] + [phasing.PS_HEADER] + HEADER[2:] + ROWS)
    assert hap_vcf.write_vcf(src + ".gz", _assigned(), out) == 3 and open(out).read() == got
    # nothing assigned: every byte as it was, but for the header line
    assert hap_vcf.write_vcf(src, {}, out) == 0 and open(out).read() == "".join(HEADER[:2]) + phasing.PS_HEADER + HEADER[2] + "".join(ROWS)


def test_the_compressed_output_reads_back_as_the_assigned_sites(tmp_path):
    src, out = str(tmp_path / "in.vcf"), str(tmp_path / "out.vcf.gz")
    with open(src, "w") as f:
        f.writelines(HEADER + ROWS)
    assert hap_vcf.write_vcf(src, _assigned(), out) == 3
    assert os.path.isfile(out) and os.path.isfile(out + ".tbi") and not os.path.exists(out[:-3])
    per = phasedvcf.read_all_phase_sites(out)
    assert sorted(per) == ["chr1", "chr2", "chr3"] and len(per["chr3"][0]) == 0
    assert per["chr1"][0].tobytes() == _assigned()["chr1"][:2].tobytes() and per["chr2"][0].tobytes() == _assigned()["chr2"][1:].tobytes()
    with gzip.open(out, "rt") as f:
        assert f.read() == "".join(HEADER[:2]) + phasing.PS_HEADER + HEADER[2] + "".join(WANT)


def test_phase_vcf_writer_shares_the_row_rewrite_and_keeps_its_output(tmp_path):
    src, out = str(tmp_path / "in.vcf"), str(tmp_path / "phased_chr1.vcf.gz")
    with open(src, "w") as f:
        f.writelines(HEADER + ROWS)
    assert phasing.write_phased_vcf(src, "chr1", _assigned()["chr1"], out) == 2
    with gzip.open(out, "rt") as f:
        assert f.read() == "".join(HEADER[:2]) + phasing.PS_HEADER + HEADER[2] + "".join(WANT[:6])


def test_the_counts_file_lines():
    q = HC.make_query([(10, "A", "C", 7), (20, "G", "T", 7)])
    c = np.arange(18, dtype=np.uint32).reshape(2, 3, 3)
    out = q.copy()
    out["ps"][1], out["h1"][0] = -1, 1
    assert hap_vcf.counts_lines("chrX", q, out, c) == ["chrX\t10\tA\tC\t7\t1|0\t3\t4\t5\t6\t7\t8\t0\t1\t2\n",
                                                      "chrX\t20\tG\tT\t7\t0/1\t12\t13\t14\t15\t16\t17\t9\t10\t11\n"]
    assert len(hap_vcf.COLUMNS) == 15 and hap_vcf.COLUMNS[6:] == ("HP1_REF", "HP1_ALT", "HP1_OTHER", "HP2_REF", "HP2_ALT", "HP2_OTHER", "NONE_REF", "NONE_ALT", "NONE_OTHER")
