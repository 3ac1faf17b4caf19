"""CPU tests of the haplotagging feature: the hand-derived known answers that pin tests/hapref.py (the restatement of the rule the GPU tests
compare k_haplotag with), the generator's properties, and phasedvcf.read_phase_sites on a literal VCF."""
import gzip

import numpy as np
import pytest

from clair3_rna_amd import phasedvcf
from tests import hapref


@pytest.mark.parametrize("case", hapref.CASES, ids=[c[0] for c in hapref.CASES])
def test_known_answers(case):
    rs, sites = hapref.case_inputs(case)
    by_pos = {int(s["pos"]): s for s in sites}
    got = [hapref.tag_read(rs, i, by_pos)[:3] for i in range(len(rs))]
    assert got == case[3], (case[0], got)
    hp, st, _ = hapref.haplotag(rs, sites)
    assert hp.tolist() == [e[0] for e in case[3]]
    assert st["n_reads"] == len(rs) == st["n_hp1"] + st["n_hp2"] + st["n_no_vote"] + st["n_tie"]


def test_case_table_covers_what_it_should():
    """The table holds every situation the rule names (by the names of its cases) and both outcomes of every choice."""
    names = " ".join(c[0] for c in hapref.CASES)
    for word in ("first_and_last", "position_1", "deletion", "ref_skip", "soft_clips", "insertion", "eq_and_x", "base_eq_n_third", "l_seq_shorter",
                 "h1_0_ref", "h1_0_alt", "h1_1_ref", "h1_1_alt", "tie", "earlier_first_site", "later_set_with_more"):
        assert word in names, word
    assert {e[0] for c in hapref.CASES for e in c[3]} == {0, 1, 2}


def test_stats_tell_ties_from_no_votes():
    rs, sites = hapref.case_inputs(("x", [(0, "2M", "AC"), (0, "2M", "GG"), (0, "2M", "AA"), (0, "2M", "CC")],
                                    [(1, "A", "C", 0, 1), (2, "A", "C", 0, 1)], None))
    hp, st, n_ps = hapref.haplotag(rs, sites)
    assert hp.tolist() == [0, 0, 1, 2] and n_ps.tolist() == [1, 0, 1, 1]
    assert st == dict(n_reads=4, n_hp1=1, n_hp2=1, n_no_vote=1, n_tie=1, n_votes=6)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_generated_cases_hold_what_the_gpu_tests_need(seed):
    """The conditions tests/test_gpu_haplotag.py asserts on its input, and that the tags recover the haplotype the reads were drawn from."""
    ref, rs, sites, truth = hapref.gen_case(seed)
    hp, st, n_ps = hapref.haplotag(rs, sites)
    assert 350 <= len(rs) <= 400 and len(sites) == 120 and np.all(np.diff(sites["pos"]) > 0)
    assert st["n_hp1"] >= 100 and st["n_hp2"] >= 100 and st["n_no_vote"] >= 5 and st["n_tie"] >= 1 and n_ps.max() >= 9, (st, n_ps.max())
    assert int((n_ps >= 2).sum()) > 300
    tagged = hp > 0
    assert int((hp[tagged] != truth[tagged]).sum()) <= 3, (hp[tagged] != truth[tagged]).sum()
    # the phase sets interleave: some set's sites are not one block of the table
    ps = sites["ps"].tolist()
    assert any(ps[i] != ps[i + 1] and ps[i] in ps[i + 2:] for i in range(len(ps) - 2))


VCF = """##fileformat=VCFv4.2
##contig=<ID=chr1>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2
chr1\t100\t.\tA\tC\t30\tPASS\t.\tGT:GQ:PS\t0|1:30:100\t1|0:1:5
chr1\t200\t.\tG\tT\t30\tLowQual\t.\tGT:PS\t1|0:100\t0|1:100
chr1\t300\t.\tA\tC\t30\tPASS\t.\tGT:PS\t0/1:100
chr1\t400\t.\tA\tC\t30\tPASS\t.\tGT:PS\t1|1:100
chr1\t500\t.\tA\tC,G\t30\tPASS\t.\tGT:PS\t1|2:100
chr1\t600\t.\tAT\tA\t30\tPASS\t.\tGT:PS\t0|1:100
chr1\t650\t.\tA\tAT\t30\tPASS\t.\tGT:PS\t0|1:100
chr1\t700\t.\tA\tC,T\t30\tPASS\t.\tGT:PS\t0|1:100
chr1\t800\t.\tc\tg\t30\tPASS\t.\tGT:PS\t1|0:800
chr1\t900\t.\tT\tA\t30\tPASS\t.\tGT\t0|1
chr1\t950\t.\tT\tG\t30\tPASS\t.\tGT:PS\t1|0:.
chr1\t100\t.\tA\tG\t30\tPASS\t.\tGT:PS\t1|0:7
chr2\t100\t.\tA\tC\t30\tPASS\t.\tGT:PS\t0|1:100
chr1\t50\t.\tG\tA\t30\tPASS\t.\tGT:PS\t0|1:50
"""
#        pos  ps  ref alt h1   (A 1, C 2, G 4, T 8; the last row of chr1 comes first: the table is sorted)
KEPT = [(50, 50, 4, 1, 0), (100, 100, 1, 2, 0), (200, 100, 4, 8, 1), (800, 800, 2, 4, 1), (900, 0, 8, 1, 0), (950, 0, 8, 4, 1)]
SKIPPED = dict(other_contig=1, malformed=0, not_snv=4, not_phased_het=2, duplicate_pos=1)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gzipped"])
def test_read_phase_sites(tmp_path, gz):
    fn = str(tmp_path / ("p.vcf.gz" if gz else "p.vcf"))
    with (gzip.open(fn, "wt") if gz else open(fn, "w")) as f:
        f.write(VCF)
    sites, skipped = phasedvcf.read_phase_sites(fn, "chr1")
    assert sites.dtype == hapref.PHASE_SITE_DTYPE and sites.dtype.itemsize == 12
    assert [tuple(int(v) for v in (s["pos"], s["ps"], s["ref"], s["alt"], s["h1"])) for s in sites] == KEPT
    assert skipped == SKIPPED
    s2, k2 = phasedvcf.read_phase_sites(fn, "chr2")
    assert s2["pos"].tolist() == [100] and k2["other_contig"] == 13
    s3, k3 = phasedvcf.read_phase_sites(fn, "chrX")
    assert len(s3) == 0 and k3["other_contig"] == 14
    per = phasedvcf.read_all_phase_sites(fn)
    assert sorted(per) == ["chr1", "chr2"] and per["chr1"][0].tobytes() == sites.tobytes() and per["chr2"][0].tobytes() == s2.tobytes()
