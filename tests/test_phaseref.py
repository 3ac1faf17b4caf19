"""The phasing rule without a GPU: tests/phaseref.py pinned by hand-derived known answers, c3r_phase_resolve (host code of libc3r.so)
against it, the VCF reader and writer of clair3_rna_amd/phasing.py, and what the rule guarantees on error-free reads."""
import gzip
import random

import numpy as np
import pytest

from tests import phaseref as P

K = P.K


def _sites(n, first=100, step=10):
    return P.make_sites([(first + step * j, "A", "C") for j in range(n)])


def _table(n, entries):
    """{(j, k): (cis, trans)} -> the (n, K, 2) link table."""
    lk = np.zeros((n, K, 2), dtype=np.uint32)
    for (j, k), ct in entries.items():
        assert 1 <= k <= K and j - k >= 0
        lk[j, k - 1] = ct
    return lk


# ---- hand-derived known answers for the rule: (name, n sites, {(j, k): (cis, trans)}, min_reads, min_agree_pct, [(block's first site or
# None for a site alone in its block, h1)] per site).  Site j stands at position 100 + 10 j.  Every expectation was worked out by hand.
RULE_CASES = [
    # site 1 sees site 0 (h1 0) with the same allele three times: v0 = 3, v1 = 0 -> same orientation
    ("two_sites_in_cis", 2, {(1, 1): (3, 0)}, 2, 75, [(0, 0), (0, 0)]),
    # ... with the other allele: v1 = 3
    ("two_sites_in_trans", 2, {(1, 1): (0, 3)}, 2, 75, [(0, 0), (0, 1)]),
    # every neighbour in trans: 0 1 0 1 (site 2: its predecessor has h1 = 1, so trans counts for v0)
    ("alternating_chain", 4, {(1, 1): (0, 4), (2, 1): (0, 4), (3, 1): (0, 4)}, 2, 75, [(0, 0), (0, 1), (0, 0), (0, 1)]),
    # the chain's orientation is carried, not the neighbour's: site 2 in cis with site 1 (h1 1) is 1 as well
    ("cis_after_trans", 3, {(1, 1): (0, 4), (2, 1): (4, 0)}, 2, 75, [(0, 0), (0, 1), (0, 1)]),
    ("balanced_site_stays_out", 3, {(1, 1): (2, 2), (2, 2): (5, 0)}, 2, 75, [(0, 0), (None, 0), (0, 0)]),
    ("agreement_74_stays_out", 2, {(1, 1): (74, 26)}, 2, 75, [(None, 0), (None, 0)]),
    ("agreement_75_gets_in", 2, {(1, 1): (75, 25)}, 2, 75, [(0, 0), (0, 0)]),
    ("agreement_75_in_trans", 2, {(1, 1): (1, 3)}, 2, 75, [(0, 0), (0, 1)]),
    ("one_read_below_min_reads", 2, {(1, 1): (1, 0)}, 2, 75, [(None, 0), (None, 0)]),
    ("two_reads_at_min_reads", 2, {(1, 1): (2, 0)}, 2, 75, [(0, 0), (0, 0)]),
    ("one_read_with_min_reads_1", 2, {(1, 1): (0, 1)}, 1, 75, [(0, 0), (0, 1)]),
    # min_reads counts the block's reads, not one pair's: one read each to sites 0 and 1 of one block make two
    ("min_reads_sums_over_the_block", 3, {(1, 1): (2, 0), (2, 1): (1, 0), (2, 2): (1, 0)}, 2, 75, [(0, 0), (0, 0), (0, 0)]),
    # ... and so does the agreement: 3 of 4 = 75 %
    ("agreement_sums_over_the_block", 3, {(1, 1): (2, 0), (2, 1): (2, 0), (2, 2): (1, 1)}, 2, 75, [(0, 0), (0, 0), (0, 0)]),
    ("linked_only_at_k_8", 9, {(8, 8): (0, 5)}, 2, 75, [(0, 0)] + [(None, 0)] * 7 + [(0, 1)]),
    # two blocks side by side, A = {0, 2, ...} and B = {1, 3, ...}: 0 and 1 are not linked, 2 joins 0 and 3 joins 1 (in trans)
    # site 4: B through site 3 (h1 1, cis 3 -> v1 = 3), A through site 2 (h1 0, trans 5 -> v1 = 5): the larger margin wins -> A, h1 1
    # site 5: A through site 4 (h1 1, cis 4 -> v1 4), B through site 3 (h1 1, trans 4 -> v0 4): margins equal, the nearer predecessor (4) is A's
    ("interleaved_blocks", 6, {(2, 2): (5, 0), (3, 2): (0, 4), (4, 1): (3, 0), (4, 2): (0, 5), (5, 1): (4, 0), (5, 2): (0, 4)}, 2, 75,
     [(0, 0), (1, 0), (0, 0), (1, 1), (0, 1), (0, 1)]),
    # the same start; site 4 now joins B (margin 5 against 3), and site 5 ties B through site 4 (k = 1) with A through site 2 (k = 3):
    # the nearer predecessor is B's, although A is the older block
    ("interleaved_blocks_tie_goes_to_the_nearer", 6, {(2, 2): (5, 0), (3, 2): (0, 4), (4, 1): (5, 0), (4, 2): (0, 3), (5, 1): (0, 4), (5, 3): (4, 0)}, 2, 75,
     [(0, 0), (1, 0), (0, 0), (1, 1), (1, 1), (1, 0)]),
    # a margin of 3 with a rejected block beside it: B has 12 reads and a margin of 4, but only 8 : 4 = 67 %
    ("a_rejected_block_does_not_compete", 4, {(2, 2): (2, 0), (3, 1): (3, 0), (3, 2): (8, 4)}, 2, 75, [(0, 0), (None, 0), (0, 0), (0, 0)]),
    ("no_sites", 0, {}, 2, 75, []),
    ("one_site", 1, {}, 2, 75, [(None, 0)]),
]


def _expected(n, exp):
    s = _sites(n)
    for j, (first, h1) in enumerate(exp):
        s[j]["ps"] = -1 if first is None else 100 + 10 * first
        s[j]["h1"] = h1
    return s


@pytest.mark.parametrize("case", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_known_answers_of_the_rule(case):
    _, n, entries, min_reads, pct, exp = case
    out, st = P.resolve(_sites(n), _table(n, entries), min_reads, pct)
    want = _expected(n, exp)
    assert P.equal_sites(out, want), (out.tolist(), want.tolist())
    sizes = {}
    for first, _ in exp:
        if first is not None:
            sizes[first] = sizes.get(first, 0) + 1
    assert st == dict(n_sites=n, n_phased=sum(sizes.values()), n_blocks=len(sizes), max_block=max(list(sizes.values()) + [1 if n else 0]))


def test_a_singleton_gets_minus_one_and_a_block_the_position_of_its_first_site():
    s = P.make_sites([(7, "A", "C"), (1234, "G", "T"), (99999, "T", "A"), (2000000000, "C", "G")])
    out, st = P.resolve(s, _table(4, {(2, 1): (0, 2), (3, 1): (2, 0)}), 2, 75)
    assert out["ps"].tolist() == [-1, 1234, 1234, 1234] and out["h1"].tolist() == [0, 0, 1, 1]
    assert out["pos"].tolist() == s["pos"].tolist() and out["ref"].tolist() == s["ref"].tolist() and out["alt"].tolist() == s["alt"].tolist()
    assert st == dict(n_sites=4, n_phased=3, n_blocks=1, max_block=3)


# ---- the links, by hand: reads of one base per site joined by N ops
def _reads(recs):
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=r[4] if len(r) > 4 else 60, hp=0) for r in recs])


def test_links_known_answers():
    s = P.make_sites([(11, "A", "C"), (12, "G", "T"), (20, "C", "A")])
    rs = _reads([(10, "2M", "AG"),                            # 0 0: cis (1, 0)
                 (10, "2M", "CG"),                            # 1 0: trans
                 (10, "2M7N1M", "CTA"),                       # 1 1 1: cis everywhere
                 (10, "2M7N1M", "AGA"),                       # 0 0 1
                 (10, "2M7N1M", "NGC"),                       # - 0 0: site 0 shows nothing
                 (10, "2M7N1M", "ATG"),                       # 0 1 -: a third base on site 2
                 (10, "2M", "AG", 0, 4),                      # MAPQ 4: no vote
                 (10, "2M", "AG", 256),                       # secondary: no vote
                 (10, "2M", "AG", 1),                         # paired, not a proper pair: no vote
                 (10, "2M", "AG", 3)])                        # a proper pair votes: cis
    lk = P.links(rs, s)
    assert lk[0].sum() == 0
    assert lk[1, 0].tolist() == [4, 2] and lk[1, 1:].sum() == 0          # (1, 0): AG CT AG AG(flag 3) cis; CG AT trans
    assert lk[2, 0].tolist() == [2, 1]                                   # (2, 1): CTA 1 1, NGC 0 0 cis; AGA 0 1 trans
    assert lk[2, 1].tolist() == [1, 1] and lk[2, 2:].sum() == 0          # (2, 0): CTA cis; AGA trans
    # with the filters off the MAPQ-4 read and the secondary one count; the anomalous pair is skipped whatever the flags say
    assert P.links(rs, s, dict(min_mq=0, excl_flags=0))[1, 0].tolist() == [6, 2]


def _far_pair(gap_sites):
    """Sites 1, 11, 21, ...: five reads that cover the first and the one `gap_sites` further on, and nothing between."""
    n = gap_sites + 1
    s = P.make_sites([(1 + 10 * j, "A", "C") for j in range(n)])
    rs = _reads([(0, "1M%dN1M" % (10 * gap_sites - 1), "AC")] * 5)
    return s, rs


def test_a_site_linked_only_at_k_8_joins_and_at_k_9_opens_a_new_block():
    s, rs = _far_pair(K)
    lk = P.links(rs, s)
    assert lk[K, K - 1].tolist() == [0, 5] and lk.sum() == 5
    out, _ = P.resolve(s, lk)
    assert out["ps"].tolist() == [1] + [-1] * (K - 1) + [1] and out["h1"][K] == 1
    s, rs = _far_pair(K + 1)
    lk = P.links(rs, s)
    assert lk.sum() == 0                                      # the ninth predecessor is not linked: the table has no place for it
    out, st = P.resolve(s, lk)
    assert out["ps"].tolist() == [-1] * (K + 2) and st["n_blocks"] == 0


# ---- c3r_phase_resolve against the restatement (no GPU: host code of libc3r.so)
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from clair3_rna_amd import capi
    return capi


@pytest.mark.parametrize("case", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_library_resolve_equals_the_restatement_on_the_known_answers(capi, case):
    _, n, entries, min_reads, pct, exp = case
    out, st = capi.phase_resolve(_sites(n), _table(n, entries), min_reads, pct)
    want, wst = P.resolve(_sites(n), _table(n, entries), min_reads, pct)
    assert P.equal_sites(out, want) and P.equal_sites(out, _expected(n, exp)) and st == wst


def _random_table(rng):
    n = rng.choice([1, 2, 3, 9, 17, 40, 80])
    s = P.make_sites([(p, "A", "G") for p in sorted(rng.sample(range(1, 100000), n))])
    s["ps"], s["h1"] = rng.randrange(100), 1                  # ignored on input
    lk = np.zeros((n, K, 2), dtype=np.uint32)
    dense = rng.choice([0.15, 0.5, 0.9])
    for j in range(n):
        for k in range(1, min(K, j) + 1):
            if rng.random() < dense:
                style = rng.randrange(4)
                lk[j, k - 1] = ((rng.randrange(7), rng.randrange(3)), (rng.randrange(3), rng.randrange(7)), (rng.randrange(4), rng.randrange(4)),
                                (rng.randrange(300), rng.randrange(100)))[style]
    return s, lk


def test_library_resolve_equals_the_restatement_on_random_tables(capi):
    rng = random.Random(20)
    blocks = 0
    for _ in range(200):
        s, lk = _random_table(rng)
        min_reads, pct = rng.choice([0, 1, 2, 2, 3, 5]), rng.choice([0, 50, 60, 75, 75, 90, 100])
        out, st = capi.phase_resolve(s, lk, min_reads, pct)
        want, wst = P.resolve(s, lk, min_reads, pct)
        assert P.equal_sites(out, want), (min_reads, pct, np.nonzero((out["ps"] != want["ps"]) | (out["h1"] != want["h1"]))[0][:5])
        assert st == wst
        blocks += st["n_blocks"]
    assert blocks > 300                                       # the tables do link


def test_library_resolve_refuses_bad_arguments(capi):
    s = _sites(3)
    with pytest.raises(ValueError):
        capi.phase_resolve(s, np.zeros((3, K - 1, 2), np.uint32))
    with pytest.raises(capi.C3RError):
        capi.phase_resolve(s, _table(3, {}), 2, 101)
    with pytest.raises(capi.C3RError):
        capi.phase_resolve(s[::-1].copy(), _table(3, {}))
    with pytest.raises(TypeError):
        capi.phase_resolve(np.zeros(3, np.int32), _table(3, {}))


# ---- the VCF reader and writer
HEAD = "##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
ROWS = [
    "chr1\t100\t.\tA\tG\t20.1\tPASS\tP\tGT:GQ:DP:AF\t0/1:20:31:0.4516",          # kept
    "chr1\t150\t.\tC\tT\t3.2\tLowQual\tP\tGT:GQ:DP:AF\t0/1:3:12:0.25",            # not_pass
    "chr1\t160\t.\tC\tCT\t18\tPASS\tP\tGT:GQ:DP:AF\t0/1:18:20:0.5",               # not_snv
    "chr1\t170\t.\tG\tA,T\t18\tPASS\tP\tGT:GQ:DP:AF\t1/2:18:20:0.5,0.4",          # not_snv
    "chr1\t180\t.\tT\tC\t25\tPASS\tP\tGT:GQ:DP:AF\t1/1:25:22:0.95",               # not_het
    "chr1\t190\t.\tT\tC\t25\tPASS\tP\tGT:GQ:DP:AF\t0/0:25:22:0.5",                # not_het
    "chr1\tx\t.\tT\tC\t25\tPASS\tP\tGT\t0/1",                                     # malformed
    "chr1\t195\t.\tT\tC\t25\tPASS\tP",                                            # malformed
    "chr2\t50\t.\tA\tC\t25\tPASS\tP\tGT:GQ\t0/1:9",                               # other_contig
    "chr1\t300\t.\tg\tt\t22\tPASS\tRNAEDIT\tGQ:GT\t22:1/0",                       # kept (lower case, GT second, 1/0)
    "chr1\t300\t.\tG\tC\t21\tPASS\tP\tGT:GQ\t0/1:21",                             # duplicate_pos
    "chr1\t250\t.\tC\tA\t30\tPASS\tP\tGT:GQ:DP:AF\t0/1:30:40:0.5",                # kept (out of order in the file)
]


def _write_vcf(path, gz):
    text = HEAD + "".join(r + "\n" for r in ROWS)
    with (gzip.open(path, "wt") if gz else open(path, "w")) as f:
        f.write(text)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
def test_candidates_from_vcf_counts_every_skip_reason(tmp_path, gz):
    from clair3_rna_amd import phasing
    fn = str(tmp_path / ("in.vcf.gz" if gz else "in.vcf"))
    _write_vcf(fn, gz)
    sites, skipped = phasing.candidates_from_vcf(fn, "chr1")
    assert sites["pos"].tolist() == [100, 250, 300]
    assert sites["ref"].tolist() == [1, 2, 4] and sites["alt"].tolist() == [4, 1, 8]
    assert sites["ps"].tolist() == [0, 0, 0] and sites["h1"].tolist() == [0, 0, 0]
    assert skipped == dict(other_contig=1, malformed=2, not_pass=1, not_snv=2, not_het=2, duplicate_pos=1)
    assert set(skipped) == set(phasing.SKIP_REASONS)
    per = phasing.candidates_from_vcf(fn, None)
    assert sorted(per) == ["chr1", "chr2"] and per["chr1"][0].tolist() == sites.tolist() and per["chr2"][0]["pos"].tolist() == [50]
    empty, sk = phasing.candidates_from_vcf(fn, "chr3")
    assert len(empty) == 0 and sk["other_contig"] == len(ROWS)


def test_phased_vcf_round_trip(tmp_path):
    from clair3_rna_amd import phasedvcf, phasing
    fn, out_fn = str(tmp_path / "in.vcf"), str(tmp_path / "phased_chr1.vcf.gz")
    _write_vcf(fn, False)
    sites, _ = phasing.candidates_from_vcf(fn, "chr1")
    out = sites.copy()
    out["ps"], out["h1"] = [100, -1, 100], [0, 0, 1]          # 100 and 300 in one block, 250 alone
    assert phasing.write_phased_vcf(fn, "chr1", out, out_fn) == 2
    back = phasedvcf.contig_sites(str(tmp_path), "chr1")
    assert back.tolist() == phasing.phased_only(out).tolist() and back["pos"].tolist() == [100, 300]
    with gzip.open(out_fn, "rt") as f:
        lines = f.read().split("\n")
    assert lines[-1] == ""
    head = [r for r in lines if r.startswith("#")]
    assert head == HEAD.rstrip("\n").split("\n")[:-1] + [phasing.PS_HEADER.rstrip("\n")] + [HEAD.rstrip("\n").split("\n")[-1]]
    body = [r for r in lines[:-1] if not r.startswith("#")]
    chr1 = [r for r in ROWS if r.startswith("chr1\t")]
    assert len(body) == len(chr1)
    for got, was in zip(body, chr1):
        if was is ROWS[0]:
            assert got == "chr1\t100\t.\tA\tG\t20.1\tPASS\tP\tGT:GQ:DP:AF:PS\t0|1:20:31:0.4516:100"
        elif was is ROWS[9]:
            assert got == "chr1\t300\t.\tg\tt\t22\tPASS\tRNAEDIT\tGQ:GT:PS\t22:1|0:100"
        else:
            assert got == was                                 # byte for byte, the unphased candidate on 250 and the second row on 300 included
    # a header that has the PS line already keeps it, once
    again = str(tmp_path / "again.vcf.gz")
    phasing.write_phased_vcf(out_fn, "chr1", np.zeros(0, out.dtype), again)
    with gzip.open(again, "rt") as f, gzip.open(out_fn, "rt") as g:
        assert f.read() == g.read()


# ---- what the rule guarantees on error-free reads
@pytest.fixture(scope="module")
def clean_cases():
    return {seed: P.gen_case(seed) for seed in (0, 1, 2, 3)}


def _shared_voters(rs, sites):
    """[j] = voting reads that observe both site j and site j - 1."""
    index_of = {int(s["pos"]): j for j, s in enumerate(sites)}
    n = np.zeros(len(sites), np.int64)
    for i in range(len(rs)):
        if P.votes(rs.reads[i], P.DEFAULT_PARAMS):
            seen = P.observe(rs, i, index_of, sites)
            for j in seen:
                if j - 1 in seen:
                    n[j] += 1
    return n


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_error_free_reads_give_no_switch_error_and_link_adjacent_sites(clean_cases, seed):
    _, rs, sites, truth, _ = clean_cases[seed]
    assert len(rs) % 16 != 0 and len(sites) > 100
    lk = P.links(rs, sites)
    out, st = P.resolve(sites, lk)
    assert st["n_blocks"] >= 1 and st["n_phased"] > len(sites) // 2
    # inside a block the orientations are the truth's or its mirror image
    for ps in set(out["ps"].tolist()) - {-1}:
        m = np.nonzero(out["ps"] == ps)[0]
        flips = (out["h1"][m] != truth[m])
        assert flips.all() or not flips.any(), (ps, m.tolist())
        assert int(sites["pos"][m[0]]) == ps
    # adjacent sites that share min_reads voting reads lie in one block
    shared = _shared_voters(rs, sites)
    assert (shared >= 2).sum() > len(sites) // 2
    for j in np.nonzero(shared >= 2)[0]:
        assert shared[j] == int(lk[j, 0].sum())
        assert out["ps"][j] != -1 and out["ps"][j] == out["ps"][j - 1], j
