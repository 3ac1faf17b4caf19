"""Per-haplotype allele counts on the device (k_haplotag's read phase sets, c3r_hap_counts / k_hap_counts) against tests/hapcountref.py, the
plain-Python restatement of the rule: element for element, no tolerance; that the call leaves tags and scans alone; and the drivers
(hap_vcf, call_sample --phase_output)."""
import gzip
import os
import random
import re

import numpy as np
import pytest

from clair3_rna_amd import hap_vcf
from tests import hapcountref as HC
from tests import hapref
from tests import phaseref as P

pytestmark = pytest.mark.gpu

_state = {}


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _clean(request):
    """Every test of this module starts and leaves its engine without phase sites and with default parameters."""
    yield
    if "eng" in request.fixturenames:
        from clair3_rna_amd import capi
        e = request.getfixturevalue("eng")
        e.set_phase_sites(None)
        e.params = capi.default_params()
        e.set_params()


def _readset(recs):
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=r[4] if len(r) > 4 else 60, hp=0) for r in recs])


def _check(eng, rs, table, query, params=HC.DEFAULT_PARAMS, load=True):
    """The engine's read phase sets and count table for (rs, table, query) under its current filters equal the restatement's under
    `params`; returns (phase sets, counts)."""
    exp_ps, exp = HC.read_phase_sets(rs, table), HC.hap_counts(rs, table, query, params)
    if load:
        eng.set_phase_sites(table)
        eng.load_reads(rs)
    ps, got = eng.read_phase_sets(), eng.hap_counts(query)
    assert ps.dtype == np.int32 and ps.tolist() == exp_ps.tolist(), np.argwhere(ps != exp_ps)[:10]
    assert got.shape == (len(query), 3, 3) and got.dtype == np.uint32
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    return exp_ps, exp


def _own_sets(table):
    q = table.copy()
    q["h1"] = 0
    return q


# ---- 1. against the restatement
@pytest.mark.parametrize("case", hapref.CASES, ids=[c[0] for c in hapref.CASES])
def test_the_haplotagging_cases(eng, case):
    rs, table = hapref.case_inputs(case)
    ps, _ = _check(eng, rs, table, _own_sets(table))
    assert [p >= 0 for p in ps.tolist()] == [e[0] != 0 for e in case[3]]
    hp, _ = eng.haplotags()
    assert hp.tolist() == [e[0] for e in case[3]]


@pytest.mark.parametrize("seed", range(4))
def test_generated_reads_with_interleaved_sets(eng, seed):
    _, rs, table, _ = hapref.gen_case(seed)
    assert 350 <= len(rs) <= 400 and len(set(table["ps"].tolist())) >= 25
    rng = random.Random(seed)
    query = _own_sets(table)
    query["ps"][::4] = [rng.choice(table["ps"].tolist()) for _ in query[::4]]       # a quarter counted against some other set
    ps, exp = _check(eng, rs, table, query)
    assert len(set(ps.tolist())) >= 20 and (ps < 0).sum() >= 1
    assert exp[:, 1].sum() > 300 and exp[:, 2].sum() > 300 and exp[:, 0].sum() > 100 and exp[:, :, 2].sum() > 20


def _chain_case(seed):
    """phaseref.gen_case(errors=True): the table is the chain's output minus every third site; the queries are all sites plus 40 random
    positions with random ref / alt, each with the set of the nearest table site."""
    if seed not in _state:
        from clair3_rna_amd import phasing
        ref, rs, sites, _, _ = P.gen_case(seed, errors=True)
        chain = phasing.phased_only(P.phase(rs, sites)[0])
        table = np.ascontiguousarray(np.delete(chain, np.arange(0, len(chain), 3)))
        rng = random.Random(100 + seed)
        taken = set(sites["pos"].tolist())
        extra = []
        for p in rng.sample([p for p in range(1, len(ref) + 1) if p not in taken], 40):
            a, b = rng.sample("ACGT", 2)
            extra.append((p, a, b, 0, 0))
        query = np.concatenate([sites, hapref.make_sites(extra)])
        query = HC.nearest_sets(query[np.argsort(query["pos"], kind="stable")], table)
        _state[seed] = (ref, rs, table, query)
    return _state[seed]


@pytest.mark.parametrize("seed", range(4))
def test_a_chains_table_with_held_out_sites_and_random_queries(eng, seed):
    _, rs, table, query = _chain_case(seed)
    assert len(table) >= 40 and len(query) >= 140 and len(rs) % 16 != 0
    ps, exp = _check(eng, rs, table, query)
    # tagged rows, the untagged row and third bases all occur
    assert exp[:, 1, :2].sum() > 300 and exp[:, 2, :2].sum() > 300 and exp[:, 0].sum() > 0 and exp[:, :, 2].sum() > 50
    # the chain leaves these reads one block: the same table cut into sets of 15 sites, so that reads of a neighbouring set occur too
    cut = table.copy()
    cut["ps"] = 1000 + np.arange(len(cut)) // 15
    ps, exp = _check(eng, rs, cut, HC.nearest_sets(query, cut))
    assert len(set(ps[ps >= 0].tolist())) >= 4 and exp[:, 0].sum() > 100 and exp[:, 1:].sum() > 1000


@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_read_counts_around_a_workgroup(eng, n):
    seqs = ["AAAA", "CCCC", "ACAC", "GGGG", "AACA"]             # 1, 2, tie, no vote, 1
    rs = _readset([(k // 3, "4M", seqs[k % 5]) for k in range(n)])
    table = hapref.make_sites([(p, "A", "C", 0, 1) for p in (3, 4, 5, 6)])
    query = HC.make_query([(p, "A", "C", 1) for p in range(1, 11)])
    _, exp = _check(eng, rs, table, query)
    assert int(exp.sum()) == sum(min(10, k // 3 + 4) - k // 3 for k in range(n))    # every base of every read shows something


@pytest.mark.parametrize("n_sites", [1, 2])
def test_one_and_two_query_sites(eng, n_sites):
    rs = _readset([(0, "6M", "ACGTAC"), (2, "6M", "GTACGT"), (4, "3M2D3M", "ACGTAC")])
    table = hapref.make_sites([(3, "G", "A", 0, 1), (5, "A", "G", 1, 1)])
    query = HC.make_query([(5, "A", "G", 1), (7, "G", "T", 1)][:n_sites])
    _, exp = _check(eng, rs, table, query)
    assert int(exp[0].sum()) == 3


def test_six_hundred_sites_on_consecutive_positions(eng):
    """600-base reads over a query with a site on every position: many sites per op, and ops whose stretch of sites starts and ends inside
    the table."""
    rng = random.Random(5)
    L = 720
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    alt = ["ACGT"[("ACGT".index(b) + 1 + rng.randrange(3)) % 4] for b in ref]
    table = hapref.make_sites([(p + 1, ref[p], alt[p], (p // 7) % 2, 1 + p // 240) for p in range(0, L, 9)])
    query = HC.make_query([(p + 1, ref[p], alt[p], 1 + (p // 200) % 3) for p in range(60, 660)])
    recs = []
    for start, cigar in ((0, "600M"), (3, "600M"), (57, "300M2D298M"), (97, "250=100X250M"), (110, "100M9N500M"), (119, "592M")):
        seq, x, hap = [], start, rng.randint(0, 1)
        for n, op in re.findall(r"(\d+)([MDN=X])", cigar):
            for _ in range(int(n)):
                if op in "M=X":
                    seq.append(rng.choice("ACGTN") if rng.random() < 0.08 else (alt[x] if (x // 7 + hap) % 2 else ref[x]))
                x += 1
        assert x < L
        recs.append((start, cigar, "".join(seq)))
    assert len(query) == 600
    _, exp = _check(eng, _readset(recs), table, query)
    assert int(exp.sum()) > 6 * 500 * 0.9 and exp[:, :, 2].sum() > 50 and exp[:, 1:].sum() > 500


@pytest.mark.parametrize("cigar", ["4M1P4M", "4M0D4M", "4M2H4M", "2S3M0I2M1P1D2M", "8M0M", "3H2M0I1P2M2H"])
def test_cigars_that_take_the_serial_walk(eng, cigar):
    seq = "ACGTACGTAC"
    table = hapref.make_sites([(p, "ACGT"[(p - 11) % 4], "ACGT"[(p - 10) % 4], p % 2, 1 + p % 2) for p in range(9, 22, 3)])
    query = HC.make_query([(p, "ACGT"[(p - 11) % 4], "ACGT"[(p - 9) % 4], 1 + (p // 2) % 2) for p in range(8, 23)])
    rs = _readset([(10, cigar, seq), (10, "8M", seq), (12, cigar, seq, 16)])
    _, exp = _check(eng, rs, table, query)
    assert int(exp.sum()) >= 12


def test_five_thousand_reads_on_one_site(eng):
    rs = _readset([(100, "2M", "AG")] * 5000)
    table = hapref.make_sites([(101, "A", "C", 0, 4)])
    _, exp = _check(eng, rs, table, HC.make_query([(102, "G", "T", 4)]))
    assert exp[0].tolist() == [[0, 0, 0], [5000, 0, 0], [0, 0, 0]]


def test_the_filters_change_the_counts_and_not_the_tags(eng):
    _, rs, table, query = _chain_case(0)
    failing = [i for i in range(len(rs)) if not P.votes(rs.reads[i], P.DEFAULT_PARAMS)]
    assert len(failing) >= 20
    ps, exp = _check(eng, rs, table, query)
    tags = eng.haplotags()
    eng.set_params(min_mq=0, excl_flags=0)                    # the reads already loaded are filtered anew
    _, loose = _check(eng, rs, table, query, dict(min_mq=0, excl_flags=0), load=False)
    assert int(loose.sum()) > int(exp.sum())
    after = eng.haplotags()
    assert after[0].tolist() == tags[0].tolist() and after[1] == tags[1] and eng.read_phase_sets().tolist() == ps.tolist()
    eng.set_params(min_mq=61)
    assert eng.hap_counts(query).sum() == 0 and eng.haplotags()[0].tolist() == tags[0].tolist()


def test_a_table_replaced_after_the_load_moves_tags_sets_and_counts_together(eng):
    _, rs, table, query = _chain_case(1)
    ps, exp = _check(eng, rs, table, query)
    tags = eng.haplotags()[0]
    other = table.copy()
    other["h1"] ^= 1
    other["ps"] += 100000                                     # (beyond every old number: the chain numbers its sets by position)
    q2 = query.copy()
    q2["ps"] += 100000
    eng.set_phase_sites(other)                                # reads stay loaded
    ps2, exp2 = _check(eng, rs, other, q2, load=False)
    tags2 = eng.haplotags()[0]
    assert ps2.tolist() == [p + 100000 if p >= 0 else -1 for p in ps.tolist()]
    assert tags2.tolist() == [{0: 0, 1: 2, 2: 1}[t] for t in tags.tolist()] == hapref.haplotag(rs, other)[0].tolist()
    assert np.array_equal(exp2, exp[:, [0, 2, 1], :]) and not np.array_equal(exp2, exp)
    # against the old numbers every read is "tagged in another set"
    old = eng.hap_counts(query)
    assert old[:, 1:].sum() == 0 and np.array_equal(old[:, 0], exp.sum(axis=1))


# ---- 2. errors and empty cases
def test_no_table_is_refused_by_both_entries(eng):
    from clair3_rna_amd import capi
    rs = _readset([(0, "4M", "ACGT")])
    eng.load_reads(rs)
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        eng.read_phase_sets()
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        eng.hap_counts(HC.make_query([(2, "C", "A", 1)]))
    eng.set_phase_sites(hapref.make_sites([(1, "A", "C", 0, 1)]))
    assert eng.hap_counts(HC.make_query([(2, "C", "A", 1)]))[0, 1, 0] == 1
    eng.set_phase_sites(None)                                 # cleared: refused again
    with pytest.raises(capi.C3RError, match="no phase sites are set"):
        eng.hap_counts(HC.make_query([(2, "C", "A", 1)]))


BAD_QUERIES = [
    ("unsorted", [(10, "A", "C", 1), (30, "A", "C", 1), (20, "A", "C", 1)], {}, 2),
    ("repeated", [(10, "A", "C", 1), (10, "A", "G", 1)], {}, 1),
    ("negative_ps", [(5, "A", "C", 1), (6, "A", "C", 1)], dict(ps=-1), 1),
    ("pos_below_1", [(0, "A", "C", 1)], {}, 0),
    ("bad_alt_code", [(5, "A", "C", 1), (6, "A", "C", 1)], dict(alt=15), 1),
    ("ref_equals_alt", [(5, "A", "C", 1)], dict(alt=1), 0),
]


@pytest.mark.parametrize("name, rows, patch, index", BAD_QUERIES, ids=[b[0] for b in BAD_QUERIES])
def test_bad_query_tables_name_the_index(eng, name, rows, patch, index):
    from clair3_rna_amd import capi
    query = HC.make_query(rows)
    for k, v in patch.items():
        query[k][index] = v
    eng.set_phase_sites(hapref.make_sites([(1, "A", "C", 0, 1)]))
    eng.load_reads(_readset([(0, "40M", "A" * 40)]))
    with pytest.raises(capi.C3RError, match="query site %d:" % index):
        eng.hap_counts(query)
    query = HC.make_query([(5, "A", "C", 1), (6, "A", "C", 1)])
    query["h1"] = 9                                           # ignored on input
    assert eng.hap_counts(query)[:, 1, 0].tolist() == [1, 1]


def test_no_query_sites_and_no_reads(eng):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    _, rs, table, query = _chain_case(0)
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    eng.set_profiling(True)
    try:
        eng.reset_kernel_stats()
        none = eng.hap_counts(np.zeros(0, capi.PHASE_SITE_DTYPE))
        assert none.shape == (0, 3, 3) and eng.hap_counts(None).shape == (0, 3, 3) and "k_hap_counts" not in eng.kernel_stats()
        eng.hap_counts(query)
        assert eng.kernel_stats()["k_hap_counts"]["launches"] == 1
        eng.load_reads(ReadSet.from_records([]))
        eng.reset_kernel_stats()
        got = eng.hap_counts(query)
        assert got.shape == (len(query), 3, 3) and got.sum() == 0 and "k_hap_counts" not in eng.kernel_stats()
        assert len(eng.read_phase_sets()) == 0
    finally:
        eng.set_profiling(False)
    far = HC.make_query([(p, "A", "C", 1) for p in (7000, 7001, 2000000000)])
    eng.load_reads(rs)
    assert eng.hap_counts(far).sum() == 0


# ---- 3. the call leaves everything else alone
def test_tags_and_a_scan_are_the_same_with_and_without_the_call(eng):
    ref, rs, table, query = _chain_case(2)
    eng.set_params(channels=30, min_coverage=2)
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    eng.set_reference(1, ref)

    def scan():
        n = eng.scan(1, len(ref))
        return n, eng.tensors(rescaled=True).tobytes(), eng.tensors(rescaled=False).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()

    plain, tags, sets = scan(), eng.haplotags(), eng.read_phase_sets().tolist()
    assert plain[0] > 20 and tags[1]["n_hp1"] > 30 and tags[1]["n_hp2"] > 30
    eng.load_reads(rs)
    assert eng.hap_counts(query).sum() > 0
    after = eng.haplotags()
    assert after[0].tolist() == tags[0].tolist() and after[1] == tags[1] and eng.read_phase_sets().tolist() == sets
    assert scan() == plain
    assert eng.hap_counts(query[::2]).sum() > 0               # after the scan: what it left is still there
    assert (eng.tensors(rescaled=True).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()) == (plain[1], plain[3], plain[4])
    assert scan() == plain


# ---- 4. drivers, on the two-contig sample of the haplotagging tests' driver cases
@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """Two contigs of hapref.gen_case reads in an untagged BAM, the phased VCFs of two thirds of their sites as a directory of
    phased_<ctg>.vcf.gz, and call_sample's phased pass on them WITHOUT --phase_output."""
    from clair3_rna_amd import bam, bamio, io, synth
    from clair3_rna_amd.reads import NT16
    tmp = str(tmp_path_factory.mktemp("hapcount_drivers"))
    contigs, reads = [], {}
    per = os.path.join(tmp, "phased_vcf")
    os.makedirs(per)
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    for name, seed in (("chr1", 11), ("chr2", 12)):
        ref, rs, sites, _ = hapref.gen_case(seed)
        contigs.append((name, ref))
        reads[name] = rs
        with gzip.open(os.path.join(per, "phased_%s.vcf.gz" % name), "wt") as f:
            f.write(head + "".join("%s\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s:%d\n" % (name, s["pos"], NT16[s["ref"]], NT16[s["alt"]], "1|0" if s["h1"] else "0|1", s["ps"])
                                   for k, s in enumerate(sites) if k % 3))
    fa, wfn = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model")
    io.write_fasta(fa, contigs)
    np.save(wfn + ".c3rw.npy", synth.random_weights(30, seed=7))    # (weights that call heterozygous SNVs here: most seeds call none)
    bam_fn = os.path.join(tmp, "plain.bam")
    bam.write_bam(bam_fn, [(n, len(r)) for n, r in contigs], reads)
    bamio.index_build(bam_fn)
    s = dict(tmp=tmp, fa=fa, wfn=wfn, bam=bam_fn, per=per, reads=reads)
    _call_sample(s, "base", ["--phased_vcf_fn", per])
    s["final"] = os.path.join(tmp, "base", "output_enable_phasing.vcf.gz")
    assert os.path.isfile(s["final"])
    return s


def _argv(s, out, extra):
    return ["--bam_fn", s["bam"], "--ref_fn", s["fa"], "--output_dir", os.path.join(s["tmp"], out), "--pileup_model_path", s["wfn"],
            "--phased_pileup_model_path", s["wfn"], "--chunk_num", "3", "--min_coverage", "2"] + list(extra)


def _call_sample(s, out, extra):
    from clair3_rna_amd import call_sample
    assert call_sample.Run(call_sample.build_parser().parse_args(_argv(s, out, ["--enable_phasing_model"] + list(extra))), log=lambda m: None) == 0


def _gz(fn):
    with gzip.open(fn, "rt") as f:
        return f.read()


def _by_hand(s, out_fn, tsv_fn, log=None):
    return hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", s["bam"], "--vcf_fn", s["final"], "--phased_vcf_fn", s["per"], "--output_fn", out_fn,
                                                           "--hap_counts_fn", tsv_fn]), log=log or (lambda m: None))


def test_hap_vcf_writes_what_the_restatement_and_the_writer_give(sample, tmp_path):
    from clair3_rna_amd import phasedvcf, phasing
    out_fn, tsv_fn = str(tmp_path / "phased.vcf.gz"), str(tmp_path / "counts.tsv")
    msgs = []
    n = _by_hand(sample, out_fn, tsv_fn, msgs.append)
    assert len(msgs) == 2 and all(m.startswith("[INFO] chr") for m in msgs)
    assigned, lines, n_cand = {}, ["\t".join(hap_vcf.COLUMNS) + "\n"], 0
    for ctg in ("chr1", "chr2"):
        table = phasedvcf.contig_sites(sample["per"], ctg)
        cands, _ = phasing.candidates_from_vcf(sample["final"], ctg)
        query = HC.nearest_sets(cands, table)
        counts = HC.hap_counts(sample["reads"][ctg], table, query)
        assigned[ctg], _ = HC.assign(query, counts)
        lines += hap_vcf.counts_lines(ctg, query, assigned[ctg], counts)
        n_cand += len(cands)
    n_phased = sum(int((a["ps"] >= 0).sum()) for a in assigned.values())
    print("candidates %d, phased %d" % (n_cand, n_phased))
    assert n_cand >= 10 and n_phased >= 3 and n == n_phased  # the comparison below is about something
    exp_fn = str(tmp_path / "exp.vcf")
    assert hap_vcf.write_vcf(sample["final"], assigned, exp_fn) == n
    assert _gz(out_fn) == open(exp_fn).read() and os.path.isfile(out_fn + ".tbi")
    assert open(tsv_fn).read() == "".join(lines)
    # read back, the output holds exactly the assigned sites
    for ctg in ("chr1", "chr2"):
        back = phasedvcf.read_phase_sites(out_fn, ctg)[0]
        keep = assigned[ctg][assigned[ctg]["ps"] >= 0]
        assert back.tobytes() == keep.tobytes()


def test_call_sample_with_phase_output_equals_hap_vcf_by_hand(sample, tmp_path):
    out_fn, tsv_fn = str(tmp_path / "phased.vcf.gz"), str(tmp_path / "counts.tsv")
    _by_hand(sample, out_fn, tsv_fn)
    _call_sample(sample, "flag", ["--phased_vcf_fn", sample["per"], "--phase_output"])
    out = os.path.join(sample["tmp"], "flag")
    assert open(os.path.join(out, "output_enable_phasing.vcf.gz"), "rb").read() == open(sample["final"], "rb").read()
    assert open(os.path.join(out, "output_enable_phasing_phased.vcf.gz"), "rb").read() == open(out_fn, "rb").read()
    assert open(os.path.join(out, "output_enable_phasing_phased.vcf.gz.tbi"), "rb").read() == open(out_fn + ".tbi", "rb").read()
    assert open(os.path.join(out, "output_enable_phasing_hap_counts.tsv")).read() == open(tsv_fn).read()
    assert "|" in _gz(out_fn) and _gz(out_fn) != _gz(sample["final"])
    # without the flag: no file more
    assert not [f for f in os.listdir(os.path.join(sample["tmp"], "base")) if "phased" in f or "hap_counts" in f]


def test_phase_output_refuses_what_it_cannot_do(sample, monkeypatch):
    from clair3_rna_amd import call_sample

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:
            call_sample.Run(call_sample.build_parser().parse_args(_argv(sample, "refused", extra)))
        assert str(e.value.code).startswith("[ERROR]") and all(w in str(e.value.code) for w in words), e.value.code

    refused(["--phase_output", "--phased_vcf_fn", sample["per"]], "--phase_output", "--enable_phasing_model")
    refused(["--phase_output", "--enable_phasing_model"], "--phase_output", "--phased_vcf_fn", "--phasing builtin")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(["--phase_output", "--enable_phasing_model", "--phased_vcf_fn", sample["per"]], "WORLD_SIZE", "one process", "clair3_rna_amd.hap_vcf")
    assert not os.path.exists(os.path.join(sample["tmp"], "refused"))
