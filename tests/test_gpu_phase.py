"""Phasing on the device (c3r_phase_links / k_phase_links, c3r_phase_resolve) against tests/phaseref.py, the plain-Python restatement of
the rule; that the call leaves scans and haplotags alone; and the drivers (phase_vcf, call_sample --phasing builtin)."""
import gzip
import os
import random

import numpy as np
import pytest

from tests import hapref
from tests import helpers as H
from tests import phaseref as P

pytestmark = pytest.mark.gpu

K = P.K
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


def _check(eng, rs, sites, params=P.DEFAULT_PARAMS):
    """The engine's link table for (rs, sites) under the engine's current filters equals phaseref's under `params`; returns it."""
    exp = P.links(rs, sites, params)
    eng.load_reads(rs)
    got = eng.phase_links(sites)
    assert got.shape == (len(sites), K, 2) and got.dtype == np.uint32
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    return exp


def _gen(seed):
    """gen_case(seed) — odd seeds with ONT-like errors — and its reference link table, computed once."""
    if seed not in _state:
        case = P.gen_case(seed, errors=bool(seed % 2))
        _state[seed] = case + (P.links(case[1], case[2]),)
    return _state[seed]


def _site_span(rs, sites):
    """hi - lo per read: the table sites on positions the read's alignment spans."""
    pos = sites["pos"].astype(np.int64)
    out = []
    for r in rs.reads:
        end = int(r["pos"]) + sum(int(c) >> 4 for c in rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])] if "MIDNSHP=X"[int(c) & 15] in "MDN=X")
        out.append(int(np.searchsorted(pos, end + 1) - np.searchsorted(pos, int(r["pos"]) + 1)))
    return out


def _takes_serial_walk(cigar):
    """What csrc/reads_kernels.hpp calls a CIGAR that is not plain: a zero-length op, a pad, a hard clip inside, equal neighbours other than
    M-like ones."""
    import re
    ops = [(int(n), o) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    fold = ["M" if o in "=X" else o for _, o in ops]
    return (any(n == 0 or o == "P" for n, o in ops) or any(o == "H" and 0 < k < len(ops) - 1 for k, (_, o) in enumerate(ops))
            or any(fold[k] == fold[k - 1] != "M" for k in range(1, len(ops))))


# ---- 1. Engine.phase_links against phaseref.links
@pytest.mark.parametrize("seed", range(8))
def test_generated_cases(eng, seed):
    _, rs, sites, _, _, exp = _gen(seed)
    assert 380 <= len(rs) <= 420 and len(rs) % 16 != 0 and 100 <= len(sites) <= 130
    assert int(exp[:, 0].sum()) > 500 and int(exp[:, K - 1].sum()) > 0 and (exp[:, :, 1].sum() > 100)
    eng.load_reads(rs)
    got = eng.phase_links(sites)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]


@pytest.mark.parametrize("seed", [4100, 4101, 4102])
def test_reads_that_take_the_serial_walk(eng, seed):
    from clair3_rna_amd.reads import ReadSet
    ref, recs = H._case(seed, phased=False)
    rng = random.Random(9000 + seed)
    covered = set()
    for r in recs:
        covered.update(range(r["pos"] + 1, r["pos"] + H.cigar_ref_len(r["cigar"]) + 1))
    rows = []
    for p in sorted(rng.sample(sorted(covered), min(60, len(covered)))):
        a, b = rng.sample("ACGT", 2)
        rows.append((p, a, b))
    rs, sites = ReadSet.from_records(recs), P.make_sites(rows)
    serial = [_takes_serial_walk(r["cigar"]) for r in recs]
    assert sum(serial) >= 5 and sum(serial) < len(recs)
    exp = _check(eng, rs, sites)
    assert int(exp.sum()) > 50
    # ... and the serial reads alone say something
    only = ReadSet.from_records([r for r, s in zip(recs, serial) if s])
    assert int(_check(eng, only, sites).sum()) > 0


def test_first_and_last_base_of_an_op(eng):
    # 0-based 10: 4M on 1-based 11..14, 6N, 3M on 21..23
    rs = _readset([(10, "4M6N3M", "ACGTCAT")] * 3 + [(10, "4M6N3M", "CCGGAAT")] * 2)
    sites = P.make_sites([(10, "T", "A"), (11, "A", "C"), (14, "T", "G"), (15, "A", "C"), (20, "A", "C"), (21, "C", "A"), (23, "T", "G"), (24, "A", "C")])
    exp = _check(eng, rs, sites)
    # sites 1, 2, 5, 6 are observed: first 0 0 0 0 three times, then 1 1 1 0 twice; the four others never
    assert exp[2, 0].tolist() == [5, 0] and exp[5, 2].tolist() == [5, 0] and exp[6, 0].tolist() == [3, 2] and exp[6, 4].tolist() == [3, 2]
    assert exp[[0, 1, 3, 4, 7]].sum() == 0 and int(exp.sum()) == 5 * 6


def test_sites_in_a_ref_skip_a_deletion_beside_an_insertion_and_in_a_soft_clip(eng):
    # 0-based 20: 3S | 4M on 1-based 21..24 | 2D 25 26 | 3M 27..29 | 2I | 3M 30..32 | 8N 33..40 | 4M 41..44 | 2S
    cigar, seq = "3S4M2D3M2I3M8N4M2S", "TTT" "ACGT" "ACG" "TT" "TAC" "GTAC" "GG"
    rs = _readset([(20, cigar, seq)] * 4 + [(20, "24M", "ACGTAAACGTACAAAAAAAAGTAC")] * 2)
    rows = [(p, "ACGTNNACGTACNNNNNNNNGTAC"[p - 21], "A" if "ACGTNNACGTACNNNNNNNNGTAC"[p - 21] != "A" else "C") for p in range(21, 45) if "ACGTNNACGTACNNNNNNNNGTAC"[p - 21] != "N"]
    rows = [(18, "T", "A"), (19, "T", "A"), (20, "T", "A")] + rows[:4] + [(25, "A", "C"), (26, "A", "C")] + rows[4:10] + [(33, "A", "C"), (40, "A", "C")] + rows[10:] + [(45, "G", "A"), (46, "G", "A")]
    sites = P.make_sites(rows)
    exp = _check(eng, rs, sites)
    pos = sites["pos"].tolist()
    at = {p: j for j, p in enumerate(pos)}
    # the spliced reads never observe the clipped, deleted or skipped positions: those rows hold the two 24M reads' counts only
    for p in (18, 19, 20, 45, 46):
        assert exp[at[p]].sum() == 0
    for p in (25, 26, 33, 40):
        assert exp[at[p], 0].sum() == 2
    # the column before the insertion (29) and the one after it (30) are linked by all six reads
    assert exp[at[30], 0].tolist() == [6, 0]
    only = _readset([(20, cigar, seq)] * 4)
    alone = _check(eng, only, sites)
    for p in (18, 19, 20, 25, 26, 33, 40, 45, 46):
        assert alone[at[p]].sum() == 0
    assert alone[at[27], 2].tolist() == [4, 0]              # 27 -> 24 across the deletion: two table sites between them


def test_a_query_offset_at_or_beyond_l_seq(eng):
    rs = _readset([(0, "6M", "AACC")] * 2)
    rs.reads["l_seq"][:] = 3                                  # the fourth nibble holds a C that is not part of the read
    sites = P.make_sites([(2, "A", "C"), (3, "A", "C"), (4, "A", "C"), (6, "A", "C")])
    exp = _check(eng, rs, sites)
    assert exp[1, 0].tolist() == [0, 2] and int(exp.sum()) == 2


def test_three_windows_per_read_with_pairs_across_the_seams(eng):
    """600-base reads over a table with a site on every position: the read's sites fill three windows of 256 that overlap by K, and every
    k from 1 to K is counted for the sites on both sides of each seam."""
    rng = random.Random(5)
    L = 720
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    alt = ["ACGT"[("ACGT".index(b) + 1 + rng.randrange(3)) % 4] for b in ref]
    sites = P.make_sites([(p + 1, ref[p], alt[p]) for p in range(L)])
    import re
    recs = []
    for start, cigar in ((0, "600M"), (3, "600M"), (57, "300M2D298M"), (97, "250=100X250M"), (110, "100M9N500M"), (119, "592M")):
        seq, x, hap = [], start, rng.randint(0, 1)
        for n, op in re.findall(r"(\d+)([MDN=X])", cigar):
            for _ in range(int(n)):
                if op in "M=X":
                    seq.append(rng.choice("ACGT") if rng.random() < 0.05 else (alt[x] if (x * 7 + hap) % 3 == 0 else ref[x]))
                x += 1
        assert x < L
        recs.append((start, cigar, "".join(seq)))
    rs = _readset(recs)
    assert all(s > 2 * 256 for s in _site_span(rs, sites))
    exp = _check(eng, rs, sites)
    # the seams of the first read lie at its sites 256 and 504 (windows advance by 256 - K): all K predecessors are counted there
    for j in (248, 255, 256, 257, 263, 496, 503, 504, 505, 511):
        assert all(int(exp[j, k].sum()) >= 1 for k in range(K)), j
    assert int(exp.sum()) > 6 * 500 * K * 0.8                 # (~590 sites a read, 95 % of them observed, K pairs each)


def test_one_site_pair_under_five_thousand_reads(eng):
    rng = random.Random(6)
    recs = [(100, "2M", rng.choice(["AG", "AG", "CT", "CT", "AT", "CG", "NG", "AA"])) for _ in range(5000)]
    sites = P.make_sites([(101, "A", "C"), (102, "G", "T")])
    exp = _check(eng, _readset(recs), sites)
    assert int(exp[1, 0, 0]) > 2000 and int(exp[1, 0, 1]) > 1000 and int(exp.sum()) < 5000


def test_the_filters_decide_who_votes(eng):
    _, rs, sites, _, _, exp = _gen(0)
    failing = [i for i in range(len(rs)) if not P.votes(rs.reads[i], P.DEFAULT_PARAMS)]
    assert len(failing) >= 20
    eng.load_reads(rs)
    assert np.array_equal(eng.phase_links(sites), exp)
    eng.set_params(min_mq=0, excl_flags=0)                    # the reads already loaded are filtered anew
    loose = dict(min_mq=0, excl_flags=0)
    got = eng.phase_links(sites)
    assert not np.array_equal(got, exp) and np.array_equal(got, P.links(rs, sites, loose))
    eng.set_params(min_mq=5, excl_flags=2316 | 16)            # the reverse strand drops out
    strict = dict(min_mq=5, excl_flags=2316 | 16)
    _check(eng, rs, sites, strict)


def test_no_sites_no_reads_and_sites_outside_every_read(eng):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    _, rs, sites, _, _, _ = _gen(0)
    eng.load_reads(rs)
    eng.set_profiling(True)
    try:
        eng.reset_kernel_stats()
        none = eng.phase_links(np.zeros(0, capi.PHASE_SITE_DTYPE))
        assert none.shape == (0, K, 2) and "k_phase_links" not in eng.kernel_stats()
        out, st = eng.phase_sites(None)
        assert len(out) == 0 and st == dict.fromkeys(P.STAT_KEYS, 0)
        eng.phase_links(sites)
        assert eng.kernel_stats()["k_phase_links"]["launches"] == 1
    finally:
        eng.set_profiling(False)
    far = P.make_sites([(p, "A", "C") for p in (7000, 7001, 7002, 9000, 2000000000)])
    assert _check(eng, rs, far).sum() == 0
    before = P.make_sites([(1, "A", "C"), (2, "A", "C"), (3, "A", "C")])
    shifted = ReadSet(rs.reads.copy(), rs.cigar, rs.seq)
    shifted.reads["pos"] += 100
    assert _check(eng, shifted, before).sum() == 0
    eng.load_reads(ReadSet.from_records([]))
    assert eng.phase_links(sites).sum() == 0 and eng.phase_links(sites).shape == (len(sites), K, 2)


BAD_SITES = [
    ("unsorted", [(10, "A", "C"), (30, "A", "C"), (20, "A", "C")], {}, 2),
    ("duplicate", [(10, "A", "C"), (10, "A", "G")], {}, 1),
    ("pos_below_1", [(0, "A", "C")], {}, 0),
    ("bad_ref_code", [(5, "A", "C"), (6, "A", "C")], dict(ref=3), 1),
    ("ref_equals_alt", [(5, "A", "C")], dict(alt=1), 0),
]


@pytest.mark.parametrize("name, rows, patch, index", BAD_SITES, ids=[b[0] for b in BAD_SITES])
def test_bad_site_tables_name_the_index(eng, name, rows, patch, index):
    from clair3_rna_amd import capi
    sites = P.make_sites(rows)
    for k, v in patch.items():
        sites[k][index] = v
    eng.load_reads(_readset([(0, "40M", "A" * 40)]))
    with pytest.raises(capi.C3RError, match="candidate site %d:" % index):
        eng.phase_links(sites)
    sites = P.make_sites([(5, "A", "C"), (6, "A", "C")])
    sites["ps"], sites["h1"] = -7, 9                          # ignored on input
    assert eng.phase_links(sites)[1, 0].tolist() == [1, 0]


# ---- 2. the call leaves everything else alone
def _scan_bytes(eng, ref):
    n = eng.scan(1, len(ref))
    return n, eng.tensors(rescaled=True).tobytes(), eng.tensors(rescaled=False).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()


@pytest.mark.parametrize("channels", [18, 30])
def test_a_scan_is_the_same_with_and_without_the_call(eng, channels):
    ref, rs, sites, _, _, _ = _gen(1)
    tagged = hapref.with_hp(rs, (np.arange(len(rs)) % 3).astype(np.uint8))
    eng.set_params(channels=channels, min_coverage=2)
    eng.load_reads(tagged)
    eng.set_reference(1, ref)
    plain = _scan_bytes(eng, ref)
    assert plain[0] > 20
    eng.load_reads(tagged)
    assert eng.phase_links(sites).sum() > 0
    assert _scan_bytes(eng, ref) == plain
    assert eng.phase_links(sites).sum() > 0                   # after the scan: what it left is still there
    assert (eng.tensors(rescaled=True).tobytes(), eng.sites().tobytes(), eng.tokens().tobytes()) == (plain[1], plain[3], plain[4])
    assert _scan_bytes(eng, ref) == plain


def test_haplotags_under_a_set_table_are_unchanged(eng):
    _, rs, sites, truth, _, _ = _gen(2)
    table = sites.copy()
    table["ps"], table["h1"] = 1000 + np.arange(len(sites)) // 10, truth
    eng.set_phase_sites(table)
    eng.load_reads(rs)
    before = eng.haplotags()
    assert before[1]["n_hp1"] > 50 and before[1]["n_hp2"] > 50
    other = sites[::2].copy()                                 # another table than the one that is set
    assert eng.phase_links(other).sum() > 0
    after = eng.haplotags()
    assert after[0].tolist() == before[0].tolist() and after[1] == before[1]
    assert before[0].tolist() == hapref.haplotag(rs, table)[0].tolist()


# ---- 3. the entry points agree
@pytest.mark.parametrize("seed", [0, 3])
def test_phase_sites_equals_the_restatement_and_feeds_the_haplotagging(eng, seed):
    from clair3_rna_amd import phasing
    _, rs, sites, truth, _, lk = _gen(seed)
    eng.load_reads(rs)
    out, st = eng.phase_sites(sites)
    want, wst = P.resolve(sites, lk)
    assert P.equal_sites(out, want) and st == wst and st["n_phased"] > len(sites) // 2
    out1, st1 = eng.phase_sites(sites, min_reads=1, min_agree_pct=100)
    want1, wst1 = P.resolve(sites, lk, 1, 100)
    assert P.equal_sites(out1, want1) and st1 == wst1
    phased = phasing.phased_only(out)
    assert len(phased) == st["n_phased"] and (phased["ps"] >= 0).all()
    eng.set_phase_sites(phased)
    tags, tst = eng.haplotags()
    exp, est, _ = hapref.haplotag(rs, phased)
    assert tags.tolist() == exp.tolist() and tst == est and est["n_hp1"] > 50 and est["n_hp2"] > 50


# ---- 4. drivers, on the two-contig BAM of the haplotagging tests' driver cases
@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    from clair3_rna_amd import bam, bamio, io, synth
    tmp = str(tmp_path_factory.mktemp("phase_drivers"))
    contigs, reads = [], {}
    for name, seed in (("chr1", 11), ("chr2", 12)):
        ref, rs, _, _ = hapref.gen_case(seed)
        contigs.append((name, ref))
        reads[name] = rs
    fa, w18, w30 = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "model18"), os.path.join(tmp, "model30")
    io.write_fasta(fa, contigs)
    np.save(w18 + ".c3rw.npy", synth.random_weights(18, seed=5))
    np.save(w30 + ".c3rw.npy", synth.random_weights(30, seed=5))
    bam_fn = os.path.join(tmp, "plain.bam")
    bam.write_bam(bam_fn, [(n, len(r)) for n, r in contigs], reads)
    bamio.index_build(bam_fn)
    s = dict(tmp=tmp, fa=fa, w18=w18, w30=w30, bam=bam_fn, reads=reads)
    # by hand, step 1: the unphased pass
    _call_sample(s, "hand", [])
    s["pass1"] = os.path.join(tmp, "hand", "output.vcf")
    assert os.path.isfile(s["pass1"])
    return s


def _argv(s, out, extra):
    return ["--bam_fn", s["bam"], "--ref_fn", s["fa"], "--output_dir", os.path.join(s["tmp"], out), "--pileup_model_path", s["w18"],
            "--chunk_num", "3", "--min_coverage", "2"] + list(extra)


def _call_sample(s, out, extra, compress=False):
    from clair3_rna_amd import call_sample
    assert call_sample.Run(call_sample.build_parser().parse_args(_argv(s, out, extra) + ([] if compress else ["--no_compress"])), log=lambda m: None) == 0


def _gz_text(fn):
    with gzip.open(fn, "rt") as f:
        return f.read()


def test_phase_vcf_writes_the_files_the_restatement_predicts(sample, tmp_path):
    from clair3_rna_amd import phase_vcf, phasing
    out_dir = os.path.join(sample["tmp"], "hand", "tmp", "phased_output", "phased_vcf")
    msgs = []
    written = phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", sample["pass1"], "--output_dir", out_dir]), log=msgs.append)
    assert len(msgs) == 2 and all(m.startswith("[INFO] chr") for m in msgs)
    n_cand = n_phased = 0
    for ctg in ("chr1", "chr2"):
        cands, _ = phasing.candidates_from_vcf(sample["pass1"], ctg)
        fn = os.path.join(out_dir, "phased_%s.vcf.gz" % ctg)
        if not len(cands):
            assert not os.path.exists(fn) and fn not in written
            continue
        want, st = P.phase(sample["reads"][ctg], cands)
        exp_fn = str(tmp_path / ("exp_%s.vcf.gz" % ctg))
        phasing.write_phased_vcf(sample["pass1"], ctg, want, exp_fn)
        assert fn in written and _gz_text(fn) == _gz_text(exp_fn)
        n_cand += len(cands)
        n_phased += st["n_phased"]
    print("candidates %d, phased %d" % (n_cand, n_phased))
    assert n_cand >= 10 and n_phased >= 2                     # the comparison above is about something
    sample["phased_dir"] = out_dir


def test_call_sample_with_builtin_phasing_equals_the_three_steps_by_hand(sample):
    if "phased_dir" not in sample:                            # (run alone: step 2 by hand)
        from clair3_rna_amd import phase_vcf
        sample["phased_dir"] = os.path.join(sample["tmp"], "hand", "tmp", "phased_output", "phased_vcf")
        phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", sample["bam"], "--vcf_fn", sample["pass1"], "--output_dir", sample["phased_dir"]]), log=lambda m: None)
    phased = ["--phased_pileup_model_path", sample["w30"], "--enable_phasing_model"]
    _call_sample(sample, "hand", phased + ["--phased_vcf_fn", sample["phased_dir"]])
    hand1, hand2 = open(sample["pass1"]).read(), open(os.path.join(sample["tmp"], "hand", "output_enable_phasing.vcf")).read()
    out = os.path.join(sample["tmp"], "builtin")
    stale = os.path.join(out, "tmp", "phased_output", "phased_vcf", "phased_chr9.vcf.gz")     # an earlier run's, of a contig this run does not see
    os.makedirs(os.path.dirname(stale))
    with gzip.open(stale, "wt") as f:
        f.write("chr9\t5\t.\tA\tC\t9\tPASS\t.\tGT:PS\t0|1:5\n")
    _call_sample(sample, "builtin", phased + ["--phasing", "builtin"], compress=True)
    assert not os.path.exists(stale)
    assert _gz_text(os.path.join(out, "output.vcf.gz")) == hand1
    assert _gz_text(os.path.join(out, "output_enable_phasing.vcf.gz")) == hand2
    for ctg in ("chr1", "chr2"):
        a, b = (os.path.join(d, "phased_%s.vcf.gz" % ctg) for d in (sample["phased_dir"], os.path.join(out, "tmp", "phased_output", "phased_vcf")))
        assert os.path.exists(a) == os.path.exists(b) and (not os.path.exists(a) or _gz_text(a) == _gz_text(b))
    # the phasing shows in the records: the comparison above can fail
    _call_sample(sample, "untagged", phased)
    assert open(os.path.join(sample["tmp"], "untagged", "output_enable_phasing.vcf")).read() != hand2


def test_builtin_phasing_refuses_what_it_cannot_do(sample, monkeypatch):
    from clair3_rna_amd import call_sample

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:
            call_sample.Run(call_sample.build_parser().parse_args(_argv(sample, "refused", extra)))
        assert str(e.value.code).startswith("[ERROR]") and all(w in str(e.value.code) for w in words), e.value.code

    refused(["--phasing", "builtin", "--phased_pileup_model_path", sample["w30"]], "--phasing builtin", "--enable_phasing_model")
    refused(["--phasing", "builtin", "--phased_pileup_model_path", sample["w30"], "--enable_phasing_model", "--phased_vcf_fn", sample["pass1"]],
            "--phasing builtin", "--phased_vcf_fn")
    refused(["--phasing", "builtin", "--enable_phasing_model"], "--phased_pileup_model_path")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(["--phasing", "builtin", "--phased_pileup_model_path", sample["w30"], "--enable_phasing_model"], "WORLD_SIZE", "one process")
    assert not os.path.exists(os.path.join(sample["tmp"], "refused"))
