"""Randomised parity: read sets with arbitrary (legal and odd) CIGARs through the HIP path vs the oracle, column by column
and line by line.  Seeds are fixed; every case is small, so a failure message carries the whole input."""
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from clair3_rna_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


_seeds, _case, _rand_cigar = H._seeds, H._case, H._rand_cigar          # the generator and the tests' bodies are shared with tests/test_gpu_deep_routes.py (tests/helpers.py)


@pytest.mark.parametrize("kw", [dict(), dict(head_tail=1), dict(splice_padding=1), dict(splice_padding=1, head_tail=1),
                                dict(channels=30), dict(channels=30, head_tail=1), dict(snp_min_af=0.0), dict(min_mq=0, min_coverage=1)])
def test_random_cigars_match_the_oracle(eng, kw):
    n_cases, n_lines = H.fuzz_match_oracle(eng, _seeds(120), kw, case_base=1000 * len(kw))
    assert n_cases == len(_seeds(120)) and n_lines > 300, n_lines


@pytest.mark.parametrize("kw", [dict(), dict(channels=30), dict(head_tail=1), dict(splice_padding=1)])
def test_random_cigars_with_the_samtools_1_11_printer(eng, kw):
    """c3r_params_t.mpileup_compat = 1: an I immediately followed by a D shows both on the insertion's column (`C+2TT-1N`: one more D / d,
    D1 / d1 count, a deletion token behind the insertion token).  The generator deals I next to D often (leading, after N, after D)
    and pads next to insertions: samtools >= 1.11 prints those inside the insertion as '*' / '#' (`+3T*T`; c3r_padins_t)."""
    n_lines, n_both, n_padded, n_refused = H.fuzz_samtools_1_11(eng, _seeds(60), kw, case_base=70000 + 100 * len(kw))
    assert n_lines > 150 and n_both > 40 and n_padded > 3 and n_refused <= 0.05 * len(_seeds(60)) + 1, (n_lines, n_both, n_padded, n_refused)


def test_samtools_1_11_printer_known_answers_and_pads(eng):
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    ref = "ACGT" * 30
    recs = [dict(pos=10, cigar="6M2I1D6M", seq="GTACGTTTTACGTA") for _ in range(4)] + [dict(pos=10, cigar="13M", seq="GTACGTACGTACG", flag=16) for _ in range(4)]
    rs = ReadSet.from_records(recs)
    out = {}
    eng.load_reads(ReadSet.from_records([]))
    for compat in (0, 1):
        eng.params = capi.default_params()
        eng.set_params(min_coverage=2, mpileup_compat=compat, head_tail=1)        # (head/tail calling: the reads are shorter than a window)
        got = H.engine_chunk(eng, rs, ref, 1, 1, len(ref))
        exp = H.oracle_chunk(rs, ref, 1, 1, len(ref), min_coverage=2, mpileup_compat=compat, head_tail=True)
        assert got["lines"] == exp["lines"] and len(got["lines"]) > 0, H.first_diff(got["lines"], exp["lines"])
        line = [l for l in got["lines"] if l.split("\t")[1] == "16"][0]                # the insertion sits on the sixth aligned base
        out[compat] = line.split("\t")[4]
        tk = got["tokens"][got["tokens"]["indel"] > 0]
        assert (tk["del_after"] == (1 if compat else 0)).all() and len(tk) >= 4
    assert out == {0: "8-ITTT 4 RT 4", 1: "8-ITTT 4 DA 4"}, out      # position 16 gains the deletion
    # samtools >= 1.11 shows the pads of a run of I ops inside the insertion: '*' for a forward read, '#' for a reverse one (--reverse-del).
    # Four forward reads `4M1I1P1I4M` and three reverse ones make two alleles of the same bases; a leading pad decides the channel
    # (key[1] in "ACGTN*": I for the forward reads, i for the reverse ones) and `I P D` shows the deletion behind the padded insertion
    padded = ([dict(pos=10, cigar="6M", seq="GTACGT")] + [dict(pos=12, cigar="4M1I1P1I4M", seq="ACGTTTACGT") for _ in range(4)] +
              [dict(pos=12, cigar="4M1I1P1I4M", seq="ACGTTTACGT", flag=16) for _ in range(3)] + [dict(pos=12, cigar="4M1P2I4M", seq="ACGTTTACGT") for _ in range(2)] +
              [dict(pos=12, cigar="4M1P2I4M", seq="ACGTTTACGT", flag=16)] + [dict(pos=12, cigar="4M2I1P1D3M", seq="ACGTTTCGT") for _ in range(2)])
    rs = ReadSet.from_records(padded)
    eng.params = capi.default_params()
    eng.set_params(min_coverage=2, mpileup_compat=1, head_tail=1)
    got = H.engine_chunk(eng, rs, ref, 1, 1, len(ref))
    exp = H.oracle_chunk(rs, ref, 1, 1, len(ref), min_coverage=2, mpileup_compat=1, head_tail=True)
    assert got["lines"] == exp["lines"] and len(got["lines"]) > 0, H.first_diff(got["lines"], exp["lines"])
    pi = eng.pad_insertions()
    assert len(pi) == 12 and set(pi["total"].tolist()) == {3} and set(pi["pad_mask"].tolist()) == {1, 2, 4} and (pi["n_bases"] == 2).all()
    alt16 = [l for l in got["lines"] if l.split("\t")[1] == "16"][0].split("\t")[4]
    assert alt16 == "13-ITT*T 4 ITT#T 3 IT*TT 2 IT#TT 1 ITTT* 2 DA 2", alt16
    row16 = [r for r in exp["rows"] if r.split("\t")[1] == "16"][0].split("\t")[4]
    assert row16.count("+3T*T") == 4 and row16.count("+3t#t") == 3 and row16.count("+3*TT") == 2 and row16.count("+3#tt") == 1 and row16.count("+3TT*-1N") == 2
    col = eng.columns()
    c16 = col["cols"][16 - col["region_start"]]
    assert (c16[4], c16[5], c16[13], c16[14]) == (8, 4, 4, 3), c16      # I = 4 + 2 + 2, I1 = 4; i = 3 + 1, i1 = 3
    # the C++ decoder builds the same allele text from the packed tokens
    w = synth_weights()
    eng.load_weights(w, 18)
    probs = eng.infer()
    from clair3_rna_amd import decode
    f = [l.split("\t") for l in exp["lines"]]
    assert eng.call_rows("chr20") == decode.vcf_rows("chr20", [int(x[1]) for x in f], [x[2] for x in f], [x[4] for x in f], probs)
    # a run of more than 64 characters is refused (the table describes the pads by a 64-bit mask); the <= 1.10 text takes it
    bad = ReadSet.from_records([dict(pos=10, cigar="6M", seq="GTACGT"), dict(pos=12, cigar="4M40I1P30I4M", seq="ACGT" + "T" * 70 + "ACGT")])
    with pytest.raises(capi.C3RError, match=r"read 1: an insertion with pads \(P ops\) of more than 64 characters"):
        eng.load_reads(bad)
    eng.params = capi.default_params()
    eng.set_params()
    eng.load_reads(bad)
    eng.set_reference(1, ref)
    eng.scan(1, len(ref))
    assert len(eng.pad_insertions()) == 0


def synth_weights():
    from clair3_rna_amd import synth
    w = synth.random_weights(18, seed=4242)
    w[-24 * 129:] *= 6.0
    return w


@pytest.mark.parametrize("mode", ["lbed", "cbed", "both_beds", "sites", "subregion", "deep"])
def test_random_cigars_with_filters_and_regions(eng, mode):
    """The same random read sets through the -l BED, the confident BED, a genotyping site list, a sub-region with a shifted
    reference slice, and at depths that cross the 216 rescale threshold."""
    n_lines = H.fuzz_filters_and_regions(eng, _seeds(60), mode, case_base=50000, rng_base=7000)
    assert n_lines > (20 if mode in ("sites", "lbed", "both_beds") else 200), (mode, n_lines)


@pytest.mark.parametrize("compat", [0, 1])
def test_random_cigars_decode_rows_cpp_equals_python_and_regions(eng, compat):
    """On the random read sets: (1) c3r_call_rows (C++: tokens -> ordered alt_info -> decode -> row text) equals the Python
    path fed with the ORACLE's alt_info strings; (2) a multi-region scan over random chunk boundaries equals successive
    scans.  Random weights make every genotype class and the decoder's retry loop show up.  compat = 1: the samtools >= 1.11
    text (a deletion token behind an insertion token travels in the packed token stream as del_after)."""
    n_rows, kinds = H.fuzz_decode_rows_and_regions(eng, _seeds(60), compat, case_base=80000, rng_base=9000)
    assert n_rows > 1500 and {"0/0", "0/1", "1/1"} <= kinds, (n_rows, kinds)


@pytest.mark.parametrize("channels", [18, 30])
def test_mpileup_depth_cap(eng, channels):
    """samtools mpileup -d (default 8000, in force in the reference): htslib discards a read that is not the first pushed
    for its start position while more than max_depth reads are live.  Small caps on replicated random read sets make the
    rule bite; the discarded reads must vanish from counts, coverage, tokens, haplotype channels and skip counts alike, and
    per region (a read may survive in one chunk's scan and not in its neighbour's)."""
    n_dropped_cases = H.fuzz_depth_cap(eng, _seeds(40), channels, case_base=60000, rng_base=4000)
    assert n_dropped_cases > 25, n_dropped_cases          # the cap changed the output in most cases
