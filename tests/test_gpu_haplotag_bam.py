"""The haplotagged BAM on the device: haplotag_bam and call_sample --haplotagged_bam write the tags k_haplotag computes, checked against the
plain-Python restatements (tests/hapref.py: tags, tests/hapcountref.py: phase sets) through tests/bamref.py — a BAM reader that shares
nothing with the writer.  Reads come from hapref.gen_case (83 reads a contig; 400 where call_sample has to call variants first): every
class (untagged, HP1, HP2) is present in every test."""
import os

import numpy as np
import pytest

from tests import bamref, hapcountref, hapref
from tests.test_haplotag_bam import PHASE, check_tagged_files, two_contig_sample

pytestmark = pytest.mark.gpu


def _haplotag(s, out_dir, extra=()):
    from clair3_rna_amd import haplotag_bam
    msgs = []
    done = haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", s["bam"], "--phased_vcf_fn", s["per"], "--output_dir", out_dir] + list(extra)),
                            log=msgs.append)
    return done, msgs


def _add_reference_and_weights(s, d):
    from clair3_rna_amd import io, synth
    s["fa"], s["w30"] = os.path.join(d, "ref.fa"), os.path.join(d, "model30")
    io.write_fasta(s["fa"], [(n, s["case"][n][0]) for n, _ in s["contigs"]] + [("chrEmpty", "ACGT" * 1250)])
    np.save(s["w30"] + ".c3rw.npy", synth.random_weights(30, seed=5))
    return s


@pytest.fixture(scope="module")
def tagged(tmp_path_factory):
    """The two-contig sample (chr1 phased, chr2 not, chrEmpty without a record) and what haplotag_bam makes of it on the device."""
    d = str(tmp_path_factory.mktemp("gpu_hapbam"))
    s = _add_reference_and_weights(two_contig_sample(d), d)
    s["out"] = os.path.join(d, "tagged")
    s["done"], s["msgs"] = _haplotag(s, s["out"], ["--threads", "4"])
    return s


def test_a_the_files_hold_the_restatements_tags_and_sets(tagged):
    assert sorted(tagged["done"]) == ["chr1", "chr2"]
    check_tagged_files(tagged, tagged["out"])                # HP and PS of every record; all three classes on chr1; chr2 untagged
    st = tagged["done"]["chr1"]
    tags = hapref.haplotag(tagged["reads"]["chr1"], tagged["case"]["chr1"][1])[0]
    assert (st["hp1"], st["hp2"], st["records"], st["unpaired"]) == (int((tags == 1).sum()), int((tags == 2).sum()), len(tags), 0)
    assert min(st["hp1"], st["hp2"], st["records"] - st["tagged"]) >= 1
    assert tagged["done"]["chr2"]["tagged"] == 0 and "every read untagged" in tagged["msgs"][1]


def _call_chunk(s, bam_fn, out, extra):
    from clair3_rna_amd import call_var_bam
    argv = ["--chkpnt_fn", s["w30"], "--bam_fn", bam_fn, "--ref_fn", s["fa"], "--ctgName", "chr1", "--pileup", "--enable_phasing_model", "True",
            "--minCoverage", "2", "--call_fn", out + ".vcf", "--tensor_dump_fn", out + ".txt"] + list(extra)
    assert call_var_bam.Run(call_var_bam.build_parser().parse_args(argv)) == 0
    return open(out + ".vcf").read(), open(out + ".txt").read()


def test_b_the_tagged_bam_alone_calls_what_the_phased_vcf_calls(tagged, tmp_path):
    """Closure: the 30-channel pass on <ctg>.bam WITHOUT --phased_vcf_fn (the BAM's own HP tags count) writes the bytes of the pass on the
    untagged BAM with --phased_vcf_fn — records and tensor lines."""
    own = _call_chunk(tagged, os.path.join(tagged["out"], "chr1.bam"), str(tmp_path / "own"), [])
    device = _call_chunk(tagged, tagged["bam"], str(tmp_path / "device"), ["--phased_vcf_fn", tagged["per"]])
    assert own == device and own[1].count("\n") > 20
    untagged = _call_chunk(tagged, tagged["bam"], str(tmp_path / "untagged"), [])
    assert untagged[1] != own[1]                              # the tags show in the tensors: the comparison above can fail
    st = tagged["done"]["chr1"]
    assert min(st["hp1"], st["hp2"], st["records"] - st["tagged"]) >= 1


def test_c_call_sample_writes_the_reference_flows_files_and_changes_nothing_else(tmp_path):
    """call_sample --phasing builtin on two contigs of gen_case reads (the sample of tests/test_gpu_phase.py's drivers), with and without
    --haplotagged_bam."""
    from clair3_rna_amd import bam, bamio, call_sample, io, phasedvcf, synth
    d = str(tmp_path)
    contigs, reads = [], {}
    for name, seed in (("chr1", 11), ("chr2", 12)):
        ref, rs, _, _ = hapref.gen_case(seed)
        contigs.append((name, ref))
        reads[name] = rs
    fa, w18, w30, bam_fn = os.path.join(d, "ref.fa"), os.path.join(d, "model18"), os.path.join(d, "model30"), os.path.join(d, "plain.bam")
    io.write_fasta(fa, contigs)
    np.save(w18 + ".c3rw.npy", synth.random_weights(18, seed=5))
    np.save(w30 + ".c3rw.npy", synth.random_weights(30, seed=5))
    bam.write_bam(bam_fn, [(n, len(r)) for n, r in contigs], reads)
    bamio.index_build(bam_fn)

    def run(out, extra):
        argv = ["--bam_fn", bam_fn, "--ref_fn", fa, "--output_dir", out, "--pileup_model_path", w18, "--phased_pileup_model_path", w30,
                "--enable_phasing_model", "--phasing", "builtin", "--chunk_num", "3", "--min_coverage", "2"] + list(extra)
        assert call_sample.Run(call_sample.build_parser().parse_args(argv), log=lambda m: None) == 0

    without, with_flag = os.path.join(d, "cs_without"), os.path.join(d, "cs_with")
    run(without, [])
    run(with_flag, ["--haplotagged_bam"])
    assert not os.path.exists(os.path.join(without, "tmp", "phased_output", "phased_bam"))
    files = lambda out: sorted(n for n in os.listdir(out) if os.path.isfile(os.path.join(out, n)))
    assert files(with_flag) == files(without) and "output_enable_phasing.vcf.gz" in files(without) and "output.vcf.gz" in files(without)
    for n in files(without):                                  # no file more and no byte different
        if n.endswith((".vcf.gz", ".tbi")):
            assert open(os.path.join(with_flag, n), "rb").read() == open(os.path.join(without, n), "rb").read(), n
    bam_dir = os.path.join(with_flag, "tmp", "phased_output", "phased_bam")
    assert sorted(os.listdir(bam_dir)) == ["chr1.bam", "chr1.bam.bai", "chr2.bam", "chr2.bam.bai"]      # one indexed BAM per processed contig
    classes = set()
    for ctg in ("chr1", "chr2"):
        table = phasedvcf.contig_sites(os.path.join(with_flag, "tmp", "phased_output", "phased_vcf"), ctg)     # what the second pass read
        rs = reads[ctg]
        got = bamref.Bam(os.path.join(bam_dir, ctg + ".bam"))
        hp = [r.tag("HP")[1] if r.tag("HP") else 0 for r in got.records]
        assert len(hp) == len(rs) and hp == hapref.haplotag(rs, table)[0].tolist()
        assert [r.tag("PS")[1] if r.tag("PS") else -1 for r in got.records] == hapcountref.read_phase_sets(rs, table).tolist()
        assert b"@PG\tID:c3r_haplotag\t" in got.text
        with bamio.BamFile(os.path.join(bam_dir, ctg + ".bam")) as bf:
            assert bf.has_index and bf.fetch(ctg, 2000, 2500).reads["hp"].tolist() == [h for h, r in zip(hp, got.records) if r.pos < 2500 and _end(r) > 2000]
        classes |= set(hp)
    assert classes == {0, 1, 2}


def _end(r):
    return r.pos + max(1, sum(c >> 4 for c in r.cigar if (c & 15) in (0, 2, 3, 7, 8)))


def test_d_wrong_tags_in_the_input_are_replaced_by_the_devices(tmp_path):
    s = two_contig_sample(str(tmp_path), tag_input=True)
    assert all(r.tag("HP") == ("C", 2) for r in bamref.Bam(s["bam"]).records)
    out = str(tmp_path / "tagged")
    done, _ = _haplotag(s, out)
    check_tagged_files(s, out)                                # chr1: the restatement's tags, all three classes; chr2: stripped
    assert done["chr1"]["stripped"] == len(s["reads"]["chr1"]) and done["chr2"]["stripped"] == len(s["reads"]["chr2"])
    assert not any(t in PHASE for r in bamref.Bam(os.path.join(out, "chr2.bam")).records for t, _, _ in r.aux)
