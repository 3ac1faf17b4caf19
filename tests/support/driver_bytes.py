"""What the five drivers write for one small sample WITHOUT --left_align_indels, as hashes: tests/test_gpu_left_align.py holds them against
tests/golden/left_align_parent_bytes.json, which was recorded by running this file's `hashes` with the parent commit's package on the same
input files.  It imports nothing of tests/ and takes the package from sys.path, so that it can be run against another tree:

    python tests/support/driver_bytes.py <directory with ref.fa, plain.bam, with_indels.vcf, model18 / model30> <output directory>

Hashed: the data rows and the #CHROM line of every VCF (the ## lines name paths and commands), the counts file as it is, and the records
of the haplotagged BAM (its @PG line names the command)."""
import gzip
import hashlib
import json
import os
import sys


def _vcf(fn):
    with (gzip.open(fn, "rt") if fn.endswith(".gz") else open(fn)) as f:
        return hashlib.sha256("".join(l for l in f if not l.startswith("##")).encode()).hexdigest()


def _bam(fn):
    from clair3_rna_amd import io
    rs = io.load_reads(fn, "chr1")
    return hashlib.sha256(rs.reads.tobytes() + rs.cigar.tobytes() + rs.seq.tobytes()).hexdigest()


def hashes(src, out):
    """{name: sha256} of the files the drivers write for the sample in `src`, under `out`."""
    from clair3_rna_amd import call_sample, call_var_bam, hap_vcf, haplotag_bam, phase_vcf
    fa, bam, with_, w18, w30 = (os.path.join(src, n) for n in ("ref.fa", "plain.bam", "with_indels.vcf", "model18", "model30"))
    quiet = lambda m: None
    got = {}
    # 1. the one-command flow with every indel step behind it
    one = os.path.join(out, "one")
    argv = ["--bam_fn", bam, "--ref_fn", fa, "--output_dir", one, "--pileup_model_path", w18, "--phased_pileup_model_path", w30, "--chunk_num", "3", "--min_coverage", "2",
            "--enable_phasing_model", "--phasing", "builtin", "--phasing_indels", "--phase_output", "--phase_indels", "--haplotagged_bam"]
    assert call_sample.Run(call_sample.build_parser().parse_args(argv), log=quiet) == 0
    for name in ("output.vcf.gz", "output_enable_phasing.vcf.gz", "output_enable_phasing_phased.vcf.gz", os.path.join("tmp", "phased_output", "phased_vcf", "phased_chr1.vcf.gz")):
        got["call_sample/" + name] = _vcf(os.path.join(one, name))
    with open(os.path.join(one, "output_enable_phasing_hap_counts.tsv"), "rb") as f:
        got["call_sample/hap_counts.tsv"] = hashlib.sha256(f.read()).hexdigest()
    got["call_sample/chr1.bam"] = _bam(os.path.join(one, "tmp", "phased_output", "phased_bam", "chr1.bam"))
    # 2. the three stand-alone drivers on the VCF that holds every planted row
    pdir = os.path.join(out, "phased_vcf")
    phase_vcf.Run(phase_vcf.build_parser().parse_args(["--bam_fn", bam, "--vcf_fn", with_, "--output_dir", pdir, "--indels", "--merge_levels", "1"]), log=quiet)
    got["phase_vcf/phased_chr1.vcf.gz"] = _vcf(os.path.join(pdir, "phased_chr1.vcf.gz"))
    hv = os.path.join(out, "hap.vcf")
    hap_vcf.Run(hap_vcf.build_parser().parse_args(["--bam_fn", bam, "--vcf_fn", with_, "--phased_vcf_fn", pdir, "--output_fn", hv, "--hap_counts_fn", hv + ".tsv", "--indels",
                                                   "--haplotag_indels"]), log=quiet)
    got["hap_vcf/hap.vcf"] = _vcf(hv)
    with open(hv + ".tsv", "rb") as f:
        got["hap_vcf/hap_counts.tsv"] = hashlib.sha256(f.read()).hexdigest()
    bdir = os.path.join(out, "phased_bam")
    haplotag_bam.Run(haplotag_bam.build_parser().parse_args(["--bam_fn", bam, "--phased_vcf_fn", pdir, "--output_dir", bdir, "--haplotag_indels"]), log=quiet)
    got["haplotag_bam/chr1.bam"] = _bam(os.path.join(bdir, "chr1.bam"))
    # 3. one chunk of the per-chunk driver, tagged from the allele table
    chunk = os.path.join(out, "chunk.vcf")
    argv = ["--chkpnt_fn", w30, "--bam_fn", bam, "--ref_fn", fa, "--call_fn", chunk, "--ctgName", "chr1", "--pileup", "--chunk_id", "2", "--chunk_num", "3", "--minCoverage", "2",
            "--enable_phasing_model", "True", "--phased_vcf_fn", pdir, "--haplotag_indels"]
    call_var_bam.Run(call_var_bam.build_parser().parse_args(argv))
    got["call_var_bam/chunk.vcf"] = _vcf(chunk)
    return got


if __name__ == "__main__":
    print(json.dumps(hashes(sys.argv[1], sys.argv[2]), indent=1, sort_keys=True))
