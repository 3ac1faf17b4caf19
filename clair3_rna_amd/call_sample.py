"""Whole-sample pileup calling in ONE process: STEP 1 + STEP 2 of run_clair3_rna without the per-chunk processes and files.

The reference runs `parallel ... clair3_rna.py call_var_bam ... :::: tmp/CHUNK_LIST` (run_clair3_rna:678-708: one Python +
pypy + samtools process group per (contig, chunk_id, chunk_num) row, each writing tmp/pileup_output/pileup_{ctg}_{chunk}.vcf)
and then `sort_vcf` over that directory (run_clair3_rna:710-726).  Here the same CHUNK_LIST (contig selection and chunk
counts of run_clair3_rna:310-449) is walked contig by contig: all chunks of a contig go through the tensor build in one
c3r_pileup_scan_regions call and through the network as one batch, the rows are decoded by libc3r's host threads and merged
in memory by sort_vcf.SampleMerger.  The result — `<output_dir>/<output_prefix>.vcf.gz` (+ .tbi, + `_no_tagging`) — is
byte-identical to running call_var_bam per CHUNK_LIST row and merging with sort_vcf (tests/test_gpu_sample.py).

One thing is pinned that the reference leaves open.  Adjacent chunks overlap by the 33 bp halo; the seam position itself is
emitted by both, and with head/tail calling both also emit the candidates inside the halo — from different windows (one
chunk's stream ends there, the other's begins).  sort_vcf keeps the row of whichever per-chunk file os.listdir returns last
(src/sort_vcf.py:204-236), i.e. an arbitrary one.  Here the LATER chunk's row is kept, always.

The host stages overlap on threads (the GIL is released inside libc3r / libc3r_io):
    fetch    BAM region fetch + reference slice of the next contigs          (libc3r_io.so, FASTA read; --fetch_threads)
    context  per contig, on one of --contexts GPU contexts, each with its own thread and HIP stream: read normalisation +
             uploads, tensor build, network, alt_info + genotype decode + row text (libc3r.so) — while one context waits
             for its kernels the others prepare or decode
    merge    per-record rules + order, in calling order as the contigs come out (libc3r_io.so)

In this file: `_plan` checks the flags — all of their rules, before anything is created — and lists the steps of the run (the pass or passes, and
phase_vcf / hap_vcf / haplotag_bam around them); `Run` executes them.  A pass (`_run_pass`) is four stages: set-up (`_set_up` -> one `_Pass` object:
ranks and host budget, paths, plan_chunks, BED split, CMD, the index link, this rank's contigs, the REDIportal table), the contexts' bring-up
(`_Engines`), the per-contig pipeline (`_Pipeline`, with `_FetchJoin`, `_device_stage` and `_decode_stage`; a contig goes from stage to stage as one
`ContigResult`), and rank 0's assembly and finalisation (`_assemble`, `_finish`).  Which phase table a contig gets is phasedvcf.PhaseSource's business.

Not covered (use the reference's own orchestration around call_var_bam for these): gVCF.  `--enable_phasing_model` runs the 30-channel pass only — the second half of
run_clair3_rna:729-852 — either on an already haplotagged BAM (HP tags), or, with `--phased_vcf_fn`, on the ORIGINAL BAM plus
the phased VCF(s) the phasing step wrote: the reads are then haplotagged on the GPU while they are prepared (c3r_set_phase_sites),
and the reference's "Haplotag the BAM" commands (run_clair3_rna:769-801: whatshap / longphase haplotag, samtools index) are not needed.
`--enable_phasing_model --phasing builtin` (both model paths, no --phased_vcf_fn) is the whole phased flow in this process, with no external
tool between the passes: the unphased run (<prefix>.vcf.gz), phase_vcf on that file — the built-in phasing of its heterozygous SNVs from read
linkage on the GPU, a greedy linkage chain, not whatshap's wMEC (include/c3r.h: c3r_phase_links / c3r_phase_resolve) — into
<output_dir>/tmp/phased_output/phased_vcf, then the run with --phased_vcf_fn on that directory (<prefix>_enable_phasing.vcf.gz).
`--phase_merge_levels N` (default 0: off) is handed to phase_vcf as --merge_levels: up to N levels of the block-merge stage after the chain.  One process
only: under torch.distributed.run (WORLD_SIZE > 1) it exits with an [ERROR] line — run the three steps as three commands there.
`--phasing_indels` (with --phasing builtin; default off, as `whatshap phase --indels` is) hands phase_vcf --indels: heterozygous insertions, deletions and
1/2 rows are phased between the passes too (include/c3r.h: c3r_phase_allele_links; CIGAR-position alleles, no realignment), and the second pass — and
--phase_output / --haplotagged_bam behind it — reads the directory with the allele table, as `--phased_vcf_fn DIR --haplotag_indels` does.
`--phase_output` (with --enable_phasing_model and --phased_vcf_fn or --phasing builtin; one process only) adds a step behind the phased pass:
hap_vcf phases the heterozygous SNVs of <prefix>_enable_phasing.vcf.gz from per-haplotype allele counts on the GPU into
<prefix>_enable_phasing_phased.vcf.gz and writes the counts to <prefix>_enable_phasing_hap_counts.tsv; without the flag nothing changes.
`--phase_indels` (with --phase_output) hands hap_vcf --indels: heterozygous insertions, deletions and rows with two ALT alleles are phased too,
by CIGAR-position alleles (no realignment, no left-alignment, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes)); without it both files are what they were.
`--hap_realign [W]` (with --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin; excludes --left_align_indels) lifts "no realignment" for every
step that holds reads against a site table: the flag and --ref_fn are handed to phase_vcf, to the 30-channel pass, to hap_vcf and to haplotag_bam (include/c3r.h:
c3r_set_hap_realign); the unphased pass holds its reads against no table and does not get it.  Unit costs, no quality weights; a window stops at a splice junction
unless `--hap_realign_spliced` is given, which goes to exactly the steps that get `--hap_realign` (include/c3r.h: c3r_set_hap_realign_spliced).
`--left_align_indels` (with one of --phase_indels, --haplotag_indels, --phasing_indels) lifts "no left-alignment" for every step that reads indels: the flag and
--ref_fn are handed to phase_vcf, to the 30-channel pass, to hap_vcf and to haplotag_bam (include/c3r.h: c3r_set_hap_left_align).  A shift stops at a read's M run's
start, at an N or another indel; there is still no realignment and there are no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes); agreement with whatshap is not measured.
`--haplotagged_bam` (same conditions as --phase_output, and combinable with it) adds the step the reference's "Haplotag the BAM" commands stand
for: haplotag_bam writes <output_dir>/tmp/phased_output/phased_bam/<ctg>.bam + .bai for the contigs the run processed — every record of the
contig, with the HP / PS tags the GPU computed from the phase table the second pass read; without the flag nothing changes.
`--hap_expression_bed BED` (same conditions, combinable with both) adds one more step behind them: hap_expr counts the reads of each haplotype
and phase set over every interval of BED on the GPU (include/c3r.h: the rule `hap_regions`) into <prefix>_enable_phasing_hap_expression.tsv,
with the tagging flags haplotag_bam gets; `--hap_expression_stranded same|reverse` is handed over as --stranded; without the flag nothing changes.
`--hap_expression_group_by_name` (needs --hap_expression_bed) hands hap_expr --group_by_name: the gene-level count, the BED lines of one name one
group and a read counted once per group (include/c3r.h: the rule `hap_groups`), into <prefix>_enable_phasing_hap_expression_by_name.tsv instead.
`--hap_junctions` (same conditions, combinable with all three) adds one more step behind them: hap_junctions counts, on the GPU, the reads of
each haplotype and phase set per splice junction the reads hold (include/c3r.h: the rule `hap_junctions`) into
<prefix>_enable_phasing_hap_junctions.tsv, with the tagging flags hap_expr gets and --ref_fn for MOTIF / STRAND; without the flag nothing changes.

    python -m clair3_rna_amd.call_sample --bam_fn x.bam --ref_fn ref.fa --pileup_model_path W --output_dir out
    python -m clair3_rna_amd.call_sample --bam_fn x.bam --ref_fn ref.fa --pileup_model_path W --phased_pileup_model_path W30 \
        --enable_phasing_model --phased_vcf_fn out/tmp/phased_output/phased_vcf --output_dir out
    python -m clair3_rna_amd.call_sample --bam_fn x.bam --ref_fn ref.fa --pileup_model_path W --phased_pileup_model_path W30 \
        --enable_phasing_model --phasing builtin --output_dir out
"""
import argparse
import collections
import importlib
import os
import sys
import threading
from concurrent.futures import ThreadPoolExecutor
from time import time

import numpy as np

from . import io, mpileup_compat, sort_vcf, vcf
from .reads import READ_DTYPE, ReadSet
from .call_var_bam import existing, resolve_region


def _env_precision():
    from . import capi           # (ctypes declarations only: libc3r.so is opened when an Engine is made)
    return capi.env_precision()

MAJOR_CONTIGS_ORDER = ["chr" + str(a) for a in list(range(1, 23)) + ["X", "Y"]] + [str(a) for a in list(range(1, 23)) + ["X", "Y"]]
CHUNK_SIZE = 5000000            # shared/param_p.py:91
EXPAND = 33                     # param.no_of_positions: split_extend_bed widens every interval by one window


def _bed_contigs(bed_fn):
    names = []
    with io._open_text(bed_fn) as f:
        for row in f:
            if row.strip() and row[0] != "#":
                c = row.split()[0]
                if c not in names:
                    names.append(c)
    return names


def _vcf_contigs(vcf_fn):
    names = set()
    with io._open_text(vcf_fn) as f:
        for row in f:
            if row[0] != "#":
                names.add(row.split(None, 1)[0])
    return names


def plan_chunks(ref_fn, ctg_name=None, include_all_ctgs=False, bed_fn=None, vcf_fn=None, chunk_size=CHUNK_SIZE, chunk_num=None):
    """-> ([contig, ...] in calling order, {contig: chunk_num}): run_clair3_rna:310-389 + :441-449 (CHUNK_LIST)."""
    listed = set(ctg_name.split(",")) if ctg_name else None
    in_bed = set(_bed_contigs(bed_fn)) if bed_fn else None
    in_vcf = _vcf_contigs(vcf_fn) if vcf_fn else None
    contig_set = set(listed) if listed else set()
    if listed:
        if in_bed is not None:
            contig_set &= in_bed
        if in_vcf is not None:
            contig_set &= in_vcf
    else:
        if in_bed is not None:
            contig_set |= in_bed
        if in_vcf is not None:
            contig_set |= in_vcf
    restricted = bool(in_bed is not None or listed or in_vcf is not None)
    chunks = {}
    for name, length, _o, _b, _w in io.read_fai(ref_fn):
        if not include_all_ctgs and not restricted and name not in MAJOR_CONTIGS_ORDER:
            continue
        if in_bed is not None and name not in in_bed:
            continue
        if (listed or in_vcf is not None) and name not in contig_set:
            continue
        contig_set.add(name)
        n = length // chunk_size + 1 if length % chunk_size else length // chunk_size
        chunks[name] = chunk_num if chunk_num else max(n, 1)
    order = MAJOR_CONTIGS_ORDER + sorted(contig_set - set(MAJOR_CONTIGS_ORDER))
    contigs = sorted((c for c in contig_set if c in chunks), key=order.index)
    return contigs, chunks


def split_extend_bed(bed_fn, out_dir, contig_set):
    """run_clair3_rna:268-296: per-contig BED files with every interval widened by 33 bp on both sides."""
    per = {}
    with io._open_text(bed_fn) as f:
        for i, row in enumerate(f):
            if not row.strip() or row[0] == "#":
                continue
            c = row.strip().split()
            if contig_set and c[0] not in contig_set:
                continue
            s, e = int(c[1]), int(c[2])
            if e < s or s < 0 or e < 0:
                sys.exit("[ERROR] Invalid BED input at the %d-th row %s %d %d" % (i + 1, c[0], s, e))
            per.setdefault(c[0], []).append("%s %d %d" % (c[0], max(0, s - EXPAND), max(0, e + EXPAND)))
    os.makedirs(out_dir, exist_ok=True)
    for name, rows in per.items():
        with open(os.path.join(out_dir, name), "w") as f:
            f.write("\n".join(rows))


def build_parser():
    p = argparse.ArgumentParser(description="Clair3-RNA pileup calling of a whole sample on MI355X (in-process STEP 1 + STEP 2 of run_clair3_rna)")
    a = p.add_argument
    a("-b", "--bam_fn", type=str, required=True)
    a("-f", "--ref_fn", type=str, required=True)
    a("-o", "--output_dir", type=str, required=True)
    a("-p", "--platform", type=str, default="ont")
    a("--pileup_model_path", type=str, required=True, help="checkpoint prefix (…/variables), as passed to call_var_bam --chkpnt_fn")
    a("--phased_pileup_model_path", type=str, default=None)
    a("--enable_phasing_model", action="store_true", help="30-channel pass on an already haplotagged BAM, or on an untagged one with --phased_vcf_fn")
    a("--phased_vcf_fn", type=str, default=None,
      help="with --enable_phasing_model: one phased VCF for all contigs (plain or gzipped), or a directory that holds phased_<ctg>.vcf.gz "
           "(what `whatshap phase` / `longphase phase` write per contig); the reads are haplotagged on the GPU from its phased heterozygous "
           "SNVs and HP tags of the BAM are ignored.  A contig without phased sites runs with all reads untagged")
    a("--phasing", type=str, default=None, choices=["builtin"],
      help="with --enable_phasing_model and without --phased_vcf_fn: run the whole flow in this process — the unphased pass (<prefix>.vcf.gz), "
           "the built-in phasing of its heterozygous SNVs from read linkage on the GPU (phase_vcf: a greedy linkage chain, not whatshap's wMEC) "
           "into <output_dir>/tmp/phased_output/phased_vcf, then the 30-channel pass on those files.  Needs both model paths; one process only "
           "(not under torch.distributed.run)")
    a("--phase_merge_levels", type=int, default=0,
      help="with --phasing builtin: handed to phase_vcf as --merge_levels — up to that many levels of the block-merge stage after the chain, "
           "which joins the blocks that reads bridge across a run of unlinked sites (0: off)")
    a("--phase_output", action="store_true",
      help="with --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin: after the 30-channel pass, phase the heterozygous SNVs of "
           "<prefix>_enable_phasing.vcf.gz from per-haplotype allele counts on the GPU (hap_vcf: SNVs only, a majority rule over CIGAR-position "
           "alleles) into <prefix>_enable_phasing_phased.vcf.gz and write the counts to <prefix>_enable_phasing_hap_counts.tsv.  One process only "
           "(not under torch.distributed.run)")
    a("--phasing_indels", action="store_true",
      help="with --phasing builtin: the phasing between the passes links heterozygous insertions, deletions and 1/2 rows too (phase_vcf "
           "--indels: alleles read off the CIGAR position, no realignment, a greedy chain), and the second pass — and --phase_output / "
           "--haplotagged_bam behind it — haplotags the reads from all of them.  Off by default, as `whatshap phase --indels` is")
    a("--haplotag_indels", action="store_true",
      help="with --phased_vcf_fn: haplotag the reads from the phased insertions, deletions and two-ALT rows (`1|2`) of the phased VCF too, not "
           "from its biallelic SNVs alone (include/c3r.h: c3r_set_phase_alleles) — the rows that --phase_output --phase_indels and `whatshap "
           "phase --indels` write.  Not with --phasing builtin (the phasing between the passes is SNV-only): run with --phase_output "
           "--phase_indels first, then rerun with --phased_vcf_fn <prefix>_enable_phasing_phased.vcf.gz --haplotag_indels")
    a("--left_align_indels", action="store_true",
      help="with --phase_indels, --haplotag_indels or --phasing_indels: left-align the indels those steps read — the tables' against --ref_fn, "
           "every read's inside its own M run, on the device (include/c3r.h: c3r_set_hap_left_align) — so that a read whose aligner placed an "
           "indel elsewhere in a homopolymer or short tandem repeat shows the allele and not the reference; the flag is handed to every such "
           "step.  A shift stops at the M run's start, at an N or another indel; no realignment, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes)")
    from . import phasing as _phasing
    _phasing.add_hap_realign_flag(a)
    _phasing.add_hap_bq_weights_flag(a, "with --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin: handed to the 30-channel pass, to hap_vcf (--phase_output) "
                                        "and to haplotag_bam (--haplotagged_bam, which then writes PC); not to the unphased pass, which haplotags nothing, and not to "
                                        "phase_vcf, whose links stay unweighted.  ")
    a("--hap_min_bq", type=int, default=0, metavar="N",
      help="with --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin: a base whose quality is below N does not vote — every step that "
           "holds reads against a site table (phase_vcf between the passes, the 30-channel pass's haplotagging, hap_vcf, haplotag_bam) gets the flag, "
           "fetches the qualities and reads such a base as N (include/c3r.h: c3r_set_hap_min_bq; 0 .. 93, default 0: off).  The tensor build and "
           "the unphased pass never look at it.  A threshold, not whatshap's quality weights (--hap_bq_weights are those); an indel's own quality is not modelled; reads "
           "without qualities are never masked; agreement with whatshap is not measured")
    a("--phase_indels", action="store_true",
      help="with --phase_output: handed to hap_vcf as --indels — heterozygous insertions, deletions and rows with two ALT alleles (GT 1/2) are "
           "phased too, by CIGAR-position alleles (no realignment, no left-alignment of the reads' indels unless --left_align_indels is given, no base qualities "
           "(`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes)), and the counts "
           "file gets the column ALLELES")
    a("-c", "--ctg_name", type=str, default=None)
    a("--bed_fn", type=str, default=None)
    a("--genotyping_mode_vcf_fn", type=str, default=None)
    a("-q", "--qual", type=int, default=None)
    a("--snp_min_af", type=float, default=0.08)
    a("--indel_min_af", type=float, default=0.15)
    a("--min_coverage", type=int, default=4)
    a("--min_mq", type=int, default=5)
    a("--chunk_size", type=int, default=CHUNK_SIZE)
    a("--chunk_num", type=int, default=None)
    a("-s", "--sample_name", type=str, default="SAMPLE")
    a("--output_prefix", type=str, default="output")
    a("--include_all_ctgs", action="store_true")
    a("--print_ref_calls", action="store_true")
    a("--enable_variant_calling_at_sequence_head_and_tail", action="store_true")
    a("--enable_padding_in_splice_junction_regions", action="store_true")
    a("--tag_variant_using_readiportal", action="store_true")
    a("--readiportal_source_fn", type=str, default=None)
    a("--readiportal_database_filter_tag", type=str, default=None)
    a("--no_compress", action="store_true", help="leave <prefix>.vcf uncompressed (tests)")
    a("--samtools", type=str, default="samtools", help="as in run_clair3_rna; never piped, only asked for its version (--mpileup_compat auto)")
    a("--mpileup_compat", type=str, default=mpileup_compat.env_default(), choices=list(mpileup_compat.CHOICES),
      help="which samtools mpileup text the tensor build restates: auto = ask `--samtools --version` (>= 1.11 -> 1, <= 1.10 -> 0, not "
           "runnable -> 1); 0 = samtools <= 1.10; 1 = samtools >= 1.11.  Default: $C3R_MPILEUP_COMPAT, else auto")
    a("--haplotagged_bam", action="store_true",
      help="with --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin: after the passes, write the haplotagged BAM of every "
           "processed contig with the tags the GPU computed to <output_dir>/tmp/phased_output/phased_bam/<ctg>.bam + .bai (haplotag_bam: the "
           "files the reference's `whatshap haplotag` + `samtools index` step leaves).  One process only.  Off: no file more and no byte different")
    a("--hap_expression_bed", type=str, default=None, metavar="BED",
      help="with --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin (combinable with --phase_output and --haplotagged_bam): after "
           "the passes, count the reads of each haplotype and phase set over every interval of BED (exons, genes) on the GPU, with the tags the "
           "30-channel pass called with, into <prefix>_enable_phasing_hap_expression.tsv (hap_expr: allele-specific expression; a read counts in "
           "every region it overlaps, no gene-level union, no statistics).  One process only.  Off: no file more and no byte different")
    from . import hap_expr as _hap_expr
    _hap_expr.add_stranded_flag(a, "--hap_expression_stranded")
    a("--hap_expression_group_by_name", action="store_true",
      help="with --hap_expression_bed: the gene-level count — the BED lines with the same name (column 4) are one group and a read counts once per "
           "group, however many of its intervals it overlaps (hap_expr --group_by_name) — into <prefix>_enable_phasing_hap_expression_by_name.tsv "
           "in place of <prefix>_enable_phasing_hap_expression.tsv.  No GTF reader, no fractional assignment, no statistics")
    a("--hap_junctions", action="store_true",
      help="with --enable_phasing_model and one of --phased_vcf_fn / --phasing builtin (combinable with --phase_output, --haplotagged_bam and "
           "--hap_expression_bed): after the passes, count on the GPU the reads of each haplotype and phase set per splice junction (every N op of a "
           "counted read), with the tags the 30-channel pass called with, into <prefix>_enable_phasing_hap_junctions.tsv (hap_junctions: "
           "allele-specific splicing; no minimum intron or anchor length, no annotation, no statistics; agreement with an external junction "
           "counter is not measured).  One process only.  Off: no file more and no byte different")
    a("--gpu_id", type=int, default=None, help="default: $C3R_DEVICE, else LOCAL_RANK under torch.distributed.run, else 0")
    a("--gpu_precision", type=str, default=_env_precision(), choices=["f32", "f16x3", "f16+f8", "auto"],
      help="network arithmetic (c3r_set_precision): f16x3 = fp32-equivalent split-f16 (default); auto = the faster fp8-corrected path where a "
           "calibration run through the loaded weights agrees with f16x3 to 4e-5, else f16x3")
    a("--fetch_threads", type=int, default=8, help="threads that fetch alignments (long contigs as several position ranges, BGZF inflate on C3R_FETCH_INFLATE threads each) and reference slices ahead of the contexts; capped by the rank's share of the cores under torch.distributed")
    a("--contexts", type=int, default=2, help="GPU contexts (each with its own host thread and HIP stream) working side by side: while one waits for its kernels the other normalises reads or decodes (every context sizes its own device buffers on its first contig; first uses take turns)")
    return p


def _all_ranks_ok(dist, world, err, what):
    """Rendezvous of all ranks that also carries a failure flag: a rank that failed still arrives, and then every rank raises.
    (A rank that simply returned would leave the others in dist.barrier() until the gloo timeout.)"""
    if world > 1:
        import torch
        flag = torch.tensor([1 if err is not None else 0], dtype=torch.int32)
        dist.all_reduce(flag)
        if err is None and int(flag.item()):
            raise RuntimeError("another rank failed while %s" % what)
    if err is not None:
        raise err


class _Fetcher(object):
    """Stage 1: a contig's alignments + reference slice, one BAM handle per worker thread.  A long contig is fetched as several
    position ranges on several threads (`plan` / `part` / `join`): the first contig of a sample is then ready after a fraction of
    the 0.4 s a cold handle needs for a whole chromosome, and the contexts start that much earlier."""

    PART_BP = 24_000_000                 # shortest range worth a fetch of its own

    def __init__(self, bam_fn, ref_fn, want_quals=False):
        self.bam_fn, self.ref_fn, self.tls = bam_fn, ref_fn, threading.local()
        self.want_quals = bool(want_quals)   # --hap_min_bq: the parts carry the base qualities, two bytes per sequence byte
        self.handles, self.fai = [], None
        self.lock = threading.Lock()

    def _handle(self):
        from . import bamio
        bf = getattr(self.tls, "bf", None)
        if bf is None:
            bf = self.tls.bf = bamio.BamFile(self.bam_fn, threads=int(os.environ.get("C3R_FETCH_INFLATE", "8")))
            with self.lock:
                self.handles.append(bf)
        return bf

    def plan(self, length, max_parts):
        """-> [(beg0, end0), ...] position ranges of one contig, in order (one range: the whole contig)."""
        if self.bam_fn.endswith(".npz") or max_parts <= 1:
            return [(0, None)]
        n = max(1, min(max_parts, length // int(os.environ.get("C3R_FETCH_PART_BP", self.PART_BP))))      # (the variable: tests split small contigs)
        if n > 1 and not self._handle().has_index:
            n = 1
        edges = [length * k // n for k in range(n + 1)]
        return [(edges[k], edges[k + 1] if k + 1 < n else None) for k in range(n)]

    def part(self, ctg, beg0, end0):
        """The alignments that START in [beg0, end0) (a fetch returns everything that overlaps the range: what started before it
        belongs to the range before) -> ReadSet views, offsets relative to this part."""
        if self.bam_fn.endswith(".npz"):
            return io.load_reads(self.bam_fn, ctg, **(dict(want_quals=True) if self.want_quals else {}))
        rs = self._handle().fetch(ctg, beg0, end0, **(dict(want_quals=True) if self.want_quals else {}))
        if beg0 > 0 and len(rs.reads):
            i0 = int(np.searchsorted(rs.reads["pos"], beg0, side="left"))
            if i0:
                if i0 >= len(rs.reads):
                    return _empty_reads()
                c0, s0 = int(rs.reads["cigar_off"][i0]), int(rs.reads["seq_off"][i0])
                out = ReadSet.__new__(ReadSet)
                out.reads, out.cigar, out.seq = rs.reads[i0:], rs.cigar[c0:], rs.seq[s0:]
                if rs.qual is not None:
                    out.qual = rs.qual[2 * s0:]
                out.base = (c0, s0)
                return out
        return rs

    def reference(self, ctg, length):
        from . import bamio
        with self.lock:
            if self.fai is None:
                self.fai = {r[0]: r for r in io.read_fai(self.ref_fn)}
        # the whole contig, upper-cased, line ends dropped, by parallel pread (c3r_fasta_fetch) — a 250-Mb chromosome went
        # through Python's bytes.replace in 0.4 s with the GIL held, which stalled every other thread of the process
        return bamio.fasta_fetch(self.ref_fn, self.fai[ctg], 0, length)

    @staticmethod
    def join(parts):
        """Parts in position order -> one ReadSet (arrays from c3r_io_alloc, offsets moved)."""
        parts = [p_ for p_ in parts if len(p_.reads)]
        if not parts:
            return _empty_reads()
        if len(parts) == 1 and getattr(parts[0], "base", (0, 0)) == (0, 0):
            return parts[0]
        from . import bamio
        out = ReadSet.__new__(ReadSet)
        out.reads = bamio.huge_empty(sum(len(p_.reads) for p_ in parts), READ_DTYPE)
        out.cigar = bamio.huge_empty(sum(len(p_.cigar) for p_ in parts), np.uint32)
        out.seq = bamio.huge_empty(sum(len(p_.seq) for p_ in parts), np.uint8)
        if parts[0].qual is not None:
            out.qual = bamio.huge_empty(2 * len(out.seq), np.uint8)
        r0 = c0 = s0 = 0
        for p_ in parts:
            nr, nc, ns = len(p_.reads), len(p_.cigar), len(p_.seq)
            bc, bs = getattr(p_, "base", (0, 0))
            out.reads[r0:r0 + nr] = p_.reads
            out.reads["cigar_off"][r0:r0 + nr] += np.uint32((c0 - bc) & 0xffffffff)      # (modular: the sum is the new offset)
            out.reads["seq_off"][r0:r0 + nr] += np.uint64((s0 - bs) & 0xffffffffffffffff)
            out.cigar[c0:c0 + nc] = p_.cigar
            out.seq[s0:s0 + ns] = p_.seq
            if out.qual is not None:
                out.qual[2 * s0:2 * (s0 + ns)] = p_.qual
            r0 += nr; c0 += nc; s0 += ns
        return out

    def __call__(self, ctg, length):
        """The whole contig on the calling thread -> (ReadSet, reference array or b"", seconds)."""
        t0 = time()
        rs = self.join([self.part(ctg, 0, None)])
        ref = self.reference(ctg, length) if len(rs.reads) else b""
        return rs, ref, time() - t0

    def close(self):
        for bf in self.handles:
            bf.close()


def _empty_reads():
    out = ReadSet.__new__(ReadSet)
    out.reads, out.cigar, out.seq = np.zeros(0, READ_DTYPE), np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    return out


def _index_link(bam_fn, out_dir):
    """None when `bam_fn` needs no index of ours (not a BAM, or one with an index of its own), else the path of the link in tmp/ that gets
    one beside it (asked of the BAM itself, not guessed from a link that an earlier run in this directory may have left to another file)."""
    if not bam_fn.endswith(".bam"):
        return None
    from . import bamio
    with bamio.BamFile(bam_fn) as probe:
        if probe.has_index:
            return None
    return os.path.join(out_dir, "tmp", "input.bam")


def _indexed_bam(args):
    """The BAM the steps around the passes read: this run's, or — when IT has no index — the link with an index beside it that a pass left in tmp/."""
    link = _index_link(args.bam_fn, args.output_dir)
    if link and os.path.exists(link + ".bai") and os.path.realpath(link) == os.path.realpath(args.bam_fn):
        return link
    return args.bam_fn


_Step = collections.namedtuple("_Step", "name handed needs")


def _plan(args):
    """Every rule about the phasing flags, in one place, before anything is created: exits with the [ERROR] line of the first rule that is
    broken, else -> the steps of the run, in order, as _Step(name, handed, needs):
        pass                                  handed: the args of that pass (_run_pass)
        clear                                 handed: (directory, which names are an earlier run's files): they are removed, the directory is made
        phase_vcf | hap_vcf | haplotag_bam    handed: that module's argv; --bam_fn is added when the step runs (_indexed_bam)
    `needs` is the file without which Run skips the step (None: never skipped).
    One pass; with `--phasing builtin` the unphased pass, phase_vcf on the file it wrote, and the 30-channel pass with --phased_vcf_fn on
    phase_vcf's directory (--phasing_indels: phase_vcf --indels, and that pass reads the directory as under --haplotag_indels); with
    `--phase_output` / `--haplotagged_bam` one further step each behind them.  Nothing inside a pass changes."""
    import copy
    builtin, phased = args.phasing is not None, args.enable_phasing_model

    def one_process(what, instead):
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("[ERROR] %s runs in one process: under torch.distributed.run (WORLD_SIZE > 1) %s" % (what, instead))
    if args.phase_indels and not args.phase_output:
        sys.exit("[ERROR] --phase_indels belongs to --phase_output (it phases the indels of the final VCF): it needs --phase_output")
    if args.haplotag_indels and builtin:
        sys.exit("[ERROR] --haplotag_indels changes nothing under --phasing builtin: the phasing between the passes is SNV-only, so the table the "
                 "reads are haplotagged from holds no indel.  The two-step way: 1. run with --phase_output --phase_indels; 2. rerun with "
                 "--phased_vcf_fn <prefix>_enable_phasing_phased.vcf.gz --haplotag_indels.  In one command, without --haplotag_indels: "
                 "--phasing builtin --phasing_indels phases the indels between the passes and tags the reads from them")
    if args.haplotag_indels and not args.phased_vcf_fn:
        sys.exit("[ERROR] --haplotag_indels needs --phased_vcf_fn (it widens the table the reads are haplotagged from)")
    if args.phasing_indels and not builtin:
        sys.exit("[ERROR] --phasing_indels belongs to the built-in phasing (it phases indels and 1/2 rows between the passes): it needs --phasing builtin")
    for flag, on, why, instead in (
            ("--phase_output", args.phase_output, "it phases the 30-channel pass's VCF",
             "run the pass without it and then `python -m clair3_rna_amd.hap_vcf --bam_fn ... --vcf_fn <prefix>_enable_phasing.vcf.gz "
             "--phased_vcf_fn ... --output_fn ...`"),
            ("--haplotagged_bam", args.haplotagged_bam, "it writes the tags the 30-channel pass called with",
             "run the pass without it and then `python -m clair3_rna_amd.haplotag_bam --bam_fn ... --phased_vcf_fn ... --output_dir "
             "<output_dir>/tmp/phased_output/phased_bam`"),
            ("--hap_expression_bed", bool(getattr(args, "hap_expression_bed", None)), "it counts reads by the tags the 30-channel pass called with",
             "run the pass without it and then `python -m clair3_rna_amd.hap_expr --bam_fn ... --phased_vcf_fn ... --regions_bed_fn ... "
             "--output_fn ...`"),
            ("--hap_junctions", bool(getattr(args, "hap_junctions", False)), "it counts junction reads by the tags the 30-channel pass called with",
             "run the pass without it and then `python -m clair3_rna_amd.hap_junctions --bam_fn ... --phased_vcf_fn ... --ref_fn ... --output_fn ...`")):
        if on:
            if not phased:
                sys.exit("[ERROR] %s needs --enable_phasing_model (%s)" % (flag, why))
            if not builtin and not args.phased_vcf_fn:
                sys.exit("[ERROR] %s needs a phased VCF to haplotag the reads from: --phased_vcf_fn or --phasing builtin" % flag)
            one_process(flag, instead)
    if getattr(args, "hap_expression_bed", None) and not os.path.isfile(args.hap_expression_bed):
        sys.exit("[ERROR] file %s not found" % args.hap_expression_bed)
    if getattr(args, "hap_expression_group_by_name", False) and not getattr(args, "hap_expression_bed", None):
        sys.exit("[ERROR] --hap_expression_group_by_name belongs to --hap_expression_bed (it groups the lines of that BED by their name): it needs --hap_expression_bed")
    if getattr(args, "hap_expression_stranded", "no") != "no" and not getattr(args, "hap_expression_bed", None):
        sys.exit("[ERROR] --hap_expression_stranded belongs to --hap_expression_bed (it chooses the strand of the reads counted there): it needs --hap_expression_bed")
    left_align =bool(getattr(args, "left_align_indels", False))
    if left_align and not (args.phase_indels or args.haplotag_indels or args.phasing_indels):
        sys.exit("[ERROR] --left_align_indels needs one of --phase_indels, --haplotag_indels, --phasing_indels (it left-aligns the indels those steps read)")
    la = ["--left_align_indels", "--ref_fn", args.ref_fn] if left_align else []
    from . import phasing
    min_bq = phasing.hap_min_bq_arg(args, bool(phased and (builtin or args.phased_vcf_fn)),
                                    "--enable_phasing_model and one of --phased_vcf_fn / --phasing builtin: without a phase table no step holds the reads against one")
    bq = ["--hap_min_bq", str(min_bq)] if min_bq else []
    # (--hap_bq_weights goes to the steps that haplotag reads: the 30-channel pass, hap_vcf and haplotag_bam; phase_vcf's links stay unweighted)
    weights = phasing.hap_bq_weights_arg(args, bool(phased and (builtin or args.phased_vcf_fn)), "--enable_phasing_model and one of --phased_vcf_fn / --phasing builtin: without a phase table no step haplotags the reads")
    bw = ["--hap_bq_weights"] if weights else []
    # (--hap_realign goes to every step that holds reads against a table: phase_vcf, the 30-channel pass, hap_vcf and haplotag_bam)
    realign, _ = phasing.hap_realign_arg(args, bool(phased and (builtin or args.phased_vcf_fn)),
                                         "--enable_phasing_model and one of --phased_vcf_fn / --phasing builtin: without a phase table no step holds the reads against one")
    ra = ["--hap_realign", str(realign), "--ref_fn", args.ref_fn] + (["--hap_realign_spliced"] if phasing.hap_realign_spliced_arg(args) else []) if realign else []
    ext = ".vcf" if args.no_compress else ".vcf.gz"
    phased_dir = os.path.join(args.output_dir, "tmp", "phased_output", "phased_vcf")
    ctg = ["--ctg_name", args.ctg_name] if args.ctg_name else []
    gpu = ["--gpu_id", str(args.gpu_id)] if args.gpu_id is not None else []
    if not builtin:
        if args.phase_merge_levels:
            sys.exit("[ERROR] --phase_merge_levels belongs to the built-in phasing: it needs --phasing builtin")
        if args.phased_vcf_fn and not phased:
            sys.exit("[ERROR] --phased_vcf_fn needs --enable_phasing_model (haplotags only enter the 30-channel tensors)")
        if args.phased_vcf_fn and not os.path.exists(args.phased_vcf_fn):
            sys.exit("[ERROR] file %s not found" % args.phased_vcf_fn)
        if phased and args.phased_pileup_model_path is None:
            sys.exit("[ERROR] --phased_pileup_model_path is required with --enable_phasing_model")
        steps = [_Step("pass", args, None)]
    else:
        if not phased:
            sys.exit("[ERROR] --phasing builtin needs --enable_phasing_model (it prepares the 30-channel pass)")
        if args.phase_merge_levels < 0:
            sys.exit("[ERROR] --phase_merge_levels must be >= 0")
        if args.phased_vcf_fn:
            sys.exit("[ERROR] --phasing builtin and --phased_vcf_fn exclude each other: the built-in phasing writes the phased VCFs itself")
        if not args.phased_pileup_model_path:
            sys.exit("[ERROR] --phased_pileup_model_path is required with --enable_phasing_model")
        one_process("--phasing builtin", "run the unphased pass, `python -m clair3_rna_amd.phase_vcf`, and the pass with --phased_vcf_fn as three commands")
        first, second = copy.copy(args), copy.copy(args)
        first.phasing, first.enable_phasing_model = None, False
        first.hap_min_bq = 0                                  # (the unphased pass holds its reads against no site table: phase_vcf loads them itself)
        first.hap_realign = 0
        first.hap_realign_spliced = False
        first.hap_bq_weights = False
        second.phasing, second.phased_vcf_fn = None, phased_dir
        if args.phasing_indels:
            second.haplotag_indels = True                     # (the table of c3r_set_phase_alleles, as --phased_vcf_fn DIR --haplotag_indels)
        unphased = os.path.join(args.output_dir, args.output_prefix + ext)
        # phased_<ctg>.vcf.gz of an earlier run in this directory: a contig without a row in this run's VCF would keep its file, and the
        # second pass would haplotag from it
        steps = [_Step("pass", first, None),
                 _Step("clear", (phased_dir, lambda name: name.startswith("phased_") and name.endswith(".vcf.gz")), None),
                 _Step("phase_vcf", ["--vcf_fn", unphased, "--output_dir", phased_dir, "--min_mq", str(args.min_mq), "--merge_levels", str(args.phase_merge_levels)]
                       + (["--indels"] + la if args.phasing_indels else []) + bq + ra + ctg + gpu, unphased),
                 _Step("pass", second, None)]
    stem = os.path.join(args.output_dir, args.output_prefix + "_enable_phasing")
    source = phased_dir if builtin else args.phased_vcf_fn
    # (--phasing_indels: the steps behind the passes read phase_vcf --indels' directory with the allele table)
    tag_indels = ["--haplotag_indels"] if args.haplotag_indels or args.phasing_indels else []
    # (--left_align_indels goes to every step that reads indels: its candidates, its tags, or both)
    if args.phase_output:
        steps.append(_Step("hap_vcf", ["--vcf_fn", stem + ext, "--phased_vcf_fn", source, "--output_fn", stem + "_phased" + ext, "--hap_counts_fn",
                                       stem + "_hap_counts.tsv", "--min_mq", str(args.min_mq)] + (["--indels"] if args.phase_indels else []) + tag_indels
                           + (la if args.phase_indels or tag_indels else []) + bq + bw + ra + ctg + gpu,
                           stem + ext))
    if args.haplotagged_bam:
        # the reference's names (run_clair3_rna:787,799), for the contigs the passes processed (--ctg_name: added when the step runs); an
        # earlier run's files in this directory, for contigs this run did not process, go first
        bam_dir = os.path.join(args.output_dir, "tmp", "phased_output", "phased_bam")
        steps += [_Step("clear", (bam_dir, lambda name: name.endswith(".bam") or name.endswith(".bam.bai")), stem + ext),
                  _Step("haplotag_bam", ["--phased_vcf_fn", source, "--output_dir", bam_dir] + tag_indels + (la if tag_indels else []) + bq + bw + ra + gpu, stem + ext)]
    if getattr(args, "hap_expression_bed", None):
        # the tagging flags haplotag_bam gets: the counts are by the tags of the pass; the contigs the passes processed are added when the step runs
        by_name = bool(getattr(args, "hap_expression_group_by_name", False))
        steps.append(_Step("hap_expr", ["--phased_vcf_fn", source, "--regions_bed_fn", args.hap_expression_bed,
                                        "--output_fn", stem + ("_hap_expression_by_name.tsv" if by_name else "_hap_expression.tsv"),
                                        "--min_mq", str(args.min_mq), "--stranded", args.hap_expression_stranded] + (["--group_by_name"] if by_name else [])
                           + tag_indels + (la if tag_indels else []) + bq + bw + ra + gpu, stem + ext))
    if getattr(args, "hap_junctions", False):
        # the tagging flags hap_expr gets, and the reference for MOTIF / STRAND (argparse keeps the one --ref_fn, whoever names it again)
        steps.append(_Step("hap_junctions", ["--phased_vcf_fn", source, "--output_fn", stem + "_hap_junctions.tsv", "--min_mq", str(args.min_mq), "--ref_fn", args.ref_fn]
                           + tag_indels + (la if tag_indels else []) + bq + bw + ra + gpu, stem + ext))
    return steps


def Run(args, log=None):
    """The steps of _plan, one after the other.  A step whose file is missing is skipped: no contig was found, and the pass wrote nothing."""
    for step in _plan(args):
        if step.needs is not None and not os.path.isfile(step.needs):
            continue
        if step.name == "pass":
            rc = _run_pass(step.handed, log)
            if rc:
                return rc
        elif step.name == "clear":
            io.remove_stale(*step.handed)
            os.makedirs(step.handed[0], exist_ok=True)
        else:
            argv = ["--bam_fn", _indexed_bam(args)] + step.handed
            if step.name in ("haplotag_bam", "hap_expr", "hap_junctions"):
                contigs, _ = plan_chunks(args.ref_fn, args.ctg_name, args.include_all_ctgs, existing(args.bed_fn), existing(args.genotyping_mode_vcf_fn),
                                         args.chunk_size, args.chunk_num)
                argv += ["--ctg_name", ",".join(contigs)]
            module = importlib.import_module("." + step.name, __package__)
            module.Run(module.build_parser().parse_args(argv), log)
    return 0


# ---- one pass.  Stage 1: set-up
class _Pass(object):
    """What set-up (_set_up) leaves for the other stages of a pass, as plain attributes; nothing is added to it afterwards:
        the run        args, log, t_all, timeline, compat (which samtools' column text), channels, qual_rows, qual_merge, weights,
                       hap_min_bq (--hap_min_bq of a pass with a phase table, else 0), hap_bq_weights (--hap_bq_weights, likewise)
        the ranks      rank, world, dist (torch.distributed or None), n_thr (the threads this process may count on)
        the paths      out_dir, out_fn, out_nt_fn, parts_dir, split_dir, cmd_fn, bed_fn, vcf_fn (genotyping mode), bam_fn (the one fetched from)
        the plan       all_contigs and chunk_nums (plan_chunks), contigs (this rank's, in calling order), fai ({contig: length})
        the objects    table (REDIportal, or None), edits (its per-contig lists), merger (rank 0's SampleMerger, else None), fetcher,
                       phase_source (phasedvcf.PhaseSource of --phased_vcf_fn, or None)"""

    def mark(self, ctg, what, t0):
        """A C3R_TIMING timeline line (tools/timeline_view.py reads them)."""
        if self.timeline:
            self.log("[timeline] %-6s %-8s %7.3f -> %7.3f s" % (ctg, what, t0 - self.t_all, time() - self.t_all))


def _host_budget(args, world):
    """-> the threads this process may count on.  One process per GPU shares the node's cores with its peers: this rank's slice of them (its
    GPU's NUMA node when the topology says which), and thread counts cut to match — decode (C3R_THREADS), fetch, compression.  The same for
    one process on the host slice a rank of an N-GPU run would get (C3R_HOST_SLICE, tools/host_slice.py)."""
    if world == 1 and not os.environ.get("C3R_HOST_SLICE"):
        return os.cpu_count() or 8
    from . import shard
    n_thr, _cpus = shard.host_budget(apply=True)
    args.fetch_threads = max(1, min(args.fetch_threads, n_thr // 2 or 1))
    os.environ.setdefault("C3R_FETCH_INFLATE", str(max(1, n_thr // args.fetch_threads)))    # inflate threads per fetch handle
    return n_thr


def _set_up(args, log, t_all):
    """Ranks and host budget, paths, the plan of contigs and chunks, the split BED, CMD, the BAM index, this rank's contigs, the REDIportal
    table, the weights, the merger and the fetcher -> _Pass, or None when no contig was found."""
    p = _Pass()
    p.args, p.log, p.t_all, p.timeline = args, log, t_all, os.environ.get("C3R_TIMING") is not None
    # which samtools the column text follows: asked in a child process before anything touches the GPU (rank 0's line is the one printed)
    p.compat = mpileup_compat.resolve(args.mpileup_compat, args.samtools, log if int(os.environ.get("RANK", "0")) == 0 else (lambda m: None))
    # one process per GPU (`python -m torch.distributed.run --nproc-per-node N -m clair3_rna_amd.call_sample ...`): contigs are
    # dealt to the ranks largest-first, every rank leaves the merged records of its contigs under tmp/parts/, rank 0 puts the
    # file together.  No data-path collective: torch.distributed (gloo) is the barrier, nothing else.
    p.rank, p.world, p.dist = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), None
    if p.world > 1:
        import torch.distributed as dist
        p.dist = dist
        if not dist.is_initialized():
            dist.init_process_group("gloo")
        if args.gpu_id is None:
            args.gpu_id = int(os.environ.get("LOCAL_RANK", str(p.rank)))
    p.n_thr = _host_budget(args, p.world)
    if args.gpu_id is None:
        args.gpu_id = int(os.environ.get("C3R_DEVICE", "0"))
    for need in (args.bam_fn, args.ref_fn):
        if not os.path.isfile(need):
            sys.exit("[ERROR] file %s not found" % need)
    p.bed_fn, p.vcf_fn = existing(args.bed_fn), existing(args.genotyping_mode_vcf_fn)
    p.channels = 30 if args.enable_phasing_model else 18
    p.out_dir = out_dir = args.output_dir
    os.makedirs(os.path.join(out_dir, "tmp"), exist_ok=True)
    suffix = "_enable_phasing" if args.enable_phasing_model else ""
    p.out_fn = os.path.join(out_dir, args.output_prefix + suffix + ".vcf")
    p.out_nt_fn = os.path.join(out_dir, args.output_prefix + "_no_tagging" + suffix + ".vcf")
    p.parts_dir = os.path.join(out_dir, "tmp", "parts")

    p.all_contigs, p.chunk_nums = plan_chunks(args.ref_fn, args.ctg_name, args.include_all_ctgs, p.bed_fn, p.vcf_fn, args.chunk_size, args.chunk_num)
    if not p.all_contigs:
        log("[WARNING] Exit calling because no contig was found in BAM!")
        return None
    p.fai = {n: L for n, L, _o, _b, _w in io.read_fai(args.ref_fn)}
    priv = os.path.join(out_dir, "tmp") if p.rank == 0 else os.path.join(out_dir, "tmp", "rank%d" % p.rank)
    os.makedirs(priv, exist_ok=True)
    p.split_dir = os.path.join(priv, "split_beds")
    if p.bed_fn:
        split_extend_bed(p.bed_fn, p.split_dir, set(p.all_contigs))
    p.cmd_fn = os.path.join(out_dir, "tmp", "CMD")                      # run_clair3_rna:613-667: stamped into the VCF header
    if p.rank == 0 and not os.path.exists(p.cmd_fn):
        with open(p.cmd_fn, "w") as f:
            f.write(" ".join(sys.argv) + "\n")
    p.bam_fn = _ensure_index(p)
    p.contigs = _deal_contigs(p)
    p.table = _rediportal_table(args, p.contigs, log)
    model = args.phased_pileup_model_path if args.enable_phasing_model else args.pileup_model_path
    p.weights = io.load_weights(model, p.channels)
    p.qual_rows = args.qual if args.qual is not None else 2            # call_variants.py:1827 (STEP 1 never passes --qual)
    p.qual_merge = args.qual if args.qual is not None else 2           # sort_vcf's own default
    header = vcf.header(args.ref_fn, p.cmd_fn, args.sample_name) + "\n"
    # (compressed output is written as it is produced — bgzip blocks and the tabix index grow contig by contig — so that no
    # compression pass is left after the last contig)
    p.edits = sort_vcf.ContigEdits(p.table)                            # (one for all the per-contig mergers of this rank)
    p.merger = sort_vcf.SampleMerger(p.out_fn, header, p.qual_merge, args.print_ref_calls, p.table, p.out_nt_fn, stream_gz=not args.no_compress,
                                     edits=p.edits) if p.rank == 0 else None
    p.hap_min_bq = int(getattr(args, "hap_min_bq", 0) or 0) if args.phased_vcf_fn else 0       # (only a pass with a phase table tags reads)
    p.hap_realign = int(getattr(args, "hap_realign", 0) or 0) if args.phased_vcf_fn else 0     # (--hap_realign, likewise)
    p.hap_realign_spliced = bool(getattr(args, "hap_realign_spliced", False)) and bool(p.hap_realign)      # (--hap_realign_spliced goes where it goes)
    p.hap_bq_weights = bool(getattr(args, "hap_bq_weights", False)) and bool(args.phased_vcf_fn)   # (--hap_bq_weights, likewise)
    p.fetcher = _Fetcher(p.bam_fn, args.ref_fn, want_quals=bool(p.hap_min_bq or p.hap_bq_weights))
    p.phase_source = None                                              # --phased_vcf_fn: every contig's table is read on a fetch thread
    if args.phased_vcf_fn:
        from . import phasedvcf
        ref_of = None
        if getattr(args, "left_align_indels", False) and args.haplotag_indels:         # (asked from the fetch threads: nothing shared)
            ref_of = lambda c: (1, io.fetch_reference(args.ref_fn, c, 1, 2 ** 31, raw=True))
        p.phase_source = phasedvcf.PhaseSource(args.phased_vcf_fn, args.haplotag_indels, *(() if ref_of is None else (None, ref_of)),
                                               **(dict(realign=p.hap_realign) if p.hap_realign else {}))
    return p


def _ensure_index(p):
    """-> the BAM the pass fetches from: the run's own, or the link in tmp/ with the index built here beside it."""
    link = _index_link(p.args.bam_fn, p.out_dir)
    if link is None:
        return p.args.bam_fn
    # without an index every contig would cost a pass over the whole file: build one next to a link in tmp/
    # (run_clair3_rna insists on an existing index, :469-477; samtools is not a dependency here).  Rank 0 alone builds it,
    # under temporary names that are renamed into place, and the other ranks open the BAM only after the barrier: nobody
    # ever sees a missing link or a half-written .bai
    build_err = None
    if p.rank == 0:
        from . import bamio
        try:
            tmp_link, tmp_bai = link + ".tmp%d" % os.getpid(), link + ".bai.tmp%d" % os.getpid()
            if os.path.lexists(tmp_link):
                os.remove(tmp_link)
            os.symlink(os.path.abspath(p.args.bam_fn), tmp_link)
            p.log("[INFO] %s has no .bai: building %s.bai" % (p.args.bam_fn, link))
            try:
                bamio.index_build(tmp_link, tmp_bai)
                os.replace(tmp_bai, link + ".bai")
                os.replace(tmp_link, link)
            finally:
                for t_ in (tmp_link, tmp_bai):
                    if os.path.lexists(t_):
                        os.remove(t_)
        except Exception as e:           # the other ranks are waiting at the barrier: reach it, then fail together
            build_err = e
    _all_ranks_ok(p.dist, p.world, build_err, "building the BAM index")
    return link


def _deal_contigs(p):
    """-> this rank's contigs, in calling order: all of them in one process."""
    if p.world == 1:
        return p.all_contigs
    from . import shard
    os.makedirs(p.parts_dir, exist_ok=True)
    p.dist.barrier()                                                    # CMD is in place before anybody builds the header
    # contigs are dealt by the WORK they hold ("by read count ... from the read index"): the mapped reads the BAM
    # index reports per contig (pseudo-bin 37450), else the compressed bytes its records span, else its length.  RNA coverage is
    # nowhere near proportional to length (chr19 against chr13), so a deal by length balances the wrong thing.
    costs, basis = shard.contig_costs(p.bam_fn, p.all_contigs, p.fai)
    plan = shard.lpt_assign(costs, p.world)
    if p.rank == 0:
        p.log("[INFO] %d contigs dealt to %d ranks by %s: load imbalance %.3f" % (len(p.all_contigs), p.world, basis, shard.imbalance(costs, plan)))
    return [p.all_contigs[i] for i in plan[p.rank]]


def _rediportal_table(args, contigs, log):
    """-> {(contig, pos): hit} of --readiportal_source_fn for `contigs`; {} when the file is missing; None without the flag."""
    if not args.tag_variant_using_readiportal:
        return None
    src = args.readiportal_source_fn
    if src is None or src.upper() == "NONE" or not os.path.exists(src):
        log("[WARNING] Enabled tagging variant using readiportal, but --readiportal_source_fn %s file not found, skip tagging!" % src)
        return {}
    tags = set(args.readiportal_database_filter_tag.split(":")) if args.readiportal_database_filter_tag is not None else None
    return sort_vcf.load_rediportal(src, contigs, tags)


# ---- stage 2: the GPU contexts
class _Engines(object):
    """The GPU contexts: created, given the weights and the arithmetic once the first fetches are under way (0.1-0.2 s that used to come
    before the first BAM byte was read).  Each context on a thread of its own: context 0 takes the first contig the moment IT is ready
    — HIP start-up and its own weights, 0.2 s in a fresh process — while the others' weights are still being packed (they are not needed
    before the second contig has been fetched)."""

    def __init__(self, p, n_ctx):
        self.p = p
        self.engines = [None] * n_ctx
        self.ready = [threading.Event() for _ in range(n_ctx)]
        self.errs, self.threads = [], []

    def start(self):
        """Returns at once; `get` waits for its engine."""
        for k in range(len(self.engines)):
            t_ = threading.Thread(target=self._bring_up, args=(k,), name="c3r-bringup%d" % k, daemon=True)
            self.threads.append(t_)
            t_.start()

    def _bring_up(self, k):
        from . import capi           # (capi.Engine is looked up here, when a context is made: tests put a stand-in there)
        p, args = self.p, self.p.args
        try:
            if k > 0:
                # (the process' first c3r_create starts HIP, and two contexts that pack and calibrate their weights at once take twice as long
                # each: context 0 first — it is the one the first contig waits for —, the others are ready long before their contig is fetched)
                self.ready[0].wait()
            t0 = time()
            e = capi.Engine(args.gpu_id)
            self.engines[k] = e
            p.mark("ctx%d" % k, "create", t0)
            t0 = time()
            e.load_weights(p.weights, p.channels)             # (packing the weights into the kernels' layouts is host work: side by side)
            p.mark("ctx%d" % k, "weights", t0)
            t0 = time()
            e.set_precision(args.gpu_precision)
            p.mark("ctx%d" % k, "precision", t0)
            if k == 0 and args.gpu_precision != "f16x3":
                p.log("[INFO] network arithmetic: %s -> %s (calibration max |dP| %s)" % ((args.gpu_precision,) + tuple(e.precision())))
        except BaseException as ex:
            self.errs.append(ex)
        finally:
            self.ready[k].set()

    def get(self, k):
        """Context k's engine, once it is up (raises what its bring-up raised)."""
        self.ready[k].wait()
        if self.errs:
            raise self.errs[0]
        return self.engines[k]

    def close(self):
        """After the pipeline has stopped: no thread is inside libc3r any more."""
        for t_ in self.threads:
            t_.join()
        for e in self.engines:
            if e is not None:
                e.close()


# ---- stage 3: the per-contig pipeline
class ContigResult(object):
    """What has become of a contig, as the stages hand it on — `kind` says which case holds, `value` is that case's payload:
        NO_READS   nothing mapped there: no payload
        RESIDENT   tensors built and the network launched: the number of candidates left resident in the context
        CHUNKS     genotyping mode, still to run chunk by chunk (each has its own site list): [((start, end), sites), ...]
        ROWS       the contig's rows as bytes, still to merge
        DECODING   decode (and merge) detached to a worker: a Future of a MERGED result
        MERGED     merged on the worker: SampleMerger.merge_only's result, for the ordered write — None when the worker wrote this
                   rank's part files itself (several ranks)"""
    NO_READS, RESIDENT, CHUNKS, ROWS, DECODING, MERGED = "no_reads", "resident", "chunks", "rows", "decoding", "merged"

    def __init__(self, kind, value=None):
        self.kind, self.value = kind, value


class _FetchJoin(object):
    """A contig's fetch as tasks of the fetch pool — one per position range (_Fetcher.plan), one for the reference and, with
    --phased_vcf_fn, one for the phase table — joined by whichever finishes last.  `future`: (ReadSet, reference, seconds, phase table or None)."""

    def __init__(self, p, pool, ctg):
        from concurrent.futures import Future
        self.p, self.ctg, self.t0, self.future = p, ctg, time(), Future()
        self.ranges = p.fetcher.plan(p.fai[ctg], max(1, p.args.fetch_threads))
        self.parts, self.ref, self.phase, self.err = [None] * len(self.ranges), b"", None, None
        self.left, self.lock = len(self.ranges) + 1 + int(p.phase_source is not None), threading.Lock()
        for k, (beg, end) in enumerate(self.ranges):
            pool.submit(self._task, self._part, k, beg, end)
        pool.submit(self._task, self._reference)
        if p.phase_source is not None:
            pool.submit(self._task, self._phase)

    def _part(self, k, beg, end):
        self.parts[k] = self.p.fetcher.part(self.ctg, beg, end)

    def _reference(self):
        self.ref = self.p.fetcher.reference(self.ctg, self.p.fai[self.ctg])

    def _phase(self):
        self.phase = self.p.phase_source.table(self.ctg)

    def _task(self, work, *a):
        try:
            work(*a)
        except BaseException as e:
            self.err = e
        with self.lock:
            self.left -= 1
            last = self.left == 0
        if not last:
            return
        p = self.p
        try:
            if self.err is not None:
                raise self.err
            rs = p.fetcher.join(self.parts)
            p.mark(self.ctg, "fetch", self.t0)
            if p.timeline:
                p.log("[timeline-fetch %s] %d range(s): %d reads, %d CIGAR ops, %.0f MB of bases, %.0f Mb of reference" % (self.ctg, len(self.ranges), len(rs.reads), len(rs.cigar), len(rs.seq) / 1e6, len(self.ref) / 1e6))
            self.future.set_result((rs, self.ref if len(rs.reads) else b"", time() - self.t0, self.phase))
        except BaseException as e:
            self.future.set_exception(e)


def _device_stage(p, eng, ctg, rs, ref, phase):
    """Reads, reference, tensor build and the network's launch on one context -> ContigResult RESIDENT, or CHUNKS in genotyping mode.
    phase: the contig's phase table (--phased_vcf_fn; None without the flag)."""
    from . import capi
    args = p.args
    extend_bed = existing(os.path.join(p.split_dir, ctg)) if p.bed_fn else None
    regions, site_sets, ext_iv = [], [], []
    for k in range(1, p.chunk_nums[ctg] + 1):
        a, b, sites, ext_iv = resolve_region(p.fai[ctg], ctg, k, p.chunk_nums[ctg], None, None, p.bed_fn, extend_bed, p.vcf_fn)
        if sites is not None and not sites:
            continue
        regions.append((a, b))
        site_sets.append(sites)
    if not regions:
        return ContigResult(ContigResult.RESIDENT, 0)
    eng.params = capi.default_params()
    eng.set_bed(0, ext_iv if extend_bed else None)
    eng.set_bed(1, io.read_bed(p.bed_fn, ctg)[0] if p.bed_fn else None)
    eng.set_params(channels=p.channels, min_mq=args.min_mq, min_coverage=args.min_coverage, snp_min_af=args.snp_min_af,
                   indel_min_af=args.indel_min_af, head_tail=int(args.enable_variant_calling_at_sequence_head_and_tail),
                   splice_padding=int(args.enable_padding_in_splice_junction_regions), genotyping_mode=int(p.vcf_fn is not None),
                   mpileup_compat=p.compat)
    if phase is not None:                            # (--phased_vcf_fn; without it a context never holds a table)
        eng.load_reads(_empty_reads())               # (the previous contig's reads are done with: a new table would tag them again first)
        if p.phase_source.left_align is not None:    # (--left_align_indels: the tagging reads the whole contig's reference, set below again for the scan)
            eng.set_reference(1, ref, upper_view=not isinstance(ref, (bytes, str)))
        if p.hap_realign:                            # (--hap_realign: the whole contig's reference likewise, then the switch)
            from . import phasing
            phasing.apply_hap_realign(eng, p.hap_realign, (1, ref), p.hap_realign_spliced, upper_view=not isinstance(ref, (bytes, str)))
        p.phase_source.apply(eng, phase)             # before the reads: they are tagged while they are prepared
        note = p.phase_source.indel_note(phase, "[INFO] %s: %d phased sites in the table of --haplotag_indels, " % (ctg, len(phase)))
        if note:
            p.log(note)
        if not len(phase):
            rs.reads["hp"] = 0                       # nothing phased on this contig: every read untagged (the BAM's own HP tags do not count beside a phased VCF)
    t = [time()]
    from . import phasing
    phasing.load_reads_min_bq(eng, rs, p.hap_min_bq if phase is not None else 0, ctg, p.log, **(dict(weights=True) if p.hap_bq_weights and phase is not None else {})); t.append(time())
    eng.set_reference(1, ref, upper_view=not isinstance(ref, (bytes, str))); t.append(time())      # (the fetcher's array: upper-cased, used in place)
    if p.vcf_fn is not None:
        return ContigResult(ContigResult.CHUNKS, list(zip(regions, site_sets)))                   # genotyping mode: one scan per chunk (its own site list)
    eng.begin_batch()
    eng.scan_regions(regions)
    eng.end_batch()
    n = eng.n_candidates
    t.append(time())
    if n:
        # (launched as soon as the tensors exist, side by side with the other context's pass: making the contexts take
        # turns for the network — one copies while the other computes — measured 3.1-3.3 s against 2.7-2.8 s)
        eng.infer(fetch=False)
    t.append(time())
    if os.environ.get("C3R_TIMING"):
        p.log("[device_stage %s] load_reads %.0f ms, set_reference %.0f ms, scan %.0f ms, infer launch %.0f ms (%d reads, %d sites)"
              % (ctg, 1e3 * (t[1] - t[0]), 1e3 * (t[2] - t[1]), 1e3 * (t[3] - t[2]), 1e3 * (t[4] - t[3]), len(rs.reads), n))
    return ContigResult(ContigResult.RESIDENT, n)


def _decode_stage(p, eng, ctg, todo):
    """The rows of a RESIDENT or CHUNKS contig, decoded on the context's own thread -> ContigResult ROWS."""
    show_ref = p.args.print_ref_calls
    rows = b""
    if todo.kind == ContigResult.CHUNKS:
        for (a, b), sites in todo.value:
            eng.set_sites(sites)
            if eng.scan(a, b):
                eng.infer(fetch=False)
                rows += eng.call_rows_text(ctg, qual=p.qual_rows, show_ref=show_ref)[0]
    elif todo.value:
        rows = eng.call_rows_text(ctg, qual=p.qual_rows, show_ref=show_ref)[0]
    return ContigResult(ContigResult.ROWS, rows)


class _Pipeline(object):
    """Fetch threads -> look-ahead slots -> context threads -> decode workers -> the ordered write.  Everything the threads share is made
    here, before any of them starts."""

    def __init__(self, p):
        import queue
        self.p, args = p, p.args
        self.n_ctx = n_ctx = max(1, args.contexts)
        self.engines = _Engines(p, n_ctx)
        # contigs fetched (or being fetched) but not yet through their context: every context busy + every fetch thread running ahead.
        # (n_ctx + 2 starved the contexts: a fetch takes ~100 ms, a context needs a new contig every ~35 ms)
        self.slots = threading.BoundedSemaphore(n_ctx + max(2, args.fetch_threads))
        self.stats, self.lock = dict(fetch=0.0, dev=0.0, sites=0), threading.Lock()
        # candidates per kb of contig: ~3 on the synthetic GRCh38-sized samples, so a contig past ~50 Mb fills a whole network slice
        self.reserve_sites = min(262144, int(max(p.fai[c] for c in p.contigs) * 0.005)) if p.contigs else 0
        self.ctx_queue = queue.Queue()                                       # (contig, fetch future, result future) in calling order; None ends a worker
        self.ctx_threads = [threading.Thread(target=self.context_worker, args=(k,), name="c3r-ctx%d" % k, daemon=True) for k in range(n_ctx)]
        # snapshots -> rows (-> merged records), beside the contexts.  A large contig's merge is 0.2-0.7 s on one thread when every
        # candidate is a record: with n_ctx + 1 workers the snapshots queued up behind three merges (full-length GRCh38 timeline)
        self.n_dec = int(os.environ.get("C3R_DECODE_WORKERS", "0")) or max(2, min(8, (p.n_thr if p.world > 1 else (os.cpu_count() or 8)) // 4))
        self.decode_pool = ThreadPoolExecutor(self.n_dec)
        self.snap_slots = threading.Semaphore(self.n_dec + 2)                # snapshots taken but not decoded yet
        self.eng_decodes = [[] for _ in range(n_ctx)]                        # decode futures per context (its worker waits for them before it closes the engine)
        self.stop = threading.Event()
        self.tasks = [None] * len(p.contigs)                                 # per contig: the Future of its ContigResult, once submitted
        self.submitted = [threading.Event() for _ in p.contigs]
        self.feeder_err = []
        self.part_counts = {}                                                # several ranks: {index in all_contigs: (read, kept, tagged)}
        self.t_merge, self.called = 0.0, []

    def merge_contig(self, ctg, rows):
        p = self.p
        if p.world == 1:
            p.merger.add_contig(ctg, rows)
        else:                                 # this contig's records on their own; rank 0 concatenates in calling order
            k = p.all_contigs.index(ctg)
            m = sort_vcf.SampleMerger(os.path.join(p.parts_dir, "%05d.vcf" % k), "", p.qual_merge, p.args.print_ref_calls, p.table,
                                      os.path.join(p.parts_dir, "%05d_nt.vcf" % k), edits=p.edits)
            m.add_contig(ctg, rows)
            # (close: an empty part — nothing was written to it — is made anew as the empty file it was, and the warning about it is rank 0's to
            # give for the whole output, not a part's)
            self.part_counts[k] = m.close(log=lambda _m: None)

    def context_task(self, k, eng, ctg, fut):
        """One contig on context k, whose thread took it from the queue (contigs are taken in calling order by whichever context
        is free): host preparation + uploads, tensor build, network, snapshot.  Contexts work side by side — while one waits for
        its kernels another queues its uploads and scans.  -> ContigResult NO_READS, ROWS or DECODING."""
        p = self.p
        try:
            rs, ref, dt, phase = fut.result()
            if not len(rs.reads):
                return ContigResult(ContigResult.NO_READS)
            # (A context sizes its device buffers on its first contig.  Round 2 made first uses take turns, each on a quiet GPU,
            # because a multi-GB hipMalloc under another context's kernels took 0.3-0.5 s; with the network's buffers reserved
            # ahead (c3r_reserve) what is left is cheaper than the wait: 1.38-1.47 s against 1.58-1.60 s on 22 half-length contigs.)
            t0 = time()
            todo = _device_stage(p, eng, ctg, rs, ref, phase)
            t1 = time()
            p.mark(ctg, "device", t0)
            with self.lock:
                self.stats["fetch"] += dt
                self.stats["dev"] += t1 - t0
                self.stats["sites"] += todo.value if todo.kind == ContigResult.RESIDENT else 0
            if todo.kind == ContigResult.RESIDENT and todo.value and hasattr(eng, "rows_begin"):
                # the decode inputs leave the context as a host snapshot (c3r_rows_begin): this thread goes on to the next contig
                # while a decode worker turns the snapshot into rows and — single process — merges them (c3r_vcf_merge)
                # (snapshots hold ~0.3 GB of staging and their contig's reference: the contexts may not run further ahead of the decode
                # pool than it has workers + 2)
                self.snap_slots.acquire()
                try:
                    # (without --print_ref_calls the sites the decoder's early RefCall exit would drop anyway stay on the device; the decoder
                    # reads inserted bases from the fetched arrays in place — the snapshot keeps them alive)
                    snap = eng.rows_begin(drop_ref_calls=not p.args.print_ref_calls)
                except BaseException:
                    self.snap_slots.release()
                    raise
                p.mark(ctg, "snapshot", t1)
                fut_d = self.decode_pool.submit(self.decode_task, snap, ctg)     # (the look-ahead slot is free: the fetched arrays are done with)
                self.eng_decodes[k].append(fut_d)
                return ContigResult(ContigResult.DECODING, fut_d)
            res = _decode_stage(p, eng, ctg, todo)
            p.mark(ctg, "decode", t1)
            return res
        finally:
            self.slots.release()

    def decode_task(self, snap, ctg):
        """On a decode worker: a snapshot -> rows -> merged records (one process) or this rank's part files -> ContigResult MERGED."""
        p = self.p
        try:
            t0 = time()
            # (rows stay a uint8 array from here to the compressed piece: no 100-MB bytes objects built under the GIL)
            rows = snap.decode(ctg, qual=p.qual_rows, show_ref=p.args.print_ref_calls, as_array=True)[0]
            p.mark(ctg, "decode", t0)
            t1 = time()
            if p.world == 1:
                res = ContigResult(ContigResult.MERGED, p.merger.merge_only(ctg, rows))
            else:
                self.merge_contig(ctg, rows)               # this rank's part files of the contig, written here on the worker
                res = ContigResult(ContigResult.MERGED)
            p.mark(ctg, "merge", t1)
            return res
        finally:
            self.snap_slots.release()

    def context_worker(self, k):
        """Thread of context k: contigs from the shared queue until the end marker, then — once the decodes that still read this
        context's snapshots are through — the context is released: device and page-locked memory go back while the last contigs
        are still being decoded and written."""
        p = self.p
        try:
            eng = self.engines.get(k)
        except BaseException as e:           # the bring-up failed: every contig this worker takes fails with that
            while True:
                item = self.ctx_queue.get()
                if item is None:
                    return
                if item[2].set_running_or_notify_cancel():
                    item[2].set_exception(e)
        if self.reserve_sites and hasattr(eng, "reserve"):
            # the network's buffers (8.9 GB for a full slice: 0.25-0.4 s of a first hipMalloc) while the first fetch is under way
            t0 = time()
            try:
                eng.reserve(self.reserve_sites)
            except Exception:
                pass                      # (the first infer() sizes them, and reports whatever is wrong)
            p.mark("ctx%d" % k, "reserve", t0)
        while True:
            item = self.ctx_queue.get()
            if item is None:
                break
            ctg, fut, out = item
            if not out.set_running_or_notify_cancel():          # (cancelled by the failure path, which released its slot)
                continue
            try:
                out.set_result(self.context_task(k, eng, ctg, fut))
            except BaseException as e:
                out.set_exception(e)
        t0 = time()
        for f in list(self.eng_decodes[k]):
            try:
                f.result()
            except BaseException:
                pass                      # (reported by the main loop, which holds the same future)
        if not self.stop.is_set():
            eng.close()
            p.mark("ctx%d" % k, "close", t0)

    def stop_workers(self):
        """Failure path: nothing may still be inside a c3r_* call (or queued to make one) when the engines are destroyed.  Queued
        contigs are cancelled, the running ones finish, and the feeder — possibly parked on a look-ahead slot that a cancelled task
        will never release — is told to stop and woken.  Idempotent."""
        import queue
        self.stop.set()
        while True:                       # contigs no context has taken yet are cancelled; the running ones finish
            try:
                item = self.ctx_queue.get_nowait()
            except queue.Empty:
                break
            if item is not None:
                item[2].cancel()
                try:
                    self.slots.release()
                except ValueError:
                    pass
        for _ in range(self.n_dec + self.n_ctx + 4):   # (a context parked on a snapshot slot whose decode will be cancelled below)
            self.snap_slots.release()
        for _t in self.ctx_threads:
            self.ctx_queue.put(None)
        for t_ in self.ctx_threads:
            if t_.is_alive():
                t_.join()
        self.decode_pool.shutdown(wait=True, cancel_futures=True)
        for _ in range(len(self.p.contigs) + self.n_ctx + self.p.args.fetch_threads + 2):
            try:
                self.slots.release()
            except ValueError:           # (bounded semaphore: every slot is free again)
                break

    def feeder(self, fetch_pool):
        """Takes the look-ahead slot BEFORE it submits a contig's fetch, strictly in calling order.  (Taken inside the fetch workers, a
        later contig could grab the last slot while the one its context needs next was still waiting for one — every context consumes
        its contigs in order, so nothing would ever have released a slot again.)"""
        from concurrent.futures import Future
        try:
            for i, c in enumerate(self.p.contigs):
                self.slots.acquire()
                if self.stop.is_set():
                    break
                fut = _FetchJoin(self.p, fetch_pool, c).future
                self.tasks[i] = Future()
                self.ctx_queue.put((c, fut, self.tasks[i]))
                self.submitted[i].set()
            for _k in range(self.n_ctx):
                self.ctx_queue.put(None)
        except BaseException as e:          # (e.g. the pools were shut down by a failure below)
            self.feeder_err.append(e)
        finally:
            for ev in self.submitted:
                ev.set()

    def close_fetcher(self, feed, fetch_pool):
        """The BAM handles (the mapped file, the record buffers of the largest contig each thread fetched) go as soon as
        the last fetch is through, beside the contexts' last contigs."""
        feed.join()
        fetch_pool.shutdown(wait=True)          # (every fetch has been submitted; the with-block's own shutdown is then a no-op)
        t0 = time()
        self.p.fetcher.close()
        self.p.mark("all", "bam_close", t0)

    def collect(self, i, ctg):
        """The main thread's step per contig, in calling order: its result, merged (if a worker has not done that) and written."""
        p = self.p
        self.submitted[i].wait()
        if self.tasks[i] is None:
            raise RuntimeError("contig %s was never submitted: %r" % (ctg, self.feeder_err[:1]))
        res = self.tasks[i].result()
        self.tasks[i] = None
        if res.kind == ContigResult.NO_READS:
            p.log("[WARNING] Contig name %s provided but no mapped reads found in BAM, skip!" % ctg)
            return
        if res.kind == ContigResult.DECODING:
            res = res.value.result()
        t0 = time()
        if res.kind == ContigResult.MERGED:
            if res.value is not None:
                p.merger.write_merged(res.value)               # merged on the worker: only the ordered write is left
        else:
            self.merge_contig(ctg, res.value)
        self.t_merge += time() - t0
        p.mark(ctg, "write" if res.kind == ContigResult.MERGED else "merge", t0)
        self.called.append(ctg)

    def run(self):
        """All contigs of this rank through the pipeline.  On any failure the workers are stopped first (stop_workers) and the error
        goes on to the caller."""
        p = self.p
        with ThreadPoolExecutor(max(1, p.args.fetch_threads)) as fetch_pool:
            feed = threading.Thread(target=self.feeder, args=(fetch_pool,), name="c3r-feeder", daemon=True)
            feed.start()
            closer = threading.Thread(target=self.close_fetcher, args=(feed, fetch_pool), name="c3r-closer", daemon=True)
            closer.start()
            try:
                t0 = time()
                self.engines.start()                                       # (the first fetches are running)
                p.mark("all", "engines", t0)
                for t_ in self.ctx_threads:
                    t_.start()
                for i, ctg in enumerate(p.contigs):                        # merge in calling order as the contigs come out
                    self.collect(i, ctg)
            except BaseException:
                self.stop_workers()      # before the fetch pool's own shutdown waits for fetches nobody will consume
                raise
        t0 = time()
        for t_ in self.ctx_threads:
            t_.join()
        self.decode_pool.shutdown()
        closer.join()
        p.mark("all", "shutdown", t0)


# ---- stage 4: rank assembly and finalisation
def _load_part(merger, fns):
    """One contig's merged records as the ranks left them -> what SampleMerger.append_part takes: with compressed output a piece
    compressed and indexed here, on a pool thread (the ordered step is then a file append), else the text."""
    out = []
    for fn_, want in ((fns[0], True), (fns[1], merger.out_nt_fn is not None)):
        if not want or not os.path.exists(fn_):
            out.append(None)
        elif merger.stream_gz:
            from . import bamio
            data = np.fromfile(fn_, dtype=np.uint8)
            out.append(bamio.VcfPiece(data) if data.size else None)
        else:
            out.append(open(fn_).read())
    return out


def _assemble(p):
    """Rank 0 under several ranks: the parts of all ranks, in calling order, into the output -> (contigs called, candidate sites)."""
    import json
    called_set, n_sites, counts = set(), 0, {}
    for r in range(p.world):
        j = json.load(open(os.path.join(p.parts_dir, "rank%d.json" % r)))
        called_set.update(j["called"])
        n_sites += j["n_sites"]
        counts.update((int(k), tuple(v)) for k, v in j["counts"].items())
    todo = []
    for k, c in enumerate(p.all_contigs):
        fn = os.path.join(p.parts_dir, "%05d.vcf" % k)
        if c in called_set and os.path.exists(fn) and os.path.getsize(fn):
            todo.append((k, (fn, os.path.join(p.parts_dir, "%05d_nt.vcf" % k))))
    with ThreadPoolExecutor(max(1, min(8, p.n_thr // 4 or 1))) as part_pool:
        for (k, _fns), (main_part, nt_part) in zip(todo, part_pool.map(lambda job: _load_part(p.merger, job[1]), todo)):
            p.merger.append_part(main_part, nt_part, counts.pop(k, (0, 0, 0)))
    for c in counts.values():                                          # (contigs that left no record still count as read)
        p.merger.append_part(None, None, c)
    return [c for c in p.all_contigs if c in called_set], n_sites


def _finish(p, called, n_sites, t_setup, t_fetch, t_dev, t_merge):
    """The output closed (and compressed, unless it was streamed), tmp/CONTIGS and tmp/CHUNK_LIST, the summary lines."""
    args, log = p.args, p.log
    t0 = time()
    n_read, n_kept, n_tag = p.merger.close(log)
    p.mark("all", "close_out", t0)
    # tmp/CONTIGS and tmp/CHUNK_LIST as run_clair3_rna leaves them (:436-449): contigs without reads are dropped by its
    # `samtools idxstats` check (:184-210) before they are written; here that is known once the contig has been fetched
    with open(os.path.join(p.out_dir, "tmp", "CONTIGS"), "w") as f:
        f.write("\n".join(called))
    with open(os.path.join(p.out_dir, "tmp", "CHUNK_LIST"), "w") as f:
        for c in called:
            for k in range(1, p.chunk_nums[c] + 1):
                f.write("%s %d %d\n" % (c, k, p.chunk_nums[c]))
    t0 = time()
    if not args.no_compress and not getattr(p.merger, "streamed", False):      # (streamed: <out>.vcf.gz + .tbi are complete already)
        sort_vcf.compress_vcf(p.out_fn)
        if p.table is not None and n_kept:
            sort_vcf.compress_vcf(p.out_nt_fn)
    if p.table is not None:
        log("[INFO] Dataset size:%d, total variants tagged by REDIportal dataset: %d" % (len(p.table), n_tag))
    log("[INFO] %d contigs, %d candidate sites, %d records written to %s%s" % (len(called), n_sites, n_kept, p.out_fn, "" if args.no_compress else ".gz"))
    t_gz = time() - t0
    log("[INFO] set-up %.2f s, fetch %.2f s (overlapped), device stage %.2f s, merge %.2f s, bgzip+tabix %.2f s, total %.2f s"
        % (t_setup, t_fetch, t_dev, t_merge, t_gz, time() - p.t_all))


def _run_pass(args, log=None):
    """One pass over the sample: set-up (_set_up), the contexts' bring-up and the per-contig pipeline (_Pipeline), then — on rank 0 —
    assembly and finalisation (_assemble, _finish).  With several ranks every rank reaches each of the three rendezvous, whatever failed."""
    log = log or (lambda m: print(m, file=sys.stderr))
    t_all = time()
    p = _set_up(args, log, t_all)
    if p is None:
        return 0
    t_setup = time() - t_all
    pipe = _Pipeline(p)
    work_err = None
    try:
        pipe.run()
    except Exception as e:               # with several ranks: reach the rendezvous first, then every rank fails
        work_err = e
        pipe.stop_workers()              # (idempotent) no thread is inside libc3r any more
        if p.merger is not None:
            p.merger.discard()           # no truncated output.vcf.gz (without EOF block) beside a stale .tbi
        if p.world == 1:
            pipe.engines.close()
            raise
    pipe.engines.close()
    called, n_sites = pipe.called, pipe.stats["sites"]
    if p.world > 1:
        import json
        with open(os.path.join(p.parts_dir, "rank%d.json" % p.rank), "w") as f:
            json.dump(dict(counts={str(k): v for k, v in pipe.part_counts.items()}, called=called, n_sites=n_sites), f)
        _all_ranks_ok(p.dist, p.world, work_err, "calling its contigs")
        if p.rank != 0:
            _all_ranks_ok(p.dist, p.world, None, "assembling the output")  # leave only when rank 0 has written the result
            return 0
    fin_err = None
    try:
        if p.world > 1:
            called, n_sites = _assemble(p)
        _finish(p, called, n_sites, t_setup, pipe.stats["fetch"], pipe.stats["dev"], pipe.t_merge)
    except Exception as e:               # rank 0 still meets the others at the last rendezvous, and all of them fail
        fin_err = e
        if p.merger is not None:
            p.merger.discard()
        if p.world == 1:
            raise
    if p.world > 1:
        _all_ranks_ok(p.dist, p.world, fin_err, "assembling the output")
    return 0


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        try:
            return Run(args)
        finally:
            try:                          # the 8.9-GB blocks libc3r.so keeps for a process's next context: this process has none
                from . import capi
                capi.trim()
            except Exception:
                pass
    except SystemExit:
        raise
    except Exception as e:       # fail loudly: there is no CPU fallback
        print("[ERROR] call_sample (MI355X path) failed: %s" % e, file=sys.stderr)
        return 1
    finally:
        # (the command-line run owns the process group Run() created: taken down here rather than by the interpreter's exit)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            try:
                import torch.distributed as dist
                if dist.is_initialized():
                    dist.destroy_process_group()
            except Exception:
                pass


if __name__ == "__main__":
    sys.exit(main())
