"""Phase the first pass's heterozygous SNVs on the GPU from read linkage: what `whatshap phase` / `longphase phase` do between the two
passes of the reference flow (run_clair3_rna:749-761), without an external tool.

Per contig: the alignments (io.load_reads) -> Engine.load_reads -> Engine.phase_sites on the contig's candidates (phasing.candidates_from_vcf:
PASS, biallelic SNV, GT 0/1) -> <output_dir>/phased_<ctg>.vcf.gz, the names `--phased_vcf_fn <output_dir>` of call_sample and call_var_bam
consume (phasedvcf.contig_file).  A contig without candidates writes no file.  One [INFO] line per contig.

--merge_levels N (default 0: off) runs up to N levels of the block-merge stage after the chain (include/c3r.h: c3r_phase_unit_links /
c3r_phase_merge): blocks that reads bridge across a run of unlinked sites — RNA-editing sites called 0/1 — become one.  The [INFO] line
then also says how many units joined in how many levels.

--indels (default off, as `whatshap phase --indels` is): the candidates are every heterozygous row whose alleles are SNVs, insertions or
deletions — `0/1` with one ALT, `1/2` with two (phasing.allele_candidates_from_vcf) —, phased by Engine.phase_allele_sites (include/c3r.h:
c3r_phase_allele_links) and written as `0|1` / `1|0` / `1|2` / `2|1` + PS.  The alleles are read off the CIGAR position: no realignment,
no left-alignment of the reads' indels, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes); homozygous rows and rows with three or more ALTs are not candidates.  The
second pass reads such a directory with `--haplotag_indels`.

--left_align_indels (default off; needs --indels and --ref_fn) lifts "no left-alignment": the candidates' indels are brought to their
left-most form against the reference (phasing.left_align_table) and each read's indel to its left-most place inside its own M run, on the
device (include/c3r.h: c3r_set_hap_left_align), so that a read whose aligner placed the indel elsewhere in a homopolymer or a short tandem
repeat shows the allele and not the reference.  A row whose alleles cannot move together is no candidate (`not_left_alignable`), nor is the
later of two that land on one position (`same_pos_after_left_align`).  Written rows keep their POS, REF and ALT.  What remains: a shift
stops at the M run's start, at an N or another indel, and at the contig's ends; no realignment, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes); agreement with whatshap
is not measured.

The rule (include/c3r.h: c3r_phase_links / c3r_phase_resolve) is a greedy linkage chain, not whatshap's wMEC: agreement with whatshap has
not been measured.

    python -m clair3_rna_amd.phase_vcf --bam_fn x.bam --vcf_fn out/output.vcf.gz --output_dir out/tmp/phased_output/phased_vcf

--hap_realign [W] (default off; needs --ref_fn; excludes --left_align_indels) lifts "no realignment": every read's window of W reference bases
around a site is compared with the site's two alleles and the smaller unit-cost edit distance decides (include/c3r.h: c3r_set_hap_realign;
phasing.apply_hap_realign).  Without --indels the SNV candidates go through the allele calls, which give the SNV calls' results bit for bit
with the switch off, so only the observation changes.  No quality weights, no affine gaps; a window stops at a splice junction
unless --hap_realign_spliced is given (include/c3r.h: c3r_set_hap_realign_spliced): then it is counted in the read's own spliced positions.
"""
import argparse
import os
import sys

from . import io, phasing


def build_parser():
    p = argparse.ArgumentParser(description="Phase the heterozygous SNVs of a pileup VCF from read linkage on MI355X (stands where `whatshap phase` stands in run_clair3_rna)")
    a = p.add_argument
    a("-b", "--bam_fn", type=str, required=True, help="the BAM (or flat read archive .npz) the VCF was called from")
    a("--vcf_fn", type=str, required=True, help="the first pass's VCF, plain or gzipped")
    a("-o", "--output_dir", type=str, required=True, help="receives phased_<ctg>.vcf.gz per contig")
    a("-c", "--ctg_name", type=str, default=None, help="contigs, comma-separated; default: every contig of the VCF")
    a("--min_mq", type=int, default=5, help="reads below it do not vote (the tensor build's filter)")
    a("--min_reads", type=int, default=2, help="fewest linking observations that let a site join a block")
    a("--min_agree_pct", type=int, default=75, help="fewest per cent of them that agree on the orientation")
    a("--merge_levels", type=int, default=0,
      help="levels of the block-merge stage after the chain: joins the blocks that reads bridge across a run of unlinked sites (0: off)")
    a("--indels", action="store_true",
      help="also phase heterozygous insertions, deletions and 1/2 rows (alleles read off the CIGAR position, no left-alignment unless "
           "--left_align_indels is given; default: SNVs only)")
    a("--left_align_indels", action="store_true",
      help="with --indels: left-align the candidates' indels against --ref_fn and every read's indel inside its M run, on the device "
           "(default: the alleles are read off the CIGAR position as they stand)")
    a("--ref_fn", type=str, default=None, help="the reference FASTA with its .fai: needed by --left_align_indels and --hap_realign only")
    phasing.add_hap_realign_flag(a)
    a("--hap_min_bq", type=int, default=0, metavar="N",
      help="a base whose quality is below N does not vote: the steps that hold reads against a site table read it as N (include/c3r.h: c3r_set_hap_min_bq; 0 .. 93, default 0: off).  A threshold, not whatshap's quality weights (--hap_bq_weights are those); an indel's own quality is not modelled; reads without qualities are never masked; agreement with whatshap is not measured")
    a("--gpu_id", type=int, default=None, help="default: $C3R_DEVICE, else 0")
    return p


def left_align_reference(args, needs, has):
    """The contig -> reference slice function of --left_align_indels, or None without the flag; refuses the flag without its
    prerequisite (`needs`: the flag's name, `has`: is it given) or without --ref_fn."""
    if not getattr(args, "left_align_indels", False):
        return None
    if not has:
        sys.exit("[ERROR] --left_align_indels needs %s" % needs)
    ref_fn = getattr(args, "ref_fn", None)
    if not ref_fn:
        sys.exit("[ERROR] --left_align_indels needs --ref_fn")
    if not os.path.isfile(ref_fn):
        sys.exit("[ERROR] file %s not found" % ref_fn)
    return io.contig_reference(ref_fn)


def Run(args, log=None):
    from . import capi
    log = log or (lambda m: print(m, file=sys.stderr))
    for need in (args.bam_fn, args.vcf_fn):
        if not os.path.isfile(need):
            sys.exit("[ERROR] file %s not found" % need)
    if args.min_reads < 0 or not 0 <= args.min_agree_pct <= 100:
        sys.exit("[ERROR] --min_reads must be >= 0 and --min_agree_pct between 0 and 100")
    merge_levels = getattr(args, "merge_levels", 0)
    if merge_levels < 0:
        sys.exit("[ERROR] --merge_levels must be >= 0")
    indels = bool(getattr(args, "indels", False))
    ref_of = left_align_reference(args, "--indels", indels)
    min_bq = phasing.hap_min_bq_arg(args, True, "")
    realign, realign_ref = phasing.hap_realign_arg(args)
    per = phasing.allele_candidates_from_vcf(args.vcf_fn, None, *(() if ref_of is None else (ref_of,))) if indels else phasing.candidates_from_vcf(args.vcf_fn, None)
    what = "heterozygous SNV / indel / two-ALT" if indels else "heterozygous SNV"
    contigs = args.ctg_name.split(",") if args.ctg_name else list(per)
    os.makedirs(args.output_dir, exist_ok=True)
    gpu_id = args.gpu_id if args.gpu_id is not None else int(os.environ.get("C3R_DEVICE", "0"))
    eng = None
    written = []
    try:
        for ctg in contigs:
            sites, *rest = per.get(ctg, (None, None))
            skipped = rest[-1]
            if sites is None or not len(sites):
                io.remove_stale(args.output_dir, lambda name: name == "phased_%s.vcf.gz" % ctg)     # (an earlier run's: the second pass would read it)
                log("[INFO] %s: no %s candidates, nothing written" % (ctg, what))
                continue
            if eng is None:
                eng = capi.Engine(gpu_id)
                eng.set_params(min_mq=args.min_mq)
            rs = io.load_reads(args.bam_fn, ctg, **(dict(want_quals=True) if min_bq else {}))
            if ref_of is not None:                            # (the whole contig: it covers every read)
                eng.set_reference(*ref_of(ctg))
                eng.set_hap_left_align(True)
            if realign:
                phasing.apply_hap_realign(eng, realign, realign_ref(ctg), phasing.hap_realign_spliced_arg(args))
            phasing.load_reads_min_bq(eng, rs, min_bq, ctg, log)
            fn = os.path.join(args.output_dir, "phased_%s.vcf.gz" % ctg)
            if indels:
                pool, strings = rest[0], rest[1]
                ps, h1, st = eng.phase_allele_sites(sites, pool, args.min_reads, args.min_agree_pct, merge_levels)
                phasing.write_allele_phased_vcf(args.vcf_fn, ctg, sites, strings, ps, h1, fn)
            elif realign:                                     # (the SNV table through the allele calls: only the observation changes)
                out = sites.copy()
                out["ps"], out["h1"], st = eng.phase_allele_sites(phasing.snv_sites_as_alleles(sites)[0], None, args.min_reads, args.min_agree_pct, merge_levels)
                phasing.write_phased_vcf(args.vcf_fn, ctg, out, fn)
            else:
                out, st = eng.phase_sites(sites, args.min_reads, args.min_agree_pct, merge_levels)
                phasing.write_phased_vcf(args.vcf_fn, ctg, out, fn)
            written.append(fn)
            merged = ", block merge: %d units joined in %d levels" % (st["merge_units_joined"], st["merge_levels_run"]) if merge_levels else ""
            log("[INFO] %s: %d reads, %d candidate sites%s%s (%s), %d phased in %d blocks, largest block %d sites%s -> %s"
                % (ctg, len(rs), st["n_sites"], " with indels and two-ALT rows" if indels else "", phasing.left_align_note(skipped), ", ".join("%s %d" % (k, v) for k, v in sorted(skipped.items()) if v and k != "other_contig") or "none skipped",
                   st["n_phased"], st["n_blocks"], st["max_block"], merged, fn))
    finally:
        if eng is not None:
            eng.close()
    return written


def main(argv=None):
    Run(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
