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
no left-alignment of the reads' indels, no base qualities; homozygous rows and rows with three or more ALTs are not candidates.  The
second pass reads such a directory with `--haplotag_indels`.

The rule (include/c3r.h: c3r_phase_links / c3r_phase_resolve) is a greedy linkage chain, not whatshap's wMEC: agreement with whatshap has
not been measured.

    python -m clair3_rna_amd.phase_vcf --bam_fn x.bam --vcf_fn out/output.vcf.gz --output_dir out/tmp/phased_output/phased_vcf
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
      help="also phase heterozygous insertions, deletions and 1/2 rows (alleles read off the CIGAR position; default: SNVs only)")
    a("--gpu_id", type=int, default=None, help="default: $C3R_DEVICE, else 0")
    return p


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
    per = phasing.allele_candidates_from_vcf(args.vcf_fn, None) if indels else phasing.candidates_from_vcf(args.vcf_fn, None)
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
            rs = io.load_reads(args.bam_fn, ctg)
            eng.load_reads(rs)
            fn = os.path.join(args.output_dir, "phased_%s.vcf.gz" % ctg)
            if indels:
                pool, strings = rest[0], rest[1]
                ps, h1, st = eng.phase_allele_sites(sites, pool, args.min_reads, args.min_agree_pct, merge_levels)
                phasing.write_allele_phased_vcf(args.vcf_fn, ctg, sites, strings, ps, h1, fn)
            else:
                out, st = eng.phase_sites(sites, args.min_reads, args.min_agree_pct, merge_levels)
                phasing.write_phased_vcf(args.vcf_fn, ctg, out, fn)
            written.append(fn)
            merged = ", block merge: %d units joined in %d levels" % (st["merge_units_joined"], st["merge_levels_run"]) if merge_levels else ""
            log("[INFO] %s: %d reads, %d candidate sites%s (%s), %d phased in %d blocks, largest block %d sites%s -> %s"
                % (ctg, len(rs), st["n_sites"], " with indels and two-ALT rows" if indels else "", ", ".join("%s %d" % (k, v) for k, v in sorted(skipped.items()) if v and k != "other_contig") or "none skipped",
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
