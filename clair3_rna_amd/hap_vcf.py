"""Phase the FINAL VCF of a phased run and report every call's haplotype support: per-haplotype allele counts on the GPU from the reads
that the phased VCF haplotags (include/c3r.h: c3r_hap_counts / c3r_hap_assign), without an external tool.

Per contig: the phase table through phasedvcf (exactly what the 30-channel pass reads) -> the candidates of the final VCF
(phasing.candidates_from_vcf: PASS, biallelic SNV, GT 0/1, first row of a position), each counted against the phase set of the NEAREST
table site by position (at equal distance the one before; a candidate that is itself a table site gets its own set) ->
Engine.set_params(min_mq), set_phase_sites, load_reads, hap_counts, hap_assign.  A candidate on which the haplotype-tagged reads agree
gets GT `0|1` / `1|0` and its set's PS (phasing.phased_row: the row rewrite of phase_vcf); every other row is written byte for byte.  All
contigs go to one file; an --output_fn that ends in .gz is bgzipped and tabix-indexed.  A contig whose table is empty keeps its rows
unchanged and has no line in the counts file.  One [INFO] line per contig.

--hap_counts_fn: one tab-separated line per candidate, phased or not — COLUMNS below; PS is the set the reads were counted against, GT
says whether the candidate was phased in it; HP1 / HP2 / NONE are the reads tagged 1, tagged 2 and the others (untagged, tied, or tagged in
another set), REF / ALT / OTHER the allele the read shows.

By default it covers SNVs only and is a majority rule over CIGAR-position alleles: no indels, no multi-allelic or homozygous rows, no
realignment, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes).  Agreement with `whatshap` has not been measured.

--indels (off by default, like `whatshap phase --indels`): the candidates are phasing.allele_candidates_from_vcf's — heterozygous rows whose
alleles are SNVs, insertions or deletions, GT `0/1` with one ALT or `1/2` with two (`C  T,CGG`, `ACC  A,TCC`) — counted by
Engine.hap_allele_counts (include/c3r.h: c3r_hap_allele_counts) and written as `0|1` / `1|0` / `1|2` / `2|1`.  The nearest-set rule and the
assignment are the same.  The counts file's REF / ALT columns then hold the row's strings, its REF / ALT count columns stand for allele A /
allele B, and one more column ALLELES says which they are: `0,1` or `1,2`.  The alleles are read off the CIGAR position: no realignment, no
left-alignment of the reads' indels, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes); a homozygous row or one with three or more ALTs stays as it is.  Agreement with
`whatshap --indels` has not been measured.  Without --indels both files are what they were.

--left_align_indels (off by default; needs --indels and --ref_fn) lifts "no left-alignment", as in phase_vcf: the candidates' indels are
left-aligned against the reference, each read's indel inside its own M run on the device (include/c3r.h: c3r_set_hap_left_align); with
--haplotag_indels the phase table is left-aligned too and the reads are tagged by the same observation.  Rows keep their POS, REF and ALT
in both files.  A shift stops at the M run's start, at an N or another indel and at the contig's ends; no realignment, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes);
agreement with whatshap is not measured.

    python -m clair3_rna_amd.hap_vcf --bam_fn x.bam --vcf_fn out/output_enable_phasing.vcf.gz \\
        --phased_vcf_fn out/tmp/phased_output/phased_vcf --output_fn out/phased.vcf.gz --hap_counts_fn out/hap_counts.tsv

--hap_realign [W] (off by default; needs --ref_fn; excludes --left_align_indels) lifts "no realignment", as in phase_vcf: the reads are realigned
against the two alleles of every site of the phase table and of every candidate (include/c3r.h: c3r_set_hap_realign); without --indels /
--haplotag_indels the SNV tables go through the allele calls, which give the SNV calls' results bit for bit with the switch off.
"""
import argparse
import os
import sys

import numpy as np

from . import io, phasing

COLUMNS = ("#CHROM", "POS", "REF", "ALT", "PS", "GT", "HP1_REF", "HP1_ALT", "HP1_OTHER", "HP2_REF", "HP2_ALT", "HP2_OTHER",
           "NONE_REF", "NONE_ALT", "NONE_OTHER")
ALLELE_COLUMNS = COLUMNS + ("ALLELES",)                     # --indels
_LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}


def nearest_sets(cands, table):
    """A copy of the candidate array (PHASE_SITE_DTYPE or HAP_SITE_DTYPE) whose ps is that of the nearest site of `table` (sorted by pos, not
    empty) by position; at equal distance the site before."""
    out = np.array(cands, copy=True)
    tpos = table["pos"].astype(np.int64)
    pos = out["pos"].astype(np.int64)
    after = np.searchsorted(tpos, pos, side="left")           # first table site at or behind the candidate
    before = after - 1
    a, b = np.clip(after, 0, len(tpos) - 1), np.clip(before, 0, len(tpos) - 1)
    take_after = (before < 0) | ((after < len(tpos)) & (tpos[a] - pos < pos - tpos[b]))
    out["ps"] = table["ps"][np.where(take_after, a, b)]
    if "h1" in out.dtype.names:
        out["h1"] = 0
    return out


def counts_lines(contig, cands, assigned, counts):
    """The counts file's lines for one contig's candidates (query sites, hap_assign's output, (n, 3, 3) counts)."""
    lines = []
    for c, o, t in zip(cands, assigned, counts):
        gt = ("1|0" if int(o["h1"]) else "0|1") if int(o["ps"]) >= 0 else "0/1"
        lines.append("\t".join([contig, str(int(c["pos"])), _LETTER[int(c["ref"])], _LETTER[int(c["alt"])], str(int(c["ps"])), gt]
                               + [str(int(t[r][a])) for r in (1, 2, 0) for a in (0, 1, 2)]) + "\n")
    return lines


def allele_counts_lines(contig, cands, strings, assigned, counts):
    """counts_lines under --indels: candidates of phasing.allele_candidates_from_vcf (query sites and their rows' (REF, ALT) strings),
    hap_assign's output, (n, 3, 3) counts."""
    lines = []
    for j, (c, o, t) in enumerate(zip(cands, assigned, counts)):
        ref, alt = strings[j][0], strings[j][1]
        a, b = ("1", "2") if "," in alt else ("0", "1")
        gt = (b + "|" + a if int(o["h1"]) else a + "|" + b) if int(o["ps"]) >= 0 else a + "/" + b
        lines.append("\t".join([contig, str(phasing.row_pos(cands, strings, j)), ref, alt, str(int(c["ps"])), gt]
                               + [str(int(t[r][k])) for r in (1, 2, 0) for k in (0, 1, 2)] + [a + "," + b]) + "\n")
    return lines


def write_vcf(in_vcf, assigned_by_contig, out_fn, strings_by_contig=None):
    """Every row of `in_vcf` to `out_fn` (a name that ends in .gz: bgzip + tabix): the rows of the sites of {contig: hap_assign's output} with
    ps >= 0 rewritten by phasing.phased_row, every other row byte for byte, the PS header line added unless present.  Returns the number
    of rows rewritten.  strings_by_contig ({contig: [(REF, ALT)] beside the sites}, --indels): phasing.allele_phased_row rewrites them."""
    from .io import _open_text
    if strings_by_contig is None:
        phased = {c: {int(s["pos"]): s for s in a if int(s["ps"]) >= 0} for c, a in assigned_by_contig.items()}
        rewrite = phasing.phased_row
    else:
        phased = {c: {phasing.row_pos(a, strings_by_contig[c], j): (strings_by_contig[c][j][0], strings_by_contig[c][j][1], int(s["ps"]), int(s["h1"]))
                      for j, s in enumerate(a) if int(s["ps"]) >= 0}
                  for c, a in assigned_by_contig.items()}
        rewrite = phasing.allele_phased_row
    plain = out_fn[:-3] if out_fn.endswith(".gz") else out_fn
    n, has_ps = 0, False
    with _open_text(in_vcf) as f, open(plain, "w") as out:
        for line in f:
            if line.startswith("#"):
                text, has_ps = phasing.header_row(line, has_ps)
                out.write(text)
                continue
            f_ = line.rstrip("\r\n").split("\t")
            table = phased.get(f_[0])
            if not table:
                out.write(line)
                continue
            text, done = rewrite(line, f_, table)
            out.write(text)
            n += int(done)
    if plain != out_fn:
        from . import sort_vcf
        sort_vcf.compress_vcf(plain)
    return n


def build_parser():
    p = argparse.ArgumentParser(description="Phase the heterozygous SNVs of the final VCF of a phased run from per-haplotype allele counts on MI355X, and report the counts")
    a = p.add_argument
    a("-b", "--bam_fn", type=str, required=True, help="the BAM (or flat read archive .npz) the VCF was called from")
    a("--vcf_fn", type=str, required=True, help="the VCF to phase (<prefix>_enable_phasing.vcf.gz), plain or gzipped")
    a("--phased_vcf_fn", type=str, required=True,
      help="what the 30-channel pass read: one phased VCF for all contigs, or a directory that holds phased_<ctg>.vcf.gz")
    a("-o", "--output_fn", type=str, required=True, help="the phased VCF, all contigs; a name that ends in .gz is bgzipped and tabix-indexed")
    a("--hap_counts_fn", type=str, default=None, help="receives one line of per-haplotype allele counts per candidate")
    a("-c", "--ctg_name", type=str, default=None, help="contigs to phase, comma-separated; default: every contig of the VCF (the others' rows are copied)")
    a("--min_mq", type=int, default=5, help="reads below it are not counted (the tensor build's filter)")
    a("--min_reads", type=int, default=2, help="fewest haplotype-tagged observations that phase a candidate")
    a("--min_agree_pct", type=int, default=75, help="fewest per cent of them that agree on the orientation")
    a("--indels", action="store_true",
      help="also phase heterozygous insertions, deletions and rows with two ALT alleles (GT 1/2), by CIGAR-position alleles: no realignment, no "
           "left-alignment (--left_align_indels lifts it), no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes); the counts file gets the column ALLELES.  Off: SNVs only, both files as they were")
    a("--haplotag_indels", action="store_true",
      help="tag the reads from the phased insertions, deletions and two-ALT rows of --phased_vcf_fn too, not from its biallelic SNVs alone "
           "(what the 30-channel pass did when it ran with this flag; include/c3r.h: c3r_set_phase_alleles)")
    a("--left_align_indels", action="store_true",
      help="with --indels: left-align the candidates' indels (and, with --haplotag_indels, the phase table's) against --ref_fn and every read's "
           "indel inside its M run, on the device (default: the alleles are read off the CIGAR position as they stand)")
    a("--ref_fn", type=str, default=None, help="the reference FASTA with its .fai: needed by --left_align_indels and --hap_realign only")
    phasing.add_hap_realign_flag(a)
    phasing.add_hap_bq_weights_flag(a, "the reads' tags — by which the counts are split — come from quality-weighted votes; the counts themselves stay counts of reads: ")
    a("--hap_min_bq", type=int, default=0, metavar="N",
      help="a base whose quality is below N does not vote: the steps that hold reads against a site table read it as N (include/c3r.h: c3r_set_hap_min_bq; 0 .. 93, default 0: off).  A threshold, not whatshap's quality weights (--hap_bq_weights are those); an indel's own quality is not modelled; reads without qualities are never masked; agreement with whatshap is not measured")
    a("--gpu_id", type=int, default=None, help="default: $C3R_DEVICE, else 0")
    return p


def Run(args, log=None):
    from . import capi, phasedvcf
    log = log or (lambda m: print(m, file=sys.stderr))
    for need in (args.bam_fn, args.vcf_fn):
        if not os.path.isfile(need):
            sys.exit("[ERROR] file %s not found" % need)
    from .phase_vcf import left_align_reference
    indels = bool(getattr(args, "indels", False))
    tag_indels = bool(getattr(args, "haplotag_indels", False))
    ref_of = left_align_reference(args, "--indels", indels or tag_indels)     # (or --haplotag_indels alone: then only the tags' table is left-aligned)
    realign, realign_ref = phasing.hap_realign_arg(args)
    source = phasedvcf.PhaseSource(args.phased_vcf_fn, tag_indels, *(() if ref_of is None or not tag_indels else (None, ref_of)), **(dict(realign=realign) if realign else {}))
    min_bq = phasing.hap_min_bq_arg(args, True, "")
    weights = phasing.hap_bq_weights_arg(args)
    if args.min_reads < 0 or not 0 <= args.min_agree_pct <= 100:
        sys.exit("[ERROR] --min_reads must be >= 0 and --min_agree_pct between 0 and 100")
    per = phasing.allele_candidates_from_vcf(args.vcf_fn, None, *(() if ref_of is None else (ref_of,))) if indels else phasing.candidates_from_vcf(args.vcf_fn, None)
    contigs = args.ctg_name.split(",") if args.ctg_name else list(per)
    gpu_id = args.gpu_id if args.gpu_id is not None else int(os.environ.get("C3R_DEVICE", "0"))
    eng = None
    assigned, strings, lines = {}, {}, ["\t".join(ALLELE_COLUMNS if indels else COLUMNS) + "\n"]
    try:
        for ctg in contigs:
            cands, skipped = (per[ctg][0], per[ctg][-1]) if ctg in per else (None, None)
            table = source.table(ctg)                         # (its pos / ps serve nearest_sets and the log, whatever its kind)
            note = source.indel_note(table, "[INFO] %s: --haplotag_indels: %d phased sites in the table, " % (ctg, len(table)))
            if note:
                log(note)
            if cands is None or not len(cands) or not len(table):
                log("[INFO] %s: %d phased sites in the table, %d heterozygous %s candidates: rows copied unchanged"
                    % (ctg, len(table), 0 if cands is None else len(cands), "SNV / indel / two-ALT" if indels else "SNV"))
                continue
            if eng is None:
                eng = capi.Engine(gpu_id)
                eng.set_params(min_mq=args.min_mq)
            query = nearest_sets(cands, table.sites)
            rs = io.load_reads(args.bam_fn, ctg, **(dict(want_quals=True) if min_bq or weights else {}))
            if ref_of is not None:                            # (the whole contig: it covers every read)
                eng.set_reference(*ref_of(ctg))
                eng.set_hap_left_align(True)
            if realign:
                phasing.apply_hap_realign(eng, realign, realign_ref(ctg), phasing.hap_realign_spliced_arg(args))
            source.apply(eng, table)
            phasing.load_reads_min_bq(eng, rs, min_bq, ctg, log, **(dict(weights=True) if weights else {}))
            if indels:
                counts = eng.hap_allele_counts(query, per[ctg][1])
                out, st = capi.hap_assign(capi.hap_site_keys(query), counts, args.min_reads, args.min_agree_pct)
                strings[ctg] = per[ctg][2]
                lines += allele_counts_lines(ctg, query, strings[ctg], out, counts)
            elif realign:                                     # (the SNV queries through the allele call: only the observation changes)
                counts = eng.hap_allele_counts(phasing.snv_sites_as_alleles(query)[0])
                out, st = capi.hap_assign(query, counts, args.min_reads, args.min_agree_pct)
                lines += counts_lines(ctg, query, out, counts)
            else:
                counts = eng.hap_counts(query)
                out, st = capi.hap_assign(query, counts, args.min_reads, args.min_agree_pct)
                lines += counts_lines(ctg, query, out, counts)
            assigned[ctg] = out
            log("[INFO] %s: %d reads, %d phased sites in %d sets, %d candidate sites%s (%s), %d phased, %d with too few tagged reads, %d without agreement -> %s"
                % (ctg, len(rs), len(table), len(set(table.ps.tolist())), st["n_sites"], phasing.left_align_note(skipped),
                   ", ".join("%s %d" % (k, v) for k, v in sorted(skipped.items()) if v and k != "other_contig") or "none skipped",
                   st["n_phased"], st["n_few_reads"], st["n_disagree"], args.output_fn))
    finally:
        if eng is not None:
            eng.close()
    n = write_vcf(args.vcf_fn, assigned, args.output_fn, strings if indels else None)
    if args.hap_counts_fn:
        with open(args.hap_counts_fn, "w") as f:
            f.writelines(lines)
    return n


def main(argv=None):
    Run(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
