"""Haplotype-resolved splice-junction counts — allele-specific splicing — from the tags the DEVICE computes, without the haplotagged BAM:
per junction that the reads of a contig hold, how many reads hold it and, per phase set, how many of them carry haplotype 1 and 2
(include/c3r.h: the rule `hap_junctions`, c3r_hap_junction_counts; csrc/hapjunction_kernels.hpp: k_hap_junction_counts).

Per contig of the BAM header (--ctg_name restricts them), what hap_expr does up to the tags — the phase table through
phasedvcf.PhaseSource -> the whole-contig fetch -> Engine.set_phase_sites / set_phase_alleles -> Engine.load_reads — and then
Engine.hap_junction_counts.  Unlike hap_expr, a contig without a phased site — and every contig when --phased_vcf_fn is not given — is
still loaded and counted: all its reads are untagged and its junctions have no rows, a plain junction counter.

Output: one TSV, tab-separated, `#CHROM START END MOTIF STRAND READS REVERSE PS HP1 HP2 UNTAGGED`, junctions by (START, END) within a
contig, 0-based half-open: the intron's first base and the base behind its last.  Per junction one summary line (PS HP1 HP2 = `.`), then
one line per phase set in which one of its reads was tagged, in PS order (READS REVERSE UNTAGGED = `.`); READS = UNTAGGED + the sum of
HP1 + HP2 over its lines.  --min_reads N drops the junctions with fewer than N reads, with their rows.  With --ref_fn, on the host only,
MOTIF is the intron's first two and last two reference bases, upper-cased (`GT-AG`; `.` where the contig's sequence does not cover them)
and STRAND is `+` for GT-AG, GC-AG, AT-AC, `-` for CT-AC, CT-GC, GT-AT and `.` otherwise; without --ref_fn both are `.`.
Written under a temporary name and renamed; an error leaves no file.  One [INFO] line per contig.

The counted reads are those the tensor build keeps (--min_mq, the default flag filter: no secondary, supplementary, duplicate or failed
alignments); a junction is an N op of the read's CIGAR, whatever lies beside it.  Not done: no minimum intron length or anchor length, no
annotation, no statistics (no test of imbalance); a read tagged in a set counts in that set's row even where the set has no site near
the junction; agreement with any external junction counter has not been measured.

The tagging flags are haplotag_bam's, through the same helpers: the tags are those of a pass that ran with them.

    python -m clair3_rna_amd.hap_junctions --bam_fn x.bam --phased_vcf_fn out/tmp/phased_output/phased_vcf --ref_fn ref.fa \\
        --output_fn out/hap_junctions.tsv
"""
import argparse
import os
import sys

HEADER = "#CHROM\tSTART\tEND\tMOTIF\tSTRAND\tREADS\tREVERSE\tPS\tHP1\tHP2\tUNTAGGED"
MOTIF_STRAND = {"GT-AG": "+", "GC-AG": "+", "AT-AC": "+", "CT-AC": "-", "CT-GC": "-", "GT-AT": "-"}


def motif(seq, start, end):
    """(MOTIF, STRAND) of the intron [start, end) on the contig's sequence `seq` (its first base is position 0; None: no reference)."""
    if seq is None or start < 0 or end < 2 or start + 2 > len(seq) or end > len(seq):
        return ".", "."
    first, last = seq[start:start + 2], seq[end - 2:end]
    if isinstance(first, bytes):                                  # (io.contig_reference hands the file's bytes)
        first, last = first.decode("ascii", "replace"), last.decode("ascii", "replace")
    m = (first + "-" + last).upper()
    return m, MOTIF_STRAND.get(m, ".")


def junction_lines(ctg, junctions, rows, seq=None, min_reads=1):
    """The TSV lines of one contig from Engine.hap_junction_counts' two arrays."""
    lines = []
    for j in range(len(junctions)):
        e = junctions[j]
        if int(e["reads"]) < min_reads:
            continue
        start, end = int(e["start"]), int(e["end"])
        head = [ctg, str(start), str(end)] + list(motif(seq, start, end))
        lines.append("\t".join(head + [str(int(e["reads"])), str(int(e["reverse"])), ".", ".", ".", str(int(e["untagged"]))]))
        top = int(junctions[j + 1]["row_off"]) if j + 1 < len(junctions) else len(rows)
        for r in range(int(e["row_off"]), top):
            lines.append("\t".join(head + [".", ".", str(int(rows[r]["ps"])), str(int(rows[r]["hp1"])), str(int(rows[r]["hp2"])), "."]))
    return lines


def build_parser():
    p = argparse.ArgumentParser(
        description="Reads per splice junction, haplotype and phase set (allele-specific splicing), counted on MI355X from the tags it computes from "
                    "the phased VCF; without one, a plain junction counter.  A junction is an N op of a read's CIGAR: no minimum intron length or "
                    "anchor length, no annotation, no statistics; agreement with any external junction counter has not been measured")
    a = p.add_argument
    a("-b", "--bam_fn", type=str, required=True, help="the BAM (coordinate-sorted; the one the phased VCF was made from)")
    a("-o", "--output_fn", type=str, required=True, help="the TSV")
    a("--phased_vcf_fn", type=str, default=None, help="one phased VCF for all contigs, or a directory that holds phased_<ctg>.vcf.gz; without it every read is untagged")
    a("-c", "--ctg_name", type=str, default=None, help="contigs, comma-separated; default: every contig of the BAM header")
    a("--min_mq", type=int, default=5, help="reads below this MAPQ are not counted (default 5)")
    a("--min_reads", type=int, default=1, metavar="N", help="write only the junctions that at least N counted reads hold (default 1)")
    a("--haplotag_indels", action="store_true", help="tag the reads from the phased insertions, deletions and two-ALT rows of --phased_vcf_fn too (include/c3r.h: c3r_set_phase_alleles)")
    a("--left_align_indels", action="store_true", help="with --haplotag_indels: left-align the table's indels against --ref_fn and every read's indel inside its own M run (include/c3r.h: c3r_set_hap_left_align)")
    a("--ref_fn", type=str, default=None, help="the reference FASTA with its .fai: fills MOTIF and STRAND (on the host), and is needed by --left_align_indels and --hap_realign")
    from . import phasing
    phasing.add_hap_realign_flag(a)
    a("--hap_min_bq", type=int, default=0, metavar="N", help="a base whose quality is below N does not vote for the read's tag (include/c3r.h: c3r_set_hap_min_bq; 0 .. 93, default 0: off)")
    phasing.add_hap_bq_weights_flag(a, "the tags of a 30-channel pass that ran with this flag: ")
    a("--gpu_id", type=int, default=None, help="default: $C3R_DEVICE, else 0")
    a("--threads", type=int, default=0, help="BGZF inflate threads; default: the CPUs this process may run on, 32 at the most")
    return p


def Run(args, log=None):
    """-> {contig: dict(junctions, written, rows, reads, sites)} of what was counted and written."""
    from . import bamio, capi, io, phasedvcf, phasing
    log = log or (lambda m: print(m, file=sys.stderr))
    if not os.path.isfile(args.bam_fn):
        sys.exit("[ERROR] file %s not found" % args.bam_fn)
    ref_fn = getattr(args, "ref_fn", None)
    if ref_fn and not os.path.isfile(ref_fn):
        sys.exit("[ERROR] file %s not found" % ref_fn)
    min_reads = int(getattr(args, "min_reads", 1))
    if min_reads < 1:
        sys.exit("[ERROR] --min_reads must be at least 1")
    phased = getattr(args, "phased_vcf_fn", None)
    tag_indels = bool(getattr(args, "haplotag_indels", False))
    for flag, on in (("--haplotag_indels", tag_indels), ("--hap_realign", bool(getattr(args, "hap_realign", 0))), ("--hap_min_bq", bool(getattr(args, "hap_min_bq", 0))),
                     ("--hap_bq_weights", bool(getattr(args, "hap_bq_weights", False)))):
        if on and not phased:
            sys.exit("[ERROR] %s needs --phased_vcf_fn (it changes how the reads are tagged from the phased VCF)" % flag)
    from .phase_vcf import left_align_reference
    ref_of = left_align_reference(args, "--haplotag_indels", tag_indels)
    realign, realign_ref = phasing.hap_realign_arg(args)
    source = phasedvcf.PhaseSource(phased, tag_indels, *(() if ref_of is None else (None, ref_of)), **(dict(realign=realign) if realign else {})) if phased else None
    min_bq = phasing.hap_min_bq_arg(args, True, "")
    weights = phasing.hap_bq_weights_arg(args)
    seq_of = io.contig_reference(ref_fn) if ref_fn else None
    threads = int(getattr(args, "threads", 0) or 0)
    gpu_id = args.gpu_id if args.gpu_id is not None else int(os.environ.get("C3R_DEVICE", "0"))
    wanted = args.ctg_name.split(",") if args.ctg_name else None
    out_dir = os.path.dirname(os.path.abspath(args.output_fn))
    os.makedirs(out_dir, exist_ok=True)
    tmp = args.output_fn + ".tmp"
    done, eng = {}, None
    try:
        with bamio.BamFile(args.bam_fn, threads=threads) as bf, open(tmp, "w") as f:
            f.write(HEADER + "\n")
            for ctg in [n for n, _l in bf.contigs()]:
                if wanted is not None and ctg not in wanted:
                    continue
                table = source.table(ctg) if source is not None else None
                rs = bf.fetch(ctg, **(dict(want_quals=True) if min_bq or weights else {}))
                lines, n_j, n_r = [], 0, 0
                if len(rs):
                    if eng is None:
                        eng = capi.Engine(gpu_id)
                        eng.set_params(min_mq=int(args.min_mq))
                    if ref_of is not None:
                        eng.set_reference(*ref_of(ctg))
                    if realign:
                        phasing.apply_hap_realign(eng, realign, realign_ref(ctg), phasing.hap_realign_spliced_arg(args))
                    if source is not None:
                        source.apply(eng, table)                   # (an empty table clears the previous contig's)
                    phasing.load_reads_min_bq(eng, rs, min_bq, ctg, log, **(dict(weights=True) if weights else {}))
                    junctions, rows = eng.hap_junction_counts()
                    n_j, n_r = len(junctions), len(rows)
                    lines = junction_lines(ctg, junctions, rows, seq_of(ctg)[1] if seq_of is not None and n_j else None, min_reads)
                if lines:
                    f.write("\n".join(lines) + "\n")
                n_sites = 0 if table is None else len(table)
                st = dict(junctions=n_j, written=sum(1 for l in lines if l.split("\t")[7] == "."), rows=n_r, reads=len(rs), sites=n_sites)
                done[ctg] = st
                log("[INFO] %s: %d junctions (%d with at least %d reads written), %d phase-set rows, %d reads, %d phased sites%s%s"
                    % (ctg, n_j, st["written"], min_reads, n_r, len(rs), n_sites, source.indel_note(table, " (--haplotag_indels: ", ")") if source is not None else "",
                       "" if n_sites else " (no phased site on this contig: every read is untagged)"))
        os.replace(tmp, args.output_fn)
    finally:
        if eng is not None:
            eng.close()
        if os.path.exists(tmp):
            os.remove(tmp)
    return done


def main(argv=None):
    Run(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
