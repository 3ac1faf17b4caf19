"""Haplotype-resolved read counts per BED interval — allele-specific expression — from the tags the DEVICE computes, without the haplotagged
BAM: how many reads of haplotype 1 and 2, per phase set, overlap each exon or gene of a BED file (include/c3r.h: the rule `hap_regions`,
c3r_hap_region_counts; csrc/hapregion_kernels.hpp: k_hap_region_counts).

Per contig of the BED that is in the BAM header (contigs in the header's order, --ctg_name restricts them), what haplotag_bam does up to the
tags — the phase table through phasedvcf.PhaseSource -> the whole-contig fetch -> Engine.set_phase_sites / set_phase_alleles ->
Engine.load_reads — and then Engine.hap_region_counts on the contig's intervals.  A region's rows are the distinct phase sets of the table's
sites with start < pos <= end (the sites inside the interval), so a gene that two phase sets cross gets a line for each.

Output: one TSV, tab-separated, `#CHROM START END NAME STRAND PS HP1 HP2 UNTAGGED OTHER_SET`, regions in BED order within a contig.  Per
region one summary line (PS HP1 HP2 = `.`; UNTAGGED: kept reads over the region without a tag; OTHER_SET: reads tagged in a phase set that
has no site inside the region), then one line per row in ps order (PS HP1 HP2 filled; UNTAGGED and OTHER_SET = `.`).  A contig without a
phased site or without a read launches nothing: its regions get their summary lines with UNTAGGED and OTHER_SET = `.` (not counted — not 0).
Written under a temporary name and renamed; an error leaves no file.  One [INFO] line per contig.

The counted reads are those the tensor build keeps (--min_mq, the default flag filter: no secondary, supplementary, duplicate or failed
alignments), each once in EVERY region that one of its M / = / X / D ops overlaps — introns do not count.  --stranded same / reverse counts
a read only in regions of its own / the opposite strand (BED column 6; a region without a strand always counts).  Not done: no union over a
gene's exon lines unless --group_by_name asks for it (below; without it a read over two exons of one gene counts in both), no fractional
assignment, no statistics; agreement with featureCounts / htseq-count has not been measured.  A table in which one region lies over more than 4096 later ones
(C3R_HAP_REGION_MAX_BACK) is counted in two calls, long and short regions apart, when that brings both under the bound, else refused.

--group_by_name: the gene-level count (include/c3r.h: the rule `hap_groups`, c3r_hap_group_counts; csrc/hapgroup_kernels.hpp).  Per contig,
the BED lines with the same column 4 are one group (a line named `.` is a group of its own); a group's intervals are sorted and overlapping or
abutting ones merged; its strand is the lines' if they all agree, else none (one [WARNING] line per contig counts such groups); its rows are
the distinct phase sets of the sites inside any merged interval.  A read counts ONCE per group of which it covers a position of an interval,
and a read that lies only in a gene's introns is not in the gene.  Header `#CHROM START END NAME STRAND INTERVALS LENGTH PS HP1 HP2 UNTAGGED
OTHER_SET`: START / END the group's span, INTERVALS / LENGTH the number and the summed length of its merged intervals; groups in order of
first appearance; summary and row lines as above.  No GTF reader: the names come from BED column 4.

The tagging flags are haplotag_bam's, through the same helpers: the tags are those of a pass that ran with them.

    python -m clair3_rna_amd.hap_expr --bam_fn x.bam --phased_vcf_fn out/tmp/phased_output/phased_vcf --regions_bed_fn exons.bed \\
        --output_fn out/hap_expression.tsv
"""
import argparse
import os
import sys

import numpy as np

HEADER = "#CHROM\tSTART\tEND\tNAME\tSTRAND\tPS\tHP1\tHP2\tUNTAGGED\tOTHER_SET"
GROUP_HEADER = "#CHROM\tSTART\tEND\tNAME\tSTRAND\tINTERVALS\tLENGTH\tPS\tHP1\tHP2\tUNTAGGED\tOTHER_SET"
STRANDED = {"no": 0, "same": 1, "reverse": 2}
STRAND_CODE = {None: 0, "+": 1, "-": 2}


def add_stranded_flag(add, name="--stranded"):
    add(name, type=str, choices=sorted(STRANDED), default="no",
        help="count a read only in regions of its own strand (same) or of the opposite strand (reverse), by BED column 6; a region without a "
             "strand always counts (default: no)")


def bed_contigs(bed_fn):
    """The contig names of a BED file, in order of first appearance."""
    from .io import _open_text
    seen = []
    with _open_text(bed_fn) as f:
        for row in f:
            if not row.strip() or row[0] == "#" or row.startswith(("track", "browser")):
                continue
            c = row.split(None, 1)[0]
            if c not in seen:
                seen.append(c)
    return seen


def region_table(regions, pos, ps):
    """[(start, end, name, strand)] in any order and the phase table's pos (1-based, sorted) / ps -> (HAP_REGION_DTYPE array sorted by (start,
    end), int32 row_ps, order) with order[k] = the index in `regions` of table entry k.  A region's rows: the distinct ps of the sites with
    start < pos <= end, increasing."""
    from .capi import HAP_REGION_DTYPE
    order = sorted(range(len(regions)), key=lambda j: (regions[j][0], regions[j][1]))
    tab = np.zeros(len(order), dtype=HAP_REGION_DTYPE)
    pos, ps = np.asarray(pos, dtype=np.int64), np.asarray(ps, dtype=np.int64)
    rows = []
    for k, j in enumerate(order):
        start, end, _name, strand = regions[j]
        mine = np.unique(ps[np.searchsorted(pos, start, "right"):np.searchsorted(pos, end, "right")])
        tab[k]["start"], tab[k]["end"], tab[k]["row_off"], tab[k]["strand"] = start, end, len(rows), STRAND_CODE[strand]
        rows += mine.tolist()
    return tab, np.array(rows, dtype=np.int32).reshape(len(rows)), order


def max_back(tab):
    """max_j (j - first_open[j]) of a sorted table: first_open[j] is the smallest i <= j with end_i > start_j (include/c3r.h)."""
    f, worst = 0, 0
    start, end = tab["start"].tolist(), tab["end"].tolist()
    for j in range(len(start)):
        while f < j and end[f] <= start[j]:
            f += 1
        worst = max(worst, j - f)
    return worst


def count_regions(eng, regions, pos, ps, stranded=0):
    """Engine.hap_region_counts for BED-order regions -> per region ((untagged, other_set), [(ps, hp1, hp2)]).  A table over
    capi.HAP_REGION_MAX_BACK goes up in two calls, the regions longer than the median length apart from the others, when both halves are
    under the bound; else in one, which the library refuses with its message."""
    from .capi import HAP_REGION_MAX_BACK
    out = [None] * len(regions)
    parts = [list(range(len(regions)))]
    if max_back(region_table(regions, pos, ps)[0]) > HAP_REGION_MAX_BACK:
        median = sorted(r[1] - r[0] for r in regions)[len(regions) // 2]
        halves = [[j for j in parts[0] if regions[j][1] - regions[j][0] <= median], [j for j in parts[0] if regions[j][1] - regions[j][0] > median]]
        if all(h and max_back(region_table([regions[j] for j in h], pos, ps)[0]) <= HAP_REGION_MAX_BACK for h in halves):
            parts = halves
    for part in parts:
        tab, row_ps, order = region_table([regions[j] for j in part], pos, ps)
        rc, wc = eng.hap_region_counts(tab, row_ps, stranded)
        for k, o in enumerate(order):
            lo = int(tab[k]["row_off"])
            top = int(tab[k + 1]["row_off"]) if k + 1 < len(tab) else len(row_ps)
            out[part[o]] = ((int(rc[k, 0]), int(rc[k, 1])), [(int(row_ps[r]), int(wc[r, 0]), int(wc[r, 1])) for r in range(lo, top)])
    return out


def count_lines(heads, counted):
    """The TSV lines of one contig from every owner's leading columns: per owner its summary line, then a line per row.  counted: the list
    of count_regions or count_groups, or None when nothing was launched."""
    lines = []
    for j, head in enumerate(heads):
        (untagged, other), rows = counted[j] if counted is not None else ((".", "."), [])
        lines.append("\t".join(head + [".", ".", ".", str(untagged), str(other)]))
        for ps, h1, h2 in rows:
            lines.append("\t".join(head + [str(ps), str(h1), str(h2), ".", "."]))
    return lines


def region_lines(ctg, regions, counted):
    """The TSV lines of one contig; counted: count_regions' list, or None when nothing was launched."""
    return count_lines([[ctg, str(start), str(end), name, strand or "."] for start, end, name, strand in regions], counted)


def group_by_name(regions):
    """BED lines [(start, end, name, strand)] -> ([(name, strand, [(start, end)])], n_mixed): the lines with one name are one group, a line
    named `.` a group of its own, in order of first appearance; a group's intervals sorted, overlapping and abutting ones merged; strand:
    the lines' if they all agree, else None — n_mixed counts those groups."""
    groups, at = [], {}
    for start, end, name, strand in regions:
        g = at.get(name) if name != "." else None
        if g is None:
            g = len(groups)
            groups.append((name, [], []))
            if name != ".":
                at[name] = g
        groups[g][1].append(strand)
        groups[g][2].append((start, end))
    out, n_mixed = [], 0
    for name, strands, ivs in groups:
        merged = []
        for start, end in sorted(ivs):
            if merged and start <= merged[-1][1]:
                merged[-1] = (merged[-1][0], max(merged[-1][1], end))
            else:
                merged.append((start, end))
        mixed = any(x != strands[0] for x in strands)
        n_mixed += mixed
        out.append((name, None if mixed else strands[0], merged))
    return out, n_mixed


def group_table(groups, pos, ps):
    """group_by_name's groups and the phase table's pos (1-based, sorted) / ps -> (HAP_INTERVAL_DTYPE array sorted by (start, end), int32
    group_row_off, int32 row_ps).  A group's rows: the distinct ps of the sites with start < pos <= end for one of its intervals, increasing."""
    from .capi import HAP_INTERVAL_DTYPE
    pos, ps = np.asarray(pos, dtype=np.int64), np.asarray(ps, dtype=np.int64)
    ivs = sorted((start, end, g, STRAND_CODE[strand]) for g, (_name, strand, merged) in enumerate(groups) for start, end in merged)
    tab = np.zeros(len(ivs), dtype=HAP_INTERVAL_DTYPE)
    for k, (start, end, g, strand) in enumerate(ivs):
        tab[k]["start"], tab[k]["end"], tab[k]["group"], tab[k]["strand"] = start, end, g, strand
    off, rows = [], []
    for _name, _strand, merged in groups:
        off.append(len(rows))
        inside = [ps[np.searchsorted(pos, start, "right"):np.searchsorted(pos, end, "right")] for start, end in merged]
        rows += np.unique(np.concatenate(inside)).tolist()
    return tab, np.array(off, dtype=np.int32).reshape(len(off)), np.array(rows, dtype=np.int32).reshape(len(rows))


def count_groups(eng, groups, pos, ps, stranded=0):
    """Engine.hap_group_counts for group_by_name's groups -> per group ((untagged, other_set), [(ps, hp1, hp2)])."""
    tab, off, row_ps = group_table(groups, pos, ps)
    gc, wc = eng.hap_group_counts(tab, len(groups), off, row_ps, stranded)
    tops = off.tolist()[1:] + [len(row_ps)]
    return [((int(gc[g, 0]), int(gc[g, 1])), [(int(row_ps[r]), int(wc[r, 0]), int(wc[r, 1])) for r in range(int(off[g]), tops[g])]) for g in range(len(groups))]


def group_lines(ctg, groups, counted):
    """The TSV lines of one contig under --group_by_name; counted: count_groups' list, or None when nothing was launched."""
    return count_lines([[ctg, str(merged[0][0]), str(merged[-1][1]), name, strand or ".", str(len(merged)), str(sum(end - start for start, end in merged))]
                        for name, strand, merged in groups], counted)


def build_parser():
    p = argparse.ArgumentParser(
        description="Reads per haplotype and phase set over every interval of a BED file (allele-specific expression), counted on MI355X from the "
                    "tags it computes from the phased VCF.  A read counts once in every region one of its aligned or deleted stretches overlaps; no "
                    "gene-level union of exon lines, no fractional assignment, no statistics; agreement with featureCounts / htseq-count has not been measured")
    a = p.add_argument
    a("-b", "--bam_fn", type=str, required=True, help="the BAM the phased VCF was made from (coordinate-sorted)")
    a("--phased_vcf_fn", type=str, required=True, help="one phased VCF for all contigs, or a directory that holds phased_<ctg>.vcf.gz")
    a("--regions_bed_fn", type=str, required=True, help="BED: contig, start, end, and optionally name (column 4) and strand (column 6).  Lines with end <= start are skipped")
    a("-o", "--output_fn", type=str, required=True, help="the TSV")
    a("-c", "--ctg_name", type=str, default=None, help="contigs, comma-separated; default: every contig of the BED that the BAM header holds")
    a("--min_mq", type=int, default=5, help="reads below this MAPQ are not counted (default 5)")
    add_stranded_flag(a)
    a("--group_by_name", action="store_true",
      help="the gene-level count: per contig the BED lines with the same name (column 4; `.` names nothing) are one group, its overlapping or "
           "abutting intervals merged, and a read counts once per group it overlaps, however many of the group's intervals (include/c3r.h: "
           "c3r_hap_group_counts).  The TSV gets the columns INTERVALS and LENGTH.  No GTF reader, no fractional assignment, no statistics")
    a("--haplotag_indels", action="store_true", help="tag the reads from the phased insertions, deletions and two-ALT rows of --phased_vcf_fn too (include/c3r.h: c3r_set_phase_alleles)")
    a("--left_align_indels", action="store_true", help="with --haplotag_indels: left-align the table's indels against --ref_fn and every read's indel inside its own M run (include/c3r.h: c3r_set_hap_left_align)")
    a("--ref_fn", type=str, default=None, help="the reference FASTA with its .fai: needed by --left_align_indels and --hap_realign only")
    from . import phasing
    phasing.add_hap_realign_flag(a)
    a("--hap_min_bq", type=int, default=0, metavar="N", help="a base whose quality is below N does not vote for the read's tag (include/c3r.h: c3r_set_hap_min_bq; 0 .. 93, default 0: off)")
    phasing.add_hap_bq_weights_flag(a, "the tags of a 30-channel pass that ran with this flag: ")
    a("--gpu_id", type=int, default=None, help="default: $C3R_DEVICE, else 0")
    a("--threads", type=int, default=0, help="BGZF inflate threads; default: the CPUs this process may run on, 32 at the most")
    return p


def Run(args, log=None):
    """-> {contig: dict(regions, skipped, rows, reads, launched)} of what was written."""
    from . import bamio, capi, io, phasedvcf, phasing
    log = log or (lambda m: print(m, file=sys.stderr))
    for fn in (args.bam_fn, args.regions_bed_fn):
        if not os.path.isfile(fn):
            sys.exit("[ERROR] file %s not found" % fn)
    from .phase_vcf import left_align_reference
    tag_indels = bool(getattr(args, "haplotag_indels", False))
    ref_of = left_align_reference(args, "--haplotag_indels", tag_indels)
    realign, realign_ref = phasing.hap_realign_arg(args)
    source = phasedvcf.PhaseSource(args.phased_vcf_fn, tag_indels, *(() if ref_of is None else (None, ref_of)), **(dict(realign=realign) if realign else {}))
    min_bq = phasing.hap_min_bq_arg(args, True, "")
    weights = phasing.hap_bq_weights_arg(args)
    stranded = STRANDED[getattr(args, "stranded", "no") or "no"]
    by_name = bool(getattr(args, "group_by_name", False))
    threads = int(getattr(args, "threads", 0) or 0)
    gpu_id = args.gpu_id if args.gpu_id is not None else int(os.environ.get("C3R_DEVICE", "0"))
    in_bed = bed_contigs(args.regions_bed_fn)
    wanted = args.ctg_name.split(",") if args.ctg_name else None
    out_dir = os.path.dirname(os.path.abspath(args.output_fn))
    os.makedirs(out_dir, exist_ok=True)
    tmp = args.output_fn + ".tmp"
    done, eng = {}, None
    try:
        with bamio.BamFile(args.bam_fn, threads=threads) as bf, open(tmp, "w") as f:
            f.write((GROUP_HEADER if by_name else HEADER) + "\n")
            for ctg in [n for n, _l in bf.contigs()]:
                if ctg not in in_bed or (wanted is not None and ctg not in wanted):
                    continue
                regions = io.read_bed_regions(args.regions_bed_fn, ctg)
                if by_name:
                    groups, n_mixed = group_by_name(regions)
                    if n_mixed:
                        log("[WARNING] %s: %d groups have BED lines of more than one strand: they are counted without a strand" % (ctg, n_mixed))
                table = source.table(ctg)
                rs = bf.fetch(ctg, **(dict(want_quals=True) if min_bq or weights else {})) if len(table) and len(regions) else None
                counted = None
                if rs is not None and len(rs):
                    if eng is None:
                        eng = capi.Engine(gpu_id)
                        eng.set_params(min_mq=int(args.min_mq))
                    if ref_of is not None:
                        eng.set_reference(*ref_of(ctg))
                    if realign:
                        phasing.apply_hap_realign(eng, realign, realign_ref(ctg), phasing.hap_realign_spliced_arg(args))
                    source.apply(eng, table)
                    phasing.load_reads_min_bq(eng, rs, min_bq, ctg, log, **(dict(weights=True) if weights else {}))
                    counted = count_groups(eng, groups, table.pos, table.ps, stranded) if by_name else count_regions(eng, regions, table.pos, table.ps, stranded)
                lines = group_lines(ctg, groups, counted) if by_name else region_lines(ctg, regions, counted)
                if lines:
                    f.write("\n".join(lines) + "\n")
                st = dict(regions=len(regions), skipped=regions.n_skipped, rows=len(lines) - (len(groups) if by_name else len(regions)), reads=0 if rs is None else len(rs), launched=counted is not None)
                if by_name:
                    st["groups"] = len(groups)
                done[ctg] = st
                log("[INFO] %s: %s%d regions (%d BED lines with end <= start skipped), %d phase-set rows, %d reads, %d phased sites%s%s"
                    % (ctg, "%d groups of " % len(groups) if by_name else "", st["regions"], st["skipped"], st["rows"], st["reads"], len(table), source.indel_note(table, " (--haplotag_indels: ", ")"),
                       "" if counted is not None else " (no phased site or no read on this contig: nothing counted, UNTAGGED and OTHER_SET are `.`)"))
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
