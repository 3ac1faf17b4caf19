"""The haplotagged BAM of a phased run, one file per contig: what the reference flow's "Haplotag the BAM" step leaves under
tmp/phased_output/phased_bam (run_clair3_rna:769-801: `whatshap haplotag` / `longphase haplotag`, then `samtools index`), written with the
tags the DEVICE computes — the very tags the 30-channel pass calls with under --phased_vcf_fn — and without an external tool.

Per contig, exactly what the second pass does, except that the load is the whole contig so that every record gets its tag: the phase table
through phasedvcf.contig_sites -> the whole-contig fetch (io.load_reads(bam, ctg)) -> Engine.set_phase_sites -> Engine.load_reads -> Engine.haplotags() and
Engine.read_phase_sets() -> bamio.BamFile.write_haplotagged -> <output_dir>/<ctg>.bam -> bamio.index_build -> <ctg>.bam.bai.  Every record
of the contig is copied byte for byte, the ones the tensor build never sees (no CIGAR) included; old HP / PS / PC aux fields are removed from
all of them, and a read tagged 1 or 2 gets `HP:C:<tag>` and `PS` (its phase set, the smallest unsigned type) behind its other aux fields
(include/c3r_io.h: c3r_bam_write_haplotagged).  The header is the input's plus one @PG line (ID:c3r_haplotag, chained to the last @PG by PP).
A contig with no phased site gets its file too — every record untagged and stripped, nothing launched on the GPU for it, as call_var_bam's
"nothing phased on this contig: every read untagged".  Files are written under a temporary name and renamed: a failed contig leaves no
partial file.  One [INFO] line per contig.

Contigs: --ctg_name, else every contig of the BAM header; a contig without a record is not processed and gets no file.

The tag rule is the one of include/c3r.h (c3r_set_phase_sites): ALL loaded reads are tagged, whatever excl_flags / min_mq say (secondary and
supplementary alignments and MAPQ 0 included); every phased heterozygous SNV a read covers is one vote of unit weight for the haplotype
whose allele the read shows at the CIGAR position; the read's set is the one with the most votes.  No realignment, no base qualities
(`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes), no
indels, no tagging of a supplementary alignment after its primary.  Agreement with `whatshap haplotag` / `longphase haplotag` has not been
measured.  --haplotag_indels: the phased insertions, deletions and two-ALT rows of the phased VCF vote too (c3r_set_phase_alleles:
phasedvcf.contig_alleles -> Engine.set_phase_alleles), still as CIGAR-position alleles without left-alignment — unless --left_align_indels (with
--ref_fn) is given: then the table's indels are left-aligned against the reference and every read's indel inside its own M run, on the device
(include/c3r.h: c3r_set_hap_left_align); a shift stops at the run's start, at an N or another indel; still no realignment, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes).

    python -m clair3_rna_amd.haplotag_bam --bam_fn x.bam --phased_vcf_fn out/tmp/phased_output/phased_vcf \\
        --output_dir out/tmp/phased_output/phased_bam

--hap_realign [W] (default off; needs --ref_fn; excludes --left_align_indels): the reads are realigned against the two alleles of every site
before they vote (include/c3r.h: c3r_set_hap_realign), as in phase_vcf; without --haplotag_indels the SNV table goes through the allele call.
"""
import argparse
import os
import sys

import numpy as np

PG_ID = "c3r_haplotag"


def pg_line(header_text, version, command):
    """The @PG line (no newline) this step adds to a header (bytes or str): ID:c3r_haplotag, with .1, .2, ... appended while that ID exists;
    PN; VN; PP = the ID of the header's last @PG line when there is one; CL = the command (tabs and line ends become spaces)."""
    if isinstance(header_text, bytes):
        header_text = header_text.decode("utf-8", "replace")
    ids = []
    for line in header_text.rstrip("\x00").split("\n"):
        if line.startswith("@PG\t"):
            ids += [f[3:] for f in line.rstrip("\r").split("\t")[1:] if f.startswith("ID:")][:1]
    new, k = PG_ID, 0
    while new in ids:
        k += 1
        new = "%s.%d" % (PG_ID, k)
    fields = ["@PG", "ID:" + new, "PN:clair3_rna_amd", "VN:" + version.replace("\t", " ")]
    if ids:
        fields.append("PP:" + ids[-1])
    fields.append("CL:" + " ".join(command.split()))
    return "\t".join(fields)


def build_parser():
    p = argparse.ArgumentParser(
        description="Write the haplotagged BAM of a phased run (one indexed <ctg>.bam per contig) with the HP / PS tags MI355X computes from the phased "
                    "VCF: all loaded reads are tagged whatever their flags or MAPQ, unit-weight votes of CIGAR-position alleles at phased "
                    "heterozygous SNVs, no realignment, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes).  Agreement with whatshap / longphase haplotag has not been measured")
    a = p.add_argument
    a("-b", "--bam_fn", type=str, required=True, help="the BAM the phased VCF was made from (coordinate-sorted; an index beside it keeps every contig's pass short)")
    a("--phased_vcf_fn", type=str, required=True,
      help="what the 30-channel pass read: one phased VCF for all contigs, or a directory that holds phased_<ctg>.vcf.gz")
    a("-o", "--output_dir", type=str, required=True, help="receives <ctg>.bam and <ctg>.bam.bai")
    a("-c", "--ctg_name", type=str, default=None, help="contigs, comma-separated; default: every contig of the BAM header.  A contig without a record gets no file")
    a("--haplotag_indels", action="store_true",
      help="tag the reads from the phased insertions, deletions and two-ALT rows of --phased_vcf_fn too, not from its biallelic SNVs alone "
           "(include/c3r.h: c3r_set_phase_alleles): the tags of a 30-channel pass that ran with this flag")
    a("--left_align_indels", action="store_true",
      help="with --haplotag_indels: left-align the table's indels against --ref_fn and every read's indel inside its own M run, on the device "
           "(include/c3r.h: c3r_set_hap_left_align): the tags of a 30-channel pass that ran with this flag.  A shift stops at the M run's "
           "start, at an N or another indel; no realignment, no base qualities (`--hap_min_bq` lifts it as a threshold, `--hap_bq_weights` as weights of the haplotag votes); agreement with whatshap is not measured")
    a("--ref_fn", type=str, default=None, help="the reference FASTA with its .fai: needed by --left_align_indels and --hap_realign only")
    from . import phasing
    phasing.add_hap_realign_flag(a)
    a("--hap_min_bq", type=int, default=0, metavar="N",
      help="a base whose quality is below N does not vote: the steps that hold reads against a site table read it as N (include/c3r.h: c3r_set_hap_min_bq; 0 .. 93, default 0: off).  A threshold, not whatshap's quality weights (--hap_bq_weights are those); an indel's own quality is not modelled; reads without qualities are never masked; agreement with whatshap is not measured")
    phasing.add_hap_bq_weights_flag(a, "the tags of a 30-channel pass that ran with this flag, and PC (the difference of the two haplotypes' weight sums, "
                                       "in the smallest unsigned type) behind PS of every tagged record: ")
    a("--gpu_id", type=int, default=None, help="default: $C3R_DEVICE, else 0")
    a("--threads", type=int, default=0, help="BGZF inflate / deflate threads; default: the CPUs this process may run on, 32 at the most")
    return p


def _version():
    from . import capi
    return capi.load_library().c3r_version().decode()


def Run(args, log=None):
    """-> {contig: dict(records, tagged, stripped, unpaired, hp1, hp2, path)} of the files written."""
    from . import bamio, capi, phasedvcf, phasing
    log = log or (lambda m: print(m, file=sys.stderr))
    if not os.path.isfile(args.bam_fn):
        sys.exit("[ERROR] file %s not found" % args.bam_fn)
    from .phase_vcf import left_align_reference
    tag_indels = bool(getattr(args, "haplotag_indels", False))
    ref_of = left_align_reference(args, "--haplotag_indels", tag_indels)
    realign, realign_ref = phasing.hap_realign_arg(args)
    source = phasedvcf.PhaseSource(args.phased_vcf_fn, tag_indels, *(() if ref_of is None else (None, ref_of)), **(dict(realign=realign) if realign else {}))
    min_bq = phasing.hap_min_bq_arg(args, True, "")
    weights = phasing.hap_bq_weights_arg(args)
    threads = int(getattr(args, "threads", 0) or 0)
    command = getattr(args, "command", None) or " ".join(sys.argv)
    os.makedirs(args.output_dir, exist_ok=True)
    gpu_id = args.gpu_id if args.gpu_id is not None else int(os.environ.get("C3R_DEVICE", "0"))
    done, eng = {}, None
    with bamio.BamFile(args.bam_fn, threads=threads) as bf:
        in_bam = [n for n, _l in bf.contigs()]
        line = pg_line(bf.header_text(), _version(), command)
        try:
            for ctg in (args.ctg_name.split(",") if args.ctg_name else in_bam):
                if ctg not in in_bam:
                    log("[INFO] %s: not in the header of %s: no file" % (ctg, args.bam_fn))
                    continue
                table = source.table(ctg)
                rs = hp = ps = pc = None
                if len(table):
                    rs = bf.fetch(ctg, **(dict(want_quals=True) if min_bq or weights else {}))                             # io.load_reads(bam, ctg) on the handle that is open already (--threads)
                if rs is not None and len(rs):
                    if eng is None:
                        eng = capi.Engine(gpu_id)
                        eng.set_params()
                    if ref_of is not None:                         # (the whole contig: it covers every read)
                        eng.set_reference(*ref_of(ctg))
                    if realign:
                        phasing.apply_hap_realign(eng, realign, realign_ref(ctg), phasing.hap_realign_spliced_arg(args))
                    source.apply(eng, table)
                    phasing.load_reads_min_bq(eng, rs, min_bq, ctg, log, **(dict(weights=True) if weights else {}))
                    hp, ps = eng.haplotags()[0], eng.read_phase_sets()
                    if weights:                                    # (PC: |w1 - w2| of the set the tag was decided in)
                        w = eng.haplotag_weights().astype(np.int64)
                        pc = np.abs(w[:, 0] - w[:, 1]).astype(np.uint32)
                elif rs is not None:                               # (no read record: nothing to launch; the contig's other records still go out)
                    hp, ps = np.zeros(0, np.uint8), np.zeros(0, np.int32)
                    pc = np.zeros(0, np.uint32) if weights else None
                out = os.path.join(args.output_dir, ctg + ".bam")
                tmp, tmp_bai = out + ".tmp", out + ".bai.tmp"
                try:
                    st = bf.write_haplotagged(ctg, tmp, rs, hp, ps, pg_line=line, threads=threads, **(dict(pc=pc) if pc is not None else {}))
                    if st["records"] == 0:                         # (header + EOF: through an index that costs nothing)
                        os.remove(tmp)
                        log("[INFO] %s: no record in %s: no file" % (ctg, args.bam_fn))
                        continue
                    bamio.index_build(tmp, tmp_bai)
                    os.replace(tmp, out)
                    os.replace(tmp_bai, out + ".bai")
                finally:
                    for leftover in (tmp, tmp_bai):
                        if os.path.exists(leftover):
                            os.remove(leftover)
                st["hp1"], st["hp2"] = (int((hp == 1).sum()), int((hp == 2).sum())) if hp is not None else (0, 0)
                st["path"] = out
                done[ctg] = st
                log("[INFO] %s: %d records, %d HP1, %d HP2, %d untagged, %d unpaired (not read records: copied, never tagged), %d phased sites%s -> %s"
                    % (ctg, st["records"], st["hp1"], st["hp2"], st["records"] - st["tagged"] - st["unpaired"], st["unpaired"], len(table),
                       source.indel_note(table, " (--haplotag_indels: ", ")")
                       + ("" if len(table) else " (nothing phased on this contig: every read untagged)"), out))
        finally:
            if eng is not None:
                eng.close()
    return done


def main(argv=None):
    Run(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
