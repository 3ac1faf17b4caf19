#!/usr/bin/env python3
"""Pin the "parity unpinned" halves against the third-party tools themselves, the day they exist beside this repository
(neither samtools nor TensorFlow nor whatshap is in the build image).

  python tools/pin_third_party.py --samtools /path/to/samtools            # A1: reads -> mpileup text
  python tools/pin_third_party.py --tf --reference_repo /path/to/Clair3-RNA   # F5: a TensorFlow-written checkpoint through tfckpt.py
  python tools/pin_third_party.py --whatshap /path/to/whatshap            # K0: haplotags against `whatshap haplotag`  (NEVER RUN: no whatshap on any machine so far)

A1.  Every known-answer case of tests/test_oracle_mpileup.py (harvested by running those tests with a recording `pile`), plus the depth-cap
     case (8000 / 8001 reads starting on one position, `-d 8000`), is written as SAM + FASTA, turned into an indexed BAM by the given
     samtools, and piled up with the reference's own flag set (src/create_tensor_pileup.py:436-451: `mpileup <bam> -r <region> --reverse-del
     --min-MQ 5 --min-BQ 0 --excl-flags 2316 [--max-depth N] [--output-extra HP]`).  Columns (position, depth, bases[, HP]) are compared with
     orc_mpileup's in the printer that samtools version calls for (clair3_rna_amd/mpileup_compat.py).  A mismatch prints both columns; the
     one-constant switches for the depth cap are PLP_POOL_EXTRA (csrc/c3r_lib.hip) and ORC_PLP_POOL_EXTRA (oracle/c3r_oracle.c).
F5.  Builds the reference's Keras model (clair3_rna/model.py) for 18 and 30 channels, save_weights() into a temporary directory, reads the
     bundle with clair3_rna_amd/tfckpt.py and compares every tensor with model.get_weights() bit for bit
     (clair3_rna/call_variants.py:1472 is where the reference loads such a bundle).
K0.  NEVER RUN.  The random two-haplotype read sets of tests/hapref.py (gen_case, seeds 0-2) are written as an indexed BAM (bam.write_bam,
     reads named r1, r2, ... in load order) with a FASTA and a phased VCF, `whatshap haplotag --output-haplotag-list` tags them, and the list is
     compared with our tags (the GPU's when a device is there, else tests/hapref.py, which the GPU tests hold equal to it).  The two rules
     are NOT the same — whatshap realigns reads around each variant and weights votes by base quality; ours reads the allele off the CIGAR
     position with unit weights (include/c3r.h) — so this leg REPORTS agreement (reads tagged alike / differently / by one side only) and
     fails only when fewer than 95 % of the reads both sides tag carry the same haplotype.  That figure is a guess until the leg has run.
     A second leg, also NEVER RUN: the built-in phasing (c3r_phase_links / c3r_phase_resolve — a greedy linkage chain, not whatshap's wMEC)
     against `whatshap phase` on tests/phaseref.py's generated cases with ONT-like errors (seeds 1, 3, 5): both phase the same unphased VCF
     from the same BAM, and `whatshap compare` prints switch errors, flips and block statistics between the two phased VCFs.  This leg
     only REPORTS (whatshap's table goes to stdout): what agreement to ask for is unknown until it has run.
Exit status 0: everything agreed."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def harvest_cases():
    """(records, beg, end, kwargs) of every pile() call the known-answer tests make."""
    import tests.test_oracle_mpileup as T
    cases, orig = [], T.pile

    def pile(records, beg=1, end=60, **kw):
        cases.append(([dict(r) for r in records], beg, end, dict(kw)))
        return orig(records, beg, end, **kw)
    T.pile = pile
    try:
        for name in sorted(dir(T)):
            if name.startswith("test_"):
                try:
                    getattr(T, name)()
                except Exception:          # noqa: BLE001 (only the inputs are wanted here)
                    pass
    finally:
        T.pile = orig
    return cases


def cap_cases():
    seq = "ACGTACGTAC" * 6
    out = []
    for n in (8000, 8001):
        recs = [dict(pos=9, cigar="60M", seq=seq, flag=16 * (i % 2), mapq=60, hp=0) for i in range(n)]
        recs += [dict(pos=20, cigar="40M", seq=seq[11:51], flag=0, mapq=60, hp=0) for _ in range(5)]
        out.append((recs, 1, 80, dict(max_depth=8000)))
    return out


def write_sam(path, records, ref_len, with_hp):
    with open(path, "w") as f:
        f.write("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:%d\n" % ref_len)
        for i, r in enumerate(sorted(records, key=lambda r: r["pos"])):
            seq = r["seq"]
            tags = "\tHP:i:%d" % r["hp"] if (with_hp and r.get("hp")) else ""
            f.write("r%d\t%d\tc\t%d\t%d\t%s\t*\t0\t0\t%s\t%s%s\n" % (i, r.get("flag", 0), r["pos"] + 1, r.get("mapq", 60), r["cigar"], seq, "I" * len(seq), tags))


def run_samtools_case(samtools, compat, case, tmp):
    from clair3_rna_amd.reads import ReadSet
    from oracle import oracle as orc
    records, beg, end, kw = case
    with_hp = bool(kw.get("with_hp"))
    ref_len = max(end + 100, max(r["pos"] for r in records) + 5000)
    sam, bam, fa = os.path.join(tmp, "x.sam"), os.path.join(tmp, "x.bam"), os.path.join(tmp, "x.fa")
    write_sam(sam, records, ref_len, with_hp)
    with open(fa, "w") as f:
        f.write(">c\n" + "N" * ref_len + "\n")
    subprocess.check_call([samtools, "view", "-b", "-o", bam, sam])
    subprocess.check_call([samtools, "index", bam])
    cmd = [samtools, "mpileup", bam, "-r", "c:%d-%d" % (beg, end), "--reverse-del", "--min-MQ", str(kw.get("min_mq", 5)), "--min-BQ", "0",
           "--excl-flags", str(kw.get("excl_flags", 2316))]
    if "max_depth" in kw:
        cmd += ["--max-depth", str(kw["max_depth"])]
    if with_hp:
        cmd += ["--output-extra", "HP"]
    got = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, check=True).stdout.rstrip("\n").split("\n")
    rs = ReadSet.from_records(records)
    okw = {k: v for k, v in kw.items() if k in ("min_mq", "excl_flags", "with_hp", "max_depth")}
    exp = orc.mpileup(rs.reads, rs.cigar, rs.seq, "c", beg, end, compat=compat, **okw)

    def cols(rows):
        out = {}
        for row in rows:
            f = row.split("\t")
            if len(f) >= 5:
                out[int(f[1])] = (f[3], f[4]) + ((f[6],) if with_hp and len(f) > 6 else ())
        return out
    g, e = cols(got), cols(exp)
    bad = [(p, g.get(p), e.get(p)) for p in sorted(set(g) | set(e)) if g.get(p) != e.get(p)]
    return bad


def pin_samtools(samtools):
    from clair3_rna_amd import mpileup_compat
    compat = mpileup_compat.resolve("auto", samtools)
    ver = subprocess.run([samtools, "--version"], stdout=subprocess.PIPE, text=True).stdout.split("\n")[0]
    print("%s -> printer %d" % (ver, compat))
    cases = harvest_cases() + cap_cases()
    n_bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for k, case in enumerate(cases):
            bad = run_samtools_case(samtools, compat, case, tmp)
            if bad:
                n_bad += 1
                print("case %d (%d reads, %s): %d columns differ" % (k, len(case[0]), case[3], len(bad)))
                for p, g, e in bad[:6]:
                    print("   pos %d  samtools %r  oracle %r" % (p, g, e))
    print("A1: %d cases, %d differ" % (len(cases), n_bad))
    return n_bad == 0


def pin_tf(reference_repo):
    import numpy as np
    sys.path.insert(0, reference_repo)
    import tensorflow as tf  # noqa: F401
    from clair3_rna import model as ref_model
    from clair3_rna_amd import tfckpt
    ok = True
    for channels in (18, 30):
        try:
            m = ref_model.Clair3_P(add_indel_length=False, predict=True)      # (clair3_rna/call_variants.py:1466; the channel count comes with the input)
            m(np.zeros((1, 33, channels), np.float32))
        except Exception as ex:          # noqa: BLE001
            print("F5: could not build the reference model for %d channels: %r" % (channels, ex))
            ok = False
            continue
        with tempfile.TemporaryDirectory() as tmp:
            prefix = os.path.join(tmp, "pileup")
            m.save_weights(prefix)
            blob = tfckpt.weights_from_bundle(prefix, channels=channels)
            ours = np.asarray(blob, np.float32)
            theirs = np.concatenate([w.reshape(-1) for w in m.get_weights()]).astype(np.float32)
            same = ours.size == theirs.size and np.array_equal(np.sort(ours), np.sort(theirs))
            print("F5: %d channels: %d parameters read, %d in the model, multiset %s" % (channels, ours.size, theirs.size, "equal" if same else "DIFFERS"))
            ok = ok and same
    return ok


def pin_whatshap(whatshap):
    """K0 (never run): our haplotags against `whatshap haplotag --output-haplotag-list` on tests/hapref.py's generated cases."""
    import gzip
    import numpy as np
    from clair3_rna_amd import bam, bamio, io
    from clair3_rna_amd.reads import NT16
    from tests import hapref
    ok = True
    for seed in (0, 1, 2):
        ref, rs, sites, _ = hapref.gen_case(seed)
        try:
            from clair3_rna_amd import capi
            eng = capi.Engine(0)
            eng.set_phase_sites(sites)
            eng.load_reads(rs)
            ours, who = eng.haplotags()[0], "k_haplotag"
            eng.close()
        except Exception:          # noqa: BLE001 (no device here: the restatement of the rule)
            ours, who = hapref.haplotag(rs, sites)[0], "tests/hapref.py"
        with tempfile.TemporaryDirectory() as tmp:
            fa, bm, vcf, lst = (os.path.join(tmp, n) for n in ("ref.fa", "in.bam", "phased.vcf.gz", "tags.tsv"))
            io.write_fasta(fa, [("c", ref)])
            bam.write_bam(bm, [("c", len(ref))], {"c": rs})
            bamio.index_build(bm)
            with gzip.open(vcf, "wt") as f:          # (whatshap wants bgzip + tabix: `bgzip` / `tabix -p vcf` beside it do that; plain gzip is tried first)
                f.write("##fileformat=VCFv4.2\n##contig=<ID=c,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"\">\n"
                        "##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n" % len(ref))
                for s_ in sites:
                    f.write("c\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s:%d\n" % (s_["pos"], NT16[s_["ref"]], NT16[s_["alt"]], "1|0" if s_["h1"] else "0|1", s_["ps"]))
            subprocess.check_call([whatshap, "haplotag", "--reference", fa, "--ignore-read-groups", "--output-haplotag-list", lst, "-o", os.path.join(tmp, "out.bam"), vcf, bm])
            theirs = np.zeros(len(rs), np.uint8)
            for row in open(lst):
                f_ = row.split("\t")
                if row[0] != "#" and f_[0][0] == "r" and f_[1] in ("H1", "H2"):
                    theirs[int(f_[0][1:]) - 1] = 1 if f_[1] == "H1" else 2
        both = (ours > 0) & (theirs > 0)
        same = int((ours[both] == theirs[both]).sum())
        print("K0 seed %d (%s): %d reads, both tag %d (same %d, different %d), only ours %d, only whatshap %d" %
              (seed, who, len(rs), int(both.sum()), same, int(both.sum()) - same, int(((ours > 0) & (theirs == 0)).sum()), int(((ours == 0) & (theirs > 0)).sum())))
        ok = ok and both.sum() > 0 and same >= 0.95 * both.sum()
    return ok


def compare_phasing(whatshap):
    """K0, second leg (never run): `whatshap compare` between our phased VCF and `whatshap phase`'s, tests/phaseref.py's cases with errors."""
    import gzip
    from clair3_rna_amd import bam, bamio, io, phasing
    from clair3_rna_amd.reads import NT16
    from tests import phaseref
    for seed in (1, 3, 5):
        ref, rs, sites, _, _ = phaseref.gen_case(seed, errors=True)
        from clair3_rna_amd import capi
        try:
            eng = capi.Engine(0)
        except (ImportError, capi.C3RError) as ex:           # no library or no device here: the restatement of the rule, and the line says so
            print("K0 phasing: no engine (%s)" % ex)
            eng = None
        if eng is None:
            ours, who = phaseref.phase(rs, sites)[0], "tests/phaseref.py"
        else:                                                # (an error of the library from here on is an error of this leg)
            eng.set_params()
            eng.load_reads(rs)
            ours, who = eng.phase_sites(sites)[0], "k_phase_links + c3r_phase_resolve"
            eng.close()
        with tempfile.TemporaryDirectory() as tmp:
            fa, bm, vcf, mine, theirs = (os.path.join(tmp, n) for n in ("ref.fa", "in.bam", "unphased.vcf", "phased_c.vcf.gz", "whatshap.vcf"))
            io.write_fasta(fa, [("c", ref)])
            bam.write_bam(bm, [("c", len(ref))], {"c": rs})
            bamio.index_build(bm)
            with open(vcf, "w") as f:
                f.write("##fileformat=VCFv4.2\n##contig=<ID=c,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"\">\n"
                        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n" % len(ref))
                for s_ in sites:
                    f.write("c\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT\t0/1\n" % (s_["pos"], NT16[s_["ref"]], NT16[s_["alt"]]))
            phasing.write_phased_vcf(vcf, "c", ours, mine)
            subprocess.check_call([whatshap, "phase", "--reference", fa, "--ignore-read-groups", "--distrust-genotypes", "-o", theirs, vcf, bm])
            print("K0 phasing, seed %d (%s): %d of %d sites phased by us; whatshap compare (ours, whatshap):" % (seed, who, int((ours["ps"] >= 0).sum()), len(sites)), flush=True)
            subprocess.check_call([whatshap, "compare", "--names", "builtin,whatshap", mine, theirs])
    return True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samtools")
    ap.add_argument("--tf", action="store_true")
    ap.add_argument("--whatshap", help="K0 (never run): compare our haplotags with `whatshap haplotag --output-haplotag-list`, and our phased VCF with `whatshap phase`'s through `whatshap compare`")
    ap.add_argument("--reference_repo", default="/root/reference")
    ap.add_argument("--list", action="store_true", help="only count the harvested cases (needs neither tool)")
    a = ap.parse_args()
    ok = True
    if a.list:
        c = harvest_cases() + cap_cases()
        print("%d cases (%d reads in the largest)" % (len(c), max(len(x[0]) for x in c)))
    if a.samtools:
        ok = pin_samtools(a.samtools) and ok
    if a.tf:
        ok = pin_tf(a.reference_repo) and ok
    if a.whatshap:
        ok = pin_whatshap(a.whatshap) and ok
        ok = compare_phasing(a.whatshap) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
