"""The rule `hap_junctions` of include/c3r.h (c3r_hap_junction_counts) restated in plain Python: one read at a time, its CIGAR normalised
here, a dict of junctions.  It shares nothing with csrc/hapjunction_kernels.hpp — no hash table, no slots, no LDS, no lanes, no growth —
and is what the tests compare the kernel and the drivers with.  The keep rule and the normalisation are its own; a read's tag comes from
hapref.haplotag and its phase set from hapcountref.read_phase_sets.  It also restates the TSV lines and the motif table of
clair3_rna_amd/hap_junctions.py.  Its own behaviour is pinned by the hand-derived cases of tests/test_hapjunction_ref.py."""
import numpy as np

from clair3_rna_amd.capi import HAP_JUNCTION_DTYPE, HAP_JUNCTION_ROW_DTYPE
from tests import hapcountref, hapref

DEFAULT_PARAMS = dict(min_mq=5, excl_flags=2316)             # c3r_default_params
HEADER = "#CHROM\tSTART\tEND\tMOTIF\tSTRAND\tREADS\tREVERSE\tPS\tHP1\tHP2\tUNTAGGED"
PLUS, MINUS = ("GT-AG", "GC-AG", "AT-AC"), ("CT-AC", "CT-GC", "GT-AT")


def kept(read, params):
    """The tensor build keeps the read: mapped, no excluded flag bit, not a pair that is not a proper pair, MAPQ at least min_mq."""
    flag = int(read["flag"])
    if flag & 4 or flag & int(params["excl_flags"]):
        return False
    if flag & 1 and not flag & 2:
        return False
    return int(read["mapq"]) >= int(params["min_mq"])


def normalised(rs, i):
    """[(letter, length)] of read i: ops of length 0, H and P dropped; = and X are M; equal neighbours merged."""
    r = rs.reads[i]
    out = []
    for k in range(int(r["n_cigar"])):
        c = int(rs.cigar[int(r["cigar_off"]) + k])
        op, ln = "MIDNSHP=X"[c & 15], c >> 4
        if ln == 0 or op in "HP":
            continue
        op = "M" if op in "=X" else op
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + ln)
        else:
            out.append((op, ln))
    return out


def read_junctions(rs, i):
    """[(start, end)] 0-based half-open: the N ops of read i's normalised CIGAR."""
    x, out = int(rs.reads[i]["pos"]), []
    for op, ln in normalised(rs, i):
        if op == "N":
            out.append((x, x + ln))
        if op in "MDN":
            x += ln
    return out


def ref_span(rs, i):
    return sum(ln for op, ln in normalised(rs, i) if op in "MDN")


def counts(rs, table=None, params=DEFAULT_PARAMS):
    """{(start, end): dict(reads, reverse, untagged, rows={ps: [hp1, hp2]})} of the counted reads.  table: the phase table
    (PHASE_SITE_DTYPE) the reads are tagged by; None or empty: every read is untagged."""
    if table is not None and len(table):
        hp, sets = hapref.haplotag(rs, table)[0], hapcountref.read_phase_sets(rs, table)
    else:
        hp, sets = np.zeros(len(rs), np.uint8), np.full(len(rs), -1, np.int32)
    out = {}
    for i in range(len(rs)):
        r = rs.reads[i]
        if not kept(r, params) or ref_span(rs, i) <= 0:
            continue
        for key in read_junctions(rs, i):
            e = out.setdefault(key, dict(reads=0, reverse=0, untagged=0, rows={}))
            e["reads"] += 1
            e["reverse"] += 1 if int(r["flag"]) & 16 else 0
            if hp[i] == 0:
                e["untagged"] += 1
            else:
                e["rows"].setdefault(int(sets[i]), [0, 0])[int(hp[i]) - 1] += 1
    return out


def arrays(found):
    """counts' dict as Engine.hap_junction_counts returns it: (HAP_JUNCTION_DTYPE array by (start, end), HAP_JUNCTION_ROW_DTYPE array, a
    junction's rows by ps)."""
    keys = sorted(found)
    j, rows = np.zeros(len(keys), dtype=HAP_JUNCTION_DTYPE), []
    for k, key in enumerate(keys):
        e = found[key]
        j[k] = (key[0], key[1], e["reads"], e["reverse"], e["untagged"], len(rows))
        rows += [(ps, e["rows"][ps][0], e["rows"][ps][1]) for ps in sorted(e["rows"])]
    r = np.zeros(len(rows), dtype=HAP_JUNCTION_ROW_DTYPE)
    for k, row in enumerate(rows):
        r[k] = row
    return j, r


def invariant(found):
    """reads == untagged + the sum of hp1 + hp2 over the rows, every row holds a read, reverse <= reads."""
    return all(e["reads"] == e["untagged"] + sum(a + b for a, b in e["rows"].values()) and e["reverse"] <= e["reads"] and e["reads"] >= 1
               and all(a + b >= 1 for a, b in e["rows"].values()) for e in found.values())


def motif(seq, start, end):
    """(MOTIF, STRAND): the first two and the last two bases of [start, end) on `seq` (position 0 first; None: no reference)."""
    if seq is None:
        return ".", "."
    first, last = seq[start:start + 2], seq[max(end - 2, 0):end]
    if len(first) != 2 or len(last) != 2 or end > len(seq):
        return ".", "."
    m = "%s-%s" % (first.upper(), last.upper())
    return m, "+" if m in PLUS else "-" if m in MINUS else "."


def lines(ctg, found, seq=None, min_reads=1):
    """The contig's TSV lines from counts' dict."""
    out = []
    for key in sorted(found):
        e = found[key]
        if e["reads"] < min_reads:
            continue
        head = "%s\t%d\t%d\t%s\t%s" % ((ctg, key[0], key[1]) + motif(seq, key[0], key[1]))
        out.append("%s\t%d\t%d\t.\t.\t.\t%d" % (head, e["reads"], e["reverse"], e["untagged"]))
        out += ["%s\t.\t.\t%d\t%d\t%d\t." % (head, ps, e["rows"][ps][0], e["rows"][ps][1]) for ps in sorted(e["rows"])]
    return out


def readset(recs):
    """[(pos, cigar, seq[, flag[, mapq]])] -> ReadSet."""
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3] if len(r) > 3 else 0, mapq=r[4] if len(r) > 4 else 60, hp=0) for r in recs])


def forced_serial(rs, every=1):
    """The same reads with an empty op (`0D`) behind the first op of every `every`-th read: an op the device's plain walk does not take, so
    those reads go through its serial walk, and one the rule does not see."""
    from clair3_rna_amd.reads import ReadSet
    cig, reads, off = [], rs.reads.copy(), 0
    for i, r in enumerate(rs.reads):
        c = rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])].tolist()
        if i % every == 0:
            c = c[:1] + [2] + c[1:]                              # (length 0 << 4 | D)
        reads[i]["cigar_off"], reads[i]["n_cigar"] = off, len(c)
        cig += c
        off += len(c)
    return ReadSet(reads, np.array(cig, dtype=np.uint32), rs.seq.copy())


# ---- hand-derived known answers.  The phase table is one site, 1-based 103 A > C with h1 = 0 in set 7: a read at 0-based 100 whose third
# base is A has tag 1 in set 7, one whose third base is C has tag 2 in set 7, one whose third base is G has no vote.
# (name, [(pos, cigar, seq, flag, mapq)], {(start, end): (reads, reverse, untagged, {ps: (hp1, hp2)})}): worked out by hand from the rule.
A20, C20, G20 = "A" * 20, "AAC" + "A" * 17, "AAG" + "A" * 17
HAND_SITES = [(103, "A", "C", 0, 7)]
HAND = [
    ("one_junction", [(100, "10M50N10M", A20)], {(110, 160): (1, 0, 0, {7: (1, 0)})}),
    ("same_start_other_end", [(100, "10M50N10M", A20), (100, "10M60N10M", C20)], {(110, 160): (1, 0, 0, {7: (1, 0)}), (110, 170): (1, 0, 0, {7: (0, 1)})}),
    ("same_end_other_start", [(100, "10M50N10M", A20), (100, "12M48N8M", G20)], {(110, 160): (1, 0, 0, {7: (1, 0)}), (112, 160): (1, 0, 1, {})}),
    ("both_haplotypes_and_an_untagged_read_on_one_junction", [(100, "10M50N10M", A20), (100, "10M50N10M", C20), (100, "10M50N10M", G20), (100, "10M50N10M", C20)],
     {(110, 160): (4, 0, 1, {7: (1, 2)})}),
    # 5M 3I 10N 5M at 100: the M ends at 105, the insertion consumes no reference
    ("insertion_before_the_junction", [(100, "5M3I10N5M", "A" * 13)], {(105, 115): (1, 0, 0, {7: (1, 0)})}),
    # 10M 2D 100N 10M at 100: the deletion covers [110, 112)
    ("deletion_before_the_junction", [(100, "10M2D100N10M", A20)], {(112, 212): (1, 0, 0, {7: (1, 0)})}),
    ("an_empty_n_is_no_junction", [(100, "10M0N10M", A20)], {}),
    ("an_empty_n_beside_a_junction", [(100, "10M0N50N10M", A20)], {(110, 160): (1, 0, 0, {7: (1, 0)})}),
    ("eq_x_hard_clip_pad_and_empty_ops", [(100, "2H4=0D1X1P5M50N1P4=6X3H", A20)], {(110, 160): (1, 0, 0, {7: (1, 0)})}),
    ("adjacent_n_ops_are_one_junction", [(100, "10M20N30N10M", A20)], {(110, 160): (1, 0, 0, {7: (1, 0)})}),
    ("n_ops_a_pad_apart_are_one_junction", [(100, "10M20N1P0I30N10M", A20)], {(110, 160): (1, 0, 0, {7: (1, 0)})}),
    ("two_junctions_of_one_read", [(100, "5M10N5M20N10M", A20)], {(105, 115): (1, 0, 0, {7: (1, 0)}), (120, 140): (1, 0, 0, {7: (1, 0)})}),
    ("mapq_0_and_supplementary_do_not_count", [(100, "10M50N10M", A20, 0, 0), (100, "10M50N10M", A20, 2048), (100, "10M50N10M", A20)], {(110, 160): (1, 0, 0, {7: (1, 0)})}),
    ("forward_and_reverse", [(100, "10M50N10M", A20), (100, "10M50N10M", A20, 16)], {(110, 160): (2, 1, 0, {7: (2, 0)})}),
    ("junction_at_position_0", [(0, "7N10M", "A" * 10)], {(0, 7): (1, 0, 1, {})}),
    ("junction_ending_at_2_31_minus_1", [(2147483547, "10M90N", "A" * 10)], {(2147483557, 2147483647): (1, 0, 1, {})}),
    ("no_junction_at_all", [(100, "20M", A20), (100, "5M2D5M3I7M", A20)], {}),
]


def hand_inputs(case):
    """(ReadSet, phase table, expected counts dict) of one entry of HAND."""
    _, reads, want = case
    return readset(reads), hapref.make_sites(HAND_SITES), {k: dict(reads=v[0], reverse=v[1], untagged=v[2], rows={ps: list(c) for ps, c in v[3].items()}) for k, v in want.items()}


# ---- the generated cases of the GPU tests
def shared_case(seed):
    """phaseref.gen_case(seed) — spliced reads over twelve exons, dozens of reads per junction — with a table made of its sites, the
    generator's truth as h1 and ps = 1000 + (site index mod 3): -> (ReadSet, table)."""
    from tests import phaseref
    _, rs, sites, truth, _ = phaseref.gen_case(seed)
    table = sites.copy()
    table["h1"], table["ps"] = truth, 1000 + np.arange(len(table)) % 3
    return rs, table


def distinct_case(seed):
    """hapref.gen_case(seed): 400 reads with up to 40 random introns each, nearly all junctions distinct: -> (ReadSet, table)."""
    _, rs, table, _ = hapref.gen_case(seed)
    return rs, table


# ---- the drivers' sample
def driver_sample(d, n_reads=83):
    """chr1 (phaseref.gen_case reads, which share their junctions; phased: a directory with phased_chr1.vcf.gz made of shared_case's
    table), chr2 (hapref.gen_case reads, nothing phased), chrEmpty (no record) on their references, indexed, and the FASTA."""
    import gzip
    import os
    from clair3_rna_amd import bam, bamio, io
    from clair3_rna_amd.reads import NT16
    contigs, reads, case, refs = [], {}, {}, {}
    from tests import phaseref
    for name in ("chr1", "chr2"):
        if name == "chr1":
            ref, rs, sites, truth, _ = phaseref.gen_case(1, n_reads=n_reads)
            sites = sites.copy()
            sites["h1"], sites["ps"] = truth, 1000 + np.arange(len(sites)) % 3
        else:
            ref, rs, sites, _ = hapref.gen_case(1, n_reads=n_reads)
        ref = ref[:3000].lower() + ref[3000:]                 # (a lower-case half: MOTIF is upper-cased)
        contigs.append((name, len(ref)))
        reads[name], case[name], refs[name] = rs, sites, ref
    refs["chrEmpty"] = "ACGT" * 1250
    bam_fn = os.path.join(d, "plain.bam")
    bam.write_bam(bam_fn, contigs + [("chrEmpty", 5000)], reads)
    bamio.index_build(bam_fn)
    fa = os.path.join(d, "ref.fa")
    io.write_fasta(fa, [(n, refs[n]) for n in ("chr1", "chr2", "chrEmpty")])
    per = os.path.join(d, "phased_vcf")
    os.makedirs(per)
    with gzip.open(os.path.join(per, "phased_chr1.vcf.gz"), "wt") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")
        for s in case["chr1"]:
            f.write("chr1\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s:%d\n" % (s["pos"], NT16[s["ref"]], NT16[s["alt"]], "1|0" if s["h1"] else "0|1", s["ps"]))
    return dict(bam=bam_fn, per=per, fa=fa, reads=reads, case=case, refs=refs)


def predicted_lines(s, ctg, with_ref=False, min_reads=1, params=DEFAULT_PARAMS, table=None, phased=True):
    """The contig's lines from the restatement alone.  chr1 is the phased contig of driver_sample; `table` overrides its table."""
    if table is None:
        table = s["case"][ctg] if phased and ctg == "chr1" else None
    return lines(ctg, counts(s["reads"][ctg], table, params), s["refs"][ctg] if with_ref else None, min_reads)
