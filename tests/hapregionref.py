"""The rule `hap_regions` of include/c3r.h (c3r_hap_region_counts) restated in plain Python: one read at a time, one region at a time, a list
of the stretches the read covers.  It shares nothing with csrc/hapregion_kernels.hpp — no sorted table, no first_open, no searches, no
lanes — and is what the tests compare the kernel and the drivers with.  A read's tag comes from hapref.haplotag, its phase set from
hapcountref.read_phase_sets, the voters from phaseref.votes.  Its own behaviour is pinned by the hand-derived cases of
tests/test_hapregion_ref.py.

gen_regions(seed, table) builds the random interval tables of the GPU tests."""
import random

import numpy as np

from clair3_rna_amd.capi import HAP_REGION_DTYPE
from tests import hapcountref, hapref, phaseref

DEFAULT_PARAMS = phaseref.DEFAULT_PARAMS
MAX_BACK = 4096                                              # C3R_HAP_REGION_MAX_BACK
STRAND = {".": 0, "+": 1, "-": 2, None: 0}


def covered(rs, i):
    """[(first, past the last)] 0-based reference stretches under the M / = / X / D ops of read i, in order: adjacent M-like ops are one
    stretch (the normalised CIGAR has them as one op); H, P and empty ops are nothing."""
    r = rs.reads[i]
    x, out, last = int(r["pos"]), [], None
    for k in range(int(r["n_cigar"])):
        c = int(rs.cigar[int(r["cigar_off"]) + k])
        op, ln = "MIDNSHP=X"[c & 15], c >> 4
        if ln == 0 or op in "HP":
            continue
        kind = "M" if op in "M=X" else op
        if kind in "MD":
            if kind == last and kind == "M":
                out[-1] = (out[-1][0], x + ln)
            else:
                out.append((x, x + ln))
            x += ln
        elif kind == "N":
            x += ln
        last = kind
    return out


def row_table(regions, table):
    """The driver's rows: per region (start, end, ...) the distinct ps of the phase table's sites with start < pos <= end, in increasing
    order.  -> list of lists."""
    return [sorted({int(s["ps"]) for s in table if r[0] < int(s["pos"]) <= r[1]}) for r in regions]


def pack(regions, rows):
    """[(start, end, strand 0 / 1 / 2)] in table order and their rows -> (HAP_REGION_DTYPE array, int32 row_ps)."""
    a = np.zeros(len(regions), dtype=HAP_REGION_DTYPE)
    ps = []
    for j, r in enumerate(regions):
        a[j]["start"], a[j]["end"], a[j]["strand"], a[j]["row_off"] = r[0], r[1], r[2], len(ps)
        ps += rows[j]
    return a, np.array(ps, dtype=np.int32).reshape(len(ps))


def counts(rs, table, regions, row_ps, stranded=0, params=DEFAULT_PARAMS, detail=None):
    """(region_counts uint32 (n, 2), row_counts uint32 (n_rows, 2)) of a HAP_REGION_DTYPE array and its row_ps.  table: the phase table
    (PHASE_SITE_DTYPE) the reads are tagged by.  detail: a dict that receives `multi_op_pairs`, the (read, region) pairs counted in which two
    or more stretches of the read overlap the region."""
    n, n_rows = len(regions), len(row_ps)
    hp = hapref.haplotag(rs, table)[0]
    sets = hapcountref.read_phase_sets(rs, table)
    rc, wc = np.zeros((n, 2), dtype=np.uint32), np.zeros((n_rows, 2), dtype=np.uint32)
    multi = 0
    for i in range(len(rs)):
        r = rs.reads[i]
        cov = covered(rs, i)
        if not phaseref.votes(r, params) or not cov:
            continue
        own = 2 if int(r["flag"]) & 16 else 1
        for j in range(n):
            e = regions[j]
            hits = sum(1 for a, b in cov if a < int(e["end"]) and b > int(e["start"]))
            if hits == 0:
                continue
            es = int(e["strand"])
            if stranded and es and (es == own) != (stranded == 1):
                continue
            multi += hits >= 2
            lo = int(e["row_off"])
            top = int(regions[j + 1]["row_off"]) if j + 1 < n else n_rows
            if hp[i] == 0:
                rc[j, 0] += 1
                continue
            for row in range(lo, top):
                if int(row_ps[row]) == int(sets[i]):
                    wc[row, int(hp[i]) - 1] += 1
                    break
            else:
                rc[j, 1] += 1
    if detail is not None:
        detail["multi_op_pairs"] = multi
    return rc, wc


def first_open(regions):
    """[smallest i <= j with end_i > start_j] by trying every i."""
    return [min(i for i in range(j + 1) if int(regions[i]["end"]) > int(regions[j]["start"])) for j in range(len(regions))]


def max_back(regions):
    fo = first_open(regions)
    return max([j - f for j, f in enumerate(fo)] or [0])


def gen_regions(seed, table, L=6000):
    """(HAP_REGION_DTYPE array, row_ps): 48 random regions on the 6-kb generators plus two exact duplicates of two of them, sorted by (start,
    end) — 10 % of length 1, 30 % of 2-50, 50 % of 50-600, 10 % of 2000-5000 —, strand drawn from (0, 0, 1, 2), rows by the driver's policy
    (row_table).  Starts keep 500 bases off the reference's end, where hapref.gen_case starts no read."""
    rng = random.Random(1000003 * seed + 17)
    regs = []
    for _ in range(48):
        u = rng.random()
        ln = 1 if u < 0.1 else rng.randint(2, 50) if u < 0.4 else rng.randint(50, 600) if u < 0.9 else rng.randint(2000, 5000)
        start = rng.randrange(0, max(1, L - 500 - ln))
        regs.append((start, start + ln, rng.choice((0, 0, 1, 2))))
    regs += [regs[3], regs[29]]
    regs.sort(key=lambda r: (r[0], r[1]))                    # (a stable sort: equal regions keep their strands' order, whatever it is)
    return pack(regs, row_table(regs, table))


def phase_case_exons(seed, L=6000, n_exons=12):
    """The exons [(start, end)] of phaseref.gen_case(seed): the generator draws them right after the reference, from the same stream."""
    rng = random.Random(seed)
    for _ in range(L):
        rng.choice("ACGT")
    cuts = sorted(rng.sample(range(60, L - 60), 2 * n_exons))
    return [(cuts[2 * e], cuts[2 * e + 1]) for e in range(n_exons) if cuts[2 * e + 1] - cuts[2 * e] >= 8]


# ---- hand-derived known answers.  Every read is 20 bases of A (G where noted) at 0-based 100 unless the case says otherwise; the phase table
# is one site, 1-based 103 A > C with h1 = 0 in set 7, so a read whose base there is A has tag 1 in set 7 and one whose base is G has no
# vote.  (name, [(pos, cigar, seq, flag, mapq)], [(start, end, strand, [rows])] sorted, stranded, region_counts, row_counts): every
# expectation was worked out by hand from the rule.
A20 = "A" * 20
HAND_SITES = [(103, "A", "C", 0, 7)]
SPLICED = (100, "10M50N10M", A20, 0, 60)                     # covers [100, 110) and [160, 170)
HAND = [
    ("intron_only", [SPLICED], [(120, 150, 0, [7])], 0, [(0, 0)], [(0, 0)]),
    ("from_the_intron_into_the_second_exon", [SPLICED], [(140, 165, 0, [7])], 0, [(0, 0)], [(1, 0)]),
    ("over_both_exons_counts_once", [SPLICED], [(90, 200, 0, [7])], 0, [(0, 0)], [(1, 0)]),
    ("both_exons_and_the_set_is_no_row", [SPLICED], [(90, 200, 0, [])], 0, [(0, 1)], []),
    ("rows_that_do_not_hold_the_set", [SPLICED], [(90, 200, 0, [3, 6, 8])], 0, [(0, 1)], [(0, 0), (0, 0), (0, 0)]),
    ("the_set_among_several_rows", [SPLICED], [(90, 200, 0, [3, 7, 8])], 0, [(0, 0)], [(0, 0), (1, 0), (0, 0)]),
    ("untagged_read", [(100, "10M50N10M", "AAGAAAAAAAAAAAAAAAAA", 0, 60)], [(90, 200, 0, [7])], 0, [(1, 0)], [(0, 0)]),
    # 5M 3D 5M at 100: M [100, 105), D [105, 108), M [108, 113)
    ("only_a_deletion", [(100, "5M3D5M", "A" * 10, 0, 60)], [(105, 108, 0, [7]), (106, 107, 0, [])], 0, [(0, 0), (0, 1)], [(1, 0)]),
    # 5M 3I 10N 5M at 100: M [100, 105), the insertion between 104 and 105, intron [105, 115), M [115, 120)
    ("only_an_insertion_and_the_intron_behind_it", [(100, "5M3I10N5M", "A" * 13, 0, 60)], [(105, 115, 0, [7])], 0, [(0, 0)], [(0, 0)]),
    # 3S 5M 2S at 100: the clips would lie on [97, 100) and [105, 107)
    ("only_a_soft_clip", [(100, "3S5M2S", "A" * 10, 0, 60)], [(97, 100, 0, [7]), (105, 107, 0, [7])], 0, [(0, 0), (0, 0)], [(0, 0), (0, 0)]),
    ("length_1_on_the_first_and_last_base_and_one_outside",
     [SPLICED], [(99, 100, 0, []), (100, 101, 0, []), (109, 110, 0, []), (110, 111, 0, []), (159, 160, 0, []), (160, 161, 0, []), (169, 170, 0, []), (170, 171, 0, [])], 0,
     [(0, 0), (0, 1), (0, 1), (0, 0), (0, 0), (0, 1), (0, 1), (0, 0)], []),
    ("equal_regions", [SPLICED], [(100, 110, 0, [7]), (100, 110, 0, [7]), (100, 110, 0, [])], 0, [(0, 0), (0, 0), (0, 1)], [(1, 0), (1, 0)]),
    ("nested_regions", [SPLICED], [(90, 300, 0, []), (100, 101, 0, []), (120, 130, 0, []), (165, 166, 0, [])], 0, [(0, 1), (0, 1), (0, 0), (0, 1)], []),
    # a forward and a reverse read; regions without a strand, +, -
    ("stranded_off", [SPLICED, (100, "10M50N10M", A20, 16, 60)], [(100, 110, 0, []), (100, 110, 1, []), (100, 110, 2, [])], 0, [(0, 2), (0, 2), (0, 2)], []),
    ("stranded_same", [SPLICED, (100, "10M50N10M", A20, 16, 60)], [(100, 110, 0, [7]), (100, 110, 1, [7]), (100, 110, 2, [7])], 1, [(0, 0)] * 3, [(2, 0), (1, 0), (1, 0)]),
    ("stranded_same_forward_only", [SPLICED], [(100, 110, 0, []), (100, 110, 1, []), (100, 110, 2, [])], 1, [(0, 1), (0, 1), (0, 0)], []),
    ("stranded_reverse_forward_only", [SPLICED], [(100, 110, 0, []), (100, 110, 1, []), (100, 110, 2, [])], 2, [(0, 1), (0, 0), (0, 1)], []),
    ("stranded_reverse_reverse_only", [(100, "10M50N10M", A20, 16, 60)], [(100, 110, 0, []), (100, 110, 1, []), (100, 110, 2, [])], 2, [(0, 1), (0, 1), (0, 0)], []),
    ("mapq_0_and_supplementary_do_not_count", [(100, "10M50N10M", A20, 0, 0), (100, "10M50N10M", A20, 2048, 60), SPLICED], [(90, 200, 0, [7])], 0, [(0, 0)], [(1, 0)]),
    ("eq_x_hard_clip_pad_and_empty_ops", [(100, "2H4=0D1X1P5M50N10M3H", A20, 0, 60)], [(90, 200, 0, [7]), (109, 161, 0, [7])], 0, [(0, 0), (0, 0)], [(1, 0), (1, 0)]),
]


def hand_inputs(case):
    """(ReadSet, phase table, HAP_REGION_DTYPE array, row_ps, stranded, expected region_counts, expected row_counts) of one entry of HAND."""
    from clair3_rna_amd.reads import ReadSet
    _, reads, regions, stranded, rc, wc = case
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3], mapq=r[4], hp=0) for r in reads])
    tab, row_ps = pack([r[:3] for r in regions], [r[3] for r in regions])
    return (rs, hapref.make_sites(HAND_SITES), tab, row_ps, stranded, np.array(rc, dtype=np.uint32).reshape(len(rc), 2),
            np.array(wc, dtype=np.uint32).reshape(len(wc), 2))


# ---- the drivers' sample and the lines the restatement predicts for it
def driver_sample(d, n_reads=83):
    """chr1 (phased: a directory with phased_chr1.vcf.gz), chr2 (reads, nothing phased), chrEmpty (no record), chrNoBed (reads, no BED line)
    of gen_case reads, indexed, and a BED over chr2, chr1 (not in the header's order), chrEmpty and a contig the BAM does not know."""
    import gzip
    import os
    from clair3_rna_amd import bam, bamio
    from clair3_rna_amd.reads import NT16
    contigs, reads, case = [], {}, {}
    for name, seed in (("chr1", 0), ("chr2", 1), ("chrNoBed", 2)):
        ref, rs, sites, _ = hapref.gen_case(seed, n_reads=n_reads)
        contigs.append((name, len(ref)))
        reads[name], case[name] = rs, sites
    bam_fn = os.path.join(d, "plain.bam")
    bam.write_bam(bam_fn, contigs + [("chrEmpty", 5000)], reads)
    bamio.index_build(bam_fn)
    per = os.path.join(d, "phased_vcf")
    os.makedirs(per)
    with gzip.open(os.path.join(per, "phased_chr1.vcf.gz"), "wt") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")
        for s in case["chr1"]:
            f.write("chr1\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s:%d\n" % (s["pos"], NT16[s["ref"]], NT16[s["alt"]], "1|0" if s["h1"] else "0|1", s["ps"]))
    bed = {"chr1": [(2000, 2600, "late", "+"), (100, 4000, "gene1", "-"), (500, 501, "one", None), (2000, 2600, "late_again", None), (3000, 3300, "exon", "+")],
           "chr2": [(10, 900, "g2", "+")], "chrEmpty": [(1, 2, "nothing", None)], "chrOther": [(1, 2, "unknown", None)]}
    bed_fn = os.path.join(d, "regions.bed")
    with open(bed_fn, "w") as f:
        for ctg in ("chr2", "chr1", "chrEmpty", "chrOther"):
            for start, end, name, strand in bed[ctg]:
                f.write("%s\t%d\t%d\t%s\t0\t%s\n" % (ctg, start, end, name, strand or "."))
            if ctg == "chr1":
                f.write("chr1\t700\t700\tskipped\t0\t+\n")
    return dict(bam=bam_fn, per=per, reads=reads, case=case, bed=bed, bed_fn=bed_fn)


def predicted_lines(s, ctg, stranded=0, params=DEFAULT_PARAMS, table=None):
    """The contig's lines from the restatement alone: regions in BED order, rows by row_table."""
    regions = s["bed"][ctg]
    table = s["case"][ctg] if table is None else table
    order = sorted(range(len(regions)), key=lambda j: (regions[j][0], regions[j][1]))
    regs = [(regions[j][0], regions[j][1], STRAND[regions[j][3]]) for j in order]
    tab, row_ps = pack(regs, row_table(regs, table))
    rc, wc = counts(s["reads"][ctg], table, tab, row_ps, stranded, params)
    lines = [None] * len(regions)
    for k, j in enumerate(order):
        start, end, name, strand = regions[j]
        head = "%s\t%d\t%d\t%s\t%s" % (ctg, start, end, name, strand or ".")
        lo, top = int(tab[k]["row_off"]), (int(tab[k + 1]["row_off"]) if k + 1 < len(tab) else len(row_ps))
        lines[j] = [head + "\t.\t.\t.\t%d\t%d" % (rc[k, 0], rc[k, 1])] + [head + "\t%d\t%d\t%d\t.\t." % (row_ps[r], wc[r, 0], wc[r, 1]) for r in range(lo, top)]
    return [x for block in lines for x in block]


def uncounted_lines(s, ctg):
    return ["%s\t%d\t%d\t%s\t%s\t.\t.\t.\t.\t." % (ctg, a, b, name, strand or ".") for a, b, name, strand in s["bed"][ctg]]
