"""The rule `hap_groups` of include/c3r.h (c3r_hap_group_counts) restated in plain Python: one read at a time, one group at a time — "any
covered stretch of the read meets any interval of the group that admits the read".  It shares nothing with csrc/hapgroup_kernels.hpp — no
chain of a group's intervals, no sorted table, no searches, no lanes — and is what the tests compare the kernel and the drivers with.  The
covered stretches are hapregionref.covered's, a read's tag hapref.haplotag's, its phase set hapcountref.read_phase_sets', the voters
phaseref.votes'.  Its own behaviour is pinned by the hand-derived cases of tests/test_hapgroup_ref.py."""
import numpy as np

from clair3_rna_amd.capi import HAP_INTERVAL_DTYPE
from tests import hapcountref, hapref, phaseref
from tests import hapregionref as HR

DEFAULT_PARAMS = phaseref.DEFAULT_PARAMS
STRAND = HR.STRAND


def pack(intervals, group_rows):
    """[(start, end, group, strand 0 / 1 / 2)] in table order and the rows of every group [[ps]] -> (HAP_INTERVAL_DTYPE array,
    int32 group_row_off [n_groups], int32 row_ps)."""
    a = np.zeros(len(intervals), dtype=HAP_INTERVAL_DTYPE)
    for j, e in enumerate(intervals):
        a[j]["start"], a[j]["end"], a[j]["group"], a[j]["strand"] = e
    off, ps = [], []
    for rows in group_rows:
        off.append(len(ps))
        ps += rows
    return a, np.array(off, dtype=np.int32).reshape(len(off)), np.array(ps, dtype=np.int32).reshape(len(ps))


def group_rows(intervals, n_groups, table):
    """The driver's rows: per group the distinct ps of the phase table's sites inside any of its intervals (start < pos <= end), increasing."""
    return [sorted({int(s["ps"]) for s in table if any(e[2] == g and e[0] < int(s["pos"]) <= e[1] for e in intervals)}) for g in range(n_groups)]


def counts(rs, table, intervals, n_groups, group_row_off, row_ps, stranded=0, params=DEFAULT_PARAMS, detail=None):
    """(group_counts uint32 (n_groups, 2), row_counts uint32 (n_rows, 2)) of a HAP_INTERVAL_DTYPE array, its groups' row offsets and row_ps.
    table: the phase table (PHASE_SITE_DTYPE) the reads are tagged by.  detail: a dict that receives `pairs` (the counted (read, group)
    pairs), `multi_interval_pairs` (those in which the read meets two or more of the group's intervals) and `skipped_inside_pairs` (those in
    which it misses an interval of the group that lies between two it meets)."""
    n_rows = len(row_ps)
    hp = hapref.haplotag(rs, table)[0]
    sets = hapcountref.read_phase_sets(rs, table)
    gc, wc = np.zeros((n_groups, 2), dtype=np.uint32), np.zeros((n_rows, 2), dtype=np.uint32)
    members = [[] for _ in range(n_groups)]
    for e in intervals:
        members[int(e["group"])].append((int(e["start"]), int(e["end"]), int(e["strand"])))
    offs = [int(x) for x in group_row_off] + [n_rows]
    pairs = multi = skipped = 0
    for i in range(len(rs)):
        r = rs.reads[i]
        cov = HR.covered(rs, i)
        if not phaseref.votes(r, params) or not cov:
            continue
        own = 2 if int(r["flag"]) & 16 else 1
        for g in range(n_groups):
            met = []
            for start, end, es in sorted(members[g]):
                admitted = not (stranded and es and (es == own) != (stranded == 1))
                met.append(admitted and any(a < end and b > start for a, b in cov))
            if not any(met):
                continue
            pairs += 1
            multi += sum(met) >= 2
            first, last = met.index(True), len(met) - 1 - met[::-1].index(True)
            skipped += not all(met[first:last + 1])
            if hp[i] == 0:
                gc[g, 0] += 1
                continue
            for row in range(offs[g], offs[g + 1]):
                if int(row_ps[row]) == int(sets[i]):
                    wc[row, int(hp[i]) - 1] += 1
                    break
            else:
                gc[g, 1] += 1
    if detail is not None:
        detail.update(pairs=pairs, multi_interval_pairs=multi, skipped_inside_pairs=skipped)
    return gc, wc


# ---- hand-derived known answers, in the style of hapregionref.HAND.  Every read is A (G where noted) at 0-based 100 unless the case says
# otherwise; the phase table is hapregionref.HAND_SITES — one site, 1-based 103 A > C with h1 = 0 in set 7 —, so a read whose base there is A
# has tag 1 in set 7 and one whose base is G has no vote.  (name, [(pos, cigar, seq, flag, mapq)], [(start, end, group, strand)] sorted,
# [rows of every group], stranded, group_counts, row_counts): every expectation was worked out on paper from the rule.
A20, A30 = "A" * 20, "A" * 30
SPLICED = HR.SPLICED                                          # 10M50N10M: covers [100, 110) and [160, 170)
THREE = (100, "10M20N10M20N10M", A30, 0, 60)                  # covers [100, 110), [130, 140), [160, 170)
SKIP2 = (100, "10M50N10M", A20, 0, 60)                        # over exon 1 and exon 3 of the gene below; exon 2 lies in its intron
FORTY = (100, "N".join(["3M5"] * 39 + ["3M"]), "A" * 120, 0, 60)      # 40 M ops of 3 bases, 8 apart: [100 + 8 k, 103 + 8 k)
HAND = [
    ("two_exons_of_one_gene_count_once", [SPLICED], [(100, 110, 0, 0), (160, 170, 0, 0)], [[7]], 0, [(0, 0)], [(1, 0)]),
    ("three_exons_of_one_gene_count_once", [THREE], [(95, 105, 0, 0), (130, 140, 0, 0), (165, 200, 0, 0)], [[7]], 0, [(0, 0)], [(1, 0)]),
    ("exon_1_and_3_and_exon_2_in_the_intron", [SKIP2], [(100, 110, 0, 0), (120, 150, 0, 0), (160, 170, 0, 0)], [[7]], 0, [(0, 0)], [(1, 0)]),
    # 5M 3D 50N 10M at 100: M [100, 105), D [105, 108), intron [108, 158), M [158, 168)
    ("an_earlier_exon_met_only_by_a_deletion", [(100, "5M3D50N10M", "A" * 15, 0, 60)], [(106, 108, 0, 0), (160, 170, 0, 0)], [[7]], 0, [(0, 0)], [(1, 0)]),
    # the read begins at 100, where the earlier exon ends: not covered, the later exon counts
    ("an_earlier_exon_that_ends_where_the_read_begins", [SPLICED], [(50, 100, 0, 0), (105, 108, 0, 0)], [[7]], 0, [(0, 0)], [(1, 0)]),
    ("only_in_the_intron_of_the_gene", [(120, "20M", A20, 0, 60)], [(100, 110, 0, 0), (160, 170, 0, 0)], [[7]], 0, [(0, 0)], [(0, 0)]),
    ("spliced_over_the_gene_but_the_exons_lie_in_its_intron", [SPLICED], [(110, 130, 0, 0), (140, 160, 0, 0)], [[7]], 0, [(0, 0)], [(0, 0)]),
    # 10M 3I 10M at 100: M [100, 110), M [110, 120) — two ops, abutting on the reference
    ("an_insertion_between_the_two_m_ops", [(100, "10M3I10M", "A" * 23, 0, 60)], [(105, 110, 0, 0), (110, 115, 0, 0), (118, 130, 1, 0)], [[7], []], 0, [(0, 0), (0, 1)], [(1, 0)]),
    # 3S 10M 50N 10M at 100: the clip would lie on [97, 100) and covers nothing, so gene 0 is met in its second exon only
    ("a_soft_clip_before_the_first_m_op", [(100, "3S10M50N10M", "A" * 23, 0, 60)], [(97, 100, 0, 0), (100, 101, 1, 0), (160, 170, 0, 0)], [[7], [7]], 0, [(0, 0), (0, 0)], [(1, 0), (1, 0)]),
    ("abutting_intervals_of_one_group", [(100, "20M", A20, 0, 60)], [(90, 105, 0, 0), (105, 110, 0, 0), (110, 200, 0, 0)], [[7]], 0, [(0, 0)], [(1, 0)]),
    # genes 0 and 1 alternate: 0 has [100, 105) and [160, 165), 1 has [105, 110) and [165, 170); a third has only [130, 140) in the intron
    ("two_genes_with_alternating_exons", [SPLICED], [(100, 105, 0, 0), (105, 110, 1, 0), (130, 140, 2, 0), (160, 165, 0, 0), (165, 170, 1, 0)], [[7], [], [7]], 0,
     [(0, 0), (0, 1), (0, 0)], [(1, 0), (0, 0)]),
    # the table neighbour before the later exon of gene 0 belongs to gene 1 and is not met: gene 0 still counts once, gene 1 not at all
    ("the_chain_follows_the_group_not_the_neighbour", [SPLICED], [(100, 110, 0, 0), (120, 150, 1, 0), (160, 170, 0, 0), (180, 190, 1, 0)], [[7], [7]], 0,
     [(0, 0), (0, 0)], [(1, 0), (0, 0)]),
    ("a_gene_nested_in_anothers_intron", [SPLICED, (125, "10M", "A" * 10, 0, 60)], [(100, 110, 0, 0), (120, 140, 1, 0), (160, 170, 0, 0)], [[], []], 0,
     [(0, 1), (1, 0)], []),
    ("equal_intervals_in_different_groups", [SPLICED], [(100, 110, 0, 0), (100, 110, 1, 0), (160, 170, 1, 0), (160, 170, 2, 0)], [[7], [], [3, 7, 8]], 0,
     [(0, 0), (0, 1), (0, 0)], [(1, 0), (0, 0), (1, 0), (0, 0)]),
    ("forty_m_ops_over_forty_exons", [FORTY], [(100 + 8 * k, 103 + 8 * k, 0, 0) for k in range(40)], [[7]], 0, [(0, 0)], [(1, 0)]),
    # the same read over two genes that take the exons in turn, and one gene that has only the last
    ("forty_m_ops_over_two_interleaved_genes", [FORTY], [(100 + 8 * k, 103 + 8 * k, k % 2, 0) for k in range(40)] + [(414, 500, 2, 0)], [[7], [], [7]], 0,
     [(0, 0), (0, 1), (0, 0)], [(1, 0), (1, 0)]),
    # a forward and a reverse read; genes without a strand, +, - of two exons each
    ("stranded_off", [SPLICED, (100, "10M50N10M", A20, 16, 60)], [(100, 110, 0, 0), (100, 110, 1, 1), (100, 110, 2, 2), (160, 170, 0, 0), (160, 170, 1, 1), (160, 170, 2, 2)],
     [[], [], []], 0, [(0, 2), (0, 2), (0, 2)], []),
    ("stranded_same", [SPLICED, (100, "10M50N10M", A20, 16, 60)], [(100, 110, 0, 0), (100, 110, 1, 1), (100, 110, 2, 2), (160, 170, 0, 0), (160, 170, 1, 1), (160, 170, 2, 2)],
     [[7], [7], [7]], 1, [(0, 0)] * 3, [(2, 0), (1, 0), (1, 0)]),
    ("stranded_reverse_forward_only", [SPLICED], [(100, 110, 0, 0), (100, 110, 1, 1), (100, 110, 2, 2), (160, 170, 0, 0), (160, 170, 1, 1), (160, 170, 2, 2)],
     [[], [], []], 2, [(0, 1), (0, 0), (0, 1)], []),
    ("stranded_reverse_reverse_only", [(100, "10M50N10M", A20, 16, 60)], [(100, 110, 0, 0), (100, 110, 1, 1), (100, 110, 2, 2), (160, 170, 0, 0), (160, 170, 1, 1), (160, 170, 2, 2)],
     [[], [], []], 2, [(0, 1), (0, 1), (0, 0)], []),
    ("the_set_among_several_rows", [SPLICED], [(100, 110, 0, 0), (160, 170, 0, 0)], [[3, 7, 8]], 0, [(0, 0)], [(0, 0), (1, 0), (0, 0)]),
    ("the_set_is_no_row", [SPLICED], [(100, 110, 0, 0), (160, 170, 0, 0)], [[3, 6, 8]], 0, [(0, 1)], [(0, 0), (0, 0), (0, 0)]),
    ("untagged_read", [(100, "10M50N10M", "AAGAAAAAAAAAAAAAAAAA", 0, 60)], [(100, 110, 0, 0), (160, 170, 0, 0)], [[7]], 0, [(1, 0)], [(0, 0)]),
    ("mapq_0_and_supplementary_do_not_count", [(100, "10M50N10M", A20, 0, 0), (100, "10M50N10M", A20, 2048, 60), SPLICED], [(100, 110, 0, 0), (160, 170, 0, 0)], [[7]], 0,
     [(0, 0)], [(1, 0)]),
]


def hand_inputs(case):
    """(ReadSet, phase table, HAP_INTERVAL_DTYPE array, n_groups, group_row_off, row_ps, stranded, expected group_counts, expected row_counts)
    of one entry of HAND."""
    from clair3_rna_amd.reads import ReadSet
    _, reads, intervals, rows, stranded, gc, wc = case
    rs = ReadSet.from_records([dict(pos=r[0], cigar=r[1], seq=r[2], flag=r[3], mapq=r[4], hp=0) for r in reads])
    tab, off, row_ps = pack(intervals, rows)
    return (rs, hapref.make_sites(HR.HAND_SITES), tab, len(rows), off, row_ps, stranded, np.array(gc, dtype=np.uint32).reshape(len(gc), 2),
            np.array(wc, dtype=np.uint32).reshape(len(wc), 2))


def singletons(regions):
    """A HAP_REGION_DTYPE array as the interval table in which every interval is a group of its own -> (intervals, n_groups, group_row_off)."""
    a = np.zeros(len(regions), dtype=HAP_INTERVAL_DTYPE)
    a["start"], a["end"], a["strand"], a["group"] = regions["start"], regions["end"], regions["strand"], np.arange(len(regions))
    return a, len(regions), regions["row_off"].astype(np.int32)


# ---- the fuzz tables of tests/test_gpu_hapgroup.py
def fuzz_table(seed, grouping, table, L=6000):
    """The exons of phaseref.gen_case(seed) (hapregionref.phase_case_exons) grouped — `triples`: exons 3 g, 3 g + 1, 3 g + 2 are gene g;
    `interleaved`: the even exons are one gene, the odd ones another — plus five random intervals as groups of their own, sorted by
    (start, end); strand by group number; rows by the driver's policy.  -> (intervals, n_groups, group_row_off, row_ps)."""
    import random
    rng = random.Random(7919 * seed + 3)
    exons = HR.phase_case_exons(seed, L)
    if grouping == "triples":
        group_of = [k // 3 for k in range(len(exons))]
    else:
        assert grouping == "interleaved"
        group_of = [k % 2 for k in range(len(exons))]
    n_groups = max(group_of) + 1
    ivs = [(a, b, group_of[k], (1, 2, 0)[group_of[k] % 3]) for k, (a, b) in enumerate(exons)]
    for _ in range(5):
        ln = rng.choice((1, rng.randint(2, 50), rng.randint(50, 600), rng.randint(2000, 5000)))
        start = rng.randrange(0, L - ln)
        ivs.append((start, start + ln, n_groups, rng.choice((0, 0, 1, 2))))
        n_groups += 1
    ivs.sort(key=lambda e: (e[0], e[1]))
    return (n_groups,) + pack(ivs, group_rows(ivs, n_groups, table))


# ---- the drivers: hap_expr --group_by_name on hapregionref.driver_sample with a BED that names exons by gene
GENE_BED = {
    # geneA: three lines, two of which overlap and one abuts them -> [100, 900) and [2000, 2600); geneB (-): two disjoint exons; `.`: each
    # line a group of its own; geneMixed: + and - lines -> no strand (one [WARNING]); geneA again after other names: still the same group
    "chr1": [(100, 400, "geneA", "+"), (3000, 3300, "geneB", "-"), (300, 700, "geneA", "+"), (500, 501, ".", None), (700, 900, "geneA", "+"),
             (1000, 1200, "geneMixed", "+"), (4000, 4500, "geneB", "-"), (2000, 2600, "geneA", "+"), (600, 650, ".", "+"), (1500, 1800, "geneMixed", "-")],
    "chr2": [(10, 900, "g2", "+"), (1000, 1100, "g2", "+")],
    "chrEmpty": [(1, 2, "nothing", None)],
    "chrOther": [(1, 2, "unknown", None)],
}


def write_gene_bed(fn, bed=GENE_BED):
    with open(fn, "w") as f:
        for ctg in ("chr2", "chr1", "chrEmpty", "chrOther"):
            for start, end, name, strand in bed[ctg]:
                f.write("%s\t%d\t%d\t%s\t0\t%s\n" % (ctg, start, end, name, strand or "."))
            if ctg == "chr1":
                f.write("chr1\t700\t700\tgeneA\t0\t+\n")      # end <= start: skipped


def grouped(lines):
    """BED lines [(start, end, name, strand)] -> [(name, strand or None, [(start, end)] merged and sorted)] in order of first appearance, by
    the driver's policy, written out independently of it: same name, same group (`.`: alone); overlapping or abutting intervals merged;
    the strand if all lines agree, else none."""
    out, at = [], {}
    for start, end, name, strand in lines:
        if name == "." or name not in at:
            if name != ".":
                at[name] = len(out)
            out.append([name, {strand}, [(start, end)]])
        else:
            out[at[name]][1].add(strand)
            out[at[name]][2].append((start, end))
    res = []
    for name, strands, ivs in out:
        merged = []
        for a, b in sorted(ivs):
            if merged and a <= merged[-1][1]:
                merged[-1] = (merged[-1][0], max(merged[-1][1], b))
            else:
                merged.append((a, b))
        res.append((name, strands.pop() if len(strands) == 1 else None, merged))
    return res


def predicted_lines(s, ctg, bed=GENE_BED, stranded=0, params=DEFAULT_PARAMS, table=None):
    """The contig's lines of hap_expr --group_by_name from the restatement alone."""
    table = s["case"][ctg] if table is None else table
    groups = grouped(bed[ctg])
    ivs = sorted(((a, b, g, STRAND[strand]) for g, (_n, strand, merged) in enumerate(groups) for a, b in merged), key=lambda e: (e[0], e[1]))
    rows = group_rows(ivs, len(groups), table)
    tab, off, row_ps = pack(ivs, rows)
    gc, wc = counts(s["reads"][ctg], table, tab, len(groups), off, row_ps, stranded, params)
    lines, r = [], 0
    for g, (name, strand, merged) in enumerate(groups):
        head = "%s\t%d\t%d\t%s\t%s\t%d\t%d" % (ctg, merged[0][0], merged[-1][1], name, strand or ".", len(merged), sum(b - a for a, b in merged))
        lines.append(head + "\t.\t.\t.\t%d\t%d" % (gc[g, 0], gc[g, 1]))
        for ps in rows[g]:
            lines.append(head + "\t%d\t%d\t%d\t.\t." % (ps, wc[r, 0], wc[r, 1]))
            r += 1
    return lines


def uncounted_lines(ctg, bed=GENE_BED):
    return ["%s\t%d\t%d\t%s\t%s\t%d\t%d\t.\t.\t.\t.\t." % (ctg, m[0][0], m[-1][1], name, strand or ".", len(m), sum(b - a for a, b in m)) for name, strand, m in grouped(bed[ctg])]
