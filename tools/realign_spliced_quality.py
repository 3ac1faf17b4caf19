#!/usr/bin/env python3
"""What --hap_realign_spliced changes beside the switched-off rule and beside --hap_realign alone (include/c3r.h:
c3r_set_hap_realign_spliced) — against a GENERATOR's truth, not real data, and no default is chosen from it: the default stays off.
Agreement with whatshap is NOT MEASURED.  Plain Python (tests/realignref.py and tests/realignspliceref.py, the restatements of the two
rules): no GPU.

    python tools/realign_spliced_quality.py [--commit ID] [--out profiles/realign_spliced_quality.txt] [--overhang 10]

The generator of tools/realign_quality.py (tests/leftalignref.gen_repeats(seed, jitter=True, errors=True), seeds 0-7; its reads are joined
over exons by N ops of their own) with its planted alignment errors — per (read, site) pair, with probability 0.25, one base deleted from or
inserted into the read inside an M op — of which a QUARTER is moved from "within 10 bases of the site" to "within W bases of one of the
read's exon edges" (the nearest edge to the site), where aligners misplace bases most often.  Three columns per seed:
    off   the rows and the reads as they are, CIGAR-position alleles;
    ra    --hap_realign W: the reads through the realigned observation, a window stops at an N;
    rs    --hap_realign W --hap_realign_spliced: the window counted in the read's spliced positions.
Per column, tools/left_align_quality.measure's figures — indel sites whose phase agrees with the truth, reads tagged against their
haplotype, switch errors — and for `ra` and `rs` the share of observations (a read that holds a site's anchor) that fell back to the
CIGAR-position rule, with the share of all observations that fell back because of an N op (ra: one touches [s, t]; rs: one holds a
position of the site's core)."""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))


def errors_near_sites_and_edges(rs, table, seed, W, p=0.25, reach=10, at_edges=0.25):
    """realign_quality.near_site_indels with a share `at_edges` of the planted errors moved to 1 .. W bases inside the exon from the read's
    N op nearest to the site (reads without an N op keep theirs near the site).  (read set, errors planted, of them at an exon edge)"""
    from clair3_rna_amd.reads import ReadSet
    from tests import hapalleleref as HA
    rng = random.Random(1000 + seed)
    anchors = [s["pos"] - 1 for s in table]
    recs, n_err, n_edge = [], 0, 0
    for i in range(len(rs)):
        r = rs.reads[i]
        ops = [[op, n] for op, n in HA.read_ops(rs, i)]
        seq = list(rs.read_bases(i, 0, int(r["l_seq"])))
        def landing(target):
            """(op index, offset in the op, query offset of the op) of the M op that holds `target` off its first and last base, or None"""
            x, y = int(r["pos"]), 0
            for k, (op, n) in enumerate(ops):
                if op in "M=X" and x < target < x + n - 1:
                    return k, target - x, y
                if op in "M=XDN":
                    x += n
                if op in "M=XIS":
                    y += n
            return None
        for a in anchors:
            if rng.random() >= p:
                continue
            at = landing(a + rng.choice((-1, 1)) * rng.randint(2, reach))
            if at is None:                                    # (realign_quality's: the read does not hold the place)
                continue
            edge = False
            if rng.random() < at_edges:                       # this error moves to the read's exon edge nearest to the site, when it has one
                x, edges = int(r["pos"]), []                  # (last position before an intron, first position behind it)
                for op, n in ops:
                    if op == "N":
                        edges += [(x - 1, -1), (x + n, 1)]
                    if op in "M=XDN":
                        x += n
                if edges:
                    e, inward = min(edges, key=lambda t: abs(t[0] - a))
                    moved = landing(e + inward * rng.randint(1, W))
                    if moved is not None:
                        at, edge = moved, True
            k, d, y = at
            op, n = ops[k]
            if rng.random() < 0.5:
                ops[k:k + 1] = [[op, d], ["D", 1], [op, n - d - 1]]
                del seq[y + d]
            else:
                ops[k:k + 1] = [[op, d], ["I", 1], [op, n - d]]
                seq.insert(y + d, rng.choice("ACGT"))
            n_err += 1
            n_edge += edge
        recs.append(dict(pos=int(r["pos"]), cigar="".join("%d%s" % (n, op) for op, n in ops), seq="".join(seq), flag=int(r["flag"]), mapq=int(r["mapq"]), hp=int(r["hp"])))
    out = ReadSet.from_records(recs)
    assert [int(v) for v in out.reads["pos"]] == [int(v) for v in rs.reads["pos"]]              # (the order, and so `hap`, is kept)
    return out, n_err, n_edge


def fallbacks(rs, table, ref, W):
    """(observations, ra: fell back, ra: because an N op touches [s, t], rs: fell back, rs: because an N op holds a position of the core)"""
    from tests import realignref as RR
    from tests import realignspliceref as RS
    n = ra_back = ra_n = rs_back = rs_n = 0
    for i in range(len(rs)):
        sp = RS.spliced(rs, i)
        cov = (sp[1], None)
        for site in table:
            if not RR.anchored(rs, i, site, cov):
                continue
            n += 1
            p0, D, _, s, t = RR.window(site, W)
            if RR.realigned_window(rs, i, ref, site, W, (sp[1], max(sp[0]) + 1)) is None:
                ra_back += 1
                ra_n += any(sp[1].get(p, ("-",))[0] == "N" for p in range(s, t + 1))
            if RS.spliced_window(rs, i, ref, site, W, sp) is None:
                rs_back += 1
                rs_n += any(sp[1].get(p, ("-",))[0] == "N" for p in range(p0, p0 + D + 1))
    return n, ra_back, ra_n, rs_back, rs_n


def case(seed, W):
    import left_align_quality as Q
    from realign_quality import memo
    from tests import hapalleleref as HA
    from tests import leftalignref as LA
    from tests import realignref as RR
    from tests import realignspliceref as RS
    ref, rs, rows, truth, planted, hap = LA.gen_repeats(seed, True, errors=True)
    table, is_snv = LA.table_of_case(rows, truth, planted)
    rs, n_err, n_edge = errors_near_sites_and_edges(rs, table, seed, W)
    return (dict(off=Q.measure(rs, hap, table, is_snv, memo(HA.observe)), ra=Q.measure(rs, hap, table, is_snv, memo(RR.observer((0, ref), W))),
                 rs=Q.measure(rs, hap, table, is_snv, memo(RS.observer((0, ref), W)))), fallbacks(rs, table, (0, ref), W), (n_err, n_edge))


def main():
    import phase_time
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "realign_spliced_quality.txt"))
    ap.add_argument("--overhang", type=int, default=10)
    a = ap.parse_args()
    lines = ["== realign_spliced_quality: commit %s, overhang %d; a GENERATOR's result (tests/leftalignref.gen_repeats(seed, jitter=True, errors=True): 403 reads a seed over "
             "exons joined by N ops, 5 %% substitutions, 1 %% N, an indel of 1-3 every ~60 bases; plus one inserted or deleted base for a quarter of the (read, site) pairs, three "
             "quarters of them within 10 bases of the site and a quarter within %d bases of the read's exon edge nearest to the site), by the restatements tests/realignref.py "
             "and tests/realignspliceref.py on the CPU.  Not real data; no default is chosen from it: the default stays off; agreement with whatshap: NOT MEASURED"
             % (a.commit or phase_time.commit_id(), a.overhang, a.overhang),
             "   seed  switch  indel sites  phased  agree  SNV switch errors  reads tagged  wrong  REF votes by carriers"]
    total = {k: [0] * 7 for k in ("off", "ra", "rs")}
    fb, planted = [0] * 5, [0, 0]

    def fallback_line(head, f):
        pct = lambda x: 100.0 * x / max(1, f[0])
        return ("%s%d observations; ra: %d fell back (%.1f %%), %d of them because an N op touches the window (%.1f %% of all); rs: %d fell back (%.1f %%), %d of them because an N "
                "op holds a position of the core (%.1f %% of all)" % (head, f[0], f[1], pct(f[1]), f[2], pct(f[2]), f[3], pct(f[3]), f[4], pct(f[4])))
    for seed in range(8):
        got, f, e = case(seed, a.overhang)
        fb = [x + y for x, y in zip(fb, f)]
        planted = [x + y for x, y in zip(planted, e)]
        for name in ("off", "ra", "rs"):
            total[name] = [t + v for t, v in zip(total[name], got[name])]
            lines.append("   %4d  %-6s  %11d  %6d  %5d  %17d  %12d  %5d  %21d" % ((seed, name) + got[name]))
        lines.append(fallback_line("         %d errors planted, %d of them at an exon edge; " % e, f))
        print("\n".join(lines[-4:]), flush=True)
    for name in ("off", "ra", "rs"):
        lines.append("   all   %-6s  %11d  %6d  %5d  %17d  %12d  %5d  %21d" % ((name,) + tuple(total[name])))
    lines.append(fallback_line("   all   %d errors planted, %d of them at an exon edge; " % tuple(planted), fb))
    print("\n".join(lines[-4:]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
