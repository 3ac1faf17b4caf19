#!/usr/bin/env python3
"""What --hap_realign changes beside the switched-off rule and beside --left_align_indels (include/c3r.h: c3r_set_hap_realign) — against a
GENERATOR's truth, not real data, and no default is chosen from it: the default stays off.  Agreement with whatshap is NOT MEASURED.
Plain Python (tests/realignref.py and tests/leftalignref.py, the restatements of the two rules): no GPU.

    python tools/realign_quality.py [--commit ID] [--out profiles/realign_quality.txt] [--overhang 10]

The generator of tools/left_align_quality.py with its read-error setting (tests/leftalignref.gen_repeats(seed, jitter=True, errors=True),
seeds 0-7), plus alignment errors near the sites: for every (read, site) pair, with probability 0.25, one base within 10 bases of the site is
deleted from or inserted into the read inside an M op (near_site_indels below).  Three columns per seed:
    off   the rows and the reads as they are, CIGAR-position alleles;
    la    --left_align_indels: the table through align_sites, the reads through the left-aligned observation;
    ra    --hap_realign W: the rows as they are, the reads through the realigned observation.
Per column, tools/left_align_quality.measure's figures — indel sites whose phase agrees with the truth, reads tagged against their
haplotype, votes for REF by reads that carry the event, switch errors — and for `ra` the share of observations (a read that holds a site's
anchor) that fell back to the CIGAR-position rule, with the share of all observations that fell back because an N op touches the window."""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))


def near_site_indels(rs, table, seed, p=0.25, reach=10):
    """The read set with, per (read, site the read covers) and probability p, one base deleted or inserted at a reference position 2 .. reach
    bases from the site's anchor, where that position lies inside an M op (not on its first or last base)."""
    from clair3_rna_amd.reads import CIGAR_OPS, ReadSet
    from tests import hapalleleref as HA
    rng = random.Random(1000 + seed)
    anchors = [s["pos"] - 1 for s in table]
    recs = []
    for i in range(len(rs)):
        r = rs.reads[i]
        ops = [[op, n] for op, n in HA.read_ops(rs, i)]
        seq = list(rs.read_bases(i, 0, int(r["l_seq"])))
        for a in anchors:
            if rng.random() >= p:
                continue
            target = a + rng.choice((-1, 1)) * rng.randint(2, reach)
            x, y = int(r["pos"]), 0
            for k, (op, n) in enumerate(ops):
                if op in "M=X" and x < target < x + n - 1:
                    d = target - x
                    if rng.random() < 0.5:
                        ops[k:k + 1] = [[op, d], ["D", 1], [op, n - d - 1]]
                        del seq[y + d]
                    else:
                        ops[k:k + 1] = [[op, d], ["I", 1], [op, n - d]]
                        seq.insert(y + d, rng.choice("ACGT"))
                    break
                if op in "M=XDN":
                    x += n
                if op in "M=XIS":
                    y += n
        recs.append(dict(pos=int(r["pos"]), cigar="".join("%d%s" % (n, op) for op, n in ops), seq="".join(seq), flag=int(r["flag"]), mapq=int(r["mapq"]), hp=int(r["hp"])))
    out = ReadSet.from_records(recs)
    assert [int(v) for v in out.reads["pos"]] == [int(v) for v in rs.reads["pos"]]              # (the order, and so `hap`, is kept)
    return out


def fallbacks(rs, table, ref, W):
    """(observations, fell back, fell back because an N op touches [s, t])"""
    from tests import hapalleleref as HA
    from tests import realignref as RR
    n = back = by_n = 0
    for i in range(len(rs)):
        cov = RR.cover(HA.read_ops(rs, i), int(rs.reads[i]["pos"]))
        for site in table:
            if not RR.anchored(rs, i, site, cov):
                continue
            n += 1
            if RR.realigned_window(rs, i, ref, site, W, cov) is None:
                back += 1
                _, _, _, s, t = RR.window(site, W)
                by_n += any(cov[0].get(p, ("-",))[0] == "N" for p in range(s, t + 1))
    return n, back, by_n


def memo(obs):
    seen = {}

    def once(rs, i, site_at):
        if i not in seen:
            seen[i] = obs(rs, i, site_at)
        return seen[i]
    return once


def case(seed, W):
    import left_align_quality as Q
    from tests import hapalleleref as HA
    from tests import leftalignref as LA
    from tests import realignref as RR
    ref, rs, rows, truth, planted, hap = LA.gen_repeats(seed, True, errors=True)
    t_jit, is_snv = LA.table_of_case(rows, truth, planted)
    rs = near_site_indels(rs, t_jit, seed)
    t_on, src, _, _ = LA.align_sites(t_jit, (ref, 0))
    return dict(off=Q.measure(rs, hap, t_jit, is_snv, memo(HA.observe)),
                la=Q.measure(rs, hap, t_on, [is_snv[j] for j in src], memo(LA.observer((ref, 0)))),
                ra=Q.measure(rs, hap, t_jit, is_snv, memo(RR.observer((0, ref), W)))), fallbacks(rs, t_jit, (0, ref), W)


def main():
    import phase_time
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "realign_quality.txt"))
    ap.add_argument("--overhang", type=int, default=10)
    a = ap.parse_args()
    lines = ["== realign_quality: commit %s, overhang %d; a GENERATOR's result (tests/leftalignref.gen_repeats(seed, jitter=True, errors=True): 403 reads a seed, 5 %% "
             "substitutions, 1 %% N, an indel of 1-3 every ~60 bases; plus one inserted or deleted base within 10 bases of a site for a quarter of the (read, site) pairs), "
             "by the restatements tests/realignref.py and tests/leftalignref.py on the CPU.  Not real data; no default is chosen from it: the default stays off; "
             "agreement with whatshap: NOT MEASURED" % (a.commit or phase_time.commit_id(), a.overhang),
             "   seed  switch  indel sites  phased  agree  SNV switch errors  reads tagged  wrong  REF votes by carriers"]
    total = {k: [0] * 7 for k in ("off", "la", "ra")}
    fb = [0, 0, 0]
    for seed in range(8):
        got, f = case(seed, a.overhang)
        fb = [x + y for x, y in zip(fb, f)]
        for name in ("off", "la", "ra"):
            total[name] = [t + v for t, v in zip(total[name], got[name])]
            lines.append("   %4d  %-6s  %11d  %6d  %5d  %17d  %12d  %5d  %21d" % ((seed, name) + got[name]))
        lines.append("         ra: %d observations, %d fell back (%.1f %%), %d of them because an N op touches the window (%.1f %% of all)"
                     % (f[0], f[1], 100.0 * f[1] / max(1, f[0]), f[2], 100.0 * f[2] / max(1, f[0])))
        print("\n".join(lines[-4:]), flush=True)
    for name in ("off", "la", "ra"):
        lines.append("   all   %-6s  %11d  %6d  %5d  %17d  %12d  %5d  %21d" % ((name,) + tuple(total[name])))
    lines.append("   all   ra: %d observations, %d fell back (%.1f %%), %d because an N op touches the window (%.1f %% of all)"
                 % (fb[0], fb[1], 100.0 * fb[1] / max(1, fb[0]), fb[2], 100.0 * fb[2] / max(1, fb[0])))
    print("\n".join(lines[-4:]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
