#!/usr/bin/env python3
"""What --left_align_indels changes for indels in homopolymers and short tandem repeats (include/c3r.h: c3r_set_hap_left_align) — against a
GENERATOR's truth, not real data: it shows what the rule does with reads and rows that place an indel anywhere in its repeat, not how good
the phasing of a real sample is.  Agreement with whatshap is NOT MEASURED (the tool is on none of our machines).  Plain Python
(tests/leftalignref.py, the restatement of the rule): no GPU.

    python tools/left_align_quality.py [--commit ID] [--out profiles/left_align_quality.txt]

tests/leftalignref.gen_repeats(seed, jitter=True), seeds 0-7, without and with read errors (5 % substitutions, 1 % N, an indel of 1-3 every
~60 bases): 403 reads over 6 kb from two haplotypes that differ at 100 SNVs and up to 36 insertions and deletions of whole repeat units.
Switch off: the rows and the reads as they are.  Switch on: the table through align_sites, the reads through the left-aligned observation.
Per seed:
    indel sites phased by the chain (c3r_phase_allele_links + c3r_phase_resolve), and of those the ones whose orientation agrees with the
        generator's truth (relative to the majority of their block);
    switch errors between neighbouring SNVs of one block;
    reads tagged from the generator's truth as the table, and tagged against their source haplotype;
    votes for REF: observations of allele A at a 0/1 indel site by reads (that pass the filters) of the haplotype that carries the event."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))


def measure(rs, hap, table, is_snv, obs):
    """(indel sites, phased, agreeing, switch errors, reads tagged, tagged wrong, REF votes by carriers)"""
    from tests import hapalleleref as HA
    from tests import leftalignref as LA
    from tests import phaseindelref as PI
    from tests import phaseref
    ps, h1, _ = PI.resolve(table, LA.links(rs, table, obs))
    blocks = {}
    for j, p in enumerate(ps):
        if p >= 0:
            blocks.setdefault(p, []).append(j)
    phased = agree = switches = 0
    for members in blocks.values():
        flip = [h1[j] ^ table[j]["h1"] for j in members]
        major = 1 if 2 * sum(flip) > len(flip) else 0
        indel = [f for j, f in zip(members, flip) if not is_snv[j]]
        phased += len(indel)
        agree += sum(1 for f in indel if f == major)
        snv = [f for j, f in zip(members, flip) if is_snv[j]]
        switches += sum(1 for a, b in zip(snv, snv[1:]) if a != b)
    hp, _, _ = LA.haplotag(rs, table, obs)
    tagged = hp > 0
    site_at = {s["pos"]: (j, s) for j, s in enumerate(table)}
    ref_votes = 0
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], phaseref.DEFAULT_PARAMS):
            continue
        for j, col in obs(rs, i, site_at).items():
            s = table[j]
            carrier = (s["h1"] == 1) == (int(hap[i]) == 1)                     # this read's haplotype carries allele B
            if not is_snv[j] and s["A"][1] == HA.NONE and carrier and col == 0:
                ref_votes += 1
    return (len(is_snv) - sum(is_snv), phased, agree, switches, int(tagged.sum()), int((hp != hap)[tagged].sum()), ref_votes)


def case(seed, errors):
    from tests import hapalleleref as HA
    from tests import leftalignref as LA
    ref, rs, rows, truth, planted, hap = LA.gen_repeats(seed, True, errors=errors)
    t_jit, is_snv = LA.table_of_case(rows, truth, planted)
    t_on, src, skipped, _ = LA.align_sites(t_jit, (ref, 0))
    off = measure(rs, hap, t_jit, is_snv, HA.observe)
    on = measure(rs, hap, t_on, [is_snv[j] for j in src], LA.observer((ref, 0)))
    return off, on, skipped


def main():
    import phase_time
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "left_align_quality.txt"))
    a = ap.parse_args()
    lines = ["== left_align_quality: commit %s; a GENERATOR's result (tests/leftalignref.gen_repeats(seed, jitter=True), 403 reads a seed, every indel in a "
             "homopolymer or a 2-3-base repeat, reads and rows at random equivalent placements), by the restatement tests/leftalignref.py on the CPU.  "
             "Not real data; agreement with whatshap: NOT MEASURED" % (a.commit or phase_time.commit_id())]
    worse = []
    for errors in (False, True):
        lines.append("-- read errors: %s" % ("5 %% substitutions, 1 %% N, an indel of 1-3 every ~60 bases" % () if errors else "none"))
        lines.append("   seed  switch  indel sites  phased  agree  SNV switch errors  reads tagged  wrong  REF votes by carriers")
        total = {"off": [0] * 7, "on": [0] * 7}
        for seed in range(8):
            off, on, skipped = case(seed, errors)
            for name, row in (("off", off), ("on", on)):
                total[name] = [t + v for t, v in zip(total[name], row)]
                lines.append("   %4d  %-6s  %11d  %6d  %5d  %17d  %12d  %5d  %21d" % ((seed, name) + row))
            if on[3] > off[3]:
                worse.append((errors, seed))
            if any(skipped.values()):
                lines.append("         (dropped by the table's left-alignment: %s)" % ", ".join("%s %d" % kv for kv in sorted(skipped.items()) if kv[1]))
        for name in ("off", "on"):
            lines.append("   all   %-6s  %11d  %6d  %5d  %17d  %12d  %5d  %21d" % ((name,) + tuple(total[name])))
    lines.append("-- condition: no seed has more SNV switch errors with the switch on than off: %s" % ("HOLDS" if not worse else "BROKEN for (errors, seed) %s" % worse))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
