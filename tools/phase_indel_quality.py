#!/usr/bin/env python3
"""What indel and two-ALT sites add to the phasing between the passes (include/c3r.h: c3r_phase_allele_links against c3r_phase_links) —
against a GENERATOR's truth, not real data: it shows what the greedy chain does with links it used to have no sites for, not how good the
phase of a real sample is.  Agreement with `whatshap phase --indels` is NOT MEASURED (the tool is on none of our machines).  Plain Python
(tests/phaseindelref.py, the restatement of the rule): no GPU.

    python tools/phase_indel_quality.py [--commit ID] [--out profiles/phase_indel_quality.txt]

tests/hapalleleref.gen_case(seed, errors=True), seeds 0-7: 403 reads over 6 kb — exons joined by N ops, 5 % substitutions, 1 % N, an indel
of 1-3 every ~60 bases — from two haplotypes that differ at 120 SNVs, 36 insertions and deletions of 1-6 bases and 10 two-ALT sites.  The
SNV-only chain (phaseref: what phase_vcf does) against the chain over SNVs + planted sites (phase_vcf --indels), both with the defaults
(min_reads 2, min_agree_pct 75, no merge level).  `sparse`: every fourth SNV only.  Per seed, all against the generator's truth:
    among the true SNVs: phased, blocks that hold one, switch errors between neighbouring SNVs of one block (errors / pairs);
    indel and 1/2 sites: phased, agreeing with the orientation of the nearest phased SNV of their block, disagreeing (no SNV in the block:
    neither);
    the reads tagged afterwards from the phased table (tests/hapindelref.haplotag), and those tagged against the generator's haplotype —
    per block the orientation is fixed by the majority of its sites, so a block phased consistently upside down counts as right."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))


def case(seed, every):
    from tests import hapalleleref as HA
    from tests import phaseindelref as PI
    _, rs, rows, truth, planted, hap = HA.gen_case(seed, errors=True)
    keep = list(zip(rows, truth))[::every]
    sites, tr, is_snv = PI.table_of_case([r for r, _ in keep], [t for _, t in keep], planted)
    return rs, hap, sites, tr, is_snv


def measure(rs, hap, sites, truth, is_snv, ps, h1):
    """(SNVs phased, blocks with an SNV, switch errors, pairs, other sites phased, agreeing, disagreeing, reads tagged, tagged wrong)"""
    from tests import hapindelref as HI
    blocks = {}
    for j, p in enumerate(ps):
        if p >= 0:
            blocks.setdefault(p, []).append(j)
    n_snv = n_blocks = err = pairs = n_other = agree = disagree = 0
    flip = {}
    for p, members in blocks.items():
        snvs = [j for j in members if is_snv[j]]
        n_snv += len(snvs)
        n_blocks += 1 if snvs else 0
        for a, b in zip(snvs, snvs[1:]):
            pairs += 1
            err += (h1[a] ^ truth[a]) != (h1[b] ^ truth[b])
        rel = [h1[j] ^ truth[j] for j in members]
        flip[p] = 1 if 2 * sum(rel) > len(rel) else 0
        for j in members:
            if is_snv[j]:
                continue
            n_other += 1
            if snvs:
                near = min(snvs, key=lambda s: (abs(s - j), s))
                if (h1[j] ^ truth[j]) == (h1[near] ^ truth[near]):
                    agree += 1
                else:
                    disagree += 1
    table = [dict(s, ps=ps[j], h1=h1[j]) for j, s in enumerate(sites) if ps[j] >= 0]
    tagged = wrong = 0
    if table:
        hp, _, sets = HI.haplotag(rs, table)
        for i in range(len(rs)):
            if hp[i]:
                tagged += 1
                wrong += (int(hp[i]) if not flip[int(sets[i])] else 3 - int(hp[i])) != int(hap[i])
    return n_snv, n_blocks, err, pairs, n_other, agree, disagree, tagged, wrong


def main():
    import phase_time
    from tests import phaseindelref as PI
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_indel_quality.txt"))
    a = ap.parse_args()
    lines = ["== phase_indel_quality: commit %s; a GENERATOR's result (tests/hapalleleref.gen_case(seed, errors=True), 403 reads a seed), by the restatement "
             "tests/phaseindelref.py on the CPU.  Not real data; agreement with `whatshap phase --indels`: NOT MEASURED" % (a.commit or phase_time.commit_id())]
    head = "SNVs phased  blocks  switches/pairs  other phased  agree  disagree  reads tagged  wrong"
    worse = []
    for label, every in (("every SNV", 1), ("sparse: every fourth SNV", 4)):
        lines.append("-- %s" % label)
        lines.append("   seed  SNVs/other   SNV-only chain: %s   |  SNV + indel chain: %s" % (head, head))
        total = [0] * 18
        for seed in range(8):
            rs, hap, sites, truth, is_snv = case(seed, every)
            snv_idx = [j for j in range(len(sites)) if is_snv[j]]
            only = [sites[j] for j in snv_idx]
            ps0, h0, _ = PI.phase(rs, only)
            m0 = measure(rs, hap, only, [truth[j] for j in snv_idx], [True] * len(only), ps0, h0)
            ps1, h1, _ = PI.phase(rs, sites)
            m1 = measure(rs, hap, sites, truth, is_snv, ps1, h1)
            if m1[2] > m0[2]:
                worse.append((label, seed, m0[2], m1[2]))
            total = [t + v for t, v in zip(total, m0 + m1)]
            fmt = "%11d  %6d  %8d/%-5d  %12d  %5d  %8d  %12d  %5d"
            lines.append(("   %4d  %4d/%-5d                  " + fmt + "   |                     " + fmt) % ((seed, len(only), len(sites) - len(only)) + m0 + m1))
        lines.append(("   all                              " + fmt + "   |                     " + fmt) % tuple(total))
        if total[11] > total[2]:
            lines.append("   REGRESSION over the eight seeds: the SNV + indel chain makes %d switch errors between neighbouring SNVs, the SNV-only chain %d" % (total[11], total[2]))
    for label, seed, s0, s1 in worse:
        lines.append("   more switch errors with the indel sites than without, %s, seed %d: %d against %d" % (label, seed, s1, s0))
    if not worse:
        lines.append("   no seed has more switch errors between neighbouring SNVs with the indel sites than without")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
