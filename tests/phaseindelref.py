"""The phasing over an allele table (include/c3r.h: c3r_phase_allele_links / c3r_phase_allele_unit_links) restated in plain Python.  The header
states that rule as the join of two others, and so does this file: the observation is hapalleleref.observe (one read, one base at a time,
its own CIGAR normalisation) with the columns 0 / 1 kept and column 2 dropped, the voters are phaseref.votes, the chain is phaseref.resolve
on the pseudo-table (pos, A>C) of the sites, and the unit rule is phasemergeref's — majority per unit, a tie is nothing, links to the K unit
numbers before — with that observation in the place of the nibble compare.  Nothing is shared with csrc/phase_kernels.hpp, capi.py or
phase_vcf.py.

A site is hapalleleref's dict (pos, ps, A, B, ref, alt); a resolved table is the list of those dicts with ps and one more key, h1 (0: allele A
lies on haplotype 1)."""
import numpy as np

from tests import hapalleleref as HA
from tests import phasemergeref as PM
from tests import phaseref

K = phaseref.K


def seen_of(rs, i, site_at):
    """{site index: allele index 0 / 1} of read i: hapalleleref.observe without column 2."""
    return {j: c for j, c in HA.observe(rs, i, site_at).items() if c in (0, 1)}


def links(rs, sites, params=phaseref.DEFAULT_PARAMS):
    """uint32 (n, K, 2): phaseref.links' sums over the allele observation."""
    site_at = {s["pos"]: (j, s) for j, s in enumerate(sites)}
    out = np.zeros((len(sites), K, 2), dtype=np.uint32)
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], params):
            continue
        seen = seen_of(rs, i, site_at)
        for j, a in seen.items():
            for k in range(1, K + 1):
                if j - k in seen:
                    out[j, k - 1, 0 if seen[j - k] == a else 1] += 1
    return out


def pseudo(sites, ps=None, h1=None):
    """The pseudo-table the chain and the merge read: pos, A>C, and ps / h1 when given."""
    t = phaseref.make_sites([(s["pos"], "A", "C") for s in sites])
    if ps is not None:
        t["ps"], t["h1"] = ps, h1
    return t


def resolve(sites, lk, min_reads=2, min_agree_pct=75):
    """(int ps per site, int h1 per site, stats): phaseref.resolve on the pseudo-table."""
    out, st = phaseref.resolve(pseudo(sites), lk, min_reads, min_agree_pct)
    return [int(v) for v in out["ps"]], [int(v) for v in out["h1"]], st


def unit_links(rs, sites, ps, h1, params=phaseref.DEFAULT_PARAMS):
    """uint32 (U, K, 2): phasemergeref.unit_links' rule over the allele observation; ps / h1 per site as the chain leaves them."""
    units = sorted({p for p in ps if p >= 0})
    number = {p: u for u, p in enumerate(units)}
    site_at = {s["pos"]: (j, s) for j, s in enumerate(sites)}
    out = np.zeros((len(units), K, 2), dtype=np.uint32)
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], params):
            continue
        count = {}
        for j, allele in seen_of(rs, i, site_at).items():
            if ps[j] < 0:
                continue
            c = count.setdefault(number[ps[j]], [0, 0])
            c[0 if allele == h1[j] else 1] += 1
        shown = {u: (1 if c[0] > c[1] else 2) for u, c in count.items() if c[0] != c[1]}
        for u, h in shown.items():
            for k in range(1, K + 1):
                if u - k in shown:
                    out[u, k - 1, 0 if shown[u - k] == h else 1] += 1
    return out


def phase(rs, sites, levels=0, params=phaseref.DEFAULT_PARAMS, min_reads=2, min_agree_pct=75):
    """The chain, then up to `levels` merge levels: (ps per site, h1 per site, stats as Engine.phase_allele_sites gives them)."""
    ps, h1, st = resolve(sites, links(rs, sites, params), min_reads, min_agree_pct)
    if levels > 0:
        run = joined = 0
        while run < levels:
            out, st, n = PM.merge(pseudo(sites, ps, h1), unit_links(rs, sites, ps, h1, params), min_reads, min_agree_pct)
            ps, h1 = [int(v) for v in out["ps"]], [int(v) for v in out["h1"]]
            run += 1
            joined += n
            if n == 0:
                break
        st = dict(st, merge_levels_run=run, merge_units_joined=joined)
    return ps, h1, st


def table_of_case(rows, truth, planted):
    """(sites sorted by pos, truth per site — 1 when haplotype 1 carries allele B —, is the site an SNV row)."""
    ent = [(dict(pos=r[0], ps=0, A=(r[1], HA.NONE), B=(r[2], HA.NONE), ref=r[1], alt=r[2]), int(t), True) for r, t in zip(rows, truth)]
    ent += [(s, int(p["truth"]), False) for s, p in zip(HA.planted_sites(planted), planted)]
    ent.sort(key=lambda e: e[0]["pos"])
    return [e[0] for e in ent], [e[1] for e in ent], [e[2] for e in ent]


# ---- the hand-made bridge: SNV s1, a heterozygous 2-base deletion d, SNV s2; reads of one kind cover s1 + d, of the other d + s2, none s1 + s2
BRIDGE_REF = "ACGTACGTAC" * 12                                 # 120 bases; s1 at 1-based 21, d anchored at 61 (deletes 62-63), s2 at 101
BRIDGE_SITES = [dict(pos=21, ps=0, A=("A", HA.NONE), B=("G", HA.NONE), ref="A", alt="G"),
                dict(pos=61, ps=0, A=("A", HA.NONE), B=("A", ("del", 2)), ref="ACG", alt="A"),
                dict(pos=101, ps=0, A=("A", HA.NONE), B=("T", HA.NONE), ref="A", alt="T")]
BRIDGE_TRUTH = [1, 0, 1]                                       # haplotype 1 carries: s1 ALT, d REF, s2 ALT


def bridge_reads(per=6, only_d=2):
    """(ReadSet, source haplotype per read).  `per` reads a kind and haplotype: kind L covers 1-based 11 .. 80 (s1 and d), kind R covers
    51 .. 115 (d and s2); `only_d` reads a haplotype cover 51 .. 80 only (d and no SNV).  Haplotype h shows allele B of a site where
    (truth == 1) == (h == 1)."""
    def read(lo, hi, hap):                                     # 1-based closed
        seq, cig, run, x = [], [], 0, lo
        while x <= hi:
            b = BRIDGE_REF[x - 1]
            for s, t in zip(BRIDGE_SITES, BRIDGE_TRUTH):
                if s["pos"] == x and (t == 1) == (hap == 1):
                    b = s["B"][0]
            seq.append(b)
            run += 1
            x += 1
            if x - 1 == 61 and (BRIDGE_TRUTH[1] == 1) == (hap == 1):
                cig += ["%dM" % run, "2D"]
                run, x = 0, x + 2
        cig.append("%dM" % run)
        return dict(pos=lo - 1, cigar="".join(cig), seq="".join(seq), flag=0, mapq=60, hp=0, truth=hap)
    recs = []
    for hap in (1, 2):
        recs += [read(11, 80, hap) for _ in range(per)] + [read(51, 115, hap) for _ in range(per)] + [read(51, 80, hap) for _ in range(only_d)]
    recs.sort(key=lambda r: r["pos"])
    from clair3_rna_amd.reads import ReadSet
    return ReadSet.from_records(recs), [r["truth"] for r in recs]
