"""The block-merge stage of include/c3r.h (c3r_phase_unit_links / c3r_phase_merge) restated in plain Python: one read at a time, one base at
a time, dicts.  It takes the observation rule, the voters, the chain's resolution and the read model from tests/phaseref.py and nothing from
the library or from csrc/phase_kernels.hpp — no unit_of array, no walks per unit, no bit masks.  Its own behaviour is pinned by the
hand-derived cases of tests/test_phasemerge_ref.py.

gen_fragmented(seed, run) is phaseref.gen_case's read model plus two runs of RNA-editing sites, the input that cuts the chain's blocks."""
import random

import numpy as np

from tests.phaseref import DEFAULT_PARAMS, K, gen_case, make_sites, observe, resolve, votes

PHASE_SITE_DTYPE = make_sites([]).dtype


def units_of(sites):
    """The distinct ps >= 0 of the table in increasing order: unit u is the block whose ps is units_of(sites)[u]."""
    return sorted({int(s["ps"]) for s in sites if int(s["ps"]) >= 0})


def unit_links(rs, sites, params=DEFAULT_PARAMS):
    """uint32 (U, K, 2): [u][k - 1][0] voting reads that show unit u and unit u - k with the same haplotype, [1] with different ones."""
    units = units_of(sites)
    number = {ps: u for u, ps in enumerate(units)}
    index_of = {int(s["pos"]): j for j, s in enumerate(sites)}
    out = np.zeros((len(units), K, 2), dtype=np.uint32)
    for i in range(len(rs)):
        if not votes(rs.reads[i], params):
            continue
        count = {}                                           # unit -> [c1, c2]
        for j, allele in observe(rs, i, index_of, sites).items():
            if int(sites[j]["ps"]) < 0:
                continue
            c = count.setdefault(number[int(sites[j]["ps"])], [0, 0])
            c[0 if allele == int(sites[j]["h1"]) else 1] += 1
        shown = {u: (1 if c[0] > c[1] else 2) for u, c in count.items() if c[0] != c[1]}
        for u, h in shown.items():
            for k in range(1, K + 1):
                if u - k in shown:
                    out[u, k - 1, 0 if shown[u - k] == h else 1] += 1
    return out


def table_stats(sites):
    """The statistics of a table, counted from it: a block is a ps >= 0."""
    size = {}
    for s in sites:
        if int(s["ps"]) >= 0:
            size[int(s["ps"])] = size.get(int(s["ps"]), 0) + 1
    alone = any(int(s["ps"]) < 0 for s in sites)
    return dict(n_sites=len(sites), n_phased=sum(size.values()), n_blocks=len(size), max_block=max(list(size.values()) + ([1] if alone else [0])))


def merge(sites, ulinks, min_reads=2, min_agree_pct=75):
    """One level: (table, its statistics, units that joined)."""
    units = units_of(sites)
    assert len(ulinks) == len(units)
    pseudo = make_sites([(ps, "A", "C") for ps in units])
    res, _ = resolve(pseudo, ulinks, min_reads, min_agree_pct)
    new = {ps: (int(r["ps"]), int(r["h1"])) for ps, r in zip(units, res) if int(r["ps"]) >= 0}
    out = np.array(sites, dtype=PHASE_SITE_DTYPE, copy=True)
    for j in range(len(out)):
        hit = new.get(int(out[j]["ps"]))
        if hit is not None:
            out[j]["ps"], out[j]["h1"] = hit[0], int(out[j]["h1"]) ^ hit[1]
        out[j]["reserved"] = 0
    return out, table_stats(out), sum(1 for ps, (ps2, _) in new.items() if ps2 != ps)


def merge_levels(rs, sites, levels, params=DEFAULT_PARAMS, min_reads=2, min_agree_pct=75):
    """Levels until one joins nothing or `levels` have run, on a chain's table: (table, statistics, levels run, units joined)."""
    out, st, run, joined = sites, table_stats(sites), 0, 0
    while run < levels:
        out, st, n = merge(out, unit_links(rs, out, params), min_reads, min_agree_pct)
        run += 1
        joined += n
        if n == 0:
            break
    return out, st, run, joined


def phase(rs, sites, lk, levels, params=DEFAULT_PARAMS, min_reads=2, min_agree_pct=75):
    """The chain on the site link table lk (phaseref.links), then the levels: (table, statistics, with merge_levels_run /
    merge_units_joined when levels > 0)."""
    out, st = resolve(sites, lk, min_reads, min_agree_pct)
    if levels > 0:
        out, st, run, joined = merge_levels(rs, out, levels, params, min_reads, min_agree_pct)
        st = dict(st, merge_levels_run=run, merge_units_joined=joined)
    return out, st


# ---- the fragmenting input
def gen_fragmented(seed, run=9, n_reads=403, at=(20, 60), p_alt=0.3):
    """gen_case(seed, errors=True) with `run` editing sites put into the table before each of its indices `at` (run = 0: none): positions
    inside exons that carry no SNV, the nearest free ones at or after the SNV of that index, each with alt = the base every read shows
    with probability p_alt whatever its haplotype (drawn per read and site, after the read's own errors).
    -> (ref, ReadSet, unphased site array, truth h1 per site (0 for an editing site), set of table indices of the editing sites)."""
    from clair3_rna_amd.reads import ReadSet
    ref, rs, sites, truth, _ = gen_case(seed, n_reads=n_reads, errors=True)
    rng = random.Random(7700 + seed)
    taken = {int(s["pos"]) for s in sites}
    # positions some read covers with an M-like op: the exons, as the reads show them
    covered = set()
    edit = {}                                                # 1-based pos -> (ref letter, alt letter)
    for i in range(len(rs)):
        r = rs.reads[i]
        x = int(r["pos"])
        for k in range(int(r["n_cigar"])):
            c = int(rs.cigar[int(r["cigar_off"]) + k])
            op, ln = "MIDNSHP=X"[c & 15], c >> 4
            if op in "M=X":
                covered.update(range(x + 1, x + ln + 1))
            if op in "MDN=X":
                x += ln
    if run:
        for a in at:
            p, got = int(sites[min(a, len(sites) - 1)]["pos"]) + 1, 0
            while got < run and p <= len(ref):
                if p in covered and p not in taken and p not in edit:
                    rb = ref[p - 1]
                    edit[p] = (rb, {"A": "G", "C": "T", "G": "A", "T": "C"}[rb])
                    got += 1
                p += 1
    # rewrite the reads' bases on the editing sites
    code = {"A": 1, "C": 2, "G": 4, "T": 8}
    seq = rs.seq.copy()
    for i in range(len(rs)):
        r = rs.reads[i]
        x, y = int(r["pos"]), 0
        for k in range(int(r["n_cigar"])):
            c = int(rs.cigar[int(r["cigar_off"]) + k])
            op, ln = "MIDNSHP=X"[c & 15], c >> 4
            if op in "M=X":
                for d in range(ln):
                    e = edit.get(x + d + 1)
                    q = y + d
                    if e is None or q >= int(r["l_seq"]):
                        continue
                    at_byte = int(r["seq_off"]) + q // 2
                    old = int(seq[at_byte])
                    cur = old & 15 if q % 2 else old >> 4
                    if cur not in (code[e[0]], code[e[1]]):
                        continue                             # (a sequencing error or an N stays)
                    b = code[e[1]] if rng.random() < p_alt else code[e[0]]
                    seq[at_byte] = (old & 0xF0) | b if q % 2 else (b << 4) | (old & 15)
                x += ln
                y += ln
            elif op in "DN":
                x += ln
            elif op in "IS":
                y += ln
    rows = sorted([(int(s["pos"]), "ACGT"[(1, 2, 4, 8).index(int(s["ref"]))], "ACGT"[(1, 2, 4, 8).index(int(s["alt"]))], int(t)) for s, t in zip(sites, truth)]
                  + [(p, e[0], e[1], -1) for p, e in edit.items()])
    table = make_sites([r[:3] for r in rows])
    editing = {j for j, r in enumerate(rows) if r[3] < 0}
    truth2 = np.array([max(r[3], 0) for r in rows], np.uint8)
    return ref, ReadSet(rs.reads.copy(), rs.cigar, seq), table, truth2, editing


def quality(out, truth, editing):
    """Of a phased table against the truth: dict(phased = sites in a block, blocks = blocks that hold a true SNV, switches = (errors, pairs)
    over adjacent true SNVs of one block, editing = editing sites in a block)."""
    blocks = {}
    for j in range(len(out)):
        if int(out[j]["ps"]) >= 0 and j not in editing:
            blocks.setdefault(int(out[j]["ps"]), []).append(j)
    err = pairs = 0
    for members in blocks.values():
        for a, b in zip(members, members[1:]):
            pairs += 1
            if (int(out[a]["h1"]) ^ int(truth[a])) != (int(out[b]["h1"]) ^ int(truth[b])):
                err += 1
    return dict(phased=int(sum(1 for s in out if int(s["ps"]) >= 0)), blocks=len(blocks), switches=(err, pairs),
                editing=sum(1 for j in editing if int(out[j]["ps"]) >= 0))
