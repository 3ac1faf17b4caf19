"""The per-haplotype allele counts of include/c3r.h (c3r_get_read_phase_sets / c3r_hap_counts / c3r_hap_assign) and hap_vcf's nearest-set
rule restated in plain Python: one read at a time, one base at a time, dicts.  It shares nothing with csrc/hapcount_kernels.hpp,
c3r_hap_assign or hap_vcf.nearest_sets — no searches of a sorted table, no lanes, no arrays of indices — and is what the tests compare
them with.  A read's tag and phase set come from hapref.tag_read's per-set tally.  Its own behaviour is pinned by the hand-derived cases
of tests/test_hapcount_ref.py."""
import numpy as np

from clair3_rna_amd.capi import PHASE_SITE_DTYPE
from tests import hapref
from tests import phaseref

DEFAULT_PARAMS = phaseref.DEFAULT_PARAMS
STAT_KEYS = ("n_sites", "n_phased", "n_few_reads", "n_disagree")


def make_query(rows):
    """[(pos, ref letter, alt letter, ps)] -> PHASE_SITE_DTYPE array with h1 = 0 (as given: the caller sorts)."""
    return hapref.make_sites([(p, r, a, 0, ps) for p, r, a, ps in rows])


def read_tag_and_set(rs, i, by_pos):
    """(hp, phase set the tag was decided in or -1 when hp is 0) of read i; by_pos: {1-based pos: table site}."""
    hp, _, _, tally = hapref.tag_read(rs, i, by_pos)
    if hp == 0:
        return 0, -1
    # most votes; equal: the set whose first voting site comes first on the read
    best = max(tally.items(), key=lambda kv: (kv[1][0] + kv[1][1], -kv[1][2]))
    return hp, best[0]


def read_phase_sets(rs, table):
    """int32[n]: every read's phase set, -1 where its tag is 0."""
    by_pos = {int(s["pos"]): s for s in table}
    return np.array([read_tag_and_set(rs, i, by_pos)[1] for i in range(len(rs))], dtype=np.int32).reshape(len(rs))


def observe(rs, i, query_at):
    """{query index: column 0 (ref) / 1 (alt) / 2 (another of A, C, G, T)} of read i; query_at: {1-based pos: (index, site)}."""
    r = rs.reads[i]
    x, y = int(r["pos"]), 0                                  # 0-based reference cursor, query cursor
    seen = {}
    for k in range(int(r["n_cigar"])):
        c = int(rs.cigar[int(r["cigar_off"]) + k])
        op, ln = "MIDNSHP=X"[c & 15], c >> 4
        if op in "M=X":
            for d in range(ln):
                hit = query_at.get(x + d + 1)
                q = y + d
                if hit is None or q >= int(r["l_seq"]):
                    continue
                byte = int(rs.seq[int(r["seq_off"]) + q // 2])
                b = byte & 15 if q % 2 else byte >> 4
                if b not in (1, 2, 4, 8):
                    continue
                j, s = hit
                seen[j] = 0 if b == int(s["ref"]) else 1 if b == int(s["alt"]) else 2
            x += ln
            y += ln
        elif op in "DN":
            x += ln
        elif op in "IS":
            y += ln
    return seen


def hap_counts(rs, table, query, params=DEFAULT_PARAMS):
    """uint32 (n, 3, 3): [j][row][column] over the reads that pass the filters; row = the read's tag where its phase set is query j's ps,
    else 0."""
    by_pos = {int(s["pos"]): s for s in table}
    query_at = {int(s["pos"]): (j, s) for j, s in enumerate(query)}
    out = np.zeros((len(query), 3, 3), dtype=np.uint32)
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], params):
            continue
        hp, ps = read_tag_and_set(rs, i, by_pos)
        for j, col in observe(rs, i, query_at).items():
            row = hp if hp and ps == int(query[j]["ps"]) else 0
            out[j, row, col] += 1
    return out


def assign(query, counts, min_reads=2, min_agree_pct=75):
    """(sites with ps kept and h1 set where the tagged reads agree, ps = -1 and h1 = 0 elsewhere; stats dict like capi.hap_assign)."""
    out = np.array(query, dtype=PHASE_SITE_DTYPE, copy=True)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["n_sites"] = len(query)
    for j in range(len(query)):
        t = [[int(v) for v in row] for row in counts[j]]     # Python integers: no width
        v1, v0 = t[1][1] + t[2][0], t[1][0] + t[2][1]
        w = v0 + v1
        out[j]["reserved"] = 0
        if w < min_reads:
            st["n_few_reads"] += 1
        elif v0 == v1 or 100 * max(v0, v1) < min_agree_pct * w:
            st["n_disagree"] += 1
        else:
            st["n_phased"] += 1
            out[j]["h1"] = 1 if v1 > v0 else 0
            continue
        out[j]["ps"], out[j]["h1"] = -1, 0
    return out, st


def nearest_sets(cands, table):
    """Candidates with the ps of the nearest table site by position; at equal distance the one before."""
    out = np.array(cands, dtype=PHASE_SITE_DTYPE, copy=True)
    for j in range(len(out)):
        p = int(out[j]["pos"])
        best = None
        for s in table:                                      # in table order: a later site replaces an earlier one only when it is nearer
            d = abs(int(s["pos"]) - p)
            if best is None or d < best[0]:
                best = (d, int(s["ps"]))
        out[j]["ps"], out[j]["h1"] = best[1], 0
    return out
