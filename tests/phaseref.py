"""The phasing rule of include/c3r.h (c3r_phase_links / c3r_phase_resolve) restated in plain Python: one read at a time, one base at a
time, dicts of observations and of votes.  It shares nothing with csrc/phase_kernels.hpp or c3r_phase_resolve — no searches of a sorted
table, no windows, no lanes, no fixed-size arrays — and is what the tests compare both with.  Its own behaviour is pinned by the
hand-derived cases of tests/test_phaseref.py.

gen_case(seed) builds the random two-haplotype spliced read sets of the CPU and GPU tests."""
import random

import numpy as np

from clair3_rna_amd.capi import PHASE_SITE_DTYPE
from clair3_rna_amd.reads import ReadSet

K = 8                                                        # C3R_PHASE_LINKS
CODE = {"A": 1, "C": 2, "G": 4, "T": 8}
DEFAULT_PARAMS = dict(min_mq=5, excl_flags=2316)             # c3r_default_params
STAT_KEYS = ("n_sites", "n_phased", "n_blocks", "max_block")


def make_sites(rows):
    """[(pos, ref letter, alt letter)] -> unphased PHASE_SITE_DTYPE array (as given: the caller sorts)."""
    a = np.zeros(len(rows), dtype=PHASE_SITE_DTYPE)
    for k, r in enumerate(rows):
        a[k] = (r[0], 0, CODE[r[1]], CODE[r[2]], 0, 0)
    return a


def votes(read, params):
    """The read is one the tensor build keeps: none of the excluded flag bits, mapped, no anomalous pair, MAPQ at least min_mq."""
    flag, excl = int(read["flag"]), int(params["excl_flags"])
    if flag & excl or flag & 4 or (flag & 1 and not flag & 2):
        return False
    return int(read["mapq"]) >= int(params["min_mq"])


def observe(rs, i, index_of, sites):
    """{site index: allele 0 / 1} of read i; index_of: {1-based pos: site index}."""
    r = rs.reads[i]
    x, y = int(r["pos"]), 0                                  # 0-based reference cursor, query cursor
    seen = {}
    for k in range(int(r["n_cigar"])):
        c = int(rs.cigar[int(r["cigar_off"]) + k])
        op, ln = "MIDNSHP=X"[c & 15], c >> 4
        if op in "M=X":
            for d in range(ln):
                j = index_of.get(x + d + 1)
                q = y + d
                if j is None or q >= int(r["l_seq"]):
                    continue
                byte = int(rs.seq[int(r["seq_off"]) + q // 2])
                b = byte & 15 if q % 2 else byte >> 4
                if b == int(sites[j]["ref"]):
                    seen[j] = 0
                elif b == int(sites[j]["alt"]):
                    seen[j] = 1
            x += ln
            y += ln
        elif op in "DN":
            x += ln
        elif op in "IS":
            y += ln
    return seen


def links(rs, sites, params=DEFAULT_PARAMS):
    """uint32 (n, K, 2): [j][k - 1][0] voting reads that show sites j and j - k with the same allele index, [1] with different ones."""
    index_of = {int(s["pos"]): j for j, s in enumerate(sites)}
    out = np.zeros((len(sites), K, 2), dtype=np.uint32)
    for i in range(len(rs)):
        if not votes(rs.reads[i], params):
            continue
        seen = observe(rs, i, index_of, sites)
        for j, a in seen.items():
            for k in range(1, K + 1):
                if j - k in seen:
                    out[j, k - 1, 0 if seen[j - k] == a else 1] += 1
    return out


def resolve(sites, lk, min_reads=2, min_agree_pct=75):
    """(sites with ps / h1 filled in, stats dict like capi.phase_resolve)."""
    n = len(sites)
    block, h1, members = [], [], []                          # per site: block number, orientation; per block: its sites
    for j in range(n):
        tally = {}                                           # block -> [v0, v1, distance of its nearest member]
        for k in range(1, K + 1):
            i = j - k
            if i < 0:
                break
            cis, trans = int(lk[j][k - 1][0]), int(lk[j][k - 1][1])
            t = tally.setdefault(block[i], [0, 0, k])
            t[1] += cis if h1[i] else trans
            t[0] += trans if h1[i] else cis
        ok = [(abs(v1 - v0), -near, b) for b, (v0, v1, near) in tally.items()
              if v0 + v1 >= min_reads and v0 != v1 and 100 * max(v0, v1) >= min_agree_pct * (v0 + v1)]
        if ok:
            b = max(ok)[2]                                   # (distances differ between blocks: the block number never decides)
            block.append(b)
            h1.append(1 if tally[b][1] > tally[b][0] else 0)
            members[b].append(j)
        else:
            block.append(len(members))
            h1.append(0)
            members.append([j])
    out = np.array(sites, dtype=PHASE_SITE_DTYPE, copy=True)
    for j in range(n):
        m = members[block[j]]
        out[j]["ps"] = int(sites[m[0]]["pos"]) if len(m) >= 2 else -1
        out[j]["h1"] = h1[j] if len(m) >= 2 else 0
        out[j]["reserved"] = 0
    big = [len(m) for m in members if len(m) >= 2]
    st = dict(n_sites=n, n_phased=sum(big), n_blocks=len(big), max_block=max([len(m) for m in members] or [0]))
    return out, st


def equal_sites(a, b):
    """Field for field."""
    return all(a[f].tolist() == b[f].tolist() for f in ("pos", "ps", "ref", "alt", "h1", "reserved"))


def phase(rs, sites, params=DEFAULT_PARAMS, min_reads=2, min_agree_pct=75):
    return resolve(sites, links(rs, sites, params), min_reads, min_agree_pct)


# ---- random cases
def gen_case(seed, L=6000, n_reads=403, n_sites=120, errors=False, n_exons=12):
    """(ref, ReadSet, unphased site array, truth h1 per site, source haplotype 1 / 2 per read): a random reference cut into n_exons exons
    with introns of 20-300 between them; n_sites heterozygous SNVs inside the exons, each with a random alt and a random truth h1; reads
    drawn from one of the two haplotypes, each starting inside an exon and running through 1-5 exons joined by N ops, 15 % of them
    skipping one exon on the way, 30 % with a leading soft clip.  errors: ONT-like — 5 % substitutions, 1 % N, a deletion or an insertion
    of 1-3 every ~60 bases — else none.  12 % of the reads fail the default filters (MAPQ below 5, secondary, supplementary, unmapped,
    an anomalous pair); their bases are drawn like the others'.  The read count is kept off the multiples of 16."""
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    # exons: [start, end) 0-based, in order
    cuts = sorted(rng.sample(range(60, L - 60), 2 * n_exons))
    exons = [(cuts[2 * e], cuts[2 * e + 1]) for e in range(n_exons) if cuts[2 * e + 1] - cuts[2 * e] >= 8]
    inside = [p for a, b in exons for p in range(a, b)]
    rows, truth = [], []
    for p0 in sorted(rng.sample(inside, min(n_sites, len(inside)))):
        rb = ref[p0]
        rows.append((p0 + 1, rb, rng.choice([b for b in "ACGT" if b != rb])))
        truth.append(rng.randint(0, 1))
    smap = {r[0]: (r, t) for r, t in zip(rows, truth)}
    recs = []
    while len(recs) < n_reads:
        hap = rng.randint(1, 2)
        e = rng.randrange(len(exons))
        x = rng.randrange(exons[e][0], exons[e][1])
        p0, cig, seq = x, [], []
        if rng.random() < 0.3:
            n = rng.randint(1, 20)
            cig.append("%dS" % n)
            seq += [rng.choice("ACGT") for _ in range(n)]
        n_ex = rng.randint(1, 5)
        skipped = rng.random() >= 0.15
        run = 0                                              # aligned bases since the last non-M op
        for step in range(n_ex):
            end = exons[e][1] if step + 1 < n_ex else rng.randrange(x + 1, exons[e][1] + 1)
            while x < end:
                b = ref[x]
                if x + 1 in smap:
                    (_, rb, ab), h1 = smap[x + 1]
                    b = ab if (h1 == 1) == (hap == 1) else rb          # haplotype 1 carries ALT where the truth is 1|0
                if errors:
                    u = rng.random()
                    if u < 0.05:
                        b = rng.choice("ACGT")
                    elif u < 0.06:
                        b = "N"
                seq.append(b)
                x += 1
                run += 1
                if errors and run >= 2 and x + 4 < end and rng.random() < 1 / 60.0:
                    cig.append("%dM" % run)
                    run = 0
                    n = rng.randint(1, 3)
                    if rng.random() < 0.5:
                        cig.append("%dD" % n)
                        x += n
                    else:
                        cig.append("%dI" % n)
                        seq += [rng.choice("ACGT") for _ in range(n)]
            if run:
                cig.append("%d%s" % (run, rng.choice("=X") if rng.random() < 0.1 else "M"))
                run = 0
            if step + 1 == n_ex:
                break
            nxt = e + 1
            if not skipped and nxt + 1 < len(exons):
                nxt, skipped = e + 2, True
            if nxt >= len(exons):
                break
            cig.append("%dN" % (exons[nxt][0] - x))
            x, e = exons[nxt][0], nxt
        flag, mapq = 16 * rng.randint(0, 1), 60
        if rng.random() < 0.12:
            u = rng.randrange(5)
            if u == 0:
                mapq = rng.randint(0, 4)
            else:
                flag |= (256, 2048, 4, 1)[u - 1]
        recs.append(dict(pos=p0, cigar="".join(cig), seq="".join(seq), flag=flag, mapq=mapq, hp=0, truth=hap))
    if len(recs) % 16 == 0:
        recs.pop()
    recs.sort(key=lambda r: r["pos"])
    return ref, ReadSet.from_records(recs), make_sites(rows), np.array(truth, np.uint8), np.array([r["truth"] for r in recs], np.uint8)
