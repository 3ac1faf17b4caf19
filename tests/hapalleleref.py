"""The allele rule of include/c3r.h (c3r_hap_allele_counts: SNVs, insertions, deletions and two-ALT rows) restated in plain Python: one read at
a time, one base at a time, strings and dicts, with its own CIGAR normalisation written from the comment at csrc/reads_kernels.hpp.  It
shares no code with csrc/hapcount_kernels.hpp, phasing.py or hap_vcf.py and is what the tests compare them with.  A read's tag and phase set
come from hapcountref (the restatement of the tagging).  Its own behaviour is pinned by the hand-derived cases of
tests/test_hapallele_ref.py.

A site here is a dict: pos (1-based), ps, A and B — each (base letter, event), event = ("none",) / ("ins", letters) / ("del", n) — and the
row's ref / alt strings; base_matters / event_matters are derived where they are needed.

gen_case(seed, errors) builds two-haplotype read sets with planted heterozygous insertions and deletions and a few 1/2 sites."""
import random

import numpy as np

from clair3_rna_amd.capi import HAP_SITE_DTYPE
from clair3_rna_amd.reads import ReadSet
from tests import hapcountref as HC
from tests import phaseref

LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}
CODE = {"A": 1, "C": 2, "G": 4, "T": 8}
NONE = ("none",)
REASONS = ("other_contig", "malformed", "not_pass", "not_snv", "not_het", "duplicate_pos", "multi_alt", "complex_allele", "same_alleles")


# ---- alleles of a row
def reduce(ref, alt):
    """(base letter, event) of one ALT against REF, or None when the pair is not an SNV, an insertion or a deletion anchored on POS."""
    r, a = ref.upper(), alt.upper()
    if r == "" or a == "" or any(c not in "ACGT" for c in r + a):
        return None
    while len(r) > 1 and len(a) > 1 and r[-1] == a[-1]:
        r, a = r[:-1], a[:-1]
    if len(r) == 1 and len(a) == 1:
        return (a, NONE) if a != r else None
    if len(r) == 1 and a.startswith(r):
        return (r, ("ins", a[1:]))
    if len(a) == 1 and r.startswith(a):
        return (r[0], ("del", len(r) - 1))
    return None


def site_of_row(pos, ref, alt, gt, ps=0):
    """The site of one PASS row, or the reason it is skipped for."""
    alts = alt.split(",")
    if gt in ("0/1", "1/0"):
        if len(alts) != 1:
            return "multi_alt"
        b = reduce(ref, alts[0])
        if b is None:
            return "complex_allele"
        return dict(pos=pos, ps=ps, A=(ref[0].upper(), NONE), B=b, ref=ref, alt=alt)
    if gt in ("1/2", "2/1"):
        if len(alts) < 2:
            return "not_het"
        if len(alts) > 2:
            return "multi_alt"
        a, b = reduce(ref, alts[0]), reduce(ref, alts[1])
        if a is None or b is None:
            return "complex_allele"
        if a == b:
            return "same_alleles"
        return dict(pos=pos, ps=ps, A=a, B=b, ref=ref, alt=alt)
    return "not_het"


def flags(site):
    """(base_matters, event_matters): one of the two alleles is an SNV / an insertion or deletion.  An SNV is an allele without an event whose
    base is not the reference's, and the reference base is the anchor base of every indel allele and of the REF allele."""
    ref_base = site["ref"][0].upper()
    return (any(ev == NONE and base != ref_base for base, ev in (site["A"], site["B"])),
            any(ev != NONE for _, ev in (site["A"], site["B"])))


def candidates(lines, contig):
    """(sites sorted by pos, {reason: rows skipped}) of `contig`'s rows of a VCF's lines."""
    skipped = dict.fromkeys(REASONS, 0)
    kept = []
    for line in lines:
        if line.startswith("#") or not line.strip():
            continue
        f = line.rstrip("\r\n").split("\t")
        if f[0] != contig:
            skipped["other_contig"] += 1
            continue
        if len(f) < 10 or not f[1].isdigit() or int(f[1]) < 1:
            skipped["malformed"] += 1
            continue
        if f[6] != "PASS":
            skipped["not_pass"] += 1
            continue
        fmt = dict(zip(f[8].split(":"), f[9].split(":")))
        s = site_of_row(int(f[1]), f[3], f[4], fmt.get("GT", ""))
        if isinstance(s, str):
            skipped[s] += 1
            continue
        kept.append(s)
    out, seen = [], set()
    for s in sorted(kept, key=lambda s: s["pos"]):           # (stable: rows of one position stay in file order)
        if s["pos"] in seen:
            skipped["duplicate_pos"] += 1
            continue
        seen.add(s["pos"])
        out.append(s)
    return out, skipped


# ---- one read at one site
def normalise(ops):
    """[(op letter, length)] of a read -> its normalised form: H, empty ops and pads dropped — a pad survives (as P of length 1) only when the
    next real op is a D and the op kept before it is not an I —, = and X folded into M, equal neighbours merged."""
    out = []
    for k, (op, n) in enumerate(ops):
        if op in "=X":
            op = "M"
        if n == 0 or op == "H":
            continue
        if op == "P":
            real = [o for o, m in ops[k + 1:] if m > 0 and o not in "PH"]
            if not real or real[0] != "D" or (out and out[-1][0] == "I"):
                continue
            n = 1
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + n)
        else:
            out.append((op, n))
    return out


def read_ops(rs, i):
    r = rs.reads[i]
    return [("MIDNSHP=X"[int(c) & 15], int(c) >> 4) for c in rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]]


def code_at(rs, i, q):
    byte = int(rs.seq[int(rs.reads[i]["seq_off"]) + q // 2])
    return byte & 15 if q % 2 else byte >> 4


def observe(rs, i, site_at):
    """{site index: column 0 (allele A) / 1 (allele B) / 2 (anything else)} of read i; site_at: {1-based pos: (index, site)}."""
    ops = normalise(read_ops(rs, i))
    l_seq = int(rs.reads[i]["l_seq"])
    x, y = int(rs.reads[i]["pos"]), 0
    seen = {}
    for k, (op, n) in enumerate(ops):
        if op == "M":
            for d in range(n):
                hit = site_at.get(x + d + 1)
                if hit is None or y + d >= l_seq:
                    continue
                j, site = hit
                b = code_at(rs, i, y + d)
                base_matters, event_matters = flags(site)
                event = NONE                                  # (not looked at where no allele of the site is an indel)
                if event_matters and d == n - 1 and k + 1 < len(ops):
                    nop, nlen = ops[k + 1]
                    if nop == "I":
                        if k + 2 < len(ops) and ops[k + 2][0] == "D":
                            event = ("other",)
                        elif y + n + nlen > l_seq:
                            continue                          # the insertion is cut off by a short SEQ: no observation
                        else:
                            event = ("ins", tuple(code_at(rs, i, y + n + t) for t in range(nlen)))
                    elif nop == "D":
                        event = ("del", nlen)
                if base_matters and b not in (1, 2, 4, 8):
                    continue
                col = 2
                for c, (base, ev) in ((1, site["B"]), (0, site["A"])):      # (A last: it wins where both would match)
                    if ev[0] == "ins":
                        ev = ("ins", tuple(CODE[t] for t in ev[1]))
                    if (not base_matters or b == CODE[base]) and (not event_matters or event == ev):
                        col = c
                seen[j] = col
            x, y = x + n, y + n
        elif op in "DN":
            x += n
        elif op in "IS":
            y += n
    return seen


def counts(rs, table, sites, params=HC.DEFAULT_PARAMS):
    """uint32 (n, 3, 3): [j][row][column] over the reads that pass the filters; row = the read's tag where its phase set is site j's ps,
    else 0."""
    by_pos = {int(s["pos"]): s for s in table}
    site_at = {s["pos"]: (j, s) for j, s in enumerate(sites)}
    out = np.zeros((len(sites), 3, 3), dtype=np.uint32)
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], params):
            continue
        hp, ps = HC.read_tag_and_set(rs, i, by_pos)
        for j, col in observe(rs, i, site_at).items():
            out[j, hp if hp and ps == sites[j]["ps"] else 0, col] += 1
    return out


def assign(sites, table, min_reads=2, min_agree_pct=75):
    """[(ps or -1, h1)] per site from its (3, 3) counts: A on haplotype 1 and B on haplotype 2 speak for h1 = 0 (GT A|B), the other two
    for h1 = 1 (GT B|A)."""
    out = []
    for s, t in zip(sites, table):
        v1, v0 = int(t[1][1]) + int(t[2][0]), int(t[1][0]) + int(t[2][1])
        w = v0 + v1
        ok = w >= min_reads and v0 != v1 and 100 * max(v0, v1) >= min_agree_pct * w
        out.append((s["ps"], 1 if v1 > v0 else 0) if ok else (-1, 0))
    return out


def nearest_sets(sites, table):
    """The sites with the ps of the nearest table site by position; at equal distance the one before."""
    out = []
    for s in sites:
        best = None
        for t in table:
            d = abs(int(t["pos"]) - s["pos"])
            if best is None or d < best[0]:
                best = (d, int(t["ps"]))
        out.append(dict(s, ps=best[1]))
    return out


def gt_text(site, decided):
    """The GT of a site after assign: phased A|B / B|A, else unphased."""
    a, b = ("1", "2") if "," in site["alt"] else ("0", "1")
    ps, h1 = decided
    return a + "/" + b if ps < 0 else (b + "|" + a if h1 else a + "|" + b)


def rewritten(line, site, decided):
    """The VCF row of an accepted site as the writer must leave it: GT replaced, PS appended."""
    f = line.rstrip("\n").split("\t")
    keys, vals = f[8].split(":"), f[9].split(":")
    vals[keys.index("GT")] = gt_text(site, decided)
    return "\t".join(f[:8] + [f[8] + ":PS", ":".join(vals) + ":%d" % decided[0]]) + "\n"


def counts_line(contig, site, decided, t):
    a, b = ("1", "2") if "," in site["alt"] else ("0", "1")
    return "\t".join([contig, str(site["pos"]), site["ref"], site["alt"], str(site["ps"]), gt_text(site, decided)]
                     + [str(int(t[r][c])) for r in (1, 2, 0) for c in (0, 1, 2)] + [a + "," + b]) + "\n"


# ---- the engine's form of a list of sites
def to_query(sites, lead=0):
    """(HAP_SITE_DTYPE array, packed pool) of a list of sites; `lead` bases (A) go into the pool first, which moves every insertion's
    offset."""
    q = np.zeros(len(sites), dtype=HAP_SITE_DTYPE)
    pool = [1] * lead
    for k, s in enumerate(sites):
        q[k]["pos"], q[k]["ps"] = s["pos"], s["ps"]
        q[k]["base_matters"], q[k]["event_matters"] = [int(v) for v in flags(s)]
        for name in "ab":
            base, ev = s[name.upper()]
            q[k][name + "_base"] = CODE[base]
            q[k][name + "_kind"] = ("none", "ins", "del").index(ev[0])
            if ev[0] == "ins":
                q[k][name + "_len"], q[k][name + "_ins_off"] = len(ev[1]), len(pool)
                pool += [CODE[c] for c in ev[1]]
            elif ev[0] == "del":
                q[k][name + "_len"] = ev[1]
    pool += [0] * (len(pool) % 2)
    packed = np.array([pool[k] << 4 | pool[k + 1] for k in range(0, len(pool), 2)], dtype=np.uint8)
    return q, packed


def snv_sites(query, ref_of=None):
    """PHASE_SITE_DTYPE query sites (REF / ALT single bases) as sites of this module."""
    return [dict(pos=int(s["pos"]), ps=int(s["ps"]), A=(LETTER[int(s["ref"])], NONE), B=(LETTER[int(s["alt"])], NONE),
                 ref=LETTER[int(s["ref"])], alt=LETTER[int(s["alt"])]) for s in query]


# ---- random cases
def gen_case(seed, errors=False, L=6000, n_reads=403, n_snv=120, n_indel=36, n_two=10, n_exons=12):
    """(ref, ReadSet, SNV table rows [(pos, ref, alt)], their truth h1, planted sites (dicts with ref / alt / gt and `truth`: 1 when
    haplotype 1 carries allele B), source haplotype per read).  phaseref.gen_case's reads — exons joined by N ops, soft clips, 12 % failing
    the filters, errors: 5 % substitutions, 1 % N, an indel of 1-3 every ~60 bases — with, beside the SNVs, heterozygous insertions and
    deletions of 1-6 bases (GT 0/1) and a few 1/2 sites (two SNVs, two insertions, two deletions, an indel and an SNV) on the two
    haplotypes, every planted site at least 9 bases from the next variant and from its exon's end."""
    rng = random.Random(7000 + seed)
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    cuts = sorted(rng.sample(range(60, L - 60), 2 * n_exons))
    exons = [(cuts[2 * e], cuts[2 * e + 1]) for e in range(n_exons) if cuts[2 * e + 1] - cuts[2 * e] >= 8]
    room = [p for a, b in exons for p in range(a + 1, b - 9)]
    taken, planted = set(), []

    def other(b):
        return rng.choice([c for c in "ACGT" if c != b])

    def allele(kind, rb):
        if kind == "snv":
            return (other(rb), "", 0)
        n = rng.randint(1, 6)
        return (rb, "".join(rng.choice("ACGT") for _ in range(n)), 0) if kind == "ins" else (rb, "", n)

    for k in range(n_indel + n_two):
        free = [p for p in room if all(abs(p - t) > 9 for t in taken)]
        if not free:
            break
        p0 = rng.choice(free)
        taken.add(p0)
        rb = ref[p0]
        if k < n_indel:
            pair = [(rb, "", 0), allele(rng.choice(("ins", "del")), rb)]
            gt = "0/1"
        else:
            while True:
                pair = [allele(rng.choice(("snv", "ins", "del")), rb) for _ in range(2)]
                if pair[0] != pair[1]:
                    break
            gt = "1/2"
        span = max(a[2] for a in pair)
        vref = ref[p0:p0 + 1 + span]
        alts = [a[0] + a[1] + ref[p0 + 1 + a[2]:p0 + 1 + span] for a in pair]
        planted.append(dict(pos=p0 + 1, ref=vref, alt=",".join(alts[1:] if gt == "0/1" else alts), gt=gt, truth=rng.randint(0, 1), pair=pair))
    planted.sort(key=lambda s: s["pos"])
    snv_room = [p for a, b in exons for p in range(a, b) if all(p < t - 1 or p > t + 8 for t in taken)]
    rows, truth = [], []
    for p0 in sorted(rng.sample(snv_room, min(n_snv, len(snv_room)))):
        rows.append((p0 + 1, ref[p0], other(ref[p0])))
        truth.append(rng.randint(0, 1))
    smap = {r[0]: (r, t) for r, t in zip(rows, truth)}
    pmap = {s["pos"]: s for s in planted}
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
        run = 0
        for step in range(n_ex):
            end = exons[e][1] if step + 1 < n_ex else rng.randrange(x + 1, exons[e][1] + 1)
            while x < end:
                b, event = ref[x], None
                if x + 1 in smap:
                    (_, rb, ab), h1 = smap[x + 1]
                    b = ab if (h1 == 1) == (hap == 1) else rb
                elif x + 1 in pmap:
                    s = pmap[x + 1]
                    b, ins, dele = s["pair"][1 if (s["truth"] == 1) == (hap == 1) else 0]      # haplotype 1 carries B where the truth is 1
                    event = (ins, dele)
                if errors:
                    u = rng.random()
                    if u < 0.05:
                        b = rng.choice("ACGT")
                    elif u < 0.06:
                        b = "N"
                seq.append(b)
                x += 1
                run += 1
                if event and (event[0] or event[1]) and x + event[1] + 1 < end:
                    cig.append("%dM" % run)
                    run = 0
                    if event[0]:
                        cig.append("%dI" % len(event[0]))
                        seq += list(event[0])
                    else:
                        cig.append("%dD" % event[1])
                        x += event[1]
                elif errors and run >= 2 and x + 4 < end and rng.random() < 1 / 60.0:
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
    return ref, ReadSet.from_records(recs), rows, np.array(truth, np.uint8), planted, np.array([r["truth"] for r in recs], np.uint8)


def planted_sites(planted):
    """The planted sites of gen_case as sites of this module (ps = 0)."""
    out = []
    for p in planted:
        s = site_of_row(p["pos"], p["ref"], p["alt"], p["gt"])
        assert not isinstance(s, str), (p, s)
        out.append(s)
    return out
