"""The left-alignment rule of include/c3r.h (c3r_set_hap_left_align / c3r_hap_left_align_sites) restated in plain Python: strings, lists and
dicts, one shift at a time.  The observation is built on hapalleleref.normalise and laid out like hapalleleref.observe; the tags, the count
table and the link tables are the joins hapindelref and phaseindelref write, with the observation as an argument so that the same lines
serve the switch off (hapalleleref.observe) and on (observe of this file).  Nothing is shared with csrc/haplotag_kernels.hpp, c3r_lib.hip,
capi.py, phasing.py or phasedvcf.py.  Its own behaviour is pinned by the hand-derived cases of tests/test_leftalign_ref.py.

A reference here is (text, lo): text[0] is the 0-based position lo.  A site is hapalleleref's dict (pos, ps, A, B, ref, alt; h1 where tags
are made).

gen_repeats(seed, jitter) builds two-haplotype read sets whose planted indels all sit in homopolymers and short tandem repeats."""
import random

import numpy as np

from clair3_rna_amd.reads import ReadSet
from tests import hapalleleref as HA
from tests import hapcountref as HC
from tests import hapref
from tests import phaseref

K = phaseref.K
NEW_REASONS = ("not_left_alignable", "same_pos_after_left_align")


# ---- the rule
def base_at(ref, p):
    """The upper-case letter on 0-based position p when the slice holds an A, C, G or T there, else None."""
    text, lo = ref
    if p < lo or p >= lo + len(text):
        return None
    c = text[p - lo].upper()
    return c if c in "ACGT" else None


def left_align(ref, a, kind, n, s=""):
    """(k, s'): the shifts of an event behind 0-based anchor a — kind "del" with n bases, or "ins" with the letters s — and the rotated
    insertion.  One step: the base on the anchor equals the event's last base, both are A, C, G, T, and so is the base the anchor moves to."""
    k = 0
    s = s.upper()
    while True:
        on_anchor = base_at(ref, a - k)
        if on_anchor is None or base_at(ref, a - k - 1) is None:
            break
        last = s[-1] if kind == "ins" else base_at(ref, a - k + n)
        if last is None or last not in "ACGT" or last != on_anchor:
            break
        if kind == "ins":
            s = on_anchor + s[:-1]
        k += 1
    return k, s


# ---- the table
def align_sites(sites, ref):
    """(the sites that stay, sorted by pos; the input index of each; {reason: sites dropped}; sites moved)."""
    skipped = dict.fromkeys(NEW_REASONS, 0)
    kept, moved = [], 0
    for idx, site in enumerate(sites):
        base_matters, _ = HA.flags(site)
        shifts, new = [], {}
        for name in "AB":
            base, ev = site[name]
            if ev[0] == "none":
                new[name] = ev
                continue
            k, s = left_align(ref, site["pos"] - 1, ev[0], ev[1] if ev[0] == "del" else len(ev[1]), ev[1] if ev[0] == "ins" else "")
            shifts.append(k)
            new[name] = ("ins", s) if ev[0] == "ins" else ev
        k = shifts[0] if shifts else 0
        if any(v != k for v in shifts) or (k > 0 and base_matters):
            skipped["not_left_alignable"] += 1
            continue
        out = dict(site)
        if k > 0:
            anchor = base_at(ref, site["pos"] - 1 - k)
            # (`ref` gets the new anchor's letter in front, which is all hapalleleref.flags reads of it: no allele of a moved site is an SNV)
            out.update(pos=site["pos"] - k, A=(anchor, new["A"]), B=(anchor, new["B"]), ref=anchor + site["ref"][1:])
            moved += 1
        kept.append((out, idx))
    kept.sort(key=lambda e: (e[0]["pos"], e[1]))
    table, src, seen = [], [], set()
    for site, idx in kept:
        if site["pos"] in seen:
            skipped["same_pos_after_left_align"] += 1
            continue
        seen.add(site["pos"])
        table.append(site)
        src.append(idx)
    return table, src, skipped, moved


# ---- one read at one site, the events brought to their left-most place inside their M run
def observe(rs, i, site_at, ref):
    """{site index: column 0 / 1 / 2} of read i, like hapalleleref.observe; site_at: {1-based pos: (index, site)}."""
    ops = HA.normalise(HA.read_ops(rs, i))
    l_seq = int(rs.reads[i]["l_seq"])
    x, y = int(rs.reads[i]["pos"]), 0
    seen = {}
    for k, (op, n) in enumerate(ops):
        if op == "M":
            # the event behind this run and the offset in the run where it shows
            shown, at = HA.NONE, None
            cut = False
            if y + n - 1 < l_seq and k + 1 < len(ops):
                nop, nlen = ops[k + 1]
                if nop == "I" and k + 2 < len(ops) and ops[k + 2][0] == "D":
                    shown, at = ("other",), n - 1
                elif nop == "I" and y + n + nlen > l_seq:
                    cut, at = True, n - 1
                elif nop in "ID":
                    letters = "".join(HA.LETTER.get(HA.code_at(rs, i, y + n + t), "N") for t in range(nlen)) if nop == "I" else ""
                    shift, _ = left_align(ref, x + n - 1, "ins" if nop == "I" else "del", nlen, letters)
                    shift = min(shift, n - 1)                 # the cap: the anchor stays inside the run
                    letters = rotate(ref, x + n - 1, letters, shift)
                    shown = ("ins", tuple(HA.CODE.get(c, 15) for c in letters)) if nop == "I" else ("del", nlen)
                    at = n - 1 - shift
            for d in range(n):
                hit = site_at.get(x + d + 1)
                if hit is None or y + d >= l_seq:
                    continue
                j, site = hit
                b = HA.code_at(rs, i, y + d)
                base_matters, event_matters = HA.flags(site)
                event = HA.NONE
                if event_matters and d == at:
                    if cut:
                        continue
                    event = shown
                if base_matters and b not in (1, 2, 4, 8):
                    continue
                col = 2
                for c, (base, ev) in ((1, site["B"]), (0, site["A"])):
                    if ev[0] == "ins":
                        ev = ("ins", tuple(HA.CODE[t] for t in ev[1]))
                    if (not base_matters or b == HA.CODE[base]) and (not event_matters or event == ev):
                        col = c
                seen[j] = col
            x, y = x + n, y + n
        elif op in "DN":
            x += n
        elif op in "IS":
            y += n
    return seen


def rotate(ref, a, s, k):
    """s after k steps of the rule, whatever the rule says about a (k + 1)-th: s_k = (ref[a - k + 1 .. a] + s)[:len(s)]."""
    for j in range(k):
        s = base_at(ref, a - j) + s[:-1]
    return s


# ---- the four tables, with the observation as an argument: obs(rs, i, site_at) -> {index: column}
def observer(ref):
    """obs for the switch on."""
    return lambda rs, i, site_at: observe(rs, i, site_at, ref)


def tag_read(rs, i, sites, site_at, obs):
    """hapindelref.tag_read under obs: (hp, phase set or -1, votes)."""
    votes = sorted((j, c) for j, c in obs(rs, i, site_at).items() if c in (0, 1))
    if not votes:
        return 0, -1, 0
    pseudo = ReadSet.from_records([dict(pos=0, cigar="%dM" % len(votes), seq="".join("AC"[c] for _, c in votes), flag=0, mapq=60, hp=0)])
    by_pos = {k + 1: dict(pos=k + 1, ref=1, alt=2, h1=sites[j]["h1"], ps=sites[j]["ps"]) for k, (j, _) in enumerate(votes)}
    hp, ps = HC.read_tag_and_set(pseudo, 0, by_pos)
    assert hp == hapref.tag_read(pseudo, 0, by_pos)[0]
    return hp, ps, len(votes)


def haplotag(rs, sites, obs=HA.observe):
    """(uint8[n] tags, stats like Engine.haplotags(), int32[n] phase sets)."""
    site_at = {s["pos"]: (j, s) for j, s in enumerate(sites)}
    hp, ps = np.zeros(len(rs), np.uint8), np.full(len(rs), -1, np.int32)
    st = dict.fromkeys(hapref.STAT_KEYS, 0)
    st["n_reads"] = len(rs)
    for i in range(len(rs)):
        hp[i], ps[i], n = tag_read(rs, i, sites, site_at, obs)
        st["n_votes"] += n
        st["n_hp1" if hp[i] == 1 else "n_hp2" if hp[i] == 2 else "n_tie" if n else "n_no_vote"] += 1
    return hp, st, ps


def allele_counts(rs, hp, ps, query, obs=HA.observe, params=HC.DEFAULT_PARAMS):
    """uint32 (n, 3, 3): what c3r_hap_allele_counts returns under these tags."""
    site_at = {s["pos"]: (j, s) for j, s in enumerate(query)}
    out = np.zeros((len(query), 3, 3), dtype=np.uint32)
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], params):
            continue
        for j, col in obs(rs, i, site_at).items():
            out[j, int(hp[i]) if hp[i] and int(ps[i]) == query[j]["ps"] else 0, col] += 1
    return out


def links(rs, sites, obs=HA.observe, params=phaseref.DEFAULT_PARAMS):
    """uint32 (n, K, 2): what c3r_phase_allele_links returns."""
    site_at = {s["pos"]: (j, s) for j, s in enumerate(sites)}
    out = np.zeros((len(sites), K, 2), dtype=np.uint32)
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], params):
            continue
        seen = {j: c for j, c in obs(rs, i, site_at).items() if c in (0, 1)}
        for j, a in seen.items():
            for k in range(1, K + 1):
                if j - k in seen:
                    out[j, k - 1, 0 if seen[j - k] == a else 1] += 1
    return out


def unit_links(rs, sites, ps, h1, obs=HA.observe, params=phaseref.DEFAULT_PARAMS):
    """uint32 (U, K, 2): what c3r_phase_allele_unit_links returns; ps / h1 per site as the chain leaves them."""
    units = sorted({p for p in ps if p >= 0})
    number = {p: u for u, p in enumerate(units)}
    site_at = {s["pos"]: (j, s) for j, s in enumerate(sites)}
    out = np.zeros((len(units), K, 2), dtype=np.uint32)
    for i in range(len(rs)):
        if not phaseref.votes(rs.reads[i], params):
            continue
        count = {}
        for j, allele in obs(rs, i, site_at).items():
            if allele not in (0, 1) or ps[j] < 0:
                continue
            c = count.setdefault(number[ps[j]], [0, 0])
            c[0 if allele == h1[j] else 1] += 1
        shown = {u: (1 if c[0] > c[1] else 2) for u, c in count.items() if c[0] != c[1]}
        for u, h in shown.items():
            for k in range(1, K + 1):
                if u - k in shown:
                    out[u, k - 1, 0 if shown[u - k] == h else 1] += 1
    return out


# ---- random cases: every planted indel in a homopolymer or a short tandem repeat
UNITS = [u for u in ["A", "C", "G", "T"] + [a + b for a in "ACGT" for b in "ACGT"] + [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
         if len(u) == 1 or len(set(u)) > 1]


def placements(ref, a, kind, n, s=""):
    """[(anchor, s)] of every equivalent placement of an event whose LEFT-MOST one is (a, s), going right: a deletion moves on while the base
    that leaves it equals the base that enters, an insertion while its first base equals the reference base behind the anchor."""
    out = [(a, s)]
    while True:
        nxt = base_at(ref, a + 1)
        if nxt is None or (kind == "del" and nxt != base_at(ref, a + 1 + n)) or (kind == "ins" and nxt != s[0]):
            return out
        a, s = a + 1, (s[1:] + nxt if kind == "ins" else s)
        out.append((a, s))


def gen_repeats(seed, jitter, errors=False, L=6000, n_reads=403, n_snv=100, n_indel=30, n_two=6, n_exons=12):
    """(ref, ReadSet, SNV rows [(pos, ref, alt)], their truth h1, planted sites — dicts with pos / ref / alt / gt, `truth` (1: haplotype 1
    carries allele B) and `left` (the 1-based left-most anchor) —, source haplotype per read).  The reads are drawn the way
    hapalleleref.gen_case draws them (exons joined by N ops, soft clips, 12 % failing the filters; errors: 5 % substitutions, 1 % N, an
    indel of 1-3 every ~60 bases).  Every planted indel (GT 0/1, and a few 1/2 sites with two different indels) inserts or deletes one or
    two whole units of a homopolymer or a 2-3-base tandem repeat of 3 to 8 units that is written into the reference; the base before the
    tract differs from the unit's last base and the base behind it from its first.  A tract keeps at least its own length plus the event
    plus 2 from its exon's ends and from every other variant, and no SNV lies in a tract.  A read carries an event when it covers the
    left-most anchor and runs on past the tract and the event.  jitter = False: every read places the event left-most and so do the VCF
    rows.  jitter = True: every read, and every row, takes a random one of the equivalent placements — from a second random stream, so the
    reads' sequences are those of jitter = False."""
    rng, jit = random.Random(9000 + seed), random.Random(19000 + seed)
    ref = [rng.choice("ACGT") for _ in range(L)]
    cuts = sorted(rng.sample(range(60, L - 60), 2 * n_exons))
    exons = [(cuts[2 * e], cuts[2 * e + 1]) for e in range(n_exons) if cuts[2 * e + 1] - cuts[2 * e] >= 8]
    blocked = []                                               # [lo, hi) 0-based: no other variant in there
    tracts = []
    for k in range(n_indel + n_two):
        for _ in range(200):
            unit = rng.choice(UNITS)
            units = rng.randint(3, 8)
            T = len(unit) * units
            kinds = [rng.choice(("ins", "del"))] if k < n_indel else rng.choice((["ins", "ins"], ["del", "del"], ["ins", "del"]))
            counts = [rng.randint(1, 2) for _ in kinds]
            if len(kinds) == 2 and kinds[0] == kinds[1]:
                counts = [1, 2]
            ev = len(unit) * max(counts)
            margin = T + ev + 2
            a, b = exons[rng.randrange(len(exons))]
            if b - a < T + 2 * margin + 2:
                continue
            t0 = rng.randrange(a + margin + 1, b - margin - T)
            lo, hi = t0 - 1 - margin, t0 + T + margin
            if any(lo < bh and bl < hi for bl, bh in blocked):
                continue
            blocked.append((lo, hi))
            ref[t0:t0 + T] = list(unit * units)
            ref[t0 - 1] = rng.choice([c for c in "ACGT" if c != unit[-1]])
            ref[t0 + T] = rng.choice([c for c in "ACGT" if c != unit[0]])
            tracts.append(dict(t0=t0, T=T, unit=unit, kinds=kinds, counts=counts, gt="0/1" if k < n_indel else "1/2", truth=rng.randint(0, 1)))
            break
    ref = "".join(ref)
    whole = (ref, 0)
    planted = []
    for t in tracts:
        a = t["t0"] - 1                                        # 0-based left-most anchor
        events = []
        for kind, c in zip(t["kinds"], t["counts"]):
            n = len(t["unit"]) * c
            s = t["unit"] * c if kind == "ins" else ""
            assert left_align(whole, a, kind, n, s)[0] == 0
            events.append((kind, n, placements(whole, a, kind, n, s)))
        pair = events if t["gt"] == "1/2" else [None] + events  # per allele A, B: None = the reference allele
        common = min(len(e[2]) for e in events)                # the row's anchor must be a placement of both alleles
        row_at = jit.randrange(common) if jitter else 0
        p0 = a + row_at
        span = max(e[1] for e in events if e[0] == "del") if any(e[0] == "del" for e in events) else 0
        alts = []
        for e in events:
            ins = e[2][row_at][1] if e[0] == "ins" else ""
            dele = e[1] if e[0] == "del" else 0
            alts.append(ref[p0] + ins + ref[p0 + 1 + dele:p0 + 1 + span])
        planted.append(dict(pos=p0 + 1, left=a + 1, ref=ref[p0:p0 + 1 + span], alt=",".join(alts), gt=t["gt"], truth=t["truth"], pair=pair,
                            reach=a + t["T"] + max(e[1] for e in events) + 2))
    planted.sort(key=lambda s: s["left"])
    snv_room = [p for a, b in exons for p in range(a, b) if not any(bl <= p < bh for bl, bh in blocked)]
    rows, truth = [], []
    for p0 in sorted(rng.sample(snv_room, min(n_snv, len(snv_room)))):
        rows.append((p0 + 1, ref[p0], rng.choice([c for c in "ACGT" if c != ref[p0]])))
        truth.append(rng.randint(0, 1))
    smap = {r[0]: (r, t) for r, t in zip(rows, truth)}
    pmap = {s["left"]: s for s in planted}
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
        pending = None                                         # (0-based anchor, inserted letters, deleted bases) of the event to come
        for step in range(n_ex):
            end = exons[e][1] if step + 1 < n_ex else rng.randrange(x + 1, exons[e][1] + 1)
            while x < end:
                b = ref[x]
                if x + 1 in smap:
                    (_, rb, ab), h1 = smap[x + 1]
                    b = ab if (h1 == 1) == (hap == 1) else rb
                elif x + 1 in pmap:
                    s = pmap[x + 1]
                    event = s["pair"][1 if (s["truth"] == 1) == (hap == 1) else 0]
                    pick = jit.random()                        # (drawn for every read that meets the site: one stream for both settings)
                    if event is not None and s["reach"] < end:
                        places = event[2]
                        at, ins = places[int(pick * len(places)) if jitter else 0]
                        pending = (at, ins, event[1] if event[0] == "del" else 0)
                if errors:
                    u = rng.random()
                    if u < 0.05:
                        b = rng.choice("ACGT")
                    elif u < 0.06:
                        b = "N"
                seq.append(b)
                x += 1
                run += 1
                if pending is not None and pending[0] == x - 1:
                    cig.append("%dM" % run)
                    run = 0
                    if pending[1]:
                        cig.append("%dI" % len(pending[1]))
                        seq += list(pending[1])
                    else:
                        cig.append("%dD" % pending[2])
                        x += pending[2]
                    pending = None
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
    order = sorted(range(len(recs)), key=lambda k: recs[k]["pos"])
    recs = [recs[k] for k in order]
    return ref, ReadSet.from_records(recs), rows, np.array(truth, np.uint8), planted, np.array([r["truth"] for r in recs], np.uint8)


def table_of_case(rows, truth, planted, ps=0):
    """(sites sorted by pos — SNV rows and planted rows, with h1 = the truth —, is the site an SNV row)."""
    ent = [(dict(pos=r[0], ps=ps, A=(r[1], HA.NONE), B=(r[2], HA.NONE), ref=r[1], alt=r[2], h1=int(t)), True) for r, t in zip(rows, truth)]
    for p in planted:
        s = HA.site_of_row(p["pos"], p["ref"], p["alt"], p["gt"], ps)
        assert not isinstance(s, str), (p, s)
        ent.append((dict(s, h1=int(p["truth"])), False))
    ent.sort(key=lambda e: e[0]["pos"])
    return [e[0] for e in ent], [e[1] for e in ent]


# ---- hand-derived known answers for the read side: one reference, one table (NOT normalised: sites 2 and 5 sit on right-hand placements
# on purpose), reads of 4 to 12 bases.  Every expectation was worked out by hand from the rule in include/c3r.h.
#               0         1
#               0123456789012345678      0-based; a homopolymer AAAA on 2 .. 5 behind a C, (AC)3 on 10 .. 15 behind a G
HAND_REF = "GCAAAATCGGACACACTTG"
HAND_ROWS = [(2, "CA", "C", "0/1"),             # 0: DEL 1 behind the C on 0-based 1 — the left-most place of a deleted A
             (4, "AA", "A", "0/1"),             # 1: the same deletion two places to the right
             (5, "AA", "A", "0/1"),             # 2: and three places
             (8, "C", "T", "0/1"),              # 3: an SNV: the event is not looked at
             (10, "G", "GAC,GACAC", "1/2"),     # 4: INS AC (A) / INS ACAC (B) behind the G on 9 — left-most
             (14, "C", "CAC", "0/1")]           # 5: INS AC behind the C on 13: a right-hand placement of 4's allele A
# (name, (slice text, its first 0-based position), (pos0, cigar, seq[, l_seq]), {table index: column})
HAND_READS = [
    # the deletion already left-most: run GC, 0 shifts (C != A)
    ("shift_0", (HAND_REF, 0), (0, "2M1D5M", "GCAAATC"), {0: 1, 1: 0, 2: 0, 3: 0}),
    # run GCA, D on 3: one shift (A == A), then C != A: shown on 0-based 1; site 1 lies under the D, site 2 starts the next run
    ("shift_1", (HAND_REF, 0), (0, "3M1D4M", "GCAAATC"), {0: 1, 2: 0, 3: 0}),
    # the read starts inside the tract: run AA on 3, 4; the rule says 3 shifts, the run allows 1: shown on its first base
    ("cap_at_run_start", (HAND_REF, 0), (3, "2M1D2M", "AATC"), {1: 1, 2: 0, 3: 0}),
    ("run_of_one", (HAND_REF, 0), (4, "1M1D3M", "ATCG"), {2: 1, 3: 0}),
    # 3M2= is a run of 5 (0 .. 4): 3 shifts, shown on 1; plain CIGAR, and the same with an empty op that sends the read down the serial walk
    ("m_like_run_plain", (HAND_REF, 0), (0, "3M2=1D2M", "GCAAATC"), {0: 1, 1: 0, 2: 0, 3: 0}),
    ("m_like_run_serial", (HAND_REF, 0), (0, "3M2=0I1D2M", "GCAAATC"), {0: 1, 1: 0, 2: 0, 3: 0}),
    # run 9 .. 13, INS AC behind 13: C=C, A=A, C=C, A=A, then G: 4 shifts (k >= n), the rotation ends on AC again: allele A of site 4
    ("ins_rotated_plain", (HAND_REF, 0), (9, "2X3M2I3M", "GACACACACT"), {4: 0, 5: 0}),
    ("ins_rotated_serial", (HAND_REF, 0), (9, "2X3M0D2I3M", "GACACACACT"), {4: 0, 5: 0}),
    # an I with a D at once behind it: OTHER, on the run's last base only, never shifted
    ("ins_then_del", (HAND_REF, 0), (9, "5M2I1D2M", "GACACACCT"), {4: 2, 5: 2}),
    # SEQ ends inside the insertion: no observation on the run's last base, no event elsewhere
    ("ins_cut_off", (HAND_REF, 0), (9, "5M2I3M", "GACACACACT", 6), {4: 2}),
    # INS ACAC behind 11: two shifts (k < n): s' = ref[10 .. 11] + AC = ACAC: allele B of site 4
    ("ins_longer_than_shift", (HAND_REF, 0), (7, "5M4I3M", "CGGACACACACA"), {3: 0, 4: 1, 5: 0}),
    # the first step compares ref[4] with ref[5]: the slice's last base — and with a slice one base shorter nothing moves
    ("del_compare_on_last_base", (HAND_REF[:6], 0), (0, "5M1D1M", "GCAAAT"), {0: 1, 1: 0, 2: 0}),
    ("del_compare_past_slice", (HAND_REF[:5], 0), (0, "5M1D1M", "GCAAAT"), {0: 0, 1: 0, 2: 1}),
]


def hand_table():
    out = []
    for row in HAND_ROWS:
        s = HA.site_of_row(*row)
        assert not isinstance(s, str), (row, s)
        out.append(s)
    return out


def hand_readset(read):
    rs = ReadSet.from_records([dict(pos=read[0], cigar=read[1], seq=read[2], flag=0, mapq=60, hp=0)])
    if len(read) > 3:
        rs.reads["l_seq"][0] = read[3]
    return rs


def boundary_reads(seed=5):
    """(ref, [(name, (pos0, cigar, seq))], table rows): reads of 17, 32 and 33 ops whose event — a deleted A of a homopolymer — is their
    16th or 17th op, so that the M run before it and the event fall on either side of the 16-op lane boundary of the plain walk.  The ops
    before are 1M1I pairs."""
    rng = random.Random(seed)
    ref = list("".join(rng.choice("CGT") for _ in range(90)))
    out, rows = [], []
    for k, (name, lead_s, n_after, tail_s) in enumerate((("ops17_event_op16", 0, 0, 0), ("ops32_event_op17", 1, 7, 0), ("ops33_event_op17", 1, 7, 1))):
        p0 = 3 + 28 * k
        # 7 x 1M1I over p0 .. p0 + 6, 4M over p0 + 7 .. p0 + 10 (G AAA), D on p0 + 11 (A), then 3M (or 2M and 7 x 1I1M)
        ref[p0 + 7:p0 + 13] = list("GAAAAT")
        cig, seq = (["2S"], ["A", "A"]) if lead_s else ([], [])
        x = p0
        for _ in range(7):
            cig += ["1M", "1I"]
            seq += [ref[x], rng.choice("ACGT")]
            x += 1
        cig += ["4M", "1D"]
        seq += ref[x:x + 4]
        x += 5
        m = 2 if n_after else 3
        cig.append("%dM" % m)
        seq += ref[x:x + m]
        x += m
        for _ in range(n_after):
            cig += ["1I", "1M"]
            seq += [rng.choice("ACGT"), ref[x]]
            x += 1
        if tail_s:
            cig.append("1S")
            seq.append("A")
        assert len(cig) == int(name[3:5])
        out.append((name, (p0, "".join(cig), "".join(seq))))
        rows += [(p0 + 8, "GA", "G", "0/1"), (p0 + 11, "AA", "A", "0/1")]       # the left-most place and the read's own
    return "".join(ref), out, rows
