"""The rule `realign` of include/c3r.h (c3r_set_hap_realign) restated in plain Python: one read at one site, strings and lists, a textbook
dynamic-programming edit distance and a CIGAR map of its own that steps through the raw ops one reference position at a time.  It shares
no code with csrc/realign.hpp, csrc/haplotag_kernels.hpp or the drivers and is what the tests compare them with.  Where a read is not
realigned at a site the observation is hapalleleref.observe's (the restatement of the switch-off rule); the four tables under an
observation are leftalignref's (haplotag, allele_counts, links, unit_links take the observation as an argument).  Its own behaviour is
pinned by the hand-derived cases of tests/test_realign_ref.py.

A reference here is (first 0-based position of the slice, its letters); a site is hapalleleref's dict.

gen_fuzz(seed) builds the fuzz of the tests: a 400-base reference, 200 reads of 80 to 160 bases from two haplotypes with 5 % substitutions
and 3 % indels, a site every 15 bases of which every third is an indel or a two-ALT site."""
import random

from clair3_rna_amd.reads import ReadSet
from tests import hapalleleref as HA

MAX_W, MAX_LEN = 16, 64
LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}


# ---- the edit distance
def levenshtein(a, b):
    """Global unit-cost edit distance of two sequences; an element of `a` that is None equals nothing."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            same = a[i - 1] is not None and a[i - 1] == b[j - 1]
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if same else 1))
        prev = cur
    return prev[len(b)]


# ---- reference, window, haplotype strings
def ref_letter(ref, p):
    """The upper-case letter of 0-based position p when it lies in the slice and is one of A, C, G, T, else None."""
    beg0, text = ref
    if p < beg0 or p >= beg0 + len(text):
        return None
    c = text[p - beg0].upper()
    return c if c in "ACGT" else None


def window(site, W):
    """(p0, D, I, s, t) of a site."""
    p0 = site["pos"] - 1
    D = max([ev[1] for _, ev in (site["A"], site["B"]) if ev[0] == "del"] + [0])
    I = max([len(ev[1]) for _, ev in (site["A"], site["B"]) if ev[0] == "ins"] + [0])
    return p0, D, I, p0 - W, p0 + 1 + D + W


def realignable(ref, site, W):
    p0, D, I, s, t = window(site, W)
    return all(ref_letter(ref, p) is not None for p in range(s, t)) and 2 * W + 1 + D + I <= MAX_LEN


def haplotype(ref, site, which, W):
    """The haplotype string of allele `which` ("A" / "B") of a realignable site."""
    p0, D, I, s, t = window(site, W)
    base, ev = site[which]
    ins = ev[1] if ev[0] == "ins" else ""
    dele = ev[1] if ev[0] == "del" else 0
    return "".join(ref_letter(ref, p) for p in range(s, p0)) + base + ins + "".join(ref_letter(ref, p) for p in range(p0 + 1 + dele, t))


# ---- the map, one reference position at a time
def cover(ops, pos):
    """{reference position: (op letter M / D / N, query offset)} of a read's RAW ops [(letter, length)]: q = the offset of the read's base
    on the position under an M-like op, and of the next base of the read under a D or an N."""
    out = {}
    x, y = pos, 0
    for op, n in ops:
        if op in "M=X":
            for d in range(n):
                out[x + d] = ("M", y + d)
            x, y = x + n, y + n
        elif op in "DN":
            for d in range(n):
                out[x + d] = (op, y)
            x += n
        elif op in "IS":
            y += n
        # H, P: nothing
    return out, x


def realigned_window(rs, i, ref, site, W, cov=None):
    """(q(s), q(t)) when read i is realigned at the site, else None.  cov: cover()'s pair for the read, when the caller has it."""
    if W < 1 or not realignable(ref, site, W):
        return None
    p0, D, I, s, t = window(site, W)
    r = rs.reads[i]
    cov, end = cov or cover(HA.read_ops(rs, i), int(r["pos"]))
    if not (int(r["pos"]) <= s and t < end):
        return None
    if any(cov[p][0] == "N" for p in range(s, t + 1)):
        return None
    qs, qt = cov[s][1], cov[t][1]
    if qt > int(r["l_seq"]) or qt - qs > MAX_LEN:
        return None
    return qs, qt


def realigned_column(rs, i, ref, site, W, cov=None):
    """None: not realigned; else 0, 1 or "tie"."""
    w = realigned_window(rs, i, ref, site, W, cov)
    if w is None:
        return None
    read = [LETTER.get(HA.code_at(rs, i, q)) for q in range(w[0], w[1])]
    dA, dB = levenshtein(read, haplotype(ref, site, "A", W)), levenshtein(read, haplotype(ref, site, "B", W))
    return 0 if dA < dB else 1 if dB < dA else "tie"


def anchored(rs, i, site, cov=None):
    """Does the site's anchor lie under an M op of read i at a query offset below l_seq?"""
    cov, _ = cov or cover(HA.read_ops(rs, i), int(rs.reads[i]["pos"]))
    hit = cov.get(site["pos"] - 1)
    return hit is not None and hit[0] == "M" and hit[1] < int(rs.reads[i]["l_seq"])


def observe(rs, i, site_at, ref, W, detail=None):
    """{site index: column 0 / 1 / 2} of read i under the switch (W = 0: hapalleleref.observe).  detail (a dict) receives
    {site index: True when the read was realigned there} for every site whose anchor the read holds."""
    plain = HA.observe(rs, i, site_at)
    if W == 0:
        return plain
    out = {}
    cov = cover(HA.read_ops(rs, i), int(rs.reads[i]["pos"]))
    for pos, (j, site) in site_at.items():
        if not anchored(rs, i, site, cov):
            continue
        col = realigned_column(rs, i, ref, site, W, cov)
        if detail is not None:
            detail[j] = col is not None
        if col is None:
            if j in plain:
                out[j] = plain[j]
        elif col != "tie":
            out[j] = col
    return out


def observer(ref, W):
    """obs(rs, i, site_at) for leftalignref's four tables."""
    return lambda rs, i, site_at: observe(rs, i, site_at, ref, W)


def column_of(rs, i, site, ref, W):
    """(column 0 / 1 / 2, or 3 for no observation; realigned) of read i at one site: what c3r_hap_realign_column returns."""
    detail = {}
    seen = observe(rs, i, {site["pos"]: (0, site)}, ref, W, detail)
    return seen.get(0, 3), bool(detail.get(0, False))


# ---- the fuzz
def gen_fuzz(seed, L=400, n_reads=200, step=15, sub=0.05, indel=0.03, serial_half=True, quals=False):
    """(reference (0, letters), table of site dicts with h1 and ps, ReadSet).  Reads come from two haplotypes (haplotype 1 carries allele A
    where h1 = 0), with read errors written as the truth has them except that half of the substitutions are written `1D1I` — what the
    rule is for.  With serial_half every second read gets = / X ops or a pad, which sends it down the serial walk; with quals every base gets a quality of 2 .. 40 (the reads themselves
    do not change)."""
    rng, qrng = random.Random(seed), random.Random(seed + 1000)
    letters = []
    while len(letters) < L:
        letters.append(letters[-1] if letters and rng.random() < 0.3 else rng.choice("ACGT"))
    text = "".join(letters)
    table = []
    for k, p0 in enumerate(range(20, L - 20, step)):
        r = text[p0]
        others = [c for c in "ACGT" if c != r]
        if k % 3 == 2:
            kind = rng.choice(("ins", "del", "two"))
            if kind == "ins":
                row = (p0 + 1, r, r + "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 3))), "0/1")
            elif kind == "del":
                n = rng.randint(1, 3)
                row = (p0 + 1, text[p0:p0 + 1 + n], r, "0/1")
            else:
                row = (p0 + 1, r, rng.choice(others) + "," + r + "".join(rng.choice("ACGT") for _ in range(2)), "1/2")
        else:
            row = (p0 + 1, r, rng.choice(others), "0/1")
        site = HA.site_of_row(*row)
        assert not isinstance(site, str), (row, site)
        site["h1"], site["ps"] = rng.randint(0, 1), 21
        table.append(site)
    by_p0 = {s["pos"] - 1: s for s in table}
    recs = []
    for n in range(n_reads):
        span = rng.randint(80, 160)
        start = rng.randint(0, L - span)
        hap = rng.randint(1, 2)
        cig, seq = [], []                                               # cig: one letter per column, run-length encoded at the end

        def put(op, bases=""):
            cig.append(op)
            seq.append(bases)
        x = start
        while x < start + span:
            edge = x < start + 2 or x >= start + span - 2               # (a read begins and ends on clean matches)
            site = by_p0.get(x)
            if site is not None:
                base, ev = site["A" if (site["h1"] == 0) == (hap == 1) else "B"]
                put("M", base)
                if ev[0] == "ins":
                    for c in ev[1]:
                        put("I", c)
                elif ev[0] == "del":
                    for _ in range(ev[1]):
                        put("D")
                    x += ev[1]
                x += 1
                continue
            u = rng.random()
            if edge or u >= sub + indel:
                put("M", text[x])
            elif u < sub:
                wrong = rng.choice([c for c in "ACGT" if c != text[x]])
                if rng.random() < 0.5:
                    put("D")
                    put("I", wrong)
                else:
                    put("M", wrong)
            elif rng.random() < 0.5:
                put("D")
            else:
                put("M", text[x])
                for _ in range(rng.randint(1, 2)):
                    put("I", rng.choice("ACGT"))
            x += 1
        serial = serial_half and n % 2 == 1
        if serial and n % 4 == 1:                                       # = / X in the place of M
            y = start
            for k, op in enumerate(cig):
                if op == "M":
                    cig[k] = "=" if seq[k] == text[y] else "X"
                if op in "M=XD":
                    y += 1
        ops = []
        for op in cig:
            if ops and ops[-1][0] == op:
                ops[-1][1] += 1
            else:
                ops.append([op, 1])
        if serial and n % 4 == 3:                                       # a pad inside the first M op of three or more
            for k, (op, m) in enumerate(ops):
                if op == "M" and m >= 3:
                    ops[k:k + 1] = [["M", 1], ["P", 1], ["M", m - 1]]
                    break
        bases = "".join(seq)
        if n % 5 == 0:                                                  # soft clips count in the query offsets
            ops = [["S", 3]] + ops + [["S", 2]]
            bases = "TTT" + bases + "GG"
        recs.append(dict(pos=start, cigar="".join("%d%s" % (m, op) for op, m in ops), seq=bases, flag=0, mapq=60, hp=0))
        if quals:
            recs[-1]["qual"] = [qrng.randint(2, 40) for _ in bases]
    return (0, text), table, ReadSet.from_records(recs)


def fuzz_profile(ref, table, rs, W):
    """(observations, of them realigned, columns that differ from hapalleleref.observe's) of a fuzz under overhang W."""
    site_at = {s["pos"]: (j, s) for j, s in enumerate(table)}
    n = n_ra = n_diff = 0
    for i in range(len(rs)):
        detail = {}
        seen, plain = observe(rs, i, site_at, ref, W, detail), HA.observe(rs, i, site_at)
        n += len(detail)
        n_ra += sum(detail.values())
        n_diff += sum(1 for j in set(seen) | set(plain) if seen.get(j, 3) != plain.get(j, 3))
    return n, n_ra, n_diff


# ---- the hand-derived cases (tests/test_realign_ref.py works them out; tests/test_gpu_realign.py runs them on the device)
#      0         1         2
#      012345678901234567890123456789
REF = "GATTACAGCTCGATCGGATCCTAGCATGCA"
SNV = (14, "T", "C", "0/1")            # anchor 13 (T).  W = 3: s = 10, t = 17, ref[10, 17) = CGATCGG; A = CGATCGG, B = CGACCGG
DEL = (14, "TC", "T", "0/1")           # anchor 13, DEL of the C on 14.  W = 3: D = 1, s = 10, t = 18; A = CGATCGGA, B = CGATGGA
NO = 3                                 # no observation

# (name, reference (first 0-based position, letters), row, W, (pos0, cigar, seq), (column, realigned) with the switch on, column with it off)
HAND = [
    # the window is seq[5:12] = CGATCGG: dA = 0, dB = 1
    ("clean_read", (0, REF), SNV, 3, (5, "20M", REF[5:25]), (0, True), 0),
    # the read carries C on 13 and an A for the G on 11: window CAACCGG; against A two substitutions, against B one
    ("one_substitution", (0, REF), SNV, 3, (5, "20M", REF[5:11] + "A" + REF[12] + "C" + REF[14:25]), (1, True), 1),
    # the read carries C on 13; the aligner deleted 12 and inserted behind 13, so the CIGAR puts the A of 12 on the anchor: off, another
    # allele; on, the window seq[5:12] = CGACCGG is B itself
    ("1D1I_for_a_substitution", (0, REF), SNV, 3, (5, "7M1D1M1I11M", REF[5:13] + "C" + REF[14:25]), (1, True), 2),
    # a REF read whose wrong base on 14 is written 1D1I behind the anchor: off, it is the deletion; on, CGATAGGA is one edit from both
    ("tie", (0, REF), DEL, 3, (5, "9M1D1I10M", REF[5:14] + "A" + REF[15:25]), (NO, True), 1),
    # TT inserted directly before s = 10: outside, the window is ref[10, 17) itself
    ("insertion_before_s_is_outside", (0, REF), SNV, 3, (5, "5M2I15M", REF[5:10] + "TT" + REF[10:25]), (0, True), 0),
    # TT inserted directly before t = 17: inside, the window CGATCGGTT is two from A and three from B
    ("insertion_before_t_is_inside", (0, REF), SNV, 3, (5, "12M2I8M", REF[5:17] + "TT" + REF[17:25]), (0, True), 0),
    # 9 and 10 deleted: q(s) is the base on 11; the window GATCGG is one from A, two from B
    ("D_under_s", (0, REF), SNV, 3, (5, "4M2D14M", REF[5:9] + REF[11:25]), (0, True), 0),
    # 16 and 17 deleted: q(t) is the base on 18; the window CGATCG is one from A, two from B
    ("D_under_t", (0, REF), SNV, 3, (5, "11M2D7M", REF[5:16] + REF[18:25]), (0, True), 0),
    # an N on t: the window is not usable, the column is the switch-off one; an N that starts behind t does not matter
    ("N_on_t", (0, REF), SNV, 3, (5, "12M5N3M", REF[5:17] + REF[22:25]), (0, False), 0),
    ("N_behind_t", (0, REF), SNV, 3, (5, "13M4N3M", REF[5:18] + REF[22:25]), (0, True), 0),
    # an N that ends on s - 1 does not touch [s, t] either; one that ends on s does
    ("N_before_s", (0, REF), SNV, 3, (3, "2M5N15M", REF[3:5] + REF[10:25]), (0, True), 0),
    ("N_on_s", (0, REF), SNV, 3, (3, "2M6N14M", REF[3:5] + REF[11:25]), (0, False), 0),
    # the read's end: t < end is needed
    ("read_ends_at_t", (0, REF), SNV, 3, (5, "12M", REF[5:17]), (0, False), 0),
    ("read_ends_behind_t", (0, REF), SNV, 3, (5, "13M", REF[5:18]), (0, True), 0),
    ("read_starts_at_s", (0, REF), SNV, 3, (10, "10M", REF[10:20]), (0, True), 0),
    ("read_starts_behind_s", (0, REF), SNV, 3, (11, "10M", REF[11:21]), (0, False), 0),
    # q(t) <= l_seq: SEQ is one base short of t's offset (the anchor is still below l_seq)
    ("seq_ends_at_t", (0, REF), SNV, 3, (5, "20M", REF[5:17]), (0, True), 0),
    ("seq_ends_before_t", (0, REF), SNV, 3, (5, "20M", REF[5:16]), (0, False), 0),
    # a reference base of the window that is not A, C, G or T; the slice's edge
    ("n_in_the_reference", (0, REF[:16] + "N" + REF[17:]), SNV, 3, (5, "20M", REF[5:25]), (0, False), 0),
    ("window_past_the_slice", (0, REF[:16]), SNV, 3, (5, "20M", REF[5:25]), (0, False), 0),
    ("slice_starts_behind_s", (11, REF[11:]), SNV, 3, (5, "20M", REF[5:25]), (0, False), 0),
    ("lower_case_slice", (10, REF[10:17].lower()), SNV, 3, (5, "20M", REF[5:25]), (0, True), 0),
    # a masked base (N in the read) equals nothing: window CGANCGG is one from both
    ("read_n_on_the_anchor", (0, REF), SNV, 3, (5, "20M", REF[5:13] + "N" + REF[14:25]), (NO, True), NO),
    # soft clips count, hard clips, pads and empty ops do not: the first case again
    ("clips_and_pads", (0, REF), SNV, 3, (5, "2H3S4M0D1P16=", "AAA" + REF[5:25]), (0, True), 0),
    # the anchor under a deletion: nothing, whatever the window says
    ("anchor_under_D", (0, REF), SNV, 3, (5, "8M1D11M", REF[5:13] + REF[14:25]), (NO, False), NO),
]


def one_read(read):
    return ReadSet.from_records([dict(pos=read[0], cigar=read[1], seq=read[2], flag=0, mapq=60, hp=0)])


def site_of(row):
    s = HA.site_of_row(*row)
    assert not isinstance(s, str), (row, s)
    return s


# ---- the two limits of 64, on a reference of 160 letters without a repeat longer than two
LONG = "".join("ACGT"[(k * 7 + k // 4 + k // 16) % 4] for k in range(160))


def long_read(p0, allele_ins, extra_at=None):
    """A read over [p0 - 30, p0 + 70) that carries an insertion behind p0, and one more inserted base behind `extra_at`."""
    seq, cig = [], []
    for x in range(p0 - 30, p0 + 70):
        seq.append(LONG[x])
        cig.append("M")
        for c in (allele_ins if x == p0 else "T" if x == extra_at else ""):
            seq.append(c)
            cig.append("I")
    ops = []
    for op in cig:
        if ops and ops[-1][0] == op:
            ops[-1][1] += 1
        else:
            ops.append([op, 1])
    return p0 - 30, "".join("%d%s" % (n, op) for op, n in ops), "".join(seq)
