"""The rule `realign_spliced` of include/c3r.h (c3r_set_hap_realign_spliced) restated in plain Python: a read's spliced positions as a sorted
list, the window counted in that list, strings and the textbook edit distance.  It shares no code with csrc/realign.hpp,
csrc/haplotag_kernels.hpp or the drivers and is what the tests compare them with; of the other restatements it uses realignref.cover (the
map, one reference position at a time), realignref.levenshtein and hapalleleref's readers.  Where a read is not realigned at a site the
observation is hapalleleref.observe's; the four tables under an observation are leftalignref's.  Its own behaviour is pinned by the
hand-derived cases below (tests/test_realign_spliced_ref.py works them out).

plant() is the intron planter of the tests: it cuts a reference at chosen positions, puts random letters there, shifts sites and reads and
writes the matching N op into every read that crosses a cut — the input on which the rule must give what `realign` gives without introns."""
import random

import numpy as np

from clair3_rna_amd.reads import ReadSet
from tests import hapalleleref as HA
from tests import realignref as RR

MAX_LEN = 64
LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}


# ---- the window in spliced positions
def spliced(rs, i):
    """(x_0 < x_1 < ...: the reference positions under the M-like and D ops of read i's raw CIGAR; realignref.cover's map)."""
    cov, _ = RR.cover(HA.read_ops(rs, i), int(rs.reads[i]["pos"]))
    return sorted(p for p, (op, _) in cov.items() if op != "N"), cov


def core(site):
    """(p0, D, I) of a site."""
    p0, D, I, _, _ = RR.window(site, 0)
    return p0, D, I


def spliced_window(rs, i, ref, site, W, sp=None):
    """(q(x_ks), q(x_kt), xs, k0) when read i is realigned at the site under the rule, else None.  sp: spliced()'s pair, when the caller has it."""
    if W < 1:
        return None
    p0, D, I = core(site)
    if 2 * W + 1 + D + I > MAX_LEN:
        return None
    xs, cov = sp or spliced(rs, i)
    if p0 not in cov or cov[p0][0] == "N":
        return None
    k0 = xs.index(p0)
    ks, kt = k0 - W, k0 + 1 + D + W
    if ks < 0 or kt >= len(xs):
        return None
    if xs[k0:k0 + D + 1] != list(range(p0, p0 + D + 1)):                 # an N holds a position of the core
        return None
    if any(RR.ref_letter(ref, p) is None for p in xs[ks:kt]):
        return None
    qs, qt = cov[xs[ks]][1], cov[xs[kt]][1]
    if qt > int(rs.reads[i]["l_seq"]) or qt - qs > MAX_LEN:
        return None
    return qs, qt, xs, k0


def haplotype(ref, site, which, xs, k0, W):
    """The haplotype string of allele `which` ("A" / "B") along the spliced positions xs around index k0."""
    _, D, _ = core(site)
    base, ev = site[which]
    ins = ev[1] if ev[0] == "ins" else ""
    dele = ev[1] if ev[0] == "del" else 0
    return ("".join(RR.ref_letter(ref, xs[k]) for k in range(k0 - W, k0)) + base + ins +
            "".join(RR.ref_letter(ref, xs[k]) for k in range(k0 + 1 + dele, k0 + 1 + D + W)))


def strings_of(rs, i, site, ref, W):
    """(haplotype string A, haplotype string B, the read's window as letters with "?" for a code that equals nothing) of a realigned read."""
    qs, qt, xs, k0 = spliced_window(rs, i, ref, site, W)
    return (haplotype(ref, site, "A", xs, k0, W), haplotype(ref, site, "B", xs, k0, W),
            "".join(LETTER.get(HA.code_at(rs, i, q), "?") for q in range(qs, qt)))


def realigned_column(rs, i, ref, site, W, sp=None):
    """None: not realigned; else 0, 1 or "tie"."""
    w = spliced_window(rs, i, ref, site, W, sp)
    if w is None:
        return None
    qs, qt, xs, k0 = w
    read = [LETTER.get(HA.code_at(rs, i, q)) for q in range(qs, qt)]
    dA, dB = RR.levenshtein(read, haplotype(ref, site, "A", xs, k0, W)), RR.levenshtein(read, haplotype(ref, site, "B", xs, k0, W))
    return 0 if dA < dB else 1 if dB < dA else "tie"


def observe(rs, i, site_at, ref, W, detail=None):
    """{site index: column 0 / 1 / 2} of read i under both switches (W = 0: hapalleleref.observe).  detail (a dict) receives
    {site index: True when the read was realigned there} for every site whose anchor the read holds."""
    plain = HA.observe(rs, i, site_at)
    if W == 0:
        return plain
    out = {}
    sp = spliced(rs, i)
    l_seq = int(rs.reads[i]["l_seq"])
    for pos, (j, site) in site_at.items():
        hit = sp[1].get(pos - 1)
        if hit is None or hit[0] != "M" or hit[1] >= l_seq:              # the anchor: under an M op at a query offset below l_seq
            continue
        col = realigned_column(rs, i, ref, site, W, sp)
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
    """(column 0 / 1 / 2, or 3 for no observation; realigned) of read i at one site: what c3r_hap_realign_column_spliced returns."""
    detail = {}
    seen = observe(rs, i, {site["pos"]: (0, site)}, ref, W, detail)
    return seen.get(0, 3), bool(detail.get(0, False))


def profile(ref, table, rs, W):
    """Over all (read, site) pairs of a set: (anchored pairs, of them realigned under `realign`, realigned under the rule here, columns
    that differ between the two)."""
    site_at = {s["pos"]: (j, s) for j, s in enumerate(table)}
    n = n_plain = n_spliced = n_diff = 0
    for i in range(len(rs)):
        d_plain, d_spliced = {}, {}
        a, b = RR.observe(rs, i, site_at, ref, W, d_plain), observe(rs, i, site_at, ref, W, d_spliced)
        assert set(d_plain) == set(d_spliced)
        n += len(d_spliced)
        n_plain += sum(d_plain.values())
        n_spliced += sum(d_spliced.values())
        n_diff += sum(1 for j in set(a) | set(b) if a.get(j, 3) != b.get(j, 3))
    return n, n_plain, n_spliced, n_diff


# ---- the intron planter
CUTS = (58, 118, 178, 238, 298, 358)      # on realignref.gen_fuzz's 400 bases: 8 bases behind the sites on 50, 110, ...; they touch no site's core


def plant(ref, table, rs, cuts=CUTS, seed=0):
    """(reference, table, ReadSet) with an intron of 40 .. 300 random letters put before every 0-based position of `cuts`: sites and reads
    behind a cut move, and every read with bases on both sides of a cut gets the N op — where an I op (or a pad) stands at the cut, at
    random before or after it.  Reads and sites keep their indices; SEQ and the qualities do not change.  The reads hold no N op yet."""
    rng = random.Random(seed)
    beg0, text = ref
    cuts = sorted(cuts)
    assert all(beg0 < c < beg0 + len(text) for c in cuts)
    intron = {c: "".join(rng.choice("ACGT") for _ in range(rng.randint(40, 300))) for c in cuts}
    moved = lambda p: p + sum(len(intron[c]) for c in cuts if c <= p)
    pieces, at = [], beg0
    for c in cuts:
        pieces += [text[at - beg0:c - beg0], intron[c]]
        at = c
    new_ref = (beg0, "".join(pieces) + text[at - beg0:])
    new_table = []
    for s in table:
        p0, D, _ = core(s)
        assert not any(p0 < c <= p0 + D for c in cuts), "a cut inside the core of the site on %d" % s["pos"]
        new_table.append(dict(s, pos=moved(p0) + 1))
    reads = rs.reads.copy()
    words = []
    for i in range(len(rs)):
        x = int(reads[i]["pos"])
        out, behind_ref = [], 0                                          # behind_ref: the place in `out` right behind the last M / D op
        for op, n in HA.read_ops(rs, i):
            assert op != "N"
            if op in "M=XD" and n > 0:
                for c in cuts:
                    if c == x and behind_ref > 0:                       # the cut lies between two ops: before or after what stands there
                        out.insert(behind_ref if rng.random() < 0.5 else len(out), ("N", len(intron[c])))
                    elif x < c < x + n:                                  # inside the op: split it
                        out += [(op, c - x), ("N", len(intron[c]))]
                        x, n = c, n - (c - x)
                out.append((op, n))
                behind_ref = len(out)
                x += n
            else:
                out.append((op, n))
        reads[i]["pos"] = moved(int(reads[i]["pos"]))
        reads[i]["cigar_off"], reads[i]["n_cigar"] = len(words), len(out)
        words += [(n << 4) | "MIDNSHP=X".index(op) for op, n in out]
    return new_ref, new_table, ReadSet(reads, np.array(words, np.uint32), rs.seq.copy(), None if rs.qual is None else rs.qual.copy())


def n_ops(rs):
    return int(sum(1 for c in rs.cigar if int(c) & 15 == 3))


# ---- the hand-derived cases (tests/test_realign_spliced_ref.py works them out; tests/test_gpu_realign_spliced.py runs them on the device)
#      0         1         2
#      012345678901234567890123456789
# REF  GATTACAGCTCGATCGGATCCTAGCATGCA     the SNV T > C on anchor 13, W = 3: without an N the strings are CGATCGG and CGACCGG
REF, SNV, DEL, NO = RR.REF, RR.SNV, RR.DEL, RR.NO

# (name, reference, row, W, (pos0, cigar, seq), (column, realigned) under the rule, (column, realigned) under plain `realign`, column with
#  both off, (string A, string B, window) of a realigned read or None)
HAND = [
    # x_kt = 22 behind the intron 17 .. 21; the right flank 14, 15, 16 lies before it: the window is seq[5:12]
    ("N_on_t", (0, REF), SNV, 3, (5, "12M5N3M", REF[5:17] + REF[22:25]), (0, True), (0, False), 0, ("CGATCGG", "CGACCGG", "CGATCGG")),
    # the read carries C on 13, written 1D1I: the CIGAR puts the A of 12 on the anchor (another allele).  The right flank is 14, 20, 21
    ("1D1I_beside_a_junction", (0, REF), SNV, 3, (5, "7M1D1M1I1M5N5M", REF[5:13] + "C" + REF[14] + REF[20:25]), (1, True), (2, False), 2,
     ("CGATCCT", "CGACCCT", "CGACCCT")),
    # the intron 7 .. 10 inside the left flank: x_ks = 6, the flank is 6, 11, 12; the read carries the ALT
    ("N_inside_the_left_flank", (0, REF), SNV, 3, (2, "5M4N13M", REF[2:7] + REF[11:13] + "C" + REF[14:24]), (1, True), (1, False), 1,
     ("AGATCGG", "AGACCGG", "AGACCGG")),
    # a micro-exon 18, 19 between two introns: the right flank is 14, 18, 19 and x_kt = 23
    ("two_N_ops_in_one_window", (0, REF), SNV, 3, (5, "10M3N2M3N5M", REF[5:15] + REF[18:20] + REF[23:28]), (0, True), (0, False), 0,
     ("CGATCTC", "CGACCTC", "CGATCTC")),
    # the deletion site's core is [13, 14] and the intron starts on 14: the CIGAR's column (T and no event: the REF allele)
    ("N_inside_the_core_of_a_deletion", (0, REF), DEL, 3, (5, "9M4N8M", REF[5:14] + REF[18:26]), (0, False), (0, False), 0, None),
    # the same read at the SNV, whose core is 13 alone: the right flank is 18, 19, 20 and x_kt = 21
    ("N_directly_behind_the_anchor", (0, REF), SNV, 3, (5, "9M4N8M", REF[5:14] + REF[18:26]), (0, True), (0, False), 0, ("CGATTCC", "CGACTCC", "CGATTCC")),
    # two spliced positions before the anchor (4, 12) and three (4, 5, 12)
    ("two_positions_before_the_anchor", (0, REF), SNV, 3, (4, "1M7N12M", REF[4] + REF[12:24]), (0, False), (0, False), 0, None),
    ("three_positions_before_the_anchor", (0, REF), SNV, 3, (4, "2M6N12M", REF[4:6] + REF[12:24]), (0, True), (0, False), 0, ("ACATCGG", "ACACCGG", "ACATCGG")),
    # kt = 12: the read has 12 spliced positions (kt is none of its indices: `realign`'s read_ends_at_t) and 13 (kt is the last one:
    # `realign`'s read_ends_behind_t)
    ("kt_behind_the_last_position", (0, REF), SNV, 3, (5, "9M4N3M", REF[5:14] + REF[18:21]), (0, False), (0, False), 0, None),
    ("kt_on_the_last_position", (0, REF), SNV, 3, (5, "9M4N4M", REF[5:14] + REF[18:22]), (0, True), (0, False), 0, ("CGATTCC", "CGACTCC", "CGATTCC")),
    # TT inserted directly before x_kt = 22, listed before the N and behind it: inside both times, two from A and three from B
    ("insertion_before_the_N_before_x_kt", (0, REF), SNV, 3, (5, "12M2I5N3M", REF[5:17] + "TT" + REF[22:25]), (0, True), (0, False), 0,
     ("CGATCGG", "CGACCGG", "CGATCGGTT")),
    ("insertion_behind_the_N_before_x_kt", (0, REF), SNV, 3, (5, "12M5N2I3M", REF[5:17] + "TT" + REF[22:25]), (0, True), (0, False), 0,
     ("CGATCGG", "CGACCGG", "CGATCGGTT")),
    # and directly before x_ks = 10, on either side of the intron 6 .. 9 (which ends before s: `realign` realigns too): outside both times
    ("insertion_before_the_N_before_x_ks", (0, REF), SNV, 3, (3, "3M2I4N14M", REF[3:6] + "TT" + REF[10:24]), (0, True), (0, True), 0,
     ("CGATCGG", "CGACCGG", "CGATCGG")),
    ("insertion_behind_the_N_before_x_ks", (0, REF), SNV, 3, (3, "3M4N2I14M", REF[3:6] + "TT" + REF[10:24]), (0, True), (0, True), 0,
     ("CGATCGG", "CGACCGG", "CGATCGG")),
    # 16 deleted before the intron 17 .. 21: it is a spliced position, the window CGATCG is one from A and two from B; and 22 deleted behind
    # the intron: x_kt = 22 lies under the D and q(x_kt) is the base on 23
    ("D_before_an_N", (0, REF), SNV, 3, (5, "11M1D5N3M", REF[5:16] + REF[22:25]), (0, True), (0, False), 0, ("CGATCGG", "CGACCGG", "CGATCG")),
    ("D_behind_an_N", (0, REF), SNV, 3, (5, "12M5N1D2M", REF[5:17] + REF[23:25]), (0, True), (0, False), 0, ("CGATCGG", "CGACCGG", "CGATCGG")),
    # the slice ends behind 16: the intron and x_kt lie outside it and only the flank matters; it ends behind 15: position 16 of the flank is outside
    ("intron_outside_the_slice", (0, REF[:17]), SNV, 3, (5, "12M5N3M", REF[5:17] + REF[22:25]), (0, True), (0, False), 0, ("CGATCGG", "CGACCGG", "CGATCGG")),
    ("flank_outside_the_slice", (0, REF[:16]), SNV, 3, (5, "12M5N3M", REF[5:17] + REF[22:25]), (0, False), (0, False), 0, None),
    # a letter of the intron that is not A, C, G or T is never read
    ("n_in_the_intron", (0, REF[:18] + "NN" + REF[20:]), SNV, 3, (5, "12M5N3M", REF[5:17] + REF[22:25]), (0, True), (0, False), 0, ("CGATCGG", "CGACCGG", "CGATCGG")),
]
