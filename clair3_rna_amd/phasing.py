"""The host side of the built-in phasing (include/c3r.h: c3r_phase_links / c3r_phase_resolve; capi.Engine.phase_sites): the candidate
sites of a contig from the first pass's VCF, and the phased VCF that the second pass reads back (phasedvcf.contig_sites) — what `whatshap
phase` / `longphase phase` read and write between the two passes of the reference flow (run_clair3_rna:729-767).

The rule is a greedy linkage chain over the reads that cover two heterozygous SNVs at once, not whatshap's wMEC; how far the two agree has
not been measured.

candidates_from_vcf keeps a row when FILTER is PASS, REF and ALT are single letters of ACGT and the first sample's GT is `0/1` or `1/0`; of
several rows on one position the first is kept; everything else is counted by reason and skipped.

allele_candidates_from_vcf / allele_phased_row are the same two steps for the FINAL VCF of a phased run under `hap_vcf --indels`
(include/c3r.h: c3r_hap_allele_counts states the rule): heterozygous rows whose alleles are SNVs, insertions or deletions, GT `0/1` / `1/0`
with one ALT or `1/2` / `2/1` with two.  The phasing between the two passes (phase_vcf) reads and writes them too under `phase_vcf
--indels` (write_allele_phased_vcf; include/c3r.h: c3r_phase_allele_links); without that flag it stays SNV-only."""
import gzip

import numpy as np

from .capi import HAP_EV_DEL, HAP_EV_INS, HAP_EV_NONE, HAP_SITE_DTYPE, PHASE_SITE_DTYPE, pack_nibbles
from .io import _open_text
from .phasedvcf import BASE_CODE

SKIP_REASONS = ("other_contig", "malformed", "not_pass", "not_snv", "not_het", "duplicate_pos")
# allele_candidates_from_vcf: the same reasons (not_snv stays 0 there) and three more
ALLELE_SKIP_REASONS = SKIP_REASONS + ("multi_alt", "complex_allele", "same_alleles")
PS_HEADER = '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set identifier">\n'


def _parse(lines, contig):
    """-> {contig: ([(pos, ref, alt)] in file order, {reason: rows skipped})}; contig None: every contig of the file."""
    out = {}
    other = 0
    for line in lines:
        if not line or line[0] == "#":
            continue
        f = line.rstrip("\r\n").split("\t")
        if not f[0] or f == [""]:
            continue
        if contig is not None and f[0] != contig:
            other += 1
            continue
        rows, skipped = out.setdefault(f[0], ([], dict.fromkeys(SKIP_REASONS, 0)))
        if len(f) < 10 or not f[1].isdigit() or int(f[1]) < 1:
            skipped["malformed"] += 1
            continue
        if f[6] != "PASS":
            skipped["not_pass"] += 1
            continue
        ref, alt = f[3].upper(), f[4].upper()
        if ref not in BASE_CODE or alt not in BASE_CODE or ref == alt:
            skipped["not_snv"] += 1
            continue
        keys, vals = f[8].split(":"), f[9].split(":")
        gt = vals[keys.index("GT")] if "GT" in keys and keys.index("GT") < len(vals) else ""
        if gt not in ("0/1", "1/0"):
            skipped["not_het"] += 1
            continue
        rows.append((int(f[1]), BASE_CODE[ref], BASE_CODE[alt]))
    if contig is not None:
        rows, skipped = out.setdefault(contig, ([], dict.fromkeys(SKIP_REASONS, 0)))
        skipped["other_contig"] = other
    return out


def _table(rows, skipped):
    rows = sorted(enumerate(rows), key=lambda kr: (kr[1][0], kr[0]))           # by position; rows of one position in file order
    keep, last = [], None
    for _, r in rows:
        if r[0] == last:
            skipped["duplicate_pos"] += 1
            continue
        keep.append(r)
        last = r[0]
    a = np.zeros(len(keep), dtype=PHASE_SITE_DTYPE)
    for k, name in enumerate(("pos", "ref", "alt")):
        a[name] = [r[k] for r in keep]
    return a, skipped


def candidates_from_vcf(vcf_fn, contig):
    """(unphased PHASE_SITE_DTYPE array sorted by pos — ps and h1 are 0 —, {reason: rows skipped}) for `contig` of a plain or gzipped
    VCF; contig None: {contig: (array, skipped)} for every contig of the file, in one pass."""
    with _open_text(vcf_fn) as f:
        per = _parse(f, contig)
    if contig is None:
        return {c: _table(rows, skipped) for c, (rows, skipped) in per.items()}
    return _table(*per[contig])


def reduce_allele(ref, alt):
    """One ALT of a row against its REF (the rule of include/c3r.h) -> (base letter, kind, length, inserted letters), or None when the pair
    is not an SNV, an insertion or a deletion anchored on POS (letters other than ACGT, a complex allele, an indel longer than 65535)."""
    r, a = ref.upper(), alt.upper()
    if not r or not a or set(r + a) - set("ACGT"):
        return None
    while len(r) > 1 and len(a) > 1 and r[-1] == a[-1]:
        r, a = r[:-1], a[:-1]
    if len(r) == 1 and len(a) == 1:
        return (a, HAP_EV_NONE, 0, "") if r != a else None
    if len(r) == 1 and a[0] == r and len(a) - 1 <= 0xffff:
        return (r, HAP_EV_INS, len(a) - 1, a[1:])
    if len(a) == 1 and r[0] == a and len(r) - 1 <= 0xffff:
        return (a, HAP_EV_DEL, len(r) - 1, "")
    return None


def _parse_alleles(lines, contig, phased=False):
    """-> {contig: ([(pos, allele A, allele B, REF string, ALT string)] in file order, {reason: rows skipped})}; an allele is
    reduce_allele's tuple.  The checks of a row, in this order: malformed, not_pass, not_het (GT is none of 0/1, 1/0, 1/2, 2/1, or 1/2 with
    one ALT), multi_alt (three or more ALTs, or two under GT 0/1), complex_allele (an allele does not reduce), same_alleles (two ALTs that
    reduce to one allele).
    phased (phasedvcf.read_phase_alleles: the rows of a PHASED VCF, the table that tags the reads): the same loop with the GTs 0|1, 1|0,
    1|2, 2|1 (reason not_phased_het), FILTER ignored, the reasons of phasedvcf.ALLELE_SKIP_REASONS, and two more elements in a row: ps — the
    integer PS field, 0 when it is absent or `.`, malformed when it is anything else — and h1 — 1 for 1|0 and 2|1."""
    from . import phasedvcf
    reasons = phasedvcf.ALLELE_SKIP_REASONS if phased else ALLELE_SKIP_REASONS
    sep, not_het = ("|", "not_phased_het") if phased else ("/", "not_het")
    out = {}
    other = 0
    for line in lines:
        if not line or line[0] == "#":
            continue
        f = line.rstrip("\r\n").split("\t")
        if not f[0] or f == [""]:
            continue
        if contig is not None and f[0] != contig:
            other += 1
            continue
        rows, skipped = out.setdefault(f[0], ([], dict.fromkeys(reasons, 0)))
        if len(f) < 10 or not f[1].isdigit() or int(f[1]) < 1:
            skipped["malformed"] += 1
            continue
        if not phased and f[6] != "PASS":
            skipped["not_pass"] += 1
            continue
        keys, vals = f[8].split(":"), f[9].split(":")
        gt = vals[keys.index("GT")] if "GT" in keys and keys.index("GT") < len(vals) else ""
        alts = f[4].split(",")
        two = gt in ("1" + sep + "2", "2" + sep + "1")
        if (gt not in ("0" + sep + "1", "1" + sep + "0") and not two) or (two and len(alts) < 2):
            skipped[not_het] += 1
            continue
        if len(alts) != (2 if two else 1):
            skipped["multi_alt"] += 1
            continue
        reduced = [reduce_allele(f[3], a) for a in alts]
        if None in reduced:
            skipped["complex_allele"] += 1
            continue
        if two and reduced[0] == reduced[1]:
            skipped["same_alleles"] += 1
            continue
        a, b = reduced if two else ((f[3][0].upper(), HAP_EV_NONE, 0, ""), reduced[0])
        row = (int(f[1]), a, b, f[3], f[4])
        if phased:
            ps = vals[keys.index("PS")] if "PS" in keys and keys.index("PS") < len(vals) else "."
            if ps not in (".", "") and not (ps.isdigit() and int(ps) < 2 ** 31):
                skipped["malformed"] += 1
                continue
            row += (0 if ps in (".", "") else int(ps), 1 if gt in ("1|0", "2|1") else 0)
        rows.append(row)
    if contig is not None:
        rows, skipped = out.setdefault(contig, ([], dict.fromkeys(reasons, 0)))
        skipped["other_contig"] = other
    return out


def _first_rows(rows, skipped):
    """The rows sorted by position, of several on one position the first of the file; the others are counted as duplicate_pos."""
    rows = sorted(enumerate(rows), key=lambda kr: (kr[1][0], kr[0]))           # by position; rows of one position in file order
    keep, last = [], None
    for _, r in rows:
        if r[0] == last:
            skipped["duplicate_pos"] += 1
            continue
        keep.append(r)
        last = r[0]
    return keep


def _allele_table(rows, skipped):
    keep = _first_rows(rows, skipped)
    sites, pool = _allele_sites(keep)
    return sites, pool, [(r[3], r[4]) for r in keep], skipped


def _allele_sites(keep):
    """(HAP_SITE_DTYPE array with ps = 0, packed pool of the insertions' bases) of the kept rows of _parse_alleles."""
    sites = np.zeros(len(keep), dtype=HAP_SITE_DTYPE)
    pool = []
    for k, (pos, a, b, *_) in enumerate(keep):
        s = sites[k]
        s["pos"] = pos
        s["base_matters"] = int(any(x[1] == HAP_EV_NONE and x[0] != keep[k][3][0].upper() for x in (a, b)))     # one of them is an SNV
        s["event_matters"] = int(any(x[1] != HAP_EV_NONE for x in (a, b)))
        for name, (base, kind, length, ins) in (("a", a), ("b", b)):
            s[name + "_base"], s[name + "_kind"], s[name + "_len"] = BASE_CODE[base], kind, length
            if kind == HAP_EV_INS:
                s[name + "_ins_off"] = len(pool)
                pool += [BASE_CODE[c] for c in ins]
    return sites, pack_nibbles(pool)


LEFT_ALIGN_REASONS = ("not_left_alignable", "same_pos_after_left_align")


class LeftAligned(dict):
    """{reason: rows skipped} of a table that left_align_table has been through — the reasons of the parse and LEFT_ALIGN_REASONS — with
    `moved`: the sites whose anchor moved.  Compares like the plain dict."""

    def __init__(self, skipped, stats):
        dict.__init__(self, skipped)
        self.update({k: stats["n_" + k] for k in LEFT_ALIGN_REASONS})
        self.moved = stats["n_moved"]


def left_align_table(sites, pool, ref, pool_bases=None):
    """The one place where a driver's table meets --left_align_indels (include/c3r.h: c3r_hap_left_align_sites, host code): a
    HAP_SITE_DTYPE array and its pool, and `ref` = (1-based position of the slice's first base, the slice: str / bytes / uint8 array) ->
    (the sites that stay, left-aligned and sorted by pos; their pool; the bases in it; the input index of every output site; the
    statistics).  A site whose alleles cannot move together is dropped (`not_left_alignable`), and so is the later of two that land on one
    position (`same_pos_after_left_align`)."""
    from .capi import hap_left_align_sites
    return hap_left_align_sites(sites, pool, ref[0], ref[1], pool_bases)


def left_align_note(skipped):
    """A driver's words about what --left_align_indels did to a table, and "" without the flag (`skipped` is then a plain dict)."""
    return ", %d left-aligned" % skipped.moved if isinstance(skipped, LeftAligned) else ""


def hap_min_bq_arg(args, has_consumer, needs):
    """A driver's --hap_min_bq (0: off, also when the parser has no such flag); refuses a value outside 0 .. 93 and the flag without a
    step that holds reads against a site table (`has_consumer`; `needs`: what the message asks for)."""
    import sys
    q = int(getattr(args, "hap_min_bq", 0) or 0)
    if q == 0:
        return 0
    if not 0 < q <= 93:
        sys.exit("[ERROR] --hap_min_bq must lie between 0 and 93 (phred; 0: off)")
    if not has_consumer:
        sys.exit("[ERROR] --hap_min_bq needs %s (it masks low-quality bases for the steps that hold reads against a site table)" % needs)
    return q


def reads_without_quals(rs):
    """How many reads of a ReadSet with qualities have bases and no quality (BAM: 0xff throughout; the first byte says it)."""
    r = rs.reads[rs.reads["l_seq"] > 0]
    return int((rs.qual[2 * r["seq_off"].astype(np.int64)] == 0xff).sum()) if len(r) else 0


def load_reads_min_bq(eng, rs, q, ctg, log, weights=False):
    """The one place where a driver's engine meets --hap_min_bq (include/c3r.h: c3r_set_hap_min_bq): Engine.load_reads under the
    threshold q.  q = 0: the plain load, nothing else.  Otherwise `rs` must carry qualities (io.load_reads(..., want_quals=True)); the
    threshold is set before the load, one [INFO] line gives masked / total bases, and one [WARNING] line counts the reads without
    qualities when there are any — they are not refused: none of their bases is masked.
    weights: --hap_bq_weights, which needs the same qualities on the same way (apply_hap_bq_weights, before the load)."""
    apply_hap_bq_weights(eng, weights, rs, ctg, log)
    if not q:
        eng.load_reads(rs)
        return
    if getattr(rs, "qual", None) is None:
        raise ValueError("--hap_min_bq %d: the reads of %s were fetched without their qualities" % (q, ctg))
    eng.set_hap_min_bq(q)
    eng.load_reads(rs)
    total = int(rs.reads["l_seq"].sum(dtype=np.int64)) if len(rs.reads) else 0
    log("[INFO] %s: --hap_min_bq %d: %d of %d bases masked for haplotagging, counts and phasing votes" % (ctg, q, eng.hap_min_bq()[1], total))
    without = reads_without_quals(rs)
    if without:
        log("[WARNING] %s: %d of %d reads carry no base qualities: --hap_min_bq masks none of their bases" % (ctg, without, len(rs.reads)))


def add_hap_bq_weights_flag(add, where=""):
    """--hap_bq_weights on a driver's parser (`add`: its add_argument; `where`: what the driver has to say about its own steps)."""
    add("--hap_bq_weights", action="store_true",
        help="%sweigh every haplotag vote by the quality of the read's base on the site where it otherwise counts 1 (include/c3r.h: "
             "c3r_set_hap_bq_weights; default off): one Q30 base outvotes two Q5 bases, a base without a quality weighs 1.  The tagging only: "
             "the count tables and the links of the built-in phasing stay unweighted.  An indel's own quality and the inserted bases' are "
             "not modelled; under --hap_realign the weight is still the anchor base's; that whatshap weights by phred is recalled, not "
             "checked; agreement with whatshap is not measured" % where)


def hap_bq_weights_arg(args, has_consumer=True, needs=""):
    """A driver's --hap_bq_weights (False also when the parser has no such flag); refuses the flag without a step that tags reads
    (`has_consumer`; `needs`: what the message asks for)."""
    import sys
    if not getattr(args, "hap_bq_weights", False):
        return False
    if not has_consumer:
        sys.exit("[ERROR] --hap_bq_weights needs %s (it weighs the votes of the step that haplotags the reads from a site table)" % needs)
    return True


def apply_hap_bq_weights(eng, on, rs, ctg, log):
    """The one place where a driver's engine meets --hap_bq_weights (include/c3r.h: c3r_set_hap_bq_weights), before the contig's reads
    are loaded: `rs` must carry qualities (io.load_reads(..., want_quals=True)); one [WARNING] line counts the reads without qualities
    when there are any — they are not refused: their votes weigh 1."""
    if not on:
        return
    if getattr(rs, "qual", None) is None:
        raise ValueError("--hap_bq_weights: the reads of %s were fetched without their qualities" % ctg)
    eng.set_hap_bq_weights(True)
    without = reads_without_quals(rs)
    if without:
        log("[WARNING] %s: %d of %d reads carry no base qualities: under --hap_bq_weights each of their votes weighs 1" % (ctg, without, len(rs.reads)))


HAP_REALIGN_DEFAULT = 10      # --hap_realign without a value (recalled as whatshap's default overhang, not checked)


def add_hap_realign_flag(add):
    """--hap_realign [W] on a driver's parser (`add`: its add_argument)."""
    add("--hap_realign", type=int, nargs="?", const=HAP_REALIGN_DEFAULT, default=0, metavar="W",
        help="realign every read's window of W reference bases around a site against the site's two alleles before deciding which one the read "
             "shows (include/c3r.h: c3r_set_hap_realign; W = 1 .. 16, %d without a value, default off; needs --ref_fn, excludes "
             "--left_align_indels).  Unit costs, no quality weights, no affine gaps; a window stops at a splice junction unless "
             "--hap_realign_spliced is given; agreement with whatshap is not measured" % HAP_REALIGN_DEFAULT)
    add("--hap_realign_spliced", action="store_true",
        help="with --hap_realign: count a read's window in the read's own spliced positions, so that it crosses an N op and follows the read's "
             "splicing on the reference side (include/c3r.h: c3r_set_hap_realign_spliced; default off).  A junction inside a site's core "
             "still falls back to the CIGAR-position allele")


def hap_realign_arg(args, has_consumer=True, needs=""):
    """A driver's --hap_realign: (W, contig -> (1-based start, reference slice)), or (0, None) without the flag (also when the parser has
    none).  Refuses a value outside 1 .. 16, the flag beside --left_align_indels, without a step that holds reads against a table
    (`needs` names it) and without --ref_fn."""
    import os
    import sys
    from . import io
    w = getattr(args, "hap_realign", 0)
    w = 0 if w is None else int(w)
    if w == 0 and hap_realign_spliced_arg(args):
        sys.exit("[ERROR] --hap_realign_spliced needs --hap_realign (it says how the window of --hap_realign is counted)")
    if w == 0:
        return 0, None
    if not 1 <= w <= 16:
        sys.exit("[ERROR] --hap_realign must lie between 1 and 16 (the overhang in reference bases; without a value: %d)" % HAP_REALIGN_DEFAULT)
    if getattr(args, "left_align_indels", False):
        sys.exit("[ERROR] --hap_realign and --left_align_indels exclude each other (include/c3r.h: c3r_set_hap_realign)")
    if not has_consumer:
        sys.exit("[ERROR] --hap_realign needs %s (it realigns reads for the steps that hold them against a site table)" % needs)
    ref_fn = getattr(args, "ref_fn", None)
    if not ref_fn:
        sys.exit("[ERROR] --hap_realign needs --ref_fn")
    if not os.path.isfile(ref_fn):
        sys.exit("[ERROR] file %s not found" % ref_fn)
    return w, io.contig_reference(ref_fn)


def hap_realign_spliced_arg(args):
    """A driver's --hap_realign_spliced (False when the parser has none); hap_realign_arg refuses it without --hap_realign."""
    return bool(getattr(args, "hap_realign_spliced", False))


def snv_sites_as_alleles(sites):
    """A PHASE_SITE_DTYPE table as the allele table that says the same (include/c3r.h: on REF-and-one-SNV sites the allele calls give the
    SNV calls' results bit for bit with the switches off): (HAP_SITE_DTYPE array with A = REF and B = ALT, uint8 h1).  Under --hap_realign
    a step that would use the SNV table goes through this, so that only the observation changes."""
    import numpy as np
    from .capi import HAP_SITE_DTYPE
    out = np.zeros(len(sites), dtype=HAP_SITE_DTYPE)
    out["pos"], out["ps"], out["base_matters"] = sites["pos"], sites["ps"], 1
    out["a_base"], out["b_base"] = sites["ref"], sites["alt"]
    return out, np.ascontiguousarray(sites["h1"], dtype=np.uint8)


def apply_hap_realign(eng, w, ref, spliced=False, **how):
    """The one place where a driver's engine meets --hap_realign and --hap_realign_spliced (include/c3r.h: c3r_set_hap_realign,
    c3r_set_hap_realign_spliced), before the contig's table and reads: the reference slice that covers every read of the contig (`ref`:
    (1-based start, letters); `how`: Engine.set_reference's options), then the switches.  Without --hap_realign_spliced the engine's
    second switch is never touched."""
    if w:
        eng.set_reference(*ref, **how)
        if spliced:
            eng.set_hap_realign_spliced(True)
        eng.set_hap_realign(w)


def _left_aligned_candidates(table, ref):
    """_allele_table's tuple after left_align_table; a row's strings get a third element, the row's own POS (the site may have moved)."""
    sites, pool, strings, skipped = table
    out, opool, _, src, st = left_align_table(sites, pool, ref)
    return out, opool, [(strings[j][0], strings[j][1], int(sites["pos"][j])) for j in src], LeftAligned(skipped, st)


def row_pos(sites, strings, j):
    """The POS of the VCF row that site j of a candidate table came from: the site's own unless --left_align_indels moved it."""
    return strings[j][2] if len(strings[j]) > 2 else int(sites["pos"][j])


def allele_candidates_from_vcf(vcf_fn, contig, left_align=None):
    """(HAP_SITE_DTYPE array sorted by pos — ps is 0 —, the packed pool of the insertions' bases (capi.pack_nibbles), [(REF string, ALT
    string)] of the rows as the file spells them, {reason: rows skipped}) for `contig` of a plain or gzipped VCF; contig None: {contig: that
    tuple} for every contig of the file, in one pass.  A row is kept when FILTER is PASS, its GT is `0/1` / `1/0` with one ALT (A = REF,
    B = the ALT) or `1/2` / `2/1` with two ALTs (A = the first, B = the second), every ALT reduces to an SNV, an insertion or a deletion
    anchored on POS (reduce_allele) and the two alleles differ; of several such rows on one position the first is kept.
    left_align (--left_align_indels; None: off): a function contig -> (1-based start, reference slice).  The table then goes through
    left_align_table: sites may move to the left and some are dropped, the dict is a LeftAligned, and a row's strings are (REF, ALT, the
    row's POS)."""
    with _open_text(vcf_fn) as f:
        per = _parse_alleles(f, contig)
    done = {c: _allele_table(rows, skipped) for c, (rows, skipped) in per.items()}
    if left_align is not None:
        done = {c: _left_aligned_candidates(t, left_align(c)) for c, t in done.items()}
    return done if contig is None else done[contig]


def phased_only(sites_out):
    """The sites that got a block (ps >= 0): what goes to Engine.set_phase_sites."""
    return np.ascontiguousarray(sites_out[sites_out["ps"] >= 0])


def header_row(line, has_ps):
    """A header line of a VCF that is being phased -> (text to write, has_ps): the ##FORMAT line for PS goes before the #CHROM line unless the
    header has one."""
    has_ps = has_ps or line.startswith("##FORMAT=<ID=PS,")
    if line.startswith("#CHROM") and not has_ps:
        return PS_HEADER + line, has_ps
    return line, has_ps


def phased_row(line, f_, phased):
    """One data row (`f_`: its tab-separated fields) -> (text to write, rewritten): the first row on the position of a site of `phased`
    ({pos: site with ps >= 0}) whose REF and ALT are that site's, FILTER PASS and GT `0/1` or `1/0`, gets GT `0|1` / `1|0`, a PS key appended
    to FORMAT and its value appended to the sample column, and the site leaves `phased` (a later row on the position stays as it is); every
    other row comes back byte for byte."""
    s = phased.get(int(f_[1])) if len(f_) >= 10 and f_[1].isdigit() else None
    keys = f_[8].split(":") if s is not None else []
    if (s is None or "GT" not in keys or "PS" in keys or f_[6] != "PASS" or BASE_CODE.get(f_[3].upper()) != int(s["ref"])
            or BASE_CODE.get(f_[4].upper()) != int(s["alt"])):
        return line, False
    vals = f_[9].split(":")
    if keys.index("GT") >= len(vals) or vals[keys.index("GT")] not in ("0/1", "1/0"):
        return line, False
    vals[keys.index("GT")] = "1|0" if int(s["h1"]) else "0|1"
    f_ = list(f_)
    f_[8], f_[9] = f_[8] + ":PS", ":".join(vals) + ":%d" % int(s["ps"])
    del phased[int(f_[1])]
    return "\t".join(f_) + line[len(line.rstrip("\r\n")):], True


def allele_phased_row(line, f_, phased):
    """phased_row for the candidates of allele_candidates_from_vcf.  `phased`: {pos: (REF string, ALT string, ps, h1)} of the accepted
    candidates.  The first row on such a position whose REF and ALT are those strings, FILTER PASS, without a PS key and with GT `0/1` /
    `1/0` (one ALT) or `1/2` / `2/1` (two ALTs) gets GT A|B — `0|1`, `1|2` — when h1 is 0 and B|A — `1|0`, `2|1` — when it is 1, and PS as
    phased_row writes it; the site leaves `phased`.  Every other row comes back byte for byte."""
    s = phased.get(int(f_[1])) if len(f_) >= 10 and f_[1].isdigit() else None
    keys = f_[8].split(":") if s is not None else []
    if s is None or "GT" not in keys or "PS" in keys or f_[6] != "PASS" or f_[3] != s[0] or f_[4] != s[1]:
        return line, False
    vals = f_[9].split(":")
    two = "," in s[1]
    if keys.index("GT") >= len(vals) or vals[keys.index("GT")] not in (("1/2", "2/1") if two else ("0/1", "1/0")):
        return line, False
    a, b = ("1", "2") if two else ("0", "1")
    vals[keys.index("GT")] = b + "|" + a if int(s[3]) else a + "|" + b
    f_ = list(f_)
    f_[8], f_[9] = f_[8] + ":PS", ":".join(vals) + ":%d" % int(s[2])
    del phased[int(f_[1])]
    return "\t".join(f_) + line[len(line.rstrip("\r\n")):], True


def write_phased_vcf(in_vcf, contig, sites_out, out_fn):
    """Write `contig`'s rows of the first pass's VCF `in_vcf` to the gzipped VCF `out_fn`: the first row on the position of a phased site
    (Engine.phase_sites: ps >= 0) whose REF and ALT are that site's gets GT `0|1` / `1|0`, a PS key appended to FORMAT and its value
    appended to the sample column; every other row is written byte for byte as it was.  The header gets a ##FORMAT line for PS before
    the #CHROM line unless it has one.  Returns the number of rows rewritten.  (The per-row part is header_row / phased_row, which
    hap_vcf's writer shares.)"""
    phased = {int(s["pos"]): s for s in sites_out if int(s["ps"]) >= 0}
    n, has_ps = 0, False
    with _open_text(in_vcf) as f, gzip.open(out_fn, "wt") as out:
        for line in f:
            if line.startswith("#"):
                text, has_ps = header_row(line, has_ps)
                out.write(text)
                continue
            f_ = line.rstrip("\r\n").split("\t")
            if f_[0] != contig:
                continue
            text, done = phased_row(line, f_, phased)
            out.write(text)
            n += int(done)
    return n


def write_allele_phased_vcf(in_vcf, contig, sites, strings, ps, h1, out_fn):
    """write_phased_vcf for `phase_vcf --indels`: `sites` and `strings` as allele_candidates_from_vcf gives them for `contig`, `ps` / `h1`
    per site as Engine.phase_allele_sites leaves them (ps < 0: the site stays unphased).  The rows of the phased sites are rewritten by
    allele_phased_row (`0|1` / `1|0` / `1|2` / `2|1` + PS), every other row is written byte for byte.  Returns the number of rows rewritten."""
    phased = {row_pos(sites, strings, j): (strings[j][0], strings[j][1], int(ps[j]), int(h1[j])) for j in range(len(sites)) if int(ps[j]) >= 0}
    n, has_ps = 0, False
    with _open_text(in_vcf) as f, gzip.open(out_fn, "wt") as out:
        for line in f:
            if line.startswith("#"):
                text, has_ps = header_row(line, has_ps)
                out.write(text)
                continue
            f_ = line.rstrip("\r\n").split("\t")
            if f_[0] != contig:
                continue
            text, done = allele_phased_row(line, f_, phased)
            out.write(text)
            n += int(done)
    return n
