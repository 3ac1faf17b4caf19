"""Phased heterozygous SNVs of a phased VCF — what `whatshap phase` / `longphase phase` write between the two passes of the reference flow
(run_clair3_rna:729-767) — as the site table of the device's haplotagging (capi.Engine.set_phase_sites, include/c3r.h: c3r_set_phase_sites).

A row is kept when its REF and ALT are single characters of ACGTacgt and the first sample's GT is exactly `0|1` or `1|0`; `ps` is the integer
PS FORMAT field (0 when it is absent or `.`); FILTER is ignored; of several rows on one position the first is kept.  Everything else is
counted by reason and skipped: that table votes on biallelic SNVs only (no indels, no multi-allelic sites).

read_phase_alleles / read_all_phase_alleles / contig_alleles are the same for the table of capi.Engine.set_phase_alleles (include/c3r.h:
c3r_set_phase_alleles; --haplotag_indels): a row is kept when the first sample's GT is exactly `0|1` / `1|0` with one ALT (allele A = REF,
B = the ALT) or `1|2` / `2|1` with two ALTs (A = the first, B = the second) and every ALT reduces to an SNV, an insertion or a deletion
anchored on POS (phasing._parse_alleles and reduce_allele: one row loop and one implementation of that rule for both files); h1 is 1 for `1|0` and `2|1`.  PS, FILTER and rows that share a
position are treated as above.  On a file of biallelic SNV rows the kept positions, ps and orientation are read_phase_sites'."""
import numpy as np

from .capi import HAP_EV_INS, HAP_SITE_DTYPE, PHASE_SITE_DTYPE
from .io import _open_text

BASE_CODE = {"A": 1, "C": 2, "G": 4, "T": 8}                 # BAM 4-bit codes (reads.NT16)
SKIP_REASONS = ("other_contig", "malformed", "not_snv", "not_phased_het", "duplicate_pos")
# read_phase_alleles: the same reasons (not_snv stays 0 there) and three more, with the meanings they have in phasing.py
ALLELE_SKIP_REASONS = SKIP_REASONS + ("multi_alt", "complex_allele", "same_alleles")


def contig_file(path, contig):
    """The file that holds `contig`'s phased variants: `path` itself, or <path>/phased_<contig>.vcf.gz when `path` is a directory (what the
    reference's phasing step writes, run_clair3_rna:740,753) — None when the directory has no file for the contig (nothing was phased
    there).  Exits with an [ERROR] line when `path` is neither a file nor a directory."""
    import os
    import sys
    if os.path.isdir(path):
        fn = os.path.join(path, "phased_%s.vcf.gz" % contig)
        return fn if os.path.isfile(fn) else None
    if not os.path.isfile(path):
        sys.exit("[ERROR] file %s not found" % path)
    return path


def contig_sites(path, contig):
    """The site table of `contig` from a phased VCF or a directory of per-contig ones (contig_file); empty when nothing was phased there."""
    fn = contig_file(path, contig)
    return read_phase_sites(fn, contig)[0] if fn else np.zeros(0, dtype=PHASE_SITE_DTYPE)


def _parse(lines, contig):
    """-> {contig: ([(pos, ps, ref, alt, h1)] in file order, {reason: rows skipped})}; contig None: every contig of the file."""
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
        ref, alt = f[3].upper(), f[4].upper()
        if ref not in BASE_CODE or alt not in BASE_CODE or ref == alt:
            skipped["not_snv"] += 1
            continue
        keys, vals = f[8].split(":"), f[9].split(":")
        gt = vals[keys.index("GT")] if "GT" in keys and keys.index("GT") < len(vals) else ""
        if gt not in ("0|1", "1|0"):
            skipped["not_phased_het"] += 1
            continue
        ps = vals[keys.index("PS")] if "PS" in keys and keys.index("PS") < len(vals) else "."
        if ps in (".", ""):
            ps = 0
        elif ps.isdigit() and int(ps) < 2 ** 31:
            ps = int(ps)
        else:
            skipped["malformed"] += 1
            continue
        rows.append((int(f[1]), ps, BASE_CODE[ref], BASE_CODE[alt], 1 if gt == "1|0" else 0))
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
    for k, name in enumerate(("pos", "ps", "ref", "alt", "h1")):
        a[name] = [r[k] for r in keep]
    return a, skipped


def read_phase_sites(vcf_fn, contig):
    """(PHASE_SITE_DTYPE array sorted by pos, {reason: rows skipped}) for `contig` of a plain or gzipped VCF."""
    with _open_text(vcf_fn) as f:
        rows, skipped = _parse(f, contig)[contig]
    return _table(rows, skipped)


def read_all_phase_sites(vcf_fn):
    """{contig: (array, skipped)} for every contig of the file, in one pass (call_sample with one VCF for the whole sample)."""
    with _open_text(vcf_fn) as f:
        per = _parse(f, None)
    return {c: _table(rows, skipped) for c, (rows, skipped) in per.items()}


# ---- the table of Engine.set_phase_alleles: SNVs, insertions, deletions and two-ALT rows
def _allele_table(rows, skipped, ref=None):
    """read_phase_alleles' tuple from the rows of phasing._parse_alleles(phased=True): (pos, allele A, allele B, REF, ALT, ps, h1).
    ref (--left_align_indels; None: off): (1-based start, reference slice) — the table goes through phasing.left_align_table."""
    from . import phasing                                    # (phasing imports this module: not at import time)
    keep = phasing._first_rows(rows, skipped)
    sites, pool = phasing._allele_sites(keep)                 # (flags and pool: as for hap_vcf --indels)
    sites["ps"] = [r[5] for r in keep]
    h1 = np.array([r[6] for r in keep], dtype=np.uint8)
    moved = None
    if ref is not None:
        sites, pool, _, src, st = phasing.left_align_table(sites, pool, ref)
        keep, h1 = [keep[j] for j in src], np.ascontiguousarray(h1[src])
        skipped, moved = dict(skipped, **{k: st["n_" + k] for k in phasing.LEFT_ALIGN_REASONS}), st["n_moved"]
    pool_bases = int(sum(int(sites[n + "_len"][sites[n + "_kind"] == HAP_EV_INS].sum()) for n in "ab"))
    return sites, h1, pool, pool_bases, Skipped(skipped, indel=int((sites["event_matters"] != 0).sum()), two_alt=sum("," in r[4] for r in keep), moved=moved)


class Skipped(dict):
    """{reason: rows skipped} of an allele table, with `kept`: dict(indel = the sites kept with an insertion or deletion among their two
    alleles, two_alt = the sites kept from rows with two ALTs) — what the drivers' [INFO] lines count — and, under --left_align_indels,
    `moved`: the sites whose anchor moved (None without the flag).  Compares like the plain dict."""

    def __init__(self, skipped, indel=0, two_alt=0, moved=None):
        dict.__init__(self, skipped)
        self.kept = dict(indel=indel, two_alt=two_alt)
        self.moved = moved


def empty_alleles():
    """The empty table of set_phase_alleles: (sites, h1, pool, pool_bases, skipped)."""
    return np.zeros(0, dtype=HAP_SITE_DTYPE), np.zeros(0, np.uint8), np.zeros(0, np.uint8), 0, Skipped(dict.fromkeys(ALLELE_SKIP_REASONS, 0))


def read_phase_alleles(vcf_fn, contig, left_align=None):
    """(HAP_SITE_DTYPE array sorted by pos, uint8 h1 per site, packed pool of the insertions' bases, number of bases in the pool, {reason: rows
    skipped}) for `contig` of a plain or gzipped VCF: the arguments of Engine.set_phase_alleles.  left_align (--left_align_indels; None:
    off): a function contig -> (1-based start, reference slice); the table is then left-aligned against it (_allele_table)."""
    from . import phasing
    with _open_text(vcf_fn) as f:
        rows, skipped = phasing._parse_alleles(f, contig, phased=True)[contig]
    return _allele_table(rows, skipped, left_align(contig) if left_align else None)


def read_all_phase_alleles(vcf_fn, left_align=None):
    """{contig: read_phase_alleles' tuple} for every contig of the file, in one pass."""
    from . import phasing
    with _open_text(vcf_fn) as f:
        per = phasing._parse_alleles(f, None, phased=True)
    return {c: _allele_table(*v, left_align(c) if left_align else None) for c, v in per.items()}


def contig_alleles(path, contig):
    """read_phase_alleles' tuple for `contig` from a phased VCF or a directory of per-contig ones (contig_file); the empty table when nothing
    was phased there."""
    fn = contig_file(path, contig)
    return read_phase_alleles(fn, contig) if fn else empty_alleles()


class PhaseTable(object):
    """One contig's table, of either kind: `sites` (sorted by pos; the fields pos and ps exist in both dtypes), `skipped` ({reason: rows
    skipped}) and `kept` (dict(indel, two_alt): both 0 in the table of biallelic SNVs).  len() is the number of sites."""

    def __init__(self, sites, skipped, rest=()):
        self.sites, self.skipped, self._rest = sites, skipped, rest             # _rest: (h1, pool, pool_bases) of an allele table
        self.kept = getattr(skipped, "kept", dict(indel=0, two_alt=0))
        self.pos, self.ps = sites["pos"], sites["ps"]

    def __len__(self):
        return len(self.sites)


class PhaseSource(object):
    """What `--phased_vcf_fn PATH [--haplotag_indels]` means, for every driver: which table a contig gets (`table`), and which engine call
    takes it (`apply`).  PATH is a directory of phased_<ctg>.vcf.gz, read file by file, or one VCF for all contigs, parsed once by
    whichever thread asks first (call_sample asks from its fetch threads) — or, with `only`, for that one contig alone (the per-chunk
    driver never asks for another).  A contig without a file or without a row gets the empty table of the source's kind."""

    def __init__(self, path, tag_indels=False, only=None, left_align=None, realign=0):
        """left_align (--left_align_indels, with tag_indels only; None: off): a function contig -> (1-based start, reference slice).  The
        allele table is left-aligned against it where it is read, and `apply` switches the engine's observation to match."""
        import os
        import sys
        import threading
        if not os.path.exists(path):
            sys.exit("[ERROR] file %s not found" % path)
        if left_align is not None and not tag_indels:
            sys.exit("[ERROR] --left_align_indels needs --haplotag_indels")
        self.path, self.tag_indels, self.only, self.left_align = path, bool(tag_indels), only, left_align
        self.realign = int(realign)                           # --hap_realign (0: off): apply hands an SNV table to the allele call
        self.per_contig = os.path.isdir(path) or only is not None
        self.all, self.lock = None, threading.Lock()

    def table(self, contig):
        if self.per_contig:
            fn = contig_file(self.path, contig)
            extra = () if self.left_align is None else (self.left_align,)
            hit = (read_phase_alleles(fn, contig, *extra) if self.tag_indels else read_phase_sites(fn, contig)) if fn else None
        else:
            with self.lock:
                if self.all is None:
                    extra = () if self.left_align is None else (self.left_align,)
                    self.all = read_all_phase_alleles(self.path, *extra) if self.tag_indels else read_all_phase_sites(self.path)
            hit = self.all.get(contig)
        if self.tag_indels:
            sites, h1, pool, pool_bases, skipped = hit or empty_alleles()
            return PhaseTable(sites, skipped, (h1, pool, pool_bases))
        return PhaseTable(*(hit or (np.zeros(0, dtype=PHASE_SITE_DTYPE), dict.fromkeys(SKIP_REASONS, 0))))

    def apply(self, engine, table):
        """Before the contig's reads: they are tagged while they are prepared.  Under --left_align_indels the caller has set a reference
        slice that covers the contig's reads before this."""
        if self.tag_indels:
            if self.left_align is not None:
                engine.set_hap_left_align(True)
            engine.set_phase_alleles(table.sites, *table._rest)
        elif self.realign and len(table):
            from . import phasing
            sites, h1 = phasing.snv_sites_as_alleles(table.sites)
            engine.set_phase_alleles(sites, h1)
        else:
            engine.set_phase_sites(table.sites)

    def indel_note(self, table, head, tail=""):
        """A driver's words about the table of --haplotag_indels — `head`, the two counts, `tail` — and "" without the flag."""
        if not self.tag_indels:
            return ""
        moved = getattr(table.skipped, "moved", None)
        la = "" if moved is None else ", --left_align_indels: %d left-aligned, %d not_left_alignable, %d same_pos_after_left_align" % (
            moved, table.skipped.get("not_left_alignable", 0), table.skipped.get("same_pos_after_left_align", 0))
        return "%s%d with an insertion or deletion, %d with two ALTs%s%s" % (head, table.kept["indel"], table.kept["two_alt"], la, tail)
