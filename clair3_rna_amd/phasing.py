"""The host side of the built-in phasing (include/c3r.h: c3r_phase_links / c3r_phase_resolve; capi.Engine.phase_sites): the candidate
sites of a contig from the first pass's VCF, and the phased VCF that the second pass reads back (phasedvcf.contig_sites) — what `whatshap
phase` / `longphase phase` read and write between the two passes of the reference flow (run_clair3_rna:729-767).

The rule is a greedy linkage chain over the reads that cover two heterozygous SNVs at once, not whatshap's wMEC; how far the two agree has
not been measured.

candidates_from_vcf keeps a row when FILTER is PASS, REF and ALT are single letters of ACGT and the first sample's GT is `0/1` or `1/0`; of
several rows on one position the first is kept; everything else is counted by reason and skipped."""
import gzip

import numpy as np

from .capi import PHASE_SITE_DTYPE
from .io import _open_text
from .phasedvcf import BASE_CODE

SKIP_REASONS = ("other_contig", "malformed", "not_pass", "not_snv", "not_het", "duplicate_pos")
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
