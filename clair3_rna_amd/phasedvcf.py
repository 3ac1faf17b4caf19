"""Phased heterozygous SNVs of a phased VCF — what `whatshap phase` / `longphase phase` write between the two passes of the reference flow
(run_clair3_rna:729-767) — as the site table of the device's haplotagging (capi.Engine.set_phase_sites, include/c3r.h: c3r_set_phase_sites).

A row is kept when its REF and ALT are single characters of ACGTacgt and the first sample's GT is exactly `0|1` or `1|0`; `ps` is the integer
PS FORMAT field (0 when it is absent or `.`); FILTER is ignored; of several rows on one position the first is kept.  Everything else is
counted by reason and skipped: haplotagging here votes on biallelic SNVs only (no indels, no multi-allelic sites)."""
import numpy as np

from .capi import PHASE_SITE_DTYPE
from .io import _open_text

BASE_CODE = {"A": 1, "C": 2, "G": 4, "T": 8}                 # BAM 4-bit codes (reads.NT16)
SKIP_REASONS = ("other_contig", "malformed", "not_snv", "not_phased_het", "duplicate_pos")


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
