"""Phasing over an allele table, without a device: the restatement (tests/phaseindelref.py) against phaseref on SNV tables and on the
hand-made bridge, the rows `phase_vcf --indels` writes and their way back through phasedvcf.contig_alleles, and the drivers' refusals."""
import gzip
import os

import numpy as np
import pytest

from clair3_rna_amd import capi, phasedvcf, phasing
from tests import hapalleleref as HA
from tests import phaseindelref as PI
from tests import phaseref


def test_on_an_snv_only_table_the_restatement_is_phaserefs():
    for seed, errors in ((0, False), (1, True)):
        _, rs, sites, _, _ = phaseref.gen_case(seed, errors=errors)
        lk = PI.links(rs, HA.snv_sites(sites))
        assert np.array_equal(lk, phaseref.links(rs, sites)) and lk.sum() > 0
        ps, h1, st = PI.resolve(HA.snv_sites(sites), lk)
        out, st0 = phaseref.resolve(sites, lk)
        assert ps == out["ps"].tolist() and h1 == out["h1"].tolist() and st == st0


def test_the_hand_made_bridge():
    rs, hap = PI.bridge_reads()
    s1, d, s2 = PI.BRIDGE_SITES
    # no read covers s1 and s2 together
    site_at = {s["pos"]: (j, s) for j, s in enumerate(PI.BRIDGE_SITES)}
    for i in range(len(rs)):
        assert not {0, 2} <= set(HA.observe(rs, i, site_at))
    # the SNV-only chain leaves both unphased
    snv = phaseref.make_sites([(s1["pos"], "A", "G"), (s2["pos"], "A", "T")])
    out, st = phaseref.phase(rs, snv)
    assert out["ps"].tolist() == [-1, -1] and st["n_phased"] == 0
    # with d in the table all three share one block, oriented as the generator made them
    lk = PI.links(rs, PI.BRIDGE_SITES)
    assert lk[1, 0].tolist() == [0, 12] and lk[2, 0].tolist() == [0, 12] and lk[2, 1].tolist() == [0, 0]      # 6 reads a kind and haplotype, all trans
    ps, h1, st = PI.phase(rs, PI.BRIDGE_SITES)
    assert ps == [21, 21, 21] and st == dict(n_sites=3, n_phased=3, n_blocks=1, max_block=3)
    assert [a ^ b for a, b in zip(h1, PI.BRIDGE_TRUTH)] in ([0, 0, 0], [1, 1, 1])


# ---- phase_vcf --indels: the rows it writes, and the way back
HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
ROWS = [
    ("chr1", 21, "A", "G", "PASS", "GT:GQ", "0/1:9"),             # candidate: SNV
    ("chr1", 40, "C", "CAGT", "PASS", "GT", "1/0"),               # candidate: insertion
    ("chr1", 50, "T", "G", "PASS", "GT", "1/1"),                  # not a candidate: homozygous
    ("chr1", 61, "ACG", "A", "PASS", "GT", "0/1"),                # candidate: deletion
    ("chr1", 70, "G", "A,C,T", "PASS", "GT", "1/2"),              # not a candidate: three ALTs
    ("chr1", 80, "C", "T,CGG", "PASS", "GT:DP", "1/2:30"),        # candidate: two ALTs
    ("chr1", 90, "A", "C", "LowQual", "GT", "0/1"),               # not a candidate: FILTER
    ("chr1", 101, "A", "T", "PASS", "GT", "0/1"),                 # candidate: SNV, stays unphased below
    ("chr1", 110, "ACC", "A,TCC", "PASS", "GT", "2/1"),           # candidate: two ALTs, a deletion and an SNV
    ("chr2", 5, "A", "AGG", "PASS", "GT", "0/1"),                 # another contig: no reads there in the stub
]
RESOLVED = {21: (21, 0), 40: (21, 1), 61: (21, 0), 80: (21, 1), 101: (-1, 0), 110: (21, 1)}          # pos -> (ps, h1) the stub hands back for chr1


def _write(path, rows):
    with open(path, "w") as f:
        f.write(HEAD + "".join("%s\t%d\t.\t%s\t%s\t30\t%s\t.\t%s\t%s\n" % r for r in rows))
    return str(path)


class _Engine:
    """Stands where capi.Engine stands in phase_vcf: keeps what it is given, answers RESOLVED."""
    calls = []

    def __init__(self, gpu_id):
        pass

    def set_params(self, **kw):
        pass

    def load_reads(self, rs):
        pass

    def phase_sites(self, *a, **k):
        raise AssertionError("--indels phases with phase_allele_sites")

    def phase_allele_sites(self, sites, pool, min_reads, min_agree_pct, merge_levels):
        _Engine.calls.append((sites.copy(), pool.copy(), min_reads, min_agree_pct, merge_levels))
        res = [RESOLVED.get(int(p), (int(p), 0)) for p in sites["pos"]]
        ps, h1 = np.array([r[0] for r in res], np.int32), np.array([r[1] for r in res], np.uint8)
        n = int((ps >= 0).sum())
        return ps, h1, dict(n_sites=len(sites), n_phased=n, n_blocks=1, max_block=n, merge_levels_run=1, merge_units_joined=0)

    def close(self):
        pass


def test_phase_vcf_indels_rows_and_round_trip(tmp_path, monkeypatch):
    from clair3_rna_amd import io, phase_vcf
    vcf = _write(tmp_path / "pass1.vcf", ROWS)
    bam = tmp_path / "x.bam"
    bam.write_bytes(b"")
    monkeypatch.setattr(capi, "Engine", _Engine)
    monkeypatch.setattr(io, "load_reads", lambda fn, ctg: PI.bridge_reads()[0])
    _Engine.calls = []
    logs = []
    out = str(tmp_path / "phased_vcf")
    written = phase_vcf.Run(phase_vcf.build_parser().parse_args(["-b", str(bam), "--vcf_fn", vcf, "-o", out, "--indels", "--ctg_name", "chr1", "--merge_levels", "2"]), logs.append)
    assert written == [os.path.join(out, "phased_chr1.vcf.gz")] and len(_Engine.calls) == 1
    given, pool, min_reads, pct, levels = _Engine.calls[0]
    cand = phasing.allele_candidates_from_vcf(vcf, "chr1")
    assert np.array_equal(given, cand[0]) and np.array_equal(pool, cand[1]) and (min_reads, pct, levels) == (2, 75, 2)
    assert given["pos"].tolist() == [21, 40, 61, 80, 101, 110]
    # the [INFO] line counts the skip reasons of the candidates' parser
    assert len(logs) == 1 and logs[0].startswith("[INFO] chr1:") and "not_het 1" in logs[0] and "multi_alt 1" in logs[0] and "not_pass 1" in logs[0] and "other_contig" not in logs[0]
    # the rows: candidates with ps >= 0 rewritten, everything else byte for byte
    with gzip.open(written[0], "rt") as f:
        lines = f.read().split("\n")
    src = (HEAD + "".join("%s\t%d\t.\t%s\t%s\t30\t%s\t.\t%s\t%s\n" % r for r in ROWS if r[0] == "chr1")).split("\n")
    assert lines[0] == src[0] and lines[1] == phasing.PS_HEADER.rstrip("\n") and lines[2] == src[1]
    body, exp = lines[3:], src[2:]
    assert len(body) == len(exp)
    want_gt = {21: "0|1", 40: "1|0", 61: "0|1", 80: "2|1", 110: "2|1"}
    for got, was in zip(body, exp):
        f_ = was.split("\t")
        if len(f_) > 1 and int(f_[1]) in want_gt:
            vals = f_[9].split(":")
            vals[0] = want_gt[int(f_[1])]
            assert got == "\t".join(f_[:8] + [f_[8] + ":PS", ":".join(vals) + ":21"]), was
        else:
            assert got == was
    # the way back: exactly the table that was resolved
    sites, h1, pool2, pool_bases, skipped = phasedvcf.contig_alleles(out, "chr1")
    keep = np.array([RESOLVED[int(p)][0] >= 0 for p in given["pos"]])
    exp_sites = given[keep].copy()
    exp_sites["ps"] = [RESOLVED[int(p)][0] for p in exp_sites["pos"]]
    assert np.array_equal(sites, exp_sites) and h1.tolist() == [RESOLVED[int(p)][1] for p in exp_sites["pos"]]
    assert np.array_equal(pool2, pool) and pool_bases == 5          # AGT of 40, GG of 80 (the unphased site is an SNV: it holds no bases)
    assert skipped["not_phased_het"] == 4 and skipped["multi_alt"] == 0          # 50 (1/1), 70 (1/2 with three ALTs stays unphased), 90, 101
    # without --indels the same command asks for the SNV chain, as before
    with pytest.raises(AssertionError, match="phase_allele_sites"):
        phase_vcf.Run(phase_vcf.build_parser().parse_args(["-b", str(bam), "--vcf_fn", vcf, "-o", out, "--ctg_name", "chr1"]), logs.append)


def test_the_restatement_predicts_the_bridge_file(tmp_path):
    """The bridge's three rows through the writer with the restatement's answer: one block, PS = 21."""
    rs, _ = PI.bridge_reads()
    rows = [("chr1", s["pos"], s["ref"], s["alt"], "PASS", "GT", "0/1") for s in PI.BRIDGE_SITES]
    vcf = _write(tmp_path / "b.vcf", rows)
    sites, pool, strings, _ = phasing.allele_candidates_from_vcf(vcf, "chr1")
    assert np.array_equal(sites, HA.to_query(PI.BRIDGE_SITES)[0]) and len(pool) == 0
    ps, h1, _ = PI.phase(rs, PI.BRIDGE_SITES)
    fn = str(tmp_path / "phased_chr1.vcf.gz")
    assert phasing.write_allele_phased_vcf(vcf, "chr1", sites, strings, ps, h1, fn) == 3
    got, gh1, _, _, _ = phasedvcf.read_phase_alleles(fn, "chr1")
    assert got["ps"].tolist() == [21, 21, 21] and gh1.tolist() == h1


# ---- flags
def _no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(capi, "Engine", boom)


def test_the_flags_are_off_by_default():
    from clair3_rna_amd import call_sample, phase_vcf
    assert phase_vcf.build_parser().parse_args(["-b", "b", "--vcf_fn", "v", "-o", "o"]).indels is False
    assert call_sample.build_parser().parse_args(["-b", "b", "-f", "r", "-o", "o", "--pileup_model_path", "m"]).phasing_indels is False


def test_the_new_refusals(tmp_path, monkeypatch):
    from clair3_rna_amd import call_sample
    _no_engine(monkeypatch)
    out = str(tmp_path / "out")
    base = ["--bam_fn", str(tmp_path / "x.bam"), "--ref_fn", str(tmp_path / "x.fa"), "--output_dir", out, "--pileup_model_path", "m", "--phased_pileup_model_path", "m",
            "--enable_phasing_model"]
    # without --phasing builtin
    for extra in (["--phasing_indels"], ["--phasing_indels", "--phased_vcf_fn", str(tmp_path / "p.vcf")], ["--phasing_indels", "--phase_output"]):
        with pytest.raises(SystemExit) as e:
            call_sample.Run(call_sample.build_parser().parse_args(base + extra))
        msg = str(e.value.code)
        assert msg.startswith("[ERROR]") and "--phasing_indels" in msg and "--phasing builtin" in msg, extra
        assert not os.path.exists(out)
    # several ranks stay refused as for --phasing builtin
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        call_sample.Run(call_sample.build_parser().parse_args(base + ["--phasing", "builtin", "--phasing_indels"]))
    assert str(e.value.code).startswith("[ERROR]") and "one process" in str(e.value.code) and not os.path.exists(out)
    monkeypatch.delenv("WORLD_SIZE")
    # --haplotag_indels under --phasing builtin stays refused with the new flag too, and the message now names it
    with pytest.raises(SystemExit) as e:
        call_sample.Run(call_sample.build_parser().parse_args(base + ["--phasing", "builtin", "--phasing_indels", "--haplotag_indels"]))
    msg = str(e.value.code)
    assert msg.startswith("[ERROR]") and "SNV-only" in msg and msg.rstrip().endswith("tags the reads from them") and "--phasing_indels" in msg
    assert not os.path.exists(out)
