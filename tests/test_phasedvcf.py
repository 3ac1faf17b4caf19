"""phasedvcf.PhaseSource: the one place that decides which phase table a contig gets from `--phased_vcf_fn` (one VCF or a directory of
phased_<ctg>.vcf.gz) with or without `--haplotag_indels`, and which engine call takes it.  CPU-only."""
import gzip
import os
import threading

import numpy as np
import pytest

from clair3_rna_amd import phasedvcf

HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
ROWS = {      # chr1: rows only the allele table keeps, a duplicate position, an unphased row; chr2: SNVs; chr4: a file whose only row is unphased
    "chr1": [(1200, "A", "G", "0|1:1200"), (2500, "C", "T", "1|0:1200"), (2500, "C", "G", "0|1:1200"), (2600, "G", "GAC", "0|1:1200"),
             (2700, "TCA", "T", "1|0:1200"), (3100, "A", "C,G", "1|2:1200"), (9000, "T", "C", "0/1:."), (20500, "G", "A", "1|0:20500")],
    "chr2": [(700, "C", "A", "0|1:700"), (15000, "G", "T", "0|1:15000")],
    "chr4": [(50, "C", "A", "0/1:.")],
}
CONTIGS = ["chr1", "chr2", "chr3", "chr4"]          # chr3: no file in the directory, no row in the single VCF


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("phased"))
    text = {c: "".join("%s\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:PS\t%s\n" % (c, p, r, a, g) for p, r, a, g in rows) for c, rows in ROWS.items()}
    one, per = os.path.join(tmp, "all.vcf"), os.path.join(tmp, "dir")
    with open(one, "w") as f:
        f.write(HEAD + "".join(text.values()))
    os.makedirs(per)
    for c, rows in text.items():
        with gzip.open(os.path.join(per, "phased_%s.vcf.gz" % c), "wt") as f:
            f.write(HEAD + rows)
    return one, per


def _handed(src, table):
    """What `apply` hands the engine: the setter's arguments."""
    eng = _Recorder()
    src.apply(eng, table)
    return eng.calls[0][1]


def _same(src, table, want_arrays, want_skipped):
    assert len(table) == len(want_arrays[0]) == len(table.pos) == len(table.ps)
    assert len(_handed(src, table)) == len(want_arrays)
    for got, want in zip(_handed(src, table), want_arrays):
        assert np.array_equal(got, want) and np.asarray(got).dtype == np.asarray(want).dtype
    assert np.array_equal(table.pos, want_arrays[0]["pos"]) and np.array_equal(table.ps, want_arrays[0]["ps"])
    assert dict(table.skipped) == dict(want_skipped)
    assert table.kept == getattr(want_skipped, "kept", dict(indel=0, two_alt=0))


@pytest.mark.parametrize("tag_indels", [False, True], ids=["snv_table", "allele_table"])
@pytest.mark.parametrize("kind", ["one_vcf", "directory", "one_vcf_one_contig"])
def test_table_is_what_the_readers_give(inputs, kind, tag_indels):
    one, per = inputs
    path = per if kind == "directory" else one
    whole = (phasedvcf.read_all_phase_alleles if tag_indels else phasedvcf.read_all_phase_sites)(one)
    sizes = {}
    for ctg in CONTIGS:
        src = phasedvcf.PhaseSource(path, tag_indels, only=ctg if kind == "one_vcf_one_contig" else None)
        table = src.table(ctg)
        sizes[ctg] = len(table)
        if kind == "one_vcf":
            want = whole.get(ctg)
        else:
            fn = phasedvcf.contig_file(path, ctg)
            want = (phasedvcf.read_phase_alleles if tag_indels else phasedvcf.read_phase_sites)(fn, ctg) if fn else None
        if want is None:                                     # no file / no row: the empty table of the source's kind
            assert ctg == "chr3"
            want = phasedvcf.empty_alleles() if tag_indels else (np.zeros(0, dtype=phasedvcf.PHASE_SITE_DTYPE), dict.fromkeys(phasedvcf.SKIP_REASONS, 0))
        _same(src, table, want[:-1], want[-1])
        # ... and what the per-contig readers the drivers used to call give
        if tag_indels:
            assert np.array_equal(table.sites, phasedvcf.contig_alleles(path, ctg)[0])
        else:
            assert np.array_equal(table.sites, phasedvcf.contig_sites(path, ctg))
    assert sizes == ({"chr1": 6, "chr2": 2, "chr3": 0, "chr4": 0} if tag_indels else {"chr1": 3, "chr2": 2, "chr3": 0, "chr4": 0})
    if tag_indels:
        assert phasedvcf.PhaseSource(path, True).table("chr1").kept == dict(indel=2, two_alt=1)


@pytest.mark.parametrize("tag_indels", [False, True], ids=["snv_table", "allele_table"])
def test_sixteen_threads_parse_one_vcf_once(inputs, tag_indels, monkeypatch):
    one, _per = inputs
    name = "read_all_phase_alleles" if tag_indels else "read_all_phase_sites"
    real, calls = getattr(phasedvcf, name), []

    def counted(fn):
        calls.append(fn)
        return real(fn)
    monkeypatch.setattr(phasedvcf, name, counted)
    src = phasedvcf.PhaseSource(one, tag_indels)
    start, got, errs = threading.Barrier(16), [None] * 16, []

    def ask(k):
        try:
            start.wait()
            got[k] = src.table(CONTIGS[k % len(CONTIGS)])
        except BaseException as e:
            errs.append(e)
    threads = [threading.Thread(target=ask, args=(k,)) for k in range(16)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs and calls == [one]
    for k in range(16):
        first = got[k % len(CONTIGS)]
        assert np.array_equal(got[k].sites, first.sites) and dict(got[k].skipped) == dict(first.skipped) and got[k].kept == first.kept
        assert all(np.array_equal(a, b) for a, b in zip(_handed(src, got[k]), _handed(src, first)))


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def set_phase_sites(self, *a):
        self.calls.append(("set_phase_sites", a))

    def set_phase_alleles(self, *a):
        self.calls.append(("set_phase_alleles", a))


def test_apply_calls_the_setter_of_the_sources_kind(inputs):
    one, per = inputs
    for path in (one, per):
        for ctg in ("chr1", "chr3"):
            eng, src = _Recorder(), phasedvcf.PhaseSource(path, False)
            src.apply(eng, src.table(ctg))
            (name, a), = eng.calls
            assert name == "set_phase_sites" and len(a) == 1 and np.array_equal(a[0], phasedvcf.contig_sites(path, ctg))
            assert a[0].dtype == phasedvcf.PHASE_SITE_DTYPE
            eng, src = _Recorder(), phasedvcf.PhaseSource(path, True)
            src.apply(eng, src.table(ctg))
            (name, a), = eng.calls
            want = phasedvcf.contig_alleles(path, ctg)
            assert name == "set_phase_alleles" and len(a) == 4 and a[3] == want[3]
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], want[:3])) and a[0].dtype == phasedvcf.HAP_SITE_DTYPE


def test_the_drivers_words_about_the_allele_table(inputs):
    one, _per = inputs
    src = phasedvcf.PhaseSource(one, True)
    assert src.indel_note(src.table("chr1"), "[INFO] chr1: ", ")") == "[INFO] chr1: 2 with an insertion or deletion, 1 with two ALTs)"
    plain = phasedvcf.PhaseSource(one, False)
    assert plain.indel_note(plain.table("chr1"), "x") == ""
    with pytest.raises(SystemExit) as e:
        phasedvcf.PhaseSource(one + ".absent")
    assert str(e.value.code) == "[ERROR] file %s.absent not found" % one
