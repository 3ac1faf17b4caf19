"""The child of tests/test_gpu_hap_poison.py: `python -m tests.support.hap_tour_worker OUT.npz` from the repository root walks the tour of
tests/haptour.py on device 0 three times — context 1: set A, then set B; context 2, a fresh one: set B alone — and writes every result
array into OUT.npz under "<context><set>/<stop>/<field>" ("1A/...", "1B/...", "2B/..."), with the kernel labels each stop reached under
"<context><set>/<stop>/kernels".  It asserts nothing about values: the parent compares.  Exit status 0 only if every library call returned
normally.  C3R_POISON, when the parent sets it, is read by the library itself."""
import sys

import numpy as np

from tests import haptour as T


def reset(e):
    """The switches back to their defaults, as each feature suite's _clean fixture leaves them."""
    from clair3_rna_amd import capi
    e.set_phase_sites(None)
    e.set_hap_bq_weights(False)
    e.set_hap_realign(0)
    e.set_hap_realign_spliced(False)
    e.set_hap_left_align(False)
    e.set_hap_min_bq(0)
    e.set_hap_junction_direct(False)
    e.set_hap_group_direct(False)
    e.set_bed(0, None)
    e.set_bed(1, None)
    e.params = capi.default_params()
    e.set_params()


def tag_fields(e, weighted):
    hp, st = e.haplotags()
    out = dict(hp=hp, st=T.stat_array(st), ps=e.read_phase_sets(), words=e.haplotag_words())
    if weighted:
        out["w12"] = e.haplotag_weights()
    return out


def switch_on(e, form, ref):
    """One switch at a time: the forms exclude each other."""
    if form != "plain":
        e.set_reference(ref[0] + 1, ref[1])
    if form == "la":
        e.set_hap_left_align(True)
    if form in ("ra", "rs"):
        e.set_hap_realign_spliced(form == "rs")
        e.set_hap_realign(T.W)


def tour(e, which, out, prefix):
    d = T.inputs(which)
    stops = iter(T.STOPS)

    def stop(fields):
        """Close the stop that just ran: its arrays and the labels it reached; then the defaults again."""
        name, _ = next(stops)
        for k, v in fields.items():
            out["%s/%s/%s" % (prefix, name, k)] = np.ascontiguousarray(v)
        out["%s/%s/kernels" % (prefix, name)] = np.array(sorted(e.kernel_stats()), dtype="U64")
        reset(e)
        e.reset_kernel_stats()
        return name

    reset(e)
    e.set_profiling(True)
    e.reset_kernel_stats()
    snv = d["snv"]
    rs, table = snv["rs"], snv["table"]
    # a. mask
    e.load_reads(rs)
    e.set_hap_min_bq(T.Q)
    assert stop(dict(seq=e.hap_seq(), n=np.array([e.hap_min_bq()[1]], np.int64))) == "mask"
    # b. SNV tags: unit weights, quality weights, and under the threshold
    e.load_reads(rs)
    e.set_phase_sites(table)
    stop(tag_fields(e, False))
    e.load_reads(rs)
    e.set_hap_bq_weights(True)
    e.set_phase_sites(table)
    stop(tag_fields(e, True))
    e.load_reads(rs)
    e.set_hap_min_bq(T.Q)
    e.set_phase_sites(table)
    assert stop(tag_fields(e, False)) == "tags_q"
    # c. allele tags in the four forms, without and with weights
    for f in T.FORMS:
        a = d[f]
        q, h1, pool, _, _ = T.allele_args(a)
        for weighted in (False, True):
            switch_on(e, f, a["ref"])
            e.load_reads(a["rs"])
            e.set_hap_bq_weights(weighted)
            e.set_phase_alleles(q, h1, pool)
            name = stop(tag_fields(e, weighted))
        assert name == "alleles_%s_w" % f
    # d. counts
    e.load_reads(rs)
    e.set_phase_sites(table)
    assert stop(dict(counts=e.hap_counts(snv["query"]))) == "counts"
    for f in T.FORMS:
        a = d[f]
        q, h1, pool, _, _ = T.allele_args(a)
        switch_on(e, f, a["ref"])
        e.load_reads(a["rs"])
        e.set_phase_alleles(q, h1, pool)
        assert stop(dict(counts=e.hap_allele_counts(q, pool))) == "allele_counts_" + f
    # e. links
    e.load_reads(d["phase"]["rs"])
    assert stop(dict(links=e.phase_links(d["phase"]["sites"]))) == "links"
    e.load_reads(d["frag"]["rs"])
    assert stop(dict(ulinks=e.phase_unit_links(d["frag"]["chain"]))) == "unit_links"
    for f in T.FORMS:
        a = d[f]
        q, _, pool, qu, uh1 = T.allele_args(a)
        switch_on(e, f, a["ref"])
        e.load_reads(a["rs"])
        stop(dict(links=e.phase_allele_links(q, pool)))
        switch_on(e, f, a["ref"])
        e.load_reads(a["rs"])
        assert stop(dict(ulinks=e.phase_allele_unit_links(qu, uh1, pool))) == "allele_unit_links_" + f
    # f. regions, groups and junctions
    e.load_reads(rs)
    e.set_phase_sites(table)
    fields = {}
    for s in T.STRANDED:
        fields["region%d" % s], fields["row%d" % s] = e.hap_region_counts(snv["regions"], snv["row_ps"], s)
    assert stop(fields) == "regions"
    e.load_reads(rs)
    e.set_phase_sites(table)
    fields = {}
    for s in T.STRANDED:
        fields["group%d" % s], fields["row%d" % s] = e.hap_group_counts(snv["intervals"], snv["n_groups"], snv["group_row_off"], snv["group_row_ps"], s)
    assert stop(fields) == "groups"
    for name in ("snv", "phase"):
        for direct in (False, True):
            e.load_reads(d[name]["rs"])
            e.set_phase_sites(d[name]["table"])
            e.set_hap_junction_direct(direct)
            fields = {}
            for hint in (1, 0):                               # (the smallest tables first: they grow)
                fields["j%d" % hint], fields["r%d" % hint] = e.hap_junction_counts(hint)
            assert stop(fields) == "junctions_%s_%s" % (name, "direct" if direct else "lds")
    # g. without a table: the tag words of the last tagged load are still in their buffer
    e.load_reads(rs)
    e.set_phase_sites(table)
    e.set_phase_sites(None)
    fields = {}
    fields["j0"], fields["r0"] = e.hap_junction_counts()
    assert stop(fields) == "junctions_bare"
    # h. row export
    first, last = snv["rows"]
    e.set_params(snp_min_af=0.0, min_coverage=2)
    e.load_reads(snv["rs_plain"])
    e.set_reference(1, snv["ref"])
    e.scan(first, last)
    e.load_weights(T.row_weights(), 18)
    e.set_precision("f16x3")
    probs = e.infer()
    fields = dict(sites=e.sites(), tokens=e.tokens(), raw=e.tensors(rescaled=False), tensors=e.tensors(rescaled=True), probs=probs)
    for key, drop, show in (("snap_all", False, True), ("snap_all_noref", False, False), ("snap_drop", True, False)):
        snap = e.rows_begin(drop_ref_calls=drop)
        fields[key + "_info"] = np.array(snap.info(), np.int64)
        fields[key] = np.frombuffer(snap.decode(T.CTG, show_ref=show)[0], np.uint8)
    fields["snap_device_reads"] = np.frombuffer(e.rows_begin(drop_ref_calls=True, host_reads=False).decode(T.CTG, show_ref=False)[0], np.uint8)
    fields["call_rows"] = T.text(e.call_rows(T.CTG))
    fields["call_rows_noref"] = T.text(e.call_rows(T.CTG, show_ref=False))
    assert stop(fields) == "rows" and next(stops, None) is None
    e.set_profiling(False)


def main(path):
    from clair3_rna_amd import capi
    out = {}
    e = capi.Engine(0)
    tour(e, "A", out, "1A")
    tour(e, "B", out, "1B")
    e.close()
    e = capi.Engine(0)
    tour(e, "B", out, "2B")
    e.close()
    np.savez(path, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
