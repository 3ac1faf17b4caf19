"""The inputs of tests/haptour.py have teeth (no GPU): conditions on the two input sets and on what the restatements alone give on them, so
that tests/test_gpu_hap_poison.py compares something at every stop.  The floors are conditions, not measurements; beside each stands what
the restatements give (printed again by every run)."""
import numpy as np
import pytest

from tests import hapalleleref as HA
from tests import hapjunctionref as HJ
from tests import hapref
from tests import haptour as T
from tests import hapweightref as HW
from tests import leftalignref as LA

SETS = ("A", "B")
READ_SETS = ("snv", "phase", "frag", "plain", "la", "ra", "rs")


def _table(d):
    for k in ("table", "chain", "sites"):
        if k in d:
            return d[k]


def _pool_bytes(d):
    return len(T.allele_args(d)[2])


def _junctions(which, name):
    d = T.inputs(which)[name]
    return HJ.counts(d["rs"], d["table"])


# ---- size conditions
def test_b_is_strictly_smaller_than_a_in_everything_a_buffer_is_sized_by():
    a, b = T.inputs("A"), T.inputs("B")
    for name in READ_SETS:
        sizes = [(len(d[name]["rs"]), len(d[name]["rs"].cigar), len(d[name]["rs"].seq), len(_table(d[name]))) for d in (a, b)]
        print("%s: reads, CIGAR ops, packed sequence bytes, table sites: A %s, B %s" % (name, sizes[0], sizes[1]))
        assert all(y < x for x, y in zip(*sizes)), (name, sizes)
    #   snv (260, 7957, 71809, 120) / (88, 2894, 26547, 60)      phase (203, 1006, 41517, 1400) / (82, 446, 23275, 70)
    #   frag (203, 3419, 40044, 138) / (83, 1720, 20892, 128)    plain (203, 4222, 33364, 138) / (83, 1760, 16594, 80)
    #   la (203, 5528, 61254, 109) / (83, 1934, 23211, 65)       ra (150, 3220, 9214, 24) / (69, 1426, 4106, 12)
    #   rs (150, 3755, 9327, 24) / (70, 1690, 4290, 12)
    assert len(b["snv"]["rs_plain"]) < len(a["snv"]["rs_plain"]) and len(b["snv"]["rs_plain"].seq) < len(a["snv"]["rs_plain"].seq)
    for f in T.FORMS:
        pools = _pool_bytes(a[f]), _pool_bytes(b[f])
        units = [len({u for u in T.allele_args(d[f])[3]["ps"].tolist() if u >= 0}) for d in (a, b)]
        print("%s: inserted-base pool bytes A %d, B %d; units A %d, B %d" % (f, pools[0], pools[1], units[0], units[1]))
        assert pools[1] < pools[0] and pools[1] > 0 and units[1] < units[0]       # plain 37 / 6, la 31 / 12, ra 6 / 4, rs 10 / 4; units 46 / 27, 37 / 22, 8 / 4, 8 / 4
    other = dict(query=[len(d["snv"]["query"]) for d in (a, b)], regions=[len(d["snv"]["regions"]) for d in (a, b)],
                 region_rows=[len(d["snv"]["row_ps"]) for d in (a, b)], group_intervals=[len(d["snv"]["intervals"]) for d in (a, b)],
                 groups=[d["snv"]["n_groups"] for d in (a, b)], group_rows=[len(d["snv"]["group_row_ps"]) for d in (a, b)], chain_units=[len(T.expected(w)["unit_links/ulinks"]) for w in SETS],
                 junctions_snv=[len(_junctions(w, "snv")) for w in SETS], junctions_phase=[len(_junctions(w, "phase")) for w in SETS],
                 junction_rows_snv=[sum(len(e["rows"]) for e in _junctions(w, "snv").values()) for w in SETS],
                 candidate_rows=[len(T.oracle_rows(w)[0]) for w in SETS], scan_end=[T.inputs(w)["snv"]["rows"][1] for w in SETS])
    print(other)
    # query 120 / 60, regions 50 / 25, region rows 182 / 70, chain units 6 / 2, junctions 1342 / 499 and 21 / 17, rows 1329 / 487, candidates 1429 / 277
    assert all(y < x for x, y in other.values()), other


@pytest.mark.parametrize("name", READ_SETS + ("snv/rs_plain",))
def test_b_ends_ragged(name):
    d = T.inputs("B")[name.split("/")[0]]
    rs = d[name.split("/")[1]] if "/" in name else d["rs"]
    print("%s: %d reads, %d packed bytes, last read of %d bases" % (name, len(rs), len(rs.seq), int(rs.reads[-1]["l_seq"])))
    assert len(rs) % T.PREP_READS and len(rs.seq) % 16 and int(rs.reads[-1]["l_seq"]) % 2
    assert rs.qual is not None and len(rs.qual) == 2 * len(rs.seq) and rs.qual[-1] == 0xff


@pytest.mark.parametrize("which", SETS)
def test_every_read_set_carries_qualities_and_serial_reads(which):
    for name, d in T.inputs(which).items():
        rs = d["rs"]
        ops = [[int(c) & 15 for c in rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]] + [int(c) >> 4 == 0 for c in
               rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]] for r in rs.reads]
        serial = sum(1 for o in ops if 6 in o[:len(o) // 2] or 7 in o[:len(o) // 2] or 8 in o[:len(o) // 2] or True in o[len(o) // 2:])
        with_q = int(sum((rs.qual[2 * int(r["seq_off"]):2 * int(r["seq_off"]) + int(r["l_seq"])] != 0xff).any() for r in rs.reads))
        print("%s %s: %d of %d reads hold a pad, an = / X op or an empty op, %d carry qualities" % (which, name, serial, len(rs), with_q))
        assert rs.qual is not None and serial >= len(rs) // 4 and len(rs) > with_q >= len(rs) // 2


# ---- non-trivial expected results
@pytest.mark.parametrize("which", SETS)
def test_tags_of_both_haplotypes_untagged_reads_and_weights_that_decide(which):
    e = T.expected(which)
    for stop in ["tags", "tags_q"] + ["alleles_" + f for f in T.FORMS]:
        n = np.bincount(e[stop + "/hp"], minlength=3).tolist()
        print(which, stop, "untagged / hp1 / hp2:", n, "phase sets:", len(set(e[stop + "/ps"].tolist()) - {-1}))
        assert min(n) >= 3 and len(set(e[stop + "/ps"].tolist()) - {-1}) >= 2, (stop, n)      # the smallest: B alleles_plain untagged 8; B alleles_rs 2 sets
    for stop in ["tags"] + ["alleles_" + f for f in T.FORMS]:
        moved = int(((e[stop + "/hp"] != e[stop + "_w/hp"]) | (e[stop + "/ps"] != e[stop + "_w/ps"])).sum())
        print(which, stop, "reads whose tag or set differs under weights:", moved, "weight sum", int(e[stop + "_w/w12"].sum()))
        assert moved >= 2 and int(e[stop + "_w/w12"].sum()) > 1000       # A 111, 58, 38, 71, 65; B 28, 12, 15, 32, 36
    masked = int((e["tags/hp"] != e["tags_q/hp"]).sum())
    print(which, "bases masked by Q = %d:" % T.Q, int(e["mask/n"][0]), "reads whose tag differs under the mask:", masked)
    assert int(e["mask/n"][0]) >= 1000 and masked >= 3 and not np.array_equal(e["mask/seq"], T.inputs(which)["snv"]["rs"].seq)      # A 60695, 20; B 22685, 3


@pytest.mark.parametrize("which", SETS)
def test_a_read_decided_in_a_second_phase_set(which):
    """Reads that vote in two or more sets and whose tag was decided in another set than the one of their first voting site."""
    snv, e = T.inputs(which)["snv"], T.expected(which)
    by_pos = {int(s["pos"]): s for s in snv["table"]}
    n = 0
    for i in range(len(snv["rs"])):
        hp, _, _, tally = hapref.tag_read(snv["rs"], i, by_pos)
        if hp and len(tally) >= 2 and int(e["tags/ps"][i]) != min(tally.items(), key=lambda kv: kv[1][2])[0]:
            n += 1
    print(which, "reads decided in a set other than their first:", n)
    assert n >= 10                                            # A 146, B 39


@pytest.mark.parametrize("which", SETS)
def test_every_count_column_and_row_cis_and_trans(which):
    e = T.expected(which)
    for key in ["counts/counts"] + ["allele_counts_%s/counts" % f for f in T.FORMS]:
        cols, rows = e[key].sum(axis=(0, 1)).tolist(), e[key].sum(axis=(0, 2)).tolist()
        print(which, key, "columns", cols, "rows", rows)
        assert min(cols) >= 1 and min(rows) >= 40, (key, cols, rows)       # the smallest column: A allele_counts_rs 2, B allele_counts_ra / _rs 1
    for key in ["links/links", "unit_links/ulinks"] + ["allele_links_%s/links" % f for f in T.FORMS] + ["allele_unit_links_%s/ulinks" % f for f in T.FORMS]:
        cis, trans = int(e[key][..., 0].sum()), int(e[key][..., 1].sum())
        print(which, key, e[key].shape, "cis", cis, "trans", trans)
        assert cis >= 3 and trans >= 3 and len(e[key]) >= 2, (key, cis, trans)      # the smallest: B unit_links 4 / 3 on 2 units
    for s in T.STRANDED:
        reg, row = e["regions/region%d" % s], e["regions/row%d" % s]
        print(which, "stranded", s, "region columns", reg.sum(axis=0).tolist(), "row columns", row.sum(axis=0).tolist())
        assert reg.sum(axis=0).min() >= 5 and row.sum(axis=0).min() >= 50      # the least: A regions [24, 1342], B rows [141, 115]
    assert not np.array_equal(e["regions/region0"], e["regions/region1"]) and not np.array_equal(e["regions/row1"], e["regions/row2"])
    for s in T.STRANDED:
        grp, row = e["groups/group%d" % s], e["groups/row%d" % s]
        print(which, "stranded", s, "group columns", grp.sum(axis=0).tolist(), "row columns", row.sum(axis=0).tolist())
        assert grp.sum(axis=0).min() >= 1 and row.sum(axis=0).min() >= 1       # all four kinds of count word occur; the least: B stranded 1 groups [8, 49]
    assert not np.array_equal(e["groups/group0"], e["groups/group1"]) and not np.array_equal(e["groups/row1"], e["groups/row2"])


def test_the_group_tables_of_a_and_b_differ():
    """What the groups stop of B finds behind its own table in the shared buffers is A's, and A's is something else."""
    a, b = T.expected("A"), T.expected("B")
    for s in T.STRANDED:
        for k in ("groups/group%d" % s, "groups/row%d" % s):
            n = min(len(a[k]), len(b[k]))
            print(k, "A", a[k].shape, int(a[k].sum()), "B", b[k].shape, int(b[k].sum()))
            assert len(b[k]) < len(a[k]) and a[k].sum() > 0 and b[k].sum() > 0 and not np.array_equal(a[k][:n], b[k][:n])


def test_a_read_of_a_takes_a_second_window_of_the_link_kernels():
    ph = T.inputs("A")["phase"]
    pos = ph["sites"]["pos"].astype(np.int64)
    most = 0
    for i in range(len(ph["rs"])):
        a = int(ph["rs"].reads[i]["pos"])
        most = max(most, int(((pos > a) & (pos <= a + HJ.ref_span(ph["rs"], i))).sum()))
    print("most table sites in one read's range: %d of %d (PHASE_WIN = %d)" % (most, len(pos), T.PHASE_WIN))
    assert most > 2 * T.PHASE_WIN                             # 939: a fourth window


@pytest.mark.parametrize("which", SETS)
def test_junctions_with_rows_with_untagged_reads_and_more_than_the_smallest_table_holds(which):
    for name in ("snv", "phase"):
        found = _junctions(which, name)
        two, untagged = sum(len(x["rows"]) >= 2 for x in found.values()), sum(x["untagged"] > 0 for x in found.values())
        print(which, name, "%d junctions, %d with two or more rows, %d with untagged reads" % (len(found), two, untagged))
        assert len(found) > T.HJ_MIN_SLOTS                    # slots_hint = 1 must grow: A 1342 and 21, B 499 and 17
        assert (two >= 10) if name == "phase" else (untagged >= 10)      # phase: A 15, B 12 with two rows; snv: A 13, B 12 with untagged reads
    bare = T.expected(which)["junctions_bare/j0"]
    assert len(T.expected(which)["junctions_bare/r0"]) == 0 and (bare["untagged"] == bare["reads"]).all() and len(bare) == len(_junctions(which, "snv"))


@pytest.mark.parametrize("which", SETS)
def test_rows_of_several_kinds_and_refcalls_to_drop(which):
    lines, rows = T.oracle_rows(which)
    kinds = {}
    for r in rows:
        f = r.split("\t")
        kinds[(f[6], f[9].split(":")[0])] = kinds.get((f[6], f[9].split(":")[0]), 0) + 1
    print(which, len(lines), "candidates;", kinds)
    # A 1429: RefCall 819, LowQual 1/1 233, 0/1 196, 1/2 75, PASS 0/1 55, 1/1 27, 1/2 24;  B 277: RefCall 248, PASS 0/1 11, LowQual 1/1 10, 0/1 5, 1/2 2, PASS 1/1 1
    assert len(kinds) >= 4 and kinds.get(("RefCall", "0/0"), 0) >= 100 and len(rows) - kinds[("RefCall", "0/0")] >= 25


# ---- form conditions: a stop that silently ran a sibling kernel would not pass
@pytest.mark.parametrize("which", SETS)
def test_each_form_differs_from_the_plain_form_on_its_own_reads(which):
    d, e = T.inputs(which), T.expected(which)
    for f in ("la", "ra", "rs"):
        a = d[f]
        for other in ["plain"] + (["ra"] if f == "rs" else []):
            obs = T.memo(T.observer(other, a["ref"]))
            t = HW.haplotag(a["rs"], a["table"], obs, weighted=False)
            tags = int(((t["hp"] != e["alleles_%s/hp" % f]) | (t["words"] != e["alleles_%s/words" % f])).sum())
            counts = int((LA.allele_counts(a["rs"], t["hp"], t["ps"], a["table"], obs) != e["allele_counts_%s/counts" % f]).sum())
            links = int((LA.links(a["rs"], a["table"], obs) != e["allele_links_%s/links" % f]).sum())
            print(which, "%s against %s on the same reads: %d tags or tag words, %d counts, %d links differ" % (f, other, tags, counts, links))
            assert tags >= 1 and counts >= 1 and links >= 1, (f, other, tags, counts, links)     # the fewest: B rs against ra 5, 11, 9
