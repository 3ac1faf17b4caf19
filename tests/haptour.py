"""One compact tour through every device entry point that holds the loaded reads against a site table — the base-quality mask, the
haplotaggers and their _w siblings, the count tables, the link tables of phasing, region, gene and junction counts — and through row export:
the inputs and, from the plain-Python restatements under tests/*ref.py, the expected arrays.  No GPU is touched here.

tests/support/hap_tour_worker.py walks the tour on the device (`STOPS` names what it writes, in its order), tests/test_gpu_hap_poison.py
compares, tests/test_haptour_ref.py checks that the inputs have teeth.

Two input sets: A (large) and B (small), each a dict of seven read sets made by the generators the feature suites own, B's with smaller
parameters.  Every read set carries base qualities; where a generator has no serial reads of its own, every third read gets an empty op
and so takes the device's serial walk.  B's read sets are cut at the end until the number of reads is no multiple of PREP_READS, the
packed sequence no multiple of 16 bytes and the last read of odd length: what lies behind B in a buffer that A filled is A's."""
import random

import numpy as np

from clair3_rna_amd.reads import ReadSet
from tests import hapalleleref as HA
from tests import hapcountref as HC
from tests import hapgroupref as HG
from tests import hapindelref as HI
from tests import hapjunctionref as HJ
from tests import hapref
from tests import hapregionref as HR
from tests import hapweightref as HW
from tests import leftalignref as LA
from tests import phasemergeref as PM
from tests import phaseref as P
from tests import qualref as QR
from tests import realignref as RR
from tests import realignspliceref as RS

PREP_READS = 16                                              # reads of one workgroup (csrc/reads_kernels.hpp)
PHASE_WIN = 256                                              # table sites of one window of the link kernels (csrc/phase_kernels.hpp)
HJ_MIN_SLOTS = 16                                            # the smallest junction table (2^HJ_MIN_LOG, csrc/hapjunction_kernels.hpp)
Q = 10                                                       # set_hap_min_bq of the mask stops
W = 10                                                       # set_hap_realign of the realigned forms
QUALS = (3, 5, 8, 12, 20, 30, 40)
FORMS = ("plain", "la", "ra", "rs")                          # the observation forms of the allele kernels, and the read set each runs on
SUFFIX = {"plain": "", "la": "_la", "ra": "_ra", "rs": "_rs"}
STRANDED = (0, 1, 2)
CTG = "chr20"

# what each set's generators are called with (A: the suites' own sizes or near them; B: smaller in every one)
SIZES = {
    "A": dict(snv=dict(n_reads=260, n_sites=120, n_ps=30), phase=dict(n_reads=203, n_sites=1400), frag=dict(n_reads=203),
              plain=dict(n_reads=203, n_snv=100, n_indel=30, n_two=8), la=dict(n_reads=203, n_snv=80, n_indel=24, n_two=5),
              ra=dict(n_reads=150, step=15), rs=dict(n_reads=150, step=15), regions=1, groups=9, rows=(1, 1500)),
    "B": dict(snv=dict(n_reads=90, n_sites=60, n_ps=12), phase=dict(n_reads=83, n_sites=70), frag=dict(n_reads=83, run=4),
              plain=dict(n_reads=83, n_snv=60, n_indel=16, n_two=4), la=dict(n_reads=83, n_snv=50, n_indel=12, n_two=3),
              ra=dict(n_reads=70, step=30), rs=dict(n_reads=70, step=30), regions=2, groups=5, rows=(1, 700)),
}
SEED = {"A": 5, "B": 6}                                      # the generators' seed per set ...
FUZZ_SEED = {"A": dict(ra=5, rs=4), "B": dict(ra=8, rs=4, plain=4)}      # ... but where another one is needed for tests/test_haptour_ref.py's conditions

LEAD = {"A": 5, "B": 0}                                      # bases put into the inserted-base pool before the table's own (hapalleleref.to_query): A's pools are the larger ones, at odd offsets

_cache = {}


def memo(obs):
    """An observation computed once per read (each table of a restatement asks for it)."""
    seen = {}

    def once(rs, i, site_at):
        if i not in seen:
            seen[i] = obs(rs, i, site_at)
        return seen[i]
    return once


# ---- read sets
def with_quals(rs, seed):
    """The reads with a quality on every base: one in sixteen 0, the others from QUALS, every tenth read without (0xff)."""
    rng = random.Random(seed)
    qual = np.full(2 * len(rs.seq), 0xff, np.uint8)
    for i, r in enumerate(rs.reads):
        o, n = 2 * int(r["seq_off"]), int(r["l_seq"])
        if i % 10 != 7:
            qual[o:o + n] = [0 if rng.random() < 1 / 16 else rng.choice(QUALS) for _ in range(n)]
    return ReadSet(rs.reads.copy(), rs.cigar.copy(), rs.seq.copy(), qual)


def head(rs, n):
    """The first n reads of a set whose arrays lie in read order."""
    last = rs.reads[n - 1]
    n_cig, n_seq = int(last["cigar_off"]) + int(last["n_cigar"]), int(last["seq_off"]) + (int(last["l_seq"]) + 1) // 2
    return ReadSet(rs.reads[:n].copy(), rs.cigar[:n_cig].copy(), rs.seq[:n_seq].copy(), None if rs.qual is None else rs.qual[:2 * n_seq].copy())


def ragged(rs):
    """The longest head of the set whose read count is no multiple of PREP_READS, whose packed sequence is no multiple of 16 bytes and whose
    last read has odd length."""
    for n in range(len(rs), 0, -1):
        h = head(rs, n)
        if n % PREP_READS and len(h.seq) % 16 and int(h.reads[-1]["l_seq"]) % 2:
            return h
    raise AssertionError("no head of the set is ragged")


def serial_third(rs):
    """Every third read through the serial walk (hapjunctionref.forced_serial: an empty op the rules do not see)."""
    return HJ.forced_serial(rs, 3)


def _finish(rs, which, seed, serial=True):
    rs = with_quals(serial_third(rs) if serial else rs, seed) if rs.qual is None else rs
    return ragged(rs) if which == "B" else rs


def _units(n, h1):
    """Units of three table sites, every seventh site in none, oriented by the sites' h1 (the chain's output, as the suites make it up)."""
    return [-1 if j % 7 == 5 else 1 + j // 3 for j in range(n)], [int(h) for h in h1]


def _spread_sets(table, per):
    """The table with its sites dealt to consecutive phase sets of `per` sites, every fifth site to the set two further on."""
    return [dict(s, ps=1 + j // per + (2 if j % 5 == 3 else 0)) for j, s in enumerate(table)]


def inputs(which):
    """The seven read sets of set `which` ('A' or 'B'), each a dict; made once."""
    if ("in", which) in _cache:
        return _cache[("in", which)]
    sz, seed = SIZES[which], SEED[which]
    out = {}
    # snv: hapref.gen_case (= hapjunctionref.distinct_case) — mask, SNV tags, hap_counts, regions, groups, junctions, rows
    ref, rs, table, _ = hapref.gen_case(seed, **sz["snv"])
    plain = with_quals(rs, seed + 100)
    rs = _finish(rs, which, seed + 100)
    query = table.copy()
    query["h1"] = 0
    query["ps"][::4] = 1000                                   # (a quarter of the query counts against set 1000, whatever the site's own)
    regs, row_ps = HR.gen_regions(seed, table)
    keep = [(int(r["start"]), int(r["end"]), int(r["strand"])) for r in regs][::sz["regions"]]
    regs, row_ps = HR.pack(keep, HR.row_table(keep, table))
    # the gene table: hapgroupref.fuzz_table's triples of exons and five single intervals (nine groups), cut to the first sz["groups"] groups
    _, gtab, _, _ = HG.fuzz_table(seed, "triples", table, len(ref))
    ivs = [(int(e["start"]), int(e["end"]), int(e["group"]), int(e["strand"])) for e in gtab if int(e["group"]) < sz["groups"]]
    gtab, goff, grow_ps = HG.pack(ivs, HG.group_rows(ivs, sz["groups"], table))
    out["snv"] = dict(ref=ref, rs=rs, rs_plain=ragged(plain) if which == "B" else plain, table=table, query=query, regions=regs, row_ps=row_ps,
                      intervals=gtab, n_groups=sz["groups"], group_row_off=goff, group_row_ps=grow_ps, rows=sz["rows"])
    # phase: phaseref.gen_case (= hapjunctionref.shared_case) — phase_links, junctions shared by many reads
    ref, rs, sites, truth, _ = P.gen_case(seed, **sz["phase"])
    jtable = sites.copy()
    jtable["h1"], jtable["ps"] = truth, 1000 + np.arange(len(jtable)) % 3
    out["phase"] = dict(ref=ref, rs=_finish(rs, which, seed + 200), sites=sites, table=jtable)
    # frag: phasemergeref.gen_fragmented — phase_unit_links on the chain's own table
    ref, rs, sites, _, _ = PM.gen_fragmented(seed, **sz["frag"])
    rs = _finish(rs, which, seed + 300)
    out["frag"] = dict(ref=ref, rs=rs, chain=P.resolve(sites, P.links(rs, sites))[0])
    # plain: hapalleleref.gen_case — the allele kernels without a switch
    ref, rs, rows, truth, planted, _ = HA.gen_case(FUZZ_SEED[which].get("plain", seed), errors=True, **sz["plain"])
    out["plain"] = dict(ref=(0, ref), rs=_finish(rs, which, FUZZ_SEED[which].get("plain", seed) + 400), table=_spread_sets(LA.table_of_case(rows, truth, planted)[0], 12))
    # la: leftalignref.gen_repeats, reads and rows placing their indels anywhere in a repeat; the table left-aligned as the host call does
    ref, rs, rows, truth, planted, _ = LA.gen_repeats(seed, True, errors=True, **sz["la"])
    t_on, _, skipped, moved = LA.align_sites(LA.table_of_case(rows, truth, planted)[0], (ref, 0))
    assert moved > 3 and not any(skipped.values()), (moved, skipped)
    out["la"] = dict(ref=(0, ref), rs=_finish(rs, which, seed + 500), table=_spread_sets(t_on, 12))
    # ra: hapweightref.gen_fuzz (realignref.gen_fuzz with three phase sets, wrongly phased sites and qualities 0 .. 40)
    fs = FUZZ_SEED[which]["ra"]
    if sz["ra"]["step"] == 15:
        ref, table, rs = HW.gen_fuzz(fs, n_reads=sz["ra"]["n_reads"])
    else:                                                     # (the generator has no spacing of its own to pass on: the same steps by hand)
        ref, table, rs = RR.gen_fuzz(fs, quals=True, **sz["ra"])
        table, rs = _deal(table, rs, fs)
    out["ra"] = dict(ref=ref, rs=_finish(rs, which, 0), table=table)
    # rs: the fuzz of tests/test_realign_spliced_ref.py — realignref.gen_fuzz with an intron planted at realignspliceref.CUTS
    fs = FUZZ_SEED[which]["rs"]
    ref, table, rs = RS.plant(*RR.gen_fuzz(fs, quals=True, **sz["rs"]), cuts=RS.CUTS, seed=fs)
    table, rs = _deal(table, rs, fs)
    out["rs"] = dict(ref=ref, rs=_finish(rs, which, 0), table=table)
    for f in FORMS:
        out[f]["lead"] = LEAD[which]
    _cache[("in", which)] = out
    return out


def _deal(table, rs, seed):
    """What hapweightref.gen_fuzz does to realignref.gen_fuzz's table and reads, drawn as it draws them: the sites dealt to three interleaved
    phase sets, a third of them phased the other way round than the reads were made, a quality of 0 .. 40 on every base (one in sixteen 0,
    a tenth of the reads without qualities).  -> (table, ReadSet)"""
    rng = random.Random(seed + 500)
    table = [dict(s) for s in table]
    for k, s in enumerate(table):
        s["ps"] = 21 + (k * 3 // len(table) if rng.random() < 0.6 else rng.randrange(3))
        if rng.random() < 0.35:
            s["h1"] = 1 - s["h1"]
    qual = rs.qual.copy()
    for i, r in enumerate(rs.reads):
        o, n = 2 * int(r["seq_off"]), int(r["l_seq"])
        qual[o:o + n] = 0xff if i % 10 == 7 else [0 if rng.random() < 1 / 16 else rng.choice((3, 5, 8, 12, 20, 30, 40)) for _ in range(n)]
    return table, HW.with_qual(rs, qual)


def observer(form, ref):
    """The observation of an allele form on a reference (first 0-based position, letters)."""
    return {"plain": lambda: HA.observe, "la": lambda: LA.observer((ref[1], ref[0])), "ra": lambda: RR.observer(ref, W), "rs": lambda: RS.observer(ref, W)}[form]()


def allele_args(d):
    """What the engine takes of an allele read set: (query, h1, pool, unit query, unit h1)."""
    q, pool = HA.to_query(d["table"], d["lead"])
    h1 = np.array([s["h1"] for s in d["table"]], np.uint8)
    ups, uh1 = _units(len(d["table"]), h1)
    qu = q.copy()
    qu["ps"] = ups
    return q, h1, pool, qu, np.array(uh1, np.uint8)


# ---- the stops: (name, the kernel labels the stop must reach)
def _stops():
    s = [("mask", ["k_mask_low_bq"]), ("tags", ["k_haplotag"]), ("tags_w", ["k_haplotag_w"]), ("tags_q", ["k_mask_low_bq", "k_haplotag"])]
    for f in FORMS:
        s += [("alleles_" + f, ["k_haplotag_alleles" + SUFFIX[f]]), ("alleles_%s_w" % f, ["k_haplotag_alleles%s_w" % SUFFIX[f]])]
    s.append(("counts", ["k_hap_counts"]))
    s += [("allele_counts_" + f, ["k_hap_allele_counts" + SUFFIX[f]]) for f in FORMS]
    s += [("links", ["k_phase_links"]), ("unit_links", ["k_phase_unit_links"])]
    for f in FORMS:
        s += [("allele_links_" + f, ["k_phase_allele_links" + SUFFIX[f]]), ("allele_unit_links_" + f, ["k_phase_allele_unit_links" + SUFFIX[f]])]
    s += [("regions", ["k_hap_region_counts"]), ("groups", ["k_hap_group_counts"])]
    for d in ("snv", "phase"):
        s += [("junctions_%s_lds" % d, ["k_hap_junction_counts"]), ("junctions_%s_direct" % d, ["k_hap_junction_counts_direct"])]
    s.append(("junctions_bare", ["k_hap_junction_counts"]))
    s.append(("rows", ["k_excl_scan", "k_pack_tokens"]))      # (the row-export launches that carry a label: the scan behind k_row_keep / k_site_ntok, both packers)
    return s


STOPS = _stops()
STAT_KEYS = hapref.STAT_KEYS


def stat_array(st):
    return np.array([st[k] for k in STAT_KEYS], np.int64)


def _tag_fields(t, weighted):
    out = dict(hp=t["hp"], st=stat_array(t["st"]), ps=t["ps"], words=t["words"])
    if weighted:
        out["w12"] = t["w12"]
    return out


def _junction_fields(found, hints=(0, 1)):
    assert HJ.invariant(found)
    j, r = HJ.arrays(found)
    return {"%s%d" % (k, h): a for h in hints for k, a in (("j", j), ("r", r))}


def expected(which):
    """{"<stop>/<field>": array} of set `which` for every stop but `rows` (whose text the parent derives from the engine's own
    probabilities), from the restatements; made once."""
    if ("exp", which) in _cache:
        return _cache[("exp", which)]
    d = inputs(which)
    out = {}

    def put(stop, fields):
        for k, v in fields.items():
            out["%s/%s" % (stop, k)] = v

    # a, b: the mask and the SNV tagger
    snv = d["snv"]
    rs, table = snv["rs"], snv["table"]
    seq, n = QR.mask(rs, Q)
    put("mask", dict(seq=seq, n=np.array([n], np.int64)))
    as_sites = HI.from_snv_table(table)
    unit = HW.haplotag(rs, as_sites, memo(HA.observe), weighted=False)
    hp, st, _ = hapref.haplotag(rs, table)
    assert np.array_equal(hp, unit["hp"]) and st == unit["st"] and np.array_equal(unit["ps"], HC.read_phase_sets(rs, table))
    put("tags", _tag_fields(unit, False))
    put("tags_w", _tag_fields(HW.haplotag(rs, as_sites, memo(HA.observe), weighted=True), True))
    put("tags_q", _tag_fields(HW.haplotag(HW.masked_as_n(rs, Q), as_sites, memo(HA.observe), weighted=False), False))
    # c, d, e: the allele forms
    for f in FORMS:
        a = d[f]
        obs = memo(observer(f, a["ref"]))
        t = HW.haplotag(a["rs"], a["table"], obs, weighted=False)
        put("alleles_" + f, _tag_fields(t, False))
        put("alleles_%s_w" % f, _tag_fields(HW.haplotag(a["rs"], a["table"], obs, weighted=True), True))
        put("allele_counts_" + f, dict(counts=LA.allele_counts(a["rs"], t["hp"], t["ps"], a["table"], obs)))
        put("allele_links_" + f, dict(links=LA.links(a["rs"], a["table"], obs)))
        ups, uh1 = _units(len(a["table"]), [s["h1"] for s in a["table"]])
        put("allele_unit_links_" + f, dict(ulinks=LA.unit_links(a["rs"], a["table"], ups, uh1, obs)))
    put("counts", dict(counts=HC.hap_counts(rs, table, snv["query"])))
    put("links", dict(links=P.links(d["phase"]["rs"], d["phase"]["sites"])))
    put("unit_links", dict(ulinks=PM.unit_links(d["frag"]["rs"], d["frag"]["chain"])))
    # f, g: regions and junctions
    for s in STRANDED:
        reg, row = HR.counts(rs, table, snv["regions"], snv["row_ps"], s)
        put("regions", {"region%d" % s: reg, "row%d" % s: row})
        grp, row = HG.counts(rs, table, snv["intervals"], snv["n_groups"], snv["group_row_off"], snv["group_row_ps"], s)
        put("groups", {"group%d" % s: grp, "row%d" % s: row})
    for name in ("snv", "phase"):
        fields = _junction_fields(HJ.counts(d[name]["rs"], d[name]["table"]))
        put("junctions_%s_lds" % name, fields)
        put("junctions_%s_direct" % name, fields)
    put("junctions_bare", _junction_fields(HJ.counts(rs, None), hints=(0,)))
    _cache[("exp", which)] = out
    return out


# ---- h: rows
def row_weights():
    """synth.random_weights with the output layers sharpened, as helpers.fuzz_decode_rows_and_regions does: not everything decodes to RefCall."""
    from clair3_rna_amd import synth
    w = synth.random_weights(18, seed=4242)
    w[-24 * 129:] *= 6.0
    return w


def rows_from(which, sites, raw, toks, probs):
    """decode.vcf_rows fed with a scan's own sites, raw tensors, tokens and probabilities (altinfo.format_lines makes the alt_info text):
    (rows with RefCalls shown, rows without)."""
    from clair3_rna_amd import altinfo, decode
    snv = inputs(which)["snv"]
    lines = altinfo.format_lines(CTG, sites, raw, toks, snv["rs_plain"], snv["ref"], 1)
    f = [l.split("\t") for l in lines]
    args = (CTG, [int(x[1]) for x in f], [x[2] for x in f], [x[4] for x in f], probs)
    return decode.vcf_rows(*args), decode.vcf_rows(*args, show_ref=False)


def text(rows):
    return np.frombuffer("".join(r + "\n" for r in rows).encode(), np.uint8)


def oracle_rows(which):
    """The CPU oracle's candidates of the rows stop and the reference network on them: (alt_info lines, rows with RefCalls shown).  The
    probabilities are the oracle's, not the device's: for the conditions of tests/test_haptour_ref.py only."""
    if ("rows", which) in _cache:
        return _cache[("rows", which)]
    from clair3_rna_amd import decode
    from oracle import oracle as orc
    from tests import helpers as H
    snv = inputs(which)["snv"]
    first, last = snv["rows"]
    exp = H.oracle_chunk(snv["rs_plain"], snv["ref"], 1, first, last, min_coverage=2, snp_af=0.0)
    lines, rows = exp["lines"], []
    if lines:
        f = [l.split("\t") for l in lines]
        rows = decode.vcf_rows(CTG, [int(x[1]) for x in f], [x[2] for x in f], [x[4] for x in f], orc.forward(row_weights(), exp["X"]))
    _cache[("rows", which)] = (lines, rows)
    return lines, rows
