"""Shared helpers for the parity tests: run the CPU oracle and the HIP engine on the same inputs."""
import numpy as np

from oracle import oracle as orc

CTG = "chr20"


def oracle_chunk(rs, ref, ref_start, ctg_start, ctg_end, channels=18, lbed=None, **pk):
    """Oracle A1..A5 for one chunk.  Returns dict(rows, lines, X, depth)."""
    es, ee = max(1, ctg_start - 33), ctg_end + 33
    rows = orc.mpileup(rs.reads, rs.cigar, rs.seq, CTG, es, ee, min_mq=pk.pop("min_mq", 5), excl_flags=pk.pop("excl_flags", 2316),
                       bed=lbed, with_hp=(channels == 30), max_depth=pk.pop("max_depth", 8000), compat=pk.pop("mpileup_compat", 0))
    P = orc.make_params(phased=(channels == 30), **pk)
    # the reference upper-cases the whole slice when it loads it ("uppercase for masked sequences", shared/utils.py:186-187)
    lines = orc.create_tensor(rows, CTG, ref.upper(), ref_start, P)
    X, depth = orc.batch_from_lines(lines, channels)
    return dict(rows=rows, lines=lines, X=X, depth=depth)


def engine_chunk(eng, rs, ref, ref_start, ctg_start, ctg_end):
    """HIP A1..A5 for one chunk through the C-ABI.  Returns dict(lines, X, raw, sites, tokens)."""
    from clair3_rna_amd import altinfo
    eng.load_reads(rs)
    eng.set_reference(ref_start, ref)
    n = eng.scan(ctg_start, ctg_end)
    raw = eng.tensors(rescaled=False)
    X = eng.tensors(rescaled=True)
    sites, toks = eng.sites(), eng.tokens()
    lines = altinfo.format_lines(CTG, sites, raw, toks, rs, ref.upper(), ref_start, padins=eng.pad_insertions())
    return dict(n=n, lines=lines, X=X, raw=raw, sites=sites, tokens=toks)


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            fx, fy = x.split("\t"), y.split("\t")
            for k in range(min(len(fx), len(fy))):
                if fx[k] != fy[k]:
                    if k == 3:
                        vx, vy = np.array(fx[3].split(), int), np.array(fy[3].split(), int)
                        d = np.nonzero(vx != vy)[0]
                        return "line %d pos %s field 3 idx %s got %s exp %s" % (i, fx[1], d[:8], vx[d[:8]], vy[d[:8]])
                    return "line %d pos %s/%s field %d: %r vs %r" % (i, fx[1], fy[1], k, fx[k][:120], fy[k][:120])
    return "length %d vs %d" % (len(a), len(b))


def merge_readsets(a, b):
    """ReadSet holding the reads of both, in position order (stable: a's reads before b's at equal positions)."""
    from clair3_rna_amd.reads import ReadSet
    rb = b.reads.copy()
    rb["cigar_off"] += len(a.cigar)
    rb["seq_off"] += len(a.seq)
    reads = np.concatenate([a.reads, rb])
    order = np.argsort(reads["pos"], kind="stable")
    return ReadSet(reads[order], np.concatenate([a.cigar, b.cigar]), np.concatenate([a.seq, b.seq]))


def indel_next_to_indel_reads(ref, pos0, n=6, seed=7):
    """Hand-made reads at 0-based pos0 whose columns differ between the two samtools printers: `40M2I1D40M` (an insertion with a
    deletion right behind it) and `40M1I1P1I40M` (a pad inside the run of I ops), both strands."""
    import random
    from clair3_rna_amd.reads import ReadSet
    rng = random.Random(seed)
    recs = []
    for k in range(n):
        flag = 16 if k % 2 else 0
        left, right = ref[pos0:pos0 + 40].upper(), ref[pos0 + 41:pos0 + 81].upper()
        recs.append(dict(pos=pos0, cigar="40M2I1D40M", seq=left + "TG" + right, flag=flag))
        recs.append(dict(pos=pos0, cigar="40M1I1P1I40M", seq=left + "CA" + ref[pos0 + 40:pos0 + 80].upper(), flag=flag))
    return ReadSet.from_records(recs)


def fake_samtools(path, version):
    """An executable that answers `--version` like samtools <version> (the drivers' --mpileup_compat auto asks it)."""
    import os
    with open(path, "w") as f:
        f.write("#!/bin/sh\necho 'samtools %s'\necho 'Using htslib %s'\n" % (version, version))
    os.chmod(path, 0o755)
    return path


# ---- random-CIGAR read sets and the parity checks run on them (tests/test_gpu_fuzz.py with one engine and the natural thresholds,
# tests/test_gpu_deep_routes.py with every span forced through the deep-span kernels) --------------------------------------------
def _seeds(n):
    """CI runs seeds 0..n-1; a soak run sets C3R_FUZZ_BASE / C3R_FUZZ_SCALE to walk further seeds (tests/evidence/README.md)."""
    import os
    base, scale = int(os.environ.get("C3R_FUZZ_BASE", "0")), int(os.environ.get("C3R_FUZZ_SCALE", "1"))
    return range(base, base + n * scale)


def _rand_cigar(rng, want_q, pads=True):
    """Random op sequence: M/=/X/I/D/N/S/H/P incl. zero-length ops, leading/trailing I or D, runs of D D, I I, N next to
    I or D, pads between insertions (pads = False: a short M in their place).  Returns (cigar string, query length)."""
    ops = []
    if rng.random() < 0.15:
        ops.append((rng.randint(1, 5), "H"))
    if rng.random() < 0.25:
        ops.append((rng.randint(1, 6), "S"))
    n_core = rng.randint(1, 9)
    for k in range(n_core):
        r = rng.random()
        if r < 0.45:
            ops.append((rng.randint(1, 25), rng.choice("MMMM=X")))
        elif r < 0.58:
            ops.append((rng.randint(1, 4) if rng.random() < 0.9 else rng.randint(17, 22), "I"))
        elif r < 0.72:
            ops.append((rng.randint(1, 5), "D"))
        elif r < 0.84:
            ops.append((rng.randint(1, 40), "N"))
        elif r < 0.90:
            ops.append((rng.randint(1, 3), "P" if pads else "M"))
        elif r < 0.95:
            ops.append((0, rng.choice("MID")))              # zero-length op
        else:
            ops.append((rng.randint(1, 3), "D")); ops.append((rng.randint(1, 3), "D"))   # split deletion
    if rng.random() < 0.25:
        ops.append((rng.randint(1, 6), "S"))
    if rng.random() < 0.1:
        ops.append((rng.randint(1, 5), "H"))
    if not any(o in "M=X" and l > 0 for l, o in ops):
        ops.insert(len(ops) // 2, (rng.randint(2, 12), "M"))
    qlen = sum(l for l, o in ops if o in "MIS=X")
    return "".join("%d%s" % lo for lo in ops), qlen


def _case(seed, phased, pads=True, info=None):
    """info: a dict that receives `hot`, the 0-based centre of the pile (place() puts it on a chosen coordinate)."""
    import random
    import re
    rng = random.Random(seed)
    L = rng.choice([300, 420, 777])
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    if rng.random() < 0.3:          # some IUPAC / N / lower-case reference letters
        ref = list(ref)
        for _ in range(6):
            ref[rng.randrange(L)] = rng.choice("NRYacgtn")
        ref = "".join(ref)
    recs = []
    n_reads = rng.randint(25, 90)
    hot = rng.randint(30, L - 120)
    if info is not None:
        info["hot"] = hot
    for _ in range(n_reads):
        pos = max(1, int(rng.gauss(hot, 40)))
        cg, qlen = _rand_cigar(rng, 0, pads)
        if rng.random() < 0.1:
            qlen = max(1, qlen - rng.randint(1, 3))          # query shorter than the CIGAR claims
        seq = "".join(rng.choice("ACGTACGTACGTACGTN=RY") for _ in range(qlen))
        flag = (16 if rng.random() < 0.5 else 0) | rng.choice([0] * 14 + [256, 2048, 4, 1024, 512, 8, 1, 3, 65, 131])
        mapq = rng.choice([60] * 8 + [0, 3, 5, 4, 20, 255])
        hp = rng.choice([0, 1, 2, 1, 2]) if phased else 0
        recs.append(dict(pos=pos, cigar=cg, seq=seq, flag=flag, mapq=mapq, hp=hp))
    recs.sort(key=lambda r: r["pos"])
    # alignments must lie inside the contig (the reference indexes the reference string with every covered position)
    end = max(r["pos"] + sum(int(n) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", r["cigar"]) if o in "MDN=X") for r in recs)
    if end + 40 > len(ref):
        ref = ref + "".join(rng.choice("ACGT") for _ in range(end + 40 - len(ref)))
    return ref, recs


# ---- coordinates: the same cases translated to chromosome scale and to the end of the accepted domain (tests/test_coords_ref.py: the references do
# not depend on the translation; tests/test_gpu_coords.py: neither does the engine).  A translation is an int, or f(L, hot) -> int for one that
# depends on the case (L: the length of its reference, hot: the 0-based centre of its pile).
INT32_MAX = 2 ** 31 - 1
CTG_END_MAX = 2147482590            # C3R_CTG_END_MAX (include/c3r.h): the last ctg_end a scan accepts; a read may END on INT32_MAX (0-based, exclusive)
CHR1_LEN = 248956422                # GRCh38 chr1
K_LOW = 1000                        # magnitude as in every other test: only the phases against bins and tiles move


def K_CHR1(L, hot):
    """the case's last reference base sits on the last base of chr1"""
    return CHR1_LEN - L


def K_2_28(L, hot):
    """the centre of the pile sits on 0-based 2^28 (the length limit of one CIGAR op: no human contig reaches it, the accepted domain does)"""
    return (1 << 28) - hot


def K_TOP(L, hot):
    """the scan of the whole case ends on the last accepted ctg_end"""
    return CTG_END_MAX - L


def k_plus(K, phi):
    """K + phi: the reads' phase against the bins (pos >> 5)"""
    if not callable(K):
        return K + phi
    return lambda L, hot: K(L, hot) + phi


PHIS = (0, 1, 31)                   # reads against bins
FRONTS = (0, 1, 223, 255)           # tile starts (ctg_start - 34) against reads, bins (32) and coarse bins (256); spans are 224 positions


def shift_records(recs, K):
    return recs if K == 0 else [dict(r, pos=r["pos"] + K) for r in recs]


def place(ref, recs, shift, front, hot, seed):
    """A case at its coordinates: (K, records with pos + K, reference slice with `front` random bases before the case's first base, 1-based
    position `first` of the slice's first base = 1 + K - front).  A scan of the whole case runs from `first` to first + len(slice) - 1: nothing
    covers the front positions, they only move the first tile's p0 = first - 34 (front > 0 requires K >= front + 34: no clamp at 1).  Engine and
    oracle get the same slice; the front bases show only where head/tail calling prints the reference under a window that begins before the case."""
    import random
    K = shift(len(ref), hot) if callable(shift) else int(shift)
    if front:
        assert K >= front + 34, (K, front)
        rng = random.Random(911 * seed + front)
        ref = "".join(rng.choice("ACGT") for _ in range(front)) + ref
    return K, shift_records(recs, K), ref, 1 + K - front


def placed_case(seed, phased, shift=0, front=0, pads=True):
    """(ReadSet, reference slice, first, last, records) of _case(seed) at its coordinates (place)."""
    from clair3_rna_amd.reads import ReadSet
    info = {}
    ref, recs = _case(seed, phased=phased, pads=pads, info=info)
    K, recs, ref, first = place(ref, recs, shift, front, info["hot"], seed)
    return ReadSet.from_records(recs), ref, first, first + len(ref) - 1, recs


def shift_readset(rs, K):
    """The same reads K positions further (CIGARs and bases shared)."""
    from clair3_rna_amd.reads import ReadSet
    reads = rs.reads.copy()
    assert int(reads["pos"].max(initial=0)) + K <= INT32_MAX
    reads["pos"] += K
    return ReadSet(reads, rs.cigar, rs.seq)


def readset_end(rs):
    """The largest 0-based exclusive end of the reads' alignments."""
    best = 0
    for r in rs.reads:
        c = rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]
        best = max(best, int(r["pos"]) + int(sum(int(x) >> 4 for x in c if "MIDNSHP=X"[int(x) & 15] in "MDN=X")))
    return best


def shift_sites(sites, K, ps=False):
    """A site table (PHASE_SITE_DTYPE / HAP_SITE_DTYPE) K positions further; ps (phase-set names) stay unless ps=True."""
    out = sites.copy()
    out["pos"] += K
    if ps:
        out["ps"] = np.where(out["ps"] >= 0, out["ps"] + K, out["ps"])
    return out


def shift_lines(lines, K, field=1):
    """Tab-separated lines with the position field moved by K (the oracle's lines and mpileup rows, VCF rows)."""
    out = []
    for l in lines:
        f = l.split("\t")
        f[field] = str(int(f[field]) + K)
        out.append("\t".join(f))
    return out


def _scanned(on_scan, eng, exp):
    """on_scan(eng, exp): a caller's look at the engine after a scan (Engine.scan_counts(): which kernels built the spans; it stands until the
    next scan, the raw re-run behind tensors(rescaled=False) and columns() leave it alone); exp is the oracle's result for that scan, or a list
    of them for a scan of several regions."""
    if on_scan is not None:
        on_scan(eng, exp)


def fuzz_match_oracle(eng, seeds, kw, case_base, on_scan=None, shift=0, front=0):
    """The random read sets case_base + seed through the engine with the parameters kw: every line equals the oracle's, and (18 channels,
    no splice padding) every column of the scan equals generate_tensor on the oracle's mpileup row.  Returns (cases, lines) seen.
    shift, front (here and in the helpers below): the case translated by place() — reads, reference slice, region, BED intervals and sites move
    together; the defaults are the case as generated."""
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    channels = kw.get("channels", 18)
    okw = dict(kw)
    okw.pop("channels", None)
    for k in ("head_tail", "splice_padding"):
        if k in okw:
            okw[k] = bool(okw[k])
    if "snp_min_af" in okw:
        okw["snp_af"] = okw.pop("snp_min_af")
    n_cases, n_lines = 0, 0
    for seed in seeds:
        rs, ref, first, last, recs = placed_case(case_base + seed, channels == 30, shift, front)
        eng.params = capi.default_params()
        eng.set_bed(0, None); eng.set_bed(1, None)
        eng.set_params(min_coverage=kw.get("min_coverage", 2), **{k: v for k, v in kw.items() if k != "min_coverage"})
        exp = oracle_chunk(rs, ref, first, first, last, channels=channels, min_coverage=kw.get("min_coverage", 2),
                           **{k: v for k, v in okw.items() if k != "min_coverage"})
        got = engine_chunk(eng, rs, ref, first, first, last)
        _scanned(on_scan, eng, exp)
        assert got["lines"] == exp["lines"], (seed, recs, first_diff(got["lines"], exp["lines"]))
        if channels == 18 and not kw.get("splice_padding"):
            col = eng.columns()
            rows = exp["rows"]
            assert len(rows) == int((col["flags"] & 1).sum()), (seed, recs)
            for row in rows:
                f = row.split("\t")
                pos = int(f[1])
                o = orc.generate_tensor(f[4], ref[pos - first].upper(), pos, ref.upper(), first, snp_af=okw.get("snp_af", 0.08))
                i = pos - col["region_start"]
                assert col["cols"][i].tolist() == o["tensor"], (seed, pos, f[4], recs)
                assert col["depth"][i] == o["depth"], (seed, pos)
        n_cases += 1
        n_lines += len(exp["lines"])
    eng.params = capi.default_params()
    eng.set_params()
    return n_cases, n_lines


def fuzz_samtools_1_11(eng, seeds, kw, case_base, on_scan=None, shift=0, front=0):
    """The same with c3r_params_t.mpileup_compat = 1 (pads inside insertions, a deletion right behind an insertion).  Returns
    (lines, columns that show an insertion with a deletion behind it, padded alleles, cases the pad table refused)."""
    import re
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    channels = kw.get("channels", 18)
    okw = {k: bool(v) for k, v in kw.items() if k != "channels"}
    n_lines, n_both, n_padded, n_refused = 0, 0, 0, 0
    eng.load_reads(ReadSet.from_records([]))
    for seed in seeds:
        rs, ref, first, last, recs = placed_case(case_base + seed, channels == 30, shift, front)
        eng.params = capi.default_params()
        eng.set_bed(0, None); eng.set_bed(1, None)
        eng.set_params(min_coverage=2, mpileup_compat=1, **kw)
        exp = oracle_chunk(rs, ref, first, first, last, channels=channels, min_coverage=2, mpileup_compat=1, **okw)
        try:
            got = engine_chunk(eng, rs, ref, first, first, last)
            _scanned(on_scan, eng, exp)
        except capi.C3RError as e:
            # the documented limit of the pad table (c3r_padins_t: a 64-bit mask per run of I and P ops); the generator reaches it on a few seeds
            assert "more than 64 characters" in str(e), (seed, e)
            n_refused += 1
            continue
        assert got["lines"] == exp["lines"], (seed, recs, first_diff(got["lines"], exp["lines"]))
        n_lines += len(exp["lines"])
        n_both += sum(1 for r in exp["rows"] if re.search(r"[+][0-9]+[ACGTNacgtn=RYry*#]+-[0-9]+[Nn]", r.split("\t")[4]))
        n_padded += sum(1 for l in exp["lines"] if re.search(r" I[ACGT][A-Z=]*[*#]", l.split("\t")[4]))
        if seed % 20 == 0:                      # the same reads with the <= 1.10 text: the records are rebuilt when the parameter changes
            eng.set_params(min_coverage=2, mpileup_compat=0, **kw)
            n0 = eng.scan(first, last)
            old = oracle_chunk(rs, ref, first, first, last, channels=channels, min_coverage=2, **okw)
            _scanned(on_scan, eng, old)
            assert n0 == len(old["lines"])
    eng.params = capi.default_params()
    eng.set_params()
    return n_lines, n_both, n_padded, n_refused


def filters_case(seed, mode, case_base, rng_base, head_tail=None, shift=0, front=0):
    """The inputs of one case of fuzz_filters_and_regions at their coordinates (place): dict(rs, ref, ref_start, a, b, lbed, cbed, sites, ht).
    The random draws are made in the case's own coordinates and translated afterwards, so a case is the same case at every translation."""
    import random
    from clair3_rna_amd.reads import ReadSet
    rng = random.Random(rng_base + seed)
    info = {}
    ref, recs = _case(case_base + seed, phased=False, info=info)
    if mode == "deep":              # replicate the reads: depth 150-400 with identical alleles (I1/D1 multiplicities, rescale)
        rep = rng.randint(6, 9)
        recs = [dict(r) for r in recs for _ in range(rep)]
        recs.sort(key=lambda r: r["pos"])
    L = len(ref)

    def intervals(k):
        out = []
        for _ in range(k):
            a = rng.randint(0, L - 2)
            out.append((a, min(L, a + rng.choice([1, 2, 5, 17, 33, 60, 150]))))
        return out
    lbed = intervals(rng.randint(1, 6)) if mode in ("lbed", "both_beds") else None
    cbed = intervals(rng.randint(1, 6)) if mode in ("cbed", "both_beds") else None
    sites = sorted(set(rng.randint(1, L) for _ in range(rng.randint(1, 25)))) if mode == "sites" else None
    ref_start, a, b = 1, 1, L
    if mode == "subregion":
        a = rng.randint(2, L // 2); b = rng.randint(a, L)
        ref_start = rng.randint(1, max(1, a - 49))   # the slice starts before the region's halo and its windows (the
                                                     # reference fetches ctg_start - 1000: every row and flank is covered)
    if mode == "sites":
        a, b = min(sites), max(sites)
    ht = seed % 2 if head_tail is None else int(head_tail)
    K, recs, ref, first = place(ref, recs, shift, front, info["hot"], case_base + seed)
    if K:
        lbed = lbed and [(x + K, y + K) for x, y in lbed]
        cbed = cbed and [(x + K, y + K) for x, y in cbed]
        sites = sites and [x + K for x in sites]
    # (the slice: `front` more bases before ref_start; the region: `front` more positions before a)
    return dict(rs=ReadSet.from_records(recs), ref=ref[ref_start - 1:], ref_start=ref_start + K - front, a=a + K - front, b=b + K,
                lbed=lbed, cbed=cbed, sites=sites, ht=ht)


def filters_oracle(c):
    return oracle_chunk(c["rs"], c["ref"], c["ref_start"], c["a"], c["b"], lbed=c["lbed"], bed=c["cbed"], sites=c["sites"], min_coverage=2,
                        head_tail=bool(c["ht"]))


def fuzz_filters_and_regions(eng, seeds, mode, case_base, rng_base, head_tail=None, on_scan=None, shift=0, front=0):
    """The random read sets through the -l BED, the confident BED, a genotyping site list, a sub-region with a shifted reference slice,
    and at depths that cross the 216 rescale threshold.  head_tail: None = on for the odd seeds, else that value for every case.
    Returns the lines seen."""
    from clair3_rna_amd import capi
    n_lines = 0
    for seed in seeds:
        c = filters_case(seed, mode, case_base, rng_base, head_tail, shift, front)
        lbed, cbed, sites = c["lbed"], c["cbed"], c["sites"]
        eng.params = capi.default_params()
        eng.set_bed(0, lbed); eng.set_bed(1, cbed)
        if sites is not None:
            eng.set_sites(sites)
        eng.set_params(min_coverage=2, genotyping_mode=int(sites is not None), head_tail=c["ht"])
        exp = filters_oracle(c)
        got = engine_chunk(eng, c["rs"], c["ref"], c["ref_start"], c["a"], c["b"])
        _scanned(on_scan, eng, exp)
        assert got["lines"] == exp["lines"], (mode, seed, lbed, cbed, sites, (c["ref_start"], c["a"], c["b"]), first_diff(got["lines"], exp["lines"]))
        assert np.array_equal(got["X"], exp["X"]), (mode, seed)
        n_lines += len(exp["lines"])
    eng.params = capi.default_params()
    eng.set_bed(0, None); eng.set_bed(1, None)
    eng.set_params()
    return n_lines


def fuzz_decode_rows_and_regions(eng, seeds, compat, case_base, rng_base, on_scan=None, shift=0, front=0):
    """On the random read sets: (1) c3r_call_rows (C++: tokens -> ordered alt_info -> decode -> row text) equals the Python path fed with the
    ORACLE's alt_info strings; (2) a multi-region scan over random chunk boundaries equals successive scans.  Returns (rows, genotypes seen)."""
    import random
    from clair3_rna_amd import capi, decode, synth
    from clair3_rna_amd.reads import ReadSet
    w = synth.random_weights(18, seed=4242)
    w[-24 * 129:] *= 6.0                       # sharper output layers: not everything decodes to RefCall
    eng.load_weights(w, 18)
    eng.set_precision("f16x3")
    n_rows, kinds = 0, set()
    seeds = list(seeds)
    for seed in seeds:
        rng = random.Random(rng_base + seed)
        rs, ref, first, last, recs = placed_case(case_base + seed, False, shift, front)
        L, K = last - first + 1 - front, first + front - 1          # (the case's own length; its translation)
        eng.params = capi.default_params()
        eng.set_bed(0, None); eng.set_bed(1, None)
        if seed == seeds[0]:
            eng.load_reads(ReadSet.from_records([]))
        eng.set_params(min_coverage=2, mpileup_compat=compat)
        exp = oracle_chunk(rs, ref, first, first, last, min_coverage=2, mpileup_compat=compat)
        got = engine_chunk(eng, rs, ref, first, first, last)
        _scanned(on_scan, eng, exp)
        assert got["lines"] == exp["lines"]
        if exp["lines"]:
            probs = eng.infer()
            po = orc.forward(w, exp["X"])
            assert np.abs(probs - po).max() < 1e-4
            f = [l.split("\t") for l in exp["lines"]]
            py = decode.vcf_rows("chr20", [int(x[1]) for x in f], [x[2] for x in f], [x[4] for x in f], probs)
            cpp = eng.call_rows("chr20")
            assert cpp == py, (seed, [a for a, b in zip(cpp, py) if a != b][:2], [b for a, b in zip(cpp, py) if a != b][:2])
            n_rows += len(py)
            kinds.update(r.split("\t")[9].split(":")[0] for r in py)
        # random chunking of the same contig
        cuts = sorted(set([1, L] + [rng.randint(2, L - 1) for _ in range(rng.randint(1, 5))]))
        cuts = [first] + [c + K for c in cuts[1:]]
        chunks = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]
        eng.begin_batch()
        for a, b in chunks:
            eng.scan(a, b)
            _scanned(on_scan, eng, None)
        eng.end_batch()
        X1, S1, T1 = eng.tensors(), eng.sites(), eng.tokens()
        eng.begin_batch(); eng.scan_regions(chunks); eng.end_batch()
        _scanned(on_scan, eng, None)
        assert np.array_equal(X1, eng.tensors()) and S1.tobytes() == eng.sites().tobytes() and T1.tobytes() == eng.tokens().tobytes(), (seed, chunks)
    eng.params = capi.default_params()
    eng.set_params()
    return n_rows, kinds


def fuzz_depth_cap(eng, seeds, channels, case_base, rng_base, splice_padding=None, head_tail=None, on_scan=None, shift=0, front=0):
    """samtools mpileup -d on replicated random read sets, small caps: the engine equals the oracle for the region and for its two halves
    (a two-region scan equals two successive scans equals the per-region oracle).  splice_padding / head_tail: None = by the seed's
    low bits, else that value for every case.  Returns the cases in which the cap changed the output."""
    import random
    from clair3_rna_amd import capi
    from clair3_rna_amd.reads import ReadSet
    n_dropped_cases = 0
    for seed in seeds:
        rng = random.Random(rng_base + seed)
        info = {}
        ref, recs = _case(case_base + seed, phased=(channels == 30), info=info)
        rep = rng.randint(3, 7)
        recs = [dict(r) for r in recs for _ in range(rep)]
        recs.sort(key=lambda r: r["pos"])
        L = len(ref)
        K, recs, ref, first = place(ref, recs, shift, front, info["hot"], case_base + seed)
        rs = ReadSet.from_records(recs)
        cap = rng.choice([8, 20, 60, 150])
        sp = seed % 2 if splice_padding is None else int(splice_padding)
        ht = (seed // 2) % 2 if head_tail is None else int(head_tail)
        kw = dict(min_coverage=2, max_depth=cap, splice_padding=sp, head_tail=ht)
        okw = dict(channels=channels, min_coverage=2, splice_padding=bool(sp), head_tail=bool(ht))
        eng.params = capi.default_params()
        eng.set_bed(0, None); eng.set_bed(1, None)
        eng.set_params(channels=channels, **kw)
        a = rng.randint(1, L // 3); b = rng.randint(2 * L // 3, L)
        a, b = a + K - front, b + K
        exp = oracle_chunk(rs, ref, first, a, b, max_depth=cap, **okw)
        got = engine_chunk(eng, rs, ref, first, a, b)
        _scanned(on_scan, eng, exp)
        nocap = oracle_chunk(rs, ref, first, a, b, max_depth=0, **okw)
        n_dropped_cases += int(exp["lines"] != nocap["lines"])
        assert got["lines"] == exp["lines"], (seed, cap, first_diff(got["lines"], exp["lines"]))
        assert np.array_equal(got["X"], exp["X"])
        # the same through a two-region scan (masks are per region)
        mid = (a + b) // 2
        e1 = oracle_chunk(rs, ref, first, a, mid, max_depth=cap, **okw)
        e2 = oracle_chunk(rs, ref, first, mid, b, max_depth=cap, **okw)
        eng.begin_batch()
        eng.scan(a, mid); _scanned(on_scan, eng, e1)
        eng.scan(mid, b); _scanned(on_scan, eng, e2)
        eng.end_batch()
        X1, S1 = eng.tensors(), eng.sites()
        eng.begin_batch(); eng.scan_regions([(a, mid), (mid, b)]); eng.end_batch()
        _scanned(on_scan, eng, [e1, e2])
        assert np.array_equal(X1, eng.tensors()) and S1.tobytes() == eng.sites().tobytes()
        assert [int(l.split("\t")[1]) for l in e1["lines"] + e2["lines"]] == S1["pos"].tolist()
        assert np.array_equal(X1, np.concatenate([e1["X"], e2["X"]])) if len(S1) else True
    eng.params = capi.default_params()
    eng.set_params()
    return n_dropped_cases


# ---- the deep routes (tests/test_gpu_deep_routes.py, tests/test_gpu_coords.py): environment variables that the library reads at every scan
NEVER = str(1 << 30)
ROUTES = {
    # every listed span: k_fused_deep, no arrival-order buffer — a span above 3072 events walks its records again
    "deep_walk_twice": dict(C3R_DEEP_MIN="1", C3R_SPLIT_MIN=NEVER, C3R_EVWG="0"),
    # every listed span: k_fused_deep, events taken from the workgroup's buffer (up to 49152)
    "deep_event_buffer": dict(C3R_DEEP_MIN="1", C3R_SPLIT_MIN=NEVER, C3R_EVWG="1"),
    # every listed span: k_deep_walk in 64-record slices, alleles from k_deep_alleles' table (the soak of tests/evidence/README.md)
    "giant_slices": dict(C3R_DEEP_MIN="1", C3R_SPLIT_MIN="1", C3R_GIANT="1", C3R_EVWG="1", C3R_SPLIT_CUS="1000000000", C3R_SPLIT_SLICE="64"),
    # the natural thresholds
    "default": dict(),
    # (control) every span: k_fused_tiles
    "tiles_only": dict(C3R_DEEP_MIN=NEVER),
}
ROUTE_VARS = sorted(set(k for r in ROUTES.values() for k in r))
SLICE, MAX_SLICES, SLOTS = 64, 32, 256         # C3R_SPLIT_SLICE above; GIANT_MAX_HELP; GIANT_SLOTS


def _set_route(monkeypatch, route):
    for k in ROUTE_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)


def routed_get(monkeypatch, engines):
    """The body of a test module's `routed` fixture.  routed(route) -> the route's engine: a context of its own, created after the route's
    variables are set, kept in the module's `engines` (which the module closes at its end)."""
    def get(route, fresh=False):
        from clair3_rna_amd import capi
        _set_route(monkeypatch, route)
        if fresh:
            return capi.Engine(0)
        if route not in engines:
            engines[route] = capi.Engine(0)
        return engines[route]
    return get


def _most_aligned(exp):
    """The most reads that show a base or a deletion on one position (each is a record of the span that holds the position)."""
    best = 0
    for row in exp["rows"]:
        f = row.split("\t")
        if int(f[3]) > best:                       # (mpileup's own depth counts ref-skips too: an upper bound, so look closer only then)
            b = f[4]
            best = max(best, int(f[3]) - b.count("<") - b.count(">"))
    return best


def route_check(route, seen=None):
    """on_scan(eng, exp) for the fuzz helpers above: the assertions on Engine.scan_counts() that hold after EVERY scan of a route."""
    def on_scan(eng, exp):
        c = eng.scan_counts()
        exps = [e for e in (exp if isinstance(exp, list) else [exp]) if e is not None]
        if any(e["lines"] for e in exps):
            assert c["listed"] > 0, (route, c)
        if route in ("deep_walk_twice", "deep_event_buffer"):
            assert c["deep"] == c["listed"] and c["giant"] == 0 and c["slices"] == 0, (route, c)
        elif route == "giant_slices":
            assert c["deep"] == c["listed"] and c["giant"] == c["listed"] and c["slices"] >= min(c["giant"], SLOTS), (route, c)
            if c["giant"] <= SLOTS and any(_most_aligned(e) > SLICE for e in exps):
                assert c["slices"] > c["giant"], (route, c)
        elif route == "tiles_only":
            assert c["deep"] == 0 and c["giant"] == 0 and c["slices"] == 0, (route, c)
        if seen is not None:
            for k in c:
                seen[k] = seen.get(k, 0) + c[k]
            seen["scans"] = seen.get("scans", 0) + 1
    return on_scan


# ---- read sets sized for the thresholds of the deep-span kernels (tests/test_gpu_deep_routes.py) ------------------------------------------
def _zoo_alleles(rng, n, compat):
    """n indel alleles as (cigar ops, inserted bases, reference length): insertions of 1-22 bases (the event key holds 16: pairs that agree in
    their first 16 bases and differ behind them), '='-only insertions (no strand), deletions of 1-5 bases whole, split `D D` and with a
    zero-length op inside; compat = 1 adds `I P I` runs and an I with a D right behind it (what samtools >= 1.11 prints differently).
    The three most frequent alleles are such a pair and a third sibling: a comparison that stops at the key would merge them into a count
    that no true allele of the column has (long_insertions_tell)."""
    b = "".join(rng.choice("ACGT") for _ in range(20))
    out = [("20I", b, 0), ("20I", b[:16] + ("A" if b[16] != "A" else "C") + b[17:], 0), ("20I", b[:-1] + ("G" if b[-1] != "G" else "T"), 0)]
    while len(out) < n:
        r = rng.random()
        if r < 0.40:
            k = rng.randint(1, 4)
            out.append(("%dI" % k, "".join(rng.choice("ACGT") for _ in range(k)), 0))
        elif r < 0.55:                                            # longer than the key: siblings that differ in base 17 and in the last base
            k = rng.randint(17, 22)
            b = "".join(rng.choice("ACGT") for _ in range(k))
            out.append(("%dI" % k, b, 0))
            out.append(("%dI" % k, b[:16] + ("A" if b[16] != "A" else "C") + b[17:], 0))
            out.append(("%dI" % k, b[:-1] + ("G" if b[-1] != "G" else "T"), 0))
            out.append(("%dI" % (k - 1), b[:-1], 0))              # (and its prefix: same key, another length)
        elif r < 0.62:
            k = rng.choice([1, 2, 3, 16, 17, 18])
            out.append(("%dI" % k, "=" * k, 0))
            if k > 16:
                out.append(("%dI" % k, "=" * (k - 1) + "A", 0))    # '=' in the key, a base behind it: that one has a strand
        elif r < 0.85:
            k = rng.randint(1, 5)
            out.append(("%dD" % k, "", k))
            if k > 1:
                j = rng.randint(1, k - 1)
                out.append(("%dD%dD" % (j, k - j), "", k))
                out.append(("%dD0%s%dD" % (j, rng.choice("MI"), k - j), "", k))
        elif compat:
            if rng.random() < 0.5:
                j, k, q = rng.randint(1, 3), rng.randint(1, 3), rng.randint(1, 2)
                out.append(("%dI%dP%dI" % (j, q, k), "".join(rng.choice("ACGT") for _ in range(j + k)), 0))
            else:
                k, d = rng.randint(1, 3), rng.randint(1, 3)
                out.append(("%dI%dD" % (k, d), "".join(rng.choice("ACGT") for _ in range(k)), d))
    return out[:n]


def _ip_run_chars(cigar):
    """The longest printed run of I and P ops of a CIGAR (the pad table of mpileup_compat = 1 takes 64 characters)."""
    import re
    best = cur = 0
    for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar):
        if o in "IP":
            cur += int(n)
            best = max(best, cur)
        elif int(n) > 0:
            cur = 0
    return best


def allele_zoo(n_reads, seed, compat=0, events_per_read=1, random_share=0.1, n_alleles=300, anchors=(300, 303, 306), offset=0, ref=None):
    """(ref, records): short reads around two or three anchor columns (0-based, + offset), every read with an insertion or a deletion on its
    anchor drawn from a skewed (1 / rank) distribution over n_alleles alleles (_zoo_alleles), both strands, three haplotype tags, 5 % mismatches.
    events_per_read = 1: `aM <indel> bM`, a and b in 2 .. 5.  events_per_read = k > 1: `1M (<indel> 1M) * k` with the indels that take at most one
    reference base, all starting within three positions — more than 0.375 events per record, all of them inside 17 positions.  random_share of
    the reads take a CIGAR, flags and a mapping quality from the random generator instead (runs of I and P ops within the pad table's 64 characters)."""
    import random
    rng = random.Random(seed)
    alleles = _zoo_alleles(rng, n_alleles, compat)
    if events_per_read > 1:
        alleles = [a for a in alleles if a[2] <= 1]
    weights = [1.0 / (k + 1) for k in range(len(alleles))]
    L = 900 + offset
    if ref is None:
        ref = "".join(rng.choice("ACGT") for _ in range(L))

    def aligned(p, n):
        return "".join(c if rng.random() >= 0.05 else rng.choice("ACGT") for c in ref[p:p + n])
    recs = []
    n_random = int(round(n_reads * random_share))
    picks = rng.choices(range(len(alleles)), weights=weights, k=(n_reads - n_random) * events_per_read)
    for r in range(n_reads - n_random):
        if events_per_read == 1:
            ops, ins, dl = alleles[picks[r]]
            a, b = rng.randint(2, 5), rng.randint(2, 5)
            p0 = offset + rng.choice(anchors) - a
            cigar, seq = "%dM%s%dM" % (a, ops, b), aligned(p0, a) + ins + aligned(p0 + a + dl, b)
        else:
            p0 = offset + anchors[0] + rng.randint(0, 2)
            cigar, seq, p = "1M", aligned(p0, 1), p0 + 1
            for e in range(events_per_read):
                ops, ins, dl = alleles[picks[r * events_per_read + e]]
                cigar += ops + "1M"
                seq += ins + aligned(p + dl, 1)
                p += dl + 1
        recs.append(dict(pos=p0, cigar=cigar, seq=seq, flag=16 if rng.random() < 0.5 else 0, mapq=60, hp=rng.choice([0, 1, 2])))
    for _ in range(n_random):
        while True:
            cg, qlen = _rand_cigar(rng, 0, pads=True)
            if _ip_run_chars(cg) <= 64:
                break
        if rng.random() < 0.1:
            qlen = max(1, qlen - rng.randint(1, 3))
        recs.append(dict(pos=max(1, offset + int(rng.gauss(anchors[0], 40))), cigar=cg, seq="".join(rng.choice("ACGTACGTACGTACGTN=RY") for _ in range(qlen)),
                         flag=(16 if rng.random() < 0.5 else 0) | rng.choice([0] * 14 + [256, 2048, 4, 1024, 512, 8, 1, 3, 65, 131]),
                         mapq=rng.choice([60] * 8 + [0, 3, 5, 4, 20, 255]), hp=rng.choice([0, 1, 2])))
    recs.sort(key=lambda r: r["pos"])
    end = max(r["pos"] + cigar_ref_len(r["cigar"]) for r in recs)
    if end + 40 > len(ref):
        ref = ref + "".join(rng.choice("ACGT") for _ in range(end + 40 - len(ref)))
    return ref, recs


def long_insertions_tell(recs, min_mq=5, excl_flags=2316):
    """True if a comparison of insertions that looked at the 16 bases of the event key only would change I1 or i1 somewhere: on some column and
    strand the plain insertions (`aM kI ...`, no pads) that share length and first 16 bases outnumber the most frequent insertion allele."""
    import re
    full, trunc = {}, {}
    for r in recs:
        if r.get("mapq", 60) < min_mq or (r.get("flag", 0) & excl_flags):
            continue
        ops = re.findall(r"(\d+)([MIDNSHP=X])", r["cigar"])
        p, q = r["pos"], 0
        for k, (ln, o) in enumerate(ops):
            ln = int(ln)
            if o == "I":
                where = (p, r.get("flag", 0) & 16)
                alone = (k == 0 or ops[k - 1][1] in "M=X") and (k + 1 == len(ops) or ops[k + 1][1] in "M=X")
                bases = r["seq"][q:q + ln] if alone else "%d:%s" % (k, r["cigar"])          # (runs of ops: every CIGAR an allele of its own)
                full.setdefault(where, {}).setdefault((ln, bases), 0)
                full[where][(ln, bases)] += 1
                trunc.setdefault(where, {}).setdefault((ln, bases[:16] if alone else bases), 0)
                trunc[where][(ln, bases[:16] if alone else bases)] += 1
            if o in "M=XDN":
                p += ln
            if o in "MIS=X":
                q += ln
    return any(max(trunc[w].values()) > max(full[w].values()) for w in full)


def cigar_ref_len(cigar):
    import re
    return sum(int(n) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if o in "MDN=X")


def span_bounds(recs, rows, ref, ref_start=1, min_mq=5, excl_flags=2316):
    """What the largest span of a scan must and may hold, from the CIGARs (records) and the oracle's columns (indel events; rows: its mpileup
    rows for the scan).  A span builds the columns of up to 256 positions — its own 224 and 16 on either side — from every record that touches
    them, so:
      * at least: whatever lies within 16 consecutive positions (the span that holds the first of them reaches 16 further), hence also what
        lies on one position, and total / (ceil(extent / 224) + 1) when everything lies within `extent` positions;
      * at most: the total.
    Records: one per M / = / X / D piece of at most 30 positions plus one per insertion, counted at their first position (the insertion: at the
    base before it); the lower bound takes the reads that pass the filters and no insertion, the upper one every read and every op.
    Events: the I + i + D + d counts of the oracle's column.  Returns dict(rec_lo, rec_hi, ev_lo, ev_hi, max_depth)."""
    import re
    n = max(r["pos"] + cigar_ref_len(r["cigar"]) for r in recs) + 64
    starts = np.zeros(n + 32, np.int64)
    rec_hi = 0
    for r in recs:
        ok = r.get("mapq", 60) >= min_mq and not (r.get("flag", 0) & excl_flags)
        p = r["pos"]
        for ln, o in re.findall(r"(\d+)([MIDNSHP=X])", r["cigar"]):
            ln = int(ln)
            if o in "M=XD":
                for q in range(0, ln, 30):
                    rec_hi += 1
                    if ok:
                        starts[p + q] += 1
                p += ln
            elif o == "N":
                p += ln
            elif o == "I":
                rec_hi += 1
    ev = np.zeros(n + 32, np.int64)
    depth = 0
    up = ref.upper()
    for row in rows:
        f = row.split("\t")
        pos = int(f[1])
        o = orc.generate_tensor(f[4], up[pos - ref_start], pos, up, ref_start)
        t = o["tensor"]
        ev[pos - 1] = t[4] + t[6] + t[13] + t[15]                 # I, D, i, d
        depth = max(depth, o["depth"])

    def lower(v):
        nz = np.nonzero(v)[0]
        if len(nz) == 0:
            return 0
        c = np.concatenate([[0], np.cumsum(v)])
        extent = int(nz[-1] - nz[0] + 1)
        return int(max((c[16:] - c[:-16]).max(), -(-int(v.sum()) // (-(-extent // 224) + 1))))
    return dict(rec_lo=max(lower(starts), depth), rec_hi=rec_hi, ev_lo=lower(ev), ev_hi=int(ev.sum()), max_depth=depth)


# ---- network inputs and weights shared by the network tests ---------------------------------------------------------------------
def blob_offsets(C):
    """start of (LSTM1 dir0 K, R, b | dir1 ... | LSTM2 ... | L4 W, b | heads) in the weight blob (include/c3r.h, c3r_load_weights)."""
    H1, H2 = 128, 160
    n1 = C * 4 * H1 + H1 * 4 * H1 + 4 * H1
    n2 = 2 * H1 * 4 * H2 + H2 * 4 * H2 + 4 * H2
    return dict(l1=0, l1_bias0=C * 4 * H1 + H1 * 4 * H1, l2=2 * n1, l2_bias0=2 * n1 + 2 * H1 * 4 * H2 + H2 * 4 * H2, l4=2 * n1 + 2 * n2, l4_bias=2 * n1 + 2 * n2 + 33 * 320 * 128)


def scaled_weights(C, seed=1234):
    """Weights that need a run-time scale in every split-f16 layer (the RTS kernels): a layer-1 weight of 20, a layer-2 bias of 30 and
    an L4 weight of 100 on top of synth.random_weights — the values of the guard tests."""
    from clair3_rna_amd import synth
    o = blob_offsets(C)
    w = synth.random_weights(C, seed=seed)
    w[o["l1"] + 5] = 20.0
    w[o["l2_bias0"] + 3] = 30.0
    w[o["l2"] + 11] = 9.0
    w[o["l4"] + 99] = 100.0
    return w


def pileup_like(n, C, seed):
    """Windows shaped like the pileup tensor (tools/precision_probe.py): negative reference channels, a few alt counts, mixed depths."""
    r = np.random.RandomState(seed)
    X = np.zeros((n, 33, C), np.int32)
    for s in range(n):
        depth = int(r.choice([6, 12, 20, 40, 90, 216]))
        for t in range(33):
            k = r.randint(0, 4)
            fwd = r.binomial(depth, 0.5)
            X[s, t, k] = -fwd
            X[s, t, 9 + k] = -(depth - fwd)
            for _ in range(r.randint(0, 3)):
                X[s, t, r.randint(0, C)] += r.randint(1, max(2, depth // 3))
    return X


def deep_flank_windows(n, C, D, seed):
    """Windows of a candidate in a shallow locus beside a deep one.  The A5 rescale divides a window by the depth of its CENTRE position
    only (clair3_rna/utils.py:88-92), so a centre of 216 reads or fewer leaves the counts of the whole window as they are — also where
    its flank reaches into an exon covered by thousands of reads.  Pileup-shaped: the reference base's channels carry minus the strand
    totals, a few alt counts on top; centre depth from {6 .. 320} (above 216 the window is rescaled by 216 / depth, as the tensor build
    would); a contiguous run of 4 .. 16 positions at one end of the window with depths from [D / 2, D], split over the strands by a
    per-site ratio (so that the counts are of both parities)."""
    r = np.random.RandomState(seed)
    X = np.zeros((n, 33, C), np.int64)
    for s in range(n):
        centre = int(r.choice([6, 12, 20, 40, 90, 216, 320]))
        run, left, p = r.randint(4, 17), r.randint(0, 2), r.uniform(0.3, 0.7)
        for t in range(33):
            deep = t < run if left else t >= 33 - run
            depth = int(r.randint(D // 2, D + 1)) if deep else max(1, centre + int(r.randint(-centre // 4, centre // 4 + 1)))
            k = r.randint(0, 4)
            fwd = int(r.binomial(depth, p))
            X[s, t, k] = -fwd
            X[s, t, 9 + k] = -(depth - fwd)
            for _ in range(r.randint(0, 3)):
                X[s, t, r.randint(0, C)] += r.randint(1, max(2, depth // 3))
        if centre > 216:
            X[s] = (X[s] * (216.0 / centre)).astype(np.int64)                  # (the reference truncates toward zero: int(x * 216 / depth))
    assert np.abs(X).max() < 2 ** 31
    return X.astype(np.int32)


EDGE_COUNTS = (2047, 2048, 2049, 4097, 65504, 65505)


def edge_count_windows(C, seed):
    """Shallow pileup-shaped windows with ONE entry each set to +-v, v around the ends of what one f16 holds (integers to 2048, 65504 at
    most): four windows per value and sign, the entry at varying positions and channels."""
    r = np.random.RandomState(seed)
    vals = [sg * v for v in EDGE_COUNTS for sg in (1, -1) for _ in range(4)]
    X = pileup_like(len(vals), C, seed + 1)
    for s, v in enumerate(vals):
        X[s, r.randint(0, 33), r.randint(0, C)] = v
    return X


def shallow_locus_beside_a_deep_one(n_deep, deep_len=60, n_shallow=12, fwd_every=3, seed=5):
    """(ref, ReadSet): n_deep reads `<deep_len>M` that END at 0-based 159, one in `fwd_every` on the reverse strand (fwd_every = 0: all
    forward), and n_shallow reads 60M at 150 with a SNP 20 bases in (0-based 170): one candidate of depth n_shallow whose window
    (154 .. 186) reaches six positions into the deep pile."""
    import random
    from clair3_rna_amd.reads import ReadSet
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(400))
    p0 = 160 - deep_len
    recs = [dict(pos=p0, cigar="%dM" % deep_len, seq=ref[p0:160], flag=16 if fwd_every and i % fwd_every == 0 else 0) for i in range(n_deep)]
    alt = "A" if ref[170] != "A" else "C"
    recs += [dict(pos=150, cigar="60M", seq=ref[150:170] + alt + ref[171:210], flag=16 * (i % 2)) for i in range(n_shallow)]
    return ref, ReadSet.from_records(recs)


# ---- read sets sized for the limits of c3r_load_reads (reads_kernels.hpp: k_prep, k_prefmax_bins, k_bin_scan; c3r_lib.hip: prepare_tables).
# tests/test_load_edges_ref.py holds each generator in its bracket against the oracle alone, tests/test_gpu_load_edges.py runs the engine.
# The numbers below are the kernels' constants; tests/c/layout_check.hip ties each to its name.
LOAD_BIN, LOAD_CBIN = 32, 256                  # positions of a bin (C3R_BIN_SHIFT = 5) and of a coarse bin (CBIN_SHIFT = 3)
PREP_READS, HB, HB_PROBES, WG_TAB_PAIRS = 16, 1024, 16, 510          # reads of a k_prep workgroup; slots and probes of its LDS hash; pairs of its slab
PM_BLK, BS_BLK = 1024, 4096                    # reads of a k_prefmax_bins block; bins of a k_bin_scan block
BIN_END_GUESS = 1 << 21                        # prepare_tables sizes the bin table to the last read's start plus this
OP_CHOP = 30                                   # positions of one record


def random_reference(n, seed):
    """n random bases as str, built with numpy."""
    return np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(seed).randint(0, 4, n)].tobytes().decode()


def _with_subs(ref, p0, n, sites):
    """ref[p0:p0 + n] with a substitution on every reference position of `sites` that it covers (A, or C where the reference has A)."""
    seq = list(ref[p0:p0 + n])
    for p in sites:
        if p0 <= p < p0 + n:
            seq[p - p0] = "A" if ref[p] != "A" else "C"
    return "".join(seq)


def record_start_bins(recs):
    """Per read, the set of 32-position bins that hold the start of one of its records — plain `<n>M` reads and the `aM0DbM` form that
    the serial walk merges into one M: a record every OP_CHOP positions from the read's start."""
    import re
    out = []
    for r in recs:
        assert re.fullmatch(r"\d+M(0D\d+M)?", r["cigar"]), r["cigar"]
        out.append(set((r["pos"] + q) // LOAD_BIN for q in range(0, cigar_ref_len(r["cigar"]), OP_CHOP)))
    return out


def workgroup_bins(recs):
    """Per k_prep workgroup (16 consecutive reads): the distinct bins its records start in."""
    b = record_start_bins(recs)
    return [len(set().union(*b[i:i + PREP_READS])) for i in range(0, len(b), PREP_READS)]


def workgroup_whole_bins(recs):
    """Per k_prep workgroup: the bins that lie wholly inside one of its reads.  Records are cut every 30 positions, a bin has 32: every such
    bin holds a record start, so this is a lower bound of workgroup_bins that needs no knowledge of where the cuts fall."""
    out = []
    for i in range(0, len(recs), PREP_READS):
        bins = set()
        for r in recs[i:i + PREP_READS]:
            a, b = r["pos"], r["pos"] + cigar_ref_len(r["cigar"])
            bins.update(range(-(-a // LOAD_BIN), b // LOAD_BIN))
        out.append(len(bins))
    return out


def line_positions(lines):
    return [int(l.split("\t")[1]) for l in lines]


def reads_with_a_line(recs, lines):
    """Per read: does some line's position (1-based) lie inside the read's alignment?"""
    pos = np.array(sorted(set(line_positions(lines))), np.int64) - 1
    return [bool(np.searchsorted(pos, r["pos"] + cigar_ref_len(r["cigar"])) > np.searchsorted(pos, r["pos"])) for r in recs]


HASH_LOCI, HASH_PITCH, HASH_RLEN = 24, 8000, 5500


def hash_exhaustion_case(seed=31):
    """(ref, records): 24 loci 8000 positions apart, each two reads of 5500 M — the second 3 bases after the first, on the other strand and
    with the other haplotype — with a substitution every 97 bases on the same reference positions in both; every third locus is written
    `2750M0D2750M` (the serial walk).  Sixteen consecutive reads are eight loci that share no bin: 8 x 171 bins wholly inside a read, more
    than the 1024 slots of k_prep's hash."""
    L = 500 + HASH_LOCI * HASH_PITCH
    ref = random_reference(L, seed)
    recs = []
    for i in range(HASH_LOCI):
        p0 = 500 + i * HASH_PITCH
        sites = range(p0 + 40, p0 + HASH_RLEN, 97)
        cigar = "%dM0D%dM" % (HASH_RLEN // 2, HASH_RLEN // 2) if i % 3 == 0 else "%dM" % HASH_RLEN
        for rep in range(2):
            recs.append(dict(pos=p0 + 3 * rep, cigar=cigar, seq=_with_subs(ref, p0 + 3 * rep, HASH_RLEN, sites), flag=16 * rep, hp=1 + rep))
    return ref, recs


def hash_exhaustion_regions(L):
    """Chunks of 20000 positions: their boundaries fall inside loci 2, 4, 7, ... (a locus covers 500 + 8000 i .. + 5503)."""
    return [(a, min(a + 19999, L)) for a in range(1, L + 1, 20000)]


def slab_overflow_case(seed=11):
    """(ref, records) of tests/test_gpu_load.py's recount case: 12 loci of five reads, then 48 lone reads of 1300 M, one per 4 kb — sixteen
    of them are a workgroup of 16 x 41 = 656 bins, above the slab's 510 pairs and below the hash's 1024 slots.  The lone reads carry a
    substitution every 31 bases: with min_coverage = 1 every one is a candidate, and the 33-position windows of neighbouring candidates
    overlap, so every position of a lone read — every record that a recounting workgroup places — lies inside a compared window."""
    import random
    rng = random.Random(seed)
    pitch, rlen, n_loci, n_lone = 4000, 1300, 12, 48
    L = (n_loci + n_lone) * pitch + 3000
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    recs = []
    for i in range(n_loci):                          # loci of five reads with the same mismatches
        for rep in range(5):
            p0 = 500 + i * pitch + rep * 3
            seq = list(ref[p0:p0 + rlen])
            for q in range(60 - rep * 3, rlen, 97):
                seq[q] = "A" if ref[p0 + q] != "A" else "C"
            recs.append(dict(pos=p0, cigar="%dM" % rlen, seq="".join(seq), flag=16 * (rep % 2)))
    for i in range(n_lone):                          # ... and lone long reads, one per 4 kb
        p0 = 500 + (n_loci + i) * pitch
        recs.append(dict(pos=p0, cigar="%dM" % rlen, seq=_with_subs(ref, p0, rlen, range(p0 + 7, p0 + rlen, 31)), flag=16 * (i % 2)))
    recs.sort(key=lambda r: r["pos"])
    return ref, recs


EDGE_REF_LEN, BRIDGE_CIGAR, BRIDGE_SKIP = 2300000, "60M2200000N60M", 2200000
_edge_ref = []


def edge_reference():
    """The 2.3-Mb reference shared by the regrowth and the depth-cap-gate cases (built once)."""
    if not _edge_ref:
        _edge_ref.append(random_reference(EDGE_REF_LEN, 77))
    return _edge_ref[0]


def bridging_read(ref, pos, flag=0, mapq=60, hp=0, sites=None):
    """`60M2200000N60M` at 0-based pos with substitutions on the reference positions `sites` (default: 20 and 45 bases into either segment)."""
    far = pos + 60 + BRIDGE_SKIP
    if sites is None:
        sites = (pos + 20, pos + 45, far + 20, far + 45)
    return dict(pos=pos, cigar=BRIDGE_CIGAR, seq=_with_subs(ref, pos, 60, sites) + _with_subs(ref, far, 60, sites), flag=flag, mapq=mapq, hp=hp)


REGROW_BRIDGES, REGROW_SHORT, REGROW_SHORT0 = (1000, 1010, 1020, 1020), 3000, 2000


def regrowth_case(bridge_mapq=7):
    """(ref, records, near region, far region): four bridging reads that start at 1000, 1010 and 1020 (twice: mpileup's depth cap
    can discard only a read that is not the first on its position) and end beyond 2.2 Mb, then 3000
    reads of 50 M 20 positions apart (three blocks of k_prefmax_bins) with a substitution on every 37th reference position.  The last read
    starts near 62 kb: the bridging reads' end lies beyond that plus 2 Mb, so the first pass of the load runs twice; the far region's
    first read is found through prefix maxima that the bridging reads hold for all 3000 reads behind them."""
    ref = edge_reference()
    far = REGROW_BRIDGES[0] + 60 + BRIDGE_SKIP
    sites = [q + o for q in (REGROW_BRIDGES[0], far) for o in (24, 33, 42, 51)]          # (positions that all four bridging reads cover)
    recs = [bridging_read(ref, p, flag=16 * (k % 2), mapq=bridge_mapq, hp=1 + k % 2, sites=sites) for k, p in enumerate(REGROW_BRIDGES)]
    for k in range(REGROW_SHORT):
        p0 = REGROW_SHORT0 + 20 * k
        recs.append(dict(pos=p0, cigar="50M", seq=_with_subs(ref, p0, 50, range(-(-p0 // 37) * 37, p0 + 50, 37)), flag=16 * (k % 2), hp=k % 3))
    return ref, recs, (1, REGROW_SHORT0 + 20 * REGROW_SHORT + 100), (far - 250, far + 350)


GATE_K, GATE_M = 30, 10
GATE_FIRSTS, GATE_EDGES, GATE_DS = (1000, 1024), ("device", "host"), (-1, 0, 1)
GATE_CAPS = (GATE_K + 2, GATE_K + GATE_M + 1, 0)


def gate_edge(first, kind):
    """The 0-based position on which a 256-position coarse bin begins, two bins behind the first read: the device counts its coarse bins from
    the first read's 32-position bin (k_prep, k_bin_scan), the host's hot zones are absolute (depth_cap_mask)."""
    return ((first >> 5) << 5) + 512 if kind == "device" else ((first >> 8) + 2) << 8


def gate_case(first, kind, d, far=False):
    """(ref, records, last position to scan): an anchor pair at `first`, K = 30 reads of 60 M whose exclusive end is edge + d, M = 10 reads of
    60 M that start on the edge; every group with substitutions of its own.  far: one bridging read in front of the anchors, on the same
    position — the bin table then spans more than 4096 coarse bins (k_bin_scan's coarse chain has more than one block)."""
    ref = edge_reference()
    edge = gate_edge(first, kind)
    recs = [bridging_read(ref, first, mapq=60)] if far else []
    recs += [dict(pos=first, cigar="60M", seq=_with_subs(ref, first, 60, (first + 30,)), flag=16 * k) for k in range(2)]
    p0 = edge + d - 60
    recs += [dict(pos=p0, cigar="60M", seq=_with_subs(ref, p0, 60, (p0 + 11, p0 + 50)), flag=16 * (k % 2), hp=k % 3) for k in range(GATE_K)]
    recs += [dict(pos=edge, cigar="60M", seq=_with_subs(ref, edge, 60, (edge + 9, edge + 40)), flag=16 * (k % 2), hp=k % 3) for k in range(GATE_M)]
    last = edge + 200
    return (ref if far else ref[:last + 100]), recs, last


DEEP_TIE_TOKENS = (63, 64, 65, 128, 129, 200)


def deep_tie_loci(seed=11, n_ref_reads=4):
    """Hand-made reads for the row-export tests: one locus per entry of DEEP_TIE_TOKENS, 200 bp apart.  Every read of a locus spans 81 bp
    around its column and shows there one of: two mismatching bases (equal read counts), two insertion alleles (equal counts), two deletion
    lengths (equal counts); an odd total gets one read with a third base.  The carriers are interleaved in BAM order and alternate strands, so
    the FIRST read of each kind decides every tie of the decoder's allele choice — which a token order other than BAM order changes.
    n_ref_reads reads per locus show the reference.  Returns (ref, ReadSet, [1-based column of each locus])."""
    import random
    from clair3_rna_amd.reads import ReadSet
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(200 * len(DEEP_TIE_TOKENS) + 200))
    recs, cols = [], []
    for k, total in enumerate(DEEP_TIE_TOKENS):
        c = 100 + 200 * k                      # 0-based column
        s = c - 40
        cols.append(c + 1)
        others = [b for b in "ACGT" if b != ref[c]]
        rng.shuffle(others)
        pair = total // 2
        n_ins = n_del = pair // 3
        n_snv = pair - n_ins - n_del
        left, right = ref[s:c], ref[c + 1:s + 81]
        kinds = ([("X0", i) for i in range(n_snv)] + [("X1", i) for i in range(n_snv)] + [("I0", i) for i in range(n_ins)] + [("I1", i) for i in range(n_ins)] +
                 [("D0", i) for i in range(n_del)] + [("D1", i) for i in range(n_del)] + [("X2", 0)] * (total & 1) + [("R", i) for i in range(n_ref_reads)])
        kinds.sort(key=lambda t: (t[1], rng.random()))            # round-robin over the kinds, their order shuffled within a round
        ins = ("TG", "CAT") if ref[c + 1] != "T" else ("GT", "CAG")
        for j, (kind, _i) in enumerate(kinds):
            flag = 16 if j % 2 else 0
            if kind[0] == "X":
                recs.append(dict(pos=s, cigar="81M", seq=left + others[int(kind[1])] + right, flag=flag))
            elif kind[0] == "I":
                a = ins[int(kind[1])]
                recs.append(dict(pos=s, cigar="41M%dI40M" % len(a), seq=left + ref[c] + a + right, flag=flag))
            elif kind[0] == "D":
                d = (1, 3)[int(kind[1])]
                recs.append(dict(pos=s, cigar="41M%dD40M" % d, seq=left + ref[c] + ref[c + 1 + d:c + 1 + d + 40], flag=flag))
            else:
                recs.append(dict(pos=s, cigar="81M", seq=left + ref[c] + right, flag=flag))
    return ref, ReadSet.from_records(recs), cols


def build_row_export_check(exe, timeout=None):
    """tests/c/row_export_check.hip -> exe (hipcc cross-compiles for gfx950 without a GPU); None when there is no hipcc"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    cc = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function",
                         os.path.join(root, "tests", "c", "row_export_check.hip"), "-o", exe], capture_output=True, text=True, timeout=timeout)
    assert cc.returncode == 0 and "warning:" not in cc.stderr, cc.stderr[-3000:]
    return exe


# ---- scans at the fused scan's allocator switch (tests/test_scan_shards_ref.py holds every input on its floor with the oracle alone,
# tests/test_gpu_scan_shards.py runs the engine).  A scan of SHARD_TILES tiles or more hands rows and token slots out through ALLOC_SHARDS
# sub-allocators whose sizes come from what the context's previous sharded scan needed (c3r_lib.hip, scan_fused: hint_rows / hint_toks);
# the numbers below are that code's constants.
SPAN, SHARD_TILES, ALLOC_SHARDS = 224, 4096, 16
FRESH_ROWS, FRESH_TOKS = 4096, 131072           # per shard, a context that has made no sharded scan yet
PRIMED_ROWS, PRIMED_TOKS = 64, 2048             # per shard, after a sharded scan that found nothing: 1.25 x 0 + 64 rows / 2048 token slots
DENSE_END, SHARD_END = 917247, 917248           # ctg_end of a scan from 1 with 4095 / 4096 tiles
SHARD_REF_LEN = 1920000                         # the reference slice of every case: the reads lie in its first 918 kb, the rest is `A`
PRIME_REGION = (1000001, 1000001 + 917300)      # 4096 tiles or more and no read: a scan of it leaves the hints at PRIMED_ROWS / PRIMED_TOKS


def scan_tiles(regions):
    """The tiles of a scan of `regions` ((ctg_start, ctg_end) pairs): every region with its 33-position halo, in spans of 224."""
    return sum(-(-(b + 33 - (max(1, a - 33) - 1)) // SPAN) for a, b in regions)


def edge_regions(n_last):
    """64 adjacent regions: 63 of 64 tiles and a last one of n_last."""
    regs = [(100 + 14270 * k, 100 + 14270 * k + 14269) for k in range(64)]
    a, _b = regs[-1]
    regs[-1] = (a, a + 14269 - SPAN * (64 - n_last))
    return regs


def padded_reference(parts):
    """SHARD_REF_LEN bases: `A` everywhere but on the (0-based offset, bases) parts."""
    buf = bytearray(b"A" * SHARD_REF_LEN)
    for off, s in parts:
        buf[off:off + len(s)] = s.encode()
    return buf.decode()


_burst_cache = {}


def burst_case(channels, offset, seed=77, iupac=False):
    """(ref, ReadSet): synth.small_case(seed, 9 kb, 3 genes, depth 30, reads of ~500) moved `offset` positions into the padded reference
    — with snp_min_af = 0 and min_coverage = 2 more than 1200 candidates within 9 kb (about 41 spans, 130 reads).  iupac: one read shows an
    `M` on a covered column (30 channels: the ordered recompute, which a context builds its tables for only after meeting such a column)."""
    from clair3_rna_amd import synth
    from clair3_rna_amd.reads import ReadSet
    key = (channels, seed)
    if key not in _burst_cache:
        _burst_cache[key] = synth.small_case(seed=seed, ref_len=9000, n_genes=3, depth=30, mean_len=500, phased=(channels == 30),
                                             platform="hifi" if channels == 30 else "ont")[:2]
    ref, rs = _burst_cache[key]
    if iupac:
        seq = rs.seq.copy()
        r = rs.reads[len(rs.reads) // 2]
        q = 0                                                       # a query position well inside the read's first long match
        for c in rs.cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]:
            op, ln = int(c) & 15, int(c) >> 4
            if op in (0, 7, 8) and ln >= 12:
                q += 6
                break
            if op in (0, 1, 4, 7, 8):
                q += ln
        byte, hi = int(r["seq_off"]) + q // 2, q % 2 == 0
        seq[byte] = ((3 << 4) | (seq[byte] & 15)) if hi else ((seq[byte] & 0xf0) | 3)       # 'M' (A or C) there
        rs = ReadSet(rs.reads, rs.cigar, seq)
    return padded_reference([(offset, ref)]), shift_readset(rs, offset)


DEEP_PILE_RLEN, DEEP_PILE_COLS = 60, 28         # reads of 60 M: two records each; the 28 columns that have 16 covered positions on either side


def deep_piles(depth, n_piles, offset, pitch=1000, seed=5):
    """(ref, ReadSet, records): n_piles piles `pitch` apart, each `depth` reads `60M` on one position, nine in ten with a substitution on
    each of the pile's 28 central columns (the only ones with a whole window), alternating strands.  Default gates: 28 candidates per pile
    and 0.9 x depth tokens per candidate; a span holds at most one pile, 2 x depth records.
    Two piles, not three: a regrowth sizes the shards by the fullest one of the attempt that failed, and the scan gives up after two, so k
    equally heavy spans that happen to land 1, then 2, then 3 in one shard would end it with an error; with two the third attempt fits
    wherever they land."""
    from clair3_rna_amd.reads import ReadSet
    ref = random_reference(n_piles * pitch + 200, seed)
    recs = []
    for k in range(n_piles):
        p0 = 100 + k * pitch
        alt = _with_subs(ref, p0, DEEP_PILE_RLEN, range(p0 + 16, p0 + 16 + DEEP_PILE_COLS))
        recs += [dict(pos=offset + p0, cigar="%dM" % DEEP_PILE_RLEN, seq=ref[p0:p0 + DEEP_PILE_RLEN] if i % 10 == 9 else alt, flag=16 * (i % 2), hp=i % 3)
                 for i in range(depth)]
    return padded_reference([(offset, ref)]), ReadSet.from_records(recs), recs


WIDE_RLEN, WIDE_DEPTH, WIDE_AT = 500, 6200, 224 * 1000 - 16      # (its first candidate column is the first position of a span)


def wide_pile(seed=9):
    """(ref, ReadSet): WIDE_DEPTH reads `500M` on one position, nine in ten with a substitution on each of the 468 columns that have a whole
    window — 2.6 M tokens, more than the 16 x 131072 slots of a context that has made no sharded scan, in spans of 224, 224 and 20 candidates
    (the first of them alone is more than a fresh shard holds, and 1.25 x the two large ones hold all three: the third attempt always fits)."""
    from clair3_rna_amd.reads import ReadSet
    ref = random_reference(WIDE_RLEN + 100, seed)
    alt = _with_subs(ref, 0, WIDE_RLEN, range(16, WIDE_RLEN - 16))
    recs = [dict(pos=WIDE_AT, cigar="%dM" % WIDE_RLEN, seq=ref[:WIDE_RLEN] if i % 10 == 9 else alt, flag=16 * (i % 2), hp=i % 3) for i in range(WIDE_DEPTH)]
    return padded_reference([(WIDE_AT, ref)]), ReadSet.from_records(recs)


def oracle_regions(rs, ref, regions, channels=18, **pk):
    """The oracle's result for a scan of several regions: dict(lines, X) of the regions one after the other."""
    parts = [oracle_chunk(rs, ref, 1, a, b, channels=channels, **pk) for a, b in regions]
    return dict(lines=[l for p in parts for l in p["lines"]], X=np.concatenate([p["X"].reshape(-1, 33, channels) for p in parts]),
                rows=[r for p in parts for r in p["rows"]], depth=np.concatenate([np.asarray(p["depth"]).reshape(-1) for p in parts]))


def alt_tokens(lines):
    """A lower bound of the tokens behind the lines: the counts of their alt_info fields (`<depth>-<allele> <count> ...`) without the
    reference's (`R<base>`) — every such count is one read's token; reads inside a deletion have tokens that alt_info does not count."""
    n = 0
    for l in lines:
        f = l.split("\t")[4].split("-", 1)[1].split()
        n += sum(int(v) for k, v in zip(f[0::2], f[1::2]) if not k.startswith("R"))
    return n


def max_span_candidates(lines, ctg_start=1):
    """The most candidates that one span of a scan from ctg_start holds: a span is one workgroup's and takes its rows from one shard."""
    first = max(1, ctg_start - 33)
    return int(np.bincount([(p - first) // SPAN for p in line_positions(lines)]).max())


BURST_AT, BURST_AT2, PILES_AT = 400000, 123457, 600000            # offsets of the inputs in the padded reference (0-based)
BURST_KW = dict(snp_min_af=0.0, min_coverage=2)


def shard_case(name, channels=18):
    """The inputs of tests/test_gpu_scan_shards.py by name -> dict(ref, rs, kw: engine parameters, okw: the oracle's).
    burst / burst2: burst_case at BURST_AT / BURST_AT2; burst_iupac: with the IUPAC base; piles_tile / piles_deep: deep_piles of 2 x 1000 and
    2 x 2600 reads (2000 and 5200 records in a span: k_fused_tiles' and k_fused_deep's at the natural thresholds); batch: the burst at 20000
    and piles_deep at PILES_AT in one read set, gates of the burst; wide: wide_pile."""
    okw = dict(channels=channels)
    kw = dict(channels=channels)
    if name.startswith("burst"):
        ref, rs = burst_case(channels, BURST_AT2 if name == "burst2" else BURST_AT, iupac=(name == "burst_iupac"))
    elif name == "piles_tile":
        ref, rs, _ = deep_piles(1000, 2, PILES_AT)
    elif name == "piles_deep":
        ref, rs, _ = deep_piles(2600, 2, PILES_AT)
    elif name == "wide":
        ref, rs = wide_pile()
    elif name == "batch":
        ref_b, rs_b = burst_case(channels, 20000)
        ref_p, rs_p, _ = deep_piles(2600, 2, PILES_AT)
        ref = padded_reference([(20000, ref_b[20000:29000]), (PILES_AT, ref_p[PILES_AT:PILES_AT + 2200])])
        rs = merge_readsets(rs_b, rs_p)
    else:
        raise KeyError(name)
    if name.startswith("burst") or name == "batch":
        kw.update(BURST_KW)
        okw.update(snp_af=0.0, min_coverage=2)
    return dict(ref=ref, rs=rs, kw=kw, okw=okw)


# the batch of tests/test_gpu_scan_shards.py on shard_case("batch"): (region, kind) in scan order — `prime` scans find nothing and leave the
# hints at their floor, so that the sharded scan behind each must grow and repeat
BATCH_SCANS = [((20001, 23000), "dense"), (PRIME_REGION, "prime"), ((1, SHARD_END), "sharded"), ((23000, 29500), "dense"), (PRIME_REGION, "prime"),
               ((30001, 30001 + 917300), "sharded"), ((PILES_AT, PILES_AT + 600), "dense")]
