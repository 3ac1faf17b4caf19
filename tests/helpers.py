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
