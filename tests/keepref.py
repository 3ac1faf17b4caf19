"""The rule of k_row_keep (csrc/pileup_kernels.hpp) in numpy float32: which candidates can print a row when the decoder runs without show_ref.
A site is dropped when its probabilities take the decoder's early RefCall exit (clair3_rna/call_variants.py:540-542: P(0/0) >= 0.5 and
P(gt21 = ref ref) >= 0.5) or when no class product exceeds P(0/0) * P(ref ref) in the first round of its arg-max (decode.call_site:
`top == p_ref`) and that product is at least 1e-30 (a normal float32: the kernel keeps what it cannot compare safely).  One float32
multiply per product, as decode.call_site and decode.hpp make them.  tests/c/row_export_check.hip holds the same rule in C++; the case
families below are that program's, with IUPAC centres only (decode.call_site raises on any other letter)."""
import numpy as np

IUPAC2ACGT = dict(zip("ACGTURYSWKMBDHVN", "ACGTTACCAGACAAAA"))
REF_CLASS = {"A": 0, "C": 4, "G": 7, "T": 9}                        # gt21 index of AA, CC, GG, TT
Z1_CLASSES = [0, 4, 7, 9, 15, 10]                                   # homozygous: AA CC GG TT InsIns DelDel
Z2_CLASSES = [1, 2, 3, 5, 6, 8, 15, 10, 16, 17, 18, 19, 11, 12, 13, 14, 20]
SLOTS = [(1, g) for g in Z1_CLASSES] + [(2, g) for g in Z2_CLASSES]  # the 23 competing class products


def keep(probs, centres):
    """probs [n][24] (21 gt21 + 3 zygosity), centres: n IUPAC letters -> bool [n], True = the site leaves the device"""
    p = np.ascontiguousarray(probs, dtype=np.float32).reshape(-1, 24)
    rr = np.array([REF_CLASS[IUPAC2ACGT[c]] for c in centres], dtype=np.int64)
    assert len(rr) == len(p)
    z0, z1, z2 = p[:, 21], p[:, 22], p[:, 23]
    g_rr = p[np.arange(len(p)), rr]
    early = (z0 >= np.float32(0.5)) & (g_rr >= np.float32(0.5))
    p_ref = z0 * g_rr
    prods = np.concatenate([z1[:, None] * p[:, Z1_CLASSES], z2[:, None] * p[:, Z2_CLASSES]], axis=1)
    assert p_ref.dtype == np.float32 and prods.dtype == np.float32 and prods.shape[1] == 23
    top = prods.max(axis=1) if len(p) else np.zeros(0, np.float32)
    return ~(early | ((p_ref >= np.float32(1e-30)) & (p_ref >= top)))


def edge_cases():
    """-> (centres, probs [n][24], expected keep [n]): every IUPAC centre, z0 and g[rr] around 0.5, each of the 23 class products one ulp
    below / at / one ulp above P(ref ref), P(ref ref) around 1e-30, at zero and denormal.  Built from exactly representable values."""
    f32, homo = np.float32, [0, 4, 7, 9]
    C, P, E = [], [], []

    def add(c, expect, **kv):
        p = np.zeros(24, np.float32)
        for k, v in kv.items():
            p[int(k[1:])] = v
        C.append(c); P.append(p); E.append(bool(expect))
    for c in "ACGTURYSWKMBDHVN":
        rr = REF_CLASS[IUPAC2ACGT[c]]
        for h in homo:
            add(c, h != rr, **dict({"p%d" % o: 0.0625 for o in homo if o != h}, **{"p%d" % h: 0.75, "p21": 0.75, "p22": 0.25}))
    half = [np.nextafter(f32(0.5), f32(0)), f32(0.5), np.nextafter(f32(0.5), f32(1))]
    for ci, c in enumerate("ACGT"):
        rr, other = homo[ci], homo[(ci + 1) & 3]
        for a in range(3):
            for b in range(3):
                add(c, False, p21=half[a], **{"p%d" % rr: half[b]})
                add(c, not (a >= 1 and b >= 1), p21=half[a], p22=0.5, **{"p%d" % rr: half[b], "p%d" % other: 0.75})
    zk = [np.nextafter(f32(0.375), f32(0)), f32(0.375), np.nextafter(f32(0.375), f32(1))]
    for ci, c in enumerate("ACGT"):
        rr = homo[ci]
        for z, g in SLOTS:
            for rel in range(3):
                if z == 1 and g == rr:
                    add(c, rel == 2, p21=0.375, p22=zk[rel], **{"p%d" % rr: 0.5})
                else:
                    add(c, rel == 2, p21=0.75, **{"p%d" % rr: 0.25, "p%d" % g: 0.5, "p%d" % (21 + z): zk[rel]})
    tiny = [np.nextafter(f32(1e-30), f32(0)), f32(1e-30), np.nextafter(f32(1e-30), f32(1)), f32(0), f32(1e-40)]
    for t in tiny:
        for above in (False, True):
            for ci, c in enumerate("ACGT"):
                rr, other = homo[ci], homo[(ci + 2) & 3]
                add(c, above or t < f32(1e-30), p21=t, p22=(0.25 if above else t * f32(0.5)), **{"p%d" % rr: 1.0, "p%d" % other: 1.0})
    return C, np.stack(P), np.array(E)


def softmax_cases(n, seed=20240607):
    """n seeded softmax vectors at three sharpnesses, every other one leaning towards the centre's own class and 0/0 as a model's output does"""
    rng = np.random.RandomState(seed)
    letters = "ACGTURYSWKMBDHVN"
    centres = [letters[rng.randint(4)] if rng.randint(4) else letters[rng.randint(16)] for _ in range(n)]
    sharp = np.array([1.0, 4.0, 16.0])[np.arange(n) % 3][:, None]
    lg, lz = rng.normal(size=(n, 21)) * sharp, rng.normal(size=(n, 3)) * sharp
    lean = np.arange(n) % 2 == 0
    rr = np.array([REF_CLASS[IUPAC2ACGT[c]] for c in centres])
    lg[np.arange(n)[lean], rr[lean]] += 1.2 * sharp[lean, 0]
    lz[lean, 0] += 1.2 * sharp[lean, 0]
    sm = lambda l: (np.exp(l - l.max(1, keepdims=True)) / np.exp(l - l.max(1, keepdims=True)).sum(1, keepdims=True))
    return centres, np.concatenate([sm(lg), sm(lz)], axis=1).astype(np.float32)


ALT_INFOS = ["30-", "30-XC 7 XG 3 XT 2 XA 4 RA 14", "30-IAC 5 IACG 3 DC 4 DCG 2 RA 16", "27-XA 3 XC 3 XG 3 XT 3 IAT 3 IATT 3 DC 3 DCG 3 RA 3"]
