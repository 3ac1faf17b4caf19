"""ctypes binding of libc3r.so (include/c3r.h).  There is no CPU fallback: if the HIP library is
missing or no MI355X is visible, construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

from .reads import READ_DTYPE, ReadSet

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("C3R_LIB") or os.path.join(HERE, "libc3r.so")        # C3R_LIB: A/B builds of the kernels (development)

SITE_DTYPE = np.dtype([("pos", "<i4"), ("depth", "<i4"), ("ref33", "S36"), ("n_tok", "<i4"), ("tok_off", "<u4")], align=True)
TOKEN_DTYPE = np.dtype([("read_idx", "<u4"), ("indel", "<i4"), ("qpos", "<u4"), ("base", "u1"), ("rev", "u1"), ("del_after", "<u2")],
                       align=True)
PADINS_DTYPE = np.dtype([("read_idx", "<u4"), ("qpos", "<u4"), ("n_bases", "<u4"), ("total", "<u4"), ("pad_mask", "<u8")], align=True)
# c3r_phase_site_t: one phased heterozygous SNV (phasedvcf.read_phase_sites); ref / alt are BAM 4-bit base codes (A 1, C 2, G 4, T 8)
PHASE_SITE_DTYPE = np.dtype([("pos", "<i4"), ("ps", "<i4"), ("ref", "u1"), ("alt", "u1"), ("h1", "u1"), ("reserved", "u1")], align=True)
# c3r_hap_site_t: one heterozygous call with its two alleles (phasing.allele_candidates_from_vcf): per allele the anchor base's code, the
# event behind it (HAP_EV_*), its length and, for an insertion, the offset of its bases in the pool of inserted bases
HAP_EV_NONE, HAP_EV_INS, HAP_EV_DEL = 0, 1, 2
HAP_SITE_DTYPE = np.dtype([("pos", "<i4"), ("ps", "<i4"), ("base_matters", "u1"), ("event_matters", "u1"), ("reserved", "u1", (6,)),
                           ("a_base", "u1"), ("a_kind", "u1"), ("a_len", "<u2"), ("a_ins_off", "<u4"),
                           ("b_base", "u1"), ("b_kind", "u1"), ("b_len", "<u2"), ("b_ins_off", "<u4")], align=True)
# c3r_hap_region_t: one interval of c3r_hap_region_counts (0-based, half-open; strand 0 none, 1 +, 2 -) and where its rows start
HAP_REGION_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4"), ("row_off", "<i4"), ("strand", "u1"), ("reserved", "u1", (3,))], align=True)
HAP_REGION_MAX_BACK = 4096
assert HAP_REGION_DTYPE.itemsize == 16
# c3r_hap_interval_t: one interval of c3r_hap_group_counts (0-based, half-open; strand 0 none, 1 +, 2 -) and the group it belongs to
HAP_INTERVAL_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4"), ("group", "<i4"), ("strand", "u1"), ("reserved", "u1", (3,))], align=True)
assert HAP_INTERVAL_DTYPE.itemsize == 16
# c3r_hap_junction_t / c3r_hap_junction_row_t: one splice junction of c3r_hap_junction_counts (0-based, half-open; its rows are
# rows[row_off : the next junction's row_off]) and one phase set of a junction
HAP_JUNCTION_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4"), ("reads", "<u4"), ("reverse", "<u4"), ("untagged", "<u4"), ("row_off", "<i4")], align=True)
HAP_JUNCTION_ROW_DTYPE = np.dtype([("ps", "<i4"), ("hp1", "<u4"), ("hp2", "<u4")], align=True)
assert HAP_JUNCTION_DTYPE.itemsize == 24 and HAP_JUNCTION_ROW_DTYPE.itemsize == 12
assert SITE_DTYPE.itemsize == 52 and TOKEN_DTYPE.itemsize == 16 and PADINS_DTYPE.itemsize == 24 and PHASE_SITE_DTYPE.itemsize == 12
assert HAP_SITE_DTYPE.itemsize == 32 and HAP_SITE_DTYPE.fields["a_base"][1] == 16 and HAP_SITE_DTYPE.fields["b_ins_off"][1] == 28

C3R_ERRORS = {-1: "EINVAL", -2: "ENODEVICE", -3: "EHIP", -4: "ENOMEM", -5: "EUNSUPPORTED", -6: "EOVERFLOW"}


class Params(C.Structure):
    _fields_ = [("channels", C.c_int32), ("min_mq", C.c_int32), ("excl_flags", C.c_int32), ("min_coverage", C.c_int32),
                ("snp_min_af", C.c_double), ("indel_min_af", C.c_double), ("head_tail", C.c_int32),
                ("splice_padding", C.c_int32), ("genotyping_mode", C.c_int32), ("max_depth_rescale", C.c_int32),
                ("max_depth", C.c_int32), ("mpileup_compat", C.c_int32)]


class HaplotagStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_reads", "n_hp1", "n_hp2", "n_no_vote", "n_tie", "n_votes")]


PHASE_LINKS = 8                                              # C3R_PHASE_LINKS (include/c3r_types.h): predecessors every site is linked to


class PhaseParams(C.Structure):
    _fields_ = [("min_reads", C.c_int32), ("min_agree_pct", C.c_int32)]


class PhaseStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_sites", "n_phased", "n_blocks", "max_block")]


class HapAssignStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_sites", "n_phased", "n_few_reads", "n_disagree")]


class LeftAlignStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_in", "n_out", "n_moved", "n_not_left_alignable", "n_same_pos_after_left_align")]


class C3RError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libc3r: %s (%s)" % (msg, C3R_ERRORS.get(code, code)))
        self.code = code


EXPORTS = ["c3r_version", "c3r_create", "c3r_destroy", "c3r_trim", "c3r_last_error", "c3r_synchronize", "c3r_stream",
           "c3r_default_params", "c3r_set_params", "c3r_load_reads", "c3r_host_alloc", "c3r_host_free", "c3r_set_reference", "c3r_set_reference_view", "c3r_set_bed", "c3r_set_sites",
           "c3r_pileup_scan", "c3r_pileup_scan_regions", "c3r_batch_begin", "c3r_batch_end", "c3r_batch_count", "c3r_get_tensors", "c3r_get_sites", "c3r_token_count", "c3r_get_tokens", "c3r_get_pad_insertions", "c3r_get_columns",
           "c3r_weight_count", "c3r_load_weights", "c3r_set_precision", "c3r_get_precision", "c3r_get_precision_guard", "c3r_reserve", "c3r_infer", "c3r_get_probs", "c3r_call_rows", "c3r_get_rows", "c3r_rows_begin", "c3r_rows_begin_ex", "c3r_rows_decode", "c3r_rows_get", "c3r_rows_info", "c3r_rows_free", "c3r_decode_text", "c3r_set_profiling", "c3r_reset_kernel_stats",
           "c3r_get_kernel_stats", "c3r_get_scan_counts", "c3r_set_phase_sites", "c3r_get_haplotags", "c3r_phase_links", "c3r_phase_resolve",
           "c3r_phase_unit_links", "c3r_phase_merge", "c3r_get_read_phase_sets", "c3r_hap_counts", "c3r_hap_assign", "c3r_hap_region_counts",
           "c3r_hap_allele_counts", "c3r_set_phase_alleles", "c3r_phase_allele_links", "c3r_phase_allele_unit_links",
           "c3r_set_hap_left_align", "c3r_hap_left_align_sites",
           "c3r_load_reads_q", "c3r_set_hap_min_bq", "c3r_get_hap_min_bq", "c3r_get_hap_seq",
           "c3r_set_hap_realign", "c3r_get_hap_realign", "c3r_hap_realign_column",
           "c3r_set_hap_realign_spliced", "c3r_get_hap_realign_spliced", "c3r_hap_realign_column_spliced",
           "c3r_set_hap_bq_weights", "c3r_get_hap_bq_weights", "c3r_get_haplotag_weights", "c3r_get_haplotag_words",
           "c3r_hap_junction_counts", "c3r_get_hap_junctions", "c3r_set_hap_junction_direct",
           "c3r_hap_group_counts", "c3r_set_hap_group_direct", "c3r_get_hap_group_direct"]

_lib = None


def load_library():
    """dlopen libc3r.so and declare prototypes.  Raises ImportError when the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libc3r.so not found at %s — run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.c3r_version.restype = C.c_char_p
    L.c3r_create.argtypes = [i32, vp, C.POINTER(vp)]
    L.c3r_destroy.argtypes = [vp]
    L.c3r_destroy.restype = None
    L.c3r_trim.argtypes = []
    L.c3r_trim.restype = C.c_int64
    L.c3r_last_error.argtypes = [vp]
    L.c3r_last_error.restype = C.c_char_p
    L.c3r_synchronize.argtypes = [vp]
    L.c3r_stream.argtypes = [vp]
    L.c3r_stream.restype = vp
    L.c3r_default_params.argtypes = [C.POINTER(Params)]
    L.c3r_default_params.restype = None
    L.c3r_set_params.argtypes = [vp, C.POINTER(Params)]
    L.c3r_load_reads.argtypes = [vp, vp, i64, vp, i64, vp, i64]
    L.c3r_load_reads_q.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64]
    L.c3r_set_hap_min_bq.argtypes = [vp, i32]
    L.c3r_get_hap_min_bq.argtypes = [vp, C.POINTER(i32), C.POINTER(i64)]
    L.c3r_get_hap_seq.argtypes = [vp, vp, i64]
    L.c3r_set_hap_bq_weights.argtypes = [vp, i32]
    L.c3r_get_hap_bq_weights.argtypes = [vp, C.POINTER(i32)]
    L.c3r_get_haplotag_weights.argtypes = [vp, vp, i64]
    L.c3r_get_haplotag_words.argtypes = [vp, vp, i64]
    L.c3r_host_alloc.argtypes = [C.c_size_t]
    L.c3r_host_alloc.restype = vp
    L.c3r_host_free.argtypes = [vp]
    L.c3r_host_free.restype = None
    L.c3r_set_reference.argtypes = [vp, i64, vp, i64]
    L.c3r_set_reference_view.argtypes = [vp, i64, vp, i64]
    L.c3r_set_bed.argtypes = [vp, i32, vp, i64]
    L.c3r_set_sites.argtypes = [vp, vp, i64]
    L.c3r_set_phase_sites.argtypes = [vp, vp, i64]
    L.c3r_get_haplotags.argtypes = [vp, vp, i64, C.POINTER(HaplotagStats)]
    L.c3r_phase_links.argtypes = [vp, vp, i64, vp]
    L.c3r_phase_resolve.argtypes = [vp, i64, vp, C.POINTER(PhaseParams), vp, C.POINTER(PhaseStats)]
    L.c3r_phase_unit_links.argtypes = [vp, vp, i64, vp, i64, C.POINTER(i64)]
    L.c3r_phase_merge.argtypes = [vp, i64, vp, i64, C.POINTER(PhaseParams), vp, C.POINTER(PhaseStats), C.POINTER(i64)]
    L.c3r_get_read_phase_sets.argtypes = [vp, vp, i64]
    L.c3r_hap_counts.argtypes = [vp, vp, i64, vp]
    L.c3r_hap_allele_counts.argtypes = [vp, vp, i64, vp, i64, vp]
    L.c3r_hap_region_counts.argtypes = [vp, vp, i64, vp, i64, C.c_int32, vp, vp]
    L.c3r_hap_junction_counts.argtypes = [vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.c3r_get_hap_junctions.argtypes = [vp, vp, i64, vp, i64]
    L.c3r_set_hap_junction_direct.argtypes = [vp, i32]
    L.c3r_hap_group_counts.argtypes = [vp, vp, i64, i64, vp, vp, i64, C.c_int32, vp, vp]
    L.c3r_set_hap_group_direct.argtypes = [vp, i32]
    L.c3r_get_hap_group_direct.argtypes = [vp, C.POINTER(i32)]
    L.c3r_phase_allele_links.argtypes = [vp, vp, i64, vp, i64, vp]
    L.c3r_phase_allele_unit_links.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, C.POINTER(i64)]
    L.c3r_set_phase_alleles.argtypes = [vp, vp, vp, i64, vp, i64]
    L.c3r_hap_assign.argtypes = [vp, i64, vp, C.POINTER(PhaseParams), vp, C.POINTER(HapAssignStats)]
    L.c3r_set_hap_left_align.argtypes = [vp, i32]
    L.c3r_set_hap_realign.argtypes = [vp, i32]
    L.c3r_get_hap_realign.argtypes = [vp, C.POINTER(i32)]
    L.c3r_hap_realign_column.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.c3r_set_hap_realign_spliced.argtypes = [vp, i32]
    L.c3r_get_hap_realign_spliced.argtypes = [vp, C.POINTER(i32)]
    L.c3r_hap_realign_column_spliced.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.c3r_hap_left_align_sites.argtypes = [vp, i64, vp, i64, i64, vp, i64, vp, vp, i64, C.POINTER(i64), vp, C.POINTER(i64), C.POINTER(LeftAlignStats)]
    L.c3r_pileup_scan.argtypes = [vp, i64, i64, C.POINTER(i64)]
    L.c3r_pileup_scan_regions.argtypes = [vp, C.c_int32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.c3r_batch_begin.argtypes = [vp]
    L.c3r_batch_end.argtypes = [vp]
    L.c3r_batch_count.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.c3r_get_tensors.argtypes = [vp, i32, vp, i64]
    L.c3r_get_sites.argtypes = [vp, vp, i64]
    L.c3r_token_count.argtypes = [vp, C.POINTER(i64)]
    L.c3r_get_tokens.argtypes = [vp, vp, i64]
    L.c3r_get_pad_insertions.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.c3r_get_columns.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), vp, vp, vp, i64]
    L.c3r_weight_count.argtypes = [i32]
    L.c3r_weight_count.restype = i64
    L.c3r_load_weights.argtypes = [vp, vp, i64, i32]
    L.c3r_set_precision.argtypes = [vp, i32]
    L.c3r_get_precision.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double)]
    L.c3r_get_precision_guard.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(i32)]
    L.c3r_infer.argtypes = [vp, vp, i64, vp]
    L.c3r_reserve.argtypes = [vp, i64]
    L.c3r_get_probs.argtypes = [vp, vp, i64]
    L.c3r_call_rows.argtypes = [vp, C.c_char_p, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    L.c3r_get_rows.argtypes = [vp, vp, i64]
    L.c3r_rows_begin.argtypes = [vp, C.POINTER(vp)]
    L.c3r_rows_begin_ex.argtypes = [vp, i32, vp, vp, C.POINTER(vp)]
    L.c3r_rows_decode.argtypes = [vp, C.c_char_p, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    L.c3r_rows_get.argtypes = [vp, vp, i64]
    L.c3r_rows_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.c3r_rows_free.argtypes = [vp]
    L.c3r_rows_free.restype = None
    L.c3r_decode_text.argtypes = [C.c_char_p, i64, vp, vp, i32, C.POINTER(C.c_char_p), vp, i32, i32, vp, i64, C.POINTER(i64)]
    L.c3r_set_profiling.argtypes = [vp, i32]
    L.c3r_reset_kernel_stats.argtypes = [vp]
    L.c3r_get_kernel_stats.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(i64), i32, C.POINTER(i32)]
    L.c3r_get_scan_counts.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    _lib = L
    return L


PRECISIONS = {"f32": 0, "f16x3": 1, "f16+f8": 2, "auto": 3}          # c3r_set_precision modes


def env_precision(default="f16x3"):
    """The C3R_PRECISION environment default of the drivers' --gpu_precision flag, validated like the flag itself (argparse does
    not run `choices` on defaults)."""
    v = os.environ.get("C3R_PRECISION", default)
    if v not in PRECISIONS:
        raise SystemExit("C3R_PRECISION=%r: must be one of %s" % (v, ", ".join(sorted(PRECISIONS))))
    return v


CTG_END_MAX = 2147482590          # C3R_CTG_END_MAX (include/c3r.h, "coordinates"): the last ctg_end a scan accepts


def default_params():
    p = Params()
    load_library().c3r_default_params(C.byref(p))
    return p


def pinned_copy(a):
    """A copy of numpy array `a` in page-locked host memory (c3r_host_alloc): uploads from it are asynchronous DMA transfers.
    The block is freed when the last array that views it is collected."""
    import weakref
    a = np.ascontiguousarray(a)
    L = load_library()
    nbytes = max(1, a.nbytes)
    p = L.c3r_host_alloc(nbytes)
    if not p:
        raise MemoryError("c3r_host_alloc(%d) failed" % nbytes)
    flat = np.frombuffer((C.c_char * nbytes).from_address(p), dtype=np.uint8)      # every later view keeps `flat` alive as its base
    weakref.finalize(flat, L.c3r_host_free, p)
    out = flat[:a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def pinned_readset(rs):
    """ReadSet with its arrays — the qualities too, when it carries them — in page-locked memory."""
    out = ReadSet.__new__(ReadSet)
    out.reads, out.cigar, out.seq = pinned_copy(rs.reads), pinned_copy(rs.cigar), pinned_copy(rs.seq)
    if getattr(rs, "qual", None) is not None:
        out.qual = pinned_copy(rs.qual)
    return out


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def trim():
    """Give the device blocks libc3r.so keeps between contexts back to the driver (c3r_trim); returns the bytes released."""
    return int(load_library().c3r_trim())


class Engine(object):
    """One GPU context: tensor build (A1-A5) + network forward (A6/A7) on one MI355X."""

    def __init__(self, device=0, stream=None):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.c3r_create(device, stream, C.byref(h))
        if rc != 0:
            raise C3RError(rc, "c3r_create(device=%d) failed: no usable MI355X/HIP device (no CPU fallback)" % device)
        self.h = h
        self.params = default_params()
        self.n_candidates = 0
        self._keep = []
        import weakref
        self._snaps = weakref.WeakSet()          # row snapshots must be released before the context goes

    def close(self):
        if getattr(self, "h", None):
            for sn in list(getattr(self, "_snaps", ())):
                sn.free()
            self.L.c3r_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise C3RError(rc, self.L.c3r_last_error(self.h).decode())

    # ---- configuration / inputs
    def set_params(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise KeyError(k)
            setattr(self.params, k, v)
        self._chk(self.L.c3r_set_params(self.h, C.byref(self.params)))

    def load_reads(self, rs):
        assert isinstance(rs, ReadSet)
        self.readset = rs
        if getattr(rs, "qual", None) is not None:        # (the base qualities go along: c3r_load_reads_q, for set_hap_min_bq)
            self._chk(self.L.c3r_load_reads_q(self.h, _ptr(rs.reads), len(rs.reads), _ptr(rs.cigar), len(rs.cigar), _ptr(rs.seq), len(rs.seq),
                                              _ptr(rs.qual), len(rs.qual)))
            return
        self._chk(self.L.c3r_load_reads(self.h, _ptr(rs.reads), len(rs.reads), _ptr(rs.cigar), len(rs.cigar), _ptr(rs.seq), len(rs.seq)))

    def set_reference(self, ref_start, seq, upper_view=False):
        """seq: str, bytes, or a uint8 array (bamio.fasta_fetch) — an array is handed over by pointer, no copy on this side.
        upper_view: the array is upper-cased already and is used in place (c3r_set_reference_view); this object and the row
        snapshots taken from it keep the array alive for as long as the library reads it."""
        if isinstance(seq, np.ndarray):
            b = np.ascontiguousarray(seq, dtype=np.uint8)
            self.ref_start, self._ref_bytes, self._ref_upper = ref_start, b, None
            self._chk((self.L.c3r_set_reference_view if upper_view else self.L.c3r_set_reference)(self.h, ref_start, b.ctypes.data, b.size))
            return
        b = seq.encode() if isinstance(seq, str) else (seq if isinstance(seq, bytes) else bytes(seq))
        self.ref_start, self._ref_bytes, self._ref_upper = ref_start, b, None
        self._chk(self.L.c3r_set_reference(self.h, ref_start, C.cast(C.c_char_p(b), C.c_void_p), len(b)))

    @property
    def ref_seq(self):
        """Upper-cased reference slice as str (debug dumps only: 40 ms per 64 MB contig, so built on demand)."""
        if self._ref_upper is None:
            self._ref_upper = bytes(self._ref_bytes).decode().upper()
        return self._ref_upper

    def set_bed(self, which, intervals):
        a = np.ascontiguousarray(np.asarray(intervals if intervals is not None else [], dtype=np.int32).reshape(-1, 2))
        self._chk(self.L.c3r_set_bed(self.h, which, _ptr(a), len(a)))

    def set_sites(self, sites):
        a = np.ascontiguousarray(np.asarray(sites, dtype=np.int32))
        self._chk(self.L.c3r_set_sites(self.h, _ptr(a), len(a)))

    def set_phase_sites(self, sites):
        """The contig's phased heterozygous SNVs (a PHASE_SITE_DTYPE array sorted by pos, phasedvcf.read_phase_sites): from now on
        load_reads haplotags every read on the device and the 30-channel build uses those tags instead of the records' own hp.  None or
        an empty array clears the table.  Reads that are already loaded are tagged at once."""
        a = np.zeros(0, PHASE_SITE_DTYPE) if sites is None else np.asarray(sites)
        if a.dtype != PHASE_SITE_DTYPE:
            raise TypeError("phase sites must be a capi.PHASE_SITE_DTYPE array, got %r" % (a.dtype,))
        a = np.ascontiguousarray(a)
        self._chk(self.L.c3r_set_phase_sites(self.h, _ptr(a), len(a)))

    def set_phase_alleles(self, sites, h1, pool=None, pool_bases=None):
        """set_phase_sites for a table that may hold phased insertions, deletions and two-ALT sites beside the SNVs (c3r_set_phase_alleles;
        phasedvcf.read_phase_alleles): `sites` a HAP_SITE_DTYPE array sorted by pos with ps >= 0, `h1` a uint8 array of the same length — 0:
        allele A on haplotype 1 (GT 0|1, 1|2), 1: allele B (GT 1|0, 2|1) —, `pool` the packed pool of the insertions' bases (pack_nibbles;
        None when no allele is an insertion) and `pool_bases` the number of bases in it (None: two per byte).  It replaces the table of
        set_phase_sites, and that call replaces this one's; None or an empty array clears the table.  Reads that are already loaded are
        tagged at once."""
        a = np.zeros(0, HAP_SITE_DTYPE) if sites is None else np.asarray(sites)
        if a.dtype != HAP_SITE_DTYPE:
            raise TypeError("sites must be a capi.HAP_SITE_DTYPE array, got %r" % (a.dtype,))
        a = np.ascontiguousarray(a)
        h = np.zeros(0, np.uint8) if h1 is None else np.ascontiguousarray(h1)
        if h.dtype != np.uint8 or h.shape != (len(a),):
            raise TypeError("h1 must be a uint8 array with one entry per site")
        pl = np.zeros(0, np.uint8) if pool is None else np.ascontiguousarray(pool)
        if pl.dtype != np.uint8 or pl.ndim != 1:
            raise TypeError("pool must be a one-dimensional uint8 array of packed bases (capi.pack_nibbles)")
        nb = 2 * len(pl) if pool_bases is None else int(pool_bases)
        if nb < 0 or (nb + 1) // 2 > len(pl):
            raise ValueError("pool_bases = %d does not fit a pool of %d bytes" % (nb, len(pl)))
        self._chk(self.L.c3r_set_phase_alleles(self.h, _ptr(a), _ptr(h) if len(h) else None, len(a), _ptr(pl) if nb else None, nb))

    def set_hap_left_align(self, on):
        """The opt-in switch of --left_align_indels (c3r_set_hap_left_align, default off): while on, hap_allele_counts, phase_allele_links,
        phase_allele_unit_links and the tagging of set_phase_alleles / load_reads bring each read's insertion or deletion to its left-most
        place inside its M run before they compare it with the table — which the caller normalises with hap_left_align_sites — and need a
        reference (set_reference) that covers the loaded reads.  With an allele table set and reads loaded the reads are tagged again."""
        self._chk(self.L.c3r_set_hap_left_align(self.h, 1 if on else 0))

    def set_hap_realign(self, overhang):
        """The opt-in switch of --hap_realign (c3r_set_hap_realign, overhang 0 .. 16, default 0 = off): while above 0, hap_allele_counts,
        phase_allele_links, phase_allele_unit_links and the tagging of set_phase_alleles / load_reads compare each read's window of
        `overhang` reference bases around a site with the site's two haplotypes (the rule `realign` of include/c3r.h) where the read can be
        realigned there, and need a reference (set_reference).  It excludes set_hap_left_align.  With an allele table set and reads loaded
        the reads are tagged again."""
        self._chk(self.L.c3r_set_hap_realign(self.h, int(overhang)))

    def hap_realign(self):
        """The overhang of set_hap_realign (c3r_get_hap_realign; 0: off)."""
        w = C.c_int32(0)
        self._chk(self.L.c3r_get_hap_realign(self.h, C.byref(w)))
        return int(w.value)

    def set_hap_realign_spliced(self, on):
        """The opt-in switch of --hap_realign_spliced (c3r_set_hap_realign_spliced, default off): while it is on AND set_hap_realign is
        above 0, a read's window is counted in the read's own spliced positions and so crosses an N op (the rule `realign_spliced` of
        include/c3r.h).  It may be set at any time; with the overhang above 0, an allele table set and reads loaded the reads are tagged
        again."""
        self._chk(self.L.c3r_set_hap_realign_spliced(self.h, 1 if on is True else 0 if on is False else int(on)))

    def hap_realign_spliced(self):
        """The value of set_hap_realign_spliced (c3r_get_hap_realign_spliced)."""
        on = C.c_int32(0)
        self._chk(self.L.c3r_get_hap_realign_spliced(self.h, C.byref(on)))
        return bool(on.value)

    def set_hap_min_bq(self, q):
        """The opt-in threshold of --hap_min_bq (c3r_set_hap_min_bq, 0 .. 93, default 0 = off): while above 0, every call that holds the
        loaded reads against a site table — the tagging of set_phase_sites / set_phase_alleles / load_reads, hap_counts, hap_allele_counts,
        phase_links, phase_unit_links and their allele forms — reads a base whose quality is below q as N (a base without a quality, 0xff,
        never).  Needs reads loaded with qualities (a ReadSet with `qual`); valid before or after load_reads with the same result; with a
        phase table set and reads loaded the reads are tagged again.  A threshold, not quality weights (set_hap_bq_weights are those)."""
        self._chk(self.L.c3r_set_hap_min_bq(self.h, int(q)))

    def hap_min_bq(self):
        """(q, n_masked): the threshold and the number of bases of the loaded reads that it masks (c3r_get_hap_min_bq)."""
        q, n = C.c_int(), C.c_int64()
        self._chk(self.L.c3r_get_hap_min_bq(self.h, C.byref(q), C.byref(n)))
        return int(q.value), int(n.value)

    def set_hap_bq_weights(self, on):
        """The opt-in switch of --hap_bq_weights (c3r_set_hap_bq_weights, default off): while on, the tagging of set_phase_sites /
        set_phase_alleles / load_reads weighs every vote by the quality of the read's base on the site (the rule `bq_weights` of
        include/c3r.h; a base without a quality, 0xff, weighs 1) where it otherwise counts 1.  The count tables and the links do not look
        at it.  Needs reads loaded with qualities (a ReadSet with `qual`); valid before or after load_reads with the same result; with a
        phase table set and reads loaded the reads are tagged again."""
        self._chk(self.L.c3r_set_hap_bq_weights(self.h, 1 if on else 0))

    def hap_bq_weights(self):
        """The switch of set_hap_bq_weights (c3r_get_hap_bq_weights)."""
        on = C.c_int(0)
        self._chk(self.L.c3r_get_hap_bq_weights(self.h, C.byref(on)))
        return bool(on.value)

    def haplotag_weights(self):
        """uint32 (n, 2): (w1, w2), the weight sums of the phase set every loaded read's tag was decided in, in load order; a tie's pair
        where the tag is 0, (0, 0) for a read without an observation (c3r_get_haplotag_weights).  An error while no phase sites are set
        or set_hap_bq_weights is off."""
        st = HaplotagStats()
        self._chk(self.L.c3r_get_haplotags(self.h, None, 0, C.byref(st)))
        w = np.zeros((st.n_reads, 2), dtype=np.uint32)
        self._chk(self.L.c3r_get_haplotag_weights(self.h, _ptr(w) if len(w) else None, len(w)))
        return w

    def haplotag_words(self):
        """uint32[n]: the tag word of every loaded read, in load order: tag | observations on all phase sets << 2 (c3r_get_haplotag_words).
        An error while no phase sites are set."""
        st = HaplotagStats()
        self._chk(self.L.c3r_get_haplotags(self.h, None, 0, C.byref(st)))
        w = np.zeros(st.n_reads, dtype=np.uint32)
        self._chk(self.L.c3r_get_haplotag_words(self.h, _ptr(w) if len(w) else None, len(w)))
        return w

    def hap_seq(self):
        """uint8[n_seq_bytes]: the packed bases that the site-table kernels read — the masked copy, or with q = 0 the loaded sequence
        (c3r_get_hap_seq)."""
        n = len(self.readset.seq) if getattr(self, "readset", None) is not None else 0
        out = np.zeros(n, np.uint8)
        self._chk(self.L.c3r_get_hap_seq(self.h, _ptr(out) if n else None, n))
        return out

    @staticmethod
    def hap_left_align_sites(sites, pool, ref_start, ref, pool_bases=None):
        """capi.hap_left_align_sites (host only: no device is touched)."""
        return hap_left_align_sites(sites, pool, ref_start, ref, pool_bases)

    def haplotags(self):
        """(uint8[n] tags of the loaded reads in load order, dict(n_reads, n_hp1, n_hp2, n_no_vote, n_tie, n_votes)); an error while no
        phase sites are set."""
        st = HaplotagStats()
        self._chk(self.L.c3r_get_haplotags(self.h, None, 0, C.byref(st)))
        hp = np.zeros(st.n_reads, dtype=np.uint8)
        self._chk(self.L.c3r_get_haplotags(self.h, _ptr(hp), len(hp), C.byref(st)))
        return hp, {k: int(getattr(st, k)) for k, _ in HaplotagStats._fields_}

    def read_phase_sets(self):
        """int32[n]: the phase set every loaded read's tag was decided in, in load order; -1 where the tag is 0 (c3r_get_read_phase_sets).  An
        error while no phase sites are set."""
        st = HaplotagStats()
        self._chk(self.L.c3r_get_haplotags(self.h, None, 0, C.byref(st)))
        ps = np.zeros(st.n_reads, dtype=np.int32)
        self._chk(self.L.c3r_get_read_phase_sets(self.h, _ptr(ps), len(ps)))
        return ps

    def hap_counts(self, sites):
        """uint32 (n, 3, 3): at every query site (a PHASE_SITE_DTYPE array sorted by pos; ps = the phase set to count against, h1 is ignored)
        the loaded reads that pass the current filters, by row — 0: the read is untagged, tied or tagged in another set, 1 / 2: its haplotype —
        and by column — REF, ALT, another base (c3r_hap_counts).  Needs a table (set_phase_sites).  Leaves the reads' haplotags, the table and
        every scan as they are."""
        a = _phase_site_array(sites)
        counts = np.zeros((len(a), 3, 3), dtype=np.uint32)
        self._chk(self.L.c3r_hap_counts(self.h, _ptr(a), len(a), _ptr(counts)))
        return counts

    def hap_region_counts(self, regions, row_ps, stranded=0):
        """(region_counts uint32 (n, 2), row_counts uint32 (n_rows, 2)): the loaded reads that pass the current filters, per interval of
        `regions` (a HAP_REGION_DTYPE array sorted by (start, end); region j's rows are row_ps[row_off[j] : row_off[j + 1]], phase-set numbers
        strictly increasing inside a region) — region_counts: untagged reads, reads tagged in a set that is none of the region's rows;
        row_counts: haplotype 1, haplotype 2 of the row's set (c3r_hap_region_counts, the rule `hap_regions`).  A read counts once in every
        region that one of its M / = / X / D ops overlaps.  stranded: 0 off, 1 same, 2 reverse.  Needs a phase table; leaves tags, table
        and scans as they are."""
        a = np.zeros(0, HAP_REGION_DTYPE) if regions is None else np.asarray(regions)
        if a.dtype != HAP_REGION_DTYPE:
            raise TypeError("regions must be a capi.HAP_REGION_DTYPE array, got %r" % (a.dtype,))
        a = np.ascontiguousarray(a)
        ps = np.ascontiguousarray(np.zeros(0, np.int32) if row_ps is None else row_ps, dtype=np.int32)
        if ps.ndim != 1:
            raise TypeError("row_ps must be one-dimensional")
        region_counts, row_counts = np.zeros((len(a), 2), dtype=np.uint32), np.zeros((len(ps), 2), dtype=np.uint32)
        self._chk(self.L.c3r_hap_region_counts(self.h, _ptr(a) if len(a) else None, len(a), _ptr(ps) if len(ps) else None, len(ps), int(stranded),
                                               _ptr(region_counts) if len(a) else None, _ptr(row_counts) if len(ps) else None))
        return region_counts, row_counts

    def hap_group_counts(self, intervals, n_groups, group_row_off, row_ps, stranded=0):
        """(group_counts uint32 (n_groups, 2), row_counts uint32 (n_rows, 2)): the loaded reads that pass the current filters, per GROUP of
        `intervals` (a HAP_INTERVAL_DTYPE array sorted by (start, end); the intervals of one group disjoint and of one strand; group g's rows
        are row_ps[group_row_off[g] : group_row_off[g + 1]], the last group's end at len(row_ps), phase-set numbers strictly increasing inside
        a group) — group_counts: untagged reads, reads tagged in a set that is none of the group's rows; row_counts: haplotype 1, haplotype 2
        of the row's set (c3r_hap_group_counts, the rule `hap_groups`).  A read counts once in every group of which it covers a position of
        an interval, however many intervals: the gene-level count, a gene being the group of its exons.  stranded: 0 off, 1 same, 2 reverse.
        Needs a phase table; leaves tags, table and scans as they are."""
        a = np.zeros(0, HAP_INTERVAL_DTYPE) if intervals is None else np.asarray(intervals)
        if a.dtype != HAP_INTERVAL_DTYPE:
            raise TypeError("intervals must be a capi.HAP_INTERVAL_DTYPE array, got %r" % (a.dtype,))
        a = np.ascontiguousarray(a)
        off = np.ascontiguousarray(np.zeros(0, np.int32) if group_row_off is None else group_row_off, dtype=np.int32)
        ps = np.ascontiguousarray(np.zeros(0, np.int32) if row_ps is None else row_ps, dtype=np.int32)
        n_groups = int(n_groups)
        if off.ndim != 1 or ps.ndim != 1 or n_groups < 0 or len(off) != n_groups:
            raise TypeError("group_row_off must be one-dimensional with one entry per group, row_ps one-dimensional")
        group_counts, row_counts = np.zeros((n_groups, 2), dtype=np.uint32), np.zeros((len(ps), 2), dtype=np.uint32)
        self._chk(self.L.c3r_hap_group_counts(self.h, _ptr(a) if len(a) else None, len(a), n_groups, _ptr(off) if n_groups else None,
                                              _ptr(ps) if len(ps) else None, len(ps), int(stranded),
                                              _ptr(group_counts) if n_groups else None, _ptr(row_counts) if len(ps) else None))
        return group_counts, row_counts

    def set_hap_group_direct(self, on):
        """c3r_set_hap_group_direct (default off): hap_group_counts runs its kernel without the per-workgroup LDS stage.  Same result."""
        self._chk(self.L.c3r_set_hap_group_direct(self.h, 1 if on else 0))

    def hap_group_direct(self):
        """c3r_get_hap_group_direct: whether hap_group_counts runs without its LDS stage."""
        on = C.c_int(0)
        self._chk(self.L.c3r_get_hap_group_direct(self.h, C.byref(on)))
        return bool(on.value)

    def hap_junction_counts(self, slots_hint=0):
        """(junctions, rows): every splice junction that a loaded read which passes the current filters holds — an N op [start, end) of its
        normalised CIGAR — as a HAP_JUNCTION_DTYPE array sorted by (start, end) with reads / reverse / untagged, and per junction and phase set
        in which one of its reads was tagged a HAP_JUNCTION_ROW_DTYPE row (ps, hp1, hp2), junction j's rows at rows[row_off[j] :
        row_off[j + 1]] in ps order (c3r_hap_junction_counts, the rule `hap_junctions`).  No phase table: every read is untagged and there
        are no rows.  slots_hint: the initial size of the device's hash tables (0: the library's default); the result does not depend on
        it.  Leaves tags, table and scans as they are."""
        nj, nr = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.c3r_hap_junction_counts(self.h, int(slots_hint), C.byref(nj), C.byref(nr)))
        junctions, rows = np.zeros(nj.value, dtype=HAP_JUNCTION_DTYPE), np.zeros(nr.value, dtype=HAP_JUNCTION_ROW_DTYPE)
        self._chk(self.L.c3r_get_hap_junctions(self.h, _ptr(junctions) if len(junctions) else None, len(junctions), _ptr(rows) if len(rows) else None, len(rows)))
        return junctions, rows

    def set_hap_junction_direct(self, on):
        """c3r_set_hap_junction_direct (default off): hap_junction_counts runs its kernel without the per-workgroup LDS stage.  Same
        result; a switch for measurements."""
        self._chk(self.L.c3r_set_hap_junction_direct(self.h, 1 if on else 0))

    def hap_allele_counts(self, sites, ins_pool=None):
        """uint32 (n, 3, 3) like hap_counts, for query sites whose two alleles may be SNVs, insertions or deletions (a HAP_SITE_DTYPE array
        sorted by pos; `ins_pool`: the packed pool of the insertions' bases, uint8 with two codes to a byte as a read's SEQ has them —
        pack_nibbles — or None when no allele is an insertion): columns — allele A, allele B, anything else (c3r_hap_allele_counts).  Needs a
        table; leaves tags, table and scans as they are."""
        a = np.zeros(0, HAP_SITE_DTYPE) if sites is None else np.asarray(sites)
        if a.dtype != HAP_SITE_DTYPE:
            raise TypeError("sites must be a capi.HAP_SITE_DTYPE array, got %r" % (a.dtype,))
        a = np.ascontiguousarray(a)
        pool = np.zeros(0, np.uint8) if ins_pool is None else np.ascontiguousarray(ins_pool)
        if pool.dtype != np.uint8 or pool.ndim != 1:
            raise TypeError("ins_pool must be a one-dimensional uint8 array of packed bases (capi.pack_nibbles)")
        counts = np.zeros((len(a), 3, 3), dtype=np.uint32)
        self._chk(self.L.c3r_hap_allele_counts(self.h, _ptr(a), len(a), _ptr(pool) if len(pool) else None, 2 * len(pool), _ptr(counts)))
        return counts

    def phase_links(self, sites):
        """uint32 (n, PHASE_LINKS, 2) cis / trans counts between every candidate site (a PHASE_SITE_DTYPE array sorted by pos; ps and h1 are
        ignored) and the PHASE_LINKS sites before it in the table, from the loaded reads that pass the current filters
        (c3r_phase_links).  Leaves the reads' haplotags, the table of set_phase_sites and every scan as they are."""
        a = _phase_site_array(sites)
        links = np.zeros((len(a), PHASE_LINKS, 2), dtype=np.uint32)
        self._chk(self.L.c3r_phase_links(self.h, _ptr(a), len(a), _ptr(links)))
        return links

    def phase_unit_links(self, sites):
        """uint32 (U, PHASE_LINKS, 2) same / different haplotype counts between every unit of a chain's table (a PHASE_SITE_DTYPE array as
        phase_resolve leaves it: ps = -1 or >= 1, h1; the units are its distinct ps >= 0 in increasing order) and the PHASE_LINKS units
        before it, from the loaded reads that pass the current filters (c3r_phase_unit_links, the block-merge stage of include/c3r.h).
        Leaves the reads' haplotags, the table of set_phase_sites and every scan as they are."""
        a = _phase_site_array(sites)
        ulinks = np.zeros((len(a), PHASE_LINKS, 2), dtype=np.uint32)          # (U <= n)
        u = C.c_int64(0)
        self._chk(self.L.c3r_phase_unit_links(self.h, _ptr(a), len(a), _ptr(ulinks), len(a), C.byref(u)))
        return np.ascontiguousarray(ulinks[:u.value])

    def phase_sites(self, sites, min_reads=2, min_agree_pct=75, merge_levels=0):
        """phase_links, then the greedy chain of phase_resolve: (PHASE_SITE_DTYPE array with ps / h1 filled in — ps = -1: the site stays
        unphased, drop it before set_phase_sites —, dict(n_sites, n_phased, n_blocks, max_block)).  merge_levels > 0: then up to that many
        levels of the block-merge stage (phase_unit_links + phase_merge), ending early at a level that joins nothing; the dict then also
        holds merge_levels_run and merge_units_joined.  merge_levels = 0 calls nothing of it."""
        if int(merge_levels) < 0:
            raise ValueError("merge_levels must be >= 0, got %r" % (merge_levels,))
        a = _phase_site_array(sites)
        out, st = phase_resolve(a, self.phase_links(a), min_reads, min_agree_pct)
        if int(merge_levels) == 0:
            return out, st
        levels = joined = 0
        while levels < int(merge_levels):
            out, st, n = phase_merge(out, self.phase_unit_links(out), min_reads, min_agree_pct)
            levels += 1
            joined += n
            if n == 0:
                break
        st["merge_levels_run"], st["merge_units_joined"] = levels, joined
        return out, st

    def phase_allele_links(self, sites, pool=None, pool_bases=None):
        """phase_links over a table that may hold insertions, deletions and two-ALT sites beside the SNVs (c3r_phase_allele_links): `sites` a
        HAP_SITE_DTYPE array sorted by pos (ps is ignored), `pool` the packed pool of the insertions' bases (pack_nibbles; None when no allele
        is an insertion), `pool_bases` the number of bases in it (None: two per byte).  uint32 (n, PHASE_LINKS, 2) cis / trans by allele
        index (A 0, B 1).  Needs no table; leaves tags, a table that is set and every scan as they are."""
        a, pl, nb = _hap_site_array(sites), *_pool_args(pool, pool_bases)
        links = np.zeros((len(a), PHASE_LINKS, 2), dtype=np.uint32)
        self._chk(self.L.c3r_phase_allele_links(self.h, _ptr(a), len(a), _ptr(pl) if nb else None, nb, _ptr(links)))
        return links

    def phase_allele_unit_links(self, sites, h1, pool=None, pool_bases=None):
        """phase_unit_links over the allele table (c3r_phase_allele_unit_links): `sites` with ps = -1 or >= 1 as the chain leaves it, `h1` a
        uint8 array of the same length (0: allele A lies on haplotype 1).  uint32 (U, PHASE_LINKS, 2)."""
        a, pl, nb = _hap_site_array(sites), *_pool_args(pool, pool_bases)
        h = np.zeros(0, np.uint8) if h1 is None else np.ascontiguousarray(h1)
        if h.dtype != np.uint8 or h.shape != (len(a),):
            raise TypeError("h1 must be a uint8 array with one entry per site")
        ulinks = np.zeros((len(a), PHASE_LINKS, 2), dtype=np.uint32)          # (U <= n)
        u = C.c_int64(0)
        self._chk(self.L.c3r_phase_allele_unit_links(self.h, _ptr(a), _ptr(h) if len(h) else None, len(a), _ptr(pl) if nb else None, nb,
                                                     _ptr(ulinks), len(a), C.byref(u)))
        return np.ascontiguousarray(ulinks[:u.value])

    def phase_allele_sites(self, sites, pool=None, min_reads=2, min_agree_pct=75, merge_levels=0, pool_bases=None):
        """phase_sites over the allele table: phase_allele_links, the greedy chain of phase_resolve on the pseudo-table of the sites (pos, ps,
        h1: all the rule reads), then up to merge_levels levels of phase_allele_unit_links + phase_merge.  -> (int32 ps per site, -1: the
        site stays unphased; uint8 h1 per site, 0: allele A lies on haplotype 1; the statistics dict of phase_sites)."""
        if int(merge_levels) < 0:
            raise ValueError("merge_levels must be >= 0, got %r" % (merge_levels,))
        a = _hap_site_array(sites)
        out, st = phase_resolve(hap_site_keys(a), self.phase_allele_links(a, pool, pool_bases), min_reads, min_agree_pct)
        if int(merge_levels) > 0:
            levels = joined = 0
            while levels < int(merge_levels):
                t = a.copy()
                t["ps"] = out["ps"]
                out, st, n = phase_merge(out, self.phase_allele_unit_links(t, np.ascontiguousarray(out["h1"]), pool, pool_bases), min_reads, min_agree_pct)
                levels += 1
                joined += n
                if n == 0:
                    break
            st["merge_levels_run"], st["merge_units_joined"] = levels, joined
        return np.ascontiguousarray(out["ps"]), np.ascontiguousarray(out["h1"]), st

    # ---- tensor build
    def scan(self, ctg_start, ctg_end):
        n = C.c_int64(0)
        self._chk(self.L.c3r_pileup_scan(self.h, ctg_start, ctg_end, C.byref(n)))
        tot = C.c_int64(0)
        self._chk(self.L.c3r_batch_count(self.h, C.byref(tot), None))
        self.n_candidates = tot.value          # resident candidates (== n outside batch mode)
        return n.value

    def scan_regions(self, regions):
        """All (ctg_start, ctg_end) regions — e.g. the chunks of a contig — in one set of launches; same candidates, in
        the same order, as successive scan() calls in batch mode."""
        starts = np.ascontiguousarray([r[0] for r in regions], dtype=np.int64)
        ends = np.ascontiguousarray([r[1] for r in regions], dtype=np.int64)
        n = C.c_int64(0)
        self._chk(self.L.c3r_pileup_scan_regions(self.h, len(starts), starts.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 ends.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n)))
        tot = C.c_int64(0)
        self._chk(self.L.c3r_batch_count(self.h, C.byref(tot), None))
        self.n_candidates = tot.value
        return n.value

    def scan_counts(self):
        """dict(listed, deep, giant, slices): the spans of the last scan and the kernels that built them (c3r_get_scan_counts) — listed spans,
        those left to k_fused_deep, the giant ones among them and the slices listed for k_deep_walk.  Zeros after a column-store scan."""
        v = [C.c_int32(0) for _ in range(4)]
        self._chk(self.L.c3r_get_scan_counts(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("listed", "deep", "giant", "slices"), (x.value for x in v)))

    def begin_batch(self):
        """Scans append to the device-resident batch until end_batch(); infer() then covers all of them."""
        self._chk(self.L.c3r_batch_begin(self.h))
        self.n_candidates = 0

    def end_batch(self):
        self._chk(self.L.c3r_batch_end(self.h))

    def tensors(self, rescaled=True):
        n, Cc = self.n_candidates, self.params.channels
        out = np.zeros((n, 33, Cc), dtype=np.int32)
        if n:
            self._chk(self.L.c3r_get_tensors(self.h, int(rescaled), _ptr(out), n))
        return out

    def sites(self):
        out = np.zeros(self.n_candidates, dtype=SITE_DTYPE)
        if self.n_candidates:
            self._chk(self.L.c3r_get_sites(self.h, _ptr(out), len(out)))
        return out

    def tokens(self):
        n = C.c_int64(0)
        self._chk(self.L.c3r_token_count(self.h, C.byref(n)))
        out = np.zeros(n.value, dtype=TOKEN_DTYPE)
        if n.value:
            self._chk(self.L.c3r_get_tokens(self.h, _ptr(out), len(out)))
        return out

    def pad_insertions(self):
        """mpileup_compat = 1: the loaded reads' insertions that hold pads (PADINS_DTYPE; empty for aligner-made CIGARs) —
        altinfo.format_lines needs them beside the tokens to print `+3T*T` alleles."""
        n = C.c_int64(0)
        self._chk(self.L.c3r_get_pad_insertions(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=PADINS_DTYPE)
        if n.value:
            self._chk(self.L.c3r_get_pad_insertions(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    def columns(self):
        rs, n = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.c3r_get_columns(self.h, C.byref(rs), C.byref(n), None, None, None, 0))
        Cc = self.params.channels
        cols = np.zeros((n.value, Cc), dtype=np.int32)
        depth = np.zeros(n.value, dtype=np.int32)
        flags = np.zeros(n.value, dtype=np.uint8)
        self._chk(self.L.c3r_get_columns(self.h, C.byref(rs), C.byref(n), _ptr(cols), _ptr(depth), _ptr(flags), n.value))
        return dict(region_start=rs.value, cols=cols, depth=depth, flags=flags)

    # ---- network
    def load_weights(self, blob, channels=None):
        channels = channels or self.params.channels
        w = np.ascontiguousarray(blob, dtype=np.float32)
        self._chk(self.L.c3r_load_weights(self.h, _ptr(w), w.size, channels))

    PRECISIONS = PRECISIONS

    def set_precision(self, mode):
        """'f32' (fp32 MFMA), 'f16x3' (split-f16, fp32-equivalent; default), 'f16+f8' (f16 main term + fp8 corrections, opt-in) or
        'auto' ('f16+f8' where a calibration run through the loaded weights agrees with 'f16x3' to 4e-5, else 'f16x3')."""
        self._chk(self.L.c3r_set_precision(self.h, self.PRECISIONS[mode]))

    def precision(self):
        """(mode in use, calibration max |dP| or -1.0)."""
        m, e = C.c_int32(0), C.c_double(-1.0)
        self._chk(self.L.c3r_get_precision(self.h, C.byref(m), C.byref(e)))
        return {v: k for k, v in self.PRECISIONS.items()}[m.value], e.value

    def precision_guard(self):
        """dict(f16_err = max |dP| of split-f16 against the fp32 MFMA path on the calibration windows (-1 before weights are loaded),
        scale_log2 = the power-of-two scales of LSTM 1 / LSTM 2 / L4, fell_back = the guard sent the request to the fp32 path)."""
        e, sc, fb = C.c_double(-1.0), (C.c_int32 * 3)(), C.c_int32(0)
        self._chk(self.L.c3r_get_precision_guard(self.h, C.byref(e), sc, C.byref(fb)))
        return dict(f16_err=e.value, scale_log2=[int(v) for v in sc], fell_back=bool(fb.value))

    def infer(self, tensors=None, n=None, fetch=True):
        if tensors is None:
            n = self.n_candidates if n is None else n
            x = None
        else:
            x = np.ascontiguousarray(tensors, dtype=np.int32)
            n = x.shape[0]
        probs = np.zeros((n, 24), dtype=np.float32) if fetch else None
        self._chk(self.L.c3r_infer(self.h, _ptr(x), n, _ptr(probs)))
        return probs

    def fetch_probs(self, n):
        """Probabilities of the last infer(fetch=False): waits for the context's stream, then copies [n][24]."""
        probs = np.zeros((n, 24), dtype=np.float32)
        self._chk(self.L.c3r_get_probs(self.h, _ptr(probs), n))
        return probs

    def call_rows_text(self, ctg, qual=2, show_ref=True):
        """A8 on host threads (C++): the VCF rows of the resident candidates as ONE bytes object (newline-terminated rows),
        ready to be appended to the chunk's VCF; returns (text, n_rows).  After infer()."""
        n, nr = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.c3r_call_rows(self.h, ctg.encode(), -1 if qual is None else int(qual), int(show_ref), C.byref(n), C.byref(nr)))
        buf = C.create_string_buffer(n.value + 1)
        self._chk(self.L.c3r_get_rows(self.h, buf, n.value + 1))
        return buf.raw[:n.value], nr.value

    def reserve(self, n_sites):
        """Size the network's device buffers for batches of up to n_sites candidates now rather than in the first infer()."""
        self._chk(self.L.c3r_reserve(self.h, int(n_sites)))

    def rows_begin(self, drop_ref_calls=False, host_reads=True):
        """Detach the decode inputs of the resident batch (sites, tokens, probabilities, read bases; after infer()) into a host
        snapshot: the engine is free for the next contig, RowSnapshot.decode() may run on any thread.
        drop_ref_calls: only the sites that can print a row WITHOUT show_ref leave the device (the decoder's early RefCall exit is applied
        there; decode such a snapshot with show_ref=False only).  host_reads: the decoder reads inserted bases from the ReadSet handed to
        load_reads (kept alive by the snapshot) instead of from a copy fetched back from the device."""
        h = C.c_void_p()
        rs = getattr(self, "readset", None) if host_reads else None
        if rs is not None and not (rs.reads.flags.c_contiguous and rs.seq.flags.c_contiguous and rs.reads.dtype == READ_DTYPE and len(rs.reads)):
            rs = None
        self._chk(self.L.c3r_rows_begin_ex(self.h, int(bool(drop_ref_calls)), _ptr(rs.reads) if rs is not None else None,
                                           _ptr(rs.seq) if rs is not None else None, C.byref(h)))
        snap = RowSnapshot(self.L, h)
        snap._ref_keep = getattr(self, "_ref_bytes", None)       # (c3r_set_reference_view: the decoder reads this array)
        snap._rs_keep = rs                                       # (c3r_rows_begin_ex: and these)
        snap.dropped_ref_calls = bool(drop_ref_calls)
        self._snaps.add(snap)
        return snap

    def call_rows(self, ctg, qual=2, show_ref=True):
        """The same as a list of row strings (tests; 200 k Python strings cost more than producing the rows)."""
        text, _ = self.call_rows_text(ctg, qual, show_ref)
        return text.decode().split("\n")[:-1] if text else []

    # ---- measurement
    def synchronize(self):
        self._chk(self.L.c3r_synchronize(self.h))

    def stream(self):
        return self.L.c3r_stream(self.h)

    def set_profiling(self, on):
        self._chk(self.L.c3r_set_profiling(self.h, int(on)))

    def reset_kernel_stats(self):
        self._chk(self.L.c3r_reset_kernel_stats(self.h))

    def kernel_stats(self):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        cnt = (C.c_int64 * cap)()
        n = C.c_int(0)
        self._chk(self.L.c3r_get_kernel_stats(self.h, names, ms, cnt, cap, C.byref(n)))
        return {names[i].decode(): dict(total_ms=ms[i], launches=cnt[i]) for i in range(min(n.value, cap))}


def pack_nibbles(codes):
    """4-bit codes, one per element -> uint8 array with two to a byte, the first in the high nibble, as a read's SEQ is packed (an odd
    number: the last low nibble is 0)."""
    c = np.zeros(0, np.uint8) if codes is None else np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1)
    if len(c) and int(c.max()) > 15:
        raise ValueError("4-bit codes must be 0 .. 15")
    padded = np.concatenate([c, np.zeros(len(c) % 2, np.uint8)])
    return np.ascontiguousarray((padded[0::2] << 4) | padded[1::2])


def hap_sites_from_snvs(sites):
    """PHASE_SITE_DTYPE query sites (c3r_hap_counts) -> the same query as a HAP_SITE_DTYPE array (c3r_hap_allele_counts): allele A = (ref, no
    event), allele B = (alt, no event), the base matters and events do not."""
    a = _phase_site_array(sites)
    out = np.zeros(len(a), dtype=HAP_SITE_DTYPE)
    out["pos"], out["ps"], out["base_matters"], out["a_base"], out["b_base"] = a["pos"], a["ps"], 1, a["ref"], a["alt"]
    return out


def hap_site_keys(sites):
    """HAP_SITE_DTYPE array -> PHASE_SITE_DTYPE array with its pos and ps and placeholder bases (A, C): what hap_assign takes — its rule
    reads the counts, pos and ps only, with allele A in the place of REF and allele B in the place of ALT."""
    out = np.zeros(len(sites), dtype=PHASE_SITE_DTYPE)
    out["pos"], out["ps"], out["ref"], out["alt"] = sites["pos"], sites["ps"], 1, 2
    return out


def _hap_site_array(sites):
    a = np.zeros(0, HAP_SITE_DTYPE) if sites is None else np.asarray(sites)
    if a.dtype != HAP_SITE_DTYPE:
        raise TypeError("sites must be a capi.HAP_SITE_DTYPE array, got %r" % (a.dtype,))
    return np.ascontiguousarray(a)


def _pool_args(pool, pool_bases):
    """(the packed pool as a contiguous uint8 array, the number of bases in it): pool_bases None means two per byte."""
    pl = np.zeros(0, np.uint8) if pool is None else np.ascontiguousarray(pool)
    if pl.dtype != np.uint8 or pl.ndim != 1:
        raise TypeError("pool must be a one-dimensional uint8 array of packed bases (capi.pack_nibbles)")
    nb = 2 * len(pl) if pool_bases is None else int(pool_bases)
    if nb < 0 or (nb + 1) // 2 > len(pl):
        raise ValueError("pool_bases = %d does not fit a pool of %d bytes" % (nb, len(pl)))
    return pl, nb


def _phase_site_array(sites):
    a = np.zeros(0, PHASE_SITE_DTYPE) if sites is None else np.asarray(sites)
    if a.dtype != PHASE_SITE_DTYPE:
        raise TypeError("sites must be a capi.PHASE_SITE_DTYPE array, got %r" % (a.dtype,))
    return np.ascontiguousarray(a)


def hap_left_align_sites(sites, pool, ref_start, ref, pool_bases=None):
    """The table half of the left-alignment rule of include/c3r.h on the host (c3r_hap_left_align_sites; no GPU, no engine): a
    HAP_SITE_DTYPE array (any order), its packed pool and a reference slice (`ref`: str / bytes / uint8 array whose first letter is 1-based
    `ref_start`) -> (the sites that stay, left-aligned and sorted by pos; their packed pool; its number of bases; int64 input index of
    every output site; dict(n_in, n_out, n_moved, n_not_left_alignable, n_same_pos_after_left_align))."""
    L = load_library()
    a = _hap_site_array(sites)
    pl, nb = _pool_args(pool, pool_bases)
    r = np.frombuffer(ref.encode() if isinstance(ref, str) else bytes(ref), dtype=np.uint8) if not isinstance(ref, np.ndarray) else np.ascontiguousarray(ref, dtype=np.uint8)
    cap = int(a["a_len"][a["a_kind"] == HAP_EV_INS].sum()) + int(a["b_len"][a["b_kind"] == HAP_EV_INS].sum())
    out, out_pool, src = np.zeros(len(a), dtype=HAP_SITE_DTYPE), np.zeros((cap + 1) // 2, dtype=np.uint8), np.zeros(len(a), dtype=np.int64)
    m, ob, st = C.c_int64(0), C.c_int64(0), LeftAlignStats()
    rc = L.c3r_hap_left_align_sites(_ptr(a), len(a), _ptr(pl) if nb else None, nb, int(ref_start), _ptr(r) if len(r) else None, len(r),
                                    _ptr(out), _ptr(out_pool) if cap else None, cap, C.byref(ob), _ptr(src), C.byref(m), C.byref(st))
    if rc != 0:
        raise C3RError(rc, "c3r_hap_left_align_sites: pos >= 1, flags 0 / 1, kinds 0 .. 2, an indel has a length and every insertion lies inside the pool")
    return (np.ascontiguousarray(out[:m.value]), np.ascontiguousarray(out_pool[:(ob.value + 1) // 2]), int(ob.value), np.ascontiguousarray(src[:m.value]),
            {k: int(getattr(st, k)) for k, _ in LeftAlignStats._fields_})


def hap_realign_column(site, pool, ref_start, ref, read, cigars, seq4, overhang, spliced=False):
    """The rule `realign` of include/c3r.h — with spliced=True the rule `realign_spliced` — for one read at one site on the host
    (c3r_hap_realign_column / c3r_hap_realign_column_spliced; no GPU, no engine): one
    HAP_SITE_DTYPE record, the packed pool, a reference slice (`ref`: str / bytes whose first letter is 1-based `ref_start`), one READ_DTYPE
    record and the uint32 CIGAR and packed sequence arrays its offsets index -> (column 0 / 1 / 2, or 3 for no observation; whether the
    read was realigned at the site)."""
    L = load_library()
    a = _hap_site_array(np.asarray(site).reshape(1))
    pl, nb = _pool_args(pool, None)
    r = np.frombuffer(ref.encode() if isinstance(ref, str) else bytes(ref), dtype=np.uint8)
    for k in "ab":                                            # (the C entry carries no pool length: checked here)
        if int(a[0][k + "_kind"]) == HAP_EV_INS and int(a[0][k + "_ins_off"]) + int(a[0][k + "_len"]) > nb:
            raise ValueError("allele %s: the insertion runs past the pool of %d bases" % (k.upper(), nb))
    rd = np.ascontiguousarray(np.asarray(read, dtype=READ_DTYPE).reshape(1))
    cg, sq = np.ascontiguousarray(cigars, dtype=np.uint32), np.ascontiguousarray(seq4, dtype=np.uint8)
    col, ra = C.c_int32(0), C.c_int32(0)
    where = (_ptr(a), _ptr(pl) if nb else None, int(ref_start), _ptr(r) if len(r) else None, len(r), _ptr(rd), _ptr(cg) if len(cg) else None, _ptr(sq) if len(sq) else None,
             int(overhang))
    rc = L.c3r_hap_realign_column_spliced(*where, 1, C.byref(col), C.byref(ra)) if spliced else L.c3r_hap_realign_column(*where, C.byref(col), C.byref(ra))
    if rc != 0:
        raise C3RError(rc, "c3r_hap_realign_column: overhang 0 .. 16, pos >= 1, kinds 0 .. 2, an indel has a length, and a CIGAR that a load accepts")
    return int(col.value), bool(ra.value)


def phase_resolve(sites, links, min_reads=2, min_agree_pct=75):
    """The resolution rule of include/c3r.h on the host (c3r_phase_resolve; no GPU, no engine): candidate sites and their (n, PHASE_LINKS, 2)
    link table -> (sites with ps / h1 filled in, ps = -1 for a site alone in its block; dict(n_sites, n_phased, n_blocks, max_block))."""
    L = load_library()
    a = _phase_site_array(sites)
    lk = np.ascontiguousarray(links, dtype=np.uint32)
    if lk.shape != (len(a), PHASE_LINKS, 2):
        raise ValueError("links must have shape (%d, %d, 2), got %r" % (len(a), PHASE_LINKS, lk.shape))
    out = np.zeros(len(a), dtype=PHASE_SITE_DTYPE)
    p, st = PhaseParams(int(min_reads), int(min_agree_pct)), PhaseStats()
    rc = L.c3r_phase_resolve(_ptr(a), len(a), _ptr(lk), C.byref(p), _ptr(out), C.byref(st))
    if rc != 0:
        raise C3RError(rc, "c3r_phase_resolve: sites must be sorted by strictly increasing pos, min_reads >= 0, 0 <= min_agree_pct <= 100")
    return out, {k: int(getattr(st, k)) for k, _ in PhaseStats._fields_}


def hap_assign(sites, counts, min_reads=2, min_agree_pct=75):
    """The assignment rule of include/c3r.h on the host (c3r_hap_assign; no GPU, no engine): query sites and their (n, 3, 3) count table
    (Engine.hap_counts) -> (sites with h1 filled in and ps kept where the haplotype-tagged reads agree, ps = -1 and h1 = 0 elsewhere;
    dict(n_sites, n_phased, n_few_reads, n_disagree))."""
    L = load_library()
    a = _phase_site_array(sites)
    ct = np.ascontiguousarray(counts, dtype=np.uint32)
    if ct.shape != (len(a), 3, 3):
        raise ValueError("counts must have shape (%d, 3, 3), got %r" % (len(a), ct.shape))
    out = np.zeros(len(a), dtype=PHASE_SITE_DTYPE)
    p, st = PhaseParams(int(min_reads), int(min_agree_pct)), HapAssignStats()
    rc = L.c3r_hap_assign(_ptr(a), len(a), _ptr(ct), C.byref(p), _ptr(out), C.byref(st))
    if rc != 0:
        raise C3RError(rc, "c3r_hap_assign: min_reads >= 0, 0 <= min_agree_pct <= 100")
    return out, {k: int(getattr(st, k)) for k, _ in HapAssignStats._fields_}


class RowSnapshot(object):
    """Host-side decode inputs of one batch (c3r_rows_begin); decode() needs no GPU and no engine."""

    def __init__(self, L, h):
        self.L, self.h, self._ref_keep, self._rs_keep, self.dropped_ref_calls = L, h, None, None, False

    def decode(self, ctg, qual=2, show_ref=True, as_array=False):
        """-> (bytes of newline-terminated VCF rows, number of rows); releases the snapshot.  as_array: the rows as a uint8 array
        instead (a large contig's rows are ~100 MB: turning them into a bytes object is a copy made with the GIL held, which
        stalls every other thread of a whole-sample run)."""
        if show_ref and self.dropped_ref_calls:
            raise ValueError("this snapshot was taken without the RefCall sites (rows_begin(drop_ref_calls=True)): decode it with show_ref=False")
        try:
            n, nr = C.c_int64(0), C.c_int64(0)
            rc = self.L.c3r_rows_decode(self.h, ctg.encode(), -1 if qual is None else int(qual), int(show_ref), C.byref(n), C.byref(nr))
            if rc != 0:
                raise C3RError(rc, "c3r_rows_decode failed")
            from . import bamio
            buf = bamio.huge_empty(n.value + 1, np.uint8)
            rc = self.L.c3r_rows_get(self.h, buf.ctypes.data, n.value + 1)
            if rc != 0:
                raise C3RError(rc, "c3r_rows_get failed")
            return (buf[:n.value] if as_array else buf[:n.value].tobytes()), nr.value
        finally:
            self.free()

    def info(self):
        """-> (sites, token bytes, indel records) that the snapshot brought off the device (c3r_rows_info)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = self.L.c3r_rows_info(self.h, C.byref(a), C.byref(b), C.byref(c))
        if rc != 0:
            raise C3RError(rc, "c3r_rows_info failed")
        return a.value, b.value, c.value

    def free(self):
        if self.h:
            self.L.c3r_rows_free(self.h)
            self.h = None
        self._ref_keep = None
        self._rs_keep = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def decode_text(ctg, positions, ref33_list, alt_info_list, probs, qual=2, show_ref=True):
    """The C++ decoder on caller-supplied text (no GPU needed): list of VCF rows."""
    L = load_library()
    n = len(positions)
    pos = np.ascontiguousarray(positions, dtype=np.int32)
    r33 = np.zeros((n, 36), dtype="S1")
    refs = np.frombuffer(b"".join(r.encode().ljust(36, b"\0") for r in ref33_list), dtype=np.uint8).copy() if n else np.zeros(0, np.uint8)
    alts = (C.c_char_p * max(n, 1))(*[a.encode() for a in alt_info_list])
    pr = np.ascontiguousarray(probs, dtype=np.float32)
    need = C.c_int64(0)
    rc = L.c3r_decode_text(ctg.encode(), n, _ptr(pos), _ptr(refs), 36, alts, _ptr(pr), -1 if qual is None else int(qual), int(show_ref), None, 0,
                           C.byref(need))
    buf = C.create_string_buffer(need.value + 1)
    rc = L.c3r_decode_text(ctg.encode(), n, _ptr(pos), _ptr(refs), 36, alts, _ptr(pr), -1 if qual is None else int(qual), int(show_ref), buf,
                           need.value + 1, C.byref(need))
    if rc != 0:
        raise C3RError(rc, "c3r_decode_text failed")
    text = buf.value.decode()
    return text.split("\n")[:-1] if text else []


def phase_merge(sites, ulinks, min_reads=2, min_agree_pct=75):
    """One level of the block-merge stage of include/c3r.h on the host (c3r_phase_merge; no GPU, no engine): a chain's table and the
    (U, PHASE_LINKS, 2) link table of its units -> (table with the joined units' ps / h1 rewritten, dict(n_sites, n_phased, n_blocks,
    max_block) of that table, number of units that joined)."""
    L = load_library()
    a = _phase_site_array(sites)
    lk = np.ascontiguousarray(ulinks, dtype=np.uint32)
    if lk.ndim != 3 or lk.shape[1:] != (PHASE_LINKS, 2):
        raise ValueError("ulinks must have shape (units, %d, 2), got %r" % (PHASE_LINKS, lk.shape))
    out = np.zeros(len(a), dtype=PHASE_SITE_DTYPE)
    p, st, joined = PhaseParams(int(min_reads), int(min_agree_pct)), PhaseStats(), C.c_int64(0)
    rc = L.c3r_phase_merge(_ptr(a), len(a), _ptr(lk), lk.shape[0], C.byref(p), _ptr(out), C.byref(st), C.byref(joined))
    if rc != 0:
        raise C3RError(rc, "c3r_phase_merge: sites must be sorted by strictly increasing pos with ps = -1 or >= 1 and h1 0 or 1, ulinks must "
                           "hold one row per distinct ps >= 0, min_reads >= 0, 0 <= min_agree_pct <= 100")
    return out, {k: int(getattr(st, k)) for k, _ in PhaseStats._fields_}, int(joined.value)
