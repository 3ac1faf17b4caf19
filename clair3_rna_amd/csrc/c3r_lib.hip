// c3r_lib.hip — host side of libc3r.so: the C-ABI of include/c3r.h over the gfx950 kernels.
// No CPU fallback: every compute entry point needs a HIP device.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <queue>
#include <chrono>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include <new>

#include "../../include/c3r.h"
#include "decode.hpp"
#include "net_host.hpp"
#include "pileup_kernels.hpp"
#include "export_kernels.hpp"
#include "reads_kernels.hpp"
#include "haplotag_kernels.hpp"
#include "phase_kernels.hpp"
#include "hapcount_kernels.hpp"
#include "hapregion_kernels.hpp"
#include "hapjunction_kernels.hpp"
#include "hapgroup_kernels.hpp"
#include "qual_kernels.hpp"
#include <sched.h>

using namespace c3r;

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct KStat { double ms = 0; int64_t n = 0; };

// what a fused scan reads back: the head of its control block (totals, overflow bits, span counts) and the allocator words
struct ScanReadback { ScanCtl ctl; unsigned long long alloc[ALLOC_SHARDS * ALLOC_STRIDE]; };

}  // namespace

struct c3r_rows;
// host copies of a loaded contig's read headers and packed bases (the decoder reads inserted bases from them): made by the first row
// snapshot after c3r_load_reads and shared by every later one of the same contig — genotyping mode decodes a contig chunk by chunk
// (c3r_call_rows ~50 times for chr1) and used to copy 100+ MB each time
struct HostReads { std::vector<DevRead> reads; std::vector<uint8_t> seq; };
typedef std::vector<c3r_padins_t> PadInsTab;
struct c3r_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    // With C3R_TWO_STREAMS=1 (opt-in; by default everything runs on ONE stream) a context that owns its streams keeps TWO: `stream` (the
    // device's highest priority) for everything but the network, and `net_stream` (lowest priority) for A6's kernels, chained by events
    // inside c3r_infer.  A layer-2 workgroup owns its CU (8 waves x
    // 256 VGPRs, 148 KB of LDS: nothing co-resides), and with one priority for all queues the dispatcher did not start another
    // queue's kernel before the running LSTM kernel had handed out its last workgroup: the ~10 short kernels of another context's
    // load_reads + scan each waited out most of a 7-14 ms kernel (profiles/r4/prep_beside_network.txt: 75-110 ms beside a network
    // pass against 2 ms alone).  At high priority they take the CUs as LSTM workgroups retire (one lives ~1.2 ms).
    hipStream_t net_stream = nullptr;
    hipEvent_t ev_x = nullptr, ev_net = nullptr;
    std::string err;
    c3r_params_t prm;
    bool profiling = false;
    std::map<std::string, KStat> kstats;
    std::vector<std::string> kstat_names;   // stable storage for c3r_get_kernel_stats
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // k_fused_deep runs BESIDE k_fused_tiles on its own stream (created at the first fused scan), forked and joined by two events
    hipStream_t deep_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_up = nullptr;            // c3r_load_reads: "my uploads have landed" (the per-device upload gate)

    // ---- inputs: the device holds the read tables; host copies are fetched on demand (depth cap, decode)
    int32_t n_reads = 0;                   // of the loaded contig
    int64_t n_indel_ops = 0;               // I + D ops of the passing reads: bounds the indel-event scratch of a scan
    int64_t n_seq_bytes = 0, n_cigar_ops = 0;
    DevBuf d_rawreads, d_rawcig;           // the caller's records as they arrived (c3r_read_t, BAM-encoded ops)
    // the pile table (reads_kernels.hpp): bin counters {cnt | sc | ec | pc}, their prefix sums, the records, per-read notes of k_prep
    DevBuf d_bincnt, d_binoff, d_rtab, d_recs, d_serial, d_nind, d_lbk, d_stats;
    BinGeo bins{0, 0};
    int32_t first_pos = 0;                 // pos of the first read (the bins start there)
    int64_t last_pos = 0;                  // pos of the last read (first guess of where the bins end)
    bool bins_dirty = true;                // the counters are not all zero (failed load)
    size_t bins_zeroed = 0;                // bytes of d_bincnt known to be zero when !bins_dirty
    // legacy tables for token_at (30-channel mode only), built on demand: normalised CIGARs, aligned segments in read order
    DevBuf d_lcnt;
    bool legacy_valid = false;
    bool legacy_wanted = false;           // a fused 30-channel scan of this context has met a column whose haplotype channels depend on the reads' order
    LoadStats *h_stats = nullptr;          // pinned
    int32_t *h_lstm = nullptr;             // pinned: this context's copy of the layer-2 time-out word (queue_lstm_status)
    // large copies from / to ORDINARY host memory go through two page-locked 8-MB buffers the context owns (big_h2d / big_d2h): the
    // runtime would pin the caller's pages for every copy and unpin them afterwards, which takes the process's memory-map lock — the
    // lock the BAM fetchers' page faults take as well (call_sample: 8-120 ms for a contig's records where the transfer is 3 ms)
    char *pin_buf[2] = {nullptr, nullptr};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_busy[2] = {false, false};
    DevBuf d_tokb, d_tokrec, d_recoff;     // packed tokens of a row snapshot (c3r_rows_begin)
    DevBuf d_rowctl; RowCtl *h_rowctl = nullptr;   // the control words of row export (export_kernels.hpp) and their page-locked host mirror (row_ctl)
    DevBuf d_keep, d_sites_c, d_probs_c;   // c3r_rows_begin_ex(drop_ref_calls): keep flags / row numbers, the kept sites' records and probabilities
    std::vector<DevRead> h_reads;          // lazily: ensure_host_reads
    std::vector<int32_t> h_prefmax;        // lazily: host copy of the prefix max of read ends (passing reads)
    std::vector<uint32_t> h_zone_sc, h_zone_ec;   // depth_cap_mask: reads per 256-position bin by start / by exclusive end
    bool host_reads_valid = false;
    DevBuf d_reads, d_cigar, d_seq, d_prefmax;
    DevBuf d_wgtab;                        // k_prep's per-workgroup bin tables between its two passes
    // mpileup_compat = 1: the insertions of the loaded reads that hold pads (c3r_padins_t), on the device for ev_equal and on the host for
    // the decoder (row snapshots share the vector); empty for every CIGAR an aligner emits
    DevBuf d_padins;
    std::shared_ptr<PadInsTab> padins;
    DevBuf d_aftab;                        // the AF gates as integer thresholds per depth (ScanArgs::af_tab), rebuilt when the AFs change
    double aftab_snp = -1.0, aftab_indel = -1.0;
    DevBuf d_dbg;                          // C3R_SCAN_DBG: phase timers of k_scan_tiles
    DevBuf d_tile_cand;                    // [n_tiles] {first candidate, count} of the most recent scan (k_compact_write -> k_tile_tokens)
    DevBuf d_tile_cols, d_tile_rng, d_tile_list, d_tile_list2, d_rsegs, d_rseg_first;
    ScanArgs last_scan;                    // arguments of the most recent scan (c3r_get_columns completes the pruned tiles with them)
    bool last_scan_pruned = false;
    // the fused path (k_fused_tiles): look-back words and counters, region bounds, what the last scan covered
    DevBuf d_lb, d_regb, d_span, d_spanbase, d_meta, d_spanrec, d_deep;       // (d_deep: list positions of the deep spans, k_fused_deep)
    DevBuf d_evwg;                         // k_fused_deep: an arrival-order event buffer per workgroup (DEEP_EVG_CAP records each), allocated once a scan has met a deep span
    bool seen_deep = false;
    DevBuf d_giant, d_giant_ev, d_giant_tab;            // k_deep_walk: the giant spans' accumulator slots (+ the slice list) and event buffers, allocated once a scan has met a giant span
    bool seen_giant = false;
    // the resident windows are int16 unless a scan of this read set has met a position that 32,768 reads or more cover (possible only above mpileup's
    // default cap, max_depth = 0 or > 32,767): that scan is repeated with int32 windows and the context keeps them from then on (a context that
    // has met such depth will meet it again: every pass over the same sample would otherwise scan twice)
    bool win32 = false;
    int n_cu = 0;                          // compute units of the device (k_fused_deep: one workgroup each)
    DevBuf d_winidx;                       // [resident candidates] row of the i-th site's window in d_tensors (the fused path writes windows as they arrive)
    DevBuf d_rawidx, d_export;             // c3r_get_tensors: index of a raw re-run, windows gathered into position order
    DevBuf d_tokexp, d_tokoff;             // c3r_get_tokens: tokens gathered into site order, their offsets there
    ScanReadback *h_scan = nullptr;        // pinned
    int32_t scan_counts[4] = {0, 0, 0, 0}; // the last scan's spans: listed, deep, giant, slices listed for k_deep_walk (c3r_get_scan_counts)
    bool last_fused = false;
    std::vector<int64_t> last_starts, last_ends;
    // page-locked buffers for the upper-cased reference slice (upload source, decoder's view).  Three of them: a row snapshot
    // (c3r_rows_begin) keeps the buffer of ITS contig alive while the context already works on the next one
    struct RefBuf { char *p = nullptr; size_t cap = 0; std::atomic<int> users{0}; hipEvent_t ev = nullptr; };
    RefBuf refbuf[3];
    int ref_cur = -1;                                             // the slot c3r_set_reference filled last
    char *h_ref = nullptr; size_t ref_len = 0;                    // = refbuf[ref_cur].p
    int64_t ref_start1 = 1;
    std::mutex pool_mu;                                           // guards stage_pool (snapshots are released from other threads)
    std::vector<std::pair<void *, size_t>> stage_pool;            // staging blocks of released row snapshots (stage_pinned())
    c3r_rows *rows_snap = nullptr;                                // c3r_call_rows keeps its snapshot here for c3r_get_rows
    std::shared_ptr<HostReads> host_cache;                        // of the loaded contig (null until a snapshot needs it)
    DevBuf d_ref;
    std::vector<int32_t> h_bed[2];
    DevBuf d_bed[2];
    bool has_bed[2] = {false, false};
    std::vector<int32_t> h_sites;
    DevBuf d_sites;
    // haplotagging (c3r_set_phase_sites): the contig's phased SNVs and, once reads have been loaded under them, the reads' tags
    // (tag | votes << 2 per read, k_haplotag) and the phase set each tag was decided in.  Nothing is allocated or launched while the table
    // is empty.
    // c3r_set_phase_alleles: the same for a table of SNVs, indels and two-ALT sites (k_haplotag_alleles).  One table at a time: n_phase counts
    // the sites of whichever is set, phase_alleles says which; d_phasea holds c3r_hap_site_t with h1 in reserved[0], d_phasepool the inserted bases.
    int64_t n_phase = 0;
    bool phase_alleles = false;
    bool hap_la = false;                      // c3r_set_hap_left_align: the four allele kernels run their _la instantiation against d_ref
    int hap_ra = 0;                           // c3r_set_hap_realign: the overhang W; above 0 they run their _ra instantiation against d_ref (never with hap_la)
    bool hap_rs = false;                      // c3r_set_hap_realign_spliced: while hap_ra is above 0 they run their _rs instantiation in the _ra one's place
    DevBuf d_phase, d_hptag, d_hpps, d_phasea, d_phasepool;
    // c3r_set_hap_min_bq: the threshold; whether the loaded reads came with qualities (c3r_load_reads_q); the qualities (2 n_seq_bytes, then
    // 32 bytes of 0xff), the masked copy of d_seq that read_args hands out while the threshold is above 0 (n_seq_bytes, then 16 zeroed bytes,
    // like d_seq) and the count of masked bases (k_mask_low_bq).  Nothing of it is allocated without qualities.
    int hap_min_bq = 0;
    bool has_qual = false;
    DevBuf d_qual, d_hapseq, d_nmasked;
    // c3r_set_hap_bq_weights: the tagging kernels run their _w instantiation, which weighs a vote by d_qual's byte and stores the chosen
    // set's (w1, w2) per read in d_hpw ([n_reads][2]; allocated by the first tagging launch under the switch, never without it)
    bool hap_w = false;
    DevBuf d_hpw;
    // phasing (c3r_phase_links): the candidate sites and their link table, allocated by the first call and kept
    DevBuf d_plsites, d_links, d_unitof;  // (d_unitof: c3r_phase_unit_links, which shares the two others)
    // per-haplotype allele counts (c3r_hap_counts): the query sites and their count table, allocated by the first call and kept
    DevBuf d_hcsites, d_hcounts;
    DevBuf d_hasites, d_hapool;               // c3r_hap_allele_counts: its query sites and the pool of inserted bases (the counts share d_hcounts)
    // c3r_hap_region_counts and c3r_hap_group_counts (hap_interval_table): the table's entries, first_open, the groups' row offsets, row_ps
    // and the count table of whichever call came last, allocated by the first call and kept; c3r_set_hap_group_direct
    DevBuf d_hientries, d_hifirst, d_hioff, d_hips, d_hicounts;
    bool hg_direct = false;
    // c3r_hap_junction_counts: the junction table (keys, then [slots][3] counters), the row table (keys, then [slots][2] counters) and the
    // overflow word, allocated by the first call and kept; the compacted, sorted result of the last call (hj_valid: there is one — until the
    // next c3r_load_reads); c3r_set_hap_junction_direct
    DevBuf d_hjtab, d_hjrows, d_hjover;
    std::vector<c3r_hap_junction_t> hj_junctions;
    std::vector<c3r_hap_junction_row_t> hj_rows;
    bool hj_valid = false, hj_direct = false;
    DevBuf d_pasites, d_papool;               // c3r_phase_allele_links / c3r_phase_allele_unit_links: their candidate sites and pool (the links share d_links, the units d_unitof)

    // ---- scan state
    int32_t reg_beg0 = 0, reg_end0 = 0;   // first region of the most recent scan (c3r_get_columns)
    int64_t n_pos = 0;                    // position slots of the most recent scan (all regions, tile-padded)
    int32_t max_cover = 0;                // upper bound of htslib's read list at any read's start (LoadStats): below max_depth the cap cannot bite
    std::vector<uint32_t> h_drop;         // depth cap of the most recent scan: [n_regions][drop_words] bit per read
    DevBuf d_drop;
    std::vector<TileGeo> h_geo;           // tile geometry of the most recent scan; re-uploaded only when it changes
    std::vector<int64_t> geo_key;         // the (start, end) list h_geo was built for
    DevBuf d_geo, d_lastrow;
    int32_t n_regions = 0;
    DevBuf d_cols, d_depth, d_ncov, d_flags, d_skipmax, d_ev, d_small /* cursor,last_row,totals */, d_blockcnt, d_scan_tops;
    int64_t n_cand = 0, n_tok = 0;        // totals resident on the device (all scans of the current batch)
    // rows of d_tensors / slots of d_tok taken by the batch so far: more than n_cand / n_tok when a large fused scan handed them out through
    // several sub-allocators (pileup_kernels.hpp, ALLOC_SHARDS) — sites reach their window and tokens through win_idx / tok_off
    int64_t n_rows = 0, n_tokspace = 0;
    int32_t hint_rows = 4096, hint_toks = 131072;      // per-shard sizes the last sharded scan needed (+ 25 %)
    int32_t last_shards = 1, last_shard_rows = 0;      // the most recent fused scan's row space (raw re-run of c3r_get_tensors)
    int64_t last_cand = 0, last_base = 0; // candidates of the most recent scan and their offset in the batch
    bool batching = false;
    DevBuf d_cand, d_tensors, d_raw, d_sites_out, d_tokcnt, d_tok;

    // ---- network
    NetState net;
    int precision_req = 1;                 // what c3r_set_precision asked for (3 = auto); net.precision is what runs
    double mx_calib_err = -1.0;            // max |dP| of precision 2 against precision 1 on the calibration windows (-1: not measured)
    double f16_calib_err = -1.0;           // max |dP| of split-f16 against the fp32 MFMA path on the same windows, measured at c3r_load_weights
    bool f16_fell_back = false;            // the guard sent a split-f16 request to the fp32 path
};

namespace {

// CPUs this process may run on (its affinity mask: one process per GPU is pinned to its share of the node, shard.host_budget), not the
// machine's: what default thread counts are taken from
static inline unsigned usable_cpus() {
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0) { const int n = CPU_COUNT(&set); if (n > 0) return (unsigned)n; }
    return std::max(1u, std::thread::hardware_concurrency());
}

typedef std::chrono::steady_clock::time_point TimePt;         // (the C3R_TIMING reports)
inline TimePt now() { return std::chrono::steady_clock::now(); }
inline double ms(TimePt a, TimePt b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

int fail(c3r_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define HIPCHK(ctx, call)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return fail(ctx, C3R_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// The layer-2 kernels meet their wavefronts through LDS counters with bounded waits (net_kernels.hpp, lds_wait): a wait that ever gives
// up raises the context's time-out word (NetState::d_tmo) instead of hanging the GPU.  Whoever hands probabilities to the host reads the
// word first — queued behind the network on the same stream, so it costs no extra synchronisation — and fails the call rather than pass
// on numbers computed from a half-written h_t.  The word belongs to the CONTEXT and c3r_infer clears it before it queues a network pass:
// the faulty batch fails (every fetch of its probabilities, until the next c3r_infer), a healthy context beside it does not, and a host
// application that embeds the library goes on with the next batch or a fresh context (round 4 kept one word per process and never cleared it).
int queue_lstm_status(c3r_ctx *ctx, int32_t **slot) {
    if (!ctx->h_lstm) HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_lstm, 64, hipHostMallocDefault));
    *ctx->h_lstm = 0;
    if (ctx->net.d_tmo) HIPCHK(ctx, hipMemcpyAsync(ctx->h_lstm, ctx->net.d_tmo, 4, hipMemcpyDeviceToHost, ctx->stream));
    *slot = ctx->h_lstm;
    return C3R_OK;
}
int check_lstm_status(c3r_ctx *ctx, const int32_t *slot) {
    if (slot && *slot)
        return fail(ctx, C3R_EHIP, "internal: a layer-2 wavefront rendezvous timed out in this batch — its probabilities are not valid (the flag is cleared by the next c3r_infer of this context)");
    return C3R_OK;
}

// Debug aid (tests/test_gpu_poison.py): C3R_POISON=<byte> fills every fresh device allocation with that byte, so that a
// kernel reading memory nobody wrote shows up as a parity failure instead of depending on what the allocator handed out.
inline int poison_byte() {
    static const int v = [] { const char *e = getenv("C3R_POISON"); return e && *e ? atoi(e) & 0xff : -1; }();
    return v;
}

// Staging blocks of row snapshots (sites | tokens | probabilities of one batch, ~0.3 GB for a large contig): ordinary memory by
// default — the runtime stages the three copies (~30 ms for a large contig), but nothing has to be pinned on the first contigs and
// unpinned when the context goes (0.1 ms per MB each way: 22 full-length contigs ran 3.4 s against 3.6-3.8 s with page-locked
// blocks).  C3R_SNAPSHOT_PINNED=1 takes page-locked blocks.
inline bool stage_pinned() {
    static const bool v = [] { const char *e = getenv("C3R_SNAPSHOT_PINNED"); return e && *e == '1'; }();
    return v;
}
inline void stage_free(void *p) { if (!p) return; if (stage_pinned()) (void)hipHostFree(p); else free(p); }
// 2-MB aligned and advised huge (C3R_IO_HUGE=0: ordinary pages): a fresh 0.3-GB block is touched for the first time by the copies into it
// and handed back page by page when the context goes — 512 times fewer pages where transparent huge pages are available.  free() releases it.
inline void *huge_alloc(size_t bytes) {
    void *p = nullptr;
    const size_t cap = (std::max<size_t>(bytes, 1) + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    if (posix_memalign(&p, (size_t)2 << 20, cap) != 0) return nullptr;
    static const bool huge = [] { const char *e = getenv("C3R_IO_HUGE"); return !(e && *e == '0'); }();
    if (huge) (void)madvise(p, cap, MADV_HUGEPAGE);
    return p;
}

int ensure(c3r_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap && b.p) return C3R_OK;
    size_t want = std::max(bytes, (size_t)256);
    want = want + want / 4;   // grow-only with slack so steady-state steps never reallocate
    const bool timing = getenv("C3R_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    if (b.p) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    const auto t1 = std::chrono::steady_clock::now();
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        // (which buffer: its offset inside the context says so — a size in the hundreds of GB is a bad count read back from the device, not a full GPU)
        return fail(ctx, C3R_ENOMEM, "hipMalloc of %zu bytes (asked for: %zu) failed for the device buffer at context offset %zu", want, bytes, (size_t)((char *)&b - (char *)ctx));
    }
    if (timing) {
        const auto t2 = std::chrono::steady_clock::now();
        const double a = std::chrono::duration<double, std::milli>(t1 - t0).count(), m = std::chrono::duration<double, std::milli>(t2 - t1).count();
        if (a + m > 1.0) fprintf(stderr, "[ensure %p] %.1f MB: sync+free %.1f ms, malloc %.1f ms\n", (void *)ctx, want / 1e6, a, m);
    }
    if (poison_byte() >= 0) { HIPCHK(ctx, hipMemsetAsync(b.p, poison_byte(), want, ctx->stream)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); }
    b.cap = want;
    return C3R_OK;
}

// The pool of staging blocks (c3r_ctx::stage_pool; snapshots are released from other threads).  take: a pooled block of at least `need` bytes, else —
// when `grow` — a fresh one with a quarter to spare; null when there is none.  give: the pool keeps three blocks.
void *stage_take(c3r_ctx *ctx, size_t need, bool grow, size_t *cap) {
    {   std::lock_guard<std::mutex> g(ctx->pool_mu);
        for (auto it = ctx->stage_pool.begin(); it != ctx->stage_pool.end(); ++it)
            if (it->second >= need) { void *p = it->first; *cap = it->second; ctx->stage_pool.erase(it); return p; }
    }
    void *p = nullptr;
    *cap = need * 5 / 4 + 4096;
    if (grow && !stage_pinned()) p = huge_alloc(*cap);
    else if (grow && hipHostMalloc(&p, *cap, hipHostMallocDefault) != hipSuccess) p = nullptr;
    return p;
}
void stage_give(c3r_ctx *ctx, void *p, size_t cap) {
    std::lock_guard<std::mutex> g(ctx->pool_mu);
    if (ctx->stage_pool.size() < 3) ctx->stage_pool.push_back({p, cap}); else stage_free(p);
}
// The control block of row export on the device (whoever counts in it clears it first) and its page-locked mirror, made at first use.
int row_ctl(c3r_ctx *ctx, RowCtl **d_ctl) {
    if (!ctx->h_rowctl && hipHostMalloc((void **)&ctx->h_rowctl, sizeof(RowCtl), hipHostMallocDefault) != hipSuccess) return fail(ctx, C3R_ENOMEM, "hipHostMalloc(64) failed");
    const int rc = ensure(ctx, ctx->d_rowctl, sizeof(RowCtl));
    *d_ctl = (RowCtl *)ctx->d_rowctl.p;
    return rc;
}

// grow a buffer but keep its first `used` bytes (batch mode appends scan after scan)
int ensure_keep(c3r_ctx *ctx, DevBuf &b, size_t bytes, size_t used) {
    if (bytes <= b.cap && b.p) return C3R_OK;
    if (!b.p || used == 0) return ensure(ctx, b, bytes);
    size_t want = bytes + bytes / 2;
    void *np_ = nullptr;
    HIPCHK(ctx, hipMalloc(&np_, want));
    if (poison_byte() >= 0) HIPCHK(ctx, hipMemsetAsync(np_, poison_byte(), want, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(np_, b.p, used, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipFree(b.p));
    b.p = np_; b.cap = want;
    return C3R_OK;
}

int big_h2d_fwd(c3r_ctx *ctx, void *dst, const void *src, size_t bytes);
template <typename T>
int upload(c3r_ctx *ctx, DevBuf &b, const T *src, size_t n) {
    int rc = ensure(ctx, b, std::max<size_t>(n * sizeof(T), 16));
    if (rc) return rc;
    if (n) return big_h2d_fwd(ctx, b.p, src, n * sizeof(T));
    return C3R_OK;
}

// ---- large copies between ordinary (pageable) host memory and the device, staged through the context's two page-locked buffers
constexpr size_t PIN_CHUNK = (size_t)8 << 20, PIN_MIN = (size_t)1 << 20;
bool pin_ring_on() {
    static const bool on = [] { const char *e = getenv("C3R_PIN_RING"); return !(e && *e == '0'); }();
    return on;
}
bool host_is_page_locked(const void *p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}
int pin_ring_init(c3r_ctx *ctx) {
    for (int k = 0; k < 2; ++k) {
        if (!ctx->pin_buf[k]) HIPCHK(ctx, hipHostMalloc((void **)&ctx->pin_buf[k], PIN_CHUNK, hipHostMallocDefault));
        if (!ctx->pin_ev[k]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->pin_ev[k], hipEventDisableTiming));
    }
    return C3R_OK;
}
// host -> device; on return the caller's bytes have been read (the last chunks may still be on their way to the device, in stream order)
int big_h2d(c3r_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return C3R_OK;
    if (bytes < PIN_MIN || !pin_ring_on() || host_is_page_locked(src)) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return C3R_OK;
    }
    int rc = pin_ring_init(ctx);
    if (rc) return rc;
    size_t off = 0;
    for (int i = 0; off < bytes; ++i) {
        const int k = i & 1;
        const size_t n = std::min(PIN_CHUNK, bytes - off);
        if (ctx->pin_busy[k]) HIPCHK(ctx, hipEventSynchronize(ctx->pin_ev[k]));          // the transfer out of this buffer is through
        memcpy(ctx->pin_buf[k], (const char *)src + off, n);
        HIPCHK(ctx, hipMemcpyAsync((char *)dst + off, ctx->pin_buf[k], n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipEventRecord(ctx->pin_ev[k], ctx->stream));
        ctx->pin_busy[k] = true;
        off += n;
    }
    return C3R_OK;
}
// device -> host, complete on return (the transfer of chunk i runs beside the host copy of chunk i - 1)
int big_d2h(c3r_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return C3R_OK;
    if (bytes < PIN_MIN || !pin_ring_on() || host_is_page_locked(dst)) {
        HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return C3R_OK;
    }
    int rc = pin_ring_init(ctx);
    if (rc) return rc;
    size_t off = 0, prev_off = 0, prev_n = 0;
    int i = 0;
    for (; off < bytes; ++i) {
        const int k = i & 1;
        const size_t n = std::min(PIN_CHUNK, bytes - off);
        if (ctx->pin_busy[k]) HIPCHK(ctx, hipEventSynchronize(ctx->pin_ev[k]));          // (an upload that used the buffer before)
        HIPCHK(ctx, hipMemcpyAsync(ctx->pin_buf[k], (const char *)src + off, n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipEventRecord(ctx->pin_ev[k], ctx->stream));
        ctx->pin_busy[k] = true;
        if (i > 0) {
            const int pk = k ^ 1;
            HIPCHK(ctx, hipEventSynchronize(ctx->pin_ev[pk]));
            memcpy((char *)dst + prev_off, ctx->pin_buf[pk], prev_n);
            ctx->pin_busy[pk] = false;
        }
        prev_off = off; prev_n = n; off += n;
    }
    const int lk = (i - 1) & 1;
    HIPCHK(ctx, hipEventSynchronize(ctx->pin_ev[lk]));
    memcpy((char *)dst + prev_off, ctx->pin_buf[lk], prev_n);
    ctx->pin_busy[lk] = false;
    return C3R_OK;
}

int big_h2d_fwd(c3r_ctx *ctx, void *dst, const void *src, size_t bytes) { return big_h2d(ctx, dst, src, bytes); }

// Launch helper: optional per-kernel HIP-event timing on the context's stream.
struct Launch {
    c3r_ctx *ctx;
    const char *name;
    Launch(c3r_ctx *c, const char *n) : ctx(c), name(n) {
        if (ctx->profiling) (void)hipEventRecord(ctx->ev0, ctx->stream);
    }
    ~Launch() {
        if (ctx->profiling) {
            (void)hipEventRecord(ctx->ev1, ctx->stream);
            (void)hipEventSynchronize(ctx->ev1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
            KStat &k = ctx->kstats[name];
            k.ms += ms; k.n += 1;
        }
    }
};

// ---- the kernels that hold the loaded reads against a site table (haplotag_kernels.hpp, hapcount_kernels.hpp, phase_kernels.hpp)
// What c3r_load_reads left on the device, as the base of such a kernel's (zeroed) arguments.
template <class Args>
Args read_args(const c3r_ctx *ctx, int n) {
    Args a;
    memset(&a, 0, sizeof a);
    a.reads = (const DevRead *)ctx->d_reads.p; a.n_reads = n; a.serial = (const uint8_t *)ctx->d_serial.p; a.cigars = (const uint32_t *)ctx->d_rawcig.p;
    a.seq = (const uint8_t *)(ctx->hap_min_bq > 0 && ctx->has_qual ? ctx->d_hapseq.p : ctx->d_seq.p);      // (c3r_set_hap_min_bq: the masked copy)
    return a;
}
// c3r_set_hap_min_bq above 0 and qualities on the device: the masked copy of d_seq, on the context's stream (nothing waits).  Flat over the
// packed sequence, so it depends on neither the filters nor the read tables.
int mask_low_bq(c3r_ctx *ctx) {
    if (ctx->hap_min_bq <= 0 || !ctx->has_qual) return C3R_OK;
    const long long nsb = ctx->n_seq_bytes, n_chunks = (nsb + 7) / 8;
    if (int rc = ensure(ctx, ctx->d_hapseq, (size_t)nsb + 16)) return rc;
    constexpr size_t count_bytes = (size_t)MASKBQ_SLOTS * MASKBQ_SLOT_WORDS * 8;
    if (int rc = ensure(ctx, ctx->d_nmasked, count_bytes)) return rc;
    HIPCHK(ctx, hipMemsetAsync((char *)ctx->d_hapseq.p + nsb, 0, 16, ctx->stream));         // (the walks read the packed bases 16 bytes at a time)
    HIPCHK(ctx, hipMemsetAsync(ctx->d_nmasked.p, 0, count_bytes, ctx->stream));
    if (n_chunks == 0) return C3R_OK;
    {
        Launch L(ctx, "k_mask_low_bq");
        const long long blocks = std::min<long long>((n_chunks + MASKBQ_THREADS - 1) / MASKBQ_THREADS, MASKBQ_MAX_BLOCKS);      // (the kernel strides over the rest)
        hipLaunchKernelGGL(k_mask_low_bq, dim3((unsigned)blocks), dim3(MASKBQ_THREADS), 0, ctx->stream,
                           (const uint8_t *)ctx->d_qual.p, (const uint8_t *)ctx->d_seq.p, (uint8_t *)ctx->d_hapseq.p, nsb, n_chunks, ctx->hap_min_bq,
                           (unsigned long long *)ctx->d_nmasked.p);
    }
    HIPCHK(ctx, hipGetLastError());
    return C3R_OK;
}
// The reference slice as the left-aligned and the realigned observation read it (c3r_set_hap_left_align, c3r_set_hap_realign), and the refusal
// of their four calls without one.
HapRef hap_ref(const c3r_ctx *ctx) {
    HapRef r;
    r.ref = (const uint8_t *)ctx->d_ref.p; r.beg0 = (int32_t)(ctx->ref_start1 - 1); r.len = (int32_t)ctx->ref_len;
    return r;
}
int hap_needs_ref(c3r_ctx *ctx, const char *call) {
    if (ctx->hap_la && ctx->ref_len == 0) return fail(ctx, C3R_EINVAL, "%s: c3r_set_hap_left_align is on and no reference is set (c3r_set_reference)", call);
    if (ctx->hap_ra > 0 && ctx->ref_len == 0) return fail(ctx, C3R_EINVAL, "%s: c3r_set_hap_realign is on and no reference is set (c3r_set_reference)", call);
    return C3R_OK;
}
// One launch of such a kernel: a group of PREP_GRP lanes per read.
template <class Args>
void launch_per_read(c3r_ctx *ctx, const char *label, void (*kernel)(Args), const Args &a) {
    Launch L(ctx, label);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.n_reads + PREP_READS - 1) / PREP_READS)), dim3(PREP_THREADS), 0, ctx->stream, a);
}
// The launch of a tagging kernel: `kernel`, or under c3r_set_hap_bq_weights its _w sibling with the qualities and the pair buffer behind
// the same arguments.
template <class Args>
int launch_tagger(c3r_ctx *ctx, const char *label, void (*kernel)(Args), const char *label_w, void (*kernel_w)(HapWeighted<Args>), const Args &a) {
    if (!ctx->hap_w) { launch_per_read<Args>(ctx, label, kernel, a); return C3R_OK; }
    if (!ctx->has_qual) return fail(ctx, C3R_EINVAL, "internal: c3r_set_hap_bq_weights is on and the loaded reads have no qualities");
    if (int rc = ensure(ctx, ctx->d_hpw, (size_t)a.n_reads * 8 + 16)) return rc;
    HapWeighted<Args> w;
    memset(&w, 0, sizeof w);
    static_cast<Args &>(w) = a;
    w.qual = (const uint8_t *)ctx->d_qual.p; w.w12 = (uint32_t *)ctx->d_hpw.p;
    launch_per_read(ctx, label_w, kernel_w, w);
    return C3R_OK;
}
// The tags of the n reads from the phase table that is set (k_haplotag*): the one choice of the kernel, from the table's kind, the
// observation (c3r_set_hap_left_align, c3r_set_hap_realign) and the weights (c3r_set_hap_bq_weights).  Nothing here waits for the device.
int launch_haplotag(c3r_ctx *ctx, int n) {
    int rc;
    if ((rc = ensure(ctx, ctx->d_hptag, (size_t)n * 4 + 16)) || (rc = ensure(ctx, ctx->d_hpps, (size_t)n * 4 + 16))) return rc;
    auto tag_args = [&](auto h) { h.hp_reads = (DevRead *)ctx->d_reads.p; h.tags = (uint32_t *)ctx->d_hptag.p; h.read_ps = (int32_t *)ctx->d_hpps.p; h.n_sites = (int32_t)ctx->n_phase; return h; };
    if (!ctx->phase_alleles) {
        HapArgs h = tag_args(read_args<HapArgs>(ctx, n));
        h.sites = (const c3r_phase_site_t *)ctx->d_phase.p;
        return launch_tagger<HapArgs>(ctx, "k_haplotag", k_haplotag, "k_haplotag_w", k_haplotag_w, h);
    }
    if ((rc = hap_needs_ref(ctx, "c3r_load_reads"))) return rc;
    HapAlleleTagRaArgs h = tag_args(read_args<HapAlleleTagRaArgs>(ctx, n));
    h.sites = (const c3r_hap_site_t *)ctx->d_phasea.p; h.pool = (const uint8_t *)ctx->d_phasepool.p;
    if (ctx->hap_ra > 0 && ctx->hap_rs) { h.ref = hap_ref(ctx); h.overhang = (uint32_t)ctx->hap_ra; return launch_tagger<HapAlleleTagRaArgs>(ctx, "k_haplotag_alleles_rs", k_haplotag_alleles_rs, "k_haplotag_alleles_rs_w", k_haplotag_alleles_rs_w, h); }
    if (ctx->hap_ra > 0) { h.ref = hap_ref(ctx); h.overhang = (uint32_t)ctx->hap_ra; return launch_tagger<HapAlleleTagRaArgs>(ctx, "k_haplotag_alleles_ra", k_haplotag_alleles_ra, "k_haplotag_alleles_ra_w", k_haplotag_alleles_ra_w, h); }
    if (ctx->hap_la) { h.ref = hap_ref(ctx); return launch_tagger<HapAlleleTagLaArgs>(ctx, "k_haplotag_alleles_la", k_haplotag_alleles_la, "k_haplotag_alleles_la_w", k_haplotag_alleles_la_w, h); }
    return launch_tagger<HapAlleleTagArgs>(ctx, "k_haplotag_alleles", k_haplotag_alleles, "k_haplotag_alleles_w", k_haplotag_alleles_w, h);
}
// A table of `words` 32-bit counters that one such launch adds to: zeroed in `buf`, filled by launch(the table on the device), copied to
// `out`.  Waits for the device: the arrays the caller handed in may go once this returns, and the table is there.
template <class LaunchOn>
int counter_table(c3r_ctx *ctx, DevBuf &buf, size_t words, uint32_t *out, LaunchOn &&launch) {
    if (int rc = ensure(ctx, buf, words * 4)) return rc;
    HIPCHK(ctx, hipMemsetAsync(buf.p, 0, words * 4, ctx->stream));
    launch((uint32_t *)buf.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, buf.p, words * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}

// c3r_hap_counts and c3r_hap_allele_counts once their n query sites are checked: the counts of `kernel` by the tags of the phase table
// that is set.  upload_sites(args) puts the query table on the device and into the arguments.
template <class Args, class Upload>
int hap_count_table(c3r_ctx *ctx, const char *label, void (*kernel)(Args), int64_t n, uint32_t *counts, Upload &&upload_sites) {
    if (ctx->n_phase == 0) return fail(ctx, C3R_EINVAL, "no phase sites are set (c3r_set_phase_sites / c3r_set_phase_alleles): the reads carry no tags to count by");
    if (n == 0) return C3R_OK;
    const size_t words = (size_t)n * 9;
    if (ctx->n_reads == 0) { memset(counts, 0, words * 4); return C3R_OK; }              // (no voters: nothing to launch)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Args a = read_args<Args>(ctx, ctx->n_reads);
    if (int rc = upload_sites(a)) return rc;
    a.n_sites = (int32_t)n;
    a.tags = (const uint32_t *)ctx->d_hptag.p; a.read_ps = (const int32_t *)ctx->d_hpps.p;
    a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags;
    return counter_table(ctx, ctx->d_hcounts, words, counts, [&](uint32_t *t) { a.counts = t; launch_per_read(ctx, label, kernel, a); });
}

// ---- c3r_hap_region_counts and c3r_hap_group_counts: what the two calls check of a sorted interval table, and everything behind the checks
// Entry j of the caller's table (`noun`: what a message calls an entry): a half-open interval, sorted by (start, end), a strand, reserved
// bytes of 0; then own_checks(), what the call asks of the entry beyond that; then first_open[j] and its bound (`advice`: the end of that
// refusal).
template <class Entry, class Own>
int check_interval(c3r_ctx *ctx, const char *noun, const char *advice, const Entry *v, int64_t j, std::vector<int32_t> &first_open, Own &&own_checks) {
    const Entry &e = v[j];
    if (e.start < 0 || e.start >= e.end) return fail(ctx, C3R_EINVAL, "%s %lld: [%d, %d) is not a 0-based half-open interval with start < end", noun, (long long)j, e.start, e.end);
    if (j > 0 && (e.start < v[j - 1].start || (e.start == v[j - 1].start && e.end < v[j - 1].end)))
        return fail(ctx, C3R_EINVAL, "%s %lld: the table must be sorted by (start, end) ([%d, %d) after [%d, %d))", noun, (long long)j, e.start, e.end, v[j - 1].start, v[j - 1].end);
    if (e.strand > 2 || e.reserved[0] || e.reserved[1] || e.reserved[2]) return fail(ctx, C3R_EINVAL, "%s %lld: strand must be 0, 1 or 2 and the reserved bytes 0", noun, (long long)j);
    if (int rc = own_checks()) return rc;
    // first_open[j]: starts never decrease, so an entry closed at start_(j - 1) stays closed and first_open never decreases either: on from
    // first_open[j - 1] to the first entry whose end lies behind this start (n + the table's length steps in all)
    int64_t f = j > 0 ? first_open[(size_t)j - 1] : 0;
    while (f < j && v[f].end <= e.start) ++f;
    first_open[(size_t)j] = (int32_t)f;
    if (j - f > C3R_HAP_REGION_MAX_BACK)
        return fail(ctx, C3R_EINVAL, "%s %lld: [%d, %d) starts while %s %lld, %lld entries before it, is still open ([%d, %d)): more than C3R_HAP_REGION_MAX_BACK = %d%s",
                    noun, (long long)j, e.start, e.end, noun, (long long)f, (long long)(j - f), v[f].start, v[f].end, C3R_HAP_REGION_MAX_BACK, advice);
    return C3R_OK;
}

// The rows of owner g of n_owners (`noun`: a region or a group; `off_name`: what the caller calls off(g), the owner's first row): offsets
// that start at 0 and never decrease, fewer than 2^24 rows, phase sets that are not negative and strictly increasing.  -> *row_end.
template <class Off>
int check_row_run(c3r_ctx *ctx, const char *noun, const char *off_name, Off &&off, int64_t g, int64_t n_owners, const int32_t *row_ps, int64_t n_rows, int64_t *row_end) {
    const int32_t lo = off(g);
    if ((g == 0 ? lo != 0 : lo < off(g - 1)) || (int64_t)lo > n_rows)
        return fail(ctx, C3R_EINVAL, "%s %lld: %s %d must start at 0, never decrease and stay within the %lld rows", noun, (long long)g, off_name, lo, (long long)n_rows);
    // (the next owner's offset is checked when its turn comes: until then only its use as this owner's end has to be safe)
    const int64_t top = g + 1 < n_owners ? std::min<int64_t>(std::max<int64_t>(off(g + 1), lo), n_rows) : n_rows;
    if (top - lo >= (1 << 24)) return fail(ctx, C3R_EINVAL, "%s %lld: %lld rows are more than a %s takes (2^24 - 1)", noun, (long long)g, (long long)(top - lo), noun);
    for (int64_t r = lo; r < top; ++r) {
        if (row_ps[r] < 0) return fail(ctx, C3R_EINVAL, "row %lld (%s %lld): phase set %d is negative", (long long)r, noun, (long long)g, row_ps[r]);
        if (r > lo && row_ps[r] <= row_ps[r - 1])
            return fail(ctx, C3R_EINVAL, "row %lld (%s %lld): phase sets must be strictly increasing inside a %s (%d after %d)", (long long)r, noun, (long long)g, noun, row_ps[r], row_ps[r - 1]);
    }
    *row_end = top;
    return C3R_OK;
}

// Both calls once their table is checked: the counts of the n_owners owners and n_rows rows by the tags of the phase table that is set.
// `dev`: the entries as the kernel loads them; `off`: the owners' row offsets where the kernel reads them from an array of their own
// (d_hioff), else empty.  launch(args) sets what its kernel takes beyond HapIntervalArgs and launches it.  One set of buffers serves both
// calls: each waits for the device before it returns (counter_table).
template <class Args, class DevEntry, class LaunchOn>
int hap_interval_table(c3r_ctx *ctx, const std::vector<DevEntry> &dev, const std::vector<int32_t> &first_open, const std::vector<int32_t> &off, const int32_t *row_ps,
                       int64_t n_owners, int64_t n_rows, int32_t stranded, uint32_t *owner_counts, uint32_t *row_counts, LaunchOn &&launch) {
    if (ctx->n_phase == 0) return fail(ctx, C3R_EINVAL, "no phase sites are set (c3r_set_phase_sites / c3r_set_phase_alleles): the reads carry no tags to count by");
    const size_t n = dev.size();
    if (n == 0) return C3R_OK;
    const size_t owner_words = 2 * (size_t)n_owners, row_words = 2 * (size_t)n_rows;
    if (ctx->n_reads == 0) {                                           // (no voters: nothing to launch)
        memset(owner_counts, 0, owner_words * 4);
        if (n_rows) memset(row_counts, 0, row_words * 4);
        return C3R_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Args a = read_args<Args>(ctx, ctx->n_reads);
    int rc;
    if ((rc = upload(ctx, ctx->d_hientries, dev.data(), n)) || (rc = upload(ctx, ctx->d_hifirst, first_open.data(), n)) ||
        (rc = upload(ctx, ctx->d_hioff, off.data(), off.size())) || (rc = upload(ctx, ctx->d_hips, row_ps, (size_t)n_rows))) return rc;
    a.entries = (const DevEntry *)ctx->d_hientries.p; a.n_entries = (int32_t)n; a.first_open = (const int32_t *)ctx->d_hifirst.p;
    a.row_ps = (const int32_t *)ctx->d_hips.p; a.n_owners = (int32_t)n_owners; a.stranded = stranded;
    a.tags = (const uint32_t *)ctx->d_hptag.p; a.read_ps = (const int32_t *)ctx->d_hpps.p;
    a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags;
    std::vector<uint32_t> table(owner_words + row_words);
    rc = counter_table(ctx, ctx->d_hicounts, table.size(), table.data(), [&](uint32_t *t) { a.counts = t; launch(a); });
    if (rc) return rc;
    memcpy(owner_counts, table.data(), owner_words * 4);
    if (n_rows) memcpy(row_counts, table.data() + owner_words, row_words * 4);
    return C3R_OK;
}

}  // namespace
static int device_excl_scan(c3r_ctx *ctx, int32_t *d, int n, int32_t *d_total);
namespace {

// ---- the device tables of the loaded reads (reads_kernels.hpp): headers, prefix maxima, the pile table.  Everything depends on the
// filters (records exist only for reads that pass them), so c3r_set_params with new --min-MQ / --excl-flags runs this again on the raw
// records the device still holds.  Four kernels, one host wait (sizes and validation errors).
// mpileup_compat = 1, reads with pads inside a run of I ops (k_prep counted them): the table of those runs, from the raw records the device
// holds (the caller's arrays may be gone when c3r_set_params switches the printer).  Same run rule as walk_serial's first look: I and P ops
// in a row, zero-length ops and hard clips skipped; the entry's key is the query offset of the run's first inserted base.
int build_padins(c3r_ctx *ctx, int n) {
    std::vector<c3r_read_t> rd((size_t)n);
    std::vector<uint32_t> cg((size_t)std::max<int64_t>(ctx->n_cigar_ops, 1));
    HIPCHK(ctx, hipMemcpyAsync(rd.data(), ctx->d_rawreads.p, (size_t)n * sizeof(c3r_read_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(cg.data(), ctx->d_rawcig.p, (size_t)ctx->n_cigar_ops * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    auto tab = std::make_shared<PadInsTab>();
    for (int i = 0; i < n; ++i) {
        const c3r_read_t &r = rd[(size_t)i];
        if ((int64_t)r.cigar_off + r.n_cigar > ctx->n_cigar_ops) continue;
        uint32_t y = 0;
        c3r_padins_t e;
        memset(&e, 0, sizeof e);
        bool open = false;
        auto close = [&]() { if (open && e.n_bases && e.pad_mask && e.total <= 64) tab->push_back(e); open = false; };
        for (uint32_t k = 0; k < r.n_cigar; ++k) {
            const uint32_t c = cg[(size_t)r.cigar_off + k], op = c & 15u, len = c >> 4;
            if (len == 0 || op == C3R_CIG_H) continue;
            if (op == C3R_CIG_I || op == C3R_CIG_P) {
                if (!open) { memset(&e, 0, sizeof e); e.read_idx = (uint32_t)i; e.qpos = y; open = true; }
                for (uint32_t j = 0; j < len && e.total <= 64; ++j, ++e.total) if (op == C3R_CIG_P && e.total < 64) e.pad_mask |= 1ull << e.total;
                if (op == C3R_CIG_I) { e.n_bases += len; y += len; }
            } else {
                close();
                if (op == C3R_CIG_M || op == C3R_CIG_EQ || op == C3R_CIG_X || op == C3R_CIG_S) y += len;
            }
        }
        close();
    }
    ctx->padins = tab;
    if (tab->empty()) return C3R_OK;
    int rc = upload(ctx, ctx->d_padins, tab->data(), tab->size());
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}

// Uploads of a contig's records take the device's whole PCIe link for milliseconds.  When several contexts of one process share a device
// (two pipelined contexts: one uploads while the other computes), two uploads at once halve each other's rate and BOTH contexts then compute
// at the same time — the link idles while the kernels run and the kernels wait while the link is busy.  One upload at a time per device keeps
// the contexts out of phase: the gate is taken before the first copy of c3r_load_reads and released at that call's first host wait (the
// read-back of the table sizes, by which the copies have landed).
static std::mutex &upload_gate(int device) {
    static std::mutex gates[64];
    return gates[(unsigned)device % 64u];
}
static std::atomic<int> &upload_waiters(int device) {          // contexts parked at the gate: whoever holds it lets go as soon as its copies have landed
    static std::atomic<int> w[64];
    return w[(unsigned)device % 64u];
}

int prepare_tables(c3r_ctx *ctx, int n, int64_t last_pos, bool timing, std::unique_lock<std::mutex> *gate = nullptr) {
    int rc;
    ctx->host_reads_valid = false; ctx->legacy_valid = false;
    if (!ctx->h_stats) HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_stats, sizeof(LoadStats), hipHostMallocDefault));
    if ((rc = ensure(ctx, ctx->d_stats, sizeof(LoadStats))) || (rc = ensure(ctx, ctx->d_reads, (size_t)n * sizeof(DevRead))) ||
        (rc = ensure(ctx, ctx->d_serial, (size_t)n + 16)) || (rc = ensure(ctx, ctx->d_nind, (size_t)n * 4 + 16)) || (rc = ensure(ctx, ctx->d_prefmax, (size_t)n * 4 + 16)))
        return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    // bins from the first read's position (the records are sorted) to a guess of the largest end: the last read's position plus 2 Mb —
    // when a read reaches further (the device knows after the first pass) the table grows and the pass runs again
    int64_t want_end = std::max<int64_t>(last_pos, ctx->first_pos) + BIN_END_GUESS;
    LoadStats hs;
    for (int attempt = 0;; ++attempt) {
        const int32_t base = ctx->first_pos >> BIN_SHIFT;
        want_end = std::min<int64_t>(want_end, (int64_t)INT32_MAX);
        const int32_t nb = (int32_t)((want_end >> BIN_SHIFT) - base + 2), nbc = (nb >> CBIN_SHIFT) + 2;
        const int32_t nb_pad = (nb + 1023) & ~1023;                           // (the bin counters are laid out in whole blocks of 1024: cnt_at)
        const size_t cnt_bytes = ((size_t)nb_pad + 3 * (size_t)nbc) * 4;      // records per bin | reads started | ended | prefix-max histogram per coarse bin
        if (ctx->d_bincnt.cap < cnt_bytes || !ctx->d_bincnt.p) ctx->bins_zeroed = 0;                                    // (a fresh block)
        if ((rc = ensure(ctx, ctx->d_bincnt, cnt_bytes)) || (rc = ensure(ctx, ctx->d_binoff, (size_t)(nb + 1) * 4 + 16)) || (rc = ensure(ctx, ctx->d_rtab, (size_t)(nbc + 1) * sizeof(int4)))) return rc;
        ctx->bins = BinGeo{base, nb, nbc, 0};
        // the counter arrays lie back to back and every pass leaves them all zero (k_bin_scan, k_prep<true>): nothing to clear as long as
        // they stay inside what has been cleared once
        if (ctx->bins_dirty || cnt_bytes > ctx->bins_zeroed) {
            HIPCHK(ctx, hipMemsetAsync(ctx->d_bincnt.p, 0, std::max(cnt_bytes, ctx->bins_zeroed), ctx->stream));
            ctx->bins_zeroed = std::max(cnt_bytes, ctx->bins_zeroed);
        }
        ctx->bins_dirty = true;                               // until this pass has come through
        const int nb_pm = (n + PM_BLK - 1) / PM_BLK, nb_bs = (nb + BS_BLK - 1) / BS_BLK, nb_bc = (nbc + BS_BLK - 1) / BS_BLK;
        const size_t lbk_bytes = 64 + (size_t)(nb_pm + nb_bs + 2 * nb_bc) * 8;
        if ((rc = ensure(ctx, ctx->d_lbk, lbk_bytes))) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->d_lbk.p, 0, lbk_bytes, ctx->stream));
        LoadStats init;
        memset(&init, 0, sizeof init);
        init.err = ~0ull;
        *ctx->h_stats = init;
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_stats.p, ctx->h_stats, sizeof init, hipMemcpyHostToDevice, ctx->stream));
        PrepArgs a;
        memset(&a, 0, sizeof a);
        a.reads = (const c3r_read_t *)ctx->d_rawreads.p; a.n_reads = n; a.cigars = (const uint32_t *)ctx->d_rawcig.p;
        a.n_cigar_ops = ctx->n_cigar_ops; a.n_seq_bytes = ctx->n_seq_bytes; a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags; a.compat = ctx->prm.mpileup_compat;
        a.geo = ctx->bins;
        uint32_t *cnt = (uint32_t *)ctx->d_bincnt.p;
        a.cnt = cnt; a.sc = cnt + nb_pad; a.ec = a.sc + nbc; uint32_t *pc = a.ec + nbc;
        a.rec_off = (const uint32_t *)ctx->d_binoff.p; a.out = (DevRead *)ctx->d_reads.p; a.serial = (uint8_t *)ctx->d_serial.p; a.nind = (int32_t *)ctx->d_nind.p;
        a.st = (LoadStats *)ctx->d_stats.p;
        char *lbk = (char *)ctx->d_lbk.p;
        const unsigned grid = (unsigned)((n + PREP_READS - 1) / PREP_READS);
        if ((rc = ensure(ctx, ctx->d_wgtab, (size_t)grid * WG_TAB_WORDS * 4))) return rc;    // what the workgroups counted, kept for the second pass
        a.wg_tab = (uint32_t *)ctx->d_wgtab.p;
        {
            Launch L(ctx, "k_prep_count");
            hipLaunchKernelGGL(k_prep<false>, dim3(grid), dim3(PREP_THREADS), 0, ctx->stream, a);
        }
        {
            Launch L(ctx, "k_prefmax_bins");
            hipLaunchKernelGGL(k_prefmax_bins, dim3(nb_pm), dim3(1024), 0, ctx->stream, (const DevRead *)ctx->d_reads.p, n, ctx->prm.min_mq, ctx->prm.excl_flags, ctx->bins,
                               (const int32_t *)ctx->d_nind.p, (int32_t *)ctx->d_prefmax.p, pc, a.st, (int32_t *)lbk, (unsigned long long *)(lbk + 64));
        }
        {
            Launch L(ctx, "k_bin_scan");
            hipLaunchKernelGGL(k_bin_scan, dim3(nb_bs + nb_bc), dim3(1024), 0, ctx->stream, (const uint32_t *)a.cnt, a.sc, pc, a.ec, ctx->bins, nb_bs, (uint32_t *)ctx->d_binoff.p,
                               (int4 *)ctx->d_rtab.p, a.st, (int32_t *)(lbk + 4), (unsigned long long *)(lbk + 64 + (size_t)nb_pm * 8),
                               (unsigned long long *)(lbk + 64 + (size_t)(nb_pm + nb_bs) * 8), (unsigned long long *)(lbk + 64 + (size_t)(nb_pm + nb_bs + nb_bc) * 8));
        }
        // ---- the one synchronisation: sizes, errors
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_stats, ctx->d_stats.p, sizeof(LoadStats), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (gate && gate->owns_lock()) gate->unlock();          // (the uploads have landed: the next context's may start)
        HIPCHK(ctx, hipGetLastError());
        hs = *ctx->h_stats;
        if (hs.err != ~0ull) {
            const long long i = (long long)(hs.err >> 8);
            switch ((int)(hs.err & 0xff)) {
                case LD_UNSORTED: return fail(ctx, C3R_EINVAL, "reads must be sorted by pos (read %lld)", i);
                case LD_CIGAR_RANGE: return fail(ctx, C3R_EINVAL, "cigar range of read %lld out of bounds", i);
                case LD_SEQ_RANGE: return fail(ctx, C3R_EINVAL, "seq range of read %lld out of bounds", i);
                case LD_BAD_OP: return fail(ctx, C3R_EINVAL, "bad cigar op in read %lld", i);
                case LD_OP_LONG: return fail(ctx, C3R_EINVAL, "cigar op too long in read %lld", i);
                case LD_END_2G: return fail(ctx, C3R_EINVAL, "read %lld ends beyond 2^31", i);
                case LD_SEG_OPS: return fail(ctx, C3R_EINVAL, "read %lld: more than 65535 CIGAR ops between two N ops", i);
                case LD_PAD_INS: return fail(ctx, C3R_EINVAL, "read %lld: an insertion with pads (P ops) of more than 64 characters is not supported with mpileup_compat = 1", i);
                default: return fail(ctx, C3R_EINVAL, "invalid read %lld", i);
            }
        }
        if ((int64_t)hs.max_end <= (((int64_t)base + nb) << BIN_SHIFT)) break;
        if (attempt >= 1) return fail(ctx, C3R_EINVAL, "internal: the position bins did not grow to the reads' ends");
        want_end = (int64_t)hs.max_end + 64;                  // a read reaches beyond the table: the counts of its far bins were clamped
    }
    if (hs.n_rec < 0) return fail(ctx, C3R_EINVAL, "too many CIGAR ops");
    ctx->padins.reset();
    if (hs.n_padreads > 0 && (rc = build_padins(ctx, n))) return rc;          // (hand-made CIGARs only: off the measured path)
    const auto t_sync = std::chrono::steady_clock::now();
    // ---- haplotags from the phase sites, if the caller has set any: the records have passed the range checks above, and the second pass
    // takes every read's hp from the header this kernel writes it to (nothing here waits for the device)
    if (ctx->n_phase > 0 && (rc = launch_haplotag(ctx, n))) return rc;
    // ---- second pass (nothing below waits for the device): every record into its bin
    if ((rc = ensure(ctx, ctx->d_recs, (size_t)hs.n_rec * sizeof(PileRec) + 64))) return rc;
    {
        PrepArgs a;
        memset(&a, 0, sizeof a);
        a.n_reads = n; a.cigars = (const uint32_t *)ctx->d_rawcig.p; a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags; a.compat = ctx->prm.mpileup_compat; a.geo = ctx->bins;
        a.cnt = (uint32_t *)ctx->d_bincnt.p; a.rec_off = (const uint32_t *)ctx->d_binoff.p; a.out = (DevRead *)ctx->d_reads.p; a.serial = (uint8_t *)ctx->d_serial.p;
        a.recs = (PileRec *)ctx->d_recs.p;
        a.wg_tab = (uint32_t *)ctx->d_wgtab.p;
        Launch L(ctx, "k_prep_write");
        hipLaunchKernelGGL(k_prep<true>, dim3((unsigned)((n + PREP_READS - 1) / PREP_READS)), dim3(PREP_THREADS), 0, ctx->stream, a);
    }
    HIPCHK(ctx, hipGetLastError());
    ctx->bins_dirty = false;                                  // (the record counters are back at zero once k_prep<true> is through)
    ctx->n_reads = n; ctx->n_indel_ops = hs.n_indel; ctx->max_cover = hs.max_cover;
    // (under the profiler: how many workgroups of the second pass counted their records again — no kernel, `launches` is the count)
    if (ctx->profiling && hs.n_recount > 0) ctx->kstats["k_prep_recount_workgroups"].n += hs.n_recount;
    if (timing) {
        fprintf(stderr, "[c3r_load_reads] %d reads, %d records in %d bins: first pass until the sync %.2f ms, second pass queued in %.2f ms\n", n, hs.n_rec, ctx->bins.nb,
                ms(t_begin, t_sync), ms(t_sync, std::chrono::steady_clock::now()));
    }
    return C3R_OK;
}

// New filters for the reads already loaded (c3r_set_params changed --min-MQ / --excl-flags): the tables are rebuilt from the raw records.
int refilter(c3r_ctx *ctx) {
    const int n = ctx->n_reads;
    if (n == 0) return C3R_OK;
    ctx->n_reads = 0;
    return prepare_tables(ctx, n, ctx->last_pos, false);
}

// The legacy tables (reads_kernels.hpp): only token_at reads them — the ordered haplotype recompute of flagged columns, 30 channels.
int ensure_legacy_tables(c3r_ctx *ctx) {
    if (ctx->legacy_valid || ctx->n_reads == 0) return C3R_OK;
    const int n = ctx->n_reads;
    int rc;
    if ((rc = ensure(ctx, ctx->d_lcnt, (size_t)(n + 2) * sizeof(int2)))) return rc;
    // sizes without asking the device: normalisation only drops or merges ops, and a read with k ref-skips has k + 1 segments out of at least
    // 2 k + 1 ops — (ops + reads) / 2 segments at most.  (Round 4 read the two totals back: a host wait in every 30-channel pass.)
    const size_t max_ops = (size_t)ctx->n_cigar_ops, max_segs = ((size_t)ctx->n_cigar_ops + (size_t)n) / 2 + 1;
    if ((rc = ensure(ctx, ctx->d_cigar, max_ops * 4 + 16)) || (rc = ensure(ctx, ctx->d_rsegs, max_segs * sizeof(DevSeg) + 16)) ||
        (rc = ensure(ctx, ctx->d_rseg_first, (size_t)(n + 1) * 4)))
        return rc;
    Launch L(ctx, "k_legacy_tables");
    hipLaunchKernelGGL(k_legacy_count, dim3((unsigned)(n / 256 + 1)), dim3(256), 0, ctx->stream, (const DevRead *)ctx->d_reads.p, n, (const uint32_t *)ctx->d_rawcig.p, (int2 *)ctx->d_lcnt.p);
    hipLaunchKernelGGL(k_legacy_scan, dim3(1), dim3(1024), 0, ctx->stream, (int2 *)ctx->d_lcnt.p, n + 1, (int2 *)ctx->d_lcnt.p + (n + 1));
    hipLaunchKernelGGL(k_legacy_write, dim3((unsigned)(n / 256 + 1)), dim3(256), 0, ctx->stream, (const DevRead *)ctx->d_reads.p, n, (const uint32_t *)ctx->d_rawcig.p,
                       (const int2 *)ctx->d_lcnt.p, (uint32_t *)ctx->d_cigar.p, (DevSeg *)ctx->d_rsegs.p, (uint32_t *)ctx->d_rseg_first.p);
    HIPCHK(ctx, hipGetLastError());
    ctx->legacy_valid = true;
    return C3R_OK;
}

// Host copies, fetched only by the path that walks reads on the host: mpileup's depth cap (sequential by nature).  (The decoder's copies — inserted
// bases of the alt alleles — belong to the row snapshots: HostReads, rows_read_source.)
int ensure_host_reads(c3r_ctx *ctx) {
    if (ctx->host_reads_valid) return C3R_OK;
    ctx->h_reads.resize((size_t)ctx->n_reads); ctx->h_prefmax.resize((size_t)ctx->n_reads);
    if (ctx->n_reads) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_reads.data(), ctx->d_reads.p, (size_t)ctx->n_reads * sizeof(DevRead), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_prefmax.data(), ctx->d_prefmax.p, (size_t)ctx->n_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->host_reads_valid = true;
    return C3R_OK;
}

// sort + merge intervals into a disjoint union (the overlap test against the union equals the
// reference's any-interval overlap, shared/interval_tree.py:77-87)
void merge_intervals(std::vector<int32_t> &iv) {
    std::vector<std::pair<int32_t, int32_t>> v;
    for (size_t i = 0; i + 1 < iv.size(); i += 2) v.push_back({iv[i], iv[i + 1]});
    std::sort(v.begin(), v.end());
    iv.clear();
    for (auto &x : v) {
        if (x.second <= x.first) continue;
        if (!iv.empty() && x.first <= iv.back()) iv.back() = std::max(iv.back(), x.second);
        else { iv.push_back(x.first); iv.push_back(x.second); }
    }
}

}  // namespace

// Developer knobs of the scan path: environment variables, never needed in production.  Read once per entry into the scan code
// — c3r_pileup_scan_regions, c3r_get_columns, the raw re-run of c3r_get_tensors — and passed down, so a test may change them between two scans.
struct ScanKnobs {
    int abl, deep_min, split_min, split_slice, split_cus, giant_wgs, list_grid;
    int evwg, giant;              // 0: never, 1: from the first scan on, -1 (unset, or anything else): once a scan of the context has met such a span
    bool dbg, no_shift, no_fuse, no_prune, no_giant_tab, legacy_eager, one_shard, deep_serial, cap_all;
};
static ScanKnobs read_scan_knobs(const c3r_ctx *ctx) {
    const auto set = [](const char *e) { return e != nullptr; };
    const auto is1 = [](const char *e) { return e && *e == '1'; };
    const auto at_least_1 = [](const char *e, int dflt) { return e ? std::max(1, atoi(e)) : dflt; };
    const auto never_or_now = [](const char *e) { return !e ? -1 : *e == '0' ? 0 : *e == '1' ? 1 : -1; };
    ScanKnobs k;
    { const char *e = getenv("C3R_SCAN_ABL"); k.abl = e ? atoi(e) : 0; }       // ablation bits of the diagnostic build (ScanArgs::abl)
    k.dbg = set(getenv("C3R_SCAN_DBG"));                                       // phase clocks of the tile kernels, printed after the scan
    k.deep_min = at_least_1(getenv("C3R_DEEP_MIN"), DEEP_MIN_RECORDS);         // records from which a span is k_fused_deep's
    k.split_min = at_least_1(getenv("C3R_SPLIT_MIN"), SPLIT_MIN_RECORDS);      // records from which a span is giant
    k.split_slice = at_least_1(getenv("C3R_SPLIT_SLICE"), GIANT_SLICE);        // records per slice of a giant span
    k.split_cus = at_least_1(getenv("C3R_SPLIT_CUS"), ctx->n_cu > 0 ? ctx->n_cu : 256);   // the CU count of the share rule (giant_on)
    k.no_shift = is1(getenv("C3R_NO_SHIFT"));                                  // spans on the regions' fixed grid
    k.no_fuse = set(getenv("C3R_NO_FUSE"));                                    // the plain mode through the column store
    k.no_prune = set(getenv("C3R_NO_PRUNE"));                                  // the column store scans intron-only tiles too
    k.evwg = never_or_now(getenv("C3R_EVWG"));                                 // k_fused_deep's per-workgroup event buffers
    k.giant = never_or_now(getenv("C3R_GIANT"));                               // the giant-span pool
    k.no_giant_tab = set(getenv("C3R_NO_GIANT_TAB"));                          // giant spans' alleles counted by the span's own workgroup
    k.legacy_eager = is1(getenv("C3R_LEGACY_EAGER"));                          // 30 channels: op / segment tables before the first flagged column
    k.one_shard = set(getenv("C3R_ONE_SHARD"));                                // one allocator however large the scan
    k.deep_serial = set(getenv("C3R_DEEP_SERIAL"));                            // k_fused_deep behind k_fused_tiles on one stream
    k.giant_wgs = at_least_1(getenv("C3R_GIANT_WGS"), 2);                      // workgroups per CU of k_deep_walk / k_deep_alleles
    { const char *e = getenv("C3R_LIST_GRID"); k.list_grid = e && atoi(e) > 0 ? atoi(e) : LIST_GRID; }   // workgroups of the column store's tile kernels
    k.cap_all = is1(getenv("C3R_CAP_ALL"));                                    // the depth-cap rule over every read, not only the hot zones (A/B aid)
    return k;
}

// f(std::integral_constant<int, C>) for the context's channel count: picks the instance of a kernel templated on it
template <class F>
static void with_channels(const c3r_ctx *ctx, F &&f) {
    if (ctx->prm.channels == C3R_CH) f(std::integral_constant<int, C3R_CH>{});
    else f(std::integral_constant<int, C3R_CH_PHASED>{});
}

extern "C" {

const char *c3r_version(void) { return "c3r 0.1 (gfx950, HIP)"; }

void c3r_default_params(c3r_params_t *p) {
    memset(p, 0, sizeof *p);
    p->max_depth = 8000;
    p->channels = C3R_CH;
    p->min_mq = 5;
    p->excl_flags = 2316;
    p->min_coverage = 4;
    p->snp_min_af = 0.08;
    p->indel_min_af = 0.15;
    p->max_depth_rescale = 144;
}

int c3r_create(int device_id, void *stream, c3r_ctx **out) {
    if (!out) return C3R_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return C3R_ENODEVICE;
    if (device_id < 0 || device_id >= n) return C3R_EINVAL;
    if (hipSetDevice(device_id) != hipSuccess) return C3R_ENODEVICE;
    c3r_ctx *ctx = new c3r_ctx();
    ctx->device = device_id;
    { int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess) ctx->n_cu = cu; }
    c3r_default_params(&ctx->prm);
    if (stream) ctx->stream = (hipStream_t)stream;
    else {
        const char *two = getenv("C3R_TWO_STREAMS");
        if (!(two && *two && *two != '0')) {
            if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return C3R_EHIP; }
        } else {
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, greatest) != hipSuccess) { delete ctx; return C3R_EHIP; }
            ctx->owns_stream = true;
            if (hipStreamCreateWithPriority(&ctx->net_stream, hipStreamNonBlocking, least) != hipSuccess ||
                hipEventCreateWithFlags(&ctx->ev_x, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_net, hipEventDisableTiming) != hipSuccess) { c3r_destroy(ctx); return C3R_EHIP; }
        }
        ctx->owns_stream = true;
    }
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) { delete ctx; return C3R_EHIP; }
    *out = ctx;
    return C3R_OK;
}

void c3r_destroy(c3r_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->net_stream) (void)hipStreamSynchronize(ctx->net_stream);
    if (ctx->deep_stream) (void)hipStreamSynchronize(ctx->deep_stream);
    (void)hipStreamSynchronize(ctx->stream);
    const bool timing = getenv("C3R_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf *bufs[] = {&ctx->d_wgtab, &ctx->d_rawreads, &ctx->d_rawcig, &ctx->d_bincnt, &ctx->d_binoff, &ctx->d_rtab, &ctx->d_recs, &ctx->d_serial, &ctx->d_nind, &ctx->d_lbk, &ctx->d_lcnt, &ctx->d_tokexp, &ctx->d_tokoff,
                      &ctx->d_stats, &ctx->d_lb, &ctx->d_regb, &ctx->d_span, &ctx->d_spanbase, &ctx->d_meta, &ctx->d_spanrec, &ctx->d_deep, &ctx->d_evwg, &ctx->d_giant, &ctx->d_giant_ev, &ctx->d_giant_tab, &ctx->d_winidx, &ctx->d_rawidx, &ctx->d_export, &ctx->d_dbg, &ctx->d_tile_cand, &ctx->d_reads, &ctx->d_cigar, &ctx->d_seq, &ctx->d_prefmax, &ctx->d_tile_cols, &ctx->d_tile_rng, &ctx->d_tile_list, &ctx->d_tile_list2, &ctx->d_rsegs, &ctx->d_rseg_first, &ctx->d_ref, &ctx->d_bed[0], &ctx->d_bed[1],
                      &ctx->d_sites, &ctx->d_phase, &ctx->d_phasea, &ctx->d_phasepool, &ctx->d_qual, &ctx->d_hapseq, &ctx->d_nmasked, &ctx->d_hpw, &ctx->d_hptag, &ctx->d_hpps, &ctx->d_hcsites, &ctx->d_hcounts, &ctx->d_hasites, &ctx->d_hapool, &ctx->d_hientries, &ctx->d_hifirst, &ctx->d_hioff, &ctx->d_hips, &ctx->d_hicounts, &ctx->d_hjtab, &ctx->d_hjrows, &ctx->d_hjover, &ctx->d_pasites, &ctx->d_papool, &ctx->d_plsites, &ctx->d_links, &ctx->d_unitof, &ctx->d_cols, &ctx->d_depth, &ctx->d_ncov, &ctx->d_flags, &ctx->d_skipmax, &ctx->d_geo, &ctx->d_lastrow, &ctx->d_drop, &ctx->d_ev, &ctx->d_small,
                      &ctx->d_blockcnt, &ctx->d_scan_tops, &ctx->d_cand, &ctx->d_tensors, &ctx->d_raw, &ctx->d_sites_out, &ctx->d_tokcnt, &ctx->d_tok, &ctx->d_tokb, &ctx->d_tokrec, &ctx->d_recoff, &ctx->d_rowctl, &ctx->d_padins, &ctx->d_aftab, &ctx->d_keep, &ctx->d_sites_c, &ctx->d_probs_c};
    int n_dev = 0; size_t b_dev = 0, b_pin = 0, cap = 0;
    for (DevBuf *b : bufs) if (b->p) { (void)hipFree(b->p); ++n_dev; b_dev += b->cap; }
    const auto t1 = std::chrono::steady_clock::now();
    net_free(ctx->net);
    const auto t2 = std::chrono::steady_clock::now();
    if (ctx->rows_snap) c3r_rows_free(ctx->rows_snap);
    while (void *p = stage_take(ctx, 0, false, &cap)) { stage_free(p); b_pin += cap; }
    if (ctx->h_stats) (void)hipHostFree(ctx->h_stats);
    if (ctx->h_rowctl) (void)hipHostFree(ctx->h_rowctl);
    for (int k = 0; k < 2; ++k) { if (ctx->pin_buf[k]) (void)hipHostFree(ctx->pin_buf[k]); if (ctx->pin_ev[k]) (void)hipEventDestroy(ctx->pin_ev[k]); }
    if (ctx->h_lstm) (void)hipHostFree(ctx->h_lstm);
    if (ctx->h_scan) (void)hipHostFree(ctx->h_scan);
    for (auto &rb : ctx->refbuf) { if (rb.p) { (void)hipHostFree(rb.p); b_pin += rb.cap; } if (rb.ev) (void)hipEventDestroy(rb.ev); }
    const auto t3 = std::chrono::steady_clock::now();
    if (ctx->deep_stream) (void)hipStreamDestroy(ctx->deep_stream);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_up) (void)hipEventDestroy(ctx->ev_up);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->net_stream) (void)hipStreamDestroy(ctx->net_stream);
    if (ctx->ev_x) (void)hipEventDestroy(ctx->ev_x);
    if (ctx->ev_net) (void)hipEventDestroy(ctx->ev_net);
    if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    if (timing) {
        fprintf(stderr, "[c3r_destroy %p] %d device buffers (%.0f MB) %.1f ms, network buffers %.1f ms, host blocks (%.0f MB) %.1f ms, events + stream %.1f ms\n",
                (void *)ctx, n_dev, b_dev / 1e6, ms(t0, t1), ms(t1, t2), b_pin / 1e6, ms(t2, t3), ms(t3, std::chrono::steady_clock::now()));
    }
    delete ctx;
}

int64_t c3r_trim(void) { return (int64_t)big_trim(); }

const char *c3r_last_error(const c3r_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int c3r_synchronize(c3r_ctx *ctx) {
    if (!ctx) return C3R_EINVAL;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}

void *c3r_stream(c3r_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int c3r_set_params(c3r_ctx *ctx, const c3r_params_t *p) {
    if (!ctx || !p) return C3R_EINVAL;
    if (p->channels != C3R_CH && p->channels != C3R_CH_PHASED) return fail(ctx, C3R_EINVAL, "channels must be 18 or 30");
    if (p->mpileup_compat != 0 && p->mpileup_compat != 1) return fail(ctx, C3R_EINVAL, "mpileup_compat must be 0 (samtools <= 1.10) or 1 (samtools >= 1.11)");
    // (the pile table holds the records of the reads that pass the filters, with the indel look-ahead of the chosen samtools)
    const bool refilter = p->min_mq != ctx->prm.min_mq || p->excl_flags != ctx->prm.excl_flags || p->mpileup_compat != ctx->prm.mpileup_compat;
    ctx->prm = *p;
    if (ctx->prm.max_depth_rescale <= 0) ctx->prm.max_depth_rescale = 144;
    ctx->last_scan_pruned = false;
    if (refilter) return ::refilter(ctx);
    return C3R_OK;
}

int c3r_load_reads(c3r_ctx *ctx, const c3r_read_t *reads, int64_t n_reads, const uint32_t *cigars, int64_t n_cigar_ops,
                   const uint8_t *seq4, int64_t n_seq_bytes) {
    return c3r_load_reads_q(ctx, reads, n_reads, cigars, n_cigar_ops, seq4, n_seq_bytes, nullptr, 0);
}

int c3r_load_reads_q(c3r_ctx *ctx, const c3r_read_t *reads, int64_t n_reads, const uint32_t *cigars, int64_t n_cigar_ops,
                     const uint8_t *seq4, int64_t n_seq_bytes, const uint8_t *qual, int64_t n_qual_bytes) {
    if (!ctx || n_reads < 0 || n_cigar_ops < 0 || n_seq_bytes < 0 || (n_reads && (!reads || !cigars || !seq4))) return C3R_EINVAL;
    if (qual && n_qual_bytes != 2 * n_seq_bytes)
        return fail(ctx, C3R_EINVAL, "c3r_load_reads_q: %lld quality bytes for %lld sequence bytes (there are two per byte)", (long long)n_qual_bytes, (long long)n_seq_bytes);
    if (!qual && n_qual_bytes != 0) return fail(ctx, C3R_EINVAL, "c3r_load_reads_q: %lld quality bytes and no array", (long long)n_qual_bytes);
    if (!qual && n_reads > 0 && ctx->hap_min_bq > 0)               // (before anything of the previous load is given up)
        return fail(ctx, C3R_EINVAL, "c3r_load_reads: c3r_set_hap_min_bq is %d and the reads come without qualities (c3r_load_reads_q)", ctx->hap_min_bq);
    if (!qual && n_reads > 0 && ctx->hap_w)
        return fail(ctx, C3R_EINVAL, "c3r_load_reads: c3r_set_hap_bq_weights is on and the reads come without qualities (c3r_load_reads_q)");
    if (n_reads >= INT32_MAX) return fail(ctx, C3R_EINVAL, "too many reads");
    if (n_cigar_ops >= INT32_MAX) return fail(ctx, C3R_EINVAL, "too many CIGAR ops");
    if (ctx->phase_alleles) if (int rc0 = hap_needs_ref(ctx, "c3r_load_reads")) return rc0;       // (before anything of the previous load is given up)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool timing = getenv("C3R_TIMING") != nullptr;
    // whatever happens below, the previous contig's tables are gone
    ctx->n_reads = 0; ctx->n_indel_ops = 0; ctx->n_seq_bytes = 0; ctx->n_cigar_ops = 0; ctx->max_cover = 0;
    ctx->host_reads_valid = false; ctx->last_scan_pruned = false; ctx->legacy_valid = false;
    ctx->hj_valid = false; ctx->hj_junctions.clear(); ctx->hj_rows.clear();
    ctx->host_cache.reset();              // (snapshots of the previous contig keep their copy alive)
    ctx->padins.reset();
    const int n = (int)n_reads;
    int rc;
    // ---- the caller's records go up as they are (three copies; truly asynchronous when the caller's arrays are pinned, see
    // c3r_host_alloc) and every table the tile kernels need is derived from them on the device
    if ((rc = ensure(ctx, ctx->d_rawreads, std::max<size_t>((size_t)n * sizeof(c3r_read_t), 16))) || (rc = ensure(ctx, ctx->d_rawcig, std::max<size_t>((size_t)n_cigar_ops * 4, 16))) ||
        (rc = ensure(ctx, ctx->d_seq, (size_t)n_seq_bytes + 16))) return rc;
    ctx->has_qual = false;
    if (qual && (rc = ensure(ctx, ctx->d_qual, 2 * (size_t)n_seq_bytes + 32))) return rc;
    upload_waiters(ctx->device).fetch_add(1);
    std::unique_lock<std::mutex> gate(upload_gate(ctx->device));
    upload_waiters(ctx->device).fetch_sub(1);
    {
        Launch l(ctx, "h2d_reads");           // (profiling: the three uploads as one entry of the kernel statistics — PCIe time, not a kernel)
        if ((rc = upload(ctx, ctx->d_rawreads, reads, (size_t)n)) || (rc = upload(ctx, ctx->d_rawcig, cigars, (size_t)n_cigar_ops))) return rc;
        if (n_seq_bytes && (rc = big_h2d(ctx, ctx->d_seq.p, seq4, (size_t)n_seq_bytes))) return rc;
        if (qual && n_seq_bytes && (rc = big_h2d(ctx, ctx->d_qual.p, qual, 2 * (size_t)n_seq_bytes))) return rc;
    }
    if (qual) HIPCHK(ctx, hipMemsetAsync((char *)ctx->d_qual.p + 2 * n_seq_bytes, 0xff, 32, ctx->stream));    // (k_mask_low_bq reads them 16 bytes at a time)
    HIPCHK(ctx, hipMemsetAsync((char *)ctx->d_seq.p + n_seq_bytes, 0, 16, ctx->stream));        // (the walk reads the packed bases 16 bytes at a time)
    if (upload_waiters(ctx->device).load() > 0) {
        // another context is waiting to upload: the link is handed over when THESE copies are through, not a first table pass later
        if (!ctx->ev_up) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_up, hipEventDisableTiming));
        HIPCHK(ctx, hipEventRecord(ctx->ev_up, ctx->stream));
        HIPCHK(ctx, hipEventSynchronize(ctx->ev_up));
        gate.unlock();
    }
    ctx->n_seq_bytes = n_seq_bytes; ctx->n_cigar_ops = n_cigar_ops;
    ctx->has_qual = qual != nullptr;
    if ((rc = mask_low_bq(ctx))) return rc;                       // (before the haplotag launch of prepare_tables, on the same stream)
    if (n == 0) return C3R_OK;
    ctx->first_pos = std::max(reads[0].pos, 0);
    // the last read's position bounds the first guess of the bins (the records are sorted; an unsorted set fails in the first pass)
    const int64_t last_pos = std::max(reads[n - 1].pos, reads[0].pos);
    ctx->last_pos = last_pos;
    return prepare_tables(ctx, n, last_pos, timing, &gate);
}

void *c3r_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void c3r_host_free(void *p) { if (p) (void)hipHostFree(p); }

int c3r_set_reference(c3r_ctx *ctx, int64_t ref_start, const char *ref, int64_t len) {
    if (!ctx || !ref || len < 0 || ref_start < 1) return C3R_EINVAL;
    if (ref_start - 1 + len > INT32_MAX) return fail(ctx, C3R_EINVAL, "reference slice ends beyond 2^31");          // (the kernels index it by 32-bit offsets)
    ctx->last_scan_pruned = false;       // (c3r_get_columns completes a pruned scan with the arguments of that scan: stale now)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // The slice is upper-cased straight into a page-locked buffer the context keeps (one pass over the caller's bytes, on threads for a
    // whole chromosome), which is both the source of an asynchronous DMA upload — nothing here waits for the device — and the decoder's
    // view of the reference.  The previous upload must have left the buffer before it is overwritten.
    ctx->ref_len = 0;
    // a buffer no snapshot holds: the current one if it is free, else another (waiting for a decode to finish if all three are held)
    int slot = -1;
    for (int waited = 0; slot < 0; ++waited) {
        if (ctx->ref_cur >= 0 && ctx->refbuf[ctx->ref_cur].users.load() == 0) slot = ctx->ref_cur;
        for (int k = 0; k < 3 && slot < 0; ++k) if (k != ctx->ref_cur && ctx->refbuf[k].users.load() == 0) slot = k;
        if (slot >= 0) break;
        if (waited > 600000) return fail(ctx, C3R_EINVAL, "all three reference buffers are held by row snapshots that were never released (c3r_rows_free)");
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    c3r_ctx::RefBuf &rb = ctx->refbuf[slot];
    if (!rb.ev) HIPCHK(ctx, hipEventCreateWithFlags(&rb.ev, hipEventDisableTiming));
    else HIPCHK(ctx, hipEventSynchronize(rb.ev));                 // (its previous upload has left the buffer)
    if ((size_t)len + 16 > rb.cap) {
        if (rb.p) (void)hipHostFree(rb.p);
        rb.p = nullptr; rb.cap = 0;
        const size_t cap = (size_t)len + (size_t)len / 8 + 4096;
        HIPCHK(ctx, hipHostMalloc((void **)&rb.p, cap, hipHostMallocDefault));
        rb.cap = cap;
    }
    ctx->ref_cur = slot; ctx->h_ref = rb.p;
    {
        char *dst = ctx->h_ref;
        auto upper = [&](int64_t a, int64_t e) {
            for (int64_t i = a; i < e; ++i) {        // branch-free, so the loop vectorises
                const unsigned char c = (unsigned char)ref[i];
                dst[i] = (char)(c - (((unsigned)(c - 'a') < 26u) << 5));
            }
        };
        // a 250 MB chromosome is memory-bound work for one core: split it
        int64_t nt = std::max<int64_t>(1, std::min<int64_t>({8, (int64_t)usable_cpus(), len >> 23}));
        if (const char *e = getenv("C3R_THREADS")) nt = std::max<int64_t>(1, std::min<int64_t>(nt, atoi(e)));
        std::vector<std::thread> th;
        for (int64_t t = 1; t < nt; ++t) th.emplace_back(upper, len * t / nt, len * (t + 1) / nt);
        upper(0, len / nt);
        for (auto &x : th) x.join();
    }
    ctx->ref_start1 = ref_start;
    int rc = ensure(ctx, ctx->d_ref, std::max<size_t>((size_t)len, 16));
    if (rc) return rc;
    if (len) HIPCHK(ctx, hipMemcpyAsync(ctx->d_ref.p, ctx->h_ref, (size_t)len, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(rb.ev, ctx->stream));
    ctx->ref_len = (size_t)len;
    return C3R_OK;
}

int c3r_set_reference_view(c3r_ctx *ctx, int64_t ref_start, const char *ref_upper, int64_t len) {
    if (!ctx || !ref_upper || len < 0 || ref_start < 1) return C3R_EINVAL;
    if (ref_start - 1 + len > INT32_MAX) return fail(ctx, C3R_EINVAL, "reference slice ends beyond 2^31");          // (the kernels index it by 32-bit offsets)
    ctx->last_scan_pruned = false;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // Nothing is copied on the host: the decoder reads the caller's bytes (kept alive and unchanged by the caller, see c3r.h) and the
    // upload takes them as they are — from pageable memory the runtime stages the copy itself and returns once the bytes have left.
    ctx->ref_len = 0;
    ctx->ref_cur = -1; ctx->h_ref = const_cast<char *>(ref_upper);
    ctx->ref_start1 = ref_start;
    int rc = ensure(ctx, ctx->d_ref, std::max<size_t>((size_t)len, 16));
    if (rc) return rc;
    if (len && (rc = big_h2d(ctx, ctx->d_ref.p, ref_upper, (size_t)len))) return rc;
    ctx->ref_len = (size_t)len;
    return C3R_OK;
}

int c3r_set_bed(c3r_ctx *ctx, int which, const int32_t *pairs, int64_t n) {
    if (!ctx || which < 0 || which > 1 || n < 0 || (n && !pairs)) return C3R_EINVAL;
    ctx->last_scan_pruned = false;       // (c3r_get_columns completes a pruned scan with the arguments of that scan: stale now)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->has_bed[which] = n > 0;
    ctx->h_bed[which].assign(pairs, pairs + 2 * n);
    merge_intervals(ctx->h_bed[which]);
    int rc = upload(ctx, ctx->d_bed[which], ctx->h_bed[which].data(), ctx->h_bed[which].size());
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}

int c3r_set_sites(c3r_ctx *ctx, const int32_t *sites, int64_t n) {
    if (!ctx || n < 0 || (n && !sites)) return C3R_EINVAL;
    ctx->last_scan_pruned = false;       // (c3r_get_columns completes a pruned scan with the arguments of that scan: stale now)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->h_sites.assign(sites, sites + n);
    std::sort(ctx->h_sites.begin(), ctx->h_sites.end());
    ctx->h_sites.erase(std::unique(ctx->h_sites.begin(), ctx->h_sites.end()), ctx->h_sites.end());
    int rc = upload(ctx, ctx->d_sites, ctx->h_sites.data(), ctx->h_sites.size());
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}

// The checks of a site table: `phased` = c3r_set_phase_sites (h1 and ps count), else c3r_phase_links (they are ignored).
static int check_phase_sites(c3r_ctx *ctx, const char *what, const c3r_phase_site_t *sites, int64_t n, bool phased) {
    if (n >= INT32_MAX) return fail(ctx, C3R_EINVAL, "too many %ss", what);
    for (int64_t i = 0; i < n; ++i) {
        const c3r_phase_site_t &e = sites[i];
        auto base = [](uint8_t c) { return c == 1 || c == 2 || c == 4 || c == 8; };
        if (e.pos < 1) return fail(ctx, C3R_EINVAL, "%s %lld: pos %d is not a 1-based position", what, (long long)i, e.pos);
        if (i > 0 && e.pos <= sites[i - 1].pos) return fail(ctx, C3R_EINVAL, "%s %lld: positions must be strictly increasing (%d after %d)", what, (long long)i, e.pos, sites[i - 1].pos);
        if (!base(e.ref) || !base(e.alt)) return fail(ctx, C3R_EINVAL, "%s %lld: ref / alt must be base codes 1, 2, 4 or 8 (got %d / %d)", what, (long long)i, e.ref, e.alt);
        if (e.ref == e.alt) return fail(ctx, C3R_EINVAL, "%s %lld: ref and alt are the same base", what, (long long)i);
        if (phased && e.h1 > 1) return fail(ctx, C3R_EINVAL, "%s %lld: h1 must be 0 (GT 0|1) or 1 (GT 1|0)", what, (long long)i);
        if (phased && e.ps < 0) return fail(ctx, C3R_EINVAL, "%s %lld: phase set %d is negative", what, (long long)i, e.ps);
    }
    return C3R_OK;
}

// The close of c3r_set_phase_sites and c3r_set_phase_alleles: the table on the device counts from here (one table at a time: either call
// replaces the other's), and the reads already loaded get their tables again, from the records the device holds (what c3r_set_params
// does for new filters).
static int phase_table_set(c3r_ctx *ctx, int64_t n, bool alleles) {
    ctx->n_phase = n;
    ctx->phase_alleles = alleles && n > 0;
    ctx->last_scan_pruned = false;
    ctx->host_cache.reset();
    return ::refilter(ctx);
}

int c3r_set_phase_sites(c3r_ctx *ctx, const c3r_phase_site_t *sites, int64_t n) {
    if (!ctx || n < 0 || (n && !sites)) return C3R_EINVAL;
    if (int rc = check_phase_sites(ctx, "phase site", sites, n, true)) return rc;
    if (n == 0 && ctx->n_phase == 0) return C3R_OK;               // (nothing set, nothing to clear: no copy, no wait, no rebuild)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n) {
        int rc = upload(ctx, ctx->d_phase, sites, (size_t)n);
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));           // (the caller's array may go once this returns)
    }
    return phase_table_set(ctx, n, false);
}

int c3r_phase_links(c3r_ctx *ctx, const c3r_phase_site_t *sites, int64_t n, uint32_t *links) {
    if (!ctx || n < 0 || (n && (!sites || !links))) return C3R_EINVAL;
    if (int rc = check_phase_sites(ctx, "candidate site", sites, n, false)) return rc;
    if (n == 0) return C3R_OK;
    const size_t words = (size_t)n * C3R_PHASE_LINKS * 2;
    if (ctx->n_reads == 0) { memset(links, 0, words * 4); return C3R_OK; }               // (no voters: nothing to launch)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = upload(ctx, ctx->d_plsites, sites, (size_t)n)) return rc;
    LinkArgs a = read_args<LinkArgs>(ctx, ctx->n_reads);
    a.sites = (const c3r_phase_site_t *)ctx->d_plsites.p; a.n_sites = (int32_t)n;
    a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags;
    return counter_table(ctx, ctx->d_links, words, links, [&](uint32_t *t) { a.links = t; launch_per_read(ctx, "k_phase_links", k_phase_links, a); });
}

int c3r_phase_resolve(const c3r_phase_site_t *in, int64_t n, const uint32_t *links, const c3r_phase_params_t *p, c3r_phase_site_t *out, c3r_phase_stats_t *stats) {
    if (n < 0 || (n && (!in || !links || !out))) return C3R_EINVAL;
    const int64_t min_reads = p ? p->min_reads : 2, pct = p ? p->min_agree_pct : 75;
    if (min_reads < 0 || pct < 0 || pct > 100) return C3R_EINVAL;
    for (int64_t j = 1; j < n; ++j) if (in[j].pos <= in[j - 1].pos) return C3R_EINVAL;
    constexpr int K = C3R_PHASE_LINKS;
    std::vector<int64_t> block((size_t)n), first, size;              // block of every site; per block: its first site, its sites
    std::vector<uint8_t> h1((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        // the blocks of the K predecessors, in the order of their nearest member (k ascending)
        int nb = 0;
        int64_t bid[K];
        uint64_t v0[K], v1[K];
        for (int k = 1; k <= K && k <= j; ++k) {
            const int64_t i = j - k;
            const uint64_t cis = links[((size_t)j * K + (size_t)(k - 1)) * 2], trans = links[((size_t)j * K + (size_t)(k - 1)) * 2 + 1];
            int b = 0;
            while (b < nb && bid[b] != block[(size_t)i]) ++b;
            if (b == nb) { bid[nb] = block[(size_t)i]; v0[nb] = 0; v1[nb] = 0; ++nb; }
            v1[b] += h1[(size_t)i] ? cis : trans;
            v0[b] += h1[(size_t)i] ? trans : cis;
        }
        int best = -1;
        uint64_t best_diff = 0;
        for (int b = 0; b < nb; ++b) {
            const uint64_t w = v0[b] + v1[b], hi = std::max(v0[b], v1[b]), diff = hi - std::min(v0[b], v1[b]);
            if (w < (uint64_t)min_reads || diff == 0 || 100 * hi < (uint64_t)pct * w) continue;
            if (best < 0 || diff > best_diff) { best = b; best_diff = diff; }          // (equal: the earlier entry holds the nearer predecessor)
        }
        if (best >= 0) { block[(size_t)j] = bid[best]; h1[(size_t)j] = v1[best] > v0[best] ? 1 : 0; size[(size_t)bid[best]] += 1; }
        else { block[(size_t)j] = (int64_t)first.size(); h1[(size_t)j] = 0; first.push_back(j); size.push_back(1); }
    }
    c3r_phase_stats_t st;
    memset(&st, 0, sizeof st);
    st.n_sites = n;
    for (size_t b = 0; b < size.size(); ++b) {
        if (size[b] >= 2) { st.n_blocks += 1; st.n_phased += size[b]; }
        st.max_block = std::max(st.max_block, size[b]);
    }
    for (int64_t j = 0; j < n; ++j) {
        const size_t b = (size_t)block[(size_t)j];
        c3r_phase_site_t e = in[j];
        const bool phased = size[b] >= 2;
        e.ps = phased ? in[first[b]].pos : -1;                       // (out == in: pos is written back unchanged)
        e.h1 = phased ? h1[(size_t)j] : 0;
        e.reserved = 0;
        out[j] = e;
    }
    if (stats) *stats = st;
    return C3R_OK;
}

// The units of the block-merge stage: the distinct ps >= 0 of a chain's table in increasing order (unit_ps), and every site's unit
// (unit_of, -1 for a singleton).  The table has been checked: ps is -1 or >= 1.
static void phase_units(const c3r_phase_site_t *sites, int64_t n, std::vector<int32_t> &unit_ps, std::vector<int32_t> &unit_of) {
    unit_ps.clear();
    for (int64_t j = 0; j < n; ++j) if (sites[j].ps >= 0) unit_ps.push_back(sites[j].ps);
    std::sort(unit_ps.begin(), unit_ps.end());
    unit_ps.erase(std::unique(unit_ps.begin(), unit_ps.end()), unit_ps.end());
    unit_of.assign((size_t)n, -1);
    for (int64_t j = 0; j < n; ++j)
        if (sites[j].ps >= 0) unit_of[(size_t)j] = (int32_t)(std::lower_bound(unit_ps.begin(), unit_ps.end(), sites[j].ps) - unit_ps.begin());
}

int c3r_phase_unit_links(c3r_ctx *ctx, const c3r_phase_site_t *sites, int64_t n, uint32_t *ulinks, int64_t cap_units, int64_t *n_units) {
    if (!ctx || n < 0 || cap_units < 0 || (n && !sites)) return C3R_EINVAL;
    if (int rc = check_phase_sites(ctx, "unit site", sites, n, false)) return rc;
    for (int64_t i = 0; i < n; ++i) {
        if (sites[i].ps != -1 && sites[i].ps < 1) return fail(ctx, C3R_EINVAL, "unit site %lld: ps %d is neither -1 (no block) nor a 1-based position", (long long)i, sites[i].ps);
        if (sites[i].h1 > 1) return fail(ctx, C3R_EINVAL, "unit site %lld: h1 must be 0 (GT 0|1) or 1 (GT 1|0)", (long long)i);
    }
    std::vector<int32_t> unit_ps, unit_of;
    phase_units(sites, n, unit_ps, unit_of);
    const int64_t U = (int64_t)unit_ps.size();
    if (n_units) *n_units = U;
    if (!ulinks) return C3R_OK;                                     // (the caller asks for the count)
    if (cap_units < U) return fail(ctx, C3R_EOVERFLOW, "the links of %lld units do not fit %lld slots", (long long)U, (long long)cap_units);
    const size_t words = (size_t)U * C3R_PHASE_LINKS * 2;
    if (U < 2 || ctx->n_reads == 0) { if (words) memset(ulinks, 0, words * 4); return C3R_OK; }      // (nothing to link, or no voters: nothing to launch)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = upload(ctx, ctx->d_plsites, sites, (size_t)n)) || (rc = upload(ctx, ctx->d_unitof, unit_of.data(), (size_t)n))) return rc;
    UnitLinkArgs a = read_args<UnitLinkArgs>(ctx, ctx->n_reads);
    a.sites = (const c3r_phase_site_t *)ctx->d_plsites.p; a.n_sites = (int32_t)n;
    a.unit_of = (const int32_t *)ctx->d_unitof.p; a.n_units = (int32_t)U;
    a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags;
    return counter_table(ctx, ctx->d_links, words, ulinks, [&](uint32_t *t) { a.ulinks = t; launch_per_read(ctx, "k_phase_unit_links", k_phase_unit_links, a); });   // (unit_of lives until it returns)
}

int c3r_phase_merge(const c3r_phase_site_t *in, int64_t n, const uint32_t *ulinks, int64_t n_units, const c3r_phase_params_t *p, c3r_phase_site_t *out,
                    c3r_phase_stats_t *stats, int64_t *n_joined) {
    if (n < 0 || n >= INT32_MAX || n_units < 0 || (n && (!in || !out)) || (n_units && !ulinks)) return C3R_EINVAL;
    for (int64_t j = 0; j < n; ++j)
        if ((j > 0 && in[j].pos <= in[j - 1].pos) || (in[j].ps != -1 && in[j].ps < 1) || in[j].h1 > 1) return C3R_EINVAL;
    std::vector<int32_t> unit_ps, unit_of;
    phase_units(in, n, unit_ps, unit_of);
    const size_t U = unit_ps.size();
    if ((int64_t)U != n_units) return C3R_EINVAL;
    // the chain's rule on the pseudo-table of units (pos = the unit's ps): one copy of the rule, c3r_phase_resolve
    std::vector<c3r_phase_site_t> unit(U);
    for (size_t u = 0; u < U; ++u) { memset(&unit[u], 0, sizeof unit[u]); unit[u].pos = unit_ps[u]; unit[u].ref = 1; unit[u].alt = 2; }
    if (int rc = c3r_phase_resolve(unit.data(), (int64_t)U, ulinks, p, unit.data(), nullptr)) return rc;
    int64_t joined = 0;
    for (size_t u = 0; u < U; ++u) if (unit[u].ps >= 0 && unit[u].ps != unit_ps[u]) joined += 1;
    for (int64_t j = 0; j < n; ++j) {
        c3r_phase_site_t e = in[j];
        const int32_t u = unit_of[(size_t)j];
        if (u >= 0 && unit[(size_t)u].ps >= 0) { e.ps = unit[(size_t)u].ps; e.h1 ^= unit[(size_t)u].h1; }
        e.reserved = 0;
        out[j] = e;
    }
    if (stats) {
        // from the final table: a block is a ps >= 0, whatever its size; max_block counts a site without one as a block of its own
        c3r_phase_stats_t st;
        memset(&st, 0, sizeof st);
        st.n_sites = n;
        std::vector<int32_t> ps;
        for (int64_t j = 0; j < n; ++j) { if (out[j].ps >= 0) ps.push_back(out[j].ps); else st.max_block = 1; }
        std::sort(ps.begin(), ps.end());
        st.n_phased = (int64_t)ps.size();
        for (size_t k = 0, k0 = 0; k <= ps.size(); ++k)
            if (k == ps.size() || ps[k] != ps[k0]) { if (k > k0) { st.n_blocks += 1; st.max_block = std::max(st.max_block, (int64_t)(k - k0)); } k0 = k; }
        *stats = st;
    }
    if (n_joined) *n_joined = joined;
    return C3R_OK;
}

int c3r_get_haplotags(c3r_ctx *ctx, uint8_t *hp, int64_t cap, c3r_haplotag_stats_t *stats) {
    if (!ctx) return C3R_EINVAL;
    if (ctx->n_phase == 0) return fail(ctx, C3R_EINVAL, "no phase sites are set (c3r_set_phase_sites / c3r_set_phase_alleles): the reads carry their records' own hp");
    const int64_t n = ctx->n_reads;
    if (hp && cap < n) return fail(ctx, C3R_EOVERFLOW, "haplotags of %lld reads do not fit %lld slots", (long long)n, (long long)cap);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> t((size_t)n);
    if (n) {
        HIPCHK(ctx, hipMemcpyAsync(t.data(), ctx->d_hptag.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    c3r_haplotag_stats_t st;
    memset(&st, 0, sizeof st);
    st.n_reads = n;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t tag = t[(size_t)i] & 3u, votes = t[(size_t)i] >> 2;
        if (hp) hp[i] = (uint8_t)tag;
        st.n_votes += votes;
        if (tag == 1) st.n_hp1 += 1; else if (tag == 2) st.n_hp2 += 1; else if (votes == 0) st.n_no_vote += 1; else st.n_tie += 1;
    }
    if (stats) *stats = st;
    return C3R_OK;
}

int c3r_get_read_phase_sets(c3r_ctx *ctx, int32_t *ps, int64_t cap) {
    if (!ctx || cap < 0) return C3R_EINVAL;
    if (ctx->n_phase == 0) return fail(ctx, C3R_EINVAL, "no phase sites are set (c3r_set_phase_sites / c3r_set_phase_alleles): the reads have no phase set");
    const int64_t n = ctx->n_reads;
    if (n && (!ps || cap < n)) return fail(ctx, C3R_EOVERFLOW, "phase sets of %lld reads do not fit %lld slots", (long long)n, (long long)cap);
    if (n == 0) return C3R_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(ps, ctx->d_hpps.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}

int c3r_hap_counts(c3r_ctx *ctx, const c3r_phase_site_t *sites, int64_t n, uint32_t *counts) {
    if (!ctx || n < 0 || (n && (!sites || !counts))) return C3R_EINVAL;
    if (int rc = check_phase_sites(ctx, "query site", sites, n, false)) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (sites[i].ps < 0) return fail(ctx, C3R_EINVAL, "query site %lld: phase set %d is negative", (long long)i, sites[i].ps);
    return hap_count_table(ctx, "k_hap_counts", k_hap_counts, n, counts, [&](HapCountArgs &a) {
        if (int rc = upload(ctx, ctx->d_hcsites, sites, (size_t)n)) return rc;
        a.sites = (const c3r_phase_site_t *)ctx->d_hcsites.p;
        return (int)C3R_OK;
    });
}

// The rule `hap_regions` of include/c3r.h: the table's checks, first_open and the bound on the host, then one launch of k_hap_region_counts.
int c3r_hap_region_counts(c3r_ctx *ctx, const c3r_hap_region_t *regions, int64_t n, const int32_t *row_ps, int64_t n_rows, int32_t stranded,
                          uint32_t *region_counts, uint32_t *row_counts) {
    if (!ctx || n < 0 || n_rows < 0 || (n && (!regions || !region_counts)) || (n_rows && (!row_ps || !row_counts))) return C3R_EINVAL;
    if (stranded < 0 || stranded > 2) return fail(ctx, C3R_EINVAL, "c3r_hap_region_counts: stranded %d is not 0 (off), 1 (same) or 2 (reverse)", stranded);
    if (n >= INT32_MAX / 2 || n_rows >= INT32_MAX / 2) return fail(ctx, C3R_EINVAL, "c3r_hap_region_counts: too many regions or rows");
    if (n == 0 && n_rows != 0) return fail(ctx, C3R_EINVAL, "c3r_hap_region_counts: %lld rows and no region", (long long)n_rows);
    std::vector<DevHapRegion> dev((size_t)n);
    std::vector<int32_t> first_open((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        const c3r_hap_region_t &e = regions[j];
        int64_t row_end = 0;
        if (int rc = check_interval(ctx, "region", "; count long and short regions (genes and exons) in separate calls", regions, j, first_open, [&] {
                return check_row_run(ctx, "region", "row_off", [&](int64_t g) { return regions[g].row_off; }, j, n, row_ps, n_rows, &row_end);
            })) return rc;
        DevHapRegion &o = dev[(size_t)j];
        o.start = e.start; o.end = e.end; o.row_off = e.row_off; o.strand_rows = (uint32_t)e.strand | ((uint32_t)(row_end - e.row_off) << 8);
    }
    return hap_interval_table<HapRegionArgs>(ctx, dev, first_open, {}, row_ps, n, n_rows, stranded, region_counts, row_counts,
                                             [&](const HapRegionArgs &a) { launch_per_read(ctx, "k_hap_region_counts", k_hap_region_counts, a); });
}

// The rule `hap_groups` of include/c3r.h: the table's checks, first_open, the bound and every interval's predecessor in its group on the
// host, then one launch of k_hap_group_counts.
int c3r_hap_group_counts(c3r_ctx *ctx, const c3r_hap_interval_t *intervals, int64_t n, int64_t n_groups, const int32_t *group_row_off,
                         const int32_t *row_ps, int64_t n_rows, int32_t stranded, uint32_t *group_counts, uint32_t *row_counts) {
    if (!ctx || n < 0 || n_groups < 0 || n_rows < 0 || (n && !intervals) || (n_groups && (!group_row_off || !group_counts)) || (n_rows && (!row_ps || !row_counts))) return C3R_EINVAL;
    if (stranded < 0 || stranded > 2) return fail(ctx, C3R_EINVAL, "c3r_hap_group_counts: stranded %d is not 0 (off), 1 (same) or 2 (reverse)", stranded);
    if (n >= INT32_MAX / 2 || n_groups >= INT32_MAX / 2 || n_rows >= INT32_MAX / 2) return fail(ctx, C3R_EINVAL, "c3r_hap_group_counts: too many intervals, groups or rows");
    if (n == 0 && (n_groups != 0 || n_rows != 0)) return fail(ctx, C3R_EINVAL, "c3r_hap_group_counts: %lld groups, %lld rows and no interval", (long long)n_groups, (long long)n_rows);
    std::vector<DevHapInterval> dev((size_t)n);
    std::vector<int32_t> first_open((size_t)n), last_of((size_t)n_groups, -1), off((size_t)n_groups + 1);
    for (int64_t j = 0; j < n; ++j) {
        const c3r_hap_interval_t &e = intervals[j];
        int32_t prev = -1;
        if (int rc = check_interval(ctx, "interval", "", intervals, j, first_open, [&] {
                if (e.group < 0 || (int64_t)e.group >= n_groups) return fail(ctx, C3R_EINVAL, "interval %lld: group %d is not in [0, %lld)", (long long)j, e.group, (long long)n_groups);
                // the group's previous interval in table order: starts never decrease and the group's earlier intervals are disjoint, so it
                // holds the group's largest end, and this interval overlaps one of them iff it starts before that end
                prev = last_of[(size_t)e.group];
                if (prev >= 0 && intervals[prev].end > e.start)
                    return fail(ctx, C3R_EINVAL, "interval %lld: [%d, %d) overlaps interval %d, [%d, %d), of the same group %d: the intervals of a group must be disjoint (merge them)",
                                (long long)j, e.start, e.end, prev, intervals[prev].start, intervals[prev].end, e.group);
                if (prev >= 0 && intervals[prev].strand != e.strand)
                    return fail(ctx, C3R_EINVAL, "interval %lld: strand %d, and interval %d of the same group %d has strand %d: a group carries one strand", (long long)j, e.strand, prev, e.group, intervals[prev].strand);
                last_of[(size_t)e.group] = (int32_t)j;
                return (int)C3R_OK;
            })) return rc;
        DevHapInterval &o = dev[(size_t)j];
        o.start = e.start; o.end = e.end; o.prev = prev; o.group_strand = ((uint32_t)e.group << 2) | (uint32_t)e.strand;
    }
    for (int64_t g = 0; g < n_groups; ++g) {
        if (last_of[(size_t)g] < 0) return fail(ctx, C3R_EINVAL, "group %lld: no interval of the table belongs to it", (long long)g);
        int64_t row_end;
        if (int rc = check_row_run(ctx, "group", "group_row_off", [&](int64_t k) { return group_row_off[k]; }, g, n_groups, row_ps, n_rows, &row_end)) return rc;
        off[(size_t)g] = group_row_off[g];
    }
    off[(size_t)n_groups] = (int32_t)n_rows;
    return hap_interval_table<HapGroupArgs>(ctx, dev, first_open, off, row_ps, n_groups, n_rows, stranded, group_counts, row_counts, [&](HapGroupArgs &a) {
        a.group_row_off = (const int32_t *)ctx->d_hioff.p;
        if (ctx->hg_direct) launch_per_read(ctx, "k_hap_group_counts_direct", k_hap_group_counts<false>, a);
        else launch_per_read(ctx, "k_hap_group_counts", k_hap_group_counts<true>, a);
    });
}

int c3r_set_hap_group_direct(c3r_ctx *ctx, int on) {
    if (!ctx) return C3R_EINVAL;
    if (on != 0 && on != 1) return fail(ctx, C3R_EINVAL, "c3r_set_hap_group_direct: %d is neither 0 nor 1", on);
    ctx->hg_direct = on != 0;
    return C3R_OK;
}

int c3r_get_hap_group_direct(c3r_ctx *ctx, int *on) {
    if (!ctx || !on) return C3R_EINVAL;
    *on = ctx->hg_direct ? 1 : 0;
    return C3R_OK;
}

// The rule `hap_junctions` of include/c3r.h: k_hap_junction_counts into the two hash tables, the scan allocator's grow-and-repeat when one
// of them had no place for a key, then the tables compacted and sorted on the host into the context.
int c3r_hap_junction_counts(c3r_ctx *ctx, int64_t slots_hint, int64_t *n_junctions, int64_t *n_rows) {
    if (!ctx || !n_junctions || !n_rows) return C3R_EINVAL;
    if (slots_hint < 0) return fail(ctx, C3R_EINVAL, "c3r_hap_junction_counts: slots_hint %lld is negative", (long long)slots_hint);
    ctx->hj_valid = false; ctx->hj_junctions.clear(); ctx->hj_rows.clear();
    *n_junctions = 0; *n_rows = 0;
    if (ctx->n_reads == 0) { ctx->hj_valid = true; return C3R_OK; }              // (no reads: nothing to launch)
    uint32_t jlog = HJ_MIN_LOG;
    while (jlog < (uint32_t)HJ_MAX_LOG && ((int64_t)1 << jlog) < (slots_hint ? slots_hint : (int64_t)C3R_HAP_JUNCTION_SLOTS)) ++jlog;
    uint32_t rlog = jlog;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HapJunctionArgs a = read_args<HapJunctionArgs>(ctx, ctx->n_reads);
    if (ctx->n_phase > 0) { a.tags = (const uint32_t *)ctx->d_hptag.p; a.read_ps = (const int32_t *)ctx->d_hpps.p; }       // (else null: every read is untagged)
    a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags;
    int rc;
    if ((rc = ensure(ctx, ctx->d_hjover, 16))) return rc;
    for (int round = 0;; ++round) {
        const size_t js = (size_t)1 << jlog, rs = (size_t)1 << rlog;
        if ((rc = ensure(ctx, ctx->d_hjtab, js * 20)) || (rc = ensure(ctx, ctx->d_hjrows, rs * 16))) return rc;
        a.jkeys = (unsigned long long *)ctx->d_hjtab.p; a.jcounts = (uint32_t *)((char *)ctx->d_hjtab.p + js * 8); a.jlog = jlog;
        a.rkeys = (unsigned long long *)ctx->d_hjrows.p; a.rcounts = (uint32_t *)((char *)ctx->d_hjrows.p + rs * 8); a.rlog = rlog;
        a.overflow = (uint32_t *)ctx->d_hjover.p;
        HIPCHK(ctx, hipMemsetAsync(a.jkeys, 0xff, js * 8, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(a.jcounts, 0, js * 12, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(a.rkeys, 0xff, rs * 8, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(a.rcounts, 0, rs * 8, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(a.overflow, 0, 4, ctx->stream));
        if (ctx->hj_direct) launch_per_read(ctx, "k_hap_junction_counts_direct", k_hap_junction_counts<false>, a);
        else launch_per_read(ctx, "k_hap_junction_counts", k_hap_junction_counts<true>, a);
        HIPCHK(ctx, hipGetLastError());
        uint32_t over = 0;
        HIPCHK(ctx, hipMemcpyAsync(&over, a.overflow, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (!over) break;
        if (over & HJ_OVER_JUNCTIONS) ++jlog;
        if (over & HJ_OVER_ROWS) ++rlog;
        if (round + 1 >= C3R_HAP_JUNCTION_MAX_ROUNDS || jlog > (uint32_t)HJ_MAX_LOG || rlog > (uint32_t)HJ_MAX_LOG)
            return fail(ctx, C3R_EOVERFLOW, "c3r_hap_junction_counts: the tables still had no place for a key after %d launches (2^%u junction slots, 2^%u row slots)",
                        round + 1, jlog, rlog);
    }
    // the tables as they are, then: occupied slots in key order — (start << 32) | end of non-negative positions orders by (start, end).
    // (The host's copies are as large as the tables: one that does not fit the host's memory is C3R_ENOMEM, not an exception through the C ABI.)
    try {
    const size_t js = (size_t)1 << jlog, rs = (size_t)1 << rlog;
    std::vector<unsigned long long> jt(js * 5 / 2 + 1), rt(rs * 2);
    HIPCHK(ctx, hipMemcpyAsync(jt.data(), ctx->d_hjtab.p, js * 20, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(rt.data(), ctx->d_hjrows.p, rs * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t *jc = (const uint32_t *)(jt.data() + js), *rcn = (const uint32_t *)(rt.data() + rs);
    std::vector<std::pair<unsigned long long, uint32_t>> order;                 // (key, slot)
    for (size_t s = 0; s < js; ++s) if (jt[s] != HJ_EMPTY) order.push_back({jt[s], (uint32_t)s});
    std::sort(order.begin(), order.end());
    std::vector<int32_t> rank(js, -1);
    ctx->hj_junctions.resize(order.size());
    for (size_t j = 0; j < order.size(); ++j) {
        const uint32_t s = order[j].second;
        rank[s] = (int32_t)j;
        c3r_hap_junction_t &o = ctx->hj_junctions[j];
        o.start = (int32_t)(order[j].first >> 32); o.end = (int32_t)(uint32_t)order[j].first;
        o.reads = jc[3 * (size_t)s]; o.reverse = jc[3 * (size_t)s + 1]; o.untagged = jc[3 * (size_t)s + 2]; o.row_off = 0;
    }
    std::vector<std::pair<std::pair<int32_t, int32_t>, uint32_t>> rows;        // ((junction, ps), slot)
    for (size_t s = 0; s < rs; ++s) {
        if (rt[s] == HJ_EMPTY) continue;
        const uint64_t slot = rt[s] >> 32;
        if (slot >= js || rank[slot] < 0) return fail(ctx, C3R_EHIP, "internal: a row of the junction table names slot %llu, which holds no junction", (unsigned long long)slot);
        rows.push_back({{rank[slot], (int32_t)(uint32_t)rt[s]}, (uint32_t)s});
    }
    std::sort(rows.begin(), rows.end());
    ctx->hj_rows.resize(rows.size());
    size_t r = 0;
    for (size_t j = 0; j < order.size(); ++j) {
        ctx->hj_junctions[j].row_off = (int32_t)r;
        for (; r < rows.size() && (size_t)rows[r].first.first == j; ++r) {
            c3r_hap_junction_row_t &o = ctx->hj_rows[r];
            o.ps = rows[r].first.second; o.hp1 = rcn[2 * (size_t)rows[r].second]; o.hp2 = rcn[2 * (size_t)rows[r].second + 1];
        }
    }
    } catch (const std::bad_alloc &) {
        ctx->hj_junctions.clear(); ctx->hj_rows.clear();
        return fail(ctx, C3R_ENOMEM, "c3r_hap_junction_counts: no host memory for the copies of the tables (2^%u junction slots, 2^%u row slots)", jlog, rlog);
    }
    ctx->hj_valid = true;
    *n_junctions = (int64_t)ctx->hj_junctions.size(); *n_rows = (int64_t)ctx->hj_rows.size();
    return C3R_OK;
}

int c3r_get_hap_junctions(c3r_ctx *ctx, c3r_hap_junction_t *junctions, int64_t cap_j, c3r_hap_junction_row_t *rows, int64_t cap_r) {
    if (!ctx || cap_j < 0 || cap_r < 0) return C3R_EINVAL;
    if (!ctx->hj_valid) return fail(ctx, C3R_EINVAL, "c3r_get_hap_junctions: nothing has been counted since the last c3r_load_reads (c3r_hap_junction_counts)");
    const size_t nj = ctx->hj_junctions.size(), nr = ctx->hj_rows.size();
    if ((nj && (!junctions || (size_t)cap_j < nj)) || (nr && (!rows || (size_t)cap_r < nr)))
        return fail(ctx, C3R_EINVAL, "c3r_get_hap_junctions: %zu junctions and %zu rows do not fit %lld and %lld slots", nj, nr, (long long)cap_j, (long long)cap_r);
    if (nj) memcpy(junctions, ctx->hj_junctions.data(), nj * sizeof(c3r_hap_junction_t));
    if (nr) memcpy(rows, ctx->hj_rows.data(), nr * sizeof(c3r_hap_junction_row_t));
    return C3R_OK;
}

int c3r_set_hap_junction_direct(c3r_ctx *ctx, int on) {
    if (!ctx) return C3R_EINVAL;
    if (on != 0 && on != 1) return fail(ctx, C3R_EINVAL, "c3r_set_hap_junction_direct: %d is neither 0 nor 1", on);
    ctx->hj_direct = on != 0;
    return C3R_OK;
}

// The checks of a table of c3r_hap_site_t: c3r_hap_allele_counts' (h1 = NULL) and c3r_set_phase_alleles' (the same and h1 <= 1).  any_ps:
// ps is not looked at (c3r_phase_allele_links, which ignores it, and c3r_phase_allele_unit_links, which has a rule of its own for it).
static int check_hap_sites(c3r_ctx *ctx, const char *what, const c3r_hap_site_t *sites, int64_t n, const uint8_t *ins_pool, int64_t pool_bases, const uint8_t *h1, bool any_ps = false) {
    if (n >= INT32_MAX) return fail(ctx, C3R_EINVAL, "too many %ss", what);
    auto base = [](uint8_t c) { return c == 1 || c == 2 || c == 4 || c == 8; };
    auto pool_at = [&](uint64_t q) { const uint8_t byte = ins_pool[q >> 1]; return (uint8_t)((q & 1) ? (byte & 15) : (byte >> 4)); };
    for (int64_t i = 0; i < n; ++i) {
        const c3r_hap_site_t &e = sites[i];
        if (e.pos < 1) return fail(ctx, C3R_EINVAL, "%s %lld: pos %d is not a 1-based position", what, (long long)i, e.pos);
        if (i > 0 && e.pos <= sites[i - 1].pos) return fail(ctx, C3R_EINVAL, "%s %lld: positions must be strictly increasing (%d after %d)", what, (long long)i, e.pos, sites[i - 1].pos);
        if (!any_ps && e.ps < 0) return fail(ctx, C3R_EINVAL, "%s %lld: phase set %d is negative", what, (long long)i, e.ps);
        if (e.base_matters > 1 || e.event_matters > 1) return fail(ctx, C3R_EINVAL, "%s %lld: base_matters / event_matters must be 0 or 1", what, (long long)i);
        for (const c3r_hap_allele_t *al : {&e.a, &e.b}) {
            const char which = al == &e.a ? 'A' : 'B';
            if (!base(al->base)) return fail(ctx, C3R_EINVAL, "%s %lld: allele %c: the base must be a code 1, 2, 4 or 8 (got %d)", what, (long long)i, which, al->base);
            if (al->kind > C3R_HAP_EV_DEL) return fail(ctx, C3R_EINVAL, "%s %lld: allele %c: unknown kind %d", what, (long long)i, which, al->kind);
            if (al->kind == C3R_HAP_EV_NONE ? al->len != 0 : al->len == 0)
                return fail(ctx, C3R_EINVAL, "%s %lld: allele %c: an insertion or deletion has a length of 1 or more, any other allele 0 (got %d)", what, (long long)i, which, al->len);
            if (al->kind == C3R_HAP_EV_INS) {
                if ((int64_t)al->ins_off + al->len > pool_bases)
                    return fail(ctx, C3R_EINVAL, "%s %lld: allele %c: the insertion (%u + %d bases) runs past the pool of %lld bases", what, (long long)i, which, al->ins_off, al->len, (long long)pool_bases);
                for (uint32_t j = 0; j < al->len; ++j)
                    if (!base(pool_at((uint64_t)al->ins_off + j)))
                        return fail(ctx, C3R_EINVAL, "%s %lld: allele %c: inserted base %u must be a code 1, 2, 4 or 8 (got %d)", what, (long long)i, which, j, pool_at((uint64_t)al->ins_off + j));
            }
        }
        bool same = e.a.base == e.b.base && e.a.kind == e.b.kind && e.a.len == e.b.len;
        if (same && e.a.kind == C3R_HAP_EV_INS)
            for (uint32_t j = 0; j < e.a.len && same; ++j) same = pool_at((uint64_t)e.a.ins_off + j) == pool_at((uint64_t)e.b.ins_off + j);
        if (same) return fail(ctx, C3R_EINVAL, "%s %lld: the two alleles are the same", what, (long long)i);
        if (h1 && h1[i] > 1) return fail(ctx, C3R_EINVAL, "%s %lld: h1 must be 0 (allele A on haplotype 1) or 1 (allele B on haplotype 1)", what, (long long)i);
    }
    return C3R_OK;
}

int c3r_set_phase_alleles(c3r_ctx *ctx, const c3r_hap_site_t *sites, const uint8_t *h1, int64_t n, const uint8_t *ins_pool, int64_t pool_bases) {
    if (!ctx || n < 0 || pool_bases < 0 || (n && (!sites || !h1)) || (pool_bases && !ins_pool)) return C3R_EINVAL;
    if (int rc = check_hap_sites(ctx, "phase allele site", sites, n, ins_pool, pool_bases, h1)) return rc;
    if (n) if (int rc = hap_needs_ref(ctx, "c3r_set_phase_alleles")) return rc;
    if (n == 0 && ctx->n_phase == 0) return C3R_OK;               // (nothing set, nothing to clear: no copy, no wait, no rebuild)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n) {
        std::vector<c3r_hap_site_t> t(sites, sites + n);          // the device's table: h1 rides in reserved[0], the rest of `reserved` is 0
        for (int64_t i = 0; i < n; ++i) { memset(t[(size_t)i].reserved, 0, sizeof t[(size_t)i].reserved); t[(size_t)i].reserved[0] = h1[i]; }
        // From here on the buffers of an allele table set before are being overwritten: a device failure (C3R_ENOMEM, C3R_EHIP) must not leave
        // half of the new table under the old count, so the context holds NO table until both copies have landed.
        if (ctx->phase_alleles) { ctx->n_phase = 0; ctx->phase_alleles = false; }
        int rc;
        if ((rc = upload(ctx, ctx->d_phasea, t.data(), (size_t)n)) || (rc = upload(ctx, ctx->d_phasepool, ins_pool, (size_t)((pool_bases + 1) / 2)))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));           // (the caller's arrays, and `t`, may go once this returns)
    }
    return phase_table_set(ctx, n, true);
}

int c3r_hap_allele_counts(c3r_ctx *ctx, const c3r_hap_site_t *sites, int64_t n, const uint8_t *ins_pool, int64_t pool_bases, uint32_t *counts) {
    if (!ctx || n < 0 || pool_bases < 0 || (n && (!sites || !counts)) || (pool_bases && !ins_pool)) return C3R_EINVAL;
    if (int rc = check_hap_sites(ctx, "query site", sites, n, ins_pool, pool_bases, nullptr)) return rc;
    if (int rc = hap_needs_ref(ctx, "c3r_hap_allele_counts")) return rc;
    auto upload_sites = [&](HapAlleleArgs &a) {
        int rc;
        if ((rc = upload(ctx, ctx->d_hasites, sites, (size_t)n)) || (rc = upload(ctx, ctx->d_hapool, ins_pool, (size_t)((pool_bases + 1) / 2)))) return rc;
        a.sites = (const c3r_hap_site_t *)ctx->d_hasites.p; a.pool = (const uint8_t *)ctx->d_hapool.p;
        return (int)C3R_OK;
    };
    if (ctx->hap_ra > 0 && ctx->hap_rs)
        return hap_count_table(ctx, "k_hap_allele_counts_rs", k_hap_allele_counts_rs, n, counts, [&](HapAlleleRaArgs &a) { a.ref = hap_ref(ctx); a.overhang = (uint32_t)ctx->hap_ra; return upload_sites(a); });
    if (ctx->hap_ra > 0)
        return hap_count_table(ctx, "k_hap_allele_counts_ra", k_hap_allele_counts_ra, n, counts, [&](HapAlleleRaArgs &a) { a.ref = hap_ref(ctx); a.overhang = (uint32_t)ctx->hap_ra; return upload_sites(a); });
    if (ctx->hap_la) return hap_count_table(ctx, "k_hap_allele_counts_la", k_hap_allele_counts_la, n, counts, [&](HapAlleleLaArgs &a) { a.ref = hap_ref(ctx); return upload_sites(a); });
    return hap_count_table(ctx, "k_hap_allele_counts", k_hap_allele_counts, n, counts, upload_sites);
}

int c3r_phase_allele_links(c3r_ctx *ctx, const c3r_hap_site_t *sites, int64_t n, const uint8_t *ins_pool, int64_t pool_bases, uint32_t *links) {
    if (!ctx || n < 0 || pool_bases < 0 || (n && (!sites || !links)) || (pool_bases && !ins_pool)) return C3R_EINVAL;
    if (int rc = check_hap_sites(ctx, "candidate site", sites, n, ins_pool, pool_bases, nullptr, true)) return rc;
    if (int rc = hap_needs_ref(ctx, "c3r_phase_allele_links")) return rc;
    if (n == 0) return C3R_OK;
    const size_t words = (size_t)n * C3R_PHASE_LINKS * 2;
    if (ctx->n_reads == 0) { memset(links, 0, words * 4); return C3R_OK; }               // (no voters: nothing to launch)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = upload(ctx, ctx->d_pasites, sites, (size_t)n)) || (rc = upload(ctx, ctx->d_papool, ins_pool, (size_t)((pool_bases + 1) / 2)))) return rc;
    AlleleLinkRaArgs a = read_args<AlleleLinkRaArgs>(ctx, ctx->n_reads);
    a.sites = (const c3r_hap_site_t *)ctx->d_pasites.p; a.n_sites = (int32_t)n; a.pool = (const uint8_t *)ctx->d_papool.p;
    a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags;
    if (ctx->hap_la || ctx->hap_ra > 0) a.ref = hap_ref(ctx);
    a.overhang = (uint32_t)ctx->hap_ra;
    return counter_table(ctx, ctx->d_links, words, links, [&](uint32_t *t) {
        a.links = t;
        if (ctx->hap_ra > 0 && ctx->hap_rs) launch_per_read(ctx, "k_phase_allele_links_rs", k_phase_allele_links_rs, a);
        else if (ctx->hap_ra > 0) launch_per_read(ctx, "k_phase_allele_links_ra", k_phase_allele_links_ra, a);
        else if (ctx->hap_la) launch_per_read<AlleleLinkLaArgs>(ctx, "k_phase_allele_links_la", k_phase_allele_links_la, a);
        else launch_per_read<AlleleLinkArgs>(ctx, "k_phase_allele_links", k_phase_allele_links, a);
    });
}

int c3r_phase_allele_unit_links(c3r_ctx *ctx, const c3r_hap_site_t *sites, const uint8_t *h1, int64_t n, const uint8_t *ins_pool, int64_t pool_bases, uint32_t *ulinks,
                                int64_t cap_units, int64_t *n_units) {
    if (!ctx || n < 0 || pool_bases < 0 || cap_units < 0 || (n && (!sites || !h1)) || (pool_bases && !ins_pool)) return C3R_EINVAL;
    if (int rc = check_hap_sites(ctx, "unit site", sites, n, ins_pool, pool_bases, h1, true)) return rc;
    if (int rc = hap_needs_ref(ctx, "c3r_phase_allele_unit_links")) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (sites[i].ps != -1 && sites[i].ps < 1) return fail(ctx, C3R_EINVAL, "unit site %lld: ps %d is neither -1 (no block) nor a 1-based position", (long long)i, sites[i].ps);
    std::vector<int32_t> unit_ps, unit_of;
    {
        std::vector<c3r_phase_site_t> pseudo((size_t)n);            // phase_units reads ps only
        for (int64_t i = 0; i < n; ++i) { memset(&pseudo[(size_t)i], 0, sizeof pseudo[0]); pseudo[(size_t)i].pos = sites[i].pos; pseudo[(size_t)i].ps = sites[i].ps; }
        phase_units(pseudo.data(), n, unit_ps, unit_of);
    }
    const int64_t U = (int64_t)unit_ps.size();
    if (n_units) *n_units = U;
    if (!ulinks) return C3R_OK;                                     // (the caller asks for the count)
    if (cap_units < U) return fail(ctx, C3R_EOVERFLOW, "the links of %lld units do not fit %lld slots", (long long)U, (long long)cap_units);
    const size_t words = (size_t)U * C3R_PHASE_LINKS * 2;
    if (U < 2 || ctx->n_reads == 0) { if (words) memset(ulinks, 0, words * 4); return C3R_OK; }      // (nothing to link, or no voters: nothing to launch)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<c3r_hap_site_t> t(sites, sites + n);                // the device's table: h1 rides in reserved[0], as in c3r_set_phase_alleles
    for (int64_t i = 0; i < n; ++i) { memset(t[(size_t)i].reserved, 0, sizeof t[(size_t)i].reserved); t[(size_t)i].reserved[0] = h1[i]; }
    int rc;
    if ((rc = upload(ctx, ctx->d_pasites, t.data(), (size_t)n)) || (rc = upload(ctx, ctx->d_papool, ins_pool, (size_t)((pool_bases + 1) / 2))) ||
        (rc = upload(ctx, ctx->d_unitof, unit_of.data(), (size_t)n))) return rc;
    AlleleUnitLinkRaArgs a = read_args<AlleleUnitLinkRaArgs>(ctx, ctx->n_reads);
    a.sites = (const c3r_hap_site_t *)ctx->d_pasites.p; a.n_sites = (int32_t)n; a.pool = (const uint8_t *)ctx->d_papool.p;
    a.unit_of = (const int32_t *)ctx->d_unitof.p; a.n_units = (int32_t)U;
    a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags;
    if (ctx->hap_la || ctx->hap_ra > 0) a.ref = hap_ref(ctx);
    a.overhang = (uint32_t)ctx->hap_ra;
    return counter_table(ctx, ctx->d_links, words, ulinks, [&](uint32_t *t2) {                                  // (t and unit_of live until it returns)
        a.ulinks = t2;
        if (ctx->hap_ra > 0 && ctx->hap_rs) launch_per_read(ctx, "k_phase_allele_unit_links_rs", k_phase_allele_unit_links_rs, a);
        else if (ctx->hap_ra > 0) launch_per_read(ctx, "k_phase_allele_unit_links_ra", k_phase_allele_unit_links_ra, a);
        else if (ctx->hap_la) launch_per_read<AlleleUnitLinkLaArgs>(ctx, "k_phase_allele_unit_links_la", k_phase_allele_unit_links_la, a);
        else launch_per_read<AlleleUnitLinkArgs>(ctx, "k_phase_allele_unit_links", k_phase_allele_unit_links, a);
    });
}

int c3r_set_hap_left_align(c3r_ctx *ctx, int on) {
    if (!ctx) return C3R_EINVAL;
    const bool want = on != 0;
    if (want == ctx->hap_la) return C3R_OK;
    if (want && ctx->hap_ra > 0) return fail(ctx, C3R_EINVAL, "c3r_set_hap_left_align: c3r_set_hap_realign is on (%d); the two exclude each other", ctx->hap_ra);
    const bool retag = ctx->phase_alleles && ctx->n_reads > 0;    // the tags on the device are those of the other observation
    if (retag && want && ctx->ref_len == 0)
        return fail(ctx, C3R_EINVAL, "c3r_set_hap_left_align: an allele table is set and reads are loaded, and no reference is set (c3r_set_reference)");
    ctx->hap_la = want;
    if (!retag) return C3R_OK;
    ctx->last_scan_pruned = false;
    ctx->host_cache.reset();
    return ::refilter(ctx);
}

int c3r_set_hap_realign(c3r_ctx *ctx, int overhang) {
    if (!ctx) return C3R_EINVAL;
    if (overhang < 0 || overhang > (int)RA_MAX_W) return fail(ctx, C3R_EINVAL, "c3r_set_hap_realign: overhang %d is outside 0 .. %d", overhang, (int)RA_MAX_W);
    if (overhang == ctx->hap_ra) return C3R_OK;
    if (overhang > 0 && ctx->hap_la) return fail(ctx, C3R_EINVAL, "c3r_set_hap_realign: c3r_set_hap_left_align is on; the two exclude each other");
    const bool retag = ctx->phase_alleles && ctx->n_reads > 0;    // the tags on the device are those of another observation
    if (retag && overhang > 0 && ctx->ref_len == 0)
        return fail(ctx, C3R_EINVAL, "c3r_set_hap_realign: an allele table is set and reads are loaded, and no reference is set (c3r_set_reference)");
    ctx->hap_ra = overhang;
    if (!retag) return C3R_OK;
    ctx->last_scan_pruned = false;
    ctx->host_cache.reset();
    return ::refilter(ctx);
}

int c3r_get_hap_realign(c3r_ctx *ctx, int *overhang) {
    if (!ctx) return C3R_EINVAL;
    if (overhang) *overhang = ctx->hap_ra;
    return C3R_OK;
}

int c3r_set_hap_realign_spliced(c3r_ctx *ctx, int on) {
    if (!ctx) return C3R_EINVAL;
    if (on != 0 && on != 1) return fail(ctx, C3R_EINVAL, "c3r_set_hap_realign_spliced: %d is neither 0 nor 1", on);
    const bool want = on != 0;
    if (want == ctx->hap_rs) return C3R_OK;
    const bool retag = ctx->hap_ra > 0 && ctx->phase_alleles && ctx->n_reads > 0;       // the tags on the device are those of the other window
    if (retag && ctx->ref_len == 0)
        return fail(ctx, C3R_EINVAL, "c3r_set_hap_realign_spliced: an allele table is set and reads are loaded, and no reference is set (c3r_set_reference)");
    ctx->hap_rs = want;
    if (!retag) return C3R_OK;
    ctx->last_scan_pruned = false;
    ctx->host_cache.reset();
    return ::refilter(ctx);
}

int c3r_get_hap_realign_spliced(c3r_ctx *ctx, int *on) {
    if (!ctx) return C3R_EINVAL;
    if (on) *on = ctx->hap_rs ? 1 : 0;
    return C3R_OK;
}

// The rules `realign` and `realign_spliced` of include/c3r.h for one read at one site on the host: the serial walk finds the M op of the
// normalised CIGAR that holds the anchor, as walk_sites does, and hap_observe_ra / hap_observe_rs — the functions the _ra and the _rs
// kernels call — decide there.
int c3r_hap_realign_column(const c3r_hap_site_t *site, const uint8_t *ins_pool, int64_t ref_start, const char *ref, int64_t ref_len, const c3r_read_t *read,
                           const uint32_t *cigars, const uint8_t *seq4, int overhang, int *column, int *realigned) {
    return c3r_hap_realign_column_spliced(site, ins_pool, ref_start, ref, ref_len, read, cigars, seq4, overhang, 0, column, realigned);
}

int c3r_hap_realign_column_spliced(const c3r_hap_site_t *site, const uint8_t *ins_pool, int64_t ref_start, const char *ref, int64_t ref_len, const c3r_read_t *read,
                                   const uint32_t *cigars, const uint8_t *seq4, int overhang, int spliced, int *column, int *realigned) {
    if (!site || (spliced != 0 && spliced != 1) || !read || !column || ref_len < 0 || ref_start < 1 || (ref_len && !ref) || (read->n_cigar && !cigars) || (read->l_seq && !seq4) || overhang < 0 ||
        overhang > (int)RA_MAX_W || site->pos < 1)
        return C3R_EINVAL;
    const c3r_hap_allele_t *al[2] = {&site->a, &site->b};
    for (int w = 0; w < 2; ++w)
        if (al[w]->kind > C3R_HAP_EV_DEL || (al[w]->kind == C3R_HAP_EV_NONE ? al[w]->len != 0 : al[w]->len == 0) || (al[w]->kind == C3R_HAP_EV_INS && !ins_pool)) return C3R_EINVAL;
    struct HostRef {                                               // HapRef on the caller's letters, any case
        const char *ref; int64_t beg0, len;
        uint32_t code(long long p) const {
            const long long o = p - beg0;
            if (o < 0 || o >= len) return 0u;
            switch (ref[o]) { case 'A': case 'a': return 1u; case 'C': case 'c': return 2u; case 'G': case 'g': return 4u; case 'T': case 't': return 8u; default: return 0u; }
        }
    };
    const HostRef R{ref, ref_start - 1, ref_len};
    ReadInfo ri;
    ri.cig = cigars ? cigars + read->cigar_off : nullptr; ri.pos = read->pos; ri.n_cig = read->n_cigar; ri.l_seq = read->l_seq; ri.read_idx = 0; ri.wbits = 0;
    ri.seq_off = read->seq_off; ri.compat = 0; ri.padbit = 0;
    const uint8_t *rseq = seq4 ? seq4 + read->seq_off : nullptr;
    uint32_t col = HAP_NOTHING;
    bool ra = false;
    const c3r_hap_site_t e = *site;
    const int err = walk_serial_ops(ri, [&](uint32_t op, uint32_t len, long long x, uint32_t y, const OpCtx &cx) {
        if (op != C3R_CIG_M) return;
        const long long dd = (long long)e.pos - 1 - x;
        if (dd < 0 || dd >= (long long)len) return;
        const unsigned long long q = (unsigned long long)y + (unsigned long long)dd;
        if (q >= ri.l_seq) return;
        col = spliced ? hap_observe_rs(e, ri, rseq, ins_pool, R, (uint32_t)overhang, q, dd == (long long)len - 1, (unsigned long long)y + len, cx, &ra)
                      : hap_observe_ra(e, ri, rseq, ins_pool, R, (uint32_t)overhang, q, dd == (long long)len - 1, (unsigned long long)y + len, cx, &ra);
    });
    if (err) return C3R_EINVAL;
    *column = (int)col;
    if (realigned) *realigned = ra ? 1 : 0;
    return C3R_OK;
}

int c3r_set_hap_min_bq(c3r_ctx *ctx, int min_bq) {
    if (!ctx) return C3R_EINVAL;
    if (min_bq < 0 || min_bq > 93) return fail(ctx, C3R_EINVAL, "c3r_set_hap_min_bq: %d is outside 0 .. 93", min_bq);
    if (min_bq == ctx->hap_min_bq) return C3R_OK;
    if (min_bq > 0 && ctx->n_reads > 0 && !ctx->has_qual)
        return fail(ctx, C3R_EINVAL, "c3r_set_hap_min_bq: the loaded reads came without qualities (c3r_load_reads_q)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the copy first: while it cannot be made (its buffers are allocated before anything is written) the old threshold stays, and with it
    // what read_args hands out
    const int old_bq = ctx->hap_min_bq;
    ctx->hap_min_bq = min_bq;
    if (int rc = mask_low_bq(ctx)) { ctx->hap_min_bq = old_bq; return rc; }
    if (!(ctx->n_phase > 0 && ctx->n_reads > 0 && ctx->has_qual)) return C3R_OK;
    ctx->last_scan_pruned = false;                                 // the tags on the device are those of the other sequence
    ctx->host_cache.reset();
    return ::refilter(ctx);
}

int c3r_get_hap_min_bq(c3r_ctx *ctx, int *min_bq, int64_t *n_masked) {
    if (!ctx) return C3R_EINVAL;
    if (min_bq) *min_bq = ctx->hap_min_bq;
    if (n_masked) {
        unsigned long long m = 0;
        if (ctx->hap_min_bq > 0 && ctx->has_qual && ctx->d_nmasked.p) {
            std::vector<unsigned long long> slots((size_t)MASKBQ_SLOTS * MASKBQ_SLOT_WORDS);
            HIPCHK(ctx, hipSetDevice(ctx->device));
            HIPCHK(ctx, hipMemcpyAsync(slots.data(), ctx->d_nmasked.p, slots.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            for (int s = 0; s < MASKBQ_SLOTS; ++s) m += slots[(size_t)s * MASKBQ_SLOT_WORDS];
        }
        *n_masked = (int64_t)m;
    }
    return C3R_OK;
}

int c3r_set_hap_bq_weights(c3r_ctx *ctx, int on) {
    if (!ctx) return C3R_EINVAL;
    if (on != 0 && on != 1) return fail(ctx, C3R_EINVAL, "c3r_set_hap_bq_weights: %d is neither 0 nor 1", on);
    const bool want = on != 0;
    if (want == ctx->hap_w) return C3R_OK;
    if (want && ctx->n_reads > 0 && !ctx->has_qual)
        return fail(ctx, C3R_EINVAL, "c3r_set_hap_bq_weights: the loaded reads came without qualities (c3r_load_reads_q)");
    ctx->hap_w = want;
    if (!(ctx->n_phase > 0 && ctx->n_reads > 0)) return C3R_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->last_scan_pruned = false;                                 // the tags on the device are those of the other weights
    ctx->host_cache.reset();
    // the pair buffer first: while it cannot be had the old switch stays, and with it the tags on the device (a failure of the tagging
    // that follows loses the loaded reads' tables, as a failed c3r_set_params does, and the switch goes back all the same)
    if (want) if (int rc = ensure(ctx, ctx->d_hpw, (size_t)ctx->n_reads * 8 + 16)) { ctx->hap_w = false; return rc; }
    const int rc = ::refilter(ctx);
    if (rc) ctx->hap_w = !want;
    return rc;
}

int c3r_get_hap_bq_weights(c3r_ctx *ctx, int *on) {
    if (!ctx) return C3R_EINVAL;
    if (on) *on = ctx->hap_w ? 1 : 0;
    return C3R_OK;
}

int c3r_get_haplotag_weights(c3r_ctx *ctx, uint32_t *w12, int64_t cap) {
    if (!ctx || cap < 0) return C3R_EINVAL;
    if (ctx->n_phase == 0) return fail(ctx, C3R_EINVAL, "no phase sites are set (c3r_set_phase_sites / c3r_set_phase_alleles): the reads have no weights");
    if (!ctx->hap_w) return fail(ctx, C3R_EINVAL, "c3r_get_haplotag_weights: c3r_set_hap_bq_weights is off: the tags were decided by unit weights");
    const int64_t n = ctx->n_reads;
    if (n && (!w12 || cap < n)) return fail(ctx, C3R_EOVERFLOW, "weight pairs of %lld reads do not fit %lld slots", (long long)n, (long long)cap);
    if (n == 0) return C3R_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(w12, ctx->d_hpw.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}

int c3r_get_haplotag_words(c3r_ctx *ctx, uint32_t *words, int64_t cap) {
    if (!ctx || cap < 0) return C3R_EINVAL;
    if (ctx->n_phase == 0) return fail(ctx, C3R_EINVAL, "no phase sites are set (c3r_set_phase_sites / c3r_set_phase_alleles): the reads have no tag words");
    const int64_t n = ctx->n_reads;
    if (n && (!words || cap < n)) return fail(ctx, C3R_EOVERFLOW, "tag words of %lld reads do not fit %lld slots", (long long)n, (long long)cap);
    if (n == 0) return C3R_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(words, ctx->d_hptag.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}

int c3r_get_hap_seq(c3r_ctx *ctx, uint8_t *seq4, int64_t cap) {
    if (!ctx || cap < 0 || (cap && !seq4)) return C3R_EINVAL;
    if (cap < ctx->n_seq_bytes) return fail(ctx, C3R_EOVERFLOW, "c3r_get_hap_seq: %lld bytes offered, %lld needed", (long long)cap, (long long)ctx->n_seq_bytes);
    if (ctx->n_seq_bytes == 0) return C3R_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const void *src = ctx->hap_min_bq > 0 && ctx->has_qual ? ctx->d_hapseq.p : ctx->d_seq.p;
    return big_d2h(ctx, seq4, src, (size_t)ctx->n_seq_bytes);
}

// The rule `left_align` of include/c3r.h on the host, for the table: base codes 1, 2, 4, 8 of the slice (0: outside, or not A, C, G, T).
namespace {
struct LaRef {
    const char *ref; int64_t beg0, len;
    uint8_t code(int64_t p) const {
        const int64_t o = p - beg0;
        if (o < 0 || o >= len) return 0;
        switch (ref[o]) { case 'A': case 'a': return 1; case 'C': case 'c': return 2; case 'G': case 'g': return 4; case 'T': case 't': return 8; default: return 0; }
    }
};
// k and, for an insertion, the rotated bases in s (n codes, in place)
int64_t la_shift(const LaRef &R, int64_t a, bool ins, int64_t n, std::vector<uint8_t> &s) {
    int64_t k = 0;
    for (;; ++k) {
        const uint8_t r = R.code(a - k);
        if (!r || !R.code(a - k - 1)) break;
        const uint8_t t = ins ? s[(size_t)n - 1] : R.code(a - k + n);
        if (r != t) break;
        if (ins) { s.pop_back(); s.insert(s.begin(), r); }
    }
    return k;
}
}  // namespace

int c3r_hap_left_align_sites(const c3r_hap_site_t *sites, int64_t n, const uint8_t *ins_pool, int64_t pool_bases, int64_t ref_start, const char *ref,
                             int64_t ref_len, c3r_hap_site_t *out_sites, uint8_t *out_pool, int64_t out_pool_cap, int64_t *out_pool_bases,
                             int64_t *src_index, int64_t *n_out, c3r_left_align_stats_t *stats) {
    if (n < 0 || pool_bases < 0 || ref_len < 0 || ref_start < 1 || out_pool_cap < 0 || (n && (!sites || !out_sites || !src_index)) || (pool_bases && !ins_pool) ||
        (ref_len && !ref) || (out_pool_cap && !out_pool) || !n_out)
        return C3R_EINVAL;
    const LaRef R{ref, ref_start - 1, ref_len};
    auto pool_at = [&](uint64_t q) { const uint8_t byte = ins_pool[q >> 1]; return (uint8_t)((q & 1) ? (byte & 15) : (byte >> 4)); };
    c3r_left_align_stats_t st;
    memset(&st, 0, sizeof st);
    st.n_in = n;
    struct Moved { c3r_hap_site_t e; int64_t src; std::vector<uint8_t> ins[2]; };
    std::vector<Moved> kept;
    kept.reserve((size_t)n);
    int64_t need = 0;
    for (int64_t i = 0; i < n; ++i) {
        Moved m;
        m.e = sites[i]; m.src = i;
        if (m.e.pos < 1 || m.e.base_matters > 1 || m.e.event_matters > 1) return C3R_EINVAL;
        c3r_hap_allele_t *al[2] = {&m.e.a, &m.e.b};
        int64_t k = -1;
        bool ok = true;
        for (int w = 0; w < 2; ++w) {
            const c3r_hap_allele_t &x = *al[w];
            if (x.kind > C3R_HAP_EV_DEL || (x.kind == C3R_HAP_EV_NONE ? x.len != 0 : x.len == 0)) return C3R_EINVAL;
            if (x.kind == C3R_HAP_EV_NONE) continue;
            if (x.kind == C3R_HAP_EV_INS) {
                if ((int64_t)x.ins_off + x.len > pool_bases) return C3R_EINVAL;
                for (uint32_t j = 0; j < x.len; ++j) m.ins[w].push_back(pool_at((uint64_t)x.ins_off + j));
                need += x.len;
            }
            const int64_t kw = la_shift(R, (int64_t)m.e.pos - 1, x.kind == C3R_HAP_EV_INS, x.len, m.ins[w]);
            if (k >= 0 && kw != k) ok = false;
            k = kw;
        }
        if (k < 0) k = 0;                                              // (no event allele: nothing to shift)
        if (!ok || (k > 0 && m.e.base_matters)) { st.n_not_left_alignable += 1; continue; }
        if (k > 0) {
            m.e.pos = (int32_t)(m.e.pos - k);
            m.e.a.base = m.e.b.base = R.code((int64_t)m.e.pos - 1);
            st.n_moved += 1;
        }
        kept.push_back(std::move(m));
    }
    if (need > out_pool_cap) return C3R_EOVERFLOW;
    std::stable_sort(kept.begin(), kept.end(), [](const Moved &x, const Moved &y) { return x.e.pos != y.e.pos ? x.e.pos < y.e.pos : x.src < y.src; });
    if (out_pool_cap) memset(out_pool, 0, (size_t)((out_pool_cap + 1) / 2));
    int64_t m_out = 0, nb = 0;
    for (size_t i = 0; i < kept.size(); ++i) {
        Moved &m = kept[i];
        if (m_out > 0 && out_sites[m_out - 1].pos == m.e.pos) { st.n_same_pos_after_left_align += 1; continue; }
        c3r_hap_allele_t *al[2] = {&m.e.a, &m.e.b};
        for (int w = 0; w < 2; ++w) {
            if (al[w]->kind != C3R_HAP_EV_INS) continue;
            al[w]->ins_off = (uint32_t)nb;
            for (uint8_t c : m.ins[w]) { out_pool[nb >> 1] |= (uint8_t)((nb & 1) ? c : c << 4); ++nb; }
        }
        out_sites[m_out] = m.e;
        src_index[m_out] = m.src;
        ++m_out;
    }
    st.n_out = m_out;
    *n_out = m_out;
    if (out_pool_bases) *out_pool_bases = nb;
    if (stats) *stats = st;
    return C3R_OK;
}

int c3r_hap_assign(const c3r_phase_site_t *in, int64_t n, const uint32_t *counts, const c3r_phase_params_t *p, c3r_phase_site_t *out,
                   c3r_hap_assign_stats_t *stats) {
    if (n < 0 || (n && (!in || !counts || !out))) return C3R_EINVAL;
    const int64_t min_reads = p ? p->min_reads : 2, pct = p ? p->min_agree_pct : 75;
    if (min_reads < 0 || pct < 0 || pct > 100) return C3R_EINVAL;
    c3r_hap_assign_stats_t st;
    memset(&st, 0, sizeof st);
    st.n_sites = n;
    for (int64_t j = 0; j < n; ++j) {
        const uint32_t *c = counts + (size_t)j * 9;                  // [row][allele]
        const uint64_t v1 = (uint64_t)c[1 * 3 + 1] + c[2 * 3 + 0], v0 = (uint64_t)c[1 * 3 + 0] + c[2 * 3 + 1], w = v0 + v1, hi = std::max(v0, v1);
        c3r_phase_site_t e = in[j];
        if (w < (uint64_t)min_reads) { st.n_few_reads += 1; e.ps = -1; e.h1 = 0; }
        else if (v0 == v1 || 100 * hi < (uint64_t)pct * w) { st.n_disagree += 1; e.ps = -1; e.h1 = 0; }
        else { st.n_phased += 1; e.h1 = v1 > v0 ? 1 : 0; }
        e.reserved = 0;
        out[j] = e;
    }
    if (stats) *stats = st;
    return C3R_OK;
}

// ------------------------------------------------------------------------------------------------
// dst16: the windows go out as int16 (the resident, rescaled tensors), else int32 (c3r_get_tensors' raw export)
static int run_gather(c3r_ctx *ctx, int rescale, void *dst, bool with_sites, bool dst16) {
    // operates on the candidates of the most recent scan; `dst` already points at their slot
    GatherArgs g;
    g.cols = (const int32_t *)ctx->d_cols.p; g.depth = (const int32_t *)ctx->d_depth.p; g.ncov = (const int32_t *)ctx->d_ncov.p;
    g.flags = (const uint8_t *)ctx->d_flags.p; g.tile_cols = (const uint8_t *)ctx->d_tile_cols.p; g.cand_idx = (const int32_t *)ctx->d_cand.p; g.n_cand = (int32_t)ctx->last_cand;
    g.n_pos = (int32_t)ctx->n_pos; g.geo = (const TileGeo *)ctx->d_geo.p;
    g.ref = (const uint8_t *)ctx->d_ref.p; g.ref_beg0 = (int32_t)(ctx->ref_start1 - 1); g.ref_len = (int32_t)ctx->ref_len;
    g.head_tail = ctx->prm.head_tail; g.last_row = (const int32_t *)ctx->d_lastrow.p;
    g.rescale = rescale; g.max_depth = ctx->prm.max_depth_rescale;
    g.tensors = dst; g.x16 = dst16 ? 1 : 0;
    g.raw = nullptr; g.skipmax = nullptr;
    g.sites = with_sites ? (c3r_site_t *)ctx->d_sites_out.p + ctx->last_base : nullptr;
    g.tok_cnt = with_sites ? (int32_t *)ctx->d_tokcnt.p : nullptr;
    const int blocks = (int)((ctx->last_cand * 64 + 255) / 256);
    if (ctx->prm.splice_padding) {
        // in-place column edits, candidate after candidate: runs once per scan and also keeps the raw windows
        g.raw = (int32_t *)ctx->d_raw.p; g.skipmax = (const int32_t *)ctx->d_skipmax.p;
        Launch L(ctx, "k_splice_gather");
        with_channels(ctx, [&](auto c) { hipLaunchKernelGGL(k_splice_gather<decltype(c)::value>, dim3(blocks), dim3(256), 0, ctx->stream, g); });
        return C3R_OK;
    }
    Launch L(ctx, "k_gather");
    with_channels(ctx, [&](auto c) { hipLaunchKernelGGL(k_gather<decltype(c)::value>, dim3(blocks), dim3(256), 0, ctx->stream, g); });
    return C3R_OK;
}

// exclusive scan of n ints in place on the context's stream, total to *d_total: one block for short inputs, three launches for long
static int device_excl_scan(c3r_ctx *ctx, int32_t *d, int n, int32_t *d_total) {
    const int nb = excl_scan_tops(n);                // (the routing and the launches: pileup_kernels.hpp, launch_excl_scan)
    int rc;
    if (nb && (rc = ensure(ctx, ctx->d_scan_tops, (size_t)nb * 4 + 16))) return rc;
    Launch L(ctx, "k_excl_scan");
    launch_excl_scan(ctx->stream, d, n, d_total, (int32_t *)ctx->d_scan_tops.p);
    return C3R_OK;
}

// Capacity of the indel-event scratch of one scan: a tile workgroup reserves (its events rounded up to 16) records.  An I / D op
// yields at most one event per region whose rows it falls into, and regions may overlap arbitrarily (the same region twice, chunks
// shorter than their +-33 bp halos): (I / D ops of the whole contig) x (the most regions any one position falls into), plus the
// rounding slack of every tile.  An upper bound that needs no host copy of the reads.
static size_t event_capacity(const c3r_ctx *ctx, int n_regions, const int64_t *ctg_starts, const int64_t *ctg_ends, int n_tiles, int spans_per_position) {
    size_t ev_cap = 16 * (size_t)n_tiles + 16;
    std::vector<std::pair<int64_t, int>> edge;
    for (int r = 0; r < n_regions; ++r) { edge.push_back({ctg_starts[r] - C3R_WINDOW - 2, +1}); edge.push_back({ctg_ends[r] + C3R_WINDOW + 2, -1}); }
    std::sort(edge.begin(), edge.end(), [](const std::pair<int64_t, int> &x, const std::pair<int64_t, int> &y) { return x.first != y.first ? x.first < y.first : x.second > y.second; });
    int cur = 0, maxov = 0;
    for (auto &e : edge) { cur += e.second; maxov = std::max(maxov, cur); }
    // (fused path: a position lies in its own span and in the flank of at most one neighbour)
    // (a deep tile also takes 2 x 8-byte hash slots per event behind its events: 2/3 of a record each)
    return ev_cap + 2 * ((size_t)maxov * (size_t)spans_per_position * (size_t)ctx->n_indel_ops);
}

// samtools mpileup -d (default 8000), restated from htslib's bam_plp_push / bam_plp_next (third-party, absent: parity
// unpinned; the oracle restates the same rule independently): reads arrive in file order, filtered, and only those
// overlapping the region; a read is discarded iff it is not the first read pushed for its start position and the
// engine's node pool — the kept reads with exclusive end > start - 1, plus the list's empty tail node — holds more than
// max_depth nodes (`iter->mp->cnt > iter->maxcnt`): reads that all start on one position pile up to exactly max_depth.  Sequential by
// nature, so it runs here on the host, per region, and only when the data can reach the cap at all (then the reads'
// headers are fetched back from the device).  *d_drop: the per-region bit masks on the device, or null when no read is discarded.
//
// Only inside the contig's HOT ZONES: with the reads counted into 256-position bins by start and by exclusive end,
//   B(c) = reads started before the end of bin c  -  reads whose end lies before bin c
// bounds the list at the push of every read that starts in bin c (whatever was discarded earlier, whatever the region), so a read that
// starts in a bin with B(c) <= max_depth is always kept.  The sequential rule runs over the maximal runs of bins above the cap, each
// entered with the list it would hold there: the kept reads from before the zone that reach into it.  A contig with one 20,000x locus
// costs a counting pass over its read headers and a heap over that locus' reads, not a heap over every read of every region.
constexpr int PLP_POOL_EXTRA = 1;      // nodes of htslib's pool that are not reads: the list's empty tail
static int depth_cap_mask(c3r_ctx *ctx, const ScanKnobs &kn, int n_regions, const int64_t *ctg_starts, const int64_t *ctg_ends, const uint32_t **d_drop, int *drop_words_out) {
    *d_drop = nullptr;
    const int drop_words = (int)(((size_t)ctx->n_reads + 31) / 32);
    *drop_words_out = drop_words;
    // (max_cover bounds the engine's read list at every read's start, k_prep / k_bin_scan: below the cap no read can be discarded)
    if (!(ctx->prm.max_depth > 0 && (int64_t)ctx->max_cover + PLP_POOL_EXTRA > ctx->prm.max_depth)) return C3R_OK;
    int rc;
    if ((rc = ensure_host_reads(ctx))) return rc;
    const std::vector<DevRead> &R = ctx->h_reads;
    const size_t n = R.size();
    if (!n) return C3R_OK;
    auto kept_by_filters = [&](const DevRead &rd) { return !(flag_fails(rd.flag, ctx->prm.excl_flags) || rd.mapq < ctx->prm.min_mq || rd.end <= rd.pos); };
    // ---- hot zones [z0, z1) in positions, ascending
    constexpr int ZSH = 8;
    const int64_t zb0 = (int64_t)R.front().pos >> ZSH;
    int64_t top = R.front().pos;
    for (size_t i = 0; i < n; ++i) if (kept_by_filters(R[i])) top = std::max<int64_t>(top, R[i].end);
    const size_t nz = (size_t)((top >> ZSH) - zb0) + 2;
    std::vector<uint32_t> &sc = ctx->h_zone_sc, &ec = ctx->h_zone_ec;
    sc.assign(nz, 0u); ec.assign(nz, 0u);
    for (size_t i = 0; i < n; ++i) {
        if (!kept_by_filters(R[i])) continue;
        ++sc[(size_t)(((int64_t)R[i].pos >> ZSH) - zb0)];
        ++ec[(size_t)(((int64_t)R[i].end >> ZSH) - zb0)];
    }
    std::vector<std::pair<int64_t, int64_t>> zones;
    {
        int64_t started = 0, ended_before = 0;
        bool open = false;
        for (size_t c = 0; c < nz; ++c) {
            started += sc[c];
            const bool hot = started - ended_before + PLP_POOL_EXTRA > (int64_t)ctx->prm.max_depth;
            const int64_t p = ((int64_t)c + zb0) << ZSH;
            if (hot && !open) { zones.push_back({p, p}); open = true; }
            if (open) { if (hot) zones.back().second = p + (1 << ZSH); else open = false; }
            ended_before += ec[c];
        }
    }
    if (zones.empty()) return C3R_OK;
    if (kn.cap_all) { zones.clear(); zones.push_back({(int64_t)R.front().pos, top + 1}); }     // (A/B aid: the rule over every read, as before round 5)
    ctx->h_drop.assign((size_t)n_regions * drop_words, 0u);
    bool any = false;
    auto first_at_or_after = [&](int64_t p) {           // first read with pos >= p (reads are sorted by pos)
        size_t lo = 0, hi = n;
        while (lo < hi) { const size_t m = (lo + hi) / 2; if ((int64_t)R[m].pos < p) lo = m + 1; else hi = m; }
        return lo;
    };
    for (int r = 0; r < n_regions; ++r) {
        int64_t es = ctg_starts[r] - C3R_WINDOW, ee = ctg_ends[r] + C3R_WINDOW;
        if (es < 1) es = 1;
        const int32_t beg0 = (int32_t)(es - 1), end0 = (int32_t)ee;                // rows for [beg0, end0)
        uint32_t *drop = ctx->h_drop.data() + (size_t)r * drop_words;
        // the first read fetched for this region: the first one whose end (as a prefix maximum) passes beg0
        const size_t i_region = (size_t)(std::upper_bound(ctx->h_prefmax.begin(), ctx->h_prefmax.end(), beg0) - ctx->h_prefmax.begin());
        for (const auto &z : zones) {
            if (z.first >= end0) break;
            const size_t i0 = std::max(first_at_or_after(z.first), i_region);
            if (i0 >= n || R[i0].pos >= end0 || (int64_t)R[i0].pos >= z.second) continue;
            std::priority_queue<int32_t, std::vector<int32_t>, std::greater<int32_t>> live;
            // the list on entry: kept reads of this region from before i0 that still reach R[i0].pos - 1 ... (popped lazily below, so "reach
            // the zone" is enough)
            const int32_t reach = (int32_t)std::max<int64_t>(std::max<int64_t>(z.first - 1, beg0), INT32_MIN);
            size_t j = (size_t)(std::upper_bound(ctx->h_prefmax.begin(), ctx->h_prefmax.end(), reach) - ctx->h_prefmax.begin());
            for (j = std::max(j, i_region); j < i0; ++j) {
                const DevRead &rd = R[j];
                if (!kept_by_filters(rd) || rd.end <= beg0 || rd.end <= reach) continue;
                if (drop[j >> 5] >> (j & 31) & 1u) continue;                         // discarded in an earlier zone
                live.push(rd.end);
            }
            int32_t last_pos = INT_MIN;
            // (the read before i0 starts before the zone or was not fetched: R[i0] is the first pushed for its position either way — unless
            // i0 is the region's first read, where the rule starts afresh as well)
            for (size_t i = i0; i < n; ++i) {
                const DevRead &rd = R[i];
                if (rd.pos >= end0 || (int64_t)rd.pos >= z.second) break;
                if (!kept_by_filters(rd)) continue;
                if (rd.end <= beg0) continue;                                            // not fetched for this region
                while (!live.empty() && live.top() <= rd.pos - 1) live.pop();
                const bool first = rd.pos != last_pos;
                last_pos = rd.pos;
                if (!first && (int64_t)live.size() + PLP_POOL_EXTRA > ctx->prm.max_depth) {
                    drop[i >> 5] |= 1u << (i & 31);
                    any = true;
                    continue;
                }
                live.push(rd.end);
            }
        }
    }
    if (any) {
        if ((rc = upload(ctx, ctx->d_drop, ctx->h_drop.data(), ctx->h_drop.size()))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));        // (h_drop is rebuilt by the next scan)
        *d_drop = (const uint32_t *)ctx->d_drop.p;
    }
    return C3R_OK;
}

// The reference's AF gates divide in float64 (float(count) / denominator >= minimum_af, src/create_tensor_pileup.py:267-285).  For every
// depth below AF_TAB the smallest count that passes is found HERE with that very division, so that the kernels compare integers: the
// quotient grows with the count, hence "count >= threshold" is the same predicate, bit for bit.  65535: no count passes (af > 1).
static int af_table(c3r_ctx *ctx) {
    if (ctx->d_aftab.p && ctx->aftab_snp == ctx->prm.snp_min_af && ctx->aftab_indel == ctx->prm.indel_min_af) return C3R_OK;
    std::vector<uint32_t> tab((size_t)AF_TAB);
    auto thr = [](int d, double af) -> uint32_t {
        const double denom = d > 0 ? (double)d : 1.0;
        const int top = std::max(d, 1);
        // an AF no count can reach (well above 65534 / depth: a user's AF > 1 at every depth of the table; NaN) is "never" at once, not after 65 k
        // divisions (the margin leaves the last ulp to the divisions below)
        if (!(af * denom <= 65536.0)) return 65535u;
        int c = (int)std::ceil(af * denom);                       // near the answer; settled by the division itself
        c = std::max(1, std::min(c, top + 1));
        while (c > 1 && (double)(c - 1) / denom >= af) --c;
        while (c <= top && !((double)c / denom >= af)) ++c;
        // (counts above the depth exist: insertions on ref-skip columns are not part of the depth)
        while (c <= 65534 && !((double)c / denom >= af)) ++c;
        return c > 65534 ? 65535u : (uint32_t)c;
    };
    for (int d = 0; d < AF_TAB; ++d) tab[(size_t)d] = thr(d, ctx->prm.snp_min_af) | (thr(d, ctx->prm.indel_min_af) << 16);
    int rc = upload(ctx, ctx->d_aftab, tab.data(), tab.size());
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));               // (tab is a temporary)
    ctx->aftab_snp = ctx->prm.snp_min_af; ctx->aftab_indel = ctx->prm.indel_min_af;
    return C3R_OK;
}

// the inputs every tile kernel sees, the regions' depth-cap masks among them (the output side is filled in by the two scan paths)
static int scan_inputs(c3r_ctx *ctx, const ScanKnobs &kn, ScanArgs &a, int n_regions, const int64_t *ctg_starts, const int64_t *ctg_ends, int n_tiles) {
    memset(&a, 0, sizeof a);
    if (int rc = depth_cap_mask(ctx, kn, n_regions, ctg_starts, ctg_ends, &a.drop, &a.drop_words)) return rc;
    a.reads = (const DevRead *)ctx->d_reads.p; a.seq = (const uint8_t *)ctx->d_seq.p; a.n_reads = ctx->n_reads; a.compat = ctx->prm.mpileup_compat;
    a.recs = (const PileRec *)ctx->d_recs.p; a.rec_off = (const uint32_t *)ctx->d_binoff.p; a.rtab = (const int4 *)ctx->d_rtab.p; a.bins = ctx->bins;
    a.n_tiles = n_tiles;
    a.ref = (const uint8_t *)ctx->d_ref.p; a.ref_beg0 = (int32_t)(ctx->ref_start1 - 1); a.ref_len = (int32_t)ctx->ref_len;
    a.geo = (const TileGeo *)ctx->d_geo.p;
    a.lbed = (const int32_t *)ctx->d_bed[0].p; a.n_lbed = (int32_t)(ctx->h_bed[0].size() / 2); a.has_lbed = ctx->has_bed[0];
    a.cbed = (const int32_t *)ctx->d_bed[1].p; a.n_cbed = (int32_t)(ctx->h_bed[1].size() / 2); a.has_cbed = ctx->has_bed[1];
    a.sites = (const int32_t *)ctx->d_sites.p; a.n_sites = (int32_t)ctx->h_sites.size(); a.genotyping = ctx->prm.genotyping_mode;
    a.min_mq = ctx->prm.min_mq; a.excl_flags = ctx->prm.excl_flags; a.min_cov = ctx->prm.min_coverage;
    a.snp_af = ctx->prm.snp_min_af; a.indel_af = ctx->prm.indel_min_af; a.af_tab = (const uint32_t *)ctx->d_aftab.p;
    a.head_tail = ctx->prm.head_tail; a.splice = ctx->prm.splice_padding;
    if (ctx->padins && !ctx->padins->empty()) { a.padins = (const c3r_padins_t *)ctx->d_padins.p; a.n_padins = (int32_t)ctx->padins->size(); }
    a.abl = kn.abl; a.deep_min = kn.deep_min; a.split_min = kn.split_min; a.split_slice = kn.split_slice; a.no_shift = kn.no_shift ? 1 : 0;
    return C3R_OK;
}

// ---- what the two scan routes share
// The tile geometry of a scan.  Per region, rows: 1-based [max(1, ctg_start-33), ctg_end+33]  (src/create_tensor_pileup.py:411-415), cut into
// tiles of `step` positions; the slots of tile t are t * TILE + (p - p0).  guard_tile: the column store's layout — an empty tile behind every region
// (pileup_kernels.hpp, TileGeo); without: the fused path's spans.  Rebuilt and uploaded only when the regions or the layout have changed; then
// regb takes the regions' [beg0, end0).  geo_key is empty while h_geo or d_geo are not what a key says (a failure below, or in the caller's own upload).
static int scan_geometry(c3r_ctx *ctx, int32_t n_regions, const int64_t *ctg_starts, const int64_t *ctg_ends, int step, bool guard_tile, std::vector<int2> *regb = nullptr) {
    std::vector<int64_t> key{guard_tile ? -1 : -2};                    // (which of the two layouts, then the regions)
    for (int r = 0; r < n_regions; ++r) { key.push_back(ctg_starts[r]); key.push_back(ctg_ends[r]); }
    if (key != ctx->geo_key) {
        ctx->geo_key.clear();
        ctx->h_geo.clear();
        for (int r = 0; r < n_regions; ++r) {
            int64_t es = ctg_starts[r] - C3R_WINDOW, ee = ctg_ends[r] + C3R_WINDOW;
            if (es < 1) es = 1;
            const int32_t beg0 = (int32_t)(es - 1), end0 = (int32_t)ee;
            for (int32_t p0 = beg0; p0 < end0; p0 += step) ctx->h_geo.push_back(TileGeo{p0, std::min(p0 + step, end0), r, 0});
            if (guard_tile) ctx->h_geo.push_back(TileGeo{end0, end0, r, 0});
            if (regb) regb->push_back(make_int2(beg0, end0));
            if (r == 0) { ctx->reg_beg0 = beg0; ctx->reg_end0 = end0; }
        }
        if ((int64_t)ctx->h_geo.size() * TILE > INT32_MAX - TILE) return fail(ctx, C3R_EINVAL, "regions too large for one scan (2^31 slots)");
        if (int rc = upload(ctx, ctx->d_geo, ctx->h_geo.data(), ctx->h_geo.size())) return rc;
        ctx->geo_key = key;
    }
    ctx->n_regions = n_regions;
    ctx->n_pos = (int64_t)ctx->h_geo.size() * TILE;
    return C3R_OK;
}

// a scan that produces candidates starts here: outside a batch the resident totals start over
static void scan_output_begin(c3r_ctx *ctx) {
    if (!ctx->batching) { ctx->n_cand = 0; ctx->n_tok = 0; ctx->n_rows = 0; ctx->n_tokspace = 0; }
    ctx->last_cand = 0; ctx->last_base = ctx->n_cand;
}

// C3R_SCAN_DBG: the phase clocks of the tile kernels (timing aid, off in production)
static int scan_dbg_buffer(c3r_ctx *ctx, const ScanKnobs &kn, ScanArgs &a) {
    if (!kn.dbg) return C3R_OK;                                       // (a.dbg is null: scan_inputs)
    if (int rc = ensure(ctx, ctx->d_dbg, 32 * 8)) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_dbg.p, 0, 32 * 8, ctx->stream));
    a.dbg = (unsigned long long *)ctx->d_dbg.p;
    return C3R_OK;
}

// bytes of a resident window: int16 (a caller sees int32: c3r_get_tensors) unless the context has met a position too deep for it
static size_t window_bytes(const c3r_ctx *ctx) { return (size_t)C3R_WINDOW * ctx->prm.channels * (ctx->win32 ? sizeof(int32_t) : sizeof(int16_t)); }

// the two refusals that either route may end in
static int refuse_depth16_in_batch(c3r_ctx *ctx) { return fail(ctx, C3R_EOVERFLOW, "a position is covered by more than 32,767 reads and the batch already holds 16-bit windows: scan this region first, or alone"); }
static int refuse_event_scratch(c3r_ctx *ctx, size_t ev_cap) { return fail(ctx, C3R_EOVERFLOW, "internal: indel-event scratch too small (%zu records) — nothing was written past it", ev_cap); }

// ---- the column-store path: columns, depth and flags of every position go to HBM (k_scan_tiles), then window selection, ordered
// compaction, gather and tokens as separate kernels, with two host read-backs for sizes.  columns_only: c3r_get_columns after a
// fused scan — the columns and flags of the given region, nothing else is touched.
static int scan_column_store(c3r_ctx *ctx, const ScanKnobs &kn, int32_t n_regions, const int64_t *ctg_starts, const int64_t *ctg_ends, int64_t *n_candidates, bool columns_only) {
    const int C = ctx->prm.channels;
    int rc;
    if ((rc = scan_geometry(ctx, n_regions, ctg_starts, ctg_ends, TILE, true))) return rc;
    const int n_tiles = (int)ctx->h_geo.size();
    if (!columns_only) scan_output_begin(ctx);
    const int64_t base_cand = ctx->n_cand, base_row = ctx->n_rows, base_tok = ctx->n_tokspace;
    const int64_t n_pos = ctx->n_pos;
    const int n_cblocks = (int)((n_pos + CMP_BLOCK - 1) / CMP_BLOCK);
    const int grid = std::min(n_tiles, kn.list_grid);
    if ((rc = ensure(ctx, ctx->d_lastrow, (size_t)n_regions * 4 + 16))) return rc;
    if ((rc = ensure(ctx, ctx->d_cols, (size_t)n_pos * C * 4))) return rc;
    if ((rc = ensure(ctx, ctx->d_depth, (size_t)n_pos * 4))) return rc;
    if ((rc = ensure(ctx, ctx->d_ncov, (size_t)n_pos * 4))) return rc;
    if ((rc = ensure(ctx, ctx->d_flags, (size_t)n_pos))) return rc;
    const size_t ev_cap = event_capacity(ctx, n_regions, ctg_starts, ctg_ends, n_tiles, 1);
    if ((rc = ensure(ctx, ctx->d_ev, ev_cap * sizeof(EvRec)))) return rc;
    if ((rc = ensure(ctx, ctx->d_small, sizeof(ColCtl)))) return rc;
    if ((rc = ensure(ctx, ctx->d_tile_cols, (size_t)n_tiles + 16))) return rc;
    if ((rc = ensure(ctx, ctx->d_tile_rng, (size_t)n_tiles * 16 + 16))) return rc;
    if ((rc = ensure(ctx, ctx->d_tile_list, (size_t)n_tiles * 4 + 16))) return rc;
    if ((rc = ensure(ctx, ctx->d_tile_list2, (size_t)n_tiles * 4 + 16))) return rc;
    if ((rc = ensure(ctx, ctx->d_tile_cand, (size_t)n_tiles * 8 + 16))) return rc;
    if ((rc = ensure(ctx, ctx->d_blockcnt, (size_t)(n_cblocks + 1) * 4))) return rc;
    if (ctx->prm.splice_padding && (rc = ensure(ctx, ctx->d_skipmax, (size_t)n_pos * 4))) return rc;
    ColCtl *const ctl = (ColCtl *)ctx->d_small.p;                 // (device memory: only its fields' addresses are taken here)
    const ColCtl init{};
    HIPCHK(ctx, hipMemcpyAsync(ctl, &init, offsetof(ColCtl, unused), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_lastrow.p, 0xff, (size_t)n_regions * 4, ctx->stream));      // -1
    HIPCHK(ctx, hipMemsetAsync(ctx->d_flags.p, 0, (size_t)n_pos, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_tile_cols.p, 0, (size_t)n_tiles, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_tile_cand.p, 0, (size_t)n_tiles * 8, ctx->stream));

    ScanArgs a;
    if ((rc = scan_inputs(ctx, kn, a, n_regions, ctg_starts, ctg_ends, n_tiles))) return rc;
    a.tile_cols = (uint8_t *)ctx->d_tile_cols.p;
    a.tile_rng = (int4 *)ctx->d_tile_rng.p; a.tile_list = (int32_t *)ctx->d_tile_list.p;
    a.n_tile_list = &ctl->n_tile_list;
    // rows of intron-only tiles far from every aligned segment only matter to the end-of-stream rule (head/tail), to splice
    // padding and to genotyping sites: in the plain mode they are left out of the scan
    a.prune = (!columns_only && !ctx->prm.head_tail && !ctx->prm.splice_padding && !ctx->prm.genotyping_mode && !kn.no_prune) ? 1 : 0;
    a.tile_list2 = (int32_t *)ctx->d_tile_list2.p; a.n_tile_list2 = &ctl->n_tile_list2;
    if ((rc = scan_dbg_buffer(ctx, kn, a))) return rc;
    a.cols = (int32_t *)ctx->d_cols.p; a.depth = (int32_t *)ctx->d_depth.p; a.ncov = (int32_t *)ctx->d_ncov.p; a.flags = (uint8_t *)ctx->d_flags.p;
    a.ev = (EvRec *)ctx->d_ev.p; a.ev_cursor = &ctl->ev_cursor; a.last_row = (int32_t *)ctx->d_lastrow.p;
    a.ev_cap = (unsigned long long)ev_cap; a.ev_overflow = &ctl->ev_overflow;
    a.skipmax = (int32_t *)ctx->d_skipmax.p;
    if (!columns_only) { ctx->last_scan = a; ctx->last_scan_pruned = a.prune && a.n_reads > 0; }
    if (a.n_reads > 0) {
        { Launch L(ctx, "k_tile_ranges"); hipLaunchKernelGGL(k_tile_ranges, dim3((n_tiles + 255) / 256), dim3(256), 0, ctx->stream, a); }
        Launch L(ctx, "k_scan_tiles");
        with_channels(ctx, [&](auto c) { hipLaunchKernelGGL(k_scan_tiles<decltype(c)::value>, dim3(grid), dim3(SCAN_THREADS), 0, ctx->stream, a); });
    }
    if (a.n_reads > 0 && C == C3R_CH_PHASED) {
        if ((rc = ensure_legacy_tables(ctx))) return rc;
        PhaseArgs f;
        f.tile_list = a.tile_list; f.n_tile_list = a.n_tile_list; f.tile_rng = a.tile_rng; f.geo = a.geo;
        f.reads = a.reads; f.rsegs = (const DevSeg *)ctx->d_rsegs.p; f.rseg_first = (const uint32_t *)ctx->d_rseg_first.p;
        f.cigar = (const uint32_t *)ctx->d_cigar.p; f.seq = a.seq; f.flags = a.flags; f.cols = a.cols; f.min_mq = a.min_mq; f.excl_flags = a.excl_flags;
        f.drop = a.drop; f.drop_words = a.drop_words;
        Launch L(ctx, "k_phase_recompute");
        hipLaunchKernelGGL(k_phase_recompute, dim3(grid), dim3(TILE), 0, ctx->stream, f);
    }
    if (a.n_reads > 0 && a.splice) {
        HIPCHK(ctx, hipMemsetAsync(ctx->d_skipmax.p, 0, (size_t)n_pos * 4, ctx->stream));
        Launch L(ctx, "k_skip_counts");
        hipLaunchKernelGGL(k_skip_counts, dim3(grid), dim3(SCAN_THREADS), 0, ctx->stream, a);
    }
    // candidates live in tiles that hold aligned bases — except in genotyping mode, where any row of the site list is one
    const uint8_t *heavy = ctx->prm.genotyping_mode ? nullptr : (const uint8_t *)ctx->d_tile_cols.p;
    {
        Launch L(ctx, "k_select");
        hipLaunchKernelGGL(k_select, dim3(grid), dim3(TILE), 0, ctx->stream, (uint8_t *)ctx->d_flags.p,
                           (int)n_pos, (const TileGeo *)ctx->d_geo.p, ctx->prm.head_tail, (const int32_t *)ctx->d_lastrow.p, heavy,
                           (const int32_t *)ctx->d_tile_list.p, (const int32_t *)&ctl->n_tile_list);
    }
    if (columns_only) { HIPCHK(ctx, hipGetLastError()); return C3R_OK; }
    {
        Launch L(ctx, "k_compact_count");
        hipLaunchKernelGGL(k_compact_count, dim3(n_cblocks), dim3(CMP_THREADS), 0, ctx->stream, (const uint8_t *)ctx->d_flags.p, (int)n_pos,
                           (int32_t *)ctx->d_blockcnt.p, heavy);
    }
    if ((rc = device_excl_scan(ctx, (int32_t *)ctx->d_blockcnt.p, n_cblocks, &ctl->n_cand))) return rc;
    ColCtl h{};                          // host copy: the words read back below, and no others
    HIPCHK(ctx, hipMemcpyAsync(&h.ev_overflow, &ctl->ev_overflow, offsetof(ColCtl, n_tok) - offsetof(ColCtl, ev_overflow), hipMemcpyDeviceToHost, ctx->stream));   // ev_overflow, n_cand
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    if (a.dbg) {
        unsigned long long d[16];
        HIPCHK(ctx, hipMemcpy(d, ctx->d_dbg.p, sizeof d, hipMemcpyDeviceToHost));
        const double nt = d[15] ? (double)d[15] : 1.0;
        fprintf(stderr, "[k_scan_tiles] %llu heavy tiles; per tile: segments in range %.1f, listed %.1f, ops %.1f; us per tile: zero %.2f | cover+list+walk %.2f | scans %.2f | events %.2f | gates %.2f | store %.2f | first-seen %.2f\n",
                d[15], d[13] / nt, d[12] / nt, d[14] / nt, d[0] / nt / 100, d[1] / nt / 100, d[2] / nt / 100, d[3] / nt / 100, d[4] / nt / 100, d[5] / nt / 100, d[6] / nt / 100);
    }
    if ((h.ev_overflow & EV_OVF_DEPTH16) && !ctx->win32) {
        ctx->last_scan_pruned = false;
        if (columns_only) { /* columns are int32 anyway */ }
        else if (base_row != 0) return refuse_depth16_in_batch(ctx);
        else { ctx->win32 = true; return scan_column_store(ctx, kn, n_regions, ctg_starts, ctg_ends, n_candidates, columns_only); }
    }
    if (h.ev_overflow & EV_OVF_SCRATCH) { ctx->last_scan_pruned = false; return refuse_event_scratch(ctx, ev_cap); }
    const int32_t n_cand = h.n_cand;
    ctx->last_cand = n_cand;
    if (n_candidates) *n_candidates = n_cand;
    if (n_cand == 0) return C3R_OK;
    const size_t tbytes = window_bytes(ctx);
    if ((rc = ensure(ctx, ctx->d_cand, (size_t)n_cand * 4))) return rc;
    if ((rc = ensure_keep(ctx, ctx->d_tensors, (size_t)(base_row + n_cand) * tbytes, (size_t)base_row * tbytes))) return rc;
    if ((rc = ensure_keep(ctx, ctx->d_sites_out, (size_t)(base_cand + n_cand) * sizeof(c3r_site_t), (size_t)base_cand * sizeof(c3r_site_t)))) return rc;
    if ((rc = ensure(ctx, ctx->d_tokcnt, (size_t)(n_cand + 1) * 4))) return rc;
    if (ctx->prm.splice_padding && (rc = ensure(ctx, ctx->d_raw, (size_t)n_cand * C3R_WINDOW * C * sizeof(int32_t)))) return rc;      // (raw windows: int32)
    {
        Launch L(ctx, "k_compact_write");
        hipLaunchKernelGGL(k_compact_write, dim3(n_cblocks), dim3(CMP_THREADS), 0, ctx->stream, (const uint8_t *)ctx->d_flags.p, (int)n_pos,
                           (const int32_t *)ctx->d_blockcnt.p, (int32_t *)ctx->d_cand.p, heavy, (int2 *)ctx->d_tile_cand.p);
    }
    if ((rc = run_gather(ctx, 1, (char *)ctx->d_tensors.p + (size_t)base_row * tbytes, true, !ctx->win32))) return rc;
    if ((rc = ensure_keep(ctx, ctx->d_winidx, (size_t)(base_cand + n_cand) * 4, (size_t)base_cand * 4))) return rc;
    hipLaunchKernelGGL(k_iota, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, ctx->stream, (int32_t *)ctx->d_winidx.p + base_cand, (int)n_cand, (int)base_row);      // (windows in site order)
    {
        // token SLOTS per candidate (the gates' bound of the reads with something to say, TileOut::cov) -> first slots; [n_cand] = their total
        HIPCHK(ctx, hipMemsetAsync((int32_t *)ctx->d_tokcnt.p + n_cand, 0, 4, ctx->stream));
        if ((rc = device_excl_scan(ctx, (int32_t *)ctx->d_tokcnt.p, (int)n_cand + 1, &ctl->n_tok))) return rc;
    }
    HIPCHK(ctx, hipMemcpyAsync(&h.n_tok, &ctl->n_tok, sizeof h.n_tok, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                  // (h.n_tok: slots)
    if ((rc = ensure_keep(ctx, ctx->d_tok, std::max<size_t>((size_t)(base_tok + h.n_tok) * sizeof(c3r_token_t), 16),
                          (size_t)base_tok * sizeof(c3r_token_t)))) return rc;
    {
        TileTokArgs t;
        t.a = a;
        t.cand_idx = (const int32_t *)ctx->d_cand.p; t.tile_cand = (const int2 *)ctx->d_tile_cand.p;
        t.tok_off = (const int32_t *)ctx->d_tokcnt.p; t.sites = (c3r_site_t *)ctx->d_sites_out.p + base_cand;
        t.tok = (c3r_token_t *)ctx->d_tok.p; t.tok_base = (int32_t)base_tok;     // (sized exactly above)
        t.totals = &ctl->tok_written;                                             // ([1]: tok_lost)
        Launch L(ctx, "k_tokens");
        hipLaunchKernelGGL(k_tile_tokens, dim3(grid), dim3(SCAN_THREADS), 0, ctx->stream, t);
    }
    HIPCHK(ctx, hipMemcpyAsync(&h.tok_written, &ctl->tok_written, offsetof(ColCtl, unused) - offsetof(ColCtl, tok_written), hipMemcpyDeviceToHost, ctx->stream));   // tok_written, tok_lost
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (h.tok_lost) return fail(ctx, C3R_EOVERFLOW, "internal: %d tokens found no slot (the gates' bound of a site's tokens was too small)", h.tok_lost);
    ctx->n_cand = base_cand + n_cand;
    ctx->n_tok += h.tok_written;
    ctx->n_rows = base_row + n_cand; ctx->n_tokspace = base_tok + h.n_tok;
    HIPCHK(ctx, hipGetLastError());
    return C3R_OK;
}

// ---- the fused path (pileup_kernels.hpp, k_fused_tiles): memset of the look-back words, k_tile_ranges_fused, k_fused_tiles (windows
// AND tokens), k_order_spans, k_finalize_sites, and ONE read-back at the end (totals + overflow flags).  Output buffers are sized from what earlier passes needed;
// kernels never write past them, and when the totals say something did not fit the buffers grow and the scan is repeated (the first
// pass of a context; steady-state passes run once, without talking to the host in between).
// raw_rerun: c3r_get_tensors(rescaled = 0) — the same scan again, un-rescaled windows only, into d_raw.
static int scan_fused(c3r_ctx *ctx, const ScanKnobs &kn, int32_t n_regions, const int64_t *ctg_starts, const int64_t *ctg_ends, int64_t *n_candidates, bool raw_rerun) {
    const int C = ctx->prm.channels;
    int rc;
    std::vector<int2> regb;
    if ((rc = scan_geometry(ctx, n_regions, ctg_starts, ctg_ends, FUSE_IN, false, &regb))) return rc;
    if (!regb.empty()) {                                              // (the geometry is new)
        if ((rc = upload(ctx, ctx->d_regb, regb.data(), regb.size()))) { ctx->geo_key.clear(); return rc; }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));               // (the copy reads regb)
    }
    const int n_tiles = (int)ctx->h_geo.size();
    if (!raw_rerun) scan_output_begin(ctx);
    const int64_t base_cand = raw_rerun ? 0 : ctx->n_cand, base_row = raw_rerun ? 0 : ctx->n_rows, base_tok = raw_rerun ? 0 : ctx->n_tokspace;
    if (ctx->n_reads == 0 || n_tiles == 0) return C3R_OK;
    const size_t ev_cap = event_capacity(ctx, n_regions, ctg_starts, ctg_ends, n_tiles, 2);
    const int nblk = (n_tiles + 255) / 256;
    const ScanCtlLayout lay(nblk);                                // (pileup_kernels.hpp, ScanCtl: the control block's head and what follows it)
    if ((rc = ensure(ctx, ctx->d_ev, ev_cap * sizeof(EvRec))) || (rc = ensure(ctx, ctx->d_lb, lay.bytes)) || (rc = ensure(ctx, ctx->d_tile_rng, (size_t)n_tiles * 16 + 16)) ||
        (rc = ensure(ctx, ctx->d_tile_list, (size_t)n_tiles * 4 + 16)) ||
        (rc = ensure(ctx, ctx->d_span, (size_t)n_tiles * sizeof(int4) + 16)) || (rc = ensure(ctx, ctx->d_spanbase, (size_t)n_tiles * 4 + 16)) ||
        (rc = ensure(ctx, ctx->d_spanrec, (size_t)n_tiles * sizeof(SpanRec) + 16)) || (rc = ensure(ctx, ctx->d_deep, (size_t)n_tiles * 4 + 16)))
        return rc;
    if (!ctx->h_scan) HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_scan, sizeof(ScanReadback), hipHostMallocDefault));
    const ScanReadback &h = *ctx->h_scan;
    char *const lb = (char *)ctx->d_lb.p;
    ScanCtl *const ctl = (ScanCtl *)lb;                           // (device memory: only its fields' addresses are taken here)
    FusedArgs f;
    memset(&f, 0, sizeof f);
    ScanArgs &a = f.a;
    if ((rc = scan_inputs(ctx, kn, a, n_regions, ctg_starts, ctg_ends, n_tiles))) return rc;
    a.tile_rng = (int4 *)ctx->d_tile_rng.p; a.tile_list = (int32_t *)ctx->d_tile_list.p; a.n_tile_list = &ctl->n_listed;
    a.ev = (EvRec *)ctx->d_ev.p; a.ev_cursor = &ctl->ev_cursor; a.ev_cap = (unsigned long long)ev_cap; a.ev_overflow = &ctl->ev_overflow;
    if ((rc = scan_dbg_buffer(ctx, kn, a))) return rc;
    f.span_rec = (const SpanRec *)ctx->d_spanrec.p;
    // the deep kernel's per-workgroup event buffers (every event of a span in arrival order: a span that outgrows the LDS store is bucketed from there
    // instead of walking its records again): 300 MB, so only for a context that has met a deep span (its first such scan walks twice)
    const int deep_grid = std::min(n_tiles, ctx->n_cu > 0 ? ctx->n_cu : 256);
    if ((ctx->seen_deep || kn.evwg == 1) && kn.evwg != 0) {
        if ((rc = ensure(ctx, ctx->d_evwg, (size_t)deep_grid * DEEP_EVG_CAP * sizeof(EvRec)))) return rc;
        a.ev_wg = (EvRec *)ctx->d_evwg.p; a.ev_wg_cap = DEEP_EVG_CAP;
    }
    // giant spans (k_deep_walk, k_deep_alleles): GIANT_SLOTS = 256 accumulator slots + the slice list (8.5 MB), a pool of 12 M events (288 MB) and their allele table
    // (192 MB), for a context that has met one
    const size_t giant_acc_bytes = (size_t)GIANT_SLOTS * GIANT_STRIDE * 4 + 16;          // (+ the pool's cursor: cleared with the slots)
    a.n_giant = &ctl->n_giant; a.n_help = &ctl->n_help;
    if ((ctx->seen_giant || kn.giant == 1) && kn.giant != 0) {
        if ((rc = ensure(ctx, ctx->d_giant, giant_acc_bytes + (size_t)GIANT_SLOTS * GIANT_MAX_HELP * sizeof(int4))) ||
            (rc = ensure(ctx, ctx->d_giant_ev, (size_t)GIANT_POOL_EVENTS * sizeof(EvRec)))) return rc;
        a.giant_acc = (int32_t *)ctx->d_giant.p; a.help_list = (int4 *)((char *)ctx->d_giant.p + giant_acc_bytes); a.giant_ev = (EvRec *)ctx->d_giant_ev.p;
        a.giant_pool = GIANT_POOL_EVENTS; a.n_giant_ev = (int32_t *)((char *)ctx->d_giant.p + giant_acc_bytes - 16);
        a.deep_recs = (unsigned long long *)((char *)ctx->d_giant.p + giant_acc_bytes - 8);
        a.split_cus = kn.split_cus;
        if (!kn.no_giant_tab) {
            // (the allele table is all-zero between scans: cleared here when it is new, by k_fused_deep as it reads afterwards)
            const size_t tab_bytes = (size_t)GIANT_POOL_EVENTS * 2 * sizeof(uint2);
            const bool fresh = ctx->d_giant_tab.cap < tab_bytes;
            if ((rc = ensure(ctx, ctx->d_giant_tab, tab_bytes))) return rc;
            if (fresh) HIPCHK(ctx, hipMemsetAsync(ctx->d_giant_tab.p, 0, tab_bytes, ctx->stream));
            a.giant_tab = (uint2 *)ctx->d_giant_tab.p;
        }
    }
    f.ticket = (int32_t *)(lb + lay.ticket); f.alloc = (unsigned long long *)(lb + lay.alloc); f.overflow = &ctl->overflow;
    f.rescale = raw_rerun ? 0 : 1; f.max_depth = ctx->prm.max_depth_rescale;
    f.span_info = (int4 *)ctx->d_span.p;
    // 30 channels: the per-read op / segment tables behind the ordered recompute of a flagged column (an IUPAC read base, an indel right
    // behind a ref-skip) are built only for a context that has met such a column: aligners emit neither, and the tables cost 0.12 ms of
    // a 0.7-ms MAS-Seq chr20 pass.  Without them a flagged column raises FUSED_OVF_ORDER_TABLES and the scan is repeated with them.
    if (C == C3R_CH_PHASED && (ctx->legacy_wanted || kn.legacy_eager) && (rc = ensure_legacy_tables(ctx))) return rc;
    const bool have_tables = C == C3R_CH_PHASED && ctx->legacy_valid;
    f.ph.reads = a.reads; f.ph.rsegs = have_tables ? (const DevSeg *)ctx->d_rsegs.p : nullptr; f.ph.rseg_first = have_tables ? (const uint32_t *)ctx->d_rseg_first.p : nullptr;
    f.ph.cigar = (const uint32_t *)ctx->d_cigar.p; f.ph.seq = a.seq;
    f.ph.min_mq = a.min_mq; f.ph.excl_flags = a.excl_flags; f.ph.drop = a.drop; f.ph.drop_words = a.drop_words;
    const size_t tbytes = window_bytes(ctx);
    // What this scan may write.  A small scan has one allocator and dense output: whatever the buffers can take beyond what the batch
    // already holds.  A large one hands rows and token slots out through ALLOC_SHARDS sub-allocators of equal size, sized from what the
    // previous large scan needed; when a shard runs over, the scan is repeated with what the counters say it needs.
    const int nsh = raw_rerun ? ctx->last_shards : ((n_tiles >= 4096 && !kn.one_shard) ? ALLOC_SHARDS : 1);
    int64_t want_c, want_t;            // per shard
    if (raw_rerun) { want_c = ctx->last_shard_rows; want_t = 0; }
    else if (nsh == 1) {
        want_c = std::min<int64_t>({(int64_t)(ctx->d_tensors.cap / tbytes) - base_row, (int64_t)(ctx->d_sites_out.cap / sizeof(c3r_site_t)) - base_cand,
                                    (int64_t)(ctx->d_winidx.cap / 4) - base_cand, (int64_t)(ctx->d_cand.cap / 4), (int64_t)(ctx->d_meta.cap / sizeof(CandMeta))});
        want_t = (int64_t)(ctx->d_tok.cap / sizeof(c3r_token_t)) - base_tok;
        if (want_c < 1024) want_c = 65536;
        if (want_t < 1024) want_t = 32 * want_c;
    } else { want_c = ctx->hint_rows; want_t = ctx->hint_toks; }
    int32_t n_cand = 0, n_tok = 0;
    for (int attempt = 0;; ++attempt) {
        FinalizeArgs z;
        memset(&z, 0, sizeof z);
        want_c = std::min<int64_t>(want_c, INT32_MAX / nsh); want_t = std::min<int64_t>(want_t, (INT32_MAX - base_tok) / nsh);
        const int64_t rows = want_c * nsh, toks = want_t * nsh;
        if ((rc = ensure(ctx, ctx->d_meta, std::max<size_t>((size_t)rows * sizeof(CandMeta), 16)))) return rc;
        if (raw_rerun) {
            if ((rc = ensure(ctx, ctx->d_raw, std::max<size_t>((size_t)rows * C3R_WINDOW * C * sizeof(int32_t), 16))) || (rc = ensure(ctx, ctx->d_rawidx, std::max<size_t>((size_t)rows * 4, 16)))) return rc;
            f.tensors = ctx->d_raw.p; f.x16 = 0;
            z.win_idx = (int32_t *)ctx->d_rawidx.p; z.row_base = 0;
        } else {
            if ((rc = ensure(ctx, ctx->d_cand, (size_t)rows * 4)) ||
                (rc = ensure_keep(ctx, ctx->d_tensors, (size_t)(base_row + rows) * tbytes, (size_t)base_row * tbytes)) ||
                (rc = ensure_keep(ctx, ctx->d_sites_out, (size_t)(base_cand + rows) * sizeof(c3r_site_t), (size_t)base_cand * sizeof(c3r_site_t))) ||
                (rc = ensure_keep(ctx, ctx->d_winidx, (size_t)(base_cand + rows) * 4, (size_t)base_cand * 4)) ||
                (rc = ensure_keep(ctx, ctx->d_tok, (size_t)(base_tok + toks) * sizeof(c3r_token_t), (size_t)base_tok * sizeof(c3r_token_t))))
                return rc;
            f.tensors = (char *)ctx->d_tensors.p + (size_t)base_row * tbytes; f.x16 = ctx->win32 ? 0 : 1;
            z.sites = (c3r_site_t *)ctx->d_sites_out.p + base_cand;
            z.cand_idx = (int32_t *)ctx->d_cand.p;
            z.win_idx = (int32_t *)ctx->d_winidx.p + base_cand; z.row_base = (int32_t)base_row; z.tok_base = (int32_t)base_tok;
            f.tok = (c3r_token_t *)ctx->d_tok.p; f.tok_base = (int32_t)base_tok; f.tok_cap = (int32_t)toks;
        }
        f.meta = (CandMeta *)ctx->d_meta.p;
        f.n_shards = nsh; f.shard_rows = (int32_t)want_c; f.shard_toks = (int32_t)want_t;
        f.cand_cap = (int32_t)rows;
        z.meta = f.meta; z.span_info = f.span_info; z.span_base = (const int32_t *)ctx->d_spanbase.p; z.alloc = f.alloc; z.n_shards = nsh; z.shard_rows = f.shard_rows; z.overflow = f.overflow;
        z.ref = a.ref; z.ref_beg0 = a.ref_beg0; z.ref_len = a.ref_len;
        HIPCHK(ctx, hipMemsetAsync(ctx->d_lb.p, 0, lay.bytes, ctx->stream));
        if (a.giant_acc) HIPCHK(ctx, hipMemsetAsync(a.giant_acc, 0, giant_acc_bytes, ctx->stream));
        {
            Launch L(ctx, "k_tile_ranges");
            hipLaunchKernelGGL(k_tile_ranges_fused, dim3(nblk), dim3(256), 0, ctx->stream, a, &ctl->ticket_ranges, (unsigned long long *)(lb + lay.lb_ranges), nblk, (const int2 *)ctx->d_regb.p,
                               (SpanRec *)ctx->d_spanrec.p, (int32_t *)ctx->d_deep.p, &ctl->n_deep, (unsigned long long *)(lb + lay.lb_runs));
        }
        // the deep spans k_fused_tiles leaves out go to k_fused_deep: one workgroup of sixteen wavefronts per CU, spans by ticket (no deep span: the
        // workgroups leave at once).  The two kernels share nothing but the allocators and run side by side, the deep one on its own stream; under
        // the profiler (one kernel at a time, each timed on the context's stream) they run one after the other.
        const bool side = !ctx->profiling && !kn.deep_serial;
        // the giant spans' walks and allele counts, slice by slice on every CU (two workgroups each: the allele pass is round trips), before the deep
        // kernel takes the spans
        const int help_grid = (ctx->n_cu > 0 ? ctx->n_cu : 256) * kn.giant_wgs;
        auto launch_deep_kernels = [&](hipStream_t st) {          // (the timers: under the profiler only, where st is the context's stream)
            WalkArgs w{(const SpanRec *)ctx->d_spanrec.p, &ctl->ticket_walk};
            DeepArgs d{(const int32_t *)ctx->d_deep.p, &ctl->n_deep, &ctl->ticket_deep};
            with_channels(ctx, [&](auto c) {
                constexpr int CH = decltype(c)::value;
                if (a.giant_acc) { Launch L(ctx, "k_deep_walk"); hipLaunchKernelGGL(k_deep_walk<CH>, dim3(help_grid), dim3(DEEP_THREADS), 0, st, a, w); }
                if (a.giant_tab) { Launch L(ctx, "k_deep_alleles"); hipLaunchKernelGGL(k_deep_alleles<CH>, dim3(help_grid), dim3(DEEP_THREADS), 0, st, a, &ctl->ticket_alleles); }
                Launch L(ctx, "k_fused_deep");
                hipLaunchKernelGGL(k_fused_deep<CH>, dim3(deep_grid), dim3(DEEP_THREADS), 0, st, f, d);
            });
        };
        if (side) {
            if (!ctx->deep_stream) {
                // (the device's highest priority: the deep spans are the long ones — their sixteen-wavefront workgroups should get their CUs before
                // k_fused_tiles' small workgroups have filled every CU's LDS, not after)
                int least = 0, greatest = 0;
                if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); greatest = 0; }
                HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->deep_stream, hipStreamNonBlocking, greatest));
                HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
                HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
            }
            HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->deep_stream, ctx->ev_fork, 0));
            launch_deep_kernels(ctx->deep_stream);
            HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->deep_stream));
        }
        {
            Launch L(ctx, "k_fused_tiles");
            const int grid = std::min(n_tiles, 2048);
            with_channels(ctx, [&](auto c) { hipLaunchKernelGGL(k_fused_tiles<decltype(c)::value>, dim3(grid), dim3(SCAN_THREADS), 0, ctx->stream, f); });
        }
        if (side) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        else launch_deep_kernels(ctx->stream);
        {
            Launch L(ctx, "k_order_sites");
            hipLaunchKernelGGL(k_order_spans, dim3(nblk), dim3(256), 0, ctx->stream, (const int4 *)ctx->d_span.p, (const int32_t *)&ctl->n_listed, &ctl->ticket_order,
                               (unsigned long long *)(lb + lay.lb_order), (int32_t *)ctx->d_spanbase.p, &ctl->n_cand /* totals: n_cand, n_tok */);
            hipLaunchKernelGGL(k_finalize_sites, dim3((unsigned)std::min<int64_t>((rows + 15) / 16 + 1, 8192)), dim3(256), 0, ctx->stream, z);
        }
        HIPCHK(ctx, hipMemcpyAsync(&ctx->h_scan->ctl, ctl, sizeof(ScanCtl), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_scan->alloc, lb + lay.alloc, sizeof h.alloc, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        n_cand = h.ctl.n_cand; n_tok = h.ctl.n_tok;
        if (h.ctl.n_deep > 0) ctx->seen_deep = true;
        if (h.ctl.n_deep > 0 && h.ctl.n_giant != 0) ctx->seen_giant = true;
        int64_t need_c = 0, need_t = 0;          // the fullest shard
        for (int sh = 0; sh < nsh; ++sh) {
            const unsigned long long v = h.alloc[(size_t)sh * ALLOC_STRIDE];
            need_c = std::max<int64_t>(need_c, (int64_t)(uint32_t)v); need_t = std::max<int64_t>(need_t, (int64_t)(v >> 32));
        }
        if (a.dbg && a.giant_acc) {
            // events met by the giant spans' walks, slot by slot
            std::vector<int32_t> evn(GIANT_SLOTS, 0);
            for (int g = 0; g < GIANT_SLOTS; ++g)
                HIPCHK(ctx, hipMemcpy(&evn[g], a.giant_acc + (size_t)g * GIANT_STRIDE + GIANT_META, 4, hipMemcpyDeviceToHost));
            std::sort(evn.begin(), evn.end(), std::greater<int32_t>());
            fprintf(stderr, "[giant spans] %d met; events per slot, largest first:", h.ctl.n_giant);
            for (int g = 0; g < GIANT_SLOTS && evn[g] > 0; ++g) fprintf(stderr, " %d", evn[g]);
            fprintf(stderr, "\n");
        }
        if (a.dbg) {
            unsigned long long d[32];
            HIPCHK(ctx, hipMemcpy(d, ctx->d_dbg.p, sizeof d, hipMemcpyDeviceToHost));
            const double nt = d[15] ? (double)d[15] : 1.0;
            fprintf(stderr, "[k_fused_tiles] %llu spans; per span: reads in range %.1f, records in range %.1f, indel events %.1f; us per span: zero %.2f | cover+walk %.2f | scans %.2f | event buckets (LDS store) %.2f | events %.2f | gates %.2f | first-seen %.2f | select+store %.2f | tokens %.2f\n",
                    d[15], d[13] / nt, d[14] / nt, d[12] / nt, d[0] / nt / 100, d[1] / nt / 100, d[2] / nt / 100, d[5] / nt / 100, d[3] / nt / 100, d[4] / nt / 100, d[6] / nt / 100, d[7] / nt / 100, d[8] / nt / 100);
            fprintf(stderr, "   tail: row mask %.2f | scan %.2f | allocator atomic %.2f us\n", d[9] / nt / 100, d[10] / nt / 100, d[11] / nt / 100);
            fprintf(stderr, "   LDS event store: leader search (thread 0) %.2f | wait for the others %.2f us\n", d[16] / nt / 100, d[17] / nt / 100);
            if (d[18]) fprintf(stderr, "   k_fused_deep: the longest span took %.1f us (%llu records in range)\n", (double)(d[18] >> 24) / 100.0, (d[18] & 0xffffffull) << 4);
        }
        if ((h.ctl.overflow & FUSED_OVF_ORDER_TABLES) && !f.ph.rsegs) {
            // a flagged column and no tables yet: build them (this context keeps doing so from now on) and run the scan again
            ctx->legacy_wanted = true;
            if ((rc = ensure_legacy_tables(ctx))) return rc;
            f.ph.rsegs = (const DevSeg *)ctx->d_rsegs.p; f.ph.rseg_first = (const uint32_t *)ctx->d_rseg_first.p; f.ph.cigar = (const uint32_t *)ctx->d_cigar.p;
            --attempt;
            continue;
        }
        if ((h.ctl.ev_overflow & EV_OVF_DEPTH16) && !ctx->win32 && !raw_rerun) {
            if (base_row != 0) return refuse_depth16_in_batch(ctx);
            ctx->win32 = true;                 // (16-bit windows cannot hold this scan's counts: once more, with int32 windows)
            return scan_fused(ctx, kn, n_regions, ctg_starts, ctg_ends, n_candidates, false);
        }
        if (h.ctl.ev_overflow & EV_OVF_SCRATCH) return refuse_event_scratch(ctx, ev_cap);
        if (h.ctl.overflow & FUSED_OVF_TOKEN_LOST) return fail(ctx, C3R_EOVERFLOW, "internal: tokens found no slot (the gates' bound of a site's tokens was too small)");
        if (n_cand < 0 || n_tok < 0) return fail(ctx, C3R_EOVERFLOW, "too many candidates or tokens for one scan");
        if (raw_rerun) {
            if (h.ctl.overflow & FUSED_OVF_SHARD) {
                // a shard ran over: which workgroup takes a span depends on dynamic tickets and stealing across queues, so the shards' loads
                // differ from run to run and a shard that fitted in the scan itself may not fit now — grow and repeat like the scan does
                // (d_raw / d_rawidx are private to the re-run)
                if (attempt >= 2) return fail(ctx, C3R_EOVERFLOW, "internal: the raw re-run's buffers are still too small after growing (%d candidates)", n_cand);
                want_c = std::max<int64_t>(want_c, need_c + need_c / 4 + 1024);
                continue;
            }
            if (n_cand != ctx->last_cand) return fail(ctx, C3R_EINVAL, "internal: the raw re-run found %d candidates, the scan %lld", n_cand, (long long)ctx->last_cand);
            return C3R_OK;
        }
        if (need_c <= want_c && need_t <= want_t && !(h.ctl.overflow & FUSED_OVF_SHARD)) {
            if (nsh > 1) { ctx->hint_rows = (int32_t)std::min<int64_t>(need_c + need_c / 4 + 64, INT32_MAX / nsh); ctx->hint_toks = (int32_t)std::min<int64_t>(need_t + need_t / 4 + 2048, INT32_MAX / nsh); }
            break;
        }
        if (attempt >= 2) return fail(ctx, C3R_EOVERFLOW, "internal: output buffers still too small after growing (%d candidates, %d tokens)", n_cand, n_tok);
        want_c = std::max<int64_t>(want_c, need_c + need_c / 4 + 1024);
        want_t = std::max<int64_t>(want_t, need_t + need_t / 4 + 1024);
    }
    ctx->last_cand = n_cand; ctx->last_shards = nsh; ctx->last_shard_rows = (int32_t)want_c;
    ctx->scan_counts[0] = h.ctl.n_listed; ctx->scan_counts[1] = h.ctl.n_deep; ctx->scan_counts[2] = h.ctl.n_giant; ctx->scan_counts[3] = h.ctl.n_help;
    if (n_candidates) *n_candidates = n_cand;
    ctx->n_cand = base_cand + n_cand;
    ctx->n_tok += n_tok;
    // (one allocator: dense output, the next scan of the batch appends; several: the scan's whole row / token space is taken)
    ctx->n_rows = base_row + (nsh == 1 ? (int64_t)n_cand : want_c * nsh);
    // (token SLOTS: what the allocators handed out — a site reserves the gates' bound and n_tok counts what was written)
    ctx->n_tokspace = base_tok + (nsh == 1 ? (int64_t)(h.alloc[0] >> 32) : want_t * nsh);
    return C3R_OK;
}

int c3r_pileup_scan_regions(c3r_ctx *ctx, int32_t n_regions, const int64_t *ctg_starts, const int64_t *ctg_ends, int64_t *n_candidates) {
    if (!ctx || n_regions < 1 || !ctg_starts || !ctg_ends) return C3R_EINVAL;
    if (ctx->ref_len == 0) return fail(ctx, C3R_EINVAL, "c3r_set_reference must be called before c3r_pileup_scan");
    for (int r = 0; r < n_regions; ++r) {
        if (ctg_ends[r] < ctg_starts[r]) return C3R_EINVAL;
        // (the scan kernels add up to two tiles and a flank to a region position in plain int: C3R_CTG_END_MAX leaves them 1024, include/c3r.h)
        if (ctg_ends[r] > C3R_CTG_END_MAX) return fail(ctx, C3R_EINVAL, "region %d ends beyond C3R_CTG_END_MAX = %lld (2^31 - 1 - 33 - 1024)", r, (long long)C3R_CTG_END_MAX);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n_candidates) *n_candidates = 0;
    { const int rc_af = af_table(ctx); if (rc_af) return rc_af; }
    ctx->last_starts.assign(ctg_starts, ctg_starts + n_regions); ctx->last_ends.assign(ctg_ends, ctg_ends + n_regions);
    ctx->last_scan_pruned = false;
    memset(ctx->scan_counts, 0, sizeof ctx->scan_counts);          // (a fused scan that succeeds fills them in)
    // The plain mode runs in one fused tile kernel (k_fused_tiles).  Head/tail calling (the end-of-stream rule needs the last row of the
    // whole region), splice padding (in-place column edits, candidate after candidate) and genotyping mode (candidates in intron-only
    // spans) keep the column store and its selection / compaction / gather kernels.
    const ScanKnobs kn = read_scan_knobs(ctx);
    const bool fused = !ctx->prm.head_tail && !ctx->prm.splice_padding && !ctx->prm.genotyping_mode && !kn.no_fuse;
    ctx->last_fused = fused;
    return fused ? scan_fused(ctx, kn, n_regions, ctg_starts, ctg_ends, n_candidates, false)
                 : scan_column_store(ctx, kn, n_regions, ctg_starts, ctg_ends, n_candidates, false);
}

int c3r_pileup_scan(c3r_ctx *ctx, int64_t ctg_start, int64_t ctg_end, int64_t *n_candidates) {
    return c3r_pileup_scan_regions(ctx, 1, &ctg_start, &ctg_end, n_candidates);
}

int c3r_batch_begin(c3r_ctx *ctx) {
    if (!ctx) return C3R_EINVAL;
    ctx->batching = true; ctx->n_cand = 0; ctx->n_tok = 0; ctx->n_rows = 0; ctx->n_tokspace = 0; ctx->last_cand = 0; ctx->last_base = 0;
    return C3R_OK;
}

int c3r_batch_end(c3r_ctx *ctx) {
    if (!ctx) return C3R_EINVAL;
    ctx->batching = false;
    return C3R_OK;
}

int c3r_get_scan_counts(c3r_ctx *ctx, int32_t *listed, int32_t *deep, int32_t *giant, int32_t *slices) {
    if (!ctx) return C3R_EINVAL;
    if (listed) *listed = ctx->scan_counts[0];
    if (deep) *deep = ctx->scan_counts[1];
    if (giant) *giant = ctx->scan_counts[2];
    if (slices) *slices = ctx->scan_counts[3];
    return C3R_OK;
}

int c3r_batch_count(c3r_ctx *ctx, int64_t *n_sites, int64_t *n_tokens) {
    if (!ctx) return C3R_EINVAL;
    if (n_sites) *n_sites = ctx->n_cand;
    if (n_tokens) *n_tokens = ctx->n_tok;
    return C3R_OK;
}

int c3r_get_tensors(c3r_ctx *ctx, int rescaled, int32_t *tensors, int64_t cap_sites) {
    if (!ctx || !tensors) return C3R_EINVAL;
    if (cap_sites < ctx->n_cand) return fail(ctx, C3R_EOVERFLOW, "need room for %lld sites", (long long)ctx->n_cand);
    if (ctx->n_cand == 0) return C3R_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int row_ints = C3R_WINDOW * ctx->prm.channels;
    const size_t bytes = (size_t)ctx->n_cand * row_ints * 4;
    const void *src = ctx->d_tensors.p;
    const int32_t *idx = (const int32_t *)ctx->d_winidx.p;       // the fused path stores windows in arrival order
    if (!rescaled) {
        // raw (un-rescaled) windows are rebuilt for the most recent scan only
        if (ctx->last_base != 0 || ctx->last_cand != ctx->n_cand)
            return fail(ctx, C3R_EINVAL, "raw tensors are only available for a single (non-batched) scan");
        if (ctx->last_fused) {               // the fused path keeps no columns: the scan runs again, un-rescaled windows only
            int rc = scan_fused(ctx, read_scan_knobs(ctx), (int32_t)ctx->last_starts.size(), ctx->last_starts.data(), ctx->last_ends.data(), nullptr, true);
            if (rc) return rc;
            idx = (const int32_t *)ctx->d_rawidx.p;
        } else {
            if (!ctx->prm.splice_padding) {     // (splice padding: the scan already kept the raw windows, the columns have moved on)
                int rc = ensure(ctx, ctx->d_raw, bytes);
                if (rc) return rc;
                if ((rc = run_gather(ctx, 0, ctx->d_raw.p, false, false))) return rc;
            }
            idx = nullptr;
        }
        src = ctx->d_raw.p;
    }
    if (idx) {
        int rc = ensure(ctx, ctx->d_export, bytes);
        if (rc) return rc;
        // (the resident windows are int16 rows in arrival order: gathered into position order and widened; a raw re-run's are int32)
        hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)std::min<int64_t>((ctx->n_cand + 3) / 4, 8192)), dim3(256), 0, ctx->stream, src, idx, (int)ctx->n_cand, row_ints,
                           (int32_t *)ctx->d_export.p, (rescaled && !ctx->win32) ? 1 : 0);
        src = ctx->d_export.p;
    }
    HIPCHK(ctx, hipMemcpyAsync(tensors, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}

int c3r_get_sites(c3r_ctx *ctx, c3r_site_t *sites, int64_t cap_sites) {
    if (!ctx || !sites) return C3R_EINVAL;
    if (cap_sites < ctx->n_cand) return fail(ctx, C3R_EOVERFLOW, "need room for %lld sites", (long long)ctx->n_cand);
    if (ctx->n_cand == 0) return C3R_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(sites, ctx->d_sites_out.p, (size_t)ctx->n_cand * sizeof(c3r_site_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // on the device a site's tokens lie where its span's token slots were handed out; c3r_get_tokens returns them site after site
    uint32_t off = 0;
    for (int64_t i = 0; i < ctx->n_cand; ++i) { sites[i].tok_off = off; off += (uint32_t)sites[i].n_tok; }
    return C3R_OK;
}

int c3r_token_count(c3r_ctx *ctx, int64_t *n_tokens) {
    if (!ctx || !n_tokens) return C3R_EINVAL;
    *n_tokens = ctx->n_tok;
    return C3R_OK;
}

int c3r_get_tokens(c3r_ctx *ctx, c3r_token_t *tokens, int64_t cap_tokens) {
    if (!ctx || !tokens) return C3R_EINVAL;
    if (cap_tokens < ctx->n_tok) return fail(ctx, C3R_EOVERFLOW, "need room for %lld tokens", (long long)ctx->n_tok);
    if (ctx->n_tok == 0) return C3R_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // site order (see c3r_get_sites): offsets = exclusive sums of the sites' token counts, then one wavefront per site copies its run
    const int n = (int)ctx->n_cand;
    int rc; RowCtl *ctl = nullptr;
    if ((rc = ensure(ctx, ctx->d_tokoff, (size_t)(n + 2) * 4)) || (rc = ensure(ctx, ctx->d_tokexp, (size_t)ctx->n_tok * sizeof(c3r_token_t))) || (rc = row_ctl(ctx, &ctl))) return rc;
    hipLaunchKernelGGL(k_site_ntok, dim3((unsigned)(n / 256 + 1)), dim3(256), 0, ctx->stream, (const c3r_site_t *)ctx->d_sites_out.p, n, (int32_t *)ctx->d_tokoff.p);
    if ((rc = device_excl_scan(ctx, (int32_t *)ctx->d_tokoff.p, n + 1, &ctl->export_toks))) return rc;
    hipLaunchKernelGGL(k_export_tokens, dim3((unsigned)std::min<int64_t>((n + 3) / 4, 8192)), dim3(256), 0, ctx->stream, (const c3r_site_t *)ctx->d_sites_out.p,
                       (const int32_t *)ctx->d_tokoff.p, n, (const c3r_token_t *)ctx->d_tok.p, (c3r_token_t *)ctx->d_tokexp.p);
    HIPCHK(ctx, hipMemcpyAsync(tokens, ctx->d_tokexp.p, (size_t)ctx->n_tok * sizeof(c3r_token_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    return C3R_OK;
}

int c3r_get_pad_insertions(c3r_ctx *ctx, c3r_padins_t *out, int64_t cap, int64_t *n) {
    if (!ctx || !n) return C3R_EINVAL;
    const int64_t have = ctx->padins ? (int64_t)ctx->padins->size() : 0;
    *n = have;
    if (!out) return C3R_OK;
    if (cap < have) return fail(ctx, C3R_EOVERFLOW, "need room for %lld entries", (long long)have);
    if (have) memcpy(out, ctx->padins->data(), (size_t)have * sizeof(c3r_padins_t));
    return C3R_OK;
}

int c3r_get_columns(c3r_ctx *ctx, int64_t *region_start, int64_t *n_pos, int32_t *cols, int32_t *depth, uint8_t *flags, int64_t cap_pos) {
    if (!ctx) return C3R_EINVAL;
    if (region_start) *region_start = (int64_t)ctx->reg_beg0 + 1;
    // the first region of the most recent scan (its slots start at 0 and are contiguous)
    const int64_t npos0 = (int64_t)ctx->reg_end0 - ctx->reg_beg0;
    if (n_pos) *n_pos = npos0;
    if (!cols && !depth && !flags) return C3R_OK;
    if (cap_pos < npos0) return fail(ctx, C3R_EOVERFLOW, "need room for %lld positions", (long long)npos0);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const ScanKnobs kn = read_scan_knobs(ctx);
    if (ctx->last_fused) {
        // the fused path never materialises columns: build those of the scan's first region now, through the column store
        if (ctx->last_starts.empty()) return fail(ctx, C3R_EINVAL, "no scan yet");
        int rc = af_table(ctx);
        if (!rc) rc = scan_column_store(ctx, kn, 1, ctx->last_starts.data(), ctx->last_ends.data(), nullptr, true);
        ctx->geo_key.clear();                // (the device now holds the column store's geometry)
        if (rc) return rc;
    }
    if (ctx->last_scan_pruned) {
        // the scan skipped intron-only tiles that no candidate window can reach: compute their row flags now
        ScanArgs a = ctx->last_scan;
        a.tile_list = a.tile_list2; a.n_tile_list = a.n_tile_list2;
        with_channels(ctx, [&](auto c) { hipLaunchKernelGGL(k_scan_tiles<decltype(c)::value>, dim3(std::min((int)a.n_tiles, kn.list_grid)), dim3(SCAN_THREADS), 0, ctx->stream, a); });
        ctx->last_scan_pruned = false;
        HIPCHK(ctx, hipGetLastError());
    }
    const size_t n = (size_t)npos0;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(cols, ctx->d_cols.p, n * ctx->prm.channels * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (depth) HIPCHK(ctx, hipMemcpyAsync(depth, ctx->d_depth.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (flags) HIPCHK(ctx, hipMemcpyAsync(flags, ctx->d_flags.p, n, hipMemcpyDeviceToHost, ctx->stream));
    const size_t n_tiles = (n + TILE - 1) / TILE;
    std::vector<uint8_t> tc(n_tiles);
    HIPCHK(ctx, hipMemcpyAsync(tc.data(), ctx->d_tile_cols.p, n_tiles, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // tiles that hold no aligned base are not materialised on the device: their columns are all-zero by definition
    for (size_t t = 0; t < n_tiles; ++t) {
        if (tc[t]) continue;
        const size_t p0 = t * TILE, p1 = std::min(n, p0 + TILE);
        if (cols) memset(cols + p0 * ctx->prm.channels, 0, (p1 - p0) * ctx->prm.channels * 4);
        if (depth) for (size_t q = p0; q < p1; ++q) depth[q] = 0;        // (rows of such a tile show ref-skips only: depth 0)
    }
    return C3R_OK;
}

// ------------------------------------------------------------------------------------------------
int64_t c3r_weight_count(int channels) { return net_weight_count(channels); }

// Precision "auto" (3): the fp8-corrected path (precision 2) is ~10x less exact than the split-f16 path and its error grows fast with
// the weights' norm, so it is used only where it has been MEASURED: both paths run on 2048 pileup-shaped
// windows drawn from a fixed seed and the probabilities must agree to C3R_MX_GUARD, a 2.5x margin under the 1e-4 tolerance.
static constexpr double C3R_MX_GUARD = 4e-5;
// The split-f16 path itself (precision 1, the default) is fp32-equivalent only while its operands fit f16 with the layer's scale and the
// products do not cancel pathologically; nothing in clair3_rna/model.py:126-172 bounds a trained model's weights.  So it is MEASURED too:
// the same calibration windows through the fp32 MFMA path (precision 0) and through split-f16 must agree to C3R_F16_GUARD, else the context
// runs the fp32 path and says so (stderr, c3r_get_precision, c3r_get_precision_guard).  The guard is the parity tolerance itself, 1e-4, and
// not a fraction of it, because of what the two paths were measured to do as the weights' gain grows (profiles/r5/f16_guard_vs_weight_norm.txt:
// N(0, 0.05) test weights times 1 / 2 / 3 / 4 / 6): they drift apart by 2.9e-6 / 2.3e-5 / 8.4e-5 / 1.4e-4 / 2.7e-4 — and each of them drifts
// from the fp32 oracle by the SAME 2.4e-6 / 1.8e-5 / 7.9e-5 / 8.8e-5 / 3.3e-4: at high gain the network is ill-conditioned in fp32 itself
// (summation order, hardware exp2 / rcp), and the fp32 MFMA path is no closer to the oracle than split-f16 is.  A tighter guard would send
// such weights to a path three times slower for no gain in parity; what the guard is for — an operand that overflows f16, a scale that
// flushes lo halves, a NaN — shows up as a disagreement of 1e-3 .. 1.
static constexpr double C3R_F16_GUARD = 1e-4;
static void calibration_windows(int C, int n, std::vector<int32_t> &X) {
    X.assign((size_t)n * C3R_WINDOW * C, 0);
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint32_t m) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)((st >> 11) % m); };
    static const int depths[6] = {6, 12, 20, 40, 90, 216};
    for (int s_ = 0; s_ < n; ++s_) {
        const int depth = depths[rnd(6)];
        for (int t = 0; t < C3R_WINDOW; ++t) {
            int32_t *col = &X[((size_t)s_ * C3R_WINDOW + t) * C];
            const int k = (int)rnd(4);
            int fwd = 0;
            for (int i = 0; i < depth; ++i) fwd += (int)rnd(2);
            col[k] = -fwd; col[9 + k] = -(depth - fwd);                     // the reference-base channels carry minus the strand totals
            for (int r = (int)rnd(3); r > 0; --r) col[rnd((uint32_t)C)] += 1 + (int)rnd((uint32_t)std::max(1, depth / 3));
        }
    }
}
// max |dP| between two precisions on the calibration windows (a NaN on either side counts as 1.0)
static int calibrate_pair(c3r_ctx *ctx, int mode_a, int mode_b, double *err_out) {
    const int C = ctx->net.channels, n = 2048;
    std::vector<int32_t> X;
    calibration_windows(C, n, X);
    int32_t *d_x = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d_x, X.size() * 4));
    std::vector<float> p1((size_t)n * C3R_NPROB), p2(p1.size());
    const int keep = ctx->net.precision;
    auto run = [&](int mode, std::vector<float> &out) -> int {
        ctx->net.precision = mode;
        std::string e;
        int rc = net_forward(ctx->net, d_x, nullptr, n, ctx->stream, [](const char *, int) {}, e);
        if (rc) return fail(ctx, rc, "%s", e.c_str());
        HIPCHK(ctx, hipMemcpyAsync(out.data(), ctx->net.d_probs, out.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return C3R_OK;
    };
    int rc = C3R_OK;
    if (hipMemcpyAsync(d_x, X.data(), X.size() * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = C3R_EHIP;
    if (!rc) rc = run(mode_a, p1);
    if (!rc) rc = run(mode_b, p2);
    (void)hipFree(d_x);
    ctx->net.precision = keep;
    if (rc) return rc;
    double worst = 0.0;
    for (size_t i = 0; i < p1.size(); ++i) {
        const double d = std::fabs((double)p1[i] - (double)p2[i]);
        worst = (d == d) ? std::max(worst, d) : 1.0;                          // (a NaN disqualifies)
    }
    *err_out = worst;
    return C3R_OK;
}
static int apply_precision(c3r_ctx *ctx) {
    const int req = ctx->precision_req;
    ctx->net.precision = req == 3 ? 1 : req;
    ctx->f16_fell_back = false;
    if (!ctx->net.loaded || req == 0) return C3R_OK;                          // decided when the weights arrive
    const bool rts = ctx->net.wlog2[0] != 12 || ctx->net.wlog2[1] != 12 || ctx->net.wlog2[2] != 12;
    int rc;
    // ---- the guard of the split-f16 arithmetic: once per set of weights
    // (C3R_NO_F16_GUARD=1: development aid for timing probes whose kernels compute garbage on purpose, such as profiles/r5/y1_traffic_probe.txt's)
    static const bool no_guard = [] { const char *e = getenv("C3R_NO_F16_GUARD"); return e && *e == '1'; }();
    if (no_guard) ctx->f16_calib_err = 0.0;
    if (ctx->f16_calib_err < 0.0) {
        double err = 1.0;
        if ((rc = calibrate_pair(ctx, 0, 1, &err))) { ctx->net.precision = 0; return rc; }
        ctx->f16_calib_err = err;
    }
    if (ctx->f16_calib_err > C3R_F16_GUARD) {
        ctx->net.precision = 0; ctx->f16_fell_back = true;
        fprintf(stderr, "[c3r] warning: with these weights the split-f16 network differs from the fp32 one by %.3g on the calibration windows (guard %.0e): "
                        "running the fp32 MFMA path (c3r_set_precision 0), about a third of the speed\n", ctx->f16_calib_err, C3R_F16_GUARD);
        return C3R_OK;
    }
    if (req == 1) return C3R_OK;
    if (rts) {                                                                // (the fp8 fragments are built for the 2^12 scale)
        if (req == 2) { ctx->net.precision = 1; return fail(ctx, C3R_EINVAL, "precision 2 (f16 + fp8 corrections) needs weights that fit the 2^12 split-f16 scale: max |w| < 8 per layer"); }
        ctx->net.precision = 1;
        return C3R_OK;
    }
    if (req == 2) return C3R_OK;
    double err = -1.0;
    if ((rc = calibrate_pair(ctx, 1, 2, &err))) { ctx->net.precision = 1; return rc; }
    ctx->mx_calib_err = err;
    ctx->net.precision = err <= C3R_MX_GUARD ? 2 : 1;
    return C3R_OK;
}

int c3r_load_weights(c3r_ctx *ctx, const float *blob, int64_t n_floats, int channels) {
    if (!ctx || !blob) return C3R_EINVAL;
    if (channels != C3R_CH && channels != C3R_CH_PHASED) return fail(ctx, C3R_EINVAL, "channels must be 18 or 30");
    if (n_floats != net_weight_count(channels))
        return fail(ctx, C3R_EINVAL, "weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)net_weight_count(channels));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string e;
    int rc = net_load(ctx->net, blob, channels, ctx->stream, e);
    if (rc) return fail(ctx, rc, "%s", e.c_str());
    ctx->mx_calib_err = -1.0; ctx->f16_calib_err = -1.0;
    return apply_precision(ctx);
}

int c3r_set_precision(c3r_ctx *ctx, int mode) {
    if (!ctx || mode < 0 || mode > 3) return C3R_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->precision_req = mode;
    return apply_precision(ctx);
}

int c3r_get_precision(c3r_ctx *ctx, int *mode_in_use, double *calibration_err) {
    if (!ctx) return C3R_EINVAL;
    if (mode_in_use) *mode_in_use = ctx->net.precision;
    if (calibration_err) *calibration_err = ctx->mx_calib_err;
    return C3R_OK;
}

int c3r_get_precision_guard(c3r_ctx *ctx, double *f16_err, int32_t *scale_log2, int *fell_back) {
    if (!ctx) return C3R_EINVAL;
    if (f16_err) *f16_err = ctx->f16_calib_err;
    if (scale_log2) for (int l = 0; l < 3; ++l) scale_log2[l] = ctx->net.wlog2[l];
    if (fell_back) *fell_back = ctx->f16_fell_back ? 1 : 0;
    return C3R_OK;
}

int c3r_reserve(c3r_ctx *ctx, int64_t n_sites) {
    if (!ctx || n_sites < 0) return C3R_EINVAL;
    if (!ctx->net.loaded) return fail(ctx, C3R_EINVAL, "c3r_load_weights must be called before c3r_reserve");
    if (n_sites == 0) return C3R_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string e;
    int rc = net_reserve(ctx->net, n_sites, ctx->stream, e);
    if (rc) return fail(ctx, rc, "%s", e.c_str());
    return C3R_OK;
}

int c3r_infer(c3r_ctx *ctx, const int32_t *tensors, int64_t n, float *probs) {
    if (!ctx || n < 0) return C3R_EINVAL;
    if (!ctx->net.loaded) return fail(ctx, C3R_EINVAL, "c3r_load_weights must be called before c3r_infer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int C = ctx->net.channels;
    const void *d_x = nullptr;
    const int32_t *d_rows = nullptr;
    const bool x16 = tensors == nullptr && !ctx->win32;  // the resident windows are int16 (unless the read set needed int32), a caller's batch int32
    if (tensors == nullptr) {
        if (C != ctx->prm.channels) return fail(ctx, C3R_EINVAL, "weights are for %d channels, scan produced %d", C, ctx->prm.channels);
        if (n != ctx->n_cand) return fail(ctx, C3R_EINVAL, "n=%lld but %lld candidates are resident", (long long)n, (long long)ctx->n_cand);
        d_x = ctx->d_tensors.p;
        d_rows = (const int32_t *)ctx->d_winidx.p;       // windows lie in arrival order (k_fused_tiles)
    } else if (n > 0) {
        int rc = ensure(ctx, ctx->d_raw, (size_t)n * C3R_WINDOW * C * 4);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_raw.p, tensors, (size_t)n * C3R_WINDOW * C * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!probs) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // the caller's buffer must be free to go when we return
        d_x = ctx->d_raw.p;
    }
    if (n == 0) return C3R_OK;
    {
        // layer 1 addresses a window by a 32-bit element index (k_lstm1_rs): the rows it can be asked for — the resident windows' row space, or the
        // caller's batch — must stay below 2^32 / (33 * channels) = 7.2 M rows at 18 channels (a GRCh38 chromosome holds one to two million candidates)
        const int64_t rows = tensors == nullptr ? std::max<int64_t>(ctx->n_rows, n) : n;
        if ((uint64_t)rows * (uint64_t)(C3R_WINDOW * C) >= (1ull << 32))
            return fail(ctx, C3R_EINVAL, "%lld window rows of %d channels exceed the network's 32-bit row addressing: call c3r_infer on smaller batches", (long long)rows, C);
    }
    std::string e;
    if (ctx->net.d_tmo) HIPCHK(ctx, hipMemsetAsync(ctx->net.d_tmo, 0, 4, ctx->stream));     // (a time-out fails the batch it happened in, not the ones after it)
    // the network's kernels go to the context's default-priority stream, behind everything queued on `stream` so far (the tensors, an
    // uploaded batch); whatever is queued on `stream` afterwards (probabilities, rows, the next batch's tensors) comes behind them
    hipStream_t nst = ctx->net_stream ? ctx->net_stream : ctx->stream;
    if (ctx->net_stream) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_x, ctx->stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->net_stream, ctx->ev_x, 0));
    }
    auto prof = [&](const char *name, int phase) {
        if (!ctx->profiling) return;
        if (phase == 0) (void)hipEventRecord(ctx->ev0, nst);
        else {
            (void)hipEventRecord(ctx->ev1, nst); (void)hipEventSynchronize(ctx->ev1);
            float ms = 0; (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
            KStat &k = ctx->kstats[name]; k.ms += ms; k.n += 1;
        }
    };
    int rc = net_forward(ctx->net, d_x, d_rows, n, nst, prof, e, x16);
    if (ctx->net_stream) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_net, ctx->net_stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_net, 0));
    }
    if (rc) return fail(ctx, rc, "%s", e.c_str());
    if (probs) {
        int32_t *st = nullptr;
        if ((rc = queue_lstm_status(ctx, &st))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(probs, ctx->net.d_probs, (size_t)n * C3R_NPROB * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if ((rc = check_lstm_status(ctx, st))) return rc;
    }
    HIPCHK(ctx, hipGetLastError());
    return C3R_OK;
}

int c3r_get_probs(c3r_ctx *ctx, float *probs, int64_t n) {
    if (!ctx || !probs || n < 0) return C3R_EINVAL;
    if (n == 0) return C3R_OK;
    if (!ctx->net.d_probs || n > ctx->net.cap_probs) return fail(ctx, C3R_EINVAL, "no probabilities resident for %lld sites", (long long)n);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t *st = nullptr;
    int rc = queue_lstm_status(ctx, &st);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(probs, ctx->net.d_probs, (size_t)n * C3R_NPROB * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return check_lstm_status(ctx, st);
}

// ------------------------------------------------------------------------------------------------ A8 on the host
int c3r_decode_text(const char *ctg, int64_t n, const int32_t *pos, const char *ref33s, int ref33_stride, const char *const *alt_infos,
                    const float *probs, int qual, int show_ref, char *out, int64_t cap, int64_t *out_len) {
    if (!ctg || n < 0 || (n && (!pos || !ref33s || !alt_infos || !probs)) || !out_len) return C3R_EINVAL;
    std::string rows;
    for (int64_t i = 0; i < n; ++i) {
        int depth; AltDict alt;
        parse_alt_info(alt_infos[i], depth, alt);
        vcf_row(ctg, pos[i], ref33s + (size_t)i * ref33_stride, depth, alt, probs + (size_t)i * C3R_NPROB, qual, show_ref != 0, rows);
    }
    *out_len = (int64_t)rows.size();
    if (!out || cap < (int64_t)rows.size() + 1) return C3R_EOVERFLOW;
    memcpy(out, rows.c_str(), rows.size() + 1);
    return C3R_OK;
}

// ---- row snapshots: everything the decoder needs of one batch, on the host, detached from the context
}  // extern "C"
struct c3r_rows {
    c3r_ctx *ctx = nullptr;
    // one staging block (rows_stage): sites | token bytes | probabilities | indel-record offsets
    void *stage = nullptr; size_t stage_cap = 0;
    int64_t n = 0;
    c3r_site_t *sites = nullptr; uint8_t *tokb = nullptr; float *probs = nullptr; uint32_t *rec_off = nullptr;
    std::shared_ptr<HostReads> hr;                        // the contig's read headers and packed bases (inserted bases of the alt alleles)
    std::shared_ptr<PadInsTab> padins;                    // mpileup_compat = 1: its insertions with pads (null / empty otherwise)
    const DevRead *reads = nullptr; const uint8_t *seq = nullptr;
    const c3r_read_t *creads = nullptr;                   // c3r_rows_begin_ex: the caller's own records and bases are read in place (no copy back)
    TokRec *recs = nullptr; int64_t n_recs = 0;           // the tokens that carry an indel (k_pack_tokens), own allocation
    int ref_slot = -1; const char *ref = nullptr; size_t ref_len = 0; int64_t ref_start1 = 1;
    std::string rows; int64_t rows_count = 0;
    int64_t info_sites = 0, info_tokb = 0, info_recs = 0; // c3r_rows_info: what left the device (kept when the inputs are released)
};
namespace {
// device -> the snapshot's (ordinary) memory, in stream order; the large arrays through the context's page-locked buffers (big_d2h: complete on return)
int rows_d2h(c3r_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes >= PIN_MIN && pin_ring_on()) return big_d2h(ctx, dst, src, bytes);
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return C3R_OK;
}
// drop_ref_calls: only the sites that can print a row without --show_ref leave the device.  k_row_keep flags them, an exclusive scan turns the flags into row
// numbers (d_keep, read by k_pack_rows) and the host waits for their count.  (the keep decision reads the probabilities: the layer-2 time-out word is checked
// with the same wait, before the count is acted on — a timed-out batch whose garbage looks like RefCalls must fail, not come back as an empty snapshot)
int rows_keep_count(c3r_ctx *ctx, RowCtl *ctl, int64_t n_all, int64_t *n_keep) {
    int rc; int32_t *lstm_st = nullptr;
    if ((rc = ensure(ctx, ctx->d_keep, (size_t)(n_all + 2) * 4))) return rc;
    hipLaunchKernelGGL(k_row_keep, dim3((unsigned)(n_all / 256 + 1)), dim3(256), 0, ctx->stream, (const c3r_site_t *)ctx->d_sites_out.p, (const float *)ctx->net.d_probs, (int)n_all,
                       (int32_t *)ctx->d_keep.p);
    if ((rc = device_excl_scan(ctx, (int32_t *)ctx->d_keep.p, (int)n_all + 1, &ctl->n_keep)) || (rc = queue_lstm_status(ctx, &lstm_st))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(&ctx->h_rowctl->n_keep, &ctl->n_keep, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *n_keep = ctx->h_rowctl->n_keep;
    return check_lstm_status(ctx, lstm_st);
}
// the staging block for r->n sites and, at most, the token bytes of the whole slot space.  -> *need: its bytes
int rows_stage(c3r_ctx *ctx, c3r_rows *r, size_t *need) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t n = (size_t)r->n, b_sites = up(n * sizeof(c3r_site_t)), b_tokb = up((size_t)std::max<int64_t>(ctx->n_tokspace, 1)), b_probs = up(n * C3R_NPROB * sizeof(float));
    *need = b_sites + b_tokb + b_probs + up(n * 4);
    r->stage = stage_take(ctx, *need, true, &r->stage_cap);
    if (!r->stage) return fail(ctx, C3R_ENOMEM, "staging block of %zu bytes: allocation failed", r->stage_cap);
    r->sites = (c3r_site_t *)r->stage; r->tokb = (uint8_t *)r->stage + b_sites;
    r->probs = (float *)(r->tokb + b_tokb); r->rec_off = (uint32_t *)(r->tokb + b_tokb + b_probs);
    return C3R_OK;
}
// where the decoder reads inserted bases: the caller's own arrays, else the context's host copy of the loaded contig.  -> that copy is new and still to be filled
// (rows_copy_out; the context gets it when the snapshot is complete: a half-copied cache is no cache)
bool rows_read_source(c3r_ctx *ctx, c3r_rows *r, const c3r_read_t *host_reads, const uint8_t *host_seq) {
    r->padins = ctx->padins;
    if (host_reads) { r->creads = host_reads; r->seq = host_seq; return false; }
    r->hr = ctx->host_cache;
    if (!r->hr) r->hr = std::make_shared<HostReads>(HostReads{std::vector<DevRead>((size_t)std::max(ctx->n_reads, 1)), std::vector<uint8_t>((size_t)ctx->n_seq_bytes + 16)});
    r->reads = r->hr->reads.data(); r->seq = r->hr->seq.data();
    return !ctx->host_cache;
}
// tokens leave the device packed (export_kernels.hpp: a byte per token, 16-byte records for the tokens with an indel): all n_all sites where they lie, or — `drop` —
// the r->n kept ones back to back, their records and probabilities with them
int rows_pack(c3r_ctx *ctx, const c3r_rows *r, RowCtl *ctl, bool drop, int64_t n_all) {
    const size_t n_tok = (size_t)std::max<int64_t>(ctx->n_tokspace, 1);   // (token bytes are addressed through the sites' tok_off: the whole slot space)
    int rc;
    if ((rc = ensure(ctx, ctx->d_tokb, n_tok)) || (rc = ensure(ctx, ctx->d_tokrec, n_tok * sizeof(TokRec))) || (rc = ensure(ctx, ctx->d_recoff, (size_t)r->n * 4))) return rc;
    if (drop && ((rc = ensure(ctx, ctx->d_sites_c, (size_t)r->n * sizeof(c3r_site_t))) || (rc = ensure(ctx, ctx->d_probs_c, (size_t)r->n * C3R_NPROB * sizeof(float))))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctl, 0, offsetof(RowCtl, n_keep), ctx->stream));         // n_recs, n_bytes
    Launch L(ctx, "k_pack_tokens");
    if (drop)
        hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)((n_all + 3) / 4)), dim3(256), 0, ctx->stream, (const c3r_site_t *)ctx->d_sites_out.p, (const c3r_token_t *)ctx->d_tok.p,
                           (const float *)ctx->net.d_probs, (const int32_t *)ctx->d_keep.p, n_all, (c3r_site_t *)ctx->d_sites_c.p, (float *)ctx->d_probs_c.p, (uint8_t *)ctx->d_tokb.p,
                           (TokRec *)ctx->d_tokrec.p, (uint32_t *)ctx->d_recoff.p, &ctl->n_recs);
    else
        hipLaunchKernelGGL(k_pack_tokens, dim3((unsigned)((n_all + 3) / 4)), dim3(256), 0, ctx->stream, (const c3r_site_t *)ctx->d_sites_out.p, (const c3r_token_t *)ctx->d_tok.p, n_all,
                           (uint8_t *)ctx->d_tokb.p, (TokRec *)ctx->d_tokrec.p, (uint32_t *)ctx->d_recoff.p, &ctl->n_recs);
    return C3R_OK;
}
// counters, sites, token bytes, record offsets, the read source when it is fresh, probabilities: one wait at the end, behind the time-out word (only the snapshot
// without RefCalls sizes its token copy from the counters and waits for them); then (*t_main) the indel records, in an allocation of the snapshot's own
int rows_copy_out(c3r_ctx *ctx, c3r_rows *r, const RowCtl *ctl, bool drop, bool fresh_reads, TimePt *t_main) {
    const size_t n = (size_t)r->n;
    int64_t n_tok = ctx->n_tokspace;
    int rc; int32_t *lstm_st = nullptr;
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_rowctl, ctl, offsetof(RowCtl, n_keep), hipMemcpyDeviceToHost, ctx->stream));
    if (drop) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); n_tok = (int64_t)ctx->h_rowctl->n_bytes; }      // (the kept sites' token bytes lie back to back)
    const void *d_sites = drop ? ctx->d_sites_c.p : ctx->d_sites_out.p, *d_probs = drop ? ctx->d_probs_c.p : (const void *)ctx->net.d_probs;
    if ((rc = rows_d2h(ctx, r->sites, d_sites, n * sizeof(c3r_site_t))) || (rc = rows_d2h(ctx, r->tokb, ctx->d_tokb.p, (size_t)n_tok)) || (rc = rows_d2h(ctx, r->rec_off, ctx->d_recoff.p, n * 4)) ||
        (fresh_reads && ((rc = rows_d2h(ctx, r->hr->reads.data(), ctx->d_reads.p, (size_t)ctx->n_reads * sizeof(DevRead))) || (rc = rows_d2h(ctx, r->hr->seq.data(), ctx->d_seq.p, (size_t)ctx->n_seq_bytes + 16)))) ||
        (rc = queue_lstm_status(ctx, &lstm_st)) || (rc = rows_d2h(ctx, r->probs, d_probs, n * C3R_NPROB * sizeof(float))))
        return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    r->n_recs = (int64_t)ctx->h_rowctl->n_recs;
    r->info_sites = r->n; r->info_tokb = n_tok; r->info_recs = r->n_recs;
    *t_main = now();
    if ((rc = check_lstm_status(ctx, lstm_st)) || r->n_recs <= 0) return rc;
    r->recs = (TokRec *)huge_alloc((size_t)r->n_recs * sizeof(TokRec));
    if (!r->recs) return fail(ctx, C3R_ENOMEM, "indel records of %lld tokens: allocation failed", (long long)r->n_recs);
    if ((rc = rows_d2h(ctx, r->recs, ctx->d_tokrec.p, (size_t)r->n_recs * sizeof(TokRec)))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return C3R_OK;
}
}  // namespace
extern "C" {

int c3r_rows_begin(c3r_ctx *ctx, c3r_rows **out) { return c3r_rows_begin_ex(ctx, 0, nullptr, nullptr, out); }

int c3r_rows_begin_ex(c3r_ctx *ctx, int drop_ref_calls, const c3r_read_t *host_reads, const uint8_t *host_seq, c3r_rows **out) {
    if (!ctx || !out || ((host_reads == nullptr) != (host_seq == nullptr))) return C3R_EINVAL;
    *out = nullptr;
    const int64_t n_all = ctx->n_cand;
    if (n_all > 0 && (!ctx->net.d_probs || n_all > ctx->net.cap_probs)) return fail(ctx, C3R_EINVAL, "c3r_infer must run before c3r_call_rows");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<c3r_rows, void (*)(c3r_rows *)> guard(new c3r_rows(), c3r_rows_free);        // (every exit but release() frees the snapshot)
    c3r_rows *const r = guard.get();
    r->ctx = ctx; r->n = n_all;
    const bool drop = drop_ref_calls != 0;
    int rc; size_t need = 0; RowCtl *ctl = nullptr;
    if (n_all && ((rc = row_ctl(ctx, &ctl)) || (drop && (rc = rows_keep_count(ctx, ctl, n_all, &r->n))))) return rc;
    if (r->n == 0) { *out = guard.release(); return C3R_OK; }       // (no candidates, or none kept)
    if ((rc = rows_stage(ctx, r, &need))) return rc;
    const bool fresh_reads = rows_read_source(ctx, r, host_reads, host_seq);
    const bool timing = getenv("C3R_TIMING") != nullptr;
    const auto t0 = now();
    if (timing) (void)hipStreamSynchronize(ctx->stream);              // (separates the wait for the network from the copies in the report)
    auto t1 = now(), t2 = t1;
    if ((rc = rows_pack(ctx, r, ctl, drop, n_all)) || (rc = rows_copy_out(ctx, r, ctl, drop, fresh_reads, &t2))) return rc;
    if (timing)
        fprintf(stderr, "[rows_begin %p] %lld sites, %lld tokens (%lld with an indel): wait %.1f ms, pack + copies (%.0f MB) %.1f ms, indel records (%.0f MB) %.1f ms\n", (void *)ctx,
                (long long)r->n, (long long)r->info_tokb, (long long)r->n_recs, ms(t0, t1), need / 1e6, ms(t1, t2), r->n_recs * sizeof(TokRec) / 1e6, ms(t2, now()));
    r->ref_slot = ctx->ref_cur; r->ref = ctx->h_ref; r->ref_len = ctx->ref_len; r->ref_start1 = ctx->ref_start1;
    if (r->ref_slot >= 0) ctx->refbuf[r->ref_slot].users.fetch_add(1);
    if (fresh_reads) ctx->host_cache = r->hr;
    *out = guard.release();
    return C3R_OK;
}

int c3r_rows_decode(c3r_rows *r, const char *ctg, int qual, int show_ref, int64_t *out_len, int64_t *n_rows) {
    if (!r || !ctg || !out_len) return C3R_EINVAL;
    r->rows.clear(); r->rows_count = 0;
    *out_len = 0; if (n_rows) *n_rows = 0;
    const int64_t n = r->n;
    if (n == 0) return C3R_OK;
    const c3r_site_t *sites = r->sites; const uint8_t *tokb = r->tokb; const TokRec *recs = r->recs; const uint32_t *rec_off = r->rec_off; const float *probs = r->probs;
    const uint8_t *seq = r->seq;
    const DevRead *reads = r->reads;
    const RefView refv{r->ref, r->ref_len};
    const int64_t ref_start1 = r->ref_start1;
    const c3r_read_t *creads = r->creads;
    auto get_read = [&](uint32_t k) { return creads ? ReadView{seq, creads[k].seq_off, creads[k].l_seq} : ReadView{seq, reads[k].seq_off, reads[k].l_seq}; };
    const PadView pads{r->padins && !r->padins->empty() ? r->padins->data() : nullptr, r->padins ? r->padins->size() : 0};
    // host threads: C3R_THREADS, else up to 32 (one process per GPU shares the node's cores with its peers)
    unsigned nt = std::max(1u, std::min(32u, usable_cpus()));
    if (const char *e = getenv("C3R_THREADS")) nt = (unsigned)std::max(1, atoi(e));
    if ((int64_t)nt * 64 > n) nt = 1;
    std::vector<std::string> part(nt);
    std::vector<int64_t> cnt(nt, 0);
    auto work = [&](unsigned t) {
        const int64_t a = n * t / nt, b = n * (t + 1) / nt;
        AltDict alt;
        for (int64_t i = a; i < b; ++i) {
            int depth_tok;
            const uint8_t *tb = tokb + sites[(size_t)i].tok_off;
            const TokRec *rc_ = recs ? recs + rec_off[(size_t)i] : nullptr;      // this site's indel records, in token order
            alt_from_stream(sites[(size_t)i].n_tok, [tb, rc_](int k) mutable {
                const uint8_t by = tb[k];
                if (by & 0x80) { const TokRec &q = *rc_++; return TokView{by & 31, q.indel, q.read_idx, q.qpos, q.del_after, (by & 0x20) != 0}; }
                return TokView{by & 31, 0, 0u, 0u, 0u, (by & 0x20) != 0};
            }, get_read, refv, ref_start1, sites[(size_t)i].pos, alt, depth_tok, pads, sites[(size_t)i].depth);
            if (vcf_row(ctg, sites[(size_t)i].pos, sites[(size_t)i].ref33, sites[(size_t)i].depth, alt, probs + (size_t)i * C3R_NPROB, qual,
                        show_ref != 0, part[t]))
                cnt[t]++;
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    size_t total = 0;
    for (unsigned t = 0; t < nt; ++t) total += part[t].size();
    r->rows.reserve(total + 1);
    for (unsigned t = 0; t < nt; ++t) { r->rows += part[t]; r->rows_count += cnt[t]; }
    *out_len = (int64_t)r->rows.size();
    if (n_rows) *n_rows = r->rows_count;
    return C3R_OK;
}

int c3r_rows_info(const c3r_rows *r, int64_t *n_sites, int64_t *n_token_bytes, int64_t *n_indel_records) {
    if (!r) return C3R_EINVAL;
    if (n_sites) *n_sites = r->info_sites;
    if (n_token_bytes) *n_token_bytes = r->info_tokb;
    if (n_indel_records) *n_indel_records = r->info_recs;
    return C3R_OK;
}

int c3r_rows_get(c3r_rows *r, char *out, int64_t cap) {
    if (!r || !out) return C3R_EINVAL;
    if (cap < (int64_t)r->rows.size() + 1) return C3R_EOVERFLOW;
    memcpy(out, r->rows.c_str(), r->rows.size() + 1);
    return C3R_OK;
}

// give back what only the decode needed (reference buffer, staging block, read copies); the rows text stays
static void rows_release_inputs(c3r_rows *r) {
    c3r_ctx *ctx = r->ctx;
    if (r->ref_slot >= 0) { ctx->refbuf[r->ref_slot].users.fetch_sub(1); r->ref_slot = -1; r->ref = nullptr; r->ref_len = 0; }
    if (r->stage) stage_give(ctx, r->stage, r->stage_cap);
    r->stage = nullptr; r->stage_cap = 0; r->sites = nullptr; r->tokb = nullptr; r->probs = nullptr; r->rec_off = nullptr; r->reads = nullptr; r->seq = nullptr; r->creads = nullptr;
    if (r->recs) { free(r->recs); r->recs = nullptr; r->n_recs = 0; }
    r->n = 0;
}

void c3r_rows_free(c3r_rows *r) {
    if (!r) return;
    rows_release_inputs(r);
    delete r;
}

// the one-call form: snapshot + decode on this thread; the rows stay with the context until the next call
int c3r_call_rows(c3r_ctx *ctx, const char *ctg, int qual, int show_ref, int64_t *out_len, int64_t *n_rows) {
    if (!ctx || !ctg || !out_len) return C3R_EINVAL;
    if (ctx->rows_snap) { c3r_rows_free(ctx->rows_snap); ctx->rows_snap = nullptr; }
    *out_len = 0; if (n_rows) *n_rows = 0;
    const bool timing = getenv("C3R_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = c3r_rows_begin(ctx, &ctx->rows_snap);
    if (rc) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    rc = c3r_rows_decode(ctx->rows_snap, ctg, qual, show_ref, out_len, n_rows);
    rows_release_inputs(ctx->rows_snap);          // (only the text is kept for c3r_get_rows: no reference buffer stays pinned by it)
    if (timing)
        fprintf(stderr, "[c3r_call_rows] snapshot (D2H of sites, tokens, probabilities, read bases) %.1f ms, decode %.1f ms\n", ms(t0, t1), ms(t1, now()));
    return rc;
}

int c3r_get_rows(c3r_ctx *ctx, char *out, int64_t cap) {
    if (!ctx || !out) return C3R_EINVAL;
    static const std::string empty;
    const std::string &rows = ctx->rows_snap ? ctx->rows_snap->rows : empty;
    if (cap < (int64_t)rows.size() + 1) return fail(ctx, C3R_EOVERFLOW, "need %lld bytes", (long long)rows.size() + 1);
    memcpy(out, rows.c_str(), rows.size() + 1);
    return C3R_OK;
}

// ------------------------------------------------------------------------------------------------
int c3r_set_profiling(c3r_ctx *ctx, int enabled) {
    if (!ctx) return C3R_EINVAL;
    ctx->profiling = enabled != 0;
    return C3R_OK;
}
int c3r_reset_kernel_stats(c3r_ctx *ctx) {
    if (!ctx) return C3R_EINVAL;
    ctx->kstats.clear();
    return C3R_OK;
}
int c3r_get_kernel_stats(c3r_ctx *ctx, const char **names, double *total_ms, int64_t *launches, int cap, int *n) {
    if (!ctx || !n) return C3R_EINVAL;
    ctx->kstat_names.clear();
    for (auto &kv : ctx->kstats) ctx->kstat_names.push_back(kv.first);
    int i = 0;
    for (auto &kv : ctx->kstats) {
        if (i < cap) {
            if (names) names[i] = ctx->kstat_names[i].c_str();
            if (total_ms) total_ms[i] = kv.second.ms;
            if (launches) launches[i] = kv.second.n;
        }
        ++i;
    }
    *n = i;
    return C3R_OK;
}

}  // extern "C"
