/* c3r.h — C-ABI of libc3r.so, the MI355X-native pileup variant-calling hot path for Clair3-RNA.
 *
 * The reference has NO plugin / FFI seam for this path: the boundary is a pair of sub-processes joined
 * by a text pipe, launched per (contig, chunk) by clair3_rna/call_var_bam.py:288-295.  This header is
 * therefore the seam the build defines; each entry point names the reference code it
 * replaces.  INTEGRATION.md shows the ctypes stub a maintainer adds to call_var_bam.py.
 *
 * Conventions: plain C, no exceptions across the boundary.  Every call returns 0 on success or a
 * negative C3R_E* code; c3r_last_error(ctx) returns a human-readable message.  The caller owns all
 * host buffers; the library owns all device memory inside the opaque c3r_ctx.  One context = one
 * GPU = one HIP stream (plus, inside the library, a second one on which the tensor build's deep-span kernel runs beside the
 * other); contexts are independent (one process or thread per GPU, no collectives: chunks are independent work items,
 * run_clair3_rna:681-706).  Several contexts of one process may share a device, each driven by its own host thread (two
 * pipelined contexts: one uploads while the other computes): c3r_load_reads lets only one of them upload at a time per device, so
 * that they stay out of phase on the PCIe link.  A single context is not re-entrant.
 *
 * There is NO CPU fallback: every compute entry point fails with C3R_ENODEVICE when no gfx950 device
 * is usable.
 */
#ifndef C3R_H
#define C3R_H

#include <stddef.h>
#include <stdint.h>

#include "c3r_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define C3R_OK 0
#define C3R_EINVAL (-1)       /* bad argument / call order */
#define C3R_ENODEVICE (-2)    /* no usable HIP device */
#define C3R_EHIP (-3)         /* a HIP runtime call failed */
#define C3R_ENOMEM (-4)
#define C3R_EUNSUPPORTED (-5) /* valid in the reference, not implemented on the GPU path yet */
#define C3R_EOVERFLOW (-6)    /* caller buffer too small */

typedef struct c3r_ctx c3r_ctx;
typedef struct c3r_rows c3r_rows;   /* a batch's decode inputs on the host, detached from the context (c3r_rows_begin) */

/* ---- lifetime ------------------------------------------------------------------------------ */
/* Library version string, e.g. "c3r 0.1 (gfx950)". */
const char *c3r_version(void);
/* Create a context on HIP device `device_id`.  `stream` may be NULL (the library creates its own
 * non-blocking stream) or an existing hipStream_t the caller wants the work ordered on. */
int c3r_create(int device_id, void *stream, c3r_ctx **out);
void c3r_destroy(c3r_ctx *ctx);
/* c3r_destroy keeps up to two of the largest device blocks (the 8.9-GB layer-1 output of a full network slice) for the process's next
 * context: the driver clears freed memory before it hands it out again, 0.8 s for a block of that size.  c3r_trim() gives them back
 * (for a host application that destroys its contexts to return HBM to other users of the GPU); returns the bytes released.
 * C3R_NO_BLOCK_CACHE=1 turns the cache off. */
int64_t c3r_trim(void);
const char *c3r_last_error(const c3r_ctx *ctx);
/* Block until all work queued on the context's stream is complete. */
int c3r_synchronize(c3r_ctx *ctx);
/* The hipStream_t the context launches on (for event timing by the caller). */
void *c3r_stream(c3r_ctx *ctx);

/* ---- configuration ------------------------------------------------------------------------- */
/* Fill `p` with the defaults run_clair3_rna forwards to call_var_bam (run_clair3_rna:684-705;
 * shared/param_p.py:20,41,88-90). */
void c3r_default_params(c3r_params_t *p);
/* Replaces the argparse surface of src/create_tensor_pileup.py:660-778 that affects tensors.
 * splice_padding=1 (src/create_tensor_pileup.py:573-593) is supported, also together with head_tail=1
 * (including the reference's shared pre-fill column, [[0]*C]*33, that padding edits in place). */
int c3r_set_params(c3r_ctx *ctx, const c3r_params_t *p);

/* ---- coordinates --------------------------------------------------------------------------- */
/* Positions are 32-bit on the device.  The accepted domain, and what refuses a value outside it (C3R_EINVAL with a message):
 *   reads (c3r_load_reads): pos is 0-based and >= 0; the 0-based EXCLUSIVE end pos + reference length of the CIGAR is at most INT32_MAX
 *     (2,147,483,647), i.e. a read's last base lies on 1-based 2,147,483,647 at most — "read <i> ends beyond 2^31".  One CIGAR op holds 2^28 - 1.
 *   regions (c3r_pileup_scan, c3r_pileup_scan_regions): 1-based, ctg_start <= ctg_end <= C3R_CTG_END_MAX = 2,147,482,590 — "region <r> ends
 *     beyond C3R_CTG_END_MAX".  The rows of a region reach ctg_end + 33, and the kernels add up to two tiles of 256 positions and a flank of 16 to
 *     a row's position in 32-bit arithmetic: the limit leaves them 1024 below INT32_MAX.  A start below 34 is clamped (rows begin at 1).
 *     Reads may lie, and end, above the last accepted region end; a scan never looks at more of them than its rows.
 *   reference slice (c3r_set_reference, c3r_set_reference_view): 1-based ref_start >= 1 and ref_start - 1 + len <= INT32_MAX — "reference slice
 *     ends beyond 2^31".
 *   BED intervals (c3r_set_bed): 0-based half-open int32 pairs, 0 <= start < end <= INT32_MAX; they are only compared with row positions.
 *   genotyping sites (c3r_set_sites): 1-based int32, 1 .. INT32_MAX; only compared.
 *   phase sites and query sites (c3r_set_phase_sites, c3r_set_phase_alleles, c3r_hap_counts, c3r_hap_allele_counts, c3r_phase_links, c3r_phase_unit_links, c3r_phase_allele_links, c3r_phase_allele_unit_links): 1-based
 *     int32 pos, 1 .. INT32_MAX, compared with read positions in 64-bit arithmetic; ps is a name (a position by convention), -1 or 0 .. INT32_MAX.
 * GRCh38 chr1 is 248,956,422 bp; BAI indexing ends at 2^29.  tests/test_gpu_coords.py runs the kernels at chr1 scale, at 2^28 and on the last
 * accepted and first refused values above. */
#define C3R_CTG_END_MAX 2147482590LL          /* INT32_MAX - 33 - 1024 */

/* ---- inputs -------------------------------------------------------------------------------- */
/* Hand over one contig's aligned reads, sorted by pos (BAM order), as flat host-resident records.  Replaces the BAM side of
 * `samtools mpileup <bam> -r ...` (src/create_tensor_pileup.py:446-451): the records are copied to the device as they are and
 * everything htslib's per-read CIGAR cursor would do while streaming them — dropping pads / hard clips / empty ops, folding
 * = and X, the split at N ops into aligned segments with their reference / query offsets, the segment order, the expanded op
 * table — happens there (csrc/reads_kernels.hpp), with one host synchronisation to report sizes and validation errors.
 * Filtering by excl_flags / min_mq happens on the device too.  cigars: BAM-encoded ops; seq4: 4-bit packed bases.
 * This call is part of the measured path (bench.py times it inside every step). */
int c3r_load_reads(c3r_ctx *ctx, const c3r_read_t *reads, int64_t n_reads,
                   const uint32_t *cigars, int64_t n_cigar_ops, const uint8_t *seq4, int64_t n_seq_bytes);
/* Page-locked host memory for the arrays handed to c3r_load_reads: from such buffers the three uploads are truly asynchronous
 * DMA transfers (~55 GB/s); from ordinary pageable memory the HIP runtime stages them through its own buffer first.  Optional —
 * any host pointer works.  The caller frees with c3r_host_free. */
void *c3r_host_alloc(size_t bytes);
void c3r_host_free(void *p);
/* Upload the reference slice covering the region.  ref[0] is 1-based position `ref_start`;
 * replaces reference_sequence_from / `samtools faidx` (shared/utils.py:168-194,
 * src/create_tensor_pileup.py:424-428).  Upper-cased on upload like the reference does. */
int c3r_set_reference(c3r_ctx *ctx, int64_t ref_start, const char *ref, int64_t len);
/* The same for a slice the caller already holds UPPER-CASED (c3r_fasta_fetch, include/c3r_io.h) and keeps alive and unchanged until
 * the context has been given another reference AND every row snapshot (c3r_rows_begin) taken meanwhile has been freed: no host copy
 * is made — the upload reads the caller's bytes and so does the decoder.  (c3r_set_reference's pass over a 250-Mb chromosome is
 * 40-250 ms of the calling thread.) */
int c3r_set_reference_view(c3r_ctx *ctx, int64_t ref_start, const char *ref_upper, int64_t len);
/* Optional interval filters, 0-based half-open, for the current contig.  which=0: `-l` column
 * filter (mpileup -l extend_bed, src/create_tensor_pileup.py:443); which=1: confident-bed candidate
 * filter (is_region_in, src/create_tensor_pileup.py:551-554).  n=0 clears. */
int c3r_set_bed(c3r_ctx *ctx, int which, const int32_t *start_end_pairs, int64_t n);
/* Genotyping mode site list (--vcf_fn; src/create_tensor_pileup.py:399-407,555-556), 1-based. */
int c3r_set_sites(c3r_ctx *ctx, const int32_t *sites, int64_t n);
/* Haplotagging on the device: the phased heterozygous SNVs of the contig (what `whatshap phase` / `longphase phase` wrote,
 * run_clair3_rna:729-767), sorted by strictly increasing pos.  While a table is set, every c3r_load_reads computes each read's haplotype from
 * it as part of read preparation (k_haplotag, csrc/haplotag_kernels.hpp) and the 30-channel tensor build uses that tag INSTEAD of the
 * record's own hp — the "Haplotag the BAM" step of the reference flow (run_clair3_rna:769-801: whatshap / longphase haplotag, samtools
 * index) is not needed.  The rule, per read, whatever excl_flags / min_mq say: walk the CIGAR (M, = and X consume reference and query, D and
 * N the reference, I and S the query, H, P and empty ops nothing); a site under an M / = / X op at a query offset below l_seq votes when
 * the read's base there is the site's ref (allele 0) or alt (allele 1) — for haplotype 1 when allele == h1, else for haplotype 2; votes
 * are counted per phase set as (c1, c2); the read's phase set is the one with the most votes (equal: the one whose first voting site on
 * the read comes first); hp = 1 if c1 > c2, 2 if c2 > c1, else 0.  This is whatshap's per-phase-set majority with unit weights and the
 * allele read off the CIGAR position: no realignment (c3r_set_hap_realign lifts it), and no base-quality weights (c3r_set_hap_min_bq, below, lifts it as far as a threshold does,
 * c3r_set_hap_bq_weights, below, with the weights themselves).
 * n = 0 clears the table: nothing is launched then and the records' own hp count again.  C3R_EINVAL, naming the first bad index, for an
 * unsorted or repeated position, pos < 1, a base code other than 1, 2, 4, 8, ref == alt, h1 > 1 or ps < 0.  Valid before or after c3r_load_reads
 * with the same result: when reads are loaded their tables are rebuilt from the records the device holds (as c3r_set_params does for new
 * filters).  The table stays for later c3r_load_reads calls until it is replaced. */
int c3r_set_phase_sites(c3r_ctx *ctx, const c3r_phase_site_t *sites, int64_t n);
/* The tags of the loaded reads, in load order (hp: [cap], cap >= the number of loaded reads; may be NULL), and their statistics (may be
 * NULL).  C3R_EINVAL when no phase sites are set. */
int c3r_get_haplotags(c3r_ctx *ctx, uint8_t *hp, int64_t cap, c3r_haplotag_stats_t *stats);
/* The phase set every loaded read's tag was decided in, in load order (ps: [cap], cap >= the number of loaded reads): the ps of the set the
 * rule above picks — most votes, equal: the earlier first voting site — and -1 for a read whose tag is 0 (no vote, or a tie).  k_haplotag
 * stores it beside the tag, so it follows the table like the tags do.  C3R_EINVAL when no phase sites are set. */
int c3r_get_read_phase_sets(c3r_ctx *ctx, int32_t *ps, int64_t cap);
/* Per-haplotype allele counts at called sites, and the phase of a heterozygous call from them: what phases the FINAL VCF once the reads are
 * tagged, and, written out, the haplotype support of every call.  c3r_hap_counts: biallelic SNVs only; c3r_hap_allele_counts (below):
 * SNVs, insertions, deletions and sites with two ALT alleles.  Both are a majority rule over CIGAR-position alleles (no realignment (c3r_set_hap_realign lifts it), no
 * base qualities).
 *
 * Query sites (c3r_hap_counts): sorted by strictly increasing pos; ref and alt are valid; ps >= 0 is the phase set to count against; h1 is
 * ignored; validated as in c3r_set_phase_sites (except h1), naming the first bad index.
 * Voters: as for c3r_phase_links — the loaded reads that the tensor build keeps under the current parameters (read_kept), without the
 * depth cap: the counts describe the reads the caller sees.
 * Observation: as in c3r_set_phase_sites — a site under an M / = / X op at a query offset below l_seq; a = 0 when the read's base there is
 * the site's ref, 1 when it is alt, 2 when it is another one of the codes 1, 2, 4, 8; nothing for any other code (=, N, IUPAC).
 * Row: t = the read's tag (1 or 2) when the read's phase set (c3r_get_read_phase_sets) equals the site's ps, else t = 0 — untagged reads,
 * ties and reads tagged in another set.
 * Counts: every observation adds one to counts[j][t][a], uint32 [n][3][3].  All sums are integers: neither read order nor arrival order
 * shows.
 * Assignment (c3r_hap_assign), per site: v1 = counts[j][1][1] + counts[j][2][0] (ALT on haplotype-1 reads, REF on haplotype-2 reads),
 * v0 = counts[j][1][0] + counts[j][2][1], w = v0 + v1.  The site is accepted iff w >= min_reads, v0 != v1 and
 * 100 max(v0, v1) >= min_agree_pct w — the agreement test of c3r_phase_resolve, in 64-bit products.  Accepted: ps = the query's ps,
 * h1 = (v1 > v0).  Otherwise ps = -1, h1 = 0.  The t = 0 row and the a = 2 column never enter the decision: they are reported, not used.
 *
 * c3r_hap_counts needs a phase table (C3R_EINVAL without one, whatever n is); no reads loaded: every count is 0; n = 0 succeeds and launches
 * nothing.  It uploads the sites, clears a device table, runs k_hap_counts (csrc/hapcount_kernels.hpp) on the context's stream and reads
 * the table back (36 n bytes).  It changes neither the reads' haplotags, nor the table of c3r_set_phase_sites, nor anything a scan reads.
 * Its device buffers are allocated at the first call and kept.
 * c3r_hap_assign is host code like c3r_phase_resolve: no context, no device.  p = NULL: the defaults (2, 75).  C3R_EINVAL for
 * min_reads < 0 or min_agree_pct outside 0 .. 100.  stats may be NULL.  out may be `in`. */
int c3r_hap_counts(c3r_ctx *ctx, const c3r_phase_site_t *sites, int64_t n, uint32_t *counts);
int c3r_hap_assign(const c3r_phase_site_t *in, int64_t n, const uint32_t *counts, const c3r_phase_params_t *p, c3r_phase_site_t *out,
                   c3r_hap_assign_stats_t *stats);
/* The same counts for a heterozygous call whose two alleles may be SNVs, insertions or deletions: `0/1` rows with an indel ALT and `1/2` rows
 * (`C  T,CGG`, `ACC  A,TCC`).  Opt-in (hap_vcf --indels), like `whatshap phase --indels`.  The alleles are read off the CIGAR position: no
 * realignment, no left-alignment of the reads' indels, no base qualities (c3r_set_hap_min_bq lifts it as a threshold, c3r_set_hap_bq_weights as weights of the tagging's votes); agreement with `whatshap --indels` is not measured.  This is where
 * the rule is stated; phasing.allele_candidates_from_vcf, csrc/hapcount_kernels.hpp and tests/hapalleleref.py restate it.
 *
 * Alleles of a VCF row: REF r and an ALT a, upper-cased, letters of ACGT only; the common SUFFIX is stripped while both are longer than one
 * letter (only suffixes: the anchor is always POS).  Then: one letter each and different — an SNV (base = the ALT letter, event NONE); r
 * one letter, a longer and starting with r — an insertion (base = r[0], event INS(the rest of a)); a one letter, r longer and starting with
 * a — a deletion (base = r[0], event DEL(len(r) - 1)); anything else — the row is skipped (`complex_allele`).  The REF allele is (r[0], NONE).
 * GT 0/1 or 1/0 with one ALT: A = REF, B = the ALT; GT 1/2 or 2/1 with two ALTs that both reduce and differ: A = the first, B = the second.
 * base_matters = one of A, B is an SNV; event_matters = one of them is an insertion or a deletion.
 *
 * Observation of a read at a site with anchor P, on the read's NORMALISED CIGAR (H, empty ops and pads dropped — a pad survives, as an op that
 * consumes nothing, only directly before a D that does not follow an I —, = and X folded into M, equal neighbours merged): P must lie under an
 * M op (first reference base x, first query base y, length len) at offset dd with q = y + dd < l_seq, else nothing (a P under D or N:
 * nothing).  b = the read's 4-bit code at q.  Event: dd < len - 1: NONE.  dd = len - 1: by the next op — an I directly followed by a D:
 * OTHER (the `+<ins>-<del>` column; equals no allele's event); an I of n bases that do not all lie below l_seq: no observation; an I of n
 * bases: INS(the codes at y + len .. y + len + n - 1); a D of n: DEL(n); anything else (N, S, the pad before a D, the read's end): NONE.
 * Where event_matters is 0 the event is not looked at (an insertion cut off by a short SEQ then does not drop the base before it).
 * base_matters and b not one of 1, 2, 4, 8: no observation.  The read shows allele (B, E) when (base_matters is 0 or b == B) and
 * (event_matters is 0 or the event equals E — INS: the same length and the same codes).  Column = 0 for A, else 1 for B, else 2.
 * On a site whose alleles are REF and one SNV this is c3r_hap_counts' rule: events are ignored.
 * Voters, row and counts are those of c3r_hap_counts, and c3r_hap_assign runs on the table with "REF" read as allele A and "ALT" as allele B
 * (it reads pos and ps only): accepted with h1 = 0 the GT is A|B (0|1, 1|2), with h1 = 1 it is B|A (1|0, 2|1).
 *
 * ins_pool: the inserted bases of all INS alleles, 4-bit packed like a read's SEQ (base 2k in the high nibble of byte k), pool_bases of them
 * (NULL when 0).  Preconditions and side effects are c3r_hap_counts': it needs a phase table; n = 0 launches nothing; no reads loaded: every
 * count is 0; it changes nothing a scan or the tags read; its device buffers are allocated at the first call and kept
 * (k_hap_allele_counts, csrc/hapcount_kernels.hpp).  C3R_EINVAL, naming the first bad index, for an unsorted or repeated pos, pos < 1,
 * ps < 0, a flag other than 0 / 1, a base code (of an allele or in the pool of an insertion) outside 1, 2, 4, 8, an unknown kind, an indel
 * of length 0 (or a length on kind NONE), an insertion that runs past the pool, or two equal alleles. */
int c3r_hap_allele_counts(c3r_ctx *ctx, const c3r_hap_site_t *sites, int64_t n, const uint8_t *ins_pool, int64_t pool_bases, uint32_t *counts);
/* Haplotagging from a table that also holds phased insertions, deletions and two-ALT sites (`0|1` rows with an indel ALT, `1|2` rows): what
 * `--phase_output --phase_indels` and `whatshap phase --indels` write.  Opt-in (--haplotag_indels).  It is c3r_set_phase_sites with the
 * observation of c3r_hap_allele_counts in the place of "the read's base is ref or alt" — the two contracts above, joined, and nothing else:
 *  Table: sites sorted by strictly increasing pos, ps >= 0; alleles A and B, base_matters, event_matters and the pool exactly as in
 *   c3r_hap_allele_counts.  h1[j] = 0: allele A lies on haplotype 1 (GT 0|1 or 1|2); h1[j] = 1: allele B does (GT 1|0 or 2|1).
 *  Voters: c3r_set_phase_sites' — every loaded read, whatever excl_flags / min_mq say (not read_kept).
 *  Observation: the column of c3r_hap_allele_counts at the site (normalised CIGAR, the event behind the anchor as defined there): columns 0
 *   (A) and 1 (B) vote, column 2 (another allele) and no observation do not; the vote is for haplotype 1 when the column equals h1[j],
 *   else for haplotype 2.
 *  Decision: c3r_set_phase_sites', unchanged — votes per phase set, the set with the most votes (equal: the one whose first voting site
 *   comes first in the table), hp = 1 / 2 / 0 from c1 against c2; the winning set is kept for c3r_get_read_phase_sets.
 * On a table whose sites are all REF-and-one-SNV this IS c3r_set_phase_sites' rule, bit for bit (tags, sets and statistics): there the
 * column is 0 for ref, 1 for alt, and 2 or nothing for every other code.
 * Limits, as for both parents: the alleles are read off the CIGAR position — no realignment (c3r_set_hap_realign lifts it), no left-alignment of the reads' indels, no
 * base qualities; a read whose aligner placed an indel one repeat unit away from the VCF's anchor shows "another allele" and does not
 * vote.  Agreement with `whatshap haplotag` (which, as far as we recall and have not checked, reads indel rows of a phased VCF too) is
 * not measured.
 * One table at a time: this call replaces the table of c3r_set_phase_sites and that call replaces this one's; n = 0 on either clears the
 * table (nothing is launched then and the records' own hp count again).  Valid before or after c3r_load_reads with the same result (the
 * tags are rebuilt as c3r_set_phase_sites rebuilds them); the caller's arrays may go once the call returns (the device holds a copy
 * with h1 folded into the site records).  c3r_load_reads runs k_haplotag_alleles (csrc/haplotag_kernels.hpp) in k_haplotag's place
 * while this table is the one set.  c3r_get_haplotags, c3r_get_read_phase_sets, c3r_hap_counts and c3r_hap_allele_counts treat either
 * table as "a phase table is set".  C3R_EINVAL, naming the first bad index, for everything c3r_hap_allele_counts refuses and for
 * h1 > 1; after such a refusal (and only then) the table set before stays in force.  A device failure while the new table is copied
 * (C3R_ENOMEM, C3R_EHIP) is different: where the table before was an allele table its buffers are the ones being overwritten, so the
 * context then holds no table at all (the getters answer as without one) until a setter succeeds; a table of c3r_set_phase_sites, which
 * lives in buffers of its own, stays. */
int c3r_set_phase_alleles(c3r_ctx *ctx, const c3r_hap_site_t *sites, const uint8_t *h1, int64_t n, const uint8_t *ins_pool, int64_t pool_bases);
/* Phasing on the device from read linkage: what stands where `whatshap phase` / `longphase phase` stand in the reference flow
 * (run_clair3_rna:729-767), in two steps.  It is a GREEDY LINKAGE CHAIN, not whatshap's wMEC: every heterozygous SNV gets a block and an
 * orientation from the reads that cover it together with one of the K = C3R_PHASE_LINKS sites before it, once, in table order.
 *
 * Input: the contig's candidate sites, sorted by strictly increasing pos; ref and alt are valid, ps and h1 are ignored; validated as in
 * c3r_set_phase_sites (except ps and h1).
 * Voters: the loaded reads that the tensor build keeps under the current c3r_params — the excl_flags / min_mq test of read preparation
 * (one function, csrc/pileup_kernels.hpp: read_kept) — without the depth cap.  This DIFFERS from c3r_set_phase_sites, where every loaded
 * read is tagged whatever the filters say: a phase inferred from MAPQ-0 reads is worse than none.
 * Observation: exactly as in c3r_set_phase_sites — a site under an M / = / X op at a query offset below l_seq shows allele 0 when the read's
 * base there is the site's ref, allele 1 when it is alt, otherwise nothing.
 * Links (c3r_phase_links): links[j][k - 1][0] = the voting reads that observe both site j and site j - k with the SAME allele index (cis),
 * links[j][k - 1][1] = those with different indices (trans), k = 1 .. K.  The predecessors are the K sites before j in the table, not "on
 * the read".  Entries with j - k < 0 are 0.  All sums are integers: neither read order nor arrival order shows.
 * Resolution (c3r_phase_resolve), sequential over j = 0 .. n - 1, every processed site holding (block_j, h1_j): group the predecessors
 * i = j - k by block; per block b, v1_b = sum over its i of (h1_i ? cis : trans), v0_b = sum of (h1_i ? trans : cis), w_b = v0_b + v1_b.
 * b is accepted iff w_b >= min_reads, v0_b != v1_b and 100 max(v0_b, v1_b) >= min_agree_pct w_b.  Among the accepted blocks the one with
 * the largest |v1_b - v0_b| is taken (equal: the block that holds the nearest predecessor); block_j = b, h1_j = (v1_b > v0_b).  No accepted
 * block: j opens a new block with h1_j = 0.  Blocks are NEVER MERGED afterwards (a site that links two blocks joins one of them).  The
 * agreement test keeps sites that are not haplotype-linked (an A>G RNA-editing site called 0/1: cis and trans near equal) out of a block
 * instead of letting them flip one.
 * Output: a site in a block of two or more gets ps = the pos of the block's first site (whatshap's convention) and its h1; a site alone in
 * its block gets ps = -1 and h1 = 0 — the caller drops it before c3r_set_phase_sites.
 *
 * c3r_phase_links needs c3r_load_reads before it (no reads loaded: every count is 0); it uploads the sites, clears a device table, runs
 * k_phase_links (csrc/phase_kernels.hpp) on the context's stream and reads the table back (links: [n][K][2], 64 n bytes).  It changes
 * neither the reads' haplotags, nor the table of c3r_set_phase_sites, nor anything a scan reads.  n = 0 succeeds and launches nothing.
 * Its device buffers are allocated at the first call and kept.
 * c3r_phase_resolve is host code: no context, no device (it works on a machine without a GPU).  The resolution is a dependency chain of
 * n steps of K terms — tens of thousands of sites per contig: under a millisecond on one core, tens of milliseconds on one wavefront —
 * and the table it reads is 64 n bytes, so it is not a kernel.  p = NULL: the defaults (2, 75).  stats may be NULL.  out may be `in`. */
int c3r_phase_links(c3r_ctx *ctx, const c3r_phase_site_t *sites, int64_t n, uint32_t *links);
int c3r_phase_resolve(const c3r_phase_site_t *in, int64_t n, const uint32_t *links, const c3r_phase_params_t *p, c3r_phase_site_t *out,
                      c3r_phase_stats_t *stats);
/* The block-merge stage: an optional step after the chain that joins the blocks which reads bridge.  The chain gives a site its block from
 * the K table sites before it and from nothing else, so a run of K + 1 or more sites that belong to no haplotype (RNA-editing sites called
 * 0/1, a hyper-edited Alu stretch: they fail the agreement test, stay alone and still fill the predecessor slots) cuts a block in two
 * however many reads span the run.  The stage applies the chain's own rule once more, one level up: to whole blocks instead of sites.
 *
 * Input: a table as c3r_phase_resolve leaves it — ps = -1 (a site without a block) or ps >= 1, and h1 (0 or 1).
 * One LEVEL:
 *  1. Units: the distinct ps >= 0 of the table, numbered 0 .. U - 1 by increasing ps.  A site with ps = -1 is no unit and takes no part.  The
 *     sites of a unit need not be contiguous in the table (blocks interleave).
 *  2. Voters: as for c3r_phase_links — the loaded reads that the tensor build keeps under the current c3r_params, without the depth cap.
 *  3. A read's observation of unit u: over the unit's sites that the read observes (the observation rule of c3r_phase_links), c1 = those
 *     whose allele index equals the site's h1, c2 = the others.  The read shows haplotype 1 when c1 > c2, haplotype 2 when c2 > c1 and
 *     NOTHING when c1 == c2 (a tied unit is not observed, and neither is one with no observed site).
 *  4. Unit links (c3r_phase_unit_links): ulinks[u][k - 1][0] = the voting reads that observe both unit u and unit u - k with the same
 *     haplotype, [1] = with different ones, k = 1 .. K = C3R_PHASE_LINKS: the K unit NUMBERS before u, observed by the read or not.
 *     uint32 [U][K][2], the shape of the site link table; entries with u - k < 0 are 0.
 *  5. Resolution (c3r_phase_merge): c3r_phase_resolve's rule, unchanged and with the same parameters, on the pseudo-table of the units
 *     (pos = the unit's ps, links = ulinks).  A unit that comes out with ps' >= 0 has joined a super-block: every one of its sites gets
 *     ps = ps' and h1 ^= h1'.  The other units and the sites with ps = -1 stay as they are.  n_joined = the units whose ps changed (the
 *     first unit of a super-block keeps its own).  The statistics are counted from the table that results: n_phased = sites with
 *     ps >= 0, n_blocks = distinct ps >= 0, max_block = the most sites on one ps (a site without a block counts as a block of one, as in c3r_phase_resolve).
 * A caller repeats levels until n_joined == 0 or as often as it likes: a later level links the super-blocks, which a level made
 * neighbours in the numbering.  Sites are never re-oriented inside their block and a site without a block never gets one.
 *
 * c3r_phase_unit_links validates the table like c3r_phase_links and in addition refuses, naming the index, a ps that is neither -1 nor
 * >= 1 and an h1 above 1.  *n_units (may be NULL) receives U.  ulinks = NULL: only that.  Otherwise cap_units >= U (C3R_EOVERFLOW if
 * not); the call uploads the sites and every site's unit, clears a device table, runs k_phase_unit_links (csrc/phase_kernels.hpp) on the
 * context's stream and reads U rows back.  U < 2, n = 0 or no reads loaded: nothing is launched and the U rows are 0.  Like
 * c3r_phase_links it changes neither the reads' haplotags, nor the table of c3r_set_phase_sites, nor anything a scan reads.
 * c3r_phase_merge is host code like c3r_phase_resolve (no context, no device) and calls it for step 5.  C3R_EINVAL for positions that do
 * not increase, such a ps or h1, parameters out of range, or an n_units that is not the table's U.  stats and n_joined may be NULL; out
 * may be `in`. */
int c3r_phase_unit_links(c3r_ctx *ctx, const c3r_phase_site_t *sites, int64_t n, uint32_t *ulinks, int64_t cap_units, int64_t *n_units);
int c3r_phase_merge(const c3r_phase_site_t *in, int64_t n, const uint32_t *ulinks, int64_t n_units, const c3r_phase_params_t *p,
                    c3r_phase_site_t *out, c3r_phase_stats_t *stats, int64_t *n_joined);
/* The phasing above over a table that also holds heterozygous insertions, deletions and two-ALT sites (`0/1` rows with an indel ALT, `1/2`
 * rows).  Opt-in (phase_vcf --indels), like `whatshap phase --indels`.  It is the join of two contracts that are already here, and nothing
 * else:
 *  Table: as c3r_hap_allele_counts — sites sorted by strictly increasing pos; alleles A and B, base_matters, event_matters and the pool
 *   exactly as there.
 *  Voters: c3r_phase_links' — the loaded reads that pass read_kept under the current c3r_params, without the depth cap.
 *  Observation: the column of c3r_hap_allele_counts at the site (normalised CIGAR, the event behind the anchor as defined there): column 0
 *   is allele index 0 (A), column 1 is allele index 1 (B); column 2 (another allele) and no observation are nothing.
 *  Links and resolution: those of c3r_phase_links / c3r_phase_resolve, and of c3r_phase_unit_links / c3r_phase_merge, unchanged.
 *   c3r_phase_resolve and c3r_phase_merge read pos, ps and h1 only: the caller hands them a pseudo-table (pos, ref = 1, alt = 2, ps, h1),
 *   as c3r_phase_merge itself does for the units.  h1 = 0: allele A lies on haplotype 1 (GT 0|1, 1|2); h1 = 1: allele B (GT 1|0, 2|1).
 * On a table whose sites are all REF-and-one-SNV both calls give the words of c3r_phase_links / c3r_phase_unit_links.
 * Limits, as for both parents: the alleles are read off the CIGAR position — no realignment (c3r_set_hap_realign lifts it), no left-alignment of the reads' indels, no
 * base qualities; the chain is greedy, not wMEC; agreement with `whatshap phase --indels` is not measured.
 *
 * c3r_phase_allele_links: links [n][K][2] cis / trans.  ps is IGNORED (a negative one is accepted); every other validation is
 * c3r_hap_allele_counts' (one checker), C3R_EINVAL naming the first bad index.  It needs no phase table.  n = 0: nothing is launched; no
 * reads loaded: every count is 0.  It runs k_phase_allele_links (csrc/phase_kernels.hpp).
 * c3r_phase_allele_unit_links: c3r_phase_unit_links over the allele table.  sites[j].ps is -1 or >= 1 as the chain leaves it, h1[j] is 0
 * or 1 (refused otherwise, naming the index).  Units, the tie rule, ulinks = NULL (only *n_units), C3R_EOVERFLOW for cap_units < U, and
 * U < 2 / n = 0 / no reads loaded (nothing is launched, the U rows are 0) are c3r_phase_unit_links'.  It runs k_phase_allele_unit_links on
 * a copy of the table with h1 folded into the site records.
 * Both keep device buffers of their own for the sites and the pool, allocated at the first call and kept: they change neither a table
 * set by c3r_set_phase_sites / c3r_set_phase_alleles, nor the reads' haplotags and phase sets, nor anything a scan or
 * c3r_hap_allele_counts reads.  The caller's arrays may go once a call returns. */
int c3r_phase_allele_links(c3r_ctx *ctx, const c3r_hap_site_t *sites, int64_t n, const uint8_t *ins_pool, int64_t pool_bases, uint32_t *links);
int c3r_phase_allele_unit_links(c3r_ctx *ctx, const c3r_hap_site_t *sites, const uint8_t *h1, int64_t n, const uint8_t *ins_pool, int64_t pool_bases,
                                uint32_t *ulinks, int64_t cap_units, int64_t *n_units);
/* Left-alignment of indels for the four calls that hold reads against an allele table (c3r_hap_allele_counts, c3r_phase_allele_links,
 * c3r_phase_allele_unit_links and the tagging of c3r_set_phase_alleles / c3r_load_reads).  Opt-in (--left_align_indels); switched off,
 * every path, launch and output byte is what the contracts above say.  It lifts their "no left-alignment of the reads' indels": in a
 * homopolymer or a short tandem repeat the aligner may place a read's indel one or more repeat units away from the VCF's anchor, and such
 * a read then shows (base, NONE) there — a vote for REF.  Switched on, the table's alleles are brought to their left-most form against the
 * reference (host: c3r_hap_left_align_sites), each read's event is brought to its left-most form inside its own M run (device), and the two
 * are compared as above.  This is where the rule is stated; csrc/haplotag_kernels.hpp (hap_observe_la), c3r_hap_left_align_sites and
 * tests/leftalignref.py restate it.
 *
 * left_align(ref, a, kind, n, s) -> (k, s'), for an event behind the 0-based anchor a: shift by one while the reference base on the anchor
 * equals the event's last base and both are one of A, C, G, T.  Step j = 0, 1, ...: for DEL(n) the condition is ref[a - j] == ref[a - j + n];
 * for INS(s) it is ref[a - j] == last(s_j), with s_0 = s and s_{j+1} = ref[a - j] + s_j[:-1].  `ref` is the slice given (c3r_set_reference;
 * the arguments of c3r_hap_left_align_sites), compared in upper case: a position outside it stops the shift — a - j, a - j + n, and the
 * anchor the step would move to, a - j - 1 — and so does any code other than A, C, G, T on one of the three.  k is the number of shifts, s' = s_k the rotated
 * insertion (= (ref[a - k + 1 .. a] + s)[:n]).
 *
 * Table (c3r_hap_left_align_sites, host code: no context, no device).  Input: n sites as c3r_hap_allele_counts takes them (pos need not be
 * sorted; ps is copied), their pool, and a reference slice (ref_start 1-based, any letter case).  Per site, k_A / k_B = left_align's count
 * for each allele that is an insertion or a deletion, with a = pos - 1.  The site moves to pos - k when every such allele of the site
 * shifts by the same k, and k == 0 or base_matters == 0.  A moved site (k > 0) takes the reference base at the new anchor as both alleles'
 * base (an A, C, G or T by the rule; base_matters is 0, so it is never compared) and the rotated bases s' in the pool.  A site that meets neither condition is dropped (`not_left_alignable`).  The table is then sorted by pos again (stable);
 * of two sites on one position the first in input order stays, the other is dropped (`same_pos_after_left_align`).  Output: the m sites
 * that stay in out_sites (cap n), their pool in out_pool (rebuilt: insertion k of the output starts where insertion k - 1 ended;
 * out_pool_cap bases must hold the inserted bases of all input alleles, C3R_EOVERFLOW if not), *out_pool_bases, src_index[j] = the input
 * index of output site j (the caller's map to its VCF rows and its h1), and the statistics.  *n_out = m.  C3R_EINVAL for pos < 1, a flag
 * other than 0 / 1, an unknown kind, an indel of length 0 (or a length on kind NONE) or an insertion that runs past the pool.
 *
 * Read (device), on the read's NORMALISED CIGAR, where adjacent M-like ops are one run (`3M2=` before a D is a run of 5).  Take an event
 * E — the I or D op directly behind an M run that covers the reference positions [x, x + len), as in c3r_hap_allele_counts — and k =
 * min(left_align's count with a = x + len - 1, len - 1): the anchor stays inside the run.  At the site whose anchor is x + len - 1 - k the
 * read shows E, an insertion with s' (the rotation takes reference bases, whatever the read shows there).  At every other site of the run —
 * the run's last base included when k > 0 — the event is NONE.  Not shifted, and seen on the run's last base only, as before: an I with a
 * D at once behind it (OTHER), and an insertion that l_seq cuts off (no observation).  A run whose last base lies at or past l_seq carries
 * no event.  The read's base on a site is the one the CIGAR puts there, and everything else of the observation is unchanged.  The result
 * does not depend on the walk a read takes: a read whose CIGAR holds two M-like ops in a row takes the serial walk while the switch is on
 * (the plain walk hands them out one by one; aligners that write = / X pay one lane per read there).
 * What remains: a shift stops at the M run's start, at an N or another indel, and at the slice's edge; there is no realignment (c3r_set_hap_realign lifts it) and there
 * are no base qualities (c3r_set_hap_min_bq lifts it as a threshold, c3r_set_hap_bq_weights as weights of the tagging's votes); agreement with whatshap is not measured.
 *
 * c3r_set_hap_left_align(ctx, on): default 0.  While on, the four calls above run k_*_la (the same launches, one kernel each, with
 * hap_observe_la in hap_observe's place) against the slice of c3r_set_reference that is current when they run, and return C3R_EINVAL with a
 * message when no reference is set (c3r_set_phase_alleles with n = 0 still clears).  The caller hands them a table that
 * c3r_hap_left_align_sites has normalised against the same reference; the slice must cover every loaded read's [pos, end) for the
 * results to be those of the rule on the whole reference.  Toggling the switch with an allele table set and reads loaded tags the reads
 * again, as setting a table does (C3R_EINVAL, and the switch stays, when that needs a reference and none is set).  A later
 * c3r_set_reference does NOT tag again: the tags are those of the slice that was set when they were made.  The table of
 * c3r_set_phase_sites and the four SNV kernels never look at the switch. */
typedef struct { int64_t n_in, n_out, n_moved, n_not_left_alignable, n_same_pos_after_left_align; } c3r_left_align_stats_t;
int c3r_set_hap_left_align(c3r_ctx *ctx, int on);
int c3r_hap_left_align_sites(const c3r_hap_site_t *sites, int64_t n, const uint8_t *ins_pool, int64_t pool_bases, int64_t ref_start, const char *ref,
                             int64_t ref_len, c3r_hap_site_t *out_sites, uint8_t *out_pool, int64_t out_pool_cap, int64_t *out_pool_bases,
                             int64_t *src_index, int64_t *n_out, c3r_left_align_stats_t *stats);
/* Allele realignment for the same four calls (c3r_hap_allele_counts, c3r_phase_allele_links, c3r_phase_allele_unit_links and the tagging of
 * c3r_set_phase_alleles / c3r_load_reads).  Opt-in (--hap_realign [W]); switched off, every path, launch and output byte is what the
 * contracts above say.  It lifts their "no realignment": where the aligner wrote a substitution as `1D1I` beside the site, or put an indel a
 * few bases from an SNV, the CIGAR-position allele is wrong although the read's bases are right.  Switched on, the read's local window is
 * compared with the two haplotypes of the site — the step that stands behind `whatshap phase` and `whatshap haplotag` in the reference flow
 * (run_clair3_rna:749-794) — with unit costs.  This is where the rule is stated; csrc/realign.hpp with csrc/haplotag_kernels.hpp
 * (hap_observe_ra), c3r_hap_realign_column and tests/realignref.py restate it.
 *
 * realign, with overhang W: W = 0 is off, the legal range is 1 .. 16.  The drivers' default for the flag without a value is 10, which we
 * recall as whatshap's default and have not checked.
 * Site and window.  Site e (c3r_hap_site_t) has the 0-based anchor p0 = pos - 1.  D = the larger DEL length of its two alleles (0 if
 *  neither is a deletion), I = the larger INS length.  Reference interval [s, t): s = p0 - W, t = p0 + 1 + D + W.  Haplotype string of
 *  allele X = ref[s, p0) + X.base + X.ins + ref[p0 + 1 + X.del, t): both strings cover the same reference interval.
 * A site is realignable when [s, t) lies inside the slice of c3r_set_reference and every reference base in it is A, C, G or T, and
 *  2W + 1 + D + I <= 64.
 * Query offset q(p) of a reference position p in a read: p is covered by the CIGAR op with first reference base x and first query base y
 *  (soft clips count in y, as everywhere else); q(p) = y + (p - x) under an M-like op, q(p) = y under a D; under an N the window is not
 *  usable.  H, P and empty ops consume nothing, = and X are M: the raw CIGAR and the normalised one give the same answer.  Hence an
 *  insertion directly before s is outside the window and one directly before t is inside.
 * A read is realigned at the site when the site is realignable, read.pos <= s and t < read.end, no N op holds a position of [s, t],
 *  q(t) <= l_seq and m = q(t) - q(s) <= 64.
 * Observation of a realigned read: the window is the m codes at q(s) .. q(t) - 1 of the sequence the kernels read (the masked copy under
 *  c3r_set_hap_min_bq); dA, dB = the global unit-cost edit distances (Levenshtein) of the window to the two haplotype strings, where a read
 *  code other than 1, 2, 4, 8 (N, a masked base) equals no base.  Column 0 when dA < dB, column 1 when dB < dA, NO OBSERVATION when
 *  dA == dB: the realigned observation never yields column 2.  base_matters and event_matters are not looked at.
 * Unchanged: the anchor must lie under an M op of the normalised CIGAR at a query offset below l_seq (an anchor under D or N: nothing), as
 *  c3r_hap_allele_counts says.  Where the read is NOT realigned at the site the observation is c3r_hap_allele_counts', unchanged (a read's
 *  ends, a splice junction within W, a long allele, a site near the slice's edge): the set of observed (read, site) pairs never shrinks
 *  by anything but ties.
 * The result depends neither on the walk a read takes nor on where inside (s, t) the CIGAR places its indels.
 * What remains: the window stops at an N (c3r_set_hap_realign_spliced, below, lifts it); there are no quality weights (c3r_set_hap_min_bq composes by construction: a masked base matches
 *  nothing) and no affine gaps; agreement with whatshap is not measured.  A table row at a different but equivalent placement has another
 *  window: c3r_hap_left_align_sites stays useful for rows (it does not look at reads or at this switch).
 *
 * c3r_set_hap_realign(ctx, overhang): default 0; C3R_EINVAL outside 0 .. 16.  While above 0 the four calls run k_*_ra — k_*_rs under c3r_set_hap_realign_spliced, below — (the same launches,
 * one kernel each, hap_observe_ra in hap_observe's place, no atomics of their own) against the slice of c3r_set_reference that is current
 * when they run, and return C3R_EINVAL with a message when no reference is set (c3r_set_phase_alleles with n = 0 still clears).  Changing
 * the value with an allele table set and reads loaded tags the reads again (C3R_EINVAL, and the value stays, when that needs a reference
 * and none is set); a later c3r_set_reference does NOT tag again.  Realign and left-align exclude each other: turning one on while the
 * other is on is C3R_EINVAL and changes nothing.  The table of c3r_set_phase_sites and the four SNV kernels never look at the switch.
 * c3r_get_hap_realign: the value.
 * c3r_hap_realign_column is host code (no context, no device), compiled from the header the kernels use: the column (0, 1, 2, or 3 = no
 * observation) of ONE read at ONE site and whether the read was realigned there (0: the column is c3r_hap_allele_counts').  site and
 * ins_pool as in c3r_hap_allele_counts; the slice as in c3r_hap_left_align_sites (any letter case); read, cigars and seq4 as c3r_load_reads
 * takes them (cigars and seq4 are the arrays that read->cigar_off and read->seq_off index).  The call carries no pool length: the CALLER
 * guarantees that an insertion allele's ins_off + len lies inside ins_pool, as c3r_hap_allele_counts checks it (capi.hap_realign_column does).  overhang 0: the observation with the switch
 * off.  C3R_EINVAL for a NULL it needs, an overhang outside 0 .. 16, pos < 1, a malformed allele or a CIGAR the load would refuse. */
int c3r_set_hap_realign(c3r_ctx *ctx, int overhang);
int c3r_get_hap_realign(c3r_ctx *ctx, int *overhang);
int c3r_hap_realign_column(const c3r_hap_site_t *site, const uint8_t *ins_pool, int64_t ref_start, const char *ref, int64_t ref_len, const c3r_read_t *read,
                           const uint32_t *cigars, const uint8_t *seq4, int overhang, int *column, int *realigned);
/* Allele realignment across splice junctions, for the same four calls.  Opt-in (--hap_realign_spliced beside --hap_realign [W]); switched
 * off, every path, launch and output byte is what the contracts above say.  It lifts `realign`'s "the window stops at an N": exons are
 * short, so a site within W bases of an exon's edge is seen by every spliced read through the CIGAR-position rule — just where aligners
 * misplace bases most often.  An N op consumes no query base, so the read's window stays one stretch of SEQ across a junction; only the
 * reference side has to follow the read's own splicing.  Both haplotype strings follow the same splicing, so a junction the aligner put a
 * base or two off costs both strings the same and cancels in dA against dB.  This is where the rule is stated; csrc/realign.hpp
 * (ra_column_spliced) with csrc/haplotag_kernels.hpp (hap_observe_rs), c3r_hap_realign_column_spliced and tests/realignspliceref.py
 * restate it.
 *
 * realign_spliced, in force only while this switch is on AND c3r_set_hap_realign is above 0.  W, D, I, p0 and q(p) are `realign`'s.
 * Spliced positions of a read: the reference positions under an M-like or a D op of its raw CIGAR, in increasing order x_0 < x_1 < ...
 *  Positions under an N are not among them.  H, P and empty ops consume nothing, = and X are M.
 * Window.  k0 is the index with x_k0 = p0 (the anchor must lie under an M op at a query offset below l_seq, as ever: otherwise there is
 *  nothing to observe).  The read is realigned at the site when all of these hold:
 *   x_(k0+j) = p0 + j for j = 0 .. D: no N holds a position of the site's core [p0, p0 + D];
 *   ks = k0 - W >= 0;
 *   kt = k0 + 1 + D + W is an index of the read (`realign`'s t < read.end);
 *   2W + 1 + D + I <= 64;
 *   every reference base that the strings use — the positions x_ks .. x_(kt-1), core included as in `realign` — lies inside the slice of
 *    c3r_set_reference and is A, C, G or T.  Introns are never read, so only those positions need the slice;
 *   q(x_kt) <= l_seq and m = q(x_kt) - q(x_ks) <= 64.
 *  Haplotype string of allele X = ref[x_ks .. x_(k0-1)] + X.base + X.ins + ref[x_(k0+1+X.del) .. x_(kt-1)].
 *  The read's window is the m codes at q(x_ks) .. q(x_kt) - 1.  The distances, the tie (no observation, never column 2) and the masked
 *  base that equals nothing are `realign`'s.  An insertion directly before x_ks is outside the window; one directly before x_kt is inside,
 *  on whichever side of an N the CIGAR lists it.
 * Otherwise: where the read is not realigned at the site the observation is c3r_hap_allele_counts', unchanged.
 * Consequences.  A read with no N in [s, t] gets exactly `realign`'s result (x_ks = s and x_kt = t).  The set of realigned (read, site)
 *  pairs never shrinks against `realign`.  The result depends neither on the walk a read takes nor on where inside the window the CIGAR
 *  places its indels, nor on the introns' lengths or letters: cut the introns out of reference, sites and reads and `realign` gives the
 *  same columns.
 * What remains: an N inside the core falls back; left-align does not cross an N; the rest of `realign`'s list.
 *
 * c3r_set_hap_realign_spliced(ctx, on): default 0; anything but 0 or 1 is C3R_EINVAL.  It may be set at any time and has effect only
 * while the overhang is above 0: then the four calls run k_*_rs (the same launches and arguments as k_*_ra, hap_observe_rs in
 * hap_observe_ra's place, no atomics of their own).  Flipping it with the overhang above 0, an allele table set and reads loaded tags the
 * reads again, as a new overhang does.  A refusal leaves the context as it was.  Left-align keeps excluding realign.
 * c3r_get_hap_realign_spliced: the value.
 * c3r_hap_realign_column_spliced: c3r_hap_realign_column with `spliced` (0 or 1, else C3R_EINVAL) choosing the rule; host code, no
 * context and no device.  c3r_hap_realign_column is this call with spliced = 0 and returns what it returned. */
int c3r_set_hap_realign_spliced(c3r_ctx *ctx, int on);
int c3r_get_hap_realign_spliced(c3r_ctx *ctx, int *on);
int c3r_hap_realign_column_spliced(const c3r_hap_site_t *site, const uint8_t *ins_pool, int64_t ref_start, const char *ref, int64_t ref_len, const c3r_read_t *read,
                                   const uint32_t *cigars, const uint8_t *seq4, int overhang, int spliced, int *column, int *realigned);
/* A base-quality threshold for the twelve kernels that hold the loaded reads against a site table: k_haplotag, k_hap_counts, k_phase_links,
 * k_phase_unit_links, k_haplotag_alleles, k_hap_allele_counts, k_phase_allele_links, k_phase_allele_unit_links and the four _la
 * instantiations — the tagging of c3r_set_phase_sites / c3r_set_phase_alleles / c3r_load_reads, c3r_hap_counts, c3r_hap_allele_counts,
 * c3r_phase_links, c3r_phase_unit_links, c3r_phase_allele_links and c3r_phase_allele_unit_links.  Opt-in (--hap_min_bq); switched off,
 * every launch, upload and output byte is what the contracts above say.  It lifts their "no base qualities" as far as a threshold does: on
 * ONT direct-RNA reads a wrong base on a phased site is a unit-weight vote for the wrong haplotype, and its quality is the only evidence
 * the read carries against it.  This is where the rule is stated; csrc/qual_kernels.hpp and tests/qualref.py restate it.
 *
 * Qualities (c3r_load_reads_q): qual[2 * n_seq_bytes]; the quality of base j of read i is byte 2 * reads[i].seq_off + j — one byte where
 * the sequence has a nibble, so c3r_read_t has no field for it.  Values are phred as BAM stores them; a record without qualities holds
 * 0xff throughout; the padding byte behind a read of odd length is 0xff (c3r_bam_copy_quals, include/c3r_io.h, delivers this layout).
 *
 * Rule: Q = hap_min_bq, 0 <= Q <= 93, Q = 0 is off.  With Q > 0, base j of a read is MASKED iff its quality byte q satisfies
 * q < Q && q != 0xff: a base without a quality is never masked.  The twelve kernels read the reads' bases from a masked copy of the packed
 * sequence in which a masked base is code 15 (N), and nothing else changes for them.  The contracts above say what an N means: no
 * observation at an SNV site and at an allele site with base_matters; a pure indel site is still observed by its event; an insertion that
 * holds an N equals no allele (column 2 of the counts, no vote in tags and links); under c3r_set_hap_left_align a shift stops at an N
 * (an N never equals a reference code).  Hence the results with (qualities, Q) equal, element for element,
 * the results with Q = 0 on reads whose masked bases the caller replaced by N.  Everything else reads the sequence as it was loaded: the
 * tensor build and its tokens, the ordered recompute, the decoder's copy of the bases, c3r_rows_begin_ex.
 * What remains: it is a threshold, not whatshap's quality-weighted votes (c3r_set_hap_bq_weights, below, are those); an indel's own quality is not modelled (an indel carries none in
 * BAM); agreement with whatshap is not measured; the default is 0.
 *
 * c3r_load_reads_q is c3r_load_reads plus the qualities (c3r_load_reads is this call with qual = NULL, n_qual_bytes = 0).
 * n_qual_bytes != 2 * n_seq_bytes: C3R_EINVAL.  The qualities go up like the three other arrays and stay on the device (2 bytes per
 * sequence byte) until the next load; their buffer exists only once qualities were handed over.  With Q > 0 the masked copy is made
 * (k_mask_low_bq, on the context's stream, before the tags) inside the load.  A load of n_reads > 0 WITHOUT qualities while Q > 0 is
 * C3R_EINVAL, before anything of the previous load is given up: a threshold that silently does not apply is refused.  n_reads = 0 is allowed.
 * c3r_set_hap_min_bq: C3R_EINVAL for a value outside 0 .. 93 (a threshold above every legal quality would mask everything) and for Q > 0
 * while reads are loaded that came without qualities; the context stays as it was, and so it does when the masked copy cannot be made
 * (C3R_ENOMEM, C3R_EHIP: the old threshold stays in force; a failure of the tagging that follows loses the loaded reads' tables, as a
 * failed c3r_set_params does).  Valid before or after the load with the same result:
 * with reads loaded the copy is made again, and with a phase table set the reads are tagged again, as c3r_set_hap_left_align does.  The copy
 * depends on neither min_mq nor excl_flags: c3r_set_params does not make it again.
 * c3r_get_hap_min_bq: Q and the number of masked bases of the loaded reads (0 with Q = 0 or without qualities); either pointer may be NULL.
 * c3r_get_hap_seq: the n_seq_bytes bytes that the twelve kernels read — the masked copy, or with Q = 0 the sequence itself — into
 * seq4[cap]; C3R_EOVERFLOW when cap is smaller. */
int c3r_load_reads_q(c3r_ctx *ctx, const c3r_read_t *reads, int64_t n_reads, const uint32_t *cigars, int64_t n_cigar_ops, const uint8_t *seq4,
                     int64_t n_seq_bytes, const uint8_t *qual, int64_t n_qual_bytes);
int c3r_set_hap_min_bq(c3r_ctx *ctx, int min_bq);
int c3r_get_hap_min_bq(c3r_ctx *ctx, int *min_bq, int64_t *n_masked);
int c3r_get_hap_seq(c3r_ctx *ctx, uint8_t *seq4, int64_t cap);
/* Quality-weighted votes for the tagging — the decision of c3r_set_phase_sites / c3r_set_phase_alleles inside c3r_load_reads* — and for
 * nothing else.  Opt-in (--hap_bq_weights); switched off, every launch, upload and output byte is what the contracts above say.  Whatshap
 * sums the phred quality of the read's base on each phased site where the rule above counts 1; this switch is that weighting.  This is
 * where the rule `bq_weights` is stated; csrc/haplotag_kernels.hpp (HapTallyW, the four _w kernels) and tests/hapweightref.py restate it.
 *
 * Rule: hap_bq_weights is 0 or 1.  Voters, the observation (also under c3r_set_hap_left_align / c3r_set_hap_realign, where only the
 * observation differs) and the membership of a site in a phase set are the contracts above.  The WEIGHT of a vote is the quality byte of
 * the read's base on the site's position, qual[2 * seq_off + q], q being the query offset of that base: the anchor base of an indel or
 * two-ALT site.  A byte 0xff (no quality; such a record is 0xff throughout) weighs 1, so a read without qualities gets its unit-weight
 * result.  Weight 0 is legal: the observation counts as one and adds nothing.  No cap, no rescaling: a read's sum is at most l_seq x 254.
 * Per phase set the read has (w1, w2), the weight sums for haplotype 1 and 2, n, the number of observations, and the first voting site.
 * The read's phase set is the one with the largest w1 + w2 (equal: the one whose first voting site on the read comes first);
 * hp = 1 if w1 > w2, 2 if w2 > w1, else 0.  The tag word and c3r_haplotag_stats_t keep their meaning: n_votes sums the observations of
 * all sets, n_no_vote counts reads with no observation, n_tie reads with w1 == w2 in the chosen set.  With c3r_set_hap_min_bq a masked
 * base is an N and no observation, as there; the weight of an unmasked base is its own quality.
 * The count tables (c3r_hap_counts, c3r_hap_allele_counts) and the four link calls do not look at the switch: they count reads, by the
 * tags and sets this rule decided.
 * What remains: an indel's own quality and the inserted bases' qualities are not modelled; under c3r_set_hap_realign the weight is still
 * the anchor's quality, not a difference of alignment costs; the links of the built-in phasing stay unweighted; that whatshap weights by
 * phred and writes PC is recalled, not checked; agreement with whatshap is not measured; the default is off.
 *
 * c3r_set_hap_bq_weights: C3R_EINVAL for a value other than 0 or 1, and for 1 while reads are loaded that came without a quality array
 * (c3r_load_reads); the context stays as it was.  While the switch is on, a c3r_load_reads of n_reads > 0 without qualities is C3R_EINVAL
 * before anything of the previous load is given up: a weight that silently does not apply is refused.  Valid before or after the load with
 * the same result: with reads loaded and a table set the reads are tagged again, as c3r_set_hap_min_bq does.
 * c3r_get_hap_bq_weights: the switch.
 * c3r_get_haplotag_weights: (w1, w2) of the set every loaded read's tag was decided in, in load order (w12: [cap][2], cap >= the number
 * of loaded reads): a tie's pair for a read tagged 0 with observations, (0, 0) without one.  Their difference is what
 * the BAM writer of include/c3r_io.h writes as PC.  C3R_EINVAL when no phase sites are set or the switch is off;
 * C3R_EOVERFLOW when cap is smaller.  The pairs' buffer on the device exists only once the switch was on.
 * c3r_get_haplotag_words: the tag word of every loaded read, in load order (words: [cap], cap >= the number of loaded reads): tag | n << 2
 * with n the read's observations on all phase sets — what c3r_get_haplotags sums into n_votes —, with the switch on or off.  C3R_EINVAL
 * when no phase sites are set; C3R_EOVERFLOW when cap is smaller.
 * A re-tag that fails inside c3r_set_hap_bq_weights leaves the switch as it was before the call. */
int c3r_set_hap_bq_weights(c3r_ctx *ctx, int on);
int c3r_get_hap_bq_weights(c3r_ctx *ctx, int *on);
int c3r_get_haplotag_weights(c3r_ctx *ctx, uint32_t *w12, int64_t cap);
int c3r_get_haplotag_words(c3r_ctx *ctx, uint32_t *words, int64_t cap);

/* Haplotype-resolved read counts per interval (the rule `hap_regions`): how many loaded reads of each haplotype, per phase set, overlap each
 * interval of a table — the exons or genes of a BED file.  Allele-specific expression from the tags the device already holds, without the
 * haplotagged BAM.  Opt-in: nothing calls it unless asked (hap_expr, call_sample --hap_expression_bed).
 *
 * Inputs.  regions[n]: start, end 0-based half-open with start < end; sorted by (start, end), equal and nested regions allowed; strand 0 none,
 * 1 `+`, 2 `-`; reserved = 0.  The rows of region j are [row_off[j], row_off[j + 1]), the last region's end at n_rows; row_off is
 * non-decreasing, row_off[0] = 0 and no row_off exceeds n_rows.  row_ps[n_rows]: phase-set numbers >= 0, strictly increasing inside one
 * region.  stranded: 0 off, 1 same, 2 reverse.
 * Voters: the loaded reads that the tensor build keeps under the current parameters (read_kept with min_mq / excl_flags: the voters of
 * c3r_hap_counts) and that have end > pos.  No depth cap.
 * Overlap: a read overlaps a region iff at least one reference position under one of its M-like (M, =, X) or D ops of the normalised CIGAR
 * lies in [start, end).  Introns (N) do not count; I, S, H and P consume no reference.  A read counts once per region, however many of its
 * ops overlap it, and in every region it overlaps.
 * Strand: with stranded != 0 and region.strand != 0 the read counts only if its strand (flag & 16: `-`) equals the region's (stranded = 1)
 * or is the opposite (stranded = 2).  A region with strand = 0 always counts.
 * Where the one count goes: (tag, set) are those of c3r_get_haplotags / c3r_get_read_phase_sets.  Tag 0: region_counts[j][0] (untagged).
 * Tag 1 or 2 and the set is row r of region j: row_counts[r][tag - 1].  Tag 1 or 2 and the set is none of the region's rows:
 * region_counts[j][1] (tagged in another set).
 * Output: region_counts uint32 [n][2], row_counts uint32 [n_rows][2].  All sums are integers: neither read order nor arrival order shows.
 *
 * The bound.  first_open[j] is the smallest i <= j with end_i > start_j (the library computes it): the regions an op [x, x + len) can
 * overlap lie from first_open[k], k the last region with start <= x, up to the first region with start >= x + len.  A table with
 * max_j (j - first_open[j]) > C3R_HAP_REGION_MAX_BACK is refused (C3R_EINVAL naming the region): one long region lying over thousands of
 * short ones makes every op scan them all.  It is a safety condition that bounds one op's scan to 4096 loads, not a tuned number; count long
 * and short regions (genes and exons) in separate calls then.  That gene annotations stay far below it — a few thousand genes per
 * chromosome, the longest spanning well under a hundred others — is recalled, not checked.
 *
 * c3r_hap_region_counts needs a phase table (C3R_EINVAL without one, whatever n is); n = 0 succeeds and launches nothing; no reads loaded:
 * every count is 0 and nothing is launched.  C3R_EINVAL, naming the first bad region or row, for start >= end, start < 0, an unsorted table,
 * a strand above 2, a non-zero reserved byte, a row_off that is not 0 at region 0, decreases or exceeds n_rows, a region of 2^24 rows or
 * more, a negative ps, ps not strictly increasing inside a region, stranded outside 0 .. 2 and a table over the bound.  It uploads regions,
 * first_open and row_ps into buffers that it shares with c3r_hap_group_counts (each call waits for the device before it returns, so
 * neither call finds the other's table), clears one device table of 2 n + 2 n_rows words, runs k_hap_region_counts
 * (csrc/hapregion_kernels.hpp) on the context's stream and reads the table back.  It changes neither the reads' haplotags and phase sets,
 * nor the phase table, nor anything a scan or another count table reads.  The device buffers are allocated at the first call and kept.
 * Not done: no union of a gene's exon rows here (a read over two exons of one gene counts in both: the gene-level count is the rule
 * `hap_groups` below, c3r_hap_group_counts), no fractional assignment of a read that overlaps several regions, no statistics (no test of
 * allelic imbalance); agreement with featureCounts / htseq-count is not measured. */
#define C3R_HAP_REGION_MAX_BACK 4096
typedef struct { int32_t start, end, row_off; uint8_t strand, reserved[3]; } c3r_hap_region_t;
int c3r_hap_region_counts(c3r_ctx *ctx, const c3r_hap_region_t *regions, int64_t n, const int32_t *row_ps, int64_t n_rows, int32_t stranded,
                          uint32_t *region_counts, uint32_t *row_counts);

/* Haplotype-resolved read counts per GROUP of intervals (the rule `hap_groups`): the gene-level count — a gene is the group of its exons,
 * and a read counts once per gene it overlaps, however many of the gene's exons it lies over.  Voters, overlap, strand and (tag, set) are
 * those of `hap_regions` above.  Opt-in: nothing calls it unless asked (hap_expr --group_by_name, call_sample
 * --hap_expression_group_by_name).
 *
 * Inputs.  intervals[n]: start, end 0-based half-open with start < end, sorted by (start, end); group in [0, n_groups); strand 0 none,
 * 1 `+`, 2 `-`; reserved = 0.  The intervals of one group are pairwise disjoint (abutting is allowed) and carry one strand; intervals of
 * different groups may overlap, nest or be equal; every group has at least one interval.  The rows of group g are
 * row_ps[group_row_off[g] .. group_row_off[g + 1]), the last group's end at n_rows (group_row_off: [n_groups], 0 at group 0, never
 * decreasing, never above n_rows); phase-set numbers >= 0, strictly increasing inside one group.  stranded: 0 off, 1 same, 2 reverse.
 * Counting.  A voter counts in group g exactly once iff at least one reference position under one of its M-like or D ops lies in at least
 * one interval of g that the strand test of `hap_regions` admits (one strand per group: it admits all of g's intervals or none).  How many
 * ops and how many of the group's intervals are involved does not matter; a read that lies only in the group's introns is not in it.
 * Where the one count goes.  Tag 0: group_counts[g][0] (untagged).  Tag 1 or 2 and the set is row r of g: row_counts[r][tag - 1].  Tag 1
 * or 2 and the set is none of g's rows: group_counts[g][1] (tagged in another set).
 * Output: group_counts uint32 [n_groups][2], row_counts uint32 [n_rows][2]; integer sums, neither read order nor arrival order shows.
 * With every interval a group of its own the two tables are c3r_hap_region_counts' tables element for element.
 *
 * c3r_hap_group_counts needs a phase table (C3R_EINVAL without one, whatever n is); n = 0 (then n_groups = 0 and n_rows = 0) succeeds and
 * launches nothing; no reads loaded: every count is 0 and nothing is launched.  C3R_EINVAL, naming the first bad interval, group or row,
 * for start >= end, start < 0, an unsorted table, a strand above 2, a non-zero reserved byte, a group id outside [0, n_groups), two
 * intervals of one group that overlap, two strands in one group, a group without an interval, a group_row_off that is not 0 at group 0,
 * decreases or exceeds n_rows, a group of 2^24 rows or more, a negative ps, ps not strictly increasing inside a group, stranded outside
 * 0 .. 2 and an interval table over C3R_HAP_REGION_MAX_BACK (the bound of `hap_regions`, on the interval table).  The library computes
 * first_open and, per interval, the previous interval of its group in table order; it uploads them with the rows into the buffers of
 * c3r_hap_region_counts, clears one device table of 2 n_groups + 2 n_rows words, runs k_hap_group_counts (csrc/hapgroup_kernels.hpp) on the context's stream and
 * reads the table back.  It changes neither the reads' haplotags and phase sets, nor the phase table, nor anything a scan or another count
 * table reads.  Its device buffers are allocated at the first call and kept.
 * c3r_set_hap_group_direct(ctx, on): default 0; anything but 0 or 1 is C3R_EINVAL.  0: the counts of a workgroup's reads are summed in LDS
 * first and every touched word gets one global add per workgroup.  1: the same kernel body without the LDS stage, one global add per
 * (read, group).  The results are identical.  c3r_get_hap_group_direct reads the switch.
 * Not done: no GTF reader (the groups come from the caller), no fractional assignment of a read that lies in several genes (it counts once
 * in each), no statistics (no test of allelic imbalance); agreement with featureCounts / htseq-count is not measured. */
typedef struct { int32_t start, end, group; uint8_t strand, reserved[3]; } c3r_hap_interval_t;
int c3r_hap_group_counts(c3r_ctx *ctx, const c3r_hap_interval_t *intervals, int64_t n, int64_t n_groups, const int32_t *group_row_off,
                         const int32_t *row_ps, int64_t n_rows, int32_t stranded, uint32_t *group_counts, uint32_t *row_counts);
int c3r_set_hap_group_direct(c3r_ctx *ctx, int on);
int c3r_get_hap_group_direct(c3r_ctx *ctx, int *on);

/* Haplotype-resolved splice-junction counts (the rule `hap_junctions`): which haplotype uses which intron — per junction that the loaded
 * reads hold, how many reads hold it, and per phase set how many of them carry each haplotype.  Allele-specific splicing from the tags the
 * device already holds, without the haplotagged BAM.  Opt-in: nothing calls it unless asked (hap_junctions, call_sample --hap_junctions).
 *
 * Counted reads: the loaded reads that the tensor build keeps under the current parameters (read_kept with min_mq / excl_flags: the
 * voters of `hap_regions`) and that have end > pos.  No depth cap.
 * A junction of a read: every N op of length >= 1 of its NORMALISED CIGAR (zero-length ops, H and P dropped, = and X folded into M, equal
 * neighbours merged — the form both walks of the device deliver, so adjacent N ops are one junction and `0N` is none).  An op at reference
 * position x (0-based) of length len is the junction [x, x + len), 0-based half-open.  What lies on either side does not matter:
 * `5M3I10N5M` and `10M2D100N10M` count as written.  Reference positions increase along a read, so a read holds a junction at most once.
 * Per junction: reads — the counted reads that hold it; reverse — those with flag bit 16; untagged — those whose tag is 0; and one row
 * per phase set in which at least one of them was tagged, with hp1 / hp2, the reads tagged 1 / 2 in that set ((tag, set) are those of
 * c3r_get_haplotags / c3r_get_read_phase_sets).  reads == untagged + the sum of hp1 + hp2 over the junction's rows.
 * No phase table is needed: without one, or with a table under which no read was tagged, every counted read is untagged and there are no
 * rows — a plain junction counter.
 * Output order: junctions by (start, end), a junction's rows by ps; rows of junction j are [row_off_j, row_off_(j + 1)), the last
 * junction's end at the number of rows.  All sums are integers: neither read order, arrival order nor the hash shows.
 *
 * c3r_hap_junction_counts runs k_hap_junction_counts (csrc/hapjunction_kernels.hpp) on the context's stream: two insert-only hash tables
 * on the device (junctions; rows), counted into per-workgroup tables in LDS first.  slots_hint: the initial number of junction slots (the
 * row table starts with as many); 0: the library's default, C3R_HAP_JUNCTION_SLOTS; rounded up to a power of two and clamped to
 * 16 .. 2^28; negative: C3R_EINVAL.  A table without a place for a key within 256 probes (or its size, if smaller: linear probing, so a
 * table grows at a load factor near 0.9, before probing degenerates) is doubled, both are cleared and the launch is repeated — exact,
 * the counts being sums —, at most C3R_HAP_JUNCTION_MAX_ROUNDS times, then C3R_EOVERFLOW with a message.  The host reads both whole
 * tables back (20 and 16 bytes per slot; C3R_ENOMEM when its copies do not fit).  Measured at load factors of 0.16 and 0.04 only: a
 * contig whose distinct junctions come near the table's size costs more probes per claim and one or more repeated launches, neither measured.  The host compacts and sorts, and
 * the context keeps the result until the next call or the next c3r_load_reads.  *n_junctions / *n_rows (both required) receive the sizes.
 * No reads loaded: both are 0 and nothing is launched.  It changes neither the reads' haplotags and phase sets, nor the phase table, nor
 * anything a scan or another count table reads.  Its device buffers are allocated at the first call and kept.
 * c3r_get_hap_junctions copies the kept result (either array may be NULL when its count is 0); C3R_EINVAL when a capacity is smaller than
 * the count or nothing has been counted since the last c3r_load_reads.
 * c3r_set_hap_junction_direct(ctx, on): default 0; anything but 0 or 1 is C3R_EINVAL.  1: the same kernel body without its LDS stage —
 * every count goes to the global tables directly.  The results are identical; the switch exists to measure what the aggregation buys.
 * Not done: no minimum intron length or anchor length; no annotation; no statistics (no test of imbalance); a read tagged in a set counts
 * in that set's row even where the set has no site near the junction; agreement with any external junction counter is not measured. */
#define C3R_HAP_JUNCTION_SLOTS 65536
#define C3R_HAP_JUNCTION_MAX_ROUNDS 48
typedef struct { int32_t start, end; uint32_t reads, reverse, untagged; int32_t row_off; } c3r_hap_junction_t;   /* 24 bytes */
typedef struct { int32_t ps; uint32_t hp1, hp2; } c3r_hap_junction_row_t;                                        /* 12 bytes */
int c3r_hap_junction_counts(c3r_ctx *ctx, int64_t slots_hint, int64_t *n_junctions, int64_t *n_rows);
int c3r_get_hap_junctions(c3r_ctx *ctx, c3r_hap_junction_t *junctions, int64_t cap_j, c3r_hap_junction_row_t *rows, int64_t cap_r);
int c3r_set_hap_junction_direct(c3r_ctx *ctx, int on);

/* ---- tensor build (A1-A5) ------------------------------------------------------------------ */
/* Phase 1+2: CIGAR walk over the reads overlapping [ctg_start-33, ctg_end+33] (1-based, clamped
 * at 1; src/create_tensor_pileup.py:411-415), per-position channel counts, candidate gates, window
 * selection, window gather with the depth>216 rescale (clair3_rna/utils.py:88-92).  Tensors and
 * site records stay resident on the device.  Returns the number of emitted candidates.
 * max_depth (samtools mpileup -d, default 8000): htslib's rule — a read that is not the first one pushed for its start
 * position is discarded while more than max_depth reads are live — is applied per region before the walk.
 * A scan that meets a position covered by more than 32,767 kept reads (only with the cap off or raised) is repeated with 32-bit resident windows,
 * which the context keeps from then on; C3R_EOVERFLOW only when the batch already holds 16-bit windows. */
int c3r_pileup_scan(c3r_ctx *ctx, int64_t ctg_start, int64_t ctg_end, int64_t *n_candidates);
/* The same for several regions (the chunks of one contig) in ONE set of kernel launches: results are exactly those of
 * n_regions successive c3r_pileup_scan calls in batch mode — candidates of region 0 first, each region with its own
 * +-33 bp halo, head/tail flush and window rule — but the chip sees ~20 k tiles at once instead of 13 latency-bound
 * launches of ~1.5 k.  *n_candidates receives the total. */
int c3r_pileup_scan_regions(c3r_ctx *ctx, int32_t n_regions, const int64_t *ctg_starts, const int64_t *ctg_ends, int64_t *n_candidates);
/* Batch mode: between c3r_batch_begin and c3r_batch_end every scan APPENDS its candidates (tensors, sites,
 * tokens) to the device-resident batch instead of replacing it, so that the chunks of a whole contig go through
 * the network in one launch per layer (the reference batches 200 sites, shared/param_p.py:51; 288 GB of HBM let
 * us batch a whole contig).  c3r_batch_count returns the totals; c3r_infer(NULL, n_total) and the c3r_get_*
 * calls then cover all accumulated candidates in scan order. */
int c3r_batch_begin(c3r_ctx *ctx);
int c3r_batch_end(c3r_ctx *ctx);
int c3r_batch_count(c3r_ctx *ctx, int64_t *n_sites, int64_t *n_tokens);
/* Copy out what the last scan (or the current batch) produced.  Any pointer may be NULL.  tensors: int32 [n][33][C]
 * row-major (the 594/990 integers of a create_tensor line, after the A5 rescale when
 * `rescaled` != 0, raw otherwise); sites: [n]; tokens: [n_tokens] (see c3r_token_count), site after site (tok_off / n_tok of
 * c3r_get_sites), each site's in BAM order. */
int c3r_get_tensors(c3r_ctx *ctx, int rescaled, int32_t *tensors, int64_t cap_sites);
int c3r_get_sites(c3r_ctx *ctx, c3r_site_t *sites, int64_t cap_sites);
int c3r_token_count(c3r_ctx *ctx, int64_t *n_tokens);
int c3r_get_tokens(c3r_ctx *ctx, c3r_token_t *tokens, int64_t cap_tokens);
/* mpileup_compat = 1: the insertions of the loaded reads that hold pads (c3r_padins_t, sorted by read and query offset) — what a caller that
 * rebuilds alt_info from c3r_get_tokens needs beside the read bases (`+3T*T`, samtools >= 1.11).  out may be NULL to ask for the count; empty
 * for every CIGAR an aligner emits.  Valid after c3r_load_reads / c3r_set_params. */
int c3r_get_pad_insertions(c3r_ctx *ctx, c3r_padins_t *out, int64_t cap, int64_t *n);
/* Debug / parity: per-position columns of the last scan.  cols: int32 [n_pos][C]; depth: int32
 * [n_pos]; flags: uint8 [n_pos] (bit0 = row exists, bit1 = candidate gate passed, bit2 = emitted).
 * Position i is 1-based ctg position region_start + i where region_start is returned. */
int c3r_get_columns(c3r_ctx *ctx, int64_t *region_start, int64_t *n_pos, int32_t *cols, int32_t *depth,
                    uint8_t *flags, int64_t cap_pos);

/* ---- network (A6/A7) ----------------------------------------------------------------------- */
/* Upload network weights: a flat fp32 blob in Keras layout (documented in DESIGN.md §weights):
 * per LSTM layer and direction K[in,4H], R[H,4H], b[4H] (gate order i,f,c,o); then L4, L5_1, L5_2,
 * Y_gt21, Y_genotype (W[in,out], b[out]).  Replaces m.load_weights (clair3_rna/call_variants.py:1472).
 * `channels` is 18 or 30 and must match c3r_set_params. */
int c3r_load_weights(c3r_ctx *ctx, const float *blob, int64_t n_floats, int channels);
int64_t c3r_weight_count(int channels);
/* Arithmetic of the network GEMMs: 0 = fp32 in / fp32 accumulate (v_mfma_f32_32x32x2_f32); 1 (default) = split-f16:
 * every fp32 operand carried as hi + lo halves, products hi*hi + hi*lo + lo*hi accumulated in fp32 on the f16 matrix
 * pipe (fp32-equivalent: both modes meet the 1e-4 probability tolerance against the fp32 oracle).  The input counts are no exception in
 * modes 1, 2 and 3: layer 1 carries every int32 count as up to four f16 integers that sum to it exactly (one f16 holds integers only up to
 * 2048 and ends at 65504, and a window's flank is not bounded by the depth > 216 rescale, which divides by the centre position's depth),
 * so any count a caller or the tensor build delivers is taken as it is — nothing is rounded, nothing refused, no mode steps down;
 * 2 = f16 main term + both correction terms on the block-scaled fp8 pipe (v_mfma_scale_f32_32x32x64_f8f6f4): ~1.15x the
 * throughput of mode 1, max |dP| 2-3e-5 on N(0, 0.05) weights but NOT robust to weights of 2-3x that norm — opt-in;
 * 3 = auto: mode 2 if it agrees with mode 1 to 4e-5 on 2048 calibration windows run through the loaded weights (measured at
 * c3r_load_weights / here), else mode 1.  Modes 2 and 3 need 18- or 30-channel weights like the others. */
int c3r_set_precision(c3r_ctx *ctx, int mode);
/* The mode the network runs in (after "auto" and the split-f16 guard have decided) and the fp8 calibration's max |dP| (-1: not measured). */
int c3r_get_precision(c3r_ctx *ctx, int *mode_in_use, double *calibration_err);
/* The guard of the split-f16 arithmetic itself.  Nothing in clair3_rna/model.py:126-172 bounds a trained model's weights, and f16 ends at
 * 65504: c3r_load_weights refuses non-finite values, packs every layer (LSTM 1, LSTM 2, L4) with the largest power-of-two scale <= 2^12
 * that keeps 2^s max|w| <= 2^15 (scale_log2[3]; 12 12 12 for ordinary weights), and runs 2048 pileup-shaped calibration windows through the
 * fp32 MFMA path and the split-f16 path: f16_err = max |dP| between them.  Above 1e-4 (the parity tolerance: the two paths drift apart with
 * the weights' gain exactly as each drifts from an fp32 CPU evaluation) a request for mode 1, 2 or 3 is served by mode 0
 * (fp32 MFMA, about a third of the speed), *fell_back = 1, and a warning goes to stderr.  Any pointer may be NULL. */
int c3r_get_precision_guard(c3r_ctx *ctx, double *f16_err, int32_t *scale_log2, int *fell_back);
/* Optional: size the network's device buffers for batches of up to n_sites candidates now (after c3r_load_weights) instead of
 * inside the first c3r_infer.  The layer-1 output of a full 2^18-site slice is 8.9 GB, and a first hipMalloc of that size takes
 * 0.25-0.4 s: a caller that is still waiting for its input (a BAM fetch) spends them here for free. */
int c3r_reserve(c3r_ctx *ctx, int64_t n_sites);
/* Forward pass over tensors.  tensors==NULL: use the device-resident tensors of the last scan.
 * Otherwise `tensors` is a host int32 [n][33][C] array.  probs (host, [n][24]) may be NULL to keep
 * the result on the device only.  Replaces m.predict_on_batch (clair3_rna/call_variants.py:1505). */
int c3r_infer(c3r_ctx *ctx, const int32_t *tensors, int64_t n, float *probs);
/* Fetch the [n][24] probabilities of the last c3r_infer(…, probs = NULL) — lets the caller queue the network on this
 * context's stream, do other work (e.g. the tensor build of the next contig on a second context), and collect later. */
int c3r_get_probs(c3r_ctx *ctx, float *probs, int64_t n);

/* ---- decode on the host (A8) --------------------------------------------------------------- */
/* Probabilities -> genotype / ALT / QUAL -> VCF text rows, replacing batch_output / output_with / output_from
 * (clair3_rna/call_variants.py:1077-1392, :684-1020).  c3r_call_rows works on the resident candidates after
 * c3r_infer: it rebuilds each site's ordered alt_info from the per-read tokens (src/create_tensor_pileup.py:221-261,
 * 595-596), decodes on host threads and caches the '\n'-terminated rows; c3r_get_rows copies them out.
 * qual < 0 means "no quality cut-off" (--qual None); show_ref != 0 keeps RefCall rows (--showRef). */
int c3r_call_rows(c3r_ctx *ctx, const char *ctg, int qual, int show_ref, int64_t *out_len, int64_t *n_rows);
int c3r_get_rows(c3r_ctx *ctx, char *out, int64_t cap);
/* The same in two steps, so that the context can go on to the next contig while host threads decode this one: c3r_rows_begin (after
 * c3r_infer) copies sites, tokens, probabilities and the read bases to the host and returns a snapshot; from then on the context may load
 * new reads / a new reference (the snapshot keeps its contig's reference buffer alive).  c3r_rows_decode / c3r_rows_get work on the
 * snapshot from ANY thread, no GPU involved.  c3r_rows_free must be called before c3r_destroy of the context that made the snapshot. */
int c3r_rows_begin(c3r_ctx *ctx, c3r_rows **out);
/* The same with two ways of moving less.  drop_ref_calls != 0: the snapshot holds only the sites that can print a row when the decoder runs
 * WITHOUT show_ref — a site whose probabilities take the decoder's early RefCall exit (P(0/0) >= 0.5 and P(gt21 = ref ref) >= 0.5,
 * clair3_rna/call_variants.py:540-542) or whose reference class wins the first round of its arg-max (:730-760: no class product exceeds
 * P(0/0) * P(ref ref)) prints nothing then, whatever its alt_info holds, so neither its record nor its tokens nor its
 * probabilities leave the device (a trained model calls ~97 % of the candidates that way); decoding such a snapshot with show_ref != 0 is
 * an error of the caller (those rows are gone).  host_reads / host_seq: the arrays that were handed to c3r_load_reads for the loaded contig,
 * if the caller keeps them alive and unchanged until c3r_rows_free — the decoder then reads inserted bases from them in place instead of
 * from a copy fetched back from the device (both NULL: fetched back, as c3r_rows_begin does). */
int c3r_rows_begin_ex(c3r_ctx *ctx, int drop_ref_calls, const c3r_read_t *host_reads, const uint8_t *host_seq, c3r_rows **out);
int c3r_rows_decode(c3r_rows *rows, const char *ctg, int qual, int show_ref, int64_t *out_len, int64_t *n_rows);
int c3r_rows_get(c3r_rows *rows, char *out, int64_t cap);
/* What the snapshot brought off the device (read-only, valid until c3r_rows_free, also after c3r_rows_decode): the sites it holds
 * (drop_ref_calls: the kept ones), the bytes of its packed token stream (one per token of the kept sites; without drop_ref_calls the whole
 * token slot space, which the sites' tok_off address) and its indel records (one per token with indel != 0).  Any pointer may be NULL. */
int c3r_rows_info(const c3r_rows *rows, int64_t *n_sites, int64_t *n_token_bytes, int64_t *n_indel_records);
void c3r_rows_free(c3r_rows *rows);
/* The same decoder on caller-supplied text (no GPU, no context): n sites, alt_info strings "<depth>-<k v ...>".
 * Returns C3R_EOVERFLOW (with *out_len = bytes needed, excluding the NUL) when `out` is too small. */
int c3r_decode_text(const char *ctg, int64_t n, const int32_t *pos, const char *ref33s, int ref33_stride, const char *const *alt_infos,
                    const float *probs, int qual, int show_ref, char *out, int64_t cap, int64_t *out_len);

/* ---- measurement --------------------------------------------------------------------------- */
/* When enabled, every kernel launch is bracketed by HIP events on the context's stream and the
 * elapsed times are accumulated per kernel name. */
int c3r_set_profiling(c3r_ctx *ctx, int enabled);
int c3r_reset_kernel_stats(c3r_ctx *ctx);
/* Writes up to cap entries; returns the number of distinct kernels via *n.  names[i] points into
 * storage owned by the context. */
int c3r_get_kernel_stats(c3r_ctx *ctx, const char **names, double *total_ms, int64_t *launches, int cap, int *n);
/* Which kernels built the spans of the last c3r_pileup_scan / c3r_pileup_scan_regions (read-only; tests and tuning).  listed: the spans
 * that met enough records to be built at all; deep: those of 2048 records or more in range, left to k_fused_deep (the others are
 * k_fused_tiles'); giant: those of 8192 records or more; slices: the record slices listed for k_deep_walk — 0 while the context has no
 * giant-span pool yet (it is allocated after the first scan that met a giant span), and only the first 256 giant spans of a scan are
 * sliced.  All zero after a scan that took the column store (head/tail calling, splice padding, genotyping mode) or found nothing to
 * scan.  Any pointer may be NULL. */
int c3r_get_scan_counts(c3r_ctx *ctx, int32_t *listed, int32_t *deep, int32_t *giant, int32_t *slices);

#ifdef __cplusplus
}
#endif
#endif /* C3R_H */
