/*
 * grafimo_hip.h -- C ABI of libgrafimo_hip.so, the MI355X (gfx950) implementation of
 * GRAFIMO's k-mer scoring hot path.
 *
 * GRAFIMO has no FFI of its own for this path: its native pieces are a Cython module
 * (`motif_processing`) and a numba-jitted function.  Each entry point below names the
 * reference interface it replaces (paths relative to /root/reference/src/grafimo/);
 * INTEGRATION.md shows the ctypes stubs a GRAFIMO maintainer would add to call them.
 *
 * Conventions
 *  - plain C types only; matrices are row-major [4][W] with rows A,C,G,T;
 *    L = 1000*W + 1 is the length of every per-score table (RANGE=1000, utils.py:26);
 *  - every function returns GFM_OK (0) or a negative GFM_ERR_* code and never throws;
 *    gfm_last_error() returns a thread-local message for the last failure;
 *  - pointers named h_* are host memory, d_* are device memory of the current HIP device
 *    (e.g. torch tensors' data_ptr()); the library never keeps a caller pointer after return
 *    (one exception, by its purpose: gfm_graph_hit_columns_start, until its _wait has returned);
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Functions that take
 *    a stream only enqueue work (no allocation, no synchronisation: graph-capturable);
 *  - HIP is initialised lazily by the first call that needs a device, never at load time,
 *    so a host that forks workers later (extract_regions.py:128) stays legal.
 */
#ifndef GRAFIMO_HIP_H
#define GRAFIMO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFM_ABI_VERSION 12

#define GFM_OK 0
#define GFM_ERR_INVALID (-1)  /* bad argument (NULL, width out of range, ...)            */
#define GFM_ERR_ASSERT (-2)   /* a reference `assert` would fire (bg<=0, prob<=0, ...)   */
#define GFM_ERR_HIP (-3)      /* HIP runtime failure, text in gfm_last_error()           */
#define GFM_ERR_NOMEM (-4)
#define GFM_ERR_NODEVICE (-5) /* no usable gfx950 device                                 */
#define GFM_ERR_IO (-6)       /* file could not be read / malformed row                  */
#define GFM_ERR_OVERFLOW (-7) /* an output buffer was too small                          */

#define GFM_MAX_WIDTH 64      /* widest motif the kernels are instantiated for           */
#define GFM_NO_SELECT INT32_MAX
/* flags */
#define GFM_FLAG_RESET_HITS 1u /* start the hit list at 0 instead of appending at *d_hit_count */
#define GFM_FLAG_CLEAR_HIST 2u /* gfm_qvalue_table: zero the histogram after reading it        */
/* gfm_score_kmers with a tail stream: the caller guarantees (by its own stream order, or because the
 * host has seen it complete) that the tail work of the call GFM_WORKSPACE_RING (four) before this one on the same handle
 * has finished -- the handle's scoring workspace is a ring of that many -- so the library need not make the main
 * stream wait for it (an event wait is a barrier packet in front of the score kernel: several
 * microseconds of an idle GPU per step).  The library honours the flag only while the GFM_WORKSPACE_RING calls before this one
 * on the handle were made with the same (stream, tail_stream) pair -- a second user of the handle in between (another
 * scanner, a batched call) makes it fall back to its own event wait. */
#define GFM_FLAG_CALLER_ORDERS_REUSE 4u
#define GFM_WORKSPACE_RING 4
/* gfm_score_kmers with a tail stream, together with GFM_FLAG_CALLER_ORDERS_REUSE: consecutive calls have no data
 * dependency on each other, so their score kernels need not run in stream order.  The library then launches the kernel
 * on one of two streams of the handle's own, taken in turn, instead of on `stream`: no barrier stands between the
 * kernels of calls k and k+1, the workgroups of k+1 take the compute units as those of k leave them, and the ramp-down
 * of one kernel overlaps the ramp-up of the next.  What a flagged call promises and gets:
 *   - the k-mers are COMPLETE when the call is made, and stay untouched until the call's tail work is done: the kernel
 *     is not ordered behind `stream`.  The library checks the cheap half of that: when hipStreamQuery(stream) finds
 *     anything pending on `stream` (possibly the k-mers' producer) this call's kernel -- and, unasked, those of the next
 *     three flagged calls -- waits for an event recorded on `stream` at the call: ordered behind all that `stream` holds
 *     then, still not behind the previous call's kernel.  An event wait appears nowhere else;
 *   - d_scores, d_hist and d_hit_* are ordered behind `tail_stream` at this point, and NOT behind `stream`: a consumer
 *     waits for the tail stream (an event recorded on it after the call), also for the scores;
 *   - the promise of GFM_FLAG_CALLER_ORDERS_REUSE extends to d_scores and d_kmers: whoever read or wrote them before
 *     is done when the call is made.
 * Honoured only where GFM_FLAG_CALLER_ORDERS_REUSE is (the GFM_WORKSPACE_RING calls before this one on the handle came
 * from the same stream pair), and not for a call that appends to a hit list (selection without GFM_FLAG_RESET_HITS:
 * its kernel reads the count the previous call's tail publishes).  Whether to pass it is the caller's choice per
 * call: under overlap the next kernel's first workgroups take the compute units a split call leaves free for the tail,
 * so a long tail (a q-value threshold: q-table, then the selection) finishes later (scan.KmerScanner does not pass the
 * flag for such batches).  gfm_motif_set_overlap(m, 0) makes a handle ignore
 * the flag (A/B runs, bisecting: the Python binding calls it for every handle it creates while the environment
 * variable GRAFIMO_SCORE_OVERLAP is 0).  gfm_score_kmers_multi, the streamed scan and the graph calls never overlap
 * their launches. */
#define GFM_FLAG_OVERLAP_LAUNCHES 8u
/* a hit-list entry packs the global row id and the row's scaled score:
 * entry = (row << GFM_HIT_SCORE_BITS) | score   (score <= 1000*64 < 2^20) */
#define GFM_HIT_SCORE_BITS 20

/* ------------------------------------------------------------------ library / device */
int gfm_abi_version(void);
const char *gfm_last_error(void);
int gfm_device_count(int *count);
int gfm_set_device(int ordinal);

/* ------------------------------------------------------------------ motif preprocessing
 * replaces compute_log_odds(probs_matrix, width, bgs, alphabet, nucsmap, debug)
 * (motif_processing.pyx:512-548 -> :444-507; lg2 utils.py:479-493):
 *   out[n][j] = ln(probs[n][j] / bg[n]) * 1.44269504   (host libm, f64). */
int gfm_compute_log_odds(const double *h_probs, int width, const double *h_bg,
                         double *h_logodds_out);

/* replaces scale_pwm(motif_matrix, alphabet, motif_width, nucsmap, debug)
 * (motif_ops.py:1027-1111): integer scaling to [0,1000], round-half-to-even. */
int gfm_scale_pwm(const double *h_logodds, int width, int64_t *h_score_matrix_out,
                  int *min_val, int *max_val, int *scale, double *offset);

/* replaces comp_pval_mat(motif, debug) (motif_processing.pyx:608-632 -> :552-603):
 * Staden-1994 score-distribution DP, run ON DEVICE; h_pmf_out has L doubles
 * (last DP row, un-normalised), bit-identical to the reference's. */
int gfm_comp_pval_mat(const int64_t *h_score_matrix, int width, const double *h_bg,
                      double *h_pmf_out);
/* The same for a motif set in one device pass (one DP launch, one workgroup per motif).
 * h_score_matrices: the [4, W_i] matrices concatenated; h_bgs: [n_motifs][4];
 * h_pmf_out: motif i at offset sum_{j<i} (1000*W_j + 1).  Every motif is checked before
 * the device is touched; an error message names the failing motif's index. */
int gfm_comp_pval_mat_many(int n_motifs, const int64_t *h_score_matrices, const int *widths,
                           const double *h_bgs, double *h_pmf_out);

/* ------------------------------------------------------------------ device-resident motif
 * The numeric content of a reference `Motif` (motif.py:18) that scoring reads:
 * score_matrix, bg, min_val, scale, offset, width, pval_matrix. */
typedef struct gfm_motif *gfm_motif_t;

/* Uploads the tables to the current device.  min_val must be the minimum of h_score_matrix
 * (Motif.min_val: what a k-mer holding N scores).  If h_pmf is NULL the DP of
 * gfm_comp_pval_mat runs on device; otherwise h_pmf (L doubles) is taken as the motif's
 * pval_matrix.  Also builds p_table[s] = sum(pmf[s:]) / sum(pmf) on device -- the O(1)
 * form of score_sequences.py:390-391 -- and the kernel workspace. */
int gfm_motif_create(const int64_t *h_score_matrix, int width, const double *h_bg,
                     int min_val, int scale, double offset, const double *h_pmf,
                     gfm_motif_t *out);
/* n_motifs handles in one device pass: one DP launch for the motifs whose h_pmfs[i] is NULL
 * (h_pmfs itself may be NULL: every DP runs on device), one tail-table launch for all, one
 * synchronisation.  Arrays as gfm_comp_pval_mat_many, min_vals / scales / offsets [n_motifs].
 * Checks and codes are gfm_motif_create's, each message names the motif's index.  All or
 * nothing: on failure every out[i] is NULL and nothing stays allocated.  Each handle is
 * destroyed on its own (gfm_motif_destroy). */
int gfm_motif_create_many(int n_motifs, const int64_t *h_score_matrices, const int *widths,
                          const double *h_bgs, const int *min_vals, const int *scales,
                          const double *offsets, const double *const *h_pmfs, gfm_motif_t *out);
void gfm_motif_destroy(gfm_motif_t m);
int gfm_motif_width(gfm_motif_t m);
int gfm_motif_table_len(gfm_motif_t m); /* L */
/* lowest / highest reachable scaled score (support of the pmf) */
int gfm_motif_score_range(gfm_motif_t m, int32_t *lo, int32_t *hi);
/* host copies of the device tables (either pointer may be NULL) */
int gfm_motif_tables(gfm_motif_t m, double *h_pmf_out, double *h_ptable_out);
/* smallest scaled score s with p_table[s] < threshold (strict, resultsTmp.py:303-307);
 * L if none. */
int gfm_motif_pvalue_cutoff(gfm_motif_t m, double threshold, int32_t *cutoff);
/* (scaled score) -> log-odds and p-value for a few rows on the host:
 * logodds = s/scale + W*offset (score_sequences.py:393), p = p_table[s]. */
int gfm_motif_annotate(gfm_motif_t m, const int32_t *h_scores, int64_t n,
                       double *h_logodds_out, double *h_pvalue_out);

/* ------------------------------------------------------------------ scoring
 * replaces the per-row body of score_seqs + compute_score_seq
 * (score_sequences.py:273-321, :331-396) for a dense batch of k-mers.
 *   d_kmers    uint8 [n][W], ASCII, row-major, 16-byte aligned base: the KMER column of
 *              the vg TSV rows.  A/a C/c G/g T/t score; a row holding 'N' (or any other
 *              byte whose bits 1-3 do not name A,C,G,T) scores min_val (:376-378).
 *   d_scores   int32 [n] out: scaled integer scores (16-byte aligned for the fastest stores;
 *              4-byte alignment is accepted); NULL: no score is stored -- the histogram and the hit
 *              list are all the caller wants (what the product's scans ask for: with a threshold the
 *              cutoff is known before scoring, so the array would never be read; 4 of the W + 4
 *              bytes a k-mer moves).
 *   d_hist     uint64 [L] in/out or NULL: d_hist[s] += #rows scored s.
 *   select_cutoff / d_hit_*: if select_cutoff != GFM_NO_SELECT, rows with
 *              score >= select_cutoff get the entry ((row_base + row) << 20 | score)
 *              appended to d_hit_rows (unordered) starting at *d_hit_count (at 0 with
 *              GFM_FLAG_RESET_HITS) and *d_hit_count updated; hits beyond hit_capacity are
 *              counted but not stored.
 * Enqueues the score kernel on `stream` and the small kernel that finishes d_hist and the hit
 * list on `tail_stream` (NULL = `stream`), ordered by events inside the library; with a separate
 * tail stream the next score kernel overlaps that tail and d_hist / d_hit_* are complete when
 * `tail_stream` reaches this point.  No host synchronisation. */
int gfm_score_kmers(gfm_motif_t m, const uint8_t *d_kmers, int64_t n, int32_t *d_scores,
                    uint64_t *d_hist, int32_t select_cutoff, int64_t row_base,
                    int64_t *d_hit_rows, int64_t hit_capacity, uint64_t *d_hit_count,
                    uint32_t flags, void *stream, void *tail_stream);

/* Batched form for motifs of ONE width (BASELINE config 5): the k-mer matrix is read once per
 * group of up to three motifs (as many as fit the LDS: tables, per-motif histogram windows and hit
 * queues), so per (k-mer, motif) pair the bytes moved drop from W + 4 to W/M + 4.  Arrays of
 * n_motifs entries; d_hist / select_cutoffs / d_hit_* may be NULL (or hold NULL / GFM_NO_SELECT
 * entries) exactly like the scalar arguments of gfm_score_kmers; d_scores may be NULL or hold only NULL
 * entries (no scores stored for any motif of the call).  Results are identical to
 * n_motifs separate gfm_score_kmers calls.  Single stream. */
int gfm_score_kmers_multi(const gfm_motif_t *motifs, int n_motifs, const uint8_t *d_kmers,
                          int64_t n, int32_t *const *d_scores, uint64_t *const *d_hist,
                          const int32_t *select_cutoffs, int64_t row_base,
                          int64_t *const *d_hit_rows, const int64_t *hit_capacity,
                          uint64_t *const *d_hit_count, uint32_t flags, void *stream);

/* Number of score kernels this handle has launched on its own launch streams with nothing in front of them so far
 * (GFM_FLAG_OVERLAP_LAUNCHES honoured, `stream` found empty); a flagged call that stayed on `stream` or waited for it
 * does not count. */
int gfm_overlapped_launches(gfm_motif_t m, uint64_t *count);
/* enabled == 0: this handle ignores GFM_FLAG_OVERLAP_LAUNCHES from now on (its launches stay on the caller's stream);
 * != 0: it honours the flag again (the default). */
int gfm_motif_set_overlap(gfm_motif_t m, int enabled);

/* How gfm_score_kmers_multi would group these motifs (no device work): group_size_out[i] = number of motifs of the
 * launch motif i rides in (1..3), waves_out[i] = waves per workgroup of that launch (16 or 8).  with_hist[i] != 0
 * (NULL = all): motif i accumulates a histogram, which is what limits a group (LDS windows).  Either output may be
 * NULL.  Lets a caller (and the parity tests) see which score_quad_kernel<W, MM> instantiation a call uses. */
int gfm_score_kmers_multi_plan(const gfm_motif_t *motifs, int n_motifs, const int32_t *with_hist,
                               int32_t *group_size_out, int32_t *waves_out);

/* Measurement aid (bench.py): with slots > 0 every `every`-th later gfm_score_kmers call
 * brackets the score kernel ALONE (not the post kernel that follows it) with a hipEvent pair
 * on the launch stream, in a ring of `slots` pairs; slots = 0 turns it off.  (The events ride on the
 * kernel's dispatch packet: start and completion of the kernel itself.)  gfm_profile_read waits for the recorded
 * events and returns the kernel durations in ms, oldest first. */
int gfm_profile_enable(gfm_motif_t m, int slots, int every);
int gfm_profile_read(gfm_motif_t m, float *h_ms_out, int capacity, int *n_out);
/* The TAIL of a timed gfm_score_kmers call that was given a tail stream: the library records a start event on the
 * tail stream behind its wait for the score kernel (i.e. when the tail may begin); gfm_profile_mark_tail records the
 * stop event on `stream` -- call it after everything that belongs to the step's tail has been enqueued (post kernel,
 * the all-reduce of the histogram, q-table, hit gather) on the stream the last of it runs on; a no-op when the last
 * call was not a timed one.  gfm_profile_read_tail returns the durations in ms, oldest first. */
int gfm_profile_mark_tail(gfm_motif_t m, void *stream);
int gfm_profile_read_tail(gfm_motif_t m, float *h_ms_out, int capacity, int *n_out);

/* Measurement aid (bench.py `peak_measured`): what THIS device sustains for a bare stream with the score kernel's
 * byte mix -- every lane issues `loads_per_store` 16-byte non-temporal loads per 16-byte store, loads and stores
 * interleaved in one pass, one step prefetched (the shape score_quad_kernel has; W = 19: 4.75 -> 5 loads per store).
 * in_bytes are read per launch (two input buffers used in turn), in_bytes / loads_per_store written, the output
 * rotating over three buffers;
 * store_policy 0 = nt, 1 = write-through (sc0 sc1).  Allocates and frees its own buffers; synchronous.
 * *us_per_launch = average of `launches` launches (HIP events), *bytes_per_launch = bytes read + written. */
int gfm_calibrate_stream(int loads_per_store, int64_t in_bytes, int store_policy, int launches,
                         double *us_per_launch, double *bytes_per_launch);

/* replaces compute_qvalues(pvalues, debug) (score_sequences.py:401-428; statsmodels
 * fdr_bh): Benjamini-Hochberg q-value of every scaled score, from the score histogram
 * of ALL scored rows:  q(s) = min(1, min_{s'<=s, hist[s']>0} p(s') / (C(s')/n)),
 * C(s') = #rows with score >= s'.  Also the selection cutoff: the smallest s with
 * (on_qvalue ? q(s) : p(s)) < threshold.  All outputs are device memory; any may be NULL. */
int gfm_qvalue_table(gfm_motif_t m, uint64_t *d_hist, double threshold, int on_qvalue,
                     double *d_qtable_out, int32_t *d_cutoff_out, uint64_t *d_nrows_out,
                     uint32_t flags, void *stream);
/* The same for n_motifs DISTINCT motifs (any widths) in three launches per eight motifs instead of three per
 * motif: the per-motif compute_qvalues calls of a motif set (score_sequences.py:401-428 once per motif,
 * grafimo.py:181-195).  Arrays of n_motifs entries; d_qtable_out / d_cutoff_out / d_nrows_out may be NULL or hold
 * NULL entries.  Results are identical to n_motifs gfm_qvalue_table calls. */
int gfm_qvalue_table_multi(const gfm_motif_t *motifs, int n_motifs, uint64_t *const *d_hist,
                           double threshold, int on_qvalue, double *const *d_qtable_out,
                           int32_t *const *d_cutoff_out, uint64_t *const *d_nrows_out, uint32_t flags,
                           void *stream);

/* replaces the threshold filter of ResultTmp.to_df (resultsTmp.py:303-307) on device:
 * appends the packed entry of every row with d_scores[row] >= *d_cutoff. */
int gfm_select_hits(gfm_motif_t m, const int32_t *d_scores, int64_t n, const int32_t *d_cutoff,
                    int64_t row_base, int64_t *d_hit_rows, int64_t hit_capacity,
                    uint64_t *d_hit_count, uint32_t flags, void *stream);
/* The same result -- the hit list restarted, holding the packed entry of every row with d_scores[row] >= *d_cutoff --
 * taken from a CANDIDATE list instead of the n scores when that list is complete: d_cand_rows / *d_cand_count is a
 * hit list as the fused selection of gfm_score_kmers left it for a cutoff that is known to be <= *d_cutoff.  With a
 * q-value threshold t (--qvalueT) the cutoff needs the global histogram, but q >= p (BH), so the rows with q < t
 * are among those with p < t: score with select_cutoff = gfm_motif_pvalue_cutoff(t) into the candidate list,
 * build the q-table, then call this -- it reads the few candidates, not every score (1e8 rows: 400 MB).  If the
 * candidate list overflowed (*d_cand_count > cand_capacity) the rows are taken from d_scores as gfm_select_hits
 * does (decided on the device, no host synchronisation).  Candidate and hit buffers must differ.  d_scores may be NULL for a
 * caller that stored no scores (gfm_score_kmers with d_scores == NULL) and has read *d_cand_count <= cand_capacity itself. */
int gfm_select_hits_from(gfm_motif_t m, const int32_t *d_scores, int64_t n, const int32_t *d_cutoff,
                         int64_t row_base, const int64_t *d_cand_rows, int64_t cand_capacity,
                         const uint64_t *d_cand_count, int64_t *d_hit_rows, int64_t hit_capacity,
                         uint64_t *d_hit_count, void *stream);

/* ------------------------------------------------------------------ strand-max and per-region best hit
 * BASELINE.json north_star: "wavefront-level reductions for forward/reverse-strand max ... RCCL only for the final
 * top-hit gather".  The reference has neither: every strand is a row of its own (score_sequences.py:279-321) and the
 * report lists rows.  Its one consumer of "the best hit of a region" is --top-graphs, which takes the first N
 * distinct sequence_names of the table sorted by p-value (res_writer.py:153-157) -- the regions ranked by their best
 * reported hit.  These entry points compute that key on the device and NEVER change the reported rows;
 * grafimo_amd/top_hits.py builds the top-regions table from them and, under torch.distributed, gathers
 * n_regions entries per rank instead of every hit.
 *
 * Rows taking part: score >= max(min_score, *d_cutoff) (d_cutoff may be NULL; the q-value cutoff of gfm_qvalue_table
 * lives on the device), a region id in [0, n_regions), and -- if d_freq is given -- d_freq[row] > 0 (the rows
 * ResultTmp.to_df keeps without --recomb, resultsTmp.py:309-310).
 *
 * gfm_region_best: d_best[r] = max over the rows of region r of  (score << GFM_BEST_ROW_BITS) | (2^44 - 1 - row),
 *   row = row_base + index: the best score, the lowest row among equals; 0 = no such row.  d_best is in/out
 *   (atomic max: batches and chunks accumulate; the caller zeroes it).  d_region int32 [n], any order -- rows of one
 *   region that are contiguous (TSV files, extraction rows) cost one atomic per wavefront instead of one per row.
 * gfm_region_ids: the d_region array of rows laid out region after region, from d_region_off int64 [n_regions + 1]
 *   (rows [off[r], off[r+1]) belong to region r): the TSV scan's files, row_base per file.
 * gfm_locus_max: d_locus_max[i] = the best score among the rows of i's locus -- same region, same
 *   {start, stop} as a set: the reference span of the k-mer whatever its strand ('-' rows carry start > stop,
 *   score_sequences.py:288-291) -- i.e. the forward/reverse-strand maximum at that span; -1 for rows that take no part.
 *   d_work: gfm_locus_max_workspace(n) bytes of scratch, 8-byte aligned; its first 8 bytes hold, afterwards, the number
 *   of rows that found no table slot (0 unless the workspace was smaller than asked for).  Enqueue only. */
#define GFM_BEST_ROW_BITS 44
int gfm_region_ids(const int64_t *d_region_off, int32_t n_regions, int64_t n, int32_t *d_region_out, void *stream);
int gfm_region_best(const int32_t *d_scores, int64_t n, const int32_t *d_region, int32_t n_regions,
                    const int64_t *d_freq, int32_t min_score, const int32_t *d_cutoff, int64_t row_base,
                    uint64_t *d_best, void *stream);
int64_t gfm_locus_max_workspace(int64_t n_rows);
int gfm_locus_max(const int32_t *d_scores, int64_t n, const int32_t *d_region, int32_t n_regions,
                  const int64_t *d_start, const int64_t *d_stop, const int64_t *d_freq, int32_t min_score,
                  const int32_t *d_cutoff, void *d_work, int64_t work_bytes, int32_t *d_locus_max, void *stream);

/* ------------------------------------------------------------------ one-call host form
 * compute_results' numeric core (score_sequences.py:44-211) for host-resident k-mers:
 * H2D, score, histogram, q-table, threshold, D2H of the hits only.
 *   h_kmers uint8 [n][W]; threshold in (0,1]; on_qvalue: threshold applies to q (--qvalueT);
 *   want_qvalues: compute q-values (0 = --no-qvalue);
 *   outputs (caller-allocated, capacity rows each; h_qvalue_out may be NULL):
 *   hit rows ascending by row index with their scaled score, log-odds, p-value, q-value. */
int gfm_scan_host(gfm_motif_t m, const uint8_t *h_kmers, int64_t n, double threshold,
                  int on_qvalue, int want_qvalues, int64_t capacity, int64_t *h_hit_rows_out,
                  int32_t *h_hit_scores_out, double *h_logodds_out, double *h_pvalue_out,
                  double *h_qvalue_out, int64_t *n_hits_out);

/* ------------------------------------------------------------------ TSV ingest (host, C++)
 * replaces the text handling of score_seqs (score_sequences.py:273-293, :305-307):
 * parses vg's 7-column rows  REGION KMER CHR:START(+|-) CHR:STOP(+|-) COUNT ref|non.ref PATH
 * into columnar arrays.  Two calls: gfm_tsv_open counts, gfm_tsv_read fills. */
typedef struct gfm_tsv *gfm_tsv_t;
/* Parses every file (host threads) and reports the number of kept rows.
 * skip_reverse: drop '-' rows before they are counted (--no-reverse, :281-282).
 * n_threads: the reference's `cores` (score_sequences.py:123); <= 0 = every hardware thread.  The library uses
 * at most that many, and never more than one per file, one per MiB of text, or 96; the threads belong to a crew
 * the library keeps for the life of the process (the VCF reader and the streamed scan share it). */
int gfm_tsv_open(const char *const *paths, int n_paths, int width, int skip_reverse,
                 int n_threads, gfm_tsv_t *out, int64_t *n_rows);
/* The first pass of the streamed scan on its own (gfm_scan_tsv_begin reads a file, counts its rows, and parses it in
 * place once every earlier file is counted): the rows gfm_tsv_open would keep of this file -- lines that hold a field,
 * minus the '-' rows with skip_reverse -- without parsing them.  Equal to the parsed count for every file the parser
 * accepts (the CPU tests hold it to that). */
int gfm_tsv_count_rows(const char *path, int skip_reverse, int64_t *n_rows);
/* Copies the parsed columns out (any pointer may be NULL):
 * kmers uint8[n][W]; start/stop int64[n]; strand uint8[n] ('+'/'-'); freq int64[n];
 * is_ref uint8[n] (1 = "ref" after the indel fix :305-307, 0 = "non.ref");
 * file_id int32[n] (index into paths); name_id int32[n] (index into the REGION names). */
int gfm_tsv_read(gfm_tsv_t t, uint8_t *kmers, int64_t *start, int64_t *stop, uint8_t *strand,
                 int64_t *freq, uint8_t *is_ref, int32_t *file_id, int32_t *name_id);
/* distinct REGION strings: count, total bytes, then offsets[count+1] + bytes */
int gfm_tsv_name_count(gfm_tsv_t t);
int64_t gfm_tsv_names_bytes(gfm_tsv_t t);
int gfm_tsv_names(gfm_tsv_t t, int64_t *offsets, char *bytes);
void gfm_tsv_close(gfm_tsv_t t);

/* ------------------------------------------------------------------ streamed scan of a TSV directory
 * compute_results' numeric core (score_sequences.py:113-157, :194-205) as ONE pipelined pass over the
 * width_W TSV files of a motif: host threads parse the files (in path order) while earlier rows are
 * already copied (pinned chunk buffers, hipMemcpyAsync on a copy stream) and scored (one score launch
 * per chunk, one histogram and one hit list for the whole scan, row ids global in path order);
 * the q-value table and the threshold run once at the end and only the hit rows come back.
 * Buffers are kept per device between calls (gfm_scan_release_buffers frees them).
 *   threshold / on_qvalue / want_qvalues as gfm_scan_host; chunk_rows: rows per chunk (<= 0: default);
 *   *n_rows = rows scored (kept rows of all files), *n_hits = rows under the threshold. */
typedef struct gfm_scan *gfm_scan_t;
typedef struct gfm_scan_stats {
    int64_t n_rows, n_hits, n_chunks, h2d_bytes;
    double total_s;      /* wall time of the call                                           */
    double parse_s;      /* until the last file was parsed (copies and kernels overlap it)   */
    double h2d_s;        /* sum of the host-to-device copy durations (hipEvents)             */
    double tail_s;       /* after the last file was parsed: last chunk, tables, hits back    */
    int32_t parse_threads, reserved;
} gfm_scan_stats_t;
int gfm_scan_tsv(gfm_motif_t m, const char *const *paths, int n_paths, int skip_reverse, int n_threads,
                 double threshold, int on_qvalue, int want_qvalues, int64_t chunk_rows, gfm_scan_t *out,
                 int64_t *n_rows, int64_t *n_hits);
/* The same pass in two phases and for several motifs of ONE width (each chunk is scored by gfm_score_kmers_multi: one
 * read of the k-mers per group of up to three motifs) -- what compute_results_many and the sharded scan
 * (grafimo_amd/distributed.py) run: the reference's loop over a motif set (grafimo.py:177-183) repeats ingest and
 * scoring per motif, and its multiprocessing has no second phase because it has no second machine.
 * gfm_scan_tsv_begin parses, uploads and scores; when it returns every motif's histogram is complete on the device
 * (d_hist[j]: the caller's buffers of L uint64 each -- zeroed here -- or NULL for the library's own) and *n_rows rows
 * were scored.  A sharded caller now all-reduces its histogram buffers over the ranks (and synchronises).
 * gfm_scan_tsv_finish derives the q-tables and cutoffs from the histograms as they are then, selects, and brings the
 * hits back: n_hits[j] rows for motif j (n_hits may be NULL).  Row ids are local to this call's files. */
int gfm_scan_tsv_begin(const gfm_motif_t *motifs, int n_motifs, const char *const *paths, int n_paths,
                       int skip_reverse, int n_threads, double threshold, int on_qvalue, int want_qvalues,
                       int64_t chunk_rows, uint64_t *const *d_hist, gfm_scan_t *out, int64_t *n_rows);
int gfm_scan_tsv_finish(gfm_scan_t s, int64_t *n_hits);
/* gfm_scan_hits for motif `motif` of a multi-motif scan */
int gfm_scan_hits_of(gfm_scan_t s, int motif, int64_t *rows, int32_t *scaled, double *logodds, double *pvalue,
                     double *qvalue, uint8_t *kmers, int64_t *start, int64_t *stop, uint8_t *strand,
                     int64_t *freq, uint8_t *is_ref, int32_t *name_id);
/* The hit rows ascending by row id, each with the columns of its TSV row (any pointer may be NULL;
 * n_hits entries each, kmers n_hits x W bytes; qvalue only if the scan computed q-values). */
int gfm_scan_hits(gfm_scan_t s, int64_t *rows, int32_t *scaled, double *logodds, double *pvalue,
                  double *qvalue, uint8_t *kmers, int64_t *start, int64_t *stop, uint8_t *strand,
                  int64_t *freq, uint8_t *is_ref, int32_t *name_id);
int gfm_scan_stats(gfm_scan_t s, gfm_scan_stats_t *out);
/* the parsed table behind the scan (REGION names: gfm_tsv_name_count / gfm_tsv_names); owned by the scan
 * handle -- do not gfm_tsv_close it */
gfm_tsv_t gfm_scan_table(gfm_scan_t s);
void gfm_scan_close(gfm_scan_t s);
void gfm_scan_release_buffers(void);

/* ------------------------------------------------------------------ k-mer extraction
 * Replaces the rows of `vg find -p CHR:S-E -x XG -H GBWT -K W -E` (extract_regions.py:180,225,326;
 * consumed by score_sequences.py:273-307) for graphs made of a linear reference plus SNP sites
 * insertions and deletions (the inputs of `vg construct -r REF -v VCF`, constructVG.py:332).  Rows are written on the device
 * in the layout gfm_score_kmers reads, so extraction -> scoring needs no TSV.  Pinned by the
 * reference's expected_seqs.tsv and by the 704 rows of real vg output in its scoring fixture
 * (SNPs, deletions, node ids and cuts also by vg's own node tables: tests/test_vg_pins.py).  Insertions, multi-base
 * substitutions and complex alleles are part of the graph too; oracle/extract_oracle.py states what no vg output pins
 * about them (coordinates of k-mers that start or end inside inserted bases, row order).
 *
 * gfm_graph_create: h_ref [ref_len] bases; sites ascending 0-based h_pos [n_sites], h_n_alts [n_sites]
 *   in 1..3, h_alt_bases [n_sites][3]; h_del_len [n_sites] (or NULL): 0 for a SNP, else the site is a
 *   deletion of that many bases after the anchor h_pos (one alternate allele; deletions may overlap -- several
 *   lengths at one anchor, anchors inside another deletion's span; at one position the substitution site comes
 *   first, then the insertions, then the deletions); h_alt_bits [n_sites][3][ceil(H/64)] =
 *   haplotypes carrying each alternate allele (bit h of word h/64; deletion carriers in slot 0), or
 *   NULL / H = 0 for no haplotype counts (freq = 0).
 *   Insertions (UNPINNED semantics, stated in oracle/extract_oracle.py): h_ins_len [n_sites] (or NULL): > 0 for a
 *   site that holds that many inserted bases h_ins_bases[h_ins_off[i] ..] behind its anchor h_pos (one alternate
 *   allele, carriers in slot 0).  At one position the substitution site comes first, then any number of
 *   insertions, then the deletion.  A walk that reads inserted bases consumes window bases but no reference span
 *   (stop = coordinate behind the last reference base it used); walks may start inside an insertion anchored at
 *   p - 1 (start = p); with insertions in the graph windows start at p in [S, E - 1] and a walk is kept if its
 *   stop lies inside the region.
 * gfm_graph_plan: regions [S, E] as vg takes them (windows start at p in [S, E - W]); returns the
 *   number of windows and of rows (2 per walk: forward, reverse complement).  Synchronous.  GFM_ERR_OVERFLOW: the rows do not
 *   fit one plan (more than 2^31 of them; a single window of more than 2^30 walks) -- plan fewer windows at a time
 *   (gfm_graph_plan_windows), or use gfm_graph_score, which writes no rows.
 * gfm_graph_emit: rows of the last plan, window-major, walks in mixed-radix order with the LAST site
 *   of the window varying fastest (windows that touch a deletion: layout-major -- the vectors of
 *   jumps over deletions in lexicographic order, "no jump" first, and on one such layout the mixed
 *   radix of the SNPs it meets), forward row then '-' row:  d_kmers [rows][W],
 *   d_start / d_stop (forward: p, e; '-': e, p; e = reference coordinate after the last base, p + W
 *   unless the walk jumps a deletion), d_strand ('+'/'-'), d_freq, d_is_ref (vg's flag: 1 = every SNP
 *   allele is the reference's, also when a deletion is taken), d_region (index into the plan's
 *   regions), d_walk (walk index inside its window).  Enqueue only. */
typedef struct gfm_graph *gfm_graph_t;
/* gfm_graph_validate: the checks gfm_graph_create makes of its arguments (minus h_alt_bits and out), on the host only:
 * GFM_OK or GFM_ERR_INVALID with the reason.  Touches no device. */
int gfm_graph_validate(const uint8_t *h_ref, int64_t ref_len, int32_t n_sites, const int32_t *h_pos,
                       const uint8_t *h_n_alts, const uint8_t *h_alt_bases, const int32_t *h_del_len,
                       const int32_t *h_ins_len, const int32_t *h_ins_off, const uint8_t *h_ins_bases,
                       int64_t ins_bytes, int32_t n_haplotypes);
int gfm_graph_create(const uint8_t *h_ref, int64_t ref_len, int32_t n_sites, const int32_t *h_pos,
                     const uint8_t *h_n_alts, const uint8_t *h_alt_bases, const int32_t *h_del_len,
                     const int32_t *h_ins_len, const int32_t *h_ins_off, const uint8_t *h_ins_bases,
                     int64_t ins_bytes, const uint64_t *h_alt_bits, int32_t n_haplotypes, gfm_graph_t *out);
void gfm_graph_destroy(gfm_graph_t g);
int gfm_graph_plan(gfm_graph_t g, int32_t n_regions, const int64_t *h_starts, const int64_t *h_stops,
                   int32_t width, int64_t *n_windows, int64_t *n_rows);
/* gfm_graph_plan for RANGES OF WINDOW STARTS: range r holds the windows p in [h_first[r], h_last[r]] of a region that ends at
 * h_limit[r] (a walk is kept if it ends inside its region) -- what a caller uses to cut a region whose rows do not fit one
 * plan (GFM_ERR_OVERFLOW: more than 2^31 rows) into several; d_region of gfm_graph_emit then indexes the ranges. */
int gfm_graph_plan_windows(gfm_graph_t g, int32_t n_ranges, const int64_t *h_first, const int64_t *h_last,
                           const int64_t *h_limit, int32_t width, int64_t *n_windows, int64_t *n_rows);
int gfm_graph_emit(gfm_graph_t g, uint8_t *d_kmers, int64_t *d_start, int64_t *d_stop, uint8_t *d_strand,
                   int64_t *d_freq, uint8_t *d_is_ref, int32_t *d_region, int32_t *d_walk, void *stream);

/* The files scan_graph leaves for GRAFIMO's own compute_results (extract_regions.py:165-170,180,225: one
 * `vg find ... > width_W/CHR_S-E.tsv` per region), written from the rows of gfm_graph_emit by host threads of the
 * library's crew: seven tab-separated columns per row as vg prints them --
 *     REGION  KMER  CHR:START(+|-)  CHR:STOP(+|-)  COUNT  ref|non.ref  NODE(+|-),NODE(+|-),...
 * -- d_* are the buffers gfm_graph_emit filled for this handle (n_rows rows, region-major), `width` the plan's;
 * h_region_stops [n_regions] the regions' E (a walk ends inside its region: the layouts of a window near the end depend on
 * it), h_labels [n_regions] column 1, h_paths [n_regions] the file of every region, chrom_name the name printed in columns 3
 * and 4.  Column 7 (vg's node ids along the walk, '-' rows reversed; the node numbering of `vg construct -m 32` on this graph,
 * pinned by vg's own .vg / .xg files) is left EMPTY with GFM_TSV_NO_NODEPATH: GRAFIMO's scoring never reads it
 * (score_sequences.py:279-293 uses columns 1-6).  h_seen [n_regions] in/out, zeroed by the caller before the first call of a
 * directory: a region whose file this sequence of calls already wrote is appended to (plans that cut one region into several
 * pieces, gfm_graph_plan_windows); regions that never get a row are left to the caller (vg's redirect leaves an empty file).
 * Synchronous: waits for `stream` (the emit), copies the rows to the host in chunks, returns when the files are closed.
 * n_threads <= 0: as many as the machine has, at most 32. */
#define GFM_TSV_NO_NODEPATH 1u
typedef struct gfm_tsv_write_stats {
    int64_t n_rows, n_files, bytes;
    double total_s, copy_s, format_s;   /* wall time; waiting for device->host copies; formatting + writing */
    int32_t threads, reserved;
} gfm_tsv_write_stats_t;
int gfm_graph_write_tsvs(gfm_graph_t g, const uint8_t *d_kmers, const int64_t *d_start, const int64_t *d_stop,
                         const uint8_t *d_strand, const int64_t *d_freq, const uint8_t *d_is_ref, const int32_t *d_region,
                         const int32_t *d_walk, int64_t n_rows, int32_t width, int32_t n_regions,
                         const int64_t *h_region_stops, const char *const *h_labels, const char *const *h_paths,
                         const char *chrom_name, uint32_t flags, int n_threads, uint8_t *h_seen, void *stream,
                         gfm_tsv_write_stats_t *stats);

/* ------------------------------------------------------------------ extraction fused into scoring
 * The join `extract_seqs -> score_seq` of the hot path without its intermediate: the reference writes every row of
 * `vg find -K W -E` to a TSV (extract_regions.py:180,225) and score_seqs reads them all back (score_sequences.py:273-321),
 * although only the rows under the threshold are ever reported (resultsTmp.py:303-310).  gfm_graph_score walks the
 * windows of the regions, scores both strands of every walk against the motif and keeps: the score histogram of ALL rows
 * (q-values are computed over all of them, score_sequences.py:194-198), the number of rows, and one 16-byte entry per row
 * with score >= select_cutoff.  gfm_graph_annotate then produces, for those entries only, the columns a TSV row would
 * have carried -- k-mer, start, stop, strand, haplotype count, vg's ref flag, region -- identical to what
 * gfm_graph_plan + gfm_graph_emit + gfm_score_kmers give for the same rows.
 *
 * gfm_graph_score: regions as gfm_graph_plan takes them; the motif's width is the k-mer width.
 *   flags: GFM_GRAPH_FORWARD_ONLY = skip the '-' rows before they are scored or counted (--no-reverse, :281-282).
 *   d_hist uint64 [L] in/out or NULL (+= rows per score); select_cutoff as gfm_score_kmers (GFM_NO_SELECT: no hits);
 *   d_hits gfm_graph_entry_t [hit_capacity], appended from *d_hit_count on (entries beyond the capacity are counted,
 *   not stored; the caller zeroes the counter); *d_n_rows += rows scored; *d_overflow (optional; the caller zeroes it
 *   with its counters, the kernels write it directly) = 1 if a window holds
 *   more than 2^40 walks, or the regions hold more than 2^20 windows of more than 64 walks each (those windows' rows are
 *   left out: score fewer regions at a time); *n_windows (host, optional) = windows of the call.  Entry order is
 *   arbitrary; the records of gfm_graph_annotate sorted by (w, q2) are in the row order of gfm_graph_emit.  Enqueue only (the first call for a
 *   (regions, width) pair builds and uploads its PLAN -- the tile table; the lists of the windows that touch an insertion /
 *   deletion and of the heavy windows follow on the device -- and later calls with the same regions and width reuse it; a handle
 *   keeps the plans of its 32 most recently used pairs: the widths of a motif set alternate, grafimo.py:177-183).
 * gfm_graph_annotate: for entry i < min(*d_hit_count, hit_capacity) the record d_records[i] of the LAST gfm_graph_score
 *   call on this handle; d_cutoff (device, optional): entries with score < *d_cutoff get keep = 0 and no columns (the
 *   p < t candidates of a --qvalueT scan that the q-value cutoff drops: q >= p); d_qtable (device, optional): the
 *   q-value of the entry's score.  Enqueue only.
 * One call at a time per graph handle: the fused calls of a handle share its scratch (overflow word, histogram slabs, the
 * plan's lists, the tile table), so a gfm_graph_score / gfm_graph_annotate on another stream than the handle's previous
 * call waits (an event, on the device) for that call's work; use one handle per stream for calls that should overlap. */
#define GFM_GRAPH_FORWARD_ONLY 1u
typedef struct gfm_graph_entry {   /* opaque to the caller, who only provides the room: */
    int32_t tile;       /* where the walk is among the call's windows (64 consecutive window starts of one region) */
    int32_t score;      /* scaled score */
    int64_t q2k;        /* window of the tile << 56 | (walk of the window * 2 + strand: 0 '+', 1 '-') */
} gfm_graph_entry_t;
typedef struct gfm_graph_hit {
    int64_t start, stop, freq, q2;
    double qvalue;
    int32_t w, score, region;
    uint8_t strand, is_ref, keep, pad;
    uint8_t kmer[GFM_MAX_WIDTH];
} gfm_graph_hit_t;
int gfm_graph_score(gfm_graph_t g, gfm_motif_t m, int32_t n_regions, const int64_t *h_starts, const int64_t *h_stops,
                    uint32_t flags, int32_t select_cutoff, uint64_t *d_hist, void *d_hits, int64_t hit_capacity,
                    uint64_t *d_hit_count, uint64_t *d_n_rows, int32_t *d_overflow, int64_t *n_windows, void *stream);
/* gfm_graph_score for up to THREE motifs of one width over ONE enumeration of the walks -- the `for motif in motif_set`
 * loop of grafimo.findmotif (grafimo.py:177-183; motifs are processed per width, motif_ops.py:303-311) for the motifs of a
 * width: tiles, site records, window classification and the walks' digits are shared, every motif has its own LDS score table,
 * histogram window, hit list and cutoff.  Arrays of n_motifs entries: select_cutoffs, d_hist (NULL or NULL entries: no
 * histogram for that motif), d_hits / hit_capacity / d_hit_count (one list per motif; the caller zeroes the counters).
 * *d_n_rows += rows scored PER MOTIF (every motif scores the same walks).  Results are identical to n_motifs gfm_graph_score
 * calls.  gfm_graph_annotate serves every motif's list in turn (the entries do not depend on the motif). */
int gfm_graph_score_multi(gfm_graph_t g, const gfm_motif_t *motifs, int32_t n_motifs, int32_t n_regions,
                          const int64_t *h_starts, const int64_t *h_stops, uint32_t flags, const int32_t *select_cutoffs,
                          uint64_t *const *d_hist, void *const *d_hits, const int64_t *hit_capacity,
                          uint64_t *const *d_hit_count, uint64_t *d_n_rows, int32_t *d_overflow, int64_t *n_windows,
                          void *stream);
/* Measurement aid (bench.py `extract.roofline`): with on != 0 the next (up to 64) gfm_graph_score[_multi] calls bracket
 * graph_score_kernel ALONE -- the kernel of the plain and one-deletion windows, the one the fused path's time is in -- with
 * a hipEvent pair on the launch stream; gfm_graph_profile_read waits for them and returns the durations in ms, oldest first.
 * gfm_graph_haplotype_classes brackets every launch of its own the same way, in launch order: per chunk of regions the key
 * kernel, the class kernel, one launch per batch of spilled regions, the verify kernel (scripts/classes_probe.py). */
int gfm_graph_profile_enable(gfm_graph_t g, int on);
int gfm_graph_profile_read(gfm_graph_t g, float *h_ms_out, int capacity, int *n_out);
int gfm_graph_annotate(gfm_graph_t g, const void *d_hits, const uint64_t *d_hit_count, int64_t hit_capacity,
                       const int32_t *d_cutoff, const double *d_qtable, void *d_records, void *stream);
/* The per-haplotype hit matrix of the entries of the LAST gfm_graph_score[_multi] call, the same list gfm_graph_annotate
 * serves: for region r of that call (0 .. n_regions - 1, the call's region list) and haplotype h of the graph (its bitset
 * order), d_counts[r * n_hap + h] = the entries with score >= *d_cutoff (d_cutoff NULL: all; --qvalueT as in annotate) of
 * region r whose walk h carries -- h is in the AND of the bitsets of the walk's allele constraints, the set whose size is
 * the record's freq -- and d_best[r * n_hap + h] = the highest scaled score among them (-1: none).  int32 [n_regions][n_hap]
 * each, device memory, overwritten.  scratch_bytes bounds the device scratch of the carrier masks (<= 0: 256 MB): the
 * entries are grouped by region on the device and taken in batches whose masks fit it; the result does not depend on it.
 * GFM_ERR_INVALID when the graph carries no haplotypes, n_regions is not that of the last call, or an output is NULL.
 * Enqueue only (stream-ordered device scratch); calls of one handle are serialised as gfm_graph_score's are. */
int gfm_graph_haplotype_hits(gfm_graph_t g, const void *d_hits, const uint64_t *d_hit_count, int64_t hit_capacity,
                             const int32_t *d_cutoff, int32_t n_regions, int32_t *d_counts, int32_t *d_best,
                             int64_t scratch_bytes, void *stream);
/* The per-hit allele table of the entries of the LAST gfm_graph_score[_multi] call, the same list gfm_graph_annotate serves,
 * indexed by the ENTRY index i (record i of gfm_graph_annotate).  For every entry with score >= *d_cutoff (d_cutoff NULL:
 * all; --qvalueT as in annotate):
 *   its alleles: the SET of (site, allele) constraints of its walk -- the constraints the haplotype counting ANDs: allele 0 =
 *     REF, 1..3 = ALT of a substitution site; 1 = an insertion read / a deletion jumped, 0 = passed by / its bases used / a
 *     deletion that would cover the window's first base -- packed site * 4 + allele, ascending, no pair twice, as CSR:
 *     d_allele_off int64 [hit_capacity + 1] (always written in full), d_alleles int32 [allele_capacity].  Constraints beyond
 *     allele_capacity are dropped: d_allele_off[hit_capacity] says how much room to come back with (allele_capacity 0 and
 *     d_alleles NULL: only ask);
 *   d_group_counts int32 [hit_capacity][n_groups]: the carriers of the entry -- the AND of the constraints' bitsets, the set
 *     whose size is the record's freq -- in each group, popcount(carriers & group).  d_group_bits uint64 [n_groups][hw]
 *     (hw = ceil(n_hap / 64), haplotype h = bit h & 63 of word h >> 6); groups may overlap and need not cover the haplotypes;
 *     n_groups 0 .. 64 (more: GFM_ERR_INVALID, nothing is truncated);
 *   d_total int32 [hit_capacity] (optional): the size of the carrier set, the kernel's own count of the record's freq;
 *   d_masks uint64 [hit_capacity][hw] (optional): the carrier set itself, the bits beyond n_hap clear.
 * Entries under the cutoff and slots behind *d_hit_count have no alleles and zeros everywhere.  A graph without haplotype
 * bitsets still gives the alleles; n_groups > 0, d_total or d_masks on it is GFM_ERR_INVALID.  scratch_bytes bounds the
 * device scratch (<= 0: 256 MB): the entries are taken in batches whose staging fits it; the result does not depend on it.
 * Enqueue only (stream-ordered device scratch); calls of one handle are serialised as gfm_graph_score's are. */
int gfm_graph_hit_alleles(gfm_graph_t g, const void *d_hits, const uint64_t *d_hit_count, int64_t hit_capacity,
                          const int32_t *d_cutoff, int32_t n_groups, const uint64_t *d_group_bits, int64_t *d_allele_off,
                          int32_t *d_alleles, int64_t allele_capacity, int32_t *d_group_counts, int32_t *d_total,
                          uint64_t *d_masks, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------ the report's rows from the hit records (host)
 * replaces what ResultTmp.to_df does with the rows that passed the threshold (resultsTmp.py:303-314): the --recomb filter
 * (:309-310: rows with haplotype_frequency == 0 are dropped unless --recomb), the ascending sort by p-value (:312; rows
 * of equal p-value stay in the order of the TSV rows -- chromosome entry, window, walk, strand -- as a stable sort over
 * the files' rows leaves them) and the columns of resultsTmp.py:270-301 as plain arrays.  No device is touched.
 *   h_ptable [table_len]: the motif's tail table (gfm_motif_tables), p-value of a row = h_ptable[score]
 *     (score_sequences.py:390-391); scale, offset, width: score = scaled / scale + width * offset (:393);
 *   h_recs[p] / n_recs[p]: the records gfm_graph_annotate wrote for one graph handle of the call, copied to the host;
 *   h_entry_of[p] (optional): int64 per region of that handle's region list -> the rank of its chromosome entry in the
 *     caller's order (rows are ordered by it first); region_base[p] (optional): added to a record's `region` in o_region;
 *   flags: GFM_HITS_DROP_ZERO_FREQ (no --recomb), GFM_HITS_FIRST_PER_REGION (only the first row of every region in
 *     report order: what --top-graphs walks, res_writer.py:153-157);
 *   outputs (caller-allocated for sum(n_recs) rows, any may be NULL): start, stop, haplotype_frequency, region,
 *     score = log-odds (score_sequences.py:393), p-value, q-value, strand (0 '+', 1 '-'), reference (1 = "ref": vg's
 *     flag AND |stop - start| == width, score_sequences.py:305-307), o_kmers [rows][width + 1] the k-mer and a '\n'
 *     (one decode + split makes the matched_sequence strings).  *n_out = rows written.
 *   A table of 4 096 rows or more is built with the help of up to four of the library's kept host threads when they are idle. */
#define GFM_HITS_DROP_ZERO_FREQ 1u
#define GFM_HITS_FIRST_PER_REGION 2u
int gfm_graph_hit_columns(const double *h_ptable, int32_t table_len, int32_t scale, double offset, int32_t width,
                          int32_t n_parts, const gfm_graph_hit_t *const *h_recs,
                          const int64_t *n_recs, const int64_t *const *h_entry_of, const int64_t *region_base,
                          uint32_t flags, int64_t *n_out, int64_t *o_start, int64_t *o_stop, int64_t *o_freq,
                          int64_t *o_region, double *o_score, double *o_pvalue, double *o_qvalue, uint8_t *o_strand,
                          uint8_t *o_ref, uint8_t *o_kmers);
/* Which record became which row: the selection and order of gfm_graph_hit_columns (the same code runs) for the same h_ptable,
 * parts, h_entry_of and flags -> for output row j of that table, o_part[j] = the part and o_index[j] = the index in
 * h_recs[o_part[j]] of the record it was made from (caller-allocated for sum(n_recs) rows, either may be NULL); *n_out =
 * rows.  What is kept per hit ENTRY beside the records (gfm_graph_hit_alleles) is gathered into report order with it.
 * GFM_HITS_FIRST_PER_REGION is refused (GFM_ERR_INVALID). */
int gfm_graph_hit_order(const double *h_ptable, int32_t table_len, int32_t n_parts, const gfm_graph_hit_t *const *h_recs,
                        const int64_t *n_recs, const int64_t *const *h_entry_of, uint32_t flags, int64_t *n_out,
                        int32_t *o_part, int64_t *o_index);
/* gfm_graph_hit_columns for the motifs of a SET without holding the caller -- grafimo.findmotif builds one table per motif
 * of the set (grafimo.py:177-183), and what a Python caller does with a table's columns next (strings, a DataFrame) holds
 * the interpreter: the jobs -- one per motif, the arguments of gfm_graph_hit_columns as a struct; `status` and `n_out`
 * are written by the library -- are taken by the library's kept host threads, _start returns at once, _wait returns when
 * every job is done (and frees the run): GFM_OK, or the code of the first job that failed with its message in
 * gfm_last_error(); jobs[i].status says which.  The jobs array and every buffer it points to stay untouched by the caller
 * from _start to _wait.  Every run that was started must be waited for. */
typedef struct gfm_hit_columns_job {
    const double *h_ptable;
    const gfm_graph_hit_t *const *h_recs;
    const int64_t *n_recs;
    const int64_t *const *h_entry_of;
    const int64_t *region_base;
    int64_t *o_start, *o_stop, *o_freq, *o_region;
    double *o_score, *o_pvalue, *o_qvalue;
    uint8_t *o_strand, *o_ref, *o_kmers;
    double offset;
    int64_t n_out;      /* out: rows written */
    int32_t table_len, scale, width, n_parts;
    uint32_t flags;
    int32_t status;     /* out: GFM_OK or this job's error code */
} gfm_hit_columns_job_t;
typedef struct gfm_hit_columns_run *gfm_hit_columns_run_t;
int gfm_graph_hit_columns_start(gfm_hit_columns_job_t *jobs, int32_t n_jobs, gfm_hit_columns_run_t *out);
int gfm_graph_hit_columns_wait(gfm_hit_columns_run_t run);
/* The sequence_name strings of regions, "CHROM:START-STOP" (extract_regions.py:165-170: the query string of `vg find -p`,
 * which score_seqs copies from column 1 of the rows), '\n'-terminated, one after the other in h_out.  Returns the bytes
 * written; with capacity too small (0 to ask) nothing is written and the room to come back with is returned. */
int64_t gfm_region_labels(const char *chrom, const int64_t *h_starts, const int64_t *h_stops, int64_t n, char *h_out,
                          int64_t capacity);

/* ------------------------------------------------------------------ per-variant motif effects
 * Which variants create or destroy a binding site: for every graph site s (a substitution site with 1-3 ALT bases, an
 * insertion, a deletion: the sites gfm_graph_create holds) and every allele a of it (0 = REF), the BEST k-mer among the rows
 * the fused report would give at threshold 1 whose walk takes allele a at s AND covers the allele's footprint (the walk
 * carries a haplotype constraint for s: SNV -- its base is in the window; deletion REF -- a deleted base is; deletion ALT
 * -- the junction; insertion ALT -- an inserted base; insertion REF -- the anchor and the base behind it).  Best: highest
 * score, then smallest start, smallest stop, '+' before '-', smallest k-mer as printed for its strand.
 *
 * gfm_graph_variant_effects: regions as gfm_graph_score takes them, motifs of ONE width; flags GFM_GRAPH_FORWARD_ONLY
 *   (--no-reverse) and GFM_VARIANT_KEEP_ZERO_FREQ (--recomb: walks no haplotype carries count too).  Per motif m:
 *   d_keys[m] uint64 [n_sites][4] zeroed by the caller (the packed best key of every (site, allele): pass 1);
 *   d_recs[m] gfm_variant_rec_t [rec_capacity[m]] and *d_rec_count[m] (zeroed by the caller): pass 2 appends EVERY walk
 *   and strand whose key equals its slot's best (records beyond the capacity are counted, not stored: call again with the
 *   count as capacity and fresh buffers).  *d_overflow (zeroed by the caller) = 1 if a window holds more than 2^24 walks
 *   (its walks are left out: the table is not complete).  *n_windows (host, optional) = windows enumerated: only those
 *   within reach of a site.  Enqueue only (host work: the window list; the handle's calls are serialised as
 *   gfm_graph_score's are).
 * gfm_variant_effect_columns (host, no device touched): the records of ONE motif and graph -> one row per (site, ALT
 *   allele) in site order, kept when either side's p-value < threshold (strict, as the report) or, with
 *   GFM_VARIANT_ALL_SITES, whenever either allele has a qualifying k-mer.  Per row: o_site, o_alt (1..3); per side
 *   k = 0 REF, 1 ALT at [2 * row + k]: o_found (0: no qualifying k-mer -- the other columns of that side are NaN / 0),
 *   o_score (log-odds: scaled / scale + width * offset), o_pvalue (h_ptable[scaled]), o_start, o_stop, o_strand (0 '+',
 *   1 '-'), o_kmers [W + 1] with a '\n' behind; o_effect: 0 none, 1 gain (ALT only), 2 loss (REF only), 3 both.  Rows
 *   are at most the sum of h_n_alts; *n_out = rows written. */
#define GFM_VARIANT_KEEP_ZERO_FREQ 2u
#define GFM_VARIANT_ALL_SITES 1u
typedef struct gfm_variant_rec {
    int32_t slot;       /* site * 4 + allele */
    int32_t score;      /* scaled score */
    int64_t start, stop;
    uint8_t strand, pad[7];
    uint8_t kmer[GFM_MAX_WIDTH];
} gfm_variant_rec_t;
int gfm_graph_variant_effects(gfm_graph_t g, const gfm_motif_t *motifs, int32_t n_motifs, int32_t n_regions,
                              const int64_t *h_starts, const int64_t *h_stops, uint32_t flags, uint64_t *const *d_keys,
                              void *const *d_recs, const int64_t *rec_capacity, uint64_t *const *d_rec_count,
                              int32_t *d_overflow, int64_t *n_windows, void *stream);
int gfm_variant_effect_columns(const double *h_ptable, int32_t table_len, int32_t scale, double offset, int32_t width,
                               int32_t n_sites, const uint8_t *h_n_alts, const gfm_variant_rec_t *h_recs, int64_t n_recs,
                               double threshold, uint32_t flags, int64_t *n_out, int32_t *o_site, int32_t *o_alt,
                               uint8_t *o_found, double *o_score, double *o_pvalue, int64_t *o_start, int64_t *o_stop,
                               uint8_t *o_strand, uint8_t *o_kmers, uint8_t *o_effect);

/* ------------------------------------------------------------------ per-haplotype best motif score (no threshold)
 * For region r of the caller's list and haplotype h of the graph (its bitset order): the best of the report's threshold-1
 * rows of r that h carries -- h is in the AND of the bitsets of the walk's allele constraints, the set whose size is
 * haplotype_frequency; equivalently the k-mers of h's own sequence under the report's region rule, both strands unless
 * GFM_GRAPH_FORWARD_ONLY.  No hit list is made.  Per motif m, d_keys[m] uint64 [n_regions][n_hap + 1], zeroed by the
 * caller, receives the packed key of that row; column n_hap is the reference path (every site at its REF allele, carried
 * or not).  Key = scaled score << 48 | (2^28 - 1 - (left - max(start, 0))) << 20 | (2^19 - 1 - (right - left)) << 1 | '+',
 * with left / right the '+' row's start / stop: the largest key is the highest score, then the smallest left, then the
 * smallest right, then '+' before '-'.  0: h has no row in r.  Motifs of ONE width (they share the call's run list).
 * windows_per_run (0: 256, at most 1 024) and haplotypes_per_block (0: as few blocks of at most 4 096 as fit, else a
 * multiple of 64) cut the work; the result does not depend on them.  *d_overflow (zeroed by the caller) = 1 if a window
 * holds more than 2^24 walks: the matrix is not complete.  GFM_ERR_INVALID when the graph carries no haplotypes, a region
 * (clipped to the chromosome) is longer than 2^28 - 1 bases, or a walk may span more than 2^19 - 1 bases.  Enqueue only
 * (host work: the run list; the handle's calls are serialised as gfm_graph_score's are). */
int gfm_graph_haplotype_scores(gfm_graph_t g, const gfm_motif_t *motifs, int32_t n_motifs, int32_t n_regions,
                               const int64_t *h_starts, const int64_t *h_stops, uint32_t flags, uint64_t *const *d_keys,
                               int32_t *d_overflow, int32_t windows_per_run, int32_t haplotypes_per_block, void *stream);

/* ------------------------------------------------------------------ per-haplotype total binding affinity (a sum, exact)
 * For region r and haplotype h: A(r, h) = the sum of w[score(row)] over the rows of gfm_graph_haplotype_scores' Rows(r, h)
 * -- every k-mer of h's own sequence under the report's region rule, once per strand (one strand with
 * GFM_GRAPH_FORWARD_ONLY) -- in uint64, with w = d_weights[m], uint64 [table_len of motif m] on the device, indexed by the
 * scaled score (a k-mer holding N scores the motif's min_val).  The table is taken as given, zeros allowed.  Per motif m,
 * d_sums[m] uint64 [n_regions][n_hap + 1], zeroed by the caller, receives the sums; column n_hap is the reference path.
 * Integer adds: the result is exact and depends neither on windows_per_run / haplotypes_per_block (as for
 * gfm_graph_haplotype_scores) nor on the order of the device's atomics.  max_weight: the largest entry of the tables.  A
 * cell holds at most rows_bound(r) = 2 * (the bases of region r clipped to the chromosome + ALL inserted bases of the graph)
 * rows -- a row per strand and base of the haplotype's sequence that starts in the region --, and a region with
 * rows_bound(r) * max_weight > 2^64 - 1 is refused with GFM_ERR_INVALID before anything is launched.  *d_overflow (zeroed by
 * the caller) = 1 if a window holds more than 2^24 walks: the sums are not complete.  GFM_ERR_INVALID also when the graph
 * carries no haplotypes.  Motifs of ONE width.  Enqueue only (host work: the run list; the handle's calls are serialised
 * as gfm_graph_score's are). */
int gfm_graph_haplotype_affinity(gfm_graph_t g, const gfm_motif_t *motifs, int32_t n_motifs,
                                 const uint64_t *const *d_weights, uint64_t max_weight, int32_t n_regions,
                                 const int64_t *h_starts, const int64_t *h_stops, uint32_t flags, uint64_t *const *d_sums,
                                 int32_t *d_overflow, int32_t windows_per_run, int32_t haplotypes_per_block, void *stream);

/* ------------------------------------------------------------------ per-variant affinity effects (sums, exact)
 * For every graph site s and allele a of it (0 = none of the site's ALTs), slot = s * 4 + a: sum = the sum of w[score] over
 * every k-mer of every haplotype's own sequence, once per strand (one strand with GFM_GRAPH_FORWARD_ONLY), that lies in at
 * least one region under the report's region rule and whose bases cover the footprint of (s, a) -- the footprints of
 * gfm_graph_variant_effects --, and rows = the number of those k-mers; a k-mer that several regions hold counts once.  On
 * the device every walk of every distinct window start adds carriers * (w[s+] + w[s-]) and carriers * strands to the slots
 * of its constraints, carriers = the popcount over all bitset words of the AND of the constraints' bitsets.  w =
 * d_weights[m], uint64 [table_len of motif m] on the device, indexed by the scaled score (a k-mer holding N scores the
 * motif's min_val), taken as given.  Per motif m, d_sums[m] uint64 [4 * n_sites][2] (sum, rows), zeroed by the caller.
 * Integer adds: the result is exact and depends neither on table_entries nor on the order of the device's atomics.
 * *d_overflow (zeroed by the caller): bit 0 = a window holds more than 2^24 walks (left out: the sums are not complete),
 * bit 1 = a 64-bit add wrapped (every add, in LDS and in global memory, is checked: old + v < v).  *n_windows (host,
 * optional) = the distinct window starts enumerated.  table_entries (0: 64, else a power of two up to 64): the entries of
 * a wavefront's LDS staging table; an add that finds it full goes to global memory.  GFM_ERR_INVALID when the graph carries
 * no haplotypes.  Motifs of ONE width.  Enqueue only (host work: the window list; the handle's calls are serialised as
 * gfm_graph_score's are). */
int gfm_graph_variant_affinity(gfm_graph_t g, const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                               int32_t n_regions, const int64_t *h_starts, const int64_t *h_stops, uint32_t flags,
                               uint64_t *const *d_sums, int32_t *d_overflow, int64_t *n_windows, int32_t table_entries,
                               void *stream);

/* ------------------------------------------------------------------ haplotype classes: distinct allele combinations per region
 * The sites of region [S, E) clipped to the chromosome, T(r): a substitution with S <= pos < E, an insertion with
 * S - 1 <= pos < E, a deletion of d bases with pos + 1 < E and pos + d >= S (the report's region rule: a row starts in [S, E)
 * and stops <= E); an empty region has none.  The state of a haplotype at a site is its bits in the site's n_alts used slots
 * (0: none of the ALTs); two haplotypes are in one class of r when their states agree on T(r).  Classes are numbered per
 * region by count descending, then by smallest member.  d_class int32 [n_regions][n_hap] receives the class of every
 * haplotype, d_n_classes int32 [n_regions] the number of classes.  Grouping is by a 64-bit Zobrist key (seed: any value;
 * key_bits 1 .. 64 truncates it, a lab knob) and VERIFIED: every haplotype is compared with its class's smallest member at
 * every site of T(r), and bit 0 of *d_status (cleared by the caller) is set when two allele combinations shared a key -- the
 * classes are then wrong and the call is repeated with another seed; with *d_status == 0 they are exact.  table_slots: the
 * slots of a region's LDS table, 0 (2048) or a power of two in [64, 2048]; a region of more than 3/4 of it classes is
 * redone over a table in global memory; the result does not depend on it.  scratch_bytes (0: 256 MB) bounds the keys and
 * tables: the regions go through in chunks (one region's worth is always taken); the result does not depend on it.
 * At most 2^20 haplotypes.  GFM_ERR_INVALID for a graph without haplotypes, h_stops[r] < h_starts[r] and bad knobs.  Waits
 * for the stream (the list of spilled regions is read on the host); the handle's calls are serialised as gfm_graph_score's. */
int gfm_graph_haplotype_classes(gfm_graph_t g, int32_t n_regions, const int64_t *h_starts, const int64_t *h_stops, uint64_t seed,
                                int32_t key_bits, int32_t table_slots, int32_t *d_class, int32_t *d_n_classes, int32_t *d_status,
                                int64_t scratch_bytes, void *stream);

/* Graph-independent: the records of the classes of a class matrix.  d_class int32 [n_regions][n_hap] with 0 <= class <
 * d_class_off[r + 1] - d_class_off[r] (other values are left out), d_class_off int64 [n_regions + 1] the exclusive scan of
 * the class counts, optionally d_group_bits uint64 [n_groups][ceil(n_hap / 64)], n_groups 0 .. 64.  Per class k of region r at
 * d_class_off[r] + k: d_count int32 (its haplotypes), d_first int32 (its smallest member) and d_group_counts int32 [n_groups]
 * (its haplotypes per group); the outputs are initialised here.  Enqueue only. */
int gfm_graph_haplotype_class_records(int32_t n_regions, int32_t n_hap, const int32_t *d_class, const int64_t *d_class_off,
                                      const uint64_t *d_group_bits, int32_t n_groups, int32_t *d_count, int32_t *d_first,
                                      int32_t *d_group_counts, void *stream);

/* ------------------------------------------------------------------ haplotype sequences: the bases a haplotype spells in a region
 * THE RULE.  Haplotype h of a graph spells one sequence over the chromosome by walking the reference: at a position the
 * substitution it carries replaces the base (its first carried ALT in slot order); the FIRST insertion in site order it carries at
 * that anchor is read behind the anchor, later ones at that anchor are not; if no insertion was read there, the first deletion
 * it carries at that anchor jumps over its span; every site anchored on a jumped-over base is ignored.  Every spelled base has
 * a coordinate -- its own reference position (0-based), or its anchor's if it was inserted -- and an inserted flag.  The region
 * sequence of h in [S, E) clipped to the chromosome is the contiguous stretch of spelled bases with coord + inserted >= S and
 * coord < E: exactly the bases a report row of the region can contain (start in [S, E), stop <= E).  A base inserted behind
 * S - 1 belongs, the anchor S - 1 itself does not; bases inserted behind E - 1 belong; an empty region gives an empty sequence;
 * a region wholly under a carried deletion gives an empty sequence or inserted bases only.  Haplotype -1 is the reference: no
 * ALT anywhere (it can be spelled on a graph without haplotypes).
 *
 * n_seqs (region, haplotype) pairs in device memory, d_seq_region / d_seq_hap int32 [n_seqs], over the n_regions host regions
 * h_starts / h_stops (0-based, half-open, clipped here).  Count first, then fill:
 *   d_bases NULL (measure only): d_len int32 [n_seqs] receives the number of bases of every pair, *h_total (host, optional)
 *     their sum.  The caller makes the exclusive scan d_off int64 [n_seqs + 1] of the lengths and allocates.
 *   d_bases uint8 [capacity]: the lengths are measured again (or, with GFM_SEQS_HAVE_LENGTHS, d_len is taken as an earlier
 *     call left it for the same pairs), then the bases of pair n are written at d_off[n] ..; d_coord int32 [capacity]
 *     (optional) receives per base its coordinate, ~coordinate for an inserted base; d_key uint64 [n_seqs] the content key of
 *     every sequence: the sum mod 2^64 over its bases of mix64(seed, offset << 8 | base), offset counted from the sequence's
 *     start, masked to key_bits (1 .. 64; below 64 a lab knob).  Equal sequences have equal keys; sequences of equal key are
 *     compared with gfm_sequences_verify.  capacity and d_off count bases.
 * Nothing is zeroed by the caller; every d_len and d_key entry is written.  GFM_ERR_INVALID: a haplotype >= the graph's number
 * of haplotypes or < -1, a region index outside 0 .. n_regions - 1, h_stops[r] < h_starts[r], key_bits outside 1 .. 64, a
 * graph without haplotypes when any haplotype >= 0 is asked for, a sequence of more than 2^31 - 1 bases -- the pairs are
 * checked on the device and nothing is filled.  GFM_ERR_OVERFLOW: capacity < the total (nothing is written), or d_off is not
 * the scan of the lengths inside capacity (the sequences that do not fit are left out; nothing is written out of bounds).
 * The call WAITS for the stream (it reads the verdict of the check and the total); the handle's calls are serialised as
 * gfm_graph_score's.  gfm_graph_profile_enable brackets the measure and the fill launch. */
#define GFM_SEQS_HAVE_LENGTHS 1u
int gfm_graph_haplotype_sequences(gfm_graph_t g, int32_t n_regions, const int64_t *h_starts, const int64_t *h_stops,
                                  int64_t n_seqs, const int32_t *d_seq_region, const int32_t *d_seq_hap, int32_t *d_len,
                                  const int64_t *d_off, int64_t capacity, uint8_t *d_bases, int32_t *d_coord, uint64_t seed,
                                  int32_t key_bits, uint64_t *d_key, uint32_t flags, int64_t *h_total, void *stream);

/* Graph-independent: n_seqs (< 2^31) sequences d_bases at d_off int64 [n_seqs + 1] (bases), d_same_as int32 [n_seqs] the
 * sequence that sequence n is claimed to equal byte for byte, or n itself.  Length first, then the bytes: bit 0 of *d_status
 * (cleared by the caller) is set on the first difference, or on a d_same_as outside 0 .. n_seqs - 1.  Enqueue only. */
int gfm_sequences_verify(int64_t n_seqs, const int64_t *d_off, const uint8_t *d_bases, const int32_t *d_same_as,
                         int32_t *d_status, void *stream);

/* ------------------------------------------------------------------ query variants: an edit applied to a spelled sequence
 * Graph-independent.  THE RULE.  A sequence x (gfm_graph_haplotype_sequences' d_bases) has per base a coordinate, ~coordinate
 * for an inserted base (its d_coord).  An edit is (pos0, ref of lr bases, alt of la bases): a variant with the bases REF and
 * ALT share at their start, then at their end, stripped; pos0 the 0-based position of the first remaining REF base; lr and la
 * at most GFM_QUERY_MAX_ALLELE, not both 0.
 *   lr > 0:  o = the offset in x of the non-inserted base with coordinate pos0.  GFM_EDIT_ABSENT unless every coordinate
 *     pos0 .. pos0 + lr - 1 is carried by a non-inserted base of x (the background deletes one); GFM_EDIT_APPLIED when
 *     x[o .. o + lr) are those bases in order, no inserted base between them, and equal ref compared without case; else
 *     GFM_EDIT_MISMATCH (the background carries another allele there).
 *   lr == 0 (a pure insertion between pos0 - 1 and pos0): o as above; ABSENT unless a non-inserted base carries pos0 - 1 too
 *     (pos0 == 0: always ABSENT); APPLIED when that base is x[o - 1], else MISMATCH (inserted bases lie between).  When no base
 *     carries pos0: APPLIED at o = len(x) if the LAST base of x is the non-inserted base pos0 - 1, MISMATCH at o = len(x) if it
 *     is a base inserted behind pos0 - 1, else ABSENT -- x is taken to run to the end of its chromosome then, which the caller
 *     knows and this entry does not (grafimo_amd.query_variants turns both into ABSENT when pos0 is not the chromosome's length).
 *   The edited sequence is y = x[:o] + alt + x[o + lr:].  REF side: the window starts s of x with s <= o + lr - 1 and
 *   s + W - 1 >= o (lr == 0: the windows across the junction), clipped to 0 <= s <= len(x) - W; ALT side: the same in y with la.
 *   A side may have no window.  Every window is scored once per strand (GFM_GRAPH_FORWARD_ONLY: the forward strand only); a
 *   k-mer holding a base that is not A, C, G, T scores min_val.  Per side: the best window by (score descending, s ascending,
 *   '+' before '-') and the sum over its windows and strands of w[score], exact in uint64 whatever the order of the adds.
 *
 * n_motifs motifs of ONE width on the current device, d_weights[m] uint64 [table length] per motif and max_weight, the largest
 * weight of all tables (host): refused when max_weight * 2 * (W + 64) passes 2^64 - 1.  The sequences: d_seq_offsets int64
 * [n_seqs + 1], d_bases uint8, d_coord int32.  The edits: d_pos0 int64 [n_edits], d_ref_off / d_alt_off int32 [n_edits + 1]
 * into d_ref_bytes / d_alt_bytes.  The items: d_item_seq / d_item_edit int32 [n_items].  d_records[m] receives one record per
 * item: status, o (-1: no base carries pos0) and, when APPLIED, per side the key -- 0: no window, else
 * (score + 1) << 8 | (64 - (s - o)) << 1 | (strand is '+') -- and the sum; keys and sums are 0 otherwise.  Every record is
 * written.  d_status int32: a device word of the caller's, cleared and read here.
 * n_items == 0 returns GFM_OK and touches nothing.  GFM_ERR_INVALID: a NULL pointer, motifs of different widths or on another
 * device than the current one, an unknown flag; and, CHECKED ON THE DEVICE per item (its record's status is GFM_EDIT_INVALID,
 * nothing is read through it): an item index outside its array, an edit with lr or la above 64 or both 0, sequence offsets
 * that descend.  What the offsets point INTO is the caller's contract: d_seq_offsets within d_bases / d_coord, the edit
 * offsets within their bytes.  The call WAITS for the stream (it reads the verdict of the check). */
#define GFM_QUERY_MAX_ALLELE 64
#define GFM_EDIT_APPLIED 0
#define GFM_EDIT_ABSENT 1
#define GFM_EDIT_MISMATCH 2
#define GFM_EDIT_INVALID 3
typedef struct {
    int32_t status, o;
    uint32_t ref_key, alt_key;
    uint64_t ref_sum, alt_sum;
} gfm_edit_record_t;
int gfm_graph_query_edits(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights, uint64_t max_weight,
                          int32_t n_seqs, const int64_t *d_seq_offsets, const uint8_t *d_bases, const int32_t *d_coord,
                          int32_t n_edits, const int64_t *d_pos0, const int32_t *d_ref_off, const uint8_t *d_ref_bytes,
                          const int32_t *d_alt_off, const uint8_t *d_alt_bytes, int64_t n_items, const int32_t *d_item_seq,
                          const int32_t *d_item_edit, uint32_t flags, gfm_edit_record_t *const *d_records, int32_t *d_status,
                          void *stream);

/* ------------------------------------------------------------------ mutation scan: every single-base change of a spelled sequence
 * Graph-independent.  THE RULE.  For a sequence x of n bases and a motif of width W, for every offset o in 0 .. n - 1 and every
 * base b in A, C, G, T:
 *   y = x with y[o] = b.
 *   REF side: the window starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).
 *   ALT side: the same starts in y.
 *   Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
 *   A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
 *   Per side: the best window by (score descending, s ascending, + before -), as the key
 *   ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus -- gfm_graph_query_edits' encoding, with s - o in -(W - 1) .. 0; key 0 means
 *   the side has no window (n < W) --, and the exact uint64 sum of w[score] over the side's windows and strands.
 *   b equal to the folded x[o] gives ALT equal to REF.
 *   An x[o] that is no base has an all-min_val REF side, and each b can repair it.
 * By construction the result for b != x[o] is field for field what gfm_graph_query_edits returns for the edit
 * (coordinate of o, x[o], b) applied to x, wherever a coordinate names o.
 *
 * n_motifs motifs of ONE width on the current device, d_weights[m] uint64 [table length] per motif and max_weight, the largest
 * weight of all tables (host): refused when max_weight * 2 * W passes 2^64 - 1.  seq_offsets: HOST, int64 [n_seqs + 1], ascending
 * from seq_offsets[0] >= 0: the bases of sequence v are d_bases[seq_offsets[v] .. seq_offsets[v + 1]); empty sequences are
 * allowed.  d_keys[m] uint32 [seq_offsets[n_seqs]][5] and d_sums[m] uint64 [seq_offsets[n_seqs]][5]: per base of d_bases the
 * columns REF, A, C, G, T.  Every row of a sequence is written, nothing is zeroed by the caller.  d_status int32: a device
 * word of the caller's, cleared and read here.
 * The work is cut into (sequence, GFM_MUTSCAN_TILE offsets) tiles by the library; the result does not depend on the tile and
 * a caller never needs it -- it is exported so that tests can aim at its edges.
 * No sequence or no base returns GFM_OK and touches nothing.  GFM_ERR_INVALID: a NULL pointer, motifs of different widths or
 * on another device than the current one, a width outside [1, 64], weights that can overflow a sum, offsets that descend, a
 * sequence of 2^31 bases or more, an unknown flag.  The call WAITS for the stream (it reads the verdict of the device's
 * check of the tile table). */
#define GFM_MUTSCAN_TILE 64
int gfm_sequence_mutation_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights, uint64_t max_weight,
                               int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases, uint32_t flags,
                               uint32_t *const *d_keys, uint64_t *const *d_sums, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------ indel scan: every one-base deletion and insertion of a spelled sequence
 * Graph-independent.  THE RULE.  For a sequence x of n bases, a motif of width W, and every offset o in 0 .. n - 1:
 *   Deletion of x[o].  y = x[:o] + x[o+1:].  This is gfm_graph_query_edits' rule with lr = 1, la = 0 at offset o.
 *     REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).  This is exactly the mutation
 *     scan's REF column.
 *     ALT side (column DEL): the starts of y across the junction, max(0, o - W + 1) <= s <= min(o - 1, n - 1 - W).
 *   Insertion of b in A, C, G, T behind x[o].  y = x[:o+1] + b + x[o+1:].  This is the query rule with lr = 0, la = 1 at offset
 *   o' = o + 1.
 *     REF side (column JUNCTION): the starts of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).
 *     ALT side (columns INS_A, INS_C, INS_G, INS_T): the starts of y with max(0, o' - W + 1) <= s <= min(o', n + 1 - W).
 *   Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
 *   A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
 *   Per column, the best window by (score descending, s ascending, + before -), as the key
 *   ((score + 1) << 8) | ((64 - rel) << 1) | plus, rel = s - o for COVER and DEL, rel = s - (o + 1) for JUNCTION and INS_*: the
 *   values a gfm_edit_record_t of the same edit holds.  Key 0 means the side has no window.
 *   Per column, the exact uint64 sum of w[score] over the side's windows and strands.
 *   A deleted N can repair its windows.  An N elsewhere leaves its windows at min_val.  An insertion before the first base of a
 *   sequence is not scanned: every row has the base it is anchored to, as a VCF row has.  An empty sequence has no rows.
 * By construction the columns equal, field for field, what gfm_graph_query_edits returns for the deletion (coordinate of o,
 * x[o], "") and the insertion (coordinate of o + 1, "", b) applied to x, wherever a coordinate can name the edit.
 *
 * The arguments, the refusals and the wait are gfm_sequence_mutation_scan's: motifs of ONE width, d_weights and max_weight
 * (refused when max_weight * 2 * W passes 2^64 - 1: a side has at most W windows), seq_offsets on the HOST, ascending from
 * seq_offsets[0] >= 0, no sequence of 2^31 bases or more.  d_keys[m] uint32 [seq_offsets[n_seqs]][7] and d_sums[m] uint64
 * [seq_offsets[n_seqs]][7]: per base of d_bases the columns COVER, DEL, JUNCTION, INS_A, INS_C, INS_G, INS_T.  Every row of a
 * sequence is written, nothing is zeroed by the caller.  The work is cut into (sequence, GFM_INDELSCAN_TILE offsets) tiles by
 * the library; the result does not depend on the tile -- it is exported only so that tests can aim at its edges.  No sequence
 * or no base returns GFM_OK and touches nothing.  The call WAITS for the stream. */
#define GFM_INDELSCAN_TILE 64
int gfm_sequence_indel_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights, uint64_t max_weight,
                            int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases, uint32_t flags,
                            uint32_t *const *d_keys, uint64_t *const *d_sums, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------ deletion scan: every block deletion of 1 .. 64 bases of a spelled sequence
 * Graph-independent.  THE RULE.  For a sequence x of n bases, a motif of width W, a strictly ascending list of lengths
 * L0 < L1 < .. with every L in 1 .. GFM_DELSCAN_MAX_LENGTH, every length L of the list and every offset o in 0 .. n - 1:
 *   If o + L > n there is no edit: both keys and both sums of the cell are 0.
 *   Otherwise y = x[:o] + x[o+L:].  This is gfm_graph_query_edits' rule with lr = L, la = 0 at offset o.
 *     REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o + L - 1, n - W).
 *     ALT side (column DEL): the starts of y across the junction, max(0, o - W + 1) <= s <= min(o - 1, n - L - W).
 *   Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
 *   A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
 *   A deleted N can repair its junction windows.  An N elsewhere cannot be repaired.
 *   Per column, the best window by (score descending, s ascending, + before -), as the key
 *   ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. L - 1 for COVER and in -(W - 1) .. -1 for DEL: the
 *   values a gfm_edit_record_t of the same edit holds.  Key 0 means the side has no window.
 *   Per column, the exact uint64 sum of w[score] over the side's windows and strands.
 *   At L = 1 the two columns equal gfm_sequence_indel_scan's COVER and DEL bit for bit.
 * By construction a cell equals, field for field, what gfm_graph_query_edits returns for the deletion (coordinate of o,
 * x[o .. o + L - 1], "") applied to x, wherever coordinates can name the block (GFM_QUERY_MAX_ALLELE is 64 as well, and the
 * key's 7-bit field holds every s - o that occurs).
 *
 * The arguments are gfm_sequence_indel_scan's and n_lengths >= 1 with lengths, int32 [n_lengths] on the HOST.  Refused when
 * max_weight * 2 * (W + Lmax - 1) passes 2^64 - 1, Lmax the longest length: a REF side has at most W + Lmax - 1 windows.
 * d_keys[m] uint32 [n_lengths][seq_offsets[n_seqs]][2], 8-byte aligned, and d_sums[m] uint64 of the same shape, 16-byte
 * aligned: per length and base of d_bases the columns COVER, DEL.  Every cell is written, nothing is zeroed by the caller.
 * The work is cut into (sequence, GFM_DELSCAN_TILE offsets) tiles by the library; the result does not depend on the tile -- it
 * is exported only so that tests can aim at its edges.  No sequence or no base returns GFM_OK and touches nothing.
 * GFM_ERR_INVALID, all before anything is launched: a NULL pointer, lengths that do not strictly ascend or lie outside
 * 1 .. GFM_DELSCAN_MAX_LENGTH, motifs of different widths or on another device than the current one, weights that can overflow
 * a sum, offsets that descend, a sequence of 2^31 bases or more, a misaligned result, an unknown flag.  The call WAITS for the
 * stream (it reads the verdict of the device's check of the tile table). */
#define GFM_DELSCAN_TILE 64
#define GFM_DELSCAN_MAX_LENGTH 64
int gfm_sequence_deletion_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights, uint64_t max_weight,
                               int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases, int32_t n_lengths,
                               const int32_t *lengths, uint32_t flags, uint32_t *const *d_keys, uint64_t *const *d_sums,
                               int32_t *d_status, void *stream);

/* ------------------------------------------------------------------ substitution scan: every block of 1 .. 64 bases replaced in place by a base map
 * Graph-independent.  THE RULE.  For a sequence x of n bases, a motif of width W, a strictly ascending list of lengths
 * L0 < L1 < .. with every L in 1 .. GFM_SUBSCAN_MAX_LENGTH, a base map f given as four codes -- the images of A, C, G, T, each
 * in 0 .. 3 for A, C, G, T; any map is allowed: fixed points, constant maps and the identity included --, every length L of
 * the list and every offset o in 0 .. n - 1:
 *   If o + L > n there is no edit: both keys and both sums of the cell are 0.
 *   Otherwise y = x[:o] + f(x[o:o+L]) + x[o+L:].  f is applied base by base.  Case is folded, as base_code does.
 *   A base that is not A/C/G/T maps to itself: unlike a deletion, a substituted N is NOT repaired.
 *   This is gfm_graph_query_edits' rule with lr = la = L at offset o, the alleles not trimmed.
 *     REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o + L - 1, n - W).  This is bit for bit the
 *     deletion scan's COVER column.
 *     ALT side (column SUB): the same starts in y.
 *   Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
 *   A window that holds a base that is not A/C/G/T scores min_val on both strands.
 *   Per column, the best window by (score descending, s ascending, + before -), as the key
 *   ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. L - 1 on both sides: the values a
 *   gfm_edit_record_t of the same edit holds.
 *   Key 0 means the side has no window.
 *   Per column, the exact uint64 sum of w[score] over the side's windows and strands.
 *   Under the identity map SUB == COVER in every cell.
 *   At L = 1, wherever x[o] is a base, SUB equals the mutation scan's column of the base f(x[o]), field for field.
 * By construction a cell equals, field for field, what gfm_graph_query_edits returns for the edit (coordinate of o,
 * x[o .. o + L - 1], f(x[o .. o + L - 1])) applied to x, wherever coordinates can name the block.
 *
 * The arguments, result shapes, alignment rules, refusals and the wait are gfm_sequence_deletion_scan's, with base_map, uint8
 * [4] on the HOST, behind the lengths: base_map[i] is the image of "ACGT"[i] as an index into "ACGT".  d_keys[m] uint32
 * [n_lengths][seq_offsets[n_seqs]][2], 8-byte aligned, and d_sums[m] uint64 of the same shape, 16-byte aligned: per length and
 * base of d_bases the columns COVER, SUB.  Every cell is written, nothing is zeroed by the caller.  Refused when max_weight * 2 *
 * (W + Lmax - 1) passes 2^64 - 1: either side has at most W + Lmax - 1 windows.  GFM_ERR_INVALID, all before anything is
 * launched: what gfm_sequence_deletion_scan refuses, a NULL base_map, a code above 3.  The call WAITS for the stream. */
#define GFM_SUBSCAN_TILE 64
#define GFM_SUBSCAN_MAX_LENGTH 64
int gfm_sequence_substitution_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                   uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                                   int32_t n_lengths, const int32_t *lengths, const uint8_t base_map[4], uint32_t flags,
                                   uint32_t *const *d_keys, uint64_t *const *d_sums, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------ insertion scan: given inserts of 1 .. 64 bases behind every base of a spelled sequence
 * Graph-independent.  THE RULE.  For a sequence x of n bases, a motif of width W, a list of K inserts with K in 1 .. 16, every
 * insert I of the list, Li its length in 1 .. 64, and every offset o in 0 .. n - 1:
 *   Every insert holds A, C, G, T only.  Case is folded, as base_code does.
 *   The edit is the insertion of I behind x[o].  Let o' = o + 1 and y = x[:o'] + I + x[o':].
 *   This is gfm_graph_query_edits' rule with lr = 0, la = Li at offset o'.
 *     REF side (column JUNCTION): the starts s of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).
 *     It does not depend on the insert.  It equals the indel scan's JUNCTION column bit for bit.
 *     ALT side (column INS): the starts s of y with max(0, o' - W + 1) <= s <= min(o' + Li - 1, n + Li - W).
 *     A window that lies wholly inside the insert counts, as the query rule counts it.
 *   Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
 *   A window that holds a base of x that is not A/C/G/T scores min_val on both strands.
 *   An insertion repairs nothing, because it removes no base.  A window that does not reach the N is clean.
 *   Per column, the best window by (score descending, s ascending, + before -), as the key
 *   ((score + 1) << 8) | ((64 - (s - o')) << 1) | plus, s - o' in -(W - 1) .. -1 for JUNCTION and in -(W - 1) .. Li - 1 for INS.
 *   Key 0 means the side has no window.
 *   Per column, the exact uint64 sum of w[score] over the side's windows and strands.
 *   An insertion before the first base of a sequence is not scanned, as in the indel scan.  An empty sequence has no rows.
 *   With the inserts ("A", "C", "G", "T") the INS columns equal the indel scan's INS_A .. INS_T bit for bit.
 *   A cell does not depend on the other inserts of the list or on their order.
 * By construction a cell equals, field for field, what gfm_graph_query_edits returns for the insertion (coordinate of o + 1,
 * "", I) applied to x, wherever coordinates can name the gap (GFM_QUERY_MAX_ALLELE is 64 as well, and the key's 7-bit field
 * holds every s - o' that occurs).
 *
 * The arguments are gfm_sequence_indel_scan's and the inserts: n_inserts in 1 .. GFM_INSSCAN_MAX_INSERTS, insert_offsets int32
 * [n_inserts + 1] on the HOST, starting at 0 and ascending, and insert_bases uint8 [insert_offsets[n_inserts]] on the HOST:
 * insert i is insert_bases[insert_offsets[i] .. insert_offsets[i + 1]), 1 .. GFM_INSSCAN_MAX_LENGTH letters of ACGTacgt.
 * Exactly those counts are read.  The library does not compare the inserts with each other.  Refused when max_weight * 2 *
 * (W + Lmax - 1) passes 2^64 - 1, Lmax the longest insert: an ALT side has at most W + Lmax - 1 windows.  d_keys[m] uint32
 * [n_inserts][seq_offsets[n_seqs]][2], 8-byte aligned, and d_sums[m] uint64 of the same shape, 16-byte aligned: per insert and
 * base of d_bases the columns JUNCTION, INS (JUNCTION is the same for every insert).  Every cell is written, nothing is zeroed
 * by the caller.  The work is cut into (sequence, GFM_INSSCAN_TILE offsets) tiles by the library; the result does not depend
 * on the tile -- it is exported only so that tests can aim at its edges.  No sequence or no base returns GFM_OK and touches
 * nothing.  GFM_ERR_INVALID, all before anything is launched, in this order: n_motifs < 1, n_seqs < 0 or n_inserts outside
 * 1 .. GFM_INSSCAN_MAX_INSERTS; an unknown flag; NULL insert_offsets or insert_bases, insert_offsets that do not start at 0 or
 * that descend; a length outside 1 .. GFM_INSSCAN_MAX_LENGTH; a letter outside ACGTacgt -- these with no sequence too --; then
 * offsets that descend, a sequence of 2^31 bases or more, a NULL pointer, a misaligned result, motifs of different widths or on
 * another device than the current one, weights that can overflow a sum.  The call WAITS for the stream (it reads the verdict
 * of the device's check of the tile table). */
#define GFM_INSSCAN_TILE 64
#define GFM_INSSCAN_MAX_LENGTH 64
#define GFM_INSSCAN_MAX_INSERTS 16
int gfm_sequence_insertion_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights, uint64_t max_weight,
                                int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases, int32_t n_inserts,
                                const int32_t *insert_offsets, const uint8_t *insert_bases, uint32_t flags,
                                uint32_t *const *d_keys, uint64_t *const *d_sums, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------ site distance: substitutions from a site, for every window of a spelled sequence
 * Graph-independent.  THE RULE.
 * Inputs: a sequence x of n bases; a motif of width W with its integer matrix as the packed table holds it, entry t[j][b] for
 * the window's forward column j and base b, one table per strand; a cutoff c in 0 .. 1000 W + 1; a cap E in 1 .. 8.
 * Every window start s in 0 .. n - W and every strand is handled independently.
 * Under GFM_GRAPH_FORWARD_ONLY only the + strand is handled.  Case is folded, as base_code does.
 * A window that holds a column with no A/C/G/T scores min_val on both strands.  Otherwise its score is the sum of its entries.
 * A window's unedited score on a strand is its `own` score.  The window is a site on that strand when own >= c.
 * Raising (the near side).  Start from the window as spelled and repeat these steps:
 *   1. If the current score >= c, stop with d = picks made.
 *   2. If E picks are made, stop with d = E + 1.
 *   3. If a non-base column remains, the next pick is the leftmost such column.  It gets the column's best base: the largest
 *      entry on this strand.  Ties go to the first of A, C, G, T.  While any non-base column remains, the score stays min_val.
 *   4. Otherwise the next pick is the unpicked base column with the largest gain.  The gain is the column's largest entry minus
 *      its present entry.  Ties go to the leftmost column.  The column gets that best base.  Ties go to the first of A, C, G, T.
 *   5. If every remaining gain is 0, stop with d = E + 1.
 * Lowering (the fragile side).
 *   1. If own < c, d = 0 and there are no picks.
 *   2. A window with a non-base column takes no picks: d = 0 if min_val < c, otherwise d = E + 1.
 *   3. Otherwise pick as above, with the loss in place of the gain.  The loss is the present entry minus the column's smallest
 *      entry.  The worst base is the smallest entry.  Ties go to the first of A, C, G, T.  Stop when the score < c, with d = picks
 *      made.  Stop at E picks, or when every remaining loss is 0, with d = E + 1.
 * Results per (window start, strand, side): d in 0 .. E + 1; the score after the picks made; the 64-bit mask of the picked
 * forward columns, bit j for column j.  d and the score do not depend on the tie rules.  Only the mask does.
 * By the exchange argument d is the true minimum whenever it is <= E.
 * Columns are always forward offsets in the window.  Bases are forward-strand bases.  The - strand reads its own half of the
 * packed table at the same forward column.
 *
 * n_motifs motifs of ONE width on the current device.  seq_offsets: HOST, int64 [n_seqs + 1], ascending from seq_offsets[0] >= 0:
 * the bases of sequence v are d_bases[seq_offsets[v] .. seq_offsets[v + 1]); empty sequences are allowed.  cutoffs: HOST, int32
 * [n_motifs], the cutoff c of every motif.  max_edits: the cap E in 1 .. GFM_SITEDIST_MAX_EDITS.  Per motif and per base n of
 * d_bases, read as a window start:
 *   d_words[m] uint32 [seq_offsets[n_seqs]][6] = own +, own -, near +, near -, fragile +, fragile -.  An own word is the score.
 *   A near or fragile word is (score_after << 4) | d.  0xFFFFFFFF in any column means "no window": a start beyond n - W, or the
 *   - columns under GFM_GRAPH_FORWARD_ONLY.
 *   d_masks[m] uint64 [seq_offsets[n_seqs]][4], 8-byte aligned = near +, near -, fragile +, fragile -: 0 where there is no window.
 * Every row of both arrays is written, nothing is zeroed by the caller.  d_status int32: a device word of the caller's, cleared
 * and read here.  The work is cut into (sequence, GFM_SITEDIST_TILE window starts) tiles by the library; the result does not
 * depend on the tile -- it is exported only so that tests can aim at its edges.  No sequence or no base returns GFM_OK and
 * touches nothing, after the checks.  GFM_ERR_INVALID, all before anything is launched and also when there is no sequence:
 * n_motifs < 1, n_seqs < 0, an unknown flag, max_edits outside 1 .. GFM_SITEDIST_MAX_EDITS, NULL cutoffs, a cutoff that no width
 * allows, offsets that descend, a sequence of 2^31 bases or more; with bases, a NULL pointer or a misaligned d_masks[m];
 * wherever motifs are given, motifs of different widths or on another device than the current one, a width outside [1, 64], a
 * cutoff outside 0 .. 1000 W + 1.  The call WAITS for the stream (it reads the verdict of the device's check of the tile
 * table). */
#define GFM_SITEDIST_TILE 64
#define GFM_SITEDIST_MAX_EDITS 8
int gfm_sequence_site_distance(const gfm_motif_t *motifs, int32_t n_motifs, int32_t n_seqs, const int64_t *seq_offsets,
                               const uint8_t *d_bases, const int32_t *cutoffs, int32_t max_edits, uint32_t flags,
                               uint32_t *const *d_words, uint64_t *const *d_masks, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------ scan fold: a motif set's gains, losses and champions per cell
 * The fold over the motif axis of what any keys/sums scan entry leaves: the dense per-motif arrays stay on the device, and a
 * running state per (row, pair of columns) keeps counts and champions of the whole motif set.  THE RULE.
 * Inputs of one call: n_motifs >= 1 motifs; motif m has a caller-given id motif_ids[m] >= 0, distinct within the call, a score
 * cutoff cutoffs[m] in 0 .. table_lens[m], a device tail table d_ptables[m] float64 [table_lens[m]], and d_keys[m] uint32
 * [n_rows][n_columns] and d_sums[m] uint64 [n_rows][n_columns] as a scan entry leaves them; n_pairs in 1 .. 8 pairs
 * (ref_column, alt_column) on the HOST, int32 [n_pairs][2], columns in 0 .. n_columns - 1, ref != alt, n_columns in 2 .. 8.
 * For every (row, pair) and every motif, with r, a the two keys' scores (key >> 8) - 1 (-1 for key 0) and R, A the two sums:
 *   A side is a site when its key is not 0 and its score >= cutoff: what gfm_motif_pvalue_cutoff means.
 *   gain when a is a site and r is not.  loss when r is a site and a is not.
 *   counts[gain] and counts[loss] count the motifs.
 *   Gain champion: the gaining motif with the smallest ptable[a].  Loss champion: the losing motif with the smallest ptable[r].
 *   Ties go to the smaller motif id.  Doubles are compared as doubles; nothing is recomputed.
 *   The state keeps the champion's id, its two keys and that p.
 *   A score >= table_len reads entry table_len - 1: nothing is read outside a table.
 *   Up champion: among motifs with A > R, the one with the largest A / R, compared exactly.  Motif 1 beats motif 2 when
 *   A1 * R2 > A2 * R1 in 128-bit unsigned arithmetic.  This holds for R = 0 too: an infinite ratio beats a finite one, and
 *   two infinite ones tie.  Ties go to the smaller id.
 *   Down champion: among A < R, the largest R / A by the same rule.  The state keeps the id and both sums.
 *   The state is a running one: folding motif sets S1 then S2 into the same state gives what folding their union in one call
 *   gives, in any order and any split.
 *   The empty state is all zero bytes.  Ids are stored as id + 1, and the caller zeroes the arrays once.
 *   Folding the same id twice into a state is the caller's error and is not detected.
 * The state, a struct of arrays, per (row, pair) 88 bytes, P = n_pairs:
 *   d_counts      uint32  [n_rows][P][2]       gain, loss
 *   d_site_motif  uint32  [n_rows][P][2]       gain, loss: id + 1, 0: none
 *   d_site_keys   uint32  [n_rows][P][2][2]    (ref key, alt key) of the gain and of the loss champion
 *   d_site_p      float64 [n_rows][P][2]
 *   d_aff_motif   uint32  [n_rows][P][2]       up, down: id + 1, 0: none
 *   d_aff_sums    uint64  [n_rows][P][2][2]    (ref sum, alt sum) of the up and of the down champion
 * The intended pairs: the mutation scan's (0,1) (0,2) (0,3) (0,4) over 5 columns; the indel scan's (0,1) (2,3) (2,4) (2,5)
 * (2,6) over 7; the block scans' (0,1) over their (COVER, ALT) cells with n_rows = n_lengths * n_bases.
 * GFM_ERR_INVALID, all before any device work: n_motifs < 1, n_rows outside 0 .. 2^40, n_columns outside 2 .. 8, n_pairs outside
 * 1 .. 8; then, with rows, a NULL pointer, a pair outside its columns or with ref == alt, a negative or repeated id (or the id
 * 2^31 - 1, which id + 1 cannot hold), table_len < 1, a cutoff outside 0 .. table_len, d_sums[m], d_ptables[m], d_site_p or
 * d_aff_sums that are not 8-byte aligned.  n_rows == 0 returns GFM_OK and touches nothing.
 * The kernels (one per 16 motifs) are enqueued on `stream`, behind whatever wrote the keys and sums there.  Unlike the scan
 * entries the call does NOT wait for the stream: it has no verdict to read.  The host arrays are read before it returns. */
int gfm_scan_fold(int32_t n_motifs, const int32_t *motif_ids, const int32_t *cutoffs, const double *const *d_ptables,
                  const int32_t *table_lens, int64_t n_rows, int32_t n_columns, int32_t n_pairs, const int32_t *pairs,
                  const uint32_t *const *d_keys, const uint64_t *const *d_sums, uint32_t *d_counts, uint32_t *d_site_motif,
                  uint32_t *d_site_keys, double *d_site_p, uint32_t *d_aff_motif, uint64_t *d_aff_sums, void *stream);

/* ------------------------------------------------------------------ shuffle null: empirical p-values for best score and total affinity
 * Graph-independent.  THE RULE.  All arithmetic on 64-bit words is modulo 2^64.
 *   G = 0x9E3779B97F4A7C15.
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
 * For a sequence x of n bases with the caller's uint64 key k, a uint64 seed and the replicates r = 0 .. K - 1:
 *   s0 = mix(mix(seed + k G) + r).
 *   y starts as a copy of x: the bytes as they are, non-ACGT and lower case included.
 *   For i = n - 1 down to 1:  u = mix(s0 + i G);  j = ((u >> 32) (i + 1)) >> 32;  swap y[i] and y[j].
 *   The multiply-shift bias is at most n / 2^32 and is part of the rule.  The permutation depends on (seed, k, r, n) only, not
 *   on the motif or on anything else in the call.
 * Scores, for a motif of width W:
 *   Every window start 0 .. n - W of a sequence is scored once per strand, + only under GFM_GRAPH_FORWARD_ONLY.
 *   A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
 *   best = the largest score over windows and strands, -1 when n < W.
 *   sum = the exact uint64 sum of w[score] over windows and strands, 0 when there are none.
 *   obs_best, obs_sum: those of x itself.
 * Per (motif, sequence): obs_best int32, obs_sum uint64, ge_best = #{r : best_r >= obs_best} and ge_sum = #{r : sum_r >= obs_sum},
 * uint32.  Ties count, the conservative choice; n < W gives ge_best = ge_sum = K.
 * Per (motif, replicate), when asked for: rep_hits[r] = the sum over the sequences v of seq_weight[v] [best_{v,r} >= cut[m]],
 * uint64; cut[m] is a scaled score in [0, L] (L: no replicate reaches it).
 * Per (motif, sequence, replicate), when asked for: the dense rep_best int32 [n_seqs][K] and rep_sum uint64 [n_seqs][K].
 * The result for one sequence depends on (seed, its key, its bytes, K, the motif, the weights, the flag) only: not on its
 * neighbours in the call, nor on how the library cuts the work.
 *
 * n_motifs motifs of ONE width on the current device, d_weights[m] uint64 [table length] per motif and max_weight, the largest
 * weight of all tables (host): refused when max_weight * 2 * (longest n - W + 1) passes 2^64 - 1.  seq_offsets: HOST, int64
 * [n_seqs + 1], ascending from seq_offsets[0] >= 0; empty sequences are allowed and have results like any other.  d_seq_keys
 * uint64 [n_seqs]; d_seq_weight uint32 [n_seqs], NULL: every weight is 1.  n_replicates = K in [1, 2^20].  cuts: HOST, int32
 * [n_motifs].  The arrays of pointers d_obs_best .. d_rep_sum hold a device pointer per motif: d_obs_best[m] int32 [n_seqs],
 * d_obs_sum[m] uint64 [n_seqs], d_ge_best[m] and d_ge_sum[m] uint32 [n_seqs]; d_rep_hits[m] uint64 [K], d_rep_best[m] int32
 * [n_seqs][K], d_rep_sum[m] uint64 [n_seqs][K], each of which may be NULL and is then not computed.  Every output that is given
 * is overwritten, nothing is zeroed by the caller.  d_status int32: a device word of the caller's, cleared and read here.
 * A sequence of up to GFM_NULL_LDS_BASES bases is shuffled in the LDS, a longer one in device memory the call allocates on the
 * stream (64 bytes a base and workgroup: a sequence it cannot allocate for gives GFM_ERR_HIP); the result does not depend on
 * which -- the constant is exported only so that tests can aim at its edge.
 * No sequence returns GFM_OK and touches nothing.  GFM_ERR_INVALID: a NULL pointer, motifs of different widths or on another
 * device than the current one, a width outside [1, 64], n_replicates outside [1, 2^20], a cut outside [0, L], weights that can
 * overflow a sum, offsets that descend, a sequence of 2^31 bases or more, an unknown flag.  The call WAITS for the stream (it
 * reads the verdict of the device's check of its sequence table). */
#define GFM_NULL_LDS_BASES 960
int gfm_sequence_shuffle_null(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights, uint64_t max_weight,
                              int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases, const uint64_t *d_seq_keys,
                              const uint32_t *d_seq_weight, int32_t n_replicates, uint64_t seed, const int32_t *cuts,
                              uint32_t flags, int32_t *const *d_obs_best, uint64_t *const *d_obs_sum, uint32_t *const *d_ge_best,
                              uint32_t *const *d_ge_sum, uint64_t *const *d_rep_hits, int32_t *const *d_rep_best,
                              uint64_t *const *d_rep_sum, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------ shuffle null of order 2: doublet-preserving replicates
 * gfm_sequence_shuffle_null with two more arguments: order 1 is THE RULE above, bit for bit (walk_cap is then not used);
 * order 2 makes the replicates by THE RULE OF ORDER 2.  mix, G, the key k, the seed and the replicates r are the order-1
 * rule's; all arithmetic on 64-bit words is modulo 2^64.
 *   draw(t, m) = ((mix(s0 + t G) >> 32) m) >> 32, with m < 2^31.
 *   Alphabet.  c[i] = base_code(x[i]): 0 .. 3 for A/C/G/T with case folded, 4 for anything else.  A replicate is a sequence of
 *   codes.  Scores are taken on codes, as now.
 *   Stream.  s0 = mix(mix(seed + k G) + r + 2^63).  The 2^63 separates the order-2 stream from the order-1 stream of the same
 *   (seed, key, replicate).
 *   Buckets.  cnt[a] = #{i < n - 1 : c[i] = a}; b[a] is the exclusive prefix sum over a = 0 .. 4.  E has length n - 1 and is
 *   the stable counting sort of the successors: for i = 0 .. n - 2 in order, c[i + 1] is appended to bucket c[i].  E is the
 *   same for all replicates of a sequence; the last entry of a bucket is x's own last exit from that symbol.
 *   Arborescence.  Wilson's algorithm, rooted at root = c[n - 1].  in_tree = {root}, a step counter t = 0, cap = walk_cap n.
 *   For u = 0 .. 4 in order, if cnt[u] > 0 and u is not in the tree: cur = u; while cur is not in the tree: if t == cap the
 *   replicate is capped and the stage stops; else e = b[cur] + draw(n + t, cnt[cur]), t += 1, last[cur] = e, cur = E[e].  Then
 *   retrace from u along E[last[.]], adding vertices to the tree.
 *   A capped replicate takes last[a] = b[a + 1] - 1 for every a: x's own last exits, which always form an arborescence.
 *   Per-bucket shuffle.  For a = 0 .. 4 with cnt[a] > 0: m = cnt[a]; if a != root, swap E[last[a]] with E[b[a + 1] - 1] and
 *   m -= 1; for i = m - 1 down to 1: p = b[a] + i, j = draw(p, i + 1), swap E[p] and E[b[a] + j].  The Fisher-Yates counters
 *   p <= n - 2 and the walk's counters >= n never meet.
 *   Euler walk.  y[0] = c[0], ptr[a] = b[a]; for i = 1 .. n - 1: y[i] = E[ptr[y[i - 1]]], then ptr[y[i - 1]] += 1.  For n <= 1,
 *   y = c.
 *   Everything else is as order 1: the windows, the strands, min_val for a window with code 4, best, sum, obs_*, ge_* with ties
 *   counting, rep_hits, rep_best, rep_sum, and n < W.
 * Every replicate has x's length, first and last code and all 25 doublet counts of x; uncapped replicates are uniform over such
 * sequences (Altschul and Erickson, with Wilson's arborescence) up to the multiply-shift bias.  The cap bounds the walk by
 * construction: t and cap are 64-bit, walk_cap lies in [0, GFM_NULL_MAX_WALK_CAP], 64 is far from typical use (a random
 * 300-base sequence walks about 6 steps, (AC)^150 G about 300), 0 caps every replicate.
 * The image, GFM_NULL_LDS_BASES and the memory path are order 1's (the E codes share the image's bytes).  GFM_ERR_INVALID
 * besides gfm_sequence_shuffle_null's: an order that is neither 1 nor 2, a walk_cap outside the range; the message names the
 * value. */
#define GFM_NULL_MAX_WALK_CAP 1024
int gfm_sequence_shuffle_null_order(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                    uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                                    const uint64_t *d_seq_keys, const uint32_t *d_seq_weight, int32_t n_replicates, uint64_t seed,
                                    int32_t order, int32_t walk_cap, const int32_t *cuts, uint32_t flags,
                                    int32_t *const *d_obs_best, uint64_t *const *d_obs_sum, uint32_t *const *d_ge_best,
                                    uint32_t *const *d_ge_sum, uint64_t *const *d_rep_hits, int32_t *const *d_rep_best,
                                    uint64_t *const *d_rep_sum, int32_t *d_status, void *stream);

/* ------------------------------------------------------------------ hit pairs: rows close to each other that share carriers
 * Graph-independent (csrc/hit_pairs.hip).  n rows (n < 2^31 - 1) in device memory, in ascending (d_group, d_lo) order:
 * d_group int32, d_lo <= d_hi int64 (|x| < 2^61), d_masks uint64 [n][hw] (hw >= 1 words of a bitset whose unused tail
 * bits are CLEAR: the library does not mask them), optionally d_group_bits uint64 [n_groups][hw], n_groups 0 .. 64.
 * A pair is two rows a < b of one group with min_gap <= gap <= max_gap, gap = max(lo_a, lo_b) - min(hi_a, hi_b) (negative:
 * they overlap by that much), and joint = popcount(mask_a & mask_b) > 0.  The result is a CSR over the first row of a pair:
 *   d_pair_off int64 [n + 1]: the pairs of row a are d_pair_off[a] .. d_pair_off[a + 1] - 1; *h_total = d_pair_off[n];
 *   d_pair_b int32 [pair_capacity]: the partner b > a, ascending within a row;  d_joint int32: joint;
 *   d_group_counts int32 [pair_capacity][n_groups]: popcount(mask_a & mask_b & group_g).
 * Count first, then allocate: the pair arrays are written only when pair_capacity >= *h_total (else they are untouched and
 * may be NULL with pair_capacity 0); the caller reads *h_total and comes back with room.  GFM_PAIRS_HAVE_OFFSETS: d_pair_off
 * already holds the offsets an earlier call made for the same rows and gap, the counting pass is not run again.
 * The order is CHECKED on the device: rows not ascending in (group, lo), lo > hi or a coordinate beyond the limit give
 * GFM_ERR_INVALID and no pair.  Rows of equal (group, lo) may come in any order; that order decides which of two rows is
 * `a`.  The call WAITS for the stream (it reads the verdict of the check and the total). */
#define GFM_PAIRS_HAVE_OFFSETS 1u
int gfm_hit_pairs(const int32_t *d_group, const int64_t *d_lo, const int64_t *d_hi, const uint64_t *d_masks, int64_t n,
                  int32_t hw, int64_t min_gap, int64_t max_gap, int32_t n_groups, const uint64_t *d_group_bits,
                  int64_t *d_pair_off, int64_t pair_capacity, int32_t *d_pair_b, int32_t *d_joint, int32_t *d_group_counts,
                  uint32_t flags, int64_t *h_total, void *stream);

/* ------------------------------------------------------------------ hit linkage: alleles in LD with a row's carriers
 * Graph-independent (csrc/hit_linkage.hip).  n_rows rows (< 2^31 - 1) in device memory in ascending d_lo order: d_lo <= d_hi
 * int64 (|x| < 2^61), d_masks uint64 [n_rows][hw]; n_sites sites (< 2^29) in ascending d_pos order (equal positions allowed):
 * d_pos int64, d_n_alts uint8 (<= 3), d_allele_bits uint64 [n_sites][3][hw] -- the slots a > n_alts are ignored whatever they
 * hold.  hw = ceil(n_haplotypes / 64), 1 <= n_haplotypes <= 32 768; the bits beyond n_haplotypes are CLEAR in the masks and the
 * used slots: the library does not mask them.  A cell (row, site, allele a = 1 .. n_alts) is a candidate when
 * max(lo - pos, pos - (hi - 1), 0) <= flank (0 <= flank < 2^61).  With n_hit = popcount(mask), n_allele = popcount(slot),
 * n_joint = popcount(mask & slot), H = n_haplotypes:  Dn = H n_joint - n_hit n_allele,
 * den = n_hit (H - n_hit) n_allele (H - n_allele), both exact in int64.  A candidate is LISTED when den != 0 and, in fp64,
 * Dn^2 >= (min_r2 - 1e-9) den (0 <= min_r2 <= 1): r^2 >= min_r2 with slack -- the caller computes r^2 from the integers and
 * makes the exact cut; the device's rounding can only list a cell too many.  The result is a CSR over the rows:
 *   d_link_off int64 [n_rows + 1]: the links of row i are d_link_off[i] .. d_link_off[i + 1] - 1; *h_total = d_link_off[n_rows];
 *   d_site int32, d_allele uint8 (1 .. 3), d_joint int32 [link_capacity]: ascending (site, allele) within a row;
 *   d_n_hit int32 [n_rows];  d_n_allele int32 [n_sites][3] (0 in the unused slots): written by every call.
 * Count first, then allocate: the link arrays are written only when link_capacity >= *h_total (else they are untouched and
 * may be NULL with link_capacity 0).  GFM_LINKAGE_HAVE_OFFSETS: d_link_off already holds the offsets an earlier call made for
 * the same input, the counting pass is not run again.  rows_per_tile (0: 32; 8, 16 or 32) and slots_per_chunk (0: 256; 64,
 * 128 or 256) cut the work; the result does not depend on them; other values give GFM_ERR_INVALID.  The input is CHECKED on
 * the device before anything is counted: rows or sites out of order, lo > hi, n_alts > 3 or a coordinate beyond the limit
 * give GFM_ERR_INVALID and no link.  The call WAITS for the stream (it reads the verdict of the check and the total). */
#define GFM_LINKAGE_HAVE_OFFSETS 1u
int gfm_hit_linkage(const int64_t *d_lo, const int64_t *d_hi, const uint64_t *d_masks, int64_t n_rows, const int64_t *d_pos,
                    const uint8_t *d_n_alts, const uint64_t *d_allele_bits, int64_t n_sites, int32_t hw, int32_t n_haplotypes,
                    int64_t flank, double min_r2, int64_t *d_link_off, int64_t link_capacity, int32_t *d_site,
                    uint8_t *d_allele, int32_t *d_joint, int32_t *d_n_hit, int32_t *d_n_allele, int32_t rows_per_tile,
                    int32_t slots_per_chunk, uint32_t flags, int64_t *h_total, void *stream);

/* Phased VCF (plain or gzip/bgzip) -> the site arrays of gfm_graph_create for one chromosome; host
 * threads parse the lines.  The reference hands the VCF to `vg construct` / `vg index -G`
 * (constructVG.py:332,394); here every ALT allele is taken apart: single-base substitutions (one site per
 * position with up to 3 alternates, also across records), insertions, plain deletions, equal-length
 * multi-base substitutions (one substitution per mismatching position) -- after normalising the ALT against REF
 * (common trailing, then leading bases dropped: the alleles of an STR record REF=ATTT ALT=A,AT,ATT become deletions of
 * 3, 2, 1 bases behind its first base; up to 64 ALT alleles per record).  What is then still none of these -- a
 * complex allele, REF=ACG ALT=TC -- becomes the substitutions of its first min(|REF|, |ALT|) bases plus an insertion /
 * deletion of the rest behind the last of them, with the allele's carriers (vg construct decomposes by alignment: same
 * haplotype sequences).  A record with an ALT that is no string of A, C, G, T (symbolic <DEL> / <CN0>, breakends, '*')
 * is left out whole, as `vg construct` without --handle-sv leaves it out; its ALT alleles are counted in *n_skipped.
 * Deletions may overlap; two records that delete the same bases merge their carriers.  Two haplotypes per sample in
 * file order.
 * gfm_vcf_read copies: pos [n], n_alts [n], alt_bases [n][3], del_len [n], alt_bits [n][3][ceil(H/64)]
 * (may be NULL). */
typedef struct gfm_vcf *gfm_vcf_t;
int gfm_vcf_open(const char *path, const char *chrom, int with_haplotypes, int n_threads, gfm_vcf_t *out,
                 int64_t *n_sites, int32_t *n_haplotypes, int64_t *n_skipped);
int gfm_vcf_read(gfm_vcf_t v, int32_t *pos, uint8_t *n_alts, uint8_t *alt_bases, int32_t *del_len,
                 uint64_t *alt_bits);
/* insertion sites: ins_len [n], ins_off [n] into ins_bases [gfm_vcf_ins_bytes()] (ins_bases may be NULL) */
int64_t gfm_vcf_ins_bytes(gfm_vcf_t v);
int gfm_vcf_read_insertions(gfm_vcf_t v, int32_t *ins_len, int32_t *ins_off, uint8_t *ins_bases);
void gfm_vcf_close(gfm_vcf_t v);

#ifdef __cplusplus
}
#endif
#endif /* GRAFIMO_HIP_H */
