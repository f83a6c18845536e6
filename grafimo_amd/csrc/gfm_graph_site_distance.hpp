// gfm_graph_site_distance.hpp -- site distance: for every window of a spelled sequence, the least number of substitutions
// that lifts it over a score cutoff (the near side) and the least number that drops a site under it (the fragile side), with
// the columns picked (included at the end of graph_extract.hip behind gfm_graph_substitution_scan.hpp; it uses base_code,
// view_motif_set, SeqMotifs, gfail, gfm_graph_table_score.hpp's window_sum and gfm_sequence_tiles.hpp's SeqTile, offset walk
// and host protocol; the kernel's device code is its own, as the mutation scan's is).  Where the scans before it enumerate their edits and score every one, this kernel selects: a
// PWM is additive, so the best set of k columns to change is the k columns with the largest gains, and no set is enumerated.
//
// THE RULE (include/grafimo_hip.h states it for the library; tests/site_distance_bruteforce.py on the host).
// Inputs: a sequence x of n bases; a motif of width W with its integer matrix as the packed table holds it, entry t[j][b] for
// the window's forward column j and base b, one table per strand; a cutoff c in 0 .. 1000 W + 1; a cap E in 1 .. 8.
// Every window start s in 0 .. n - W and every strand is handled independently.
// Under GFM_GRAPH_FORWARD_ONLY only the + strand is handled.  Case is folded, as base_code does.
// A window that holds a column with no A/C/G/T scores min_val on both strands.  Otherwise its score is the sum of its entries.
// A window's unedited score on a strand is its `own` score.  The window is a site on that strand when own >= c.
// Raising (the near side).  Start from the window as spelled and repeat these steps:
//   1. If the current score >= c, stop with d = picks made.
//   2. If E picks are made, stop with d = E + 1.
//   3. If a non-base column remains, the next pick is the leftmost such column.  It gets the column's best base: the largest
//      entry on this strand.  Ties go to the first of A, C, G, T.  While any non-base column remains, the score stays min_val.
//   4. Otherwise the next pick is the unpicked base column with the largest gain.  The gain is the column's largest entry minus
//      its present entry.  Ties go to the leftmost column.  The column gets that best base.  Ties go to the first of A, C, G, T.
//   5. If every remaining gain is 0, stop with d = E + 1.
// Lowering (the fragile side).
//   1. If own < c, d = 0 and there are no picks.
//   2. A window with a non-base column takes no picks: d = 0 if min_val < c, otherwise d = E + 1.
//   3. Otherwise pick as above, with the loss in place of the gain.  The loss is the present entry minus the column's smallest
//      entry.  The worst base is the smallest entry.  Ties go to the first of A, C, G, T.  Stop when the score < c, with d = picks
//      made.  Stop at E picks, or when every remaining loss is 0, with d = E + 1.
// Results per (window start, strand, side): d in 0 .. E + 1; the score after the picks made; the 64-bit mask of the picked
// forward columns, bit j for column j.  d and the score do not depend on the tie rules.  Only the mask does.
// By the exchange argument d is the true minimum whenever it is <= E.
// Columns are always forward offsets in the window.  Bases are forward-strand bases.  The - strand reads its own half of the
// packed table at the same forward column.
//
// Work decomposition: the mutation scan's.  The unit is a (sequence, tile of GFM_SITEDIST_TILE window starts) pair, listed by
// the entry in a tile table (scratch of the call) and checked on the device before anything is read through it; one wavefront
// is a workgroup, grid.y = motif in launches of at most kSeqMotifs, a workgroup strides over the tiles.  Per workgroup the
// motif's packed two-strand table (W x 8 words) is staged once in LDS, and beside it the per-column extremes of both strands,
// packed like the table: word x of ext_s[j] holds the largest '+' entry of column j in its low half and the largest '-' entry
// in its high half, word y the smallest ones.  A gain is then ext.x - entry and a loss entry - ext.y, one packed subtraction
// each that cannot borrow: either half of the minuend is at least that half of the subtrahend.  The two words of a column
// are read as one 8-byte word, at the same address in every lane (a broadcast).  Per tile the base codes of its window starts
// and a halo of W - 1 BEHIND them go to LDS (a position outside the sequence is no base); a lane per window start.
//   the lane's window is summed once (window_sum: W lookups; the codes 4 .. 7 hold 0 in the table, so the sum is that of the
//   base columns), the non-base columns are gathered in a 64-bit mask with the sum of their largest entries;
//   the four selections of the window -- near +, near -, fragile +, fragile - -- are SdPick records of four scalars each, all
//   in registers: the mask of the picked columns, the score, the picks made and d (-1 while picking).  Non-base columns are
//   repaired at once (the lowest min(count, E) bits of the mask); then at most E passes over the W columns, each of which
//   finds for all four selections the unpicked column with the largest gain or loss (strictly larger: the leftmost wins) from
//   ONE table word and ONE extremes word per column, and takes it.  A pass costs W x 3 LDS reads whatever the number of
//   selections still open; a lane leaves when its four are closed.  No per-lane array exists, so nothing lands in scratch.
// The six words and four masks of a window start are written with plain vector stores; no atomics but the status word's.
// LDS: 2 048 (table) + 512 (extremes) + 128 (codes) = 2 688 bytes a workgroup: 32 workgroups a CU hold 84 KiB of its 160 --
// the wavefront slots, not the LDS, bound the occupancy.
namespace {

constexpr int kSdTile = GFM_SITEDIST_TILE, kSdThreads = kSdTile;
constexpr int kSdCodes = (kSdTile + GFM_MAX_WIDTH - 1 + 15) & ~15;                   // 128
constexpr unsigned kSdNone = 0xffffffffu;
static_assert(GFM_SITEDIST_TILE == GFM_MUTSCAN_TILE, "the tiles are the mutation scan's");
static_assert(GFM_SITEDIST_MAX_EDITS <= 15, "d = E + 1 fits the word's four bits");

struct SdResults {
    unsigned *words[kSeqMotifs];
    unsigned long long *masks[kSeqMotifs];
    int cutoff[kSeqMotifs];
};

// the cutoffs a motif of width W can be asked for: 0 (every window is a site) .. 1000 W + 1 (no score reaches it)
bool sitedist_cutoff_ok(long long c, int W) { return c >= 0 && c <= 1000ll * W + 1; }
bool sitedist_edits_ok(long long E) { return E >= 1 && E <= GFM_SITEDIST_MAX_EDITS; }

// one selection of a window: near or fragile on one strand
struct SdPick {
    unsigned long long picked;
    int score, n, d;                                              // d < 0: still picking
};

// steps 1 and 2 of THE RULE: the score is on the asked side of the cutoff, or the cap is reached
template <bool kRaise>
__device__ __forceinline__ void sd_settle(SdPick &p, int c, int E)
{
    if (kRaise ? p.score >= c : p.score < c) p.d = p.n;
    else if (p.n >= E) p.d = E + 1;
}

// the end of a pass: column j moves the score by `best` (0: no unpicked column moves it, step 5)
template <bool kRaise>
__device__ __forceinline__ void sd_take(SdPick &p, unsigned best, int j, int c, int E)
{
    if (p.d >= 0) return;
    if (best == 0u) { p.d = E + 1; return; }
    p.picked |= 1ull << j;
    p.score += kRaise ? (int)best : -(int)best;
    ++p.n;
    sd_settle<kRaise>(p, c, E);
}

__device__ __forceinline__ unsigned sd_word(const SdPick &p) { return ((unsigned)p.score << 4) | (unsigned)p.d; }

__global__ void __launch_bounds__(kSdThreads)
site_distance_kernel(const SeqTile *__restrict__ tiles, long long n_tiles, const uint8_t *__restrict__ bases, long long n_bases,
                     SeqMotifs mt, SdResults res, int W, int E, int forward_only, int *__restrict__ status)
{
    __shared__ unsigned ftab_s[GFM_MAX_WIDTH * 8];
    __shared__ uint2 ext_s[GFM_MAX_WIDTH];
    __shared__ unsigned char code_s[kSdCodes];
    const int m = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < W * 8; i += kSdThreads) ftab_s[i] = mt.ftab[m][i];
    __syncthreads();
    for (int j = tid; j < W; j += kSdThreads) {
        unsigned hp = 0u, hm = 0u, lp = 0xffffu, lm = 0xffffu;
        for (int b = 0; b < 4; ++b) {
            const unsigned e = ftab_s[j * 8 + b];
            hp = max(hp, e & 0xffffu); hm = max(hm, e >> 16);
            lp = min(lp, e & 0xffffu); lm = min(lm, e >> 16);
        }
        ext_s[j] = make_uint2(hp | (hm << 16), lp | (lm << 16));
    }
    unsigned *__restrict__ words = res.words[m];
    unsigned long long *__restrict__ masks = res.masks[m];
    const int min_val = mt.min_val[m], c = res.cutoff[m];
    const int halo = W - 1;
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const SeqTile tile = tiles[t];
        // ---- the tile, checked: everything read and written below lies inside its sequence (uniform: no thread stays behind)
        if (tile.begin < 0 || tile.len <= 0 || tile.begin > n_bases - tile.len || tile.start < 0 || tile.start >= tile.len) {
            if (tid == 0) atomicOr(status, kSeqBadTile);
            continue;
        }
        const uint8_t *__restrict__ x = bases + tile.begin;
        const int len = tile.len, lo = tile.start, nt = min(kSdTile, len - lo);
        __syncthreads();                                          // (the extremes are staged; the last tile's codes are read)
        for (int i = tid; i < nt + halo; i += kSdThreads) {       // (nt + halo <= 127 < kSdCodes)
            const int p = lo + i;
            code_s[i] = (unsigned char)(p < len ? base_code(x[p]) : 4u);
        }
        __syncthreads();
        if (tid < nt) {
            const int s = lo + tid;
            unsigned *wq = words + (tile.begin + s) * 6;
            unsigned long long *mq = masks + (tile.begin + s) * 4;
            if (s > len - W) {                                        // no window starts here
                wq[0] = kSdNone; wq[1] = kSdNone; wq[2] = kSdNone; wq[3] = kSdNone; wq[4] = kSdNone; wq[5] = kSdNone;
                mq[0] = 0ull; mq[1] = 0ull; mq[2] = 0ull; mq[3] = 0ull;
            } else {
                // ---- the window as spelled: its packed sum, its non-base columns and what their best bases would add
                unsigned long long bad = 0ull;
                unsigned fix = 0u;
                const WindowSum w = window_sum(ftab_s, W, [&](int j) {
                    const unsigned code = code_s[tid + j];
                    if (code >> 2) { bad |= 1ull << j; fix += ext_s[j].x; }
                    return code;
                });
                const int own_p = plus_score(w, min_val), own_m = minus_score(w, min_val);
                SdPick np{0ull, own_p, 0, -1}, nm{0ull, own_m, 0, -1}, fp{0ull, own_p, 0, -1}, fm{0ull, own_m, 0, -1};
                if (bad) {
                    // fragile: no picks.  near: min_val may already be a site's score; else the leftmost min(count, E) are repaired
                    fp.d = fm.d = min_val < c ? 0 : E + 1;
                    if (min_val >= c) np.d = nm.d = 0;
                    else {
                        const int nb = __popcll(bad), k = min(nb, E);
                        unsigned long long rest = bad;
                        for (int i = 0; i < k; ++i) rest &= rest - 1ull;
                        np.picked = nm.picked = bad ^ rest;
                        np.n = nm.n = k;
                        if (nb > E) np.d = nm.d = E + 1;
                        else {
                            const unsigned full = w.sum + fix;            // (a half holds at most 1000 W)
                            np.score = (int)(full & 0xffffu);
                            nm.score = (int)(full >> 16);
                            sd_settle<true>(np, c, E);
                            sd_settle<true>(nm, c, E);
                        }
                    }
                } else {
                    sd_settle<true>(np, c, E);
                    sd_settle<true>(nm, c, E);
                    sd_settle<false>(fp, c, E);
                    sd_settle<false>(fm, c, E);
                }
                if (forward_only) nm.d = fm.d = 0;
                // ---- at most E passes: the largest unpicked gain or loss of every open selection, the leftmost of equal ones
                for (int pass = 0; pass < E && (np.d | nm.d | fp.d | fm.d) < 0; ++pass) {
                    unsigned bnp = 0u, bnm = 0u, bfp = 0u, bfm = 0u;
                    int jnp = 0, jnm = 0, jfp = 0, jfm = 0;
                    for (int j = 0; j < W; ++j) {
                        const unsigned e = ftab_s[j * 8 + code_s[tid + j]];
                        const uint2 ext = ext_s[j];
                        const unsigned g = ext.x - e, l = e - ext.y;      // (a non-base column: picked near, closed fragile)
                        const unsigned long long bit = 1ull << j;
                        const unsigned gp = g & 0xffffu, gm = g >> 16, lp = l & 0xffffu, lm = l >> 16;
                        if (gp > bnp && !(np.picked & bit)) { bnp = gp; jnp = j; }
                        if (gm > bnm && !(nm.picked & bit)) { bnm = gm; jnm = j; }
                        if (lp > bfp && !(fp.picked & bit)) { bfp = lp; jfp = j; }
                        if (lm > bfm && !(fm.picked & bit)) { bfm = lm; jfm = j; }
                    }
                    sd_take<true>(np, bnp, jnp, c, E);
                    sd_take<true>(nm, bnm, jnm, c, E);
                    sd_take<false>(fp, bfp, jfp, c, E);
                    sd_take<false>(fm, bfm, jfm, c, E);
                }
                // the columns own +, own -, near +, near -, fragile +, fragile -; the masks near +, near -, fragile +, fragile -
                wq[0] = (unsigned)own_p; wq[2] = sd_word(np); wq[4] = sd_word(fp);
                mq[0] = np.picked; mq[2] = fp.picked;
                if (forward_only) {
                    wq[1] = kSdNone; wq[3] = kSdNone; wq[5] = kSdNone;
                    mq[1] = 0ull; mq[3] = 0ull;
                } else {
                    wq[1] = (unsigned)own_m; wq[3] = sd_word(nm); wq[5] = sd_word(fm);
                    mq[1] = nm.picked; mq[3] = fm.picked;
                }
            }
        }
    }
}

}  // namespace

GFM_API int gfm_sequence_site_distance(const gfm_motif_t *motifs, int32_t n_motifs, int32_t n_seqs, const int64_t *seq_offsets,
                                       const uint8_t *d_bases, const int32_t *cutoffs, int32_t max_edits, uint32_t flags,
                                       uint32_t *const *d_words, uint64_t *const *d_masks, int32_t *d_status, void *stream)
{
    const std::string entry = "gfm_sequence_site_distance";
    if (n_motifs < 1) return gfail(GFM_ERR_INVALID, "gfm_sequence_site_distance: n_motifs < 1");
    if (n_seqs < 0) return gfail(GFM_ERR_INVALID, "gfm_sequence_site_distance: n_seqs < 0");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    // ---- the cap and the cutoffs: checked with no sequence too, as far as can be told without the motifs' width
    if (!sitedist_edits_ok(max_edits))
        return gfail(GFM_ERR_INVALID, "gfm_sequence_site_distance: max_edits " + std::to_string(max_edits) + " is outside 1 .. " +
                                      std::to_string(GFM_SITEDIST_MAX_EDITS));
    if (!cutoffs) return gfail(GFM_ERR_INVALID, "gfm_sequence_site_distance: NULL cutoffs");
    for (int m = 0; m < n_motifs; ++m)
        if (!sitedist_cutoff_ok(cutoffs[m], GFM_MAX_WIDTH))
            return gfail(GFM_ERR_INVALID, "gfm_sequence_site_distance: cutoff " + std::to_string(cutoffs[m]) + " of motif " +
                                          std::to_string(m) + " is outside 0 .. 1000 W + 1 for every width");
    // ---- the sequences and their tiles
    std::vector<SeqTile> tiles;
    if (const int rc = seq_tiles(entry, kSdTile, n_seqs, seq_offsets, tiles)) return rc;
    // ---- the motifs: one width, and every cutoff within that width's scores -- looked at whenever the caller gives them
    if (!tiles.empty() && (!motifs || !d_words || !d_masks || !d_status || !d_bases))
        return gfail(GFM_ERR_INVALID, "gfm_sequence_site_distance: NULL argument");
    if (!motifs) return GFM_OK;                                   // (no base, and nothing more to check)
    for (int m = 0; m < n_motifs; ++m)
        if (!motifs[m] || (!tiles.empty() && (!d_words[m] || !d_masks[m])))
            return gfail(GFM_ERR_INVALID, "NULL motif / device buffer");
    if (!tiles.empty())
        for (int m = 0; m < n_motifs; ++m)                        // (a mask is stored as one 8-byte word)
            if (reinterpret_cast<uintptr_t>(d_masks[m]) & 7u)
                return gfail(GFM_ERR_INVALID, "gfm_sequence_site_distance: d_masks[m] is 8-byte aligned");
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::PackedTable, ms)) return rc;
    const int W = ms.W;
    for (int m = 0; m < n_motifs; ++m)
        if (!sitedist_cutoff_ok(cutoffs[m], W))
            return gfail(GFM_ERR_INVALID, "gfm_sequence_site_distance: cutoff " + std::to_string(cutoffs[m]) + " of motif " +
                                          std::to_string(m) + " is outside 0 .. " + std::to_string(1000 * W + 1) + " (W = " +
                                          std::to_string(W) + ")");
    if (tiles.empty()) return GFM_OK;
    const long long n_bases = seq_offsets[n_seqs];
    const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0;
    return run_seq_tiles(entry, tiles, n_motifs, d_status, stream,
                         [&](int m0, int mm, unsigned blocks, const SeqTile *d_tiles, long long n_tiles, hipStream_t st) {
        SeqMotifs mt = {};
        SdResults res = {};
        for (int k = 0; k < mm; ++k) {
            mt.ftab[k] = ms.ftab[(size_t)(m0 + k)];
            mt.min_val[k] = ms.min_val[(size_t)(m0 + k)];
            res.words[k] = d_words[m0 + k];
            res.masks[k] = reinterpret_cast<unsigned long long *>(d_masks[m0 + k]);
            res.cutoff[k] = cutoffs[m0 + k];
        }
        hipLaunchKernelGGL(site_distance_kernel, dim3(blocks, (unsigned)mm), dim3(kSdThreads), 0, st, d_tiles, n_tiles, d_bases,
                           n_bases, mt, res, W, (int)max_edits, fwd, d_status);
    });
}
