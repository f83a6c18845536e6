// gfm_graph_substitution_scan.hpp -- substitution scan: every block of L bases of a spelled sequence replaced in place by its
// image under a base map, for a list of lengths L in 1 .. GFM_SUBSCAN_MAX_LENGTH, every window the edit touches scored before
// and after on both strands (included at the end of graph_extract.hip behind gfm_graph_deletion_scan.hpp, whose
// delscan_side_windows it shares, with gfm_graph_indel_scan.hpp's indel_stride; gfm_sequence_tiles.hpp gives it SeqTile,
// CellResults, SideBest, the COVER walk (cover_head, cover_extend: the deletion kernel calls the same two), the tile check, the
// table staging, the length mask and the host protocol; it uses base_code, view_motif_set, SeqMotifs, gfail and
// gfm_graph_table_score.hpp's strand_scores and walk_value).  It is the deletion kernel's
// sibling: every window start is scored ONCE -- over x and over x' = f(x) in the same pass --, the running DIFFERENCE of the
// two passes is kept, and every window of every substituted sequence is put together from stored pieces, with no table lookup.
//
// THE RULE (include/grafimo_hip.h states it for the library; tests/substitution_scan_bruteforce.py on the host).  For a sequence
// x of n bases, a motif of width W, a strictly ascending list of lengths L0 < L1 < .. with every L in 1 .. 64, a base map f
// given as four codes -- the images of A, C, G, T, each in 0 .. 3 for A, C, G, T; any map is allowed: fixed points, constant
// maps and the identity included --, every length L of the list and every offset o in 0 .. n - 1:
//   If o + L > n there is no edit: both keys and both sums of the cell are 0.
//   Otherwise y = x[:o] + f(x[o:o+L]) + x[o+L:].  f is applied base by base.  Case is folded, as base_code does.
//   A base that is not A/C/G/T maps to itself: unlike a deletion, a substituted N is NOT repaired.
//   This is gfm_graph_query_edits' rule with lr = la = L at offset o, the alleles not trimmed.
//     REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o + L - 1, n - W).  This is bit for bit the
//     deletion scan's COVER column.
//     ALT side (column SUB): the same starts in y.
//   Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
//   A window that holds a base that is not A/C/G/T scores min_val on both strands.
//   Per column, the best window by (score descending, s ascending, + before -), as the key
//   ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. L - 1 on both sides.
//   Key 0 means the side has no window.
//   Per column, the exact uint64 sum of w[score] over the side's windows and strands.
//   Under the identity map SUB == COVER in every cell.
//   At L = 1, wherever x[o] is a base, SUB equals the mutation scan's column of the base f(x[o]), field for field.
//
// The algebra.  Full[t] = the packed two-strand sum of window t over x, Full'[t] = the same over x' = f(x), and
// D(e, m) = (the columns 0 .. m - 1 of the window that starts at e - m, over x') - (the same over x), D(., 0) = 0.
// The window of y that starts at s, for the block (o, L):
//   s = o - m, 0 <= m, m + L <= W       Full[s] - D(o, m) + D(o + L, m + L)     (the block lies inside the window)
//   s = o - m, m + L > W                Full'[s] - D(o, m)                      (the window ends inside the block)
//   s = o + d, 1 <= d < L, L - d < W    Full[s] + D(o + L, L - d)               (the window starts inside the block)
//   s = o + d, L - d >= W               Full'[s]                                (the window lies inside the block)
// D is a difference of packed fields: either half may be negative, and a borrow of the low half runs into the high one, so a D
// word alone means nothing.  As in the indel header's "cannot borrow" argument the words are added modulo 2^32 and every
// FINISHED window holds each column exactly once -- from x or from x' --: it is the packed sum of W table entries, both of whose
// halves are below 2^16 (a motif's column maxima total below 2^16), and the word that is exact modulo 2^32 is therefore exact.
// A window of y holds a base that is none exactly when the same window of x does (f keeps a non-base, and makes none): ONE flag
// per scored window start settles it, no ballots and no run lengths per length.
//
// Work decomposition: the deletion kernel's -- one wavefront per (sequence, tile of GFM_SUBSCAN_TILE offsets) from a tile table,
// checked on the device before anything is read through it; grid.y = motif; the motif's packed table (W x 8 words) is staged
// once per workgroup.  The lengths travel as a 64-bit mask, bit L - 1 for length L, the map as four codes in one word (byte c:
// the image of code c, in base_code's numbering); both are uniform (scalar) in the kernel.  Per tile, with Lmax the longest:
//   phase 1  the codes of x[lo - 64 .. lo + 192) and their images go to LDS (outside the sequence: no base); every window start
//            lo - W + 1 .. lo + nt + Lmax - 2 is scored ONCE with two running sums, over x and over x' (2 W lookups), and on the
//            way their difference after column j is stored as D(start + j + 1, j + 1) when that row is one of
//            lo .. lo + nt + Lmax - 1; Full, Full', the non-base flag, both sequences' strand scores under the non-base rule and,
//            for the windows inside the sequence, both weights w[+ score] + w[- score] are kept;
//   phase 2  a thread per offset o.  COVER is incremental over the ascending lengths, as in the deletion kernel.  SUB per listed
//            length over its min(W - 1, o) + L starts, clipped to 0 <= s <= n - W: the windows that lie inside the block take
//            their stored scores and weight; every other one is 1 Full and 1 or 2 words of D, and the weight gathers of its two
//            strands.  Two keys and two sums a length, written with plain 8- and 16-byte stores.  No atomics but the status
//            word's.
// There is ONE table in dynamic LDS, D, [64 + Lmax rows][stride = W | 1] words (the odd stride: see the indel header).  LDS a
// workgroup: 2 048 (table) + 2 x 256 (codes) + 192 (flags) + 192 x 2 x (4 + 4 + 8) (Full, scores, weights of x and x') +
// 4 (64 + Lmax) stride: 15 280 bytes at W = 19, Lmax = 20; 42 176 at W = 64, Lmax = 64.
namespace {

constexpr int kSsTile = GFM_SUBSCAN_TILE, kSsThreads = kSsTile, kSsMaxLen = GFM_SUBSCAN_MAX_LENGTH;
constexpr int kSsSide = GFM_MAX_WIDTH;                                              // code_s[i] is x[lo - kSsSide + i]
constexpr int kSsCodes = 4 * 64;                                                    // four turns of the wave
constexpr int kSsWindows = 192;                                                     // >= kSsTile + GFM_MAX_WIDTH + kSsMaxLen - 2
static_assert(kSsTile == 64 && kSsMaxLen == 64, "a tile is one wavefront's offsets, the lengths a 64-bit mask");
static_assert(kSsTile == GFM_DELSCAN_TILE && kSsMaxLen == GFM_DELSCAN_MAX_LENGTH, "COVER is the deletion scan's, cell for cell");
static_assert(kSsTile + GFM_MAX_WIDTH + kSsMaxLen - 2 <= kSsWindows, "every scored window has a slot");
static_assert(kSsSide + kSsTile + kSsMaxLen - 2 + GFM_MAX_WIDTH <= kSsCodes, "the last scored window ends inside the staged codes");

// the kernel's static LDS: the table, Full / scores / weights of x and of x', the codes of both, the flags
constexpr size_t kSsStaticLds = sizeof(unsigned) * GFM_MAX_WIDTH * 8 + (size_t)kSsWindows * 2 * (4 + 4 + 8) + 2 * kSsCodes + kSsWindows;

__host__ __device__ constexpr size_t subscan_lds_bytes(int W, int lmax)
{
    return sizeof(unsigned) * (size_t)(kSsTile + lmax) * (size_t)indel_stride(W);
}
static_assert(kSsStaticLds + subscan_lds_bytes(GFM_MAX_WIDTH, kSsMaxLen) <= 64u * 1024u, "one D table: no launch attribute is needed");

// the map in base_code's numbering (A 0, C 1, T 2, G 3), byte c of the word the image of code c; base_map: the images of
// A, C, G, T as 0 .. 3 for A, C, G, T
__host__ constexpr unsigned subscan_code_of(unsigned letter) { return letter == 2u ? 3u : letter == 3u ? 2u : letter; }
__host__ constexpr unsigned subscan_pack_map(const uint8_t base_map[4])
{
    unsigned word = 0u;
    for (unsigned i = 0; i < 4u; ++i) word |= subscan_code_of(base_map[i]) << (8u * subscan_code_of(i));
    return word;
}

__global__ void __launch_bounds__(kSsThreads)
substitution_scan_kernel(const SeqTile *__restrict__ tiles, long long n_tiles, const uint8_t *__restrict__ bases, long long n_bases,
                         SeqMotifs mt, CellResults res, int W, unsigned long long lengths, unsigned map, int forward_only,
                         int *__restrict__ status)
{
    extern __shared__ unsigned d_s[];                             // D(lo + row, m) at [row * stride + m - 1], m = 1 .. W
    __shared__ unsigned ftab_s[GFM_MAX_WIDTH * 8];
    __shared__ unsigned long long wref_s[kSsWindows], wsub_s[kSsWindows];           // the weights of the window over x, over x'
    __shared__ unsigned wsum_s[kSsWindows], wsum2_s[kSsWindows];                    // Full, Full'
    __shared__ unsigned wsc_s[kSsWindows], wsc2_s[kSsWindows];    // + score | - score << 16, under the non-base rule
    __shared__ unsigned char code_s[kSsCodes], code2_s[kSsCodes], bad_s[kSsWindows];
    const int mi = blockIdx.y, tid = threadIdx.x;
    stage_table(ftab_s, mt.ftab[mi], W, kSsThreads);
    const unsigned long long *__restrict__ wtab = mt.wtab[mi];
    uint2 *__restrict__ keys = res.keys[mi];
    ulonglong2 *__restrict__ sums = res.sums[mi];
    const int min_val = mt.min_val[mi];
    const int stride = indel_stride(W);
    const int lmax = lengths ? 64 - __builtin_clzll(lengths) : 0;
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const SeqTile tile = tiles[t];
        if (seq_tile_bad(tile, n_bases, status)) continue;
        const uint8_t *__restrict__ x = bases + tile.begin;
        const int len = tile.len, lo = tile.start, nt = min(kSsTile, len - lo);
        __syncthreads();                                          // (the table is staged; the last tile's rows are read)
        // ---- the codes of x[lo - 64 .. lo + 192) and of their images
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long p = (long long)lo - kSsSide + k * 64 + tid;
            const unsigned c = (p >= 0 && p < len) ? base_code(x[p]) : 4u;
            code_s[k * 64 + tid] = (unsigned char)c;
            code2_s[k * 64 + tid] = (unsigned char)((c >> 2) ? c : (map >> (8u * c)) & 3u);
        }
        __syncthreads();
        // ---- phase 1: every window start lo - W + 1 .. lo + nt + lmax - 2 once; window k starts at lo - W + 1 + k
        const int n_win = nt + W + lmax - 2, last_row = nt + lmax - 1;
        for (int k = tid; k < n_win; k += kSsThreads) {
            const unsigned char *c = code_s + (k + kSsSide - W + 1), *c2 = code2_s + (k + kSsSide - W + 1);
            const int row0 = k - W + 2;                           // the row of the prefix that ends behind column 0
            WindowSum w{0u, 0u};
            unsigned sum2 = 0u;
            for (int j = 0; j < W; ++j) {
                const unsigned cj = c[j];
                w.sum += ftab_s[j * 8 + cj];
                w.bad += cj >> 2;
                sum2 += ftab_s[j * 8 + c2[j]];
                const int row = row0 + j;
                if (row >= 0 && row <= last_row) d_s[row * stride + j] = sum2 - w.sum;      // D(start + j + 1, j + 1)
            }
            const long long s = (long long)lo - W + 1 + k;
            const bool inside = s >= 0 && s <= (long long)len - W;
            const WindowSum w2{sum2, w.bad};
            const StrandScores sc = strand_scores(w, min_val), sc2 = strand_scores(w2, min_val);
            wsum_s[k] = w.sum;
            wsum2_s[k] = sum2;
            bad_s[k] = (unsigned char)(w.bad ? 1u : 0u);
            wsc_s[k] = (unsigned)sc.plus | ((unsigned)sc.minus << 16);
            wsc2_s[k] = (unsigned)sc2.plus | ((unsigned)sc2.minus << 16);
            wref_s[k] = inside ? walk_value(wtab, w, min_val, forward_only) : 0ull;
            wsub_s[k] = inside ? walk_value(wtab, w2, min_val, forward_only) : 0ull;
        }
        __syncthreads();
        // ---- phase 2: a thread per offset
        if (tid < nt) {
            const int o = lo + tid;
            const unsigned *d_o = d_s + tid * stride;             // D(o, m) = d_o[m - 1]
            const int last_start = len - W;                       // the last window start of x, and of y
            const int m_hi = min(W - 1, o);
            SideBest cover;
            cover_head(cover, wsc_s, wref_s, tid, W, o, last_start, forward_only);
            int l_prev = 0;
            long long cell = tile.begin + o;                      // of the first listed length; the next is n_bases further
            for (unsigned long long rest = lengths; rest; rest &= rest - 1ull, cell += n_bases) {
                const int L = __builtin_ctzll(rest) + 1;
                if (o + L > len) {                                // no edit (and none at any longer length)
                    store_cell(keys, sums, cell, SideBest{}, SideBest{});
                    continue;
                }
                cover_extend(cover, wsc_s, wref_s, tid, W, o, last_start, l_prev, L, forward_only);
                l_prev = L;
                const unsigned *d_l = d_o + L * stride;           // D(o + L, m) = d_l[m - 1]
                SideBest alt;
                // SUB, the starts o - m: the window holds the block's head (m + L > W) or all of it
                for (int m = m_hi; m >= 0; --m) {
                    if (o - m > last_start) continue;
                    const int k = tid + W - 1 - m;
                    const unsigned head = m ? d_o[m - 1] : 0u;
                    const unsigned word = (m + L <= W ? wsum_s[k] + d_l[m + L - 1] : wsum2_s[k]) - head;
                    const WindowSum w{word, bad_s[k]};
                    alt.add(strand_scores(w, min_val), -m, forward_only, walk_value(wtab, w, min_val, forward_only));
                }
                // SUB, the starts o + d: the window starts inside the block and leaves it (L - d < W) or lies inside it
                for (int d = 1; d < L && o + d <= last_start; ++d) {
                    const int k = tid + W - 1 + d;
                    if (L - d >= W) {                             // x' alone: stored
                        alt.add_packed(wsc2_s[k], d, forward_only, wsub_s[k]);
                        continue;
                    }
                    const WindowSum w{wsum_s[k] + d_l[L - d - 1], bad_s[k]};
                    alt.add(strand_scores(w, min_val), d, forward_only, walk_value(wtab, w, min_val, forward_only));
                }
                store_cell(keys, sums, cell, cover, alt);
            }
        }
    }
}

}  // namespace

GFM_API int gfm_sequence_substitution_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                           uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                                           int32_t n_lengths, const int32_t *lengths, const uint8_t base_map[4], uint32_t flags,
                                           uint32_t *const *d_keys, uint64_t *const *d_sums, int32_t *d_status, void *stream)
{
    const std::string entry = "gfm_sequence_substitution_scan";
    if (n_motifs < 1 || n_seqs < 0 || n_lengths < 1) return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    // ---- the lengths, then the map (four codes in 0 .. 3): both checked with no sequence too
    unsigned long long mask = 0ull;
    if (const int rc = length_mask(entry, n_lengths, lengths, kSsMaxLen, mask)) return rc;
    const int lmax = lengths[n_lengths - 1];
    if (!base_map) return gfail(GFM_ERR_INVALID, entry + ": NULL base_map");
    for (int i = 0; i < 4; ++i)
        if (base_map[i] > 3)
            return gfail(GFM_ERR_INVALID, entry + ": base_map[" + std::to_string(i) + "] = " + std::to_string((int)base_map[i]) +
                                          " is outside 0 .. 3");
    const unsigned map = subscan_pack_map(base_map);
    if (n_seqs == 0) return GFM_OK;
    std::vector<SeqTile> tiles;
    if (const int rc = seq_tiles(entry, kSsTile, n_seqs, seq_offsets, tiles)) return rc;
    if (tiles.empty()) return GFM_OK;
    if (const int rc = check_scan_buffers(entry, motifs, n_motifs, d_weights, d_keys, d_sums, d_status, d_bases)) return rc;
    if (const int rc = check_cell_alignment(entry, n_motifs, d_keys, d_sums)) return rc;
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::PackedTable, ms)) return rc;
    const int W = ms.W;
    // (a side has at most W + lmax - 1 windows, as COVER has in the deletion scan)
    if (const int rc = check_sum_capacity(entry, max_weight, delscan_side_windows(W, lmax),
                                          " (W = " + std::to_string(W) + ", longest length " + std::to_string(lmax) + ")"))
        return rc;
    const long long n_bases = seq_offsets[n_seqs];
    const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0;
    return run_seq_tiles(entry, tiles, n_motifs, d_status, stream,
                         [&](int m0, int mm, unsigned blocks, const SeqTile *d_tiles, long long n_tiles, hipStream_t st) {
        hipLaunchKernelGGL(substitution_scan_kernel, dim3(blocks, (unsigned)mm), dim3(kSsThreads), subscan_lds_bytes(W, lmax), st,
                           d_tiles, n_tiles, d_bases, n_bases, seq_motifs(ms, d_weights, m0, mm),
                           seq_results<CellResults>(d_keys, d_sums, m0, mm), W, mask, map, fwd, d_status);
    });
}
