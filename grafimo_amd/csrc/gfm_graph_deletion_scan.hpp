// gfm_graph_deletion_scan.hpp -- deletion scan: the deletion of every block of L bases of a spelled sequence, for a list of
// lengths L in 1 .. GFM_DELSCAN_MAX_LENGTH, every window the edit touches scored before and after on both strands (included at
// the end of graph_extract.hip behind gfm_graph_indel_scan.hpp, whose bits_from and indel_stride it shares;
// gfm_sequence_tiles.hpp gives it SeqTile, CellResults, SideBest, the COVER walk (cover_head, cover_extend), the tile check, the
// table staging, the length mask, seq_sum_fits and the host protocol; it uses base_code, view_motif_set, SeqMotifs, gfail and
// gfm_graph_table_score.hpp's strand_scores and walk_value).  It is the indel-scan kernel's
// deletion half stretched by the longest length: every window start is scored ONCE, the running prefixes of that pass are
// kept, and every junction window of every deletion is put together from two stored pieces.
//
// THE RULE (include/grafimo_hip.h states it for the library; tests/deletion_scan_bruteforce.py on the host).  For a sequence
// x of n bases, a motif of width W, a strictly ascending list of lengths L0 < L1 < .. with every L in 1 .. 64, every length L
// of the list and every offset o in 0 .. n - 1:
//   If o + L > n there is no edit: both keys and both sums of the cell are 0.
//   Otherwise y = x[:o] + x[o+L:].  This is gfm_graph_query_edits' rule with lr = L, la = 0 at offset o.
//     REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o + L - 1, n - W).
//     ALT side (column DEL): the starts of y across the junction, max(0, o - W + 1) <= s <= min(o - 1, n - L - W).
//   Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
//   A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
//   A deleted N can repair its junction windows.  An N elsewhere cannot be repaired.
//   Per column, the best window by (score descending, s ascending, + before -), as the key
//   ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. L - 1 for COVER and in -(W - 1) .. -1 for DEL.
//   Key 0 means the side has no window.
//   Per column, the exact uint64 sum of w[score] over the side's windows and strands.
//   At L = 1 the two columns equal the indel scan's COVER and DEL bit for bit.
//
// The algebra is the indel header's: Pre[t][m] = the packed two-strand sum of ftab[j][x[t + j]] over j < m, Full[t] =
// Pre[t][W], A(e, m) = Pre[e - m][m] -- the columns 0 .. m - 1 over x[e - m .. e - 1].  The junction window m = 1 .. W - 1
// of the deletion (o, L) starts at o - m and reads x[o - m .. o - 1] and x[o + L .. o + L + W - m - 1]:
//   A(o, m) + Full[o + L - m] - A(o + L, m)
// Full[o + L - m] holds the columns 0 .. m - 1 over x[o + L - m .. o + L - 1], which is exactly A(o + L, m), so the difference
// is the columns m .. W - 1 over the bases behind the block; the halves cannot borrow, for the reason given there (Full
// contains what is subtracted, every finished window holds each column once, a motif's column maxima total below 2^16).
// Which windows hold a base that is none is settled by the wave's FOUR ballots over the tile's codes (256 bits in scalar
// registers): dl = the run of real bases that ends at o - 1, dr(L) = the run that starts at o + L; window m is clean when
// m <= dl and W - m <= dr(L).  The deleted bases are in neither run: a deleted N repairs its windows.
//
// Work decomposition: one wavefront per (sequence, tile of GFM_DELSCAN_TILE offsets) from a tile table, checked on the device
// before anything is read through it; grid.y = motif; the motif's packed table (W x 8 words) is staged once per workgroup.
// The lengths travel as a 64-bit mask, bit L - 1 for length L: ascending and distinct by construction, and uniform (scalar)
// in the kernel.  Per tile, with Lmax the longest length:
//   phase 1  the codes of x[lo - 64 .. lo + 192) go to LDS (outside the sequence: no base), four ballots; every window start
//            lo - W + 1 .. lo + nt + Lmax - 2 is scored ONCE with W lookups (at most 190 starts: three turns of the wave), and
//            on the way the running sum after column j is stored as A(start + j + 1, j + 1) when that row is one of
//            lo .. lo + nt + Lmax - 1; Full, the two strands' scores under the non-base rule, and for the windows inside the
//            sequence the REF weight w[+ score] + w[- score] are kept;
//   phase 2  a thread per offset o.  COVER is incremental over the ascending lengths: the windows o - W + 1 .. o - 1 once, then
//            per listed length only the starts o + L_prev .. o + L - 1 (stored scores and weights: no lookup); rel is
//            relative to o, so one running key and one running sum serve every length.  DEL per listed length: the W - 1
//            junction windows, each 2 words of A, 1 Full and the weight gathers of its two strands.  Two keys and two sums a
//            length, written with plain 8- and 16-byte stores.  No atomics but the status word's.
// The A table is [64 + Lmax rows][stride = W | 1] words in dynamic LDS (the odd stride: see the indel header).  LDS a
// workgroup: 2 048 (table) + 256 (codes) + 192 x (4 + 4 + 8) (Full, scores, REF weights) + 4 (64 + Lmax) stride:
// 11 760 bytes at W = 19, Lmax = 20; 38 656 at W = 64, Lmax = 64.
namespace {

constexpr int kDsTile = GFM_DELSCAN_TILE, kDsThreads = kDsTile, kDsMaxLen = GFM_DELSCAN_MAX_LENGTH;
constexpr int kDsSide = GFM_MAX_WIDTH;                                              // code_s[i] is x[lo - kDsSide + i]
constexpr int kDsCodes = 4 * 64;                                                    // four turns of the wave, four ballots
constexpr int kDsWindows = 192;                                                     // >= kDsTile + GFM_MAX_WIDTH + kDsMaxLen - 2
static_assert(kDsTile == 64 && GFM_MAX_WIDTH == 64 && kDsMaxLen == 64, "the non-base bitmap is four 64-bit ballots, the lengths a 64-bit mask");
static_assert(kDsTile + GFM_MAX_WIDTH + kDsMaxLen - 2 <= kDsWindows, "every scored window has a slot");
static_assert(kDsSide + kDsTile + kDsMaxLen - 2 + GFM_MAX_WIDTH <= kDsCodes, "the last scored window ends inside the staged codes");

__host__ __device__ constexpr size_t delscan_lds_bytes(int W, int lmax)
{
    return sizeof(unsigned) * (size_t)(kDsTile + lmax) * (size_t)indel_stride(W);
}

// the capacity of a sum: a REF side has at most W + lmax - 1 windows, each once per strand
__host__ constexpr unsigned delscan_side_windows(int W, int lmax) { return 2u * (unsigned)(W + lmax - 1); }
__host__ constexpr bool delscan_sum_fits(uint64_t max_weight, int W, int lmax)
{
    return seq_sum_fits(max_weight, delscan_side_windows(W, lmax));
}
static_assert(delscan_sum_fits(UINT64_MAX / 254u, 64, 64) && !delscan_sum_fits(UINT64_MAX / 254u + 1u, 64, 64), "the bound is exact");

__global__ void __launch_bounds__(kDsThreads)
deletion_scan_kernel(const SeqTile *__restrict__ tiles, long long n_tiles, const uint8_t *__restrict__ bases, long long n_bases,
                     SeqMotifs mt, CellResults res, int W, unsigned long long lengths, int forward_only, int *__restrict__ status)
{
    extern __shared__ unsigned a_s[];                             // A(lo + row, m) at [row * stride + m - 1], m = 1 .. W
    __shared__ unsigned ftab_s[GFM_MAX_WIDTH * 8];
    __shared__ unsigned long long wref_s[kDsWindows];
    __shared__ unsigned wsum_s[kDsWindows];
    __shared__ unsigned wsc_s[kDsWindows];                        // + score | - score << 16, under the non-base rule
    __shared__ unsigned char code_s[kDsCodes];
    const int mi = blockIdx.y, tid = threadIdx.x;
    stage_table(ftab_s, mt.ftab[mi], W, kDsThreads);
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
        const int len = tile.len, lo = tile.start, nt = min(kDsTile, len - lo);
        __syncthreads();                                          // (the table is staged; the last tile's rows are read)
        // ---- the codes of x[lo - 64 .. lo + 192) and which of them are no base: nb[k] bit i is position lo - 64 + 64 k + i
        unsigned long long nb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long p = (long long)lo - kDsSide + k * 64 + tid;
            const unsigned c = (p >= 0 && p < len) ? base_code(x[p]) : 4u;
            code_s[k * 64 + tid] = (unsigned char)c;
            nb[k] = __builtin_amdgcn_ballot_w64((c >> 2) != 0u);
        }
        __syncthreads();
        // ---- phase 1: every window start lo - W + 1 .. lo + nt + lmax - 2 once; window k starts at lo - W + 1 + k
        const int n_win = nt + W + lmax - 2, last_row = nt + lmax - 1;
        for (int k = tid; k < n_win; k += kDsThreads) {
            const unsigned char *c = code_s + (k + kDsSide - W + 1);
            const int row0 = k - W + 2;                           // the row of the prefix that ends behind column 0
            WindowSum w{0u, 0u};
            for (int j = 0; j < W; ++j) {
                const unsigned cj = c[j];
                w.sum += ftab_s[j * 8 + cj];
                w.bad += cj >> 2;
                const int row = row0 + j;
                if (row >= 0 && row <= last_row) a_s[row * stride + j] = w.sum;     // A(start + j + 1, j + 1)
            }
            const long long s = (long long)lo - W + 1 + k;
            const StrandScores sc = strand_scores(w, min_val);
            wsum_s[k] = w.sum;
            wsc_s[k] = (unsigned)sc.plus | ((unsigned)sc.minus << 16);
            wref_s[k] = (s >= 0 && s <= (long long)len - W) ? walk_value(wtab, w, min_val, forward_only) : 0ull;
        }
        __syncthreads();
        // ---- phase 2: a thread per offset
        if (tid < nt) {
            const int o = lo + tid;
            const unsigned long long before = bits_from(nb[0], nb[1], tid);          // bit 63 is o - 1, bit 0 is o - 64
            const int dl = before ? __builtin_clzll(before) : 64;
            const unsigned *a_o = a_s + tid * stride;             // A(o, m) = a_o[m - 1]
            const int last_start = len - W;                       // the last window start of x
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
                // DEL: the junction window m starts at o - m and ends W - m bases behind the block
                const int g = tid + 64 + L;                       // the bitmap's bit of position o + L: 65 .. 191
                const int sh = g & 63;
                const unsigned long long behind = (g >> 6) == 1 ? bits_from(nb[1], nb[2], sh) : bits_from(nb[2], nb[3], sh);
                const int dr = behind ? __builtin_ctzll(behind) : 64;
                const int r = len - L - o;                        // the bases behind the block
                const unsigned *a_l = a_o + L * stride;           // A(o + L, m) = a_l[m - 1]
                const unsigned *full_l = wsum_s + (tid + L + W - 1);                 // Full[o + L - m] = full_l[-m]
                SideBest del;
                for (int m = max(1, W - r); m <= min(W - 1, o); ++m) {
                    const WindowSum w{a_o[m - 1] + full_l[-m] - a_l[m - 1], (m <= dl && W - m <= dr) ? 0u : 1u};
                    del.add(strand_scores(w, min_val), -m, forward_only, walk_value(wtab, w, min_val, forward_only));
                }
                store_cell(keys, sums, cell, cover, del);
            }
        }
    }
}

}  // namespace

GFM_API int gfm_sequence_deletion_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                       uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                                       int32_t n_lengths, const int32_t *lengths, uint32_t flags, uint32_t *const *d_keys,
                                       uint64_t *const *d_sums, int32_t *d_status, void *stream)
{
    const std::string entry = "gfm_sequence_deletion_scan";
    if (n_motifs < 1 || n_seqs < 0 || n_lengths < 1) return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    // ---- the lengths, checked with no sequence too
    unsigned long long mask = 0ull;
    if (const int rc = length_mask(entry, n_lengths, lengths, kDsMaxLen, mask)) return rc;
    const int lmax = lengths[n_lengths - 1];
    if (n_seqs == 0) return GFM_OK;
    std::vector<SeqTile> tiles;
    if (const int rc = seq_tiles(entry, kDsTile, n_seqs, seq_offsets, tiles)) return rc;
    if (tiles.empty()) return GFM_OK;
    if (const int rc = check_scan_buffers(entry, motifs, n_motifs, d_weights, d_keys, d_sums, d_status, d_bases)) return rc;
    if (const int rc = check_cell_alignment(entry, n_motifs, d_keys, d_sums)) return rc;
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::PackedTable, ms)) return rc;
    const int W = ms.W;
    if (const int rc = check_sum_capacity(entry, max_weight, delscan_side_windows(W, lmax),
                                          " (W = " + std::to_string(W) + ", longest length " + std::to_string(lmax) + ")"))
        return rc;
    const long long n_bases = seq_offsets[n_seqs];
    const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0;
    return run_seq_tiles(entry, tiles, n_motifs, d_status, stream,
                         [&](int m0, int mm, unsigned blocks, const SeqTile *d_tiles, long long n_tiles, hipStream_t st) {
        hipLaunchKernelGGL(deletion_scan_kernel, dim3(blocks, (unsigned)mm), dim3(kDsThreads), delscan_lds_bytes(W, lmax), st, d_tiles,
                           n_tiles, d_bases, n_bases, seq_motifs(ms, d_weights, m0, mm),
                           seq_results<CellResults>(d_keys, d_sums, m0, mm), W, mask, fwd, d_status);
    });
}
