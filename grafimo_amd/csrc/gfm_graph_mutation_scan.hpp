// gfm_graph_mutation_scan.hpp -- mutation scan: every single-base change at every offset of a spelled sequence, every window
// the change touches scored before and after on both strands (included at the end of graph_extract.hip behind
// gfm_sequence_tiles.hpp, whose SeqTile, ColumnResults and host side -- the offset walk, the buffer checks, the capacity rule
// and the protocol around the launches -- it uses, with base_code, view_motif_set, SeqMotifs, gfail and
// gfm_graph_table_score.hpp's window_sum, strand_scores, walk_value and edit_key.  The KERNEL shares none of that header's
// device functions: with SideBest for its five columns it took two more VGPRs and measured 1 to 2 % slower, so its device
// code is instruction for instruction what it was, profiles/sequence_scan_refactor.txt).
// Where query_edits_kernel
// scores the 2 W windows of ONE edit with W lookups each, this kernel scores every window of a sequence ONCE and derives the
// windows of all 4 n changes from the stored sums: an ALT window differs from its REF window in one table entry.
//
// THE RULE (include/grafimo_hip.h states it for the library; tests/mutation_scan_bruteforce.py on the host).  For a sequence x of
// n bases and a motif of width W, for every offset o in 0 .. n - 1 and every base b in A, C, G, T:
//   y = x with y[o] = b.  REF side: the window starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).  ALT side: the same
//   starts in y.  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.  A window that holds a base
//   that is not A/C/G/T scores min_val on both strands; case is folded, as base_code does.  Per side: the best window by (score
//   descending, s ascending, + before -), as the key ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. 0,
//   key 0: the side has no window (n < W); and the exact uint64 sum of w[score] over the side's windows and strands.  b equal
//   to the folded x[o] gives ALT equal to REF; an x[o] that is no base has an all-min_val REF side, and each b can repair it.
//
// Work decomposition: the unit is a (sequence, tile of GFM_MUTSCAN_TILE offsets) pair, listed by the entry in a tile table
// (scratch of the call) and checked on the device before anything is read through it; grid.y = motif, a workgroup strides
// over the tiles.  Per workgroup the motif's packed two-strand table (W x 8 words) is staged once in LDS.  Per tile:
//   phase 1  the base codes of the tile and a halo of W - 1 on each side go to LDS (a position outside the sequence is no
//            base); every window start under them -- at most TILE + W - 1 -- is scored ONCE: the packed two-strand sum (W LDS
//            lookups), the count of its non-base positions and, for the windows inside the sequence, the REF weight
//            w[+ score] + w[- score] (the only weight loads a REF side costs) are kept in LDS;
//   phase 2  a thread per offset o walks the at most W starts s = o - j (the lanes read consecutive LDS words: no bank
//            conflict): the REF score is the stored sum, or min_val; the ALT score for b is sum - ftab[j][x[o]] + ftab[j][b]
//            -- the halves of the packed word cannot borrow: each half of the sum contains the entry that is removed --; the
//            window is valid when its non-base count minus (x[o] is no base) is 0.  The column of b == x[o] is the REF column
//            and is copied, not loaded again.  Key maximum and uint64 sum per column in registers, w[score] through the cache;
//            the five keys and five sums of o are written with plain stores.  No atomics but the status word's.
// The tile is ONE wavefront's worth of offsets (64): a workgroup is a wavefront, its barriers cost nothing, no wavefront waits
// for the halo pass of another, and a sequence wastes half a tile of lanes at its end, 32 offsets, whatever its length.
// LDS: 2 048 (table) + 192 (codes) + 128 x (4 + 1 + 8) (sums, counts, REF weights) = 3 904 bytes a workgroup: 32 workgroups
// a CU hold 122 KiB of its 160 -- the wavefront slots, not the LDS, bound the occupancy.
namespace {

constexpr int kMsTile = GFM_MUTSCAN_TILE, kMsThreads = kMsTile;
constexpr int kMsHalo = GFM_MAX_WIDTH - 1;
constexpr int kMsCodes = (kMsTile + 2 * kMsHalo + 15) & ~15;                        // 192
constexpr int kMsWindows = (kMsTile + kMsHalo + 15) & ~15;                          // 128

__global__ void __launch_bounds__(kMsThreads)
mutation_scan_kernel(const SeqTile *__restrict__ tiles, long long n_tiles, const uint8_t *__restrict__ bases, long long n_bases,
                     SeqMotifs mt, ColumnResults res, int W, int forward_only, int *__restrict__ status)
{
    __shared__ unsigned ftab_s[GFM_MAX_WIDTH * 8];
    __shared__ unsigned long long wref_s[kMsWindows];
    __shared__ unsigned wsum_s[kMsWindows];
    __shared__ unsigned char code_s[kMsCodes], bad_s[kMsWindows];
    const int m = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < W * 8; i += kMsThreads) ftab_s[i] = mt.ftab[m][i];
    const unsigned long long *__restrict__ wtab = mt.wtab[m];
    unsigned *__restrict__ keys = res.keys[m];
    unsigned long long *__restrict__ sums = res.sums[m];
    const int min_val = mt.min_val[m];
    const int halo = W - 1;
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const SeqTile tile = tiles[t];
        // ---- the tile, checked: everything read and written below lies inside its sequence (uniform: no thread stays behind)
        if (tile.begin < 0 || tile.len <= 0 || tile.begin > n_bases - tile.len || tile.start < 0 || tile.start >= tile.len) {
            if (tid == 0) atomicOr(status, kSeqBadTile);
            continue;
        }
        const uint8_t *__restrict__ x = bases + tile.begin;
        const int len = tile.len, lo = tile.start, nt = min(kMsTile, len - lo);
        const int c0 = lo - halo;                                 // code_s[i] is x[c0 + i]; window k starts at c0 + k
        __syncthreads();                                          // (the table is staged; the last tile's windows are read)
        for (int i = tid; i < nt + 2 * halo; i += kMsThreads) {
            const int p = c0 + i;
            code_s[i] = (unsigned char)((p >= 0 && p < len) ? base_code(x[p]) : 4u);
        }
        __syncthreads();
        // ---- phase 1: every window start under the tile and its halo, once
        for (int k = tid; k < nt + halo; k += kMsThreads) {
            const WindowSum w = window_sum(ftab_s, W, [&](int j) { return (unsigned)code_s[k + j]; });
            const int s = c0 + k;
            wsum_s[k] = w.sum;
            bad_s[k] = (unsigned char)w.bad;
            wref_s[k] = (s >= 0 && s <= len - W) ? walk_value(wtab, w, min_val, forward_only) : 0ull;
        }
        __syncthreads();
        // ---- phase 2: a thread per offset; the starts s = o - j of the sequence's windows over o
        if (tid < nt) {
            const int o = lo + tid;
            const unsigned xo = code_s[tid + halo], xbad = xo >> 2;
            unsigned key_r = 0u, key_b[4] = {0u, 0u, 0u, 0u};
            unsigned long long sum_r = 0ull, sum_b[4] = {0ull, 0ull, 0ull, 0ull};
            const int j_lo = max(0, o - (len - W)), j_hi = min(halo, o);
            for (int j = j_lo; j <= j_hi; ++j) {
                const int k = tid + halo - j;
                const WindowSum w{wsum_s[k], bad_s[k]};
                const StrandScores rs = strand_scores(w, min_val);
                key_r = max(key_r, edit_key(rs.plus, -j, true));  // (the window starts at s = o - j)
                if (!forward_only) key_r = max(key_r, edit_key(rs.minus, -j, false));
                sum_r += wref_s[k];
                const unsigned invalid = w.bad - xbad;            // (0: no base of the window but x[o] itself is none)
                const unsigned rest = w.sum - ftab_s[j * 8 + xo];
#pragma unroll
                for (unsigned b = 0; b < 4; ++b) {
                    if (b == xo) continue;                        // the REF column: copied below
                    const WindowSum wb{rest + ftab_s[j * 8 + b], invalid};
                    const StrandScores as = strand_scores(wb, min_val);
                    key_b[b] = max(key_b[b], edit_key(as.plus, -j, true));
                    if (!forward_only) key_b[b] = max(key_b[b], edit_key(as.minus, -j, false));
                    sum_b[b] += walk_value(wtab, wb, min_val, forward_only);
                }
            }
#pragma unroll
            for (unsigned b = 0; b < 4; ++b)
                if (b == xo) { key_b[b] = key_r; sum_b[b] = sum_r; }
            // the columns REF, A, C, G, T; the codes are A 0, C 1, T 2, G 3
            unsigned *kq = keys + (tile.begin + o) * 5;
            unsigned long long *sq = sums + (tile.begin + o) * 5;
            kq[0] = key_r; kq[1] = key_b[0]; kq[2] = key_b[1]; kq[3] = key_b[3]; kq[4] = key_b[2];
            sq[0] = sum_r; sq[1] = sum_b[0]; sq[2] = sum_b[1]; sq[3] = sum_b[3]; sq[4] = sum_b[2];
        }
    }
}

}  // namespace

GFM_API int gfm_sequence_mutation_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                       uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                                       uint32_t flags, uint32_t *const *d_keys, uint64_t *const *d_sums, int32_t *d_status,
                                       void *stream)
{
    const std::string entry = "gfm_sequence_mutation_scan";
    if (n_motifs < 1 || n_seqs < 0) return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    if (n_seqs == 0) return GFM_OK;
    std::vector<SeqTile> tiles;
    if (const int rc = seq_tiles(entry, kMsTile, n_seqs, seq_offsets, tiles)) return rc;
    if (tiles.empty()) return GFM_OK;
    if (const int rc = check_scan_buffers(entry, motifs, n_motifs, d_weights, d_keys, d_sums, d_status, d_bases)) return rc;
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::PackedTable, ms)) return rc;
    const int W = ms.W;
    // the capacity of a sum: a side has at most W windows, each once per strand
    if (const int rc = check_sum_capacity(entry, max_weight, 2u * (unsigned)W, "")) return rc;
    const long long n_bases = seq_offsets[n_seqs];
    const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0;
    return run_seq_tiles(entry, tiles, n_motifs, d_status, stream,
                         [&](int m0, int mm, unsigned blocks, const SeqTile *d_tiles, long long n_tiles, hipStream_t st) {
        hipLaunchKernelGGL(mutation_scan_kernel, dim3(blocks, (unsigned)mm), dim3(kMsThreads), 0, st, d_tiles, n_tiles, d_bases,
                           n_bases, seq_motifs(ms, d_weights, m0, mm), seq_results<ColumnResults>(d_keys, d_sums, m0, mm), W, fwd,
                           d_status);
    });
}
