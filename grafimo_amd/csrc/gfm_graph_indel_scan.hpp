// gfm_graph_indel_scan.hpp -- indel scan: the deletion of every base of a spelled sequence and the insertion of every base
// behind it, every window the edit touches scored before and after on both strands (included at the end of graph_extract.hip
// behind gfm_graph_mutation_scan.hpp; gfm_sequence_tiles.hpp gives it SeqTile, ColumnResults, SideBest, the tile check, the
// table staging and the host protocol; it uses base_code, view_motif_set, SeqMotifs, gfail and gfm_graph_table_score.hpp's
// strand_scores and walk_value).
// Where query_edits_kernel scores the up to W windows of ONE edited sequence with W lookups each, this kernel scores every
// window start of a sequence ONCE, keeps the running prefixes of that one pass, and makes every window of all 5 n edited
// sequences from two of the pieces: an edited window is the head of one scored window and the tail of its neighbour.
//
// THE RULE (include/grafimo_hip.h states it for the library; tests/indel_scan_bruteforce.py on the host).  For a sequence x of
// n bases, a motif of width W, and every offset o in 0 .. n - 1:
//   Deletion of x[o].  y = x[:o] + x[o+1:].  This is gfm_graph_query_edits' rule with lr = 1, la = 0 at offset o.
//     REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).  This is exactly the mutation
//     scan's REF column.
//     ALT side (column DEL): the starts of y across the junction, max(0, o - W + 1) <= s <= min(o - 1, n - 1 - W).
//   Insertion of b in A, C, G, T behind x[o].  y = x[:o+1] + b + x[o+1:].  This is the query rule with lr = 0, la = 1 at offset
//   o' = o + 1.
//     REF side (column JUNCTION): the starts of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).
//     ALT side (columns INS_A, INS_C, INS_G, INS_T): the starts of y with max(0, o' - W + 1) <= s <= min(o', n + 1 - W).
//   Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
//   A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
//   Per column, the best window by (score descending, s ascending, + before -), as the key
//   ((score + 1) << 8) | ((64 - rel) << 1) | plus, rel = s - o for COVER and DEL, rel = s - (o + 1) for JUNCTION and INS_*: the
//   values a gfm_edit_record_t of the same edit holds.  Key 0 means the side has no window.
//   Per column, the exact uint64 sum of w[score] over the side's windows and strands.
//   A deleted N can repair its windows.  An N elsewhere leaves its windows at min_val.  An insertion before the first base of a
//   sequence is not scanned: every row has the base it is anchored to, as a VCF row has.  An empty sequence has no rows.
//
// The algebra.  Pre[t][m] = the packed two-strand sum of ftab[j][x[t + j]] over j < m, Full[t] = Pre[t][W]; a position outside
// the sequence adds nothing (the table holds 0 for every code that is no base).  Written by where a prefix ENDS,
// A(e, m) = Pre[e - m][m] -- the columns 0 .. m - 1 over x[e - m .. e - 1] --,
//   the deletion's window m = 1 .. W - 1 (start o - m):       A(o, m) + Full[o - m + 1] - A(o + 1, m)
//   the insertion's window m = 0 .. W - 1 (start o + 1 - m):  A(o + 1, m) + ftab[m][b] + Full[o - m] - A(o + 1, m + 1)
// so the thread of offset o needs the rows e = o and e = o + 1 of A, and the Full sums it needs for COVER anyway.  The words
// are added modulo 2^32 and every finished window holds each column once, so both halves come out exact: Full contains what
// is subtracted, and a motif's column maxima total below 2^16.  o - m may be -1 (the insertion's window that starts at 0):
// position -1 adds 0 to both terms that hold it.
// Which windows hold a base that is none is NOT carried through the algebra: the wave's three ballots over the tile's codes
// are a 192-bit bitmap in scalar registers, from which a lane takes the run of real bases that ends at o - 1 (dl), at o (dl0)
// and that starts at o + 1 (dr), each with one count of leading or trailing zeros; the deletion's window m is clean when
// m <= dl and W - m <= dr, the insertion's when m <= dl0 and W - 1 - m <= dr, a window of x when m <= dl, x[o] is a base and
// W - 1 - m <= dr.
//
// Work decomposition: as mutation_scan_kernel's -- the unit is a (sequence, tile of GFM_INDELSCAN_TILE offsets) pair from a
// tile table (scratch of the call), checked on the device before anything is read through it; grid.y = motif, a workgroup
// strides over the tiles; a workgroup is ONE wavefront and stages the motif's packed table (W x 8 words) once.  Per tile:
//   phase 1  the base codes of the tile and 64 positions on each side go to LDS (outside the sequence: no base), the ballots
//            are taken; every window start t = lo - W + 1 .. lo + nt - 1 is scored ONCE with W lookups, and on the way the
//            running sum after column j is stored as A(t + j + 1, j + 1) when that row belongs to the tile (rows lo .. lo + nt);
//            Full[t] and, for the windows inside the sequence, the REF weight w[+ score] + w[- score] are kept as well;
//   phase 2  a thread per offset o walks m = 0 .. W - 1: the window start o - m serves COVER and JUNCTION (stored sum and
//            weight), the deletion's window m and the four insertions' windows m, from 2 words of A, 1 Full, 1 weight and the
//            table row m: 7 keys and 7 sums in registers, written with plain stores.  No atomics but the status word's.
// The A table is [65 rows][stride = W | 1] words in dynamic LDS: an odd stride puts the 32 lanes of a read of A(o, m) --
// addresses o * stride + m -- and of phase 1's write of A(t + j + 1, j + 1) -- (t + j) * stride + j -- on 32 different banks.
// LDS a workgroup: 2 048 (table) + 192 (codes) + 128 x (4 + 8) (Full, REF weights) + 260 stride: 8 716 bytes at W = 19,
// 20 676 at W = 64 -- 18 and 7 one-wave workgroups a CU (DESIGN 3.21 says why that is enough).
namespace {

constexpr int kIsTile = GFM_INDELSCAN_TILE, kIsThreads = kIsTile;
constexpr int kIsSide = GFM_MAX_WIDTH;                                              // code_s[i] is x[lo - kIsSide + i]
constexpr int kIsCodes = kIsTile + 2 * kIsSide;                                     // 192: three turns of the wave
constexpr int kIsWindows = (kIsTile + GFM_MAX_WIDTH - 1 + 15) & ~15;                // 128
static_assert(kIsTile == 64 && GFM_MAX_WIDTH == 64, "the non-base bitmap is three 64-bit ballots, a lane reads 64 bits of it");

__host__ __device__ constexpr int indel_stride(int W) { return W | 1; }
__host__ __device__ constexpr size_t indel_lds_bytes(int W) { return sizeof(unsigned) * (size_t)(kIsTile + 1) * (size_t)indel_stride(W); }

// bits sh .. sh + 63 of the 128-bit word (hi, lo), sh in 0 .. 63
__device__ __forceinline__ unsigned long long bits_from(unsigned long long lo, unsigned long long hi, int sh)
{
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

__global__ void __launch_bounds__(kIsThreads)
indel_scan_kernel(const SeqTile *__restrict__ tiles, long long n_tiles, const uint8_t *__restrict__ bases, long long n_bases,
                  SeqMotifs mt, ColumnResults res, int W, int forward_only, int *__restrict__ status)
{
    extern __shared__ unsigned a_s[];                             // A(lo + row, m) at [row * stride + m - 1], m = 1 .. W
    __shared__ unsigned ftab_s[GFM_MAX_WIDTH * 8];
    __shared__ unsigned long long wref_s[kIsWindows];
    __shared__ unsigned wsum_s[kIsWindows];
    __shared__ unsigned char code_s[kIsCodes];
    const int mi = blockIdx.y, tid = threadIdx.x;
    stage_table(ftab_s, mt.ftab[mi], W, kIsThreads);
    const unsigned long long *__restrict__ wtab = mt.wtab[mi];
    unsigned *__restrict__ keys = res.keys[mi];
    unsigned long long *__restrict__ sums = res.sums[mi];
    const int min_val = mt.min_val[mi];
    const int stride = indel_stride(W);
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const SeqTile tile = tiles[t];
        if (seq_tile_bad(tile, n_bases, status)) continue;
        const uint8_t *__restrict__ x = bases + tile.begin;
        const int len = tile.len, lo = tile.start, nt = min(kIsTile, len - lo);
        __syncthreads();                                          // (the table is staged; the last tile's rows are read)
        // ---- the codes of x[lo - 64 .. lo + 128) and which of them are no base: nb[k] bit i is position lo - 64 + 64 k + i
        unsigned long long nb[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const long long p = (long long)lo - kIsSide + k * 64 + tid;
            const unsigned c = (p >= 0 && p < len) ? base_code(x[p]) : 4u;
            code_s[k * 64 + tid] = (unsigned char)c;
            nb[k] = __builtin_amdgcn_ballot_w64((c >> 2) != 0u);
        }
        __syncthreads();
        // ---- phase 1: every window start lo - W + 1 .. lo + nt - 1 once; window k starts at lo - W + 1 + k
        for (int k = tid; k < nt + W - 1; k += kIsThreads) {
            const unsigned char *c = code_s + (k + kIsSide - W + 1);
            const int row0 = k - W + 2;                           // the row of the prefix that ends behind column 0
            WindowSum w{0u, 0u};
            for (int j = 0; j < W; ++j) {
                const unsigned cj = c[j];
                w.sum += ftab_s[j * 8 + cj];
                w.bad += cj >> 2;
                const int row = row0 + j;
                if (row >= 0 && row <= nt) a_s[row * stride + j] = w.sum;           // A(start + j + 1, j + 1)
            }
            const long long s = (long long)lo - W + 1 + k;
            wsum_s[k] = w.sum;
            wref_s[k] = (s >= 0 && s <= (long long)len - W) ? walk_value(wtab, w, min_val, forward_only) : 0ull;
        }
        __syncthreads();
        // ---- phase 2: a thread per offset; m = the column of the window that holds x[o], the junction or the inserted base
        if (tid < nt) {
            const int o = lo + tid, r = len - 1 - o;              // (r: the bases behind o)
            const unsigned long long before = bits_from(nb[0], nb[1], tid);          // bit 63 is o - 1, bit 0 is o - 64
            const unsigned long long from = bits_from(nb[1], nb[2], tid);            // bit 0 is o
            const unsigned long long behind = from >> 1;
            const bool xbad = (from & 1ull) != 0ull;
            const int dl = before ? __builtin_clzll(before) : 64;
            const int dr = behind ? __builtin_ctzll(behind) : 64;
            const int dl0 = xbad ? 0 : dl + 1;
            const unsigned *a_o = a_s + tid * stride, *a_o1 = a_o + stride;         // A(o, m) = a_o[m - 1], A(o + 1, m) = a_o1[m - 1]
            SideBest cover, del, junction, ins[4];
            unsigned a1 = 0u, full_next = 0u;                     // A(o + 1, m) and Full[o - m + 1], from the turn before
            for (int m = 0; m < W; ++m) {
                const int k = tid + W - 1 - m;                    // the window start o - m
                const unsigned full = wsum_s[k], a1n = a_o1[m];
                const bool tail_x = W - 1 - m <= r;               // x has the W - 1 - m bases behind o
                if (m <= o && tail_x) {                           // COVER, and JUNCTION when the window reaches o + 1
                    const WindowSum w{full, (m <= dl && !xbad && W - 1 - m <= dr) ? 0u : 1u};
                    const StrandScores rs = strand_scores(w, min_val);
                    const unsigned long long v = wref_s[k];
                    cover.add(rs, -m, forward_only, v);
                    if (m <= W - 2) junction.add(rs, -m - 1, forward_only, v);
                }
                if (m >= 1 && m <= o && W - m <= r) {             // DEL: x[o - m .. o - 1] and x[o + 1 .. o + W - m]
                    const WindowSum w{a_o[m - 1] + full_next - a1, (m <= dl && W - m <= dr) ? 0u : 1u};
                    del.add(strand_scores(w, min_val), -m, forward_only, walk_value(wtab, w, min_val, forward_only));
                }
                if (m <= o + 1 && tail_x) {                       // INS_*: x[o + 1 - m .. o], b, x[o + 1 .. o + W - 1 - m]
                    const unsigned rest = a1 + full - a1n, invalid = (m <= dl0 && W - 1 - m <= dr) ? 0u : 1u;
#pragma unroll
                    for (unsigned b = 0; b < 4; ++b) {
                        const WindowSum wb{rest + ftab_s[m * 8 + b], invalid};
                        ins[b].add(strand_scores(wb, min_val), -m, forward_only, walk_value(wtab, wb, min_val, forward_only));
                    }
                }
                a1 = a1n;
                full_next = full;
            }
            // the columns COVER, DEL, JUNCTION, INS_A, INS_C, INS_G, INS_T; the codes are A 0, C 1, T 2, G 3
            unsigned *kq = keys + (tile.begin + o) * 7;
            unsigned long long *sq = sums + (tile.begin + o) * 7;
            kq[0] = cover.key; kq[1] = del.key; kq[2] = junction.key;
            kq[3] = ins[0].key; kq[4] = ins[1].key; kq[5] = ins[3].key; kq[6] = ins[2].key;
            sq[0] = cover.sum; sq[1] = del.sum; sq[2] = junction.sum;
            sq[3] = ins[0].sum; sq[4] = ins[1].sum; sq[5] = ins[3].sum; sq[6] = ins[2].sum;
        }
    }
}

}  // namespace

GFM_API int gfm_sequence_indel_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                    uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                                    uint32_t flags, uint32_t *const *d_keys, uint64_t *const *d_sums, int32_t *d_status,
                                    void *stream)
{
    const std::string entry = "gfm_sequence_indel_scan";
    if (n_motifs < 1 || n_seqs < 0) return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    if (n_seqs == 0) return GFM_OK;
    std::vector<SeqTile> tiles;
    if (const int rc = seq_tiles(entry, kIsTile, n_seqs, seq_offsets, tiles)) return rc;
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
        hipLaunchKernelGGL(indel_scan_kernel, dim3(blocks, (unsigned)mm), dim3(kIsThreads), indel_lds_bytes(W), st, d_tiles, n_tiles,
                           d_bases, n_bases, seq_motifs(ms, d_weights, m0, mm), seq_results<ColumnResults>(d_keys, d_sums, m0, mm), W,
                           fwd, d_status);
    });
}
