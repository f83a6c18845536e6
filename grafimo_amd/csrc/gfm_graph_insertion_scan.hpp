// gfm_graph_insertion_scan.hpp -- insertion scan: the insertion of every insert of a list of 1 .. GFM_INSSCAN_MAX_INSERTS given
// blocks of 1 .. GFM_INSSCAN_MAX_LENGTH bases behind every base of a spelled sequence, every window the edit touches scored
// before and after on both strands (included at the end of graph_extract.hip behind the other scans; it shares
// gfm_graph_indel_scan.hpp's bits_from and indel_stride; gfm_sequence_tiles.hpp gives it SeqTile, CellResults, SideBest,
// store_cell, the tile check, the table staging, seq_sum_fits and the host protocol; it uses base_code, view_motif_set,
// SeqMotifs, gfail and gfm_graph_table_score.hpp's strand_scores and walk_value).  It is the indel-scan kernel's insertion
// half with the one inserted base stretched to a block: every window start of x is scored ONCE, the running prefixes of that
// pass are kept, and every window of every edited sequence is put together from at most three stored pieces.
//
// THE RULE (include/grafimo_hip.h states it for the library; tests/insertion_scan_bruteforce.py on the host).  For a sequence
// x of n bases, a motif of width W, a list of K inserts with K in 1 .. 16, every insert I of the list, Li its length in
// 1 .. 64, and every offset o in 0 .. n - 1:
//   Every insert holds A, C, G, T only.  Case is folded, as base_code does.
//   The edit is the insertion of I behind x[o].  Let o' = o + 1 and y = x[:o'] + I + x[o':].
//   This is gfm_graph_query_edits' rule with lr = 0, la = Li at offset o'.
//     REF side (column JUNCTION): the starts s of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).
//     It does not depend on the insert.  It equals the indel scan's JUNCTION column bit for bit.
//     ALT side (column INS): the starts s of y with max(0, o' - W + 1) <= s <= min(o' + Li - 1, n + Li - W).
//     A window that lies wholly inside the insert counts, as the query rule counts it.
//   Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
//   A window that holds a base of x that is not A/C/G/T scores min_val on both strands.
//   An insertion repairs nothing, because it removes no base.  A window that does not reach the N is clean.
//   Per column, the best window by (score descending, s ascending, + before -), as the key
//   ((score + 1) << 8) | ((64 - (s - o')) << 1) | plus, s - o' in -(W - 1) .. -1 for JUNCTION and in -(W - 1) .. Li - 1 for INS.
//   Key 0 means the side has no window.
//   Per column, the exact uint64 sum of w[score] over the side's windows and strands.
//   An insertion before the first base of a sequence is not scanned, as in the indel scan.  An empty sequence has no rows.
//   With the inserts ("A", "C", "G", "T") the INS columns equal the indel scan's INS_A .. INS_T bit for bit.
//   A cell does not depend on the other inserts of the list or on their order.
//
// The algebra is the indel header's: A(e, m) = the packed two-strand sum of the columns 0 .. m - 1 over x[e - m .. e - 1],
// Full[t] = the sum of all W columns over x[t .. t + W - 1]; a position outside the sequence adds 0.  With g = o + 1,
//   B(g, c) = the columns c .. W - 1 over x[g ..] = Full[g - c] - A(g, c)   for 1 <= c <= W - 1
// (Full[g - c] holds the columns 0 .. c - 1 over x[g - c .. g - 1], which is A(g, c): Full contains what is subtracted, so the
// 16-bit halves cannot borrow, as the indel header argues).  Two small tables depend on the insert and the motif alone:
//   H[m] = the sum over j < min(Li, W - m) of ftab[m + j][I[j]], m = 0 .. W - 1      the insert from column m on
//   T[k] = the sum over j < min(Li - k, W) of ftab[j][I[k + j]], k = 0 .. Li - 1     the insert's tail from k on, from column 0
// and the ALT windows of the gap g are
//   start g - m, m = 1 .. W - 1:               A(g, m) + H[m] + (m + Li < W ? B(g, m + Li) : 0)
//                                              exists when m <= g and max(W - m - Li, 0) <= n - g
//   start g + k, k = 0 .. Li - 1, c = Li - k:  T[k] + (c < W ? B(g, c) : 0)
//                                              exists when max(W - c, 0) <= n - g
// Every finished window holds each column once, so both halves come out exact.  Which windows hold a base that is none is
// settled by the wave's three ballots over the tile's codes, exactly as in the indel kernel: dl = the run of real bases that
// ends at g - 1, dr = the run that starts at g; a window is clean when what it needs of x on the left is <= dl and what it
// needs on the right -- the max(.., 0) above -- is <= dr.
//
// Work decomposition: one wavefront per (sequence, tile of GFM_INSSCAN_TILE offsets) from a tile table, checked on the device
// before anything is read through it; grid.y = motif; a workgroup strides over the tiles.  The inserts travel in the kernel's
// arguments as 2-bit codes (16 x 128 bits and 16 lengths), uniform in the kernel.  Once per workgroup the motif's packed table
// (W x 8 words) is staged and H and T of every insert are made from it in LDS; the grid is capped (kInsMaxBlocks) so that with
// many tiles that cost is paid once for several of them.  Per tile:
//   phase 1  the indel kernel's, in a copy of its own: the codes of x[lo - 64 .. lo + 128) to LDS, three ballots; every window
//            start lo - W + 1 .. lo + nt - 1 scored ONCE with W lookups, the running sum after column j stored as
//            A(start + j + 1, j + 1) for the rows lo .. lo + nt; Full, the two strands' scores under the non-base rule and, for
//            the windows inside the sequence, the REF weight w[+ score] + w[- score] are kept;
//   phase 2  a thread per offset o walks JUNCTION once from the stored scores and weights, then per insert the W - 1 + Li ALT
//            windows, each from at most four LDS words and the weight gathers of its two strands.  Two keys and two sums an
//            insert, written with plain 8- and 16-byte stores.  No atomics but the status word's.
// LDS a workgroup: 2 048 (table) + 192 (codes) + 128 x (4 + 4 + 8) (Full, scores, REF weights) + 260 stride (the A table,
// [65 rows][stride = W | 1] words: see the indel header) + 4 x the sum of W + Li over the inserts (H and T):
// 9 548 bytes at W = 19 with the inserts A, C, G, T; 29 380 at W = 64 with 16 inserts of 64 bases.
namespace {

constexpr int kInsTile = GFM_INSSCAN_TILE, kInsThreads = kInsTile, kInsMaxLen = GFM_INSSCAN_MAX_LENGTH;
constexpr int kInsMaxInserts = GFM_INSSCAN_MAX_INSERTS;
constexpr int kInsSide = GFM_MAX_WIDTH;                                             // code_s[i] is x[lo - kInsSide + i]
constexpr int kInsCodes = kInsTile + 2 * kInsSide;                                  // 192: three turns of the wave
constexpr int kInsWindows = (kInsTile + GFM_MAX_WIDTH - 1 + 15) & ~15;              // 128
constexpr unsigned kInsMaxBlocks = 4096;                  // a workgroup's H and T serve its several tiles beyond this many
static_assert(kInsTile == 64 && GFM_MAX_WIDTH == 64, "the non-base bitmap is three 64-bit ballots, a lane reads 64 bits of it");
static_assert(kInsMaxLen == 64 && kInsMaxLen == GFM_QUERY_MAX_ALLELE, "an insert's codes are 128 bits; the key's field holds every start");

// the inserts of a call: insert i has len[i] bases, base j as the 2-bit base_code in bits 2 j .. 2 j + 1 of (hi[i], lo[i])
struct InsertList {
    unsigned long long lo[kInsMaxInserts], hi[kInsMaxInserts];
    int n;
    unsigned char len[kInsMaxInserts];
};

// the words of H and T of all inserts
__host__ constexpr size_t insscan_table_words(int W, int n_inserts, int total_length)
{
    return (size_t)n_inserts * (size_t)W + (size_t)total_length;
}
__host__ constexpr size_t insscan_lds_bytes(int W, int n_inserts, int total_length)
{
    return sizeof(unsigned) * ((size_t)(kInsTile + 1) * (size_t)indel_stride(W) + insscan_table_words(W, n_inserts, total_length));
}

// the capacity of a sum: an ALT side has at most W + lmax - 1 windows, each once per strand
__host__ constexpr unsigned insscan_side_windows(int W, int lmax) { return 2u * (unsigned)(W + lmax - 1); }
__host__ constexpr bool insscan_sum_fits(uint64_t max_weight, int W, int lmax)
{
    return seq_sum_fits(max_weight, insscan_side_windows(W, lmax));
}
static_assert(insscan_sum_fits(UINT64_MAX / 254u, 64, 64) && !insscan_sum_fits(UINT64_MAX / 254u + 1u, 64, 64), "the bound is exact");

__device__ __forceinline__ unsigned insert_code(unsigned long long lo, unsigned long long hi, int j)
{
    return (unsigned)((j < 32 ? lo >> (2 * j) : hi >> (2 * (j - 32))) & 3ull);
}

__global__ void __launch_bounds__(kInsThreads)
insertion_scan_kernel(const SeqTile *__restrict__ tiles, long long n_tiles, const uint8_t *__restrict__ bases, long long n_bases,
                      SeqMotifs mt, CellResults res, int W, InsertList ins, int forward_only, int *__restrict__ status)
{
    extern __shared__ unsigned a_s[];                             // A(lo + row, m) at [row * stride + m - 1], m = 1 .. W; then H, T
    __shared__ unsigned ftab_s[GFM_MAX_WIDTH * 8];
    __shared__ unsigned long long wref_s[kInsWindows];
    __shared__ unsigned wsum_s[kInsWindows];
    __shared__ unsigned wsc_s[kInsWindows];                       // + score | - score << 16, under the non-base rule
    __shared__ unsigned char code_s[kInsCodes];
    const int mi = blockIdx.y, tid = threadIdx.x;
    stage_table(ftab_s, mt.ftab[mi], W, kInsThreads);
    const unsigned long long *__restrict__ wtab = mt.wtab[mi];
    uint2 *__restrict__ keys = res.keys[mi];
    ulonglong2 *__restrict__ sums = res.sums[mi];
    const int min_val = mt.min_val[mi];
    const int stride = indel_stride(W);
    unsigned *ht_s = a_s + (kInsTile + 1) * stride;               // insert i: H[0 .. W - 1], then T[0 .. Li - 1]
    __syncthreads();                                              // (the table is staged)
    for (int i = 0, base = 0; i < ins.n; ++i) {
        const int li = ins.len[i];
        const unsigned long long lo = ins.lo[i], hi = ins.hi[i];
        for (int e = tid; e < W + li; e += kInsThreads) {
            unsigned sum = 0u;
            if (e < W) {                                          // H[e]
                for (int j = 0; j < min(li, W - e); ++j) sum += ftab_s[(e + j) * 8 + insert_code(lo, hi, j)];
            } else {                                              // T[e - W]
                const int k = e - W;
                for (int j = 0; j < min(li - k, W); ++j) sum += ftab_s[j * 8 + insert_code(lo, hi, k + j)];
            }
            ht_s[base + e] = sum;
        }
        base += W + li;
    }
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const SeqTile tile = tiles[t];
        if (seq_tile_bad(tile, n_bases, status)) continue;
        const uint8_t *__restrict__ x = bases + tile.begin;
        const int len = tile.len, lo = tile.start, nt = min(kInsTile, len - lo);
        __syncthreads();                                          // (H and T are made; the last tile's rows are read)
        // ---- the codes of x[lo - 64 .. lo + 128) and which of them are no base: nb[k] bit i is position lo - 64 + 64 k + i
        unsigned long long nb[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const long long p = (long long)lo - kInsSide + k * 64 + tid;
            const unsigned c = (p >= 0 && p < len) ? base_code(x[p]) : 4u;
            code_s[k * 64 + tid] = (unsigned char)c;
            nb[k] = __builtin_amdgcn_ballot_w64((c >> 2) != 0u);
        }
        __syncthreads();
        // ---- phase 1: every window start lo - W + 1 .. lo + nt - 1 once; window k starts at lo - W + 1 + k
        for (int k = tid; k < nt + W - 1; k += kInsThreads) {
            const unsigned char *c = code_s + (k + kInsSide - W + 1);
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
            const StrandScores sc = strand_scores(w, min_val);
            wsum_s[k] = w.sum;
            wsc_s[k] = (unsigned)sc.plus | ((unsigned)sc.minus << 16);
            wref_s[k] = (s >= 0 && s <= (long long)len - W) ? walk_value(wtab, w, min_val, forward_only) : 0ull;
        }
        __syncthreads();
        // ---- phase 2: a thread per offset o; the gap lies before g = o + 1
        if (tid < nt) {
            const int o = lo + tid, g = o + 1, r = len - g;       // (r: the bases of x behind the gap)
            const unsigned long long before = bits_from(nb[0], nb[1], tid);          // bit 63 is o - 1, bit 0 is o - 64
            const unsigned long long from = bits_from(nb[1], nb[2], tid);            // bit 0 is o
            const unsigned long long behind = from >> 1;
            const int dl = (from & 1ull) ? 0 : (before ? __builtin_clzll(before) : 64) + 1;     // the run that ends at o
            const int dr = behind ? __builtin_ctzll(behind) : 64;                               // the run that starts at g
            // JUNCTION: the windows of x that start at g - m and reach x[g], m = 1 .. W - 1
            SideBest junction;
            for (int m = 1; m <= min(W - 1, g); ++m) {
                if (W - m > r) continue;
                const int k = tid + W - m;                        // the window start g - m
                junction.add_packed(wsc_s[k], -m, forward_only, wref_s[k]);
            }
            const unsigned *a_g = a_s + (tid + 1) * stride;       // A(g, m) = a_g[m - 1]
            const unsigned *full_g = wsum_s + (tid + W);          // Full[g - c] = full_g[-c]
            long long cell = tile.begin + o;                      // of the first insert; the next is n_bases further
            const unsigned *h_s = ht_s;
            for (int i = 0; i < ins.n; ++i, cell += n_bases) {
                const int li = ins.len[i];
                const unsigned *t_s = h_s + W;
                SideBest alt;
                // the windows that start in x: x[g - m .. g - 1], the insert from column m on, then x from g on
                for (int m = min(W - 1, g); m >= 1; --m) {
                    const int c = m + li, need = max(W - c, 0);   // (need: the bases of x behind the gap)
                    if (need > r) continue;
                    unsigned sum = a_g[m - 1] + h_s[m];
                    if (c < W) sum += full_g[-c] - a_g[c - 1];
                    const WindowSum w{sum, (m <= dl && need <= dr) ? 0u : 1u};
                    alt.add(strand_scores(w, min_val), -m, forward_only, walk_value(wtab, w, min_val, forward_only));
                }
                // the windows that start in the insert: its tail from k on, then x from g on
                for (int k = 0; k < li; ++k) {
                    const int c = li - k, need = max(W - c, 0);
                    if (need > r) break;                          // (and every later start needs more)
                    unsigned sum = t_s[k];
                    if (c < W) sum += full_g[-c] - a_g[c - 1];
                    const WindowSum w{sum, need <= dr ? 0u : 1u};
                    alt.add(strand_scores(w, min_val), k, forward_only, walk_value(wtab, w, min_val, forward_only));
                }
                store_cell(keys, sums, cell, junction, alt);
                h_s = t_s + li;
            }
        }
    }
}

// The inserts of a call, checked and packed: insert_offsets[0 .. n_inserts] and insert_bases[0 .. insert_offsets[n_inserts] - 1]
// are read, no more (the bases only once every length is known to lie in 1 .. 64) -> the list, the longest and the total length.
int insert_list(const std::string &entry, int n_inserts, const int32_t *insert_offsets, const uint8_t *insert_bases, InsertList &list,
                int &lmax, int &total)
{
    if (!insert_offsets || !insert_bases) return gfail(GFM_ERR_INVALID, entry + ": NULL argument");
    if (insert_offsets[0] != 0) return gfail(GFM_ERR_INVALID, entry + ": insert_offsets starts at 0");
    for (int i = 0; i < n_inserts; ++i)
        if (insert_offsets[i + 1] < insert_offsets[i])
            return gfail(GFM_ERR_INVALID, entry + ": insert_offsets descends at insert " + std::to_string(i));
    list = InsertList{};
    list.n = n_inserts;
    lmax = 0;
    for (int i = 0; i < n_inserts; ++i) {
        const long long li = (long long)insert_offsets[i + 1] - insert_offsets[i];
        if (li < 1 || li > kInsMaxLen)
            return gfail(GFM_ERR_INVALID, entry + ": the length " + std::to_string(li) + " of insert " + std::to_string(i) +
                                          " is outside 1 .. " + std::to_string(kInsMaxLen));
        list.len[i] = (unsigned char)li;
        lmax = std::max(lmax, (int)li);
    }
    total = insert_offsets[n_inserts];
    for (int i = 0; i < n_inserts; ++i)
        for (int j = 0; j < list.len[i]; ++j) {
            const unsigned c = insert_bases[insert_offsets[i] + j], up = c & ~0x20u;
            if (up != 'A' && up != 'C' && up != 'G' && up != 'T')
                return gfail(GFM_ERR_INVALID, entry + ": base " + std::to_string(j) + " of insert " + std::to_string(i) +
                                              " is not one of ACGTacgt");
            const unsigned long long code = (c >> 1) & 3u;        // base_code of a base: A 0, C 1, T 2, G 3
            (j < 32 ? list.lo[i] : list.hi[i]) |= code << (2 * (j & 31));
        }
    return GFM_OK;
}

}  // namespace

GFM_API int gfm_sequence_insertion_scan(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                        uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                                        int32_t n_inserts, const int32_t *insert_offsets, const uint8_t *insert_bases, uint32_t flags,
                                        uint32_t *const *d_keys, uint64_t *const *d_sums, int32_t *d_status, void *stream)
{
    const std::string entry = "gfm_sequence_insertion_scan";
    if (n_motifs < 1 || n_seqs < 0 || n_inserts < 1 || n_inserts > kInsMaxInserts) return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    // ---- the inserts, checked with no sequence too
    InsertList list;
    int lmax = 0, total = 0;
    if (const int rc = insert_list(entry, n_inserts, insert_offsets, insert_bases, list, lmax, total)) return rc;
    if (n_seqs == 0) return GFM_OK;
    std::vector<SeqTile> tiles;
    if (const int rc = seq_tiles(entry, kInsTile, n_seqs, seq_offsets, tiles)) return rc;
    if (tiles.empty()) return GFM_OK;
    if (const int rc = check_scan_buffers(entry, motifs, n_motifs, d_weights, d_keys, d_sums, d_status, d_bases)) return rc;
    if (const int rc = check_cell_alignment(entry, n_motifs, d_keys, d_sums)) return rc;
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::PackedTable, ms)) return rc;
    const int W = ms.W;
    if (const int rc = check_sum_capacity(entry, max_weight, insscan_side_windows(W, lmax),
                                          " (W = " + std::to_string(W) + ", longest insert " + std::to_string(lmax) + ")"))
        return rc;
    const long long n_bases = seq_offsets[n_seqs];
    const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0;
    return run_seq_tiles(entry, tiles, n_motifs, d_status, stream,
                         [&](int m0, int mm, unsigned blocks, const SeqTile *d_tiles, long long n_tiles, hipStream_t st) {
        hipLaunchKernelGGL(insertion_scan_kernel, dim3(std::min(blocks, kInsMaxBlocks), (unsigned)mm), dim3(kInsThreads),
                           insscan_lds_bytes(W, n_inserts, total), st, d_tiles, n_tiles, d_bases, n_bases,
                           seq_motifs(ms, d_weights, m0, mm), seq_results<CellResults>(d_keys, d_sums, m0, mm), W, list, fwd, d_status);
    });
}
