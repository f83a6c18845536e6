// gfm_sequence_tiles.hpp -- what the tile-based sequence scans share (included at the end of graph_extract.hip ahead of
// gfm_graph_mutation_scan.hpp; the mutation, indel, deletion, substitution and insertion scans and the site distance build on it; it
// uses gfail, GX_TRY, align256, kSeqMotifs and gfm_graph_table_score.hpp's StrandScores and edit_key).  The shuffle null is
// not among them: its entry lists sequences by length class, not by tile.
//   host    the tile table of a call from its seq_offsets (seq_tiles), the length list as a mask (length_mask), the checks of
//           the keys/sums entries' buffers (check_scan_buffers, check_cell_alignment), the capacity of a sum (seq_sum_fits,
//           check_sum_capacity) and the protocol every entry runs around its launches (run_seq_tiles).  Every message carries
//           the entry's name, which the caller passes; the ORDER of an entry's refusals is the entry's own: each calls these
//           in the order its tests pin.
//   device  the tile's bounds check (seq_tile_bad), the staging of a motif's packed table (stage_table), the best key and the
//           sum of one side (SideBest), and the COVER column of the two block scans (cover_head, cover_extend): the indel,
//           deletion, substitution and insertion kernels call them.  The mutation and the site-distance kernel keep their own copies
//           of the first two: they measured slower with these (profiles/sequence_scan_refactor.txt), and their device code
//           is what it was.
namespace {

constexpr int kSeqMaxBlocks = 1 << 16;
constexpr int kSeqBadTile = 1;

// the unit of work: a tile of consecutive offsets of one sequence
struct SeqTile {
    long long begin;              // the sequence's first base in d_bases (and its first row in the results)
    int len, start;               // its length; the tile's first offset
};

// the result pointers of one launch: per motif its keys and its sums
template <class K, class S>
struct SeqResults {
    using Key = K;
    using Sum = S;
    K *keys[kSeqMotifs];
    S *sums[kSeqMotifs];
};
using ColumnResults = SeqResults<unsigned, unsigned long long>;   // [n_bases][columns]: the mutation and the indel scan
using CellResults = SeqResults<uint2, ulonglong2>;                // [n_lengths][n_bases] (COVER, ALT): the two block scans

template <class R>
R seq_results(uint32_t *const *d_keys, uint64_t *const *d_sums, int m0, int mm)
{
    R res = {};
    for (int k = 0; k < mm; ++k) {
        res.keys[k] = reinterpret_cast<typename R::Key *>(d_keys[m0 + k]);
        res.sums[k] = reinterpret_cast<typename R::Sum *>(d_sums[m0 + k]);
    }
    return res;
}

// ---------------------------------------------------------------------------------------------------------------- host
// The sequences of a call and their tiles of `tile` offsets: seq_offsets[0 .. n_seqs] is read, no more (with no sequence
// nothing is read, and seq_offsets may be NULL).
int seq_tiles(const std::string &entry, int tile, int n_seqs, const int64_t *seq_offsets, std::vector<SeqTile> &tiles)
{
    if (n_seqs > 0 && !seq_offsets) return gfail(GFM_ERR_INVALID, entry + ": NULL argument");
    if (n_seqs > 0 && seq_offsets[0] < 0) return gfail(GFM_ERR_INVALID, entry + ": seq_offsets descends below 0");
    for (int v = 0; v < n_seqs; ++v) {
        const long long a = seq_offsets[v], b = seq_offsets[v + 1];
        if (b < a) return gfail(GFM_ERR_INVALID, entry + ": seq_offsets descends at sequence " + std::to_string(v));
        if (b - a > 0x7fffffffll)
            return gfail(GFM_ERR_INVALID, entry + ": sequence " + std::to_string(v) + " holds 2^31 bases or more");
        for (long long s = 0; s < b - a; s += tile) tiles.push_back(SeqTile{a, (int)(b - a), (int)s});
    }
    return GFM_OK;
}

// The lengths of a block scan, strictly ascending within 1 .. max_len (<= 64), as a mask: bit L - 1 for length L.
// lengths[0 .. n_lengths - 1] is read, no more; the longest is the last.
int length_mask(const std::string &entry, int n_lengths, const int32_t *lengths, int max_len, unsigned long long &mask)
{
    if (!lengths) return gfail(GFM_ERR_INVALID, entry + ": NULL argument");
    mask = 0ull;
    for (int i = 0; i < n_lengths; ++i) {
        if (lengths[i] < 1 || lengths[i] > max_len)
            return gfail(GFM_ERR_INVALID, entry + ": length " + std::to_string(lengths[i]) + " is outside 1 .. " +
                                          std::to_string(max_len));
        if (i > 0 && lengths[i] <= lengths[i - 1])
            return gfail(GFM_ERR_INVALID, entry + ": the lengths do not strictly ascend at " + std::to_string(i));
        mask |= 1ull << (lengths[i] - 1);
    }
    return GFM_OK;
}

// the buffers of an entry that writes keys and sums, looked at once there is a tile
int check_scan_buffers(const std::string &entry, const gfm_motif_t *motifs, int n_motifs, const uint64_t *const *d_weights,
                       uint32_t *const *d_keys, uint64_t *const *d_sums, const int32_t *d_status, const uint8_t *d_bases)
{
    if (!motifs || !d_weights || !d_keys || !d_sums || !d_status || !d_bases) return gfail(GFM_ERR_INVALID, entry + ": NULL argument");
    for (int m = 0; m < n_motifs; ++m)
        if (!motifs[m] || !d_weights[m] || !d_keys[m] || !d_sums[m]) return gfail(GFM_ERR_INVALID, "NULL motif / device buffer");
    return GFM_OK;
}

// a cell of CellResults is stored as one 8-byte and one 16-byte word
int check_cell_alignment(const std::string &entry, int n_motifs, uint32_t *const *d_keys, uint64_t *const *d_sums)
{
    for (int m = 0; m < n_motifs; ++m)
        if ((reinterpret_cast<uintptr_t>(d_keys[m]) & 7u) || (reinterpret_cast<uintptr_t>(d_sums[m]) & 15u))
            return gfail(GFM_ERR_INVALID, entry + ": d_keys[m] is 8-byte and d_sums[m] 16-byte aligned");
    return GFM_OK;
}

// the capacity of a sum: a side of `windows` windows (the strands counted), each adding at most max_weight
__host__ constexpr bool seq_sum_fits(uint64_t max_weight, unsigned windows)
{
    return (unsigned __int128)max_weight * windows <= (unsigned __int128)UINT64_MAX;
}
static_assert(seq_sum_fits(UINT64_MAX / 128u, 128u) && !seq_sum_fits(UINT64_MAX / 128u + 1u, 128u), "the bound is exact");
// `detail`: what an entry says behind the number of windows (the block scans name W and the longest length)
int check_sum_capacity(const std::string &entry, uint64_t max_weight, unsigned windows, const std::string &detail)
{
    if (seq_sum_fits(max_weight, windows)) return GFM_OK;
    return gfail(GFM_ERR_INVALID, entry + ": a side holds up to " + std::to_string(windows) + " windows" + detail +
                                  ": with weights up to " + std::to_string((unsigned long long)max_weight) +
                                  " a sum may pass 2^64 - 1");
}

// The protocol of an entry around its launches: the status word cleared, the tile table uploaded (scratch of the call; the
// host copy outlives the upload: the entry waits for the stream), launch(m0, mm, blocks, d_tiles, n_tiles, stream) once per
// kSeqMotifs motifs until an error, the verdict read back.  `launch` enqueues its kernel on the stream it is given with
// grid (blocks, mm) and nothing else.
template <class Launch>
int run_seq_tiles(const std::string &entry, const std::vector<SeqTile> &tiles, int n_motifs, int32_t *d_status, void *stream,
                  Launch launch)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    GX_TRY(hipMemsetAsync(d_status, 0, sizeof(int32_t), st));
    const size_t tile_bytes = align256(sizeof(SeqTile) * tiles.size());
    SeqTile *d_tiles = nullptr;
    GX_TRY(hipMallocAsync(reinterpret_cast<void **>(&d_tiles), tile_bytes, st));
    hipError_t e = hipMemcpyAsync(d_tiles, tiles.data(), sizeof(SeqTile) * tiles.size(), hipMemcpyHostToDevice, st);
    const unsigned blocks = (unsigned)std::min<size_t>(tiles.size(), (size_t)kSeqMaxBlocks);
    for (int m0 = 0; e == hipSuccess && m0 < n_motifs; m0 += kSeqMotifs) {
        launch(m0, std::min(kSeqMotifs, n_motifs - m0), blocks, static_cast<const SeqTile *>(d_tiles), (long long)tiles.size(), st);
        e = hipGetLastError();
    }
    int32_t verdict = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&verdict, d_status, sizeof verdict, hipMemcpyDeviceToHost, st);
    const hipError_t ef = hipFreeAsync(d_tiles, st);
    const hipError_t es = hipStreamSynchronize(st);              // (also on failure: the tile table's host copy is still read)
    if (e == hipSuccess) e = ef;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return gfail(GFM_ERR_HIP, entry + ": " + hipGetErrorString(e));
    if (verdict & kSeqBadTile) return gfail(GFM_ERR_INVALID, entry + ": a tile lies outside its sequence");
    return GFM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- device
// The tile, checked: everything a kernel reads and writes through it lies inside its sequence.  The answer is uniform -- no
// thread stays behind at the caller's `continue` -- and a bad tile is reported in the status word.
__device__ __forceinline__ bool seq_tile_bad(const SeqTile tile, long long n_bases, int *__restrict__ status)
{
    if (tile.begin < 0 || tile.len <= 0 || tile.begin > n_bases - tile.len || tile.start < 0 || tile.start >= tile.len) {
        if (threadIdx.x == 0) atomicOr(status, kSeqBadTile);
        return true;
    }
    return false;
}

// a motif's packed two-strand table (W x 8 words) into LDS, by a workgroup of `threads`
__device__ __forceinline__ void stage_table(unsigned *ftab_s, const unsigned *__restrict__ ftab, int W, int threads)
{
    for (int i = threadIdx.x; i < W * 8; i += threads) ftab_s[i] = ftab[i];
}

// One side of an edit: its best window's key (0: no window yet) and the sum of its windows' weights.  A window goes in with
// its two strands' scores, as StrandScores or as the packed word + | - << 16 the block scans keep in LDS, and with rel,
// its start minus the edit's offset.
struct SideBest {
    unsigned key = 0u;
    unsigned long long sum = 0ull;
    __device__ __forceinline__ void add(StrandScores s, int rel, int forward_only, unsigned long long value)
    {
        key = max(key, edit_key(s.plus, rel, true));
        if (!forward_only) key = max(key, edit_key(s.minus, rel, false));
        sum += value;
    }
    __device__ __forceinline__ void add_packed(unsigned sc, int rel, int forward_only, unsigned long long value)
    {
        add(StrandScores{(int)(sc & 0xffffu), (int)(sc >> 16)}, rel, forward_only, value);
    }
};

// The COVER column of the block scans (deletion, substitution): the windows of x that touch the block (o, L).  wsc_s and
// wref_s hold every scored window's packed scores and REF weight, the window that starts at o + d at [tid + W - 1 + d].
// cover_head: the part every length shares, the starts o - m for m = min(W - 1, o) .. 1.
__device__ __forceinline__ void cover_head(SideBest &cover, const unsigned *wsc_s, const unsigned long long *wref_s, int tid, int W,
                                           int o, int last_start, int forward_only)
{
    for (int m = min(W - 1, o); m >= 1; --m) {
        if (o - m > last_start) continue;
        const int k = tid + W - 1 - m;
        cover.add_packed(wsc_s[k], -m, forward_only, wref_s[k]);
    }
}
// cover_extend: from the listed length before (l_prev, 0 at the first) to L the starts o + l_prev .. o + L - 1 are new; rel
// is relative to o, so the one running side serves every length.
__device__ __forceinline__ void cover_extend(SideBest &cover, const unsigned *wsc_s, const unsigned long long *wref_s, int tid, int W,
                                             int o, int last_start, int l_prev, int L, int forward_only)
{
    for (int d = l_prev; d < L && o + d <= last_start; ++d) {
        const int k = tid + W - 1 + d;
        cover.add_packed(wsc_s[k], d, forward_only, wref_s[k]);
    }
}

// a cell of the block scans: (COVER, ALT) keys as one 8-byte word, their sums as one 16-byte word; no edit: four zeros
__device__ __forceinline__ void store_cell(uint2 *__restrict__ keys, ulonglong2 *__restrict__ sums, long long cell, const SideBest &cover,
                                           const SideBest &alt)
{
    keys[cell] = make_uint2(cover.key, alt.key);
    sums[cell] = make_ulonglong2(cover.sum, alt.sum);
}

}  // namespace
