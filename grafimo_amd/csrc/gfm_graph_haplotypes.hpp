// gfm_graph_haplotypes.hpp -- the per-haplotype hit matrix: for every region of the last fused scoring call and every
// haplotype of the graph, how many of the region's hit rows the haplotype carries and the best (highest) scaled score among
// them.  (Included at the end of graph_extract.hip: it reads the hit entries of gfm_graph_score[_multi] and the plan's tile
// table, and re-derives their walks with the function graph_annotate_kernel uses: hit_walk.)
//
// A haplotype CARRIES a row when it is in the set whose size is the row's haplotype_frequency: the AND of the bitsets of
// the walk's allele constraints.  graph_annotate_kernel keeps only the popcount of that set; here the set itself is kept.
//
// Work decomposition (no atomics in the inner loops; integer counts and maxima do not depend on order):
//   1. hh_region_count_kernel / hh_scatter_kernel: the entries that pass the cutoff grouped by region -- a count per
//      region, an exclusive scan (hipcub), a scatter of entry indices (order inside a region is arbitrary).
//   2. per batch of the grouped entries whose masks fit the scratch budget:
//      hh_mask_kernel -- a WAVEFRONT per entry re-derives the walk's constraints (hit_walk) and its lanes write
//      the AND of the bitsets, a 64-bit word per lane, the tail bits beyond n_hap cleared;
//      hh_reduce_kernel -- a workgroup per (region, 256 haplotypes), a thread per haplotype: over the region's entries of the
//      batch the 64 lanes of a wave read the SAME mask word (a broadcast load), test their bit, count and take the maximum
//      score, then add to / raise the thread's own cell of the outputs (zeroed / set to -1 before the first batch).
namespace {

constexpr int kHhReduceThreads = 256;
constexpr int kHhScanThreads = 256;
constexpr int kHhMaskBlocks = 8192;               // wavefronts of hh_mask_kernel: entries dealt over the grid, as annotate's
constexpr int kHhRegionChunk = 1 << 22;           // regions per hh_reduce_kernel launch (grid.x)
constexpr long long kHhDefaultScratch = 256ll << 20;

__device__ __forceinline__ bool hh_kept(const GraphHit &h, const int *d_cutoff) { return !d_cutoff || h.score >= *d_cutoff; }

__device__ __forceinline__ int hh_region(const Tile *__restrict__ tiles, int n_tiles, const GraphHit &h)
{
    return hit_tile(tiles, n_tiles, h).region;
}

// cnt[r] += entries of region r that pass the cutoff (--qvalueT; none: all of them, as in annotate)
__global__ void __launch_bounds__(kHhScanThreads)
hh_region_count_kernel(const Tile *__restrict__ tiles, int n_tiles, const GraphHit *__restrict__ hits,
                       const unsigned long long *__restrict__ hit_count, long long hit_cap, const int *__restrict__ d_cutoff,
                       int n_regions, int *__restrict__ cnt)
{
    const long long n = min((long long)*hit_count, hit_cap);
    for (long long i = (long long)blockIdx.x * kHhScanThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kHhScanThreads) {
        const GraphHit h = hits[i];
        if (!hh_kept(h, d_cutoff)) continue;
        const int r = hh_region(tiles, n_tiles, h);
        if ((unsigned)r < (unsigned)n_regions) atomicAdd(&cnt[r], 1);
    }
}

// perm[cursor[r]++] = entry, for the same entries (cursor: the exclusive scan of the counts)
__global__ void __launch_bounds__(kHhScanThreads)
hh_scatter_kernel(const Tile *__restrict__ tiles, int n_tiles, const GraphHit *__restrict__ hits,
                  const unsigned long long *__restrict__ hit_count, long long hit_cap, const int *__restrict__ d_cutoff,
                  int n_regions, int *__restrict__ cursor, int *__restrict__ perm)
{
    const long long n = min((long long)*hit_count, hit_cap);
    for (long long i = (long long)blockIdx.x * kHhScanThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kHhScanThreads) {
        const GraphHit h = hits[i];
        if (!hh_kept(h, d_cutoff)) continue;
        const int r = hh_region(tiles, n_tiles, h);
        if ((unsigned)r < (unsigned)n_regions) perm[atomicAdd(&cursor[r], 1)] = (int)i;
    }
}

// The carrier set of one hit entry into out[0 .. hw): the AND of the bitsets of the walk's constraints (hit_walk), a word
// per lane -- count_by_bitsets_wave keeping the words instead of their popcounts.  No such walk: no carriers.
__device__ __forceinline__ void hh_mask_hit(const GraphDev &g, int W, const Tile *__restrict__ tiles, int n_tiles,
                                            const GraphHit &hit, unsigned long long *__restrict__ out)
{
    const Tile t = hit_tile(tiles, n_tiles, hit);
    const bool found = hit_walk<false>(g, W, t, hit, nullptr, [&](int n, auto at, long long, bool) {
        for (int word = threadIdx.x & 63; word < g.hw; word += 64) out[word] = carrier_word<true>(g, n, at, word);
    });
    if (!found)
        for (int word = threadIdx.x; word < g.hw; word += 64) out[word] = 0ull;
}

// a wavefront per grouped entry i in [b0, min(b1, kept)): its mask into masks[i - b0][hw], its score into bscore[i - b0]
__global__ void __launch_bounds__(64)
hh_mask_kernel(GraphDev g, int W, const Tile *__restrict__ tiles, int n_tiles, const GraphHit *__restrict__ hits,
               const int *__restrict__ perm, const int *__restrict__ off, int n_regions, long long b0, long long b1,
               unsigned long long *__restrict__ masks, int *__restrict__ bscore)
{
    const long long n = min(b1, (long long)off[n_regions]);
    for (long long i = b0 + (long long)blockIdx.x; i < n; i += (long long)gridDim.x) {
        __syncthreads();                    // (the last entry's LDS caches are no longer read)
        const GraphHit hit = hits[perm[i]];
        hh_mask_hit(g, W, tiles, n_tiles, hit, masks + (size_t)(i - b0) * g.hw);
        if (threadIdx.x == 0) bscore[i - b0] = hit.score;
    }
}

// workgroup per (region r0 + blockIdx.x, haplotypes blockIdx.y * 256 ..): the region's entries of the batch
__global__ void __launch_bounds__(kHhReduceThreads)
hh_reduce_kernel(const unsigned long long *__restrict__ masks, const int *__restrict__ bscore, const int *__restrict__ off,
                 int n_regions, int r0, int n_hap, int hw, long long b0, long long b1, int *__restrict__ counts,
                 int *__restrict__ best)
{
    const int r = r0 + (int)blockIdx.x;
    const long long kept = off[n_regions];
    const long long lo = max((long long)off[r], b0), hi = min(min((long long)off[r + 1], b1), kept);
    const int h = (int)blockIdx.y * kHhReduceThreads + (int)threadIdx.x;
    if (lo >= hi || h >= n_hap) return;
    const int word = h >> 6;
    const unsigned long long bit = 1ull << (h & 63);
    const unsigned long long *m = masks + (size_t)(lo - b0) * hw + word;
    const int *sc = bscore + (lo - b0);
    int c = 0, b = -1;
    for (long long i = 0; i < hi - lo; ++i)
        if (m[(size_t)i * hw] & bit) { ++c; b = max(b, sc[i]); }
    if (c) {
        const size_t at = (size_t)r * n_hap + h;
        counts[at] += c;
        best[at] = max(best[at], b);
    }
}

}  // namespace

GFM_API int gfm_graph_haplotype_hits(gfm_graph_t g, const void *d_hits, const uint64_t *d_hit_count, int64_t hit_capacity,
                                     const int32_t *d_cutoff, int32_t n_regions, int32_t *d_counts, int32_t *d_best,
                                     int64_t scratch_bytes, void *stream)
{
    if (const int rc = check_hit_list(g, "gfm_graph_haplotype_hits", d_hits, d_hit_count, hit_capacity)) return rc;
    if (!has_haplotypes(*g)) return fail_no_haplotypes("gfm_graph_haplotype_hits");
    FusedPlan *P = g->plan;
    if (n_regions < 0 || (size_t)n_regions != P->f_starts.size())
        return gfail(GFM_ERR_INVALID, "gfm_graph_haplotype_hits: n_regions = " + std::to_string(n_regions) + " but the last "
                                      "gfm_graph_score call had " + std::to_string(P->f_starts.size()) + " regions");
    if (n_regions && (!d_counts || !d_best)) return gfail(GFM_ERR_INVALID, "bad argument");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int H = g->dev.n_hap, hw = g->dev.hw;
    const size_t cells = (size_t)n_regions * (size_t)H;
    if (const int rc = g->serialise(st)) return rc;
    if (cells) {
        GX_TRY(hipMemsetAsync(d_counts, 0, cells * sizeof(int32_t), st));
        GX_TRY(hipMemsetAsync(d_best, 0xff, cells * sizeof(int32_t), st));          // -1: no row
    }
    if (hit_capacity == 0 || P->f_n_tiles == 0 || n_regions == 0) return g->called(st);
    // the masks of a batch and its scores within the budget; a region's entries may span batches (the reduction adds up)
    const long long budget = scratch_bytes > 0 ? scratch_bytes : kHhDefaultScratch;
    const long long per_entry = 8ll * hw + 4;
    const long long batch = std::min<long long>(std::max(1ll, budget / per_entry), hit_capacity);
    size_t cub_bytes = 0;
    GX_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, static_cast<int *>(nullptr), static_cast<int *>(nullptr),
                                            n_regions + 1, st));
    const size_t b_cnt = align256(sizeof(int) * ((size_t)n_regions + 1));
    const size_t b_perm = align256(sizeof(int) * (size_t)hit_capacity);
    const size_t b_score = align256(sizeof(int) * (size_t)batch);
    const size_t b_mask = align256(sizeof(unsigned long long) * (size_t)batch * (size_t)hw);
    const size_t total = 2 * b_cnt + b_perm + b_score + b_mask + align256(cub_bytes);
    unsigned char *base = nullptr;
    GX_TRY(hipMallocAsync(reinterpret_cast<void **>(&base), total, st));
    int *cnt = reinterpret_cast<int *>(base);
    int *off = reinterpret_cast<int *>(base + b_cnt);
    int *perm = reinterpret_cast<int *>(base + 2 * b_cnt);
    int *bscore = reinterpret_cast<int *>(base + 2 * b_cnt + b_perm);
    auto *masks = reinterpret_cast<unsigned long long *>(base + 2 * b_cnt + b_perm + b_score);
    void *cub_tmp = base + 2 * b_cnt + b_perm + b_score + b_mask;
    const Tile *tiles = P->f_tiles.p;
    const int n_tiles = P->f_n_tiles;
    const auto *hits = static_cast<const GraphHit *>(d_hits);
    const auto *hc = reinterpret_cast<const unsigned long long *>(d_hit_count);
    const unsigned scan_blocks = (unsigned)std::min<long long>((hit_capacity + kHhScanThreads - 1) / kHhScanThreads, 4096);
    hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int) * ((size_t)n_regions + 1), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hh_region_count_kernel, dim3(scan_blocks), dim3(kHhScanThreads), 0, st, tiles, n_tiles, hits, hc,
                           (long long)hit_capacity, d_cutoff, n_regions, cnt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, cnt, off, n_regions + 1, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt, off, sizeof(int) * ((size_t)n_regions + 1), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hh_scatter_kernel, dim3(scan_blocks), dim3(kHhScanThreads), 0, st, tiles, n_tiles, hits, hc,
                           (long long)hit_capacity, d_cutoff, n_regions, cnt, perm);
        e = hipGetLastError();
    }
    for (long long b0 = 0; e == hipSuccess && b0 < hit_capacity; b0 += batch) {
        const long long b1 = std::min<long long>(b0 + batch, hit_capacity);
        hipLaunchKernelGGL(hh_mask_kernel, dim3((unsigned)std::min<long long>(b1 - b0, kHhMaskBlocks)), dim3(64), 0, st, g->dev,
                           P->f_width, tiles, n_tiles, hits, perm, off, n_regions, b0, b1, masks, bscore);
        e = hipGetLastError();
        for (int r0 = 0; e == hipSuccess && r0 < n_regions; r0 += kHhRegionChunk) {
            const unsigned nr = (unsigned)std::min(n_regions - r0, kHhRegionChunk);
            hipLaunchKernelGGL(hh_reduce_kernel, dim3(nr, (unsigned)((H + kHhReduceThreads - 1) / kHhReduceThreads)),
                               dim3(kHhReduceThreads), 0, st, masks, bscore, off, n_regions, r0, H, hw, b0, b1, d_counts, d_best);
            e = hipGetLastError();
        }
    }
    const hipError_t ef = hipFreeAsync(base, st);
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) return gfail(GFM_ERR_HIP, std::string("gfm_graph_haplotype_hits: ") + hipGetErrorString(e));
    return g->called(st);
}
