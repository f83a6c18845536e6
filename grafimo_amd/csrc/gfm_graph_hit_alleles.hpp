// gfm_graph_hit_alleles.hpp -- the per-hit allele table: for every hit entry of the last fused scoring call, the set of
// (graph site, allele) constraints of its walk, how many haplotypes of each caller-given group carry it, and (optionally) the
// carrier set itself.  (Included at the end of graph_extract.hip: it reads the hit entries of gfm_graph_score[_multi] and the
// plan's tile table and re-derives their walks as graph_annotate_kernel and hh_mask_kernel do: hit_walk.)
//
// The outputs are indexed by the ENTRY index i, so that they line up with record i of gfm_graph_annotate.  The constraints
// are the ones the haplotype counting uses -- plain window: the mixed-radix digits of the walk number, one per substitution
// site of the window; listed window: what DelEmit collects in one replay of the walk plus the deletions that cover the
// window's first base -- as a SET: packed site * 4 + allele, ascending, no pair twice.
//
// Work decomposition, per batch of entries whose staging fits the scratch budget:
//   ha_entry_kernel   -- a WAVEFRONT per entry that passes the cutoff: derives the constraints (every lane follows the same
//                        path), sorts and de-duplicates them in LDS (at most 96 of them: ranks by comparison), stages them
//                        [batch][96] with their count; then the lanes take the bitset words: the AND of the constraints'
//                        bitsets, its popcount, and per group g a wave reduction of popc(acc & group_bits[g][word]) whose sum
//                        LANE g keeps (hence at most 64 groups) -- one store per (entry, group);
//   hipcub ExclusiveSum over the batch's counts;
//   ha_compact_kernel -- off[i] = running base + scan, the staged constraints to their place in the CSR array;
//   ha_advance_kernel -- the running base moves on (a device word: nothing comes back to the host between batches).
namespace {

constexpr int kHaBlocks = 8192;                      // wavefronts of ha_entry_kernel: entries dealt over the grid, as annotate's
constexpr int kHaCompactThreads = 256;
constexpr long long kHaMaxBatch = 1ll << 24;         // entries per batch: 96 constraints each stay below 2^31 in the int scan

// The constraints of one hit entry (hit_walk) into keys[0 .. n) as site * 4 + allele, in the order they were met (duplicates
// included), at most kMaxConstraints of them -> n, or -1 when there is no such walk.  The lanes share the stores.
__device__ __forceinline__ int ha_constraints(const GraphDev &g, int W, const Tile *__restrict__ tiles, int n_tiles,
                                              const GraphHit &hit, int *keys)
{
    const Tile t = hit_tile(tiles, n_tiles, hit);
    int n = -1;
    hit_walk<false>(g, W, t, hit, nullptr, [&](int n_cons, auto at, long long, bool) {
        n = min(n_cons, kMaxConstraints);
        for (int kk = threadIdx.x & 63; kk < n; kk += 64) {
            int site, al;
            at(kk, site, al);
            keys[kk] = site * 4 + al;
        }
    });
    return n;
}

// a wavefront per entry i in [b0, min(b1, entries)) that passes the cutoff; what it skips stays as the host zeroed it
__global__ void __launch_bounds__(64)
ha_entry_kernel(GraphDev g, int W, const Tile *__restrict__ tiles, int n_tiles, const GraphHit *__restrict__ hits,
                const unsigned long long *__restrict__ hit_count, long long hit_cap, const int *__restrict__ d_cutoff,
                long long b0, long long b1, int *__restrict__ cnt, int *__restrict__ stage, int n_groups,
                const unsigned long long *__restrict__ group_bits, int *__restrict__ group_counts, int *__restrict__ total,
                unsigned long long *__restrict__ masks)
{
    __shared__ int s_key[kMaxConstraints];
    __shared__ int s_sorted[kMaxConstraints];
    const int lane = threadIdx.x & 63;
    const bool want_bits = g.alt_bits && (n_groups > 0 || total || masks);
    const long long n_entries = min(min((long long)*hit_count, hit_cap), b1);
    for (long long i = b0 + (long long)blockIdx.x; i < n_entries; i += (long long)gridDim.x) {
        __syncthreads();                    // (the last entry's LDS is no longer read)
        const GraphHit hit = hits[i];
        if (d_cutoff && hit.score < *d_cutoff) continue;           // (uniform over the wavefront)
        const int n = ha_constraints(g, W, tiles, n_tiles, hit, s_key);
        __syncthreads();
        // ascending with the duplicates side by side: the place of key k is the number of keys before it in (key, index) order
        for (int k = lane; k < n; k += 64) {
            const int key = s_key[k];
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const int kj = s_key[j];
                rank += (kj < key || (kj == key && j < k)) ? 1 : 0;
            }
            s_sorted[rank] = key;
        }
        __syncthreads();
        int n_u = 0;                        // every lane walks the sorted list (broadcast reads); lane 0 keeps the distinct keys
        for (int j = 0, prev = -1; j < n; ++j) {
            const int v = s_sorted[j];
            if (j == 0 || v != prev) {
                if (lane == 0) s_key[n_u] = v;
                ++n_u;
            }
            prev = v;
        }
        __syncthreads();
        int *st_ = stage + (size_t)(i - b0) * kMaxConstraints;
        for (int k = lane; k < n_u; k += 64) st_[k] = s_key[k];
        if (lane == 0) cnt[i - b0] = n_u;
        if (!want_bits) continue;
        int mine = 0, tot = 0;              // lane g: the carriers of group g
        for (int w0 = 0; w0 < g.hw; w0 += 64) {
            const int word = w0 + lane;
            unsigned long long acc = 0ull;
            if (word < g.hw && n >= 0) {
                auto at = [&](int k, int &site, int &al) { const int key = s_key[k]; site = key >> 2; al = key & 3; };
                acc = carrier_word<true>(g, n_u, at, word);
            }
            if (masks && word < g.hw) masks[(size_t)i * g.hw + word] = acc;
            tot += __popcll(acc);
            for (int gi = 0; gi < n_groups; ++gi) {
                const int v = wave_sum(word < g.hw ? __popcll(acc & group_bits[(size_t)gi * g.hw + word]) : 0);
                if (lane == gi) mine += v;
            }
        }
        tot = wave_sum(tot);
        if (total && lane == 0) total[i] = tot;
        if (lane < n_groups) group_counts[(size_t)i * n_groups + lane] = mine;
    }
}

// thread per entry of the batch: its offset, its staged constraints to their place (what lies beyond the room is dropped:
// the offsets say how much room to come back with)
__global__ void __launch_bounds__(kHaCompactThreads)
ha_compact_kernel(long long b0, long long nb, const int *__restrict__ cnt, const int *__restrict__ toff,
                  const int *__restrict__ stage, const long long *__restrict__ base, long long *__restrict__ off,
                  int *__restrict__ alleles, long long allele_cap)
{
    const long long t = (long long)blockIdx.x * kHaCompactThreads + threadIdx.x;
    if (t >= nb) return;
    const long long o = *base + toff[t];
    off[b0 + t] = o;
    const int n = cnt[t];
    const int *st_ = stage + (size_t)t * kMaxConstraints;
    for (int k = 0; k < n; ++k)
        if (o + k < allele_cap) alleles[o + k] = st_[k];
}

// one thread: the base of the next batch, which is also the end of this batch's last entry
__global__ void ha_advance_kernel(long long b0, long long nb, const int *__restrict__ cnt, const int *__restrict__ toff,
                                  long long *__restrict__ base, long long *__restrict__ off)
{
    const long long next = *base + toff[nb - 1] + cnt[nb - 1];
    *base = next;
    off[b0 + nb] = next;
}

}  // namespace

GFM_API int gfm_graph_hit_alleles(gfm_graph_t g, const void *d_hits, const uint64_t *d_hit_count, int64_t hit_capacity,
                                  const int32_t *d_cutoff, int32_t n_groups, const uint64_t *d_group_bits,
                                  int64_t *d_allele_off, int32_t *d_alleles, int64_t allele_capacity, int32_t *d_group_counts,
                                  int32_t *d_total, uint64_t *d_masks, int64_t scratch_bytes, void *stream)
{
    if (const int rc = check_hit_list(g, "gfm_graph_hit_alleles", d_hits, d_hit_count, hit_capacity)) return rc;
    if (n_groups < 0 || n_groups > 64)
        return gfail(GFM_ERR_INVALID, "gfm_graph_hit_alleles: " + std::to_string(n_groups) + " groups (at most 64 per call)");
    if ((n_groups > 0 || d_total || d_masks) && !has_haplotypes(*g))
        return fail_no_haplotypes("gfm_graph_hit_alleles", ": it has alleles, but no groups, totals or carrier masks");
    FusedPlan *P = g->plan;
    if (allele_capacity < 0 || !d_allele_off || (allele_capacity && !d_alleles)) return gfail(GFM_ERR_INVALID, "bad argument");
    if (n_groups > 0 && (!d_group_bits || (hit_capacity && !d_group_counts))) return gfail(GFM_ERR_INVALID, "NULL group buffer");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int hw = g->dev.hw;
    if (const int rc = g->serialise(st)) return rc;
    // what the kernel skips (entries under the cutoff, slots behind the count) reads as "nothing"
    GX_TRY(hipMemsetAsync(d_allele_off, 0, sizeof(int64_t) * ((size_t)hit_capacity + 1), st));
    if (hit_capacity) {
        if (n_groups) GX_TRY(hipMemsetAsync(d_group_counts, 0, sizeof(int32_t) * (size_t)hit_capacity * (size_t)n_groups, st));
        if (d_total) GX_TRY(hipMemsetAsync(d_total, 0, sizeof(int32_t) * (size_t)hit_capacity, st));
        if (d_masks) GX_TRY(hipMemsetAsync(d_masks, 0, sizeof(uint64_t) * (size_t)hit_capacity * (size_t)hw, st));
    }
    if (hit_capacity == 0 || P->f_n_tiles == 0) return g->called(st);
    const long long budget = scratch_bytes > 0 ? scratch_bytes : kHhDefaultScratch;
    const long long per_entry = (long long)sizeof(int) * (kMaxConstraints + 2);
    const long long batch = std::min<long long>({std::max(1ll, budget / per_entry), (long long)hit_capacity, kHaMaxBatch});
    size_t cub_bytes = 0;
    GX_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, static_cast<int *>(nullptr), static_cast<int *>(nullptr),
                                            (int)batch, st));
    const size_t b_cnt = align256(sizeof(int) * (size_t)batch);
    const size_t b_stage = align256(sizeof(int) * (size_t)batch * kMaxConstraints);
    const size_t total_bytes = 256 + 2 * b_cnt + b_stage + align256(cub_bytes);
    unsigned char *mem = nullptr;
    GX_TRY(hipMallocAsync(reinterpret_cast<void **>(&mem), total_bytes, st));
    long long *base = reinterpret_cast<long long *>(mem);
    int *cnt = reinterpret_cast<int *>(mem + 256);
    int *toff = reinterpret_cast<int *>(mem + 256 + b_cnt);
    int *stage = reinterpret_cast<int *>(mem + 256 + 2 * b_cnt);
    void *cub_tmp = mem + 256 + 2 * b_cnt + b_stage;
    const auto *hits = static_cast<const GraphHit *>(d_hits);
    const auto *hc = reinterpret_cast<const unsigned long long *>(d_hit_count);
    hipError_t e = hipMemsetAsync(base, 0, sizeof(long long), st);
    for (long long b0 = 0; e == hipSuccess && b0 < hit_capacity; b0 += batch) {
        const long long nb = std::min<long long>(batch, hit_capacity - b0);
        e = hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)nb, st);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(ha_entry_kernel, dim3((unsigned)std::min<long long>(nb, kHaBlocks)), dim3(64), 0, st, g->dev,
                           P->f_width, P->f_tiles.p, P->f_n_tiles, hits, hc, (long long)hit_capacity, d_cutoff, b0, b0 + nb, cnt,
                           stage, (int)n_groups, reinterpret_cast<const unsigned long long *>(d_group_bits), d_group_counts,
                           d_total, reinterpret_cast<unsigned long long *>(d_masks));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, cnt, toff, (int)nb, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ha_compact_kernel, dim3((unsigned)((nb + kHaCompactThreads - 1) / kHaCompactThreads)),
                               dim3(kHaCompactThreads), 0, st, b0, nb, cnt, toff, stage, base,
                               reinterpret_cast<long long *>(d_allele_off), d_alleles, (long long)allele_capacity);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ha_advance_kernel, dim3(1), dim3(1), 0, st, b0, nb, cnt, toff, base,
                               reinterpret_cast<long long *>(d_allele_off));
            e = hipGetLastError();
        }
    }
    const hipError_t ef = hipFreeAsync(mem, st);
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) return gfail(GFM_ERR_HIP, std::string("gfm_graph_hit_alleles: ") + hipGetErrorString(e));
    return g->called(st);
}
