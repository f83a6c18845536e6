// gfm_graph_hit_alleles.hpp -- the per-hit allele table: for every hit entry of the last fused scoring call, the set of
// (graph site, allele) constraints of its walk, how many haplotypes of each caller-given group carry it, and (optionally) the
// carrier set itself.  (Included at the end of graph_extract.hip: it reads the hit entries of gfm_graph_score[_multi] and the
// plan's tile table and walks the graph as graph_annotate_kernel and hh_mask_hit (gfm_graph_haplotypes.hpp) do.)
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

__device__ __forceinline__ int ha_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The constraints of one hit entry into keys[0 .. n) as site * 4 + allele, in the order they were met (duplicates
// included) -> n, or -1 when the walk was not found (cannot happen: the score kernel found it).  The derivation is
// hh_mask_hit's, which is annotate_hit's; only what is kept differs.  Every lane runs it; the lanes share the stores.
__device__ __forceinline__ int ha_constraints(const GraphDev &g, int W, const Tile *__restrict__ tiles, int n_tiles,
                                              const GraphHit &hit, int *keys)
{
    const int lane = threadIdx.x & 63;
    const Tile t = tiles[min(max(hit.tile, 0), n_tiles - 1)];
    const int k = (int)(hit.q2k >> kHitWinShift) & 0xff;
    const long long q = (hit.q2k & kHitWalkMask) >> 1;
    const long long p = t.p0 + k;
    __shared__ SiteRec a_rec[kWaveSites];
    __shared__ int a_reach[kWaveSites];
    const int staged = min(t.i_far - t.i_lo + 1, kWaveSites);
    for (int s_ = threadIdx.x; s_ < staged; s_ += 64) {
        const int i = t.i_lo + s_;
        a_rec[s_] = packed_site(g, i);
        const long long r = (i <= g.n_sites ? g.max_reach[i] : -1ll) - t.p0;
        a_reach[s_] = (int)max(-1ll, min(r, 0x7fffffffll));
    }
    __syncthreads();
    const WinInfo wi = classify_window(g, TileSites{g, a_rec, a_reach, t.p0, t.i_lo, staged}, p, W, t.limit, t.i_lo, t.i_hi);
    if (!wi.listed) {
        unsigned long long dig[2] = {0ull, 0ull};
        unsigned long long rest = (unsigned long long)q;
        for (int s_ = wi.ns - 1; s_ >= 0; --s_) {
            const int nall = 1 + g.n_alts[wi.i0 + s_];
            dig[s_ >> 5] |= (unsigned long long)take_digit(rest, nall) << (2 * (s_ & 31));
        }
        const int n = min(wi.ns, kMaxConstraints);
        for (int kk = lane; kk < n; kk += 64) keys[kk] = (wi.i0 + kk) * 4 + (int)((dig[kk >> 5] >> (2 * (kk & 31))) & 3ull);
        return n;
    }
    __shared__ SiteRec ann_cache[kSiteCache];
    if (threadIdx.x < kSiteCache) ann_cache[threadIdx.x] = g.site_rec[wi.i0 + threadIdx.x];
    __syncthreads();
    const CachedSites cs{g.site_rec, ann_cache, wi.i0, 1};
    WalkState st;
    WalkStart ws;
    NoVisitor nv;
    long long rest = q, prod = 0;
    bool found = false, more = true;
    while (!found && more) {
        int prefix = 0;
        for (;;) {
            const int rc = simulate<NoVisitor, CachedSites, kFusedMaxWalks>(g, cs, p, W, wi.i0, ws, prefix, st, nv, 0, 0, prod, t.limit);
            if (rc == WALK_OK) {
                if (rest < prod) { found = true; break; }
                rest -= prod;
            }
            prefix = next_walk(st);
            if (prefix < 0) break;
        }
        if (!found) more = next_start(g, p, wi.i0, ws);
    }
    if (!found) return -1;
    uint8_t km[2 * GFM_MAX_WIDTH];
    int src[GFM_MAX_WIDTH];
    int more_cons[kMaxConstraints - 4];
    DelEmit em(g, km, km + W, src, W, more_cons);
    long long again = 0;
    simulate<DelEmit, CachedSites, kFusedMaxWalks>(g, cs, p, W, wi.i0, ws, st.nd, st, em, rest, prod, again, t.limit);
    if (!(ws.site >= 0 && st.last == p - 1)) for_covering_deletions(g, p, wi.i0, [&](int dsite) { em.add(dsite, 0); });
    const int n = min(em.n_cons, kMaxConstraints);
    for (int kk = lane; kk < n; kk += 64) {
        const int v = em.get(kk);
        keys[kk] = (v >> 4) * 4 + (v & 3);
    }
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
                acc = ~0ull;
                if (word == g.hw - 1 && (g.n_hap & 63)) acc = (1ull << (g.n_hap & 63)) - 1ull;
                for (int k = 0; k < n_u && acc; ++k) {
                    const int key = s_key[k];
                    acc &= allele_word(g, key >> 2, key & 3, word);
                }
            }
            if (masks && word < g.hw) masks[(size_t)i * g.hw + word] = acc;
            tot += __popcll(acc);
            for (int gi = 0; gi < n_groups; ++gi) {
                const int v = ha_wave_sum(word < g.hw ? __popcll(acc & group_bits[(size_t)gi * g.hw + word]) : 0);
                if (lane == gi) mine += v;
            }
        }
        tot = ha_wave_sum(tot);
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

inline size_t ha_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

GFM_API int gfm_graph_hit_alleles(gfm_graph_t g, const void *d_hits, const uint64_t *d_hit_count, int64_t hit_capacity,
                                  const int32_t *d_cutoff, int32_t n_groups, const uint64_t *d_group_bits,
                                  int64_t *d_allele_off, int32_t *d_alleles, int64_t allele_capacity, int32_t *d_group_counts,
                                  int32_t *d_total, uint64_t *d_masks, int64_t scratch_bytes, void *stream)
{
    if (!g) return gfail(GFM_ERR_INVALID, "graph is NULL");
    if (n_groups < 0 || n_groups > 64)
        return gfail(GFM_ERR_INVALID, "gfm_graph_hit_alleles: " + std::to_string(n_groups) + " groups (at most 64 per call)");
    const bool want_bits = n_groups > 0 || d_total || d_masks;
    if (want_bits && (!g->dev.alt_bits || g->dev.n_hap <= 0))
        return gfail(GFM_ERR_INVALID, "gfm_graph_hit_alleles: the graph carries no haplotypes (no bitsets were given to "
                                      "gfm_graph_create: an XG without its GBWT, or a VCF without samples): it has alleles, "
                                      "but no groups, totals or carrier masks");
    FusedPlan *P = g->plan;
    if (!P) return gfail(GFM_ERR_INVALID, "gfm_graph_hit_alleles: no gfm_graph_score call on this handle");
    if (hit_capacity < 0 || allele_capacity < 0 || !d_allele_off || (allele_capacity && !d_alleles))
        return gfail(GFM_ERR_INVALID, "bad argument");
    if (n_groups > 0 && (!d_group_bits || (hit_capacity && !d_group_counts))) return gfail(GFM_ERR_INVALID, "NULL group buffer");
    if (hit_capacity > 0 && (!d_hits || !d_hit_count)) return gfail(GFM_ERR_INVALID, "NULL device buffer");
    if (hit_capacity > 0x7fffffffll) return gfail(GFM_ERR_INVALID, "hit capacity beyond 2^31");
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
    const size_t b_cnt = ha_align(sizeof(int) * (size_t)batch);
    const size_t b_stage = ha_align(sizeof(int) * (size_t)batch * kMaxConstraints);
    const size_t total_bytes = 256 + 2 * b_cnt + b_stage + ha_align(cub_bytes);
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
