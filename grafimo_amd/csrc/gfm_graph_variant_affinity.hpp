// gfm_graph_variant_affinity.hpp -- per-variant affinity effects: for every (site, allele) of the graph the TOTAL affinity
// of the allele's carriers over the allele's footprint -- the sum, over every k-mer of every haplotype's own sequence that
// covers the footprint, of a 64-bit integer weight looked up by the k-mer's scaled score -- beside the number of those k-mers
// (included at the end of graph_extract.hip behind gfm_graph_variant.hpp, whose window list, layout enumeration and replay it
// shares; it uses gfm_graph_table_score.hpp's window_sum, walk_value, walk_code and ConstraintAt).
//
// sums[slot] = (sum, rows), slot = site * 4 + allele (0 = none of the site's ALTs).  A walk of a window stands for the same
// k-mer of carriers(walk) haplotypes -- the popcount over ALL bitset words of the AND of its constraints -- and qualifies for
// exactly the slots of its constraints (gfm_graph_variant.hpp), so it adds carriers * (w[s+] + w[s-]) to sum and
// carriers * strands to rows of each.  A sum needs every walk exactly ONCE: the host lists every distinct window start once
// (variant_stage_windows, unique: with the largest limit of the regions that hold it, which is the union of their walks),
// for_window_layouts visits every layout of a window once and the lanes take a layout's walks q = 0 .. prod - 1 once.  One
// pass, no records.  Integer adds commute: the result is exact whatever the order of the atomics.
//
// Work decomposition: a WAVEFRONT per window, as graph_variant_kernel.  A window's walks meet a handful of slots -- those of
// the sites within W bases --, thousands of times in a dense window: the adds are staged per wave in LDS, in an open-addressed
// table keyed by slot ((key, sum, rows) x 64, linear probing, a key claimed by an LDS compare-and-swap), with 64-bit LDS
// adds, and flushed with one pair of global atomics per occupied entry when the window is done.  An add that finds the table
// full goes to global memory directly.  Every add, LDS or global, takes the old value back: old + v < v is a wrap of the
// 64-bit sum and sets bit 1 of *overflow (bit 0: a window of more than 2^24 walks, left out).
namespace {

constexpr int kVaThreads = 64;
constexpr int kVaTable = 64;                       // entries of a wave's LDS table (a power of two)
constexpr int kVaOverWalks = 1, kVaOverSum = 2;    // bits of *overflow

typedef __attribute__((address_space(3))) unsigned long long va_lds_u64;

// v into the LDS cell at `cell` -> the add wrapped.  The pointer is an address_space(3) one on purpose (lds_hist_add of
// gfm_score_quad.hpp): it can only become a ds_add, never a FLAT atomic.
__device__ __forceinline__ bool va_lds_add(unsigned long long *cell, unsigned long long v)
{
    const unsigned long long old =
        __hip_atomic_fetch_add((va_lds_u64 *)cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return old + v < v;
}

__device__ __forceinline__ bool va_global_add(unsigned long long *cell, unsigned long long v)
{
    const unsigned long long old = atomicAdd(cell, v);
    return old + v < v;
}

__global__ void __launch_bounds__(kVaThreads)
graph_variant_affinity_kernel(GraphDev g, const unsigned *__restrict__ ftab, const unsigned long long *__restrict__ wtab, int W,
                              int min_val, const VarWin *__restrict__ wins, long long n_wins, int forward_only, int table,
                              unsigned long long *__restrict__ sums, int *__restrict__ overflow)
{
    __shared__ int t_key[kVaTable];                         // slot, -1: free
    __shared__ unsigned long long t_sum[kVaTable], t_rows[kVaTable];
    const int lane = threadIdx.x;
    const unsigned long long strands = forward_only ? 1ull : 2ull;
    const bool haps = g.alt_bits && g.n_hap > 0;
    t_key[lane] = -1;
    t_sum[lane] = 0ull;
    t_rows[lane] = 0ull;
    int wrapped = 0;
    for (long long wi = blockIdx.x; wi < n_wins; wi += gridDim.x) {
        const VarWin vw = wins[wi];
        const long long p = vw.p, limit = vw.limit;
        const int i0 = lower_bound_pos(g.pos, g.n_sites, p);
        __syncthreads();                                    // (the table is free: made so above, or by the last flush)
        const bool over = for_window_layouts<kVarMaxWalks>(g, p, W, i0, limit, [&](const WalkStart &ws, const WalkState &st,
                                                                                   long long prod) {
            for (long long q = lane; haps && q < prod; q += kVaThreads) {
                uint8_t km[GFM_MAX_WIDTH], kr[GFM_MAX_WIDTH];
                int src[GFM_MAX_WIDTH];
                int more[kMaxConstraints - 4];
                DelEmit em(g, km, kr, src, W, more);
                replay_walk<kVarMaxWalks>(g, p, W, i0, ws, st, q, prod, limit, em);
                const int nc = em.n_cons;
                if (nc == 0) continue;                      // a walk over no site: no allele's footprint
                const ConstraintAt at{em};
                unsigned long long carriers = 0ull;         // the FULL count: every word, not "some haplotype"
                for (int word = 0; word < g.hw; ++word) carriers += (unsigned long long)__popcll(carrier_word<true>(g, nc, at, word));
                if (carriers == 0ull) continue;             // a walk nobody carries adds nothing
                const WindowSum w = window_sum(ftab, W, [&](int j) { return walk_code(g, src, km, j); });
                const unsigned long long value = walk_value(wtab, w, min_val, forward_only);
                // (the two strands' weights and the carriers' multiple are adds of the sum too: a wrap in them is one)
                if (!forward_only && value < wtab[strand_scores(w, min_val).plus]) wrapped = 1;
                if (__umul64hi(carriers, value)) wrapped = 1;
                const unsigned long long add = carriers * value, add_rows = carriers * strands;
                for (int k = 0; k < nc; ++k) {
                    int site, al;
                    at(k, site, al);
                    const int slot = site * 4 + al;
                    bool again = false;                     // a slot counts once per walk
                    for (int j = 0; j < k && !again; ++j) {
                        int sj, aj;
                        at(j, sj, aj);
                        again = sj * 4 + aj == slot;
                    }
                    if (again) continue;
                    int e = -1;
                    unsigned h = ((unsigned)slot * 0x9E3779B1u) >> 26;
                    for (int probe = 0; probe < table; ++probe, ++h) {
                        const int at_e = (int)(h & (unsigned)(table - 1));
                        const int was = atomicCAS(&t_key[at_e], -1, slot);
                        if (was == -1 || was == slot) { e = at_e; break; }
                    }
                    if (e >= 0) {
                        if (va_lds_add(&t_sum[e], add)) wrapped = 1;
                        if (va_lds_add(&t_rows[e], add_rows)) wrapped = 1;
                    } else {
                        if (va_global_add(&sums[2 * (size_t)slot], add)) wrapped = 1;
                        if (va_global_add(&sums[2 * (size_t)slot + 1], add_rows)) wrapped = 1;
                    }
                }
            }
        });
        __syncthreads();
        // ---- the window's entries: one pair of global adds each, the table left free
        const int slot = t_key[lane];
        if (slot >= 0) {
            if (va_global_add(&sums[2 * (size_t)slot], t_sum[lane])) wrapped = 1;
            if (va_global_add(&sums[2 * (size_t)slot + 1], t_rows[lane])) wrapped = 1;
            t_key[lane] = -1;
            t_sum[lane] = 0ull;
            t_rows[lane] = 0ull;
        }
        if (over && lane == 0) atomicOr(overflow, kVaOverWalks);
    }
    if (wrapped) atomicOr(overflow, kVaOverSum);
}

}  // namespace

GFM_API int gfm_graph_variant_affinity(gfm_graph_t g, const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                       int32_t n_regions, const int64_t *h_starts, const int64_t *h_stops, uint32_t flags,
                                       uint64_t *const *d_sums, int32_t *d_overflow, int64_t *n_windows, int32_t table_entries,
                                       void *stream)
{
    if (!g) return gfail(GFM_ERR_INVALID, "graph is NULL");
    if (!has_haplotypes(*g)) return fail_no_haplotypes("gfm_graph_variant_affinity");
    if (!motifs || n_motifs < 1 || n_regions < 0 || (n_regions && (!h_starts || !h_stops)) || !d_weights || !d_sums || !d_overflow)
        return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    if (table_entries < 0 || table_entries > kVaTable || (table_entries & (table_entries - 1)))
        return gfail(GFM_ERR_INVALID, "table_entries: 0 or a power of two up to " + std::to_string(kVaTable));
    for (int m = 0; m < n_motifs; ++m)
        if (!motifs[m] || !d_weights[m] || !d_sums[m]) return gfail(GFM_ERR_INVALID, "NULL motif / device buffer");
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::PackedTable, ms)) return rc;
    if (const int rc = check_regions(n_regions, h_starts, h_stops)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = g->serialise(st)) return rc;
    long long n_win = 0;
    if (const int rc = variant_stage_windows(g, ms.W, n_regions, h_starts, h_stops, true, st, &n_win)) return rc;
    if (n_windows) *n_windows = n_win;
    if (n_win > 0) {
        const int grid = (int)std::min<long long>(n_win, 1 << 16);
        const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0, table = table_entries ? table_entries : kVaTable;
        const VarWin *wins = static_cast<const VarWin *>(g->v_wins);
        for (int m = 0; m < n_motifs; ++m) {
            hipLaunchKernelGGL(graph_variant_affinity_kernel, dim3(grid), dim3(kVaThreads), 0, st, g->dev, ms.ftab[m],
                               reinterpret_cast<const unsigned long long *>(d_weights[m]), ms.W, ms.min_val[m], wins, n_win, fwd, table,
                               reinterpret_cast<unsigned long long *>(d_sums[m]), d_overflow);
            GX_TRY(hipGetLastError());
        }
    }
    return g->called(st);
}
