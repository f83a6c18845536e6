// gfm_graph_hapaffinity.hpp -- the per-haplotype total binding affinity: for every region of the caller's list and every
// haplotype of the graph, the SUM over every k-mer of the haplotype's own sequence in the region of a 64-bit integer weight
// looked up by the k-mer's scaled score (included at the end of graph_extract.hip behind gfm_graph_hapscores.hpp, whose
// runs, run shape, limits and walk enumeration it shares; it uses gfm_graph_table_score.hpp's window_sum, walk_value,
// walk_code, walk_is_reference and ConstraintAt).
//
// Rows(r, h) are those of gfm_graph_hapscores.hpp.  A(r, h) = sum over Rows(r, h) of w[score(row)] in uint64: integer adds
// commute, so the result is exact and depends neither on the run / block decomposition nor on the order of the atomics.
// Column n_hap is the reference path.  A sum needs every walk exactly ONCE, where the maximum did not care: the runs
// partition a region's window starts, a window is either plain (step 1) or a wavefront's (step 2), for_window_layouts
// visits every layout of a window once and the lanes take a layout's walks q = 0 .. prod - 1 once.
//
// Work decomposition: a WORKGROUP per (run of consecutive window starts of one region, block of haplotypes), as
// graph_hapscore_kernel.
//   1. plain windows, a thread each: w[s+] (+ w[s-]) into the thread's "everyone" partial;
//   2. the other windows a WAVEFRONT each, the lanes take the walks 64 at a time.  A walk without a constraint adds to the
//      everyone partial; one whose constraints are all allele 0 adds to the reference partial; every walk with a constraint
//      is a record that STAYS IN ITS LANE: the value w[s+] + w[s-] and the constraints the replay left there;
//   3. the carrier pass over the wave's (at most 64) records, per bitset word of the block: every lane makes the carrier
//      word of ITS OWN record (the AND of its constraints' bitsets: the 64 lanes' loads are in flight together), then the
//      wave steps through the records whose word is not 0 -- the word and the value broadcast from the record's lane -- and
//      each lane, owning haplotype word * 64 + lane, adds the value to a register if its bit is set.  There is no "this
//      record raises nobody" shortcut as for a maximum: every record meets every word; only a zero word is skipped.  One
//      64-bit LDS add per lane and word then goes to the block's cells (the four waves share them; the lanes of one
//      instruction touch distinct cells);
//   4. per wave the partials are reduced and added in LDS; the block writes everyone + cell to sums[region][n_hap + 1]: a
//      plain store when the run is the region's only one, else a 64-bit atomicAdd.  Block 0 writes the reference column.
namespace {

__global__ void __launch_bounds__(kHsThreads)
graph_hapaffinity_kernel(GraphDev g, const unsigned *__restrict__ ftab, const unsigned long long *__restrict__ wtab, int W,
                         int min_val, const HsRun *__restrict__ runs, long long n_runs, int forward_only, int hb,
                         unsigned long long *__restrict__ sums, int *__restrict__ overflow)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long ha_cells[];      // [hb]
    __shared__ unsigned char plain_win[kHsMaxRun];
    __shared__ unsigned long long all_sum, ref_sum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = g.n_hap, h0 = (int)blockIdx.y * hb;
    const int w0 = h0 >> 6, nw = min(g.hw - w0, hb >> 6);
    for (long long ri = blockIdx.x; ri < n_runs; ri += gridDim.x) {
        const HsRun run = runs[ri];
        const int n_win = (int)(run.p1 - run.p0);
        __syncthreads();                                     // (the last run's cells are written)
        for (int i = threadIdx.x; i < nw * 64; i += kHsThreads) ha_cells[i] = 0ull;
        if (threadIdx.x == 0) { all_sum = 0ull; ref_sum = 0ull; }
        unsigned long long all_s = 0ull, ref_s = 0ull;
        // ---- 1. plain windows, a thread each
        for (int k = threadIdx.x; k < n_win; k += kHsThreads) {
            const long long p = run.p0 + k;
            const int i0 = lower_bound_pos(g.pos, g.n_sites, p);
            bool plain = (i0 >= g.n_sites || (long long)g.pos[i0] >= p + W) && !covered_by_deletion(g, p, i0);
            for (int j = i0 - 1; plain && j >= 0 && g.pos[j] == p - 1; --j)     // (graph_hapscore_kernel's test, kept in
                if (g.ins_len[j] > 0) plain = false;                            // line: see gfm_graph_table_score.hpp)
            plain_win[k] = plain ? 1 : 0;
            if (plain && p + W <= run.limit)
                all_s += walk_value(wtab, window_sum(ftab, W, [&](int j) { return base_code(g.ref[p + j]); }), min_val, forward_only);
        }
        __syncthreads();
        // ---- 2. + 3. the other windows, a wavefront each
        for (int k = wave; k < n_win; k += kHsWaves) {
            if (plain_win[k]) continue;
            const long long p = run.p0 + k;
            const int i0 = lower_bound_pos(g.pos, g.n_sites, p);
            const bool over = for_window_layouts<kHsMaxWalks>(g, p, W, i0, run.limit, [&](const WalkStart &ws, const WalkState &st,
                                                                                          long long prod) {
                for (long long q0 = 0; q0 < prod; q0 += 64) {
                    const long long q = q0 + lane;
                    uint8_t km[GFM_MAX_WIDTH], kr[GFM_MAX_WIDTH];
                    int src[GFM_MAX_WIDTH];
                    int more[kMaxConstraints - 4];
                    DelEmit em(g, km, kr, src, W, more);
                    int nc = 0;                     // constraints of this lane's record (0: none)
                    unsigned long long value = 0ull;
                    if (q < prod) {
                        replay_walk<kHsMaxWalks>(g, p, W, i0, ws, st, q, prod, run.limit, em);
                        const WindowSum w = window_sum(ftab, W, [&](int j) { return walk_code(g, src, km, j); });
                        const unsigned long long v = walk_value(wtab, w, min_val, forward_only);
                        if (em.n_cons == 0) {
                            all_s += v;                               // a walk over no site: everyone's
                        } else {
                            if (walk_is_reference(em)) ref_s += v;
                            nc = em.n_cons;
                            value = v;
                        }
                    }
                    if (!__builtin_amdgcn_ballot_w64(nc > 0)) continue;
                    const ConstraintAt at{em};
                    for (int w = 0; w < nw; ++w) {
                        const unsigned long long mine = nc > 0 ? carrier_word<true>(g, nc, at, w0 + w) : 0ull;
                        unsigned long long add = 0ull;
                        for (unsigned long long left = __builtin_amdgcn_ballot_w64(mine != 0ull); left; left &= left - 1ull) {
                            const int r = __ffsll((long long)left) - 1;
                            const unsigned long long word = wave_readlane_ll(mine, r), v = wave_readlane_ll(value, r);
                            add += ((word >> lane) & 1ull) ? v : 0ull;     // (both read before the select: no cross-lane
                                                                           // read under a lane-divergent branch)
                        }
                        if (add) atomicAdd(&ha_cells[w * 64 + lane], add);
                    }
                }
            });
            if (over && lane == 0) atomicMax(overflow, 1);
        }
        all_s = (unsigned long long)wave_sum_ll((long long)all_s);
        ref_s = (unsigned long long)wave_sum_ll((long long)ref_s);
        if (lane == 0 && all_s) atomicAdd(&all_sum, all_s);
        if (lane == 0 && ref_s) atomicAdd(&ref_sum, ref_s);
        __syncthreads();
        // ---- 4. the block's cells of the region's row
        const unsigned long long every = all_sum;
        unsigned long long *row = sums + (size_t)run.region * (size_t)(H + 1);
        for (int hl = threadIdx.x; hl < nw * 64 && h0 + hl < H; hl += kHsThreads) {
            const unsigned long long a = every + ha_cells[hl];
            if (run.single) row[h0 + hl] = a;
            else if (a) atomicAdd(&row[h0 + hl], a);
        }
        if (blockIdx.y == 0 && threadIdx.x == 0) {
            const unsigned long long a = every + ref_sum;
            if (run.single) row[H] = a;
            else if (a) atomicAdd(&row[H], a);
        }
    }
}

}  // namespace

GFM_API int gfm_graph_haplotype_affinity(gfm_graph_t g, const gfm_motif_t *motifs, int32_t n_motifs,
                                         const uint64_t *const *d_weights, uint64_t max_weight, int32_t n_regions,
                                         const int64_t *h_starts, const int64_t *h_stops, uint32_t flags, uint64_t *const *d_sums,
                                         int32_t *d_overflow, int32_t windows_per_run, int32_t haplotypes_per_block, void *stream)
{
    if (!g) return gfail(GFM_ERR_INVALID, "graph is NULL");
    if (!has_haplotypes(*g)) return fail_no_haplotypes("gfm_graph_haplotype_affinity");
    if (!motifs || n_motifs < 1 || n_regions < 0 || (n_regions && (!h_starts || !h_stops)) || !d_weights || !d_sums || !d_overflow)
        return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    HsShape shape;
    if (const int rc = hs_run_shape(g->dev.n_hap, windows_per_run, haplotypes_per_block, shape)) return rc;
    for (int m = 0; m < n_motifs; ++m)
        if (!motifs[m] || !d_weights[m] || !d_sums[m]) return gfail(GFM_ERR_INVALID, "NULL motif / device buffer");
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::PackedTable, ms)) return rc;
    const int W = ms.W;
    if (const int rc = check_regions(n_regions, h_starts, h_stops)) return rc;
    // the capacity of a cell: a haplotype has at most one row per strand and base of its own sequence that starts in the
    // region -- the region's reference bases and, at most, every inserted base of the graph
    const long long ref_len = g->dev.ref_len;
    unsigned long long inserted = 0;
    for (const int il : g->host.ins_len) inserted += (unsigned long long)il;
    for (int r = 0; r < n_regions; ++r) {
        const long long len = std::min<long long>(h_stops[r], ref_len) - std::max<long long>(h_starts[r], 0);
        if (len <= 0) continue;
        const unsigned __int128 rows_bound = (unsigned __int128)2 * ((unsigned __int128)len + inserted);
        if (rows_bound * max_weight > (unsigned __int128)UINT64_MAX)
            return gfail(GFM_ERR_INVALID, "gfm_graph_haplotype_affinity: region " + std::to_string(r) + " may hold " +
                                          std::to_string((unsigned long long)rows_bound) + " rows per haplotype: with weights up "
                                          "to " + std::to_string((unsigned long long)max_weight) + " a sum may pass 2^64 - 1");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = g->serialise(st)) return rc;
    long long n_runs = 0;
    if (const int rc = hs_stage_runs(g, n_regions, h_starts, h_stops, W, windows_per_run, st, &n_runs)) return rc;
    if (n_runs > 0) {
        const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0, hb = shape.hb;
        const HsRun *runs = static_cast<const HsRun *>(g->v_wins);
        for (int m = 0; m < n_motifs; ++m) {
            hipLaunchKernelGGL(graph_hapaffinity_kernel, shape.grid(n_runs), dim3(kHsThreads), sizeof(unsigned long long) * (size_t)hb,
                               st, g->dev, ms.ftab[m], reinterpret_cast<const unsigned long long *>(d_weights[m]), W, ms.min_val[m],
                               runs, n_runs, fwd, hb, reinterpret_cast<unsigned long long *>(d_sums[m]), d_overflow);
            GX_TRY(hipGetLastError());
        }
    }
    return g->called(st);
}
