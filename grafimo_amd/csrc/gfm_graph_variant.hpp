// gfm_graph_variant.hpp -- per-variant motif effects: the best REF and the best ALT k-mer of every (site, allele) of the graph
// (included at the end of graph_extract.hip behind gfm_graph_table_score.hpp, whose window_sum and ConstraintAt it uses: it
// walks the graph with the machinery the extraction kernels share -- simulate(), DelEmit, for_covering_deletions,
// allele_word -- and scores with the motif's packed table of the fused path).
//
// What a k-mer qualifies for: the (site, allele) pairs its walk carries a haplotype CONSTRAINT for in the existing counting
// (DelEmit: a substitution base it reads, an insertion it reads or passes by, a deletion it jumps or whose bases it uses,
// a deletion that removes the window's first base) -- exactly the allele footprints the table is defined on.  Without
// --recomb a walk counts only if some haplotype carries it (the report's GFM_HITS_DROP_ZERO_FREQ rule).
//
// Work decomposition: the host lists the windows that can meet a site at all (window starts within reach of a site's
// footprint, inside the regions' window ranges); a WAVEFRONT per window.  The wave runs the window's layout odometer in
// step (every lane the same simulate() calls: uniform control flow), and on each layout its lanes take the walks 64 at a
// time: one replay with DelEmit gives the bases and the constraints, one lookup per base in the packed table gives both
// strands' scores.  Per (strand, constraint) a 64-bit key -- score, -start, -stop, '+' -- goes into the global key array
// by atomicMax (pass 0).  The haplotype presence test (an AND of the constraints' bitsets, stopped at the first non-zero
// word) is made only for a walk that would raise one of the maxima it covers.  Pass 1 replays the same walks and appends
// every one whose key EQUALS its slot's maximum as a record (coordinates, strand, k-mer): ties on the key are walks over the
// same coordinates, and the host picks the smallest k-mer among them (gfm_variant_effect_columns).
namespace {

// Walks of one window (beyond: *d_overflow = 1, the window is left out and the caller refuses the table).  Lower than the
// report's limits (2^30 rows per plan, 2^40 walks per window in gfm_graph_score) on purpose: here ONE wavefront replays
// every walk of a window through simulate(), twice, and a window of 2^24 walks is already ~2.6e5 rounds of one wave (seconds);
// at 2^30 or 2^40 one launch would occupy the device for minutes to days.  The report's heavy-window path (graph_heavy_kernel:
// a window's walks split over the whole grid, digits instead of replays) is what a higher limit would need.
constexpr long long kVarMaxWalks = 1ll << 24;
constexpr int kVarThreads = 64;
// key fields: score (16 bits), start and stop relative to the site's position (24 / 23 bits, stored so that SMALLER
// coordinates give larger keys), strand ('+' = 1)
constexpr long long kVarStartBias = 1ll << 23, kVarStopBias = 1ll << 22;

struct VarWin { long long p, limit; };

__device__ __forceinline__ unsigned long long variant_key(int score, long long start, long long stop, bool plus, long long site_pos)
{
    const unsigned long long fs = (unsigned long long)((2 * kVarStartBias - 1) - (start - site_pos + kVarStartBias));
    const unsigned long long fe = (unsigned long long)((2 * kVarStopBias - 1) - (stop - site_pos + kVarStopBias));
    return ((unsigned long long)score << 48) | (fs << 24) | (fe << 1) | (plus ? 1ull : 0ull);
}

// some haplotype carries every allele of the walk's constraints (count > 0), stopped at the first non-zero word
template <class F>
__device__ inline bool present_by_bitsets(const GraphDev &g, int n, F at)
{
    if (!g.alt_bits || g.n_hap <= 0) return false;
    for (int word = 0; word < g.hw; ++word)
        if (carrier_word<true>(g, n, at, word)) return true;
    return false;
}

// Every layout of window p, in the enumeration's order: the starts (plain, then inside the insertions anchored at p - 1),
// per start the layout odometer; body(ws, st, prod) per layout that exists, prod = its walks.  Uniform over a wavefront
// whose lanes all call it.  -> true: the window holds more than MAXW walks (or a layout does, or a walk decides too
// often), the enumeration was left there.
template <long long MAXW, class B>
__device__ __forceinline__ bool for_window_layouts(const GraphDev &g, long long p, int W, int i0, long long limit, B body)
{
    const GlobalSites sites{g.site_rec};
    WalkStart ws;
    long long total = 0;
    for (;;) {
        WalkState st;
        NoVisitor nv;
        int prefix = 0;
        for (;;) {
            long long prod = 0;
            const int rc = simulate<NoVisitor, GlobalSites, MAXW>(g, sites, p, W, i0, ws, prefix, st, nv, 0, 0, prod, limit);
            if (rc == WALK_OVERFLOW) return true;
            if (rc == WALK_OK) {
                total += prod;
                if (total > MAXW) return true;
                body(ws, st, prod);
            }
            prefix = next_walk(st);
            if (prefix < 0) break;
        }
        if (!next_start(g, p, i0, ws)) return false;
    }
}

// Walk q of the prod walks of layout (ws, st) replayed into `em`: its bases (src[j] >= 0: reference base src[j], to be
// fetched) and its constraints, those of the deletions that cover the window's first base included (not for a walk that
// never leaves the insertion it starts in) -> the position behind its last base.
template <long long MAXW>
__device__ __forceinline__ long long replay_walk(const GraphDev &g, long long p, int W, int i0, const WalkStart &ws,
                                                 const WalkState &st, long long q, long long prod, long long limit, DelEmit &em)
{
    WalkState s2 = st;
    long long again = 0;
    simulate<DelEmit, GlobalSites, MAXW>(g, GlobalSites{g.site_rec}, p, W, i0, ws, st.nd, s2, em, q, prod, again, limit);
    if (!(ws.site >= 0 && s2.last == p - 1)) for_covering_deletions(g, p, i0, [&](int d) { em.add(d, 0); });
    return s2.last + 1;
}

template <bool RESOLVE>
__global__ void __launch_bounds__(kVarThreads)
graph_variant_kernel(GraphDev g, const unsigned *__restrict__ ftab, int W, int min_val, const VarWin *__restrict__ wins,
                     long long n_wins, int forward_only, int keep_zero, unsigned long long *__restrict__ keys,
                     gfm_variant_rec_t *__restrict__ recs, unsigned long long *__restrict__ rec_count, long long rec_cap,
                     int *__restrict__ overflow)
{
    const int lane = threadIdx.x;
    for (long long wi = blockIdx.x; wi < n_wins; wi += gridDim.x) {
        const VarWin vw = wins[wi];
        const long long p = vw.p, limit = vw.limit;
        const int i0 = lower_bound_pos(g.pos, g.n_sites, p);
        const bool over = for_window_layouts<kVarMaxWalks>(g, p, W, i0, limit, [&](const WalkStart &ws, const WalkState &st,
                                                                                   long long prod) {
            for (long long q = lane; q < prod; q += kVarThreads) {
                uint8_t km[GFM_MAX_WIDTH], kr[GFM_MAX_WIDTH];
                int src[GFM_MAX_WIDTH];
                int more[kMaxConstraints - 4];
                DelEmit em(g, km, kr, src, W, more);
                const long long end = replay_walk<kVarMaxWalks>(g, p, W, i0, ws, st, q, prod, limit, em);
                if (em.n_cons == 0) continue;  // a walk over no site: no allele's footprint
                const StrandScores ss = strand_scores(window_sum(ftab, W, [&](int j) {        // (and the k-mers are completed)
                    if (src[j] >= 0) {
                        km[j] = g.ref[src[j]];
                        kr[W - 1 - j] = complement(km[j]);
                    }
                    return base_code(km[j]);
                }), min_val);
                const int sc[2] = {ss.plus, ss.minus};
                const ConstraintAt at{em};
                int present = keep_zero ? 1 : -1;      // -1: not tested yet
                for (int sd = 0; sd < (forward_only ? 1 : 2); ++sd) {
                    const long long start = sd ? end : p, stop = sd ? p : end;
                    for (int k = 0; k < em.n_cons; ++k) {
                        int site, al;
                        at(k, site, al);
                        const size_t slot = (size_t)site * 4 + (size_t)al;
                        const unsigned long long key = variant_key(sc[sd], start, stop, sd == 0, g.pos[site]);
                        const unsigned long long cur = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
                        if (RESOLVE ? key != cur : key <= cur) continue;
                        if (present < 0) present = present_by_bitsets(g, em.n_cons, at) ? 1 : 0;
                        if (!present) break;
                        if constexpr (!RESOLVE) {
                            atomicMax(&keys[slot], key);
                        } else {
                            const unsigned long long r = atomicAdd(rec_count, 1ull);
                            if ((long long)r < rec_cap) {
                                gfm_variant_rec_t &o = recs[r];
                                o.slot = (int32_t)slot;
                                o.score = sc[sd];
                                o.start = start;
                                o.stop = stop;
                                o.strand = sd ? '-' : '+';
                                for (int j = 0; j < W; ++j) o.kmer[j] = sd ? kr[j] : km[j];
                            }
                        }
                    }
                    if (present == 0) break;
                }
            }
        });
        if (over && lane == 0) atomicMax(overflow, 1);
    }
}

}  // namespace

// g->h_vwins, the window (or run) list of a call, into g->v_wins on `st`; the buffer grows to hold it
static int upload_vwins(gfm_graph_t g, hipStream_t st)
{
    static_assert(sizeof(VarWin) == 2 * sizeof(long long), "h_vwins holds (p, limit) pairs");
    const size_t n_vw = g->h_vwins.size() / 2;
    if (n_vw == 0) return GFM_OK;
    if (n_vw > g->v_cap) {
        if (g->v_wins) GX_TRY(hipFree(g->v_wins));
        g->v_wins = nullptr;
        g->v_cap = 0;
        GX_TRY(hipMalloc(&g->v_wins, sizeof(VarWin) * n_vw));
        g->v_cap = n_vw;
    }
    GX_TRY(hipMemcpyAsync(g->v_wins, g->h_vwins.data(), sizeof(VarWin) * n_vw, hipMemcpyHostToDevice, st));
    return GFM_OK;
}

// The windows within reach of a site: starts in [pos - W + 1, pos + 1 + del_len] (a walk that starts inside an insertion
// anchored at p - 1, on bases a deletion anchored before p removes), merged, cut to every region's window range -> *n_win
// (start, limit) pairs at g->v_wins, uploaded on `st`.  `unique`: a start that several regions hold is listed once, with the
// largest limit among them (a walk valid under a smaller limit is valid under a larger one: the union of the regions' walks).
static int variant_stage_windows(gfm_graph_t g, int W, int n_regions, const int64_t *h_starts, const int64_t *h_stops, bool unique,
                                 hipStream_t st, long long *n_win_out)
{
    const std::vector<int> &pos = g->host.pos;
    std::vector<std::pair<long long, long long>> iv;
    for (size_t i = 0; i < pos.size(); ++i) {
        const long long lo = (long long)pos[i] - W + 1, hi = (long long)pos[i] + 1 + std::max(0, g->host.del_len[i]);
        if (!iv.empty() && lo <= iv.back().second + 1) iv.back().second = std::max(iv.back().second, hi);
        else iv.emplace_back(lo, hi);
    }
    if (g->call_pending) GX_TRY(hipEventSynchronize(g->ev_call));      // the last call's upload may still read h_vwins
    g->h_vwins.clear();
    const long long tail = g->dev.n_ins > 0 ? 1 : W;
    for (int r = 0; r < n_regions; ++r) {
        const long long s = std::max<long long>(h_starts[r], 0), e = std::min<long long>(h_stops[r], g->dev.ref_len);
        const long long last = e - tail;
        if (last < s) continue;
        size_t k = (size_t)(std::lower_bound(iv.begin(), iv.end(), std::make_pair(s, LLONG_MIN),
                                             [](const std::pair<long long, long long> &a, const std::pair<long long, long long> &b) {
                                                 return a.second < b.first;
                                             }) - iv.begin());
        for (; k < iv.size() && iv[k].first <= last; ++k)
            for (long long p = std::max(s, iv[k].first); p <= std::min(last, iv[k].second); ++p) {
                g->h_vwins.push_back(p);
                g->h_vwins.push_back(e);
            }
    }
    if (unique && !g->h_vwins.empty()) {
        VarWin *b = reinterpret_cast<VarWin *>(g->h_vwins.data()), *e = b + g->h_vwins.size() / 2;
        std::sort(b, e, [](const VarWin &x, const VarWin &y) { return x.p != y.p ? x.p < y.p : x.limit > y.limit; });
        e = std::unique(b, e, [](const VarWin &x, const VarWin &y) { return x.p == y.p; });
        g->h_vwins.resize(2 * (size_t)(e - b));
    }
    *n_win_out = (long long)(g->h_vwins.size() / 2);
    return upload_vwins(g, st);
}

GFM_API int gfm_graph_variant_effects(gfm_graph_t g, const gfm_motif_t *motifs, int32_t n_motifs, int32_t n_regions,
                                      const int64_t *h_starts, const int64_t *h_stops, uint32_t flags,
                                      uint64_t *const *d_keys, void *const *d_recs, const int64_t *rec_capacity,
                                      uint64_t *const *d_rec_count, int32_t *d_overflow, int64_t *n_windows, void *stream)
{
    if (!g || !motifs || n_motifs < 1 || n_regions < 0 || (n_regions && (!h_starts || !h_stops)))
        return gfail(GFM_ERR_INVALID, "bad argument");
    if (!d_keys || !d_recs || !rec_capacity || !d_rec_count || !d_overflow) return gfail(GFM_ERR_INVALID, "NULL argument array");
    if (flags & ~(uint32_t)(GFM_GRAPH_FORWARD_ONLY | GFM_VARIANT_KEEP_ZERO_FREQ)) return gfail(GFM_ERR_INVALID, "unknown flag");
    for (int m = 0; m < n_motifs; ++m)
        if (!motifs[m] || !d_keys[m] || !d_rec_count[m] || rec_capacity[m] < 0 || (rec_capacity[m] && !d_recs[m]))
            return gfail(GFM_ERR_INVALID, "NULL motif / device buffer");
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::Key, ms)) return rc;
    const int W = ms.W;
    if (const int rc = check_regions(n_regions, h_starts, h_stops)) return rc;
    // a window's walks end within W bases plus the deletions they jump of their start: the key's coordinate fields hold that
    if ((long long)W * (g->max_del_len + 1) + W >= kVarStopBias)
        return gfail(GFM_ERR_INVALID, "a deletion too long for the variant table's coordinate fields");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = g->serialise(st)) return rc;
    long long n_win = 0;
    if (const int rc = variant_stage_windows(g, W, n_regions, h_starts, h_stops, false, st, &n_win)) return rc;
    if (n_windows) *n_windows = n_win;
    if (n_win > 0) {
        const int grid = (int)std::min<long long>(n_win, 1 << 16);
        const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0, keep0 = (flags & GFM_VARIANT_KEEP_ZERO_FREQ) ? 1 : 0;
        const VarWin *wins = static_cast<const VarWin *>(g->v_wins);
        for (int m = 0; m < n_motifs; ++m) {
            unsigned long long *keys = reinterpret_cast<unsigned long long *>(d_keys[m]);
            unsigned long long *cnt = reinterpret_cast<unsigned long long *>(d_rec_count[m]);
            gfm_variant_rec_t *recs = static_cast<gfm_variant_rec_t *>(d_recs[m]);
            hipLaunchKernelGGL(graph_variant_kernel<false>, dim3(grid), dim3(kVarThreads), 0, st, g->dev, ms.ftab[m], W, ms.min_val[m],
                               wins, n_win, fwd, keep0, keys, recs, cnt, (long long)rec_capacity[m], d_overflow);
            GX_TRY(hipGetLastError());
            hipLaunchKernelGGL(graph_variant_kernel<true>, dim3(grid), dim3(kVarThreads), 0, st, g->dev, ms.ftab[m], W, ms.min_val[m],
                               wins, n_win, fwd, keep0, keys, recs, cnt, (long long)rec_capacity[m], d_overflow);
            GX_TRY(hipGetLastError());
        }
    }
    return g->called(st);
}
