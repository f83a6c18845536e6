// gfm_graph_hapscores.hpp -- the per-haplotype best motif score: for every region of the caller's list and every haplotype
// of the graph, the highest-scoring k-mer of the haplotype's own sequence in the region, with no threshold and no hit list
// (included at the end of graph_extract.hip behind gfm_graph_variant.hpp: it enumerates a window's walks as
// graph_variant_kernel does -- for_window_layouts, replay_walk -- and scores with the motif's packed two-strand table of the
// fused path.  This kernel keeps its OWN window loops, min_val selects and reference test instead of
// gfm_graph_table_score.hpp's window_sum / strand_scores / walk_is_reference: with them it measured 0.4 % to 3.8 % slower than
// the parent at a run-to-run spread of 0.01 ms in 14.7 -- profiles/table_entries_refactor_ab.txt; a change to the scoring
// rule is made here as well as there).
//
// Rows(r, h) are the report's threshold-1 rows of region r whose walk haplotype h CARRIES (h is in the AND of the bitsets of
// the walk's allele constraints, the set whose popcount is haplotype_frequency).  The best row is the one with the largest
// 64-bit key (hs_key): the scaled score, then the smaller left coordinate (the '+' row's start), then the smaller right
// coordinate (the '+' row's stop), then '+' before '-'.  A region without a row for h keeps the caller's 0.  Column n_hap
// is the reference path: the walks whose constraints are all allele 0, whether or not a haplotype carries them.
//
// Work decomposition: a WORKGROUP per (run of consecutive window starts of one region, block of haplotypes).
//   1. plain windows -- no site in reach, no covering deletion, no insertion anchored at p - 1: one walk that every haplotype
//      carries -- a thread each, scored straight from the reference bases, into one "everyone" key;
//   2. the other windows a WAVEFRONT each (the waves take the run's windows in turn): the layout odometer in step over the
//      wave, the lanes take the walks 64 at a time, one simulate<DelEmit> replay plus one packed-table lookup per base gives
//      both strands' keys.  A walk without a constraint raises the everyone key; one whose constraints are all allele 0
//      raises the reference key; every walk with a constraint becomes a record (its better strand's key, its constraints) in
//      the wave's LDS queue;
//   3. the wave's carrier pass over its queued records: each lane owns the haplotypes lane, lane + 64, ... of the block; per
//      record and bitset word the 64 lanes read the SAME constraint words (broadcast), test their own bit and raise their
//      haplotype's key in LDS (ds_max_u64: the four waves share the block's keys).  A record whose key raises no lane's key
//      is skipped without a load;
//   4. the block's keys go to keys[region][n_hap + 1]: a plain store when the run is the region's only one, else a 64-bit
//      atomicMax (order-free: the result does not depend on the decomposition).
namespace {

constexpr int kHsThreads = 256;
constexpr int kHsWaves = kHsThreads / 64;
constexpr int kHsPool = 1024;                     // constraint words of a wave's record queue (a walk has at most kMaxConstraints)
constexpr int kHsMaxRun = 1024;                   // window starts of one run (the LDS flags of its plain windows)
constexpr int kHsDefaultRun = 256;
constexpr int kHsMaxBlockHaps = 4096;             // haplotypes of one block: 8 bytes of LDS each
constexpr long long kHsMaxWalks = kVarMaxWalks;   // walks of one window (beyond: *d_overflow = 1), as in the variant table
// key fields: score (16 bits), left - region start (28 bits), right - left (19 bits), '+' (1 bit); the coordinates stored
// so that SMALLER ones give larger keys, and the left field never 0, so that a row's key is never 0 (the caller's "none")
constexpr int kHsLeftBits = 28, kHsSpanBits = 19;
constexpr long long kHsLeftMax = (1ll << kHsLeftBits) - 1, kHsSpanMax = (1ll << kHsSpanBits) - 1;
static_assert(16 + kHsLeftBits + kHsSpanBits + 1 == 64, "the key's fields fill 64 bits");

struct HsRun { long long p0, p1, limit, base; int region, single; long long pad; };   // starts [p0, p1), walks end <= limit
static_assert(sizeof(HsRun) % sizeof(VarWin) == 0, "runs are staged in the variant table's window buffer");

__device__ __forceinline__ unsigned long long hs_key(int score, long long left, long long right, bool plus, long long base)
{
    return ((unsigned long long)score << 48) | ((unsigned long long)(kHsLeftMax - (left - base)) << (kHsSpanBits + 1)) |
           ((unsigned long long)(kHsSpanMax - (right - left)) << 1) | (plus ? 1ull : 0ull);
}

__device__ __forceinline__ unsigned long long hs_walk_key(unsigned sum, int bad, int min_val, long long left, long long right,
                                                          int forward_only, long long base)
{
    const unsigned long long kp = hs_key(bad ? min_val : (int)(sum & 0xffffu), left, right, true, base);
    if (forward_only) return kp;
    const unsigned long long km = hs_key(bad ? min_val : (int)(sum >> 16), left, right, false, base);
    return kp > km ? kp : km;
}

// the wave's carrier pass over n_rec queued records (keys rk, constraints at pool[ro .. ro + rn)): the block's bitset words
// w0 .. w0 + nw, lane `lane` of word w owning block haplotype w * 64 + lane
__device__ inline void hs_carriers(const GraphDev &g, int w0, int nw, int n_rec, const unsigned long long *rk, const int *ro,
                                   const int *rn, const int *pool, unsigned long long *keys_lds)
{
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < n_rec; ++r) {
        const unsigned long long key = rk[r];
        const int off = ro[r], n = rn[r];
        for (int w = 0; w < nw; ++w) {
            const int hl = w * 64 + lane;
            const unsigned long long cur = keys_lds[hl];        // (may be stale: the atomic settles it)
            if (!__builtin_amdgcn_ballot_w64(key > cur)) continue;
            auto at = [&](int c, int &site, int &al) { unpack_constraint(pool[off + c], site, al); };
            const unsigned long long acc = carrier_word<true>(g, n, at, w0 + w);
            if (((acc >> lane) & 1ull) && key > cur) atomicMax(&keys_lds[hl], key);
        }
    }
}

__global__ void __launch_bounds__(kHsThreads)
graph_hapscore_kernel(GraphDev g, const unsigned *__restrict__ ftab, int W, int min_val, const HsRun *__restrict__ runs,
                      long long n_runs, int forward_only, int hb, unsigned long long *__restrict__ keys, int *__restrict__ overflow)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long hs_keys[];       // [hb]
    __shared__ unsigned long long q_key[kHsWaves][64];
    __shared__ int q_off[kHsWaves][64], q_n[kHsWaves][64];
    __shared__ int q_pool[kHsWaves][kHsPool];
    __shared__ unsigned char plain_win[kHsMaxRun];
    __shared__ unsigned long long all_key, ref_key;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = g.n_hap, h0 = (int)blockIdx.y * hb;
    const int w0 = h0 >> 6, nw = min(g.hw - w0, hb >> 6);
    for (long long ri = blockIdx.x; ri < n_runs; ri += gridDim.x) {
        const HsRun run = runs[ri];
        const int n_win = (int)(run.p1 - run.p0);
        __syncthreads();                                     // (the last run's keys are written)
        for (int i = threadIdx.x; i < nw * 64; i += kHsThreads) hs_keys[i] = 0ull;
        if (threadIdx.x == 0) { all_key = 0ull; ref_key = 0ull; }
        unsigned long long all_k = 0ull, ref_k = 0ull;
        // ---- 1. plain windows, a thread each
        for (int k = threadIdx.x; k < n_win; k += kHsThreads) {
            const long long p = run.p0 + k;
            const int i0 = lower_bound_pos(g.pos, g.n_sites, p);
            bool plain = (i0 >= g.n_sites || (long long)g.pos[i0] >= p + W) && !covered_by_deletion(g, p, i0);
            for (int j = i0 - 1; plain && j >= 0 && g.pos[j] == p - 1; --j)
                if (g.ins_len[j] > 0) plain = false;
            plain_win[k] = plain ? 1 : 0;
            if (plain && p + W <= run.limit) {
                unsigned sum = 0u;
                int bad = 0;
                for (int j = 0; j < W; ++j) {
                    const unsigned c = base_code(g.ref[p + j]);
                    sum += ftab[j * 8 + (c & 7u)];
                    bad |= (int)(c >> 2);
                }
                const unsigned long long key = hs_walk_key(sum, bad, min_val, p, p + W, forward_only, run.base);
                all_k = key > all_k ? key : all_k;
            }
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
                    int nc = 0;                     // constraints this lane queues
                    unsigned long long key = 0ull;
                    if (q < prod) {
                        const long long end = replay_walk<kHsMaxWalks>(g, p, W, i0, ws, st, q, prod, run.limit, em);
                        unsigned sum = 0u;
                        int bad = 0;
                        for (int j = 0; j < W; ++j) {
                            const unsigned c = base_code(src[j] >= 0 ? g.ref[src[j]] : km[j]);
                            sum += ftab[j * 8 + (c & 7u)];
                            bad |= (int)(c >> 2);
                        }
                        key = hs_walk_key(sum, bad, min_val, p, end, forward_only, run.base);
                        bool ref = true;
                        for (int c = 0; c < em.n_cons; ++c)
                            if (em.get(c) & 3) ref = false;
                        if (em.n_cons == 0) all_k = key > all_k ? key : all_k;       // a walk over no site: everyone's
                        else nc = em.n_cons;
                        if (ref) ref_k = key > ref_k ? key : ref_k;
                    }
                    // queue the records (in pieces that fit the pool) and run the carrier pass over them
                    const int incl = wave_prefix_sum(nc), ex = incl - nc;
                    const int total_c = __shfl(incl, 63);
                    for (int done = 0; done < total_c;) {
                        const bool mine = nc > 0 && ex >= done && incl <= done + kHsPool;
                        const unsigned long long bal = __builtin_amdgcn_ballot_w64(mine);
                        if (mine) {
                            const int slot = __popcll(bal & ((1ull << lane) - 1ull));
                            q_key[wave][slot] = key;
                            q_off[wave][slot] = ex - done;
                            q_n[wave][slot] = nc;
                            for (int c = 0; c < nc; ++c) q_pool[wave][ex - done + c] = em.get(c);
                        }
                        wave_lds_sync();
                        hs_carriers(g, w0, nw, __popcll(bal), q_key[wave], q_off[wave], q_n[wave], q_pool[wave], hs_keys);
                        done = __shfl(incl, 63 - __clzll(bal));
                        wave_lds_sync();
                    }
                }
            });
            if (over && lane == 0) atomicMax(overflow, 1);
        }
        if (all_k) atomicMax(&all_key, all_k);
        if (ref_k) atomicMax(&ref_key, ref_k);
        __syncthreads();
        // ---- 4. the block's cells of the region's row
        const unsigned long long every = all_key;
        unsigned long long *row = keys + (size_t)run.region * (size_t)(H + 1);
        for (int hl = threadIdx.x; hl < nw * 64 && h0 + hl < H; hl += kHsThreads) {
            const unsigned long long k = hs_keys[hl] > every ? hs_keys[hl] : every;
            if (run.single) row[h0 + hl] = k;
            else if (k) atomicMax(&row[h0 + hl], k);
        }
        if (blockIdx.y == 0 && threadIdx.x == 0) {
            const unsigned long long k = ref_key > every ? ref_key : every;
            if (run.single) row[H] = k;
            else if (k) atomicMax(&row[H], k);
        }
    }
}

}  // namespace

// The runs of a call: every region's window starts [s, e - tail] cut into pieces of windows_per_run (0: kHsDefaultRun),
// staged in the variant table's window buffer of the handle (both are lists of the handle's last call) and uploaded on
// `st` -> *n_runs; the list is at g->v_wins.
static int hs_stage_runs(gfm_graph *g, int32_t n_regions, const int64_t *h_starts, const int64_t *h_stops, int W,
                         int32_t windows_per_run, hipStream_t st, long long *n_runs)
{
    const long long ref_len = g->dev.ref_len;
    const long long per_run = windows_per_run > 0 ? windows_per_run : kHsDefaultRun;
    const long long tail = g->dev.n_ins > 0 ? 1 : W;
    constexpr size_t kWords = sizeof(HsRun) / sizeof(long long);
    if (g->call_pending) GX_TRY(hipEventSynchronize(g->ev_call));      // the last call's upload may still read h_vwins
    g->h_vwins.clear();
    for (int r = 0; r < n_regions; ++r) {
        const long long s = std::max<long long>(h_starts[r], 0), e = std::min<long long>(h_stops[r], ref_len);
        const long long last = e - tail;
        if (last < s) continue;
        const long long pieces = (last - s + per_run) / per_run;
        for (long long p0 = s; p0 <= last; p0 += per_run) {
            const HsRun run{p0, std::min(p0 + per_run, last + 1), e, s, r, pieces == 1 ? 1 : 0, 0};
            const long long *w = reinterpret_cast<const long long *>(&run);
            g->h_vwins.insert(g->h_vwins.end(), w, w + kWords);
        }
    }
    *n_runs = (long long)(g->h_vwins.size() / kWords);
    return upload_vwins(g, st);
}

// The run shape of a call of the two run entries, checked -> the haplotypes of one block (the caller's, or (0) as few blocks
// as the LDS allows, split evenly) and the grid: the runs by the blocks of the graph's H haplotypes.
struct HsShape {
    int hb = 0;
    unsigned blocks = 0;
    dim3 grid(long long n_runs) const { return dim3((unsigned)std::min<long long>(n_runs, 1 << 16), blocks); }
};
static int hs_run_shape(int H, int32_t windows_per_run, int32_t haplotypes_per_block, HsShape &shape)
{
    if (windows_per_run < 0 || windows_per_run > kHsMaxRun)
        return gfail(GFM_ERR_INVALID, "windows_per_run outside 0 .. " + std::to_string(kHsMaxRun));
    if (haplotypes_per_block < 0 || haplotypes_per_block > kHsMaxBlockHaps || haplotypes_per_block % 64)
        return gfail(GFM_ERR_INVALID, "haplotypes_per_block: 0 or a multiple of 64 up to " + std::to_string(kHsMaxBlockHaps));
    const int blocks = (H + kHsMaxBlockHaps - 1) / kHsMaxBlockHaps;
    shape.hb = haplotypes_per_block ? haplotypes_per_block : ((H + blocks - 1) / blocks + 63) / 64 * 64;
    shape.blocks = (unsigned)((H + shape.hb - 1) / shape.hb);
    return GFM_OK;
}

GFM_API int gfm_graph_haplotype_scores(gfm_graph_t g, const gfm_motif_t *motifs, int32_t n_motifs, int32_t n_regions,
                                       const int64_t *h_starts, const int64_t *h_stops, uint32_t flags, uint64_t *const *d_keys,
                                       int32_t *d_overflow, int32_t windows_per_run, int32_t haplotypes_per_block, void *stream)
{
    if (!g) return gfail(GFM_ERR_INVALID, "graph is NULL");
    if (!has_haplotypes(*g)) return fail_no_haplotypes("gfm_graph_haplotype_scores");
    if (!motifs || n_motifs < 1 || n_regions < 0 || (n_regions && (!h_starts || !h_stops)) || !d_keys || !d_overflow)
        return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    HsShape shape;
    if (const int rc = hs_run_shape(g->dev.n_hap, windows_per_run, haplotypes_per_block, shape)) return rc;
    for (int m = 0; m < n_motifs; ++m)
        if (!motifs[m] || !d_keys[m]) return gfail(GFM_ERR_INVALID, "NULL motif / device buffer");
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::Key, ms)) return rc;
    const int W = ms.W;
    if (const int rc = check_regions(n_regions, h_starts, h_stops)) return rc;
    // the key's coordinate fields: a region's start offsets below 2^28 - 1, a walk's span (at most W bases plus W - 1 jumped
    // deletions, and never beyond the region) within 2^19 - 1
    const long long ref_len = g->dev.ref_len, walk_span = (long long)W + (long long)(W - 1) * g->max_del_len;
    for (int r = 0; r < n_regions; ++r) {
        const long long len = std::min<long long>(h_stops[r], ref_len) - std::max<long long>(h_starts[r], 0);
        if (len > kHsLeftMax)
            return gfail(GFM_ERR_INVALID, "gfm_graph_haplotype_scores: region " + std::to_string(r) + " is longer than 2^28 - 1 "
                                          "bases (the key's coordinate field)");
        if (std::min(len, walk_span) > kHsSpanMax)
            return gfail(GFM_ERR_INVALID, "gfm_graph_haplotype_scores: a walk of region " + std::to_string(r) + " may span more "
                                          "than 2^19 - 1 bases (a deletion too long for the key's coordinate field)");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = g->serialise(st)) return rc;
    long long n_runs = 0;
    if (const int rc = hs_stage_runs(g, n_regions, h_starts, h_stops, W, windows_per_run, st, &n_runs)) return rc;
    if (n_runs > 0) {
        const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0, hb = shape.hb;
        const HsRun *runs = static_cast<const HsRun *>(g->v_wins);
        for (int m = 0; m < n_motifs; ++m) {
            hipLaunchKernelGGL(graph_hapscore_kernel, shape.grid(n_runs), dim3(kHsThreads), sizeof(unsigned long long) * (size_t)hb,
                               st, g->dev, ms.ftab[m], W, ms.min_val[m], runs, n_runs, fwd, hb,
                               reinterpret_cast<unsigned long long *>(d_keys[m]), d_overflow);
            GX_TRY(hipGetLastError());
        }
    }
    return g->called(st);
}
