// gfm_graph_hapsequences.hpp -- haplotype sequences: the bases a haplotype spells in a region, for a list of (region, haplotype)
// pairs (included at the end of graph_extract.hip behind gfm_graph_hapclasses.hpp; it uses GraphDev, SiteRec, hc_mix64, the
// handle's serialise / called and has_haplotypes).
//
// THE RULE (tests/variant_bruteforce.py spell states it on the host).  Haplotype h spells one sequence over the chromosome by
// walking the reference: at a position the substitution it carries replaces the base (the first carried ALT in slot order); the
// FIRST insertion in site order it carries at that anchor is read behind the anchor, later ones at that anchor are not; if no
// insertion was read there, the first deletion it carries at that anchor jumps over its span; every site anchored on a
// jumped-over base is ignored.  Every spelled base has a coordinate -- its own reference position, or its anchor's if it was
// inserted -- and an inserted flag.  The region sequence of h in [S, E) clipped to the chromosome is the contiguous stretch of
// spelled bases with coord + inserted >= S and coord < E: exactly the bases a report row of the region can contain (start in
// [S, E), stop <= E).  A base inserted behind S - 1 belongs, the anchor S - 1 does not; bases inserted behind E - 1 belong; an
// empty region gives an empty sequence; a region wholly under a carried deletion gives an empty sequence or inserted bases only.
// Haplotype -1 is the reference: no ALT anywhere.
//
// The walk (hseq_walk) goes over the region's sites in index order and keeps x, the next reference position to spell, and cur,
// the anchor it stands on after a carried substitution (x == cur + 1, the insertions and deletions at cur are still to come).
// A site at p < x that is not at cur lies on a jumped-over base, or behind the insertion read / the jump made at its anchor:
// it is ignored.  It STARTS at a cut point x0 <= max(S - 1, 0) (S - 1: the anchor of an insertion the region holds) -- a
// position that no deletion among the earlier sites reaches (the host finds it from max_reach, stepping back over the
// deletions), so every haplotype spells the base x0 -- and not at S: a haplotype may carry a deletion upstream of the region
// whose span holds the anchor of another deletion that reaches into the region, which is then NOT made.  The site index range
// [lo, hi) is lower_bound(pos, x0) .. lower_bound(pos, E).
//
//   hseq_measure_kernel  a thread per pair: the walk with a sink that counts -> d_len; a bad pair (region index out of
//                        range, haplotype >= n_hap or < -1, a haplotype >= 0 on a graph without haplotypes, more than
//                        2^31 - 1 bases) sets bit 0 of the call's status word and has length 0.
//   hseq_fill_kernel     a wavefront per pair, the site loop wave-uniform (the pair index comes from blockIdx and a
//                        readfirstlane; the carrier bit of h is one word load per used ALT slot at word h >> 6).  Between two
//                        events the wave copies the run -- ref[x .. x + n) or the inserted bases -- lane-parallel: lane l
//                        takes the bytes l, l + 64, ...; byte loads and byte stores, 64 consecutive bytes a wave instruction,
//                        exact at every alignment of source and destination.  d_coord (optional): the coordinate,
//                        ~coordinate for an inserted base.  key(n) = the sum mod 2^64 over the bases of
//                        mix64(seed, offset << 8 | base), offset counted from the sequence's start, added up per lane, reduced
//                        across the wave, masked to key_bits.  Writes are bounded by d_len[n] and by [d_off[n], capacity):
//                        offsets that are not the scan of the lengths set bit 1 of the status word and write nothing out of
//                        bounds.  No LDS.
//   hseq_verify_kernel   graph-independent, a wavefront per sequence: sequence n against d_same_as[n], length first, then the
//                        bytes with the wave striding over them; a difference (or an index out of range) sets bit 0 of
//                        *d_status.  The key only speeds up the grouping: the result is exact.
namespace {

constexpr int kHseqThreads = 256;
constexpr int kHseqStatusPair = 1, kHseqStatusOffsets = 2;

struct HseqRegion {
    long long S, E;        // clipped to the chromosome; E <= S: empty
    long long x0;          // the cut point the walk starts at, <= max(S - 1, 0)
    int lo, hi;            // the sites with x0 <= pos < E
};

// what a walk spells goes to a sink: ref(a, b) the reference bases [a, b), ins(off, n, p) the n inserted bases at ins_bases + off
// behind the anchor p, sub(base, p) the ALT base at p -- the sink clips them to the region
template <typename Sink>
__device__ __forceinline__ void hseq_walk(const GraphDev &g, const HseqRegion &rg, int h, Sink &sink)
{
    long long x = rg.x0;
    if (h >= 0) {
        const int word = h >> 6, bit = h & 63;
        long long cur = -1;
        for (int i = rg.lo; i < rg.hi; ++i) {
            const SiteRec s = g.site_rec[i];
            const long long p = s.pos;
            if (p < x && p != cur) continue;
            const hc_u64 *w = g.alt_bits + ((size_t)i * 3) * g.hw + word;
            if (s.del_len > 0) {
                if (!((w[0] >> bit) & 1ull)) continue;
                if (p >= x) sink.ref(x, p + 1);
                x = p + 1 + s.del_len;
                cur = -1;
            } else if (s.ins_len > 0) {
                if (!((w[0] >> bit) & 1ull)) continue;
                if (p >= x) sink.ref(x, p + 1);
                x = p + 1;
                cur = -1;
                sink.ins(g.ins_off[i], s.ins_len, p);
            } else {
                int a = -1;
                for (int k = s.n_alts - 1; k >= 0; --k)
                    if ((w[(size_t)k * g.hw] >> bit) & 1ull) a = k;
                if (a < 0) continue;
                sink.ref(x, p);
                sink.sub(g.alt_bases[(size_t)i * 3 + a], p);
                x = p + 1;
                cur = p;
            }
        }
    }
    sink.ref(x, rg.E);
}

__device__ __forceinline__ bool hseq_pair_ok(const GraphDev &g, int n_regions, int r, int h)
{
    return r >= 0 && r < n_regions && h >= -1 && h < g.n_hap;       // (a graph without haplotypes has n_hap 0: only -1 passes)
}

struct HseqCount {
    long long S, E, n;
    __device__ __forceinline__ void ref(long long a, long long b)
    {
        a = a > S ? a : S;
        b = b < E ? b : E;
        if (b > a) n += b - a;
    }
    __device__ __forceinline__ void ins(int, int len, long long p) { if (p >= S - 1 && p < E) n += len; }
    __device__ __forceinline__ void sub(uint8_t, long long p) { if (p >= S && p < E) n += 1; }
};

__global__ void __launch_bounds__(kHseqThreads)
hseq_measure_kernel(GraphDev g, const HseqRegion *__restrict__ regions, int n_regions, long long n_seqs,
                    const int *__restrict__ seq_region, const int *__restrict__ seq_hap, int *__restrict__ len, int *__restrict__ status,
                    hc_u64 *__restrict__ total)
{
    const long long n = (long long)blockIdx.x * kHseqThreads + threadIdx.x;
    if (n >= n_seqs) return;
    const int r = seq_region[n], h = seq_hap[n];
    long long got = 0;
    bool bad = !hseq_pair_ok(g, n_regions, r, h);
    if (!bad) {
        const HseqRegion rg = regions[r];
        if (rg.E > rg.S) {
            HseqCount sink{rg.S, rg.E, 0};
            hseq_walk(g, rg, h, sink);
            got = sink.n;
        }
        if (got > 0x7fffffffll) { bad = true; got = 0; }
    }
    len[n] = (int)got;
    if (bad) atomicOr(status, kHseqStatusPair);
    else if (got) atomicAdd(total, (hc_u64)got);
}

struct HseqFill {
    const GraphDev &g;
    long long S, E;
    long long o;                 // the bases spelled so far (wave-uniform)
    long long limit;             // d_len[n]: nothing is written at or past it
    int lane;
    uint8_t *bases;              // the sequence's first byte
    int *coord;                  // its first coordinate, or nullptr
    hc_u64 seed, key;
    __device__ __forceinline__ void put(long long q, uint8_t b, int c)
    {
        if (q >= limit) return;
        bases[q] = b;
        if (coord) coord[q] = c;
        key += hc_mix64(seed, ((hc_u64)q << 8) | (hc_u64)b);
    }
    __device__ __forceinline__ void ref(long long a, long long b)
    {
        a = a > S ? a : S;
        b = b < E ? b : E;
        if (b <= a) return;
        const long long n = b - a;
        for (long long j = lane; j < n; j += 64) put(o + j, g.ref[a + j], (int)(a + j));
        o += n;
    }
    __device__ __forceinline__ void ins(int off, int len, long long p)
    {
        if (p < S - 1 || p >= E) return;
        for (int j = lane; j < len; j += 64) put(o + j, g.ins_bases[(size_t)off + j], ~(int)p);
        o += len;
    }
    __device__ __forceinline__ void sub(uint8_t base, long long p)
    {
        if (p < S || p >= E) return;
        if (lane == 0) put(o, base, (int)p);
        o += 1;
    }
};

__global__ void __launch_bounds__(kHseqThreads)
hseq_fill_kernel(GraphDev g, const HseqRegion *__restrict__ regions, int n_regions, long long n_seqs, const int *__restrict__ seq_region,
               const int *__restrict__ seq_hap, const int *__restrict__ len, const long long *__restrict__ off, long long capacity,
               uint8_t *__restrict__ bases, int *__restrict__ coord, hc_u64 seed, int key_bits, hc_u64 *__restrict__ keys,
               int *__restrict__ status)
{
    // the wave's pair: provably wave-uniform (blockIdx and a readfirstlane), so what the walk loads by it are scalar loads
    const long long n = (long long)blockIdx.x * (kHseqThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (n >= n_seqs) return;
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane(seq_region[n]), h = __builtin_amdgcn_readfirstlane(seq_hap[n]);
    const long long limit = len[n], at = off[n];
    hc_u64 key = 0ull;
    if (!hseq_pair_ok(g, n_regions, r, h)) {
        if (lane == 0) atomicOr(status, kHseqStatusPair);
    } else if (limit < 0 || at < 0 || at > capacity || limit > capacity - at) {
        if (lane == 0) atomicOr(status, kHseqStatusOffsets);
    } else if (limit > 0) {
        const HseqRegion rg = regions[r];
        if (rg.E > rg.S) {
            HseqFill sink{g, rg.S, rg.E, 0, limit, lane, bases + at, coord ? coord + at : nullptr, seed, 0ull};
            hseq_walk(g, rg, h, sink);
            key = sink.key;
            if (sink.o != limit && lane == 0) atomicOr(status, kHseqStatusOffsets);      // (the lengths are not this call's)
        }
    }
    for (int d = 32; d > 0; d >>= 1) key += (hc_u64)__shfl_xor((long long)key, d, 64);
    if (key_bits < 64) key &= (1ull << key_bits) - 1ull;
    if (lane == 0) keys[n] = key;
}

__global__ void __launch_bounds__(kHseqThreads)
hseq_verify_kernel(long long n_seqs, const long long *__restrict__ off, const uint8_t *__restrict__ bases, const int *__restrict__ same_as,
                 int *__restrict__ status)
{
    const long long n = (long long)blockIdx.x * (kHseqThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (n >= n_seqs) return;
    const int lane = threadIdx.x & 63;
    const long long m = same_as[n];
    if (m == n) return;
    bool bad = m < 0 || m >= n_seqs;
    if (!bad) {
        const long long a = off[n], b = off[m], len = off[n + 1] - a;
        if (len != off[m + 1] - b || len < 0) bad = true;
        else
            for (long long j = lane; j < len && !bad; j += 64) bad = bases[a + j] != bases[b + j];
    }
    if (__any(bad) && lane == 0) atomicOr(status, 1);
}

}  // namespace

GFM_API int gfm_graph_haplotype_sequences(gfm_graph_t g, int32_t n_regions, const int64_t *h_starts, const int64_t *h_stops,
                                          int64_t n_seqs, const int32_t *d_seq_region, const int32_t *d_seq_hap, int32_t *d_len,
                                          const int64_t *d_off, int64_t capacity, uint8_t *d_bases, int32_t *d_coord,
                                          uint64_t seed, int32_t key_bits, uint64_t *d_key, uint32_t flags, int64_t *h_total,
                                          void *stream)
{
    if (!g) return gfail(GFM_ERR_INVALID, "graph is NULL");
    if (n_regions < 0 || (n_regions && (!h_starts || !h_stops)) || n_seqs < 0 || n_seqs > 0x7fffffffll * (kHseqThreads / 64) ||
        (n_seqs && (!d_seq_region || !d_seq_hap || !d_len)) || capacity < 0 || (flags & ~GFM_SEQS_HAVE_LENGTHS))
        return gfail(GFM_ERR_INVALID, "bad argument");
    if (d_bases && n_seqs && (!d_off || !d_key)) return gfail(GFM_ERR_INVALID, "d_bases without d_off / d_key");
    if ((flags & GFM_SEQS_HAVE_LENGTHS) && !d_bases) return gfail(GFM_ERR_INVALID, "GFM_SEQS_HAVE_LENGTHS without d_bases");
    if (key_bits < 1 || key_bits > 64) return gfail(GFM_ERR_INVALID, "key_bits outside [1, 64]");
    for (int r = 0; r < n_regions; ++r)
        if (h_stops[r] < h_starts[r]) return gfail(GFM_ERR_INVALID, "a region ends before it starts");
    if (h_total) *h_total = 0;
    if (n_seqs == 0) return GFM_OK;
    if (n_regions == 0) return gfail(GFM_ERR_INVALID, "a region index out of range (there are no regions)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = g->serialise(st)) return rc;
    // ---- the regions: clipped, the cut point the walk starts at, the index range of the sites from there up to pos < E
    std::vector<HseqRegion> regs((size_t)n_regions);
    const std::vector<int> &pos = g->h_pos;
    const std::vector<long long> &reach = g->host.max_reach;
    const std::vector<int> &dels = g->host.del_len;
    auto first_at = [&](long long v) {
        return (int)(std::lower_bound(pos.begin(), pos.end(), v, [](int p, long long q) { return (long long)p < q; }) - pos.begin());
    };
    for (int r = 0; r < n_regions; ++r) {
        HseqRegion &x = regs[(size_t)r];
        x.S = std::max<long long>(h_starts[r], 0);
        x.E = std::min<long long>(h_stops[r], g->dev.ref_len);
        x.x0 = x.S;
        x.lo = x.hi = 0;
        if (x.E <= x.S) continue;
        if (x.x0 > 0) --x.x0;                               // (an insertion anchored at S - 1 is the region's)
        int lo = first_at(x.x0);
        while (reach[(size_t)lo] >= x.x0) {                  // a deletion among the sites before x0 reaches it: back to the last
            int d = lo - 1;                                  // deletion's anchor, which that deletion leaves in place
            while (dels[(size_t)d] == 0) --d;
            x.x0 = pos[(size_t)d];
            lo = first_at(x.x0);
        }
        x.lo = lo;
        x.hi = first_at(x.E);
    }
    // ---- the scratch: the region records, the status word, the total
    const size_t regs_bytes = align256(sizeof(HseqRegion) * (size_t)n_regions);
    GX_TRY(g->hseq_buf.reserve(regs_bytes + 256));
    HseqRegion *d_regs = reinterpret_cast<HseqRegion *>(g->hseq_buf.p);
    int *d_status = reinterpret_cast<int *>(g->hseq_buf.p + regs_bytes);
    hc_u64 *d_total = reinterpret_cast<hc_u64 *>(g->hseq_buf.p + regs_bytes + 8);
    GX_TRY(hipMemcpyAsync(d_regs, regs.data(), sizeof(HseqRegion) * (size_t)n_regions, hipMemcpyHostToDevice, st));
    GX_TRY(hipMemsetAsync(d_status, 0, 16, st));
    // gfm_graph_profile_enable: every launch between two events of its own, in launch order (measure, fill)
    auto launch = [&](auto &&enqueue) -> int {
        const bool timed = g->prof_on && g->prof_n < gfm_graph::kProfSlots;
        if (timed) GX_TRY(hipEventRecord(g->prof_ev[2 * g->prof_n], st));
        enqueue();
        GX_TRY(hipGetLastError());
        if (timed) {
            GX_TRY(hipEventRecord(g->prof_ev[2 * g->prof_n + 1], st));
            ++g->prof_n;
        }
        return GFM_OK;
    };
    struct { int status, pad; unsigned long long total; } back = {0, 0, 0ull};
    if (!(flags & GFM_SEQS_HAVE_LENGTHS)) {
        if (const int rc = launch([&] {
                hipLaunchKernelGGL(hseq_measure_kernel, dim3((unsigned)((n_seqs + kHseqThreads - 1) / kHseqThreads)), dim3(kHseqThreads), 0, st,
                                   g->dev, d_regs, (int)n_regions, (long long)n_seqs, d_seq_region, d_seq_hap, d_len, d_status, d_total);
            }))
            return rc;
        GX_TRY(hipMemcpyAsync(&back, d_status, 16, hipMemcpyDeviceToHost, st));
        GX_TRY(hipStreamSynchronize(st));                   // (regs is pageable and leaves with this call; the verdict and the total)
        if (back.status) {
            (void)g->called(st);
            return gfail(GFM_ERR_INVALID, has_haplotypes(*g) ? "a (region, haplotype) pair is out of range: regions 0 .. n_regions - 1, "
                                                               "haplotypes -1 .. n_hap - 1, at most 2^31 - 1 bases a sequence"
                                                             : "a (region, haplotype) pair is out of range: the graph carries no "
                                                               "haplotypes, only haplotype -1 (the reference) can be spelled");
        }
        if (h_total) *h_total = (int64_t)back.total;
        if (!d_bases) return g->called(st);
        if ((unsigned long long)capacity < back.total) {
            (void)g->called(st);
            return gfail(GFM_ERR_OVERFLOW, "the sequences hold " + std::to_string(back.total) + " bases, capacity is " +
                                               std::to_string(capacity));
        }
    }
    const unsigned per = kHseqThreads / 64;
    if (const int rc = launch([&] {
            hipLaunchKernelGGL(hseq_fill_kernel, dim3((unsigned)((n_seqs + per - 1) / per)), dim3(kHseqThreads), 0, st, g->dev, d_regs,
                               (int)n_regions, (long long)n_seqs, d_seq_region, d_seq_hap, d_len,
                               reinterpret_cast<const long long *>(d_off), (long long)capacity, d_bases, d_coord, (hc_u64)seed,
                               (int)key_bits, reinterpret_cast<hc_u64 *>(d_key), d_status);
        }))
        return rc;
    GX_TRY(hipMemcpyAsync(&back, d_status, 4, hipMemcpyDeviceToHost, st));
    GX_TRY(hipStreamSynchronize(st));
    if (const int rc = g->called(st)) return rc;
    if (back.status & kHseqStatusPair) return gfail(GFM_ERR_INVALID, "a (region, haplotype) pair is out of range");
    if (back.status & kHseqStatusOffsets)
        return gfail(GFM_ERR_OVERFLOW, "d_off is not the exclusive scan of the lengths inside capacity: sequences were left out");
    return GFM_OK;
}

GFM_API int gfm_sequences_verify(int64_t n_seqs, const int64_t *d_off, const uint8_t *d_bases, const int32_t *d_same_as,
                                 int32_t *d_status, void *stream)
{
    if (n_seqs < 0 || n_seqs > 0x7fffffffll || !d_status) return gfail(GFM_ERR_INVALID, "bad argument");
    if (n_seqs == 0) return GFM_OK;
    if (!d_off || !d_same_as) return gfail(GFM_ERR_INVALID, "NULL device buffer");       // (d_bases may be NULL: no base at all)
    const unsigned per = kHseqThreads / 64;
    hipLaunchKernelGGL(hseq_verify_kernel, dim3((unsigned)((n_seqs + per - 1) / per)), dim3(kHseqThreads), 0, static_cast<hipStream_t>(stream),
                       (long long)n_seqs, reinterpret_cast<const long long *>(d_off), d_bases, d_same_as, d_status);
    GX_TRY(hipGetLastError());
    return GFM_OK;
}
