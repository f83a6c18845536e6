// gfm_graph_hapclasses.hpp -- haplotype classes: for every region the haplotypes grouped by their alleles at the sites that
// can change the region's rows, the classes numbered by size (included at the end of graph_extract.hip behind
// gfm_graph_variant_affinity.hpp; it uses GraphDev, the handle's serialise / called and has_haplotypes).
//
// T(r), the sites of region [S, E) clipped to the chromosome (hc_in_region; grafimo_amd/haplotype_classes.py region_sites
// states it on the host): a substitution with S <= p < E, an insertion with S - 1 <= p < E, a deletion of d bases with
// p + 1 < E and p + d >= S; an empty region has none.  The state of haplotype h at site i: its bits in the site's n_alts used
// slots, 0 = none of the ALTs.  Two haplotypes are in one class of r when their states agree on T(r).
//
//   hc_key_kernel     (region, block of 256 haplotypes): a wavefront owns one bitset word, a lane one haplotype.  The sites of
//                     the host's index range are filtered by T(r) -- wave-uniform --, a site's three words of the wave's
//                     word index are wave-uniform loads (the word index comes from blockIdx and readfirstlane), a site whose
//                     words are all 0 for the wave is skipped, and key(h) = the sum over the sites with state != 0 of
//                     mix64(seed, site * 8 + state) mod 2^64 (a Zobrist sum: states of 0 do no work, the all-reference
//                     class has key 0), masked to key_bits.
//   hc_class_kernel   a workgroup per region: an open-addressed table of (key, first, count) in LDS -- a slot claimed by a
//                     64-bit compare-and-swap, then atomicMin(first) and atomicAdd(count) --, the occupied slots compacted,
//                     sorted by (H - count) << 32 | first with a bitonic sort, the rank scattered back to the slots, and every
//                     haplotype writes the rank of its slot.  A region that fills the table past 3/4 is appended to the spill
//                     list and redone by hc_class_spill_kernel: the same code (hc_classify) over a table of next_pow2(2 H)
//                     slots and a sort array in global memory.
//   hc_verify_kernel  classification is EXACT, the hash only speeds it up: every haplotype compares its state with its
//                     class's representative's (the smallest member, which hc_classify leaves per class) at every site of
//                     T(r); a haplotype of the class of key 0 compares with 0 and loads nothing of a representative.  A
//                     mismatch sets bit 0 of *d_status: two allele combinations shared a key, the caller takes another seed.
//   hc_record_kernel  graph-independent: count, first and per-group counts of every class from the class matrix.
//
// Memory safety under colliding (truncated) keys: the table has more slots than there can be distinct keys (LDS: the region
// spills before it passes 3/4; global: 2 H slots for at most H keys), every probe loop is bounded by the slot count, ranks are
// < the number of classes <= H, and the verify kernel reads graph memory, the class matrix and the representatives only.
namespace {

typedef unsigned long long hc_u64;
typedef __attribute__((address_space(3))) hc_u64 hc_lds_u64;
typedef __attribute__((address_space(3))) int hc_lds_int;

constexpr int kHcThreads = 256;                    // hc_key_kernel, hc_verify_kernel, hc_record_kernel: four bitset words
constexpr int kHcClassThreads = 256;
constexpr int kHcSlots = 2048;                     // slots of the LDS table: 16 + 8 + 8 KB, the sort array another 16 KB
constexpr int kHcMinSlots = 64;
constexpr int kHcMaxHap = 1 << 20;                 // the global table of a spilled region: 2^21 slots, 40 MB with its sort array
constexpr hc_u64 kHcEmpty = ~0ull;                 // a free slot (a key of this value is stored as kHcEmpty - 1)
constexpr int kHcStatusCollision = 1;
constexpr size_t kHcDefaultScratch = (size_t)256 << 20;

struct HcRegion {
    long long S, E;        // clipped to the chromosome; E <= S: empty
    int lo, hi;            // the site index range that holds T(r)
};

__device__ __forceinline__ hc_u64 hc_mix64(hc_u64 seed, hc_u64 x)
{
    hc_u64 z = x + (seed + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// site `s` is one of T(r) of the non-empty clipped region [S, E)
__device__ __forceinline__ bool hc_in_region(const SiteRec &s, long long S, long long E)
{
    const long long p = s.pos;
    if (s.del_len > 0) return p + 1 < E && p + s.del_len >= S;
    if (s.ins_len > 0) return p >= S - 1 && p < E;
    return p >= S && p < E;
}

// the wave's word index: provably wave-uniform (blockIdx and a readfirstlane), so what is loaded by it is a scalar load
__device__ __forceinline__ int hc_wave_word()
{
    return (int)blockIdx.y * (kHcThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

__global__ void __launch_bounds__(kHcThreads)
hc_key_kernel(GraphDev g, const HcRegion *__restrict__ regions, hc_u64 seed, int key_bits, hc_u64 *__restrict__ keys)
{
    const int word = hc_wave_word();
    if (word >= g.hw) return;
    const HcRegion rg = regions[blockIdx.x];
    const int lane = threadIdx.x & 63;
    const int h = word * 64 + lane;
    hc_u64 key = 0ull;
    for (int i = rg.lo; i < rg.hi; ++i) {
        const SiteRec s = g.site_rec[i];
        if (!hc_in_region(s, rg.S, rg.E)) continue;
        const hc_u64 *w = g.alt_bits + ((size_t)i * 3) * g.hw + word;
        const int na = s.n_alts;
        const hc_u64 w0 = na > 0 ? w[0] : 0ull, w1 = na > 1 ? w[g.hw] : 0ull, w2 = na > 2 ? w[2 * (size_t)g.hw] : 0ull;
        if ((w0 | w1 | w2) == 0ull) continue;
        const unsigned state = (unsigned)((w0 >> lane) & 1ull) | (unsigned)(((w1 >> lane) & 1ull) << 1) |
                               (unsigned)(((w2 >> lane) & 1ull) << 2);
        if (state) key += hc_mix64(seed, (hc_u64)i * 8ull + state);
    }
    if (key_bits < 64) key &= (1ull << key_bits) - 1ull;
    if (key == kHcEmpty) key = kHcEmpty - 1ull;
    if (h < g.n_hap) keys[(size_t)blockIdx.x * g.n_hap + h] = key;
}

// ---- the table's memory: LDS (plain accesses, ds atomics) or global (accesses that pass the vector cache, whose lines the
// atomics -- made in L2 -- do not refresh)
struct HcLds {
    typedef hc_lds_u64 *KeyPtr;
    typedef hc_lds_int *IntPtr;
    static __device__ __forceinline__ hc_u64 ld(KeyPtr p) { return *p; }
    static __device__ __forceinline__ int ld(IntPtr p) { return *p; }
    static __device__ __forceinline__ void st(KeyPtr p, hc_u64 v) { *p = v; }
    static __device__ __forceinline__ void st(IntPtr p, int v) { *p = v; }
};
struct HcGlobal {
    typedef hc_u64 *KeyPtr;
    typedef int *IntPtr;
    static __device__ __forceinline__ hc_u64 ld(KeyPtr p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ int ld(IntPtr p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void st(KeyPtr p, hc_u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void st(IntPtr p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

__device__ __forceinline__ unsigned hc_slot_of(hc_u64 key, int log_slots)
{
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> (64 - log_slots));
}

// the slot that holds `key` (it is there: every key of the region was inserted), bounded by the slot count
template <typename M>
__device__ __forceinline__ int hc_find(typename M::KeyPtr t_key, int slots, int log_slots, hc_u64 key)
{
    unsigned s = hc_slot_of(key, log_slots);
    for (int probe = 0; probe < slots; ++probe, ++s) {
        const int at = (int)(s & (unsigned)(slots - 1));
        if (M::ld(t_key + at) == key) return at;
    }
    return 0;
}

// One region by one workgroup: keys [H] -> cls [H] (the class of every haplotype), rep [n] (per class its smallest member,
// ~member for the class of key 0), *n_out = the number of classes n.  t_key / t_first / t_count: `slots` slots (a power of two);
// sorted: room for next_pow2(min(limit, H)) keys; ctl: two LDS words.  -> false: more than `limit` slots were claimed, nothing
// was written (the region spills).
template <typename M>
__device__ bool hc_classify(const hc_u64 *__restrict__ keys, int H, typename M::KeyPtr t_key, typename M::IntPtr t_first,
                            typename M::IntPtr t_count, typename M::KeyPtr sorted, int slots, int log_slots, int limit, int *ctl,
                            int *__restrict__ cls, int *__restrict__ rep, int *__restrict__ n_out)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    hc_lds_int *used = (hc_lds_int *)&ctl[0], *packed = (hc_lds_int *)&ctl[1];
    for (int s = tid; s < slots; s += nt) {
        M::st(t_key + s, kHcEmpty);
        M::st(t_first + s, 0x7fffffff);
        M::st(t_count + s, 0);
    }
    if (tid == 0) { *used = 0; *packed = 0; }
    __syncthreads();
    // ---- insert: claim by compare-and-swap, then the smallest member and the count
    for (int h = tid; h < H; h += nt) {
        const hc_u64 key = keys[h];
        unsigned s = hc_slot_of(key, log_slots);
        for (int probe = 0; probe < slots; ++probe, ++s) {
            if (__hip_atomic_load(used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > limit) break;   // (it spills)
            const int at = (int)(s & (unsigned)(slots - 1));
            hc_u64 was = kHcEmpty;
            const bool claimed = __hip_atomic_compare_exchange_strong(t_key + at, &was, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                      __HIP_MEMORY_SCOPE_AGENT);
            if (claimed) __hip_atomic_fetch_add(used, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (claimed || was == key) {
                __hip_atomic_fetch_min(t_first + at, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(t_count + at, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    __syncthreads();
    const int n = *used;
    if (n > limit) return false;
    // ---- compact the occupied slots into sort keys: more haplotypes first, then the smaller first member
    int P = 1;
    while (P < n) P <<= 1;
    for (int s = tid; s < slots; s += nt) {
        if (M::ld(t_key + s) == kHcEmpty) continue;
        const int at = __hip_atomic_fetch_add(packed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        M::st(sorted + at, ((hc_u64)(unsigned)(H - M::ld(t_count + s)) << 32) | (hc_u64)(unsigned)M::ld(t_first + s));
    }
    for (int j = n + tid; j < P; j += nt) M::st(sorted + j, kHcEmpty);
    __syncthreads();
    // ---- bitonic sort, ascending
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += nt) {
                const int other = i ^ j;
                if (other > i) {
                    const hc_u64 a = M::ld(sorted + i), b = M::ld(sorted + other);
                    if ((a > b) == ((i & k) == 0)) {
                        M::st(sorted + i, b);
                        M::st(sorted + other, a);
                    }
                }
            }
            __syncthreads();
        }
    }
    // ---- the rank back to the slots (in the count's place), the representatives out
    for (int j = tid; j < n; j += nt) {
        const int first = (int)(unsigned)(M::ld(sorted + j) & 0xffffffffull);
        const hc_u64 key = keys[first];
        const int at = hc_find<M>(t_key, slots, log_slots, key);
        M::st(t_count + at, j);
        rep[j] = key == 0ull ? ~first : first;
    }
    __syncthreads();
    for (int h = tid; h < H; h += nt) cls[h] = M::ld(t_count + hc_find<M>(t_key, slots, log_slots, keys[h]));
    if (tid == 0) *n_out = n;
    return true;
}

__global__ void __launch_bounds__(kHcClassThreads)
hc_class_kernel(const hc_u64 *__restrict__ keys, int H, int slots, int log_slots, int *__restrict__ cls, int *__restrict__ rep,
                int *__restrict__ n_classes, int *__restrict__ spill)
{
    __shared__ hc_u64 t_key[kHcSlots], sorted[kHcSlots];
    __shared__ int t_first[kHcSlots], t_count[kHcSlots], ctl[2];
    const size_t r = blockIdx.x;
    const bool done = hc_classify<HcLds>(keys + r * H, H, (hc_lds_u64 *)t_key, (hc_lds_int *)t_first, (hc_lds_int *)t_count,
                                         (hc_lds_u64 *)sorted, slots, log_slots, slots / 4 * 3, ctl, cls + r * H, rep + r * H,
                                         n_classes + r);
    if (!done && threadIdx.x == 0) spill[1 + atomicAdd(&spill[0], 1)] = (int)r;
}

// the regions spill[1 + first ...] of the chunk over tables in global memory: workgroup b owns table b and sort array b
__global__ void __launch_bounds__(kHcClassThreads)
hc_class_spill_kernel(const hc_u64 *__restrict__ keys, int H, int slots, int log_slots, int sort_len, const int *__restrict__ spill,
                      int first, hc_u64 *__restrict__ g_key, int *__restrict__ g_first, int *__restrict__ g_count,
                      hc_u64 *__restrict__ g_sorted, int *__restrict__ cls, int *__restrict__ rep, int *__restrict__ n_classes)
{
    __shared__ int ctl[2];
    const size_t r = (size_t)spill[1 + first + blockIdx.x], b = blockIdx.x;
    hc_classify<HcGlobal>(keys + r * H, H, g_key + b * slots, g_first + b * slots, g_count + b * slots, g_sorted + b * sort_len, slots,
                          log_slots, slots, ctl, cls + r * H, rep + r * H, n_classes + r);
}

__global__ void __launch_bounds__(kHcThreads)
hc_verify_kernel(GraphDev g, const HcRegion *__restrict__ regions, const int *__restrict__ cls, const int *__restrict__ rep,
                 int *__restrict__ status)
{
    const int word = hc_wave_word();
    if (word >= g.hw) return;
    const HcRegion rg = regions[blockIdx.x];
    const int lane = threadIdx.x & 63;
    const int h = word * 64 + lane, H = g.n_hap;
    const bool live = h < H;
    int mine = -1;                                              // the representative; < 0: the class of key 0, or no haplotype
    bool bad = false;
    if (live) {
        const int c = cls[(size_t)blockIdx.x * H + h];
        if ((unsigned)c >= (unsigned)H) bad = true;
        else mine = rep[(size_t)blockIdx.x * H + c];
        if (mine >= H || ~mine >= H) { bad = true; mine = -1; }
    }
    const bool some_rep = __any(mine >= 0);
    for (int i = rg.lo; i < rg.hi; ++i) {
        const SiteRec s = g.site_rec[i];
        if (!hc_in_region(s, rg.S, rg.E)) continue;
        const hc_u64 *row = g.alt_bits + ((size_t)i * 3) * g.hw;
        const int na = s.n_alts;
        const hc_u64 w0 = na > 0 ? row[word] : 0ull, w1 = na > 1 ? row[g.hw + word] : 0ull, w2 = na > 2 ? row[2 * (size_t)g.hw + word] : 0ull;
        if (!some_rep && (w0 | w1 | w2) == 0ull) continue;      // every state here is 0 and is compared with 0
        const unsigned state = (unsigned)((w0 >> lane) & 1ull) | (unsigned)(((w1 >> lane) & 1ull) << 1) |
                               (unsigned)(((w2 >> lane) & 1ull) << 2);
        unsigned other = 0u;
        if (mine >= 0) {
            const int rw = mine >> 6, rb = mine & 63;
            if (na > 0) other = (unsigned)((row[rw] >> rb) & 1ull);
            if (na > 1) other |= (unsigned)(((row[g.hw + rw] >> rb) & 1ull) << 1);
            if (na > 2) other |= (unsigned)(((row[2 * (size_t)g.hw + rw] >> rb) & 1ull) << 2);
        }
        if (live && state != other) bad = true;
    }
    if (__any(bad) && lane == 0) atomicOr(status, kHcStatusCollision);
}

// ---- the records of the classes (graph-independent)
__global__ void hc_record_init_kernel(const long long *__restrict__ class_off, int n_regions, int n_groups, int *__restrict__ count,
                                      int *__restrict__ first, int *__restrict__ group_counts)
{
    const long long total = class_off[n_regions], step = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += step) {
        count[k] = 0;
        first[k] = 0x7fffffff;
        for (int gi = 0; gi < n_groups; ++gi) group_counts[k * n_groups + gi] = 0;
    }
}

// (region, block of 256 haplotypes), a wavefront per bitset word: the lanes of one class add once -- a wave that lies in the
// region's largest class, the usual case, makes one add per output
__global__ void __launch_bounds__(kHcThreads)
hc_record_kernel(int H, int hw, const int *__restrict__ cls, const long long *__restrict__ class_off,
                 const hc_u64 *__restrict__ group_bits, int n_groups, int *__restrict__ count, int *__restrict__ first,
                 int *__restrict__ group_counts)
{
    const int word = hc_wave_word();
    if (word >= hw) return;
    const int lane = threadIdx.x & 63;
    const int h = word * 64 + lane;
    const size_t r = blockIdx.x;
    const long long base = class_off[r], n = class_off[r + 1] - base;
    int c = h < H ? cls[r * H + h] : -1;
    if (c >= n) c = -1;                                         // (not a class of this region: nothing is written for it)
    while (true) {
        const hc_u64 todo = __ballot(c >= 0);
        if (!todo) break;
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const int c0 = __builtin_amdgcn_readlane(c, leader);
        const hc_u64 same = __ballot(c == c0);
        if (lane == leader) {
            atomicAdd(&count[base + c0], __popcll(same));
            atomicMin(&first[base + c0], h);                    // (the leader is the lowest lane: the smallest of them)
            for (int gi = 0; gi < n_groups; ++gi) {
                const int v = __popcll(same & group_bits[(size_t)gi * hw + word]);
                if (v) atomicAdd(&group_counts[(base + c0) * n_groups + gi], v);
            }
        }
        if (c == c0) c = -1;
    }
}

inline int hc_log2(size_t v)
{
    int l = 0;
    while (((size_t)1 << l) < v) ++l;
    return l;
}

}  // namespace

GFM_API int gfm_graph_haplotype_classes(gfm_graph_t g, int32_t n_regions, const int64_t *h_starts, const int64_t *h_stops,
                                        uint64_t seed, int32_t key_bits, int32_t table_slots, int32_t *d_class,
                                        int32_t *d_n_classes, int32_t *d_status, int64_t scratch_bytes, void *stream)
{
    if (!g) return gfail(GFM_ERR_INVALID, "graph is NULL");
    if (!has_haplotypes(*g)) return fail_no_haplotypes("gfm_graph_haplotype_classes");
    if (n_regions < 0 || (n_regions && (!h_starts || !h_stops || !d_class || !d_n_classes)) || !d_status || scratch_bytes < 0)
        return gfail(GFM_ERR_INVALID, "bad argument");
    if (key_bits < 1 || key_bits > 64) return gfail(GFM_ERR_INVALID, "key_bits outside [1, 64]");
    if (table_slots != 0 && (table_slots < kHcMinSlots || table_slots > kHcSlots || (table_slots & (table_slots - 1))))
        return gfail(GFM_ERR_INVALID, "table_slots: 0 or a power of two in [" + std::to_string(kHcMinSlots) + ", " +
                                          std::to_string(kHcSlots) + "]");
    const int H = g->dev.n_hap, hw = g->dev.hw;
    if (H > kHcMaxHap) return gfail(GFM_ERR_INVALID, "more than " + std::to_string(kHcMaxHap) + " haplotypes");
    for (int r = 0; r < n_regions; ++r)
        if (h_stops[r] < h_starts[r]) return gfail(GFM_ERR_INVALID, "a region ends before it starts");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_regions == 0) return GFM_OK;
    if (const int rc = g->serialise(st)) return rc;
    // ---- the regions: clipped, with the index range of their sites -- from the longest deletion before S up to pos < E
    std::vector<HcRegion> regs((size_t)n_regions);
    const std::vector<int> &pos = g->h_pos;
    for (int r = 0; r < n_regions; ++r) {
        HcRegion &x = regs[(size_t)r];
        x.S = std::max<long long>(h_starts[r], 0);
        x.E = std::min<long long>(h_stops[r], g->dev.ref_len);
        x.lo = x.hi = 0;
        if (x.E <= x.S) continue;
        const long long from = x.S - 1 - g->max_del_len;
        x.lo = (int)(std::lower_bound(pos.begin(), pos.end(), from, [](int p, long long v) { return (long long)p < v; }) - pos.begin());
        x.hi = (int)(std::lower_bound(pos.begin(), pos.end(), x.E, [](int p, long long v) { return (long long)p < v; }) - pos.begin());
    }
    // ---- the scratch: the region records, then per region of a chunk its keys and representatives and a spill-list word,
    // then what is left (at least one set) for the global tables of spilled regions
    const int slots = table_slots ? table_slots : kHcSlots, log_slots = hc_log2((size_t)slots);
    const int g_log = hc_log2((size_t)2 * H), g_slots = 1 << g_log, sort_len = 1 << hc_log2((size_t)H);
    const size_t per_region = align256((size_t)H * 8) + align256((size_t)H * 4) + 4;
    const size_t per_spill = align256((size_t)g_slots * 8) + 2 * align256((size_t)g_slots * 4) + align256((size_t)sort_len * 8);
    const size_t budget = scratch_bytes ? (size_t)scratch_bytes : kHcDefaultScratch;
    size_t chunk = budget > per_spill ? (budget - per_spill) / per_region : 0;
    chunk = std::max<size_t>(1, std::min<size_t>(chunk, (size_t)n_regions));
    const size_t chunk_bytes = chunk * (align256((size_t)H * 8) + align256((size_t)H * 4)) + align256((chunk + 1) * 4);
    size_t n_tables = budget > chunk_bytes ? (budget - chunk_bytes) / per_spill : 0;
    n_tables = std::max<size_t>(1, std::min<size_t>(n_tables, chunk));
    const size_t regs_bytes = align256(sizeof(HcRegion) * (size_t)n_regions);
    GX_TRY(g->hc_buf.reserve(regs_bytes + chunk_bytes + n_tables * per_spill));
    unsigned char *at = g->hc_buf.p;
    auto take = [&](size_t bytes) { unsigned char *p = at; at += align256(bytes); return p; };
    HcRegion *d_regs = reinterpret_cast<HcRegion *>(take(regs_bytes));
    hc_u64 *d_keys = reinterpret_cast<hc_u64 *>(take(chunk * align256((size_t)H * 8)));
    int *d_rep = reinterpret_cast<int *>(take(chunk * align256((size_t)H * 4)));
    int *d_spill = reinterpret_cast<int *>(take((chunk + 1) * 4));
    hc_u64 *d_tkey = reinterpret_cast<hc_u64 *>(take(n_tables * (size_t)g_slots * 8));
    int *d_tfirst = reinterpret_cast<int *>(take(n_tables * (size_t)g_slots * 4));
    int *d_tcount = reinterpret_cast<int *>(take(n_tables * (size_t)g_slots * 4));
    hc_u64 *d_sorted = reinterpret_cast<hc_u64 *>(take(n_tables * (size_t)sort_len * 8));
    // (keys and representatives are [chunk][H] without padding between the rows: the chunk's total was rounded up per row)
    GX_TRY(hipMemcpyAsync(d_regs, regs.data(), sizeof(HcRegion) * (size_t)n_regions, hipMemcpyHostToDevice, st));
    GX_TRY(hipStreamSynchronize(st));                       // (regs is pageable and leaves with this call)
    const unsigned yblocks = (unsigned)((hw + kHcThreads / 64 - 1) / (kHcThreads / 64));
    // gfm_graph_profile_enable: every launch between two events of its own, in launch order (per chunk: keys, classes, one per
    // batch of spilled regions, verification)
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
    for (size_t r0 = 0; r0 < (size_t)n_regions; r0 += chunk) {
        const unsigned n = (unsigned)std::min<size_t>(chunk, (size_t)n_regions - r0);
        int *cls = d_class + r0 * (size_t)H;
        GX_TRY(hipMemsetAsync(d_spill, 0, 4, st));
        if (const int rc = launch([&] {
                hipLaunchKernelGGL(hc_key_kernel, dim3(n, yblocks), dim3(kHcThreads), 0, st, g->dev, d_regs + r0, (hc_u64)seed,
                                   (int)key_bits, d_keys);
            }))
            return rc;
        if (const int rc = launch([&] {
                hipLaunchKernelGGL(hc_class_kernel, dim3(n), dim3(kHcClassThreads), 0, st, d_keys, H, slots, log_slots, cls, d_rep,
                                   d_n_classes + r0, d_spill);
            }))
            return rc;
        int n_spill = 0;
        GX_TRY(hipMemcpyAsync(&n_spill, d_spill, 4, hipMemcpyDeviceToHost, st));
        GX_TRY(hipStreamSynchronize(st));                   // (the spill list decides the next launches)
        if (n_spill < 0 || (unsigned)n_spill > n) return gfail(GFM_ERR_HIP, "gfm_graph_haplotype_classes: bad spill count");
        for (int first = 0; first < n_spill; first += (int)n_tables) {
            const unsigned nb = (unsigned)std::min<size_t>(n_tables, (size_t)(n_spill - first));
            if (const int rc = launch([&] {
                    hipLaunchKernelGGL(hc_class_spill_kernel, dim3(nb), dim3(kHcClassThreads), 0, st, d_keys, H, g_slots, g_log,
                                       sort_len, d_spill, first, d_tkey, d_tfirst, d_tcount, d_sorted, cls, d_rep, d_n_classes + r0);
                }))
                return rc;
        }
        if (const int rc = launch([&] {
                hipLaunchKernelGGL(hc_verify_kernel, dim3(n, yblocks), dim3(kHcThreads), 0, st, g->dev, d_regs + r0, cls, d_rep,
                                   d_status);
            }))
            return rc;
    }
    return g->called(st);
}

GFM_API int gfm_graph_haplotype_class_records(int32_t n_regions, int32_t n_hap, const int32_t *d_class, const int64_t *d_class_off,
                                              const uint64_t *d_group_bits, int32_t n_groups, int32_t *d_count, int32_t *d_first,
                                              int32_t *d_group_counts, void *stream)
{
    if (n_regions < 0 || n_hap < 1 || n_groups < 0 || n_groups > 64) return gfail(GFM_ERR_INVALID, "bad argument");
    if (n_regions == 0) return GFM_OK;
    if (!d_class || !d_class_off || !d_count || !d_first || (n_groups > 0 && (!d_group_bits || !d_group_counts)))
        return gfail(GFM_ERR_INVALID, "NULL device buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int hw = (n_hap + 63) / 64;
    hipLaunchKernelGGL(hc_record_init_kernel, dim3(1024), dim3(256), 0, st, reinterpret_cast<const long long *>(d_class_off),
                       (int)n_regions, (int)n_groups, d_count, d_first, d_group_counts);
    GX_TRY(hipGetLastError());
    const unsigned yblocks = (unsigned)((hw + kHcThreads / 64 - 1) / (kHcThreads / 64));
    hipLaunchKernelGGL(hc_record_kernel, dim3((unsigned)n_regions, yblocks), dim3(kHcThreads), 0, st, (int)n_hap, hw, d_class,
                       reinterpret_cast<const long long *>(d_class_off), reinterpret_cast<const hc_u64 *>(d_group_bits),
                       (int)n_groups, d_count, d_first, d_group_counts);
    GX_TRY(hipGetLastError());
    return GFM_OK;
}
