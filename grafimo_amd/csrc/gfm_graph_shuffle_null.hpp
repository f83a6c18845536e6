// gfm_graph_shuffle_null.hpp -- shuffle null: K composition-preserving shuffles of every sequence, each scored like the
// sequence itself, and where the sequence's own best score and total affinity fall among them (included at the end of
// graph_extract.hip behind gfm_graph_indel_scan.hpp; it uses base_code, view_motif_set, SeqMotifs, kSeqMotifs, GX_TRY, gfail,
// align256 and gfm_graph_table_score.hpp's window_sum, strand_scores and walk_value).  The first table whose work is K times
// its input: a sequence of n bases costs K (n - 1) swaps once and K (n - W + 1) windows a motif.
//
// THE RULE (include/grafimo_hip.h states it for the library; tests/shuffle_null_bruteforce.py on the host).  All arithmetic on
// 64-bit words is modulo 2^64.  G = 0x9E3779B97F4A7C15;
//   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
// For a sequence x of n bases with the caller's key k, a seed, and the replicates r = 0 .. K - 1:
//   s0 = mix(mix(seed + k G) + r);  y = x, the bytes as they are;
//   for i = n - 1 down to 1:  u = mix(s0 + i G);  j = ((u >> 32) (i + 1)) >> 32;  swap y[i] and y[j].
//   The permutation depends on (seed, k, r, n) only.
// For a motif of width W every window start 0 .. n - W of a sequence is scored once per strand, + only under
// GFM_GRAPH_FORWARD_ONLY; a window that holds a base that is not A/C/G/T scores min_val on both strands; case is folded, as
// base_code does.  best = the largest score over windows and strands, -1 when n < W; sum = the exact uint64 sum of w[score]
// over windows and strands, 0 when there is none.  obs_best, obs_sum: those of x itself.  ge_best = #{r: best_r >= obs_best},
// ge_sum = #{r: sum_r >= obs_sum} (ties count; n < W gives K).  rep_hits[r] = the sum over the sequences v of
// seq_weight[v] [best_{v, r} >= cut].  rep_best, rep_sum [v][r]: the replicates' own pairs.
// Order 2 (gfm_sequence_shuffle_null_order) makes y another way -- every replicate keeps x's doublets -- and scores it the
// same way: ORDER 2 below replaces fill and shuffle, nothing else.
//
// Work decomposition.  The unit is a (sequence, 64 replicates) pair; a workgroup is ONE wavefront, a lane per replicate, and
// strides over the units of its launch.  The base codes of the 64 shuffles (times 4: column_window_sum says why) are a
// [position][lane] byte image: a row is 64 consecutive bytes, so a window read (all lanes at one position) touches 16
// consecutive banks once, and a swap's scatter (one position per lane) is a byte store into the lane's own column.  Per unit:
//   fill     the wave reads 64 bases at a time and writes each code as a row of 16 equal words;
//   shuffle  a lane per replicate walks i = n - 1 .. 1 in its own column -- ONCE for the up to kSeqMotifs motifs of the launch;
//   then, per motif of the launch (the packed table, W x 8 words, is staged in LDS in turn):
//   observe  the wave scores x itself, a lane per window start, read from the caller's bases; the pair is reduced over the
//            wave with shuffles (the unit of the replicates 0 .. 63 stores it);
//   score    each lane slides the window over its column, two windows and eight columns a turn (column_window_sum); w[score]
//            comes through the cache;
//   count    two ballots and popcounts, one integer add a wave to ge_best and ge_sum; rep_hits by a vector atomic a lane (the
//            lanes add to different replicates); the dense arrays by plain stores, 64 consecutive replicates a wave.
// No floating point; lanes with r >= K shuffle nothing, vote for nothing and store nothing.  The integer adds make every
// result exact in whatever order the units run.
// Where the image lives.  Sequences of up to GFM_NULL_LDS_BASES bases: dynamic LDS, 64 bytes a base of the LONGEST sequence of
// the launch -- the entry sorts the sequences into length classes (kNullClassBounds) and launches per class, so that a 300-base
// peak reserves at most 320 x 64 + 2 048 = 22 528 bytes (7 workgroups a CU) and not what a 960-base one needs (63 488: 2 a CU).  Longer
// sequences: the same kernel body (kLds = false) on a scratch in device memory, 64 n bytes a workgroup (hipMallocAsync, as the
// unit table); the workgroups of that launch are as many as kNullScratchBytes holds.  The unit table is built on the host and
// checked on the device before anything is read or written through it.
namespace {

constexpr int kNullLanes = 64;
constexpr int kNullBadSeq = 1;
constexpr int kNullMaxBlocks = 1 << 16;
constexpr int kNullLdsBases = GFM_NULL_LDS_BASES;
constexpr size_t kNullScratchBytes = (size_t)1 << 28;             // what the scratch path's images hold together
// the longest sequence of each LDS length class (a launch reserves for the longest it actually holds)
constexpr int kNullClassBounds[] = {64, 128, 192, 256, 320, 384, 448, 512, 640, 768, kNullLdsBases};
constexpr int kNullClasses = (int)(sizeof kNullClassBounds / sizeof kNullClassBounds[0]) + 1;          // the last: scratch
static_assert((size_t)kNullLdsBases * kNullLanes + sizeof(unsigned) * GFM_MAX_WIDTH * 8 <= 64 * 1024,
              "a workgroup's image and table fit the 64 KiB a launch may ask for without opting in");
constexpr unsigned long long kNullG = 0x9E3779B97F4A7C15ull;

struct NullSeq {
    long long begin;              // the sequence's first base in d_bases
    int len, seq;                 // its length; its row in the results
};

struct NullOut {
    int *obs_best[kSeqMotifs];
    unsigned long long *obs_sum[kSeqMotifs];
    unsigned *ge_best[kSeqMotifs], *ge_sum[kSeqMotifs];
    unsigned long long *rep_hits[kSeqMotifs];                     // (these three may be NULL: not computed)
    int *rep_best[kSeqMotifs];
    unsigned long long *rep_sum[kSeqMotifs];
    int cut[kSeqMotifs];
};

__device__ __forceinline__ unsigned long long null_mix(unsigned long long z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// window_sum over a lane's column, for the image's bytes: 4 x the base code, the byte offset of the code's word in a table
// row (c[j * 64] belongs to the window's column j).  Eight columns a turn: the eight byte reads are issued before the eight
// table reads that depend on them.  A workgroup is one wavefront and a CU holds few of them (the image), so nothing else hides
// the two LDS latencies a column costs.  A column costs three vector instructions beside its two reads: the table address,
// the sum, and the OR that says whether any code was none (bit 4).  The bytes are masked to 0 .. 28, which is what bounds the
// table index.
__device__ __forceinline__ WindowSum column_window_sum(const unsigned *ftab, int W, const unsigned char *c)
{
    const unsigned char *table = reinterpret_cast<const unsigned char *>(ftab);
    unsigned sum = 0u, any = 0u;
    int j = 0;
    for (; j + 8 <= W; j += 8) {
        unsigned at[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) at[k] = (unsigned)c[(size_t)(j + k) * kNullLanes] & 28u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            sum += *reinterpret_cast<const unsigned *>(table + (j + k) * 32 + at[k]);
            any |= at[k];
        }
    }
    if (j < W) {                                                  // the last W % 8 columns the same way: the rest re-read column W - 1
        unsigned at[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) at[k] = (unsigned)c[(size_t)min(j + k, W - 1) * kNullLanes] & 28u;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const unsigned word = *reinterpret_cast<const unsigned *>(table + min(j + k, W - 1) * 32 + at[k]);
            sum += j + k < W ? word : 0u;
            any |= at[k];                                         // (column W - 1 again: it is the window's own)
        }
    }
    return WindowSum{sum, any >> 4};
}

// ---- ORDER 2: doublet-preserving replicates (THE RULE OF ORDER 2: include/grafimo_hip.h; tests/doublet_null_bruteforce.py on
// the host).  The rule's alphabet is A, C, G, T = 0 .. 3 and 4 for anything else; base_code() gives A 0, C 1, T 2, G 3, so the
// two differ by c ^ (c >> 1) below 4, an involution.  A replicate is a random Euler path of x's doublet graph (Altschul and
// Erickson): the successors c[i + 1] sorted stably by c[i] are the edge lists E of the five vertices; a random arborescence
// towards the last code (Wilson) names every other vertex's LAST exit, the rest of each list is shuffled, and the walk from
// c[0] that takes every list in order spells y.
// Where E lives: in the image itself.  column_window_sum reads a byte through & 28, so bits 2 .. 4 hold 4 x the replicate's
// base_code as in order 1 and bits 5 .. 7 the E code of the same row: the image, the length classes, GFM_NULL_LDS_BASES and
// the scratch path are order 1's.  E has n - 1 entries; row n - 1 holds E bits 0.
//   fill     (the wave) cnt and b by ballots over 64 bases a turn, wave-uniform; then every position's stable rank in its bucket
//            by the same ballots, and its successor written to row b[a] + rank as 16 equal words.  Row n - 1 takes c[n - 1].
//   per lane (r < K, n >= 2; the lane's own column, no barrier inside) the arborescence, the swap and the per-bucket
//            Fisher-Yates, the walk.  last[5] and ptr[5] are indexed by a run-time symbol: select chains over named fields (Five).
// cnt, b, root and the Fisher-Yates trip counts are the same for all lanes; only the walk of the arborescence diverges, and it
// is bounded by construction: at most walk_cap n steps a lane, then x's own last exits.
constexpr int kNullSymbols = 5;

__device__ __forceinline__ unsigned rule_code(unsigned char ch)
{
    const unsigned c = base_code(ch);
    return c < 4u ? c ^ (c >> 1) : 4u;
}
__device__ __forceinline__ unsigned image_code(unsigned a) { return (a ^ (a >> 1)) << 2; }       // (4: 24, no base)

// Five integers, one a symbol, as named fields: as an array under unrolled loops they stayed in memory (the compiler made
// indexed loads from scratch memory of the select chains); fields are registers before anything can be folded.
struct Five { int a0, a1, a2, a3, a4; };
template <int A>
__device__ __forceinline__ int &at5(Five &f)
{
    static_assert(A >= 0 && A < kNullSymbols, "a symbol");
    if constexpr (A == 0) return f.a0;
    else if constexpr (A == 1) return f.a1;
    else if constexpr (A == 2) return f.a2;
    else if constexpr (A == 3) return f.a3;
    else return f.a4;
}
template <int A>
__device__ __forceinline__ int at5(const Five &f) { return at5<A>(const_cast<Five &>(f)); }
__device__ __forceinline__ int pick5(const Five &f, unsigned a)
{
    return a == 1u ? f.a1 : a == 2u ? f.a2 : a == 3u ? f.a3 : a == 4u ? f.a4 : f.a0;
}
__device__ __forceinline__ void put5(Five &f, unsigned a, int x)
{
    f.a0 = a == 0u ? x : f.a0;
    f.a1 = a == 1u ? x : f.a1;
    f.a2 = a == 2u ? x : f.a2;
    f.a3 = a == 3u ? x : f.a3;
    f.a4 = a == 4u ? x : f.a4;
}
// f(integral_constant a) for a = 0 .. 4 in order
template <class F>
__device__ __forceinline__ void each_symbol(F f)
{
    f(std::integral_constant<int, 0>{});
    f(std::integral_constant<int, 1>{});
    f(std::integral_constant<int, 2>{});
    f(std::integral_constant<int, 3>{});
    f(std::integral_constant<int, 4>{});
}

// fill of order 2 (the whole wave; n >= 1): -> cnt, b.  Every row 0 .. n - 1 of the image is written once.
__device__ __forceinline__ void doublet_fill(unsigned char *y, const uint8_t *__restrict__ x, int n, int lane, Five &cnt, Five &b)
{
    cnt = Five{0, 0, 0, 0, 0};
    for (int p0 = 0; p0 < n - 1; p0 += kNullLanes) {
        const int p = p0 + lane;
        const unsigned c = p < n - 1 ? rule_code(x[p]) : (unsigned)kNullSymbols;
        each_symbol([&](auto A) {
            constexpr int a = decltype(A)::value;
            at5<a>(cnt) += __popcll(__builtin_amdgcn_ballot_w64(c == (unsigned)a));
        });
    }
    b.a0 = 0;
    b.a1 = cnt.a0;
    b.a2 = b.a1 + cnt.a1;
    b.a3 = b.a2 + cnt.a2;
    b.a4 = b.a3 + cnt.a3;
    Five run = b;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int p0 = 0; p0 < n; p0 += kNullLanes) {
        const int p = p0 + lane, rows = min(kNullLanes, n - p0);
        const unsigned c = p < n - 1 ? rule_code(x[p]) : (unsigned)kNullSymbols;
        // the byte of the row this position fills: its successor as an E code; the last position its own code, E bits 0
        const unsigned byte = p < n - 1 ? rule_code(x[p + 1]) << 5 : (p == n - 1 ? image_code(rule_code(x[p])) : 0u);
        int e = n - 1;                                            // (the last position; the lanes beyond it store nothing)
        each_symbol([&](auto A) {
            constexpr int a = decltype(A)::value;
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(c == (unsigned)a);
            if (c == (unsigned)a) e = at5<a>(run) + __popcll(mask & below);           // < b[a] + cnt[a] <= n - 1
            at5<a>(run) += __popcll(mask);
        });
        for (int q = 0; q < rows; q += 4) {
            const int src = q + (lane >> 4);
            const int eq = __shfl(e, src);
            const unsigned bq = (unsigned)__shfl((int)byte, src);
            if (src < rows) reinterpret_cast<unsigned *>(y)[(size_t)eq * 16 + (lane & 15)] = bq * 0x01010101u;
        }
    }
}

// replicate of order 2 in the lane's own column (n >= 2): arborescence, per-bucket shuffle, walk
__device__ __forceinline__ void doublet_replicate(unsigned char *col, const uint8_t *__restrict__ x, int n, const Five &cnt,
                                                  const Five &b, unsigned long long s0, int walk_cap)
{
    // an E entry, masked before it indexes b, cnt or ptr; the row clamped to the column
    auto edge = [&](int e) { return min((unsigned)col[(size_t)min(max(e, 0), n - 1) * kNullLanes] >> 5, 4u); };
    auto draw = [&](unsigned long long t, int m) {
        return (int)(((null_mix(s0 + t * kNullG) >> 32) * (unsigned long long)(unsigned)m) >> 32);          // < m, or 0
    };
    auto swap_rows = [&](int p, int q) {
        const size_t ip = (size_t)p * kNullLanes, iq = (size_t)q * kNullLanes;
        const unsigned char a = col[ip], c = col[iq];
        col[ip] = c;
        col[iq] = a;
    };
    const unsigned first = rule_code(x[0]), root = rule_code(x[n - 1]);
    // ---- the arborescence towards root (Wilson): last[a], the E row of a's last exit
    const Five own{b.a0 + cnt.a0 - 1, b.a1 + cnt.a1 - 1, b.a2 + cnt.a2 - 1, b.a3 + cnt.a3 - 1, b.a4 + cnt.a4 - 1};  // x's last exits
    Five last = own;
    unsigned tree = 1u << root;
    unsigned long long t = 0ull;
    const unsigned long long cap = (unsigned long long)walk_cap * (unsigned long long)n;
    bool capped = false;
    each_symbol([&](auto A) {
        constexpr int u = decltype(A)::value;
        if (capped || at5<u>(cnt) == 0 || ((tree >> u) & 1u)) return;
        unsigned cur = (unsigned)u;
        while (!((tree >> cur) & 1u)) {
            if (t == cap) {
                capped = true;
                return;
            }
            const int e = pick5(b, cur) + draw((unsigned long long)n + t, pick5(cnt, cur));
            ++t;
            put5(last, cur, e);
            cur = edge(e);
        }
        cur = (unsigned)u;
        for (int k = 0; k < kNullSymbols && !((tree >> cur) & 1u); ++k) {
            tree |= 1u << cur;
            cur = edge(pick5(last, cur));
        }
    });
    if (capped) last = own;
    // ---- per bucket: the last exit to the bucket's end, the rest shuffled (the trip counts are the wave's)
    each_symbol([&](auto A) {
        constexpr int a = decltype(A)::value;
        int m = at5<a>(cnt);
        if (m == 0) return;
        const int from = at5<a>(b), top = at5<a>(own);
        if ((unsigned)a != root) {
            swap_rows(min(max(at5<a>(last), from), top), top);
            --m;
        }
        for (int i = m - 1; i >= 1; --i) swap_rows(from + i, from + draw((unsigned long long)(from + i), i + 1));
    });
    // ---- the Euler walk: y into bits 2 .. 4, the E bits stay
    Five ptr = b;
    unsigned prev = first;
    col[0] = (unsigned char)((col[0] & 0xE0u) | image_code(first));
    for (int i = 1; i < n; ++i) {
        const unsigned next = edge(min(pick5(ptr, prev), n - 2));
        put5(ptr, prev, pick5(ptr, prev) + 1);
        const size_t at = (size_t)i * kNullLanes;
        col[at] = (unsigned char)((col[at] & 0xE0u) | image_code(next));
        prev = next;
    }
}

// kOrder 1: fill and shuffle as THE RULE says; kOrder 2: doublet_fill and doublet_replicate.  Observe, score and count are shared.
template <bool kLds, int kOrder>
__global__ void __launch_bounds__(kNullLanes)
shuffle_null_kernel(const NullSeq *__restrict__ seqs, long long n_listed, int n_seqs, const uint8_t *__restrict__ bases,
                    long long n_bases, const unsigned long long *__restrict__ seq_keys, const unsigned *__restrict__ seq_weight,
                    int K, unsigned long long seed, SeqMotifs mt, NullOut out, int n_motifs, int W, int forward_only, int rows,
                    unsigned char *__restrict__ scratch, int *__restrict__ status, int walk_cap)
{
    extern __shared__ unsigned char image_s[];                    // (kLds) [rows][64]: the code of position p in replicate lane
    __shared__ unsigned ftab_s[GFM_MAX_WIDTH * 8];
    const int lane = threadIdx.x;
    unsigned char *y;
    if constexpr (kLds) y = image_s;
    else y = scratch + (size_t)blockIdx.x * (size_t)rows * kNullLanes;
    const int n_blocks = (K + kNullLanes - 1) / kNullLanes;
    const long long units = n_listed * n_blocks;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const NullSeq sq = seqs[u / n_blocks];
        const int block = (int)(u % n_blocks), r = block * kNullLanes + lane;
        // ---- the sequence, checked: everything read and written below lies inside it, its row and the image (uniform)
        if (sq.begin < 0 || sq.len < 0 || sq.len > rows || sq.begin > n_bases - sq.len || sq.seq < 0 || sq.seq >= n_seqs) {
            if (lane == 0) atomicOr(status, kNullBadSeq);
            continue;
        }
        const uint8_t *__restrict__ x = bases + sq.begin;
        const int n = sq.len, v = sq.seq;
        const bool active = r < K;
        __syncthreads();                                          // (the unit before has read its image)
        if constexpr (kOrder == 1) {
            // ---- fill: 64 bases a turn, four rows of 16 equal words a step
            for (int p0 = 0; p0 < n; p0 += kNullLanes) {
                const int p = p0 + lane, cnt = min(kNullLanes, n - p0);
                const unsigned c = (p < n ? base_code(x[p]) : 4u) * 4u;                   // (what column_window_sum reads)
                for (int q = 0; q < cnt; q += 4) {
                    const int row = q + (lane >> 4);
                    const unsigned cq = (unsigned)__shfl((int)c, row);
                    if (row < cnt) reinterpret_cast<unsigned *>(y)[(size_t)(p0 + row) * 16 + (lane & 15)] = cq * 0x01010101u;
                }
            }
            __syncthreads();
            // ---- shuffle: the lane's own column, once for every motif of the launch
            if (active) {
                const unsigned long long s0 = null_mix(null_mix(seed + seq_keys[v] * kNullG) + (unsigned long long)r);
                unsigned char *col = y + lane;
                for (int i = n - 1; i >= 1; --i) {
                    const unsigned long long uu = null_mix(s0 + (unsigned long long)i * kNullG);
                    const size_t j = (size_t)(((uu >> 32) * (unsigned long long)(i + 1)) >> 32);          // j <= i
                    const unsigned char a = col[(size_t)i * kNullLanes], b = col[j * kNullLanes];
                    col[(size_t)i * kNullLanes] = b;
                    col[j * kNullLanes] = a;
                }
            }
        } else {
            // ---- fill and, per lane, the replicate of order 2
            Five cnt, b;
            if (n >= 1) doublet_fill(y, x, n, lane, cnt, b);
            __syncthreads();
            if (active && n >= 2) {
                const unsigned long long s0 = null_mix(null_mix(seed + seq_keys[v] * kNullG) + (unsigned long long)r + (1ull << 63));
                doublet_replicate(y + lane, x, n, cnt, b, s0, walk_cap);
            }
        }
        for (int m = 0; m < n_motifs; ++m) {
            __syncthreads();                                      // (the motif before is done with the table)
            for (int i = lane; i < W * 8; i += kNullLanes) ftab_s[i] = mt.ftab[m][i];
            __syncthreads();
            const unsigned long long *__restrict__ wtab = mt.wtab[m];
            const int min_val = mt.min_val[m];
            // ---- observe: x itself, a lane per window start
            int obs_best = -1;
            unsigned long long obs_sum = 0ull;
            for (int s = lane; s <= n - W; s += kNullLanes) {
                const WindowSum w = window_sum(ftab_s, W, [&](int j) { return base_code(x[s + j]); });
                const StrandScores sc = strand_scores(w, min_val);
                obs_best = max(obs_best, forward_only ? sc.plus : max(sc.plus, sc.minus));
                obs_sum += walk_value(wtab, w, min_val, forward_only);
            }
            for (int off = kNullLanes / 2; off >= 1; off >>= 1) {
                obs_best = max(obs_best, __shfl_xor(obs_best, off));
                obs_sum += __shfl_xor(obs_sum, off);
            }
            // ---- score: the lane's shuffle
            int best = -1;
            unsigned long long sum = 0ull;
            if (active) {
                const unsigned char *col = y + lane;
                const int last = n - W;                           // two windows a turn: their reads do not depend on each other
                for (int s = 0; s <= last; s += 2) {
                    const bool two = s < last;                    // (an odd window out re-reads itself and is not counted)
                    const WindowSum w0 = column_window_sum(ftab_s, W, col + (size_t)s * kNullLanes);
                    const WindowSum w1 = column_window_sum(ftab_s, W, col + (size_t)(two ? s + 1 : s) * kNullLanes);
                    const StrandScores s0 = strand_scores(w0, min_val), s1 = strand_scores(w1, min_val);
                    const unsigned long long v0 = walk_value(wtab, w0, min_val, forward_only);
                    const unsigned long long v1 = walk_value(wtab, w1, min_val, forward_only);
                    best = max(best, forward_only ? s0.plus : max(s0.plus, s0.minus));
                    if (two) best = max(best, forward_only ? s1.plus : max(s1.plus, s1.minus));
                    sum += two ? v0 + v1 : v0;
                }
            }
            // ---- count
            const unsigned n_best = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(active && best >= obs_best));
            const unsigned n_sum = (unsigned)__popcll(__builtin_amdgcn_ballot_w64(active && sum >= obs_sum));
            if (lane == 0) {
                atomicAdd(&out.ge_best[m][v], n_best);
                atomicAdd(&out.ge_sum[m][v], n_sum);
                if (block == 0) {
                    out.obs_best[m][v] = obs_best;
                    out.obs_sum[m][v] = obs_sum;
                }
            }
            if (active) {
                if (out.rep_hits[m] && best >= out.cut[m]) {
                    const unsigned wv = seq_weight ? seq_weight[v] : 1u;
                    if (wv) atomicAdd(&out.rep_hits[m][r], (unsigned long long)wv);
                }
                if (out.rep_best[m]) out.rep_best[m][(size_t)v * (size_t)K + (size_t)r] = best;
                if (out.rep_sum[m]) out.rep_sum[m][(size_t)v * (size_t)K + (size_t)r] = sum;
            }
        }
    }
}

}  // namespace

namespace {

// what both entries do: `who` names the entry in its messages; order 1 or 2, walk_cap in [0, 1024] (checked by the caller)
int sequence_shuffle_null(const char *who_, const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                          uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                          const uint64_t *d_seq_keys, const uint32_t *d_seq_weight, int32_t n_replicates, uint64_t seed,
                          int order, int walk_cap, const int32_t *cuts, uint32_t flags, int32_t *const *d_obs_best,
                          uint64_t *const *d_obs_sum, uint32_t *const *d_ge_best, uint32_t *const *d_ge_sum,
                          uint64_t *const *d_rep_hits, int32_t *const *d_rep_best, uint64_t *const *d_rep_sum, int32_t *d_status,
                          void *stream)
{
    const std::string who = std::string(who_) + ": ";
    if (n_motifs < 1 || n_seqs < 0) return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    if (n_replicates < 1 || n_replicates > (1 << 20))
        return gfail(GFM_ERR_INVALID, who + "n_replicates " + std::to_string(n_replicates) + " outside [1, 2^20]");
    if (n_seqs == 0) return GFM_OK;
    if (!seq_offsets) return gfail(GFM_ERR_INVALID, who + "NULL argument");
    // ---- the sequences by length class (an empty sequence has results too: it is listed like any other)
    if (seq_offsets[0] < 0) return gfail(GFM_ERR_INVALID, who + "seq_offsets descends below 0");
    std::vector<NullSeq> by_class[kNullClasses];
    int longest[kNullClasses] = {};
    long long longest_of_all = 0;
    for (int v = 0; v < n_seqs; ++v) {
        const long long a = seq_offsets[v], b = seq_offsets[v + 1];
        if (b < a) return gfail(GFM_ERR_INVALID, who + "seq_offsets descends at sequence " + std::to_string(v));
        if (b - a > 0x7fffffffll)
            return gfail(GFM_ERR_INVALID, who + "sequence " + std::to_string(v) + " holds 2^31 bases or more");
        int c = 0;
        while (c < kNullClasses - 1 && b - a > kNullClassBounds[c]) ++c;
        by_class[c].push_back(NullSeq{a, (int)(b - a), v});
        longest[c] = std::max(longest[c], (int)(b - a));
        longest_of_all = std::max(longest_of_all, b - a);
    }
    const long long n_bases = seq_offsets[n_seqs];
    if (!motifs || !d_weights || !cuts || !d_obs_best || !d_obs_sum || !d_ge_best || !d_ge_sum || !d_rep_hits || !d_rep_best ||
        !d_rep_sum || !d_status || !d_seq_keys || (!d_bases && n_bases > 0))
        return gfail(GFM_ERR_INVALID, who + "NULL argument");
    for (int m = 0; m < n_motifs; ++m)
        if (!motifs[m] || !d_weights[m] || !d_obs_best[m] || !d_obs_sum[m] || !d_ge_best[m] || !d_ge_sum[m])
            return gfail(GFM_ERR_INVALID, "NULL motif / device buffer");
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::PackedTable, ms)) return rc;
    const int W = ms.W;
    for (int m = 0; m < n_motifs; ++m) {
        const int L = gfm_motif_table_len(motifs[m]);
        if (cuts[m] < 0 || cuts[m] > L)
            return gfail(GFM_ERR_INVALID, who + "the cut " + std::to_string(cuts[m]) + " of motif " +
                                          std::to_string(m) + " lies outside [0, " + std::to_string(L) + "]");
    }
    // the capacity of a sum: the longest sequence's windows, each once per strand
    const unsigned long long most_windows = longest_of_all >= W ? (unsigned long long)(longest_of_all - W + 1) : 0ull;
    if ((unsigned __int128)max_weight * 2u * most_windows > (unsigned __int128)UINT64_MAX)
        return gfail(GFM_ERR_INVALID, who + "a sequence holds up to " + std::to_string(2 * most_windows) +
                                      " windows: with weights up to " + std::to_string((unsigned long long)max_weight) +
                                      " a sum may pass 2^64 - 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int K = n_replicates;
    GX_TRY(hipMemsetAsync(d_status, 0, sizeof(int32_t), st));
    for (int m = 0; m < n_motifs; ++m) {                           // (what the kernel adds to)
        GX_TRY(hipMemsetAsync(d_ge_best[m], 0, sizeof(uint32_t) * (size_t)n_seqs, st));
        GX_TRY(hipMemsetAsync(d_ge_sum[m], 0, sizeof(uint32_t) * (size_t)n_seqs, st));
        if (d_rep_hits[m]) GX_TRY(hipMemsetAsync(d_rep_hits[m], 0, sizeof(uint64_t) * (size_t)K, st));
    }
    // ---- the scratch: the unit table, class after class, and the images of the sequences beyond the LDS cap
    std::vector<NullSeq> listed;
    size_t first[kNullClasses + 1] = {};
    for (int c = 0; c < kNullClasses; ++c) {
        first[c] = listed.size();
        listed.insert(listed.end(), by_class[c].begin(), by_class[c].end());
    }
    first[kNullClasses] = listed.size();
    const long long n_blocks = (K + kNullLanes - 1) / kNullLanes;
    const size_t table_bytes = align256(sizeof(NullSeq) * listed.size());
    const int far = kNullClasses - 1;
    const size_t image_bytes = (size_t)std::max(longest[far], 1) * kNullLanes;
    const size_t far_units = by_class[far].size() * (size_t)n_blocks;
    const size_t far_blocks = std::min(std::min(far_units, (size_t)kNullMaxBlocks), std::max<size_t>(kNullScratchBytes / image_bytes, 1));
    unsigned char *d_scratch = nullptr;
    GX_TRY(hipMallocAsync(reinterpret_cast<void **>(&d_scratch), table_bytes + far_blocks * image_bytes, st));
    NullSeq *d_listed = reinterpret_cast<NullSeq *>(d_scratch);
    hipError_t e = hipMemcpyAsync(d_listed, listed.data(), sizeof(NullSeq) * listed.size(), hipMemcpyHostToDevice, st);
    const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0;
    const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(d_seq_keys);
    const auto in_lds = order == 2 ? shuffle_null_kernel<true, 2> : shuffle_null_kernel<true, 1>;
    const auto in_memory = order == 2 ? shuffle_null_kernel<false, 2> : shuffle_null_kernel<false, 1>;
    for (int m0 = 0; e == hipSuccess && m0 < n_motifs; m0 += kSeqMotifs) {
        const int mm = std::min(kSeqMotifs, n_motifs - m0);
        NullOut out = {};
        for (int k = 0; k < mm; ++k) {
            out.obs_best[k] = d_obs_best[m0 + k];
            out.obs_sum[k] = reinterpret_cast<unsigned long long *>(d_obs_sum[m0 + k]);
            out.ge_best[k] = d_ge_best[m0 + k];
            out.ge_sum[k] = d_ge_sum[m0 + k];
            out.rep_hits[k] = reinterpret_cast<unsigned long long *>(d_rep_hits[m0 + k]);
            out.rep_best[k] = d_rep_best[m0 + k];
            out.rep_sum[k] = reinterpret_cast<unsigned long long *>(d_rep_sum[m0 + k]);
            out.cut[k] = cuts[m0 + k];
        }
        const SeqMotifs mt = seq_motifs(ms, d_weights, m0, mm);
        for (int c = 0; e == hipSuccess && c < kNullClasses; ++c) {
            const long long n_listed = (long long)(first[c + 1] - first[c]);
            if (!n_listed) continue;
            if (c < far) {
                const unsigned blocks = (unsigned)std::min<long long>(n_listed * n_blocks, kNullMaxBlocks);
                hipLaunchKernelGGL(in_lds, dim3(blocks),
                                   dim3(kNullLanes), (size_t)longest[c] * kNullLanes, st, d_listed + first[c], n_listed, n_seqs,
                                   d_bases, n_bases, keys, d_seq_weight, K, (unsigned long long)seed, mt, out, mm, W, fwd,
                                   longest[c], nullptr, d_status, walk_cap);
            } else {
                hipLaunchKernelGGL(in_memory, dim3((unsigned)far_blocks), dim3(kNullLanes), 0, st, d_listed + first[c], n_listed, n_seqs,
                                   d_bases, n_bases, keys, d_seq_weight, K, (unsigned long long)seed, mt, out, mm, W, fwd,
                                   longest[c], d_scratch + table_bytes, d_status, walk_cap);
            }
            e = hipGetLastError();
        }
    }
    int32_t verdict = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&verdict, d_status, sizeof verdict, hipMemcpyDeviceToHost, st);
    const hipError_t ef = hipFreeAsync(d_scratch, st);
    const hipError_t es = hipStreamSynchronize(st);              // (also on failure: the unit table's host copy is still read)
    if (e == hipSuccess) e = ef;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return gfail(GFM_ERR_HIP, who + hipGetErrorString(e));
    if (verdict & kNullBadSeq) return gfail(GFM_ERR_INVALID, who + "a listed sequence lies outside the call's");
    return GFM_OK;
}

}  // namespace

GFM_API int gfm_sequence_shuffle_null(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                      uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                                      const uint64_t *d_seq_keys, const uint32_t *d_seq_weight, int32_t n_replicates,
                                      uint64_t seed, const int32_t *cuts, uint32_t flags, int32_t *const *d_obs_best,
                                      uint64_t *const *d_obs_sum, uint32_t *const *d_ge_best, uint32_t *const *d_ge_sum,
                                      uint64_t *const *d_rep_hits, int32_t *const *d_rep_best, uint64_t *const *d_rep_sum,
                                      int32_t *d_status, void *stream)
{
    return sequence_shuffle_null("gfm_sequence_shuffle_null", motifs, n_motifs, d_weights, max_weight, n_seqs, seq_offsets, d_bases,
                                 d_seq_keys, d_seq_weight, n_replicates, seed, 1, 0, cuts, flags, d_obs_best, d_obs_sum, d_ge_best,
                                 d_ge_sum, d_rep_hits, d_rep_best, d_rep_sum, d_status, stream);
}

GFM_API int gfm_sequence_shuffle_null_order(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights,
                                            uint64_t max_weight, int32_t n_seqs, const int64_t *seq_offsets, const uint8_t *d_bases,
                                            const uint64_t *d_seq_keys, const uint32_t *d_seq_weight, int32_t n_replicates,
                                            uint64_t seed, int32_t order, int32_t walk_cap, const int32_t *cuts, uint32_t flags,
                                            int32_t *const *d_obs_best, uint64_t *const *d_obs_sum, uint32_t *const *d_ge_best,
                                            uint32_t *const *d_ge_sum, uint64_t *const *d_rep_hits, int32_t *const *d_rep_best,
                                            uint64_t *const *d_rep_sum, int32_t *d_status, void *stream)
{
    if (order != 1 && order != 2)
        return gfail(GFM_ERR_INVALID, "gfm_sequence_shuffle_null_order: order " + std::to_string(order) + " is neither 1 nor 2");
    if (walk_cap < 0 || walk_cap > GFM_NULL_MAX_WALK_CAP)
        return gfail(GFM_ERR_INVALID, "gfm_sequence_shuffle_null_order: walk_cap " + std::to_string(walk_cap) + " outside [0, " +
                                      std::to_string(GFM_NULL_MAX_WALK_CAP) + "]");
    return sequence_shuffle_null("gfm_sequence_shuffle_null_order", motifs, n_motifs, d_weights, max_weight, n_seqs, seq_offsets,
                                 d_bases, d_seq_keys, d_seq_weight, n_replicates, seed, order, walk_cap, cuts, flags, d_obs_best,
                                 d_obs_sum, d_ge_best, d_ge_sum, d_rep_hits, d_rep_best, d_rep_sum, d_status, stream);
}
