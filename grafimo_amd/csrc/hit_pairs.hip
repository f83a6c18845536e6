// hit_pairs.hip -- gfm_hit_pairs: which rows of a table lie close to each other AND share carriers.
//
// A banded, segmented self-join over intervals sorted by (group, lo), with a bitset intersection per candidate.  Nothing
// here knows a graph: the rows are (group, lo, hi, carrier bitset), and a pair is two rows a < b of one group with
//   min_gap <= gap <= max_gap,  gap = max(lo_a, lo_b) - min(hi_a, hi_b)   and   popcount(mask_a & mask_b) > 0.
// The candidates of row a are the rows behind it in its group while lo_b - hi_a <= max_gap: lo is ascending inside a group
// and gap >= lo_b - hi_a, so no pair lies behind the first row that fails it; the full gap test and the intersection decide.
//
// Decomposition.  A WAVEFRONT per row a (grid-stride over the rows, four per workgroup, no LDS and no barrier).  The 64
// lanes are cut into sub-groups of L = min(64, 2^ceil(log2 hw)) lanes; a sub-group takes one candidate, its lanes the
// words of the two bitsets (a loop over word chunks when hw > 64), and a log2(L)-step xor-shuffle sum gives the candidate's
// joint count.  So hw == 1 tests 64 candidates per step, one per lane, and hw >= 64 one candidate per step with every lane
// on a word.  Row a's words stay in registers when a lane has at most two of them (hw <= 128: 8 192 haplotypes).  The
// candidates' bitsets are read where they are: rows next to each other are each other's candidates, so a bitset is read
// by the waves of the 10^2 rows before it within a short time and comes from L2 (see DESIGN.md 3.12 for the traffic model).
// A ballot over the sub-groups' first lanes ranks the pairs of a step, which keeps every row's pairs in ascending b without
// an atomic.  The per-group counts are made only for pairs, lane g summing group g over the words of a transposed copy of
// the group bitsets ([word][group]: the lanes' loads are neighbours).
//
// Two passes over the candidates: pair_count_kernel counts per row, an exclusive sum makes the CSR offsets, and -- when the
// caller has room -- the same kernel body runs again and writes (count first, then allocate: no appended, unordered lists).

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>

#include "grafimo_hip.h"

#define GFM_API extern "C" __attribute__((visibility("default")))
extern "C" void gfm_set_error_(const char *msg);   // thread-local slot of grafimo_hip.hip

namespace {

int pfail(int code, const std::string &msg)
{
    gfm_set_error_(msg.c_str());
    return code;
}

#define HP_TRY(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return pfail(GFM_ERR_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_));    \
    } while (0)

constexpr int kThreads = 256;                    // four wavefronts, a row each
constexpr int kMaxBlocks = 256 * 8;
constexpr long long kCoordLimit = 1ll << 61;     // |lo|, |hi|, |gap bounds| below it: no difference of two overflows

using u64 = unsigned long long;

// thread per row: the order (group, lo) ascending, lo <= hi, coordinates inside the limit -> *bad != 0 otherwise
__global__ void __launch_bounds__(kThreads)
pair_check_kernel(const int *__restrict__ group, const long long *__restrict__ lo, const long long *__restrict__ hi,
                  long long n, int *__restrict__ bad)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long l = lo[i], h = hi[i];
    bool wrong = l > h || l <= -kCoordLimit || h >= kCoordLimit;
    if (i > 0) {
        const int g0 = group[i - 1], g1 = group[i];
        wrong = wrong || g0 > g1 || (g0 == g1 && lo[i - 1] > l);
    }
    if (wrong) *bad = 1;
}

// group_bits [G][hw] -> [hw][G]
__global__ void __launch_bounds__(kThreads)
pair_transpose_kernel(const u64 *__restrict__ in, int G, int hw, u64 *__restrict__ out)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)G * hw) return;
    const int w = (int)(t / G), g = (int)(t % G);
    out[t] = in[(size_t)g * hw + w];
}

// FILL false: counts[a] = pairs of row a.  FILL true: the pairs of row a to pair_off[a] .. in ascending b.
template <bool FILL>
__global__ void __launch_bounds__(kThreads)
pair_kernel(const int *__restrict__ group, const long long *__restrict__ lo, const long long *__restrict__ hi,
            const u64 *__restrict__ masks, long long n, int hw, int logL, long long min_gap, long long max_gap,
            long long *__restrict__ pair_off, long long capacity, int *__restrict__ pair_b, int *__restrict__ joint, int G,
            const u64 *__restrict__ group_bits_t, int *__restrict__ group_counts)
{
    const int lane = threadIdx.x & 63;
    const int L = 1 << logL, sub = lane & (L - 1), slot = lane >> logL, per_step = 64 >> logL;
    const bool in_regs = hw <= 2 * L;
    const long long waves = ((long long)gridDim.x * kThreads) >> 6;
    for (long long a = ((long long)blockIdx.x * kThreads + threadIdx.x) >> 6; a < n; a += waves) {
        const int ga = group[a];
        const long long hia = hi[a];
        const u64 *ma = masks + (size_t)a * hw;
        const u64 a0 = sub < hw ? ma[sub] : 0ull, a1 = sub + L < hw ? ma[sub + L] : 0ull;
        const long long off = FILL ? pair_off[a] : 0;
        long long cnt = 0;
        for (long long base = a + 1;; base += per_step) {
            const long long b = base + slot;
            bool valid = b < n && group[b] == ga;
            long long lob = 0;
            if (valid) {
                lob = lo[b];
                valid = lob - hia <= max_gap;
            }
            bool test = false;
            if (valid) {
                const long long gap = lob - min(hia, hi[b]);          // (lo_b >= lo_a: the order)
                test = gap >= min_gap && gap <= max_gap;
            }
            int pc = 0;
            if (test) {
                const u64 *mb = masks + (size_t)b * hw;
                if (in_regs) {
                    if (sub < hw) pc = __popcll(a0 & mb[sub]);
                    if (sub + L < hw) pc += __popcll(a1 & mb[sub + L]);
                } else {
                    for (int w = sub; w < hw; w += L) pc += __popcll(ma[w] & mb[w]);
                }
            }
            for (int d = L >> 1; d; d >>= 1) pc += __shfl_xor(pc, d);
            const bool hit = test && pc > 0 && sub == 0;
            const u64 m = __ballot(hit);
            if (FILL) {
                const long long at = off + cnt + __popcll(m & ((1ull << lane) - 1ull));
                if (hit && at < capacity) {
                    pair_b[at] = (int)b;
                    joint[at] = pc;
                }
                if (G > 0) {
                    for (u64 rest = m; rest; rest &= rest - 1ull) {
                        const int l = __ffsll((long long)rest) - 1;
                        const long long p = off + cnt + __popcll(m & ((1ull << l) - 1ull));
                        const u64 *mb = masks + (size_t)(base + (l >> logL)) * hw;
                        if (lane < G && p < capacity) {
                            int s = 0;
                            for (int w = 0; w < hw; ++w) s += __popcll(ma[w] & mb[w] & group_bits_t[(size_t)w * G + lane]);
                            group_counts[(size_t)p * G + lane] = s;
                        }
                    }
                }
            }
            cnt += __popcll(m);
            if (__ballot(!valid)) break;                               // (the first row that fails ends the candidates)
        }
        if (!FILL && lane == 0) pair_off[a] = cnt;
    }
}

}  // namespace

GFM_API int gfm_hit_pairs(const int32_t *d_group, const int64_t *d_lo, const int64_t *d_hi, const uint64_t *d_masks, int64_t n,
                          int32_t hw, int64_t min_gap, int64_t max_gap, int32_t n_groups, const uint64_t *d_group_bits,
                          int64_t *d_pair_off, int64_t pair_capacity, int32_t *d_pair_b, int32_t *d_joint,
                          int32_t *d_group_counts, uint32_t flags, int64_t *h_total, void *stream)
{
    if (n < 0 || n >= 0x7fffffffll) return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: " + std::to_string(n) + " rows (fewer than 2^31)");
    if (hw < 1) return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: hw < 1");
    if (n_groups < 0 || n_groups > 64)
        return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: " + std::to_string(n_groups) + " groups (at most 64 per call)");
    if (min_gap > max_gap) return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: min_gap > max_gap");
    if (min_gap <= -kCoordLimit || max_gap >= kCoordLimit) return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: gap bound beyond 2^61");
    if (!d_pair_off || !h_total || pair_capacity < 0 || (flags & ~GFM_PAIRS_HAVE_OFFSETS))
        return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: bad argument");
    if (n > 0 && (!d_group || !d_lo || !d_hi || !d_masks)) return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: NULL row buffer");
    if (pair_capacity > 0 && (!d_pair_b || !d_joint || (n_groups > 0 && (!d_group_bits || !d_group_counts))))
        return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: NULL pair buffer");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    int logL = 0;
    while ((1 << logL) < hw && logL < 6) ++logL;
    const auto *grp = d_group;
    const auto *lo = reinterpret_cast<const long long *>(d_lo), *hi = reinterpret_cast<const long long *>(d_hi);
    const auto *masks = reinterpret_cast<const u64 *>(d_masks);
    auto *off = reinterpret_cast<long long *>(d_pair_off);
    const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((n + 3) / 4, kMaxBlocks));
    *h_total = 0;
    if (!(flags & GFM_PAIRS_HAVE_OFFSETS)) {
        HP_TRY(hipMemsetAsync(off, 0, sizeof(long long) * ((size_t)n + 1), st));
        if (n > 0) {
            size_t cub_bytes = 0;
            HP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, off, off, (int)(n + 1), st));
            unsigned char *mem = nullptr;
            HP_TRY(hipMallocAsync(reinterpret_cast<void **>(&mem), 256 + cub_bytes, st));
            int *bad = reinterpret_cast<int *>(mem);
            hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), st);
            int h_bad = 0;
            if (e == hipSuccess) {
                hipLaunchKernelGGL(pair_check_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, grp,
                                   lo, hi, (long long)n, bad);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            // (rows out of order would end a row's candidates early: nothing is counted on them)
            if (e == hipSuccess && !h_bad) {
                hipLaunchKernelGGL(pair_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, grp, lo, hi, masks, (long long)n,
                                   (int)hw, logL, (long long)min_gap, (long long)max_gap, off, 0ll, nullptr, nullptr, 0, nullptr,
                                   nullptr);
                e = hipGetLastError();
                if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(mem + 256, cub_bytes, off, off, (int)(n + 1), st);
            }
            const hipError_t ef = hipFreeAsync(mem, st);
            if (e == hipSuccess) e = ef;
            if (e != hipSuccess) return pfail(GFM_ERR_HIP, std::string("gfm_hit_pairs: ") + hipGetErrorString(e));
            if (h_bad)
                return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: the rows are not in ascending (group, lo) order, or a row has "
                                              "lo > hi or a coordinate beyond 2^61");
        }
    }
    long long total = 0;
    HP_TRY(hipMemcpyAsync(&total, off + n, sizeof(long long), hipMemcpyDeviceToHost, st));
    HP_TRY(hipStreamSynchronize(st));
    *h_total = total;
    if (total < 0) return pfail(GFM_ERR_INVALID, "gfm_hit_pairs: d_pair_off does not hold offsets");
    if (total == 0 || pair_capacity < total) return GFM_OK;          // (nothing to write, or no room: *h_total says how much)
    u64 *gbt = nullptr;
    if (n_groups > 0) {
        const long long cells = (long long)n_groups * hw;
        HP_TRY(hipMallocAsync(reinterpret_cast<void **>(&gbt), sizeof(u64) * (size_t)cells, st));
        hipLaunchKernelGGL(pair_transpose_kernel, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           reinterpret_cast<const u64 *>(d_group_bits), (int)n_groups, (int)hw, gbt);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pair_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, grp, lo, hi, masks, (long long)n, (int)hw, logL,
                           (long long)min_gap, (long long)max_gap, off, (long long)pair_capacity, d_pair_b, d_joint, (int)n_groups,
                           gbt, d_group_counts);
        e = hipGetLastError();
    }
    if (gbt) {
        const hipError_t ef = hipFreeAsync(gbt, st);
        if (e == hipSuccess) e = ef;
    }
    if (e != hipSuccess) return pfail(GFM_ERR_HIP, std::string("gfm_hit_pairs: ") + hipGetErrorString(e));
    return GFM_OK;
}
