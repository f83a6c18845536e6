// hit_linkage.hip -- gfm_hit_linkage: which alleles around a row are carried by the same haplotypes as the row.
//
// A banded popcount "matrix product", rows x flanking alleles x bitset words.  Nothing here knows a graph: a row is
// (lo, hi, carrier bitset), a site is (pos, n_alts, up to three allele bitsets), and a cell (row, site, allele a <= n_alts)
// is a CANDIDATE when distance = max(lo - pos, pos - (hi - 1), 0) <= flank.  For a candidate
//   n_joint = popcount(row & allele),  Dn = H * n_joint - n_hit * n_allele,  den = n_hit (H - n_hit) n_allele (H - n_allele),
// and the cell is LISTED when den != 0 and Dn^2 >= (min_r2 - 1e-9) * den in fp64 -- r^2 >= min_r2 with slack and without a
// division.  Only integers leave the device; the caller computes r^2 itself and makes the final cut, so the rounding here
// can only list a cell too many.
//
// Preparation.  link_check_kernel verifies the order and the bounds and copies n_alts; an exclusive sum (hipcub) over it
// COMPACTS the (site, allele) slots -- real data is mostly biallelic, three slots per site would idle two thirds of the
// lanes --; link_slot_kernel (a wavefront per site) writes each slot's bitset row and its popcount; link_range_kernel
// (a thread per row) finds the row's slot range by binary search over pos and counts the row's carriers.  rows ascend in
// lo, so the slot ranges of consecutive rows overlap almost entirely.
//
// Main pass, link_kernel<FILL>, one body for counting and writing.  A workgroup (4 wavefronts) takes a TILE of up to 32
// consecutive rows and sweeps the union of their slot ranges in chunks of 64 k slots (k <= 4).  A chunk's allele words
// are staged in LDS 16 words at a time, laid out [word][slot] with a row stride of 257 words: the lanes of a wavefront read
// consecutive 8-byte words (conflict-free ds_read_b64), and the staging writes, which walk the words of a slot, step 514
// dwords = 2 banks per lane.  A wavefront owns 8 rows of the tile; lane = slot.  Per word and 64 slots it does ONE LDS
// read and, for each of its 8 rows, an AND with the row's word -- wave-uniform, read through the scalar cache -- and a
// popcount-accumulate into a register: LDS traffic is an eighth of the intersections and the loop is VALU-bound.  Bitsets
// wider than 16 words loop over word chunks with the 8 x k counts kept in registers.  A ballot over the lanes ranks a row's
// links of 64 slots in ascending slot order, the wavefront's running count per row orders the chunks: the table's order
// without atomics or appended lists.  Count first (per-row counts, exclusive sum), then the same body writes.
//
// Vector stores only, no inline assembly, nothing that depends on XNACK.

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>

#include "grafimo_hip.h"

#define GFM_API extern "C" __attribute__((visibility("default")))
extern "C" void gfm_set_error_(const char *msg);   // thread-local slot of grafimo_hip.hip

namespace {

int lfail(int code, const std::string &msg)
{
    gfm_set_error_(msg.c_str());
    return code;
}

#define HL_TRY(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return lfail(GFM_ERR_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_));    \
    } while (0)

constexpr int kThreads = 256;                    // four wavefronts
constexpr int kRows = 8;                         // rows of a wavefront (R)
constexpr int kMaxTile = kRows * (kThreads / 64);
constexpr int kMaxSub = 4;                       // 64-slot sub-chunks of a chunk (k)
constexpr int kWordChunk = 16;                   // words staged at a time
constexpr int kStride = 64 * kMaxSub + 1;        // LDS row stride in words: odd, so the staging writes spread over the banks
constexpr int kMaxBlocks = 256 * 8;
constexpr int kMaxHaplotypes = 32768;            // Dn^2 and den stay inside int64
constexpr long long kCoordLimit = 1ll << 61;
constexpr long long kMaxSites = 1ll << 29;       // 3 * sites stays inside int32

using u64 = unsigned long long;

// thread i: row i (lo ascending, lo <= hi, inside the limit) and site i (pos ascending, n_alts <= 3, inside the limit)
// -> *bad != 0 otherwise; slot_base[i] = n_alts[i], slot_base[n_sites] = 0 (the exclusive sum's input)
__global__ void __launch_bounds__(kThreads)
link_check_kernel(const long long *__restrict__ lo, const long long *__restrict__ hi, long long n_rows,
                  const long long *__restrict__ pos, const unsigned char *__restrict__ n_alts, long long n_sites,
                  int *__restrict__ slot_base, int *__restrict__ bad)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool wrong = false;
    if (i < n_rows) {
        const long long l = lo[i], h = hi[i];
        wrong = l > h || l <= -kCoordLimit || h >= kCoordLimit || (i > 0 && lo[i - 1] > l);
    }
    if (i < n_sites) {
        const long long p = pos[i];
        const int na = n_alts[i];
        wrong = wrong || na > 3 || p <= -kCoordLimit || p >= kCoordLimit || (i > 0 && pos[i - 1] > p);
        slot_base[i] = min(na, 3);
    } else if (i == n_sites) {
        slot_base[i] = 0;
    }
    if (wrong) *bad = 1;
}

// a wavefront per site: the bitset row (site * 3 + a - 1) and the popcount of every used slot; n_allele [n_sites][3]
__global__ void __launch_bounds__(kThreads)
link_slot_kernel(const unsigned char *__restrict__ n_alts, const u64 *__restrict__ bits, long long n_sites, int hw,
                 const int *__restrict__ slot_base, int *__restrict__ slot_src, int *__restrict__ slot_pc,
                 int *__restrict__ n_allele)
{
    const int lane = threadIdx.x & 63;
    const long long waves = ((long long)gridDim.x * kThreads) >> 6;
    for (long long s = ((long long)blockIdx.x * kThreads + threadIdx.x) >> 6; s < n_sites; s += waves) {
        const int na = n_alts[s];
        const u64 *b = bits + (size_t)s * 3 * hw;
        int c0 = 0, c1 = 0, c2 = 0;
        for (int i = lane; i < na * hw; i += 64) {
            const int pc = __popcll(b[i]), a = i / hw;
            c0 += a == 0 ? pc : 0;
            c1 += a == 1 ? pc : 0;
            c2 += a == 2 ? pc : 0;
        }
        for (int d = 32; d; d >>= 1) {
            c0 += __shfl_xor(c0, d);
            c1 += __shfl_xor(c1, d);
            c2 += __shfl_xor(c2, d);
        }
        if (lane < 3) {
            const int c = lane == 0 ? c0 : lane == 1 ? c1 : c2;
            n_allele[s * 3 + lane] = lane < na ? c : 0;
            if (lane < na) {
                const int at = slot_base[s] + lane;
                slot_src[at] = (int)(s * 3 + lane);
                slot_pc[at] = c;
            }
        }
    }
}

// thread per row: the slots of the sites with lo - flank <= pos <= hi - 1 + flank, and the row's carriers
__global__ void __launch_bounds__(kThreads)
link_range_kernel(const long long *__restrict__ lo, const long long *__restrict__ hi, const u64 *__restrict__ masks,
                  long long n_rows, int hw, const long long *__restrict__ pos, long long n_sites, long long flank,
                  const int *__restrict__ slot_base, int *__restrict__ row_begin, int *__restrict__ row_end,
                  int *__restrict__ n_hit)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_rows) return;
    const long long first = lo[i] - flank, last = hi[i] - 1 + flank;
    long long a = 0, b = n_sites;
    while (a < b) {                                   // the first site with pos >= first
        const long long m = (a + b) >> 1;
        if (pos[m] < first) a = m + 1; else b = m;
    }
    const long long s0 = a;
    b = n_sites;
    while (a < b) {                                   // the first site with pos > last
        const long long m = (a + b) >> 1;
        if (pos[m] <= last) a = m + 1; else b = m;
    }
    const int begin = slot_base[s0];
    row_begin[i] = begin;
    row_end[i] = max(begin, slot_base[a]);
    const u64 *m = masks + (size_t)i * hw;
    int c = 0;
    for (int w = 0; w < hw; ++w) c += __popcll(m[w]);
    n_hit[i] = c;
}

// FILL false: link_off[row] = links of the row.  FILL true: the links of the row to link_off[row] .. in ascending slot.
// T: rows of a tile (8, 16 or 32: T / 8 wavefronts compute, all four stage); k: 64-slot sub-chunks of a chunk; the words
// of a staging step are 2^logWC <= 16.
template <bool FILL>
__global__ void __launch_bounds__(kThreads)
link_kernel(const u64 *__restrict__ masks, long long n_rows, const u64 *__restrict__ bits, int hw, int H,
            const int *__restrict__ slot_src, const int *__restrict__ slot_pc, const int *__restrict__ row_begin,
            const int *__restrict__ row_end, const int *__restrict__ n_hit, double thr, int T, int k, int logWC,
            long long *__restrict__ link_off, long long capacity, int *__restrict__ o_site,
            unsigned char *__restrict__ o_allele, int *__restrict__ o_joint)
{
    __shared__ u64 lds[kWordChunk * kStride];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = 64 * k, wc = 1 << logWC;
    for (long long t0 = (long long)blockIdx.x * T; t0 < n_rows; t0 += (long long)gridDim.x * T) {
        const int nt = (int)min((long long)T, n_rows - t0);
        const int ub = row_begin[t0];                 // (begin ascends with lo; the ends need not)
        int ue = ub;
        for (int r = 0; r < nt; ++r) ue = max(ue, row_end[t0 + r]);
        const long long r0 = t0 + wave * kRows;       // this wavefront's rows r0 .. r0 + nr - 1, their slots gb .. ge - 1
        const int nr = wave * kRows < nt ? min(kRows, nt - wave * kRows) : 0;
        int gb = 0, ge = 0;
        if (nr) {
            gb = row_begin[r0];
            ge = gb;
            for (int r = 0; r < nr; ++r) ge = max(ge, row_end[r0 + r]);
        }
        int cnt[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) cnt[r] = 0;
        for (int c0 = ub; c0 < ue; c0 += S) {
            int acc[kMaxSub][kRows];
            bool act[kMaxSub];
#pragma unroll
            for (int j = 0; j < kMaxSub; ++j) {
                act[j] = j < k && nr && c0 + 64 * j < ge && c0 + 64 * j + 64 > gb;
#pragma unroll
                for (int r = 0; r < kRows; ++r) acc[j][r] = 0;
            }
            for (int w0 = 0; w0 < hw; w0 += wc) {
                const int nw = min(wc, hw - w0);
                __syncthreads();                      // (the words of the step before are read)
                for (int i = threadIdx.x; i < (S << logWC); i += kThreads) {
                    const int sl = i >> logWC, w = i & (wc - 1), slot = c0 + sl;
                    if (w < nw) lds[w * kStride + sl] = slot < ue ? bits[(size_t)slot_src[slot] * hw + w0 + w] : 0ull;
                }
                __syncthreads();
                if (nr) {
                    for (int w = 0; w < nw; ++w) {
                        u64 m[kRows];                 // wave-uniform: rows past the last repeat it and are not listed
#pragma unroll
                        for (int r = 0; r < kRows; ++r) m[r] = masks[(size_t)min(r0 + r, n_rows - 1) * hw + w0 + w];
#pragma unroll
                        for (int j = 0; j < kMaxSub; ++j) {
                            if (!act[j]) continue;
                            const u64 v = lds[w * kStride + 64 * j + lane];
                            const unsigned vl = (unsigned)v, vh = (unsigned)(v >> 32);
#pragma unroll
                            for (int r = 0; r < kRows; ++r) {         // (two v_and and two accumulating v_bcnt per row)
                                acc[j][r] = __popc(vl & (unsigned)m[r]) + acc[j][r];
                                acc[j][r] = __popc(vh & (unsigned)(m[r] >> 32)) + acc[j][r];
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kMaxSub; ++j) {
                if (!act[j]) continue;
                const int slot = c0 + 64 * j + lane;
                const bool in = slot < ue;
                const int na = in ? slot_pc[slot] : 0, src = in ? slot_src[slot] : 0;
#pragma unroll
                for (int r = 0; r < kRows; ++r) {
                    if (r >= nr) continue;
                    const long long row = r0 + r;
                    const int nh = n_hit[row], nj = acc[j][r];
                    bool keep = in && slot >= row_begin[row] && slot < row_end[row];
                    if (keep) {
                        const long long Dn = (long long)H * nj - (long long)nh * na;
                        const long long den = (long long)nh * (H - nh) * ((long long)na * (H - na));
                        keep = den != 0 && (double)(Dn * Dn) >= thr * (double)den;
                    }
                    const u64 b = __ballot(keep);
                    if (FILL && keep) {
                        const long long at = link_off[row] + cnt[r] + __popcll(b & ((1ull << lane) - 1ull));
                        if (at >= 0 && at < capacity) {
                            o_site[at] = src / 3;
                            o_allele[at] = (unsigned char)(src % 3 + 1);
                            o_joint[at] = nj;
                        }
                    }
                    cnt[r] += __popcll(b);
                }
            }
        }
        if (!FILL && lane == 0) {
#pragma unroll
            for (int r = 0; r < kRows; ++r)
                if (r < nr) link_off[r0 + r] = cnt[r];
        }
    }
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

GFM_API int gfm_hit_linkage(const int64_t *d_lo, const int64_t *d_hi, const uint64_t *d_masks, int64_t n_rows,
                            const int64_t *d_pos, const uint8_t *d_n_alts, const uint64_t *d_allele_bits, int64_t n_sites,
                            int32_t hw, int32_t n_haplotypes, int64_t flank, double min_r2, int64_t *d_link_off,
                            int64_t link_capacity, int32_t *d_site, uint8_t *d_allele, int32_t *d_joint, int32_t *d_n_hit,
                            int32_t *d_n_allele, int32_t rows_per_tile, int32_t slots_per_chunk, uint32_t flags,
                            int64_t *h_total, void *stream)
{
    const std::string me = "gfm_hit_linkage: ";
    if (n_rows < 0 || n_rows >= 0x7fffffffll) return lfail(GFM_ERR_INVALID, me + std::to_string(n_rows) + " rows (fewer than 2^31)");
    if (n_sites < 0 || n_sites >= kMaxSites) return lfail(GFM_ERR_INVALID, me + std::to_string(n_sites) + " sites (fewer than 2^29)");
    if (n_haplotypes < 1 || n_haplotypes > kMaxHaplotypes)
        return lfail(GFM_ERR_INVALID, me + std::to_string(n_haplotypes) + " haplotypes (1 .. 32768: Dn and den stay inside int64)");
    if (hw < 1 || (long long)(hw - 1) * 64 >= n_haplotypes || (long long)hw * 64 < n_haplotypes)
        return lfail(GFM_ERR_INVALID, me + "hw is not ceil(n_haplotypes / 64)");
    if (flank < 0 || flank >= kCoordLimit) return lfail(GFM_ERR_INVALID, me + "flank outside 0 .. 2^61");
    if (!(min_r2 >= 0.0 && min_r2 <= 1.0)) return lfail(GFM_ERR_INVALID, me + "min_r2 outside 0 .. 1");
    if (rows_per_tile == 0) rows_per_tile = kMaxTile;
    if (slots_per_chunk == 0) slots_per_chunk = 64 * kMaxSub;
    if (rows_per_tile != 8 && rows_per_tile != 16 && rows_per_tile != 32)
        return lfail(GFM_ERR_INVALID, me + "rows_per_tile is 0, 8, 16 or 32");
    if (slots_per_chunk != 64 && slots_per_chunk != 128 && slots_per_chunk != 256)
        return lfail(GFM_ERR_INVALID, me + "slots_per_chunk is 0, 64, 128 or 256");
    if (!d_link_off || !h_total || link_capacity < 0 || (flags & ~GFM_LINKAGE_HAVE_OFFSETS))
        return lfail(GFM_ERR_INVALID, me + "bad argument");
    if (n_rows > 0 && (!d_lo || !d_hi || !d_masks || !d_n_hit)) return lfail(GFM_ERR_INVALID, me + "NULL row buffer");
    if (n_sites > 0 && (!d_pos || !d_n_alts || !d_allele_bits || !d_n_allele)) return lfail(GFM_ERR_INVALID, me + "NULL site buffer");
    if (link_capacity > 0 && (!d_site || !d_allele || !d_joint)) return lfail(GFM_ERR_INVALID, me + "NULL link buffer");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const auto *lo = reinterpret_cast<const long long *>(d_lo), *hi = reinterpret_cast<const long long *>(d_hi);
    const auto *pos = reinterpret_cast<const long long *>(d_pos);
    const auto *masks = reinterpret_cast<const u64 *>(d_masks), *bits = reinterpret_cast<const u64 *>(d_allele_bits);
    auto *off = reinterpret_cast<long long *>(d_link_off);
    *h_total = 0;

    size_t cub_slots = 0, cub_rows = 0;
    HL_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_slots, (int *)nullptr, (int *)nullptr, (int)(n_sites + 1), st));
    HL_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_rows, off, off, (int)(n_rows + 1), st));
    const size_t o_base = 256, o_src = o_base + up256(sizeof(int) * ((size_t)n_sites + 1)),
                 o_pc = o_src + up256(sizeof(int) * 3 * (size_t)n_sites), o_rb = o_pc + up256(sizeof(int) * 3 * (size_t)n_sites),
                 o_re = o_rb + up256(sizeof(int) * (size_t)n_rows), o_cub = o_re + up256(sizeof(int) * (size_t)n_rows),
                 bytes = o_cub + std::max(cub_slots, cub_rows);
    unsigned char *mem = nullptr;
    HL_TRY(hipMallocAsync(reinterpret_cast<void **>(&mem), bytes, st));
    int *bad = reinterpret_cast<int *>(mem), *slot_base = reinterpret_cast<int *>(mem + o_base);
    int *slot_src = reinterpret_cast<int *>(mem + o_src), *slot_pc = reinterpret_cast<int *>(mem + o_pc);
    int *row_begin = reinterpret_cast<int *>(mem + o_rb), *row_end = reinterpret_cast<int *>(mem + o_re);
    const long long checked = std::max<long long>(n_rows, n_sites + 1);
    const unsigned row_blocks = (unsigned)((n_rows + kThreads - 1) / kThreads);
    const long long tiles = (n_rows + rows_per_tile - 1) / rows_per_tile;
    const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>(tiles, kMaxBlocks));
    const int k = slots_per_chunk / 64;
    int logWC = 0;
    while ((1 << logWC) < hw && (1 << logWC) < kWordChunk) ++logWC;
    const double thr = min_r2 - 1e-9;
    int h_bad = 0;
    long long total = 0;

    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(link_check_kernel, dim3((unsigned)((checked + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, lo, hi,
                           (long long)n_rows, pos, d_n_alts, (long long)n_sites, slot_base, bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // (sites out of order would send the binary search anywhere, n_alts > 3 a slot past the buffers: nothing runs on them)
    if (e == hipSuccess && !h_bad) {
        e = hipcub::DeviceScan::ExclusiveSum(mem + o_cub, cub_slots, slot_base, slot_base, (int)(n_sites + 1), st);
        if (e == hipSuccess && n_sites > 0) {
            const unsigned sb = (unsigned)std::min<long long>((n_sites + 3) / 4, kMaxBlocks);
            hipLaunchKernelGGL(link_slot_kernel, dim3(sb), dim3(kThreads), 0, st, d_n_alts, bits, (long long)n_sites, (int)hw,
                               slot_base, slot_src, slot_pc, d_n_allele);
            e = hipGetLastError();
        }
        if (e == hipSuccess && n_rows > 0) {
            hipLaunchKernelGGL(link_range_kernel, dim3(row_blocks), dim3(kThreads), 0, st, lo, hi, masks, (long long)n_rows, (int)hw,
                               pos, (long long)n_sites, (long long)flank, slot_base, row_begin, row_end, d_n_hit);
            e = hipGetLastError();
        }
        if (e == hipSuccess && !(flags & GFM_LINKAGE_HAVE_OFFSETS)) {
            e = hipMemsetAsync(off, 0, sizeof(long long) * ((size_t)n_rows + 1), st);
            if (e == hipSuccess && n_rows > 0) {
                hipLaunchKernelGGL(link_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, masks, (long long)n_rows, bits, (int)hw,
                                   (int)n_haplotypes, slot_src, slot_pc, row_begin, row_end, d_n_hit, thr, (int)rows_per_tile, k,
                                   logWC, off, 0ll, nullptr, nullptr, nullptr);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(mem + o_cub, cub_rows, off, off, (int)(n_rows + 1), st);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&total, off + n_rows, sizeof(long long), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess && total > 0 && link_capacity >= total) {
            hipLaunchKernelGGL(link_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, masks, (long long)n_rows, bits, (int)hw,
                               (int)n_haplotypes, slot_src, slot_pc, row_begin, row_end, d_n_hit, thr, (int)rows_per_tile, k, logWC,
                               off, (long long)link_capacity, d_site, d_allele, d_joint);
            e = hipGetLastError();
        }
    }
    const hipError_t ef = hipFreeAsync(mem, st);
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) return lfail(GFM_ERR_HIP, me + hipGetErrorString(e));
    if (h_bad)
        return lfail(GFM_ERR_INVALID, me + "the rows are not in ascending lo order or the sites not in ascending pos order, a row has "
                                           "lo > hi, a site more than 3 ALTs, or a coordinate lies beyond 2^61");
    if (total < 0) return lfail(GFM_ERR_INVALID, me + "d_link_off does not hold offsets");
    *h_total = total;
    return GFM_OK;
}
