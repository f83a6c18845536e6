// gfm_scan_fold.hpp -- the fold over the motif axis: what a keys/sums scan entry left per motif, reduced on the device to a running
// per-(row, pair) state of counts and champions (included at the end of graph_extract.hip behind the scan headers; it uses gfail,
// GX_TRY and kSeqMotifs).  The mutation profile is the first table built on it.
//
// THE RULE (include/grafimo_hip.h states it for the library; tests/mutation_profile_bruteforce.py on the host).  For every
// (row, pair (ref column, alt column)) and every motif, with r, a the two keys' scores (key >> 8) - 1 (-1 for key 0) and R, A
// the two sums:
//   A side is a site when its key is not 0 and its score >= the motif's cutoff.
//   gain when a is a site and r is not.  loss when r is a site and a is not.  counts[gain] and counts[loss] count the motifs.
//   Gain champion: the gaining motif with the smallest ptable[a].  Loss champion: the losing motif with the smallest ptable[r].
//   A score >= table_len reads entry table_len - 1.  Doubles are compared as doubles.  Ties go to the smaller motif id.
//   Up champion: among motifs with A > R, the one with the largest A / R, compared exactly: motif 1 beats motif 2 when
//   A1 * R2 > A2 * R1 in 128-bit unsigned arithmetic.  Down champion: among A < R, the largest R / A by the same rule.
//   Ties go to the smaller motif id.
//   The empty state is all zero bytes; ids are stored as id + 1.
//
// Work decomposition: a thread per (row, pair) cell, cell = row * n_pairs + pair, in a grid-stride loop; the cell's state is
// loaded once, folded over the up to kSeqMotifs motifs of the launch in registers and stored once -- one owner, no atomics.
// Every state array is [rows][P]...: consecutive lanes read and write consecutive words.  The inputs: the lanes of a wavefront
// cover 64 / P consecutive rows, a contiguous run of 64 / P * C keys and sums (a row's 20 or 40 bytes are not 16-byte
// aligned, so the loads are scalar per lane; the pairs of a row share its lines in the cache).  The motifs are taken four at
// a time: the 16 loads of a batch are issued before the first is used.  The gather into a motif's tail table happens only
// for a motif that gains or loses.  Ids, cutoffs and table lengths travel as kernel arguments, as SeqMotifs does for the scans.
namespace {

constexpr int kFoldThreads = 256;
constexpr int kFoldBatch = 4;
constexpr int kFoldMaxBlocks = 1 << 16;
constexpr int kFoldMaxColumns = 8, kFoldMaxPairs = 8;
constexpr long long kFoldMaxRows = 1ll << 40;

struct FoldMotifs {
    const unsigned *keys[kSeqMotifs];
    const unsigned long long *sums[kSeqMotifs];
    const double *ptab[kSeqMotifs];
    unsigned id1[kSeqMotifs];         // id + 1, as the state stores it
    int cutoff[kSeqMotifs];
    int last[kSeqMotifs];             // table_len - 1
};

struct FoldState {
    unsigned *counts, *site_motif, *site_keys;
    double *site_p;
    unsigned *aff_motif;
    unsigned long long *aff_sums;
};

__device__ __forceinline__ bool fold_is_site(unsigned key, int cutoff)
{
    return key != 0u && (int)(key >> 8) - 1 >= cutoff;
}

// one champion by the smallest p: (id + 1 or 0, ref key, alt key, p)
struct FoldSite {
    unsigned id1, kr, ka;
    double p;
    __device__ __forceinline__ void take(unsigned cid1, unsigned ckr, unsigned cka, double cp)
    {
        if (id1 == 0u || cp < p || (cp == p && cid1 < id1)) { id1 = cid1; kr = ckr; ka = cka; p = cp; }
    }
};

// one champion by the largest num / den, compared exactly
struct FoldRatio {
    unsigned id1;
    unsigned long long num, den;
    __device__ __forceinline__ void take(unsigned cid1, unsigned long long cnum, unsigned long long cden)
    {
        if (id1 != 0u) {
            const unsigned __int128 mine = (unsigned __int128)num * cden, theirs = (unsigned __int128)cnum * den;
            if (!(theirs > mine || (theirs == mine && cid1 < id1))) return;
        }
        id1 = cid1; num = cnum; den = cden;
    }
};

__global__ void __launch_bounds__(kFoldThreads)
scan_fold_kernel(FoldMotifs mt, int mm, long long n_cells, int C, int P, unsigned ref_cols, unsigned alt_cols, FoldState st)
{
    for (long long cell = (long long)blockIdx.x * kFoldThreads + threadIdx.x; cell < n_cells;
         cell += (long long)gridDim.x * kFoldThreads) {
        const long long row = cell / P;
        const int pair = (int)(cell - row * P);
        const long long ir = row * C + ((ref_cols >> (4 * pair)) & 15u), ia = row * C + ((alt_cols >> (4 * pair)) & 15u);
        unsigned n_gain = st.counts[2 * cell], n_loss = st.counts[2 * cell + 1];
        FoldSite gain{st.site_motif[2 * cell], st.site_keys[4 * cell], st.site_keys[4 * cell + 1], st.site_p[2 * cell]};
        FoldSite loss{st.site_motif[2 * cell + 1], st.site_keys[4 * cell + 2], st.site_keys[4 * cell + 3], st.site_p[2 * cell + 1]};
        // aff_sums keeps (ref sum, alt sum): up compares alt / ref, down ref / alt
        FoldRatio up{st.aff_motif[2 * cell], st.aff_sums[4 * cell + 1], st.aff_sums[4 * cell]};
        FoldRatio down{st.aff_motif[2 * cell + 1], st.aff_sums[4 * cell + 2], st.aff_sums[4 * cell + 3]};
        for (int m0 = 0; m0 < mm; m0 += kFoldBatch) {
            unsigned kr[kFoldBatch], ka[kFoldBatch];
            unsigned long long R[kFoldBatch], A[kFoldBatch];
#pragma unroll
            for (int j = 0; j < kFoldBatch; ++j) {
                const int m = min(m0 + j, mm - 1);                // (past the last motif: the last again, and not folded)
                kr[j] = mt.keys[m][ir]; ka[j] = mt.keys[m][ia];
                R[j] = mt.sums[m][ir]; A[j] = mt.sums[m][ia];
            }
#pragma unroll
            for (int j = 0; j < kFoldBatch; ++j) {
                const int m = m0 + j;
                if (m >= mm) break;
                const unsigned id1 = mt.id1[m];
                const bool rs = fold_is_site(kr[j], mt.cutoff[m]), as = fold_is_site(ka[j], mt.cutoff[m]);
                if (as != rs) {                                   // rare: the only read of the tail table
                    const int score = (int)((as ? ka[j] : kr[j]) >> 8) - 1;
                    const double p = mt.ptab[m][min(score, mt.last[m])];
                    if (as) { ++n_gain; gain.take(id1, kr[j], ka[j], p); }
                    else { ++n_loss; loss.take(id1, kr[j], ka[j], p); }
                }
                if (A[j] > R[j]) up.take(id1, A[j], R[j]);
                else if (A[j] < R[j]) down.take(id1, R[j], A[j]);
            }
        }
        st.counts[2 * cell] = n_gain; st.counts[2 * cell + 1] = n_loss;
        st.site_motif[2 * cell] = gain.id1; st.site_motif[2 * cell + 1] = loss.id1;
        st.site_keys[4 * cell] = gain.kr; st.site_keys[4 * cell + 1] = gain.ka;
        st.site_keys[4 * cell + 2] = loss.kr; st.site_keys[4 * cell + 3] = loss.ka;
        st.site_p[2 * cell] = gain.p; st.site_p[2 * cell + 1] = loss.p;
        st.aff_motif[2 * cell] = up.id1; st.aff_motif[2 * cell + 1] = down.id1;
        st.aff_sums[4 * cell] = up.den; st.aff_sums[4 * cell + 1] = up.num;
        st.aff_sums[4 * cell + 2] = down.num; st.aff_sums[4 * cell + 3] = down.den;
    }
}

bool fold_misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

}  // namespace

GFM_API int gfm_scan_fold(int32_t n_motifs, const int32_t *motif_ids, const int32_t *cutoffs, const double *const *d_ptables,
                          const int32_t *table_lens, int64_t n_rows, int32_t n_columns, int32_t n_pairs, const int32_t *pairs,
                          const uint32_t *const *d_keys, const uint64_t *const *d_sums, uint32_t *d_counts, uint32_t *d_site_motif,
                          uint32_t *d_site_keys, double *d_site_p, uint32_t *d_aff_motif, uint64_t *d_aff_sums, void *stream)
{
    const std::string entry = "gfm_scan_fold";
    // ---- every refusal before any device work
    if (n_motifs < 1) return gfail(GFM_ERR_INVALID, entry + ": n_motifs < 1");
    if (n_rows < 0 || n_rows > kFoldMaxRows) return gfail(GFM_ERR_INVALID, entry + ": n_rows is outside 0 .. 2^40");
    if (n_columns < 2 || n_columns > kFoldMaxColumns)
        return gfail(GFM_ERR_INVALID, entry + ": n_columns " + std::to_string(n_columns) + " is outside 2 .. " +
                                      std::to_string(kFoldMaxColumns));
    if (n_pairs < 1 || n_pairs > kFoldMaxPairs)
        return gfail(GFM_ERR_INVALID, entry + ": n_pairs " + std::to_string(n_pairs) + " is outside 1 .. " +
                                      std::to_string(kFoldMaxPairs));
    if (n_rows == 0) return GFM_OK;
    if (!motif_ids || !cutoffs || !d_ptables || !table_lens || !pairs || !d_keys || !d_sums || !d_counts || !d_site_motif ||
        !d_site_keys || !d_site_p || !d_aff_motif || !d_aff_sums)
        return gfail(GFM_ERR_INVALID, entry + ": NULL argument");
    unsigned ref_cols = 0u, alt_cols = 0u;
    for (int p = 0; p < n_pairs; ++p) {
        const int r = pairs[2 * p], a = pairs[2 * p + 1];
        if (r < 0 || r >= n_columns || a < 0 || a >= n_columns || r == a)
            return gfail(GFM_ERR_INVALID, entry + ": pair " + std::to_string(p) + " (" + std::to_string(r) + ", " + std::to_string(a) +
                                          ") is not two different columns of " + std::to_string(n_columns));
        ref_cols |= (unsigned)r << (4 * p);
        alt_cols |= (unsigned)a << (4 * p);
    }
    std::vector<int32_t> ids(motif_ids, motif_ids + n_motifs);
    std::sort(ids.begin(), ids.end());
    if (ids[0] < 0) return gfail(GFM_ERR_INVALID, entry + ": motif id " + std::to_string(ids[0]) + " is negative");
    if (ids.back() == INT32_MAX) return gfail(GFM_ERR_INVALID, entry + ": motif id 2^31 - 1 cannot be stored as id + 1");
    for (int m = 1; m < n_motifs; ++m)
        if (ids[m] == ids[m - 1]) return gfail(GFM_ERR_INVALID, entry + ": motif id " + std::to_string(ids[m]) + " is repeated");
    for (int m = 0; m < n_motifs; ++m) {
        if (table_lens[m] < 1)
            return gfail(GFM_ERR_INVALID, entry + ": table_len " + std::to_string(table_lens[m]) + " of motif " + std::to_string(m) +
                                          " is < 1");
        if (cutoffs[m] < 0 || cutoffs[m] > table_lens[m])
            return gfail(GFM_ERR_INVALID, entry + ": cutoff " + std::to_string(cutoffs[m]) + " of motif " + std::to_string(m) +
                                          " is outside 0 .. " + std::to_string(table_lens[m]));
        if (!d_ptables[m] || !d_keys[m] || !d_sums[m])
            return gfail(GFM_ERR_INVALID, entry + ": NULL device buffer of motif " + std::to_string(m));
        if (fold_misaligned8(d_sums[m]) || fold_misaligned8(d_ptables[m]))
            return gfail(GFM_ERR_INVALID, entry + ": d_sums[m] and d_ptables[m] are 8-byte aligned");
    }
    if (fold_misaligned8(d_site_p) || fold_misaligned8(d_aff_sums))
        return gfail(GFM_ERR_INVALID, entry + ": site_p and aff_sums are 8-byte aligned");
    // ---- one launch per kSeqMotifs motifs, in stream order behind whatever wrote the keys and sums; nothing is read back
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long n_cells = (long long)n_rows * n_pairs;
    const unsigned blocks = (unsigned)std::min<long long>((n_cells + kFoldThreads - 1) / kFoldThreads, (long long)kFoldMaxBlocks);
    const FoldState state{d_counts, d_site_motif, d_site_keys, d_site_p, d_aff_motif, reinterpret_cast<unsigned long long *>(d_aff_sums)};
    for (int m0 = 0; m0 < n_motifs; m0 += kSeqMotifs) {
        const int mm = std::min(kSeqMotifs, n_motifs - m0);
        FoldMotifs mt = {};
        for (int k = 0; k < mm; ++k) {
            mt.keys[k] = d_keys[m0 + k];
            mt.sums[k] = reinterpret_cast<const unsigned long long *>(d_sums[m0 + k]);
            mt.ptab[k] = d_ptables[m0 + k];
            mt.id1[k] = (unsigned)motif_ids[m0 + k] + 1u;
            mt.cutoff[k] = cutoffs[m0 + k];
            mt.last[k] = table_lens[m0 + k] - 1;
        }
        hipLaunchKernelGGL(scan_fold_kernel, dim3(blocks), dim3(kFoldThreads), 0, st, mt, mm, n_cells, (int)n_columns, (int)n_pairs,
                           ref_cols, alt_cols, state);
        GX_TRY(hipGetLastError());
    }
    return GFM_OK;
}
