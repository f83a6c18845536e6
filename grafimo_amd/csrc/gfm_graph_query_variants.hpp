// gfm_graph_query_variants.hpp -- query variants: an edit (REF -> ALT at a reference position) applied to a spelled sequence,
// every window the edit touches scored before and after on both strands (included at the end of graph_extract.hip behind
// gfm_graph_hapsequences.hpp, whose sequences -- bases and coordinates -- it reads; it uses base_code, view_motif_set, SeqMotifs,
// GX_TRY, gfail, the wave helpers and gfm_graph_table_score.hpp's window_sum, strand_scores, walk_value and edit_key).  The
// first kernel here that scores a sequence that is NOT a walk of the graph.
//
// THE RULE (include/grafimo_hip.h states it for the library; tests/query_variant_bruteforce.py on the host).  A sequence x has
// per base a coordinate, ~coordinate for an inserted base (gfm_graph_haplotype_sequences' d_coord).  An edit is (pos0, ref of
// lr bases, alt of la bases), lr, la <= 64, not both 0.
//   lr > 0:  o = the offset of the non-inserted base with coordinate pos0.  ABSENT unless every coordinate pos0 .. pos0 + lr - 1
//            is carried by a non-inserted base of x; APPLIED when x[o .. o + lr) are those bases in order (no inserted base
//            between them) and equal ref, compared without case; else MISMATCH.
//   lr == 0: o as above; ABSENT unless a non-inserted base carries pos0 - 1 as well; APPLIED when that base is x[o - 1], else
//            MISMATCH (inserted bases lie between).  No base with coordinate pos0: when the LAST base of x is the non-inserted base
//            pos0 - 1 the edit is APPLIED at o = len(x), when it is a base inserted behind pos0 - 1 it is a MISMATCH at
//            o = len(x) -- the caller vouches that x then runs to the end of its chromosome (the kernel has no chromosome) --,
//            else ABSENT.
//   y = x[:o] + alt + x[o + lr:].  REF side: the window starts s of x with s <= o + lr - 1, s + W - 1 >= o, 0 <= s <= len(x) - W;
//   ALT side: the same in y with la.  Per side the best window by (score descending, s ascending, '+' before '-') and the sum
//   over its windows and strands of w[score], exact in uint64.  A k-mer holding a base that is not A, C, G, T scores min_val.
//
// Work decomposition: grid.y = motif, a WAVEFRONT per item, grid-stride over the items (256 threads: four items in flight a
// workgroup).  The motif's packed two-strand table (W x 8 words) is staged once per workgroup in LDS; the weight table is read
// through the cache (a side meets at most 2 (W + 63) of its up to 64 001 entries).  The wave strides its lanes over the
// sequence's coordinates to find o and to count the carried coordinates, checks the REF bases with a ballot, stages the
// base codes of the used context x[max(0, o - W + 1) .. min(len, o + lr + W - 1)) and of the same stretch of y -- at most
// 2 (W - 1) + 64 = 190 bytes each -- in its own LDS slice, and each lane takes the window starts lane and lane + 64 (at most
// W + 63 <= 127 a side): W table lookups score both strands.  The key is reduced by a maximum and the weight by an integer
// sum across the wave; lane 0 writes the record.  No atomics but the status word's.
namespace {

constexpr int kQvThreads = 256, kQvWaves = kQvThreads / 64;
constexpr int kQvContext = 2 * (GFM_MAX_WIDTH - 1) + GFM_QUERY_MAX_ALLELE;          // 190
constexpr int kQvSlice = (kQvContext + 15) & ~15;
constexpr int kQvBadItem = 1, kQvBadEdit = 2, kQvBadSeq = 4;

struct QvRecords { gfm_edit_record_t *rec[kSeqMotifs]; };

struct QvInput {
    int n_seqs, n_edits;
    long long n_items;
    const long long *seq_off;
    const uint8_t *bases;
    const int *coord;
    const long long *pos0;
    const int *ref_off, *alt_off;
    const uint8_t *ref_bytes, *alt_bytes;
    const int *item_seq, *item_edit;
};

__global__ void __launch_bounds__(kQvThreads)
query_edits_kernel(QvInput in, SeqMotifs mt, QvRecords recs, int W, int forward_only, int *__restrict__ status)
{
    __shared__ unsigned ftab_s[GFM_MAX_WIDTH * 8];
    __shared__ unsigned char slices[kQvWaves][2][kQvSlice];
    const int m = blockIdx.y;
    for (int i = threadIdx.x; i < W * 8; i += kQvThreads) ftab_s[i] = mt.ftab[m][i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long *__restrict__ wtab = mt.wtab[m];
    gfm_edit_record_t *__restrict__ out = recs.rec[m];
    const int min_val = mt.min_val[m];
    unsigned char *cx = slices[wave][0], *cy = slices[wave][1];
    for (long long it = (long long)blockIdx.x * kQvWaves + wave; it < in.n_items; it += (long long)gridDim.x * kQvWaves) {
        const int v = __builtin_amdgcn_readfirstlane(in.item_seq[it]), q = __builtin_amdgcn_readfirstlane(in.item_edit[it]);
        gfm_edit_record_t rec = {GFM_EDIT_INVALID, -1, 0u, 0u, 0ull, 0ull};
        // ---- the item's sequence and edit, checked: everything read below lies inside them
        int bad = 0;
        long long a = 0, b = 0;
        int ro = 0, ao = 0, lr = 0, la = 0;
        if (v < 0 || v >= in.n_seqs || q < 0 || q >= in.n_edits) {
            bad = kQvBadItem;
        } else {
            a = in.seq_off[v];
            b = in.seq_off[v + 1];
            ro = in.ref_off[q];
            lr = in.ref_off[q + 1] - ro;
            ao = in.alt_off[q];
            la = in.alt_off[q + 1] - ao;
            if (ro < 0 || ao < 0 || lr < 0 || la < 0 || lr > GFM_QUERY_MAX_ALLELE || la > GFM_QUERY_MAX_ALLELE || lr + la == 0)
                bad = kQvBadEdit;
            else if (a < 0 || b < a || b - a > 0x7fffffffll)
                bad = kQvBadSeq;
        }
        if (bad) {
            if (lane == 0) {
                atomicOr(status, bad);
                out[it] = rec;
            }
            continue;
        }
        const int len = (int)(b - a);
        const long long p0 = in.pos0[q];
        const uint8_t *__restrict__ x = in.bases + a;
        const int *__restrict__ xc = in.coord + a;
        // ---- o, the base before it, and how many of the coordinates pos0 .. pos0 + lr - 1 are carried
        int fn = -1, fp = -1, cnt = 0;
        for (int j = lane; j < len; j += 64) {
            const int c = xc[j];
            if (c < 0) continue;
            if (c == p0) fn = j;
            if (c == p0 - 1) fp = j;
            cnt += (c >= p0 && c < p0 + lr) ? 1 : 0;
        }
        fn = wave_max(fn);
        fp = wave_max(fp);
        cnt = wave_sum(cnt);
        int st, o = fn;
        if (lr > 0) {
            if (cnt < lr) {
                st = GFM_EDIT_ABSENT;
            } else {
                bool ok = true;
                if (lane < lr) {
                    const int j = o + lane;
                    ok = j < len && xc[j] == p0 + lane && (((unsigned)x[j] ^ (unsigned)in.ref_bytes[ro + lane]) & 0xdfu) == 0u;
                }
                st = __builtin_amdgcn_ballot_w64(!ok) ? GFM_EDIT_MISMATCH : GFM_EDIT_APPLIED;
            }
        } else if (fn >= 0) {
            st = fp < 0 ? GFM_EDIT_ABSENT : fp != o - 1 ? GFM_EDIT_MISMATCH : GFM_EDIT_APPLIED;
        } else if (fp >= 0 && fp == len - 1) {
            o = len;
            st = GFM_EDIT_APPLIED;
        } else if (fp >= 0 && xc[len - 1] == ~(int)(p0 - 1)) {
            o = len;
            st = GFM_EDIT_MISMATCH;
        } else {
            st = GFM_EDIT_ABSENT;
        }
        rec.status = st;
        rec.o = o;
        if (st != GFM_EDIT_APPLIED) {
            if (lane == 0) out[it] = rec;
            continue;
        }
        // ---- the used context of x and the same stretch of y, as base codes, in the wave's slice
        const int lo = max(0, o - (W - 1)), hi = min(len, o + lr + W - 1);
        const int oc = o - lo, nx = hi - lo, ny = nx - lr + la;
        wave_lds_sync();                                     // (the last item's windows are read)
        for (int j = lane; j < nx; j += 64) cx[j] = (unsigned char)base_code(x[lo + j]);
        for (int j = lane; j < ny; j += 64) {
            const unsigned c = j < oc ? x[lo + j] : j < oc + la ? in.alt_bytes[ao + (j - oc)] : x[lo + j - la + lr];
            cy[j] = (unsigned char)base_code(c);
        }
        wave_lds_sync();
        // ---- the windows of both sides: starts 0 .. min(oc + l - 1, n - W) of the slice (oc <= W - 1: every start from 0 on
        // reaches o), the lanes take them 64 at a time
        for (int side = 0; side < 2; ++side) {
            const unsigned char *buf = side ? cy : cx;
            const int l = side ? la : lr, n = side ? ny : nx;
            const int s_hi = min(oc + l - 1, n - W);
            unsigned key = 0u;
            unsigned long long sum = 0ull;
            for (int s = lane; s <= s_hi; s += 64) {
                const WindowSum w = window_sum(ftab_s, W, [&](int j) { return (unsigned)buf[s + j]; });
                const StrandScores sc = strand_scores(w, min_val);
                key = max(key, edit_key(sc.plus, s - oc, true));              // s - o in -63 .. 63
                if (!forward_only) key = max(key, edit_key(sc.minus, s - oc, false));
                sum += walk_value(wtab, w, min_val, forward_only);
            }
            key = (unsigned)wave_max((int)key);               // (below 2^25: the order of the ints is the order of the keys)
            sum = (unsigned long long)wave_sum_ll((long long)sum);
            if (side) { rec.alt_key = key; rec.alt_sum = sum; }
            else { rec.ref_key = key; rec.ref_sum = sum; }
        }
        if (lane == 0) out[it] = rec;
    }
}

}  // namespace

GFM_API int gfm_graph_query_edits(const gfm_motif_t *motifs, int32_t n_motifs, const uint64_t *const *d_weights, uint64_t max_weight,
                                  int32_t n_seqs, const int64_t *d_seq_offsets, const uint8_t *d_bases, const int32_t *d_coord,
                                  int32_t n_edits, const int64_t *d_pos0, const int32_t *d_ref_off, const uint8_t *d_ref_bytes,
                                  const int32_t *d_alt_off, const uint8_t *d_alt_bytes, int64_t n_items, const int32_t *d_item_seq,
                                  const int32_t *d_item_edit, uint32_t flags, gfm_edit_record_t *const *d_records, int32_t *d_status,
                                  void *stream)
{
    if (n_motifs < 1 || n_seqs < 0 || n_edits < 0 || n_items < 0) return gfail(GFM_ERR_INVALID, "bad argument");
    if (flags & ~(uint32_t)GFM_GRAPH_FORWARD_ONLY) return gfail(GFM_ERR_INVALID, "unknown flag");
    if (n_items == 0) return GFM_OK;
    if (!motifs || !d_weights || !d_records || !d_status || !d_seq_offsets || !d_bases || !d_coord || !d_pos0 || !d_ref_off ||
        !d_ref_bytes || !d_alt_off || !d_alt_bytes || !d_item_seq || !d_item_edit)
        return gfail(GFM_ERR_INVALID, "gfm_graph_query_edits: NULL argument");
    for (int m = 0; m < n_motifs; ++m)
        if (!motifs[m] || !d_weights[m] || !d_records[m]) return gfail(GFM_ERR_INVALID, "NULL motif / device buffer");
    MotifSet ms;
    if (const int rc = view_motif_set(motifs, n_motifs, ScoreBits::PackedTable, ms)) return rc;
    const int W = ms.W;
    // the capacity of a sum: a side has at most W + 63 windows, each once per strand
    if ((unsigned __int128)max_weight * 2u * (unsigned)(W + GFM_QUERY_MAX_ALLELE) > (unsigned __int128)UINT64_MAX)
        return gfail(GFM_ERR_INVALID, "gfm_graph_query_edits: a side holds up to " + std::to_string(2 * (W + GFM_QUERY_MAX_ALLELE)) +
                                      " windows: with weights up to " + std::to_string((unsigned long long)max_weight) +
                                      " a sum may pass 2^64 - 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    GX_TRY(hipMemsetAsync(d_status, 0, sizeof(int32_t), st));
    QvInput in;
    in.n_seqs = n_seqs;
    in.n_edits = n_edits;
    in.n_items = n_items;
    in.seq_off = reinterpret_cast<const long long *>(d_seq_offsets);
    in.bases = d_bases;
    in.coord = d_coord;
    in.pos0 = reinterpret_cast<const long long *>(d_pos0);
    in.ref_off = d_ref_off;
    in.alt_off = d_alt_off;
    in.ref_bytes = d_ref_bytes;
    in.alt_bytes = d_alt_bytes;
    in.item_seq = d_item_seq;
    in.item_edit = d_item_edit;
    const unsigned blocks = (unsigned)std::min<long long>((n_items + kQvWaves - 1) / kQvWaves, 1 << 15);
    const int fwd = (flags & GFM_GRAPH_FORWARD_ONLY) ? 1 : 0;
    for (int m0 = 0; m0 < n_motifs; m0 += kSeqMotifs) {
        const int mm = std::min(kSeqMotifs, n_motifs - m0);
        QvRecords recs = {};
        for (int k = 0; k < mm; ++k) recs.rec[k] = d_records[m0 + k];
        hipLaunchKernelGGL(query_edits_kernel, dim3(blocks, (unsigned)mm), dim3(kQvThreads), 0, st, in,
                           seq_motifs(ms, d_weights, m0, mm), recs, W, fwd, d_status);
        GX_TRY(hipGetLastError());
    }
    int32_t verdict = 0;
    GX_TRY(hipMemcpyAsync(&verdict, d_status, sizeof verdict, hipMemcpyDeviceToHost, st));
    GX_TRY(hipStreamSynchronize(st));
    if (verdict & kQvBadItem)
        return gfail(GFM_ERR_INVALID, "gfm_graph_query_edits: an item index is out of range: sequences 0 .. n_seqs - 1, edits 0 .. "
                                      "n_edits - 1");
    if (verdict & kQvBadEdit)
        return gfail(GFM_ERR_INVALID, "gfm_graph_query_edits: an edit's REF or ALT is longer than " +
                                      std::to_string(GFM_QUERY_MAX_ALLELE) + " bases, both are empty, or its offsets descend");
    if (verdict & kQvBadSeq) return gfail(GFM_ERR_INVALID, "gfm_graph_query_edits: d_seq_offsets descends or a sequence holds 2^31 bases");
    return GFM_OK;
}
