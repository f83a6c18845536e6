// variant_table.cpp -- the per-variant effect table from the records of gfm_graph_variant_effects, on the host.
// Part of libgrafimo_hip.so (C ABI in include/grafimo_hip.h: gfm_variant_effect_columns).
//
// The kernels leave, per (site, allele) slot, every walk and strand whose packed key -- score, start, stop, strand -- equals
// the slot's best; those are walks over the same coordinates, and the order's last criterion, the k-mer as printed for its
// strand, is decided here.  Then one row per (site, ALT allele): the REF side (slot allele 0) beside the ALT side.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "grafimo_hip.h"

#define GFM_API extern "C" __attribute__((visibility("default")))

extern "C" void gfm_set_error_(const char *msg);   // thread-local slot of grafimo_hip.hip

namespace {

int vfail(int code, const std::string &msg)
{
    gfm_set_error_(msg.c_str());
    return code;
}

// a comes first under the table's order: score desc, start asc, stop asc, '+' before '-', k-mer asc
bool better(const gfm_variant_rec_t &a, const gfm_variant_rec_t &b, int W)
{
    if (a.score != b.score) return a.score > b.score;
    if (a.start != b.start) return a.start < b.start;
    if (a.stop != b.stop) return a.stop < b.stop;
    if (a.strand != b.strand) return a.strand == '+';
    return std::memcmp(a.kmer, b.kmer, (size_t)W) < 0;
}

}  // namespace

GFM_API int gfm_variant_effect_columns(const double *h_ptable, int32_t table_len, int32_t scale, double offset, int32_t width,
                                       int32_t n_sites, const uint8_t *h_n_alts, const gfm_variant_rec_t *h_recs, int64_t n_recs,
                                       double threshold, uint32_t flags, int64_t *n_out, int32_t *o_site, int32_t *o_alt,
                                       uint8_t *o_found, double *o_score, double *o_pvalue, int64_t *o_start, int64_t *o_stop,
                                       uint8_t *o_strand, uint8_t *o_kmers, uint8_t *o_effect)
{
    if (!h_ptable || table_len < 1 || scale <= 0 || width < 1 || width > GFM_MAX_WIDTH || n_sites < 0 || n_recs < 0 || !n_out)
        return vfail(GFM_ERR_INVALID, "bad argument");
    if ((n_sites && !h_n_alts) || (n_recs && !h_recs)) return vfail(GFM_ERR_INVALID, "NULL input array");
    if (!o_site || !o_alt || !o_found || !o_score || !o_pvalue || !o_start || !o_stop || !o_strand || !o_kmers || !o_effect)
        return vfail(GFM_ERR_INVALID, "NULL output array");
    if (flags & ~(uint32_t)GFM_VARIANT_ALL_SITES) return vfail(GFM_ERR_INVALID, "unknown flag");
    for (int32_t i = 0; i < n_sites; ++i)
        if (h_n_alts[i] < 1 || h_n_alts[i] > 3) return vfail(GFM_ERR_INVALID, "a site with no or more than 3 ALT alleles");
    const size_t n_slots = (size_t)n_sites * 4;
    std::vector<int64_t> best(n_slots, -1);
    for (int64_t r = 0; r < n_recs; ++r) {
        const gfm_variant_rec_t &x = h_recs[r];
        if (x.slot < 0 || (size_t)x.slot >= n_slots || (x.slot & 3) > h_n_alts[x.slot >> 2])
            return vfail(GFM_ERR_INVALID, "a record of a slot the graph does not have");
        if (x.score < 0 || x.score >= table_len || (x.strand != '+' && x.strand != '-'))
            return vfail(GFM_ERR_INVALID, "a record with a score outside the tail table or no strand");
        int64_t &b = best[(size_t)x.slot];
        if (b < 0 || better(x, h_recs[b], width)) b = r;
    }
    const bool all_sites = (flags & GFM_VARIANT_ALL_SITES) != 0;
    const double nan = std::nan("");
    int64_t out = 0;
    for (int32_t s = 0; s < n_sites; ++s) {
        const int64_t ref_b = best[(size_t)s * 4];
        for (int a = 1; a <= h_n_alts[s]; ++a) {
            const int64_t alt_b = best[(size_t)s * 4 + (size_t)a];
            if (ref_b < 0 && alt_b < 0) continue;       // no region covers the site (or no haplotype carries either side)
            const int64_t side[2] = {ref_b, alt_b};
            bool pass[2] = {false, false};
            for (int k = 0; k < 2; ++k)
                if (side[k] >= 0) pass[k] = h_ptable[h_recs[side[k]].score] < threshold;
            if (!all_sites && !pass[0] && !pass[1]) continue;
            o_site[out] = s;
            o_alt[out] = a;
            o_effect[out] = (uint8_t)((pass[1] ? 1 : 0) | (pass[0] ? 2 : 0));
            for (int k = 0; k < 2; ++k) {
                const size_t o = (size_t)out * 2 + (size_t)k;
                uint8_t *km = o_kmers + o * (size_t)(width + 1);
                if (side[k] < 0) {
                    o_found[o] = 0;
                    o_score[o] = o_pvalue[o] = nan;
                    o_start[o] = o_stop[o] = 0;
                    o_strand[o] = 0;
                    std::memset(km, 0, (size_t)width);
                } else {
                    const gfm_variant_rec_t &x = h_recs[side[k]];
                    o_found[o] = 1;
                    o_score[o] = ((double)x.score / (double)scale) + ((double)width * offset);
                    o_pvalue[o] = h_ptable[x.score];
                    o_start[o] = x.start;
                    o_stop[o] = x.stop;
                    o_strand[o] = x.strand == '-' ? 1 : 0;
                    std::memcpy(km, x.kmer, (size_t)width);
                }
                km[width] = '\n';
            }
            ++out;
        }
    }
    *n_out = out;
    return GFM_OK;
}
