// scan_fold_checks.cpp -- the argument checks of gfm_scan_fold under ASan/UBSan, without a GPU: every call below returns before
// anything is launched, and none needs a device.  The program IS graph_extract.hip (included as this translation unit's text)
// with a main of its own:
//
//   c=grafimo_amd/csrc; bash $c/build.sh    # the other objects
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -Iinclude -I$c \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined \
//         -x hip -c tests/native/scan_fold_checks.cpp -o /tmp/scan_fold_checks.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/scan_fold_checks /tmp/scan_fold_checks.o \
//         $c/grafimo_hip.o $c/score_quad_g*_m*.o $c/stream_calib.o $c/region_reduce.o $c/hit_pairs.o $c/hit_linkage.o \
//         $c/tsv_ingest.o $c/vcf_ingest.o $c/scan_stream.o $c/gfm_workers.o $c/graph_tsv_writer.o $c/hit_table.o \
//         $c/variant_table.o -lpthread -lz
//   /tmp/scan_fold_checks                   # prints "scan_fold_checks: N checks passed, 0 failed", exit status 0
//
// Only the host half is instrumented (-Xarch_host); nothing here runs on a device or is loaded into an interpreter.  The host
// arrays are heap arrays of exactly the stated sizes, so that ASan sees a read past any of them.
#include "graph_extract.hip"

#include <cstdio>
#include <cstring>
#include <memory>

namespace {

int g_checks = 0, g_failed = 0;

void expect(bool ok, const char *what)
{
    ++g_checks;
    if (!ok) {
        ++g_failed;
        std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, gfm_last_error());
    }
}

bool refused_with(int rc, const char *text)
{
    return rc == GFM_ERR_INVALID && std::strstr(gfm_last_error(), "gfm_scan_fold") && std::strstr(gfm_last_error(), text) != nullptr;
}

template <class T>
std::unique_ptr<T[]> heap(const std::vector<T> &v)
{
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

// A call the checks accept up to the fault it is given: M motifs, the `device` buffers one static block that is never read.
struct Call {
    std::vector<int32_t> ids, cutoffs, lens, pairs;
    int64_t rows = 4;
    int32_t columns = 5;
    alignas(16) static unsigned char buf[64];
    std::vector<const double *> tabs;
    std::vector<const uint32_t *> keys;
    std::vector<const uint64_t *> sums;
    void *state[6];
    explicit Call(int M = 2) : ids((size_t)M), cutoffs((size_t)M, 3), lens((size_t)M, 9), pairs{0, 1, 0, 2, 0, 3, 0, 4}
    {
        for (int m = 0; m < M; ++m) ids[(size_t)m] = 2 * (M - m);
        tabs.assign((size_t)M, reinterpret_cast<const double *>(buf));
        keys.assign((size_t)M, reinterpret_cast<const uint32_t *>(buf));
        sums.assign((size_t)M, reinterpret_cast<const uint64_t *>(buf));
        for (void *&p : state) p = buf;
    }
    int run() const
    {
        const auto i = heap(ids), c = heap(cutoffs), l = heap(lens), p = heap(pairs);
        const auto t = heap(tabs);
        const auto k = heap(keys);
        const auto s = heap(sums);
        return gfm_scan_fold((int32_t)ids.size(), i.get(), c.get(), t.get(), l.get(), rows, columns, (int32_t)(pairs.size() / 2), p.get(),
                             k.get(), s.get(), static_cast<uint32_t *>(state[0]), static_cast<uint32_t *>(state[1]),
                             static_cast<uint32_t *>(state[2]), static_cast<double *>(state[3]), static_cast<uint32_t *>(state[4]),
                             static_cast<uint64_t *>(state[5]), nullptr);
    }
};
alignas(16) unsigned char Call::buf[64];

int bare(int32_t n_motifs, int64_t rows, int32_t columns, int32_t n_pairs)
{
    return gfm_scan_fold(n_motifs, nullptr, nullptr, nullptr, nullptr, rows, columns, n_pairs, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr, nullptr);
}

}  // namespace

int main()
{
    // ---- the counts, with no row too; no row is a no-op that reads nothing
    expect(bare(1, 0, 5, 4) == GFM_OK && bare(40, 0, 2, 1) == GFM_OK && bare(1, 0, 8, 8) == GFM_OK, "no row, NULL everywhere");
    expect(refused_with(bare(0, 0, 5, 4), "n_motifs < 1") && refused_with(bare(-3, 4, 5, 4), "n_motifs < 1"), "no motif");
    expect(refused_with(bare(1, -1, 5, 4), "n_rows") && refused_with(bare(1, ((int64_t)1 << 40) + 1, 5, 4), "n_rows"), "rows out of range");
    expect(refused_with(bare(1, 0, 1, 1), "n_columns 1") && refused_with(bare(1, 0, 9, 1), "n_columns 9"), "columns out of range");
    expect(refused_with(bare(1, 0, 5, 0), "n_pairs 0") && refused_with(bare(1, 0, 5, 9), "n_pairs 9"), "pairs out of range");
    expect(refused_with(bare(1, 4, 5, 4), "NULL argument"), "rows and NULL everywhere");
    // ---- the pairs: exactly 2 n_pairs numbers are read
    {
        Call c;
        c.pairs = {0, 1, 0, 5};
        expect(refused_with(c.run(), "pair 1 (0, 5)"), "a column beyond the last");
        c.pairs = {-1, 1};
        expect(refused_with(c.run(), "pair 0 (-1, 1)"), "a negative column");
        c.pairs = {0, 1, 2, 3, 2, 4, 2, 5, 6, 6};
        c.columns = 7;
        expect(refused_with(c.run(), "pair 4 (6, 6)"), "ref == alt");
        c.pairs = {0, 1, 2, 3, 2, 4, 2, 5, 2, 6, 1, 0, 3, 2, 6, 2};
        c.ids = {3, 3};                                          // (a later fault: no call here passes every check)
        expect(refused_with(c.run(), "motif id 3 is repeated"), "eight pairs of seven columns pass the pair check");
    }
    // ---- the ids: n_motifs of them are read
    {
        Call c(3);
        c.ids = {4, -2, 0};
        expect(refused_with(c.run(), "motif id -2 is negative"), "a negative id");
        c.ids = {4, 0, 4};
        expect(refused_with(c.run(), "motif id 4 is repeated"), "a repeated id");
        c.ids = {INT32_MAX, 0, 4};
        expect(refused_with(c.run(), "cannot be stored as id + 1"), "the largest id");
        c.ids = {INT32_MIN, INT32_MAX, 0};
        expect(refused_with(c.run(), "is negative"), "the smallest id");
    }
    // ---- the tables and cutoffs
    {
        Call c(3);
        c.lens = {9, 9, 0};
        c.cutoffs = {3, 3, 0};
        expect(refused_with(c.run(), "table_len 0 of motif 2"), "an empty table");
        c.lens = {9, -5, 9};
        expect(refused_with(c.run(), "table_len -5 of motif 1"), "a negative table length");
        c.lens = {9, 9, 9};
        c.cutoffs = {0, 9, 10};
        expect(refused_with(c.run(), "cutoff 10 of motif 2 is outside 0 .. 9"), "a cutoff beyond the table; 0 and table_len pass");
        c.cutoffs = {-1, 9, 9};
        expect(refused_with(c.run(), "cutoff -1 of motif 0 is outside 0 .. 9"), "a negative cutoff");
    }
    // ---- the buffers: each NULL in turn, then the 8-byte ones misaligned
    for (int hole = 0; hole < 9; ++hole) {
        Call c;
        if (hole < 6) c.state[hole] = nullptr;
        if (hole == 6) c.tabs[1] = nullptr;
        if (hole == 7) c.keys[1] = nullptr;
        if (hole == 8) c.sums[0] = nullptr;
        expect(refused_with(c.run(), "NULL"), "a NULL buffer");
    }
    {
        Call c;
        c.sums[1] = reinterpret_cast<const uint64_t *>(Call::buf + 4);
        expect(refused_with(c.run(), "8-byte aligned"), "sums at 4 mod 8");
        Call d;
        d.tabs[0] = reinterpret_cast<const double *>(Call::buf + 4);
        expect(refused_with(d.run(), "8-byte aligned"), "a tail table at 4 mod 8");
        Call e;
        e.state[3] = Call::buf + 12;
        expect(refused_with(e.run(), "site_p and aff_sums are 8-byte aligned"), "site_p at 4 mod 8");
        Call f;
        f.state[5] = Call::buf + 4;
        expect(refused_with(f.run(), "site_p and aff_sums are 8-byte aligned"), "aff_sums at 4 mod 8");
        Call g;
        g.keys[0] = reinterpret_cast<const uint32_t *>(Call::buf + 4);       // (keys are 4-byte words: this alone would pass)
        g.state[3] = Call::buf + 4;
        expect(refused_with(g.run(), "site_p and aff_sums"), "keys at 4 mod 8 are not what is refused");
    }
    std::printf("scan_fold_checks: %d checks passed, %d failed\n", g_checks - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
