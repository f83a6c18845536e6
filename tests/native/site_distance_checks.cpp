// site_distance_checks.cpp -- the argument checks of gfm_sequence_site_distance under ASan/UBSan, without a GPU: every call
// below returns before anything is launched, and none needs a device.  The program IS graph_extract.hip (included as this
// translation unit's text, so that the entry's helpers in its anonymous namespace can be called too) with a main of its own,
// built and run exactly as deletion_scan_checks.cpp's header comment describes, with this file's name in place of that one's:
//
//   c=grafimo_amd/csrc; bash $c/build.sh    # the other objects
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -Iinclude -I$c \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined \
//         -x hip -c tests/native/site_distance_checks.cpp -o /tmp/site_distance_checks.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/site_distance_checks /tmp/site_distance_checks.o \
//         $c/grafimo_hip.o $c/score_quad_g*_m*.o $c/stream_calib.o $c/region_reduce.o $c/hit_pairs.o $c/hit_linkage.o \
//         $c/tsv_ingest.o $c/vcf_ingest.o $c/scan_stream.o $c/gfm_workers.o $c/graph_tsv_writer.o $c/hit_table.o \
//         $c/variant_table.o -lpthread -lz
//   /tmp/site_distance_checks               # prints "site_distance_checks: N checks passed", exit status 0
//
// Only the host half is instrumented (-Xarch_host); nothing here runs on a device or is loaded into an interpreter.
#include "graph_extract.hip"

#include <cstdio>
#include <cstring>

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

bool refused_with(int rc, const char *text) { return rc == GFM_ERR_INVALID && std::strstr(gfm_last_error(), text) != nullptr; }

// the entry with nothing but the arguments the host checks read
int scan(int32_t n_motifs, int32_t n_seqs, const int64_t *off, const int32_t *cutoffs, int32_t max_edits, uint32_t flags = 0)
{
    return gfm_sequence_site_distance(nullptr, n_motifs, n_seqs, off, nullptr, cutoffs, max_edits, flags, nullptr, nullptr, nullptr,
                                      nullptr);
}

}  // namespace

int main()
{
    const std::vector<int32_t> zero = {0}, three = {0, 1001, 64001};
    // ---- counts and flags
    expect(scan(1, 0, nullptr, zero.data(), 3) == GFM_OK, "no sequence is a no-op");
    expect(refused_with(scan(0, 0, nullptr, zero.data(), 3), "n_motifs < 1"), "no motif");
    expect(refused_with(scan(-4, 0, nullptr, zero.data(), 3), "n_motifs < 1"), "a negative number of motifs");
    expect(refused_with(scan(1, -1, nullptr, zero.data(), 3), "n_seqs < 0"), "a negative number of sequences");
    expect(refused_with(scan(1, 0, nullptr, zero.data(), 3, 2u), "unknown flag"), "an unknown flag");
    expect(refused_with(scan(1, 0, nullptr, zero.data(), 3, 0x80000000u), "unknown flag"), "the top flag bit");
    expect(scan(1, 0, nullptr, zero.data(), 3, GFM_GRAPH_FORWARD_ONLY) == GFM_OK, "forward only, no sequence");
    // ---- the cap: 1 .. 8, checked with no sequence too
    for (const int bad : {0, 9, -1, 16, INT32_MAX, INT32_MIN}) {
        const std::string text = "max_edits " + std::to_string(bad) + " is outside 1 .. 8";
        expect(refused_with(scan(1, 0, nullptr, zero.data(), bad), text.c_str()), "a cap outside 1 .. 8");
        expect(!sitedist_edits_ok(bad), "the cap's predicate");
    }
    for (int good = 1; good <= GFM_SITEDIST_MAX_EDITS; ++good) {
        expect(scan(1, 0, nullptr, zero.data(), good) == GFM_OK, "a good cap, no sequence");
        expect(sitedist_edits_ok(good), "the cap's predicate");
    }
    // ---- the cutoffs: exactly n_motifs of them are read (a heap array of that size: ASan sees a read past it); without the
    // motifs' width, what no width allows is refused
    expect(refused_with(scan(1, 0, nullptr, nullptr, 3), "NULL cutoffs"), "cutoffs NULL");
    expect(scan(3, 0, nullptr, three.data(), 3) == GFM_OK, "three good cutoffs, no sequence");
    for (const int bad : {-1, 64002, INT32_MAX, INT32_MIN}) {
        std::vector<int32_t> c = {5, bad};
        const std::string text = "cutoff " + std::to_string(bad) + " of motif 1";
        expect(refused_with(scan(2, 0, nullptr, c.data(), 3), text.c_str()), "a cutoff no width allows");
        c = {bad};
        expect(refused_with(scan(1, 0, nullptr, c.data(), 3), "of motif 0"), "a single cutoff no width allows");
    }
    // the predicate the entry applies once it knows W: 0 .. 1000 W + 1
    expect(sitedist_cutoff_ok(0, 1) && sitedist_cutoff_ok(1001, 1) && !sitedist_cutoff_ok(1002, 1) && !sitedist_cutoff_ok(-1, 1), "W = 1");
    expect(sitedist_cutoff_ok(19001, 19) && !sitedist_cutoff_ok(19002, 19), "W = 19");
    expect(sitedist_cutoff_ok(64001, 64) && !sitedist_cutoff_ok(64002, 64) && !sitedist_cutoff_ok(INT64_MAX, 64) &&
           !sitedist_cutoff_ok(INT64_MIN, 64), "W = 64");
    // ---- the offsets: n_seqs + 1 of them are read, no more
    expect(refused_with(scan(1, 2, nullptr, zero.data(), 3), "NULL"), "offsets NULL");
    {
        std::vector<int64_t> off = {0, 5, 3};
        expect(refused_with(scan(1, 2, off.data(), zero.data(), 3), "descends at sequence 1"), "offsets that descend");
        off = {-1, 5, 6};
        expect(refused_with(scan(1, 2, off.data(), zero.data(), 3), "below 0"), "offsets that start below 0");
        off = {0, (int64_t)1 << 31};
        expect(refused_with(scan(1, 1, off.data(), zero.data(), 3), "2^31"), "a sequence of 2^31 bases");
        off = {0, 0, 0, 0};
        expect(scan(1, 3, off.data(), zero.data(), 3) == GFM_OK, "empty sequences only");
        off = {7, 7};
        expect(scan(1, 1, off.data(), zero.data(), 8) == GFM_OK, "one empty sequence at 7");
        off = {0, 0, 130};                                       // three tiles, then the buffers are looked at
        expect(refused_with(scan(1, 2, off.data(), zero.data(), 3), "NULL"), "bases without buffers");
        // the cap and the cutoffs come before the sequences
        off = {0, 5, 3};
        expect(refused_with(scan(1, 2, off.data(), zero.data(), 0), "max_edits"), "a bad cap with bad offsets");
        const std::vector<int32_t> neg = {-1};
        expect(refused_with(scan(1, 2, off.data(), neg.data(), 3), "cutoff -1"), "a bad cutoff with bad offsets");
    }
    // ---- the buffers: each of them NULL in turn, then a misaligned mask array (all before a motif handle is read)
    {
        const int64_t off[] = {0, 10};
        alignas(16) static unsigned char buf[64];
        const gfm_motif_t motif = reinterpret_cast<gfm_motif_t>(buf);           // (never read: the checks below come first)
        uint32_t *w = reinterpret_cast<uint32_t *>(buf);
        uint64_t *k = reinterpret_cast<uint64_t *>(buf);
        int32_t *st = reinterpret_cast<int32_t *>(buf);
        for (int hole = 0; hole < 8; ++hole) {
            const gfm_motif_t m0 = nullptr;
            uint32_t *w0 = nullptr;
            uint64_t *k0 = nullptr;
            const gfm_motif_t *pm = hole == 0 ? nullptr : hole == 5 ? &m0 : &motif;
            uint32_t *const *pw = hole == 1 ? nullptr : hole == 6 ? &w0 : &w;
            uint64_t *const *pk = hole == 2 ? nullptr : hole == 7 ? &k0 : &k;
            const int rc = gfm_sequence_site_distance(pm, 1, 1, off, hole == 3 ? nullptr : buf, zero.data(), 3, 0, pw, pk,
                                                      hole == 4 ? nullptr : st, nullptr);
            expect(refused_with(rc, "NULL"), "a NULL buffer");
        }
        uint64_t *k4 = reinterpret_cast<uint64_t *>(buf + 4);
        expect(refused_with(gfm_sequence_site_distance(&motif, 1, 1, off, buf, zero.data(), 3, 0, &w, &k4, st, nullptr), "aligned"),
               "masks at 4 mod 8");
        // with no base a NULL handle among the motifs is still refused: the motifs are looked at whenever they are given
        const gfm_motif_t m0 = nullptr;
        const int64_t none[] = {0, 0};
        expect(refused_with(gfm_sequence_site_distance(&m0, 1, 1, none, nullptr, zero.data(), 3, 0, nullptr, nullptr, nullptr, nullptr),
                            "NULL motif"), "a NULL handle with no base");
    }
    // ---- the kernel's fixed sizes
    expect(kSdTile == 64 && kSdThreads == 64 && kSdCodes == 128 && kSdTile + GFM_MAX_WIDTH - 1 <= kSdCodes, "the codes of a tile and its halo");
    expect(sizeof(unsigned) * GFM_MAX_WIDTH * 8 + sizeof(uint2) * GFM_MAX_WIDTH + kSdCodes == 2688u, "the LDS of a workgroup");
    expect(((64000u << 4) | 9u) < kSdNone && GFM_SITEDIST_MAX_EDITS + 1 <= 15, "a word never reads as no window");
    std::printf("site_distance_checks: %d checks passed, %d failed\n", g_checks - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
