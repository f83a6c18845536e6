// substitution_scan_checks.cpp -- the argument checks of gfm_sequence_substitution_scan under ASan/UBSan, without a GPU: every
// call below returns before anything is launched, and none needs a device.  The program IS graph_extract.hip (included as this
// translation unit's text, so that the entry's helpers in its anonymous namespace can be called too) with a main of its own,
// built and run exactly as deletion_scan_checks.cpp's header comment describes, with this file's name in place of that one's:
//
//   c=grafimo_amd/csrc; bash $c/build.sh    # the other objects
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -Iinclude -I$c \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined \
//         -x hip -c tests/native/substitution_scan_checks.cpp -o /tmp/substitution_scan_checks.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/substitution_scan_checks /tmp/substitution_scan_checks.o \
//         $c/grafimo_hip.o $c/score_quad_g*_m*.o $c/stream_calib.o $c/region_reduce.o $c/hit_pairs.o $c/hit_linkage.o \
//         $c/tsv_ingest.o $c/vcf_ingest.o $c/scan_stream.o $c/gfm_workers.o $c/graph_tsv_writer.o $c/hit_table.o \
//         $c/variant_table.o -lpthread -lz
//   /tmp/substitution_scan_checks           # prints "substitution_scan_checks: N checks passed", exit status 0
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

const uint8_t kTransversion[4] = {1, 0, 3, 2};

// the entry with nothing but the arguments the host checks read
int scan(int32_t n_motifs, int32_t n_seqs, const int64_t *off, int32_t n_lengths, const int32_t *lengths, uint32_t flags = 0,
         const uint8_t *map = kTransversion)
{
    return gfm_sequence_substitution_scan(nullptr, n_motifs, nullptr, 1, n_seqs, off, nullptr, n_lengths, lengths, map, flags, nullptr,
                                          nullptr, nullptr, nullptr);
}

}  // namespace

int main()
{
    const int32_t one[] = {1}, all_ok[] = {1, 2, 7, 64};
    std::vector<int32_t> every(64);
    for (int i = 0; i < 64; ++i) every[(size_t)i] = i + 1;
    // ---- counts and flags
    expect(scan(0, 0, nullptr, 1, one) == GFM_ERR_INVALID, "no motif");
    expect(scan(1, -1, nullptr, 1, one) == GFM_ERR_INVALID, "a negative number of sequences");
    expect(scan(1, 0, nullptr, 0, one) == GFM_ERR_INVALID, "no length");
    expect(refused_with(scan(1, 0, nullptr, 1, one, 2u), "unknown flag"), "an unknown flag");
    // ---- the lengths: read exactly n_lengths of them (a heap array of that size: ASan sees a read past it)
    expect(refused_with(scan(1, 0, nullptr, 1, nullptr), "NULL"), "lengths NULL");
    expect(scan(1, 0, nullptr, 4, all_ok) == GFM_OK, "good lengths, no sequence");
    expect(scan(1, 0, nullptr, 64, every.data()) == GFM_OK, "all 64 lengths");
    for (const int bad : {0, -1, 65, INT32_MAX, INT32_MIN}) {
        std::vector<int32_t> l = {1, bad};
        expect(refused_with(scan(1, 0, nullptr, 2, l.data()), "outside 1 .. 64"), "a length outside 1 .. 64");
        l = {bad};
        expect(refused_with(scan(1, 0, nullptr, 1, l.data()), "outside 1 .. 64"), "a single length outside 1 .. 64");
    }
    {
        std::vector<int32_t> l = {3, 3};
        expect(refused_with(scan(1, 0, nullptr, 2, l.data()), "strictly ascend"), "equal lengths");
        l = {1, 5, 4};
        expect(refused_with(scan(1, 0, nullptr, 3, l.data()), "strictly ascend at 2"), "lengths that descend");
        l = {64, 1};
        expect(refused_with(scan(1, 0, nullptr, 2, l.data()), "strictly ascend"), "64 before 1");
    }
    // ---- the map: exactly four codes are read (a heap array of that size), each in 0 .. 3; checked with no sequence too
    expect(refused_with(scan(1, 0, nullptr, 1, one, 0u, nullptr), "NULL base_map"), "map NULL");
    for (int k = 0; k < 4; ++k)
        for (const int bad : {4, 5, 128, 255}) {
            std::vector<uint8_t> m = {0, 1, 2, 3};
            m[(size_t)k] = (uint8_t)bad;
            const std::string text = "base_map[" + std::to_string(k) + "] = " + std::to_string(bad) + " is outside 0 .. 3";
            expect(refused_with(scan(1, 0, nullptr, 1, one, 0u, m.data()), text.c_str()), "a map code above 3");
        }
    for (int a = 0; a < 4; ++a) {
        std::vector<uint8_t> m = {(uint8_t)a, (uint8_t)((a + 1) & 3), (uint8_t)a, 3};      // constant parts, fixed points
        expect(scan(1, 0, nullptr, 4, all_ok, 0u, m.data()) == GFM_OK, "a good map, no sequence");
    }
    {
        const int64_t off[] = {0, 10};                           // a bad map is refused before the buffers are looked at
        const uint8_t m[4] = {0, 1, 2, 4};
        expect(refused_with(scan(1, 1, off, 1, one, 0u, m), "base_map[3] = 4"), "a map code of 4 with a sequence");
        expect(refused_with(scan(1, 1, off, 1, one, 0u, nullptr), "NULL base_map"), "map NULL with a sequence");
    }
    // ---- the map as the kernel takes it: byte c the image of code c, A 0, C 1, T 2, G 3
    {
        const uint8_t identity[4] = {0, 1, 2, 3}, poly_a[4] = {0, 0, 0, 0}, complement[4] = {3, 2, 1, 0};
        expect(subscan_pack_map(identity) == 0x03020100u, "the identity");
        expect(subscan_pack_map(poly_a) == 0u, "poly-A");
        expect(subscan_pack_map(complement) == 0x01000302u, "the complement: A>T, C>G, T>A, G>C");
        expect(subscan_pack_map(kTransversion) == 0x02030001u, "the transversion: A>C, C>A, T>G, G>T");
    }
    // ---- the offsets: n_seqs + 1 of them are read, no more
    expect(refused_with(scan(1, 2, nullptr, 1, one), "NULL"), "offsets NULL");
    {
        std::vector<int64_t> off = {0, 5, 3};
        expect(refused_with(scan(1, 2, off.data(), 1, one), "descends at sequence 1"), "offsets that descend");
        off = {-1, 5, 6};
        expect(refused_with(scan(1, 2, off.data(), 1, one), "below 0"), "offsets that start below 0");
        off = {0, (int64_t)1 << 31};
        expect(refused_with(scan(1, 1, off.data(), 1, one), "2^31"), "a sequence of 2^31 bases");
        off = {0, 0, 0, 0};
        expect(scan(1, 3, off.data(), 4, all_ok) == GFM_OK, "empty sequences only");
        off = {7, 7};
        expect(scan(1, 1, off.data(), 1, one) == GFM_OK, "one empty sequence at 7");
        off = {0, 0, 130};                                       // three tiles, then the buffers are looked at
        expect(refused_with(scan(1, 2, off.data(), 4, all_ok), "NULL"), "bases without buffers");
    }
    // ---- the buffers: each of them NULL in turn, then misaligned results (all before a motif handle is read)
    {
        const int64_t off[] = {0, 10};
        alignas(16) static unsigned char buf[64];
        const gfm_motif_t motif = reinterpret_cast<gfm_motif_t>(buf);           // (never read: the checks below come first)
        const uint64_t *w = reinterpret_cast<const uint64_t *>(buf);
        uint32_t *k = reinterpret_cast<uint32_t *>(buf);
        uint64_t *s = reinterpret_cast<uint64_t *>(buf);
        int32_t *st = reinterpret_cast<int32_t *>(buf);
        const uint8_t *mp = kTransversion;
        for (int hole = 0; hole < 9; ++hole) {
            const gfm_motif_t *pm = hole == 0 ? nullptr : &motif;
            const gfm_motif_t m0 = nullptr;
            const uint64_t *w0 = nullptr, *const *pw = hole == 1 ? nullptr : hole == 6 ? &w0 : &w;
            uint32_t *k0 = nullptr, *const *pk = hole == 2 ? nullptr : hole == 7 ? &k0 : &k;
            uint64_t *s0 = nullptr, *const *ps = hole == 3 ? nullptr : hole == 8 ? &s0 : &s;
            const int rc = gfm_sequence_substitution_scan(hole == 5 ? &m0 : pm, 1, pw, 1, 1, off, hole == 4 ? nullptr : buf, 1, one, mp, 0,
                                                          pk, ps, st, nullptr);
            expect(refused_with(rc, "NULL"), "a NULL buffer");
        }
        expect(refused_with(gfm_sequence_substitution_scan(&motif, 1, &w, 1, 1, off, buf, 1, one, mp, 0, &k, &s, nullptr, nullptr), "NULL"),
               "status NULL");
        uint32_t *k4 = reinterpret_cast<uint32_t *>(buf + 4);
        uint64_t *s8 = reinterpret_cast<uint64_t *>(buf + 8);
        expect(refused_with(gfm_sequence_substitution_scan(&motif, 1, &w, 1, 1, off, buf, 1, one, mp, 0, &k4, &s, st, nullptr), "aligned"),
               "keys at 4 mod 8");
        expect(refused_with(gfm_sequence_substitution_scan(&motif, 1, &w, 1, 1, off, buf, 1, one, mp, 0, &k, &s8, st, nullptr), "aligned"),
               "sums at 8 mod 16");
    }
    // ---- the capacity rule (the deletion scan's predicate: either side has at most W + Lmax - 1 windows) and the LDS
    expect(delscan_side_windows(64, 64) == 254u && delscan_side_windows(1, 1) == 2u && delscan_side_windows(5, 4) == 16u, "windows a side");
    expect(delscan_sum_fits(UINT64_MAX / 2u, 1, 1) && !delscan_sum_fits(UINT64_MAX / 2u + 1u, 1, 1), "the bound at W = 1, L = 1");
    expect(delscan_sum_fits(((uint64_t)1 << 60) - 1u, 5, 4) && !delscan_sum_fits((uint64_t)1 << 60, 5, 4), "the bound at W = 5, L = 4");
    expect(delscan_sum_fits(UINT64_MAX / 254u, 64, 64) && !delscan_sum_fits(UINT64_MAX / 254u + 1u, 64, 64), "the bound at W = L = 64");
    expect(subscan_lds_bytes(64, 64) == 4u * 128u * 65u && subscan_lds_bytes(1, 1) == 4u * 65u, "the difference table's bytes");
    expect(subscan_lds_bytes(19, 20) == 4u * 84u * 19u && subscan_lds_bytes(64, 64) == delscan_lds_bytes(64, 64),
           "one table, as the deletion scan's");
    expect(kSsStaticLds == 8896u && kSsStaticLds + subscan_lds_bytes(19, 20) == 15280u && kSsStaticLds + subscan_lds_bytes(64, 64) == 42176u,
           "the LDS of a workgroup");
    expect(kSsStaticLds + subscan_lds_bytes(GFM_MAX_WIDTH, GFM_SUBSCAN_MAX_LENGTH) <= 64u * 1024u, "under 64 KB without a launch attribute");
    std::printf("substitution_scan_checks: %d checks passed, %d failed\n", g_checks - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
