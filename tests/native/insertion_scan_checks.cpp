// insertion_scan_checks.cpp -- the argument checks of gfm_sequence_insertion_scan under ASan/UBSan, without a GPU: every call
// below returns before anything is launched, and none needs a device.  The program IS graph_extract.hip (included as this
// translation unit's text, so that the entry's helpers in its anonymous namespace can be called too) with a main of its own:
//
//   c=grafimo_amd/csrc; bash $c/build.sh    # the other objects
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -Iinclude -I$c \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined \
//         -x hip -c tests/native/insertion_scan_checks.cpp -o /tmp/insertion_scan_checks.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/insertion_scan_checks /tmp/insertion_scan_checks.o \
//         $c/grafimo_hip.o $c/score_quad_g*_m*.o $c/stream_calib.o $c/region_reduce.o $c/hit_pairs.o $c/hit_linkage.o \
//         $c/tsv_ingest.o $c/vcf_ingest.o $c/scan_stream.o $c/gfm_workers.o $c/graph_tsv_writer.o $c/hit_table.o \
//         $c/variant_table.o -lpthread -lz
//   /tmp/insertion_scan_checks              # prints "insertion_scan_checks: N checks passed", exit status 0
//
// Only the host half is instrumented (-Xarch_host); nothing here runs on a device or is loaded into an interpreter.
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

bool refused_with(int rc, const char *text) { return rc == GFM_ERR_INVALID && std::strstr(gfm_last_error(), text) != nullptr; }

// The inserts of a call as heap arrays of exactly the stated sizes -- insert_offsets [count + 1] and insert_bases
// [offsets[count]] -- so that ASan sees a read past either.  `offsets` given: those instead of the inserts' own.
struct Inserts {
    int32_t count;
    std::unique_ptr<int32_t[]> offsets;
    std::unique_ptr<uint8_t[]> bases;
    explicit Inserts(const std::vector<std::string> &list, const std::vector<int32_t> &given = {})
        : count((int32_t)(given.empty() ? list.size() : given.size() - 1)), offsets(new int32_t[(size_t)count + 1])
    {
        std::string all;
        for (const std::string &s : list) all += s;
        bases.reset(new uint8_t[all.size()]);
        std::memcpy(bases.get(), all.data(), all.size());
        int32_t at = 0;
        for (int32_t i = 0; i <= count; ++i) {
            offsets[(size_t)i] = given.empty() ? at : given[(size_t)i];
            if (given.empty() && i < count) at += (int32_t)list[(size_t)i].size();
        }
    }
};

// the entry with nothing but the arguments the host checks read
int scan(int32_t n_motifs, int32_t n_seqs, const int64_t *off, const Inserts &ins, uint32_t flags = 0)
{
    return gfm_sequence_insertion_scan(nullptr, n_motifs, nullptr, 1, n_seqs, off, nullptr, ins.count, ins.offsets.get(), ins.bases.get(),
                                       flags, nullptr, nullptr, nullptr, nullptr);
}

}  // namespace

int main()
{
    const Inserts one({"A"}), four({"A", "c", "G", "t"}), mixed({"a", "CG", "GATTACA", std::string(64, 'T')});
    // ---- counts and flags
    expect(scan(0, 0, nullptr, one) == GFM_ERR_INVALID, "no motif");
    expect(scan(1, -1, nullptr, one) == GFM_ERR_INVALID, "a negative number of sequences");
    expect(refused_with(scan(1, 0, nullptr, one, 2u), "unknown flag"), "an unknown flag");
    expect(gfm_sequence_insertion_scan(nullptr, 1, nullptr, 1, 0, nullptr, nullptr, 0, one.offsets.get(), one.bases.get(), 0, nullptr,
                                       nullptr, nullptr, nullptr) == GFM_ERR_INVALID, "no insert");
    expect(gfm_sequence_insertion_scan(nullptr, 1, nullptr, 1, 0, nullptr, nullptr, -1, one.offsets.get(), one.bases.get(), 0, nullptr,
                                       nullptr, nullptr, nullptr) == GFM_ERR_INVALID, "a negative number of inserts");
    {
        const Inserts sixteen(std::vector<std::string>(16, std::string(64, 'g'))), seventeen(std::vector<std::string>(17, "A"));
        expect(scan(1, 0, nullptr, sixteen) == GFM_OK, "16 inserts of 64 bases, no sequence");
        expect(refused_with(scan(1, 0, nullptr, seventeen), "bad argument"), "17 inserts");
        expect(refused_with(scan(1, 0, nullptr, seventeen, 2u), "bad argument"), "17 inserts come before the flag");
    }
    // ---- the inserts: exactly insert_offsets[0 .. n] and insert_bases[0 .. insert_offsets[n] - 1] are read
    expect(refused_with(gfm_sequence_insertion_scan(nullptr, 1, nullptr, 1, 0, nullptr, nullptr, 1, nullptr, one.bases.get(), 0, nullptr,
                                                    nullptr, nullptr, nullptr), "NULL"), "insert_offsets NULL");
    expect(refused_with(gfm_sequence_insertion_scan(nullptr, 1, nullptr, 1, 0, nullptr, nullptr, 1, one.offsets.get(), nullptr, 0, nullptr,
                                                    nullptr, nullptr, nullptr), "NULL"), "insert_bases NULL");
    expect(scan(1, 0, nullptr, one) == GFM_OK, "one base, no sequence");
    expect(scan(1, 0, nullptr, four) == GFM_OK, "A c G t, no sequence");
    expect(scan(1, 0, nullptr, mixed) == GFM_OK, "lengths 1, 2, 7, 64, no sequence");
    expect(refused_with(scan(1, 0, nullptr, Inserts({"AC"}, {1, 2})), "insert_offsets starts at 0"), "offsets that start at 1");
    expect(refused_with(scan(1, 0, nullptr, Inserts({"ACG"}, {0, 3, 1})), "insert_offsets descends at insert 1"), "offsets that descend");
    expect(refused_with(scan(1, 0, nullptr, Inserts({"ACG"}, {0, -1, 3})), "insert_offsets descends at insert 0"), "an offset below 0");
    expect(refused_with(scan(1, 0, nullptr, Inserts({"ACG"}, {0, 3, INT32_MIN})), "descends at insert 1"), "the smallest offset");
    expect(refused_with(scan(1, 0, nullptr, Inserts({"AC", "", "G"})), "length 0 of insert 1 is outside 1 .. 64"), "an empty insert");
    expect(refused_with(scan(1, 0, nullptr, Inserts({"A", std::string(65, 'A')})), "length 65 of insert 1 is outside 1 .. 64"),
           "an insert of 65 bases");
    expect(refused_with(scan(1, 0, nullptr, Inserts({}, {0, INT32_MAX})), "outside 1 .. 64"), "the largest length: no base is read");
    expect(refused_with(scan(1, 0, nullptr, Inserts({"NNN"}, {0, 3, 2})), "descends"), "the offsets are checked before the letters");
    expect(refused_with(scan(1, 0, nullptr, Inserts({std::string(65, 'N')})), "outside 1 .. 64"), "the lengths are checked before the letters");
    for (const char *bad : {"N", "n", "U", "-", " ", "@", "B", "[", "\x01"}) {
        expect(refused_with(scan(1, 0, nullptr, Inserts({"AC", std::string("G") + bad})), "base 1 of insert 1 is not one of ACGTacgt"),
               "a letter outside ACGTacgt");
    }
    expect(refused_with(scan(1, 0, nullptr, Inserts({std::string(63, 'c') + '\0'})), "base 63 of insert 0"), "a zero byte as the last base");
    expect(refused_with(scan(1, 0, nullptr, Inserts({std::string(1, (char)0xC1)})), "base 0 of insert 0"), "a byte above 127");
    // ---- the packed list
    {
        const Inserts two({"acGT", std::string(33, 'G') + std::string(31, 'T')});
        InsertList list;
        int lmax = 0, total = 0;
        expect(insert_list("t", 2, two.offsets.get(), two.bases.get(), list, lmax, total) == GFM_OK && list.n == 2 && lmax == 64 &&
                   total == 68 && list.len[0] == 4 && list.len[1] == 64,
               "the list's counts");
        expect(list.lo[0] == (0ull | 1ull << 2 | 3ull << 4 | 2ull << 6) && list.hi[0] == 0ull, "A 0, C 1, G 3, T 2, case folded");
        expect(list.lo[1] == ~0ull && list.hi[1] == (3ull | 0xAAAAAAAAAAAAAAA8ull), "base 32 is the high word's first");
    }
    // ---- the sequence offsets: n_seqs + 1 of them are read, no more; the inserts come first
    expect(refused_with(scan(1, 2, nullptr, one), "NULL"), "offsets NULL");
    {
        std::vector<int64_t> off = {0, 5, 3};
        expect(refused_with(scan(1, 2, off.data(), one), "descends at sequence 1"), "offsets that descend");
        expect(refused_with(scan(1, 2, off.data(), Inserts({"AN"})), "ACGTacgt"), "a bad insert comes before bad offsets");
        off = {-1, 5, 6};
        expect(refused_with(scan(1, 2, off.data(), one), "below 0"), "offsets that start below 0");
        off = {0, (int64_t)1 << 31};
        expect(refused_with(scan(1, 1, off.data(), one), "2^31"), "a sequence of 2^31 bases");
        off = {0, 0, 0, 0};
        expect(scan(1, 3, off.data(), mixed) == GFM_OK, "empty sequences only");
        off = {7, 7};
        expect(scan(1, 1, off.data(), one) == GFM_OK, "one empty sequence at 7");
        off = {0, 0, 130};                                       // three tiles, then the buffers are looked at
        expect(refused_with(scan(1, 2, off.data(), mixed), "NULL"), "bases without buffers");
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
        const int32_t *io = one.offsets.get();
        const uint8_t *ib = one.bases.get();
        for (int hole = 0; hole < 9; ++hole) {
            const gfm_motif_t *pm = hole == 0 ? nullptr : &motif;
            const gfm_motif_t m0 = nullptr;
            const uint64_t *w0 = nullptr, *const *pw = hole == 1 ? nullptr : hole == 6 ? &w0 : &w;
            uint32_t *k0 = nullptr, *const *pk = hole == 2 ? nullptr : hole == 7 ? &k0 : &k;
            uint64_t *s0 = nullptr, *const *ps = hole == 3 ? nullptr : hole == 8 ? &s0 : &s;
            const int rc = gfm_sequence_insertion_scan(hole == 5 ? &m0 : pm, 1, pw, 1, 1, off, hole == 4 ? nullptr : buf, 1, io, ib, 0, pk, ps,
                                                       st, nullptr);
            expect(refused_with(rc, "NULL"), "a NULL buffer");
        }
        expect(refused_with(gfm_sequence_insertion_scan(&motif, 1, &w, 1, 1, off, buf, 1, io, ib, 0, &k, &s, nullptr, nullptr), "NULL"),
               "status NULL");
        uint32_t *k4 = reinterpret_cast<uint32_t *>(buf + 4);
        uint64_t *s8 = reinterpret_cast<uint64_t *>(buf + 8);
        expect(refused_with(gfm_sequence_insertion_scan(&motif, 1, &w, 1, 1, off, buf, 1, io, ib, 0, &k4, &s, st, nullptr), "aligned"),
               "keys at 4 mod 8");
        expect(refused_with(gfm_sequence_insertion_scan(&motif, 1, &w, 1, 1, off, buf, 1, io, ib, 0, &k, &s8, st, nullptr), "aligned"),
               "sums at 8 mod 16");
    }
    // ---- the capacity rule, which the entry applies once it knows W from the motifs' handles, and the LDS a launch asks for
    expect(insscan_side_windows(64, 64) == 254u && insscan_side_windows(1, 1) == 2u && insscan_side_windows(5, 4) == 16u, "windows a side");
    expect(insscan_sum_fits(UINT64_MAX / 2u, 1, 1) && !insscan_sum_fits(UINT64_MAX / 2u + 1u, 1, 1), "the bound at W = 1, L = 1");
    expect(insscan_sum_fits(((uint64_t)1 << 60) - 1u, 5, 4) && !insscan_sum_fits((uint64_t)1 << 60, 5, 4), "the bound at W = 5, L = 4");
    expect(insscan_sum_fits(UINT64_MAX / 254u, 64, 64) && !insscan_sum_fits(UINT64_MAX / 254u + 1u, 64, 64), "the bound at W = L = 64");
    expect(insscan_sum_fits(0u, 64, 64) && !insscan_sum_fits(UINT64_MAX, 1, 1), "the ends");
    expect(insscan_lds_bytes(64, 16, 16 * 64) == 4u * (65u * 65u + 16u * 128u) && insscan_lds_bytes(19, 4, 4) == 4u * (65u * 19u + 80u) &&
               insscan_lds_bytes(1, 1, 1) == 4u * (65u + 2u),
           "the dynamic LDS: the prefix table, then H and T");
    expect(insscan_lds_bytes(64, 16, 16 * 64) + 4288u == 29380u && insscan_lds_bytes(19, 4, 4) + 4288u == 9548u, "the header's LDS figures");
    std::printf("insertion_scan_checks: %d checks passed, %d failed\n", g_checks - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
