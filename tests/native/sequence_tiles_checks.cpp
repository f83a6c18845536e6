// sequence_tiles_checks.cpp -- what gfm_sequence_tiles.hpp gives the host side of the sequence scans, under ASan/UBSan and
// without a GPU: the offset walk (seq_tiles) and the length mask (length_mask) called directly on heap arrays of exactly the
// size they may read, and the same offset cases through gfm_sequence_mutation_scan and gfm_sequence_indel_scan, whose
// argument checks no other program here runs: every message must name the entry that was called.  Every call below returns
// before anything is launched, and none needs a device.  The program IS graph_extract.hip (included as this translation unit's
// text, so that the helpers in its anonymous namespace can be called too) with a main of its own:
//
//   c=grafimo_amd/csrc; bash $c/build.sh    # the other objects
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -Iinclude -I$c \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined \
//         -x hip -c tests/native/sequence_tiles_checks.cpp -o /tmp/sequence_tiles_checks.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/sequence_tiles_checks /tmp/sequence_tiles_checks.o \
//         $c/grafimo_hip.o $c/score_quad_g*_m*.o $c/stream_calib.o $c/region_reduce.o $c/hit_pairs.o $c/hit_linkage.o \
//         $c/tsv_ingest.o $c/vcf_ingest.o $c/scan_stream.o $c/gfm_workers.o $c/graph_tsv_writer.o $c/hit_table.o \
//         $c/variant_table.o -lpthread -lz
//   /tmp/sequence_tiles_checks              # prints "sequence_tiles_checks: N checks passed", exit status 0
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

bool refused_with(int rc, const std::string &text) { return rc == GFM_ERR_INVALID && std::strstr(gfm_last_error(), text.c_str()) != nullptr; }

// the two entries take the same arguments; with nothing but those the host checks read
using Entry = int (*)(const gfm_motif_t *, int32_t, const uint64_t *const *, uint64_t, int32_t, const int64_t *, const uint8_t *, uint32_t,
                      uint32_t *const *, uint64_t *const *, int32_t *, void *);
int scan(Entry entry, int32_t n_motifs, int32_t n_seqs, const int64_t *off, uint32_t flags = 0)
{
    return entry(nullptr, n_motifs, nullptr, 1, n_seqs, off, nullptr, flags, nullptr, nullptr, nullptr, nullptr);
}

void entry_cases(Entry entry, const std::string &name)
{
    const std::string prefix = name + ": ";
    expect(scan(entry, 0, 0, nullptr) == GFM_ERR_INVALID && !std::strcmp(gfm_last_error(), "bad argument"), "no motif");
    expect(scan(entry, 1, -1, nullptr) == GFM_ERR_INVALID && !std::strcmp(gfm_last_error(), "bad argument"), "a negative number of sequences");
    expect(scan(entry, 1, 0, nullptr, 2u) == GFM_ERR_INVALID && !std::strcmp(gfm_last_error(), "unknown flag"), "an unknown flag");
    expect(scan(entry, 1, 0, nullptr) == GFM_OK, "no sequence, no offsets");
    expect(refused_with(scan(entry, 1, 2, nullptr), prefix + "NULL argument"), "offsets NULL");
    // the offsets: n_seqs + 1 of them are read, no more (a heap array of that size: ASan sees a read past it)
    std::vector<int64_t> off = {-1, 5, 6};
    expect(refused_with(scan(entry, 1, 2, off.data()), prefix + "seq_offsets descends below 0"), "a first offset below 0");
    off = {0, 5, 9, 8};
    expect(refused_with(scan(entry, 1, 3, off.data()), prefix + "seq_offsets descends at sequence 2"), "offsets that descend at 2");
    off = {0, 5, 3};
    expect(refused_with(scan(entry, 1, 2, off.data()), prefix + "seq_offsets descends at sequence 1"), "offsets that descend at 1");
    off = {0, 3, 3 + ((int64_t)1 << 31)};
    expect(refused_with(scan(entry, 1, 2, off.data()), prefix + "sequence 1 holds 2^31 bases or more"), "a sequence of 2^31 bases");
    off = {0, 0, 0, 0};
    expect(scan(entry, 1, 3, off.data()) == GFM_OK, "empty sequences only");
    off = {7, 7};
    expect(scan(entry, 1, 1, off.data()) == GFM_OK, "one empty sequence at 7");
    off = {0, 0, 130};                                           // three tiles, then the buffers are looked at
    expect(refused_with(scan(entry, 1, 2, off.data()), prefix + "NULL argument"), "bases without buffers");
}

}  // namespace

int main()
{
    entry_cases(gfm_sequence_mutation_scan, "gfm_sequence_mutation_scan");
    entry_cases(gfm_sequence_indel_scan, "gfm_sequence_indel_scan");
    // ---- seq_tiles itself: the tiles of each sequence in order, the last one short; nothing read with no sequence
    {
        std::vector<SeqTile> tiles;
        expect(seq_tiles("e", 64, 0, nullptr, tiles) == GFM_OK && tiles.empty(), "no sequence reads nothing");
        std::vector<int64_t> off = {0, 130, 130, 194, 195};
        expect(seq_tiles("e", 64, 4, off.data(), tiles) == GFM_OK && tiles.size() == 5u, "3 + 0 + 1 + 1 tiles");
        bool ok = tiles.size() == 5u;
        const long long begin[] = {0, 0, 0, 130, 194};
        const int len[] = {130, 130, 130, 64, 1}, start[] = {0, 64, 128, 0, 0};
        for (size_t i = 0; ok && i < 5u; ++i) ok = tiles[i].begin == begin[i] && tiles[i].len == len[i] && tiles[i].start == start[i];
        expect(ok, "the tiles' fields");
        tiles.clear();
        expect(seq_tiles("e", 32, 1, off.data(), tiles) == GFM_OK && tiles.size() == 5u && tiles[4].start == 128, "another tile size");
        tiles.clear();
        off = {0, 0x7fffffffll};                                  // the longest sequence a tile's int fields hold
        expect(seq_tiles("e", 1 << 30, 1, off.data(), tiles) == GFM_OK && tiles.size() == 2u && tiles[0].len == 0x7fffffff, "2^31 - 1 bases");
        off = {5, 4};
        expect(refused_with(seq_tiles("other_entry", 64, 1, off.data(), tiles), "other_entry: seq_offsets descends at sequence 0"),
               "the message names the entry it is given");
    }
    // ---- length_mask: exactly n_lengths are read
    {
        unsigned long long mask = 0ull;
        expect(refused_with(length_mask("e", 1, nullptr, 64, mask), "e: NULL argument"), "lengths NULL");
        std::vector<int32_t> l = {1, 2, 7, 64};
        expect(length_mask("e", 4, l.data(), 64, mask) == GFM_OK && mask == ((1ull << 63) | (1ull << 6) | 3ull), "1, 2, 7, 64");
        expect(length_mask("e", 3, l.data(), 7, mask) == GFM_OK && mask == ((1ull << 6) | 3ull), "a shorter list under a smaller cap");
        expect(refused_with(length_mask("e", 4, l.data(), 63, mask), "e: length 64 is outside 1 .. 63"), "a length above the cap");
        std::vector<int32_t> every(64);
        for (int i = 0; i < 64; ++i) every[(size_t)i] = i + 1;
        expect(length_mask("e", 64, every.data(), 64, mask) == GFM_OK && mask == ~0ull, "all 64 lengths");
        for (const int bad : {0, -1, 65, INT32_MAX, INT32_MIN}) {
            l = {1, bad};
            expect(refused_with(length_mask("e", 2, l.data(), 64, mask), "e: length " + std::to_string(bad) + " is outside 1 .. 64"),
                   "a length outside 1 .. 64");
        }
        l = {3, 3};
        expect(refused_with(length_mask("e", 2, l.data(), 64, mask), "e: the lengths do not strictly ascend at 1"), "equal lengths");
        l = {1, 5, 4};
        expect(refused_with(length_mask("e", 3, l.data(), 64, mask), "e: the lengths do not strictly ascend at 2"), "lengths that descend");
    }
    // ---- the capacity of a sum: one predicate under the four entries' refusals
    expect(seq_sum_fits(UINT64_MAX / 2u, 2u) && !seq_sum_fits(UINT64_MAX / 2u + 1u, 2u), "the bound at two windows");
    expect(seq_sum_fits(UINT64_MAX / 38u, 38u) && !seq_sum_fits(UINT64_MAX / 38u + 1u, 38u), "the bound at W = 19, one base");
    expect(seq_sum_fits(0u, 254u) && seq_sum_fits(UINT64_MAX, 1u) && !seq_sum_fits(UINT64_MAX, 2u), "the ends");
    expect(seq_sum_fits(12345u, 2u * 19u) == delscan_sum_fits(12345u, 19, 1) &&
           seq_sum_fits(UINT64_MAX / 38u + 1u, 38u) == delscan_sum_fits(UINT64_MAX / 38u + 1u, 19, 1), "the one-base scans are lmax = 1");
    expect(check_sum_capacity("e", 7u, 4u, "") == GFM_OK, "a sum that fits");
    expect(refused_with(check_sum_capacity("e", UINT64_MAX, 38u, ""),
                        "e: a side holds up to 38 windows: with weights up to 18446744073709551615 a sum may pass 2^64 - 1"),
           "the one-base scans' refusal");
    expect(refused_with(check_sum_capacity("e", UINT64_MAX, 16u, " (W = 5, longest length 4)"),
                        "e: a side holds up to 16 windows (W = 5, longest length 4): with weights up to 18446744073709551615 a sum may "
                        "pass 2^64 - 1"),
           "the block scans' refusal");
    std::printf("sequence_tiles_checks: %d checks passed, %d failed\n", g_checks - g_failed, g_failed);
    return g_failed ? 1 : 0;
}
