"""The deletion scan without a GPU: the brute force (tests/deletion_scan_bruteforce.py) on sequences read by hand, the key
encoding of both sides at every length, the leftmost-duplicate filter, the frames of a table whose arrays the brute force made,
the refusals of bad lengths, the command line's refusals, the export and the header."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deletion_scan_bruteforce as bf  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_g", "is_reference", "position", "inserted",
           "length", "named", "deleted", "ref_score", "ref_pvalue", "ref_start", "ref_strand", "ref_kmer", "alt_score", "alt_pvalue",
           "alt_start", "alt_strand", "alt_kmer", "ref_log2_affinity", "alt_log2_affinity", "delta_log2_affinity", "effect"]
SUMMARY_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "length", "versions", "haplotypes", "haplotypes_gain",
                   "haplotypes_loss", "min_delta_log2_affinity", "max_delta_log2_affinity", "best_alt_score"]
SM = np.array([[1, 2], [3, 4], [5, 6], [7, 8]])                  # W = 2; rows A, C, G, T
WEIGHTS = np.arange(100, dtype=np.uint64) + 1                    # w[s] = s + 1


def _same(x, y):
    return x == y or (x != x and y != y)


def _hand(x, lengths):
    """W = 2, + only, min_val 0, w[s] = s + 1"""
    return bf.scan(x, 2, SM, 0, WEIGHTS, True, lengths)


def test_the_brute_force_on_a_homopolymer():
    """AAAA, L = 2: AA scores 3; one junction window exists only at o = 1; o = 3 does not fit; the frames keep o = 0 alone"""
    (rows,) = _hand(b"AAAA", (2,))
    assert rows[0] == [((3, 0, "+", "AA"), 8), (None, 0)]                        # starts 0, 1; y = AA has no window across 0
    assert rows[1] == [((3, -1, "+", "AA"), 12), ((3, -1, "+", "AA"), 4)]        # starts 0, 1, 2; y = AA: its one window
    assert rows[2] == [((3, -1, "+", "AA"), 8), (None, 0)]                       # starts 1, 2; the junction is y's end
    assert rows[3] == bf.NONE
    assert [bf.reported(b"AAAA", o, 2) for o in range(4)] == [True, False, False, False]


def test_the_brute_force_on_an_n_inside_and_outside_the_block():
    """a deleted N repairs its junction window; an N elsewhere leaves it at min_val"""
    (rows,) = _hand(b"ANnC", (2,))
    assert rows[1] == [((0, -1, "+", "AN"), 3), ((5, -1, "+", "AC"), 6)]         # AN, Nn, nC at 0; y = AC scores 1 + 4
    (rows,) = _hand(b"NACG", (2,))
    assert rows[1] == [((9, 1, "+", "CG"), 1 + 6 + 10), ((0, -1, "+", "NG"), 1)]  # NA 0, AC 5, CG 3 + 6; y = NG
    both = _hand(b"NACG", (1, 2))                                                # a length's rows do not depend on the list
    assert both[1] == rows and both[0][0] == [((0, 0, "+", "NA"), 1), (None, 0)]


def test_the_brute_force_on_short_sequences():
    """n < W: a block fits and has no window on either side; n = L: the whole sequence goes; o + L > n: four zeros"""
    assert _hand(b"A", (1,)) == [[[(None, 0), (None, 0)]]]
    three, = _hand(b"ACG", (3,))
    assert three[0] == [((9, 1, "+", "CG"), 6 + 10), (None, 0)] and three[1] == bf.NONE and three[2] == bf.NONE
    keys, sums = bf.scan_arrays([b"ACG", b"", b"A"], 2, SM, 0, WEIGHTS, True, (3, 4))
    assert keys[0][1:] == [[0, 0]] * 3 and sums[0][1:] == [[0, 0]] * 3 and keys[1] == [[0, 0]] * 4 and sums[1] == [[0, 0]] * 4
    assert keys[0][0] == [bf.key_of((9, 1, "+")), 0] and sums[0][0] == [16, 0]
    assert _hand(b"", (1, 64)) == [[], []]


def test_keys_decode_for_every_start_of_both_sides():
    """every start the rule allows, at both ends and in the middle of a sequence, at the shortest and the longest length, encodes
    into 7 bits and decodes to itself"""
    from grafimo_amd.deletion_scan import COLUMNS as NAMES, MAX_LENGTH
    from grafimo_amd.query_variants import decode_keys
    assert NAMES == ("COVER", "DEL") and MAX_LENGTH == 64
    for W in (1, 2, 19, 64):
        for L in (1, 7, 64):
            n = 2 * W + L + 3
            seen = {"COVER": set(), "DEL": set()}
            for o in range(n - L + 1):
                for kind, starts in (("COVER", range(max(0, o - W + 1), min(o + L - 1, n - W) + 1)),
                                     ("DEL", range(max(0, o - W + 1), min(o - 1, n - L - W) + 1))):
                    for s in starts:
                        for plus in (0, 1):
                            key = bf.key_of((64_000, s - o, "+" if plus else "-"))
                            assert 0 < key < 1 << 25
                            score, rel, strand = decode_keys(np.array([key]))
                            assert (int(score[0]), o + int(rel[0]), strand[0]) == (64_000, s, "+" if plus else "-")
                        seen[kind].add(s - o)
            assert seen["COVER"] == set(range(-(W - 1), L)) and seen["DEL"] == set(range(-(W - 1), 0)), (W, L)


def test_the_leftmost_duplicate_filter_against_a_loop():
    from grafimo_amd.deletion_scan import leftmost_deletions
    rng = np.random.default_rng(9)
    seqs = [b"", b"A", b"AAaA", b"ACACAC", b"ACCGTT", b"NNA", b""] + \
        [bytes(rng.choice(np.frombuffer(b"ACGTacgN", dtype=np.uint8), size=40).tolist()) for _ in range(6)]
    lengths = (1, 2, 3, 7, 40, 64)
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    got = leftmost_deletions(off, np.frombuffer(b"".join(seqs), dtype=np.uint8), lengths)
    want = [[bf.reported(x, o, L) for x in seqs for o in range(len(x))] for L in lengths]
    assert got.shape == (len(lengths), int(off[-1])) and got.tolist() == want
    # and the reason: a block that is reported spells a y no earlier offset of its sequence spells
    for L in lengths:
        for x in seqs:
            spelled = set()
            for o in range(len(x) - L + 1):
                y = (x[:o] + x[o + L:]).upper()
                assert bf.reported(x, o, L) == (y not in spelled), (x, o, L)
                spelled.add(y)
    assert got[0].any() and not got[0].all() and got[4].any() and not got[5].any()
    assert leftmost_deletions([0], np.zeros(0, dtype=np.uint8), (1, 2)).shape == (2, 0)


LENGTHS = (1, 2, 3)


def _hand_table(W=3, threshold=0.5, fwd=False, lengths=LENGTHS, **kw):
    """a DeletionScan over query_variant_bruteforce.hand_graph's regions whose arrays the brute force made -> (the table, the
    brute force's rows of all_rows, its rows with the blocks a repeat repeats)"""
    from oracle import oracle as orc
    from grafimo_amd.deletion_scan import DeletionScan
    from grafimo_amd.haplotype_affinity import default_weights
    idx = bf.hand_graph()
    regions = [(8, 14), (0, 20), (18, 20)]
    names = [f"c:{s}-{e}" for s, e in regions]
    m = SynMotif(W, seed=5)
    od = motif_as_oracle_dict(m)
    w, s_best = default_weights(m)
    log2_offset = -40 + (s_best / float(od["scale"]) + W * od["offset"])
    ptab = orc.p_table(od["pmf"])
    seqs = [bf.region_sequences(idx, s, e, [[1, 3]]) for s, e in regions]
    scans = [[bf.scan(d["bases"], W, od["score_matrix"], od["min_val"], w, fwd, lengths) for d in region] for region in seqs]
    flat = [(r, d, sc) for r, (region, rs) in enumerate(zip(seqs, scans)) for d, sc in zip(region, rs)]
    coord = [~p if t else p for _, d, _ in flat for p, t in d["coords"][0]]
    keys = [[[bf.key_of(b) for b, _ in row] for _, _, sc in flat for row in sc[k]] for k in range(len(lengths))]
    sums = [[[s for _, s in row] for _, _, sc in flat for row in sc[k]] for k in range(len(lengths))]
    t = DeletionScan("M", "m", W, od["scale"], od["offset"], ptab, log2_offset, threshold, names, ["g"], [r for r, _, _ in flat],
                     [d["version"] for _, d, _ in flat], [d["count"] for _, d, _ in flat], [d["group_counts"] for _, d, _ in flat],
                     [d["is_reference"] for _, d, _ in flat], np.concatenate([[0], np.cumsum([len(d["bases"]) for _, d, _ in flat])]),
                     np.frombuffer(b"".join(d["bases"] for _, d, _ in flat), dtype=np.uint8), coord, lengths,
                     np.array(keys, dtype=np.uint32).reshape(len(lengths), -1, 2),
                     np.array(sums, dtype=np.uint64).reshape(len(lengths), -1, 2), **kw)
    args = (names, seqs, scans, lambda r, d: d["coords"][0], W, od["scale"], od["offset"], ptab, log2_offset, threshold, lengths)
    return t, bf.detail_rows(*args), bf.detail_rows(*args, every=True)


ROW_KEY = ("sequence_name", "version", "position", "inserted", "length", "deleted")


@pytest.mark.parametrize("W,fwd", [(3, False), (2, True), (7, False)])
def test_frames_of_a_table_the_brute_force_filled(W, fwd):
    t, rows, every = _hand_table(W, fwd=fwd, all_rows=True)
    frame = t.to_frame()
    assert list(frame.columns) == COLUMNS
    assert len(frame) == len(rows) == len(t) and len(rows) < len(every) < len(LENGTHS) * len(t.bases)
    for k, (f, e) in enumerate(zip(frame.to_dict("records"), rows)):
        assert [f["haplotypes_g"]] == e["groups"]
        for c in COLUMNS[2:5] + COLUMNS[6:]:
            assert _same(f[c], e[c]), (k, c, f[c], e[c], e)
    assert frame["inserted"].any() and frame["is_reference"].any() and not frame["is_reference"].all()
    assert set(frame["length"]) == set(LENGTHS) and frame["named"].any() and not frame["named"].all()
    assert (frame["deleted"].str.len() == frame["length"]).all()
    if W == 3:
        assert {"both", "loss", "none"} <= set(frame["effect"]), set(frame["effect"])
    if W == 7:                                                                          # [18, 20) is shorter than W - 1
        short = frame[frame["sequence_name"] == "c:18-20"]
        assert len(short) and short["alt_score"].isna().all() and (short["alt_kmer"] == "").all() and (short["effect"] == "none").all()
    # ---- the filter
    t.all_rows = False
    kept = [e for e in rows if e["effect"] in ("gain", "loss")]
    assert [tuple(f[c] for c in ROW_KEY) for f in t.to_frame().to_dict("records")] == [tuple(e[c] for c in ROW_KEY) for e in kept]
    t.delta = 0.75
    assert len(t.to_frame()) == len([e for e in rows if e["effect"] in ("gain", "loss") or abs(e["delta_log2_affinity"]) >= 0.75])
    # ---- the summary against a loop over the rows of every block that fits
    t.delta, t.all_rows = None, True
    want = bf.summary_of(every)
    s = t.summary_frame()
    assert list(s.columns) == SUMMARY_COLUMNS and len(s) == len(want) > 0
    for f in s.to_dict("records"):
        w = want[(f["sequence_name"], f["position"], f["length"])]
        assert (f["versions"], f["haplotypes"], f["haplotypes_gain"], f["haplotypes_loss"]) == \
            (w["versions"], w["haplotypes"], w["haplotypes_gain"], w["haplotypes_loss"]), f
        assert _same(f["min_delta_log2_affinity"], min(w["deltas"]) if w["deltas"] else np.nan)
        assert _same(f["max_delta_log2_affinity"], max(w["deltas"]) if w["deltas"] else np.nan)
        assert _same(f["best_alt_score"], max(w["scores"]) if w["scores"] else np.nan)
    keys = [(t.region_names.tolist().index(f["sequence_name"]), f["position"], f["length"]) for f in s.to_dict("records")]
    assert keys == sorted(keys)
    assert sum(e["named"] for e in every) > sum(e["named"] for e in rows)        # (the summary counts blocks the detail rows drop)
    t.all_rows = False
    assert len(t.summary_frame()) == sum(1 for w in want.values() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0)
    # ---- the dense arrays keep every cell
    assert t.keys.shape == (len(LENGTHS), len(t.bases), 2) and t.log2_affinity().shape == (len(LENGTHS), len(t.bases), 2)


def test_named_and_the_leftmost_offset_on_the_hand_made_graph():
    """in [8, 14) haplotype 3 reads ACGGGTAC -- the G at 10 and two inserted behind it --, haplotype 2 reads ACAC, 10 and 11
    deleted: a block that holds an inserted base, or whose coordinates jump over the panel's deletion, is not named; of the
    three deletions of one G the frames hold the first, of the two of GG too"""
    t, rows, _ = _hand_table(3, all_rows=True)
    f = t.to_frame()
    f = f[f["sequence_name"] == "c:8-14"]
    v3 = f[f["version"] == 3]                                    # coordinates 8 9 10 ~10 ~10 11 12 13
    assert v3[v3["deleted"] == "G"][["position", "inserted", "named"]].values.tolist() == [[11, False, True]]
    assert v3[v3["deleted"] == "GG"][["position", "inserted", "named"]].values.tolist() == [[11, False, False]]
    assert v3[v3["deleted"] == "GGG"]["named"].tolist() == [False]
    assert v3[v3["deleted"] == "CG"]["named"].tolist() == [True] and v3[v3["deleted"] == "CGG"]["named"].tolist() == [False]
    assert v3[v3["deleted"] == "GT"][["inserted", "named"]].values.tolist() == [[True, False]]
    assert v3[v3["deleted"] == "TAC"]["named"].tolist() == [True]
    v2 = f[f["version"] == 2]                                    # ACAC: coordinates 8 9 12 13
    assert sorted(zip(v2["deleted"], v2["position"], v2["named"])) == \
        [("A", 9, True), ("A", 13, True), ("AC", 9, True), ("ACA", 9, False), ("C", 10, True), ("C", 14, True), ("CAC", 10, False)]
    every = t.named_blocks()
    a = int(t.seq_offsets[np.flatnonzero((t.seq_region == 0) & (t.seq_version == 2))[0]])
    assert every[:, a:a + 4].tolist() == [[True, True, True, True], [True, False, True, False], [False, False, False, False]]
    s = t.summary_frame()
    s = s[s["sequence_name"] == "c:8-14"]
    assert s[(s["position"] == 9) & (s["length"] == 2)]["versions"].tolist() == [4]
    assert s[(s["position"] == 10) & (s["length"] == 2)]["versions"].tolist() == [3]                 # AC, CA: not ACAC's C|A
    assert s[(s["position"] == 11) & (s["length"] == 2)]["versions"].tolist() == [2]                 # GT of the reference's two
    assert s[(s["position"] == 13) & (s["length"] == 2)]["versions"].tolist() == [4]                 # ACAC's second AC: not a row


def test_bad_lengths_are_value_errors():
    from grafimo_amd.deletion_scan import DeletionScan, checked_lengths, compute_deletion_scan, scan_sequences
    x = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    m = SynMotif(3, seed=1)
    for bad, text in (((0,), "1 .. 64"), ((65,), "1 .. 64"), ((-3, 2), "1 .. 64"), ((2, 2), "strictly ascend"),
                      ((5, 3), "strictly ascend"), ((), "non-empty"), ((1.5,), "integers"), (((1, 2),), "non-empty list")):
        with pytest.raises(ValueError, match=text):
            scan_sequences([m], [0, 8], x, bad)                  # (before a motif is leased or the library called)
        with pytest.raises(ValueError, match=text):
            checked_lengths(bad)
    with pytest.raises(ValueError, match="strictly ascend"):
        compute_deletion_scan(m, bf.hand_graph(), [(0, 20)], False, None, (3, 1))
    assert checked_lengths([1, 64]).tolist() == [1, 64] and checked_lengths(np.arange(1, 65)).dtype == np.int32
    with pytest.raises(ValueError, match="do not fit"):
        DeletionScan("M", "m", 3, 1, 0.0, [1.0], 0.0, 0.5, ["r"], [], [0], [0], [1], np.zeros((1, 0)), [True], [0, 8], x,
                     np.arange(8), (1, 2), np.zeros((1, 8, 2)), np.zeros((1, 8, 2)))


def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(flags),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, "-s", str(tmp_path), "--deletion-scan", "5")
    assert r.returncode != 0 and "--deletion-scan needs the graph" in r.stderr
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--deletion-all")
    assert r.returncode != 0 and "--deletion-all goes with --deletion-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--deletion-delta", "1.5")
    assert r.returncode != 0 and "--deletion-delta goes with --deletion-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--deletion-scan", "5", "--deletion-delta", "-1")
    assert r.returncode != 0 and "--deletion-delta -1.0 is not >= 0" in r.stderr
    for bad in ("0", "65"):
        r = _cli(tmp_path, *graph, "--deletion-scan", "5", bad)
        assert r.returncode != 0 and f"--deletion-scan {bad}: a length lies in 1 .. 64" in r.stderr
    r = _cli(tmp_path, *graph, "--deletion-scan")
    assert r.returncode != 0 and "expected at least one argument" in r.stderr
    r = _cli(tmp_path, "--help")
    assert r.returncode == 0 and r.stdout.count("--deletion-scan") >= 5         # its own options and the two lists it joined


def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    name = "gfm_sequence_deletion_scan"
    assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == 14
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert f"int {name}(" in header
    # before a device is touched: bad lengths, an unknown flag and descending offsets are refused, no sequence is a no-op
    call = nv.lib().gfm_sequence_deletion_scan

    def entry(n_seqs, off, lengths, flags=0):
        ln = np.array(lengths, dtype=np.int32)
        return call(None, 1, None, 1, n_seqs, None if off is None else off.ctypes.data, None, len(ln), ln.ctypes.data, flags, None,
                    None, None, None)
    assert entry(0, None, [1, 64]) == nv.GFM_OK
    assert entry(0, None, [1], flags=2) == nv.GFM_ERR_INVALID and b"unknown flag" in nv.lib().gfm_last_error()
    for bad, text in (([0], b"outside 1 .. 64"), ([65], b"outside 1 .. 64"), ([3, 3], b"strictly ascend"), ([4, 2], b"strictly ascend")):
        assert entry(0, None, bad) == nv.GFM_ERR_INVALID and text in nv.lib().gfm_last_error(), bad
    assert call(None, 1, None, 1, 0, None, None, 1, None, 0, None, None, None, None) == nv.GFM_ERR_INVALID      # lengths NULL
    assert call(None, 1, None, 1, 0, None, None, 0, None, 0, None, None, None, None) == nv.GFM_ERR_INVALID      # no length
    assert entry(2, np.array([0, 5, 3], dtype=np.int64), [2]) == nv.GFM_ERR_INVALID and b"descends" in nv.lib().gfm_last_error()
    assert entry(1, np.array([0, 1 << 31], dtype=np.int64), [2]) == nv.GFM_ERR_INVALID and b"2^31" in nv.lib().gfm_last_error()
    assert entry(2, np.array([0, 0, 0], dtype=np.int64), [2]) == nv.GFM_OK
    assert entry(1, np.array([0, 4], dtype=np.int64), [2]) == nv.GFM_ERR_INVALID and b"NULL" in nv.lib().gfm_last_error()


def test_header_defines_the_tile_and_states_the_rule():
    import re
    from grafimo_amd import _native as nv
    from grafimo_amd import deletion_scan
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    for name in ("GFM_DELSCAN_TILE", "GFM_DELSCAN_MAX_LENGTH"):
        m = re.search(rf"#define {name} (\d+)", header)
        assert m and int(m.group(1)) == getattr(nv, name) == 64
    assert nv.GFM_DELSCAN_MAX_LENGTH == nv.GFM_QUERY_MAX_ALLELE
    kernel = open(os.path.join(ROOT, "grafimo_amd", "csrc", "gfm_graph_deletion_scan.hpp")).read()
    squeeze = lambda s: " ".join(s.replace("*", " ").replace("//", " ").split())                   # noqa: E731
    texts = [squeeze(header), squeeze(deletion_scan.__doc__), squeeze(bf.__doc__), squeeze(kernel)]
    for line in ("If o + L > n there is no edit: both keys and both sums of the cell are 0.",
                 "Otherwise y = x[:o] + x[o+L:].",
                 "rule with lr = L, la = 0 at offset o.",
                 "REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o + L - 1, n - W).",
                 "ALT side (column DEL): the starts of y across the junction, max(0, o - W + 1) <= s <= min(o - 1, n - L - W).",
                 "A window that holds a base that is not A/C/G/T scores min_val on both strands.",
                 "Case is folded, as base_code does.",
                 "A deleted N can repair its junction windows. An N elsewhere cannot be repaired.",
                 "((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. L - 1 for COVER and in -(W - 1) .. -1 for DEL",
                 "Key 0 means the side has no window.",
                 "Per column, the exact uint64 sum of w[score] over the side's windows and strands."):
        for text in texts:
            assert line in text, line
