"""The insertion scan without a GPU: the brute force (tests/insertion_scan_bruteforce.py) on sequences read by hand, the repeat
rule's closed form against its definition, the key encoding of both sides, the frames of a table whose arrays the brute force
made, the refusals of bad inserts, the command line's refusals, the export, the library's host checks and the header."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import insertion_scan_bruteforce as bf  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_g", "is_reference", "position", "inserted",
           "insert", "length", "named", "ref_score", "ref_pvalue", "ref_start", "ref_strand", "ref_kmer", "alt_score", "alt_pvalue",
           "alt_start", "alt_strand", "alt_kmer", "ref_log2_affinity", "alt_log2_affinity", "delta_log2_affinity", "effect"]
SUMMARY_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "insert", "length", "versions", "haplotypes",
                   "haplotypes_gain", "haplotypes_loss", "min_delta_log2_affinity", "max_delta_log2_affinity", "best_alt_score"]
SM = np.array([[1, 2], [3, 4], [5, 6], [7, 8]])                  # W = 2; rows A, C, G, T
WEIGHTS = np.arange(100, dtype=np.uint64) + 1                    # w[s] = s + 1


def _same(x, y):
    return x == y or (x != x and y != y)


def _hand(x, inserts):
    """W = 2, + only, min_val 0, w[s] = s + 1"""
    return bf.scan(x, 2, SM, 0, WEIGHTS, True, inserts)


def test_the_brute_force_on_a_homopolymer_and_at_the_last_base():
    """AAA: AA scores 3.  Behind the last base the junction has no window and the ALT side has those that end in the insert; of
    the three insertions of A, and of AA, the frames keep the first"""
    one, two = _hand(b"AAA", (b"A", b"AA"))
    assert one[0] == [((3, -1, "+", "AA"), 4), ((3, -1, "+", "AA"), 8)]          # x's start 0; y = AAAA: starts 0, 1
    assert one[1] == [((3, -1, "+", "AA"), 4), ((3, -1, "+", "AA"), 8)]          # x's start 1; y's starts 1, 2
    assert one[2] == [(None, 0), ((3, -1, "+", "AA"), 4)]                        # the last base: y's start 2 alone
    assert two[0] == [((3, -1, "+", "AA"), 4), ((3, -1, "+", "AA"), 12)]         # y = AAAAA: starts 0, 1, 2
    assert two[2] == [(None, 0), ((3, -1, "+", "AA"), 8)]                        # y's starts 2, 3
    assert [[bf.reported(b"AAA", o, i) for o in range(3)] for i in (b"A", b"AA")] == [[True, False, False]] * 2


def test_the_brute_force_on_a_repeat_two_offsets_away():
    """ACAC with the insert AC: behind x[3] it spells ACACAC, as behind x[1]; behind x[2] it spells ACAACC, which is new"""
    (rows,) = _hand(b"ACAC", (b"ac",))
    assert rows[1] == [((5, -1, "+", "CA"), 6), ((5, -1, "+", "CA"), 18)]        # CA = 3 + 2; y = ACACAC: CA, AC, CA at 1, 2, 3
    assert [bf.reported(b"ACAC", o, b"AC") for o in range(4)] == [True, True, True, False]
    assert bf.edited(b"ACAC", 3, b"AC") == bf.edited(b"ACAC", 1, b"AC") == b"ACACAC" and bf.edited(b"ACAC", 2, b"AC") == b"ACAACC"


def test_the_brute_force_on_an_n_beside_the_gap():
    """an insertion repairs nothing: the window that holds the N stays at min_val, the one that does not reach it is clean"""
    (rows,) = _hand(b"AnC", (b"G",))
    assert rows[0] == [((0, -1, "+", "An"), 1), ((7, -1, "+", "AG"), 8 + 1)]     # y = AGnC: AG = 1 + 6, Gn 0
    assert rows[1] == [((0, -1, "+", "nC"), 1), ((9, 0, "+", "GC"), 1 + 10)]     # y = AnGC: nG 0, GC = 5 + 4


def test_the_brute_force_on_short_and_empty_sequences():
    """n < W with Li >= W: x has no window, y has the one across the junction and the one that lies wholly inside the insert"""
    assert _hand(b"A", (b"CG",)) == [[[(None, 0), ((9, 0, "+", "CG"), 6 + 10)]]]  # y = ACG: AC = 1 + 4, CG = 3 + 6
    wide = bf.scan(b"A", 3, np.array([[1, 2, 3]] * 4), 0, WEIGHTS, True, (b"CGT",))
    assert wide == [[[(None, 0), ((6, -1, "+", "ACG"), 14)]]]                     # y = ACGT: starts 0 and 1, both 6
    assert _hand(b"", (b"A", b"ACGT")) == [[], []]
    keys, sums = bf.scan_arrays([b"A", b"", b"AAA"], 2, SM, 0, WEIGHTS, True, (b"CG", b"A"))
    assert keys[0][0] == [0, bf.key_of((9, 0, "+"))] and sums[0][0] == [0, 16] and len(keys[0]) == len(keys[1]) == 4
    assert keys[1][3] == [0, bf.key_of((3, -1, "+"))] and sums[1][1:] == [[4, 8], [4, 8], [0, 4]]


def test_keys_decode_for_every_start_of_both_sides():
    """every start the rule allows, at both ends and in the middle of a sequence, at the shortest and the longest insert, encodes
    into 7 bits and decodes to itself"""
    from grafimo_amd.insertion_scan import COLUMNS as NAMES, MAX_INSERTS, MAX_LENGTH
    from grafimo_amd.query_variants import decode_keys
    assert NAMES == ("JUNCTION", "INS") and MAX_LENGTH == 64 and MAX_INSERTS == 16
    for W in (1, 2, 19, 64):
        for L in (1, 7, 64):
            n = 2 * W + 3
            seen = {"JUNCTION": set(), "INS": set()}
            for o in range(n):
                g = o + 1
                for kind, starts in (("JUNCTION", range(max(0, g - W + 1), min(g - 1, n - W) + 1)),
                                     ("INS", range(max(0, g - W + 1), min(g + L - 1, n + L - W) + 1))):
                    for s in starts:
                        for plus in (0, 1):
                            key = bf.key_of((64_000, s - g, "+" if plus else "-"))
                            assert 0 < key < 1 << 25
                            score, rel, strand = decode_keys(np.array([key]))
                            assert (int(score[0]), g + int(rel[0]), strand[0]) == (64_000, s, "+" if plus else "-")
                        seen[kind].add(s - g)
            assert seen["JUNCTION"] == set(range(-(W - 1), 0)) and seen["INS"] == set(range(-(W - 1), L)), (W, L)


def test_the_leftmost_duplicate_filter_against_the_definition():
    """leftmost_insertions' closed form against `no smaller offset spells the same y`, over a two-letter alphabet: inserts of
    period 1, 2 and 3 and primitive ones, up to 12 bases, at both ends of a sequence and across a sequence boundary of the
    concatenated array"""
    from grafimo_amd.insertion_scan import leftmost_insertions, primitive_period
    rng = np.random.default_rng(19)
    seqs = [b"", b"A", b"ACAC", b"CACA", b"AAaA", b"ACCACC", b"CAC", b""] + \
        [bytes(rng.choice(np.frombuffer(b"ACac", dtype=np.uint8), size=int(n)).tolist()) for n in rng.integers(1, 30, size=14)] + \
        [b"ACACACACAC", b"ACACACACAC", b"CCACCACCA", b"ACCACCACC"]            # (a repeat runs up to a boundary, and on behind it)
    inserts = (b"A", b"CC", b"AAAA", b"AC", b"CA", b"ACAC", b"CACACA", b"ACC", b"CAC", b"ACCACC", b"AACCA", b"ACACA", b"ACCACCACCACC",
               b"CACCAACAACCA", b"ACACACACACAC", b"C")
    assert [primitive_period(i) for i in inserts] == [1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 5, 5, 3, 12, 2, 1]
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    got = leftmost_insertions(off, np.frombuffer(b"".join(seqs), dtype=np.uint8), inserts)
    want = [[bf.reported(x, o, i) for x in seqs for o in range(len(x))] for i in inserts]
    assert got.shape == (len(inserts), int(off[-1])) and got.tolist() == want
    for k in range(len(inserts)):                                # (every insert is kept somewhere; the short periods also dropped)
        assert got[k].any() and (not got[k].all() or primitive_period(inserts[k]) > 3), inserts[k]
    for x in seqs:                                               # the first p offsets of a sequence are always kept
        for i in inserts:
            assert all(bf.reported(x, o, i) for o in range(min(len(x), primitive_period(i))))
    assert leftmost_insertions([0], np.zeros(0, dtype=np.uint8), ("A", "CG")).shape == (2, 0)


INSERTS = (b"G", b"AC", b"CGTACGT")


def _hand_table(W=3, threshold=0.5, fwd=False, inserts=INSERTS, **kw):
    """an InsertionScan over query_variant_bruteforce.hand_graph's regions whose arrays the brute force made -> (the table, the
    brute force's rows of all_rows, its rows with the gaps a repeat repeats)"""
    from oracle import oracle as orc
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.insertion_scan import InsertionScan
    idx = bf.hand_graph()
    regions = [(8, 14), (0, 20), (18, 20)]
    names = [f"c:{s}-{e}" for s, e in regions]
    m = SynMotif(W, seed=5)
    od = motif_as_oracle_dict(m)
    w, s_best = default_weights(m)
    log2_offset = -40 + (s_best / float(od["scale"]) + W * od["offset"])
    ptab = orc.p_table(od["pmf"])
    seqs = [bf.region_sequences(idx, s, e, [[1, 3]]) for s, e in regions]
    scans = [[bf.scan(d["bases"], W, od["score_matrix"], od["min_val"], w, fwd, inserts) for d in region] for region in seqs]
    flat = [(r, d, sc) for r, (region, rs) in enumerate(zip(seqs, scans)) for d, sc in zip(region, rs)]
    coord = [~p if t else p for _, d, _ in flat for p, t in d["coords"][0]]
    keys = [[[bf.key_of(b) for b, _ in row] for _, _, sc in flat for row in sc[k]] for k in range(len(inserts))]
    sums = [[[s for _, s in row] for _, _, sc in flat for row in sc[k]] for k in range(len(inserts))]
    t = InsertionScan("M", "m", W, od["scale"], od["offset"], ptab, log2_offset, threshold, names, ["g"], [r for r, _, _ in flat],
                      [d["version"] for _, d, _ in flat], [d["count"] for _, d, _ in flat], [d["group_counts"] for _, d, _ in flat],
                      [d["is_reference"] for _, d, _ in flat], np.concatenate([[0], np.cumsum([len(d["bases"]) for _, d, _ in flat])]),
                      np.frombuffer(b"".join(d["bases"] for _, d, _ in flat), dtype=np.uint8), coord, inserts,
                      np.array(keys, dtype=np.uint32).reshape(len(inserts), -1, 2),
                      np.array(sums, dtype=np.uint64).reshape(len(inserts), -1, 2), **kw)
    args = (names, seqs, scans, lambda r, d: d["coords"][0], W, od["scale"], od["offset"], ptab, log2_offset, threshold, inserts)
    return t, bf.detail_rows(*args), bf.detail_rows(*args, every=True)


ROW_KEY = ("sequence_name", "version", "position", "inserted", "insert")


@pytest.mark.parametrize("W,fwd", [(3, False), (2, True), (9, False)])
def test_frames_of_a_table_the_brute_force_filled(W, fwd):
    t, rows, every = _hand_table(W, fwd=fwd, all_rows=True)
    frame = t.to_frame()
    assert list(frame.columns) == COLUMNS
    assert len(frame) == len(rows) == len(t) and len(rows) < len(every) == len(INSERTS) * len(t.bases)
    for k, (f, e) in enumerate(zip(frame.to_dict("records"), rows)):
        assert [f["haplotypes_g"]] == e["groups"]
        for c in COLUMNS[2:5] + COLUMNS[6:]:
            assert _same(f[c], e[c]), (k, c, f[c], e[c], e)
    assert frame["inserted"].any() and frame["is_reference"].any() and not frame["is_reference"].all()
    assert set(frame["insert"]) == {i.decode() for i in INSERTS} and frame["named"].any() and not frame["named"].all()
    assert (frame["insert"].str.len() == frame["length"]).all()
    if W <= 3:                                                   # (an insert always leaves a window: every region holds 2 bases)
        assert (frame["alt_kmer"].str.len() == W).all()
    if W == 9:                                                   # [18, 20) has no window of x; only the 7-mer makes one of y
        short = frame[frame["sequence_name"] == "c:18-20"]
        assert len(short) and short["ref_score"].isna().all() and (short["ref_kmer"] == "").all()
        assert ((short["alt_kmer"] != "") == (short["length"] == 7)).all()
    # ---- the filter
    t.all_rows = False
    kept = [e for e in rows if e["effect"] in ("gain", "loss")]
    assert [tuple(f[c] for c in ROW_KEY) for f in t.to_frame().to_dict("records")] == [tuple(e[c] for c in ROW_KEY) for e in kept]
    t.delta = 0.75
    assert len(t.to_frame()) == len([e for e in rows if e["effect"] in ("gain", "loss") or abs(e["delta_log2_affinity"]) >= 0.75])
    # ---- the summary against a loop over the rows of every gap
    t.delta, t.all_rows = None, True
    want = bf.summary_of(every)
    s = t.summary_frame()
    assert list(s.columns) == SUMMARY_COLUMNS and len(s) == len(want) > 0
    for f in s.to_dict("records"):
        w = want[(f["sequence_name"], f["position"], f["insert"])]
        assert (f["versions"], f["haplotypes"], f["haplotypes_gain"], f["haplotypes_loss"], f["length"]) == \
            (w["versions"], w["haplotypes"], w["haplotypes_gain"], w["haplotypes_loss"], len(f["insert"])), f
        assert _same(f["min_delta_log2_affinity"], min(w["deltas"]) if w["deltas"] else np.nan)
        assert _same(f["max_delta_log2_affinity"], max(w["deltas"]) if w["deltas"] else np.nan)
        assert _same(f["best_alt_score"], max(w["scores"]) if w["scores"] else np.nan)
    order = [i.decode() for i in INSERTS]
    keys = [(t.region_names.tolist().index(f["sequence_name"]), f["position"], order.index(f["insert"])) for f in s.to_dict("records")]
    assert keys == sorted(keys)
    assert sum(e["named"] for e in every) > sum(e["named"] for e in rows)        # (the summary counts gaps the detail rows drop)
    t.all_rows = False
    assert len(t.summary_frame()) == sum(1 for w in want.values() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0)
    # ---- the dense arrays keep every cell
    assert t.keys.shape == (len(INSERTS), len(t.bases), 2) and t.log2_affinity().shape == (len(INSERTS), len(t.bases), 2)


def test_named_and_the_leftmost_offset_on_the_hand_made_graph():
    """in [8, 14) haplotype 3 reads ACGGGTAC -- the G at 10 and two inserted behind it --, haplotype 2 reads ACAC, 10 and 11
    deleted: a gap beside an inserted base, or at the panel's deletion, is not named; the insertion of G into the run of three
    is reported once, behind the C before it, and the summary still has a row at the coordinate of every named gap"""
    t, rows, _ = _hand_table(3, all_rows=True)
    f = t.to_frame()
    f = f[f["sequence_name"] == "c:8-14"]
    v3 = f[(f["version"] == 3) & (f["insert"] == "G")]           # coordinates 8 9 10 ~10 ~10 11 12 13
    assert v3[["position", "inserted", "named"]].values.tolist() == \
        [[9, False, True], [10, False, True], [12, False, True], [13, False, True], [14, False, True]]
    every = t.named_gaps()
    a = int(t.seq_offsets[np.flatnonzero((t.seq_region == 0) & (t.seq_version == 3))[0]])
    assert every[a:a + 8].tolist() == [True, True, False, False, False, True, True, True]
    a = int(t.seq_offsets[np.flatnonzero((t.seq_region == 0) & (t.seq_version == 2))[0]])
    assert every[a:a + 4].tolist() == [True, False, True, True]  # ACAC: coordinates 8 9 12 13; behind 9 the panel deletes
    v2 = f[(f["version"] == 2) & (f["insert"] == "AC")]          # AC behind the second C is AC behind the first
    assert v2[["position", "named"]].values.tolist() == [[9, True], [10, False], [13, True]]
    s = t.summary_frame()
    s = s[(s["sequence_name"] == "c:8-14") & (s["insert"] == "AC")]
    assert s["position"].tolist() == [9, 10, 11, 12, 13, 14]
    assert s[s["position"] == 14]["versions"].tolist() == [4]    # (every version ends at 13: ACAC's repeat there is counted)
    assert s[s["position"] == 10]["versions"].tolist() == [3]    # not ACAC: the panel's deletion lies behind its base 9
    assert s[s["position"] == 11]["versions"].tolist() == [2]    # not version 3 (inserted bases behind 10), and ACAC has no 10


def test_bad_inserts_are_value_errors():
    from grafimo_amd.insertion_scan import InsertionScan, checked_inserts, compute_insertion_scan, scan_sequences
    x = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    m = SynMotif(3, seed=1)
    for bad, text in (((), "non-empty"), (["A"] * 17, "at most 16"), (("",), "outside 1 .. 64"), (("A" * 65,), "outside 1 .. 64"),
                      (("ACN",), "one of ACGT"), (("A", "AC-"), "one of ACGT"), (("AC", "ac"), "repeats"), (("A", b"A"), "repeats"),
                      ("ACGT", "non-empty list"), ((5,), "str or bytes"), (("Aé",), "one of ACGT")):
        with pytest.raises(ValueError, match=text):
            scan_sequences([m], [0, 8], x, bad)                  # (before a motif is leased or the library called)
        with pytest.raises(ValueError, match=text):
            checked_inserts(bad)
    with pytest.raises(ValueError, match="repeats"):
        compute_insertion_scan(m, bf.hand_graph(), [(0, 20)], False, None, ("AC", "G", "AC"))
    assert checked_inserts(["a", b"Cg", "T" * 64]) == (b"A", b"CG", b"T" * 64)
    assert len(checked_inserts(["A" * k for k in range(1, 17)])) == 16
    with pytest.raises(ValueError, match="do not fit"):
        InsertionScan("M", "m", 3, 1, 0.0, [1.0], 0.0, 0.5, ["r"], [], [0], [0], [1], np.zeros((1, 0)), [True], [0, 8], x,
                      np.arange(8), ("A", "CG"), np.zeros((1, 8, 2)), np.zeros((1, 8, 2)))


def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(flags),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, "-s", str(tmp_path), "--insertion-scan", "ACGT")
    assert r.returncode != 0 and "--insertion-scan needs the graph" in r.stderr
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--insertion-all")
    assert r.returncode != 0 and "--insertion-all goes with --insertion-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--insertion-delta", "1.5")
    assert r.returncode != 0 and "--insertion-delta goes with --insertion-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--insertion-scan", "ACGT", "--insertion-delta", "-1")
    assert r.returncode != 0 and "--insertion-delta -1.0 is not >= 0" in r.stderr
    for bad, text in ((["ACGT", "ACNT"], "one of ACGT"), (["A" * 65], "outside 1 .. 64"), (["A" * k for k in range(1, 18)], "at most 16")):
        r = _cli(tmp_path, *graph, "--insertion-scan", *bad)
        assert r.returncode != 0 and "ERROR: --insertion-scan: " in r.stderr and text in r.stderr, r.stderr
    r = _cli(tmp_path, *graph, "--insertion-scan")
    assert r.returncode != 0 and "expected at least one argument" in r.stderr
    r = _cli(tmp_path, "--help")
    assert r.returncode == 0 and r.stdout.count("--insertion-scan") >= 5        # its own options and the two lists it joined


def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    name = "gfm_sequence_insertion_scan"
    assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == 15
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert f"int {name}(" in header
    # before a device is touched: bad inserts, an unknown flag and descending offsets are refused, no sequence is a no-op
    call = nv.lib().gfm_sequence_insertion_scan
    err = nv.lib().gfm_last_error

    def entry(n_seqs, off, inserts, flags=0, ioff=None, count=None):
        text = np.frombuffer(b"".join(inserts) + b"\0", dtype=np.uint8).copy()     # (never empty: its pointer is not NULL)
        io = np.array(np.concatenate([[0], np.cumsum([len(i) for i in inserts])]) if ioff is None else ioff, dtype=np.int32)
        return call(None, 1, None, 1, n_seqs, None if off is None else off.ctypes.data, None, len(inserts) if count is None else count,
                    io.ctypes.data, text.ctypes.data, flags, None, None, None, None)
    assert entry(0, None, [b"A", b"acgt" * 16]) == nv.GFM_OK
    assert entry(0, None, [b"A"] * 16) == nv.GFM_OK              # (the library does not compare the inserts)
    assert entry(0, None, [b"A"], flags=2) == nv.GFM_ERR_INVALID and b"unknown flag" in err()
    assert entry(0, None, [b"A"], count=0) == nv.GFM_ERR_INVALID and b"bad argument" in err()
    assert entry(0, None, [b"A"] * 17) == nv.GFM_ERR_INVALID and b"bad argument" in err()
    assert entry(0, None, [b"A"] * 17, flags=2) == nv.GFM_ERR_INVALID and b"bad argument" in err()       # the count comes first
    assert entry(0, None, [b"A", b""]) == nv.GFM_ERR_INVALID and b"length 0 of insert 1 is outside 1 .. 64" in err()
    assert entry(0, None, [b"A" * 65]) == nv.GFM_ERR_INVALID and b"length 65 of insert 0 is outside 1 .. 64" in err()
    assert entry(0, None, [b"AC", b"GNT"]) == nv.GFM_ERR_INVALID and b"base 1 of insert 1 is not one of ACGTacgt" in err()
    assert entry(0, None, [b"ACGT"], ioff=[0, 3, 2], count=2) == nv.GFM_ERR_INVALID and b"insert_offsets descends at insert 1" in err()
    assert entry(0, None, [b"ACGT"], ioff=[1, 3]) == nv.GFM_ERR_INVALID and b"insert_offsets starts at 0" in err()
    assert entry(0, None, [b"NN"], ioff=[0, 3, 2], count=2) == nv.GFM_ERR_INVALID and b"descends" in err()   # the offsets, then the letters
    assert entry(0, None, [b"N" * 65]) == nv.GFM_ERR_INVALID and b"outside 1 .. 64" in err()                 # the lengths, then the letters
    assert call(None, 1, None, 1, 0, None, None, 1, None, None, 0, None, None, None, None) == nv.GFM_ERR_INVALID and b"NULL" in err()
    assert entry(2, np.array([0, 5, 3], dtype=np.int64), [b"AC"]) == nv.GFM_ERR_INVALID and b"descends at sequence 1" in err()
    assert entry(2, np.array([0, 5, 3], dtype=np.int64), [b"AN"]) == nv.GFM_ERR_INVALID and b"ACGTacgt" in err()  # the inserts come first
    assert entry(1, np.array([0, 1 << 31], dtype=np.int64), [b"AC"]) == nv.GFM_ERR_INVALID and b"2^31" in err()
    assert entry(2, np.array([0, 0, 0], dtype=np.int64), [b"AC"]) == nv.GFM_OK
    assert entry(1, np.array([0, 4], dtype=np.int64), [b"AC"]) == nv.GFM_ERR_INVALID and b"NULL" in err()


def test_header_defines_the_constants_and_states_the_rule():
    import re
    from grafimo_amd import _native as nv
    from grafimo_amd import insertion_scan
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    for name, value in (("GFM_INSSCAN_TILE", 64), ("GFM_INSSCAN_MAX_LENGTH", 64), ("GFM_INSSCAN_MAX_INSERTS", 16)):
        m = re.search(rf"#define {name} (\d+)", header)
        assert m and int(m.group(1)) == getattr(nv, name) == value
    assert nv.GFM_INSSCAN_MAX_LENGTH == nv.GFM_QUERY_MAX_ALLELE
    kernel = open(os.path.join(ROOT, "grafimo_amd", "csrc", "gfm_graph_insertion_scan.hpp")).read()
    squeeze = lambda s: " ".join(s.replace("*", " ").replace("//", " ").split())                   # noqa: E731
    texts = [squeeze(header), squeeze(insertion_scan.__doc__), squeeze(bf.__doc__), squeeze(kernel)]
    for line in ("Every insert holds A, C, G, T only. Case is folded, as base_code does.",
                 "The edit is the insertion of I behind x[o]. Let o' = o + 1 and y = x[:o'] + I + x[o':].",
                 "rule with lr = 0, la = Li at offset o'.",
                 "REF side (column JUNCTION): the starts s of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).",
                 "It does not depend on the insert. It equals the indel scan's JUNCTION column bit for bit.",
                 "ALT side (column INS): the starts s of y with max(0, o' - W + 1) <= s <= min(o' + Li - 1, n + Li - W).",
                 "A window that lies wholly inside the insert counts, as the query rule counts it.",
                 "A window that holds a base of x that is not A/C/G/T scores min_val on both strands.",
                 "An insertion repairs nothing, because it removes no base. A window that does not reach the N is clean.",
                 "((score + 1) << 8) | ((64 - (s - o')) << 1) | plus, s - o' in -(W - 1) .. -1 for JUNCTION and in -(W - 1) .. Li - 1 for INS.",
                 "Key 0 means the side has no window.",
                 "Per column, the exact uint64 sum of w[score] over the side's windows and strands.",
                 "An insertion before the first base of a sequence is not scanned, as in the indel scan. An empty sequence has no rows.",
                 "With the inserts (\"A\", \"C\", \"G\", \"T\") the INS columns equal the indel scan's INS_A .. INS_T bit for bit.",
                 "A cell does not depend on the other inserts of the list or on their order."):
        for text in texts:
            assert line in text, line
