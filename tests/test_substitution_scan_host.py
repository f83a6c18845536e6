"""The substitution scan without a GPU: the brute force (tests/substitution_scan_bruteforce.py) on sequences read by hand, the
key encoding of both sides at every length, changed_bases against a loop, the frames of a table whose arrays the brute force
made, the refusals of bad maps and bad lengths, the command line's refusals, the export and the header."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import substitution_scan_bruteforce as bf  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_g", "is_reference", "position", "inserted",
           "length", "named", "map", "replaced", "replacement", "changed", "ref_score", "ref_pvalue", "ref_start", "ref_strand",
           "ref_kmer", "alt_score", "alt_pvalue", "alt_start", "alt_strand", "alt_kmer", "ref_log2_affinity", "alt_log2_affinity",
           "delta_log2_affinity", "effect"]
SUMMARY_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "length", "versions", "haplotypes", "haplotypes_gain",
                   "haplotypes_loss", "min_delta_log2_affinity", "max_delta_log2_affinity", "best_alt_score"]
SM = np.array([[1, 2], [3, 4], [5, 6], [7, 8]])                  # W = 2; rows A, C, G, T
WEIGHTS = np.arange(100, dtype=np.uint64) + 1                    # w[s] = s + 1


def _same(x, y):
    return x == y or (x != x and y != y)


def _hand(x, lengths, letters):
    """W = 2, + only, min_val 0, w[s] = s + 1"""
    return bf.scan(x, 2, SM, 0, WEIGHTS, True, lengths, letters)


def test_the_brute_force_on_a_homopolymer_under_a_constant_map():
    """AAAA, L = 2: AA scores 3.  Under AAAA nothing changes: SUB is COVER and changed is 0 in every cell.  Under CCCC the block
    becomes CC: AC 5, CC 7, CA 5."""
    (rows,) = _hand(b"AAAA", (2,), "AAAA")
    assert rows[0] == [((3, 0, "+", "AA"), 8)] * 2 and rows[1] == [((3, -1, "+", "AA"), 12)] * 2
    assert rows[2] == [((3, -1, "+", "AA"), 8)] * 2 and rows[3] == bf.NONE
    assert [bf.changed(b"AAAA", o, 2, "AAAA") for o in range(4)] == [0, 0, 0, 0]
    (rows,) = _hand(b"AAAA", (2,), "CCCC")
    assert rows[0] == [((3, 0, "+", "AA"), 8), ((7, 0, "+", "CC"), 8 + 6)]                # y = CCAA: CC 7, CA 5
    assert rows[1] == [((3, -1, "+", "AA"), 12), ((7, 0, "+", "CC"), 6 + 8 + 6)]          # y = ACCA: AC, CC, CA
    assert rows[2] == [((3, -1, "+", "AA"), 8), ((7, 0, "+", "CC"), 6 + 8)]               # y = AACC: AC, CC
    assert [bf.changed(b"AAAA", o, 2, "CCCC") for o in range(4)] == [2, 2, 2, 0]
    assert bf.changed(b"AaCN", 0, 4, "AAAA") == 1 and bf.changed(b"acgt", 0, 4, "ACGT") == 0


def test_the_brute_force_on_an_n_inside_and_outside_the_block():
    """a substituted N stays an N and its windows stay at min_val; an N elsewhere leaves its windows there too"""
    (rows,) = _hand(b"ANnC", (2,), "CATG")
    assert rows[1] == [((0, -1, "+", "AN"), 3)] * 2 and bf.changed(b"ANnC", 1, 2, "CATG") == 0   # the block Nn is its own image
    assert rows[0] == [((0, 0, "+", "AN"), 2), ((0, 0, "+", "CN"), 2)]                  # y = CNnC: CN and Nn at min_val
    (rows,) = _hand(b"NACG", (2,), "CATG")
    assert rows[1] == [((9, 1, "+", "CG"), 1 + 6 + 10), ((7, 1, "+", "AG"), 1 + 6 + 8)]  # NA 0, AC 5, CG 9; y = NCAG: NC 0, CA 5, AG 7
    both = _hand(b"NACG", (1, 2), "CATG")                                                # a length's rows do not depend on the list
    assert both[1] == rows and both[0][0] == [((0, 0, "+", "NA"), 1)] * 2
    assert bf.substituted(b"NaCG", 0, 3, "CATG") == b"NCAG" and bf.substituted(b"acgt", 1, 2, "TGCA") == b"aGCt"


def test_the_brute_force_on_short_sequences():
    """n < W: a block fits and has no window on either side; n = L: the whole sequence is replaced; o + L > n: four zeros"""
    assert _hand(b"A", (1,), "CATG") == [[[(None, 0), (None, 0)]]]
    three, = _hand(b"ACG", (3,), "CATG")
    assert three[0] == [((9, 1, "+", "CG"), 6 + 10), ((9, 1, "+", "AT"), 6 + 10)]        # y = CAT: CA 5, AT 1 + 8
    assert three[1] == bf.NONE and three[2] == bf.NONE
    keys, sums = bf.scan_arrays([b"ACG", b"", b"A"], 2, SM, 0, WEIGHTS, True, (3, 4), "CATG")
    assert keys[0][1:] == [[0, 0]] * 3 and sums[0][1:] == [[0, 0]] * 3 and keys[1] == [[0, 0]] * 4 and sums[1] == [[0, 0]] * 4
    assert keys[0][0] == [bf.key_of((9, 1, "+"))] * 2 and sums[0][0] == [16, 16]
    assert _hand(b"", (1, 64), "CATG") == [[], []]


def test_keys_decode_for_every_start_of_both_sides():
    """every start the rule allows, at both ends and in the middle of a sequence, at the shortest and the longest length, encodes
    into 7 bits and decodes to itself; both sides have the same starts"""
    from grafimo_amd.query_variants import decode_keys
    from grafimo_amd.substitution_scan import COLUMNS as NAMES, MAX_LENGTH
    assert NAMES == ("COVER", "SUB") and MAX_LENGTH == 64
    for W in (1, 2, 19, 64):
        for L in (1, 7, 64):
            n = 2 * W + L + 3
            seen = set()
            for o in range(n - L + 1):
                for s in range(max(0, o - W + 1), min(o + L - 1, n - W) + 1):
                    for plus in (0, 1):
                        key = bf.key_of((64_000, s - o, "+" if plus else "-"))
                        assert 0 < key < 1 << 25
                        score, rel, strand = decode_keys(np.array([key]))
                        assert (int(score[0]), o + int(rel[0]), strand[0]) == (64_000, s, "+" if plus else "-")
                    seen.add(s - o)
            assert seen == set(range(-(W - 1), L)), (W, L)


def test_changed_bases_against_a_loop():
    from grafimo_amd.substitution_scan import changed_bases, checked_map, mapped_bases
    rng = np.random.default_rng(9)
    seqs = [b"", b"A", b"AAaA", b"ACACAC", b"ACCGTT", b"NNA", b""] + \
        [bytes(rng.choice(np.frombuffer(b"ACGTacgN", dtype=np.uint8), size=40).tolist()) for _ in range(6)]
    lengths = (1, 2, 3, 7, 40, 64)
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    flat = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    for letters in ("CATG", "AAAA", "ACTG", "ACGT"):
        got = changed_bases(off, flat, lengths, letters)
        want = [[bf.changed(x, o, L, letters) for x in seqs for o in range(len(x))] for L in lengths]
        assert got.shape == (len(lengths), int(off[-1])) and got.dtype == np.int32 and got.tolist() == want, letters
        assert mapped_bases(flat, letters).tobytes() == b"".join(bf.image(x.upper(), letters) for x in seqs)
        assert np.array_equal(changed_bases(off, flat, lengths, checked_map(letters)), got)
    assert not changed_bases(off, flat, lengths, "ACGT").any() and not changed_bases(off, flat, (64,), "CATG").any()
    assert (changed_bases(off, flat, (1,), "AAAA")[0] == 0).any() and changed_bases(off, flat, (40,), "CATG").max() > 30
    assert changed_bases([0], np.zeros(0, dtype=np.uint8), (1, 2), "CATG").shape == (2, 0)


LENGTHS = (1, 2, 3)


def _hand_table(W=3, threshold=0.5, fwd=False, lengths=LENGTHS, letters="CATG", **kw):
    """a SubstitutionScan over query_variant_bruteforce.hand_graph's regions whose arrays the brute force made -> (the table,
    the brute force's rows of all_rows)"""
    from oracle import oracle as orc
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.substitution_scan import SubstitutionScan
    idx = bf.hand_graph()
    regions = [(8, 14), (0, 20), (18, 20)]
    names = [f"c:{s}-{e}" for s, e in regions]
    m = SynMotif(W, seed=5)
    od = motif_as_oracle_dict(m)
    w, s_best = default_weights(m)
    log2_offset = -40 + (s_best / float(od["scale"]) + W * od["offset"])
    ptab = orc.p_table(od["pmf"])
    seqs = [bf.region_sequences(idx, s, e, [[1, 3]]) for s, e in regions]
    scans = [[bf.scan(d["bases"], W, od["score_matrix"], od["min_val"], w, fwd, lengths, letters) for d in region] for region in seqs]
    flat = [(r, d, sc) for r, (region, rs) in enumerate(zip(seqs, scans)) for d, sc in zip(region, rs)]
    coord = [~p if t else p for _, d, _ in flat for p, t in d["coords"][0]]
    keys = [[[bf.key_of(b) for b, _ in row] for _, _, sc in flat for row in sc[k]] for k in range(len(lengths))]
    sums = [[[s for _, s in row] for _, _, sc in flat for row in sc[k]] for k in range(len(lengths))]
    t = SubstitutionScan("M", "m", W, od["scale"], od["offset"], ptab, log2_offset, threshold, names, ["g"], [r for r, _, _ in flat],
                         [d["version"] for _, d, _ in flat], [d["count"] for _, d, _ in flat], [d["group_counts"] for _, d, _ in flat],
                         [d["is_reference"] for _, d, _ in flat], np.concatenate([[0], np.cumsum([len(d["bases"]) for _, d, _ in flat])]),
                         np.frombuffer(b"".join(d["bases"] for _, d, _ in flat), dtype=np.uint8), coord, lengths, letters,
                         np.array(keys, dtype=np.uint32).reshape(len(lengths), -1, 2),
                         np.array(sums, dtype=np.uint64).reshape(len(lengths), -1, 2), **kw)
    rows = bf.detail_rows(names, seqs, scans, lambda r, d: d["coords"][0], W, od["scale"], od["offset"], ptab, log2_offset, threshold,
                          lengths, letters)
    return t, rows


ROW_KEY = ("sequence_name", "version", "position", "inserted", "length", "replaced")


@pytest.mark.parametrize("letters", ["CATG", "AAAA"])
@pytest.mark.parametrize("W,fwd", [(2, False), (2, True), (19, False), (19, True)])
def test_frames_of_a_table_the_brute_force_filled(W, fwd, letters):
    t, rows = _hand_table(W, fwd=fwd, letters=letters, all_rows=True)
    frame = t.to_frame()
    assert list(frame.columns) == COLUMNS
    fitting = int((t.lengths[:, None] <= np.concatenate([np.arange(n, 0, -1) for n in np.diff(t.seq_offsets)])[None, :]).sum())
    assert len(frame) == len(rows) == len(t) and 0 < len(rows) <= fitting
    assert (len(rows) < fitting) == (letters == "AAAA")                                   # (blocks of A alone are no rows)
    for k, (f, e) in enumerate(zip(frame.to_dict("records"), rows)):
        assert [f["haplotypes_g"]] == e["groups"]
        for c in COLUMNS[2:5] + COLUMNS[6:]:
            assert _same(f[c], e[c]), (k, c, f[c], e[c], e)
    assert frame["inserted"].any() and frame["is_reference"].any() and not frame["is_reference"].all()
    assert set(frame["length"]) == set(LENGTHS) and frame["named"].any() and not frame["named"].all()
    assert (frame["replaced"].str.len() == frame["length"]).all() and (frame["replacement"].str.len() == frame["length"]).all()
    assert (frame["map"] == letters).all() and frame["changed"].min() >= 1
    assert (frame["changed"] == [sum(a != b for a, b in zip(p, q)) for p, q in zip(frame["replaced"], frame["replacement"])]).all()
    if letters == "AAAA":
        assert (frame["changed"] < frame["length"]).any() and set("".join(frame["replacement"])) == {"A"}
    if W == 19:                                                                          # [18, 20) and [8, 14) are shorter than W
        short = frame[frame["sequence_name"] != "c:0-20"]
        assert len(short) and short["alt_score"].isna().all() and (short["alt_kmer"] == "").all() and (short["effect"] == "none").all()
        assert frame["alt_score"].notna().any()
    # ---- the filter
    t.all_rows = False
    kept = [e for e in rows if e["effect"] in ("gain", "loss")]
    assert [tuple(f[c] for c in ROW_KEY) for f in t.to_frame().to_dict("records")] == [tuple(e[c] for c in ROW_KEY) for e in kept]
    t.delta = 0.75
    assert len(t.to_frame()) == len([e for e in rows if e["effect"] in ("gain", "loss") or abs(e["delta_log2_affinity"]) >= 0.75])
    # ---- the summary against a loop over the rows
    t.delta, t.all_rows = None, True
    want = bf.summary_rows(rows)
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
    t.all_rows = False
    assert len(t.summary_frame()) == sum(1 for w in want.values() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0)
    # ---- the dense arrays keep every cell
    assert t.keys.shape == (len(LENGTHS), len(t.bases), 2) and t.log2_affinity().shape == (len(LENGTHS), len(t.bases), 2)
    assert t.changed().shape == (len(LENGTHS), len(t.bases))


def test_named_on_the_hand_made_graph():
    """in [8, 14) haplotype 3 reads ACGGGTAC -- the G at 10 and two inserted behind it --, haplotype 2 reads ACAC, 10 and 11
    deleted: a block that holds an inserted base, or whose coordinates jump over the panel's deletion, is not named; every
    block that changes a base is a row of its own (rows are keyed by offset and length: there is no repeat rule)"""
    t, rows = _hand_table(3, all_rows=True)
    f = t.to_frame()
    f = f[f["sequence_name"] == "c:8-14"]
    v3 = f[f["version"] == 3]                                    # coordinates 8 9 10 ~10 ~10 11 12 13
    assert v3[v3["replaced"] == "G"][["position", "inserted", "named"]].values.tolist() == \
        [[11, False, True], [11, True, False], [11, True, False]]
    assert v3[v3["replaced"] == "GG"][["position", "inserted", "named", "replacement"]].values.tolist() == \
        [[11, False, False, "TT"], [11, True, False, "TT"]]
    assert v3[v3["replaced"] == "GGG"]["named"].tolist() == [False]
    assert v3[v3["replaced"] == "CG"]["named"].tolist() == [True] and v3[v3["replaced"] == "CGG"]["named"].tolist() == [False]
    assert v3[v3["replaced"] == "GT"][["inserted", "named"]].values.tolist() == [[True, False]]
    assert v3[v3["replaced"] == "TAC"][["named", "replacement", "changed"]].values.tolist() == [[True, "GCA", 3]]
    v2 = f[f["version"] == 2]                                    # ACAC: coordinates 8 9 12 13
    assert sorted(zip(v2["replaced"], v2["position"], v2["named"])) == \
        [("A", 9, True), ("A", 13, True), ("AC", 9, True), ("AC", 13, True), ("ACA", 9, False), ("C", 10, True), ("C", 14, True),
         ("CA", 10, False), ("CAC", 10, False)]
    every = t.named_blocks()
    a = int(t.seq_offsets[np.flatnonzero((t.seq_region == 0) & (t.seq_version == 2))[0]])
    assert every[:, a:a + 4].tolist() == [[True, True, True, True], [True, False, True, False], [False, False, False, False]]
    assert [bf.named([(8, False), (9, False), (12, False), (13, False)], o, 2) for o in range(4)] == [True, False, True, False]
    s = t.summary_frame()
    s = s[s["sequence_name"] == "c:8-14"]
    assert s[(s["position"] == 9) & (s["length"] == 2)]["versions"].tolist() == [4]
    assert s[(s["position"] == 10) & (s["length"] == 2)]["versions"].tolist() == [3]                 # AC, CA: not ACAC's C|A
    assert s[(s["position"] == 11) & (s["length"] == 2)]["versions"].tolist() == [2]                 # GT of the reference's two
    assert s[(s["position"] == 13) & (s["length"] == 2)]["versions"].tolist() == [4]
    # under AAAA the reference's block AC at 9 changes one base and ACAC's A at 9 none: the summary counts the blocks that change
    t, _ = _hand_table(3, letters="AAAA", all_rows=True)
    s = t.summary_frame()
    s = s[s["sequence_name"] == "c:8-14"]
    assert s[(s["position"] == 9) & (s["length"] == 1)]["versions"].tolist() == []
    assert s[(s["position"] == 9) & (s["length"] == 2)]["versions"].tolist() == [4]


def test_bad_maps_and_bad_lengths_are_value_errors():
    from grafimo_amd.substitution_scan import MAPS, SubstitutionScan, checked_map, compute_substitution_scan, map_letters, scan_sequences
    x = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    m = SynMotif(3, seed=1)
    assert MAPS == {"transversion": "CATG", "complement": "TGCA", "transition": "GTAC"}
    assert checked_map("transversion").tolist() == [1, 0, 3, 2] and checked_map("complement").tolist() == [3, 2, 1, 0]
    assert checked_map("transition").tolist() == [2, 3, 0, 1] and checked_map("aaaa").tolist() == [0, 0, 0, 0]
    assert checked_map("AcTg").tolist() == [0, 1, 3, 2] and checked_map("ACGT").dtype == np.uint8
    assert map_letters("complement") == "TGCA" and map_letters("catg") == "CATG"
    for bad in ("", "ACG", "ACGTA", "ACGU", "ACGN", "transversions", "Complement", None, 5, ("C", "A", "T", "G"), [1, 0, 3, 2],
                np.array([1, 0, 3, 4], dtype=np.uint8)):
        with pytest.raises(ValueError, match="base map"):
            checked_map(bad)
        with pytest.raises(ValueError, match="base map"):
            scan_sequences([m], [0, 8], x, (1, 2), bad)          # (before a motif is leased or the library called)
    with pytest.raises(ValueError, match="base map"):
        compute_substitution_scan(m, bf.hand_graph(), [(0, 20)], False, None, (1, 3), "ACGX")
    for bad, text in (((0,), "1 .. 64"), ((65,), "1 .. 64"), ((-3, 2), "1 .. 64"), ((2, 2), "strictly ascend"),
                      ((5, 3), "strictly ascend"), ((), "non-empty"), ((1.5,), "integers"), (((1, 2),), "non-empty list")):
        with pytest.raises(ValueError, match=text):
            scan_sequences([m], [0, 8], x, bad, "CATG")
    with pytest.raises(ValueError, match="strictly ascend"):
        compute_substitution_scan(m, bf.hand_graph(), [(0, 20)], False, None, (3, 1))
    with pytest.raises(ValueError, match="do not fit"):
        SubstitutionScan("M", "m", 3, 1, 0.0, [1.0], 0.0, 0.5, ["r"], [], [0], [0], [1], np.zeros((1, 0)), [True], [0, 8], x,
                         np.arange(8), (1, 2), "CATG", np.zeros((1, 8, 2)), np.zeros((1, 8, 2)))
    with pytest.raises(ValueError, match="base map"):
        SubstitutionScan("M", "m", 3, 1, 0.0, [1.0], 0.0, 0.5, ["r"], [], [0], [0], [1], np.zeros((1, 0)), [True], [0, 8], x,
                         np.arange(8), (1, 2), "CAT", np.zeros((2, 8, 2)), np.zeros((2, 8, 2)))


def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(flags),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, "-s", str(tmp_path), "--substitution-scan", "5")
    assert r.returncode != 0 and "--substitution-scan needs the graph" in r.stderr
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--substitution-all")
    assert r.returncode != 0 and "--substitution-all goes with --substitution-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--substitution-delta", "1.5")
    assert r.returncode != 0 and "--substitution-delta goes with --substitution-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--substitution-map", "complement")
    assert r.returncode != 0 and "--substitution-map goes with --substitution-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--substitution-scan", "5", "--substitution-delta", "-1")
    assert r.returncode != 0 and "--substitution-delta -1.0 is not >= 0" in r.stderr
    for bad in ("0", "65"):
        r = _cli(tmp_path, *graph, "--substitution-scan", "5", bad)
        assert r.returncode != 0 and f"--substitution-scan {bad}: a length lies in 1 .. 64" in r.stderr
    for bad in ("ACGU", "ACG", "scramble"):
        r = _cli(tmp_path, *graph, "--substitution-scan", "5", "--substitution-map", bad)
        assert r.returncode != 0 and "--substitution-map: base map" in r.stderr and bad in r.stderr
    r = _cli(tmp_path, *graph, "--substitution-scan")
    assert r.returncode != 0 and "expected at least one argument" in r.stderr
    r = _cli(tmp_path, "--help")
    assert r.returncode == 0
    for flag in ("--substitution-scan L [L ...]", "--substitution-map MAP", "--substitution-delta X", "--substitution-all"):
        assert flag in r.stdout, flag


def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    name = "gfm_sequence_substitution_scan"
    assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == 15
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert f"int {name}(" in header
    # before a device is touched: bad lengths, a bad map, an unknown flag and descending offsets are refused, no sequence is a no-op
    call = nv.lib().gfm_sequence_substitution_scan

    def entry(n_seqs, off, lengths, codes=(1, 0, 3, 2), flags=0):
        ln = np.array(lengths, dtype=np.int32)
        mp = None if codes is None else np.array(codes, dtype=np.uint8)
        return call(None, 1, None, 1, n_seqs, None if off is None else off.ctypes.data, None, len(ln), ln.ctypes.data,
                    None if mp is None else mp.ctypes.data, flags, None, None, None, None)
    assert entry(0, None, [1, 64]) == nv.GFM_OK
    assert entry(0, None, [1], flags=2) == nv.GFM_ERR_INVALID and b"unknown flag" in nv.lib().gfm_last_error()
    for bad, text in (([0], b"outside 1 .. 64"), ([65], b"outside 1 .. 64"), ([3, 3], b"strictly ascend"), ([4, 2], b"strictly ascend")):
        assert entry(0, None, bad) == nv.GFM_ERR_INVALID and text in nv.lib().gfm_last_error(), bad
    assert entry(0, None, [1], codes=None) == nv.GFM_ERR_INVALID and b"NULL base_map" in nv.lib().gfm_last_error()
    for k in range(4):
        codes = [0, 1, 2, 3]
        codes[k] = 4
        assert entry(0, None, [1], codes=codes) == nv.GFM_ERR_INVALID
        assert f"base_map[{k}] = 4 is outside 0 .. 3".encode() in nv.lib().gfm_last_error()
    assert entry(0, None, [1], codes=[0, 0, 0, 255]) == nv.GFM_ERR_INVALID
    for codes in ((0, 0, 0, 0), (0, 1, 2, 3), (3, 3, 3, 3)):
        assert entry(0, None, [1], codes=codes) == nv.GFM_OK
    mp = np.array([1, 0, 3, 2], dtype=np.uint8)
    assert call(None, 1, None, 1, 0, None, None, 1, None, mp.ctypes.data, 0, None, None, None, None) == nv.GFM_ERR_INVALID   # lengths NULL
    assert call(None, 1, None, 1, 0, None, None, 0, None, mp.ctypes.data, 0, None, None, None, None) == nv.GFM_ERR_INVALID   # no length
    assert entry(2, np.array([0, 5, 3], dtype=np.int64), [2]) == nv.GFM_ERR_INVALID and b"descends" in nv.lib().gfm_last_error()
    assert entry(1, np.array([0, 1 << 31], dtype=np.int64), [2]) == nv.GFM_ERR_INVALID and b"2^31" in nv.lib().gfm_last_error()
    assert entry(2, np.array([0, 0, 0], dtype=np.int64), [2]) == nv.GFM_OK
    assert entry(1, np.array([0, 4], dtype=np.int64), [2]) == nv.GFM_ERR_INVALID and b"NULL" in nv.lib().gfm_last_error()


def test_header_defines_the_constants_and_states_the_rule():
    import re
    from grafimo_amd import _native as nv
    from grafimo_amd import substitution_scan
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    for name in ("GFM_SUBSCAN_TILE", "GFM_SUBSCAN_MAX_LENGTH"):
        m = re.search(rf"#define {name} (\d+)", header)
        assert m and int(m.group(1)) == getattr(nv, name) == 64
    assert nv.GFM_SUBSCAN_MAX_LENGTH == nv.GFM_QUERY_MAX_ALLELE == nv.GFM_DELSCAN_MAX_LENGTH and nv.GFM_SUBSCAN_TILE == nv.GFM_DELSCAN_TILE
    kernel = open(os.path.join(ROOT, "grafimo_amd", "csrc", "gfm_graph_substitution_scan.hpp")).read()
    squeeze = lambda s: " ".join(s.replace("*", " ").replace("//", " ").split())                   # noqa: E731
    texts = [squeeze(header), squeeze(substitution_scan.__doc__), squeeze(bf.__doc__), squeeze(kernel)]
    for line in ("a base map f given as four codes -- the images of A, C, G, T, each in 0 .. 3 for A, C, G, T; any map is allowed: "
                 "fixed points, constant maps and the identity included --",
                 "If o + L > n there is no edit: both keys and both sums of the cell are 0.",
                 "Otherwise y = x[:o] + f(x[o:o+L]) + x[o+L:]. f is applied base by base. Case is folded, as base_code does.",
                 "A base that is not A/C/G/T maps to itself: unlike a deletion, a substituted N is NOT repaired.",
                 "rule with lr = la = L at offset o, the alleles not trimmed.",
                 "REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o + L - 1, n - W).",
                 "This is bit for bit the deletion scan's COVER column.",
                 "ALT side (column SUB): the same starts in y.",
                 "Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY",
                 "A window that holds a base that is not A/C/G/T scores min_val on both strands.",
                 "((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. L - 1 on both sides",
                 "Key 0 means the side has no window.",
                 "Per column, the exact uint64 sum of w[score] over the side's windows and strands.",
                 "Under the identity map SUB == COVER in every cell.",
                 "At L = 1, wherever x[o] is a base, SUB equals the mutation scan's column of the base f(x[o]), field for field."):
        for text in texts:
            assert line in text, line
    # the kernel's header states the table of the four cases and why a difference word may wrap
    for line in ("Full[s] - D(o, m) + D(o + L, m + L)", "Full'[s] - D(o, m)", "Full[s] + D(o + L, L - d)", "exact modulo 2^32"):
        assert line in squeeze(kernel), line
