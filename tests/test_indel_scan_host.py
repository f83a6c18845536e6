"""The indel scan without a GPU: the key encoding of the four kinds of side, the leftmost-duplicate filter, the frames of a
table whose arrays the brute force made (tests/indel_scan_bruteforce.py), the command line's refusals, the export and the
header."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import indel_scan_bruteforce as bf  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_g", "is_reference", "position", "inserted",
           "type", "base", "ref_score", "ref_pvalue", "ref_start", "ref_strand", "ref_kmer", "alt_score", "alt_pvalue", "alt_start",
           "alt_strand", "alt_kmer", "ref_log2_affinity", "alt_log2_affinity", "delta_log2_affinity", "effect"]
SUMMARY_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "type", "base", "versions", "haplotypes", "haplotypes_gain",
                   "haplotypes_loss", "min_delta_log2_affinity", "max_delta_log2_affinity", "best_alt_score"]


def _same(x, y):
    return x == y or (x != x and y != y)


def _starts(kind, o, n, W):
    """the rule's starts of a side, and what a key's rel is relative to"""
    if kind == "COVER":
        return range(max(0, o - W + 1), min(o, n - W) + 1), o
    if kind == "DEL":
        return range(max(0, o - W + 1), min(o - 1, n - 1 - W) + 1), o
    if kind == "JUNCTION":
        return range(max(0, o + 1 - W + 1), min(o, n - W) + 1), o + 1
    return range(max(0, o + 1 - W + 1), min(o + 1, n + 1 - W) + 1), o + 1


def test_keys_decode_for_every_start_of_the_four_kinds_of_side():
    """every start the rule allows, at both ends and in the middle of a sequence, encodes into 7 bits and decodes to itself:
    the start is o + REL_ANCHOR[column] + rel"""
    from grafimo_amd.indel_scan import COLUMNS as NAMES, REL_ANCHOR
    from grafimo_amd.query_variants import decode_keys
    assert NAMES == ("COVER", "DEL", "JUNCTION", "INS_A", "INS_C", "INS_G", "INS_T")
    for W in (1, 2, 19, 64):
        n = 2 * W + 3
        seen = {k: set() for k in ("COVER", "DEL", "JUNCTION", "INS_A")}
        for o in range(n):
            for col, kind in ((0, "COVER"), (1, "DEL"), (2, "JUNCTION"), (3, "INS_A")):
                starts, anchor = _starts(kind, o, n, W)
                assert anchor == o + REL_ANCHOR[col]
                for s in starts:
                    for plus in (0, 1):
                        key = bf.key_of((64_000, s - anchor, "+" if plus else "-"))
                        assert 0 < key < 1 << 25
                        score, rel, strand = decode_keys(np.array([key]))
                        assert (int(score[0]), o + int(REL_ANCHOR[col]) + int(rel[0]), strand[0]) == (64_000, s, "+" if plus else "-")
                    seen[kind].add(s - anchor)
        assert seen["COVER"] == set(range(-(W - 1), 1)) and seen["INS_A"] == set(range(-(W - 1), 1))
        assert seen["DEL"] == set(range(-(W - 1), 0)) and seen["JUNCTION"] == set(range(-(W - 1), 0))
    # the order of the keys is the rule's: score descending, start ascending, + before -
    order = sorted([(5, -1, "+"), (5, -1, "-"), (5, 0, "+"), (6, 0, "-"), (4, -63, "+")], key=bf.key_of, reverse=True)
    assert order == [(6, 0, "-"), (5, -1, "+"), (5, -1, "-"), (5, 0, "+"), (4, -63, "+")]
    assert REL_ANCHOR[4:].tolist() == [1, 1, 1]


def test_the_brute_force_follows_the_rule_on_a_sequence_read_by_hand():
    """W = 2, + only, w[s] = s + 1, on ACN and ANC: an N leaves its windows at min_val, a deleted N repairs one, the insertion
    behind the last base has one window, and W - 1 bases have only the insertions' windows"""
    sm = np.array([[1, 2], [3, 4], [5, 6], [7, 8]])              # rows A, C, G, T
    w = np.arange(100, dtype=np.uint64) + 1
    rows = bf.scan(b"ACN", 2, sm, 0, w, True)
    assert rows[0][0] == ((5, 0, "+", "AC"), 6) and rows[0][1] == (None, 0)      # deleting A: no window starts before it
    assert rows[0][2] == ((5, -1, "+", "AC"), 6) and rows[0][3] == ((5, 0, "+", "AC"), 4 + 6)      # y = AACN: AA 3, AC 5
    assert rows[1][1] == ((0, -1, "+", "AN"), 1)                                 # deleting C: AN
    assert rows[2][0] == ((0, -1, "+", "CN"), 1) and rows[2][1] == (None, 0)     # y = AC: no window crosses its end
    assert rows[2][2] == (None, 0) and rows[2][3] == ((0, -1, "+", "NA"), 1)     # y = ACNA
    mid = bf.scan(b"AnC", 2, sm, 0, w, True)[1]
    assert mid[0] == ((0, -1, "+", "An"), 2) and mid[1] == ((5, -1, "+", "AC"), 6)                 # An and nC; y = AC
    one = bf.scan(b"G", 2, sm, 0, w, True)                       # n = W - 1
    assert [c[0] for c in one[0][:3]] == [None, None, None] and one[0][3] == ((5 + 2, -1, "+", "GA"), 8)
    assert bf.scan(b"", 2, sm, 0, w, True) == []


def test_the_leftmost_duplicate_filter_against_a_loop():
    from grafimo_amd.indel_scan import leftmost_changes
    rng = np.random.default_rng(9)
    seqs = [b"", b"A", b"AAaA", b"ACCGTT", b"NNA", b""] + [bytes(rng.choice(np.frombuffer(b"ACGTacgN", dtype=np.uint8), size=40).tolist())
                                                         for _ in range(6)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    got = leftmost_changes(off, np.frombuffer(b"".join(seqs), dtype=np.uint8))
    want, made = [], 0
    for x in seqs:
        spelled = {}
        for o in range(len(x)):
            want.append([bf.reported(x, o, kind, b) for kind, b in bf.CHANGES])
            # and the reason: a change that is reported spells a y no earlier offset of the sequence spells
            for (kind, b), keep in zip(bf.CHANGES, want[-1]):
                y = (x[:o] + x[o + 1:] if kind == "DEL" else x[:o + 1] + bytes([b]) + x[o + 1:]).upper()
                assert keep == ((kind, y) not in spelled), (x, o, kind, b)
                spelled.setdefault((kind, y), o)
                made += 1
    assert got.shape == (len(want), 5) and got.tolist() == want
    assert made == 5 * int(off[-1]) and not got.all() and got[:, 0].any() and not got[:, 1:].all(axis=0).any()
    assert leftmost_changes([0], np.zeros(0, dtype=np.uint8)).shape == (0, 5)


def _hand_table(W=3, threshold=0.5, fwd=False, **kw):
    """an IndelScan over query_variant_bruteforce.hand_graph's regions whose arrays the brute force made -> (the table, the
    brute force's rows of all_rows)"""
    from oracle import oracle as orc
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.indel_scan import IndelScan
    idx = bf.hand_graph()
    regions = [(8, 14), (0, 20), (18, 20)]
    names = [f"c:{s}-{e}" for s, e in regions]
    m = SynMotif(W, seed=5)
    od = motif_as_oracle_dict(m)
    w, s_best = default_weights(m)
    log2_offset = -40 + (s_best / float(od["scale"]) + W * od["offset"])
    ptab = orc.p_table(od["pmf"])
    seqs = [bf.region_sequences(idx, s, e, [[1, 3]]) for s, e in regions]
    scans = [[bf.scan(d["bases"], W, od["score_matrix"], od["min_val"], w, fwd) for d in region] for region in seqs]
    flat = [(r, d, sc) for r, (region, rs) in enumerate(zip(seqs, scans)) for d, sc in zip(region, rs)]
    coord = [~p if t else p for _, d, _ in flat for p, t in d["coords"][0]]
    t = IndelScan("M", "m", W, od["scale"], od["offset"], ptab, log2_offset, threshold, names, ["g"], [r for r, _, _ in flat],
                  [d["version"] for _, d, _ in flat], [d["count"] for _, d, _ in flat], [d["group_counts"] for _, d, _ in flat],
                  [d["is_reference"] for _, d, _ in flat], np.concatenate([[0], np.cumsum([len(d["bases"]) for _, d, _ in flat])]),
                  np.frombuffer(b"".join(d["bases"] for _, d, _ in flat), dtype=np.uint8), coord,
                  np.array([[bf.key_of(b) for b, _ in row] for _, _, sc in flat for row in sc], dtype=np.uint32).reshape(-1, 7),
                  np.array([[s for _, s in row] for _, _, sc in flat for row in sc], dtype=np.uint64).reshape(-1, 7), **kw)
    rows = bf.detail_rows(names, seqs, scans, lambda r, d: d["coords"][0], W, od["scale"], od["offset"], ptab, log2_offset, threshold)
    return t, rows


@pytest.mark.parametrize("W,fwd", [(3, False), (2, True), (7, False)])
def test_frames_of_a_table_the_brute_force_filled(W, fwd):
    t, rows = _hand_table(W, fwd=fwd, all_rows=True)
    frame = t.to_frame()
    assert list(frame.columns) == COLUMNS
    assert len(frame) == len(rows) == len(t) and len(rows) < 5 * len(t.bases)       # (the homopolymer GGG of haplotype 3)
    for k, (f, e) in enumerate(zip(frame.to_dict("records"), rows)):
        assert [f["haplotypes_g"]] == e["groups"]
        for c in COLUMNS[2:5] + COLUMNS[6:]:
            assert _same(f[c], e[c]), (k, c, f[c], e[c], e)
    assert frame["inserted"].any() and frame["is_reference"].any() and not frame["is_reference"].all()
    assert set(frame["type"]) == {"DEL", "INS"} and set(frame[frame["type"] == "INS"]["base"]) == set("ACGT")
    if W == 3:
        assert {"gain", "loss"} <= set(frame["effect"]), set(frame["effect"])
    if W == 7:                                                                          # [18, 20) is shorter than W - 1
        short = frame[frame["sequence_name"] == "c:18-20"]
        assert short["alt_score"].isna().all() and (short["alt_kmer"] == "").all() and (short["effect"] == "none").all()
    # ---- the filter
    t.all_rows = False
    kept = [e for e in rows if e["effect"] in ("gain", "loss")]
    assert [(f["sequence_name"], f["version"], f["position"], f["inserted"], f["type"], f["base"]) for f in t.to_frame().to_dict("records")] == \
        [(e["sequence_name"], e["version"], e["position"], e["inserted"], e["type"], e["base"]) for e in kept]
    t.delta = 0.75
    assert len(t.to_frame()) == len([e for e in rows if e["effect"] in ("gain", "loss") or abs(e["delta_log2_affinity"]) >= 0.75])
    # ---- the summary against a loop over the detail rows
    t.delta, t.all_rows = None, True
    want = bf.summary_of(frame.to_dict("records"))
    s = t.summary_frame()
    assert list(s.columns) == SUMMARY_COLUMNS and len(s) == len(want)
    for f in s.to_dict("records"):
        w = want[(f["sequence_name"], f["position"], f["type"], f["base"])]
        assert (f["versions"], f["haplotypes"], f["haplotypes_gain"], f["haplotypes_loss"]) == \
            (w["versions"], w["haplotypes"], w["haplotypes_gain"], w["haplotypes_loss"]), f
        assert _same(f["min_delta_log2_affinity"], min(w["deltas"]) if w["deltas"] else np.nan)
        assert _same(f["max_delta_log2_affinity"], max(w["deltas"]) if w["deltas"] else np.nan)
        assert _same(f["best_alt_score"], max(w["scores"]) if w["scores"] else np.nan)
    keys = [(t.region_names.tolist().index(f["sequence_name"]), f["position"], f["type"], f["base"]) for f in s.to_dict("records")]
    assert keys == sorted(keys)
    t.all_rows = False
    assert len(t.summary_frame()) == sum(1 for w in want.values() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0)
    # ---- the dense arrays keep every cell
    assert t.keys.shape == (len(t.bases), 7) and t.log2_affinity().shape == (len(t.bases), 7)


def test_a_homopolymer_is_reported_at_its_leftmost_offset():
    """haplotype 3 of the hand-made graph reads ACGGGTAC in [8, 14), the G at 10 and two inserted behind it (position 11): of
    the three deletions of a G the frames hold the first; the four ways to spell ACGGGGTAC are one row, the insertion of G
    behind the C; and behind every base but the first the insertion of that base again is the row of the offset before"""
    t, rows = _hand_table(3, all_rows=True)
    f = t.to_frame()
    v3 = f[(f["sequence_name"] == "c:8-14") & (f["version"] == 3)]
    assert len(v3) == 5 * 8 - 2 - 7
    g = v3[v3["base"] == "G"]
    assert sorted(zip(g["type"], g["position"], g["inserted"])) == \
        [("DEL", 11, False)] + [("INS", p, False) for p in (9, 10, 12, 13, 14)]
    assert len(t.keys) == len(t.bases) and (t.keys[:, 3:] > 0).all()             # the dense arrays keep every cell


def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(flags),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, "-s", str(tmp_path), "--indel-scan")
    assert r.returncode != 0 and "--indel-scan needs the graph" in r.stderr
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--indel-all")
    assert r.returncode != 0 and "--indel-all goes with --indel-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--indel-delta", "1.5")
    assert r.returncode != 0 and "--indel-delta goes with --indel-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--indel-scan", "--indel-delta", "-1")
    assert r.returncode != 0 and "--indel-delta -1.0 is not >= 0" in r.stderr
    r = _cli(tmp_path, "--help")
    assert r.returncode == 0 and r.stdout.count("--indel-scan") >= 5            # its own options and the two lists it joined


def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    name = "gfm_sequence_indel_scan"
    assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == 12
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert f"int {name}(" in header
    # before a device is touched: no sequence is a no-op, an unknown flag and descending offsets are refused
    lib = nv.lib()
    assert lib.gfm_sequence_indel_scan(None, 1, None, 1, 0, None, None, 0, None, None, None, None) == nv.GFM_OK
    assert lib.gfm_sequence_indel_scan(None, 1, None, 1, 0, None, None, 2, None, None, None, None) == nv.GFM_ERR_INVALID
    off = np.array([0, 5, 3], dtype=np.int64)
    assert lib.gfm_sequence_indel_scan(None, 1, None, 1, 2, off.ctypes.data, None, 0, None, None, None, None) == nv.GFM_ERR_INVALID
    assert b"descends" in lib.gfm_last_error()
    off = np.array([0, 0, 0], dtype=np.int64)
    assert lib.gfm_sequence_indel_scan(None, 1, None, 1, 2, off.ctypes.data, None, 0, None, None, None, None) == nv.GFM_OK


def test_header_defines_the_tile_and_states_the_rule():
    import re
    from grafimo_amd import _native as nv
    from grafimo_amd import indel_scan
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    m = re.search(r"#define GFM_INDELSCAN_TILE (\d+)", header)
    assert m and int(m.group(1)) == nv.GFM_INDELSCAN_TILE and 1 <= nv.GFM_INDELSCAN_TILE
    squeeze = lambda s: " ".join(s.replace("*", " ").split())                   # noqa: E731
    texts = [squeeze(header), squeeze(indel_scan.__doc__), squeeze(bf.__doc__)]
    for line in ("Deletion of x[o]. y = x[:o] + x[o+1:].",
                 "rule with lr = 1, la = 0 at offset o.",
                 "REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).",
                 "ALT side (column DEL): the starts of y across the junction, max(0, o - W + 1) <= s <= min(o - 1, n - 1 - W).",
                 "Insertion of b in A, C, G, T behind x[o]. y = x[:o+1] + b + x[o+1:].",
                 "This is the query rule with lr = 0, la = 1 at offset o' = o + 1.",
                 "REF side (column JUNCTION): the starts of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).",
                 "ALT side (columns INS_A, INS_C, INS_G, INS_T): the starts of y with max(0, o' - W + 1) <= s <= min(o', n + 1 - W).",
                 "A window that holds a base that is not A/C/G/T scores min_val on both strands.",
                 "Case is folded, as base_code does.",
                 "((score + 1) << 8) | ((64 - rel) << 1) | plus, rel = s - o for COVER and DEL, rel = s - (o + 1) for JUNCTION and INS_ :",
                 "Key 0 means the side has no window.",
                 "Per column, the exact uint64 sum of w[score] over the side's windows and strands.",
                 "A deleted N can repair its windows. An N elsewhere leaves its windows at min_val.",
                 "An insertion before the first base of a sequence is not scanned",
                 "An empty sequence has no rows."):
        for text in texts:
            assert line in text, line
