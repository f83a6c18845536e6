"""The site distance without a GPU: THE RULE's greedy loops (tests/site_distance_bruteforce.py) against an exhaustive minimiser
that knows nothing of gains, the word codec, cutoff_of against a loop, the frames and the histogram of a table whose arrays the
brute force made, the export, the header and the library's refusals, which return before anything is launched."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import site_distance_bruteforce as bf  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_g", "is_reference", "position", "inserted",
           "strand", "kmer", "score", "pvalue", "kind", "distance", "reached", "changes", "edited_kmer", "edited_score", "edited_pvalue"]


def _summary_columns(E):
    return (["motif_id", "motif_alt_id", "sequence_name", "position", "strand", "versions", "haplotypes", "haplotypes_site"] +
            [f"haplotypes_near_{k}" for k in range(1, E + 1)] + ["haplotypes_far", "min_site_distance", "best_score"])


def _same(x, y):
    return x == y or (x != x and y != y)


# ------------------------------------------------------------------------------------------- the rule against the minimiser
@pytest.mark.parametrize("W", [1, 2, 3, 4, 5])
def test_greedy_equals_the_exhaustive_minimiser(W):
    """d and the score after, on both strands and both sides, for random motifs and sequences with N and lower case, at the
    cutoffs 0, mid and 1000 W + 1 and two more: the exchange argument is not taken on trust"""
    rng = np.random.default_rng(8100 + W)
    seen = set()
    for trial in range(3):
        od = motif_as_oracle_dict(SynMotif(W, seed=810 + 10 * W + trial))
        sm, mv = od["score_matrix"], od["min_val"]
        tabs = bf.strand_tables(sm, W)
        assert mv <= int(sm.min(axis=0).sum())                   # (no score lies under min_val: rule 2 of the fragile side)
        x = bytearray(rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), size=26).tobytes())
        for at in rng.choice(26, size=3, replace=False).tolist():
            x[at] = ord("N") if at % 2 else ord("n")
        lo, hi = int(sm.min(axis=0).sum()), int(sm.max(axis=0).sum())
        for E in (1, 2, 3):
            for c in (0, (lo + hi) // 2, (lo + 3 * hi) // 4, hi, 1000 * W + 1):
                for s in range(len(x) - W + 1):
                    codes = bf.window_codes(bytes(x[s:s + W]))
                    for t in tabs:
                        d, after, picks = bf.raise_window(codes, t, mv, c, E)
                        assert (d, after) == bf.exhaustive(codes, t, mv, c, E, True), (W, E, c, s)
                        assert len(picks) == min(d, E) or (d == E + 1 and len(picks) < E)
                        seen.add(("near", d))
                        fd, fafter, fpicks = bf.lower_window(codes, t, mv, c, E)
                        if None in codes:                        # the rule's own case: no picks
                            assert (fd, fafter, fpicks) == (0 if mv < c else E + 1, mv, [])
                        else:
                            assert (fd, fafter) == bf.exhaustive(codes, t, mv, c, E, False), (W, E, c, s)
                        seen.add(("fragile", fd))
    want = min(W, 3)
    assert {("near", d) for d in range(want + 1)} <= seen and {("fragile", d) for d in range(want + 1)} <= seen and ("near", 4) in seen


def test_the_rule_on_a_motif_read_by_hand():
    """W = 4: two identical columns, a constant column, a column with two equal best entries (rows A, C, G, T)"""
    sm = np.array([[10, 10, 5, 9], [2, 2, 5, 9], [3, 3, 5, 1], [7, 7, 5, 0]])
    tp, tm = bf.strand_tables(sm, 4)
    assert tp == [[10, 2, 3, 7], [10, 2, 3, 7], [5, 5, 5, 5], [9, 9, 1, 0]]
    assert tm == [[0, 1, 9, 9], [5, 5, 5, 5], [7, 3, 2, 10], [7, 3, 2, 10]]          # - : the matrix at (3 - b, W - 1 - j)
    codes = bf.window_codes(b"ccAt")                             # + : 2 + 2 + 5 + 0 = 9; gains 8, 8, 0, 9
    assert bf.score_of(codes, tp, 0) == 9
    assert bf.raise_window(codes, tp, 0, 18, 3) == (1, 18, [(3, 0)])                  # column 4 gets A, the first of A and C
    assert bf.raise_window(codes, tp, 0, 19, 3) == (2, 26, [(3, 0), (0, 0)])          # then the leftmost of the equal gains
    assert bf.raise_window(codes, tp, 0, 35, 3) == (4, 34, [(3, 0), (0, 0), (1, 0)])  # the constant column is never picked
    assert bf.raise_window(codes, tp, 0, 35, 8) == (9, 34, [(3, 0), (0, 0), (1, 0)])  # every remaining gain is 0
    assert bf.raise_window(codes, tp, 0, 9, 3) == (0, 9, [])
    # AACA scores 34 with the losses 8, 8, 0, 9: the largest goes first and takes T, the worst base; then the leftmost 8
    assert bf.lower_window(bf.window_codes(b"AACA"), tp, 0, 30, 2) == (1, 25, [(3, 3)])
    assert bf.lower_window(bf.window_codes(b"AACA"), tp, 0, 26, 2) == (1, 25, [(3, 3)])
    assert bf.lower_window(bf.window_codes(b"AACA"), tp, 0, 10, 2) == (3, 17, [(3, 3), (0, 1)])
    assert bf.lower_window(bf.window_codes(b"AACA"), tp, 0, 35, 2) == (0, 34, [])
    # non-base columns: repaired from the left, the score stays min_val until the last one is
    codes = bf.window_codes(b"NnAt")
    assert bf.raise_window(codes, tp, 1, 2, 1) == (2, 1, [(0, 0)])
    assert bf.raise_window(codes, tp, 1, 2, 2) == (2, 25, [(0, 0), (1, 0)])
    assert bf.raise_window(codes, tp, 1, 26, 3) == (3, 34, [(0, 0), (1, 0), (3, 0)])
    assert bf.raise_window(codes, tp, 1, 1, 3) == (0, 1, [])                          # min_val itself reaches the cutoff
    assert bf.lower_window(codes, tp, 1, 1, 3) == (4, 1, []) and bf.lower_window(codes, tp, 1, 2, 3) == (0, 1, [])
    words, masks = bf.scan_arrays([b"NnAt", b"AC"], 4, sm, 1, 26, 3, True)
    assert words[0] == [1, bf.NO_WINDOW, (34 << 4) | 3, bf.NO_WINDOW, (1 << 4) | 0, bf.NO_WINDOW] and masks[0] == [0b1011, 0, 0, 0]
    assert words[1:] == [[bf.NO_WINDOW] * 6] * 5 and masks[1:] == [[0] * 4] * 5


# ------------------------------------------------------------------------------------------- the module's helpers
def test_word_codec():
    from grafimo_amd.site_distance import MASK_COLUMNS, NO_WINDOW, WORD_COLUMNS, decode_words, own_scores
    assert NO_WINDOW == bf.NO_WINDOW == 0xFFFFFFFF and len(WORD_COLUMNS) == 6 and len(MASK_COLUMNS) == 4
    scores = np.array([0, 1, 999, 64_000, 64_000], dtype=np.int64)
    ds = np.array([0, 9, 4, 1, 9], dtype=np.int64)
    words = ((scores << 4) | ds).astype(np.uint32)
    d, sc = decode_words(words)
    assert d.tolist() == ds.tolist() and sc.tolist() == scores.tolist() and d.dtype == np.int64
    d, sc = decode_words(np.array([[NO_WINDOW, 0x12]], dtype=np.uint32))
    assert d.tolist() == [[-1, 2]] and sc.tolist() == [[-1, 1]]
    assert own_scores(np.array([0, 64_000, NO_WINDOW], dtype=np.uint32)).tolist() == [0, 64_000, -1]
    assert int(words.max()) < NO_WINDOW                          # (no score and d collide with "no window")


def test_cutoff_of_against_a_loop():
    from grafimo_amd.site_distance import cutoff_of

    def loop(p, thr):
        for s, v in enumerate(p):
            if v < thr:
                return s
        return len(p)
    rng = np.random.default_rng(3)
    for W in (1, 3):
        p = np.sort(rng.random(1000 * W + 1))[::-1].copy()
        p[0] = 1.0
        for thr in (2.0, 1.0, 0.5, float(p[700]), float(p[-1]), 0.0, 1e-300):
            assert cutoff_of(p, thr) == loop(p, thr), (W, thr)
        assert cutoff_of(p, float(p[700])) == 701                # strict <: the score whose p equals the threshold is no site
        assert cutoff_of(p, 0.0) == 1000 * W + 1 == cutoff_of(p, float(p[-1]))       # no such score
        assert cutoff_of(p, 2.0) == 0


def test_strand_tables_are_the_brute_forces():
    from grafimo_amd.site_distance import strand_tables
    for W in (1, 4, 19):
        m = SynMotif(W, seed=31)
        got = strand_tables(m)
        tp, tm = bf.strand_tables(motif_as_oracle_dict(m)["score_matrix"], W)
        assert got.shape == (2, W, 4) and got[0].tolist() == tp and got[1].tolist() == tm


# ------------------------------------------------------------------------------------------- the frames
def _hand_table(W=3, threshold=0.5, fwd=False, E=2, **kw):
    """a SiteDistance over query_variant_bruteforce.hand_graph's regions whose arrays the brute force made -> (the table, the
    brute force's rows of all_rows)"""
    from oracle import oracle as orc
    from grafimo_amd.site_distance import SiteDistance, cutoff_of, strand_tables
    idx = bf.hand_graph()
    regions = [(8, 14), (0, 20), (18, 20)]
    names = [f"c:{s}-{e}" for s, e in regions]
    m = SynMotif(W, seed=5)
    od = motif_as_oracle_dict(m)
    ptab = orc.p_table(od["pmf"])
    cutoff = cutoff_of(ptab, threshold)
    seqs = [bf.region_sequences(idx, s, e, [[1, 3]]) for s, e in regions]
    scans = [[bf.scan(d["bases"], W, od["score_matrix"], od["min_val"], cutoff, E, fwd) for d in region] for region in seqs]
    flat = [d for region in seqs for d in region]
    coord = [~p if t else p for d in flat for p, t in d["coords"][0]]
    words, masks = bf.scan_arrays([d["bases"] for d in flat], W, od["score_matrix"], od["min_val"], cutoff, E, fwd)
    t = SiteDistance("M", "m", W, od["scale"], od["offset"], ptab, strand_tables(m), cutoff, E, threshold, names, ["g"],
                     [r for r, region in enumerate(seqs) for _ in region], [d["version"] for d in flat], [d["count"] for d in flat],
                     [d["group_counts"] for d in flat], [d["is_reference"] for d in flat],
                     np.concatenate([[0], np.cumsum([len(d["bases"]) for d in flat])]),
                     np.frombuffer(b"".join(d["bases"] for d in flat), dtype=np.uint8), coord,
                     np.array(words, dtype=np.uint32).reshape(-1, 6), np.array(masks, dtype=np.uint64).reshape(-1, 4), **kw)
    rows = bf.detail_rows(names, seqs, scans, lambda r, d: d["coords"][0], W, od["scale"], od["offset"], ptab, cutoff, E)
    return t, rows


ROW_KEY = ("sequence_name", "version", "position", "inserted", "strand")


def check_frames(t, rows, label=""):
    """every column of every detail row, the default filter, the summary against a loop over the rows and the histogram against
    a count over them (shared with the GPU tests)"""
    E = t.max_edits
    t.all_rows = True
    frame = t.to_frame()
    assert len(frame) == len(rows) == len(t), label
    for k, (f, e) in enumerate(zip(frame.to_dict("records"), rows)):
        for c in ("sequence_name", "version", "haplotypes", "is_reference", "position", "inserted", "strand", "kmer", "score", "pvalue",
                  "kind", "distance", "reached", "changes", "edited_kmer", "edited_score", "edited_pvalue"):
            assert _same(f[c], e[c]), (label, k, c, f[c], e[c], e)
        assert [f[f"haplotypes_{g}"] for g in t.group_names] == e["groups"], (label, k)
    # ---- the default filter: the sites and the near-sites
    t.all_rows = False
    kept = [e for e in rows if e["kind"] != "far"]
    assert [tuple(f[c] for c in ROW_KEY) for f in t.to_frame().to_dict("records")] == [tuple(e[c] for c in ROW_KEY) for e in kept], label
    assert len(t) == len(kept)
    # ---- the summary against a loop over the detail rows
    t.all_rows = True
    want = bf.summary_of(rows, E)
    s = t.summary_frame()
    assert list(s.columns) == _summary_columns(E) and len(s) == len(want), label
    names = {n_: k for k, n_ in enumerate(t.region_names.tolist())}
    keys = [(f["sequence_name"], f["position"], f["strand"]) for f in s.to_dict("records")]
    assert keys == sorted(want, key=lambda q: (names[q[0]], q[1], "+-".index(q[2]))), label
    for f in s.to_dict("records"):
        w = want[(f["sequence_name"], f["position"], f["strand"])]
        assert (f["versions"], f["haplotypes"], f["haplotypes_site"], f["haplotypes_far"]) == \
            (w["versions"], w["haplotypes"], w["haplotypes_site"], w["haplotypes_far"]), (label, f)
        assert [f[f"haplotypes_near_{k}"] for k in range(1, E + 1)] == w["near"], (label, f)
        assert _same(f["min_site_distance"], float(min(w["site_distances"])) if w["site_distances"] else np.nan), (label, f)
        assert _same(f["best_score"], max(w["scores"])), (label, f)
    t.all_rows = False
    kept = {q for q, w in want.items() if w["haplotypes_site"] + sum(w["near"]) > 0}
    assert {(f["sequence_name"], f["position"], f["strand"]) for f in t.summary_frame().to_dict("records")} == kept, label
    t.all_rows = True
    # ---- the histogram against a count over the rows: the near side every window-strand, the fragile side the sites
    hist = t.distance_histogram()
    assert hist.shape == (len(t.seq_count), 2, E + 2) and hist.dtype == np.int64
    seq_of = {(t.region_names[t.seq_region[q]], int(t.seq_version[q])): q for q in range(len(t.seq_count))}
    want_h = np.zeros_like(hist)
    for e in rows:
        q = seq_of[(e["sequence_name"], e["version"])]
        want_h[q, 0, e["near_d"]] += 1
        if e["kind"] == "site":
            want_h[q, 1, e["fragile_d"]] += 1
    assert np.array_equal(hist, want_h), label
    n, st = t._window_strands()
    d_near = (t.words[n, 2 + st] & 15).astype(np.int64)
    assert np.array_equal(hist[:, 0], np.stack([np.bincount(d_near[t.base_sequence[n] == q], minlength=E + 2)
                                                for q in range(len(t.seq_count))]).reshape(-1, E + 2)), label
    return frame


@pytest.mark.parametrize("W,fwd,E,threshold", [(2, False, 1, 0.3), (3, False, 2, 0.2), (3, True, 3, 0.3), (5, False, 8, 0.2),
                                               (19, False, 2, 0.5)])
def test_frames_of_a_table_the_brute_force_filled(W, fwd, E, threshold):
    t, rows = _hand_table(W, threshold, fwd, E, all_rows=True)
    frame = check_frames(t, rows, (W, fwd, E))
    assert list(frame.columns) == COLUMNS
    assert set(frame["strand"]) == ({"+"} if fwd else {"+", "-"})
    if W == 19:                                                  # [8, 14) and [18, 20) are shorter than the motif: no rows
        assert set(frame["sequence_name"]) == {"c:0-20"}
        return
    assert frame["inserted"].any() and frame["is_reference"].any() and not frame["is_reference"].all()
    assert {"site", "near"} <= set(frame["kind"])
    near = frame[frame["kind"] == "near"]
    assert (near["changes"].str.count(",") + 1 == near["distance"]).all() and near["reached"].all()
    assert (frame[frame["distance"] == 0]["changes"] == "").all()
    assert (frame[frame["distance"] == 0]["edited_kmer"] == frame[frame["distance"] == 0]["kmer"]).all()
    # a printed change names the forward offset and forward bases: applying it to the forward window gives edited_kmer
    comp = str.maketrans("ACGT", "TGCA")
    for f in frame.to_dict("records"):
        k = f["kmer"] if f["strand"] == "+" else f["kmer"].translate(comp)[::-1]
        y = list(k)
        for piece in filter(None, f["changes"].split(",")):
            at, swap = piece.split(":")
            assert y[int(at) - 1] == swap[0] and swap[1] == ">" and swap[2] in "ACGT" and swap[2] != swap[0]
            y[int(at) - 1] = swap[2]
        y = "".join(y)
        assert f["edited_kmer"] == (y if f["strand"] == "+" else y.translate(comp)[::-1])


def test_table_refuses_arrays_that_do_not_fit():
    from grafimo_amd.site_distance import SiteDistance, checked_edits
    x = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    tabs = np.zeros((2, 3, 4))
    ok = dict(words=np.zeros((8, 6)), masks=np.zeros((8, 4)))
    SiteDistance("M", "m", 3, 1, 0.0, [1.0], tabs, 0, 3, 0.5, ["r"], [], [0], [0], [1], np.zeros((1, 0)), [True], [0, 8], x, np.arange(8), **ok)
    for bad in (dict(ok, words=np.zeros((8, 5))), dict(ok, masks=np.zeros((7, 4)))):
        with pytest.raises(ValueError, match="do not fit"):
            SiteDistance("M", "m", 3, 1, 0.0, [1.0], tabs, 0, 3, 0.5, ["r"], [], [0], [0], [1], np.zeros((1, 0)), [True], [0, 8], x,
                         np.arange(8), **bad)
    for bad in (0, 9, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_edits"):
            checked_edits(bad)
    assert [checked_edits(e) for e in (1, 8, np.int64(3))] == [1, 8, 3]


# ------------------------------------------------------------------------------------------- the command line's refusals
def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(flags),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, "-s", str(tmp_path), "--site-distance", "2")
    assert r.returncode != 0 and "--site-distance needs the graph" in r.stderr
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--site-distance-all")
    assert r.returncode != 0 and "--site-distance-all goes with --site-distance" in r.stderr
    for bad in ("0", "9", "-1"):
        r = _cli(tmp_path, *graph, "--site-distance", bad)
        assert r.returncode != 0 and "--site-distance" in r.stderr and "1 .. 8" in r.stderr, bad
    r = _cli(tmp_path, "--help")
    assert r.returncode == 0
    for flag in ("--site-distance [E]", "--site-distance-all"):
        assert flag in r.stdout, flag
    assert r.stdout.count("--site-distance") >= 4                # its own two entries and the --haplotype-groups help texts


# ------------------------------------------------------------------------------------------- the export and the header
def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    name = "gfm_sequence_site_distance"
    assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == 12
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert re.search(r"#define GFM_ABI_VERSION 12\b", header)
    proto = re.search(rf"int {name}\(([^;]*)\);", header)
    assert proto
    args = [a.strip() for a in " ".join(proto.group(1).split()).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["motifs", "n_motifs", "n_seqs", "seq_offsets", "d_bases", "cutoffs", "max_edits",
                                                         "flags", "d_words", "d_masks", "d_status", "stream"]
    ctype = {"int32_t": nv.c_i32, "uint32_t": ctypes.c_uint32}
    for a, have in zip(args, nv.PROTOTYPES[name][1]):
        want = nv.c_void_p if "*" in a else ctype[a.split()[0]]
        assert have is want, a
    for const in ("GFM_SITEDIST_TILE", "GFM_SITEDIST_MAX_EDITS"):
        m = re.search(rf"#define {const} (\d+)", header)
        assert m and int(m.group(1)) == getattr(nv, const)
    assert nv.GFM_SITEDIST_TILE == nv.GFM_MUTSCAN_TILE == 64 and nv.GFM_SITEDIST_MAX_EDITS == 8


def test_library_refuses_before_a_launch():
    """through ctypes, with no device buffer at all: every call returns before a motif handle or a device is touched"""
    from grafimo_amd import _native as nv
    call, err = nv.lib().gfm_sequence_site_distance, nv.lib().gfm_last_error

    def entry(n_motifs=1, n_seqs=0, off=None, cutoffs=(0,), E=3, flags=0):
        cut = None if cutoffs is None else np.array(cutoffs, dtype=np.int32)
        return call(None, n_motifs, n_seqs, None if off is None else off.ctypes.data, None, None if cut is None else cut.ctypes.data,
                    E, flags, None, None, None, None)
    assert entry() == nv.GFM_OK
    assert entry(n_motifs=0) == nv.GFM_ERR_INVALID and b"n_motifs < 1" in err()
    assert entry(n_seqs=-1) == nv.GFM_ERR_INVALID and b"n_seqs < 0" in err()
    assert entry(flags=2) == nv.GFM_ERR_INVALID and b"unknown flag" in err()
    for bad in (0, 9, -1, 1 << 30):                              # checked with no sequence too
        assert entry(E=bad) == nv.GFM_ERR_INVALID and f"max_edits {bad} is outside 1 .. 8".encode() in err(), bad
    for good in (1, 8):
        assert entry(E=good) == nv.GFM_OK
    assert entry(cutoffs=None) == nv.GFM_ERR_INVALID and b"NULL cutoffs" in err()
    for bad in (-1, 64_002, 1 << 30):                            # no width allows them: refused without the motifs
        assert entry(cutoffs=(bad,)) == nv.GFM_ERR_INVALID and f"cutoff {bad} of motif 0".encode() in err(), bad
    assert entry(n_motifs=2, cutoffs=(5, -7)) == nv.GFM_ERR_INVALID and b"cutoff -7 of motif 1" in err()
    assert entry(cutoffs=(64_001,)) == nv.GFM_OK and entry(n_motifs=3, cutoffs=(0, 1001, 64_001)) == nv.GFM_OK
    assert entry(n_seqs=2) == nv.GFM_ERR_INVALID and b"NULL" in err()
    assert entry(n_seqs=2, off=np.array([0, 5, 3], dtype=np.int64)) == nv.GFM_ERR_INVALID and b"descends at sequence 1" in err()
    assert entry(n_seqs=1, off=np.array([-2, 5], dtype=np.int64)) == nv.GFM_ERR_INVALID and b"below 0" in err()
    assert entry(n_seqs=1, off=np.array([0, 1 << 31], dtype=np.int64)) == nv.GFM_ERR_INVALID and b"2^31" in err()
    assert entry(n_seqs=2, off=np.array([0, 0, 0], dtype=np.int64)) == nv.GFM_OK
    assert entry(n_seqs=1, off=np.array([0, 4], dtype=np.int64)) == nv.GFM_ERR_INVALID and b"NULL" in err()
    assert entry(n_seqs=1, off=np.array([0, 4], dtype=np.int64), E=9) == nv.GFM_ERR_INVALID and b"max_edits" in err()


def test_the_rule_stands_in_the_same_words_in_four_places():
    from grafimo_amd import site_distance
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    kernel = open(os.path.join(ROOT, "grafimo_amd", "csrc", "gfm_graph_site_distance.hpp")).read()
    squeeze = lambda s: " ".join(s.replace("*", " ").replace("//", " ").split())                   # noqa: E731
    texts = [squeeze(header), squeeze(kernel), squeeze(site_distance.__doc__), squeeze(bf.__doc__)]
    doc = squeeze(bf.__doc__)
    rule = doc[doc.index("Inputs: a sequence x of n bases"):doc.index("packed table at the same forward column.") + 40]
    assert len(rule) > 2000 and rule.endswith("packed table at the same forward column.")
    for text in texts:
        assert rule in text
    for line in ("a cutoff c in 0 .. 1000 W + 1; a cap E in 1 .. 8", "3. If a non-base column remains, the next pick is the leftmost such column.",
                 "Ties go to the leftmost column.", "5. If every remaining gain is 0, stop with d = E + 1.",
                 "2. A window with a non-base column takes no picks: d = 0 if min_val < c, otherwise d = E + 1.",
                 "By the exchange argument d is the true minimum whenever it is <= E."):
        assert line in rule, line
    # the kernel's header says how it is cut and that nothing lands in scratch; the include line is behind the substitution scan's
    for line in ("a halo of W - 1 BEHIND them", "one packed subtraction each that cannot borrow", "nothing lands in scratch",
                 "no atomics but the status word's"):
        assert line in squeeze(kernel), line
    extract = open(os.path.join(ROOT, "grafimo_amd", "csrc", "graph_extract.hip")).read()
    assert extract.index('#include "gfm_graph_substitution_scan.hpp"') < extract.index('#include "gfm_graph_site_distance.hpp"')
