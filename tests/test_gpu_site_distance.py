"""The site distance on the GPU: the kernel through scan_sequences against THE RULE restated in Python loops
(tests/site_distance_bruteforce.py) at the tile's edges, on a motif made by hand for the tie rules, against the mutation scan's
kernel at E = 1, the table and both frames against the brute force on the hand-made graph and three fuzz graphs, the refusals
and the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import site_distance_bruteforce as bf  # noqa: E402
import test_gpu_mutation_scan as ms  # noqa: E402  (its graphs, its regions, its motif widths)
import test_site_distance_host as host  # noqa: E402  (check_frames)
import wide_panel_cases as wp  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
THRESHOLD = ms.THRESHOLD
CAPS = (2, 3, 3, 8)                                              # the cap E of each graph of ms.GRAPHS


def _tile():
    from grafimo_amd import _native as nv
    return nv.GFM_SITEDIST_TILE


# ------------------------------------------------------------------------------------------- the kernel through scan_sequences
def _lengths(W, T):
    """in this order: window starts and empty sequences between others"""
    return [0, 1, W - 1, W, W + 1, T - 1, T, T + 1, T + W - 1, 2 * T + 3]


def _sequences(W, T, rng):
    """random sequences of _lengths with lower-case bases and N: at offsets 0 and n - 1, inside a tile's halo (behind the edge:
    the windows that start in the tile before it read it), at a tile's last offset, and a cluster of five in the longest
    sequence, so that windows hold one, two and more than three non-base columns"""
    seqs = []
    for n in _lengths(W, T):
        x = bytearray(BASES[rng.integers(0, 4, size=n)].tobytes())
        for j in np.flatnonzero(rng.random(n) < 0.15).tolist():
            x[j] |= 0x20
        if n == T + 1:
            x[0] = ord("N")
            x[n - 1] = ord("n")                                  # the second tile's only base
        if n == T + W - 1 and W > 2:
            x[T + W // 2 - 1] = ord("N")                         # behind the edge, inside the first tile's halo
        if n == 2 * T + 3:
            x[T + W // 2] = ord("N")                             # behind the first edge, inside the first tile's halo
            x[2 * T - 1] = ord("N")                              # the last offset of the second tile
            x[n - 1] = ord("N")
            for j in range(20, 30, 2):
                x[j] = ord("n") if j % 4 else ord("N")
        if n == W + 1:
            x[0] = ord("N")                                      # one window holds it, one does not
        seqs.append(bytes(x))
    return seqs


def _brute(seqs, od, cutoff, E, fwd):
    return bf.scan_arrays(seqs, od["width"], od["score_matrix"], od["min_val"], cutoff, E, fwd)


def _distances(words):
    """the d of every window-strand of the brute force's words -> (near set, fragile set)"""
    near = {w[c] & 15 for w in words for c in (2, 3) if w[c] != bf.NO_WINDOW}
    frag = {w[c] & 15 for w in words for c in (4, 5) if w[c] != bf.NO_WINDOW}
    return near, frag


@functools.lru_cache(maxsize=None)
def _kernel_case(W, n_motifs, seed):
    """-> (sequences, motifs, cutoffs, offsets, bases).  The cutoffs are chosen on the CPU: a quantile of the windows' own
    scores; at W >= 19 the first of a few quantiles at which the brute force shows, with E = 3, every d in 0 .. 4 on both sides"""
    rng = np.random.default_rng(seed)
    T = _tile()
    seqs = _sequences(W, T, rng)
    motifs = [SynMotif(W, seed=seed + 11 * k) for k in range(n_motifs)]
    cutoffs = []
    for m in motifs:
        od = motif_as_oracle_dict(m)
        own = sorted(w[c] for w in _brute(seqs, od, 0, 1, False)[0] for c in (0, 1) if w[c] != bf.NO_WINDOW)
        picks = [own[int(q * (len(own) - 1))] for q in (0.6, 0.5, 0.7, 0.4, 0.8, 0.3, 0.9)]
        if W >= 19 and n_motifs <= 2:
            picks = [c for c in picks if _distances(_brute(seqs, od, c, 3, False)[0]) == (set(range(5)), set(range(5)))]
            assert picks, (W, m.motif_id)
        cutoffs.append(int(picks[0]))
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    return seqs, motifs, cutoffs, off, np.frombuffer(b"".join(seqs), dtype=np.uint8)


def _check_kernel(W, n_motifs, seed, E, fwd, cutoffs=None):
    from grafimo_amd.site_distance import scan_sequences
    seqs, motifs, chosen, off, bases = _kernel_case(W, n_motifs, seed)
    cutoffs = chosen if cutoffs is None else cutoffs
    got = scan_sequences(motifs, off, bases, cutoffs, max_edits=E, forward_only=fwd)
    assert len(got) == n_motifs
    for m in range(n_motifs):
        words, masks = _brute(seqs, motif_as_oracle_dict(motifs[m]), cutoffs[m], E, fwd)
        assert got[m][0].shape == (len(bases), 6) and got[m][0].dtype == np.uint32
        assert got[m][1].shape == (len(bases), 4) and got[m][1].dtype == np.uint64
        assert got[m][0].tolist() == words, (W, E, fwd, m, np.argwhere(got[m][0] != np.array(words, dtype=np.uint32))[:5].tolist())
        assert got[m][1].tolist() == masks, (W, E, fwd, m, np.argwhere(got[m][1] != np.array(masks, dtype=np.uint64))[:5].tolist())
        if W > 1:
            assert any(w[0] == bf.NO_WINDOW for w in words) and any(w[0] != bf.NO_WINDOW for w in words)
        assert all((w[1] == bf.NO_WINDOW) == (fwd or w[0] == bf.NO_WINDOW) for w in words)
    return got


@pytest.mark.parametrize("fwd", [False, True])
@pytest.mark.parametrize("E", [1, 3, 8])
@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_kernel_against_brute_force(W, E, fwd):
    """all six words and all four masks of every base, exactly, for two motifs of one width (grid.y)"""
    got = _check_kernel(W, 2, 81_000 + W, E, fwd)
    assert not np.array_equal(got[0][0], got[1][0])              # (two motifs, two answers)


@pytest.mark.parametrize("W", [19, 64])
def test_the_kernel_cases_hold_every_distance_and_every_count_of_non_bases(W):
    """with the brute force alone, at E = 3: every d in 0 .. E + 1 on both sides, and windows with one, two and more than E
    non-base columns"""
    seqs, motifs, cutoffs, _, _ = _kernel_case(W, 2, 81_000 + W)
    for m, c in zip(motifs, cutoffs):
        near, frag = _distances(_brute(seqs, motif_as_oracle_dict(m), c, 3, False)[0])
        assert near == {0, 1, 2, 3, 4} and frag == {0, 1, 2, 3, 4}, (W, near, frag)
    holes = {sum(ch in b"Nn" for ch in x[s:s + W]) for x in seqs for s in range(len(x) - W + 1)}
    assert {0, 1, 2} <= holes and max(holes) > 3, holes
    T = _tile()
    long = seqs[-1]
    assert long[T + W // 2] == ord("N") and long[2 * T - 1] == ord("N") and long[0] != ord("N") and seqs[7][0] == ord("N")
    assert any(ch in b"acgt" for ch in long)


@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_cutoff_zero_and_a_cutoff_nothing_reaches(W):
    """cutoff 0: every window is a site (near d = 0 everywhere); cutoff 1000 W + 1: nothing reaches it (near d = E + 1, fragile
    d = 0 everywhere) -- one motif each, in one call"""
    got = _check_kernel(W, 2, 81_000 + W, 3, False, cutoffs=[0, 1000 * W + 1])
    some = got[0][0][:, 0] != bf.NO_WINDOW
    assert some.any() and ((got[0][0][some][:, 2:4] & 15) == 0).all() and not got[0][1][some][:, :2].any()
    assert ((got[1][0][some][:, 2:4] & 15) == 4).all() and ((got[1][0][some][:, 4:6] & 15) == 0).all()
    assert not got[1][1][some][:, 2:].any()


# ------------------------------------------------------------------------------------------- a motif made by hand
def _hand_motif():
    """W = 4 (rows A, C, G, T): columns 1 and 2 identical, column 3 constant, column 4 with two equal best entries"""
    m = SynMotif(4, seed=3)
    sm = np.array([[10, 10, 5, 9], [2, 2, 5, 9], [3, 3, 5, 1], [7, 7, 5, 0]])
    m.score_matrix = np.asarray(sm, dtype=np.asarray(m.score_matrix).dtype).reshape(np.asarray(m.score_matrix).shape)
    m.min_val = int(sm.min())                                    # (what the library asks of a motif: the smallest entry)
    m.motif_id, m.motif_name = "HAND", "hand"
    return m, sm


def test_tie_rules_on_a_motif_made_by_hand():
    """equal gains: the leftmost column; a zero-gain column: never picked; equal best entries: the first of A, C, G, T"""
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.site_distance import SiteDistance, decode_words, scan_sequences, strand_tables
    m, sm = _hand_motif()
    assert strand_tables(m)[0].tolist() == bf.strand_tables(sm, 4)[0]
    x = b"ccAtAACA"                                              # windows ccAt .. AACA
    bases = np.frombuffer(x, dtype=np.uint8)
    # ccAt scores 9 with the gains 8, 8, 0, 9: the picks are column 4 (18), column 1 (26), column 2 (34); AACA scores 34 with the
    # losses 8, 8, 0, 9: column 4 (25), column 1 (17), column 2 (9)
    for c, E, near, mask, frag_last in ((18, 3, (1, 18), 0b1000, (2, 17)), (19, 3, (2, 26), 0b1001, (2, 17)),
                                        (35, 3, (4, 34), 0b1011, (0, 34)), (35, 8, (9, 34), 0b1011, (0, 34)),
                                        (26, 2, (2, 26), 0b1001, (1, 25)), (10, 2, (1, 18), 0b1000, (3, 17))):
        words, masks = scan_sequences([m], [0, 8], bases, [c], max_edits=E, forward_only=True)[0]
        want_w, want_m = bf.scan_arrays([x], 4, sm, m.min_val, c, E, True)
        assert words.tolist() == want_w and masks.tolist() == want_m, (c, E)
        d, after = decode_words(words[0, 2])
        assert (int(d), int(after)) == near and int(masks[0, 0]) == mask, (c, E)
        assert not int(masks[0, 0]) & 0b0100 and not int(masks[4, 2]) & 0b0100      # the constant column
        d, after = decode_words(words[4, 4])
        assert (int(d), int(after)) == frag_last, (c, E)
    # the printed change: column 4 gets A, not C; the site AACA loses T at column 4 first, then C at the leftmost column
    dm = DeviceMotif.lease(m)
    try:
        ptab = dm.ptable_host()
    finally:
        dm.release()
    words, masks = scan_sequences([m], [0, 8], bases, [19], max_edits=2, forward_only=True)[0]
    t = SiteDistance("HAND", "hand", 4, int(m.scale), float(m.offset), ptab, strand_tables(m), 19, 2, 0.5, ["r"], [], [0], [0], [1],
                     np.zeros((1, 0)), [True], [0, 8], bases, np.arange(8), words, masks, all_rows=True)
    f = t.to_frame()
    assert f["kmer"].tolist() == ["CCAT", "CATA", "ATAA", "TAAC", "AACA"]
    first, last = f.iloc[0], f.iloc[4]
    assert (first["kind"], first["distance"], first["changes"], first["edited_kmer"]) == ("near", 2, "1:C>A,4:T>A", "ACAA")
    words, masks = scan_sequences([m], [0, 8], bases, [10], max_edits=2, forward_only=True)[0]
    t = SiteDistance("HAND", "hand", 4, int(m.scale), float(m.offset), ptab, strand_tables(m), 10, 2, 0.5, ["r"], [], [0], [0], [1],
                     np.zeros((1, 0)), [True], [0, 8], bases, np.arange(8), words, masks, all_rows=True)
    last = t.to_frame().iloc[4]
    assert (last["kind"], last["distance"], bool(last["reached"]), last["changes"], last["edited_kmer"]) == \
        ("site", 3, False, "1:A>C,4:A>T", "CACT")


# ------------------------------------------------------------------------------------------- motif count and repeats
def test_seventeen_motifs_take_two_launches():
    got = _check_kernel(2, 17, 82_000, 3, False)
    assert len({g[0].tobytes() for g in (got[0], got[15], got[16])}) == 3


def test_a_second_call_and_empty_input():
    """a second identical call gives identical arrays (every row is written, nothing is left from the first); no base gives
    empty arrays"""
    from grafimo_amd.site_distance import scan_sequences
    seqs, motifs, cutoffs, off, bases = _kernel_case(19, 2, 81_019)
    one = scan_sequences(motifs, off, bases, cutoffs, max_edits=3)
    two = scan_sequences(motifs, off, bases, cutoffs, max_edits=3)
    for a, b in zip(one, two):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    none = scan_sequences(motifs, [0, 0, 0], np.zeros(0, dtype=np.uint8), cutoffs)
    assert len(none) == 2 and all(w.shape == (0, 6) and k.shape == (0, 4) for w, k in none)
    assert none[0][0].dtype == np.uint32 and none[0][1].dtype == np.uint64


# ------------------------------------------------------------------------------------------- against the existing kernel
@pytest.mark.parametrize("fwd", [False, True])
@pytest.mark.parametrize("W", [5, 19])
def test_the_e_1_corner_is_the_mutation_scan(W, fwd):
    """no N, cutoff 1000 W + 1, E = 1: every near word is own + the largest gain, and the largest of those scores over a
    sequence's windows and strands is the largest ALT score of mutation_scan.scan_sequences over every (offset, column)"""
    from grafimo_amd.mutation_scan import scan_sequences as mutation_scan
    from grafimo_amd.query_variants import decode_keys
    from grafimo_amd.site_distance import decode_words, own_scores, scan_sequences, strand_tables
    rng = np.random.default_rng(83_000 + W)
    T = _tile()
    seqs = [BASES[rng.integers(0, 4, size=n)].tobytes() for n in (T + W + 9, 2 * W + 3, W)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    motifs = [SynMotif(W, seed=830 + k) for k in range(2)]
    got = scan_sequences(motifs, off, bases, [1000 * W + 1] * 2, max_edits=1, forward_only=fwd)
    scan = mutation_scan(motifs, off, bases, forward_only=fwd)
    col = np.zeros(256, dtype=np.int64)
    col[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)
    for m in range(2):
        tabs = strand_tables(motifs[m])
        words = got[m][0]
        for v, x in enumerate(seqs):
            a, n = int(off[v]), len(x)
            codes = col[np.frombuffer(x, dtype=np.uint8)]
            best = -1
            for st in range(1 if fwd else 2):
                t = tabs[st]
                for s in range(n - W + 1):
                    entries = t[np.arange(W), codes[s:s + W]]
                    own, gain = int(entries.sum()), int((t.max(axis=1) - entries).max())
                    assert int(own_scores(words[a + s, st])) == own
                    d, after = decode_words(words[a + s, 2 + st])
                    assert (int(d), int(after)) == (2, own + gain), (W, fwd, m, v, s, st)
                    best = max(best, own + gain)
            alt = decode_keys(scan[m][0][a:a + n, 1:])[0]
            assert int(alt.max()) == best, (W, fwd, m, v)


# ------------------------------------------------------------------------------------------- the table against the brute force
@functools.lru_cache(maxsize=None)
def _sequences_of(name):
    idx, regions, motifs, groups, fwd = ms._setup(name)
    return [bf.region_sequences(idx, S, E, list(groups.values())) for S, E in regions]


def _scans(name, od, cutoff, E, fwd):
    return [[bf.scan(d["bases"], od["width"], od["score_matrix"], od["min_val"], cutoff, E, fwd) for d in region]
            for region in _sequences_of(name)]


@pytest.mark.parametrize("name", ms.GRAPHS)
def test_table_against_the_brute_force(name):
    from grafimo_amd.site_distance import compute_site_distance_many, cutoff_of
    idx, regions, motifs, groups, fwd = ms._setup(name)
    E = CAPS[ms.GRAPHS.index(name)]
    seqs = _sequences_of(name)
    tables = compute_site_distance_many(motifs, idx, regions, False, wp.Args(threshold=THRESHOLD, no_reverse=fwd),
                                        haplotype_groups=groups, max_edits=E, all_rows=True)
    n_bases = sum(len(d["bases"]) for region in seqs for d in region)
    for t, m in zip(tables, motifs):
        od = motif_as_oracle_dict(m)
        W = od["width"]
        assert (t.motif_id, t.width, t.group_names, t.max_edits, t.threshold) == (m.motif_id, W, list(groups), E, THRESHOLD)
        assert t.cutoff == cutoff_of(t.ptable, THRESHOLD) and 0 < t.cutoff <= 1000 * W     # (the device's tail table, as the siblings read it)
        scans = _scans(name, od, t.cutoff, E, fwd)
        # ---- the sequences are the mutation scan's; the dense arrays against the loops
        assert len(t.seq_count) == sum(len(region) for region in seqs) and len(t.bases) == n_bases
        for r, region in enumerate(seqs):
            mine = np.flatnonzero(t.seq_region == r)
            order = sorted(mine.tolist(), key=lambda q: (t.seq_version[q] < 0, t.seq_version[q]))
            assert [(int(t.seq_version[q]), int(t.seq_count[q]), t.seq_group_counts[q].tolist(), bool(t.seq_is_reference[q]),
                     t.bases[t.seq_offsets[q]:t.seq_offsets[q + 1]].tobytes()) for q in order] == \
                [(d["version"], d["count"], d["group_counts"], d["is_reference"], d["bases"]) for d in region], (name, r)
            for q, d in zip(order, region):
                a, b = int(t.seq_offsets[q]), int(t.seq_offsets[q + 1])
                words, masks = bf.scan_arrays([d["bases"]], W, od["score_matrix"], od["min_val"], t.cutoff, E, fwd)
                assert t.words[a:b].tolist() == words and t.masks[a:b].tolist() == masks, (name, m.motif_id, r, d["version"])

        def coords_of(r, d):
            q = [int(q) for q in np.flatnonzero(t.seq_region == r) if int(t.seq_version[q]) == d["version"]]
            assert len(q) == 1, (name, r, d["version"])
            have = [(int(~c) if c < 0 else int(c), bool(c < 0)) for c in t.coord[t.seq_offsets[q[0]]:t.seq_offsets[q[0] + 1]].tolist()]
            assert have in d["coords"], (name, r, d["version"])
            return have
        rows = bf.detail_rows(t.region_names, seqs, scans, coords_of, W, od["scale"], od["offset"], t.ptable, t.cutoff, E)
        frame = host.check_frames(t, rows, (name, m.motif_id))
        assert list(frame.columns) == host.COLUMNS[:5] + [f"haplotypes_{g}" for g in groups] + host.COLUMNS[6:]
        assert (frame["motif_id"] == m.motif_id).all() and (frame["motif_alt_id"] == m.motif_name).all()
        assert len(frame) == sum(len(windows) * (1 if fwd else 2) for region in scans for windows in region)


def test_the_graphs_hold_every_case():
    """with the brute force alone (the oracle's tail table gives the cutoff): inserted window starts, a count-0 reference
    sequence, sequences shorter than the motif, sites, near-sites at d = 1 and d >= 2, a fragile d of 1"""
    from oracle import oracle as orc
    from grafimo_amd.site_distance import cutoff_of
    inserted = added = short = sites = near1 = near2 = frag1 = 0
    for k, name in enumerate(ms.GRAPHS):
        idx, regions, motifs, groups, fwd = ms._setup(name)
        seqs = _sequences_of(name)
        for m in motifs:
            od = motif_as_oracle_dict(m)
            cutoff = cutoff_of(orc.p_table(od["pmf"]), THRESHOLD)
            for region, scans in zip(seqs, _scans(name, od, cutoff, CAPS[k], fwd)):
                added += int(region[-1]["version"] < 0)
                for d, sc in zip(region, scans):
                    short += int(len(d["bases"]) < od["width"])
                    inserted += sum(int(t) for _, t in d["coords"][0][:len(sc)])
                    for strands in sc:
                        for res in strands:
                            site = res["own"] >= cutoff
                            sites += int(site)
                            near1 += int(not site and res["near"][0] == 1)
                            near2 += int(not site and 2 <= res["near"][0] <= CAPS[k])
                            frag1 += int(site and res["fragile"][0] == 1)
    assert min(inserted, added, short, sites, near1, near2, frag1) >= 1, (inserted, added, short, sites, near1, near2, frag1)


# ------------------------------------------------------------------------------------------- refusals, command line
def test_refusals(monkeypatch):
    from grafimo_amd import _native as nv
    from grafimo_amd.site_distance import compute_site_distance, scan_sequences
    x = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)
    m5, m7 = SynMotif(5, seed=1), SynMotif(7, seed=2)
    m5.motif_id = "FIVE"
    with pytest.raises(nv.NativeError, match="one width"):
        scan_sequences([m5, m7], [0, 12], x, [100, 100])
    for bad in (0, 9):
        with pytest.raises(ValueError, match="max_edits"):
            scan_sequences([m5], [0, 12], x, [100], max_edits=bad)
        lib_rc = nv.lib().gfm_sequence_site_distance(None, 1, 0, None, None, np.array([100], dtype=np.int32).ctypes.data, bad, 0, None,
                                                     None, None, None)
        assert lib_rc == nv.GFM_ERR_INVALID and b"max_edits" in nv.lib().gfm_last_error()
    for bad in (-1, 5002):
        with pytest.raises(nv.NativeError, match=f"cutoff {bad} of motif 1"):
            scan_sequences([m5, m5], [0, 12], x, [5001, bad])
    with pytest.raises(nv.NativeError, match="cutoff 5002 of motif 0 is outside 0 .. 5001"):
        scan_sequences([m5], [0, 0], np.zeros(0, dtype=np.uint8), [5002])          # with no base too
    scan_sequences([m5], [0, 12], x, [5001])
    with pytest.raises(ValueError, match="FIVE: .* 672 bytes, more than max_bytes = 671"):
        scan_sequences([m5], [0, 12], x, [100], max_bytes=671)
    both = scan_sequences([m5, m5], [0, 12], x, [100, 100], max_bytes=672)                       # one motif at a time
    assert np.array_equal(both[0][0], both[1][0]) and np.array_equal(both[0][1], scan_sequences([m5], [0, 12], x, [100])[0][1])
    with pytest.raises(ValueError, match="starts at 0"):
        scan_sequences([m5], [1, 12], x, [100])
    with pytest.raises(ValueError, match="2 cutoffs for 1 motifs"):
        scan_sequences([m5], [0, 12], x, [100, 100])
    import torch
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="the site distance is computed on one GPU"):
        compute_site_distance(m5, bf.hand_graph(), [(0, 20)], False, wp.Args())


def test_cli_writes_both_files(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.site_distance import compute_site_distance_many
    from grafimo_amd.workflow import Findmotif
    fa, vcf, bedfile = os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), os.path.join(GOLD, "regions.bed")
    bed = read_bed_regions(bedfile)
    graphs = [GraphIndex.from_fasta_vcf(fa, vcf, c[3:]) for c in bed]
    out = str(tmp_path / "o")
    r = subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", fa, "-v", vcf, "-b", bedfile,
                        "-t", "0.05", "-o", out, "--site-distance", "2"], check=True, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=600, capture_output=True, text=True)
    assert "site distance rows written to" in r.stdout and "site distance summary rows written to" in r.stdout
    wf = Findmotif(threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "MA0139.1.meme"), wf, 2, True, pvalue_matrix=False)[0]
    t = compute_site_distance_many([motif], graphs, list(bed.values()), False, wp.Args(threshold=0.05), max_edits=2)[0]
    detail = open(os.path.join(out, "grafimo_site_distance.tsv")).read()
    summary = open(os.path.join(out, "grafimo_site_distance_summary.tsv")).read()
    assert detail.split("\n", 1)[0].split("\t") == [c for c in host.COLUMNS if c != "haplotypes_g"]
    assert summary.split("\n", 1)[0].split("\t") == host._summary_columns(2)
    assert len(t) > 0 and detail == t.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    assert len(t.summary_frame()) > 0 and summary == t.summary_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    assert set(t.to_frame()["kind"]) <= {"site", "near"} and t.max_edits == 2
