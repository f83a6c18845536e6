"""The substitution scan on the GPU: the kernel through scan_sequences against the brute force
(tests/substitution_scan_bruteforce.py) at the tile's edges, its COVER column against the deletion scan's, the identity map,
length 1 against the mutation scan, against the query-variant kernel on the same block substitutions, the table and both frames
against the brute force on the graphs test_gpu_mutation_scan.py uses, the refusals and the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import substitution_scan_bruteforce as bf  # noqa: E402
import test_gpu_deletion_scan as dst  # noqa: E402  (its sequence family: the sizes and the Ns at a tile's edges)
import test_gpu_mutation_scan as mst  # noqa: E402  (its graphs, regions, motifs and default weights)
import wide_panel_cases as wp  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = mst.GOLD
BASES = mst.BASES
GRAPHS = mst.GRAPHS
THRESHOLD = mst.THRESHOLD
TABLE_LENGTHS = (1, 3, 10)
TABLE_MAP = "CATG"
LETTER = {ord(c): k for k, c in enumerate("ACGT")}


def _tile():
    from grafimo_amd import _native as nv
    return nv.GFM_SUBSCAN_TILE


def _lengths(W):
    return (1, 64) if W == 64 else (1, 2, 7, 64)


def _case(W, n_motifs=2, seed=None):
    """the deletion test's sequences for the tile T = 64 -- the sizes 0, 1, W - 1, W, W + 1, 63, 64, 65, W + 63, W + 64, T - 1,
    T, T + 1, T + W - 1, 2 T + 3, lower-case bases, an N at offset 0, at the last offset, just before and just behind a tile
    edge and inside the right halo --, motifs and weight tables in [2^40, 2^55)"""
    assert _tile() == dst._tile() == 64
    return dst._kernel_case(W, n_motifs, 96_000 + W if seed is None else seed)


@functools.lru_cache(maxsize=None)
def _expected(W, n_motifs, seed, fwd, lengths, letters):
    """the brute force of _case, once for the tests that share it"""
    seqs, motifs, weights, _, _ = _case(W, n_motifs, seed)
    out = []
    for m in range(n_motifs):
        od = motif_as_oracle_dict(motifs[m])
        out.append(bf.scan_arrays(seqs, W, od["score_matrix"], od["min_val"], weights[m], fwd, lengths, letters))
    return out


def _check_kernel(W, n_motifs, seed, fwd, lengths, letters):
    from grafimo_amd.substitution_scan import changed_bases, scan_sequences
    seqs, motifs, weights, off, bases = _case(W, n_motifs, seed)
    got = scan_sequences(motifs, off, bases, lengths, letters, weights=weights, forward_only=fwd)
    assert len(got) == n_motifs
    N, K = len(bases), len(lengths)
    left = np.concatenate([np.arange(len(x), 0, -1) for x in seqs if x])         # the bases from an offset on
    no_edit = np.array(lengths)[:, None] > left[None, :]
    assert no_edit.any() and not no_edit.all(axis=1).any()                       # no-edit cells and fitting cells, at every length
    assert any(c in b"acgt" for x in seqs for c in x) and any(c in b"Nn" for x in seqs for c in x)
    moved = changed_bases(off, bases, lengths, letters)
    assert moved.shape == (K, N) and not moved[no_edit].any() and (moved[~no_edit] > 0).any()
    if letters == "AAAA":
        assert (moved[~no_edit] == 0).any()                                      # a block that fits and changes nothing
    want = _expected(W, n_motifs, seed, fwd, lengths, letters)
    for m in range(n_motifs):
        keys, sums = want[m]
        assert got[m][0].shape == (K, N, 2) and got[m][0].dtype == np.uint32
        assert got[m][1].shape == (K, N, 2) and got[m][1].dtype == np.uint64
        assert got[m][0].tolist() == keys, (W, fwd, m, np.argwhere(got[m][0] != np.array(keys, dtype=np.uint32))[:5].tolist())
        assert got[m][1].tolist() == sums, (W, fwd, m, np.argwhere(got[m][1] != np.array(sums, dtype=np.uint64))[:5].tolist())
        # a block that does not fit has four zeros; among the blocks that fit both columns hold non-empty cells, and empty ones
        # where a sequence is shorter than W (a block of one base fits it when W >= 2); some sum no double holds
        assert not got[m][0][no_edit].any() and not got[m][1][no_edit].any()
        fits = got[m][0][~no_edit]
        for c in range(2):
            assert (fits[:, c] != 0).any(), (W, c)
            assert (fits[:, c] == 0).any() == (W > min(lengths)), (W, c)
        assert int(got[m][1].max()) > 1 << 53
        # where the map changes nothing the two columns agree
        same = (moved == 0) & ~no_edit
        assert np.array_equal(got[m][0][same][:, 0], got[m][0][same][:, 1]) and np.array_equal(got[m][1][same][:, 0], got[m][1][same][:, 1])
    return got


KERNEL_CASES = [(W, "CATG") for W in (1, 2, 19, 64)] + [(W, letters) for W in (2, 19) for letters in ("AAAA", "ACTG")]


@pytest.mark.parametrize("fwd", [False, True])
@pytest.mark.parametrize("W,letters", KERNEL_CASES)
def test_kernel_against_brute_force(W, letters, fwd):
    """both columns of every offset and length, exactly, for two motifs of one width (grid.y)"""
    got = _check_kernel(W, 2, None, fwd, _lengths(W), letters)
    assert not np.array_equal(got[0][0], got[1][0])              # (two motifs, two answers)
    assert not np.array_equal(got[0][0][..., 0], got[0][0][..., 1])              # (the map changes something)


def test_seventeen_motifs_take_two_launches():
    got = _check_kernel(2, 17, 97_000, False, (3, 64), "CATG")
    assert len({g[1].tobytes() for g in (got[0], got[15], got[16])}) == 3


@pytest.mark.parametrize("fwd", [False, True])
@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_cover_is_the_deletion_scans_cover(W, fwd):
    """the REF side does not know the map: bit for bit the deletion scan's COVER column for the same lengths"""
    from grafimo_amd import deletion_scan, substitution_scan
    _, motifs, weights, off, bases = _case(W)
    dele = deletion_scan.scan_sequences(motifs, off, bases, _lengths(W), weights=weights, forward_only=fwd)
    for letters in ("CATG", "AAAA"):
        sub = substitution_scan.scan_sequences(motifs, off, bases, _lengths(W), letters, weights=weights, forward_only=fwd)
        for m in range(2):
            assert np.array_equal(sub[m][0][..., substitution_scan.COVER], dele[m][0][..., deletion_scan.COVER]), (W, fwd, m, letters)
            assert np.array_equal(sub[m][1][..., substitution_scan.COVER], dele[m][1][..., deletion_scan.COVER]), (W, fwd, m, letters)


@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_the_identity_map_gives_sub_equal_to_cover(W):
    from grafimo_amd.substitution_scan import scan_sequences
    _, motifs, weights, off, bases = _case(W)
    for fwd in (False, True):
        got = scan_sequences(motifs, off, bases, _lengths(W), "ACGT", weights=weights, forward_only=fwd)
        for m in range(2):
            assert got[m][0].any() and np.array_equal(got[m][0][..., 0], got[m][0][..., 1]), (W, fwd, m)
            assert np.array_equal(got[m][1][..., 0], got[m][1][..., 1]), (W, fwd, m)


@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_length_one_is_the_mutation_scan(W):
    """lengths = (1,): wherever x[o] is a base, SUB is the mutation scan's column of the base f(x[o]) (the REF column's copy at
    a fixed point of the map) and COVER its REF column; where it is none, SUB is COVER"""
    from grafimo_amd import mutation_scan, substitution_scan
    _, motifs, weights, off, bases = _case(W)
    up = bytes(bases).upper()
    real = np.array([c in LETTER for c in up])
    assert real.any() and not real.all()
    at = np.flatnonzero(real)
    for fwd in (False, True):
        mut = mutation_scan.scan_sequences(motifs, off, bases, weights=weights, forward_only=fwd)
        for letters in ("CATG", "AAAA", "ACTG"):
            one = substitution_scan.scan_sequences(motifs, off, bases, (1,), letters, weights=weights, forward_only=fwd)
            column = np.array([1 + "ACGT".index(letters[LETTER[up[n]]]) for n in at])
            for m in range(2):
                assert one[m][0].shape == (1, len(bases), 2)
                for k in range(2):                                               # keys, sums
                    assert np.array_equal(one[m][k][0, at, 1], mut[m][k][at, column]), (W, fwd, letters, m, k)
                    assert np.array_equal(one[m][k][0, :, 0], mut[m][k][:, 0]), (W, fwd, letters, m, k)
                    assert np.array_equal(one[m][k][0, ~real, 1], one[m][k][0, ~real, 0]), (W, fwd, letters, m, k)


@pytest.mark.parametrize("W", [2, 19])
def test_a_lengths_cells_do_not_depend_on_the_other_lengths(W):
    from grafimo_amd.substitution_scan import scan_sequences
    _, motifs, weights, off, bases = _case(W)
    for fwd in (False, True):
        more = scan_sequences(motifs, off, bases, (1, 2, 7, 33, 64), "CATG", weights=weights, forward_only=fwd)
        for k, L in ((0, 1), (2, 7), (3, 33), (4, 64)):
            alone = scan_sequences(motifs, off, bases, (L,), "CATG", weights=weights, forward_only=fwd)
            for m in range(2):
                assert np.array_equal(more[m][0][k], alone[m][0][0]) and np.array_equal(more[m][1][k], alone[m][1][0]), (W, fwd, L, m)


def test_default_weights_a_second_call_and_empty_input():
    """the default weights are haplotype_affinity's; a second call gives the same arrays (nothing is left from the first)"""
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.substitution_scan import scan_sequences
    W, lengths = 7, (2, 9)
    seqs, motifs, _, off, bases = _case(W, 1, 98_000)
    got = scan_sequences(motifs, off, bases, lengths, "transition", temperature=2.0)[0]
    dm = DeviceMotif.lease(motifs[0])
    try:
        w = default_weights(dm, 2.0)[0]
    finally:
        dm.release()
    od = motif_as_oracle_dict(motifs[0])
    keys, sums = bf.scan_arrays(seqs, W, od["score_matrix"], od["min_val"], w, False, lengths, "GTAC")
    assert got[0].tolist() == keys and got[1].tolist() == sums
    again = scan_sequences(motifs, off, bases, lengths, "GTAC", temperature=2.0)[0]
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    none = scan_sequences(motifs, [0, 0, 0], np.zeros(0, dtype=np.uint8), (1, 5, 64), "CATG")[0]
    assert none[0].shape == (3, 0, 2) and none[1].shape == (3, 0, 2) and none[0].dtype == np.uint32 and none[1].dtype == np.uint64


# ------------------------------------------------------------------------------------------- against the existing kernel
@pytest.mark.parametrize("W", [5, 19])
def test_equals_the_query_variant_kernel_on_every_named_block(W):
    """query_variants.score_edits on the edit (coord[o], x[o : o + L], f(x[o : o + L])) of every block of 5 and of 64 bases that
    coordinates can name is applied at o, with the scan's keys and sums, field for field"""
    from grafimo_amd import _native as nv
    from grafimo_amd.query_variants import score_edits
    from grafimo_amd.substitution_scan import scan_sequences
    rng = np.random.default_rng(99_000 + W)
    T = _tile()
    lengths = (5, 64)
    seqs, coords = [], []
    for n, start, calm in ((2 * T + W + 9, 100, (30, 30 + 64 + W)), (2 * W + 3, 4000, None), (W - 1, 7, None)):
        x, c, p = bytearray(), [], start
        while len(x) < n:
            x.append(int(BASES[rng.integers(0, 4)])); c.append(p)
            quiet = calm is not None and calm[0] <= len(x) < calm[1]              # (a stretch long blocks can be named in)
            if not quiet and rng.random() < 0.08:                # bases inserted behind p
                for _ in range(int(rng.integers(1, 4))):
                    x.append(int(BASES[rng.integers(0, 4)])); c.append(~p)
            p += 1 if quiet or rng.random() > 0.05 else int(rng.integers(2, 6))  # (a deletion: coordinates are skipped)
        x, c = x[:n], c[:n]
        if n > 2 * W:
            x[W + 1] = ord("N")
            x[3] |= 0x20
        if calm:
            x[calm[0] + 40] = ord("N")                           # (inside the long blocks, and beside some of them)
        seqs.append(bytes(x)); coords.append(c)
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    coord = np.array([p for c in coords for p in c], dtype=np.int32)
    motifs = [SynMotif(W, seed=990 + k) for k in range(2)]
    weights = [rng.integers(1, 1 << 50, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    pos0, refs, item_seq, where = [], [], [], []
    for v, (x, c) in enumerate(zip(seqs, coords)):
        pairs = [(~p, True) if p < 0 else (p, False) for p in c]
        for o in range(len(x)):
            for k, L in enumerate(lengths):
                if bf.named(pairs, o, L):
                    pos0.append(c[o]); refs.append(x[o:o + L]); item_seq.append(v)
                    where.append((k, int(off[v]) + o, o))
    count = [sum(1 for w in where if w[0] == k) for k in range(2)]
    assert (coord < 0).any() and count[0] > T and count[1] >= W, count
    assert sum(1 for c in coords for a, b in zip(c, c[1:]) if a >= 0 and b >= 0 and b > a + 1) > 0    # a panel deletion
    assert any(b"N" in r for r in refs if len(r) == 64)         # (a substituted N; the short blocks have it inside and beside)
    assert any(b"N" in r for r in refs if len(r) == 5) and any(b"N" not in r for r in refs if len(r) == 5)
    k, n, o = (np.array(v) for v in zip(*where))
    for letters in ("CATG", "TGCA"):
        alts = [bf.image(r, letters) for r in refs]
        assert all(len(a) == len(r) and a != r.upper() for a, r in zip(alts, refs))
        for fwd in (False, True):
            scan = scan_sequences(motifs, off, bases, lengths, letters, weights=weights, forward_only=fwd)
            recs = score_edits(motifs, off, bases, coord, pos0, refs, alts, item_seq, np.arange(len(pos0)), weights=weights,
                               forward_only=fwd)
            for m in range(2):
                r = recs[m]
                assert (r["status"] == nv.GFM_EDIT_APPLIED).all() and np.array_equal(r["o"], o)
                assert np.array_equal(r["ref_key"], scan[m][0][k, n, 0]) and np.array_equal(r["alt_key"], scan[m][0][k, n, 1]), (W, fwd, m)
                assert np.array_equal(r["ref_sum"], scan[m][1][k, n, 0]) and np.array_equal(r["alt_sum"], scan[m][1][k, n, 1]), (W, fwd, m)


# ------------------------------------------------------------------------------------------- the table against the brute force
@functools.lru_cache(maxsize=None)
def _expected_table(name):
    """the brute force alone -> (per region its sequences, per motif (od, ptable, log2 offset, per region per sequence its scan))"""
    from oracle import oracle as orc
    idx, regions, motifs, groups, fwd = mst._setup(name)
    seqs = [bf.region_sequences(idx, S, E, list(groups.values())) for S, E in regions]
    out = []
    for m in motifs:
        od = motif_as_oracle_dict(m)
        w, log2_offset = mst._default_weights(od)
        out.append((od, orc.p_table(od["pmf"]), log2_offset,
                    [[bf.scan(d["bases"], od["width"], od["score_matrix"], od["min_val"], w, fwd, TABLE_LENGTHS, TABLE_MAP) for d in region]
                     for region in seqs]))
    return seqs, out


def _expected_rows(t, name, seqs, od, log2_offset, scans):
    """bf.detail_rows with the coordinates the table chose where a version has two sets (checked to be one of them), and the
    tail table the device made (the oracle's differs in the last digits)"""
    def coords_of(r, d):
        q = [int(q) for q in np.flatnonzero(t.seq_region == r) if int(t.seq_version[q]) == d["version"]]
        assert len(q) == 1, (name, r, d["version"])
        have = [(int(~c) if c < 0 else int(c), bool(c < 0)) for c in t.coord[t.seq_offsets[q[0]]:t.seq_offsets[q[0] + 1]].tolist()]
        assert have in d["coords"], (name, r, d["version"])
        return have
    return bf.detail_rows(t.region_names, seqs, scans, coords_of, od["width"], od["scale"], od["offset"], t.ptable, log2_offset,
                          THRESHOLD, TABLE_LENGTHS, TABLE_MAP)


def _same(x, y):
    return x == y or (x != x and y != y)


COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_a", "haplotypes_none", "is_reference",
           "position", "inserted", "length", "named", "map", "replaced", "replacement", "changed", "ref_score", "ref_pvalue",
           "ref_start", "ref_strand", "ref_kmer", "alt_score", "alt_pvalue", "alt_start", "alt_strand", "alt_kmer", "ref_log2_affinity",
           "alt_log2_affinity", "delta_log2_affinity", "effect"]
SUMMARY_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "length", "versions", "haplotypes", "haplotypes_gain",
                   "haplotypes_loss", "min_delta_log2_affinity", "max_delta_log2_affinity", "best_alt_score"]
ROW_KEY = ("sequence_name", "version", "position", "inserted", "length", "replaced")


@pytest.mark.parametrize("name", GRAPHS)
def test_table_against_the_brute_force(name):
    """the dense arrays, the detail rows of --substitution-all, the default filter, a delta, and the summary"""
    from grafimo_amd.substitution_scan import compute_substitution_scan_many
    idx, regions, motifs, groups, fwd = mst._setup(name)
    seqs, exp = _expected_table(name)
    tables = compute_substitution_scan_many(motifs, idx, regions, False, wp.Args(threshold=THRESHOLD, no_reverse=fwd), TABLE_LENGTHS,
                                            TABLE_MAP, haplotype_groups=groups, all_rows=True)
    n_bases = sum(len(d["bases"]) for region in seqs for d in region)
    K = len(TABLE_LENGTHS)
    for t, m, (od, ptab, log2_offset, scans) in zip(tables, motifs, exp):
        assert (t.motif_id, t.width, t.group_names, t.lengths.tolist()) == (m.motif_id, od["width"], list(groups), list(TABLE_LENGTHS))
        assert t.base_map.tolist() == [1, 0, 3, 2]
        # ---- the sequences: the versions by number, the count-0 reference where no version is the reference's
        assert len(t.seq_count) == sum(len(region) for region in seqs) and len(t.bases) == n_bases
        assert t.keys.shape == (K, n_bases, 2) and t.sums.shape == (K, n_bases, 2)
        for r, region in enumerate(seqs):
            mine = np.flatnonzero(t.seq_region == r)
            order = sorted(mine.tolist(), key=lambda q: (t.seq_version[q] < 0, t.seq_version[q]))
            assert [(int(t.seq_version[q]), int(t.seq_count[q]), t.seq_group_counts[q].tolist(), bool(t.seq_is_reference[q]),
                     t.bases[t.seq_offsets[q]:t.seq_offsets[q + 1]].tobytes()) for q in order] == \
                [(d["version"], d["count"], d["group_counts"], d["is_reference"], d["bases"]) for d in region], (name, r)
            # ---- the dense arrays: both columns of every base and length
            for q, d, scan in zip(order, region, scans[r]):
                a, b = int(t.seq_offsets[q]), int(t.seq_offsets[q + 1])
                for k in range(K):
                    assert t.keys[k, a:b].tolist() == [[bf.key_of(best) for best, _ in row] for row in scan[k]], (name, m.motif_id, r, k)
                    assert t.sums[k, a:b].tolist() == [[int(s) for _, s in row] for row in scan[k]], (name, m.motif_id, r, k)
        # ---- all_rows: every block that changes a base, every column
        rows = _expected_rows(t, name, seqs, od, log2_offset, scans)
        frame = t.to_frame()
        assert list(frame.columns) == COLUMNS
        assert len(frame) == len(rows) == len(t) and 0 < len(rows) <= K * n_bases
        for k, (f, e) in enumerate(zip(frame.to_dict("records"), rows)):
            assert (f["motif_id"], f["motif_alt_id"]) == (m.motif_id, m.motif_name)
            assert [f["haplotypes_a"], f["haplotypes_none"]] == e["groups"], (name, k)
            for c in COLUMNS[2:5] + COLUMNS[7:]:
                assert _same(f[c], e[c]), (name, m.motif_id, k, c, f[c], e[c], e)
        # ---- the default filter and a delta are the brute force's
        t.all_rows = False
        kept = [e for e in rows if e["effect"] in ("gain", "loss")]
        assert [tuple(f[c] for c in ROW_KEY) for f in t.to_frame().to_dict("records")] == [tuple(e[c] for c in ROW_KEY) for e in kept], name
        t.delta = 1.0
        kept = [e for e in rows if e["effect"] in ("gain", "loss") or abs(e["delta_log2_affinity"]) >= 1.0]
        assert len(t.to_frame()) == len(kept) == len(t), name
        t.delta, t.all_rows = None, True
        # ---- the summary against a loop over the rows
        want = bf.summary_rows(rows)
        s = t.summary_frame()
        assert list(s.columns) == SUMMARY_COLUMNS and len(s) == len(want)
        names = {n_: k for k, n_ in enumerate(t.region_names.tolist())}
        keys = [(f["sequence_name"], f["position"], f["length"]) for f in s.to_dict("records")]
        assert keys == sorted(want, key=lambda q: (names[q[0]], q[1], q[2])), name
        for f in s.to_dict("records"):
            w = want[(f["sequence_name"], f["position"], f["length"])]
            assert (f["versions"], f["haplotypes"], f["haplotypes_gain"], f["haplotypes_loss"]) == \
                (w["versions"], w["haplotypes"], w["haplotypes_gain"], w["haplotypes_loss"]), (name, f)
            assert _same(f["min_delta_log2_affinity"], min(w["deltas"]) if w["deltas"] else np.nan)
            assert _same(f["max_delta_log2_affinity"], max(w["deltas"]) if w["deltas"] else np.nan)
            assert _same(f["best_alt_score"], max(w["scores"]) if w["scores"] else np.nan)
        t.all_rows = False
        kept = {q for q, w in want.items() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0}
        assert {(f["sequence_name"], f["position"], f["length"]) for f in t.summary_frame().to_dict("records")} == kept
        t.delta = 1.0
        kept = {q for q, w in want.items() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0 or
                (w["deltas"] and max(abs(min(w["deltas"])), abs(max(w["deltas"]))) >= 1.0)}
        assert {(f["sequence_name"], f["position"], f["length"]) for f in t.summary_frame().to_dict("records")} == kept


def test_the_graphs_hold_every_case():
    """with the brute force alone: inserted bases, a region whose reference no haplotype spells (the count-0 row) and one where a
    version is the reference's, sides without a window, blocks no coordinates name, gains and losses"""
    inserted = added = spelled = short = unnamed = gain = loss = 0
    for name in GRAPHS:
        seqs, exp = _expected_table(name)
        for region in seqs:
            added += int(region[-1]["version"] < 0)
            spelled += int(any(d["is_reference"] and d["version"] >= 0 for d in region))
            inserted += sum(int(t) for d in region for _, t in d["coords"][0])
            for d in region:
                n = len(d["bases"])
                unnamed += sum(int(not bf.named(d["coords"][0], o, L)) for L in TABLE_LENGTHS for o in range(n - L + 1))
        for od, ptab, _, scans in exp:
            for region in scans:
                for scan in region:
                    for k, L in enumerate(TABLE_LENGTHS):
                        for o, row in enumerate(scan[k][:max(len(scan[k]) - L + 1, 0)]):
                            short += int(row[1][0] is None)
                            e = bf.effect(ptab, THRESHOLD, row[0][0], row[1][0])
                            gain += int(e == "gain")
                            loss += int(e == "loss")
    counts = (inserted, added, spelled, short, unnamed, gain, loss)
    assert min(counts) >= 1, counts


# ------------------------------------------------------------------------------------------- refusals, command line
def test_refusals(monkeypatch):
    from grafimo_amd import _native as nv
    from grafimo_amd.substitution_scan import compute_substitution_scan, scan_sequences
    x = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)
    m5, m7 = SynMotif(5, seed=1), SynMotif(7, seed=2)
    m5.motif_id = "FIVE"
    with pytest.raises(nv.NativeError, match="one width"):
        scan_sequences([m5, m7], [0, 12], x, (2,), "CATG")
    # a side holds up to 2 (W + Lmax - 1) = 16 windows: 16 (2^60 - 1) fits, 16 x 2^60 does not
    with pytest.raises(nv.NativeError, match="a side holds up to 16 windows .* may pass 2\\^64"):
        scan_sequences([m5], [0, 12], x, (1, 4), "CATG", weights=[np.full(5001, 1 << 60, dtype=np.uint64)])
    scan_sequences([m5], [0, 12], x, (1, 4), "CATG", weights=[np.full(5001, (1 << 60) - 1, dtype=np.uint64)])
    with pytest.raises(nv.NativeError, match="may pass 2\\^64"):                 # (the longest length counts, not the number)
        scan_sequences([m5], [0, 12], x, (5,), "CATG", weights=[np.full(5001, (1 << 60) - 1, dtype=np.uint64)])
    for bad in ((0,), (65,), (3, 2), (2, 2)):
        with pytest.raises(ValueError):
            scan_sequences([m5], [0, 12], x, bad, "CATG")
    for bad in ("ACG", "ACGU", "scramble", None):
        with pytest.raises(ValueError, match="base map"):
            scan_sequences([m5], [0, 12], x, (2,), bad)
    with pytest.raises(ValueError, match="FIVE: .* 576 bytes, more than max_bytes = 575"):
        scan_sequences([m5], [0, 12], x, (1, 2), "CATG", max_bytes=575)
    both = scan_sequences([m5, m5], [0, 12], x, (1, 2), "CATG", max_bytes=576)                       # one motif at a time
    assert np.array_equal(both[0][1], both[1][1]) and np.array_equal(both[0][1], scan_sequences([m5], [0, 12], x, (1, 2), "CATG")[0][1])
    with pytest.raises(ValueError, match="starts at 0"):
        scan_sequences([m5], [1, 12], x, (1,), "CATG")
    # the library's own checks of the lengths and the map, which the module never lets through
    from grafimo_amd.device import DeviceMotif
    import torch
    dm = DeviceMotif.lease(m5)
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        d_x = torch.from_numpy(x.copy()).to(dev)
        d_w = torch.ones(5001, dtype=torch.int64, device=dev)
        keys, sums = torch.full((2, 12, 2), -1, dtype=torch.int32, device=dev), torch.full((2, 12, 2), -1, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        off = np.array([0, 12], dtype=np.int64)
        import ctypes
        one = lambda p: (ctypes.c_void_p * 1)(p)                                 # noqa: E731

        def call(lengths, codes):
            ln = np.array(lengths, dtype=np.int32)
            mp = None if codes is None else np.array(codes, dtype=np.uint8)
            return nv.lib().gfm_sequence_substitution_scan(one(dm.handle), 1, one(d_w.data_ptr()), 1, 1, off.ctypes.data, d_x.data_ptr(), 2,
                                                           ln.ctypes.data, None if mp is None else mp.ctypes.data, 0,
                                                           one(keys.data_ptr()), one(sums.data_ptr()), status.data_ptr(), None)
        for bad, text in (([0, 2], b"outside 1 .. 64"), ([2, 65], b"outside 1 .. 64"), ([3, 2], b"strictly ascend"),
                          ([2, 2], b"strictly ascend")):
            assert call(bad, [1, 0, 3, 2]) == nv.GFM_ERR_INVALID and text in nv.lib().gfm_last_error(), bad
        assert call([1, 2], None) == nv.GFM_ERR_INVALID and b"NULL base_map" in nv.lib().gfm_last_error()
        assert call([1, 2], [1, 0, 4, 2]) == nv.GFM_ERR_INVALID and b"base_map[2] = 4 is outside 0 .. 3" in nv.lib().gfm_last_error()
        torch.cuda.synchronize()
        assert bool((keys == -1).all()) and bool((sums == -1).all())             # refused before anything was launched
    finally:
        dm.release()
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="the substitution scan is computed on one GPU"):
        compute_substitution_scan(m5, bf.hand_graph(), [(0, 20)], False, wp.Args(), (2,))


def _cli_case():
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    fa, vcf, bedfile = os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), os.path.join(GOLD, "regions.bed")
    bed = read_bed_regions(bedfile)
    return fa, vcf, bedfile, bed, [GraphIndex.from_fasta_vcf(fa, vcf, c[3:]) for c in bed]


def _run(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd"] + list(flags), check=True, cwd=str(tmp_path),
                          env=dict(os.environ, PYTHONPATH=ROOT), timeout=600, capture_output=True, text=True)


def test_cli_writes_both_files_and_prints_with_f(tmp_path):
    """--substitution-scan 10 3 3 (sorted, merged) with files (the map by its letters, TGCA) and with -f (by its name,
    complement): the same table, one motif"""
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.substitution_scan import compute_substitution_scan_many
    from grafimo_amd.workflow import Findmotif
    fa, vcf, bedfile, bed, graphs = _cli_case()
    meme = os.path.join(GOLD, "MA0139.1.meme")
    out = str(tmp_path / "o")
    common = ["-m", meme, "-l", fa, "-v", vcf, "-b", bedfile, "-t", "0.05", "--substitution-delta", "2.5", "--substitution-scan", "10", "3",
              "3"]
    r = _run(tmp_path, *common, "-o", out, "--substitution-map", "TGCA")
    assert "substitution scan rows written to" in r.stdout and "substitution scan summary rows written to" in r.stdout
    wf = Findmotif(threshold=0.05)
    motif = get_motif_pwm(meme, wf, 2, True, pvalue_matrix=False)[0]
    t = compute_substitution_scan_many([motif], graphs, list(bed.values()), False, wp.Args(threshold=0.05), (3, 10), "complement",
                                       delta=2.5)[0]
    detail = open(os.path.join(out, "grafimo_substitution_scan.tsv")).read()
    summary = open(os.path.join(out, "grafimo_substitution_scan_summary.tsv")).read()
    assert detail.split("\n", 1)[0].split("\t") == [c for c in COLUMNS if c not in ("haplotypes_a", "haplotypes_none")]
    assert summary.split("\n", 1)[0].split("\t") == SUMMARY_COLUMNS
    want_detail = t.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    want_summary = t.summary_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    assert len(t) > 0 and set(t.to_frame()["length"]) == {3, 10} and set(t.to_frame()["map"]) == {"TGCA"}
    assert detail == want_detail and summary == want_summary
    r = _run(tmp_path, *common, "-f", "--substitution-map", "complement")
    assert want_detail + want_summary in r.stdout


def test_cli_names_the_files_of_two_motifs(tmp_path):
    fa, vcf, bedfile, _, _ = _cli_case()
    out = str(tmp_path / "o")
    r = _run(tmp_path, "-m", os.path.join(GOLD, "MA0139.1.meme"), os.path.join(GOLD, "MA0035.4.meme"), "-l", fa, "-v", vcf, "-b", bedfile,
             "-t", "0.05", "-o", out, "--substitution-scan", "3", "10", "--substitution-all")
    assert r.stdout.count("substitution scan rows written to") == 2
    found = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs if "substitution_scan" in f)
    assert len(found) == 4 and sum("summary" in f for f in found) == 2
    assert not any(f.endswith("grafimo_substitution_scan.tsv") for f in found)
    import pandas as pd
    for f in found:                                              # (the default map is the transversion)
        if "summary" not in f:
            frame = pd.read_csv(os.path.join(out, f), sep="\t")
            assert len(frame) > 0 and set(frame["map"]) == {"CATG"} and set(frame["length"]) == {3, 10}
