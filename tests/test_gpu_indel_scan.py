"""The indel scan on the GPU: the kernel through scan_sequences against the brute force (tests/indel_scan_bruteforce.py) at the
tile's edges, against the query-variant kernel on the same one-base deletions and insertions, the table and both frames against
the brute force on the graphs test_gpu_mutation_scan.py uses, the refusals and the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import indel_scan_bruteforce as bf  # noqa: E402
import test_gpu_mutation_scan as mst  # noqa: E402  (its graphs, regions, motifs and default weights)
import wide_panel_cases as wp  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = mst.GOLD
BASES = mst.BASES
GRAPHS = mst.GRAPHS
THRESHOLD = mst.THRESHOLD


def _tile():
    from grafimo_amd import _native as nv
    return nv.GFM_INDELSCAN_TILE


# ------------------------------------------------------------------------------------------- the kernel through scan_sequences
def _lengths(W, T):
    """in this order: offsets and empty sequences between others; W - 1: the insertions make its only window"""
    return [0, 1, W - 1, W, W + 1, T - 1, T, T + 1, T + W - 1, 2 * T + 3]


def _sequences(W, T, rng):
    """random sequences of _lengths with lower-case bases and an N at offset 0 and at offset n - 1 (T + 1), just before a tile
    edge (T + W - 1: offset T - 1 when W <= 2, else inside the next tile's halo), just behind a tile edge, inside the halo, and
    at the last offset of a tile (2 T + 3)"""
    seqs = []
    for n in _lengths(W, T):
        x = bytearray(BASES[rng.integers(0, 4, size=n)].tobytes())
        for j in np.flatnonzero(rng.random(n) < 0.15).tolist():
            x[j] |= 0x20
        if n == T + 1:
            x[0] = ord("N")
            x[n - 1] = ord("n")
        if n == T + W - 1:
            x[max(T - W // 2 - 1, 0)] = ord("N")
        if n == 2 * T + 3:
            x[T + W // 2] = ord("N")
            x[2 * T - 1] = ord("N")
            x[n - 1] = ord("N")
        if n == W + 1:
            x[0] = ord("N")                                      # one window holds it, one does not; deleting it repairs one
        seqs.append(bytes(x))
    return seqs


@functools.lru_cache(maxsize=None)
def _kernel_case(W, n_motifs, seed):
    rng = np.random.default_rng(seed)
    T = _tile()
    seqs = _sequences(W, T, rng)
    motifs = [SynMotif(W, seed=seed + 11 * k) for k in range(n_motifs)]
    # large entries: a double could not hold the sums (2 W = 128 entries below 2^55 stay below 2^64)
    weights = [rng.integers(1 << 40, 1 << 55, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    return seqs, motifs, weights, off, np.frombuffer(b"".join(seqs), dtype=np.uint8)


def _check_kernel(W, n_motifs, seed, fwd):
    from grafimo_amd.indel_scan import scan_sequences
    seqs, motifs, weights, off, bases = _kernel_case(W, n_motifs, seed)
    got = scan_sequences(motifs, off, bases, weights=weights, forward_only=fwd)
    assert len(got) == n_motifs
    for m in range(n_motifs):
        od = motif_as_oracle_dict(motifs[m])
        keys, sums = bf.scan_arrays(seqs, W, od["score_matrix"], od["min_val"], weights[m], fwd)
        assert got[m][0].shape == (len(bases), 7) and got[m][0].dtype == np.uint32
        assert got[m][1].shape == (len(bases), 7) and got[m][1].dtype == np.uint64
        assert got[m][0].tolist() == keys, (W, fwd, m, np.argwhere(got[m][0] != np.array(keys, dtype=np.uint32))[:5].tolist())
        assert got[m][1].tolist() == sums, (W, fwd, m, np.argwhere(got[m][1] != np.array(sums, dtype=np.uint64))[:5].tolist())
        # the case holds empty and non-empty sides -- of every column when W > 1 -- and a sum no double holds
        # (a side across a junction needs W >= 2; n = 1 leaves COVER empty when W > 1 and the insertions when W > 2)
        for c in range(7):
            assert any(k[c] != 0 for k in keys) == (not (W == 1 and c in (1, 2))), (W, c)
            assert any(k[c] == 0 for k in keys) == (c in (1, 2) or (c == 0 and W > 1) or (c >= 3 and W > 2)), (W, c)
        assert max(max(s) for s in sums) > 1 << 53
    return got


@pytest.mark.parametrize("fwd", [False, True])
@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_kernel_against_brute_force(W, fwd):
    """all seven columns of every offset, exactly, for two motifs of one width (grid.y)"""
    got = _check_kernel(W, 2, 81_000 + W, fwd)
    assert not np.array_equal(got[0][0], got[1][0])              # (two motifs, two answers)


def test_seventeen_motifs_take_two_launches():
    got = _check_kernel(2, 17, 82_000, False)
    assert len({g[1].tobytes() for g in (got[0], got[15], got[16])}) == 3


def test_default_weights_and_a_second_call():
    """the default weights are haplotype_affinity's; a second call gives the same arrays (nothing is left from the first)"""
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.indel_scan import scan_sequences
    W = 7
    seqs, motifs, _, off, bases = _kernel_case(W, 1, 83_000)
    got = scan_sequences(motifs, off, bases, temperature=2.0)[0]
    dm = DeviceMotif.lease(motifs[0])
    try:
        w = default_weights(dm, 2.0)[0]
    finally:
        dm.release()
    od = motif_as_oracle_dict(motifs[0])
    keys, sums = bf.scan_arrays(seqs, W, od["score_matrix"], od["min_val"], w, False)
    assert got[0].tolist() == keys and got[1].tolist() == sums
    again = scan_sequences(motifs, off, bases, temperature=2.0)[0]
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    none = scan_sequences(motifs, [0, 0, 0], np.zeros(0, dtype=np.uint8))[0]
    assert none[0].shape == (0, 7) and none[1].shape == (0, 7)


# ------------------------------------------------------------------------------------------- against the existing kernel
@pytest.mark.parametrize("W", [5, 19])
def test_equals_the_query_variant_kernel_on_every_one_base_indel(W):
    """query_variants.score_edits on the deletion (coord[o], x[o], "") of every non-inserted o is applied at o, on the insertion
    (coord[o] + 1, "", b) is applied at o + 1 wherever the next base is the non-inserted coord[o] + 1 or o is the last offset;
    both with the scan's keys and sums"""
    from grafimo_amd import _native as nv
    from grafimo_amd.indel_scan import scan_sequences
    from grafimo_amd.query_variants import score_edits
    rng = np.random.default_rng(84_000 + W)
    T = _tile()
    seqs, coords = [], []
    for n, start in ((T + W + 9, 100), (2 * W + 3, 4000), (W - 1, 7)):
        x, c, p = bytearray(), [], start
        while len(x) < n:
            x.append(int(BASES[rng.integers(0, 4)])); c.append(p)
            if rng.random() < 0.08:                              # bases inserted behind p
                for _ in range(int(rng.integers(1, 4))):
                    x.append(int(BASES[rng.integers(0, 4)])); c.append(~p)
            p += 1 if rng.random() > 0.05 else int(rng.integers(2, 6))      # (a deletion: coordinates are skipped)
        x, c = x[:n], c[:n]
        if n > 2 * W:
            x[W + 1] = ord("N")
            x[3] |= 0x20
        seqs.append(bytes(x)); coords.append(c)
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    coord = np.array([p for c in coords for p in c], dtype=np.int32)
    motifs = [SynMotif(W, seed=840 + k) for k in range(2)]
    weights = [rng.integers(1, 1 << 50, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    pos0, refs, alts, item_seq, where = [], [], [], [], []
    for v, (x, c) in enumerate(zip(seqs, coords)):
        n = len(x)
        for o in range(n):
            if c[o] < 0:
                continue
            pos0.append(c[o]); refs.append(bytes([x[o]])); alts.append(b""); item_seq.append(v)
            where.append((int(off[v]) + o, 0, 1, o))
            if o == n - 1 or c[o + 1] == c[o] + 1:
                for col, b in enumerate(b"ACGT", 3):
                    pos0.append(c[o] + 1); refs.append(b""); alts.append(bytes([b])); item_seq.append(v)
                    where.append((int(off[v]) + o, 2, col, o + 1))
    assert (coord < 0).any() and len(where) > 2 * T
    assert sum(1 for w in where if w[2] == 1) > T and sum(1 for w in where if w[2] > 2) > T
    for fwd in (False, True):
        scan = scan_sequences(motifs, off, bases, weights=weights, forward_only=fwd)
        recs = score_edits(motifs, off, bases, coord, pos0, refs, alts, item_seq, np.arange(len(pos0)), weights=weights, forward_only=fwd)
        n, rcol, acol, o = (np.array(v) for v in zip(*where))
        for m in range(2):
            r = recs[m]
            assert (r["status"] == nv.GFM_EDIT_APPLIED).all() and np.array_equal(r["o"], o)
            assert np.array_equal(r["ref_key"], scan[m][0][n, rcol]) and np.array_equal(r["alt_key"], scan[m][0][n, acol]), (W, fwd, m)
            assert np.array_equal(r["ref_sum"], scan[m][1][n, rcol]) and np.array_equal(r["alt_sum"], scan[m][1][n, acol]), (W, fwd, m)


# ------------------------------------------------------------------------------------------- the table against the brute force
@functools.lru_cache(maxsize=None)
def _expected(name):
    """the brute force alone -> (per region its sequences, per motif (od, ptable, log2 offset, per region per sequence its scan))"""
    from oracle import oracle as orc
    idx, regions, motifs, groups, fwd = mst._setup(name)
    seqs = [bf.region_sequences(idx, S, E, list(groups.values())) for S, E in regions]
    out = []
    for m in motifs:
        od = motif_as_oracle_dict(m)
        w, log2_offset = mst._default_weights(od)
        out.append((od, orc.p_table(od["pmf"]), log2_offset,
                    [[bf.scan(d["bases"], od["width"], od["score_matrix"], od["min_val"], w, fwd) for d in region] for region in seqs]))
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
    return bf.detail_rows(t.region_names, seqs, scans, coords_of, od["width"], od["scale"], od["offset"], t.ptable, log2_offset, THRESHOLD)


def _same(x, y):
    return x == y or (x != x and y != y)


COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_a", "haplotypes_none", "is_reference",
           "position", "inserted", "type", "base", "ref_score", "ref_pvalue", "ref_start", "ref_strand", "ref_kmer", "alt_score",
           "alt_pvalue", "alt_start", "alt_strand", "alt_kmer", "ref_log2_affinity", "alt_log2_affinity", "delta_log2_affinity",
           "effect"]
SUMMARY_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "type", "base", "versions", "haplotypes", "haplotypes_gain",
                   "haplotypes_loss", "min_delta_log2_affinity", "max_delta_log2_affinity", "best_alt_score"]


@pytest.mark.parametrize("name", GRAPHS)
def test_table_against_the_brute_force(name):
    from grafimo_amd.indel_scan import compute_indel_scan_many
    idx, regions, motifs, groups, fwd = mst._setup(name)
    seqs, exp = _expected(name)
    tables = compute_indel_scan_many(motifs, idx, regions, False, wp.Args(threshold=THRESHOLD, no_reverse=fwd),
                                     haplotype_groups=groups, all_rows=True)
    n_bases = sum(len(d["bases"]) for region in seqs for d in region)
    for t, m, (od, ptab, log2_offset, scans) in zip(tables, motifs, exp):
        assert (t.motif_id, t.width, t.group_names) == (m.motif_id, od["width"], list(groups))
        # ---- the sequences: the versions by number, the count-0 reference where no version is the reference's
        assert len(t.seq_count) == sum(len(region) for region in seqs) and len(t.bases) == n_bases
        for r, region in enumerate(seqs):
            mine = np.flatnonzero(t.seq_region == r)
            order = sorted(mine.tolist(), key=lambda q: (t.seq_version[q] < 0, t.seq_version[q]))
            assert [(int(t.seq_version[q]), int(t.seq_count[q]), t.seq_group_counts[q].tolist(), bool(t.seq_is_reference[q]),
                     t.bases[t.seq_offsets[q]:t.seq_offsets[q + 1]].tobytes()) for q in order] == \
                [(d["version"], d["count"], d["group_counts"], d["is_reference"], d["bases"]) for d in region], (name, r)
            # ---- the dense arrays: seven columns of every base, the homopolymers' too
            for q, d, scan in zip(order, region, scans[r]):
                a, b = int(t.seq_offsets[q]), int(t.seq_offsets[q + 1])
                assert t.keys[a:b].tolist() == [[bf.key_of(best) for best, _ in row] for row in scan], (name, m.motif_id, r, d["version"])
                assert t.sums[a:b].tolist() == [[int(s) for _, s in row] for row in scan], (name, m.motif_id, r, d["version"])
        # ---- all_rows: every change a homopolymer does not repeat, every column
        rows = _expected_rows(t, name, seqs, od, log2_offset, scans)
        frame = t.to_frame()
        assert list(frame.columns) == COLUMNS
        assert len(frame) == len(rows) == len(t) and len(rows) < 5 * n_bases
        for k, (f, e) in enumerate(zip(frame.to_dict("records"), rows)):
            assert (f["motif_id"], f["motif_alt_id"]) == (m.motif_id, m.motif_name)
            assert [f["haplotypes_a"], f["haplotypes_none"]] == e["groups"], (name, k)
            for c in COLUMNS[2:5] + COLUMNS[7:]:
                assert _same(f[c], e[c]), (name, m.motif_id, k, c, f[c], e[c], e)
        # ---- the default filter and a delta are the brute force's
        t.all_rows = False
        kept = [e for e in rows if e["effect"] in ("gain", "loss")]
        got = t.to_frame()
        assert [(f["sequence_name"], f["version"], f["position"], f["inserted"], f["type"], f["base"]) for f in got.to_dict("records")] == \
            [(e["sequence_name"], e["version"], e["position"], e["inserted"], e["type"], e["base"]) for e in kept], name
        t.delta = 1.0
        kept = [e for e in rows if e["effect"] in ("gain", "loss") or abs(e["delta_log2_affinity"]) >= 1.0]
        assert len(t.to_frame()) == len(kept) == len(t), name
        t.delta, t.all_rows = None, True
        # ---- the summary against a loop over the detail rows
        want = bf.summary_of(frame.to_dict("records"))
        s = t.summary_frame()
        assert list(s.columns) == SUMMARY_COLUMNS and len(s) == len(want)
        names = {n_: k for k, n_ in enumerate(t.region_names.tolist())}
        keys = [(f["sequence_name"], f["position"], f["type"], f["base"]) for f in s.to_dict("records")]
        assert keys == sorted(want, key=lambda q: (names[q[0]], q[1], q[2], q[3])), name
        for f in s.to_dict("records"):
            w = want[(f["sequence_name"], f["position"], f["type"], f["base"])]
            assert (f["versions"], f["haplotypes"], f["haplotypes_gain"], f["haplotypes_loss"]) == \
                (w["versions"], w["haplotypes"], w["haplotypes_gain"], w["haplotypes_loss"]), (name, f)
            assert _same(f["min_delta_log2_affinity"], min(w["deltas"]) if w["deltas"] else np.nan)
            assert _same(f["max_delta_log2_affinity"], max(w["deltas"]) if w["deltas"] else np.nan)
            assert _same(f["best_alt_score"], max(w["scores"]) if w["scores"] else np.nan)
        t.all_rows = False
        kept = {q for q, w in want.items() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0}
        assert {(f["sequence_name"], f["position"], f["type"], f["base"]) for f in t.summary_frame().to_dict("records")} == kept


def test_the_graphs_hold_every_case():
    """with the brute force alone: inserted bases, a region whose reference no haplotype spells (the count-0 row) and one where a
    version is the reference's, sides without a window, homopolymers, gains and losses of deletions and of insertions"""
    inserted = added = spelled = short = repeats = 0
    gain, loss = {"DEL": 0, "INS": 0}, {"DEL": 0, "INS": 0}
    for name in GRAPHS:
        seqs, exp = _expected(name)
        for region in seqs:
            added += int(region[-1]["version"] < 0)
            spelled += int(any(d["is_reference"] and d["version"] >= 0 for d in region))
            inserted += sum(int(t) for d in region for _, t in d["coords"][0])
            repeats += sum(int(not bf.reported(d["bases"], o, "DEL", None)) for d in region for o in range(len(d["bases"])))
        for od, ptab, _, scans in exp:
            for region in scans:
                for scan in region:
                    for row in scan:
                        short += int(row[1][0] is None)
                        for col, (kind, _) in zip((1, 3, 4, 5, 6), bf.CHANGES):
                            e = bf.effect(ptab, THRESHOLD, row[bf.REF_COLUMN[kind]][0], row[col][0])
                            gain[kind] += int(e == "gain")
                            loss[kind] += int(e == "loss")
    counts = (inserted, added, spelled, short, repeats, gain["DEL"], gain["INS"], loss["DEL"], loss["INS"])
    assert min(counts) >= 1, counts


def test_rows_of_the_hand_made_graph():
    """read off query_variant_bruteforce.hand_graph: in [8, 14) haplotype 3 reads GG behind 10 -- ACGGGTAC, a homopolymer of a
    base and two inserted ones --, haplotype 2 deletes 10 and 11; the reference sequence is haplotype 0's"""
    from grafimo_amd.indel_scan import compute_indel_scan
    t = compute_indel_scan(SynMotif(3, seed=5), bf.hand_graph(), [(8, 14)], False, wp.Args(threshold=0.5), all_rows=True)
    assert t.seq_count.tolist() == [1, 1, 1, 1] and t.seq_version.tolist() == [0, 1, 2, 3] and t.seq_is_reference.tolist() == [True, False, False, False]
    assert [t.bases[a:b].tobytes() for a, b in zip(t.seq_offsets[:-1], t.seq_offsets[1:])] == [b"ACGTAC", b"ATGTAC", b"ACAC", b"ACGGGTAC"]
    assert t.keys.shape == (24, 7) and (t.keys[:, 3:] > 0).all()                 # every cell, whatever the frames drop
    f = t.to_frame()
    # behind every base but a sequence's first the insertion of that base again is the row before; GGG has one deletion
    assert len(f) == 5 * 24 - (24 - 4) - 2 == len(t)
    v3 = f[f["version"] == 3]
    g = v3[v3["base"] == "G"]
    assert sorted(zip(g["type"], g["position"], g["inserted"])) == [("DEL", 11, False)] + [("INS", p, False) for p in (9, 10, 12, 13, 14)]
    assert set(v3[v3["inserted"]]["position"]) == {11} and set(v3[v3["inserted"]]["base"]) == {"A", "C", "T"}
    s = t.summary_frame()
    dels = s[s["type"] == "DEL"]
    assert dels[dels["position"] == 9]["versions"].tolist() == [4]                                   # A at 9 in all four versions
    assert sorted(zip(dels[dels["position"] == 10]["base"], dels[dels["position"] == 10]["versions"])) == [("C", 3), ("T", 1)]
    assert dels[dels["position"] == 11]["versions"].tolist() == [3]                                  # deleted in one
    ins = s[(s["type"] == "INS") & (s["position"] == 9)]
    assert ins["base"].tolist() == ["A", "C", "G", "T"] and ins["versions"].tolist() == [4, 4, 4, 4]


# ------------------------------------------------------------------------------------------- refusals, command line
def test_refusals(monkeypatch):
    from grafimo_amd import _native as nv
    from grafimo_amd.indel_scan import compute_indel_scan, scan_sequences
    x = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)
    m5, m7 = SynMotif(5, seed=1), SynMotif(7, seed=2)
    m5.motif_id = "FIVE"
    with pytest.raises(nv.NativeError, match="one width"):
        scan_sequences([m5, m7], [0, 12], x)
    with pytest.raises(nv.NativeError, match="may pass 2\\^64"):
        scan_sequences([m5], [0, 12], x, weights=[np.full(5001, 1 << 61, dtype=np.uint64)])
    scan_sequences([m5], [0, 12], x, weights=[np.full(5001, (1 << 60) - 1, dtype=np.uint64)])        # 10 of them fit
    with pytest.raises(ValueError, match="FIVE: .* 1008 bytes, more than max_bytes = 1007"):
        scan_sequences([m5], [0, 12], x, max_bytes=1007)
    both = scan_sequences([m5, m5], [0, 12], x, max_bytes=1008)                                      # one motif at a time
    assert np.array_equal(both[0][1], both[1][1]) and np.array_equal(both[0][1], scan_sequences([m5], [0, 12], x)[0][1])
    with pytest.raises(ValueError, match="starts at 0"):
        scan_sequences([m5], [1, 12], x)
    lib = nv.lib()
    assert lib.gfm_sequence_indel_scan(None, 1, None, 1, 0, None, None, 0, None, None, None, None) == nv.GFM_OK
    assert lib.gfm_sequence_indel_scan(None, 1, None, 1, 0, None, None, 2, None, None, None, None) == nv.GFM_ERR_INVALID
    assert b"unknown flag" in lib.gfm_last_error()
    off = np.array([0, 5, 3], dtype=np.int64)
    assert lib.gfm_sequence_indel_scan(None, 1, None, 1, 2, off.ctypes.data, None, 0, None, None, None, None) == nv.GFM_ERR_INVALID
    assert b"descends" in lib.gfm_last_error()
    off = np.array([0, 1 << 31], dtype=np.int64)
    assert lib.gfm_sequence_indel_scan(None, 1, None, 1, 1, off.ctypes.data, None, 0, None, None, None, None) == nv.GFM_ERR_INVALID
    assert b"2^31" in lib.gfm_last_error()
    import torch
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="the indel scan is computed on one GPU"):
        compute_indel_scan(m5, bf.hand_graph(), [(0, 20)], False, wp.Args())


def test_cli_writes_both_files(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    from grafimo_amd.indel_scan import compute_indel_scan_many
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.workflow import Findmotif
    fa, vcf, bedfile = os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), os.path.join(GOLD, "regions.bed")
    bed = read_bed_regions(bedfile)
    graphs = [GraphIndex.from_fasta_vcf(fa, vcf, c[3:]) for c in bed]
    out = str(tmp_path / "o")
    r = subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", fa, "-v", vcf, "-b", bedfile,
                        "-t", "0.05", "-o", out, "--indel-scan", "--indel-delta", "2.5"], check=True, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=600, capture_output=True, text=True)
    assert "indel scan rows written to" in r.stdout and "indel scan summary rows written to" in r.stdout
    wf = Findmotif(threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "MA0139.1.meme"), wf, 2, True, pvalue_matrix=False)[0]
    t = compute_indel_scan_many([motif], graphs, list(bed.values()), False, wp.Args(threshold=0.05), delta=2.5)[0]
    detail = open(os.path.join(out, "grafimo_indel_scan.tsv")).read()
    summary = open(os.path.join(out, "grafimo_indel_scan_summary.tsv")).read()
    assert detail.split("\n", 1)[0].split("\t") == [c for c in COLUMNS if c not in ("haplotypes_a", "haplotypes_none")]
    assert summary.split("\n", 1)[0].split("\t") == SUMMARY_COLUMNS
    assert len(t) > 0 and detail == t.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    assert summary == t.summary_frame().to_csv(sep="\t", index=False, lineterminator="\n")
