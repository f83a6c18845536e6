"""The insertion scan on the GPU: the kernel through scan_sequences against the brute force (tests/insertion_scan_bruteforce.py)
at the tile's edges, against the indel scan with the inserts A, C, G, T, against the query-variant kernel on the same
insertions, the table and both frames against the brute force on the graphs test_gpu_mutation_scan.py uses, the refusals and
the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import insertion_scan_bruteforce as bf  # noqa: E402
import test_gpu_deletion_scan as dst  # noqa: E402  (its sequences: every size at a tile's edges, lower case, N at the edges)
import test_gpu_mutation_scan as mst  # noqa: E402  (its graphs, regions, motifs and default weights)
import wide_panel_cases as wp  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = mst.GOLD
BASES = mst.BASES
GRAPHS = mst.GRAPHS
THRESHOLD = mst.THRESHOLD
TABLE_INSERTS = (b"A", b"ACG", b"GATTACAGAT")
SEVEN = b"GATTACA"
LONG = b"ACGTTGCAAGGCTTAACCGGATATCGCGTATGCATGCAAGTCCTGAGGTTCCAAGGTCAGTCAA"
assert len(LONG) == 64


def _tile():
    from grafimo_amd import _native as nv
    return nv.GFM_INSSCAN_TILE


# ------------------------------------------------------------------------------------------- the kernel through scan_sequences
@functools.lru_cache(maxsize=None)
def _kernel_case(W, n_motifs, seed):
    rng = np.random.default_rng(seed)
    T = _tile()
    seqs = dst._sequences(W, T, rng)
    motifs = [SynMotif(W, seed=seed + 11 * k) for k in range(n_motifs)]
    # large entries: a double could not hold the sums (2 (W + 63) = 254 entries below 2^55 stay below 2^64)
    weights = [rng.integers(1 << 40, 1 << 55, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    return seqs, motifs, weights, off, np.frombuffer(b"".join(seqs), dtype=np.uint8)


def _check_kernel(W, n_motifs, seed, fwd, inserts):
    from grafimo_amd.insertion_scan import scan_sequences
    seqs, motifs, weights, off, bases = _kernel_case(W, n_motifs, seed)
    got = scan_sequences(motifs, off, bases, inserts, weights=weights, forward_only=fwd)
    assert len(got) == n_motifs
    N, K = len(bases), len(inserts)
    shortest = min(len(i) for i in inserts)
    for m in range(n_motifs):
        od = motif_as_oracle_dict(motifs[m])
        keys, sums = bf.scan_arrays(seqs, W, od["score_matrix"], od["min_val"], weights[m], fwd, inserts)
        assert got[m][0].shape == (K, N, 2) and got[m][0].dtype == np.uint32
        assert got[m][1].shape == (K, N, 2) and got[m][1].dtype == np.uint64
        assert got[m][0].tolist() == keys, (W, fwd, m, np.argwhere(got[m][0] != np.array(keys, dtype=np.uint32))[:5].tolist())
        assert got[m][1].tolist() == sums, (W, fwd, m, np.argwhere(got[m][1] != np.array(sums, dtype=np.uint64))[:5].tolist())
        # both columns hold empty and non-empty cells: the junction behind a sequence's last base has no window, and none at
        # all at W = 1; an ALT side is empty only where n + Li < W, which the sequence of one base is from W = 3 on; some sum no
        # double holds; JUNCTION is the same for every insert
        for c in range(2):
            assert (got[m][0][:, :, c] != 0).any() == (not (W == 1 and c == 0)), (W, c)
            assert (got[m][0][:, :, c] == 0).any() == (c == 0 or W > 1 + shortest), (W, c)
        assert int(got[m][1].max()) > 1 << 53
        for k in range(1, K):
            assert np.array_equal(got[m][0][k, :, 0], got[m][0][0, :, 0]) and np.array_equal(got[m][1][k, :, 0], got[m][1][0, :, 0])
    return got


@pytest.mark.parametrize("fwd", [False, True])
@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_kernel_against_brute_force(W, fwd):
    """both columns of every offset and insert, exactly, for two motifs of one width (grid.y)"""
    got = _check_kernel(W, 2, 101_000 + W, fwd, (b"A", LONG) if W == 64 else (b"A", b"CG", SEVEN, LONG))
    assert not np.array_equal(got[0][0], got[1][0])              # (two motifs, two answers)


def test_seventeen_motifs_take_two_launches():
    got = _check_kernel(2, 17, 102_000, False, (b"ACG", LONG))
    assert len({g[1].tobytes() for g in (got[0], got[15], got[16])}) == 3


@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_one_base_inserts_are_the_indel_scan(W):
    """inserts = (A, C, G, T): the columns JUNCTION and INS_A .. INS_T of indel_scan.scan_sequences, bit for bit"""
    from grafimo_amd import indel_scan, insertion_scan
    _, motifs, weights, off, bases = _kernel_case(W, 2, 101_000 + W)
    for fwd in (False, True):
        four = insertion_scan.scan_sequences(motifs, off, bases, ("A", "C", "G", "T"), weights=weights, forward_only=fwd)
        ind = indel_scan.scan_sequences(motifs, off, bases, weights=weights, forward_only=fwd)
        for m in range(2):
            assert four[m][0].shape == (4, len(bases), 2)
            for k in range(4):
                cols = [indel_scan.JUNCTION, indel_scan.INS_A + k]
                assert np.array_equal(four[m][0][k], ind[m][0][:, cols]), (W, fwd, m, k)
                assert np.array_equal(four[m][1][k], ind[m][1][:, cols]), (W, fwd, m, k)


def test_a_cell_does_not_depend_on_the_list():
    """the same insert alone, in a reordered list and in a list of sixteen: the same cells"""
    from grafimo_amd.insertion_scan import scan_sequences
    W = 19
    _, motifs, weights, off, bases = _kernel_case(W, 2, 101_000 + W)
    first = (b"A", b"CG", SEVEN, LONG)
    base = scan_sequences(motifs, off, bases, first, weights=weights)
    swapped = scan_sequences(motifs, off, bases, first[::-1], weights=weights)
    alone = [scan_sequences(motifs, off, bases, (i,), weights=weights) for i in first]
    many = tuple(bytes(BASES[(np.arange(n) * 7 + n) % 4].tolist()) for n in (3, 64, 11, 2, 33, 5, 63, 9, 17, 4, 21, 6)) + first
    assert len(many) == 16 and len(set(many)) == 16
    full = scan_sequences(motifs, off, bases, many, weights=weights)
    for m in range(2):
        for k in range(4):
            for other, j in ((swapped, 3 - k), (alone[k], 0), (full, 12 + k)):
                assert np.array_equal(other[m][0][j], base[m][0][k]) and np.array_equal(other[m][1][j], base[m][1][k]), (m, k)


def test_default_weights_a_second_call_and_empty_input():
    """the default weights are haplotype_affinity's; a second call gives the same arrays (nothing is left from the first)"""
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.insertion_scan import scan_sequences
    W, inserts = 7, (b"TG", b"ACGTACGTA")
    seqs, motifs, _, off, bases = _kernel_case(W, 1, 103_000)
    got = scan_sequences(motifs, off, bases, inserts, temperature=2.0)[0]
    dm = DeviceMotif.lease(motifs[0])
    try:
        w = default_weights(dm, 2.0)[0]
    finally:
        dm.release()
    od = motif_as_oracle_dict(motifs[0])
    keys, sums = bf.scan_arrays(seqs, W, od["score_matrix"], od["min_val"], w, False, inserts)
    assert got[0].tolist() == keys and got[1].tolist() == sums
    again = scan_sequences(motifs, off, bases, inserts, temperature=2.0)[0]
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    none = scan_sequences(motifs, [0, 0, 0], np.zeros(0, dtype=np.uint8), ("A", "ACGTT", LONG))[0]
    assert none[0].shape == (3, 0, 2) and none[1].shape == (3, 0, 2) and none[0].dtype == np.uint32 and none[1].dtype == np.uint64


# ------------------------------------------------------------------------------------------- against the existing kernel
@pytest.mark.parametrize("W", [5, 19])
def test_equals_the_query_variant_kernel_on_every_named_gap(W):
    """query_variants.score_edits on the insertion (coord[o] + 1, "", I) of a 5-mer and a 64-mer into every gap coordinates can
    name is applied at o + 1, with the scan's keys and sums, field for field"""
    from grafimo_amd import _native as nv
    from grafimo_amd.insertion_scan import scan_sequences
    from grafimo_amd.query_variants import score_edits
    rng = np.random.default_rng(104_000 + W)
    T = _tile()
    inserts = (b"GATTA", LONG)
    seqs, coords = [], []
    for n, start in ((T + W + 9, 100), (2 * W + 3, 4000), (W - 1, 7)):          # as test_gpu_indel_scan.py builds them
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
    motifs = [SynMotif(W, seed=1040 + k) for k in range(2)]
    weights = [rng.integers(1, 1 << 50, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    pos0, alts, item_seq, where = [], [], [], []
    unnamed = 0
    for v, (x, c) in enumerate(zip(seqs, coords)):
        pairs = [(~p, True) if p < 0 else (p, False) for p in c]
        for o in range(len(x)):
            if not bf.named(pairs, o):
                unnamed += 1
                continue
            for k, ins in enumerate(inserts):
                pos0.append(c[o] + 1); alts.append(ins); item_seq.append(v)
                where.append((k, int(off[v]) + o, o + 1))
    assert (coord < 0).any() and unnamed > 0 and len(where) > T
    assert any(T <= n < int(off[1]) for _, n, _ in where)        # (named gaps in the first sequence's second tile too)
    assert sum(1 for c in coords for a, b in zip(c, c[1:]) if a >= 0 and b >= 0 and b > a + 1) > 0    # a panel deletion
    assert sum(1 for v, x in enumerate(seqs) if (0, int(off[v + 1]) - 1, len(x)) in where) >= 1       # a sequence's last gap
    for fwd in (False, True):
        scan = scan_sequences(motifs, off, bases, inserts, weights=weights, forward_only=fwd)
        recs = score_edits(motifs, off, bases, coord, pos0, [b""] * len(pos0), alts, item_seq, np.arange(len(pos0)), weights=weights,
                           forward_only=fwd)
        k, n, o1 = (np.array(v) for v in zip(*where))
        for m in range(2):
            r = recs[m]
            assert (r["status"] == nv.GFM_EDIT_APPLIED).all() and np.array_equal(r["o"], o1)
            assert np.array_equal(r["ref_key"], scan[m][0][k, n, 0]) and np.array_equal(r["alt_key"], scan[m][0][k, n, 1]), (W, fwd, m)
            assert np.array_equal(r["ref_sum"], scan[m][1][k, n, 0]) and np.array_equal(r["alt_sum"], scan[m][1][k, n, 1]), (W, fwd, m)


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
                    [[bf.scan(d["bases"], od["width"], od["score_matrix"], od["min_val"], w, fwd, TABLE_INSERTS) for d in region]
                     for region in seqs]))
    return seqs, out


def _expected_rows(t, name, seqs, od, log2_offset, scans, every=False):
    """bf.detail_rows with the coordinates the table chose where a version has two sets (checked to be one of them), and the
    tail table the device made (the oracle's differs in the last digits)"""
    def coords_of(r, d):
        q = [int(q) for q in np.flatnonzero(t.seq_region == r) if int(t.seq_version[q]) == d["version"]]
        assert len(q) == 1, (name, r, d["version"])
        have = [(int(~c) if c < 0 else int(c), bool(c < 0)) for c in t.coord[t.seq_offsets[q[0]]:t.seq_offsets[q[0] + 1]].tolist()]
        assert have in d["coords"], (name, r, d["version"])
        return have
    return bf.detail_rows(t.region_names, seqs, scans, coords_of, od["width"], od["scale"], od["offset"], t.ptable, log2_offset,
                          THRESHOLD, TABLE_INSERTS, every)


def _same(x, y):
    return x == y or (x != x and y != y)


COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_a", "haplotypes_none", "is_reference",
           "position", "inserted", "insert", "length", "named", "ref_score", "ref_pvalue", "ref_start", "ref_strand", "ref_kmer",
           "alt_score", "alt_pvalue", "alt_start", "alt_strand", "alt_kmer", "ref_log2_affinity", "alt_log2_affinity",
           "delta_log2_affinity", "effect"]
SUMMARY_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "insert", "length", "versions", "haplotypes",
                   "haplotypes_gain", "haplotypes_loss", "min_delta_log2_affinity", "max_delta_log2_affinity", "best_alt_score"]
ROW_KEY = ("sequence_name", "version", "position", "inserted", "insert")


@pytest.mark.parametrize("name", GRAPHS)
def test_table_against_the_brute_force(name):
    from grafimo_amd.insertion_scan import compute_insertion_scan_many
    idx, regions, motifs, groups, fwd = mst._setup(name)
    seqs, exp = _expected(name)
    tables = compute_insertion_scan_many(motifs, idx, regions, False, wp.Args(threshold=THRESHOLD, no_reverse=fwd), TABLE_INSERTS,
                                         haplotype_groups=groups, all_rows=True)
    n_bases = sum(len(d["bases"]) for region in seqs for d in region)
    K = len(TABLE_INSERTS)
    order_of = {i.decode(): k for k, i in enumerate(TABLE_INSERTS)}
    for t, m, (od, ptab, log2_offset, scans) in zip(tables, motifs, exp):
        assert (t.motif_id, t.width, t.group_names, t.inserts) == (m.motif_id, od["width"], list(groups), TABLE_INSERTS)
        # ---- the sequences: the versions by number, the count-0 reference where no version is the reference's
        assert len(t.seq_count) == sum(len(region) for region in seqs) and len(t.bases) == n_bases
        assert t.keys.shape == (K, n_bases, 2) and t.sums.shape == (K, n_bases, 2)
        for r, region in enumerate(seqs):
            mine = np.flatnonzero(t.seq_region == r)
            order = sorted(mine.tolist(), key=lambda q: (t.seq_version[q] < 0, t.seq_version[q]))
            assert [(int(t.seq_version[q]), int(t.seq_count[q]), t.seq_group_counts[q].tolist(), bool(t.seq_is_reference[q]),
                     t.bases[t.seq_offsets[q]:t.seq_offsets[q + 1]].tobytes()) for q in order] == \
                [(d["version"], d["count"], d["group_counts"], d["is_reference"], d["bases"]) for d in region], (name, r)
            # ---- the dense arrays: both columns of every base and insert, the repeats' too
            for q, d, scan in zip(order, region, scans[r]):
                a, b = int(t.seq_offsets[q]), int(t.seq_offsets[q + 1])
                for k in range(K):
                    assert t.keys[k, a:b].tolist() == [[bf.key_of(best) for best, _ in row] for row in scan[k]], (name, m.motif_id, r, k)
                    assert t.sums[k, a:b].tolist() == [[int(s) for _, s in row] for row in scan[k]], (name, m.motif_id, r, k)
        # ---- all_rows: every gap a repeat does not repeat, every column
        rows = _expected_rows(t, name, seqs, od, log2_offset, scans)
        frame = t.to_frame()
        assert list(frame.columns) == COLUMNS
        assert len(frame) == len(rows) == len(t) and 0 < len(rows) < K * n_bases
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
        # ---- the summary against a loop over the rows of every gap
        want = bf.summary_of(_expected_rows(t, name, seqs, od, log2_offset, scans, every=True))
        s = t.summary_frame()
        assert list(s.columns) == SUMMARY_COLUMNS and len(s) == len(want)
        names = {n_: k for k, n_ in enumerate(t.region_names.tolist())}
        keys = [(f["sequence_name"], f["position"], f["insert"]) for f in s.to_dict("records")]
        assert keys == sorted(want, key=lambda q: (names[q[0]], q[1], order_of[q[2]])), name
        for f in s.to_dict("records"):
            w = want[(f["sequence_name"], f["position"], f["insert"])]
            assert (f["versions"], f["haplotypes"], f["haplotypes_gain"], f["haplotypes_loss"], f["length"]) == \
                (w["versions"], w["haplotypes"], w["haplotypes_gain"], w["haplotypes_loss"], len(f["insert"])), (name, f)
            assert _same(f["min_delta_log2_affinity"], min(w["deltas"]) if w["deltas"] else np.nan)
            assert _same(f["max_delta_log2_affinity"], max(w["deltas"]) if w["deltas"] else np.nan)
            assert _same(f["best_alt_score"], max(w["scores"]) if w["scores"] else np.nan)
        t.all_rows = False
        kept = {q for q, w in want.items() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0}
        assert {(f["sequence_name"], f["position"], f["insert"]) for f in t.summary_frame().to_dict("records")} == kept
        t.delta = 1.0
        kept = {q for q, w in want.items() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0 or
                (w["deltas"] and max(abs(min(w["deltas"])), abs(max(w["deltas"]))) >= 1.0)}
        assert {(f["sequence_name"], f["position"], f["insert"]) for f in t.summary_frame().to_dict("records")} == kept


def test_the_graphs_hold_every_case():
    """with the brute force alone: inserted anchor bases, a region whose reference no haplotype spells (the count-0 row), sides
    without a window, repeats, gaps no coordinates name, gains and losses"""
    inserted = added = short = repeats = unnamed = gain = loss = 0
    for name in GRAPHS:
        seqs, exp = _expected(name)
        for region in seqs:
            added += int(region[-1]["version"] < 0)
            inserted += sum(int(t) for d in region for _, t in d["coords"][0])
            for d in region:
                n = len(d["bases"])
                repeats += sum(int(not bf.reported(d["bases"], o, i)) for i in TABLE_INSERTS for o in range(n))
                unnamed += sum(int(not bf.named(d["coords"][0], o)) for o in range(n))
        for od, ptab, _, scans in exp:
            for region in scans:
                for scan in region:
                    for k in range(len(TABLE_INSERTS)):
                        for row in scan[k]:
                            short += int(row[0][0] is None) + int(row[1][0] is None)
                            e = bf.effect(ptab, THRESHOLD, row[0][0], row[1][0])
                            gain += int(e == "gain")
                            loss += int(e == "loss")
    counts = (inserted, added, short, repeats, unnamed, gain, loss)
    assert min(counts) >= 1, counts


# ------------------------------------------------------------------------------------------- refusals, command line
def test_refusals(monkeypatch):
    from grafimo_amd import _native as nv
    from grafimo_amd.insertion_scan import compute_insertion_scan, scan_sequences
    x = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)
    m5, m7 = SynMotif(5, seed=1), SynMotif(7, seed=2)
    m5.motif_id = "FIVE"
    with pytest.raises(nv.NativeError, match="one width"):
        scan_sequences([m5, m7], [0, 12], x, ("AC",))
    # an ALT side holds up to 2 (W + Lmax - 1) = 16 windows: 16 (2^60 - 1) fits, 16 x 2^60 does not
    with pytest.raises(nv.NativeError, match="a side holds up to 16 windows \\(W = 5, longest insert 4\\).* may pass 2\\^64"):
        scan_sequences([m5], [0, 12], x, ("A", "ACGT"), weights=[np.full(5001, 1 << 60, dtype=np.uint64)])
    scan_sequences([m5], [0, 12], x, ("A", "ACGT"), weights=[np.full(5001, (1 << 60) - 1, dtype=np.uint64)])
    with pytest.raises(nv.NativeError, match="may pass 2\\^64"):                 # (the longest insert counts, not the number)
        scan_sequences([m5], [0, 12], x, ("ACGTA",), weights=[np.full(5001, (1 << 60) - 1, dtype=np.uint64)])
    for bad in ((), ("",), ("A" * 65,), ("ANA",), ("AC", "ac"), ["A"] * 17):
        with pytest.raises(ValueError):
            scan_sequences([m5], [0, 12], x, bad)
    with pytest.raises(ValueError, match="FIVE: .* 576 bytes, more than max_bytes = 575"):
        scan_sequences([m5], [0, 12], x, ("A", "CG"), max_bytes=575)
    both = scan_sequences([m5, m5], [0, 12], x, ("A", "CG"), max_bytes=576)                          # one motif at a time
    assert np.array_equal(both[0][1], both[1][1]) and np.array_equal(both[0][1], scan_sequences([m5], [0, 12], x, ("A", "CG"))[0][1])
    with pytest.raises(ValueError, match="starts at 0"):
        scan_sequences([m5], [1, 12], x, ("A",))
    # the library's own checks of the inserts, which the module never lets through
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
        for count, ioff, text, message in ((2, [0, 2, 2], b"AC", b"length 0 of insert 1 is outside 1 .. 64"),
                                           (2, [0, 1, 66], b"A" * 66, b"length 65 of insert 1 is outside 1 .. 64"),
                                           (2, [0, 2, 4], b"ACNT", b"base 0 of insert 1 is not one of ACGTacgt"),
                                           (2, [0, 3, 1], b"ACG", b"insert_offsets descends at insert 1"),
                                           (2, [1, 2, 3], b"ACG", b"insert_offsets starts at 0"),
                                           (0, [0], b"A", b"bad argument"), (17, list(range(18)), b"A" * 17, b"bad argument")):
            io, tx = np.array(ioff, dtype=np.int32), np.frombuffer(text, dtype=np.uint8).copy()
            rc = nv.lib().gfm_sequence_insertion_scan(one(dm.handle), 1, one(d_w.data_ptr()), 1, 1, off.ctypes.data, d_x.data_ptr(), count,
                                                      io.ctypes.data, tx.ctypes.data, 0, one(keys.data_ptr()), one(sums.data_ptr()),
                                                      status.data_ptr(), None)
            assert rc == nv.GFM_ERR_INVALID and message in nv.lib().gfm_last_error(), (ioff, nv.lib().gfm_last_error())
        torch.cuda.synchronize()
        assert bool((keys == -1).all()) and bool((sums == -1).all())             # refused before anything was launched
    finally:
        dm.release()
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="the insertion scan is computed on one GPU"):
        compute_insertion_scan(m5, bf.hand_graph(), [(0, 20)], False, wp.Args(), ("AC",))


def _cli_case():
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    fa, vcf, bedfile = os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), os.path.join(GOLD, "regions.bed")
    bed = read_bed_regions(bedfile)
    return fa, vcf, bedfile, bed, [GraphIndex.from_fasta_vcf(fa, vcf, c[3:]) for c in bed]


def _run(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd"] + list(flags), check=True, cwd=str(tmp_path),
                          env=dict(os.environ, PYTHONPATH=ROOT), timeout=600, capture_output=True, text=True)


def test_cli_writes_both_files_and_prints_with_f(tmp_path):
    """--insertion-scan gattacagat ACG acg (folded, the repeat dropped, the order kept) with files and with -f, one motif"""
    from grafimo_amd.insertion_scan import compute_insertion_scan_many
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.workflow import Findmotif
    fa, vcf, bedfile, bed, graphs = _cli_case()
    meme = os.path.join(GOLD, "MA0139.1.meme")
    out = str(tmp_path / "o")
    common = ["-m", meme, "-l", fa, "-v", vcf, "-b", bedfile, "-t", "0.05", "--insertion-delta", "2.5", "--insertion-scan", "gattacagat",
              "ACG", "acg"]
    r = _run(tmp_path, *common, "-o", out)
    assert "insertion scan rows written to" in r.stdout and "insertion scan summary rows written to" in r.stdout
    wf = Findmotif(threshold=0.05)
    motif = get_motif_pwm(meme, wf, 2, True, pvalue_matrix=False)[0]
    t = compute_insertion_scan_many([motif], graphs, list(bed.values()), False, wp.Args(threshold=0.05), ("GATTACAGAT", "ACG"),
                                    delta=2.5)[0]
    detail = open(os.path.join(out, "grafimo_insertion_scan.tsv")).read()
    summary = open(os.path.join(out, "grafimo_insertion_scan_summary.tsv")).read()
    assert detail.split("\n", 1)[0].split("\t") == [c for c in COLUMNS if c not in ("haplotypes_a", "haplotypes_none")]
    assert summary.split("\n", 1)[0].split("\t") == SUMMARY_COLUMNS
    want_detail = t.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    want_summary = t.summary_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    assert len(t) > 0 and set(t.to_frame()["insert"]) == {"GATTACAGAT", "ACG"} and detail == want_detail and summary == want_summary
    r = _run(tmp_path, *common, "-f")
    assert want_detail + want_summary in r.stdout


def test_cli_names_the_files_of_two_motifs(tmp_path):
    fa, vcf, bedfile, _, _ = _cli_case()
    out = str(tmp_path / "o")
    r = _run(tmp_path, "-m", os.path.join(GOLD, "MA0139.1.meme"), os.path.join(GOLD, "MA0035.4.meme"), "-l", fa, "-v", vcf, "-b", bedfile,
             "-t", "0.05", "-o", out, "--insertion-scan", "ACG", "GATTACAGAT", "--insertion-all")
    assert r.stdout.count("insertion scan rows written to") == 2
    found = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs if "insertion_scan" in f)
    assert len(found) == 4 and sum("summary" in f for f in found) == 2 and not any(f.endswith("grafimo_insertion_scan.tsv") for f in found)
