"""The shuffle null on the GPU: the kernel through null_sequences against the brute force (tests/shuffle_null_bruteforce.py) --
dense arrays, counts and rep_hits exactly --, the scratch path at the LDS cap's edge, what the result may not depend on, the
table and the enrichment frame against the brute force on test_gpu_mutation_scan's graphs, the refusals and the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mutation_scan_bruteforce as msbf  # noqa: E402
import shuffle_null_bruteforce as bf  # noqa: E402
import test_gpu_mutation_scan as mst  # noqa: E402
import wide_panel_cases as wp  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
KS = (1, 63, 64, 65, 130)
NAMES = ("obs_best", "obs_sum", "ge_best", "ge_sum", "rep_hits", "rep_best", "rep_sum")
DTYPES = dict(obs_best=np.int32, obs_sum=np.uint64, ge_best=np.uint32, ge_sum=np.uint32, rep_hits=np.uint64, rep_best=np.int32,
              rep_sum=np.uint64)
THRESHOLD = mst.THRESHOLD
TABLE_K = 130
TABLE_SEED = 11


def _offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64), np.frombuffer(b"".join(seqs), dtype=np.uint8)


def _random_sequence(n, rng, lower=0.15):
    x = bytearray(BASES[rng.integers(0, 4, size=n)].tobytes())
    for j in np.flatnonzero(rng.random(n) < lower).tolist():
        x[j] |= 0x20
    return x


def _same(got, want, what):
    """every array of one motif, exactly: shapes, dtypes and values"""
    S, K = len(want["obs_best"]), len(want["rep_hits"])
    for name in NAMES:
        assert got[name].dtype == DTYPES[name], (what, name)
        assert got[name].shape == {"rep_hits": (K,), "rep_best": (S, K), "rep_sum": (S, K)}.get(name, (S,)), (what, name)
        assert got[name].tolist() == want[name], (what, name)


# ------------------------------------------------------------------------------------------- the kernel through null_sequences
def _lengths(W):
    """in this order: empty and short sequences between others"""
    return [0, 1, W - 1, W, W + 1, 63, 64, 65, 2 * 64 + 3]


def _sequences(W, rng):
    """random sequences of _lengths with lower-case bases; an N at offset 0, at n - 1 and in the middle of a sequence"""
    seqs = []
    for n in _lengths(W):
        x = _random_sequence(n, rng)
        if n == 65:
            x[0] = ord("N")
        if n == 64:
            x[n - 1] = ord("n")
        if n == 2 * 64 + 3:
            x[70] = ord("N")
        seqs.append(bytes(x))
    return seqs


@functools.lru_cache(maxsize=None)
def _kernel_case(W, n_motifs, seed, fwd):
    """-> (sequences, motifs, weights, keys, seq_weights, per motif the brute force's replicates for the largest K)"""
    rng = np.random.default_rng(seed)
    seqs = _sequences(W, rng)
    motifs = [SynMotif(W, seed=seed + 11 * k) for k in range(n_motifs)]
    # large entries: a double could not hold the sums (2 x 131 entries below 2^55 stay below 2^64)
    weights = [rng.integers(1 << 40, 1 << 55, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    keys = rng.integers(0, 1 << 64, size=len(seqs), dtype=np.uint64)                 # (all 64 bits of a key are used)
    seq_weights = np.array([3, 0, 1, 2, 5, 1, 7, 1, 4], dtype=np.uint32)
    reps = []
    for m, w in zip(motifs, weights):
        od = motif_as_oracle_dict(m)
        reps.append(bf.replicates(seqs, keys.tolist(), seed, max(KS), W, od["score_matrix"], od["min_val"], w, fwd))
    return seqs, motifs, weights, keys, seq_weights, reps


@pytest.mark.parametrize("fwd", [False, True])
@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_kernel_against_brute_force(W, fwd):
    """dense arrays, counts and rep_hits of two motifs for K on both sides of a wavefront's 64 replicates; the cuts 0, L and an
    observed score; non-unit weights with a 0 among them"""
    from grafimo_amd.shuffle_null import null_sequences
    seed = 81_000 + W
    seqs, motifs, weights, keys, seq_weights, reps = _kernel_case(W, 2, seed, fwd)
    off, bases = _offsets(seqs)
    L = 1000 * W + 1
    cuts_of = [0, L, reps[0]["obs_best"][-1], reps[1]["obs_best"][-1]]
    assert max(max(row) for r in reps for row in r["rep_sum"]) > 1 << 53
    assert any(b < 0 for b in reps[0]["obs_best"]) and any(b >= 0 for b in reps[0]["obs_best"])       # shorter than W, and longer
    for i, K in enumerate(KS):
        cuts = [cuts_of[i % 4], cuts_of[(i + 1) % 4]]
        got = null_sequences(motifs, off, bases, K, seed=seed, seq_keys=keys, seq_weights=seq_weights, cuts=cuts, weights=weights,
                             forward_only=fwd, keep_replicates=True)
        assert len(got) == 2
        for m in range(2):
            _same(got[m], bf.counts(reps[m], K, cuts[m], seq_weights.tolist()), (W, fwd, K, m))
            assert got[m]["cut"] == cuts[m]
        assert not np.array_equal(got[0]["rep_sum"], got[1]["rep_sum"])          # (two motifs, two answers)
        if K == max(KS):                                                        # a sequence shorter than W: ge = K
            short = [v for v, x in enumerate(seqs) if len(x) < W]
            assert got[0]["ge_best"][short].tolist() == [K] * len(short) and got[0]["ge_sum"][short].tolist() == [K] * len(short)
            assert (got[0]["ge_best"] < K).any() or W == 1                     # (W = 1: a shuffle keeps every window)
    # without keep_replicates the dense arrays are not made and the rest is the same
    lean = null_sequences(motifs, off, bases, 65, seed=seed, seq_keys=keys, seq_weights=seq_weights, cuts=[0, L], weights=weights,
                          forward_only=fwd)
    for m in range(2):
        want = bf.counts(reps[m], 65, [0, L][m], seq_weights.tolist())
        assert sorted(lean[m]) == ["cut", "ge_best", "ge_sum", "obs_best", "obs_sum", "rep_hits"]
        assert all(lean[m][name].tolist() == want[name] for name in NAMES[:5])


# ------------------------------------------------------------------------------------------- the scratch path
def test_scratch_path_at_the_edge_of_the_lds_cap():
    """one sequence of GFM_NULL_LDS_BASES + 1 bases (shuffled in device memory) and one of exactly the cap (the largest image the
    LDS holds), each equal to the brute force"""
    from grafimo_amd import _native as nv
    from grafimo_amd.shuffle_null import content_keys, null_sequences
    cap, W, K, seed = nv.GFM_NULL_LDS_BASES, 19, 65, 82_000
    rng = np.random.default_rng(seed)
    motif = SynMotif(W, seed=820)
    od = motif_as_oracle_dict(motif)
    w = rng.integers(1 << 40, 1 << 53, size=1000 * W + 1, dtype=np.uint64)
    for n in (cap + 1, cap):
        x = _random_sequence(n, rng)
        x[n // 2] = ord("N")
        seqs = [b"acgtACGT", bytes(x)]                               # (the short one: two launches in one call)
        off, bases = _offsets(seqs)
        keys = content_keys(off, bases)
        assert keys.tolist() == [bf.content_key(s) for s in seqs]
        want = bf.null(seqs, keys.tolist(), seed, K, W, od["score_matrix"], od["min_val"], w, False, 9000)
        got = null_sequences([motif], off, bases, K, seed=seed, cuts=[9000], weights=[w], keep_replicates=True)[0]
        _same(got, want, n)
        assert len(set(want["rep_best"][1])) > 1


# ------------------------------------------------------------------------------------------- invariances
def _equal(a, b):
    return all(np.array_equal(a[name], b[name]) for name in NAMES)


def test_seventeen_motifs_take_two_launches():
    """motif 0 and motif 16, given the same matrix and weights, return identical arrays: the permutations do not depend on the
    motif, nor on the launch it is in"""
    from grafimo_amd.shuffle_null import null_sequences
    W, K, seed = 2, 70, 83_000
    seqs, _, _, keys, seq_weights, _ = _kernel_case(W, 2, 81_000 + W, False)
    off, bases = _offsets(seqs)
    rng = np.random.default_rng(seed)
    motifs = [SynMotif(W, seed=seed + k) for k in range(16)] + [SynMotif(W, seed=seed)]
    weights = [rng.integers(1, 1 << 50, size=1000 * W + 1, dtype=np.uint64) for _ in range(16)]
    weights.append(weights[0])
    cuts = [700] * 17
    got = null_sequences(motifs, off, bases, K, seed=seed, seq_keys=keys, seq_weights=seq_weights, cuts=cuts, weights=weights,
                         keep_replicates=True)
    assert len(got) == 17 and _equal(got[0], got[16])
    assert len({g["rep_sum"].tobytes() for g in got[:16]}) == 16
    for m in (0, 15):
        od = motif_as_oracle_dict(motifs[m])
        _same(got[m], bf.null(seqs, keys.tolist(), seed, K, W, od["score_matrix"], od["min_val"], weights[m], False, 700,
                              seq_weights.tolist()), m)


def test_a_sequence_does_not_depend_on_its_neighbours_its_call_or_the_chunks():
    from grafimo_amd.shuffle_null import content_keys, null_sequences
    W, K, seed = 5, 70, 84_000
    rng = np.random.default_rng(seed)
    x, z = bytes(_random_sequence(90, rng)), bytes(_random_sequence(33, rng))
    seqs = [bytes(_random_sequence(140, rng)), x, b"", z, x, bytes(_random_sequence(301, rng)), x]
    off, bases = _offsets(seqs)
    keys = content_keys(off, bases)
    keys[6] += np.uint64(1)                                          # the same bytes under another key
    motifs = [SynMotif(W, seed=840 + k) for k in range(3)]
    sw = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.uint32)
    run = lambda **kw: null_sequences(motifs, off, bases, K, seed=seed, seq_keys=keys, seq_weights=sw, cuts=[2500] * 3,      # noqa: E731
                                      keep_replicates=True, **kw)
    got = run()
    # ---- a second call gives the same arrays
    again = run()
    assert all(_equal(a, b) for a, b in zip(got, again))
    # ---- equal sequences with equal keys give equal rows; with different keys the same observed pair but other replicates
    for g in got:
        for name in ("obs_best", "obs_sum", "ge_best", "ge_sum", "rep_best", "rep_sum"):
            assert np.array_equal(g[name][1], g[name][4]), name
        assert (g["obs_best"][6], g["obs_sum"][6]) == (g["obs_best"][1], g["obs_sum"][1])
        assert not np.array_equal(g["rep_sum"][6], g["rep_sum"][1])
    # ---- a sequence alone equals the same sequence and key among others
    o1, b1 = _offsets([x])
    alone = null_sequences(motifs, o1, b1, K, seed=seed, seq_keys=keys[1:2], cuts=[2500] * 3, keep_replicates=True)
    for a, g in zip(alone, got):
        for name in ("obs_best", "obs_sum", "ge_best", "ge_sum", "rep_best", "rep_sum"):
            assert np.array_equal(a[name][0], g[name][1]), name
    assert np.array_equal(alone[0]["rep_best"][0], null_sequences(motifs[:1], o1, b1, K, seed=seed, keep_replicates=True)[0]["rep_best"][0])
    # ---- another seed gives other replicates, the same observed pair
    other = null_sequences(motifs, off, bases, K, seed=seed + 1, seq_keys=keys, seq_weights=sw, cuts=[2500] * 3, keep_replicates=True)
    assert np.array_equal(other[0]["obs_sum"], got[0]["obs_sum"]) and not np.array_equal(other[0]["rep_sum"], got[0]["rep_sum"])
    # ---- max_bytes small enough to split both motifs and sequences: identical, rep_hits included
    one = 20 + 12 * K + 8 * K                                        # one sequence of one motif with its dense rows
    split = run(max_bytes=one + 2 * (20 + 12 * K))                   # three sequences a chunk, one motif a chunk
    assert all(_equal(a, b) for a, b in zip(got, split))
    assert all(_equal(a, b) for a, b in zip(got, run(max_bytes=one)))
    with pytest.raises(ValueError, match=f"{motifs[0].motif_id}: .* {one} bytes, more than max_bytes = {one - 1}"):
        run(max_bytes=one - 1)
    # ---- no sequences gives empty arrays
    none = null_sequences(motifs, [0], np.zeros(0, dtype=np.uint8), K, keep_replicates=True)
    assert len(none) == 3 and none[0]["obs_best"].shape == (0,) and none[0]["rep_best"].shape == (0, K)
    assert none[0]["rep_hits"].tolist() == [0] * K


def test_default_weights_keys_and_cuts():
    """the defaults: haplotype_affinity's weights at the temperature, content keys, unit sequence weights, the cut at L"""
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.shuffle_null import null_sequences
    W, K = 7, 66
    rng = np.random.default_rng(85_000)
    seqs = [bytes(_random_sequence(n, rng)) for n in (40, 6, 70)]
    off, bases = _offsets(seqs)
    motif = SynMotif(W, seed=850)
    dm = DeviceMotif.lease(motif)
    try:
        w = default_weights(dm, 2.0)[0]
    finally:
        dm.release()
    od = motif_as_oracle_dict(motif)
    keys = [bf.content_key(x) for x in seqs]
    got = null_sequences([motif], off, bases, K, seed=5, temperature=2.0, keep_replicates=True)[0]
    _same(got, bf.null(seqs, keys, 5, K, W, od["score_matrix"], od["min_val"], w, False, 1000 * W + 1), "defaults")
    assert got["cut"] == 1000 * W + 1 and got["rep_hits"].tolist() == [0] * K


# ------------------------------------------------------------------------------------------- the table against the brute force
@functools.lru_cache(maxsize=None)
def _expected(name):
    """the brute force alone -> (per region its sequences, per motif (od, ptable, log2 offset, replicates over the sequences in
    the table's order: by region, a region's versions by number, its reference sequence last))"""
    from oracle import oracle as orc
    idx, regions, motifs, groups, fwd = mst._setup(name)
    seqs = [msbf.region_sequences(idx, S, E, list(groups.values())) for S, E in regions]
    flat = [d["bases"] for region in seqs for d in region]
    keys = [bf.content_key(x) for x in flat]
    out = []
    for m in motifs:
        od = motif_as_oracle_dict(m)
        w, log2_offset = mst._default_weights(od)
        out.append((od, orc.p_table(od["pmf"]), log2_offset,
                    bf.replicates(flat, keys, TABLE_SEED, TABLE_K, od["width"], od["score_matrix"], od["min_val"], w, fwd)))
    return seqs, out


def _nan_same(x, y):
    return x == y or (x != x and y != y)


COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_a", "haplotypes_none", "is_reference",
           "length", "best_score", "best_pvalue", "best_null_pvalue", "log2_affinity", "affinity_null_pvalue", "replicates"]
ENRICHMENT_COLUMNS = ["motif_id", "motif_alt_id", "width", "regions", "observed_hits", "null_mean_hits", "null_max_hits",
                      "enrichment_pvalue", "replicates"]


@pytest.mark.parametrize("name", mst.GRAPHS)
def test_table_against_the_brute_force(name):
    from grafimo_amd.shuffle_null import compute_shuffle_null_many, enrichment_frame
    idx, regions, motifs, groups, fwd = mst._setup(name)
    seqs, exp = _expected(name)
    tables = compute_shuffle_null_many(motifs, idx, regions, False, wp.Args(threshold=THRESHOLD, no_reverse=fwd),
                                       haplotype_groups=groups, replicates=TABLE_K, seed=TABLE_SEED)
    flat = [(r, d) for r, region in enumerate(seqs) for d in region]
    K = TABLE_K
    loop = []
    for t, m, (od, _, log2_offset, reps) in zip(tables, motifs, exp):
        W = od["width"]
        # the cut from the tail table the device made (test_gpu_query_variants.py reads its p-values the same way: the oracle's
        # differs in the last digits); the smallest score with p < threshold, L if none
        cut = next((s for s in range(len(t.ptable)) if t.ptable[s] < THRESHOLD), len(t.ptable))
        assert t.cut == cut and len(t.ptable) == 1000 * W + 1
        sw = [int(d["version"] == 0) for _, d in flat]
        want = bf.counts(reps, K, cut, sw)
        assert (t.motif_id, t.width, t.group_names, t.replicates, t.seed) == (m.motif_id, W, list(groups), K, TABLE_SEED)
        assert t.seq_weight.tolist() == sw and sum(sw) == len(regions)
        for name_ in NAMES[:5]:
            assert getattr(t, name_).tolist() == want[name_], (name, m.motif_id, name_)
        # ---- every frame column; the count-0 reference row
        frame = t.to_frame()
        assert list(frame.columns) == COLUMNS and len(frame) == len(flat) == len(t)
        for v, (f, (r, d)) in enumerate(zip(frame.to_dict("records"), flat)):
            n, ob, os_ = len(d["bases"]), want["obs_best"][v], want["obs_sum"][v]
            e = dict(motif_id=m.motif_id, motif_alt_id=m.motif_name, sequence_name=t.region_names[r], version=d["version"],
                     haplotypes=d["count"], haplotypes_a=d["group_counts"][0], haplotypes_none=d["group_counts"][1],
                     is_reference=d["is_reference"], length=n, replicates=K,
                     best_score=float(ob) / float(od["scale"]) + float(W) * od["offset"] if n >= W else float("nan"),
                     best_pvalue=float(t.ptable[ob]) if n >= W else float("nan"),
                     best_null_pvalue=(1.0 + want["ge_best"][v]) / (K + 1.0) if n >= W else float("nan"),
                     log2_affinity=float(np.log2(float(os_))) + log2_offset if n >= W else float("nan"),
                     affinity_null_pvalue=(1.0 + want["ge_sum"][v]) / (K + 1.0) if n >= W else float("nan"))
            for c in COLUMNS:
                assert _nan_same(f[c], e[c]), (name, m.motif_id, v, c, f[c], e[c])
            if d["version"] < 0:
                assert (f["haplotypes"], f["is_reference"]) == (0, True)
                assert v + 1 == len(flat) or flat[v + 1][0] == r + 1                    # the last row of its region
        # ---- the enrichment row, by a loop
        observed = sum(sw[v] for v in range(len(flat)) if want["obs_best"][v] >= cut)
        loop.append(dict(motif_id=m.motif_id, motif_alt_id=m.motif_name, width=W, regions=len(regions), observed_hits=observed,
                         null_mean_hits=sum(want["rep_hits"]) / K, null_max_hits=max(want["rep_hits"]),
                         enrichment_pvalue=(1.0 + sum(1 for h in want["rep_hits"] if h >= observed)) / (K + 1.0), replicates=K))
    e = enrichment_frame(tables)
    assert list(e.columns) == ENRICHMENT_COLUMNS and len(e) == len(motifs)
    for f, want_row in zip(e.to_dict("records"), loop):
        for c in ENRICHMENT_COLUMNS:
            assert f[c] == want_row[c], (name, c, f[c], want_row[c])          # (the hits are integers: their mean is exact)


def test_the_graphs_hold_every_case():
    """with the brute force alone: a sequence shorter than the motif, a row with ge_best < K, a region whose version 0 is not the
    reference's, a count-0 reference row, and a replicate that reaches a cut"""
    short = below = other = added = hit = 0
    for name in mst.GRAPHS:
        seqs, exp = _expected(name)
        for region in seqs:
            other += int(not region[0]["is_reference"])
            added += int(region[-1]["version"] < 0)
        flat = [d for region in seqs for d in region]
        for od, ptab, _, reps in exp:
            cut = next((s for s in range(len(ptab)) if ptab[s] < THRESHOLD), len(ptab))
            want = bf.counts(reps, TABLE_K, cut, [int(d["version"] == 0) for d in flat])
            short += sum(int(len(d["bases"]) < od["width"]) for d in flat)
            below += sum(int(g < TABLE_K) for g in want["ge_best"])
            hit += int(max(want["rep_hits"]) > 0)
    assert min(short, below, other, added, hit) >= 1, (short, below, other, added, hit)


# ------------------------------------------------------------------------------------------- refusals, command line
def test_refusals(monkeypatch):
    from grafimo_amd import _native as nv
    from grafimo_amd.shuffle_null import compute_shuffle_null, null_sequences
    x = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)
    m5, m7 = SynMotif(5, seed=1), SynMotif(7, seed=2)
    m5.motif_id = "FIVE"
    with pytest.raises(nv.NativeError, match="one width"):
        null_sequences([m5, m7], [0, 12], x, 10)
    with pytest.raises(nv.NativeError, match="may pass 2\\^64"):
        null_sequences([m5], [0, 12], x, 10, weights=[np.full(5001, 1 << 60, dtype=np.uint64)])     # 2 x 8 windows of them
    null_sequences([m5], [0, 12], x, 10, weights=[np.full(5001, (1 << 60) - 1, dtype=np.uint64)])   # 16 of them fit
    null_sequences([m5], [0, 4], x[:4], 10, weights=[np.full(5001, (1 << 64) - 1, dtype=np.uint64)])     # no window, no sum
    for cut in (-1, 5002):
        with pytest.raises(nv.NativeError, match=f"the cut {cut} of motif 0 lies outside \\[0, 5001\\]"):
            null_sequences([m5], [0, 12], x, 10, cuts=[cut])
    null_sequences([m5], [0, 12], x, 10, cuts=[5001])
    for K in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match="outside \\[1, 1048576\\]"):
            null_sequences([m5], [0, 12], x, K)
    with pytest.raises(ValueError, match="FIVE: the results of sequence 0 alone .* 100 bytes, more than max_bytes = 99"):
        null_sequences([m5], [0, 12], x, 10, max_bytes=99)
    with pytest.raises(ValueError, match="starts at 0"):
        null_sequences([m5], [1, 12], x, 10)
    with pytest.raises(ValueError, match="seq_keys of shape"):
        null_sequences([m5], [0, 12], x, 10, seq_keys=[1, 2])
    with pytest.raises(ValueError, match="2 cuts for 1 motifs"):
        null_sequences([m5], [0, 12], x, 10, cuts=[1, 2])
    # the library's own: replicates out of range, an unknown flag, offsets that descend, 2^31 bases, a NULL pointer
    lib = nv.lib()
    def call(n_seqs, off, K, flags):
        return lib.gfm_sequence_shuffle_null(None, 1, None, 1, n_seqs, off, None, None, None, K, 0, None, flags, *([None] * 9))
    assert call(0, None, 1, 0) == nv.GFM_OK
    assert call(0, None, 1, 2) == nv.GFM_ERR_INVALID and b"unknown flag" in lib.gfm_last_error()
    assert call(0, None, (1 << 20) + 1, 0) == nv.GFM_ERR_INVALID and b"outside [1, 2^20]" in lib.gfm_last_error()
    off = np.array([0, 5, 3], dtype=np.int64)
    assert call(2, off.ctypes.data, 1, 0) == nv.GFM_ERR_INVALID and b"descends" in lib.gfm_last_error()
    off = np.array([0, 1 << 31], dtype=np.int64)
    assert call(1, off.ctypes.data, 1, 0) == nv.GFM_ERR_INVALID and b"2^31" in lib.gfm_last_error()
    off = np.array([0, 4], dtype=np.int64)
    assert call(1, off.ctypes.data, 1, 0) == nv.GFM_ERR_INVALID and b"NULL argument" in lib.gfm_last_error()
    import torch
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="the shuffle null is computed on one GPU"):
        compute_shuffle_null(m5, msbf.hand_graph(), [(0, 20)], False, wp.Args())


def test_cli_writes_both_files(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.shuffle_null import compute_shuffle_null_many, enrichment_frame
    from grafimo_amd.workflow import Findmotif
    fa, vcf, bedfile = os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), os.path.join(GOLD, "regions.bed")
    bed = read_bed_regions(bedfile)
    graphs = [GraphIndex.from_fasta_vcf(fa, vcf, c[3:]) for c in bed]
    out = str(tmp_path / "o")
    r = subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", fa, "-v", vcf, "-b", bedfile,
                        "-t", "0.05", "-o", out, "--shuffle-null", "70", "--null-seed", "3"], check=True, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=600, capture_output=True, text=True)
    assert "shuffle null rows written to" in r.stdout and "1 motif enrichment rows written to" in r.stdout
    wf = Findmotif(threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "MA0139.1.meme"), wf, 2, True, pvalue_matrix=False)[0]
    tables = compute_shuffle_null_many([motif], graphs, list(bed.values()), False, wp.Args(threshold=0.05), replicates=70, seed=3)
    table = open(os.path.join(out, "grafimo_shuffle_null.tsv")).read()
    enrichment = open(os.path.join(out, "grafimo_motif_enrichment.tsv")).read()
    assert table.split("\n", 1)[0].split("\t") == [c for c in COLUMNS if c not in ("haplotypes_a", "haplotypes_none")]
    assert enrichment.split("\n", 1)[0].split("\t") == ENRICHMENT_COLUMNS
    assert len(tables[0]) > 0 and table == tables[0].to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    assert enrichment == enrichment_frame(tables).to_csv(sep="\t", index=False, lineterminator="\n")
    assert (tables[0].to_frame()["replicates"] == 70).all()
