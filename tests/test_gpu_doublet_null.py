"""The shuffle null of order 2 on the GPU: the kernel through null_sequences(order=2) against the brute force
(tests/doublet_null_bruteforce.py) -- all seven arrays exactly --, the edge of the LDS cap, the capped branch, what a
doublet-preserving shuffle means seen through the kernel's own outputs, what the result may not depend on, order 1 untouched,
the table and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import doublet_null_bruteforce as dbf  # noqa: E402
import mutation_scan_bruteforce as msbf  # noqa: E402
import shuffle_null_bruteforce as bf  # noqa: E402
import test_doublet_null_host as host  # noqa: E402
import test_gpu_mutation_scan as mst  # noqa: E402
import wide_panel_cases as wp  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
NAMES = ("obs_best", "obs_sum", "ge_best", "ge_sum", "rep_hits", "rep_best", "rep_sum")
DTYPES = dict(obs_best=np.int32, obs_sum=np.uint64, ge_best=np.uint32, ge_sum=np.uint32, rep_hits=np.uint64, rep_best=np.int32,
              rep_sum=np.uint64)
K = 130                                                  # two full blocks of 64 replicates and a partial one


def _offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64), np.frombuffer(b"".join(seqs), dtype=np.uint8)


def _random_sequence(n, rng, lower=0.15):
    x = bytearray(BASES[rng.integers(0, 4, size=n)].tobytes())
    for j in np.flatnonzero(rng.random(n) < lower).tolist():
        x[j] |= 0x20
    return x


def _same(got, want, what):
    """every array of one motif, exactly: shapes, dtypes and values"""
    S, k = len(want["obs_best"]), len(want["rep_hits"])
    for name in NAMES:
        assert got[name].dtype == DTYPES[name], (what, name)
        assert got[name].shape == {"rep_hits": (k,), "rep_best": (S, k), "rep_sum": (S, k)}.get(name, (S,)), (what, name)
        assert got[name].tolist() == want[name], (what, name)


def _equal(a, b):
    return all(np.array_equal(a[name], b[name]) for name in NAMES)


# ------------------------------------------------------------------------------------------- the kernel against the brute force
def _by_length(W, rng):
    """empty and short sequences between others; 129: three turns of the wave's counting sort"""
    return [bytes(_random_sequence(n, rng)) for n in (0, 1, 2, 3, W - 1, W, W + 1, 63, 64, 65, 129)]


def _by_content(rng):
    """a homopolymer, (AC)^m G, all-N, lower case, and an N at offset 0, at n - 1 and in the middle"""
    first, last, middle = _random_sequence(70, rng), _random_sequence(64, rng), _random_sequence(90, rng)
    first[0], last[63], middle[45] = ord("N"), ord("n"), ord("N")
    return [b"A" * 37, b"AC" * 33 + b"G", b"N" * 21, bytes(_random_sequence(50, rng)).lower(), bytes(first), bytes(last), bytes(middle)]


@pytest.mark.parametrize("fwd", [False, True])
@pytest.mark.parametrize("W", [2, 19])
def test_kernel_against_brute_force(W, fwd):
    from grafimo_amd.shuffle_null import null_sequences
    seed = 92_000 + W
    rng = np.random.default_rng(seed)
    motif = SynMotif(W, seed=seed)
    od = motif_as_oracle_dict(motif)
    # large entries: a double could not hold the sums (2 x 128 entries below 2^55 stay below 2^64)
    w = rng.integers(1 << 40, 1 << 55, size=1000 * W + 1, dtype=np.uint64)
    varied = 0
    for seqs in (_by_length(W, rng), _by_content(rng)):
        off, bases = _offsets(seqs)
        keys = rng.integers(0, 1 << 64, size=len(seqs), dtype=np.uint64)             # (all 64 bits of a key are used)
        sw = rng.integers(0, 8, size=len(seqs)).astype(np.uint32)
        reps = dbf.replicates(seqs, keys.tolist(), seed, K, W, od["score_matrix"], od["min_val"], w, fwd)
        assert not any(any(row) for row in reps["capped"])
        cut = max(reps["obs_best"])
        got = null_sequences([motif], off, bases, K, seed=seed, seq_keys=keys, seq_weights=sw, cuts=[cut], weights=[w],
                             forward_only=fwd, keep_replicates=True, order=2)[0]
        _same(got, bf.counts(reps, K, cut, sw.tolist()), (W, fwd, len(seqs)))
        varied += sum(int(len(set(row)) > 1) for row in reps["rep_sum"])
    assert varied >= 4 or W == 2                          # (W = 2: the doublets are the windows, every replicate ties)


def test_the_edge_of_the_lds_cap():
    """one sequence of exactly GFM_NULL_LDS_BASES bases (the largest image the LDS holds: order 2 shares order 1's image) and
    one of a base more, which is made in device memory"""
    from grafimo_amd import _native as nv
    from grafimo_amd.shuffle_null import content_keys, null_sequences
    cap, W, k, seed = nv.GFM_NULL_LDS_BASES, 19, 65, 93_000
    rng = np.random.default_rng(seed)
    motif = SynMotif(W, seed=930)
    od = motif_as_oracle_dict(motif)
    w = rng.integers(1 << 40, 1 << 53, size=1000 * W + 1, dtype=np.uint64)
    for n in (cap, cap + 1):
        x = _random_sequence(n, rng)
        x[n // 2] = ord("N")
        seqs = [b"acgtACGT", bytes(x)]                               # (the short one: two launches in one call)
        off, bases = _offsets(seqs)
        keys = content_keys(off, bases)
        want = dbf.null(seqs, keys.tolist(), seed, k, W, od["score_matrix"], od["min_val"], w, False, 9000)
        got = null_sequences([motif], off, bases, k, seed=seed, cuts=[9000], weights=[w], keep_replicates=True, order=2)[0]
        _same(got, want, n)
        assert len(set(want["rep_sum"][1])) > 1


@pytest.mark.parametrize("walk_cap", [0, 1])
def test_the_capped_branch(walk_cap):
    """the host test's sequence: at walk_cap 0 every replicate takes x's own last exits, at 1 a mixture"""
    from grafimo_amd.shuffle_null import null_sequences
    W, k = 5, 128
    motif = SynMotif(W, seed=940)
    od = motif_as_oracle_dict(motif)
    w = np.random.default_rng(94_000).integers(1, 1 << 50, size=1000 * W + 1, dtype=np.uint64)
    seqs = [host.CAP_SEQUENCE, b"ACGTTGCA" * 4]
    off, bases = _offsets(seqs)
    keys = [host.CAP_KEY, 1]
    reps = dbf.replicates(seqs, keys, host.CAP_SEED, k, W, od["score_matrix"], od["min_val"], w, False, walk_cap)
    capped = sum(reps["capped"][0])
    assert capped == k if walk_cap == 0 else 13 <= capped <= k - 13
    got = null_sequences([motif], off, bases, k, seed=host.CAP_SEED, seq_keys=np.array(keys, dtype=np.uint64), cuts=[2500],
                         weights=[w], keep_replicates=True, order=2, walk_cap=walk_cap)[0]
    _same(got, bf.counts(reps, k, 2500), walk_cap)
    full = null_sequences([motif], off, bases, k, seed=host.CAP_SEED, seq_keys=np.array(keys, dtype=np.uint64), cuts=[2500],
                          weights=[w], keep_replicates=True, order=2)[0]
    assert not np.array_equal(full["rep_sum"][0], got["rep_sum"][0])             # (the cap shows in the results)


# ------------------------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("fwd", [False, True])
def test_every_replicate_keeps_the_sums_of_width_1_and_2(fwd):
    """what a doublet-preserving shuffle means, without any brute force: at W = 2 the windows of a replicate are x's doublets,
    at W = 1 its bases, so rep_sum[v][r] == obs_sum[v] for every r under order 2 -- and not under order 1 at W = 2"""
    from grafimo_amd.shuffle_null import null_sequences
    rng = np.random.default_rng(95_000)
    seqs = [bytes(_random_sequence(40, rng, lower=0.0)), bytes(_random_sequence(131, rng)), b"ACGTNNACGTNACG", b"AC" * 33 + b"G", b"T"]
    off, bases = _offsets(seqs)
    for W in (2, 1):
        motif = SynMotif(W, seed=950 + W)
        w = rng.integers(1, 1 << 50, size=1000 * W + 1, dtype=np.uint64)
        run = lambda order: null_sequences([motif], off, bases, K, seed=3, weights=[w], forward_only=fwd, keep_replicates=True,    # noqa: E731
                                           order=order)[0]
        two = run(2)
        assert (two["rep_sum"] == two["obs_sum"][:, None]).all() and two["rep_sum"].shape == (len(seqs), K)
        assert (two["rep_best"] == two["obs_best"][:, None]).all() and two["ge_sum"].tolist() == [K] * len(seqs)
        assert two["obs_sum"][0] > 0 and two["obs_sum"][4] == (0 if W == 2 else two["obs_sum"][4])
        if W == 2:
            one = run(1)
            assert np.array_equal(one["obs_sum"], two["obs_sum"]) and (one["rep_sum"][0] != one["obs_sum"][0]).any()


def test_seventeen_motifs_take_two_launches():
    """motif 0 and motif 16, given the same matrix and weights, return identical arrays: the replicates do not depend on the
    motif, nor on the launch it is in"""
    from grafimo_amd.shuffle_null import null_sequences
    W, k, seed = 3, 70, 96_000
    rng = np.random.default_rng(seed)
    seqs = _by_length(W, rng)
    off, bases = _offsets(seqs)
    motifs = [SynMotif(W, seed=seed + j) for j in range(16)] + [SynMotif(W, seed=seed)]
    weights = [rng.integers(1, 1 << 50, size=1000 * W + 1, dtype=np.uint64) for _ in range(16)]
    weights.append(weights[0])
    got = null_sequences(motifs, off, bases, k, seed=seed, cuts=[1500] * 17, weights=weights, keep_replicates=True, order=2)
    assert len(got) == 17 and _equal(got[0], got[16])
    assert len({g["rep_sum"].tobytes() for g in got[:16]}) == 16
    keys = [bf.content_key(x) for x in seqs]
    for m in (0, 15):
        od = motif_as_oracle_dict(motifs[m])
        _same(got[m], dbf.null(seqs, keys, seed, k, W, od["score_matrix"], od["min_val"], weights[m], False, 1500), m)


def test_a_sequence_does_not_depend_on_its_neighbours_or_the_chunks():
    from grafimo_amd.shuffle_null import content_keys, null_sequences
    W, k, seed = 5, 70, 97_000
    rng = np.random.default_rng(seed)
    x = bytes(_random_sequence(90, rng))
    seqs = [bytes(_random_sequence(140, rng)), x, b"", bytes(_random_sequence(33, rng)), x]
    off, bases = _offsets(seqs)
    keys = content_keys(off, bases)
    motifs = [SynMotif(W, seed=970 + j) for j in range(2)]
    sw = np.array([1, 2, 3, 4, 5], dtype=np.uint32)
    run = lambda **kw: null_sequences(motifs, off, bases, k, seed=seed, seq_keys=keys, seq_weights=sw, cuts=[2500] * 2,      # noqa: E731
                                      keep_replicates=True, order=2, **kw)
    got = run()
    o1, b1 = _offsets([x])
    alone = null_sequences(motifs, o1, b1, k, seed=seed, cuts=[2500] * 2, keep_replicates=True, order=2)
    for a, g in zip(alone, got):
        for name in ("obs_best", "obs_sum", "ge_best", "ge_sum", "rep_best", "rep_sum"):
            assert np.array_equal(a[name][0], g[name][1]) and np.array_equal(g[name][1], g[name][4]), name
        assert len(set(g["rep_sum"][1].tolist())) > 1
    one = 20 + 12 * k + 8 * k                                        # one sequence of one motif with its dense rows
    assert all(_equal(a, b) for a, b in zip(got, run(max_bytes=one + 2 * (20 + 12 * k))))     # three sequences, one motif a chunk
    assert all(_equal(a, b) for a, b in zip(got, run(max_bytes=one)))


def test_order_1_given_explicitly_is_the_default_call():
    from grafimo_amd.shuffle_null import null_sequences
    W, seed = 7, 98_000
    rng = np.random.default_rng(seed)
    seqs = _by_length(W, rng)
    off, bases = _offsets(seqs)
    motifs = [SynMotif(W, seed=980), SynMotif(W, seed=981)]
    old = null_sequences(motifs, off, bases, K, seed=seed, cuts=[3000, 3500], keep_replicates=True)
    new = null_sequences(motifs, off, bases, K, seed=seed, cuts=[3000, 3500], keep_replicates=True, order=1, walk_cap=0)
    assert all(_equal(a, b) for a, b in zip(old, new))
    od = motif_as_oracle_dict(motifs[0])
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.haplotype_affinity import default_weights
    dm = DeviceMotif.lease(motifs[0])
    try:
        w = default_weights(dm, 1.0)[0]
    finally:
        dm.release()
    keys = [bf.content_key(x) for x in seqs]
    _same(new[0], bf.null(seqs, keys, seed, K, W, od["score_matrix"], od["min_val"], w, False, 3000), "order 1")
    two = null_sequences(motifs, off, bases, K, seed=seed, cuts=[3000, 3500], keep_replicates=True, order=2)
    assert np.array_equal(two[0]["obs_sum"], old[0]["obs_sum"]) and not np.array_equal(two[0]["rep_sum"], old[0]["rep_sum"])


# ------------------------------------------------------------------------------------------- the table, the command line
TABLE_K, TABLE_SEED = 65, 12
COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "is_reference", "length", "best_score",
           "best_pvalue", "best_null_pvalue", "log2_affinity", "affinity_null_pvalue", "replicates"]
ENRICHMENT_COLUMNS = ["motif_id", "motif_alt_id", "width", "regions", "observed_hits", "null_mean_hits", "null_max_hits",
                      "enrichment_pvalue", "replicates"]


def test_table_against_the_brute_force():
    from grafimo_amd.shuffle_null import compute_shuffle_null_many, enrichment_frame
    name = mst.GRAPHS[0]
    idx, regions, motifs, groups, fwd = mst._setup(name)
    seqs = [msbf.region_sequences(idx, S, E, list(groups.values())) for S, E in regions]
    flat = [d for region in seqs for d in region]
    xs = [d["bases"] for d in flat]
    keys = [bf.content_key(x) for x in xs]
    sw = [int(d["version"] == 0) for d in flat]
    tables = compute_shuffle_null_many(motifs, idx, regions, False, wp.Args(threshold=mst.THRESHOLD, no_reverse=fwd),
                                       haplotype_groups=groups, replicates=TABLE_K, seed=TABLE_SEED, order=2)
    for t, m in zip(tables, motifs):
        od = motif_as_oracle_dict(m)
        w, _ = mst._default_weights(od)
        want = dbf.null(xs, keys, TABLE_SEED, TABLE_K, od["width"], od["score_matrix"], od["min_val"], w, fwd, t.cut, sw)
        assert t.order == 2 and len(t) == len(flat)
        for name_ in NAMES[:5]:
            assert getattr(t, name_).tolist() == want[name_], (m.motif_id, name_)
        frame = t.to_frame()
        assert list(frame.columns)[-2:] == ["replicates", "null_order"] and (frame["null_order"] == 2).all()
    e = enrichment_frame(tables)
    assert list(e.columns) == ENRICHMENT_COLUMNS + ["null_order"] and e["null_order"].tolist() == [2] * len(motifs)
    ones = compute_shuffle_null_many(motifs[:1], idx, regions, False, wp.Args(threshold=mst.THRESHOLD, no_reverse=fwd),
                                     haplotype_groups=groups, replicates=TABLE_K, seed=TABLE_SEED)
    assert ones[0].order == 1 and "null_order" not in ones[0].to_frame() and list(enrichment_frame(ones).columns) == ENRICHMENT_COLUMNS


def test_cli_writes_the_null_order_column(tmp_path):
    fa, vcf, bedfile = os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), os.path.join(GOLD, "regions.bed")
    heads = {}
    for flags in ((), ("--null-order", "2")):
        out = str(tmp_path / f"o{len(flags)}")
        subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", fa, "-v", vcf, "-b", bedfile,
                        "-t", "0.05", "-o", out, "--shuffle-null", "65", *flags], check=True, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=600, capture_output=True, text=True)
        table = open(os.path.join(out, "grafimo_shuffle_null.tsv")).read().split("\n")
        enrichment = open(os.path.join(out, "grafimo_motif_enrichment.tsv")).read().split("\n")
        heads[flags] = (table[0].split("\t"), enrichment[0].split("\t"), table[1].split("\t"), enrichment[1].split("\t"))
    assert heads[()][:2] == (COLUMNS, ENRICHMENT_COLUMNS)
    assert heads[("--null-order", "2")][:2] == (COLUMNS + ["null_order"], ENRICHMENT_COLUMNS + ["null_order"])
    two = heads[("--null-order", "2")]
    assert two[2][-1] == "2" and two[3][-1] == "2" and two[2][:8] == heads[()][2][:8]        # (the observed columns are the same)
