"""The shuffle null of order 2 without a GPU: the rule's known answers, what every replicate keeps, the uniformity over the
doublet-preserving rearrangements, the capped branch, the frames' null_order column, the export, the header and the refusals."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import doublet_null_bruteforce as dbf  # noqa: E402
import shuffle_null_bruteforce as bf  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
# (AC)^20 is doublet-poor: the walk from A leaves the head only through C's one exit to G, so at walk_cap = 1 (n steps) about a
# third of the replicates is capped; the tail's N gives the arborescence a choice, so that the capped branch can show
CAP_SEQUENCE = b"AC" * 20 + b"GTTGNGTGnTG"
CAP_KEY, CAP_SEED = 777, 5


# ------------------------------------------------------------------------------------------- the rule
def test_known_answers():
    c = dbf.codes(b"ACGATCAGTACA")
    assert c == [0, 1, 2, 0, 3, 1, 0, 2, 3, 0, 1, 0] and dbf.codes(b"acgtNn-x") == [0, 1, 2, 3, 4, 4, 4, 4]
    got = [dbf.replicate(c, 12345, 0, r, 64) for r in range(4)]
    assert [dbf.spell(y) for y, _ in got] == [b"AGTCACGATACA", b"ATCACGTAGACA", b"AGTCACACGATA", b"ACACAGATCGTA"]
    assert not any(capped for _, capped in got)
    # the key and the seed both matter; the order-2 stream is not the order-1 stream
    assert dbf.replicate(c, 12346, 0, 0)[0] != got[0][0] and dbf.replicate(c, 12345, 1, 0)[0] != got[0][0]
    assert dbf.replicate([], 1, 2, 3) == ([], False) and dbf.replicate([4], 1, 2, 3) == ([4], False)
    assert dbf.replicate([2, 3], 1, 2, 3) == ([2, 3], False)


def _doublets(c):
    return collections.Counter(zip(c[:-1], c[1:]))


@pytest.mark.parametrize("walk_cap", [64, 0])
def test_every_replicate_keeps_length_ends_and_doublets(walk_cap):
    rng = np.random.default_rng(91_000)
    some_capped = 0
    for n in range(81):
        c = rng.integers(0, 5 if n % 3 == 0 else 4, size=n).tolist()
        for r in (0, 1, 77):
            y, capped = dbf.replicate(c, 1000 + n, 9, r, walk_cap)
            assert len(y) == n and y[:1] == c[:1] and y[-1:] == c[-1:] and _doublets(y) == _doublets(c), (n, r)
            some_capped += int(capped)
            if walk_cap == 0 and capped:                            # x's own last exits: a valid arborescence, another sequence
                assert sorted(y) == sorted(c)
    assert (some_capped > 0) == (walk_cap == 0)


def _rearrangements(c):
    """every sequence with c's first code, last code and doublet counts, by DFS over the doublets left"""
    left, out = _doublets(c), []

    def walk(path):
        if len(path) == len(c):
            out.append(tuple(path))
            return
        for a in range(5):
            if left[(path[-1], a)] > 0:
                left[(path[-1], a)] -= 1
                path.append(a)
                walk(path)
                path.pop()
                left[(path[-1], a)] += 1
    walk([c[0]])
    assert all(p[-1] == c[-1] for p in out) and len(set(out)) == len(out)
    return out


def _quantile(df):
    """the 1 - 10^-6 quantile of chi-square at df degrees of freedom: scipy's, or Wilson-Hilferty with z = 4.7534"""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - 1e-6, df))
    except ImportError:
        return df * (1.0 - 2.0 / (9.0 * df) + 4.7534 * (2.0 / (9.0 * df)) ** 0.5) ** 3


@pytest.mark.parametrize("x,D", [(b"ACGATCAGTACA", 132), (b"GATTACAGATTA", 36), (b"ACGTNACGTAAC", 6)])
def test_uncapped_replicates_are_uniform(x, D):
    """1000 D replicates under key 12345, seed 0: every one a rearrangement, chi-square below the 1 - 10^-6 quantile at D - 1
    degrees of freedom (223.0, 90.5, 37.5).  The seed is fixed, so the outcome is: 143.2, 36.8 and 9.3."""
    c = dbf.codes(x)
    all_of_them = _rearrangements(c)
    assert len(all_of_them) == D
    seen = collections.Counter(tuple(dbf.replicate(c, 12345, 0, r)[0]) for r in range(1000 * D))
    assert set(seen) <= set(all_of_them)
    chi = sum((seen[p] - 1000.0) ** 2 / 1000.0 for p in all_of_them)
    print(x, D, chi, _quantile(D - 1))
    assert _quantile(D - 1) <= {132: 223.0, 36: 90.5, 6: 37.5}[D] + 0.05             # (the exact quantile at 5 is 35.9)
    assert chi < _quantile(D - 1), chi


def test_the_cap_sequence_runs_both_branches():
    """at walk_cap = 1 at least 10 % of 128 replicates are capped and at least 10 % are not; the capped ones keep the doublets
    and differ from what walk_cap = 64 gives for some r; the uncapped ones do not depend on the cap"""
    c = dbf.codes(CAP_SEQUENCE)
    one = [dbf.replicate(c, CAP_KEY, CAP_SEED, r, 1) for r in range(128)]
    full = [dbf.replicate(c, CAP_KEY, CAP_SEED, r, 64) for r in range(128)]
    capped = [cp for _, cp in one]
    assert sum(capped) >= 13 and 128 - sum(capped) >= 13 and not any(cp for _, cp in full)
    assert any(a[0] != b[0] for a, b in zip(one, full) if a[1])
    assert all(a[0] == b[0] for a, b in zip(one, full) if not a[1])
    assert all(_doublets(y) == _doublets(c) for y, _ in one)
    assert all(cp for _, cp in (dbf.replicate(c, CAP_KEY, CAP_SEED, r, 0) for r in range(8)))


def test_the_brute_force_scores_codes():
    """replicates() scores the spelled codes with the order-1 brute force's scorers: W = 2, w[s] = s + 1"""
    sm = np.array([[1, 2], [3, 4], [5, 6], [7, 8]])
    w = np.arange(100, dtype=np.uint64) + 1
    got = dbf.null([b"ACGATCAGTACA", b"a", b""], [12345, 1, 2], 0, 4, 2, sm, 0, w, True, 0)
    ys = [b"AGTCACGATACA", b"ATCACGTAGACA", b"AGTCACACGATA", b"ACACAGATCGTA"]
    assert got["rep_sum"][0] == [bf.pair(y, 2, sm, 0, w, True)[1] for y in ys]
    assert len(set(got["rep_sum"][0])) == 1 and got["rep_sum"][0][0] == got["obs_sum"][0]      # W = 2: the doublets ARE the windows
    assert got["ge_sum"] == [4, 4, 4] and got["rep_best"][1] == [-1] * 4


# ------------------------------------------------------------------------------------------- the frames
def _table(**over):
    from grafimo_amd.shuffle_null import ShuffleNull
    a = dict(motif_id="M1", motif_alt_id="m1", width=3, scale=2, offset=-1.5, ptable=np.array([1.0, 0.5, 0.5, 0.2, 0.2, 0.01]),
             log2_offset=-40.0, threshold=0.5, region_names=["c:0-9"], group_names=["g"], seq_region=[0, 0], seq_version=[0, 1],
             seq_count=[5, 1], seq_group_counts=[[2], [0]], seq_is_reference=[False, True], seq_length=[9, 10], seq_weight=[1, 0],
             replicates=3, seed=4, obs_best=[4, 3], obs_sum=[1 << 60, 12], ge_best=[0, 3], ge_sum=[2, 1], rep_hits=[0, 1, 1], cut=3)
    a.update(over)
    return ShuffleNull(**a)


def test_null_order_is_one_more_last_column_under_order_2_only():
    from grafimo_amd.shuffle_null import ENRICHMENT_COLUMNS, enrichment_frame
    one, two = _table(), _table(order=2)
    assert (one.order, two.order, _table(order=1).order) == (1, 2, 1)
    f1, f2 = one.to_frame(), two.to_frame()
    assert "null_order" not in f1 and list(f2.columns) == list(f1.columns) + ["null_order"]
    assert f2["null_order"].tolist() == [2, 2] and f2["null_order"].dtype == np.int64
    assert f2.drop(columns="null_order").equals(f1) and _table(order=1).to_frame().equals(f1)
    e1, e2 = enrichment_frame([one, one]), enrichment_frame([two, two])
    assert list(e1.columns) == ENRICHMENT_COLUMNS and list(e2.columns) == ENRICHMENT_COLUMNS + ["null_order"]
    assert e2["null_order"].tolist() == [2, 2] and e2.drop(columns="null_order").equals(e1)
    with pytest.raises(ValueError, match="order 3"):
        _table(order=3)


# ------------------------------------------------------------------------------------------- the export, the header, the refusals
N_ARGS = 24


def test_library_exports_the_order_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    name = "gfm_sequence_shuffle_null_order"
    assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == N_ARGS
    assert len(nv.PROTOTYPES["gfm_sequence_shuffle_null"][1]) == N_ARGS - 2                 # the old entry keeps its signature
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    decl = header[header.index(f"int {name}("):]
    assert decl[:decl.index(";")].count(",") == N_ARGS - 1
    assert f"#define GFM_NULL_MAX_WALK_CAP {nv.GFM_NULL_MAX_WALK_CAP}" in header and nv.GFM_NULL_MAX_WALK_CAP == 1024
    # before a device is touched: the values are refused by name; what is in range goes on to the old entry's checks
    fn = nv.lib().gfm_sequence_shuffle_null_order

    def call(order, walk_cap, K=1, flags=0):
        return fn(None, 1, None, 1, 0, None, None, None, None, K, 0, order, walk_cap, None, flags, *([None] * 9))
    for order in (0, 3, -1):
        assert call(order, 64) == nv.GFM_ERR_INVALID and f"order {order} is neither 1 nor 2".encode() in nv.lib().gfm_last_error()
    for cap in (-1, 1025):
        assert call(2, cap) == nv.GFM_ERR_INVALID and f"walk_cap {cap} outside [0, 1024]".encode() in nv.lib().gfm_last_error()
    for order, cap in ((1, 64), (2, 0), (2, 1024)):
        assert call(order, cap) == nv.GFM_OK                                          # (no sequence: a no-op)
    assert call(2, 64, flags=2) == nv.GFM_ERR_INVALID and b"unknown flag" in nv.lib().gfm_last_error()
    assert call(2, 64, K=0) == nv.GFM_ERR_INVALID and b"gfm_sequence_shuffle_null_order: n_replicates 0" in nv.lib().gfm_last_error()


def test_the_rule_is_stated_in_three_places():
    from grafimo_amd import shuffle_null
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    squeeze = lambda s: " ".join(s.replace("*", " ").split())                   # noqa: E731
    texts = [squeeze(header), squeeze(shuffle_null.__doc__), squeeze(dbf.__doc__)]
    for line in ("draw(t, m) = ((mix(s0 + t G) >> 32) m) >> 32, with m < 2^31.",
                 "c[i] = base_code(x[i]): 0 .. 3 for A/C/G/T with case folded, 4 for anything else.",
                 "s0 = mix(mix(seed + k G) + r + 2^63).",
                 "cnt[a] = #{i < n - 1 : c[i] = a}; b[a] is the exclusive prefix sum over a = 0 .. 4.",
                 "for i = 0 .. n - 2 in order, c[i + 1] is appended to bucket c[i].",
                 "Wilson's algorithm, rooted at root = c[n - 1]. in_tree = {root}, a step counter t = 0, cap = walk_cap n.",
                 "else e = b[cur] + draw(n + t, cnt[cur]), t += 1, last[cur] = e, cur = E[e].",
                 "A capped replicate takes last[a] = b[a + 1] - 1 for every a: x's own last exits",
                 "if a != root, swap E[last[a]] with E[b[a + 1] - 1] and m -= 1;",
                 "for i = m - 1 down to 1: p = b[a] + i, j = draw(p, i + 1), swap E[p] and E[b[a] + j].",
                 "y[0] = c[0], ptr[a] = b[a]; for i = 1 .. n - 1: y[i] = E[ptr[y[i - 1]]], then ptr[y[i - 1]] += 1."):
        for text in texts:
            assert line in text, line


def test_python_refusals():
    from grafimo_amd.shuffle_null import MAX_WALK_CAP, _checked_order, null_sequences
    assert MAX_WALK_CAP == 1024 and _checked_order(2, 0) == (2, 0) and _checked_order(1) == (1, 64)
    x = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)
    for order in (0, 3, "2"):
        with pytest.raises(ValueError, match=f"order {order}: the shuffle null is of order 1"):
            null_sequences([], [0, 12], x, 10, order=order)
    for cap in (-1, 1025):
        with pytest.raises(ValueError, match=f"walk_cap {cap}: outside \\[0, 1024\\]"):
            null_sequences([], [0, 12], x, 10, order=2, walk_cap=cap)


def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(flags),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--null-order", "2")
    assert r.returncode != 0 and "--null-order goes with --shuffle-null" in r.stderr
    r = _cli(tmp_path, *graph, "--null-order", "1")
    assert r.returncode != 0 and "--null-order goes with --shuffle-null" in r.stderr
    r = _cli(tmp_path, *graph, "--shuffle-null", "--null-order", "3")
    assert r.returncode != 0 and "--null-order" in r.stderr and "invalid choice" in r.stderr
    r = _cli(tmp_path, "-s", str(tmp_path), "--shuffle-null", "--null-order", "2")
    assert r.returncode != 0 and "--shuffle-null needs the graph" in r.stderr


def test_parser_defaults():
    from grafimo_amd.__main__ import get_parser
    p = get_parser()
    assert p.parse_args(["-m", "x"]).null_order is None                          # (read as 1)
    assert p.parse_args(["-m", "x", "--shuffle-null", "--null-order", "2"]).null_order == 2
    assert p.parse_args(["-m", "x", "--shuffle-null", "9", "--null-order", "1"]).null_order == 1
