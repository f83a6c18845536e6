"""Per-haplotype affinity matrix without a GPU: the default weight table, the log2 affinity of the matrix, the frame and the TSV
writer, the sum brute force (tests/haplotype_affinity_bruteforce.py) against the hit brute force with a 0/1 table, the
library's export and the CLI's refusals."""
import io
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict  # noqa: E402
from haplotype_affinity_bruteforce import haplotype_affinity_sums  # noqa: E402
from haplotype_bruteforce import haplotype_matrix  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")


def _motif(W, seed):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(4100 + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


@pytest.mark.parametrize("W,seed", [(5, 1), (19, 2), (64, 3)])
def test_default_weights(W, seed):
    from grafimo_amd.haplotype_affinity import FRACTION_BITS, default_weights
    m = _motif(W, seed)
    sm = motif_as_oracle_dict(m)["score_matrix"]
    w, s_best = default_weights(m)
    assert w.dtype == np.uint64 and w.shape == (1000 * W + 1,) and FRACTION_BITS == 40
    assert s_best == int(sm.max(axis=0).sum()) and 0 < s_best <= 1000 * W
    assert (np.diff(w.astype(np.int64)) >= 0).all() and (w >= 1).all()
    assert int(w[s_best]) == 1 << 40 and (w[s_best:] == w[s_best]).all()
    # the definition, in exact arithmetic where it is exact: s_best - k * scale is k bits below the optimum
    for k in range(0, 41):
        if s_best - k * m.scale >= 0:
            assert int(w[s_best - k * m.scale]) == 1 << (40 - k)
    # T = 2 halves the exponent: w_2[s_best - 2 d] == w_1[s_best - d]
    w2, s2 = default_weights(m, temperature=2.0)
    assert s2 == s_best
    d = np.arange(0, s_best // 2 + 1)
    assert (w2[s_best - 2 * d] == w[s_best - d]).all()
    with pytest.raises(ValueError):
        default_weights(m, temperature=0.0)


def _ha(sums, offset=0.0, mid="M1", names=("a|1", "a|2", "b|1")):
    from grafimo_amd.haplotype_affinity import HaplotypeAffinity
    sums = np.asarray(sums, dtype=np.uint64)
    return HaplotypeAffinity(mid, mid.lower(), [f"c:{k}-{k + 9}" for k in range(len(sums))], list(names), sums, offset)


def test_log2_affinity_of_a_one_row_cell_and_nan():
    """a cell of ONE row (one strand) of score s holds w[s]: its log2 affinity is that row's log-odds / T.  w[s] is the
    real weight rounded to an integer, off by at most 1/2: for w[s] >= 2^30 that moves log2 by at most
    0.5 / (2^30 ln 2) < 7e-10; float64 rounding of the sums near 20 adds some 1e-14"""
    from grafimo_amd.haplotype_affinity import FRACTION_BITS, default_weights
    m = _motif(12, 5)
    W = 12
    for T in (1.0, 0.5, 2.0):
        w, s_best = default_weights(m, temperature=T)
        off = -FRACTION_BITS + (s_best / m.scale + W * m.offset) / T
        scores = [s for s in (s_best, s_best - 1, s_best - 137, s_best - 777) if w[s] >= 1 << 30]
        assert len(scores) >= 2
        cells = [[int(w[s]) for s in scores] + [0]]
        ha = _ha(cells, off, names=[f"h{k}" for k in range(len(scores))])
        exp = np.array([(s / m.scale + W * m.offset) / T for s in scores])
        assert np.abs(ha.log2_affinity[0] - exp).max() < 1e-9
        assert np.isnan(ha.reference_log2_affinity[0])
    sums = np.array([[0, 5, 1 << 63, 0], [7, 0, 0, 1]], dtype=np.uint64)
    ha = _ha(sums)
    full = np.concatenate([ha.log2_affinity, ha.reference_log2_affinity[:, None]], axis=1)
    assert (np.isnan(full) == (sums == 0)).all()
    assert full[0, 2] == 63.0 and full[1, 3] == 0.0 and full[0, 1] == np.log2(5.0)
    assert ha.sums.dtype == np.uint64 and (ha.sums == sums[:, :3]).all() and (ha.reference_sum == sums[:, 3]).all()


def test_to_frame_columns_and_names():
    ha = _ha([[1, 2, 0, 4], [0, 0, 0, 0]], 1.5)
    f = ha.to_frame()
    assert list(f.columns) == ["motif_id", "motif_alt_id", "sequence_name", "reference", "a|1", "a|2", "b|1"]
    assert f["motif_id"].tolist() == ["M1", "M1"] and f["motif_alt_id"].tolist() == ["m1", "m1"]
    assert f["sequence_name"].tolist() == ["c:0-9", "c:1-10"]
    assert f["reference"].tolist()[0] == 3.5 and np.isnan(f["reference"].tolist()[1])
    assert f["a|1"].tolist()[0] == 1.5 and f["a|2"].tolist()[0] == 2.5 and f.iloc[1, 3:].isna().all()
    with pytest.raises(ValueError):
        _ha([[1, 2, 3]])


class _M:
    def __init__(self, mid):
        self.motif_id, self.motif_name = mid, mid.lower()


class _Out:
    def __init__(self, d):
        self.outdir = d


def test_writer_equals_pandas_byte_for_byte(tmp_path):
    from grafimo_amd.haplotype_affinity import write_haplotype_affinity
    ha = _ha([[1, 3, 0, 1 << 40], [0, 0, 0, 0], [12345678901234567, 3, 3, 0]], -40 + 17.25)
    path = write_haplotype_affinity(ha, _M("M1"), 1, _Out(str(tmp_path / "o")))
    assert os.path.basename(path) == "grafimo_haplotype_affinity.tsv"
    text = open(path).read()
    assert text == ha.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    assert text.split("\n")[2] == "M1\tm1\tc:1-10\t\t\t\t"
    pd.testing.assert_frame_equal(pd.read_csv(path, sep="\t"), ha.to_frame(), check_dtype=False)
    buf = io.BytesIO()
    assert write_haplotype_affinity(ha, None, 1, None, out=buf) is None and buf.getvalue().decode() == text
    path = write_haplotype_affinity(_ha([[1, 2, 3, 4]], mid="M2"), _M("M2"), 3, _Out(str(tmp_path / "o")))
    assert os.path.basename(path) == "grafimo_haplotype_affinity_M2.tsv"
    # many rows and many distinct sums, empty cells anywhere, no cell empty, every cell empty; any cell_bytes
    rng = np.random.default_rng(0)
    R, H = 700, 90
    sums = rng.integers(0, 1 << 62, size=(R, H + 1), dtype=np.int64).astype(np.uint64)
    sums[rng.random((R, H + 1)) < 0.3] = 0
    for s in (sums, np.maximum(sums, 1), np.zeros_like(sums)):
        ha = _ha(s, -3.25, mid="X", names=[f"h{k}" for k in range(H)])
        exp = ha.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
        for cb in (None, 1, 1000, 1 << 16):
            buf = io.BytesIO()
            write_haplotype_affinity(ha, None, 1, None, out=buf, cell_bytes=cb)
            assert buf.getvalue().decode() == exp, cb


@pytest.mark.parametrize("seed,W,kinds,no_reverse", [(1, 6, "s", False), (2, 8, "i", True), (3, 5, "d", False),
                                                     (4, 7, "sidmDOc", False), (5, 9, "sidmDOc", True)])
def test_bruteforce_with_a_zero_one_table_counts_the_hits(tmp_path, seed, W, kinds, no_reverse):
    """two independent oracles: with w[s] = (s >= cutoff) the sums are the hit brute force's counts"""
    from grafimo_amd.extract_regions import GraphIndex
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=200, n_samples=4, seed=seed, kinds=kinds)
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    od = motif_as_oracle_dict(_motif(W, seed))
    regions = [(0, 120), (90, 200), (30, 33), (-5, 400)]
    H = int(idx.n_haplotypes)
    L = 1000 * W + 1
    for cutoff in (int(np.median(od["score_matrix"].max(axis=0))) * W // 2, 0):
        w = (np.arange(L) >= cutoff).astype(np.uint64)
        sums = haplotype_affinity_sums(idx, regions, W, od["score_matrix"], od["min_val"], w, forward_only=no_reverse)
        counts, _ = haplotype_matrix(idx, regions, W, od["score_matrix"], od["min_val"], cutoff, forward_only=no_reverse)
        assert sums.shape == (len(regions), H + 1) and sums.dtype == np.uint64
        assert (sums[:, :H] == counts.astype(np.uint64)).all()
        memo = haplotype_affinity_sums(idx, regions, W, od["score_matrix"], od["min_val"], w, forward_only=no_reverse, memo=True)
        assert (memo == sums).all()
    assert (sums[3, :H] > 0).all() and sums[3, H] > 0              # (cutoff 0: every row counts)


def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    assert "gfm_graph_haplotype_affinity" in nv.PROTOTYPES and hasattr(nv.lib(), "gfm_graph_haplotype_affinity")
    assert len(nv.PROTOTYPES["gfm_graph_haplotype_affinity"][1]) == 14
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert "int gfm_graph_haplotype_affinity(" in header and "rows_bound" in header
    rc = nv.lib().gfm_graph_haplotype_affinity(None, None, 0, None, 0, 0, None, None, 0, None, None, 0, 0, None)
    assert rc == nv.GFM_ERR_INVALID


def _cli(tmp_path, *extra):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), *extra],
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, "-s", str(tmp_path), "--haplotype-affinity")
    assert r.returncode != 0 and "--haplotype-affinity needs the graph" in r.stderr and "carry no walks" in r.stderr
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--affinity-temperature", "2")
    assert r.returncode != 0 and "--affinity-temperature goes with --haplotype-affinity" in r.stderr
    for t in ("0", "-1.5"):
        r = _cli(tmp_path, *graph, "--haplotype-affinity", "--affinity-temperature", t)
        assert r.returncode != 0 and "is not > 0" in r.stderr
