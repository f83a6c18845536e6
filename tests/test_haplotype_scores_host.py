"""Per-haplotype best score matrix without a GPU: the score brute force (tests/haplotype_score_bruteforce.py) against the hit
brute force at a cutoff below every score, the key's encoding and tie order, the TSV writer, the entry point's argument
checks and the CLI's refusal."""
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
from haplotype_bruteforce import haplotype_matrix  # noqa: E402
from haplotype_score_bruteforce import haplotype_score_keys  # noqa: E402


def _motif(W, seed):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(1700 + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


@pytest.mark.parametrize("seed,W,kinds,no_reverse", [(1, 6, "s", False), (2, 8, "i", True), (3, 5, "d", False),
                                                     (4, 7, "m", False), (5, 6, "D", True), (6, 8, "O", False),
                                                     (7, 5, "c", False), (8, 9, "S", False), (9, 6, "sidmDOcS", False)])
def test_score_bruteforce_equals_hit_bruteforce_below_every_score(tmp_path, seed, W, kinds, no_reverse):
    """two independent oracles: the best key's score equals the best of the hit brute force with nothing cut"""
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.haplotype_scores import unpack_keys
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=200, n_samples=4, seed=seed, kinds=kinds)
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    od = motif_as_oracle_dict(_motif(W, seed))
    regions = [(0, 120), (90, 200), (30, 33), (-5, 400)]
    keys = haplotype_score_keys(idx, regions, W, od["score_matrix"], od["min_val"], forward_only=no_reverse)
    H = int(idx.n_haplotypes)
    assert keys.shape == (len(regions), H + 1)
    _, best = haplotype_matrix(idx, regions, W, od["score_matrix"], od["min_val"], cutoff=-(1 << 40), forward_only=no_reverse)
    got, _, _, _ = unpack_keys(keys[:, :H], np.zeros((len(regions), 1), dtype=np.int64))
    assert (got == best).all()
    assert (got[2] == -1).all() and (got[0] >= 0).all()


def test_key_round_trip_and_tie_order():
    from grafimo_amd.haplotype_scores import LEFT_MAX, SPAN_MAX, pack_key, unpack_keys
    rng = np.random.default_rng(3)
    n = 1000
    base = rng.integers(0, 1 << 30, n)
    left = base + rng.integers(0, LEFT_MAX, n)
    right = left + rng.integers(0, SPAN_MAX + 1, n)
    score = rng.integers(0, 1 << 16, n)
    plus = rng.integers(0, 2, n).astype(bool)
    k = pack_key(score, left, right, plus, base)
    assert (k != 0).all()
    b, lo, hi, pl = unpack_keys(k, base)
    assert (b == score).all() and (lo == left).all() and (hi == right).all() and (pl == plus).all()
    # the order: score, then the smaller left, then the smaller right, then '+' before '-'
    K = lambda s, lo_, hi_, p: int(pack_key(s, lo_, hi_, p, 100))   # noqa: E731
    assert K(7, 500, 520, 0) > K(6, 100, 119, 1)
    assert K(7, 100, 130, 0) > K(7, 101, 120, 1)
    assert K(7, 100, 119, 0) > K(7, 100, 120, 1)
    assert K(7, 100, 119, 1) > K(7, 100, 119, 0)
    assert K(0, 100 + LEFT_MAX - 1, 100 + LEFT_MAX - 1 + SPAN_MAX, 0) > 0
    # no row: -1, and no coordinates
    b, lo, hi, pl = unpack_keys(np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.int64))
    assert (b == -1).all() and (lo == -1).all() and (hi == -1).all() and not pl.any()


class _M:
    def __init__(self, mid):
        self.motif_id, self.motif_name = mid, mid.lower()


class _Out:
    def __init__(self, d):
        self.outdir = d


def _hs(mid="M1", names=("a|1", "a|2", "b|1", "b|2")):
    from grafimo_amd.haplotype_scores import HaplotypeScores, pack_key
    best = np.array([[-1, 3, 12, -1, 5], [-1, -1, -1, -1, -1], [9, 7, 0, 9, 9]], dtype=np.int64)   # last column: reference
    base = np.array([0, 5, 0], dtype=np.int64)
    left = base[:, None] + np.arange(5)[None, :]
    keys = np.where(best >= 0, pack_key(np.maximum(best, 0), left, left + 4, (np.arange(5) % 2)[None, :], base[:, None]), 0)
    pt = np.linspace(1.0, 0.01, 13)
    return HaplotypeScores(mid, mid.lower(), ["c:0-10", "c:5-20", "d:0-9"], list(names), keys.astype(np.uint64), base, 3, 0.25,
                           4, pt)


def test_matrix_fields():
    hs = _hs()
    assert hs.best.tolist() == [[-1, 3, 12, -1], [-1, -1, -1, -1], [9, 7, 0, 9]]
    assert hs.reference_best.tolist() == [5, -1, 9]
    assert hs.best_score[0, 1] == 3 / 3 + 4 * 0.25 and np.isnan(hs.best_score[1]).all() and np.isnan(hs.reference_score[1])
    assert hs.best_pvalue[2, 0] == hs.ptable[9] and np.isnan(hs.best_pvalue[0, 0]) and hs.reference_pvalue[0] == hs.ptable[5]
    # column k: left = base + k, right = left + 4, '+' on odd columns; '-' rows print start > stop
    assert hs.strand[0].tolist() == ["", "+", "-", ""] and hs.reference_strand.tolist() == ["-", "", "-"]
    assert hs.start[0, 1] == 1 and hs.stop[0, 1] == 5 and hs.start[0, 2] == 6 and hs.stop[0, 2] == 2
    assert hs.start[0, 0] == -1 and hs.reference_start[2] == 8 and hs.reference_stop[2] == 4


def test_tsv_layout_frame_and_stream(tmp_path):
    from grafimo_amd.haplotype_scores import write_haplotype_scores
    hs = _hs()
    path = write_haplotype_scores(hs, _M("M1"), 1, _Out(str(tmp_path / "o")))
    assert os.path.basename(path) == "grafimo_haplotype_scores.tsv"
    text = open(path).read()
    lines = text.split("\n")
    assert lines[0] == "motif_id\tmotif_alt_id\tsequence_name\treference\ta|1\ta|2\tb|1\tb|2"
    assert lines[1:] == ["M1\tm1\tc:0-10\t2.666666666666667\t\t2.0\t5.0\t", "M1\tm1\tc:5-20\t\t\t\t\t",
                         "M1\tm1\td:0-9\t4.0\t4.0\t3.3333333333333335\t1.0\t4.0", ""]
    # the same table written through pandas, as the report writes its float columns
    f = hs.to_frame()
    assert list(f.columns) == lines[0].split("\t")
    assert f.to_csv(sep="\t", index=False, lineterminator="\n") == text
    pd.testing.assert_frame_equal(pd.read_csv(path, sep="\t"), f, check_dtype=False)
    # -f: the same bytes to a stream
    buf = io.BytesIO()
    assert write_haplotype_scores(hs, None, 1, None, out=buf) is None
    assert buf.getvalue().decode() == text


def test_tsv_names_hap_columns_and_many_rows(tmp_path):
    from grafimo_amd.haplotype_scores import HaplotypeScores, pack_key, write_haplotype_scores
    path = write_haplotype_scores(_hs("M2", names=[f"hap{k}" for k in range(4)]), _M("M2"), 3, _Out(str(tmp_path / "o")))
    assert os.path.basename(path) == "grafimo_haplotype_scores_M2.tsv"
    assert open(path).readline() == "motif_id\tmotif_alt_id\tsequence_name\treference\thap0\thap1\thap2\thap3\n"
    # more rows than one chunk of the writer, many distinct scores, empty cells anywhere
    rng = np.random.default_rng(0)
    R, H = 3000, 300
    best = rng.integers(-1, 1500, size=(R, H + 1))
    keys = np.where(best >= 0, pack_key(np.maximum(best, 0), 10, 20, 1, 0), 0).astype(np.uint64)
    hs = HaplotypeScores("X", "x", [f"r{k}" for k in range(R)], [f"h{k}" for k in range(H)], keys, np.zeros(R, np.int64), 7,
                         -0.3, 12, np.ones(1500))
    path = write_haplotype_scores(hs, _M("X"), 1, _Out(str(tmp_path / "p")))
    assert open(path).read() == hs.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")


def test_entry_point_checks_arguments():
    from grafimo_amd import _native as nv
    rc = nv.lib().gfm_graph_haplotype_scores(None, None, 0, 0, None, None, 0, None, None, 0, 0, None)
    assert rc == nv.GFM_ERR_INVALID


def test_cli_refuses_haplotype_scores_with_sequences(tmp_path):
    r = subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"),
                        "-s", str(tmp_path), "--haplotype-scores"], capture_output=True, text=True, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert r.returncode != 0
    assert "--haplotype-scores needs the graph" in r.stderr and "carry no walks" in r.stderr
