"""Per-haplotype hit matrix without a GPU: the haplotype brute force (tests/haplotype_bruteforce.py) against the CPU
oracle's report rows, the haplotype names of GraphIndex (VCF samples, save / load, shards, the hap<k> fallback), the TSV
writer, the argument checks of the entry point and the CLI's refusal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict, oracle_table, variants_from_index  # noqa: E402
from haplotype_bruteforce import haplotype_matrix, integer_cutoff  # noqa: E402


def _motif(W, seed):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(700 + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


@pytest.mark.parametrize("seed,W,no_reverse,threshold", [(1, 8, False, 1e-2), (2, 8, True, 1e-2), (3, 6, False, 1e-4),
                                                         (4, 6, True, 1e-4)])
def test_bruteforce_sums_equal_oracle_frequencies(tmp_path, seed, W, no_reverse, threshold):
    """sum_h counts[r, h] == sum of haplotype_frequency over the report's rows of region r (the oracle's report)"""
    from grafimo_amd.extract_regions import GraphIndex
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=300, n_samples=5, seed=seed, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    m = _motif(W, seed)
    od = motif_as_oracle_dict(m)
    ptab = np.cumsum(od["pmf"][::-1])[::-1]
    regions = [(0, 130), (110, 300), (40, 90)]
    counts, best = haplotype_matrix(idx, regions, W, od["score_matrix"], od["min_val"], integer_cutoff(ptab, threshold),
                                    forward_only=no_reverse)
    df, _ = oracle_table(str(tmp_path / "oracle"), "c", idx.ref.tobytes(), variants_from_index(idx), regions, m,
                         threshold=threshold, no_qvalue=True, no_reverse=no_reverse)
    freq = df.groupby("sequence_name")["haplotype_frequency"].sum()
    for r, (S, E) in enumerate(regions):
        assert counts[r].sum() == int(freq.get(f"c:{S}-{E}", 0)), (S, E)
        assert (best[r] >= 0).tolist() == (counts[r] > 0).tolist()
    if threshold == 1e-2:
        assert counts.sum() > 0


def test_sample_names_from_vcf_save_load_and_shards(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex, shard_index
    from grafimo_amd.haplotype_hits import haplotype_column_names
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=300, n_samples=3, seed=5, kinds="sid", gz=True)
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    assert idx.n_haplotypes == 6 and idx.sample_names == ["s0", "s1", "s2"]
    assert haplotype_column_names(idx) == ["s0|1", "s0|2", "s1|1", "s1|2", "s2|1", "s2|2"]
    for compressed in (False, True):
        back = GraphIndex.load(idx.save(str(tmp_path / f"i{int(compressed)}"), compressed=compressed))
        assert back.sample_names == idx.sample_names
    assert shard_index(idx, [0], [100]).sample_names == idx.sample_names
    # an index written without the member (vg's files, indexes of earlier versions) loads with no names
    idx.sample_names = None
    path = idx.save(str(tmp_path / "old"))
    import zipfile
    assert "sample_names.npy" not in zipfile.ZipFile(path).namelist()
    old = GraphIndex.load(path)
    assert old.sample_names is None
    assert haplotype_column_names(old) == [f"hap{k}" for k in range(6)]


def test_tutorial_vcf_sample_names():
    from grafimo_amd.extract_regions import GraphIndex
    gold = os.path.join(ROOT, "tests", "golden", "ref_data")
    idx = GraphIndex.from_fasta_vcf(os.path.join(gold, "xy.fa"), os.path.join(gold, "xy2.vcf.gz"), "x")
    assert idx.sample_names == ["1"] and idx.n_haplotypes == 2


class _M:
    def __init__(self, mid):
        self.motif_id, self.motif_name = mid, mid.lower()


class _Out:
    def __init__(self, d):
        self.outdir = d


def _hh(mid="M1"):
    from grafimo_amd.haplotype_hits import HaplotypeHits
    counts = np.array([[0, 3, 12, 0], [0, 0, 0, 0], [101, 7, 0, 9]], dtype=np.int32)
    best = np.where(counts > 0, np.array([[0, 4, 6, 0], [0, 0, 0, 0], [9, 2, 0, 5]]), -1).astype(np.int32)
    pt = np.linspace(1.0, 0.01, 10)
    return HaplotypeHits(mid, mid.lower(), ["c:0-10", "c:5-20", "d:0-9"], ["a|1", "a|2", "b|1", "b|2"], counts, best, 10, 0.5,
                         4, pt)


def test_tsv_layout_and_frame(tmp_path):
    from grafimo_amd.haplotype_hits import write_haplotype_hits
    hh = _hh()
    path = write_haplotype_hits(hh, _M("M1"), 1, _Out(str(tmp_path / "o")))
    assert os.path.basename(path) == "grafimo_haplotype_hits.tsv"
    lines = open(path).read().split("\n")
    assert lines[0] == "motif_id\tmotif_alt_id\tsequence_name\ta|1\ta|2\tb|1\tb|2"
    assert lines[1:] == ["M1\tm1\tc:0-10\t0\t3\t12\t0", "M1\tm1\tc:5-20\t0\t0\t0\t0", "M1\tm1\td:0-9\t101\t7\t0\t9", ""]
    t = pd.read_csv(path, sep="\t")
    f = hh.to_frame()
    assert list(f.columns) == list(t.columns)
    pd.testing.assert_frame_equal(t, f, check_dtype=False)
    # best as the report gives a score: scaled / scale + W * offset; p-value from the tail table; NaN where no row
    assert hh.best_score[0, 1] == 4 / 10 + 4 * 0.5 and np.isnan(hh.best_score[1]).all()
    assert hh.best_pvalue[2, 0] == hh.ptable[9] and np.isnan(hh.best_pvalue[0, 0])


def test_tsv_names_for_several_motifs_and_many_rows(tmp_path):
    from grafimo_amd.haplotype_hits import HaplotypeHits, write_haplotype_hits
    path = write_haplotype_hits(_hh("M2"), _M("M2"), 3, _Out(str(tmp_path / "o")))
    assert os.path.basename(path) == "grafimo_haplotype_hits_M2.tsv"
    # more rows than one chunk of the writer, counts of several digits
    rng = np.random.default_rng(0)
    R, H = 2500, 7
    counts = rng.integers(0, 1200, size=(R, H)).astype(np.int32)
    hh = HaplotypeHits("X", "x", [f"r{k}" for k in range(R)], [f"h{k}" for k in range(H)], counts, counts - 1, 1, 0.0, 4,
                       np.ones(1300))
    path = write_haplotype_hits(hh, _M("X"), 1, _Out(str(tmp_path / "p")))
    t = pd.read_csv(path, sep="\t")
    assert t["sequence_name"].tolist() == [f"r{k}" for k in range(R)]
    assert (t.iloc[:, 3:].to_numpy() == counts).all()


def test_entry_point_checks_arguments():
    from grafimo_amd import _native as nv
    rc = nv.lib().gfm_graph_haplotype_hits(None, None, None, 0, None, 0, None, None, 0, None)
    assert rc == nv.GFM_ERR_INVALID


def test_cli_refuses_haplotype_hits_with_sequences(tmp_path):
    r = subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"),
                        "-s", str(tmp_path), "--haplotype-hits"], capture_output=True, text=True, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert r.returncode != 0
    assert "--haplotype-hits needs the graph" in r.stderr and "carry no walks" in r.stderr
