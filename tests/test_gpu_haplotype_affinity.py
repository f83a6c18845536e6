"""Per-haplotype affinity matrix on the GPU (gfm_graph_haplotype_affinity -> grafimo_amd.haplotype_affinity): the sums equal, AS
INTEGERS, the brute force of tests/haplotype_affinity_bruteforce.py; with a 0/1 table they are the hit matrix's counts; they do
not depend on the run / block decomposition; the refusals, the call variants, the two tutorial routes and the CLI.  No
tolerance on a sum: the device adds 64-bit integers."""
import contextlib
import ctypes
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

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")


class _Args:
    def __init__(self, threshold=1e-4, no_reverse=False, recomb=False, qvalue_t=False, no_qvalue=True):
        self.threshold, self.noreverse, self.recomb = threshold, no_reverse, recomb
        self.noqvalue, self.qvalueT = no_qvalue, qvalue_t


def _motif(W, seed=0):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(2900 + 13 * W + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


def _ctcf():
    from grafimo_amd.motif_ops import build_motif_meme_host
    return build_motif_meme_host(os.path.join(GOLD, "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]


def _expected(idx, regions, motif, weights, no_reverse, memo=False):
    od = motif_as_oracle_dict(motif)
    return haplotype_affinity_sums(idx, regions, od["width"], od["score_matrix"], od["min_val"], weights, forward_only=no_reverse,
                                   memo=memo)


def _check(ha, idx, regions, motif, no_reverse, temperature=1.0, weights=None, exp=None, memo=False):
    """every cell's sum against the brute force as integers, and what the matrix makes of the sums -> the expected sums"""
    from grafimo_amd.haplotype_affinity import FRACTION_BITS, default_weights
    off = 0.0
    if weights is None:
        weights, s_best = default_weights(motif, temperature)
        off = -FRACTION_BITS + (s_best / motif.scale + motif.width * motif.offset) / temperature
    if exp is None:
        exp = _expected(idx, regions, motif, weights, no_reverse, memo)
    H = int(idx.n_haplotypes)
    assert ha.sums.dtype == np.uint64 and ha.sums.shape == (len(regions), H) and ha.reference_sum.shape == (len(regions),)
    got = np.concatenate([ha.sums, ha.reference_sum[:, None]], axis=1)
    assert (got == exp).all(), np.argwhere(got != exp)[:5]
    full = np.concatenate([ha.log2_affinity, ha.reference_log2_affinity[:, None]], axis=1)
    assert (np.isnan(full) == (exp == 0)).all()
    some = exp > 0
    # (float64 log2 of the same integers made in another array: equal to an ulp or two of values below 100)
    assert np.allclose(full[some], np.log2(exp[some].astype(np.float64)) + off, rtol=0, atol=1e-12)
    return exp


@pytest.mark.parametrize("seed,W,no_reverse", [(1, 5, False), (2, 8, True), (3, 12, False), (4, 19, True), (5, 30, False),
                                               (6, 64, False)])
def test_bruteforce_parity(tmp_path, seed, W, no_reverse):
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=seed, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    p = idx.pos
    # overlapping, the whole chromosome, shorter than W, starting / ending on a site
    regions = [(0, int(p[len(p) // 3]) + 1), (int(p[len(p) // 3]) - 2, int(p[2 * len(p) // 3])), (int(p[-3]), 400), (0, 400),
               (3, 4), (int(p[len(p) // 2]), int(p[len(p) // 2]) + W + 3), (-10, 500)]
    motif = _motif(W, seed)
    g = DeviceGraph(idx)
    ha = compute_haplotype_affinity(motif, g, regions, False, _Args(no_reverse=no_reverse))
    exp = _check(ha, idx, regions, motif, no_reverse)
    assert (exp[3] > 0).all() and (exp[4] == 0).all()
    assert np.isnan(ha.log2_affinity[4]).all() and np.isnan(ha.reference_log2_affinity[4])
    assert ha.haplotype_names == [f"s{k}|{j}" for k in range(12) for j in (1, 2)]
    assert ha.region_names.tolist() == [f"c:{S}-{E}" for S, E in regions]
    if seed == 3:                                        # once at another temperature
        cold = compute_haplotype_affinity(motif, g, regions, False, _Args(no_reverse=no_reverse), temperature=0.5)
        assert (_check(cold, idx, regions, motif, no_reverse, temperature=0.5) != exp)[3].any()
    g.close()


@pytest.mark.parametrize("seed,W,no_reverse", [(11, 8, False), (12, 19, True)])
def test_zero_one_table_gives_the_hit_counts(tmp_path, seed, W, no_reverse):
    """an independent product route: w[s] = (s >= the integer cutoff of -t 1e-2) makes the sums compute_haplotype_hits' counts"""
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity
    from grafimo_amd.haplotype_hits import compute_haplotype_hits
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=500, n_samples=20, seed=seed, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = [(0, 250), (200, 500), (100, 101), (0, 500)]
    motif = _motif(W, seed)
    args = _Args(threshold=1e-2, no_reverse=no_reverse)
    dm = DeviceMotif.lease(motif)
    cutoff = dm.pvalue_cutoff(1e-2)
    dm.release()
    assert 0 < cutoff < 1000 * W
    w = (np.arange(1000 * W + 1) >= cutoff).astype(np.uint64)
    ha = compute_haplotype_affinity(motif, idx, regions, False, args, weights=w)
    hh = compute_haplotype_hits(motif, idx, regions, False, args)
    assert (ha.sums == hh.counts.astype(np.uint64)).all()
    assert hh.counts[3].sum() > 0
    assert np.allclose(ha.log2_affinity, np.where(hh.counts > 0, np.log2(np.maximum(hh.counts, 1)), np.nan), rtol=0, atol=1e-12,
                       equal_nan=True)


def test_decomposition_invariance(tmp_path):
    """runs of 1 and 3 windows, blocks of 64 haplotypes, H = 150: the sums bit for bit -- a run or a block added twice, or a
    reference column written by more than one block, shows here"""
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=600, n_samples=75, seed=31, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    assert idx.n_haplotypes == 150
    g = DeviceGraph(idx)
    regions = [(0, 300), (250, 600), (0, 600), (40, 45)]
    motif = _motif(8, 3)
    ref = compute_haplotype_affinity(motif, g, regions, False, _Args())
    exp = _check(ref, idx, regions, motif, False, memo=True)
    for wpr, hpb in ((1, 64), (3, 64), (3, 0), (0, 128), (1024, 192)):
        got = compute_haplotype_affinity(motif, g, regions, False, _Args(), windows_per_run=wpr, haplotypes_per_block=hpb)
        assert (got.full == ref.full).all() and (got.full == exp).all(), (wpr, hpb)
    g.close()


def _dense_window_graph(n_hap, seed=3):
    """one window of 19 bases over 18 biallelic sites (2^18 walks), haplotypes with random alleles"""
    from grafimo_amd.extract_regions import GraphIndex
    rng = np.random.default_rng(seed)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 400)]
    pos = np.arange(100, 118, dtype=np.int32)
    alt = np.zeros((len(pos), 3), np.uint8)
    alt[:, 0] = np.where(ref[pos] == ord("A"), ord("C"), ord("A"))
    hw = (n_hap + 63) // 64
    carry = rng.random((len(pos), n_hap)) < 0.4
    bits = np.zeros((len(pos), 3, hw), np.uint64)
    for h in range(n_hap):
        bits[:, 0, h >> 6] |= carry[:, h].astype(np.uint64) << np.uint64(h & 63)
    return GraphIndex("c", ref, pos, np.ones(len(pos), np.uint8), alt, bits, n_hap)


def test_dense_window():
    """a window of 2^18 walks over 203 haplotypes: thousands of rounds of 64 records per window"""
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity
    idx = _dense_window_graph(203)
    regions = [(90, 130), (0, 400)]
    motif = _ctcf()
    ha = compute_haplotype_affinity(motif, idx, regions, False, _Args())
    assert (_check(ha, idx, regions, motif, False, memo=True) > 0).all()


def test_walk_overflow_is_an_error():
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity
    ref = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    pos = np.arange(20, 33, dtype=np.int32)          # 13 sites of 3 ALTs in one window of 19: 4^13 walks
    alt = np.array([[c for c in b"ACGT" if c != ref[q]] for q in pos], dtype=np.uint8)
    idx = GraphIndex("c", ref, pos, np.full(13, 3, np.uint8), alt, np.ones((13, 3, 1), np.uint64), 2)
    # (only windows that see all 13 sites: a window of exactly 4^12 = 2^24 walks would be replayed)
    with pytest.raises(OverflowError):
        compute_haplotype_affinity(_motif(19), idx, [(14, 39)], False, _Args())


def test_sum_capacity_is_checked_before_anything_runs(tmp_path):
    """rows_bound = 2 * (region bases + all inserted bases): a table with max_weight * rows_bound > 2^64 - 1 is refused and
    nothing is launched; the largest table that fits is summed exactly"""
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex, _stream_ptr
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=300, n_samples=6, seed=41, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    assert int(idx.ins_len.sum()) > 0
    motif = _motif(8, 4)
    L = 1000 * 8 + 1
    regions = [(10, 200), (0, 300)]
    rows_bound = 2 * (300 + int(idx.ins_len.sum()))
    fits = ((1 << 64) - 1) // rows_bound
    g = DeviceGraph(idx)
    with pytest.raises(nv.NativeError) as e:
        compute_haplotype_affinity(motif, g, regions, False, _Args(), weights=np.full(L, fits + 1, dtype=np.uint64))
    assert e.value.code == nv.GFM_ERR_INVALID and "region 1" in str(e.value)
    w = np.full(L, fits, dtype=np.uint64)
    w[::3] = 0                                            # (zeros are allowed)
    ha = compute_haplotype_affinity(motif, g, regions, False, _Args(), weights=w)
    assert int(_check(ha, idx, regions, motif, False, weights=w).max()) > 1 << 62
    # the entry itself: refused with the caller's buffers untouched
    dm = DeviceMotif.lease(motif)
    vp = ctypes.c_void_p
    H = int(idx.n_haplotypes)
    sums = torch.zeros((2, H + 1), dtype=torch.int64, device=g.device)
    over = torch.zeros(1, dtype=torch.int32, device=g.device)
    tab = torch.from_numpy(np.full(L, 1 << 63, dtype=np.uint64).view(np.int64)).to(g.device)
    starts, stops = np.array([10, 0], dtype=np.int64), np.array([200, 300], dtype=np.int64)
    rc = nv.lib().gfm_graph_haplotype_affinity(g._h, (vp * 1)(dm.handle), 1, (vp * 1)(tab.data_ptr()), 1 << 63, 2, nv.ptr(starts),
                                               nv.ptr(stops), 0, (vp * 1)(sums.data_ptr()), over.data_ptr(), 0, 0, _stream_ptr(None))
    torch.cuda.synchronize()
    assert rc == nv.GFM_ERR_INVALID and int(sums.abs().sum().item()) == 0 and int(over.item()) == 0
    dm.release()
    g.close()


def test_flags_many_and_refusal(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity, compute_haplotype_affinity_many
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=500, n_samples=12, seed=29, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = [(0, 300), (200, 500)]
    m = _motif(8, 1)
    ref = compute_haplotype_affinity(m, idx, regions, False, _Args())
    _check(ref, idx, regions, m, False)
    for args in (_Args(recomb=True), _Args(threshold=1e-8), _Args(threshold=0.5, qvalue_t=True, no_qvalue=False)):
        assert (compute_haplotype_affinity(m, idx, regions, False, args).full == ref.full).all()
    for motifs in ([_motif(8, 1), _motif(8, 2), _motif(8, 3)], [_motif(8, 1), _motif(12, 2), _motif(8, 3), _motif(12, 4)]):
        many = compute_haplotype_affinity_many(motifs, idx, regions, False, _Args())
        for mo, t in zip(motifs, many):
            one = compute_haplotype_affinity(mo, idx, regions, False, _Args())
            assert t.motif_id == mo.motif_id and (t.full == one.full).all() and t.log2_offset == one.log2_offset
    # entries that share one graph: rows in the caller's entry order
    split = compute_haplotype_affinity(m, [idx, idx], [[regions[1]], [regions[0]]], False, _Args(), chrom_names=["c", "c"])
    assert (split.full == ref.full[::-1]).all() and split.region_names.tolist() == ref.region_names.tolist()[::-1]
    bare = GraphIndex("c", np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([10], np.int32), np.array([1], np.uint8),
                      np.array([[ord("A"), 0, 0]], np.uint8), None, 0)
    with pytest.raises(ValueError, match="carries no haplotypes"):
        compute_haplotype_affinity(m, bare, [(0, 100)], False, _Args())


@pytest.fixture()
def mygenome(tmp_path, monkeypatch):
    import shutil
    g = tmp_path / "data" / "mygenome"
    shutil.copytree(os.path.join(GOLD, "mygenome"), g)     # (scan_graph saves x.gfmidx.npz beside x.xg)
    monkeypatch.setenv("GRAFIMO_INDEX_CACHE", str(tmp_path / "cache"))
    monkeypatch.delenv("GRAFIMO_SCAN_OUTPUT", raising=False)
    return str(g)


def test_manifest_route_equals_fasta_vcf_route(tmp_path, mygenome, monkeypatch):
    import shutil
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex, read_bed_regions, read_manifest, scan_graph
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.workflow import Findmotif
    bed = os.path.join(tmp_path, "x.bed")
    with open(os.path.join(GOLD, "regions.bed")) as src, open(bed, "w") as dst:
        dst.writelines(line for line in src if line.startswith("chrx\t"))
    wf = Findmotif(graph_genome_dir=mygenome, bedfile=bed, cores=2, threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "example.meme"), wf, 2, True, pvalue_matrix=False)[0]
    monkeypatch.setenv("GRAFIMO_SCAN_OUTPUT", "manifest")
    with contextlib.redirect_stdout(io.StringIO()):
        loc = scan_graph({motif.width}, wf, True)
    try:
        man = read_manifest(loc)
        assert man is not None
        a = compute_haplotype_affinity(motif, man, None, False, _Args())
        idx = GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), "x")
        b = compute_haplotype_affinity(motif, DeviceGraph(idx), read_bed_regions(bed)["chrx"], False, _Args())
        assert a.haplotype_names == ["hap0", "hap1"] and b.haplotype_names == ["1|1", "1|2"]
        assert a.region_names.tolist() == b.region_names.tolist()
        assert (a.full == b.full).all() and (a.sums > 0).any()
    finally:
        shutil.rmtree(loc, ignore_errors=True)


def test_cli_writes_matrix_and_leaves_report_alone(tmp_path):
    base = [sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", os.path.join(GOLD, "xy.fa"),
            "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed"), "-t", "0.05"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run(base + ["-o", a], check=True, cwd=str(tmp_path), env=env, timeout=600)
    r = subprocess.run(base + ["-o", b, "--haplotype-affinity"], check=True, cwd=str(tmp_path), env=env, timeout=600,
                       capture_output=True, text=True)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fb == sorted(fa + ["grafimo_haplotype_affinity.tsv"])
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert "haplotype affinities written to" in r.stdout
    path = os.path.join(b, "grafimo_haplotype_affinity.tsv")
    t = pd.read_csv(path, sep="\t")
    assert list(t.columns) == ["motif_id", "motif_alt_id", "sequence_name", "reference", "1|1", "1|2"]
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity_many
    motif = _ctcf()
    bed = read_bed_regions(os.path.join(GOLD, "regions.bed"))
    graphs = [GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), c[3:]) for c in bed]
    ha = compute_haplotype_affinity_many([motif], graphs, [bed[c] for c in bed], False, _Args(threshold=0.05))[0]
    assert open(path).read() == ha.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    pd.testing.assert_frame_equal(t, ha.to_frame(), check_dtype=False)
    r = subprocess.run(base + ["-o", str(tmp_path / "c"), "-f", "--haplotype-affinity"], check=True, cwd=str(tmp_path), env=env,
                       timeout=600, capture_output=True, text=True)
    assert "motif_id\tmotif_alt_id\tsequence_name\treference\t1|1\t1|2\n" in r.stdout
    assert not os.path.exists(tmp_path / "c" / "grafimo_haplotype_affinity.tsv")
    r = subprocess.run(base + ["-o", str(tmp_path / "d"), "--affinity-temperature", "2"], cwd=str(tmp_path), env=env, timeout=600,
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--affinity-temperature goes with --haplotype-affinity" in r.stderr
