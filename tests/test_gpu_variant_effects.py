"""Per-variant motif effects on the GPU (gfm_graph_variant_effects -> grafimo_amd.variant_effects) against the haplotype
brute force of tests/variant_bruteforce.py, the report's own rows, and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict  # noqa: E402
from graph_table_checks import check_variant_effects as _check  # noqa: E402
from variant_bruteforce import best_hits  # noqa: E402
from variant_walks import best_hits_walks  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")


class _Args:
    def __init__(self, threshold=1e-4, no_reverse=False, recomb=False):
        self.threshold, self.noreverse, self.recomb = threshold, no_reverse, recomb
        self.noqvalue, self.qvalueT = True, False


def _motif(W, seed=0):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(500 + 11 * W + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


@pytest.mark.parametrize("seed,W,no_reverse,all_sites", [
    (1, 5, False, True), (2, 8, True, False), (3, 19, False, False), (4, 19, True, True), (5, 30, False, True),
    (6, 64, False, False)])
def test_bruteforce_parity(tmp_path, seed, W, no_reverse, all_sites):
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.variant_effects import compute_variant_effects
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=500, n_samples=12, seed=seed, kinds="sidmDO")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    # regions that cut sites at their edges: bounds on site positions and just beside them
    p = idx.pos
    regions = [(0, int(p[len(p) // 3]) + 1), (int(p[len(p) // 3]) - 2, int(p[2 * len(p) // 3])), (int(p[-3]), 500)]
    args = _Args(threshold=0.05 if not all_sites else 1e-4, no_reverse=no_reverse)
    df = compute_variant_effects(_motif(W, seed), idx, regions, False, args, all_sites=all_sites)
    assert len(df) > 0
    _check(df, idx, regions, _motif(W, seed), args, all_sites, name="c")


@pytest.mark.parametrize("seed,W,kinds,no_reverse", [(31, 8, "sid", False), (32, 19, "sid", True), (33, 12, "sidD", False)])
def test_recomb_parity_with_walk_enumerator(tmp_path, seed, W, kinds, no_reverse):
    """--recomb: every walk counts, also those no haplotype carries -- the reference is the walk enumerator of
    tests/variant_walks.py (the brute force cannot see recombinant walks)"""
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.variant_effects import compute_variant_effects
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=seed, kinds=kinds)
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = [(0, 150), (140, 400)]
    motif = _motif(W, seed)
    od = motif_as_oracle_dict(motif)
    args = _Args(threshold=1e-4, no_reverse=no_reverse, recomb=True)
    best = best_hits_walks(idx, regions, W, od["score_matrix"], od["min_val"], forward_only=no_reverse)
    assert best != best_hits(idx, regions, W, od["score_matrix"], od["min_val"], forward_only=no_reverse)
    df = compute_variant_effects(motif, idx, regions, False, args, all_sites=True)
    _check(df, idx, regions, motif, args, True, best=best)


def test_agrees_with_report_rows(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex, compute_results_from_graph
    from grafimo_amd.variant_effects import compute_variant_effects
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=11, kinds="sid")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = [(0, 400)]
    m = _motif(8, 3)
    eff = compute_variant_effects(m, idx, regions, False, _Args(threshold=1.0), all_sites=True)
    rep = compute_results_from_graph(m, idx, regions, False, _Args(threshold=1.0))
    have = set(zip(rep["score"], rep["strand"], rep["start"], rep["stop"], rep["matched_sequence"]))
    n = 0
    for side in ("ref", "alt"):
        for r in eff[eff[side + "_sequence"] != ""].itertuples(index=False):
            key = (getattr(r, side + "_score"), getattr(r, side + "_strand"), int(getattr(r, side + "_start")),
                   int(getattr(r, side + "_stop")), getattr(r, side + "_sequence"))
            assert key in have, key
            n += 1
    assert n > 0


def test_tutorial_graphs(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.motif_ops import build_motif_meme_host
    from grafimo_amd.variant_effects import compute_variant_effects
    motif = build_motif_meme_host(os.path.join(GOLD, "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]
    from grafimo_amd.extract_regions import read_bed_regions
    bed = read_bed_regions(os.path.join(GOLD, "regions.bed"))
    for fa, vcf, chrom, regions in (("xy.fa", "xy2.vcf.gz", "x", bed["chrx"]), ("xy.fa", "xy2.vcf.gz", "y", bed["chry"]),
                                    ("xy.fa", "xy2.vcf.gz", "x", [(0, 400)]), ("test.fa", "test.vcf.gz", "x", bed["chrx"]),
                                    ("test.fa", "test.vcf.gz", "x", [(0, 60)])):
        idx = GraphIndex.from_fasta_vcf(os.path.join(GOLD, fa), os.path.join(GOLD, vcf), chrom)
        args = _Args(threshold=1e-2)
        df = compute_variant_effects(motif, idx, regions, False, args, all_sites=True)
        _check(df, idx, regions, motif, args, True)


def test_many_equals_single(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.variant_effects import compute_variant_effects, compute_variant_effects_many
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=21, kinds="sidD")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    motifs = [_motif(8, 1), _motif(12, 2), _motif(8, 3)]
    args = _Args(threshold=0.05)
    many = compute_variant_effects_many(motifs, idx, [(0, 400)], False, args)
    for m, t in zip(motifs, many):
        one = compute_variant_effects(m, idx, [(0, 400)], False, args)
        assert t.equals(one)


def test_overflow_is_an_error():
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.variant_effects import compute_variant_effects
    ref = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    pos = np.arange(20, 33, dtype=np.int32)          # 13 sites of 3 ALTs in one window of 19: 4^13 walks
    alt = np.array([[c for c in b"ACGT" if c != ref[q]] for q in pos], dtype=np.uint8)
    idx = GraphIndex("c", ref, pos, np.full(13, 3, np.uint8), alt, np.ones((13, 3, 1), np.uint64), 2)
    with pytest.raises(OverflowError):
        compute_variant_effects(_motif(19), idx, [(0, 100)], False, _Args(threshold=1.0, recomb=True))


def test_cli_writes_table_and_leaves_report_alone(tmp_path):
    base = [sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", os.path.join(GOLD, "xy.fa"),
            "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed"), "-t", "1"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run(base + ["-o", a], check=True, cwd=str(tmp_path), env=env, timeout=600)
    subprocess.run(base + ["-o", b, "--variant-effects"], check=True, cwd=str(tmp_path), env=env, timeout=600)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fb == sorted(fa + ["grafimo_variant_effects.tsv"])
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    head = open(os.path.join(b, "grafimo_variant_effects.tsv")).readline().rstrip("\n").split("\t")
    assert head[:6] == ["motif_id", "motif_alt_id", "sequence_name", "position", "ref", "alt"] and head[-1] == "effect"


@pytest.fixture()
def mygenome(tmp_path, monkeypatch):
    import shutil
    g = tmp_path / "data" / "mygenome"
    shutil.copytree(os.path.join(GOLD, "mygenome"), g)     # (scan_graph saves x.gfmidx.npz beside x.xg)
    monkeypatch.setenv("GRAFIMO_INDEX_CACHE", str(tmp_path / "cache"))
    monkeypatch.delenv("GRAFIMO_SCAN_OUTPUT", raising=False)
    return str(g)


def test_mygenome_through_the_manifest(tmp_path, mygenome, monkeypatch):
    """vg's own x.xg / x.gbwt / y.xg / y.gbwt of the tutorial: scan_graph's manifest is a `graph` form of its own"""
    import contextlib
    import io
    import shutil
    from grafimo_amd.extract_regions import cached_host_index, read_manifest, scan_graph
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.variant_effects import compute_variant_effects
    from grafimo_amd.workflow import Findmotif
    wf = Findmotif(graph_genome_dir=mygenome, bedfile=os.path.join(GOLD, "regions.bed"), cores=2, threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "example.meme"), wf, 2, True, pvalue_matrix=False)[0]
    monkeypatch.setenv("GRAFIMO_SCAN_OUTPUT", "manifest")     # (this caller holds no compute_results to be recognised by)
    with contextlib.redirect_stdout(io.StringIO()):
        loc = scan_graph({motif.width}, wf, True)
    try:
        man = read_manifest(loc)
        assert man is not None
        args = _Args(threshold=0.05)
        df = compute_variant_effects(motif, man, None, False, args, all_sites=True)
        names = [e["chrom"] for e in man["entries"]]
        assert len(names) == 2 and list(dict.fromkeys(df["sequence_name"])) == names     # entry order
        for e in man["entries"]:
            part = df[df["sequence_name"] == e["chrom"]].reset_index(drop=True)
            regs = [tuple(int(v) for v in r) for r in e["regions"]]
            _check(part, cached_host_index(e["index"]), regs, motif, args, True)
    finally:
        shutil.rmtree(loc, ignore_errors=True)


def test_cli_on_vgs_files(tmp_path, mygenome):
    """`-d mygenome/ -b regions.bed --variant-effects`: the table beside the report, the report unchanged"""
    base = [sys.executable, "-m", "grafimo_amd", "-d", mygenome + "/", "-m", os.path.join(GOLD, "example.meme"),
            "-b", os.path.join(GOLD, "regions.bed"), "-t", "0.05", "-j", "2"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run(base + ["-o", a], check=True, cwd=str(tmp_path), env=env, timeout=600)
    r = subprocess.run(base + ["-o", b, "--variant-effects"], check=True, cwd=str(tmp_path), env=env, timeout=600,
                       capture_output=True, text=True)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fb == sorted(fa + ["grafimo_variant_effects.tsv"])
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    import pandas as pd
    t = pd.read_csv(os.path.join(b, "grafimo_variant_effects.tsv"), sep="\t")
    assert len(t) > 0 and set(t["sequence_name"]) <= {"x", "y"} and "variant effect rows written" in r.stdout
