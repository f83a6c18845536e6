"""Haplotype class table without a GPU: region_sites against the brute force's second statement of the rule
(tests/haplotype_class_bruteforce.py), the invariant the rule stands for -- haplotypes that agree on the sites of a region
spell the same rows (tests/variant_bruteforce.py spell) --, the frame, the two writers against pandas, min_haplotypes, the
CLI's refusals and the library's exports."""
import io
import os
import subprocess
import sys
import types

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from graph_table_checks import random_bitset_index  # noqa: E402
from graph_tables_fuzz_core import make_regions  # noqa: E402
from haplotype_class_bruteforce import region_classes, sites_of_region  # noqa: E402
from variant_bruteforce import haplotype_classes, spell  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
REF = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)


def _graph(seed):
    rng = np.random.default_rng(51_000 + seed)
    H = [1, 2, 7, 63, 65, 130][seed % 6]
    idx = random_bitset_index(H, 52_000 + seed, length=int(rng.integers(120, 300)), n_sites=int(rng.integers(3, 30)))
    return rng, idx


def test_region_sites_equals_the_second_statement():
    from grafimo_amd.haplotype_classes import region_sites
    seen = 0
    for seed in range(40):
        rng, idx = _graph(seed)
        L = len(idx.ref)
        regions = make_regions(rng, idx) + [(5, 5), (L, L + 9), (-9, 0), (-3, 1), (L - 1, L + 4)]
        for S, E in regions:
            got = region_sites(idx, S, E)
            assert got.dtype == np.int64 and got.tolist() == sites_of_region(idx, S, E), (seed, S, E)
            seen += len(got)
            if min(E, L) <= max(S, 0):
                assert len(got) == 0
    assert seen > 300                                    # (the seeds have sites to compare)


def test_the_rule_by_hand():
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.haplotype_classes import region_sites
    # site 0: SNV at 2; site 1: deletion of bases 5 and 6 behind the anchor 4; site 2: insertion behind the anchor 7
    idx = GraphIndex("c", REF, np.array([2, 4, 7], np.int32), np.array([1, 1, 1], np.uint8),
                     np.array([[ord("A"), 0, 0], [0, 0, 0], [0, 0, 0]], np.uint8), np.zeros((3, 3, 1), np.uint64), 2,
                     del_len=np.array([0, 2, 0], np.int32), ins_len=np.array([0, 0, 2], np.int32), ins_off=np.array([0, 0, 0], np.int32),
                     ins_bases=np.frombuffer(b"GG", dtype=np.uint8))
    for (S, E), exp in {(0, 10): [0, 1, 2], (2, 3): [0], (3, 5): [], (3, 6): [1], (6, 7): [1], (7, 8): [2], (8, 10): [2],
                        (9, 10): [], (5, 5): [], (-4, 3): [0], (6, 40): [1, 2], (10, 12): []}.items():
        assert region_sites(idx, S, E).tolist() == exp, (S, E)


def _rows(idx, h, W, S, E):
    """the rows of haplotype h in the clipped region under the report's rule: (start, stop, k-mer)"""
    seq, coord, ins, _, _ = spell(idx, h)
    S, E = max(S, 0), min(E, len(idx.ref))
    out = set()
    for o in range(len(seq) - W + 1):
        start, stop = coord[o] + (1 if ins[o] else 0), coord[o + W - 1] + 1
        if S <= start < E and stop <= E:
            out.add((start, stop, bytes(seq[o:o + W])))
    return out


def test_members_of_a_class_spell_the_same_rows():
    compared = 0
    for seed in range(20):
        rng, idx = _graph(seed)
        reps, cls = haplotype_classes(idx)               # (the classes over the WHOLE graph: one spelling each)
        for S, E in make_regions(rng, idx):
            exp = region_classes(idx, S, E)
            for W in (1, 3, 8, 20):
                rows = {}
                for h in range(int(idx.n_haplotypes)):
                    g = int(cls[h])
                    if g not in rows:
                        rows[g] = _rows(idx, int(reps[g]), W, S, E)
                    first = int(exp["first"][exp["class_of"][h]])
                    assert rows[g] == rows[int(cls[first])], (seed, S, E, W, h, first)
                    compared += 1
    assert compared > 10_000


def _index5():
    """an SNV with two ALTs at base 2, a deletion of 2 bases behind base 4, an SNV at base 8; 5 haplotypes"""
    from grafimo_amd.extract_regions import GraphIndex
    bits = np.zeros((3, 3, 1), np.uint64)
    bits[0, 0, 0], bits[0, 1, 0] = 0b00010, 0b01100
    bits[1, 0, 0] = 0b10000
    bits[2, 0, 0] = 0b00111
    alt = np.array([[ord("A"), ord("T"), 0], [0, 0, 0], [ord("G"), 0, 0]], np.uint8)
    return GraphIndex("c", REF, np.array([2, 4, 8], np.int32), np.array([2, 1, 1], np.uint8), alt, bits, 5,
                      del_len=np.array([0, 2, 0], np.int32))


def _classes(idx, regions, groups=None):
    """a HaplotypeClasses made on the host from the brute force"""
    from grafimo_amd.haplotype_classes import HaplotypeClasses
    groups = groups or {}
    per = [region_classes(idx, S, E, groups=list(groups.values())) for S, E in regions]
    H = int(idx.n_haplotypes)
    n = np.array([len(p["count"]) for p in per])
    return HaplotypeClasses([f"c:{S}-{E}" for S, E in regions], [f"hap{k}" for k in range(H)], np.stack([p["class_of"] for p in per]),
                            n, np.concatenate([[0], np.cumsum(n)]), np.concatenate([p["count"] for p in per]),
                            np.concatenate([p["first"] for p in per]), list(groups),
                            np.concatenate([p["group_counts"] for p in per]), [idx], np.zeros(len(regions), np.int64), regions)


def _numbers(R, H):
    """stand-ins for a motif's HaplotypeScores and HaplotypeAffinity over R regions and H haplotypes"""
    cell = np.arange(R * H, dtype=np.float64).reshape(R, H)
    scores = types.SimpleNamespace(best_score=cell + 0.5, best_pvalue=1.0 / (1.0 + cell), start=(cell + 1).astype(np.int64),
                                   stop=(cell + 4).astype(np.int64), strand=np.where(cell % 2 == 0, "+", "-").astype(object))
    aff = types.SimpleNamespace(log2_affinity=cell * 0.25, reference_log2_affinity=np.arange(R, dtype=np.float64))
    return scores, aff


def test_frame_columns_order_and_values():
    from grafimo_amd.haplotype_classes import class_table
    idx = _index5()
    regions = [(0, 10), (7, 10), (3, 3)]
    hc = _classes(idx, regions, {"a": [0, 1, 2], "b": [4]})
    # (0, 10): states (0,0,1) (1,0,1) (2,0,1) (2,0,0) (0,1,0): five classes of one, by smallest member
    assert hc.n_classes.tolist() == [5, 2, 1] and hc.class_of[0].tolist() == [0, 1, 2, 3, 4]
    assert hc.class_of[1].tolist() == [0, 0, 0, 1, 1] and hc.class_of[2].tolist() == [0] * 5
    assert hc.is_reference.tolist() == [False] * 5 + [False, True] + [True]
    assert hc.alleles(0, 2) == [(0, 0, 2), (0, 2, 1)] and hc.alleles(1, 1) == [] and hc.alleles(0, 4) == [(0, 1, 1)]
    scores, aff = _numbers(3, 5)
    t = class_table("M1", "m1", hc, scores, aff)
    f = t.to_frame()
    assert list(f.columns) == ["motif_id", "motif_alt_id", "sequence_name", "class", "haplotypes", "frequency", "haplotypes_a",
                               "haplotypes_b", "representative", "is_reference", "alt_alleles", "best_score", "best_pvalue",
                               "start", "stop", "strand", "log2_affinity", "delta_log2_affinity"]
    assert len(f) == len(t) == 8 and f["motif_id"].tolist() == ["M1"] * 8 and f["motif_alt_id"].tolist() == ["m1"] * 8
    assert f["sequence_name"].tolist() == ["c:0-10"] * 5 + ["c:7-10"] * 2 + ["c:3-3"]
    assert f["class"].tolist() == [0, 1, 2, 3, 4, 0, 1, 0] and f["haplotypes"].tolist() == [1, 1, 1, 1, 1, 3, 2, 5]
    assert f["frequency"].tolist() == [0.2] * 5 + [0.6, 0.4, 1.0]
    assert f["haplotypes_a"].tolist() == [1, 1, 1, 0, 0, 3, 0, 3] and f["haplotypes_b"].tolist() == [0, 0, 0, 0, 1, 0, 1, 1]
    assert f["representative"].tolist() == ["hap0", "hap1", "hap2", "hap3", "hap4", "hap0", "hap3", "hap0"]
    assert f["alt_alleles"].tolist() == ["9:A>G", "3:G>A;9:A>G", "3:G>T;9:A>G", "3:G>T", "5:ACG>A", "9:A>G", "", ""]
    assert f["is_reference"].dtype == bool and f["class"].dtype == np.int64 and f["haplotypes"].dtype == np.int64
    # a class takes its representative's column: the cell (region, first)
    cells = [0, 1, 2, 3, 4, 5, 8, 10]
    assert f["best_score"].tolist() == [c + 0.5 for c in cells] and f["start"].tolist() == [c + 1 for c in cells]
    assert f["stop"].tolist() == [c + 4 for c in cells] and f["strand"].tolist() == ["+" if c % 2 == 0 else "-" for c in cells]
    assert f["log2_affinity"].tolist() == [c * 0.25 for c in cells]
    assert f["delta_log2_affinity"].tolist() == [c * 0.25 - r for c, r in zip(cells, [0] * 5 + [1] * 2 + [2])]


def test_min_haplotypes():
    from grafimo_amd.haplotype_classes import class_table, compute_haplotype_class_table_many
    hc = _classes(_index5(), [(0, 10), (7, 10), (3, 3)])
    scores, aff = _numbers(3, 5)
    for n, rows in ((1, 8), (2, 3), (3, 2), (5, 1), (6, 0)):
        f = class_table("M", "m", hc, scores, aff, min_haplotypes=n).to_frame()
        assert len(f) == rows and (f["haplotypes"] >= n).all(), n
    assert class_table("M", "m", hc, scores, aff, 2).to_frame()["class"].tolist() == [0, 1, 0]      # (the numbers stay)
    with pytest.raises(ValueError, match="min_haplotypes"):
        compute_haplotype_class_table_many([], None, None, False, None, min_haplotypes=0)


def test_writers_equal_pandas(tmp_path):
    from grafimo_amd.haplotype_classes import class_table, write_haplotype_class_members, write_haplotype_classes

    class _M:
        motif_id, motif_name = "M1", "m1"

    class _Out:
        outdir = str(tmp_path / "o")

    rng = np.random.default_rng(5)
    idx = random_bitset_index(130, 77, length=200, n_sites=20)
    regions = [(0, 200), (40, 90), (60, 60), (150, 260)]
    hc = _classes(idx, regions, {"x": list(range(0, 130, 3))})
    scores, aff = _numbers(len(regions), 130)
    scores.best_score = rng.normal(size=scores.best_score.shape) * 7
    aff.log2_affinity = rng.normal(size=scores.best_score.shape) * 3
    aff.log2_affinity[0, 0] = np.nan
    t = class_table("M1", "m1", hc, scores, aff)
    assert hc.n_classes.max() > 10                                   # (class ids of two digits in the wide file)
    path = write_haplotype_classes(t, _M(), 1, _Out())
    assert os.path.basename(path) == "grafimo_haplotype_classes.tsv"
    assert open(path, "rb").read() == t.to_frame().to_csv(sep="\t", index=False, lineterminator="\n").encode()
    assert os.path.basename(write_haplotype_classes(t, _M(), 2, _Out())) == "grafimo_haplotype_classes_M1.tsv"
    buf = io.StringIO()
    write_haplotype_classes(t, None, 1, None, out=buf)
    assert buf.getvalue() == t.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    wide = pd.concat([pd.DataFrame({"sequence_name": hc.region_names}), pd.DataFrame(hc.class_of, columns=hc.haplotype_names)], axis=1)
    path = write_haplotype_class_members(hc, _Out())
    assert os.path.basename(path) == "grafimo_haplotype_class_members.tsv" and os.path.dirname(path) == _Out.outdir
    assert open(path, "rb").read() == wide.to_csv(sep="\t", index=False, lineterminator="\n").encode()
    raw = io.BytesIO()
    write_haplotype_class_members(hc, None, out=raw)
    assert raw.getvalue() == wide.to_csv(sep="\t", index=False, lineterminator="\n").encode()


def _cli(tmp_path, *extra):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), *extra],
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, "-s", str(tmp_path), "--haplotype-classes")
    assert r.returncode != 0 and "--haplotype-classes needs the graph" in r.stderr
    r = _cli(tmp_path, *graph, "--class-min-haplotypes", "2")
    assert r.returncode != 0 and "--class-min-haplotypes goes with --haplotype-classes" in r.stderr
    r = _cli(tmp_path, *graph, "--haplotype-classes", "--class-min-haplotypes", "0")
    assert r.returncode != 0 and "--class-min-haplotypes 0 < 1" in r.stderr
    r = _cli(tmp_path, *graph, "--haplotype-groups", "panel.txt")
    assert r.returncode != 0 and "--haplotype-groups goes with" in r.stderr and "--haplotype-classes" in r.stderr
    r = _cli(tmp_path, *graph, "--affinity-temperature", "2")
    assert r.returncode != 0 and "--affinity-temperature goes with --haplotype-affinity" in r.stderr
    assert "--haplotype-classes" in r.stderr
    r = _cli(tmp_path, *graph, "--haplotype-classes", "--affinity-temperature", "0")
    assert r.returncode != 0 and "is not > 0" in r.stderr


def test_library_exports_both_entries_at_abi_12():
    from grafimo_amd import _native as nv
    from grafimo_amd.grafimo_errors import GrafimoError, HashCollisionError
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    for name, n_args in (("gfm_graph_haplotype_classes", 12), ("gfm_graph_haplotype_class_records", 10)):
        assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == n_args
        assert f"int {name}(" in header
    assert nv.lib().gfm_graph_haplotype_classes(None, 0, None, None, 0, 64, 0, None, None, None, 0, None) == nv.GFM_ERR_INVALID
    assert nv.lib().gfm_graph_haplotype_class_records(-1, 1, None, None, None, 0, None, None, None, None) == nv.GFM_ERR_INVALID
    assert nv.lib().gfm_graph_haplotype_class_records(1, 1, None, None, None, 0, None, None, None, None) == nv.GFM_ERR_INVALID
    assert issubclass(HashCollisionError, GrafimoError)
