"""Per-variant affinity table without a GPU: the brute force (tests/variant_affinity_bruteforce.py) on hand-made graphs with the
expected numbers written out, its memo mode, the library's export, the CLI's refusals and the frame made from synthetic sums."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict  # noqa: E402
from variant_affinity_bruteforce import expected_rows, variant_affinity_sums  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
REF = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
ONES = np.ones(3001, dtype=np.uint64)                  # every k-mer weighs 1: sum == rows
FLAT = np.zeros((4, 3), dtype=np.int64)               # W = 3, every score 0


def _snv_index():
    """one SNV at base 5 (C > G), haplotype 0 REF, haplotype 1 ALT"""
    from grafimo_amd.extract_regions import GraphIndex
    bits = np.zeros((1, 3, 1), np.uint64)
    bits[0, 0, 0] = 0b10
    return GraphIndex("c", REF, np.array([5], np.int32), np.array([1], np.uint8), np.array([[ord("G"), 0, 0]], np.uint8), bits, 2)


def _del_index():
    """a 2-base deletion behind the anchor base 4 (bases 5 and 6 go), haplotype 0 REF, haplotype 1 ALT"""
    from grafimo_amd.extract_regions import GraphIndex
    bits = np.zeros((1, 3, 1), np.uint64)
    bits[0, 0, 0] = 0b10
    return GraphIndex("c", REF, np.array([4], np.int32), np.array([1], np.uint8), np.zeros((1, 3), np.uint8), bits, 2,
                      del_len=np.array([2], np.int32))


def test_one_snv_by_hand():
    """W = 3, forward only: the windows at offsets 3, 4, 5 hold base 5 -- three occurrences on each haplotype"""
    idx = _snv_index()
    for regions in ([(0, 10)], [(0, 10), (2, 9), (-3, 20)], [(3, 6), (4, 7), (5, 8)]):
        sums, rows = variant_affinity_sums(idx, regions, 3, FLAT, 0, ONES, forward_only=True)
        assert rows == {0: 3, 1: 3} and sums == rows, regions
        assert expected_rows(idx, sums, rows) == [(0, 1, 3, 3, 3, 3)]
    # the region rule: stop <= E cuts the window at offset 5 (stop 8), start >= S the one at offset 3
    sums, rows = variant_affinity_sums(idx, [(4, 7)], 3, FLAT, 0, ONES, forward_only=True)
    assert rows == {0: 1, 1: 1}
    # both strands: twice the rows, twice the sum
    sums, rows = variant_affinity_sums(idx, [(0, 10)], 3, FLAT, 0, ONES)
    assert rows == {0: 6, 1: 6} and sums == rows
    # weights by score: the ALT base G scores 5 in every column, everything else 0 -> w[5 * (number of G)]
    sm = np.zeros((4, 3), dtype=np.int64)
    sm[2, :] = 5
    w = np.arange(3001, dtype=np.uint64) + 1
    sums, rows = variant_affinity_sums(idx, [(0, 10)], 3, sm, 0, w, forward_only=True)
    # REF haplotype: TAC, ACG, CGT -> 0, 1, 1 G;  ALT: TAG, AGG, GGT -> 1, 2, 2 G
    assert sums == {0: 1 + 6 + 6, 1: 6 + 11 + 11} and rows == {0: 3, 1: 3}


def test_two_base_deletion_by_hand():
    """W = 3, forward only.  REF footprint: the deleted bases 5 and 6 -- the windows at offsets 3 .. 6 of haplotype 0.  ALT
    footprint: the junction (base 4 and the base behind the span) -- haplotype 1 spells 0 1 2 3 4 7 8 9, the windows at
    offsets 3 and 4 hold both"""
    idx = _del_index()
    sums, rows = variant_affinity_sums(idx, [(0, 10)], 3, FLAT, 0, ONES, forward_only=True)
    assert rows == {0: 4, 1: 2} and sums == rows
    assert expected_rows(idx, sums, rows) == [(0, 1, 4, 2, 4, 2)]
    # (0, 8): the REF window 6 7 8 stops at 9 > 8 and leaves; the ALT windows 3 4 7 and 4 7 8 stop at 8 and 9
    sums, rows = variant_affinity_sums(idx, [(0, 8)], 3, FLAT, 0, ONES, forward_only=True)
    assert rows == {0: 3, 1: 1}


@pytest.mark.parametrize("seed,W,no_reverse", [(1, 5, False), (2, 9, True)])
def test_memo_equals_every_haplotype(tmp_path, seed, W, no_reverse):
    from grafimo_amd import synth
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.haplotype_affinity import default_weights
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=200, n_samples=6, seed=seed, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    motif = synth.motif_object(synth.synthetic_motif(W, np.random.default_rng(7700 + seed), np.array([0.3, 0.2, 0.2, 0.3])), f"S{W}")
    od = motif_as_oracle_dict(motif)
    w, _ = default_weights(motif)
    regions = [(0, 120), (90, 200), (30, 33), (-5, 400)]
    a = variant_affinity_sums(idx, regions, W, od["score_matrix"], od["min_val"], w, forward_only=no_reverse)
    b = variant_affinity_sums(idx, regions, W, od["score_matrix"], od["min_val"], w, forward_only=no_reverse, memo=True)
    assert a == b and len(a[1]) > 0
    # a slot's rows never pass what its carriers can hold; allele 0 and the ALTs of a site share no haplotype
    assert all(v > 0 for v in a[1].values()) and set(a[0]) == set(a[1])


def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    assert "gfm_graph_variant_affinity" in nv.PROTOTYPES and hasattr(nv.lib(), "gfm_graph_variant_affinity")
    assert len(nv.PROTOTYPES["gfm_graph_variant_affinity"][1]) == 13
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert "int gfm_graph_variant_affinity(" in header
    rc = nv.lib().gfm_graph_variant_affinity(None, None, 0, None, 0, None, None, 0, None, None, None, 0, None)
    assert rc == nv.GFM_ERR_INVALID


def _cli(tmp_path, *extra):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), *extra],
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--variant-affinity-delta", "0.5")
    assert r.returncode != 0 and "--variant-affinity-delta goes with --variant-affinity" in r.stderr
    r = _cli(tmp_path, *graph, "--variant-affinity", "--variant-affinity-delta", "-1")
    assert r.returncode != 0 and "is not >= 0" in r.stderr
    r = _cli(tmp_path, "-s", str(tmp_path), "--variant-affinity")
    assert r.returncode != 0 and "--variant-affinity needs the graph" in r.stderr and "carry no walks" in r.stderr
    r = _cli(tmp_path, *graph, "--affinity-temperature", "2")
    assert r.returncode != 0 and "--affinity-temperature goes with --haplotype-affinity or --variant-affinity" in r.stderr
    r = _cli(tmp_path, *graph, "--variant-affinity", "--affinity-temperature", "0")
    assert r.returncode != 0 and "is not > 0" in r.stderr


def _three_site_index():
    """an SNV with two ALTs at base 2, the deletion of _del_index, an SNV at base 8; 5 haplotypes"""
    from grafimo_amd.extract_regions import GraphIndex
    bits = np.zeros((3, 3, 1), np.uint64)
    bits[0, 0, 0], bits[0, 1, 0] = 0b00010, 0b01100       # site 0: REF 2 haplotypes, ALT 1 one, ALT 2 two
    bits[1, 0, 0] = 0b10000                               # site 1: REF 4, ALT 1
    bits[2, 0, 0] = 0b00111                               # site 2: REF 2, ALT 3
    alt = np.array([[ord("A"), ord("T"), 0], [0, 0, 0], [ord("G"), 0, 0]], np.uint8)
    return GraphIndex("c", REF, np.array([2, 4, 8], np.int32), np.array([2, 1, 1], np.uint8), alt, bits, 5,
                      del_len=np.array([0, 2, 0], np.int32))


def test_frame_columns_dtypes_and_nan_rules():
    from grafimo_amd.variant_affinity import COLUMNS, VariantAffinity
    idx = _three_site_index()
    sums = np.zeros((3, 4, 2), dtype=np.uint64)
    sums[0, 0] = (1 << 40, 6)          # site 0 REF: 2 carriers
    sums[0, 1] = (1 << 42, 3)          # ALT 1: one carrier
    sums[0, 2] = (0, 0)                # ALT 2: no occurrence -- the row stays (the REF side has some), its ALT side is NaN
    sums[0, 3] = (99, 9)               # not an allele of the site (n_alts == 2): never a row
    sums[1, 1] = (3, 2)                # site 1: only the ALT side
    #                                    site 2: nothing on either side -- no row
    va = VariantAffinity("M1", "m1", log2_offset=-40.0)
    va.append("chr", idx, sums)
    assert len(va) == 3 and va.site.tolist() == [0, 0, 1] and va.allele.tolist() == [1, 2, 1]
    for name in ("ref_sum", "alt_sum", "ref_rows", "alt_rows"):
        assert getattr(va, name).dtype == np.uint64
    assert va.ref_sum.tolist() == [1 << 40, 1 << 40, 0] and va.alt_sum.tolist() == [1 << 42, 0, 3]
    assert va.ref_rows.tolist() == [6, 6, 0] and va.alt_rows.tolist() == [3, 0, 2]
    f = va.to_frame()
    assert list(f.columns) == COLUMNS == [
        "motif_id", "motif_alt_id", "sequence_name", "position", "ref", "alt", "ref_haplotypes", "alt_haplotypes", "ref_rows",
        "alt_rows", "ref_log2_affinity", "alt_log2_affinity", "delta_log2_affinity"]
    assert f["motif_id"].tolist() == ["M1"] * 3 and f["motif_alt_id"].tolist() == ["m1"] * 3
    assert f["sequence_name"].tolist() == ["chr"] * 3
    assert f["position"].tolist() == [3, 3, 5] and f["ref"].tolist() == ["G", "G", "ACG"] and f["alt"].tolist() == ["A", "T", "A"]
    assert f["ref_haplotypes"].tolist() == [2, 2, 4] and f["alt_haplotypes"].tolist() == [1, 2, 1]
    assert f["ref_rows"].dtype == np.uint64 and f["alt_rows"].dtype == np.uint64
    assert f["ref_haplotypes"].dtype == np.int64 and f["position"].dtype == np.int64
    for c in ("ref_log2_affinity", "alt_log2_affinity", "delta_log2_affinity"):
        assert f[c].dtype == np.float64
    # log2(sum) - log2(carriers) + offset: 40 - 1 - 40, 42 - 0 - 40; NaN exactly where the sum is 0; delta NaN if either is
    assert f["ref_log2_affinity"].tolist()[:2] == [-1.0, -1.0] and np.isnan(f["ref_log2_affinity"][2])
    assert f["alt_log2_affinity"][0] == 2.0 and np.isnan(f["alt_log2_affinity"][1])
    assert f["alt_log2_affinity"][2] == np.log2(3.0) - 40.0
    assert f["delta_log2_affinity"][0] == 3.0 and f["delta_log2_affinity"].isna().tolist() == [False, True, True]
    assert (np.isnan(va.ref_log2_affinity) == (va.ref_sum == 0)).all() and (np.isnan(va.alt_log2_affinity) == (va.alt_sum == 0)).all()
    # min_abs_delta keeps the rows with a finite |delta| >= it
    for x, n in ((3.0, 1), (3.5, 0), (1e-9, 1)):
        vb = VariantAffinity("M1", "m1", log2_offset=-40.0)
        vb.append("chr", idx, sums, min_abs_delta=x)
        assert len(vb) == n and len(vb.to_frame()) == n
    # a second graph's rows follow the first's; an empty table has the columns
    va.append("chr2", idx, sums)
    assert len(va) == 6 and va.to_frame()["sequence_name"].tolist() == ["chr"] * 3 + ["chr2"] * 3
    assert list(VariantAffinity("M", "m").to_frame().columns) == COLUMNS
    with pytest.raises(ValueError):
        va.append("chr", idx, sums[:2])


def test_writer_names_the_file(tmp_path):
    import pandas as pd
    from grafimo_amd.variant_affinity import VariantAffinity, write_variant_affinity

    class _M:
        motif_id, motif_name = "M1", "m1"

    class _Out:
        outdir = str(tmp_path / "o")

    sums = np.zeros((3, 4, 2), dtype=np.uint64)
    sums[0, 0], sums[0, 1] = (5, 2), (7, 1)
    va = VariantAffinity("M1", "m1")
    va.append("c", _three_site_index(), sums)
    path = write_variant_affinity(va, _M(), 1, _Out())
    assert os.path.basename(path) == "grafimo_variant_affinity.tsv"
    pd.testing.assert_frame_equal(pd.read_csv(path, sep="\t"), va.to_frame(), check_dtype=False)
    assert os.path.basename(write_variant_affinity(va, _M(), 2, _Out())) == "grafimo_variant_affinity_M1.tsv"
