"""Per-hit allele table on the GPU (gfm_graph_hit_alleles + gfm_graph_hit_order -> grafimo_amd.hit_alleles) against the
report itself, the haplotype brute force, the walk enumerator and first principles (tests/hit_allele_bruteforce.py), the
merged per-haplotype hit matrix, the two tutorial routes and the CLI.  Every comparison is exact."""
import contextlib
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

from extract_helpers import make_consistent_graph_files  # noqa: E402
from graph_table_checks import random_bitset_index  # noqa: E402
from hit_allele_bruteforce import check_first_principles, check_table, unpack  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")


class _Args:
    def __init__(self, threshold=1e-4, no_reverse=False, recomb=False, qvalue_t=False, no_qvalue=True):
        self.threshold, self.noreverse, self.recomb = threshold, no_reverse, recomb
        self.noqvalue, self.qvalueT = no_qvalue, qvalue_t


def _motif(W, seed=0):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(900 + 13 * W + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _groups(H, rng):
    """disjoint, overlapping and empty groups, and one of all haplotypes"""
    perm = rng.permutation(H)
    return {"A": sorted(perm[:H // 3].tolist()), "B": sorted(perm[H // 3:2 * H // 3].tolist()),
            "AB2": sorted(perm[H // 4:H // 2 + 1].tolist()), "none": [], "all": list(range(H))}


FLAGS = {"default": dict(), "no_reverse": dict(no_reverse=True), "recomb": dict(recomb=True),
         "qvalueT": dict(threshold=0.9, qvalue_t=True, no_qvalue=False), "no_qvalue": dict(no_qvalue=True),
         "qvalues": dict(no_qvalue=False), "threshold_1": dict(threshold=1.0)}


# ---- 1. `report` is the report

@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_report_is_the_report(tmp_path, flags):
    from grafimo_amd.extract_regions import GraphIndex, compute_results_from_graph
    from grafimo_amd.hit_alleles import compute_hit_alleles
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=600, n_samples=10, seed=17, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = [(0, 250), (200, 600), (100, 101), (300, 450)]
    motif = _motif(8, 5)
    args = _Args(**{**dict(threshold=1e-2), **FLAGS[flags]})
    ha = _quiet(compute_hit_alleles, motif, idx, regions, False, args, carriers=True)
    rep = _quiet(compute_results_from_graph, motif, idx, regions, False, args)
    assert len(rep) > 5
    pd.testing.assert_frame_equal(ha.report, rep)
    assert ("q-value" in rep.columns) == (not args.noqvalue)
    check_first_principles(ha, idx)
    if flags == "recomb":
        assert (rep["haplotype_frequency"] == 0).any()


def test_the_alignment_survives_the_capacity_retry():
    """a FRESH DeviceGraph and more than 2^14 reported rows: the pass starts with a hit list of 2^14 entries, fetch() takes
    the list again at the size the counters ask for, and the rows must still be the entries'"""
    from grafimo_amd.extract_regions import DeviceGraph, compute_results_from_graph
    from grafimo_amd.hit_alleles import compute_hit_alleles
    idx = random_bitset_index(130, 77, length=9000, n_sites=300)
    g = DeviceGraph(idx)
    try:
        assert getattr(g, "_fused_cap", 0) == 0
        motif = _motif(8, 3)
        args = _Args(threshold=1.0, recomb=True)
        groups = _groups(130, np.random.default_rng(5))
        ha = _quiet(compute_hit_alleles, motif, g, [(0, 9000)], False, args, carriers=True, haplotype_groups=groups)
        assert len(ha) > (1 << 14) and g.fused_buffers(0, 0)[1] > (1 << 14)
        rep = _quiet(compute_results_from_graph, motif, g, [(0, 9000)], False, args)
        pd.testing.assert_frame_equal(ha.report, rep)
        check_first_principles(ha, idx, groups)
        assert np.array_equal(ha.group_counts[:, 4], rep["haplotype_frequency"].to_numpy())
    finally:
        g.close()


# ---- 2, 3, 4. the haplotype brute force, the walk enumerator, first principles

@pytest.mark.parametrize("seed,W,H,indels,no_reverse,recomb,threshold", [
    (1, 4, 6, True, False, False, 0.05), (2, 7, 130, True, False, True, 0.05), (3, 11, 5, True, True, False, 0.2),
    (4, 8, 65, True, False, True, 1.0), (5, 6, 64, False, False, False, 0.05), (6, 19, 130, True, False, False, 0.2)])
def test_bruteforce_parity_on_random_bitsets(seed, W, H, indels, no_reverse, recomb, threshold):
    from grafimo_amd.hit_alleles import compute_hit_alleles
    idx = random_bitset_index(H, 500 + seed, length=160, n_sites=24, indels=indels)
    regions = [(0, 160), (30, 95), (-5, 40), (100, 400), (50, 50)]
    motif = _motif(W, seed)
    args = _Args(threshold=threshold, no_reverse=no_reverse, recomb=recomb)
    groups = _groups(H, np.random.default_rng(seed))
    ha = _quiet(compute_hit_alleles, motif, idx, regions, False, args, carriers=True, haplotype_groups=groups)
    rows, keys = check_table(ha, idx, regions, motif, args, groups)
    assert rows > 5 and keys > 0
    assert np.array_equal(ha.group_counts[:, list(groups).index("all")], ha.report["haplotype_frequency"].to_numpy())
    assert not ha.group_counts[:, list(groups).index("none")].any()
    assert (ha.allele_entry == 0).all()
    # names: the carriers of a row by name
    r = int(np.argmax(ha.report["haplotype_frequency"].to_numpy()))
    car = unpack(ha.carrier_bits, H)
    assert ha.carriers(r) == [f"hap{h}" for h in np.flatnonzero(car[r])]


@pytest.mark.parametrize("seed,W,kinds,no_reverse,recomb,threshold,qvalue_t", [
    (1, 5, "sidmDOc", False, False, 1e-2, False), (2, 8, "sidmDOc", True, True, 1e-2, False),
    (3, 19, "sidmDOc", False, False, 0.05, False), (4, 12, "sid", False, True, 0.9, True), (7, 12, "sidD", False, False, 1e-2, False)])
def test_bruteforce_parity_on_vcf_graphs(tmp_path, seed, W, kinds, no_reverse, recomb, threshold, qvalue_t):
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.hit_alleles import compute_hit_alleles
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=260, n_samples=6, seed=seed, kinds=kinds)
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    p = idx.pos
    regions = [(0, int(p[len(p) // 3]) + 1), (int(p[len(p) // 3]) - 2, int(p[2 * len(p) // 3])), (int(p[-3]), 260), (0, 260), (3, 4)]
    motif = _motif(W, seed)
    args = _Args(threshold=threshold, no_reverse=no_reverse, recomb=recomb, qvalue_t=qvalue_t, no_qvalue=not qvalue_t)
    groups = {"first": ["s0|1", "s0|2", "s1|1"], "second": [3, 4, 5, 6], "odd": [f"s{k}|2" for k in range(6)]}
    ha = _quiet(compute_hit_alleles, motif, idx, regions, False, args, carriers=True, haplotype_groups=groups)
    as_columns = {"first": [0, 1, 2], "second": [3, 4, 5, 6], "odd": list(range(1, 12, 2))}
    rows, _ = check_table(ha, idx, regions, motif, args, as_columns)
    assert rows > 0 or qvalue_t
    assert ha.haplotype_names == [f"s{k}|{j}" for k in range(6) for j in (1, 2)]


def test_alt_bases_written_into_the_reference_give_the_matched_sequence():
    """a substitution-only graph: the row's ALT bases in the reference window are matched_sequence"""
    from grafimo_amd.hit_alleles import compute_hit_alleles
    from variant_bruteforce import revcomp
    idx = random_bitset_index(37, 91, length=300, n_sites=40, indels=False)
    motif = _motif(10, 2)
    ha = _quiet(compute_hit_alleles, motif, idx, [(0, 300)], False, _Args(threshold=0.05, recomb=True), carriers=True)
    ref = np.asarray(idx.ref, dtype=np.uint8)
    rep = ha.report
    n_alt = 0
    for r in range(len(ha)):
        a, b = sorted((int(rep["start"].iat[r]), int(rep["stop"].iat[r])))
        win = ref[a:b].copy()
        for _, s, al in ha.alleles(r):
            assert a <= int(idx.pos[s]) < b
            if al:
                win[int(idx.pos[s]) - a] = idx.alt_bases[s, al - 1]
                n_alt += 1
        seq = bytes(win)
        assert (seq if rep["strand"].iat[r] == "+" else revcomp(seq)).decode() == rep["matched_sequence"].iat[r]
        sites_in = [s for s in range(len(idx.pos)) if a <= int(idx.pos[s]) < b]
        assert [s for _, s, _ in ha.alleles(r)] == sites_in              # every site of the window constrains the walk
    assert n_alt > 10
    check_first_principles(ha, idx)


# ---- 5. the merged per-haplotype hit matrix

@pytest.mark.parametrize("qvalue_t", [False, True])
def test_carriers_sum_to_the_haplotype_hit_matrix(tmp_path, qvalue_t):
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.haplotype_hits import compute_haplotype_hits
    from grafimo_amd.hit_alleles import compute_hit_alleles
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=600, n_samples=35, seed=17, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = [(0, 250), (200, 600), (100, 101), (300, 450)]
    motif = _motif(8, 5)
    args = _Args(threshold=0.9 if qvalue_t else 1e-2, qvalue_t=qvalue_t, no_qvalue=not qvalue_t)
    ha = _quiet(compute_hit_alleles, motif, idx, regions, False, args, carriers=True)
    hh = _quiet(compute_haplotype_hits, motif, idx, regions, False, args)
    car = unpack(ha.carrier_bits, 70).astype(np.int64)
    assert hh.counts.sum() > 0
    for r, name in enumerate(hh.region_names.tolist()):
        rows = np.flatnonzero(ha.report["sequence_name"].to_numpy() == name)
        assert np.array_equal(car[rows].sum(axis=0), hh.counts[r]), name


# ---- 6. plumbing

def _same(a, b):
    pd.testing.assert_frame_equal(a.report, b.report)
    for k in ("allele_offsets", "allele_entry", "allele_site", "allele", "group_counts"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert (a.carrier_bits is None) == (b.carrier_bits is None)
    if a.carrier_bits is not None:
        assert np.array_equal(a.carrier_bits, b.carrier_bits)
    assert a.group_names == b.group_names


def test_tiny_scratch_and_a_second_call_for_room_equal_the_default(monkeypatch):
    from grafimo_amd import hit_alleles as hal
    idx = random_bitset_index(130, 23, length=400, n_sites=60)
    regions = [(0, 200), (150, 400), (0, 400)]
    motif = _motif(8, 2)
    args = _Args(threshold=0.05, recomb=True)
    groups = _groups(130, np.random.default_rng(1))
    ref = _quiet(hal.compute_hit_alleles, motif, idx, regions, False, args, carriers=True, haplotype_groups=groups)
    assert len(ref) > 100 and len(ref.allele) > 100
    check_first_principles(ref, idx, groups)
    for entries in (1, 3, 17):
        small = _quiet(hal.compute_hit_alleles, motif, idx, regions, False, args, carriers=True, haplotype_groups=groups,
                       scratch_bytes=entries * 4 * (96 + 2))
        _same(small, ref)
    monkeypatch.setattr(hal, "_FIRST_ALLELES_PER_ENTRY", 0)          # no room at first: the call is made again with the count
    _same(_quiet(hal.compute_hit_alleles, motif, idx, regions, False, args, carriers=True, haplotype_groups=groups), ref)
    bare = _quiet(hal.compute_hit_alleles, motif, idx, regions, False, args)
    assert bare.carrier_bits is None and bare.group_names == [] and bare.group_counts.shape == (len(ref), 0)
    assert np.array_equal(bare.allele_site, ref.allele_site) and np.array_equal(bare.allele_offsets, ref.allele_offsets)


def test_many_equals_single_calls():
    from grafimo_amd.hit_alleles import compute_hit_alleles, compute_hit_alleles_many
    idx = random_bitset_index(65, 29, length=300, n_sites=40)
    motifs = [_motif(8, 1), _motif(12, 2), _motif(8, 3), _motif(8, 4), _motif(8, 5)]
    args = _Args(threshold=0.05)
    regions = [(0, 180), (120, 300)]
    groups = _groups(65, np.random.default_rng(2))
    many = _quiet(compute_hit_alleles_many, motifs, idx, regions, False, args, carriers=True, haplotype_groups=groups)
    assert len(many) == len(motifs)
    for m, t in zip(motifs, many):
        one = _quiet(compute_hit_alleles, m, idx, regions, False, args, carriers=True, haplotype_groups=groups)
        assert (t.report["motif_id"] == m.motif_id).all() and len(t) > 0
        _same(t, one)


def test_two_chromosomes_as_lists():
    from grafimo_amd.hit_alleles import compute_hit_alleles
    a = random_bitset_index(20, 31, length=200, n_sites=25, chrom="a")
    b = random_bitset_index(20, 32, length=220, n_sites=30, chrom="b")
    motif = _motif(7, 1)
    args = _Args(threshold=0.05)
    both = _quiet(compute_hit_alleles, motif, [a, b], [[(0, 200)], [(10, 220)]], False, args, carriers=True)
    one_a = _quiet(compute_hit_alleles, motif, a, [(0, 200)], False, args, carriers=True)
    one_b = _quiet(compute_hit_alleles, motif, b, [(10, 220)], False, args, carriers=True)
    assert len(both) == len(one_a) + len(one_b) and len(one_a) and len(one_b) and both.indexes[0] is a and both.indexes[1] is b
    for e, (idx, one) in enumerate(((a, one_a), (b, one_b))):
        rows = np.flatnonzero(both.report["sequence_name"].str.startswith(idx.chrom + ":").to_numpy())
        assert len(rows) == len(one)
        assert [[(e, s, al) for _, s, al in one.alleles(k)] for k in range(len(one))] == [both.alleles(int(r)) for r in rows]
        assert np.array_equal(both.carrier_bits[rows], one.carrier_bits)
    # the strings come from the entry's own index
    fr = both.to_frame()
    for r in range(len(both)):
        idx = (a, b)[0 if fr["sequence_name"].iat[r].startswith("a:") else 1]
        want = sorted(int(idx.pos[s]) + 1 for _, s, al in both.alleles(r) if al)
        got = [int(x.split(":")[0]) for x in fr["alt_alleles"].iat[r].split(";") if x]
        assert got == want


def test_a_graph_without_haplotypes_gives_alleles_and_refuses_groups():
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.hit_alleles import compute_hit_alleles
    ref = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    idx = GraphIndex("c", ref, np.array([10, 40], np.int32), np.array([1, 2], np.uint8),
                     np.array([[ord("A"), 0, 0], [ord("C"), ord("G"), 0]], np.uint8), None, 0)
    motif = _motif(8)
    args = _Args(threshold=1.0, recomb=True)
    ha = _quiet(compute_hit_alleles, motif, idx, [(0, 100)], False, args)
    assert len(ha) > 100 and ha.haplotype_names == [] and ha.carrier_bits is None
    assert (ha.report["haplotype_frequency"] == 0).all()
    per_row = np.diff(ha.allele_offsets)
    assert per_row.max() == 1 and per_row.sum() > 40          # (the two sites are 30 bases apart: one per window at most)
    assert sorted(set(zip(ha.allele_site.tolist(), ha.allele.tolist()))) == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
    assert set(ha.to_frame()["alt_alleles"]) == {"", "11:G>A", "41:A>C", "41:A>G"}
    with pytest.raises(ValueError, match="carries no haplotypes"):
        compute_hit_alleles(motif, idx, [(0, 100)], False, args, carriers=True)
    with pytest.raises(ValueError, match="carries no haplotypes"):
        compute_hit_alleles(motif, idx, [(0, 100)], False, args, haplotype_groups={"g": [0]})


def test_the_library_refuses_what_it_cannot_serve():
    """65 groups; groups, totals or masks of a graph without bitsets -- GFM_ERR_INVALID from the C call itself"""
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex, compute_results_from_graph
    from grafimo_amd.hit_alleles import compute_hit_alleles
    idx = random_bitset_index(10, 3, length=120, n_sites=10)
    with pytest.raises(ValueError, match="at most 64"):
        compute_hit_alleles(_motif(6), idx, [(0, 120)], False, _Args(threshold=0.05), haplotype_groups={f"g{k}": [0] for k in range(65)})
    g = DeviceGraph(idx)
    ref = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    bare = DeviceGraph(GraphIndex("c", ref, np.array([10], np.int32), np.array([1], np.uint8), np.array([[ord("A"), 0, 0]], np.uint8), None, 0))
    try:
        for dg in (g, bare):
            _quiet(compute_results_from_graph, _motif(6), dg, [(0, 100)], False, _Args(threshold=0.05))
        dev = g.device
        off = torch.zeros(9, dtype=torch.int64, device=dev)
        room = torch.zeros(1024, dtype=torch.int64, device=dev)
        buf, cap = g.fused_buffers(0, 0)
        call = lambda dg, b, c, G, tot, masks: nv.lib().gfm_graph_hit_alleles(      # noqa: E731
            dg._h, b.data_ptr() + 128 + 120 * c, b.data_ptr(), 8, None, G, room.data_ptr() if G else None, off.data_ptr(), None, 0,
            room.data_ptr() if G else None, room.data_ptr() if tot else None, room.data_ptr() if masks else None, 0, None)
        assert call(g, buf, cap, 65, False, False) == nv.GFM_ERR_INVALID and b"65 groups" in nv.lib().gfm_last_error()
        assert call(g, buf, cap, -1, False, False) == nv.GFM_ERR_INVALID
        assert call(g, buf, cap, 64, True, True) == nv.GFM_OK
        b2, c2 = bare.fused_buffers(0, 0)
        assert call(bare, b2, c2, 0, False, False) == nv.GFM_OK
        for G, tot, masks in ((1, False, False), (0, True, False), (0, False, True)):
            assert call(bare, b2, c2, G, tot, masks) == nv.GFM_ERR_INVALID
            assert b"carries no haplotypes" in nv.lib().gfm_last_error()
        torch.cuda.synchronize()
    finally:
        g.close()
        bare.close()


def test_zero_hits_give_an_empty_table_with_the_columns():
    from grafimo_amd.extract_regions import compute_results_from_graph
    from grafimo_amd.hit_alleles import compute_hit_alleles
    idx = random_bitset_index(10, 3, length=120, n_sites=10)
    motif = _motif(19, 1)
    args = _Args(threshold=1e-12)
    ha = _quiet(compute_hit_alleles, motif, idx, [(0, 120)], False, args, carriers=True, haplotype_groups={"g": [0, 1]})
    rep = _quiet(compute_results_from_graph, motif, idx, [(0, 120)], False, args)
    assert len(ha) == 0 and len(rep) == 0
    pd.testing.assert_frame_equal(ha.report, rep)
    assert ha.allele_offsets.tolist() == [0] and ha.group_counts.shape == (0, 1) and ha.carrier_bits.shape == (0, 1)
    assert list(ha.to_frame().columns) == list(rep.columns) + ["alt_alleles", "ref_alleles", "haplotypes_g"]


@pytest.fixture()
def mygenome(tmp_path, monkeypatch):
    import shutil
    g = tmp_path / "data" / "mygenome"
    shutil.copytree(os.path.join(GOLD, "mygenome"), g)     # (scan_graph saves x.gfmidx.npz beside x.xg)
    monkeypatch.setenv("GRAFIMO_INDEX_CACHE", str(tmp_path / "cache"))
    monkeypatch.delenv("GRAFIMO_SCAN_OUTPUT", raising=False)
    return str(g)


def test_manifest_route_equals_fasta_vcf_route(tmp_path, mygenome, monkeypatch):
    """vg's x.xg + x.gbwt through scan_graph's manifest against xy.fa + xy2.vcf.gz: the same rows, carriers and -- printed
    as VCF positions -- alleles (the two routes number their sites on their own)"""
    import shutil
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex, read_bed_regions, read_manifest, scan_graph
    from grafimo_amd.hit_alleles import compute_hit_alleles
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
        args = _Args(threshold=0.05)
        a = _quiet(compute_hit_alleles, motif, man, None, False, args, carriers=True, haplotype_groups={"one": [0], "two": [1]})
        idx = GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), "x")
        b = _quiet(compute_hit_alleles, motif, DeviceGraph(idx), read_bed_regions(bed)["chrx"], False, args, carriers=True,
                   haplotype_groups={"one": ["1|1"], "two": ["1|2"]})
        assert a.haplotype_names == ["hap0", "hap1"] and b.haplotype_names == ["1|1", "1|2"]
        assert len(a) > 0 and (a.report["reference"] == "non.ref").any()
        pd.testing.assert_frame_equal(a.to_frame(), b.to_frame())
        assert np.array_equal(a.carrier_bits, b.carrier_bits) and np.array_equal(a.group_counts, b.group_counts)
    finally:
        shutil.rmtree(loc, ignore_errors=True)


def test_cli_writes_the_table_and_leaves_the_report_alone(tmp_path):
    base = [sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", os.path.join(GOLD, "xy.fa"),
            "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed"), "-t", "0.05"]
    panel = tmp_path / "panel.txt"
    panel.write_text("sample\tpop\n1\tPOP\nnobody\tPOP\n")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run(base + ["-o", a], check=True, cwd=str(tmp_path), env=env, timeout=600)
    r = subprocess.run(base + ["-o", b, "--hit-alleles", "--haplotype-groups", str(panel)], check=True, cwd=str(tmp_path), env=env,
                       timeout=600, capture_output=True, text=True)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fb == sorted(fa + ["grafimo_hit_alleles.tsv"])
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert "hit allele rows written to" in r.stdout
    t = pd.read_csv(os.path.join(b, "grafimo_hit_alleles.tsv"), sep="\t", keep_default_na=False)
    rep = pd.read_csv(os.path.join(a, "grafimo_out.tsv"), sep="\t", index_col=0, keep_default_na=False)
    assert list(t.columns) == list(rep.columns) + ["alt_alleles", "ref_alleles", "haplotypes_POP"]      # the report's columns lead
    assert len(t) == len(rep) and t["matched_sequence"].tolist() == rep["matched_sequence"].tolist()
    assert (t["haplotypes_POP"] == t["haplotype_frequency"]).all() and (t["alt_alleles"] != "").any()
    assert ((t["reference"] == "ref") <= (t["alt_alleles"] == "")).all()
    # -f prints the table instead of writing it
    r = subprocess.run(base + ["-o", str(tmp_path / "c"), "-f", "--hit-alleles"], check=True, cwd=str(tmp_path), env=env,
                       timeout=600, capture_output=True, text=True)
    assert "\talt_alleles\tref_alleles\n" in r.stdout
    assert not os.path.exists(tmp_path / "c" / "grafimo_hit_alleles.tsv")
