"""Hit-pair table on the GPU.  Kernel level: grafimo_amd.hit_pairs.pair_rows (gfm_hit_pairs) against the O(n^2) numpy
restatement of its contract; end to end: compute_hit_pairs against the haplotype brute force and first principles
(tests/hit_pair_bruteforce.py), the manifest route and the CLI.  Every comparison is exact.
The width sweep sits on every sub-group width of pair_kernel (L = 1 .. 64 lanes a row): 130 haplotypes are 3 words (L = 4, a
lane idle), 300 are 5 (L = 8), 1 000 are 16 (= L), 1 100 are 18 (L = 32, the second register word partly used), 2 100 are 33
(L = 64), 8 192 are 128 (= 2 L, the last row kept in registers), 8 193 are 129 (the first read from memory), 12 345 are 193
(three full turns of the word loop and a partial one)."""
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

from extract_helpers import make_consistent_graph_files  # noqa: E402
from graph_table_checks import random_bitset_index  # noqa: E402
from hit_pair_bruteforce import check_pairs, pack, pairs_reference  # noqa: E402
from test_gpu_hit_alleles import FLAGS, _Args, _groups, _motif, _quiet  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")


# ---- the kernel: pair_rows against pairs_reference

def _random_rows(rng, n, H, n_groups_of_rows, span, width=(4, 20), density=0.3, sort=False):
    group = rng.integers(0, n_groups_of_rows, n).astype(np.int32)
    lo = rng.integers(0, span, n).astype(np.int64)
    hi = lo + rng.integers(width[0], width[1] + 1, n)
    member = rng.random((n, H)) < density
    member[rng.random(n) < 0.1] = False                                   # rows without carriers
    masks = pack(member)
    if sort:
        o = np.lexsort((hi, lo, group))
        group, lo, hi, masks = group[o], lo[o], hi[o], masks[o]
    return group, lo, hi, masks


def _same(got, exp):
    for g, e, name in zip(got, exp, ("a", "b", "joint", "group_counts")):
        assert g.dtype == e.dtype and g.shape == e.shape, (name, g.dtype, e.dtype, g.shape, e.shape)
        assert np.array_equal(g, e), name
    return len(exp[0])


@pytest.mark.parametrize("H", [1, 63, 64, 65, 130, 200, 300, 1000, 1100, 2100, 5096, 8192, 8193, 12345])
@pytest.mark.parametrize("G", [0, 5])
def test_pair_rows_equals_the_reference_at_every_bitset_width(H, G):
    from grafimo_amd.hit_pairs import pair_rows
    rng = np.random.default_rng(1000 + H + G)
    n = 700 if H < 5000 else 400
    group, lo, hi, masks = _random_rows(rng, n, H, 6, 400, density=0.5 if H == 1 else 0.02 if H > 1000 else 0.1)
    gb = pack(rng.random((G, H)) < 0.4) if G else None
    for min_gap, max_gap in ((0, 50), (-8, 30)):
        got = pair_rows(group, lo, hi, masks, min_gap, max_gap, group_bits=gb, n_haplotypes=H)
        exp = pairs_reference(group, lo, hi, masks, min_gap, max_gap, group_bits=gb)
        assert _same(got, exp) > 300
        # some candidates within the gap share nobody: the intersection decides
        assert len(exp[0]) < len(pairs_reference(group, lo, hi, np.ones((n, 1), np.uint64), min_gap, max_gap)[0])


@pytest.mark.parametrize("n", [0, 1, 2])
def test_zero_one_and_two_rows(n):
    from grafimo_amd.hit_pairs import pair_rows
    group, lo, hi = np.zeros(n, np.int32), np.arange(n, dtype=np.int64) * 10, np.arange(n, dtype=np.int64) * 10 + 6
    masks = np.full((n, 2), 5, np.uint64)
    gb = np.full((3, 2), 4, np.uint64)
    a, b, joint, gc = pair_rows(group, lo, hi, masks, 0, 50, group_bits=gb)
    if n < 2:
        assert len(a) == len(b) == len(joint) == 0 and gc.shape == (0, 3)
    else:
        assert (a.tolist(), b.tolist(), joint.tolist(), gc.tolist()) == ([0], [1], [4], [[2, 2, 2]])
        assert len(pair_rows(group, lo, hi, masks, 5, 50)[0]) == 0        # the gap is 4


def test_one_group_of_3000_mutually_pairable_rows():
    from grafimo_amd.hit_pairs import pair_rows
    rng = np.random.default_rng(7)
    n, H = 3000, 130
    group = np.zeros(n, np.int32)
    lo = np.sort(rng.integers(0, 40, n)).astype(np.int64)
    hi = lo + rng.integers(1, 30, n)
    member = rng.random((n, H)) < 0.2
    member[:, 0] = True                                                   # every two rows share haplotype 0
    masks = pack(member)
    gb = pack(rng.random((2, H)) < 0.5)
    got = pair_rows(group, lo, hi, masks, -100, 100, group_bits=gb, n_haplotypes=H)
    assert len(got[0]) == n * (n - 1) // 2                                # about 4.5 million
    assert _same(got, pairs_reference(group, lo, hi, masks, -100, 100, group_bits=gb)) == n * (n - 1) // 2


def test_many_tiny_groups_and_groups_around_the_wave_steps():
    """groups of 1 .. 3 rows, and groups of 63 .. 130 rows: with one word per row a step of the kernel takes 64 candidates,
    with two words 32, ...: groups that end just before, on and just behind a step"""
    from grafimo_amd.hit_pairs import pair_rows
    rng = np.random.default_rng(11)
    total = 0
    for H in (40, 100, 200, 500, 2100, 4100):
        sizes = [1, 2, 3, 1, 1, 2] * 40 + [15, 16, 17, 31, 32, 33, 34, 63, 64, 65, 66, 127, 128, 129, 130]
        group = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
        n = len(group)
        lo = rng.integers(0, 30, n).astype(np.int64)
        hi = lo + rng.integers(2, 10, n)
        masks = pack(rng.random((n, H)) < (0.03 if H < 1000 else 0.003))
        got = pair_rows(group, lo, hi, masks, -10, 40, n_haplotypes=H)
        total += _same(got, pairs_reference(group, lo, hi, masks, -10, 40))
        assert len(got[0]) > 500
    assert total > 10_000


@pytest.mark.parametrize("G", [1, 64])
def test_group_counts_of_1_and_64_groups(G):
    from grafimo_amd.hit_pairs import pair_rows
    rng = np.random.default_rng(20 + G)
    for H in (65, 5096):
        group, lo, hi, masks = _random_rows(rng, 300, H, 3, 200, density=0.05)
        gb = pack(rng.random((G, H)) < 0.3)
        gb[0] = pack(np.ones((1, H), bool))[0]                            # group 0: every haplotype
        got = pair_rows(group, lo, hi, masks, 0, 60, group_bits=gb, n_haplotypes=H)
        assert _same(got, pairs_reference(group, lo, hi, masks, 0, 60, group_bits=gb)) > 200
        assert np.array_equal(got[3][:, 0], got[2])


@pytest.mark.parametrize("min_gap,max_gap", [(-30, -1), (-5, 0), (0, 0), (3, 3), (-1000, 1000)])
def test_negative_and_zero_gaps(min_gap, max_gap):
    from grafimo_amd.hit_pairs import pair_rows
    rng = np.random.default_rng(33)
    group, lo, hi, masks = _random_rows(rng, 900, 70, 4, 300, width=(1, 40), density=0.2)
    got = pair_rows(group, lo, hi, masks, min_gap, max_gap)
    assert _same(got, pairs_reference(group, lo, hi, masks, min_gap, max_gap)) > 50


def test_tie_break_keys_decide_the_order_of_equal_intervals():
    from grafimo_amd.hit_pairs import pair_rows
    rng = np.random.default_rng(44)
    n = 400
    group = rng.integers(0, 3, n).astype(np.int32)
    lo = rng.integers(0, 12, n).astype(np.int64)                          # many equal (lo, hi)
    hi = lo + rng.integers(3, 5, n)
    masks = pack(rng.random((n, 9)) < 0.4)
    t1, t2 = rng.integers(0, 3, n), rng.permutation(n)
    got = pair_rows(group, lo, hi, masks, -4, 5, tie=(t1, t2))
    assert _same(got, pairs_reference(group, lo, hi, masks, -4, 5, tie=(t1, t2))) > 1000
    other = pair_rows(group, lo, hi, masks, -4, 5)
    assert not np.array_equal(other[0], got[0])                           # (the keys matter)
    as_set = lambda r: {(min(x, y), max(x, y), j) for x, y, j in zip(r[0].tolist(), r[1].tolist(), r[2].tolist())}      # noqa: E731
    assert as_set(other) == as_set(got)
    # torch tensors are taken as well
    import torch
    tt = pair_rows(torch.from_numpy(group), torch.from_numpy(lo).cuda(), torch.from_numpy(hi), torch.from_numpy(masks.view(np.int64)),
                   -4, 5, tie=(t1, t2))
    _same(tt, got)


def _raw_call(group, lo, hi, masks, min_gap, max_gap, cap=0, flags=0):
    """gfm_hit_pairs itself on the rows as given -> (return code, total, offsets, b, joint)"""
    import torch
    from grafimo_amd import _native as nv
    n, hw = masks.shape
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (group.astype(np.int32), lo.astype(np.int64), hi.astype(np.int64),
                                                                     masks.view(np.int64))]
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    b = torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda")
    joint = torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda")
    total = ctypes.c_int64(-1)
    rc = nv.lib().gfm_hit_pairs(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, hw, min_gap, max_gap, 0, None,
                                off.data_ptr(), cap, b.data_ptr() if cap else None, joint.data_ptr() if cap else None, None, flags,
                                ctypes.byref(total), None)
    torch.cuda.synchronize()
    return rc, int(total.value), off.cpu().numpy(), b.cpu().numpy(), joint.cpu().numpy()


def test_the_entry_refuses_unsorted_rows_and_counts_before_it_writes():
    from grafimo_amd import _native as nv
    rng = np.random.default_rng(55)
    group, lo, hi, masks = _random_rows(rng, 500, 65, 5, 300, sort=True)
    exp = pairs_reference(group, lo, hi, masks, 0, 40)
    P = len(exp[0])
    assert P > 100
    # capacity 0: the offsets and the total, nothing else
    rc, total, off, _, _ = _raw_call(group, lo, hi, masks, 0, 40)
    assert rc == nv.GFM_OK and total == P and off[0] == 0 and off[-1] == P
    assert np.array_equal(np.diff(off), np.bincount(exp[0], minlength=500))
    # too little room: untouched pair arrays, the total again
    rc, total, _, b, joint = _raw_call(group, lo, hi, masks, 0, 40, cap=P - 1)
    assert rc == nv.GFM_OK and total == P and (b == -7).all() and (joint == -7).all()
    # room: the pairs, ascending b per row
    rc, total, off2, b, joint = _raw_call(group, lo, hi, masks, 0, 40, cap=P + 3)
    assert rc == nv.GFM_OK and total == P and np.array_equal(off2, off)
    assert np.array_equal(b[:P], exp[1]) and np.array_equal(joint[:P], exp[2]) and (b[P:] == -7).all()
    # out of order: by group, by lo inside a group; lo > hi
    for swap in ("group", "lo", "lohi"):
        g2, l2, h2 = group.copy(), lo.copy(), hi.copy()
        if swap == "group":
            g2[[0, -1]] = g2[[-1, 0]]
        elif swap == "lo":
            k = int(np.flatnonzero((np.diff(group) == 0) & (np.diff(lo) > 0))[0])
            l2[[k, k + 1]] = l2[[k + 1, k]]
            h2[[k, k + 1]] = h2[[k + 1, k]]
        else:
            l2[7], h2[7] = h2[7] + 1, l2[7]
        rc, total, _, _, _ = _raw_call(g2, l2, h2, masks, 0, 40, cap=P + 3)
        assert rc == nv.GFM_ERR_INVALID and total == 0 and b"ascending (group, lo)" in nv.lib().gfm_last_error(), swap
    rc, _, _, _, _ = _raw_call(group, lo, hi, masks, 5, 4)
    assert rc == nv.GFM_ERR_INVALID


def test_max_pairs_is_refused_with_the_count():
    from grafimo_amd.hit_pairs import pair_rows
    rng = np.random.default_rng(66)
    group, lo, hi, masks = _random_rows(rng, 400, 65, 2, 100)
    P = len(pairs_reference(group, lo, hi, masks, 0, 40)[0])
    assert P > 100
    with pytest.raises(OverflowError, match=str(P)):
        pair_rows(group, lo, hi, masks, 0, 40, max_pairs=P - 1)
    assert len(pair_rows(group, lo, hi, masks, 0, 40, max_pairs=P)[0]) == P


# ---- end to end

MOTIF_SETS = {"one": [(8, 1)], "mixed": [(5, 1), (11, 2), (5, 3)], "twice": [(7, 1), (12, 2), (7, 1)]}


def _motif_set(name):
    ms = [_motif(W, s) for W, s in MOTIF_SETS[name]]
    if name == "twice":
        ms[2] = ms[0]
    return ms


def _reports_equal(hp, motifs, graph, regions, args, **kw):
    from grafimo_amd.extract_regions import compute_results_from_graph
    for m, motif in enumerate(motifs):
        try:
            rep = _quiet(compute_results_from_graph, motif, graph, regions, False, args, **kw)
        except SystemExit:
            assert len(hp.tables[m]) == 0
            continue
        pd.testing.assert_frame_equal(hp.tables[m].report, rep)


@pytest.mark.parametrize("seed,H,mset,flags,gap,least", [
    (1, 63, "mixed", "default", (0, 50), 20), (2, 65, "twice", "recomb", (-64, 10), 20), (3, 131, "one", "no_reverse", (0, 20), 3),
    (4, 5, "mixed", "threshold_1", (0, 0), 20), (9, 67, "twice", "qvalueT", (-3, 50), 20), (6, 7, "mixed", "qvalues", (-3, 50), 20),
    (7, 33, "one", "no_qvalue", (0, 50), 3)])
def test_bruteforce_parity_on_random_bitsets(seed, H, mset, flags, gap, least):
    from grafimo_amd.hit_pairs import compute_hit_pairs
    idx = random_bitset_index(H, 600 + seed, length=150, n_sites=22)
    regions = [(0, 150), (30, 95), (-5, 40), (100, 400), (50, 50), (30, 95)]              # overlapping, clipped, empty, one twice
    motifs = _motif_set(mset)
    args = _Args(**{**dict(threshold=0.05), **FLAGS[flags]})
    groups = _groups(H, np.random.default_rng(seed))
    hp = _quiet(compute_hit_pairs, motifs, idx, regions, False, args, haplotype_groups=groups, min_gap=gap[0], max_gap=gap[1])
    assert check_pairs(hp, [(idx, regions)], motifs, args, gap[0], gap[1], groups) >= least
    _reports_equal(hp, motifs, idx, regions, args)
    if len(hp):
        assert np.array_equal(hp.group_counts[:, list(groups).index("all")], hp.co_haplotypes)
        assert not hp.group_counts[:, list(groups).index("none")].any()
        # the region listed twice: the same pairs under both listings
        one, two = hp.region == 1, hp.region == 5
        assert one.sum() == two.sum() and np.array_equal(hp.co_haplotypes[one], hp.co_haplotypes[two])
    if flags == "recomb":
        assert any((t.report["haplotype_frequency"] == 0).any() for t in hp.tables)


@pytest.mark.parametrize("seed,mset,flags,gap", [
    (1, "mixed", "default", (0, 50)), (2, "twice", "recomb", (-20, 30)), (3, "one", "no_reverse", (0, 50)),
    (4, "mixed", "qvalueT", (0, 50)), (7, "twice", "qvalues", (-3, 25))])
def test_bruteforce_parity_on_vcf_graphs(tmp_path, seed, mset, flags, gap):
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.hit_pairs import compute_hit_pairs
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=260, n_samples=6, seed=seed, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    p = idx.pos
    regions = [(0, int(p[len(p) // 3]) + 1), (int(p[len(p) // 3]) - 2, int(p[2 * len(p) // 3])), (int(p[-3]), 260), (0, 260), (3, 4)]
    motifs = _motif_set(mset)
    args = _Args(**{**dict(threshold=0.05), **FLAGS[flags]})
    groups = {"first": ["s0|1", "s0|2", "s1|1"], "second": [3, 4, 5, 6]}
    hp = _quiet(compute_hit_pairs, motifs, idx, regions, False, args, haplotype_groups=groups, min_gap=gap[0], max_gap=gap[1])
    n = check_pairs(hp, [(idx, regions)], motifs, args, gap[0], gap[1], {"first": [0, 1, 2], "second": [3, 4, 5, 6]})
    assert n >= 10
    _reports_equal(hp, motifs, idx, regions, args)
    assert (~hp.reference).any() or flags == "qvalueT"


def test_two_chromosome_entries():
    from grafimo_amd.hit_pairs import compute_hit_pairs
    a = random_bitset_index(20, 31, length=200, n_sites=25, chrom="a")
    b = random_bitset_index(20, 32, length=220, n_sites=30, chrom="b")
    motifs = _motif_set("mixed")
    args = _Args(threshold=0.05)
    regs = [[(0, 200), (50, 120)], [(10, 220)]]
    hp = _quiet(compute_hit_pairs, motifs, [a, b], regs, False, args, min_gap=0, max_gap=40)
    assert check_pairs(hp, [(a, regs[0]), (b, regs[1])], motifs, args, 0, 40) > 20
    assert set(hp.region.tolist()) == {0, 1, 2}
    fr = hp.to_frame()
    assert set(fr["sequence_name"]) == {"a:0-200", "a:50-120", "b:10-220"}
    _reports_equal(hp, motifs, [a, b], regs, args)


def test_refusals():
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.hit_pairs import compute_hit_pairs
    ref = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    bare = GraphIndex("c", ref, np.array([10, 40], np.int32), np.array([1, 2], np.uint8),
                      np.array([[ord("A"), 0, 0], [ord("C"), ord("G"), 0]], np.uint8), None, 0)
    args = _Args(threshold=0.5)
    with pytest.raises(ValueError, match="carries no haplotypes"):
        compute_hit_pairs([_motif(8)], bare, [(0, 100)], False, args)
    a = random_bitset_index(20, 31, length=200, n_sites=25, chrom="a")
    b = random_bitset_index(21, 32, length=220, n_sites=30, chrom="b")
    with pytest.raises(ValueError, match="do not share one haplotype set"):
        compute_hit_pairs([_motif(8)], [a, b], [[(0, 200)], [(10, 220)]], False, args)
    with pytest.raises(ValueError, match="min_gap"):
        compute_hit_pairs([_motif(8)], a, [(0, 200)], False, args, min_gap=3, max_gap=2)
    with pytest.raises(OverflowError, match="hit pairs, more than max_pairs = 5"):
        _quiet(compute_hit_pairs, [_motif(8)], a, [(0, 200)], False, args, max_pairs=5)


def test_zero_rows_give_an_empty_table_with_the_columns():
    from grafimo_amd.hit_pairs import compute_hit_pairs
    idx = random_bitset_index(10, 3, length=120, n_sites=10)
    hp = _quiet(compute_hit_pairs, [_motif(19, 1)], idx, [(0, 120)], False, _Args(threshold=1e-12), haplotype_groups={"g": [0, 1]})
    assert len(hp) == 0 and hp.group_counts.shape == (0, 1)
    cols = list(hp.to_frame().columns)
    assert cols[0] == "sequence_name" and cols[-4:] == ["gap", "co_haplotypes", "haplotypes_g", "reference"] and len(cols) == 23


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
    from grafimo_amd.hit_pairs import compute_hit_pairs
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.workflow import Findmotif
    bed = os.path.join(tmp_path, "x.bed")
    with open(os.path.join(GOLD, "regions.bed")) as src, open(bed, "w") as dst:
        dst.writelines(line for line in src if line.startswith("chrx\t"))
    wf = Findmotif(graph_genome_dir=mygenome, bedfile=bed, cores=2, threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "example.meme"), wf, 2, True, pvalue_matrix=False)[0]
    motifs = [motif, motif]
    monkeypatch.setenv("GRAFIMO_SCAN_OUTPUT", "manifest")
    with contextlib.redirect_stdout(io.StringIO()):
        loc = scan_graph({motif.width}, wf, True)
    try:
        man = read_manifest(loc)
        assert man is not None
        args = _Args(threshold=0.05)
        a = _quiet(compute_hit_pairs, motifs, man, None, False, args, haplotype_groups={"one": [0], "two": [1]}, min_gap=-10, max_gap=60)
        idx = GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), "x")
        regions = read_bed_regions(bed)["chrx"]
        b = _quiet(compute_hit_pairs, motifs, DeviceGraph(idx), regions, False, args, haplotype_groups={"one": ["1|1"], "two": ["1|2"]},
                   min_gap=-10, max_gap=60)
        assert len(a) > 10 and (~a.reference).any()
        pd.testing.assert_frame_equal(a.to_frame(), b.to_frame())
        for k in ("region", "motif_a", "row_a", "motif_b", "row_b", "gap", "co_haplotypes", "group_counts"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert (a.motif_a != a.motif_b).any() and (a.motif_a == a.motif_b).any()
        check_pairs(b, [(idx, [tuple(r) for r in regions])], motifs, args, -10, 60, {"one": [0], "two": [1]}, chrom_names=["x"])
    finally:
        shutil.rmtree(loc, ignore_errors=True)


def test_cli_writes_the_table_and_leaves_the_report_alone(tmp_path):
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex, read_bed_regions
    from grafimo_amd.hit_pairs import compute_hit_pairs
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.workflow import Findmotif
    base = [sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "example.meme"), "-l", os.path.join(GOLD, "xy.fa"),
            "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed"), "-t", "0.05"]
    panel = tmp_path / "panel.txt"
    panel.write_text("sample\tpop\n1\tPOP\nnobody\tPOP\n")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run(base + ["-o", a], check=True, cwd=str(tmp_path), env=env, timeout=600)
    r = subprocess.run(base + ["-o", b, "--hit-pairs", "--pair-gap", "-15", "200", "--haplotype-groups", str(panel)], check=True,
                       cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fb == sorted(fa + ["grafimo_hit_pairs.tsv"])
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert "hit pair rows written to" in r.stdout
    t = pd.read_csv(os.path.join(b, "grafimo_hit_pairs.tsv"), sep="\t", keep_default_na=False)
    # the same call through the library
    wf = Findmotif(threshold=0.05, cores=2)
    motifs = get_motif_pwm(os.path.join(GOLD, "example.meme"), wf, 2, False, pvalue_matrix=False)
    graphs, regs = [], []
    for chrom, rr in read_bed_regions(os.path.join(GOLD, "regions.bed")).items():
        graphs.append(DeviceGraph(GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), chrom.split("chr")[1])))
        regs.append(rr)
    hp = _quiet(compute_hit_pairs, motifs, graphs, regs, False, wf, haplotype_groups={"POP": [0, 1]}, min_gap=-15, max_gap=200)
    assert len(hp) >= 3
    buf = io.StringIO()
    hp.to_frame().to_csv(buf, sep="\t", index=False)
    pd.testing.assert_frame_equal(t, pd.read_csv(io.StringIO(buf.getvalue()), sep="\t", keep_default_na=False))
    assert open(os.path.join(b, "grafimo_hit_pairs.tsv")).read() == buf.getvalue()
    assert (t["haplotypes_POP"] == t["co_haplotypes"]).all() and (t["gap"] >= -15).all() and (t["gap"] <= 200).all()
    # -f prints the table instead of writing it
    r = subprocess.run(base + ["-o", str(tmp_path / "c"), "-f", "--hit-pairs"], check=True, cwd=str(tmp_path), env=env,
                       timeout=600, capture_output=True, text=True)
    assert "\tgap\tco_haplotypes\treference\n" in r.stdout
    assert not os.path.exists(tmp_path / "c" / "grafimo_hit_pairs.tsv")
