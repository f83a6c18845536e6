"""Hit-linkage table on the GPU.  Kernel level: grafimo_amd.hit_linkage.link_rows (gfm_hit_linkage) against the numpy /
Python restatement of its contract on synthetic rows; end to end: compute_hit_linkage through check_linkage
(tests/hit_linkage_bruteforce.py), the manifest route and the CLI.  Every comparison is exact but check_linkage's one
against np.corrcoef.
The width sweep sits on every staging step of link_kernel (2^logWC words, logWC 0 .. 4): 300 haplotypes are 5 words (logWC 3,
a partial step), 512 are 8 (a full step of 8), 1 024 are 16 (one full step of 16, no tail mask), 1 025 are 17 (16 + 1)."""
import contextlib
import ctypes
import functools
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

from graph_table_checks import random_bitset_index  # noqa: E402
from hit_linkage_bruteforce import check_linkage, links_reference, synthetic_input  # noqa: E402
from hit_pair_bruteforce import pack  # noqa: E402
from test_gpu_hit_alleles import FLAGS, _Args, _motif, _quiet  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
CUTS = ((60, 0.2), (0, 0.8), (200, 0.5), (60, 0.0), (60, 1.0))
TILE = 32                                                     # R * waves: the rows of a tile of the kernel's default cut


# ---- the kernel: link_rows against links_reference

@functools.lru_cache(maxsize=None)
def _input(H):
    return synthetic_input(100 + H, H, n_rows=120 if H >= 5096 else 300)


@functools.lru_cache(maxsize=None)
def _expected(H, flank, min_r2):
    return links_reference(*_input(H), flank, min_r2, H)


def _same(got, exp):
    for g, e, name in zip(got, exp, ("row", "site", "allele", "n_joint", "n_hit", "n_allele")):
        assert g.dtype == e.dtype and g.shape == e.shape, (name, g.dtype, e.dtype, g.shape, e.shape)
        assert np.array_equal(g, e), name
    return len(exp[0])


# 1100 haplotypes are 18 words: one full staging step of 16 words and one of 2; 5096 are 80: five steps
@pytest.mark.parametrize("H", [1, 2, 63, 64, 65, 200, 300, 512, 1024, 1025, 1100, 5096])
def test_link_rows_equals_the_reference_at_every_bitset_width(H):
    from grafimo_amd.hit_linkage import link_rows
    for flank, min_r2 in CUTS:
        exp = _expected(H, flank, min_r2)
        L = _same(link_rows(*_input(H), flank, min_r2, H), exp)
        print(f"H {H} flank {flank} min_r2 {min_r2}: {L} links of {exp[9]} candidates")
        if H == 1:
            assert L == 0 and exp[9] > 500                    # every row is undefined
        elif H >= 63 and (flank, min_r2) == (60, 0.2):
            # (the reference gives 51 .. 178 links here; a kernel that lists everything, or nothing, fails)
            assert L >= 40 and L < 0.1 * exp[9]
        elif H >= 63 and min_r2 == 0.0:
            assert L > 0.5 * exp[9]                           # every defined candidate


def test_the_window_ends_are_inclusive():
    from grafimo_amd.hit_linkage import link_rows
    H, flank = 8, 7
    row = pack(np.array([[1, 1, 0, 0, 0, 0, 0, 0]], bool))
    lo, hi = 1000, 1012
    pos = [lo - flank - 1, lo - flank, lo, hi - 1, hi - 1 + flank, hi + flank]
    bits = np.zeros((6, 3, 1), np.uint64)
    bits[:, 0] = row[0]
    bits[:, 1:] = row[0]                                      # unused slots that would link perfectly
    got = link_rows([lo], [hi], row, pos, [1] * 6, bits, flank, 1.0, H)
    _same(got, links_reference([lo], [hi], row, pos, [1] * 6, bits, flank, 1.0, H))
    assert got[1].tolist() == [1, 2, 3, 4] and got[3].tolist() == [2] * 4
    # an empty interval (lo == hi) with flank 0 reaches no site, with flank 1 the sites at lo - 1 and lo
    e0 = link_rows([lo], [lo], row, [lo - 1, lo, lo + 1], [1] * 3, bits[:3], 0, 1.0, H)
    e1 = link_rows([lo], [lo], row, [lo - 1, lo, lo + 1], [1] * 3, bits[:3], 1, 1.0, H)
    assert len(e0[0]) == 0 and e1[1].tolist() == [0, 1]
    _same(e1, links_reference([lo], [lo], row, [lo - 1, lo, lo + 1], [1] * 3, bits[:3], 1, 1.0, H))


def test_equal_positions_and_three_alts_beside_garbage_slots():
    from grafimo_amd.hit_linkage import link_rows
    rng = np.random.default_rng(5)
    H = 70
    member = rng.random((6, 3, H)) < 0.3
    member[:, 1] &= ~member[:, 0]
    member[:, 2] &= ~(member[:, 0] | member[:, 1])
    bits = pack(member.reshape(18, H)).reshape(6, 3, 2)
    n_alts = np.array([1, 3, 2, 3, 1, 2], np.uint8)
    pos = np.array([50, 50, 50, 51, 51, 60])                  # an insertion, a SNP and a deletion may share a position
    unused = np.arange(3)[None, :] >= n_alts[:, None]
    bits[unused] = np.uint64(0xFFFFFFFFFFFFFFFF)              # garbage, bits beyond H among it
    rows = np.concatenate([member[1, 2:3], member[3, 0:1], ~member[5, 1:2], rng.random((5, H)) < 0.5])
    lo = np.array([40, 45, 52, 58, 30, 61, 50, 49])
    hi = lo + 6
    got = link_rows(lo, hi, pack(rows), pos, n_alts, bits, 10, 0.0, H)
    exp = links_reference(lo, hi, pack(rows), pos, n_alts, bits, 10, 0.0, H)
    assert _same(got, exp) > 40
    assert {(s, a) for s, a in zip(got[1].tolist(), got[2].tolist())} == {(s, a) for s in range(6) for a in range(1, n_alts[s] + 1)}
    strong = link_rows(lo, hi, pack(rows), pos, n_alts, bits, 10, 1.0, H)
    assert list(zip(strong[0].tolist(), strong[1].tolist(), strong[2].tolist())) == [(0, 1, 3), (1, 3, 1), (2, 5, 2)]


@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_row_counts_around_the_tile(n):
    from grafimo_amd.hit_linkage import link_rows
    lo, hi, masks, pos, n_alts, bits = _input(65)
    got = link_rows(lo[:n], hi[:n], masks[:n], pos, n_alts, bits, 60, 0.1, 65)
    exp = links_reference(lo[:n], hi[:n], masks[:n], pos, n_alts, bits, 60, 0.1, 65)
    assert _same(got, exp) >= (5 if n >= TILE - 1 else 0)
    assert got[4].shape == (n,)


def test_no_sites_rows_out_of_reach_and_windows_wider_than_a_chunk():
    from grafimo_amd.hit_linkage import link_rows
    H = 65
    lo, hi, masks, pos, n_alts, bits = _input(H)
    # no site at all: n_hit still comes back
    got = link_rows(lo, hi, masks, [], [], np.zeros((0, 3, 2), np.uint64), 60, 0.0, H)
    assert [len(x) for x in got] == [0, 0, 0, 0, len(lo), 0]
    assert np.array_equal(got[4], links_reference(lo, hi, masks, pos, n_alts, bits, 0, 1.0, H)[4])
    # rows before the first site, behind the last one and in a gap, among rows in reach
    far_lo = np.concatenate([lo[:40], [-5000, -4000, 9000, 20000]])
    far_hi = np.concatenate([hi[:40], [-4990, -3000, 9010, 20001]])
    far_masks = np.concatenate([masks[:40], masks[40:44]])
    _same(link_rows(far_lo, far_hi, far_masks, pos, n_alts, bits, 60, 0.1, H), links_reference(far_lo, far_hi, far_masks, pos, n_alts,
                                                                                            bits, 60, 0.1, H))
    only_far = link_rows(far_lo[40:], far_hi[40:], far_masks[40:], pos, n_alts, bits, 60, 0.0, H)
    assert len(only_far[0]) == 0 and np.array_equal(only_far[4], got[4][40:44])
    # flank 3 000: every row's window holds all ~800 slots, more than three chunks of 256
    assert int(np.asarray(n_alts).sum()) > 3 * 256
    wide = links_reference(lo[:70], hi[:70], masks[:70], pos, n_alts, bits, 3000, 0.3, H)
    assert wide[9] == 70 * int(np.asarray(n_alts).sum())
    assert _same(link_rows(lo[:70], hi[:70], masks[:70], pos, n_alts, bits, 3000, 0.3, H), wide) > 30


def test_the_widest_bitset():
    """32 768 haplotypes: 512 words, 32 staging steps; a larger H is refused"""
    from grafimo_amd.hit_linkage import link_rows
    H = 32768
    inp = synthetic_input(9, H, n_rows=40, n_sites=50, span=400)
    exp = links_reference(*inp, 60, 0.2, H)
    assert _same(link_rows(*inp, 60, 0.2, H), exp) >= 5 and len(exp[0]) < 0.2 * exp[9]
    with pytest.raises(ValueError, match="haplotypes"):
        link_rows(inp[0], inp[1], np.zeros((40, 513), np.uint64), inp[3], inp[4], np.zeros((50, 3, 513), np.uint64), 60, 0.2, H + 1)


def test_the_exact_tie_through_the_device():
    """H = 8, n_hit = 4, n_allele = 4, n_joint = 3: r2 == 0.25 exactly; listed at 0.25 and not one ulp above"""
    from grafimo_amd.hit_linkage import link_rows
    row = pack(np.array([[1, 1, 1, 1, 0, 0, 0, 0]], bool))
    allele = np.zeros((1, 3, 1), np.uint64)
    allele[0, 0] = pack(np.array([[1, 1, 1, 0, 1, 0, 0, 0]], bool))[0]
    at = link_rows([10], [14], row, [12], [1], allele, 0, 0.25, 8)
    assert [x.tolist() for x in at] == [[0], [0], [1], [3], [4], [4]]
    above = link_rows([10], [14], row, [12], [1], allele, 0, float(np.nextafter(0.25, 1)), 8)
    assert [len(x) for x in above] == [0, 0, 0, 0, 1, 0]
    # the device lists the cell either way (its cut has 1e-9 of slack): max_links counts it
    with pytest.raises(OverflowError, match="1 candidate links"):
        link_rows([10], [14], row, [12], [1], allele, 0, float(np.nextafter(0.25, 1)), 8, max_links=0)


def test_every_cut_of_the_work_and_a_tiny_budget_give_the_identical_table():
    from grafimo_amd.hit_linkage import ROWS_PER_TILE, SLOTS_PER_CHUNK, link_rows
    for H in (65, 1100):
        exp = _expected(H, 200, 0.5)
        assert len(exp[0]) > 50
        for rows_per_tile in (0,) + ROWS_PER_TILE:
            for slots_per_chunk in (0,) + SLOTS_PER_CHUNK:
                _same(link_rows(*_input(H), 200, 0.5, H, rows_per_tile=rows_per_tile, slots_per_chunk=slots_per_chunk), exp)
        hw = (H + 63) // 64
        for scratch in (1, 40 * (24 * hw + 48), 200 * (24 * hw + 48)):      # a row per batch, and batches of some dozen rows
            _same(link_rows(*_input(H), 200, 0.5, H, scratch_bytes=scratch), exp)
    with pytest.raises(ValueError, match="rows_per_tile"):
        link_rows(*_input(65), 200, 0.5, 65, rows_per_tile=64)
    with pytest.raises(ValueError, match="slots_per_chunk"):
        link_rows(*_input(65), 200, 0.5, 65, slots_per_chunk=512)


def test_max_links_is_refused_with_the_count_and_bad_input_raises():
    from grafimo_amd.hit_linkage import link_rows
    H = 64
    inp = _input(H)
    L = len(_expected(H, 60, 0.2)[0])
    with pytest.raises(OverflowError, match=f"{L} candidate links, more than max_links = {L - 1}"):
        link_rows(*inp, 60, 0.2, H, max_links=L - 1)
    assert len(link_rows(*inp, 60, 0.2, H, max_links=L)[0]) == L
    lo, hi, masks, pos, n_alts, bits = inp
    with pytest.raises(ValueError, match="ascending pos"):
        link_rows(lo, hi, masks, pos[::-1], n_alts, bits, 60, 0.2, H)
    lo63, hi63, masks63, pos63, n_alts63, bits63 = _input(63)
    wrong = masks63.copy()
    wrong[17, 0] |= np.uint64(1 << 63)
    with pytest.raises(ValueError, match="beyond the last haplotype"):
        link_rows(lo63, hi63, wrong, pos63, n_alts63, bits63, 60, 0.2, 63)
    wrong = bits63.copy()
    wrong[3, 0, 0] |= np.uint64(1 << 63)                       # (a used slot; the unused ones are full of such bits)
    with pytest.raises(ValueError, match="beyond the last haplotype"):
        link_rows(lo63, hi63, masks63, pos63, n_alts63, wrong, 60, 0.2, 63)
    # torch tensors are taken as well
    import torch
    tt = link_rows(torch.from_numpy(lo).cuda(), torch.from_numpy(hi), torch.from_numpy(masks.view(np.int64)), torch.from_numpy(pos),
                   torch.from_numpy(n_alts), torch.from_numpy(bits.view(np.int64)).cuda(), 60, 0.2, H)
    _same(tt, _expected(H, 60, 0.2))


def _raw_call(lo, hi, masks, pos, n_alts, bits, H, flank, min_r2, cap=0, flags=0, off=None):
    """gfm_hit_linkage itself on the input as given -> (return code, total, offsets, site, allele, joint)"""
    import torch
    from grafimo_amd import _native as nv
    n, hw = masks.shape
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (np.asarray(lo, np.int64), np.asarray(hi, np.int64), masks.view(np.int64),
                                                                     np.asarray(pos, np.int64), np.asarray(n_alts, np.uint8),
                                                                     bits.view(np.int64))]
    d_off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda") if off is None else torch.from_numpy(off).cuda()
    site = torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda")
    allele = torch.full((max(cap, 1),), 77, dtype=torch.uint8, device="cuda")
    joint = torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda")
    n_hit = torch.empty(n, dtype=torch.int32, device="cuda")
    n_allele = torch.empty((len(pos), 3), dtype=torch.int32, device="cuda")
    total = ctypes.c_int64(-1)
    rc = nv.lib().gfm_hit_linkage(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                                  len(pos), hw, H, flank, min_r2, d_off.data_ptr(), cap, site.data_ptr() if cap else None,
                                  allele.data_ptr() if cap else None, joint.data_ptr() if cap else None, n_hit.data_ptr(),
                                  n_allele.data_ptr(), 0, 0, flags, ctypes.byref(total), None)
    torch.cuda.synchronize()
    return rc, int(total.value), d_off.cpu().numpy(), site.cpu().numpy(), allele.cpu().numpy(), joint.cpu().numpy()


def test_the_entry_checks_its_input_and_counts_before_it_writes():
    from grafimo_amd import _native as nv
    H = 65
    lo, hi, masks, pos, n_alts, bits = _input(H)
    o = np.lexsort((hi, lo))
    lo, hi, masks = lo[o], hi[o], masks[o]
    exp = links_reference(lo, hi, masks, pos, n_alts, bits, 60, 1.0, H)          # (at 1.0 the device's slack adds no cell here)
    L = len(exp[0])
    assert L >= 3
    rc, total, off, _, _, _ = _raw_call(lo, hi, masks, pos, n_alts, bits, H, 60, 1.0)
    assert rc == nv.GFM_OK and total == L and off[0] == 0 and off[-1] == L
    assert np.array_equal(np.diff(off), np.bincount(exp[0], minlength=len(lo)))
    rc, total, _, site, allele, joint = _raw_call(lo, hi, masks, pos, n_alts, bits, H, 60, 1.0, cap=L - 1)
    assert rc == nv.GFM_OK and total == L and (site == -7).all() and (allele == 77).all() and (joint == -7).all()
    rc, total, off2, site, allele, joint = _raw_call(lo, hi, masks, pos, n_alts, bits, H, 60, 1.0, cap=L + 3)
    assert rc == nv.GFM_OK and total == L and np.array_equal(off2, off)
    assert np.array_equal(site[:L], exp[1]) and np.array_equal(allele[:L], exp[2]) and np.array_equal(joint[:L], exp[3])
    assert (site[L:] == -7).all()
    rc, total, _, site2, _, _ = _raw_call(lo, hi, masks, pos, n_alts, bits, H, 60, 1.0, cap=L, flags=nv.GFM_LINKAGE_HAVE_OFFSETS, off=off)
    assert rc == nv.GFM_OK and total == L and np.array_equal(site2, exp[1])
    # refused before anything is counted: rows or sites out of order, lo > hi, four ALTs, a coordinate beyond 2^61
    for what in ("rows", "sites", "lohi", "alts", "far row", "far site"):
        l2, h2, p2, a2 = lo.copy(), hi.copy(), pos.copy(), n_alts.copy()
        if what == "rows":
            k = int(np.flatnonzero(np.diff(lo) > 0)[0])
            l2[[k, k + 1]], h2[[k, k + 1]] = l2[[k + 1, k]], h2[[k + 1, k]]
        elif what == "sites":
            k = int(np.flatnonzero(np.diff(pos) > 0)[0])
            p2[[k, k + 1]] = p2[[k + 1, k]]
        elif what == "lohi":
            l2[7], h2[7] = h2[7] + 1, l2[7]
        elif what == "alts":
            a2[11] = 4
        elif what == "far row":
            h2[-1] = 1 << 61
        else:
            p2[-1] = 1 << 61
        rc, total, _, site, _, _ = _raw_call(l2, h2, masks, p2, a2, bits, H, 60, 1.0, cap=L + 3)
        assert rc == nv.GFM_ERR_INVALID and total == 0 and (site == -7).all(), what
        assert b"ascending" in nv.lib().gfm_last_error()


# ---- end to end

def _reports_equal(tables, motifs, graph, regions, args, **kw):
    from grafimo_amd.extract_regions import compute_results_from_graph
    for hl, motif in zip(tables, motifs):
        try:
            rep = _quiet(compute_results_from_graph, motif, graph, regions, False, args, **kw)
        except SystemExit:
            assert len(hl.table) == 0
            continue
        pd.testing.assert_frame_equal(hl.table.report, rep)


@pytest.mark.parametrize("seed,H,indels,flags", [(1, 63, True, "default"), (2, 130, False, "default"), (3, 130, True, "recomb"),
                                                 (4, 63, False, "no_reverse")])
def test_check_linkage_on_random_bitsets(seed, H, indels, flags):
    from grafimo_amd.hit_linkage import compute_hit_linkage
    idx = random_bitset_index(H, 700 + seed, length=300, n_sites=45, indels=indels)
    regions = [(0, 150), (120, 300), (-5, 40), (50, 50)]
    motif = _motif(8, seed)
    args = _Args(**{**dict(threshold=0.05), **FLAGS[flags]})
    hl = _quiet(compute_hit_linkage, motif, idx, regions, False, args, flank=40, min_r2=0.1)
    L = check_linkage(hl, [idx], 40, 0.1)
    print(f"seed {seed}: {L} links of {len(hl.table)} rows, {int(hl.in_hit.sum())} in their hit, {int((hl.distance > 0).sum())} outside it")
    # a row's carriers are the AND of its own alleles' carriers: those link, and the other ALTs of their sites link negatively
    assert L >= 10 and hl.in_hit.any() and (~hl.in_hit).any()
    _reports_equal([hl], [motif], idx, regions, args)
    if flags == "recomb":
        zero = np.flatnonzero(hl.table.report["haplotype_frequency"].to_numpy() == 0)
        assert len(zero) and not np.isin(hl.row, zero).any()
    # the defaults reach every site of this graph; a threshold of 1 leaves the perfect links
    every = _quiet(compute_hit_linkage, motif, idx, regions, False, args)
    assert check_linkage(every, [idx], 10000, 0.8) >= (every.r2 == 1.0).sum() > 0
    top = _quiet(compute_hit_linkage, motif, idx, regions, False, args, min_r2=1.0, rows_per_tile=8, slots_per_chunk=64, scratch_bytes=1 << 14)
    assert check_linkage(top, [idx], 10000, 1.0) == (every.r2 == 1.0).sum()


def test_two_chromosome_entries_and_a_motif_set_of_two_widths():
    from grafimo_amd.hit_linkage import compute_hit_linkage_many
    a = random_bitset_index(63, 31, length=200, n_sites=25, chrom="a")
    b = random_bitset_index(63, 32, length=220, n_sites=30, chrom="b")
    motifs = [_motif(5, 1), _motif(11, 2), _motif(5, 3)]
    args = _Args(threshold=0.05)
    regs = [[(0, 200), (50, 120)], [(10, 220)]]
    tables = _quiet(compute_hit_linkage_many, motifs, [a, b], regs, False, args, flank=50, min_r2=0.25)
    assert len(tables) == 3
    for hl in tables:
        assert check_linkage(hl, [a, b], 50, 0.25) >= 10
        assert set(hl.entry.tolist()) == {0, 1}
        fr = hl.to_frame()
        assert len(fr) == len(hl) and set(fr["sequence_name"]) <= {"a:0-200", "a:50-120", "b:10-220"}
        assert list(fr.columns[10:]) == ["variant", "distance", "allele_haplotypes", "co_haplotypes", "r2", "r", "d_prime", "in_hit"]
    _reports_equal(tables, motifs, [a, b], regs, args)


def test_refusals():
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.hit_linkage import compute_hit_linkage
    ref = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    bare = GraphIndex("c", ref, np.array([10, 40], np.int32), np.array([1, 2], np.uint8),
                      np.array([[ord("A"), 0, 0], [ord("C"), ord("G"), 0]], np.uint8), None, 0)
    args = _Args(threshold=0.5)
    with pytest.raises(ValueError, match="carries no haplotypes"):
        compute_hit_linkage(_motif(8), bare, [(0, 100)], False, args)
    a = random_bitset_index(20, 31, length=200, n_sites=25, chrom="a")
    with pytest.raises(ValueError, match="flank"):
        compute_hit_linkage(_motif(8), a, [(0, 200)], False, args, flank=-1)
    with pytest.raises(ValueError, match="min_r2"):
        compute_hit_linkage(_motif(8), a, [(0, 200)], False, args, min_r2=1.5)
    with pytest.raises(OverflowError, match="candidate links, more than max_links = 5"):
        _quiet(compute_hit_linkage, _motif(8), a, [(0, 200)], False, args, min_r2=0.0, max_links=5)
    empty = _quiet(compute_hit_linkage, _motif(19, 1), a, [(0, 200)], False, _Args(threshold=1e-12))
    assert len(empty) == 0 and len(empty.table) == 0 and len(empty.to_frame().columns) == 18


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
    from grafimo_amd.hit_linkage import compute_hit_linkage
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
        a = _quiet(compute_hit_linkage, motif, man, None, False, args, flank=100, min_r2=0.5)
        idx = GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), "x")
        b = _quiet(compute_hit_linkage, motif, DeviceGraph(idx), read_bed_regions(bed)["chrx"], False, args, flank=100, min_r2=0.5)
        assert len(a) >= 1
        pd.testing.assert_frame_equal(a.to_frame(), b.to_frame())
        for k in ("row", "site", "allele", "entry", "distance", "n_joint", "n_allele", "n_hit", "r2", "r", "d_prime", "in_hit"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        check_linkage(b, [idx], 100, 0.5)
    finally:
        shutil.rmtree(loc, ignore_errors=True)


def test_cli_prints_and_writes_the_table_of_the_api(tmp_path):
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex, read_bed_regions
    from grafimo_amd.hit_linkage import compute_hit_linkage_many
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.workflow import Findmotif
    base = [sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "example.meme"), "-l", os.path.join(GOLD, "xy.fa"),
            "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed"), "-t", "0.05"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = str(tmp_path / "b")
    r = subprocess.run(base + ["-o", out, "--hit-linkage", "--linkage-flank", "150", "--linkage-r2", "0.5"], check=True,
                       cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    assert "hit linkage rows written to" in r.stdout
    # the same call through the library
    wf = Findmotif(threshold=0.05, cores=2)
    motifs = get_motif_pwm(os.path.join(GOLD, "example.meme"), wf, 2, False, pvalue_matrix=False)
    graphs, regs = [], []
    for chrom, rr in read_bed_regions(os.path.join(GOLD, "regions.bed")).items():
        graphs.append(DeviceGraph(GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), chrom.split("chr")[1])))
        regs.append(rr)
    tables = _quiet(compute_hit_linkage_many, motifs, graphs, regs, False, wf, flank=150, min_r2=0.5)
    assert sum(len(hl) for hl in tables) >= 1
    texts = []
    for motif, hl in zip(motifs, tables):
        check_linkage(hl, [g.index for g in graphs], 150, 0.5)
        buf = io.StringIO()
        hl.to_frame().to_csv(buf, sep="\t", index=False)
        texts.append(buf.getvalue())
        name = "grafimo_hit_linkage.tsv" if len(motifs) == 1 else f"grafimo_hit_linkage_{motif.motif_id}.tsv"
        assert open(os.path.join(out, name)).read() == buf.getvalue()
    # -f prints the table instead of writing it
    r = subprocess.run(base + ["-o", str(tmp_path / "c"), "-f", "--hit-linkage", "--linkage-flank", "150", "--linkage-r2", "0.5"],
                       check=True, cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    for text in texts:
        assert text in r.stdout
    assert not [f for f in (os.listdir(tmp_path / "c") if os.path.isdir(tmp_path / "c") else []) if "hit_linkage" in f]
