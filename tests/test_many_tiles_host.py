"""tests/many_tiles_cases.py without a GPU: its caps are the library's (read from the headers: a changed cap fails here and does
not quietly take tests/test_gpu_scan_many_tiles.py back to one turn a workgroup), its layout at the real caps exceeds them,
holds every succession coverage() asks for and stays small, and its gather equals the brute force run over a whole call."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deletion_scan_bruteforce as dbf  # noqa: E402
import many_tiles_cases as mt  # noqa: E402
import mutation_scan_bruteforce as mbf  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

CSRC = os.path.join(ROOT, "grafimo_amd", "csrc")
T = 64                                                           # every scan's tile (grafimo_amd/_native.py: GFM_*_TILE)


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _value(text):
    """`4096` or `1 << 16`"""
    m = re.fullmatch(r"\s*(\d+)\s*(?:<<\s*(\d+))?\s*", text)
    assert m, text
    return int(m.group(1)) << int(m.group(2) or 0)


def test_the_caps_are_the_codes():
    from grafimo_amd import _native as nv
    assert {nv.GFM_MUTSCAN_TILE, nv.GFM_INDELSCAN_TILE, nv.GFM_DELSCAN_TILE, nv.GFM_SUBSCAN_TILE, nv.GFM_INSSCAN_TILE,
            nv.GFM_SITEDIST_TILE} == {T}
    tiles = _source("gfm_sequence_tiles.hpp")
    (seq,) = re.findall(r"^constexpr int kSeqMaxBlocks = ([^;]+);", tiles, flags=re.M)
    assert _value(seq) == mt.CAPS["seq"]
    assert "std::min<size_t>(tiles.size(), (size_t)kSeqMaxBlocks)" in tiles      # (the one grid every entry is handed)
    ins_text = _source("gfm_graph_insertion_scan.hpp")
    (ins,) = re.findall(r"^constexpr unsigned kInsMaxBlocks = ([^;]+);", ins_text, flags=re.M)
    assert _value(ins) == mt.CAPS["insertion"] < mt.CAPS["seq"]
    assert "dim3(std::min(blocks, kInsMaxBlocks), (unsigned)mm)" in ins_text
    qv = _source("gfm_graph_query_variants.hpp")
    (threads, per_wave) = re.findall(r"^constexpr int kQvThreads = (\d+), kQvWaves = kQvThreads / (\d+);", qv, flags=re.M)[0]
    (blocks,) = re.findall(r"std::min<long long>\(\(n_items \+ kQvWaves - 1\) / kQvWaves, ([^)]+)\);", qv)
    assert int(per_wave) == 64 and int(threads) // int(per_wave) == 4
    assert _value(blocks) * (int(threads) // int(per_wave)) == mt.CAPS["query_items"]
    assert "it += (long long)gridDim.x * kQvWaves" in qv


@pytest.mark.parametrize("turns,cap", [(2, "seq"), (2, "insertion"), (3, "insertion")])
@pytest.mark.parametrize("W", [1, 2, 19, 64])
def test_layout_at_the_real_caps(W, cap, turns):
    cap = mt.CAPS[cap]
    pool = mt.pool(W, T, np.random.default_rng(7_000 + W))
    assert len(set(pool)) == len(pool) and {len(x) for x in pool} >= set(mt.sizes(W, T)) | {70}
    assert {b"A", b"c", b"N", b"GT", b"N" * 70} <= set(pool)
    call, pairs = mt.layout(pool, T, cap, turns=turns)
    off, bases = mt.call_arrays(pool, call)
    per_copy = sum((len(x) + T - 1) // T for x in pool)
    assert mt.tile_count(off, T) == (turns - 1) * cap + 4 * per_copy > (turns - 1) * cap
    assert len(pairs) == mt.tile_count(off, T) - cap
    mt.coverage(pairs, pool, W, T)
    assert len(bases) < 100_000
    # the tail's first tile is tile number cap exactly: the first base of a later turn begins a copy of the pool
    later = mt.later_turn_bases(off, T, cap)
    first = int(np.flatnonzero(later)[0])
    assert first in off.tolist() and int(later.sum()) == len(bases) - first
    at = off.tolist().index(first)
    assert sorted(call[at:at + len(pool)]) == list(range(len(pool))) and call[at:at + len(pool)] != list(range(len(pool)))
    if turns == 2:
        assert int(later.sum()) == 4 * sum(len(x) for x in pool)


def test_the_gather_is_the_brute_force_over_the_whole_call():
    """cap = 8, W = 5: a call small enough to run the deletion and the mutation brute force over all of it"""
    W, cap = 5, 8
    rng = np.random.default_rng(7_100)
    whole = mt.pool(W, T, rng)
    pool = [next(x for x in whole if len(x) == n) for n in (1, 2, 6, 65, 70)]    # 7 tiles
    call, pairs = mt.layout(pool, T, cap, rotations=1)
    assert len(call) == 11 and call[:5] == [0, 1, 2, 3, 4] and call[5] in (0, 1) and sorted(call[6:]) == [0, 1, 2, 3, 4]
    assert len(pairs) == 7 and pairs[0][0] == (0, 0) and pairs[-1][0] == (4, 64)
    off, bases = mt.call_arrays(pool, call)
    assert mt.tile_count(off, T) == 15 and bases.tobytes() == b"".join(pool[i] for i in call)
    seqs = [pool[i] for i in call]
    od = motif_as_oracle_dict(SynMotif(W, seed=71))
    weights = rng.integers(1 << 40, 1 << 55, size=1000 * W + 1, dtype=np.uint64)
    for bf, extra, axis in ((dbf, ((1, 2, 7, 64),), 1), (mbf, (), 0)):
        full = bf.scan_arrays(seqs, W, od["score_matrix"], od["min_val"], weights, False, *extra)
        part = bf.scan_arrays(pool, W, od["score_matrix"], od["min_val"], weights, False, *extra)
        for f, p, dt in zip(full, part, (np.uint32, np.uint64)):
            got = mt.gather(np.array(p, dtype=dt), pool, call, axis)
            assert got.dtype == dt and got.tolist() == f
            assert got.any() and len({row.tobytes() for row in np.moveaxis(got, axis, 0)}) > 4 * len(pool)   # (rows that differ)
        assert max(int(v) for v in np.array(full[1], dtype=np.uint64).ravel()) > 1 << 53
