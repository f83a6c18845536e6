"""A bounded fuzz of the hit-pair table: the graphs, regions and motif sets of the graph-table fuzz
(tests/graph_tables_fuzz_core.py), random flags and gaps, the table against tests/hit_pair_bruteforce.check_pairs."""
import contextlib
import io
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from graph_tables_fuzz_core import Args, make_graph, make_motifs, make_regions  # noqa: E402
from hit_pair_bruteforce import check_pairs  # noqa: E402

pytestmark = pytest.mark.gpu


def _fuzz_seed(seed, tmp, rows_bound=3_000):
    from grafimo_amd import hit_pairs as hpm
    from grafimo_amd.extract_regions import DeviceGraph
    rng = np.random.default_rng(110_000 + seed)
    d = os.path.join(str(tmp), f"g{seed}")
    os.makedirs(d)
    idx, what = make_graph(seed, rng, d)
    regions = make_regions(rng, idx)
    motifs = make_motifs(rng, idx, regions, rows_bound)
    H = int(idx.n_haplotypes)
    qt = bool(rng.random() < 0.25)
    args = Args(threshold=0.9 if qt else float(rng.choice([0.3, 0.05, 1e-2])), noreverse=bool(rng.random() < 0.25),
                recomb=bool(rng.random() < 0.4), qvalueT=qt, noqvalue=not qt)
    lo = int(rng.choice([0, 0, -3, -64, 5]))
    gap = (lo, lo + int(rng.choice([0, 10, 50, 200])))
    perm = rng.permutation(H)
    groups = {"a": sorted(perm[:H // 2].tolist()), "b": sorted(perm[H // 3:].tolist()), "none": [], "all": list(range(H))}
    ctx = (seed, what, regions, [m.width for m in motifs], vars(args), gap)
    g = DeviceGraph(idx)
    try:
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                hp = hpm.compute_hit_pairs(motifs, g, regions, False, args, haplotype_groups=groups, min_gap=gap[0], max_gap=gap[1])
        except SystemExit:             # (a report without rows ends the command line, as the reference: no pair)
            return 0
        pairs = check_pairs(hp, [(idx, regions)], motifs, args, gap[0], gap[1], groups)
        assert np.array_equal(hp.group_counts[:, 3], hp.co_haplotypes)
    except AssertionError as e:
        raise AssertionError(f"hit-pair fuzz seed {seed}: {ctx}") from e
    finally:
        g.close()
        shutil.rmtree(d, ignore_errors=True)
    return pairs


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_seed(tmp_path, seed):
    assert _fuzz_seed(seed, tmp_path) >= 0


def test_the_seeds_reach_pairs():
    """(the bounded set is not vacuous: seeds whose tables have pairs are among it)"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert sum(_fuzz_seed(seed, tmp) for seed in (8, 9, 10)) > 0
