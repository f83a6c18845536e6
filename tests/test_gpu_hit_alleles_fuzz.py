"""A bounded fuzz of the per-hit allele table: the graphs, regions and motif sets of the graph-table fuzz
(tests/graph_tables_fuzz_core.py), random flags and work-split knobs, every motif's table against the haplotype brute force,
the walk enumerator and first principles (tests/hit_allele_bruteforce.py: its checks 2, 3 and 4)."""
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
from hit_allele_bruteforce import check_table  # noqa: E402

pytestmark = pytest.mark.gpu


def _fuzz_seed(seed, tmp, rows_bound=8_000):
    from grafimo_amd import hit_alleles as hal
    from grafimo_amd.extract_regions import DeviceGraph
    rng = np.random.default_rng(90_000 + seed)
    d = os.path.join(str(tmp), f"g{seed}")
    os.makedirs(d)
    idx, what = make_graph(seed, rng, d)
    regions = make_regions(rng, idx)
    motifs = make_motifs(rng, idx, regions, rows_bound)
    H = int(idx.n_haplotypes)
    qt = bool(rng.random() < 0.25)
    args = Args(threshold=0.9 if qt else float(rng.choice([1.0, 0.3, 0.05, 1e-2])), noreverse=bool(rng.random() < 0.25),
                recomb=bool(rng.random() < 0.4), qvalueT=qt, noqvalue=not qt)
    perm = rng.permutation(H)
    groups = {"a": sorted(perm[:H // 2].tolist()), "b": sorted(perm[H // 3:].tolist()), "none": [], "all": list(range(H))}
    scratch = int(rng.choice([0, 1, 2, 5])) * 4 * (96 + 2)
    first_room = int(rng.choice([8, 8, 0, 1]))
    ctx = (seed, what, regions, [m.width for m in motifs], vars(args), scratch, first_room)
    g = DeviceGraph(idx)
    old = hal._FIRST_ALLELES_PER_ENTRY
    hal._FIRST_ALLELES_PER_ENTRY = first_room
    rows = 0
    try:
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                tables = hal.compute_hit_alleles_many(motifs, g, regions, False, args, carriers=True, haplotype_groups=groups,
                                                      scratch_bytes=scratch)
        except SystemExit:             # (regions without a single window: the report ends the command line, as the reference)
            return 0
        for m, ha in zip(motifs, tables):
            rows += check_table(ha, idx, regions, m, args, groups)[0]
            assert np.array_equal(ha.group_counts[:, 3], ha.report["haplotype_frequency"].to_numpy())
    except AssertionError as e:
        raise AssertionError(f"hit-allele fuzz seed {seed}: {ctx}") from e
    finally:
        hal._FIRST_ALLELES_PER_ENTRY = old
        g.close()
        shutil.rmtree(d, ignore_errors=True)
    return rows


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_seed(tmp_path, seed):
    assert _fuzz_seed(seed, tmp_path) >= 0


def test_the_seeds_reach_rows():
    """(the bounded set is not vacuous: seeds whose tables have rows are among it)"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        assert sum(_fuzz_seed(seed, tmp) for seed in (8, 9)) > 0
