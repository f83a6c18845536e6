"""A few fixed seeds of the per-haplotype affinity matrix on random small graphs against the sum brute force
(tests/haplotype_affinity_bruteforce.py): VCF graphs of every variant kind (length <= 300, <= 16 samples), a random width in
4 .. 24, random regions (graph_tables_fuzz_core.make_regions: overlapping, repeated, below 0, past the end, empty, on sites,
inside deletions, at insertion anchors), a random strand flag, temperature and work split.  The sums are equal as integers."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict  # noqa: E402
from graph_tables_fuzz_core import Args, make_regions  # noqa: E402
from haplotype_affinity_bruteforce import haplotype_affinity_sums  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_fuzz_seed(tmp_path, seed):
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity, default_weights
    rng = np.random.default_rng(91_000 + seed)
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=int(rng.integers(120, 301)), n_samples=int(rng.integers(1, 17)),
                                          seed=500 + seed, kinds="sidmDOcS", dense=bool(rng.random() < 0.5))
    with contextlib.redirect_stderr(io.StringIO()):      # (S: symbolic ALTs are reported and left out)
        idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = make_regions(rng, idx)
    W = int(rng.integers(4, 25))
    motif = SynMotif(W, seed=int(rng.integers(0, 1 << 20)))
    motif.motif_id, motif.motif_name = f"F{seed}", f"f{seed}"
    fwd = bool(rng.random() < 0.3)
    T = float(rng.choice([1.0, 0.5, 3.0]))
    wpr, hpb = int(rng.choice([0, 1, 3, 7, 64, 1024])), int(rng.choice([0, 64, 128, 4096]))
    ctx = (seed, regions, W, fwd, T, wpr, hpb)
    od = motif_as_oracle_dict(motif)
    w, _ = default_weights(motif, T)
    exp = haplotype_affinity_sums(idx, regions, W, od["score_matrix"], od["min_val"], w, forward_only=fwd, memo=True)
    g = DeviceGraph(idx)
    try:
        for k in range(2):                               # (again on the same handle: the run buffer is reused)
            ha = compute_haplotype_affinity(motif, g, regions, False, Args(noreverse=fwd), temperature=T,
                                            windows_per_run=wpr if k == 0 else 0, haplotypes_per_block=hpb if k == 0 else 0)
            assert (ha.full == exp).all(), (ctx, k, np.argwhere(ha.full != exp)[:5])
    finally:
        g.close()
