"""A few fixed seeds of the per-variant affinity table on random small graphs against the brute force
(tests/variant_affinity_bruteforce.py): VCF graphs of a random allele mix (length 200 .. 400, 6 .. 20 samples), a random width in
4 .. 40, random regions (graph_tables_fuzz_core.make_regions: overlapping, repeated, below 0, past the end, empty, on sites,
inside deletions, at insertion anchors), a random strand flag, temperature and staging-table size.  The four arrays are equal
as integers.  One loop in this process, every seed once."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_fuzz_core import KINDS, SynMotif  # noqa: E402
from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict  # noqa: E402
from graph_tables_fuzz_core import Args, make_regions  # noqa: E402
from variant_affinity_bruteforce import expected_rows, variant_affinity_sums  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = [0, 1, 2, 3, 4, 5, 6, 7]


def test_fuzz_seeds(tmp_path):
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.variant_affinity import compute_variant_affinity
    rows_seen = 0
    for seed in SEEDS:
        rng = np.random.default_rng(93_000 + seed)
        d = tmp_path / f"s{seed}"
        d.mkdir()
        kinds = KINDS[int(rng.integers(0, len(KINDS)))]
        fa, vcf = make_consistent_graph_files(str(d), length=int(rng.integers(200, 401)), n_samples=int(rng.integers(6, 21)),
                                              seed=700 + seed, kinds=kinds, dense=bool(rng.random() < 0.5))
        with contextlib.redirect_stderr(io.StringIO()):      # (S: symbolic ALTs are reported and left out)
            idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
        regions = make_regions(rng, idx)
        W = int(rng.integers(4, 41))
        motif = SynMotif(W, seed=int(rng.integers(0, 1 << 20)))
        motif.motif_id, motif.motif_name = f"F{seed}", f"f{seed}"
        fwd = bool(rng.random() < 0.3)
        T = float(rng.choice([1.0, 0.5, 3.0]))
        entries = int(rng.choice([0, 1, 2, 8, 64]))
        ctx = (seed, kinds, regions, W, fwd, T, entries)
        od = motif_as_oracle_dict(motif)
        w, _ = default_weights(motif, T)
        exp = expected_rows(idx, *variant_affinity_sums(idx, regions, W, od["score_matrix"], od["min_val"], w, forward_only=fwd,
                                                        memo=True))
        g = DeviceGraph(idx)
        try:
            for k in range(2):                               # (again on the same handle: the window buffer is reused)
                va = compute_variant_affinity(motif, g, regions, False, Args(noreverse=fwd), temperature=T,
                                              table_entries=entries if k == 0 else 0)
                got = [tuple(int(x) for x in r) for r in zip(va.site, va.allele, va.ref_sum, va.alt_sum, va.ref_rows, va.alt_rows)]
                assert got == exp, (ctx, k, [(a, b) for a, b in zip(got, exp) if a != b][:5], len(got), len(exp))
        finally:
            g.close()
        rows_seen += len(exp)
    assert rows_seen > 10 * len(SEEDS)                   # (the seeds have rows to compare)
