"""Development aid (GPU box): the per-variant effect table, the per-haplotype hit matrix and the per-haplotype best score
matrix of random motif sets on random graphs against their brute forces, seed after seed for a fixed time.  One seed =
tests/graph_tables_fuzz_core.py (`pytest -m gpu` runs a bounded seed set of it).
TEST INFRASTRUCTURE (imports oracle/): not part of the product.
    python scripts/graph_tables_fuzz.py [seconds] [first_seed]"""
import os
import sys
import tempfile
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))

from graph_tables_fuzz_core import fuzz_seed  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
t0 = time.time()
stats = dict(seeds=0, tables=0, cells=0, variant_rows=0)
with tempfile.TemporaryDirectory() as tmp:
    shown = t0
    while time.time() - t0 < budget:
        fuzz_seed(seed, tmp, stats)
        seed += 1
        if time.time() - shown > 60:                     # (a sign of life per minute on long runs)
            shown = time.time()
            print(f"  {shown - t0:.0f} s: {stats['seeds']} seeds, next {seed}", file=sys.stderr, flush=True)
print(f"graph_tables_fuzz: {stats['seeds']} seeds, {stats['tables']} tables ({stats['cells']} matrix cells and "
      f"{stats['variant_rows']} variant rows compared) in {time.time() - t0:.0f} s: the three tables == their brute forces; "
      f"next seed {seed}")
