"""What makes a pass of tests/test_gpu_wide_panels.py mean something, checked on the CPU from the index and the oracle alone
(no kernel runs here).  For every case of tests/wide_panel_cases.py:

  * the bitset routes are reached: windows of four or more substitution sites that touch no indel (graph_count_kernel
    leaves exactly these to graph_count_jobs_kernel: ns > 3), and indel windows with walks whose constraints are not two or
    three neighbouring sites (the deletion kernel's jobs, or its in-place count_by_bitsets) -- some dozen expected rows each;
  * a kernel that ignored the words past its switch would fail: on the same graph cut to the first S x 64 haplotypes the
    enumerator's counts differ in at least 20 of those rows, and the haplotype-affinity sums and the hit-allele carrier
    counts are not constant over the haplotypes beyond S x 64;
  * the memoised brute forces the GPU file trusts at these sizes equal the unmemoised ones at 130 haplotypes.

The routes are told apart by the walk enumerator of tests/variant_walks.py (a walk's constraint set), whose rows and counts
are first shown to be extract_oracle.enumerate_region_variants' rows and counts, for the full and for the cut panel."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_helpers import motif_as_oracle_dict, variants_from_index  # noqa: E402
from graph_table_checks import random_bitset_index  # noqa: E402
from variant_walks import _carriers, window_walks  # noqa: E402
from wide_panel_cases import CASES, Args, graph, motif, switch_words, truncated  # noqa: E402

MIN_ROUTE_ROWS = 36          # "some dozen": three dozen expected rows on each route
MIN_CHANGED_ROWS = 20
THRESHOLD = 0.2              # the GPU file's report threshold


def route_rows(idx, regions, width, cut):
    """every walk of every window of every region, from the walk enumerator -> [(region label, start, stop, k-mer, haplotypes
    that carry it, those among the first `cut`, route)], route = "plain" (a window without an indel, four or more sites),
    "indel" (a window that touches an indel; the walk's constraints are no single site, pair of neighbours or triple of
    consecutive sites) or None (the count comes from the popcount / pair / triple tables)"""
    L, H = len(idx.ref), int(idx.n_haplotypes)
    is_indel = (np.asarray(idx.del_len) > 0) | (np.asarray(idx.ins_len) > 0)
    tail = 1 if (np.asarray(idx.ins_len) > 0).any() else width
    car = {}
    out = []
    for S, E in regions:
        s, e = max(S, 0), min(E, L)
        for p in range(s, e - tail + 1):
            walks = window_walks(idx, p, width, e)
            touches = any(is_indel[sl >> 2] for _, _, slots in walks for sl in slots)
            for kmer, stop, slots in walks:
                acc = np.ones(H, bool)
                for sl in slots:
                    if sl not in car:
                        car[sl] = _carriers(idx, sl >> 2, sl & 3)
                    acc &= car[sl]
                sites = sorted({sl >> 2 for sl in slots})
                n = len(sites)
                assert n == len(slots)
                if not touches:
                    route = "plain" if n >= 4 else None
                else:
                    by_table = n <= 1 or (n <= 3 and sites[-1] - sites[0] == n - 1)
                    route = None if by_table else "indel"
                out.append((f"{idx.chrom}:{S}-{E}", p, stop, kmer.decode(), int(acc.sum()), int(acc[:cut].sum()), route))
    return out


def enumerator_rows(idx, regions, width):
    """the '+' rows of extract_oracle.enumerate_region_variants with their counts, sorted"""
    from oracle import extract_oracle as xo
    ref, v = idx.ref.tobytes(), variants_from_index(idx)
    rows = []
    for S, E in regions:
        for label, kmer, start, stop, count, _ in xo.enumerate_region_variants(idx.chrom, ref, v, S, E, width, with_counts=True):
            if start.endswith("+"):
                rows.append((label, int(start.split(":")[1][:-1]), int(stop.split(":")[1][:-1]), kmer, count))
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def conditions(H, seed, width, regions):
    """-> the figures of one case: rows (both strands) on each route, and those whose count the cut panel changes"""
    idx = graph(H, seed)
    cut = 64 * switch_words(H)
    walks = route_rows(idx, regions, width, cut)
    assert sorted(w[:5] for w in walks) == enumerator_rows(idx, regions, width)
    assert sorted(w[:4] + (w[5],) for w in walks) == enumerator_rows(truncated(idx, cut), regions, width)
    fig = {}
    for route in ("plain", "indel"):
        mine = [w for w in walks if w[6] == route]
        fig[route] = 2 * len(mine)
        fig[route + "_changed"] = 2 * sum(1 for w in mine if w[4] != w[5])
        fig[route + "_past_switch"] = 2 * sum(1 for w in mine if w[4] > cut)
    fig["rows"] = 2 * len(walks)
    fig["above_4096"] = 2 * sum(1 for w in walks if w[4] > 4096)
    return fig


@pytest.mark.parametrize("H,seed,width,regions", CASES, ids=[f"H{c[0]}" for c in CASES])
def test_the_bitset_routes_are_reached_and_the_words_past_the_switch_decide_counts(H, seed, width, regions):
    idx = graph(H, seed)
    assert idx.hw == (H + 63) // 64 and (np.asarray(idx.del_len) > 0).any() and (np.asarray(idx.ins_len) > 0).any()
    L = len(idx.ref)
    assert regions[0] == (0, L) and any(S < 0 or E > L for S, E in regions) and any(0 < E - S < 60 for S, E in regions)
    fig = conditions(H, seed, width, tuple(regions))
    print(f"H {H} (hw {idx.hw}, cut at {switch_words(H)} words): {fig}")
    assert fig["plain"] >= MIN_ROUTE_ROWS and fig["indel"] >= MIN_ROUTE_ROWS, fig
    assert fig["plain_changed"] + fig["indel_changed"] >= MIN_CHANGED_ROWS, fig
    assert fig["plain_changed"] > 0 and fig["indel_changed"] > 0, fig


def _varies_beyond(block, reference=None):
    """`block` [rows, haplotypes beyond the cut]: not constant across the haplotypes in three rows or more; a block of one
    haplotype: not the same in every row, and not the reference path's column"""
    if block.shape[1] > 1:
        return sum(len(np.unique(b)) > 1 for b in block) >= 3
    return len(np.unique(block[:, 0])) > 1 and (reference is None or (block[:, 0] != reference).any())


@pytest.mark.parametrize("H,seed,width,regions", CASES, ids=[f"H{c[0]}" for c in CASES])
def test_affinity_sums_and_carrier_counts_vary_beyond_the_switch(H, seed, width, regions):
    from grafimo_amd.haplotype_affinity import default_weights
    from haplotype_affinity_bruteforce import haplotype_affinity_sums
    from hit_allele_bruteforce import carrier_counts, report_cutoff
    idx = graph(H, seed)
    cut = 64 * switch_words(H)
    m = motif(width)
    od = motif_as_oracle_dict(m)
    sums = haplotype_affinity_sums(idx, regions, width, od["score_matrix"], od["min_val"], default_weights(m, 1.0)[0], memo=True)
    assert _varies_beyond(sums[:, cut:H], sums[:, H])
    cutoff = report_cutoff(m, Args(threshold=THRESHOLD))
    counts = carrier_counts(idx, regions, width, od["score_matrix"], od["min_val"], cutoff, memo=True)
    block = np.array([v[cut:] for v in counts.values()])
    assert len(block) > 24 and (block.sum(axis=1) > 0).sum() >= 3 and _varies_beyond(block)


def test_the_memoised_brute_forces_equal_the_unmemoised_ones():
    """130 haplotypes over the generator's 14 sites: far fewer classes than haplotypes, so the memo does skip work"""
    from grafimo_amd.haplotype_affinity import default_weights
    from haplotype_affinity_bruteforce import haplotype_affinity_sums
    from haplotype_bruteforce import haplotype_matrix
    from haplotype_score_bruteforce import haplotype_score_keys
    from hit_allele_bruteforce import carrier_counts, report_cutoff
    from hit_pair_bruteforce import haplotype_pairs
    from variant_affinity_bruteforce import variant_affinity_sums
    from variant_bruteforce import best_hits, haplotype_classes
    idx = random_bitset_index(130, 1030, length=200, n_sites=14)
    assert 1 < len(haplotype_classes(idx)[0]) < 130
    regions = [(0, 200), (20, 90), (-5, 40), (150, 260)]
    m = motif(8, 1)
    od = motif_as_oracle_dict(m)
    base = (idx, regions, 8, od["score_matrix"], od["min_val"])
    cutoff = report_cutoff(m, Args(threshold=THRESHOLD))
    weights = default_weights(m, 1.0)[0]
    for fwd in (False, True):
        a, b = (carrier_counts(*base, cutoff, forward_only=fwd, memo=memo) for memo in (False, True))
        assert len(a) > 20 and a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) and b[k].dtype == np.int64 for k in a)
        a, b = (haplotype_pairs([(idx, regions)], [m], [cutoff], -3, 40, forward_only=fwd, memo=memo) for memo in (False, True))
        assert len(a) > 20 and a == b
        a, b = (haplotype_affinity_sums(*base, weights, forward_only=fwd, memo=memo) for memo in (False, True))
        assert (a == b).all() and len(np.unique(a[0])) > 1
        a, b = (variant_affinity_sums(*base, weights, forward_only=fwd, memo=memo) for memo in (False, True))
        assert a == b and len(a[0]) > 10
        a, b = (haplotype_matrix(*base, cutoff, forward_only=fwd, memo=memo) for memo in (False, True))
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[0].sum() > 0
        a, b = (haplotype_score_keys(*base, forward_only=fwd, memo=memo) for memo in (False, True))
        assert (a == b).all()
        assert best_hits(*base, forward_only=fwd, memo=False) == best_hits(*base, forward_only=fwd, memo=True)
