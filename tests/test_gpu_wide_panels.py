"""Every carrier-bitset kernel at cohort-size haplotype panels: the cases of tests/wide_panel_cases.py -- 1 024 .. 8 193
haplotypes over a graph of 14 sites, on both sides of every word count at which one of these kernels' loops changes shape
(16, 64 and 80 words; blocks of 4 096 haplotypes; 128 words in pair_kernel) and at the documented 5 096 -- through the
library end to end, each table against the expected side its own test file uses: the materialised rows and the fused
report against the walk enumerator of oracle/extract_oracle.py (every row's haplotype count, not a sum), the variant-effect,
hit and score tables, the two affinity tables, the hit alleles, hit pairs and hit linkage against their brute forces
(memoised on the haplotypes' alleles: tests/test_wide_panels_host.py shows the memo changes nothing, that every case reaches
the bitset routes, and that the words past each switch decide expected counts).  Every comparison is exact but for the
tolerances inside the shared checkers (p- and q-values, log2 affinities, np.corrcoef).  One DeviceGraph per case serves all
of its tests."""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_helpers import assert_table_equals_oracle, motif_as_oracle_dict, oracle_table, variants_from_index  # noqa: E402
from graph_table_checks import check_haplotype_hits, check_haplotype_scores, check_variant_effects  # noqa: E402
from graph_tables_fuzz_core import check_sums_against_report, report_cutoff  # noqa: E402
from wide_panel_cases import CASES, Args, graph, groups, motif, switch_words  # noqa: E402

pytestmark = pytest.mark.gpu
BY_H = {c[0]: c for c in CASES}
PANELS = pytest.mark.parametrize("H", sorted(BY_H))
THRESHOLD = 0.2              # a fifth of the rows: a thousand reported rows a case
SPARSE = 0.05                # for the tables that join rows: a few hundred


@pytest.fixture(scope="module")
def case():
    """H -> (GraphIndex, its DeviceGraph, W, regions, the motif); the handles are closed after the module's last test"""
    from grafimo_amd.extract_regions import DeviceGraph
    made = {}

    def get(H):
        if H not in made:
            _, seed, width, regions = BY_H[H]
            idx = graph(H, seed)
            made[H] = (idx, DeviceGraph(idx), width, list(regions), motif(width))
        return made[H]

    yield get
    for c in made.values():
        c[1].close()


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        return fn(*a, **k), out.getvalue()


@functools.lru_cache(maxsize=None)
def _enumerated(H):
    """the rows `vg find -K W -E -H` would print for the case's regions, with their haplotype counts"""
    from oracle import extract_oracle as xo
    _, seed, width, regions = BY_H[H]
    idx = graph(H, seed)
    ref, v = idx.ref.tobytes(), variants_from_index(idx)
    rows = []
    for S, E in regions:
        rows += xo.enumerate_region_variants(idx.chrom, ref, v, S, E, width, with_counts=True)
    return rows


# ---- 1. the materialised rows

@PANELS
def test_materialised_rows_equal_the_enumerator(case, H, monkeypatch):
    """k-mers, coordinates, flags and every row's haplotype count, with the job pools as they are (graph_count_jobs_kernel
    counts the deferred walks) and without room for deletion jobs (count_by_bitsets counts them in place)"""
    idx, g, width, regions, _ = case(H)
    exp = _enumerated(H)
    for pool in ("", "0"):
        if pool:
            monkeypatch.setenv("GRAFIMO_EXTRACT_DEL_POOL", pool)
        rows = g.extract(regions, width)
        strand = [chr(c) for c in rows.strand.cpu().numpy()]
        got = list(zip([k.tobytes().decode() for k in rows.kmers.cpu().numpy()],
                       [f"{idx.chrom}:{a}{s}" for a, s in zip(rows.start.cpu().numpy(), strand)],
                       [f"{idx.chrom}:{a}{s}" for a, s in zip(rows.stop.cpu().numpy(), strand)],
                       rows.freq.cpu().numpy().tolist(), ["ref" if x else "non.ref" for x in rows.is_ref.cpu().numpy()]))
        assert len(got) == len(exp)
        wrong = [(i, a, b) for i, (a, b) in enumerate(zip(got, (r[1:6] for r in exp))) if a != b]
        assert not wrong, (pool, len(wrong), wrong[:5])
    freq = np.array([r[4] for r in exp])
    assert len(exp) > 4000 and (freq > 64 * switch_words(H)).sum() > 36 and ((freq > 0) & (freq < H)).sum() > 1000


# ---- 2. the fused report

@PANELS
def test_fused_report_equals_the_oracle_table(case, H, tmp_path):
    """every reported row with its haplotype_frequency, without and with --recomb"""
    from grafimo_amd.extract_regions import compute_results_from_graph
    from grafimo_amd.workflow import Findmotif
    idx, g, width, regions, m = case(H)
    ref, v = idx.ref.tobytes(), variants_from_index(idx)
    for i, kw in enumerate((dict(threshold=THRESHOLD), dict(threshold=THRESHOLD, recomb=True))):
        exp, scanned = oracle_table(tmp_path / "oracle", idx.chrom, ref, v, regions, m, reuse_rows=i > 0, **kw)
        df, out = _quiet(compute_results_from_graph, m, g, regions, True, Findmotif(**kw))
        assert f"Scanned sequences:\t{scanned}" in out, kw
        assert_table_equals_oracle(df, exp, (H, kw))
        freq = exp["haplotype_frequency"].to_numpy()
        assert len(exp) > 500 and (freq > 64 * switch_words(H)).sum() >= 12 and ((freq > 0) & (freq < H)).sum() > 100
        assert ("recomb" in kw) == bool((freq == 0).any())


# ---- 3. the three older tables

@PANELS
def test_variant_effects(case, H):
    from grafimo_amd.variant_effects import compute_variant_effects
    idx, g, _, regions, m = case(H)
    args = Args(threshold=THRESHOLD)
    ve = compute_variant_effects(m, g, regions, False, args, all_sites=True)
    exp = check_variant_effects(ve, idx, regions, m, args, True, name=idx.chrom, memo=True)
    assert len(exp) >= 12 and sum(1 for r, x, _ in exp.values() if r is not None and x is not None) >= 6


@PANELS
def test_haplotype_hits(case, H):
    from grafimo_amd.haplotype_hits import compute_haplotype_hits
    idx, g, _, regions, m = case(H)
    args = Args(threshold=THRESHOLD)
    hh = compute_haplotype_hits(m, g, regions, False, args)
    counts = check_haplotype_hits(hh, idx, regions, m, args, memo=True)
    check_sums_against_report(hh, report_cutoff(m, g, regions, args)[1])
    assert counts.shape == (len(regions), H) and (counts.sum(axis=1) > 0).all()
    assert sum(len(np.unique(c)) > 1 for c in counts) >= 3


@PANELS
def test_haplotype_scores_with_the_default_blocks_and_blocks_of_64(case, H):
    from grafimo_amd.haplotype_scores import compute_haplotype_scores
    from haplotype_score_bruteforce import haplotype_score_keys
    idx, g, width, regions, m = case(H)
    od = motif_as_oracle_dict(m)
    exp = haplotype_score_keys(idx, regions, width, od["score_matrix"], od["min_val"], memo=True)
    for split in (dict(), dict(haplotypes_per_block=64)):
        hs = compute_haplotype_scores(m, g, regions, False, Args(), **split)
        best = check_haplotype_scores(hs, idx, regions, m, False, exp=exp)
        assert best.shape == (len(regions), H + 1) and (best >= 0).all()
        assert sum(len(np.unique(b[:H])) > 1 for b in best) >= 2


# ---- 4. the two affinity tables

@PANELS
@pytest.mark.parametrize("no_reverse", [False, True])
def test_haplotype_affinity_with_the_default_blocks_and_blocks_of_64(case, H, no_reverse):
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity
    from test_gpu_haplotype_affinity import _check
    idx, g, _, regions, m = case(H)
    args = Args(no_reverse=no_reverse)
    exp = _check(compute_haplotype_affinity(m, g, regions, False, args), idx, regions, m, no_reverse, memo=True)
    _check(compute_haplotype_affinity(m, g, regions, False, args, haplotypes_per_block=64), idx, regions, m, no_reverse, exp=exp)
    assert (exp > 0).all() and sum(len(np.unique(e[:H])) > 1 for e in exp) >= 3


@PANELS
@pytest.mark.parametrize("no_reverse", [False, True])
def test_variant_affinity_with_the_default_staging_table_and_one_entry(case, H, no_reverse):
    from grafimo_amd.variant_affinity import compute_variant_affinity
    from test_gpu_variant_affinity import _arrays, _check
    idx, g, _, regions, m = case(H)
    args = Args(no_reverse=no_reverse)
    exp = _check(compute_variant_affinity(m, g, regions, False, args), idx, regions, m, no_reverse, memo=True)
    assert _arrays(compute_variant_affinity(m, g, regions, False, args, table_entries=1)) == exp
    assert len(exp) >= 12 and sum(1 for e in exp if e[4] and e[5]) >= 6


# ---- 5. the hit alleles

@PANELS
def test_hit_alleles_with_carriers_and_groups(case, H):
    from grafimo_amd.hit_alleles import compute_hit_alleles
    from hit_allele_bruteforce import check_table
    idx, g, _, regions, m = case(H)
    args = Args(threshold=THRESHOLD)
    who = groups(H)
    assert who["past"] and min(who["past"]) == 64 * switch_words(H)
    ha = _quiet(compute_hit_alleles, m, g, regions, False, args, carriers=True, haplotype_groups=who)[0]
    rows, keys = check_table(ha, idx, regions, m, args, who, memo=True)      # (check_first_principles is its first step)
    names = list(who)
    freq = ha.report["haplotype_frequency"].to_numpy()
    assert rows > 500 and keys > 300 and (freq > 64 * switch_words(H)).sum() >= 12
    assert np.array_equal(ha.group_counts[:, names.index("all")], freq) and not ha.group_counts[:, names.index("none")].any()
    past = ha.group_counts[:, names.index("past")]
    assert (past > 0).sum() >= 12 and (past < freq).sum() >= 12


# ---- 6. hit pairs and hit linkage

@PANELS
def test_hit_pairs(case, H):
    from grafimo_amd.hit_pairs import compute_hit_pairs
    from hit_pair_bruteforce import check_pairs
    idx, g, _, regions, m = case(H)
    args = Args(threshold=SPARSE)
    who = groups(H)
    hp = _quiet(compute_hit_pairs, [m], g, regions, False, args, haplotype_groups=who, min_gap=0, max_gap=30)[0]
    assert check_pairs(hp, [(idx, regions)], [m], args, 0, 30, who, memo=True) > 100
    assert (hp.co_haplotypes > 64 * switch_words(H)).any() and (hp.group_counts[:, list(who).index("past")] > 0).sum() >= 12


@PANELS
def test_hit_linkage_with_a_flank_that_reaches_every_site(case, H):
    from grafimo_amd.hit_linkage import compute_hit_linkage
    from hit_linkage_bruteforce import check_linkage
    idx, g, _, regions, m = case(H)
    flank = len(idx.ref)
    hl = _quiet(compute_hit_linkage, m, g, regions, False, Args(threshold=SPARSE), flank=flank, min_r2=0.02)[0]
    L = check_linkage(hl, [idx], flank, 0.02)
    assert L > 100 and hl.in_hit.any() and (~hl.in_hit).any() and (hl.distance > 0).any()
