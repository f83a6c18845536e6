"""The three graph tables -- per-variant effects, the per-haplotype hit matrix, the per-haplotype best scores -- against their
brute forces: a bounded seed set of the graph-table fuzz (tests/graph_tables_fuzz_core.py), and the edges one seed rarely
reaches: haplotype counts around the bitset word, haplotype blocks and runs, more than 4 096 haplotypes, a window of exactly
2^24 walks, the key-field guards at their largest accepted input and one past it, and the variant table's record retry."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict  # noqa: E402
from graph_table_checks import (check_haplotype_hits, check_haplotype_scores, check_variant_effects,  # noqa: E402
                                random_bitset_index)
from graph_tables_fuzz_core import Args, check_sums_against_report, fuzz_seed, report_cutoff  # noqa: E402
from variant_bruteforce import int_score, revcomp  # noqa: E402

pytestmark = pytest.mark.gpu


def _motif(W, seed=0):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(6100 + 17 * W + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


def _all_three(g, idx, regions, motif, threshold=0.05, no_reverse=False, memo=False, **split):
    """the three features of `motif` on one handle, each against its brute force; the hit counts against the report's
    haplotype frequencies"""
    from grafimo_amd.haplotype_hits import compute_haplotype_hits
    from grafimo_amd.haplotype_scores import compute_haplotype_scores
    from grafimo_amd.variant_effects import compute_variant_effects
    args = Args(threshold=threshold, noreverse=no_reverse)
    ve = compute_variant_effects(motif, g, regions, False, args, all_sites=True)
    check_variant_effects(ve, idx, regions, motif, args, True, name=idx.chrom, memo=memo)
    hh = compute_haplotype_hits(motif, g, regions, False, args)
    counts = check_haplotype_hits(hh, idx, regions, motif, args, memo=memo)
    check_sums_against_report(hh, report_cutoff(motif, g, regions, args)[1])
    hs = compute_haplotype_scores(motif, g, regions, False, args, **split)
    best = check_haplotype_scores(hs, idx, regions, motif, no_reverse, memo=memo)
    return ve, counts, best


@pytest.mark.parametrize("seed", range(16))
def test_fuzz_seed(tmp_path, seed):
    stats = dict(seeds=0, tables=0, cells=0, variant_rows=0)
    fuzz_seed(seed, tmp_path, stats)
    assert stats["seeds"] == 1 and stats["tables"] > 0


def test_threshold_one_leaves_the_lowest_score_out():
    """(fuzz seed 29 found it) at threshold 1 a k-mer of the lowest score has p = 1 exactly in the report's normalised tail
    table and is no hit (p < t, strict).  The un-normalised tail sum gives it p = 0.99999999999999 and a cutoff of 0: the
    brute force's cutoff must come from the normalised table.  Here that k-mer is on the reference, read by every haplotype."""
    from oracle import oracle as orc
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.haplotype_hits import compute_haplotype_hits
    from haplotype_bruteforce import integer_cutoff
    from graph_table_checks import hit_matrix_expected
    W = 5
    m = _motif(W, 1)                                      # (a motif whose un-normalised total is below 1)
    od = motif_as_oracle_dict(m)
    assert integer_cutoff(np.cumsum(od["pmf"][::-1])[::-1], 1.0) == 0 < integer_cutoff(orc.p_table(od["pmf"]), 1.0)
    idx = _snv_index([1, 2, 3], at=20, length=100, seed=29)
    lowest = np.frombuffer(b"ACGT", dtype=np.uint8)[od["score_matrix"].argmin(0)]
    idx.ref[60:60 + W] = lowest
    regions = [(0, 100), (55, 70), (10, 40)]
    args = Args(threshold=1.0)
    g = DeviceGraph(idx)
    try:
        hh = compute_haplotype_hits(m, g, regions, False, args)
    finally:
        g.close()
    counts = check_haplotype_hits(hh, idx, regions, m, args)
    un_normalised = hit_matrix_expected(idx, regions, m, 1.0, False, cutoff=0)[0]
    assert (un_normalised[:2] > counts[:2]).all() and (un_normalised[2] == counts[2]).all()


@pytest.mark.parametrize("H", [1, 63, 64, 65, 127, 129])
def test_word_boundaries(H):
    """haplotype counts on both sides of a bitset word: the tail bits of the last word must not carry, count or score (in
    the three tables, and in the report's haplotype frequencies the hit counts are summed against)"""
    from grafimo_amd.extract_regions import DeviceGraph
    idx = random_bitset_index(H, 900 + H, length=260, n_sites=30)
    g = DeviceGraph(idx)
    try:
        regions = [(0, 260), (30, 140), (120, 121), (-3, 60), (200, 300)]
        ve, counts, best = _all_three(g, idx, regions, _motif(8, H), threshold=0.05)
        assert len(ve) > 0 and counts.sum() > 0 and (best[0] >= 0).all()
        _all_three(g, idx, regions[:2], _motif(5, H), threshold=0.2, no_reverse=True)
    finally:
        g.close()


@pytest.mark.parametrize("H", [129, 150])
@pytest.mark.parametrize("wpr", [1, 3])
def test_blocks_of_64(H, wpr):
    """blocks of 64 haplotypes (the last one partial) and runs of 1 and 3 windows against the brute force"""
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.haplotype_scores import compute_haplotype_scores
    idx = random_bitset_index(H, 1300 + H + wpr, length=300, n_sites=34)
    g = DeviceGraph(idx)
    try:
        # the whole chromosome, and short regions around sites: there the haplotypes' bests differ, so a wrong block shows
        regions = [(0, 300), (40, 47), (-10, 20)] + [(int(q) - 4, int(q) + 12) for q in idx.pos[::3]]
        m = _motif(9, wpr)
        hs = compute_haplotype_scores(m, g, regions, False, Args(), windows_per_run=wpr, haplotypes_per_block=64)
        best = check_haplotype_scores(hs, idx, regions, m, False)
        assert sum(len(np.unique(b[64:H])) > 1 for b in best) >= 3
    finally:
        g.close()


def test_more_than_4096_haplotypes():
    """4 161 haplotypes over a few sites: two blocks of the default launch, against the brute force (memoised on the
    haplotypes' alleles)"""
    from grafimo_amd.extract_regions import DeviceGraph
    idx = random_bitset_index(4161, 77, length=140, n_sites=7)
    g = DeviceGraph(idx)
    try:
        regions = [(0, 140), (20, 90), (60, 61)] + [(int(q) - 3, int(q) + 8) for q in idx.pos]
        ve, counts, best = _all_three(g, idx, regions, _motif(6, 2), threshold=0.05, memo=True)
        assert sum(len(np.unique(b[2112:4161])) > 1 for b in best) >= 3      # (the second block: 2 112 ..)
        assert sum(len(np.unique(c[2112:])) > 1 for c in counts) >= 3
    finally:
        g.close()


def _snv_index(n_alts, at=20, length=100, seed=0):
    """SNV sites with the given ALT counts at at, at + 1, ...; two haplotypes with a random allele each"""
    from grafimo_amd.extract_regions import GraphIndex
    rng = np.random.default_rng(seed)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)]
    pos = np.arange(at, at + len(n_alts), dtype=np.int32)
    alt = np.zeros((len(pos), 3), np.uint8)
    bits = np.zeros((len(pos), 3, 1), np.uint64)
    for i, (q, na) in enumerate(zip(pos, n_alts)):
        others = [c for c in b"ACGT" if c != ref[q]]
        alt[i, :na] = others[:na]
        for h in range(2):
            a = int(rng.integers(0, na + 1))
            if a:
                bits[i, a - 1, 0] |= np.uint64(1 << h)
    return GraphIndex("c", ref, pos, np.array(n_alts, np.uint8), alt, bits, 2)


def _smallest_product_above(limit, max_sites):
    """-> ALT counts of at most max_sites sites whose walk product prod(1 + n_alts) is the smallest above limit"""
    best = None
    for c in range(max_sites + 1):                        # c sites of 3 ALTs, b of 2, a of 1
        for b in range(max_sites + 1 - c):
            for a in range(max_sites + 1 - c - b):
                v = 4 ** c * 3 ** b * 2 ** a
                if v > limit and (best is None or v < best[0]):
                    best = (v, [3] * c + [2] * b + [1] * a)
    return best


def test_walk_limit_at_two_to_the_24():
    """one window of exactly 4^12 = 2^24 walks is accepted and equals the brute force (scores, and variant effects without
    --recomb); the smallest walk product above 2^24 is refused"""
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.haplotype_scores import compute_haplotype_scores
    from grafimo_amd.variant_effects import compute_variant_effects
    idx = _snv_index([3] * 12)
    g = DeviceGraph(idx)
    try:
        regions = [(20, 32)]                              # W = 12: the one window starting at 20 sees all 12 sites
        m = _motif(12, 1)
        hs = compute_haplotype_scores(m, g, regions, False, Args())
        assert (check_haplotype_scores(hs, idx, regions, m, False) >= 0).all()
        args = Args(threshold=1.0)
        ve = compute_variant_effects(m, g, regions, False, args, all_sites=True)
        check_variant_effects(ve, idx, regions, m, args, True)
        assert len(ve) > 0
    finally:
        g.close()
    v, n_alts = _smallest_product_above(1 << 24, 19)
    assert v == 3 ** 12 * 2 ** 5
    idx = _snv_index(n_alts)
    g = DeviceGraph(idx)
    try:
        regions = [(20, 39)]                              # W = 19: one window over all the sites
        with pytest.raises(OverflowError):
            compute_haplotype_scores(_motif(19), g, regions, False, Args())
        with pytest.raises(OverflowError):
            compute_variant_effects(_motif(19), g, regions, False, Args(threshold=1.0))
    finally:
        g.close()


def _one_deletion_index(D, W, top, anchor=100, tail=200):
    """a deletion of D bases behind `anchor`, haplotype 0 carrying it, haplotype 1 not; the 2-mer `top` across the
    junction (reference bases `anchor` and `anchor` + D + 1)"""
    from grafimo_amd.extract_regions import GraphIndex
    rng = np.random.default_rng(D)
    L = anchor + D + tail
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].copy()
    if top is not None:
        ref[anchor], ref[anchor + D + 1] = top
    return GraphIndex("c", ref, np.array([anchor], np.int32), np.array([1], np.uint8), np.zeros((1, 3), np.uint8),
                      np.array([[[1], [0], [0]]], np.uint64), 2, del_len=np.array([D], np.int32))


def _top_kmer(od):
    """the k-mer whose better strand scores highest"""
    import itertools
    sm, mv = od["score_matrix"], od["min_val"]
    best = max((max(int_score(bytes(k), sm, mv), int_score(revcomp(bytes(k)), sm, mv)), bytes(k))
               for k in itertools.product(b"ACGT", repeat=od["width"]))
    return best[1]


def test_score_key_span_field_at_its_largest():
    """W = 2 and a deletion of 2^19 - 3 bases: the junction walk spans exactly 2^19 - 1 bases, the key's span field; it is
    the carrier's best row (the top 2-mer at the region's first base) -- accepted and equal to the brute force.  One base
    more is refused."""
    from grafimo_amd import _native as nv
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.haplotype_scores import SPAN_MAX, compute_haplotype_scores
    m = _motif(2, 5)
    top = _top_kmer(motif_as_oracle_dict(m))
    D = (1 << 19) - 3
    idx = _one_deletion_index(D, 2, top)
    g = DeviceGraph(idx)
    try:
        regions = [(100, 100 + D + 60), (90, 100 + D + 2)]
        hs = compute_haplotype_scores(m, g, regions, False, Args())
        check_haplotype_scores(hs, idx, regions, m, False)
        assert hs.start[0, 0] in (100, 100 + D + 2) and abs(int(hs.stop[0, 0]) - int(hs.start[0, 0])) == SPAN_MAX
    finally:
        g.close()
    g = DeviceGraph(_one_deletion_index(D + 1, 2, top))
    try:
        with pytest.raises(nv.NativeError) as e:
            compute_haplotype_scores(m, g, [(100, 100 + D + 61)], False, Args())
        assert e.value.code == nv.GFM_ERR_INVALID and "2^19 - 1" in str(e.value)
    finally:
        g.close()


def test_variant_deletion_guard_at_its_largest():
    """W = 64: the longest deletion the variant table's coordinate fields take, 2^22 / 64 - 3 bases, is accepted and equals
    the brute force; one base more is refused"""
    from grafimo_amd import _native as nv
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.variant_effects import compute_variant_effects
    W = 64
    D = (1 << 22) // W - 3
    assert W * (D + 1) + W < 1 << 22 <= W * (D + 2) + W
    m = _motif(W, 3)
    idx = _one_deletion_index(D, W, None)
    g = DeviceGraph(idx)
    try:
        regions = [(0, len(idx.ref))]
        args = Args(threshold=1.0)
        ve = compute_variant_effects(m, g, regions, False, args, all_sites=True)
        check_variant_effects(ve, idx, regions, m, args, True)
        assert len(ve) == 1 and ve["ref_sequence"][0] and ve["alt_sequence"][0]
    finally:
        g.close()
    g = DeviceGraph(_one_deletion_index(D + 1, W, None))
    try:
        with pytest.raises(nv.NativeError) as e:
            compute_variant_effects(m, g, [(0, 100 + D + 200)], False, Args(threshold=1.0))
        assert e.value.code == nv.GFM_ERR_INVALID and "deletion too long" in str(e.value)
    finally:
        g.close()


def test_score_key_left_field_at_its_largest():
    """a chromosome of 2^28 bases: a region of 2^28 - 1 bases is scored (its best row 2^28 - 42 bases past the region's
    start, the key's left field near its top), one of 2^28 bases is refused.  The bases are N but for one k-mer near the
    end, so every cell's best row is known without the brute force."""
    from grafimo_amd import _native as nv
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.haplotype_scores import compute_haplotype_scores, pack_key
    W = 8
    m = _motif(W, 7)
    od = motif_as_oracle_dict(m)
    sm, mv = od["score_matrix"], od["min_val"]
    top = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[sm.argmax(0)])
    L, P = 1 << 28, (1 << 28) - 40
    ref = np.full(L, ord("N"), dtype=np.uint8)
    ref[P:P + W] = np.frombuffer(top, dtype=np.uint8)
    alt = next(c for c in b"ACGT" if c != top[3])
    idx = GraphIndex("c", ref, np.array([P + 3], np.int32), np.array([1], np.uint8), np.array([[alt, 0, 0]], np.uint8),
                     np.array([[[1], [0], [0]]], np.uint64), 2)
    g = DeviceGraph(idx)
    try:
        hs = compute_haplotype_scores(m, g, [(1, L), (-5, 60)], False, Args())

        def key(kmer):
            f, r = int_score(kmer, sm, mv), int_score(revcomp(kmer), sm, mv)
            return int(max(pack_key(f, P, P + W, 1, 1), pack_key(r, P, P + W, 0, 1)))

        mutated = top[:3] + bytes([alt]) + top[4:]
        assert key(top) > key(mutated) > int(pack_key(mv, 1, 1 + W, 1, 1))
        assert hs.keys[0].tolist() == [key(mutated), key(top), key(top)]
        assert hs.start[0, 1] in (P, P + W) and hs.best[1].tolist() == [mv, mv]
        with pytest.raises(nv.NativeError) as e:
            compute_haplotype_scores(m, g, [(0, L)], False, Args())
        assert e.value.code == nv.GFM_ERR_INVALID and "2^28 - 1" in str(e.value)
    finally:
        g.close()


def test_variant_record_retry(tmp_path, monkeypatch):
    """a first record capacity of 1: the call is made again with the count; the table equals the default call's and the brute
    force"""
    from grafimo_amd import variant_effects as ve
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=41, kinds="sidmDO")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    g = DeviceGraph(idx)
    try:
        regions = [(0, 250), (200, 400)]
        motifs = [_motif(8, 1), _motif(8, 2)]
        args = Args(threshold=1e-3)
        ref = ve.compute_variant_effects_many(motifs, g, regions, False, args, all_sites=True)
        monkeypatch.setattr(ve, "_FIRST_REC_CAPACITY", 1)
        got = ve.compute_variant_effects_many(motifs, g, regions, False, args, all_sites=True)
        for m, a, b in zip(motifs, ref, got):
            assert len(a) > 2 and a.equals(b)             # (more than one record: the first call was too small)
            check_variant_effects(b, idx, regions, m, args, True)
    finally:
        g.close()


def test_fuzz_driver_prints_its_stats(tmp_path):
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "graph_tables_fuzz.py"), "1", "3"], check=True,
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.stdout.startswith("graph_tables_fuzz: 1 seeds, "), r.stdout
