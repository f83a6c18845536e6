"""TEST INFRASTRUCTURE (imports oracle/): one seed of the graph-table fuzz -- the per-variant effect table
(grafimo_amd.variant_effects), the per-haplotype hit matrix (grafimo_amd.haplotype_hits) and the per-haplotype best score
matrix (grafimo_amd.haplotype_scores) of a random motif set on ONE random graph, every motif's table against its brute force
(tests/variant_bruteforce.py, tests/variant_walks.py under --recomb, tests/haplotype_bruteforce.py,
tests/haplotype_score_bruteforce.py).

A seed's graph is a conflict-free VCF graph of a random allele mix (extract_fuzz_core.KINDS) and 2 .. 160 haplotypes, or a
GraphIndex of random bitsets with any haplotype count (1, 63, 65, 127, 129 ...: the tail of the last bitset word).  Its
regions overlap, repeat, start below 0, end past the chromosome, are empty or shorter than a motif, and start / end on a site,
inside a deletion or at an insertion anchor.  Its flags and work-split knobs are random (threshold, --no-reverse, --recomb,
--qvalueT, windows_per_run, haplotypes_per_block, a tiny hit-mask scratch, a tiny first record capacity of the variant table).
The three features run interleaved on one DeviceGraph, three times over the same (regions, widths) -- the fused pass behind
the hit matrix lists, stores, then replays its walk cache -- and then over a longer and a shorter region list (the window
buffer the variant table and the score runs share grows and is reused).  On top of the brute force: at threshold 1 the score
matrix's best equals the hit matrix's, and a region's hit counts sum to the report's haplotype_frequency.
`pytest -m gpu` runs a bounded seed set (tests/test_gpu_graph_tables_fuzz.py); scripts/graph_tables_fuzz.py runs seeds for a
fixed time."""
import contextlib
import io
import os
import shutil

import numpy as np

from extract_fuzz_core import KINDS, SynMotif
from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict
from graph_table_checks import (check_haplotype_hits, check_haplotype_scores, check_variant_effects, hit_matrix_expected,
                                random_bitset_index)
from haplotype_score_bruteforce import haplotype_score_keys
from tables_fuzz_core import _approx_rows
from variant_bruteforce import best_hits
from variant_walks import best_hits_walks

ODD_H = [1, 63, 65, 127, 129]


class Args:
    """the members of the workflow object the three features read"""

    def __init__(self, threshold=1e-4, noreverse=False, recomb=False, qvalueT=False, noqvalue=True):
        self.threshold, self.noreverse, self.recomb, self.qvalueT, self.noqvalue = threshold, noreverse, recomb, qvalueT, noqvalue


def make_graph(seed, rng, tmp):
    """-> (GraphIndex, what): every third seed a random-bitset index (odd haplotype counts), else a VCF graph"""
    from grafimo_amd.extract_regions import GraphIndex
    if seed % 3 == 2:
        H = ODD_H[(seed // 3) % len(ODD_H)] if rng.random() < 0.6 else int(rng.integers(2, 161))
        idx = random_bitset_index(H, 80_000 + seed, length=int(rng.integers(150, 360)), n_sites=int(rng.integers(4, 36)),
                                  indels=rng.random() < 0.8)
        return idx, f"bits H={H}"
    kinds = KINDS[seed % len(KINDS)]
    n_samples = int(rng.integers(1, 81))                # 2 .. 160 haplotypes: one to three bitset words
    fa, vcf = make_consistent_graph_files(tmp, length=int(rng.integers(250, 420)), n_samples=n_samples, seed=seed, kinds=kinds,
                                          dense=rng.random() < 0.5)
    with contextlib.redirect_stderr(io.StringIO()):     # (S: symbolic ALTs are reported and left out)
        idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    return idx, f"vcf {kinds} H={2 * n_samples}"


def make_regions(rng, idx):
    """overlapping and repeated regions, below 0 and past the end, empty and short, on sites / deletions / insertions"""
    L, p = len(idx.ref), np.asarray(idx.pos, dtype=np.int64)
    r = lambda lo, hi: int(rng.integers(lo, max(hi, lo + 1)))       # noqa: E731
    cand = [(0, L)]
    s = r(0, L - 30)
    cand += [(s, s + r(20, 160))] * 2
    cand += [(-r(1, 40), r(10, 140)), (r(L // 2, L - 5), L + r(1, 60))]
    x = r(0, L)
    cand += [(x, x), (x, x + r(1, 4))]
    if len(p):
        i, j = r(0, len(p)), r(0, len(p))
        cand += [(int(p[i]), int(p[i]) + r(4, 120)), (max(0, int(p[j]) - r(4, 120)), int(p[j]) + r(0, 2))]
    dels = np.nonzero(idx.del_len > 0)[0]
    if len(dels):
        d = int(dels[r(0, len(dels))])
        inside = int(p[d]) + 1 + r(0, int(idx.del_len[d]))
        cand += [(inside, inside + r(5, 100)), (max(0, inside - r(5, 100)), inside)]
    ins = np.nonzero(idx.ins_len > 0)[0]
    if len(ins):
        k = int(ins[r(0, len(ins))])
        cand += [(int(p[k]), int(p[k]) + r(5, 100)), (max(0, int(p[k]) - r(5, 100)), int(p[k]) + 1)]
    keep = rng.permutation(len(cand))[:r(3, 9)]
    return [cand[k] for k in sorted(keep)] if rng.random() < 0.5 else [cand[k] for k in keep]


def make_motifs(rng, idx, regions, bound):
    """2 .. 4 motifs of widths in 1 .. 64 (mixed, sometimes one motif twice), the widths cut until the regions' rows at every
    width are under `bound` (the walk enumerator's and the device's work)"""
    widths = [int(w) for w in rng.choice(np.arange(1, 65), size=int(rng.integers(1, 4)), replace=False)]
    for k, w in enumerate(widths):
        while w > 1 and _approx_rows(idx, regions, w) > bound:
            w //= 2
        widths[k] = w
    motifs = [SynMotif(int(rng.choice(widths)), seed=int(rng.integers(0, 1 << 20))) for _ in range(int(rng.integers(2, 5)))]
    for i, m in enumerate(motifs):
        m.motif_id, m.motif_name = f"M{i}_{m.width}", f"m{i}"
    if rng.random() < 0.3:
        motifs.append(motifs[0])                                      # the same numbers twice in one set
    return motifs


def report_cutoff(motif, g, regions, args):
    """-> (the lowest integer score among the report's rows, the report): the cutoff of --qvalueT (the report keeps q < t, q
    falls as the score rises).  A report without rows ends the command line (SystemExit, as the reference): no row."""
    import pandas as pd
    from grafimo_amd.extract_regions import compute_results_from_graph
    od = motif_as_oracle_dict(motif)
    try:
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            rep = compute_results_from_graph(motif, g, regions, False, args)
    except SystemExit:
        rep = pd.DataFrame()
    if not len(rep):
        return len(od["pmf"]), rep
    sc = np.rint((rep["score"].to_numpy(float) - od["width"] * od["offset"]) * od["scale"]).astype(np.int64)
    assert np.array_equal(sc / od["scale"] + od["width"] * od["offset"], rep["score"].to_numpy(float))
    return int(sc.min()), rep


def check_sums_against_report(hh, rep):
    """the hit counts of a region sum to the haplotype_frequency of the report's rows of the region (a region listed twice:
    its rows twice on both sides)"""
    freq = rep.groupby("sequence_name")["haplotype_frequency"].sum() if len(rep) else {}
    sums = {}
    for name, s in zip(hh.region_names.tolist(), hh.counts.sum(axis=1).tolist()):
        sums[name] = sums.get(name, 0) + int(s)
    for name, s in sums.items():
        assert s == int(freq.get(name, 0)), (name, s, int(freq.get(name, 0)))


def fuzz_seed(seed, tmp, stats, rows_bound=40_000):
    """one graph, one motif set, the three features interleaved on one DeviceGraph.  `stats`: seeds / tables / cells"""
    from grafimo_amd import variant_effects as ve
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.haplotype_hits import compute_haplotype_hits, compute_haplotype_hits_many
    from grafimo_amd.haplotype_scores import compute_haplotype_scores, compute_haplotype_scores_many
    from grafimo_amd.variant_effects import compute_variant_effects, compute_variant_effects_many
    rng = np.random.default_rng(70_000 + seed)
    d = os.path.join(str(tmp), f"g{seed}")
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    idx, what = make_graph(seed, rng, d)
    regions = make_regions(rng, idx)
    motifs = make_motifs(rng, idx, regions, rows_bound)
    H = int(idx.n_haplotypes)
    fwd = bool(rng.random() < 0.25)
    recomb = bool(rng.random() < 0.4) and max(_approx_rows(idx, regions, m.width) for m in motifs) <= rows_bound // 4
    vargs = Args(threshold=float(rng.choice([1.0, 0.2, 0.05, 1e-3])), noreverse=fwd, recomb=recomb)
    all_sites = bool(rng.random() < 0.5)
    qt = bool(rng.random() < 0.25)
    hargs = Args(threshold=0.9 if qt else float(rng.choice([1.0, 0.3, 0.05, 1e-2, 1e-4])), noreverse=fwd, qvalueT=qt,
                 noqvalue=not qt)
    wpr = int(rng.choice([0, 1, 3, 7, 64, 1024]))
    hpb = int(rng.choice([0, 64, 128, 192, 4096]))
    hw = (H + 63) // 64
    scratch = int(rng.choice([0, 1, 2, 5])) * (8 * hw + 4)
    first_cap = int(rng.choice([0, 0, 1, 7]))
    ctx = (seed, what, regions, [m.width for m in motifs], vars(vargs), vars(hargs), all_sites, wpr, hpb, scratch, first_cap)
    od = [motif_as_oracle_dict(m) for m in motifs]
    # the brute forces, once per motif (the three calls below must all give them)
    exp_v = [(best_hits_walks(idx, regions, o["width"], o["score_matrix"], o["min_val"], forward_only=fwd) if recomb else
              best_hits(idx, regions, o["width"], o["score_matrix"], o["min_val"], forward_only=fwd, memo=True)) for o in od]
    exp_s = [haplotype_score_keys(idx, regions, o["width"], o["score_matrix"], o["min_val"], forward_only=fwd, memo=True)
             for o in od]
    exp_h = [None] * len(motifs)
    g = DeviceGraph(idx)
    old_cap = ve._FIRST_REC_CAPACITY
    ve._FIRST_REC_CAPACITY = first_cap
    try:
        for rep_k in range(3):
            tabs = compute_variant_effects_many(motifs, g, regions, False, vargs, all_sites=all_sites)
            for k, (m, t) in enumerate(zip(motifs, tabs)):
                check_variant_effects(t, idx, regions, m, vargs, all_sites, name=idx.chrom, best=exp_v[k])
                stats["variant_rows"] += len(t)
            hhs = compute_haplotype_hits_many(motifs, g, regions, False, hargs, scratch_bytes=scratch)
            for k, (m, hh) in enumerate(zip(motifs, hhs)):
                if exp_h[k] is None:
                    cut = report_cutoff(m, g, regions, hargs)[0] if qt else None
                    exp_h[k] = hit_matrix_expected(idx, regions, m, hargs.threshold, fwd, cutoff=cut, memo=True)
                check_haplotype_hits(hh, idx, regions, m, hargs, exp=exp_h[k])
                stats["cells"] += 2 * hh.counts.size
            hss = compute_haplotype_scores_many(motifs, g, regions, False, vargs, windows_per_run=wpr, haplotypes_per_block=hpb)
            for k, (m, hs) in enumerate(zip(motifs, hss)):
                check_haplotype_scores(hs, idx, regions, m, fwd, exp=exp_s[k])
                stats["cells"] += hs.keys.size
            stats["tables"] += 3 * len(motifs)
        # on top of the brute force: threshold 1 through the hit list gives the score matrix's best; the counts sum to the
        # report's haplotype frequencies
        one = Args(threshold=1.0, noreverse=fwd)
        hh1 = compute_haplotype_hits(motifs[0], g, regions, False, one)
        assert (hh1.best == hss[0].best).all(), ctx
        check_sums_against_report(hhs[0], report_cutoff(motifs[0], g, regions, hargs)[1])
        # a longer, then a shorter region list on the same handle: the shared window buffer grows, then is reused
        longer = regions + [(0, len(idx.ref))] * 2 + [(int(rng.integers(0, len(idx.ref))), len(idx.ref))]
        for regs in (longer, regions[:1]):
            m, o = motifs[-1], od[-1]
            t = compute_variant_effects(m, g, regs, False, vargs, all_sites=True)
            best = (best_hits_walks(idx, regs, o["width"], o["score_matrix"], o["min_val"], forward_only=fwd) if recomb else
                    best_hits(idx, regs, o["width"], o["score_matrix"], o["min_val"], forward_only=fwd, memo=True))
            check_variant_effects(t, idx, regs, m, vargs, True, best=best)
            hs = compute_haplotype_scores(m, g, regs, False, vargs, windows_per_run=wpr, haplotypes_per_block=hpb)
            check_haplotype_scores(hs, idx, regs, m, fwd, memo=True)
            stats["variant_rows"] += len(t)
            stats["cells"] += hs.keys.size
            stats["tables"] += 2
    except AssertionError as e:
        raise AssertionError(f"graph-table fuzz seed {seed}: {ctx}") from e
    finally:
        ve._FIRST_REC_CAPACITY = old_cap
        g.close()
        shutil.rmtree(d, ignore_errors=True)
    stats["seeds"] += 1
