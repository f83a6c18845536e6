"""TEST INFRASTRUCTURE: the checks of the three graph tables against their brute forces, shared by the feature tests
(test_gpu_variant_effects.py, test_gpu_haplotype_hits.py, test_gpu_haplotype_scores.py) and the graph-table fuzz
(graph_tables_fuzz_core.py), and a GraphIndex of random haplotype bitsets for any haplotype count (the VCF generator only
gives an even one)."""
import numpy as np

from extract_helpers import motif_as_oracle_dict
from haplotype_bruteforce import haplotype_matrix, integer_cutoff
from haplotype_score_bruteforce import haplotype_score_keys
from variant_bruteforce import best_hits, expected_rows


def check_variant_effects(df, idx, regions, motif, args, all_sites, name=None, best=None, memo=False):
    """every row of the per-variant effect table against the haplotype brute force (or `best`, the walk enumerator's under
    --recomb): the rows in site order, the effect, per side score, p-value, coordinates, strand and k-mer"""
    from oracle import oracle as orc
    od = motif_as_oracle_dict(motif)
    W = od["width"]
    if best is None:
        best = best_hits(idx, regions, W, od["score_matrix"], od["min_val"], forward_only=args.noreverse, memo=memo)
    # (which side passes the threshold: the report's tail table, normalised -- the lowest score has p = 1 exactly)
    exp = expected_rows(idx, best, orc.p_table(od["pmf"]), args.threshold, all_sites)
    assert len(df) == len(exp), (len(df), len(exp))
    for row, ((i, a), (r, x, eff)) in zip(df.itertuples(index=False), sorted(exp.items())):
        assert row.position == int(idx.pos[i]) + 1
        assert row.effect == eff, (i, a, row.effect, eff)
        for side, e in (("ref", r), ("alt", x)):
            if e is None:
                assert np.isnan(getattr(row, side + "_score")) and getattr(row, side + "_sequence") == ""
                continue
            sc, lo, pv = orc.score_kmers(np.frombuffer(e[4], dtype=np.uint8).reshape(1, W), od["score_matrix"], od["pmf"],
                                         od["min_val"], od["scale"], od["offset"])
            assert int(sc[0]) == e[0]
            assert getattr(row, side + "_score") == e[0] / od["scale"] + W * od["offset"], (i, a, side)
            assert (getattr(row, side + "_start"), getattr(row, side + "_stop"), getattr(row, side + "_strand"),
                    getattr(row, side + "_sequence")) == (e[1], e[2], e[3], e[4].decode()), (i, a, side)
            assert abs(getattr(row, side + "_pvalue") - pv[0]) <= 1e-12
        if name is not None:
            assert row.sequence_name == name
    return exp


def hit_matrix_expected(idx, regions, motif, threshold, forward_only, cutoff=None, memo=False):
    """-> (counts, best) of the hit brute force at the report's integer cutoff of `threshold` (or the given cutoff): the
    lowest score whose p-value in the report's tail table (normalised: the lowest score has p = 1 exactly) is below it"""
    from oracle import oracle as orc
    od = motif_as_oracle_dict(motif)
    if cutoff is None:
        cutoff = integer_cutoff(orc.p_table(od["pmf"]), threshold)
    return haplotype_matrix(idx, regions, od["width"], od["score_matrix"], od["min_val"], cutoff, forward_only=forward_only,
                            memo=memo)


def check_haplotype_hits(hh, idx, regions, motif, args, exp=None, memo=False):
    """counts and best of the hit matrix against the hit brute force (`exp`: its (counts, best) if already made), and the
    log-odds scores and p-values made from them"""
    od = motif_as_oracle_dict(motif)
    W = od["width"]
    ptab = np.cumsum(od["pmf"][::-1])[::-1]
    counts, best = exp if exp is not None else hit_matrix_expected(idx, regions, motif, args.threshold, args.noreverse,
                                                                   memo=memo)
    assert hh.counts.shape == counts.shape and hh.counts.dtype == np.int32
    assert (hh.counts == counts).all(), np.argwhere(hh.counts != counts)[:5]
    some = best >= 0
    assert (hh.best == np.where(some, best, -1)).all(), np.argwhere(hh.best != np.where(some, best, -1))[:5]
    exp_score = np.where(some, best / od["scale"] + W * od["offset"], np.nan)
    assert np.array_equal(hh.best_score, exp_score, equal_nan=True)
    exp_p = np.where(some, ptab[np.where(some, best, 0)], np.nan)
    assert np.allclose(hh.best_pvalue, exp_p, rtol=1e-12, atol=0, equal_nan=True)
    return counts


def check_haplotype_scores(hs, idx, regions, motif, forward_only, exp=None, memo=False):
    """every cell of the best score matrix against the score brute force (`exp`: its keys if already made): the key bit for
    bit, and the fields made from it -> the scaled best scores [R, H + 1] (column H the reference path)"""
    from grafimo_amd.haplotype_scores import unpack_keys
    od = motif_as_oracle_dict(motif)
    W = od["width"]
    if exp is None:
        exp = haplotype_score_keys(idx, regions, W, od["score_matrix"], od["min_val"], forward_only=forward_only, memo=memo)
    assert hs.keys.shape == exp.shape
    assert (hs.keys == exp).all(), np.argwhere(hs.keys != exp)[:5]
    base = np.array([max(S, 0) for S, _ in regions], dtype=np.int64)[:, None]
    best, left, right, plus = unpack_keys(exp, base)
    ptab = np.cumsum(od["pmf"][::-1])[::-1]
    some = best >= 0
    full_best = np.concatenate([hs.best, hs.reference_best[:, None]], axis=1)
    assert (full_best == best).all()
    score = np.concatenate([hs.best_score, hs.reference_score[:, None]], axis=1)
    assert np.array_equal(score, np.where(some, best / od["scale"] + W * od["offset"], np.nan), equal_nan=True)
    pv = np.concatenate([hs.best_pvalue, hs.reference_pvalue[:, None]], axis=1)
    assert np.allclose(pv, np.where(some, ptab[np.where(some, best, 0)], np.nan), rtol=1e-12, atol=0, equal_nan=True)
    start = np.concatenate([hs.start, hs.reference_start[:, None]], axis=1)
    stop = np.concatenate([hs.stop, hs.reference_stop[:, None]], axis=1)
    strand = np.concatenate([hs.strand, hs.reference_strand[:, None]], axis=1)
    assert (start == np.where(some, np.where(plus, left, right), -1)).all()
    assert (stop == np.where(some, np.where(plus, right, left), -1)).all()
    assert (strand == np.where(some, np.where(plus, "+", "-"), "")).all()
    if forward_only:
        assert not (strand == "-").any()
    return best


def random_bitset_index(n_hap: int, seed: int, length: int = 300, n_sites: int = 30, indels: bool = True, chrom: str = "c"):
    """A GraphIndex of `n_hap` haplotypes (any count: 1, 63, 65, 129 ...) with random alleles: substitution sites of 1-3
    ALTs, and with `indels` insertions of 1-5 bases and deletions of 1-6 bases, at distinct positions, no site inside a
    deletion's span -- so a haplotype never carries two alleles over one base and spells one sequence (the brute forces'
    assumption).  Sites come in clusters and alone; a site's allele frequency is random (some sites carried by none)."""
    from grafimo_amd.extract_regions import MAX_ALTS, GraphIndex
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = acgt[rng.choice(4, size=length, p=[0.3, 0.2, 0.2, 0.3])]
    pos, n_alts, alt, dl, il, io, pool = [], [], [], [], [], [], []
    p = int(rng.integers(0, 8))
    while p < length and len(pos) < n_sites:
        kind = rng.choice(["s", "i", "d"], p=[0.6, 0.2, 0.2]) if indels else "s"
        d = min(int(rng.integers(1, 7)), length - 1 - p) if kind == "d" else 0
        if kind == "d" and d < 1:
            kind = "s"
        row = np.zeros(MAX_ALTS, np.uint8)
        if kind == "s":
            others = [c for c in acgt if c != ref[p]]
            na = int(rng.integers(1, 4))
            row[:na] = rng.permutation(others)[:na]
        else:
            na = 1
        n_ins = int(rng.integers(1, 6)) if kind == "i" else 0
        pos.append(p)
        n_alts.append(na)
        alt.append(row)
        dl.append(d)
        il.append(n_ins)
        io.append(len(pool))
        pool.extend(acgt[rng.integers(0, 4, n_ins)].tolist())
        p += d + (int(rng.integers(1, 4)) if rng.random() < 0.5 else int(rng.integers(4, 30)))
    S, hw = len(pos), (n_hap + 63) // 64
    bits = np.zeros((S, MAX_ALTS, hw * 64), dtype=bool)
    for i in range(S):
        af = rng.random() ** 1.5 if rng.random() < 0.9 else 0.0
        a = np.where(rng.random(n_hap) < af, rng.integers(1, n_alts[i] + 1, size=n_hap), 0)
        for k in range(n_alts[i]):
            bits[i, k, :n_hap] = a == k + 1
    words = np.packbits(bits, axis=-1, bitorder="little").view(np.uint64).reshape(S, MAX_ALTS, hw)
    return GraphIndex(chrom, ref, np.array(pos, np.int32), np.array(n_alts, np.uint8), np.array(alt, np.uint8).reshape(S, MAX_ALTS),
                      words, n_hap, del_len=np.array(dl, np.int32), ins_len=np.array(il, np.int32), ins_off=np.array(io, np.int32),
                      ins_bases=np.array(pool, np.uint8))
