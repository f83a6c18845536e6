"""Haplotype brute force for the per-haplotype hit matrix (grafimo_amd/haplotype_hits.py) -- TEST INFRASTRUCTURE ONLY.

Every haplotype is spelled from the reference and the alleles its bitsets give it (variant_bruteforce.spell); every window
of W consecutive bases of it is a row under the report's region rule (start -- the first base's coordinate, + 1 if that
base was inserted -- in [S, E), stop -- the last base's coordinate + 1 -- <= E); the '+' row is the k-mer, the '-' row its
reverse complement unless forward_only; a row counts when its integer score (the oracle's sum over the score matrix) is
at or above `cutoff`.  counts[r, h] = the rows of haplotype h in region r that count, best[r, h] = their highest score
(-1: none).  No walk enumeration and no kernel is involved.
"""
import numpy as np

from variant_bruteforce import haplotype_classes, int_score, revcomp, spell


def haplotype_matrix(idx, regions, W: int, sm: np.ndarray, min_val: int, cutoff: int, forward_only: bool = False,
                     memo: bool = False):
    """-> (counts int64 [R, H], best int64 [R, H]).  `memo`: one haplotype per class of haplotype_classes, its columns
    copied to the class (the same result)."""
    sm = np.asarray(sm, dtype=np.int64)
    H = int(idx.n_haplotypes) if idx.alt_bits is not None else 0
    L = len(idx.ref)
    R = len(regions)
    counts = np.zeros((R, H), dtype=np.int64)
    best = np.full((R, H), -1, dtype=np.int64)
    cache = {}

    def score(k: bytes) -> int:
        s = cache.get(k)
        if s is None:
            s = cache[k] = int_score(k, sm, min_val)
        return s

    first, cls = haplotype_classes(idx) if memo else (np.arange(H), np.arange(H))
    for h in first.tolist():
        seq, coord, ins, _, _ = spell(idx, h)
        for o in range(0, len(seq) - W + 1):
            start = coord[o] + (1 if ins[o] else 0)
            stop = coord[o + W - 1] + 1
            kmer = bytes(seq[o:o + W])
            scores = [score(kmer)] + ([] if forward_only else [score(revcomp(kmer))])
            for r, (S, E) in enumerate(regions):
                if not (max(S, 0) <= start < min(E, L) and stop <= min(E, L)):
                    continue
                for s in scores:
                    if s >= cutoff:
                        counts[r, h] += 1
                        best[r, h] = max(best[r, h], s)
    return counts[:, first[cls]], best[:, first[cls]]


def integer_cutoff(ptable: np.ndarray, threshold: float) -> int:
    """the lowest integer score whose p-value is under the threshold (p < t, strict, as the report); len(ptable): none"""
    below = np.nonzero(np.asarray(ptable) < threshold)[0]
    return int(below[0]) if len(below) else len(ptable)
