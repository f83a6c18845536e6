"""Haplotype brute force for the per-haplotype affinity matrix (grafimo_amd/haplotype_affinity.py) -- TEST INFRASTRUCTURE ONLY.

Every haplotype is spelled from the reference and the alleles its bitsets give it (variant_bruteforce.spell); every window
of W consecutive bases of it is a row under the report's region rule (start -- the first base's coordinate, + 1 if that
base was inserted -- in [S, E), stop -- the last base's coordinate + 1 -- <= E), scored on both strands unless forward_only
(the '-' row is the reverse complement) with int_score.  A(r, h) = the sum of weights[score] over the rows, in Python
integers.  The reference column spells the index with every ALT bitset cleared.  No walk enumeration and no kernel is
involved.
"""
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from variant_bruteforce import haplotype_classes, int_score, revcomp, spell  # noqa: E402


def _sums(seq, coord, ins, regions, W, L, weight, forward_only):
    total = [0] * len(regions)
    for o in range(0, len(seq) - W + 1):
        start = coord[o] + (1 if ins[o] else 0)
        stop = coord[o + W - 1] + 1
        kmer = bytes(seq[o:o + W])
        v = weight(kmer) + (0 if forward_only else weight(revcomp(kmer)))
        for r, (S, E) in enumerate(regions):
            if max(S, 0) <= start < min(E, L) and stop <= min(E, L):
                total[r] += v
    return total


def haplotype_affinity_sums(idx, regions, W: int, sm: np.ndarray, min_val: int, weights, forward_only: bool = False,
                            memo: bool = False) -> np.ndarray:
    """-> sums uint64 [R, H + 1] (they must fit: asserted), column H the reference path.  `weights`: a sequence indexed by
    the integer score.  `memo`: one haplotype per class of haplotype_classes, its column copied to the class (the same
    result)."""
    sm = np.asarray(sm, dtype=np.int64)
    w = [int(x) for x in np.asarray(weights).tolist()]
    H = int(idx.n_haplotypes) if idx.alt_bits is not None else 0
    L = len(idx.ref)
    cache = {}

    def weight(k: bytes) -> int:
        v = cache.get(k)
        if v is None:
            v = cache[k] = w[int_score(k, sm, min_val)]
        return v

    out = np.zeros((len(regions), H + 1), dtype=np.uint64)

    def put(col, sums):
        assert all(0 <= s < (1 << 64) for s in sums)
        out[:, col] = np.array(sums, dtype=np.uint64)

    first, cls = haplotype_classes(idx) if memo else (np.arange(H), np.arange(H))
    for h in first.tolist():
        seq, coord, ins, _, _ = spell(idx, h)
        put(h, _sums(seq, coord, ins, regions, W, L, weight, forward_only))
    out[:, :H] = out[:, first[cls]]
    ref = copy.copy(idx)
    ref.alt_bits = None                                  # no haplotype carries an ALT allele: the reference path
    seq, coord, ins, _, _ = spell(ref, 0)
    put(H, _sums(seq, coord, ins, regions, W, L, weight, forward_only))
    return out
