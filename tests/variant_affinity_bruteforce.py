"""Haplotype brute force for the per-variant affinity table (grafimo_amd/variant_affinity.py) -- TEST INFRASTRUCTURE ONLY.

Every haplotype is spelled from the reference and the alleles its bitsets give it (variant_bruteforce.spell, which also tags
every allele's footprint on the spelled bases); every window of W consecutive bases of it is an occurrence on each strand
(the '-' row is the reverse complement) when ANY region holds it under the report's region rule -- start (the first base's
coordinate, + 1 if that base was inserted) in [S, E), stop (the last base's coordinate + 1) <= E, as
haplotype_affinity_bruteforce._sums makes them; an occurrence several regions hold counts once.  It qualifies for every slot
(site * 4 + allele) whose `single` tag lies on one of its bases or whose `junction` tag lies on one of its first W - 1 --
collected exactly as variant_bruteforce.best_hits collects them, but with no dedupe over k-mers: every offset of every
haplotype counts.  Per slot, in Python integers: sum += weights[score] per strand, rows += the strands.  No walk
enumeration and no kernel is involved.
"""
import os
import sys
from bisect import bisect_left
from typing import Dict, Tuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from variant_bruteforce import haplotype_classes, int_score, revcomp, spell  # noqa: E402


def variant_affinity_sums(idx, regions, W: int, sm: np.ndarray, min_val: int, weights, forward_only: bool = False,
                          memo: bool = False) -> Tuple[Dict[int, int], Dict[int, int]]:
    """-> ({slot: sum}, {slot: rows}) over the haplotypes' windows in the regions, Python integers; a slot without an
    occurrence is absent.  `weights`: a sequence indexed by the integer score.  `memo`: one haplotype per class of
    haplotype_classes, counted as many times as the class has haplotypes (the same result)."""
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

    if memo:
        first, cls = haplotype_classes(idx)
        todo = list(zip(first.tolist(), np.bincount(cls, minlength=len(first)).tolist()))
    else:
        todo = [(h, 1) for h in range(H)]
    sums: Dict[int, int] = {}
    rows: Dict[int, int] = {}
    strands = 1 if forward_only else 2
    for h, times in todo:
        seq, coord, ins, single, junction = spell(idx, h)
        s_keys = [t[0] for t in single]
        j_keys = [t[0] for t in junction]
        for o in range(0, len(seq) - W + 1):
            start = coord[o] + (1 if ins[o] else 0)
            stop = coord[o + W - 1] + 1
            slots = set()
            for a in range(bisect_left(s_keys, o), bisect_left(s_keys, o + W)):
                slots.add(single[a][1])
            for a in range(bisect_left(j_keys, o), bisect_left(j_keys, o + W - 1)):
                slots.add(junction[a][1])
            if not slots:
                continue
            if not any(max(S, 0) <= start < min(E, L) and stop <= min(E, L) for S, E in regions):
                continue
            kmer = bytes(seq[o:o + W])
            v = weight(kmer) + (0 if forward_only else weight(revcomp(kmer)))
            for s in slots:
                sums[s] = sums.get(s, 0) + times * v
                rows[s] = rows.get(s, 0) + times * strands
    return sums, rows


def expected_rows(idx, sums: Dict[int, int], rows: Dict[int, int]):
    """-> [(site, allele, ref_sum, alt_sum, ref_rows, alt_rows)] the table's rows from variant_affinity_sums(): one per
    (site, ALT allele) in site order, kept when either side has an occurrence"""
    out = []
    for i in range(len(idx.pos)):
        for a in range(1, int(idx.n_alts[i]) + 1):
            rr, ra = rows.get(4 * i, 0), rows.get(4 * i + a, 0)
            if rr or ra:
                out.append((i, a, sums.get(4 * i, 0), sums.get(4 * i + a, 0), rr, ra))
    return out
