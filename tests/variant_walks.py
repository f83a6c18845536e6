"""Walk enumerator for the per-variant effect table under --recomb -- TEST INFRASTRUCTURE ONLY.

The haplotype brute force (variant_bruteforce.py) only sees k-mers some haplotype spells; with --recomb every walk of a
window counts, also those no haplotype carries.  This enumerates the walks of the windows of SNV + insertion + deletion
graphs by depth-first search over the choices a walk makes -- the allele at a substitution site, which insertion (if
any) it reads at an anchor, which deletion (if any) it jumps -- with the constraints each choice puts on the haplotypes
(a site's allele; an insertion read, or passed by; a deletion jumped, or whose bases the walk uses), written here from
the semantics in oracle/extract_oracle.py, not from the kernels.  A walk qualifies for exactly the (site, allele) pairs
it carries a constraint for.  `carried_only=True` keeps the walks some haplotype carries (the AND of the constraints'
carrier sets is not empty): the table without --recomb, which the tests compare with the brute force.
"""
from typing import Dict, List

import numpy as np

from variant_bruteforce import int_score, revcomp


def _carriers(idx, i: int, a: int) -> np.ndarray:
    H = int(idx.n_haplotypes) if idx.alt_bits is not None else 0
    if not H:
        return np.zeros(0, bool)
    bits = lambda k: np.unpackbits(np.ascontiguousarray(idx.alt_bits[i, k]).view(np.uint8), bitorder="little")[:H].astype(bool)  # noqa: E731
    if a > 0:
        return bits(a - 1)
    na = 1 if (idx.del_len[i] or idx.ins_len[i]) else int(idx.n_alts[i])
    any_ = np.zeros(H, bool)
    for k in range(na):
        any_ |= bits(k)
    return ~any_


def window_walks(idx, p: int, W: int, limit: int):
    """every walk of window p (region end `limit`): -> [(bases bytes, stop, {slot})], slot = site * 4 + allele"""
    ref = bytes(np.asarray(idx.ref, dtype=np.uint8))
    L = len(ref)
    at: Dict[int, List[int]] = {}
    for i in range(len(idx.pos)):
        at.setdefault(int(idx.pos[i]), []).append(i)
    ins_sites = lambda x: [i for i in at.get(x, []) if idx.ins_len[i] > 0]     # noqa: E731
    del_sites = lambda x: [i for i in at.get(x, []) if idx.del_len[i] > 0]     # noqa: E731
    out = []

    def ins_seq(i):
        o = int(idx.ins_off[i])
        return bytes(idx.ins_bases[o:o + int(idx.ins_len[i])])

    def go(x, seq, tags):
        if x >= L:
            return                                     # runs off the chromosome
        snv = [i for i in at.get(x, []) if idx.del_len[i] == 0 and idx.ins_len[i] == 0]
        choices = [(ref[x:x + 1], set())]
        if snv:
            i = snv[0]
            choices = [(ref[x:x + 1], {4 * i})] + [(bytes([int(idx.alt_bases[i, a - 1])]), {4 * i + a})
                                                   for a in range(1, int(idx.n_alts[i]) + 1)]
        for b, t in choices:
            s2, t2 = seq + b, tags | t
            if len(s2) == W:
                if x + 1 <= limit:
                    out.append((s2, x + 1, t2))
                continue
            after_anchor(x, s2, t2)

    def after_anchor(x, seq, tags):
        ins = ins_sites(x)
        passed = set()
        for i in ins:                                  # read insertion i (the ones before it passed by)
            s2 = seq + ins_seq(i)[:W - len(seq)]
            t2 = tags | passed | {4 * i + 1}
            if len(s2) == W:
                if x + 1 <= limit:
                    out.append((s2, x + 1, t2))
            else:
                go(x + 1, s2, t2)
            passed = passed | {4 * i}
        tags = tags | passed                           # no insertion read: all passed by; then the deletions
        dels = del_sites(x)
        go(x + 1, seq, tags | {4 * d for d in dels})   # no jump: the first base of every deletion here is used
        for d in dels:                                 # jump d ("no" to the ones before it)
            ln = int(idx.del_len[d])
            land = x + ln + 1
            t2 = tags | {4 * d + 1} | {4 * k for k in dels if k != d and int(idx.del_len[k]) > ln}
            for k in range(len(idx.pos)):              # deletions anchored inside the jumped span that reach the landing base
                if idx.del_len[k] > 0 and x < int(idx.pos[k]) < land and int(idx.pos[k]) + int(idx.del_len[k]) >= land:
                    t2 = t2 | {4 * k}
            go(land, seq, t2)

    covering = {4 * d for d in range(len(idx.pos))
                if idx.del_len[d] > 0 and int(idx.pos[d]) < p <= int(idx.pos[d]) + int(idx.del_len[d])}
    go(p, b"", set(covering))
    for i in ins_sites(p - 1):                         # walks that start inside an insertion anchored at p - 1
        s = ins_seq(i)
        for t in range(len(s)):
            part = s[t:t + W]
            if len(part) == W:
                if p <= limit:
                    out.append((part, p, {4 * i + 1}))
            else:
                go(p, part, {4 * i + 1} | covering)
    return out


def best_hits_walks(idx, regions, W: int, sm, min_val: int, forward_only: bool = False, carried_only: bool = False):
    """-> {slot: (score, start, stop, strand, kmer as printed)} over every walk of every window of the regions"""
    sm = np.asarray(sm, dtype=np.int64)
    L = len(idx.ref)
    tail = 1 if (np.asarray(idx.ins_len) > 0).any() else W
    cache = {}
    best: Dict[int, tuple] = {}
    for S, E in regions:
        s, e = max(S, 0), min(E, L)
        for p in range(s, e - tail + 1):
            for kmer, stop, slots in window_walks(idx, p, W, e):
                if not slots:
                    continue
                if carried_only:
                    H = int(idx.n_haplotypes) if idx.alt_bits is not None else 0
                    acc = np.ones(H, bool)
                    for sl in slots:
                        if sl not in cache:
                            cache[sl] = _carriers(idx, sl >> 2, sl & 3)
                        acc &= cache[sl]
                    if not acc.any():
                        continue
                rows = [(int_score(kmer, sm, min_val), p, stop, "+", kmer)]
                if not forward_only:
                    rk = revcomp(kmer)
                    rows.append((int_score(rk, sm, min_val), stop, p, "-", rk))
                for r in rows:
                    key = (-r[0], r[1], r[2], r[3] != "+", r[4])
                    for sl in slots:
                        b = best.get(sl)
                        if b is None or key < (-b[0], b[1], b[2], b[3] != "+", b[4]):
                            best[sl] = r
    return best
