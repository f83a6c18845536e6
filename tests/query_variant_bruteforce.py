"""Brute force for the query-variant table (grafimo_amd/query_variants.py) -- TEST INFRASTRUCTURE ONLY, independent of the
versions machinery: one haplotype per class of variant_bruteforce.haplotype_classes (and the reference) is spelled over the
WHOLE chromosome (variant_bruteforce.spell), the edit is located, checked and applied by the rule the module's docstring states,
every window the edit touches is scored with int_score / revcomp, the sums are Python integers, and the haplotypes are grouped
by their used context."""
import numpy as np

from variant_bruteforce import haplotype_classes, int_score, revcomp, spell

APPLIED, ABSENT, MISMATCH = 0, 1, 2


def hand_graph():
    """A chromosome of 20 bases, ACGT five times, and four haplotypes: 0 the reference's; 1 a SNP C>T at 9; 2 deletes 10 and 11
    behind the anchor 9; 3 reads GG behind 10.  Small enough to read every answer off."""
    from grafimo_amd.extract_regions import GraphIndex
    bits = np.zeros((3, 3, 1), dtype=np.uint64)
    bits[0, 0, 0], bits[1, 0, 0], bits[2, 0, 0] = 0b0010, 0b0100, 0b1000
    return GraphIndex("c", np.frombuffer(b"ACGT" * 5, dtype=np.uint8), np.array([9, 9, 10], np.int32), np.array([1, 1, 1], np.uint8),
                      np.array([[ord("T"), 0, 0], [0, 0, 0], [0, 0, 0]], np.uint8), bits, 4, del_len=np.array([0, 2, 0], np.int32),
                      ins_len=np.array([0, 0, 2], np.int32), ins_off=np.array([0, 0, 0], np.int32),
                      ins_bases=np.frombuffer(b"GG", dtype=np.uint8))


def spelled(idx, h, cache=None):
    """-> (bases bytes, {coordinate: offset of the non-inserted base that carries it}, inserted list) of haplotype h over the
    chromosome; h = -1: the reference"""
    if cache is not None and h in cache:
        return cache[h]
    if h < 0:
        seq = bytes(np.asarray(idx.ref, dtype=np.uint8))
        got = (seq, {c: c for c in range(len(seq))}, [False] * len(seq))
    else:
        seq, coord, ins, _, _ = spell(idx, h)
        got = (bytes(seq), {c: j for j, (c, t) in enumerate(zip(coord, ins)) if not t}, ins)
    if cache is not None:
        cache[h] = got
    return got


def locate(x: bytes, at: dict, L: int, pos0: int, ref: bytes):
    """-> (status, o) of the edit (pos0, ref) on the spelled sequence x, `at` its coordinate map, L the chromosome's length"""
    lr = len(ref)
    if lr > 0:
        if any(pos0 + k not in at for k in range(lr)):
            return ABSENT, at.get(pos0, -1)
        o = at[pos0]
        ok = all(at[pos0 + k] == o + k for k in range(lr)) and x[o:o + lr].upper() == ref.upper()
        return (APPLIED if ok else MISMATCH), o
    if pos0 - 1 not in at:
        return ABSENT, at.get(pos0, -1)
    if pos0 == L:
        o = len(x)
    elif pos0 in at:
        o = at[pos0]
    else:
        return ABSENT, -1
    return (APPLIED if at[pos0 - 1] == o - 1 else MISMATCH), o


def side(x: bytes, o: int, l: int, W: int, sm, min_val: int, wtab, forward_only: bool):
    """-> (best (score, s - o, strand, k-mer as printed) or None, the sum of the weights) over the windows of x that touch
    [o, o + l) -- l == 0: that cross the junction before o"""
    best, key, total = None, None, 0
    for s in range(max(0, o - W + 1), min(o + l - 1, len(x) - W) + 1):
        k = x[s:s + W]
        rows = [(int_score(k, sm, min_val), "+", k)]
        if not forward_only:
            rk = revcomp(k)
            rows.append((int_score(rk, sm, min_val), "-", rk))
        for sc, strand, text in rows:
            total += int(wtab[sc])
            this = (-sc, s, strand != "+")
            if key is None or this < key:
                key, best = this, (sc, s - o, strand, text.decode())
    return best, total


def edit_result(x: bytes, o: int, ref: bytes, alt: bytes, W: int, sm, min_val: int, wtab, forward_only: bool):
    """-> (ref best, ref sum, alt best, alt sum) of the applied edit"""
    y = x[:o] + alt + x[o + len(ref):]
    return side(x, o, len(ref), W, sm, min_val, wtab, forward_only) + side(y, o, len(alt), W, sm, min_val, wtab, forward_only)


def used_context(x: bytes, o: int, lr: int, W: int):
    lo = max(0, o - W + 1)
    return x[lo:min(len(x), o + lr + W - 1)], o - lo


def variant_expected(idx, pos0: int, ref: bytes, alt: bytes, W: int, sm, min_val: int, wtab, forward_only: bool = False,
                     groups=(), classes=None, cache=None, memo=None):
    """The expected table rows of one normalised query variant -> dict: status (haplotypes applied, absent, mismatch);
    contexts, numbered by haplotypes descending then representative: each dict(count, first, group_counts, is_reference,
    members, classes -- how many haplotype classes spell it --, ref, ref_sum, alt, alt_sum); reference: (status, (ref, ref_sum,
    alt, alt_sum) or None).  `classes`: haplotype_classes(idx); `cache`: the spelled sequences; `memo`: results per (context, edit, motif) -- the caller keys it per
    motif."""
    L = len(idx.ref)
    H = int(idx.n_haplotypes)
    reps, class_of = classes if classes is not None else haplotype_classes(idx)
    memo = {} if memo is None else memo
    counts = [0, 0, 0]
    found = {}

    def result(x, o):
        ctx = used_context(x, o, len(ref), W)
        key = (ctx, ref, alt)
        if key not in memo:
            memo[key] = edit_result(x, o, ref, alt, W, sm, min_val, wtab, forward_only)
        return ctx, memo[key]

    for c, h in enumerate(np.asarray(reps).tolist()):
        members = np.flatnonzero(class_of == c)
        x, at, _ = spelled(idx, h, cache)
        status, o = locate(x, at, L, pos0, ref)
        counts[status] += len(members)
        if status != APPLIED:
            continue
        ctx, res = result(x, o)
        d = found.setdefault(ctx, dict(members=[], res=res, classes=0))
        d["members"] += members.tolist()
        d["classes"] += 1
    x, at, _ = spelled(idx, -1, cache)
    status, o = locate(x, at, L, pos0, ref)
    ref_ctx, ref_res = result(x, o) if status == APPLIED else (None, None)
    contexts = []
    for ctx, d in found.items():
        m = sorted(d["members"])
        contexts.append(dict(count=len(m), first=m[0], group_counts=[len(set(m) & set(g)) for g in groups], is_reference=ctx == ref_ctx,
                             members=m, classes=d["classes"], ref=d["res"][0], ref_sum=d["res"][1], alt=d["res"][2], alt_sum=d["res"][3]))
    contexts.sort(key=lambda d: (-d["count"], d["first"]))
    assert sum(counts) == H
    return dict(status=tuple(counts), contexts=contexts, reference=(status, ref_res))
