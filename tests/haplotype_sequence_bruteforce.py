"""Brute force for the haplotype sequence table (grafimo_amd/haplotype_sequences.py) -- TEST INFRASTRUCTURE ONLY.

Built on variant_bruteforce.spell, which spells a haplotype over the whole chromosome with a coordinate and an inserted flag
per base: the region sequence of [S, E) clipped to the chromosome is the spelled bases with coord + inserted >= S and
coord < E.  The reference (h = -1) is spelled through a copy of the index with every carrier bit cleared.  The versions of a
region are np.unique over the spelled strings of all haplotypes, numbered by count descending, then by smallest member."""
import copy

import numpy as np

from variant_bruteforce import spell


def reference_index(idx):
    """a copy of `idx` whose haplotypes carry no ALT"""
    ref = copy.copy(idx)
    if idx.alt_bits is not None:
        ref.alt_bits = np.zeros_like(np.asarray(idx.alt_bits))
    return ref


def spelled(idx, h):
    """-> (bases bytes, coord int64, inserted bool) of haplotype h over the chromosome (-1: the reference)"""
    seq, coord, ins, _, _ = spell(reference_index(idx), 0) if h < 0 else spell(idx, h)
    return bytes(seq), np.asarray(coord, dtype=np.int64), np.asarray(ins, dtype=bool)


def cut(sp, L, S, E):
    """the region's part of a spelled chromosome -> (bytes, coords list, inserted list)"""
    seq, coord, ins = sp
    S, E = max(int(S), 0), min(int(E), L)
    if E <= S:
        return b"", [], []
    keep = np.flatnonzero((coord + ins >= S) & (coord < E))
    if not len(keep):
        return b"", [], []
    a, b = int(keep[0]), int(keep[-1]) + 1
    assert len(keep) == b - a                                # (a contiguous stretch)
    return seq[a:b], coord[a:b].tolist(), ins[a:b].tolist()


def region_sequence(idx, h, S, E, cache=None):
    """-> (bytes, coords, inserted) of haplotype h (-1: the reference) in region [S, E).  `cache`: a dict that keeps the
    spelled chromosomes of `idx` between calls."""
    if cache is None:
        return cut(spelled(idx, h), len(idx.ref), S, E)
    if h not in cache:
        cache[h] = spelled(idx, h)
    return cut(cache[h], len(idx.ref), S, E)


def content_key(seq, seed=0, key_bits=64):
    """the library's content key of a sequence: the sum mod 2^64 over its bases of mix64(seed, offset << 8 | base) (the class
    table's mix64), masked to key_bits"""
    with np.errstate(over="ignore"):
        x = (np.arange(len(seq), dtype=np.uint64) << np.uint64(8)) | np.frombuffer(bytes(seq), dtype=np.uint8).astype(np.uint64)
        z = x + np.uint64((int(seed) + 1) * 0x9E3779B97F4A7C15 & (2 ** 64 - 1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        key = int(z.sum(dtype=np.uint64)) if len(seq) else 0
    return key & ((1 << key_bits) - 1)


def versions_of(strings, counts, firsts, groups_of=None, n_groups=0):
    """`strings` one per item (a haplotype, or a class with its count, smallest member and per-group counts) -> the versions:
    (version_of_item int64, count, first int64 [V], group_counts int64 [V, G], sequences list of bytes)"""
    distinct = sorted(set(strings))
    at = {s: k for k, s in enumerate(distinct)}
    inv = np.array([at[s] for s in strings], dtype=np.int64)
    count = np.zeros(len(distinct), dtype=np.int64)
    np.add.at(count, inv, np.asarray(counts, dtype=np.int64))
    first = np.full(len(distinct), np.iinfo(np.int64).max)
    np.minimum.at(first, inv, np.asarray(firsts, dtype=np.int64))
    gc = np.zeros((len(distinct), n_groups), dtype=np.int64)
    if n_groups:
        np.add.at(gc, inv, np.asarray(groups_of, dtype=np.int64).reshape(len(strings), n_groups))
    order = np.lexsort((first, -count))
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank[inv], count[order], first[order], gc[order], [distinct[k] for k in order.tolist()]


def region_versions(idx, S, E, groups=(), classes=None, cache=None):
    """-> dict: version_of int64 [H], count, first int64 [V], group_counts int64 [V, G], is_reference bool [V], sequences (list
    of bytes).  `groups`: lists of haplotype indices.  `classes`: (one haplotype of every class, the class of every haplotype)
    of variant_bruteforce.haplotype_classes -- one spelling per class instead of one per haplotype (the same result).  `cache`:
    region_sequence's."""
    H, L = int(idx.n_haplotypes), len(idx.ref)
    member = np.zeros((H, len(groups)), dtype=np.int64)
    for g, who in enumerate(groups):
        member[np.unique(np.asarray(list(who), dtype=np.int64)), g] = 1
    if classes is None:
        strings = [region_sequence(idx, h, S, E, cache)[0] for h in range(H)]
    else:
        reps, cls = classes
        per_class = [region_sequence(idx, int(h), S, E, cache)[0] for h in reps.tolist()]
        strings = [per_class[c] for c in cls.tolist()]
    version_of, count, first, gc, seqs = versions_of(strings, np.ones(H, dtype=np.int64), np.arange(H), member, len(groups))
    ref = region_sequence(idx, -1, S, E, cache)[0]
    return {"version_of": version_of, "count": count, "first": first, "group_counts": gc,
            "is_reference": np.array([s == ref for s in seqs], dtype=bool), "sequences": seqs}


def check_versions(hs, per_region, ctx=None):
    """a HaplotypeSequences against the region_versions dicts of its regions, everything exactly equal"""
    assert len(per_region) == len(hs.n_versions), ctx
    for r, exp in enumerate(per_region):
        a, b = int(hs.offsets[r]), int(hs.offsets[r + 1])
        assert int(hs.n_versions[r]) == len(exp["count"]) == b - a, (ctx, r, int(hs.n_versions[r]), len(exp["count"]))
        assert np.array_equal(hs.version_of[r], exp["version_of"]), (ctx, r)
        assert np.array_equal(hs.count[a:b], exp["count"]) and np.array_equal(hs.first[a:b], exp["first"]), (ctx, r)
        assert np.array_equal(hs.group_counts[a:b], exp["group_counts"]), (ctx, r)
        assert np.array_equal(hs.is_reference[a:b], exp["is_reference"]), (ctx, r)
        for k in range(b - a):
            assert hs.sequence(r, k) == exp["sequences"][k] and int(hs.length[a + k]) == len(exp["sequences"][k]), (ctx, r, k)
            members = hs.classes_of(r, k)
            ca = int(hs.classes.offsets[r])
            assert int(hs.classes.count[ca + members].sum()) == int(exp["count"][k]), (ctx, r, k)
            assert int(hs.classes.first[ca + members].min()) == int(exp["first"][k]), (ctx, r, k)
