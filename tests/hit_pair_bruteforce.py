"""Expected sides of the hit-pair table (grafimo_amd/hit_pairs.py) -- TEST INFRASTRUCTURE ONLY, no kernel runs here.

  * pairs_reference: an O(n^2) numpy restatement of gfm_hit_pairs' contract on arrays (rows, intervals, bitsets).
  * haplotype_pairs: the haplotype brute force -- every haplotype spelled (variant_bruteforce.spell), each motif's rows at or
    above the report's integer cutoff under the report's region rule exactly as hit_allele_bruteforce.carrier_counts takes
    them, and per haplotype and region listing the pairs of row INSTANCES within the gap counted per unordered key pair;
    key = (motif index, start, stop, strand, k-mer as printed).  No walk enumeration and no bitset.
  * enumerator_pairs: the same counts from the walk enumerator (hit_allele_bruteforce.walk_rows + variant_walks._carriers)
    through pairs_reference: the sum of joint popcounts over walk-level row pairs.  The two agree (tests/
    test_hit_pairs_host.py), so the expected side is itself checked without a GPU.
  * check_pairs: a HitPairs against all of it."""
from collections import Counter

import numpy as np

from extract_helpers import motif_as_oracle_dict
from hit_allele_bruteforce import report_cutoff, unpack, walk_rows
from variant_bruteforce import haplotype_classes, int_score, revcomp, spell
from variant_walks import _carriers


def popcount_rows(x):
    """uint64 [..., hw] -> the number of set bits over the last axis"""
    x = np.ascontiguousarray(x)
    bits = np.unpackbits(x.view(np.uint8).reshape(x.shape[:-1] + (8 * x.shape[-1],)), axis=-1)
    return bits.sum(axis=-1).astype(np.int64)


def pack(member, hw=None):
    """bool [n, H] -> uint64 [n, ceil(H / 64)] (bit h & 63 of word h >> 6)"""
    member = np.asarray(member, dtype=bool)
    n, H = member.shape
    hw = (H + 63) // 64 if hw is None else hw
    wide = np.zeros((n, hw * 64), dtype=bool)
    wide[:, :H] = member
    return np.ascontiguousarray(np.packbits(wide, axis=-1, bitorder="little").view(np.uint64).reshape(n, hw))


def pairs_reference(group, lo, hi, masks, min_gap, max_gap, group_bits=None, tie=()):
    """-> (a, b, joint, group_counts) as grafimo_amd.hit_pairs.pair_rows defines them: the rows ordered by the key
    (group, lo, hi, *tie, index); a pair = two rows of one group, key(a) < key(b), min_gap <= max(lo) - min(hi) <= max_gap,
    joint = popcount(mask_a & mask_b) > 0; listed by (key(a), key(b)); indices are the caller's"""
    group, lo, hi = np.asarray(group, np.int64), np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    masks = np.asarray(masks, np.uint64)
    n = len(group)
    G = 0 if group_bits is None else len(group_bits)
    order = np.lexsort(tuple([np.arange(n)] + [np.asarray(t, np.int64) for t in tie][::-1] + [hi, lo, group]))
    A, B, J, GC = [], [], [], []
    for k in range(n):
        i, rest = order[k], order[k + 1:]
        gap = np.maximum(lo[i], lo[rest]) - np.minimum(hi[i], hi[rest])
        cand = rest[(group[rest] == group[i]) & (gap >= min_gap) & (gap <= max_gap)]
        if not len(cand):
            continue
        both = masks[cand] & masks[i][None, :]
        joint = popcount_rows(both)
        cand, both, joint = cand[joint > 0], both[joint > 0], joint[joint > 0]
        A.append(np.full(len(cand), i, np.int64))
        B.append(cand.astype(np.int64))
        J.append(joint.astype(np.int32))
        if G:
            GC.append(np.stack([popcount_rows(both & np.asarray(group_bits, np.uint64)[g][None, :]) for g in range(G)],
                               axis=1).astype(np.int32).reshape(len(cand), G))
    if not A:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros((0, G), np.int32)
    return (np.concatenate(A), np.concatenate(B), np.concatenate(J),
            np.concatenate(GC) if G else np.zeros((sum(len(x) for x in A), 0), np.int32))


def _listings(entries):
    """entries [(GraphIndex, [(S, E)])] in the caller's order -> [(listing, idx, S, E)]"""
    out = []
    for idx, regions in entries:
        for S, E in regions:
            out.append((len(out), idx, int(S), int(E)))
    return out


def _count_pairs(out, listing, keys, lo, hi, min_gap, max_gap, times=1):
    """the pairs i < j of the instances within the gap into out[(listing, key, key)] (the smaller key first), each counted
    `times` times"""
    n = len(keys)
    if n < 2:
        return
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    gap = np.maximum(lo[:, None], lo[None, :]) - np.minimum(hi[:, None], hi[None, :])
    ok = np.triu((gap >= min_gap) & (gap <= max_gap), 1)
    ids = {}
    kid = np.array([ids.setdefault(k, len(ids)) for k in keys], dtype=np.int64)
    names = sorted(ids, key=ids.get)
    i, j = np.nonzero(ok)
    codes, counts = np.unique(kid[i] * len(names) + kid[j], return_counts=True)
    for code, c in zip(codes.tolist(), counts.tolist()):
        a, b = names[code // len(names)], names[code % len(names)]
        out[(listing,) + ((a, b) if a <= b else (b, a))] += c * times


def haplotype_pairs(entries, motifs, cutoffs, min_gap, max_gap, forward_only=False, memo=False):
    """-> Counter {(listing, key, key): over the haplotypes, the pairs of distinct row instances of the listing within the
    gap with these two keys (the smaller first)}.  `memo`: one haplotype per class of variant_bruteforce.haplotype_classes,
    counted as many times as the class has haplotypes (the same result)."""
    out = Counter()
    ods = [motif_as_oracle_dict(m) for m in motifs]
    cache = [{} for _ in motifs]

    def score(m, k):
        s = cache[m].get(k)
        if s is None:
            s = cache[m][k] = int_score(k, np.asarray(ods[m]["score_matrix"], dtype=np.int64), ods[m]["min_val"])
        return s

    for idx in {id(e[0]): e[0] for e in entries}.values():
        mine = [x for x in _listings(entries) if x[1] is idx]
        H = int(idx.n_haplotypes) if idx.alt_bits is not None else 0
        L = len(idx.ref)
        if memo:
            first, cls = haplotype_classes(idx)
            todo = list(zip(first.tolist(), np.bincount(cls, minlength=len(first)).tolist()))
        else:
            todo = [(h, 1) for h in range(H)]
        for h, times in todo:
            seq, coord, ins, _, _ = spell(idx, h)
            inst = []                                          # (start of '+', stop of '+', key)
            for m, od in enumerate(ods):
                W = od["width"]
                for o in range(0, len(seq) - W + 1):
                    start = coord[o] + (1 if ins[o] else 0)
                    stop = coord[o + W - 1] + 1
                    kmer = bytes(seq[o:o + W])
                    if score(m, kmer) >= cutoffs[m]:
                        inst.append((start, stop, (m, start, stop, "+", kmer.decode())))
                    if not forward_only:
                        rk = revcomp(kmer)
                        if score(m, rk) >= cutoffs[m]:
                            inst.append((start, stop, (m, stop, start, "-", rk.decode())))
            for listing, _, S, E in mine:
                sel = [x for x in inst if max(S, 0) <= x[0] < min(E, L) and x[1] <= min(E, L)]
                _count_pairs(out, listing, [x[2] for x in sel], [min(x[0], x[1]) for x in sel], [max(x[0], x[1]) for x in sel],
                             min_gap, max_gap, times)
    return out


def enumerator_pairs(entries, motifs, cutoffs, min_gap, max_gap, forward_only=False, recomb=False):
    """the same Counter from the walk enumerator: every walk-level row with the AND of its constraints' carrier sets, the
    pairs of pairs_reference, joint summed per key pair -> (Counter, walk-level pairs)"""
    out = Counter()
    n_pairs = 0
    for listing, idx, S, E in _listings(entries):
        H = int(idx.n_haplotypes)
        keys, lo, hi, car = [], [], [], []
        for m, motif in enumerate(motifs):
            od = motif_as_oracle_dict(motif)
            rows = walk_rows(idx, [(S, E)], od["width"], od["score_matrix"], od["min_val"], cutoffs[m], forward_only, recomb)
            for (_, a, b, strand, seq, slots), times in rows.items():
                acc = np.ones(H, bool)
                for sl in slots:
                    acc &= _carriers(idx, sl >> 2, sl & 3)
                for _ in range(times):
                    keys.append((m, a, b, strand, seq))
                    lo.append(min(a, b))
                    hi.append(max(a, b))
                    car.append(acc)
        if len(keys) < 2:
            continue
        a, b, joint, _ = pairs_reference(np.zeros(len(keys), np.int64), lo, hi, pack(np.array(car)), min_gap, max_gap)
        n_pairs += len(a)
        for i, j, w in zip(a.tolist(), b.tolist(), joint.tolist()):
            ka, kb = keys[i], keys[j]
            out[(listing,) + ((ka, kb) if ka <= kb else (kb, ka))] += w
    return out, n_pairs


def table_rows(hp):
    """the rows of every motif's table as arrays: (motif, row, listing, lo, hi, masks, is_ref), carriers or not"""
    motif, row, listing, lo, hi, masks, ref = [], [], [], [], [], [], []
    for m, t in enumerate(hp.tables):
        n = len(t)
        start, stop = t.report["start"].to_numpy(np.int64), t.report["stop"].to_numpy(np.int64)
        motif.append(np.full(n, m, np.int64))
        row.append(np.arange(n, dtype=np.int64))
        listing.append(np.asarray(t.row_region, np.int64))
        lo.append(np.minimum(start, stop))
        hi.append(np.maximum(start, stop))
        masks.append(np.asarray(t.carrier_bits, np.uint64).reshape(n, (len(t.haplotype_names) + 63) // 64))
        ref.append(t.report["reference"].to_numpy() == "ref")
    return (np.concatenate(motif), np.concatenate(row), np.concatenate(listing), np.concatenate(lo), np.concatenate(hi),
            np.concatenate(masks, axis=0), np.concatenate(ref))


def check_pairs(hp, entries, motifs, args, min_gap, max_gap, groups=None, chrom_names=None, memo=False):
    """every check of one HitPairs -> the number of pairs.  entries: [(GraphIndex, regions)] in the caller's order; groups:
    {name: [haplotype columns]} or None; `memo` goes to haplotype_pairs"""
    P = len(hp)
    H = int(entries[0][0].n_haplotypes)
    motif, row, listing, lo, hi, masks, ref = table_rows(hp)
    first = np.concatenate([[0], np.cumsum([len(t) for t in hp.tables])])
    ia, ib = first[hp.motif_a] + hp.row_a, first[hp.motif_b] + hp.row_b
    # the listings and their names
    flat = _listings(entries)
    names = [f"{(chrom_names[k] if chrom_names else None) or idx.chrom}:{S}-{E}"
             for k, (idx, regions) in enumerate(entries) for S, E in regions]
    assert list(hp.region_names) == names
    for m, t in enumerate(hp.tables):
        assert t.row_region.shape == (len(t),) and t.row_region.dtype == np.int64
        if len(t):
            assert t.row_region.min() >= 0 and t.row_region.max() < len(flat)
            assert np.array_equal(hp.region_names[t.row_region], t.report["sequence_name"].to_numpy())
    # every pair on its own: two distinct rows of one listing, the gap, the joint and group counts from the carrier bits
    assert (ia != ib).all()
    assert np.array_equal(listing[ia], hp.region) and np.array_equal(listing[ib], hp.region)
    gap = np.maximum(lo[ia], lo[ib]) - np.minimum(hi[ia], hi[ib])
    assert np.array_equal(gap, hp.gap) and (gap >= min_gap).all() and (gap <= max_gap).all()
    both = masks[ia] & masks[ib]
    assert hp.co_haplotypes.dtype == np.int32 and np.array_equal(popcount_rows(both), hp.co_haplotypes)
    assert (hp.co_haplotypes > 0).all()
    names_g = list(groups) if groups else []
    assert hp.group_names == names_g and hp.group_counts.shape == (P, len(names_g))
    car = unpack(both, H)
    for g, who in enumerate((groups or {}).values()):
        member = np.zeros(H, bool)
        member[list(who)] = True
        assert np.array_equal(hp.group_counts[:, g], (car & member).sum(axis=1)), names_g[g]
    assert np.array_equal(hp.reference, ref[ia] & ref[ib])
    # the order: key(a) < key(b), the pairs strictly ascending by (key(a), key(b)) -- so no pair twice
    key = lambda i: list(zip(listing[i].tolist(), lo[i].tolist(), hi[i].tolist(), motif[i].tolist(), row[i].tolist()))      # noqa: E731
    ka, kb = key(ia), key(ib)
    assert all(x < y for x, y in zip(ka, kb))
    both_keys = list(zip(ka, kb))
    assert all(x < y for x, y in zip(both_keys, both_keys[1:]))
    # the table is exactly the contract's join over the tables' rows
    ea, eb, ej, _ = pairs_reference(listing, lo, hi, masks, min_gap, max_gap, tie=(motif, row))
    assert np.array_equal(ea, ia) and np.array_equal(eb, ib) and np.array_equal(ej, hp.co_haplotypes)
    # the haplotype brute force: per key pair the sum of co_haplotypes is the number of instance pairs over the haplotypes
    cutoffs = [report_cutoff(m, args, t.report) for m, t in zip(motifs, hp.tables)]
    exp = haplotype_pairs(entries, motifs, cutoffs, min_gap, max_gap, args.noreverse, memo=memo)
    got = Counter()
    cols = [(t.report["start"].tolist(), t.report["stop"].tolist(), t.report["strand"].tolist(),
             t.report["matched_sequence"].tolist()) for t in hp.tables]
    k_of = lambda m, r: (m, int(cols[m][0][r]), int(cols[m][1][r]), cols[m][2][r], cols[m][3][r])      # noqa: E731
    for p in range(P):
        a, b = k_of(int(hp.motif_a[p]), int(hp.row_a[p])), k_of(int(hp.motif_b[p]), int(hp.row_b[p]))
        got[(int(hp.region[p]),) + ((a, b) if a <= b else (b, a))] += int(hp.co_haplotypes[p])
    assert set(got) == set(exp), (sorted(set(got) - set(exp))[:3], sorted(set(exp) - set(got))[:3])
    for k, v in exp.items():
        assert got[k] == v, (k, got[k], v)
    return P
