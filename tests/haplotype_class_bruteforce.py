"""Brute force for the haplotype class table (grafimo_amd/haplotype_classes.py) -- TEST INFRASTRUCTURE ONLY.

It states the rule a second time, site by site and independently of region_sites: the sites of region [S, E) clipped to the
chromosome are the substitutions with S <= pos < E, the insertions with S - 1 <= pos < E and the deletions of d bases with
pos + 1 < E and pos + d >= S; an empty region has none.  The classes of a region are np.unique over the rows of the unpacked
allele matrix of those sites (a row per haplotype, a column per (site, ALT slot) with the unused slots cleared), numbered by
count descending, then by smallest member."""
import numpy as np


def sites_of_region(idx, S, E):
    S, E = max(int(S), 0), min(int(E), len(idx.ref))
    out = []
    if E <= S:
        return out
    for i in range(len(idx.pos)):
        p, d, n = int(idx.pos[i]), int(idx.del_len[i]), int(idx.ins_len[i])
        if d > 0:
            keep = p + 1 < E and p + d >= S
        elif n > 0:
            keep = S - 1 <= p < E
        else:
            keep = S <= p < E
        if keep:
            out.append(i)
    return out


def allele_matrix(idx, sites):
    """-> uint8 [H, len(sites), 3]: haplotype h has ALT k + 1 of the site (the slots beyond n_alts are 0)"""
    H = int(idx.n_haplotypes)
    if not len(sites):
        return np.zeros((H, 0, 3), dtype=np.uint8)
    bits = np.unpackbits(np.ascontiguousarray(np.asarray(idx.alt_bits, dtype=np.uint64)[sites]).view(np.uint8), axis=-1,
                         bitorder="little")[..., :H]                     # [n, 3, H]
    used = np.arange(3)[None, :] < np.asarray(idx.n_alts, dtype=np.int64)[sites][:, None]
    return np.ascontiguousarray((bits * used[..., None]).transpose(2, 0, 1))


def region_classes(idx, S, E, entry=0, groups=()):
    """-> dict: sites, class_of int64 [H], count, first int64 [n], is_reference bool [n], alleles (per class the
    [(entry, site, allele)] of its smallest member's ALTs), group_counts int64 [n, G] (`groups`: lists of haplotype indices)"""
    H = int(idx.n_haplotypes)
    sites = sites_of_region(idx, S, E)
    m = allele_matrix(idx, sites)
    _, first, inv, count = np.unique(m.reshape(H, -1), axis=0, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.lexsort((first, -count))                                  # count descending, then the smallest member
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    class_of = rank[inv]
    first, count = first[order].astype(np.int64), count[order].astype(np.int64)
    alleles = [[(entry, sites[j], a + 1) for j in range(len(sites)) for a in range(3) if m[f, j, a]] for f in first.tolist()]
    gc = np.zeros((len(first), len(groups)), dtype=np.int64)
    for g, who in enumerate(groups):
        who = np.unique(np.asarray(list(who), dtype=np.int64))
        gc[:, g] = np.bincount(class_of[who], minlength=len(first))
    return {"sites": sites, "class_of": class_of, "count": count, "first": first,
            "is_reference": np.array([not a for a in alleles], dtype=bool), "alleles": alleles, "group_counts": gc}


def check_classes(hc, per_region, ctx=None):
    """a HaplotypeClasses against the region_classes dicts of its regions, everything exactly equal"""
    assert len(per_region) == len(hc.n_classes), ctx
    is_ref = hc.is_reference
    for r, exp in enumerate(per_region):
        a, b = int(hc.offsets[r]), int(hc.offsets[r + 1])
        assert int(hc.n_classes[r]) == len(exp["count"]) == b - a, (ctx, r, int(hc.n_classes[r]), len(exp["count"]))
        assert np.array_equal(hc.class_of[r], exp["class_of"]), (ctx, r)
        assert np.array_equal(hc.count[a:b], exp["count"]) and np.array_equal(hc.first[a:b], exp["first"]), (ctx, r)
        assert np.array_equal(is_ref[a:b], exp["is_reference"]), (ctx, r)
        assert np.array_equal(hc.group_counts[a:b], exp["group_counts"]), (ctx, r)
        for k in range(b - a):
            assert hc.alleles(r, k) == exp["alleles"][k], (ctx, r, k)
