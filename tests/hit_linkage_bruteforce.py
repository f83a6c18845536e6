"""Expected sides of the hit-linkage table (grafimo_amd/hit_linkage.py) -- TEST INFRASTRUCTURE ONLY, no kernel runs here.

  * links_reference: a plain numpy / Python restatement of the contract on arrays (rows, sites, bitsets), with Python ints
    for Dn and den and one float division per candidate.
  * synthetic_input: rows and sites made so that links exist (rows that copy a nearby allele's carriers, noisily).
  * check_linkage: a HitLinkage against links_reference over the table's own rows and the index's bitsets, against
    variant_effects._site_columns, the report, the HitAlleles CSR and np.corrcoef."""
import math

import numpy as np

from hit_pair_bruteforce import pack, popcount_rows


def unpack_bits(words, H):
    """uint64 [..., hw] -> bool [..., H]"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[:-1] + (8 * words.shape[-1],)), axis=-1, bitorder="little")
    return bits[..., :H].astype(bool)


def ld_of_counts(H, n_hit, n_allele, n_joint):
    """-> None where the LD is undefined, else (r2, r, d_prime) by the contract's formulas on Python ints"""
    H, nh, na, nj = int(H), int(n_hit), int(n_allele), int(n_joint)
    Dn = H * nj - nh * na
    den = nh * (H - nh) * na * (H - na)
    if den == 0:
        return None
    r2 = float(Dn * Dn) / float(den)
    r = math.copysign(math.sqrt(r2), Dn) if Dn else 0.0
    if Dn > 0:
        dmax = min(nh * (H - na), (H - nh) * na)
    else:
        dmax = min(nh * na, (H - nh) * (H - na))
    return r2, r, (Dn / dmax if Dn else 0.0)


def links_reference(lo, hi, masks, pos, n_alts, allele_bits, flank, min_r2, H):
    """-> (row, site, allele, n_joint, n_hit [rows], n_allele, r2, r, d_prime, candidates): the links ascending by
    (row, site, allele) in the caller's indices; `candidates` counts the cells within the flank (defined or not)"""
    lo, hi, pos = np.asarray(lo, np.int64), np.asarray(hi, np.int64), np.asarray(pos, np.int64)
    n_alts = np.asarray(n_alts, np.int64)
    masks = np.asarray(masks, np.uint64)
    masks = masks.reshape(len(lo), masks.shape[-1])
    allele_bits = np.asarray(allele_bits, np.uint64).reshape(len(pos), 3, masks.shape[-1])
    n_hit = popcount_rows(masks) if len(lo) else np.zeros(0, np.int64)
    out = []
    candidates = 0
    n_allele = popcount_rows(allele_bits) if len(pos) else np.zeros((0, 3), np.int64)
    for i in range(len(lo)):
        dist = np.maximum(np.maximum(lo[i] - pos, pos - (hi[i] - 1)), 0)
        cand = np.flatnonzero(dist <= flank)
        joint = popcount_rows(allele_bits[cand] & masks[i][None, None, :]) if len(cand) else None
        for c, s in enumerate(cand.tolist()):
            for a in range(1, int(n_alts[s]) + 1):
                candidates += 1
                na, nj = int(n_allele[s, a - 1]), int(joint[c, a - 1])
                ld = ld_of_counts(H, n_hit[i], na, nj)
                if ld is not None and ld[0] >= min_r2:
                    out.append((i, s, a, nj, na) + ld)
    col = lambda k, dt: np.array([x[k] for x in out], dtype=dt)      # noqa: E731
    return (col(0, np.int64), col(1, np.int64), col(2, np.uint8), col(3, np.int32), n_hit.astype(np.int32), col(4, np.int32),
            col(5, np.float64), col(6, np.float64), col(7, np.float64), candidates)


def synthetic_input(seed, H, n_rows=300, n_sites=400, span=3000, near=60):
    """-> (lo, hi, masks, pos, n_alts, allele_bits): sites at random positions of 0 .. span - 1 (equal positions happen),
    1 - 3 ALTs with disjoint carriers, a tenth of the sites carried by nobody, the unused slots full of garbage; rows of
    width 4 - 20, about 60 % of them with the carriers of an allele within `near` bases -- half of these complemented --
    and 5 % of the bits flipped, the rest random; about 5 % carried by everybody and 5 % by nobody."""
    rng = np.random.default_rng(seed)
    hw = (H + 63) // 64
    pos = np.sort(rng.integers(0, span, n_sites)).astype(np.int64)
    n_alts = rng.integers(1, 4, n_sites).astype(np.uint8)
    member = np.zeros((n_sites, 3, H), dtype=bool)
    for s in range(n_sites):
        af = 0.0 if rng.random() < 0.1 else rng.random() ** 1.5
        a = np.where(rng.random(H) < af, rng.integers(1, int(n_alts[s]) + 1, H), 0)
        for k in range(int(n_alts[s])):
            member[s, k] = a == k + 1
    bits = pack(member.reshape(n_sites * 3, H)).reshape(n_sites, 3, hw)
    garbage = rng.integers(0, 2 ** 63, (n_sites, 3, hw), dtype=np.uint64) | np.uint64(1 << 63)
    unused = np.arange(3)[None, :] >= n_alts[:, None]
    bits[unused] = garbage[unused]
    lo = rng.integers(0, span, n_rows).astype(np.int64)
    hi = lo + rng.integers(4, 21, n_rows)
    rows = np.zeros((n_rows, H), dtype=bool)
    for i in range(n_rows):
        close = np.flatnonzero(np.abs(pos - lo[i]) <= near)
        if rng.random() < 0.6 and len(close):
            s = int(rng.choice(close))
            v = member[s, int(rng.integers(0, int(n_alts[s])))].copy()
            if rng.random() < 0.5:
                v = ~v
            v ^= rng.random(H) < 0.05
        else:
            v = rng.random(H) < rng.random()
        u = rng.random()
        rows[i] = True if u < 0.05 else False if u < 0.10 else v
    return lo, hi, pack(rows), pos, n_alts, bits


def check_linkage(hl, entries, flank, min_r2):
    """`hl`: a HitLinkage; `entries`: per chromosome entry its GraphIndex (None for an entry without regions) -> the number
    of links.  Everything exact but the comparison with np.corrcoef (1e-12: it checks the formula, not the table)."""
    from grafimo_amd.graph_tables import _site_columns
    t = hl.table
    rep = t.report
    H = len(t.haplotype_names)
    n = len(rep)
    start, stop = rep["start"].to_numpy(np.int64), rep["stop"].to_numpy(np.int64)
    lo, hi = np.minimum(start, stop), np.maximum(start, stop)
    freq = rep["haplotype_frequency"].to_numpy(np.int64)
    row_entry = np.asarray(t.row_entry, np.int64)
    assert row_entry.shape == (n,)
    L = len(hl)
    for k in ("row", "site", "allele", "entry", "distance", "n_joint", "n_allele", "n_hit", "r2", "r", "d_prime", "in_hit"):
        assert getattr(hl, k).shape == (L,), k
    # the order: strictly ascending (row, site, allele)
    key = list(zip(hl.row.tolist(), hl.site.tolist(), hl.allele.tolist()))
    assert all(a < b for a, b in zip(key, key[1:]))
    assert np.array_equal(hl.entry, row_entry[hl.row]) and np.array_equal(hl.n_hit, freq[hl.row])
    seen = 0
    for e, idx in enumerate(entries):
        rows = np.flatnonzero(row_entry == e)
        sel = np.flatnonzero(hl.entry == e)
        if idx is None:
            assert not len(rows) and not len(sel)
            continue
        assert t.indexes[e] is not None and np.array_equal(np.asarray(t.indexes[e].pos), np.asarray(idx.pos))
        row, site, allele, nj, nh, na, r2, r, dp, _ = links_reference(lo[rows], hi[rows], t.carrier_bits[rows], idx.pos, idx.n_alts,
                                                                      idx.alt_bits, flank, min_r2, H)
        assert np.array_equal(nh, freq[rows])
        assert np.array_equal(hl.row[sel], rows[row]) and np.array_equal(hl.site[sel], site) and np.array_equal(hl.allele[sel], allele)
        assert np.array_equal(hl.n_joint[sel], nj) and np.array_equal(hl.n_allele[sel], na)
        assert np.array_equal(hl.r2[sel], r2) and np.array_equal(hl.r[sel], r) and np.array_equal(hl.d_prime[sel], dp)
        assert (hl.r2[sel] >= min_r2).all()
        if len(sel):
            assert np.array_equal(hl.n_allele[sel], _site_columns(idx, site, allele.astype(np.int64))[4])
            p = np.asarray(idx.pos, np.int64)[site]
            r_of = hl.row[sel]
            assert np.array_equal(hl.distance[sel], np.maximum(np.maximum(lo[r_of] - p, p - (hi[r_of] - 1)), 0))
            assert (hl.distance[sel] <= flank).all()
            C = unpack_bits(t.carrier_bits[r_of], H).astype(np.float64)
            A = unpack_bits(np.asarray(idx.alt_bits, np.uint64)[site, allele.astype(np.int64) - 1], H).astype(np.float64)
            for k in range(len(sel)):
                cc = np.corrcoef(C[k], A[k])[0, 1]
                assert abs(cc * cc - r2[k]) <= 1e-12 and (cc > 0) == (r[k] > 0)
        seen += len(sel)
    assert seen == L
    own = set()
    for i in range(n):
        own.update((i, ent, s, a) for ent, s, a in t.alleles(i))
    assert hl.in_hit.tolist() == [(i, e, s, a) in own for i, e, s, a in zip(hl.row.tolist(), hl.entry.tolist(), hl.site.tolist(),
                                                                              hl.allele.tolist())]
    return L
