"""Expected sides of the per-hit allele table (grafimo_amd/hit_alleles.py) -- TEST INFRASTRUCTURE ONLY.

Three independent views of one table, none of which runs a kernel:
  * carrier_counts: the haplotype brute force -- every haplotype spelled (variant_bruteforce.spell), every offset's row under
    the report's region rule exactly as haplotype_bruteforce.haplotype_matrix takes it, rows at or above the report's integer
    cutoff counted per key (region name, start, stop, strand, k-mer as printed) and haplotype.  No walk enumeration.
  * walk_rows: the walk enumerator (variant_walks.window_walks) -- every walk of every window of every region with the set
    of (site, allele) constraints its choices put on the haplotypes, one row per strand that passes the cutoff, carried by
    some haplotype unless --recomb.
  * first principles per row: the AND of variant_walks._carriers over the row's alleles.
check_table runs all of them against a HitAlleles; every row and every key takes part."""
from collections import Counter

import numpy as np

from extract_helpers import motif_as_oracle_dict
from haplotype_bruteforce import integer_cutoff
from variant_bruteforce import haplotype_classes, int_score, revcomp, spell
from variant_walks import _carriers, window_walks


def report_cutoff(motif, args, report=None):
    """the report's integer cutoff: the lowest score with p < threshold; under --qvalueT the lowest score among the report's
    rows (q falls as the score rises; no row: nothing passes)"""
    from oracle import oracle as orc
    od = motif_as_oracle_dict(motif)
    if not args.qvalueT:
        return integer_cutoff(orc.p_table(od["pmf"]), args.threshold)
    if report is None or not len(report):
        return len(od["pmf"])
    sc = np.rint((report["score"].to_numpy(float) - od["width"] * od["offset"]) * od["scale"]).astype(np.int64)
    assert np.array_equal(sc / od["scale"] + od["width"] * od["offset"], report["score"].to_numpy(float))
    return int(sc.min())


def region_name(idx, region, chrom=None):
    return f"{chrom or idx.chrom}:{region[0]}-{region[1]}"


def carrier_counts(idx, regions, W, sm, min_val, cutoff, forward_only=False, chrom=None, memo=False):
    """-> {(region name, start, stop, strand, k-mer as printed): int64 [H] rows of haplotype h with that key}.  `memo`: one
    haplotype per class of variant_bruteforce.haplotype_classes, its counts copied to the class (the same result)."""
    sm = np.asarray(sm, dtype=np.int64)
    H = int(idx.n_haplotypes) if idx.alt_bits is not None else 0
    L = len(idx.ref)
    out = {}
    cache = {}

    def score(k):
        s = cache.get(k)
        if s is None:
            s = cache[k] = int_score(k, sm, min_val)
        return s

    first, cls = haplotype_classes(idx) if memo else (np.arange(H), np.arange(H))
    for c, h in enumerate(first.tolist()):
        seq, coord, ins, _, _ = spell(idx, h)
        for o in range(0, len(seq) - W + 1):
            start = coord[o] + (1 if ins[o] else 0)
            stop = coord[o + W - 1] + 1
            kmer = bytes(seq[o:o + W])
            rows = [(start, stop, "+", kmer)] + ([] if forward_only else [(stop, start, "-", revcomp(kmer))])
            rows = [r for r in rows if score(r[3]) >= cutoff]
            if not rows:
                continue
            for S, E in regions:
                if not (max(S, 0) <= start < min(E, L) and stop <= min(E, L)):
                    continue
                for a, b, strand, printed in rows:
                    key = (region_name(idx, (S, E), chrom), a, b, strand, printed.decode())
                    v = out.get(key)
                    if v is None:
                        v = out[key] = np.zeros(len(first), dtype=np.int64)
                    v[c] += 1
    return {key: v[cls] for key, v in out.items()}


def walk_rows(idx, regions, W, sm, min_val, cutoff, forward_only=False, recomb=False, chrom=None):
    """-> Counter of (region name, start, stop, strand, k-mer as printed, frozenset(site * 4 + allele)) over the enumerator's
    walks, a row per strand at or above the cutoff; without `recomb` only walks some haplotype carries"""
    sm = np.asarray(sm, dtype=np.int64)
    H = int(idx.n_haplotypes) if idx.alt_bits is not None else 0
    L = len(idx.ref)
    tail = 1 if (np.asarray(idx.ins_len) > 0).any() else W
    car = {}
    out = Counter()
    for S, E in regions:
        s, e = max(S, 0), min(E, L)
        for p in range(s, e - tail + 1):
            for kmer, stop, slots in window_walks(idx, p, W, e):
                if not recomb:
                    acc = np.ones(H, bool)
                    for sl in slots:
                        if sl not in car:
                            car[sl] = _carriers(idx, sl >> 2, sl & 3)
                        acc &= car[sl]
                    if not acc.any():
                        continue
                name = region_name(idx, (S, E), chrom)
                if int_score(kmer, sm, min_val) >= cutoff:
                    out[(name, p, stop, "+", kmer.decode(), frozenset(slots))] += 1
                if not forward_only:
                    rk = revcomp(kmer)
                    if int_score(rk, sm, min_val) >= cutoff:
                        out[(name, stop, p, "-", rk.decode(), frozenset(slots))] += 1
    return out


def unpack(bits, H):
    """uint64 [n, hw] -> bool [n, H]"""
    b = np.ascontiguousarray(bits)
    return np.unpackbits(b.view(np.uint8).reshape(len(b), 8 * b.shape[1]), axis=1, bitorder="little")[:, :H].astype(bool)


def check_first_principles(ha, idx, groups=None):
    """check 4, every row: the AND of the alleles' carrier sets is carrier_bits; its popcount is haplotype_frequency; the
    group counts; a `ref` row has no ALT allele; no tail bit; the alleles a sorted set"""
    H = int(idx.n_haplotypes)
    n = len(ha)
    assert ha.carrier_bits is not None and ha.carrier_bits.shape == (n, (H + 63) // 64) and ha.carrier_bits.dtype == np.uint64
    assert ha.allele_offsets.shape == (n + 1,) and ha.allele_offsets[0] == 0 and ha.allele_offsets[-1] == len(ha.allele)
    assert ha.allele_offsets.dtype == np.int64 and ha.allele_site.dtype == np.int32 and ha.allele.dtype == np.uint8
    assert ha.allele_entry.dtype == np.int32 and ha.group_counts.dtype == np.int32
    car = unpack(ha.carrier_bits, H)
    if H & 63:
        assert not (ha.carrier_bits[:, -1] >> np.uint64(H & 63)).any()
    freq = ha.report["haplotype_frequency"].to_numpy()
    assert np.array_equal(car.sum(axis=1), freq)
    cache = {}
    for r in range(n):
        al = ha.alleles(r)
        keys = [(s, a) for _, s, a in al]
        assert keys == sorted(set(keys)), (r, keys)
        acc = np.ones(H, bool)
        for _, s, a in al:
            if (s, a) not in cache:
                cache[(s, a)] = _carriers(idx, s, a)
            acc &= cache[(s, a)]
        assert np.array_equal(acc, car[r]), (r, al)
        if ha.report["reference"].iat[r] == "ref":
            assert all(a == 0 for _, _, a in al), (r, al)
    if groups is not None:
        assert ha.group_names == list(groups) and ha.group_counts.shape == (n, len(groups))
        for g, who in enumerate(groups.values()):
            member = np.zeros(H, bool)
            member[list(who)] = True
            assert np.array_equal(ha.group_counts[:, g], (car & member).sum(axis=1)), list(groups)[g]
    return car


def check_against_haplotypes(ha, car, idx, regions, motif, cutoff, forward_only, chrom=None, memo=False):
    """check 2: per key the sum over the table's rows of the carrier bits equals the haplotype brute force's count, and the
    keys of the rows with carriers are exactly its keys"""
    od = motif_as_oracle_dict(motif)
    exp = carrier_counts(idx, regions, od["width"], od["score_matrix"], od["min_val"], cutoff, forward_only, chrom, memo=memo)
    got = {}
    rep = ha.report
    for r, (name, a, b, strand, seq, f) in enumerate(zip(rep["sequence_name"], rep["start"], rep["stop"], rep["strand"],
                                                         rep["matched_sequence"], rep["haplotype_frequency"])):
        if f == 0:
            assert not car[r].any()
            continue
        key = (name, int(a), int(b), strand, seq)
        got[key] = got.get(key, 0) + car[r].astype(np.int64)
    # (a region listed twice: its rows are in the report twice, and the brute force counted every listing)
    assert set(got) == set(exp), (sorted(set(got) - set(exp))[:3], sorted(set(exp) - set(got))[:3])
    for key, v in exp.items():
        assert np.array_equal(got[key], v), key
    return len(exp)


def check_against_walks(ha, idx, regions, motif, cutoff, forward_only, recomb, chrom=None):
    """check 3: the multiset of (region, start, stop, strand, k-mer, constraint set) of the table's rows is the enumerator's"""
    od = motif_as_oracle_dict(motif)
    exp = walk_rows(idx, regions, od["width"], od["score_matrix"], od["min_val"], cutoff, forward_only, recomb, chrom)
    got = Counter()
    rep = ha.report
    for r, (name, a, b, strand, seq) in enumerate(zip(rep["sequence_name"], rep["start"], rep["stop"], rep["strand"],
                                                      rep["matched_sequence"])):
        got[(name, int(a), int(b), strand, seq, frozenset(4 * s + al for _, s, al in ha.alleles(r)))] += 1
    if got != exp:
        only_got, only_exp = got - exp, exp - got
        raise AssertionError(f"rows only in the table: {sorted(only_got.items(), key=str)[:3]}; "
                             f"only in the enumerator: {sorted(only_exp.items(), key=str)[:3]}")
    return sum(exp.values())


def check_table(ha, idx, regions, motif, args, groups=None, chrom=None, memo=False):
    """checks 2, 3 and 4 of one table (made with carriers=True) -> (rows, keys); `memo` goes to carrier_counts"""
    car = check_first_principles(ha, idx, groups)
    cutoff = report_cutoff(motif, args, ha.report)
    keys = check_against_haplotypes(ha, car, idx, regions, motif, cutoff, args.noreverse, chrom, memo=memo)
    rows = check_against_walks(ha, idx, regions, motif, cutoff, args.noreverse, args.recomb, chrom)
    assert rows == len(ha)
    return rows, keys
