"""Haplotype brute force for the per-variant effect table (grafimo_amd/variant_effects.py) -- TEST INFRASTRUCTURE ONLY.

Built from a GraphIndex's arrays alone, with no walk enumeration: every haplotype is spelled from the reference and the
alleles its bitsets give it, every base remembering its reference coordinate and whether it was inserted; every allele
of every site leaves its FOOTPRINT on the spelled bases:
  * substitution site, allele a (0 = none of the ALTs): the base at the site's position;
  * deletion d not carried: every (not inserted) base inside the deleted span; carried: the JUNCTION, the anchor base and
    the base behind it;
  * insertion k carried: its inserted bases; not carried: the junction (anchor and the base behind it) -- unless the
    haplotype reads an insertion earlier in site order at that anchor (a walk that reads it never passes k by).
A window of W consecutive bases qualifies for every (site, allele) whose footprint it covers (a junction: both bases);
the region rule is the report's (start in [S, E), stop <= E); the score is the oracle's integer score of the k-mer as
printed for its strand; the best hit is the first under (-score, start, stop, strand '+' first, k-mer).
"""
from bisect import bisect_left
from typing import Dict, Tuple

import numpy as np

_COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")
_CODE = np.full(256, -1, dtype=np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def carries(idx, i: int, k: int, h: int) -> bool:
    if idx.alt_bits is None:
        return False
    return bool((int(idx.alt_bits[i, k, h >> 6]) >> (h & 63)) & 1)


def spell(idx, h: int):
    """-> (bases bytearray, coord list, inserted list, single tags [(base index, slot)], junction tags [(anchor index, slot)])
    with slot = site * 4 + allele."""
    ref = bytes(np.asarray(idx.ref, dtype=np.uint8))
    by_pos: Dict[int, list] = {}
    for i in range(len(idx.pos)):
        by_pos.setdefault(int(idx.pos[i]), []).append(i)
    out, coord, ins = bytearray(), [], []
    single, junction = [], []
    # (first, last deleted coordinate, site) of the deletions this haplotype does NOT carry -- also those anchored on bases
    # another deletion it carries removes: their bases behind that one's span are there
    del_span = [(int(idx.pos[i]) + 1, int(idx.pos[i]) + int(idx.del_len[i]), i)
                for i in range(len(idx.pos)) if idx.del_len[i] > 0 and not carries(idx, i, 0, h)]
    x, L = 0, len(ref)
    while x < L:
        sites = by_pos.get(x, [])
        b = ref[x]
        bi = len(out)
        for i in sites:
            if idx.del_len[i] == 0 and idx.ins_len[i] == 0:
                a = next((k + 1 for k in range(int(idx.n_alts[i])) if carries(idx, i, k, h)), 0)
                if a:
                    b = int(idx.alt_bases[i, a - 1])
                single.append((bi, 4 * i + a))
        out.append(b); coord.append(x); ins.append(False)
        read = None
        for i in sites:
            if idx.ins_len[i] > 0:
                if read is None and carries(idx, i, 0, h):
                    read = i
                elif read is None:
                    junction.append((bi, 4 * i))
        jump = None
        for i in sites:
            if idx.del_len[i] > 0:
                if read is None and jump is None and carries(idx, i, 0, h):
                    jump = i
        if read is not None:
            o, n = int(idx.ins_off[read]), int(idx.ins_len[read])
            for t in range(n):
                single.append((len(out), 4 * read + 1))
                out.append(int(idx.ins_bases[o + t])); coord.append(x); ins.append(True)
        if jump is not None:
            junction.append((bi, 4 * jump + 1))
            x += int(idx.del_len[jump]) + 1
        else:
            x += 1
    # the REF footprint of the deletions not carried: their bases that are there
    pos_of = {}
    for j, (c, t) in enumerate(zip(coord, ins)):
        if not t:
            pos_of[c] = j
    for lo, hi, i in del_span:
        for c in range(lo, hi + 1):
            if c in pos_of:
                single.append((pos_of[c], 4 * i))
    single.sort()
    junction.sort()
    return out, coord, ins, single, junction


def haplotype_classes(idx):
    """-> (one haplotype of every class, the class of every haplotype): haplotypes with the same allele at every site spell
    the same sequence, so a brute force may spell one per class (graphs of thousands of haplotypes over a few sites)"""
    H = int(idx.n_haplotypes) if idx.alt_bits is not None else 0
    if not H or not len(idx.pos):
        return np.zeros(min(H, 1), dtype=np.int64), np.zeros(H, dtype=np.int64)
    bits = np.unpackbits(np.ascontiguousarray(idx.alt_bits).view(np.uint8), axis=-1, bitorder="little")[..., :H]
    used = np.arange(bits.shape[1])[None, :] < np.asarray(idx.n_alts, dtype=np.int64)[:, None]
    alleles = (bits * used[..., None]).reshape(-1, H).T
    _, first, inv = np.unique(alleles, axis=0, return_index=True, return_inverse=True)
    return first.astype(np.int64), inv.reshape(-1).astype(np.int64)


def revcomp(k: bytes) -> bytes:
    return k.translate(_COMP)[::-1]


def int_score(kmer: bytes, sm: np.ndarray, min_val: int) -> int:
    c = _CODE[np.frombuffer(kmer, dtype=np.uint8)]
    if (c < 0).any():
        return int(min_val)
    return int(sm[c, np.arange(len(kmer))].sum())


def best_hits(idx, regions, W: int, sm: np.ndarray, min_val: int, forward_only: bool = False, memo: bool = False):
    """-> {slot: (score, start, stop, strand, kmer bytes as printed)} over the haplotypes' windows in the regions.
    `memo`: one haplotype per class of haplotype_classes (the same result)."""
    sm = np.asarray(sm, dtype=np.int64)
    H = int(idx.n_haplotypes) if idx.alt_bits is not None else 0
    L = len(idx.ref)
    cand: Dict[Tuple[bytes, int, int], set] = {}
    for h in (haplotype_classes(idx)[0].tolist() if memo else range(H)):
        seq, coord, ins, single, junction = spell(idx, h)
        s_keys = [t[0] for t in single]
        j_keys = [t[0] for t in junction]
        n = len(seq)
        for o in range(0, n - W + 1):
            start = coord[o] + (1 if ins[o] else 0)
            stop = coord[o + W - 1] + 1
            slots = set()
            for a in range(bisect_left(s_keys, o), bisect_left(s_keys, o + W)):
                slots.add(single[a][1])
            for a in range(bisect_left(j_keys, o), bisect_left(j_keys, o + W - 1)):
                slots.add(junction[a][1])
            if not slots:
                continue
            ok = any(max(S, 0) <= start < min(E, L) and stop <= min(E, L) for S, E in regions)
            if not ok:
                continue
            cand.setdefault((bytes(seq[o:o + W]), start, stop), set()).update(slots)
    best: Dict[int, tuple] = {}
    for (kmer, start, stop), slots in cand.items():
        rows = [(int_score(kmer, sm, min_val), start, stop, "+", kmer)]
        if not forward_only:
            rk = revcomp(kmer)
            rows.append((int_score(rk, sm, min_val), stop, start, "-", rk))
        for r in rows:
            key = (-r[0], r[1], r[2], r[3] != "+", r[4])
            for s in slots:
                b = best.get(s)
                if b is None or key < (-b[0], b[1], b[2], b[3] != "+", b[4]):
                    best[s] = r
    return best


def expected_rows(idx, best, ptable, threshold: float, all_sites: bool):
    """-> {(site, alt): (ref side or None, alt side or None, effect)} the table's rows from best_hits()"""
    rows = {}
    for i in range(len(idx.pos)):
        na = 1 if (idx.del_len[i] or idx.ins_len[i]) else int(idx.n_alts[i])
        for a in range(1, na + 1):
            r, x = best.get(4 * i), best.get(4 * i + a)
            if r is None and x is None:
                continue
            pr = r is not None and ptable[r[0]] < threshold
            px = x is not None and ptable[x[0]] < threshold
            if not (all_sites or pr or px):
                continue
            rows[(i, a)] = (r, x, {(False, False): "none", (False, True): "gain", (True, False): "loss", (True, True): "both"}[(pr, px)])
    return rows
