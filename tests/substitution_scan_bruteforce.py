"""Brute force for the substitution scan (grafimo_amd/substitution_scan.py) -- TEST INFRASTRUCTURE ONLY.

THE RULE (include/grafimo_hip.h states it for the library; grafimo_amd/substitution_scan.py for the table).  For a sequence x
of n bases, a motif of width W, a strictly ascending list of lengths L0 < L1 < .. with every L in 1 .. 64, a base map f given
as four codes -- the images of A, C, G, T, each in 0 .. 3 for A, C, G, T; any map is allowed: fixed points, constant maps and
the identity included --, every length L of the list and every offset o in 0 .. n - 1:
  If o + L > n there is no edit: both keys and both sums of the cell are 0.
  Otherwise y = x[:o] + f(x[o:o+L]) + x[o+L:].  f is applied base by base.  Case is folded, as base_code does.
  A base that is not A/C/G/T maps to itself: unlike a deletion, a substituted N is NOT repaired.
  This is gfm_graph_query_edits' rule with lr = la = L at offset o, the alleles not trimmed.
    REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o + L - 1, n - W).  This is bit for bit the
    deletion scan's COVER column.
    ALT side (column SUB): the same starts in y.
  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
  A window that holds a base that is not A/C/G/T scores min_val on both strands.
  Per column, the best window by (score descending, s ascending, + before -), as the key
  ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. L - 1 on both sides.
  Key 0 means the side has no window.
  Per column, the exact uint64 sum of w[score] over the side's windows and strands.
  Under the identity map SUB == COVER in every cell.
  At L = 1, wherever x[o] is a base, SUB equals the mutation scan's column of the base f(x[o]), field for field.

For each (x, o, L) y is literally built and query_variant_bruteforce.side is called with l = L on x and on y: every touched
window of both is scored from the score matrix on both strands -- the kernel's prefix differences are never used -- and the
sums are Python integers.  A map is given here as its four letters, the images of A, C, G, T."""
import numpy as np

from deletion_scan_bruteforce import named  # noqa: F401  (a VCF row could name the block: the same question)
from mutation_scan_bruteforce import effect, key_of, region_sequences  # noqa: F401
from query_variant_bruteforce import hand_graph, side  # noqa: F401

NONE = [(None, 0), (None, 0)]                                    # the cell of a block that does not fit its sequence


def image(block: bytes, letters: str) -> bytes:
    """f of every base of the block: A/C/G/T in either case become the map's upper-case letter, any other byte stays"""
    assert len(letters) == 4 and set(letters) <= set("ACGT"), letters
    return block.translate(bytes.maketrans(b"ACGTacgt", (letters + letters).encode()))


def substituted(x: bytes, o: int, L: int, letters: str) -> bytes:
    return x[:o] + image(x[o:o + L], letters) + x[o + L:]


def changed(x: bytes, o: int, L: int, letters: str) -> int:
    """how many bases of the block differ after the map (case apart); 0 where the block does not fit"""
    if o + L > len(x):
        return 0
    block = x[o:o + L].upper()
    return sum(int(a != b) for a, b in zip(block, image(block, letters)))


def scan(x: bytes, W: int, sm, min_val: int, wtab, forward_only: bool, lengths, letters: str):
    """-> per length, per offset o, a list of two (best or None, sum): COVER, SUB; a best's second field is the start minus o"""
    out = []
    for L in lengths:
        rows = []
        for o in range(len(x)):
            if o + L > len(x):
                rows.append(list(NONE))
                continue
            rows.append([side(x, o, L, W, sm, min_val, wtab, forward_only),
                         side(substituted(x, o, L, letters), o, L, W, sm, min_val, wtab, forward_only)])
        out.append(rows)
    return out


def scan_arrays(seqs, W: int, sm, min_val: int, wtab, forward_only: bool, lengths, letters: str):
    """the sequences' scans as the kernel lays them out -> (keys [n_lengths][n_bases][2], sums [n_lengths][n_bases][2]) lists
    of Python integers"""
    keys, sums = [[] for _ in lengths], [[] for _ in lengths]
    for x in seqs:
        for k, rows in enumerate(scan(x, W, sm, min_val, wtab, forward_only, lengths, letters)):
            keys[k] += [[key_of(b) for b, _ in row] for row in rows]
            sums[k] += [[int(s) for _, s in row] for row in rows]
    return keys, sums


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def detail_rows(region_names, seqs, scans, coords_of, W: int, scale: int, offset: float, ptab, log2_offset: float, threshold: float,
                lengths, letters: str):
    """The detail rows of all_rows as dicts, in the frame's order: regions in order, a region's versions by number, its
    reference sequence last, offsets ascending, lengths ascending, the blocks that change a base alone.  `seqs`, `scans` (this
    module's scan()) and coords_of as mutation_scan_bruteforce.detail_rows takes them; the floats are made as the table documents
    them."""
    rows = []
    for r, region in enumerate(seqs):
        for d, sc in zip(region, scans[r]):
            coord = coords_of(r, d)
            x = d["bases"].upper()
            for o in range(len(x)):
                for k, L in enumerate(lengths):
                    moved = changed(x, o, L, letters)
                    if not moved:
                        continue
                    (rb, rs), (ab, as_) = sc[k][o]
                    y = substituted(x, o, L, letters)
                    e = dict(sequence_name=region_names[r], version=d["version"], haplotypes=d["count"], groups=list(d["group_counts"]),
                             is_reference=d["is_reference"], position=coord[o][0] + 1, inserted=coord[o][1], length=L,
                             named=named(coord, o, L), map=letters, replaced=x[o:o + L].decode(), replacement=y[o:o + L].decode(),
                             changed=moved, effect=effect(ptab, threshold, rb, ab))
                    for sd, best, total, text in (("ref", rb, rs, x), ("alt", ab, as_, y)):
                        e[sd + "_score"] = float(best[0]) / float(scale) + float(W) * offset if best else float("nan")
                        e[sd + "_pvalue"] = float(ptab[best[0]]) if best else float("nan")
                        e[sd + "_start"] = float(best[1]) if best else float("nan")
                        e[sd + "_strand"] = best[2] if best else ""
                        kmer = text[o + best[1]:o + best[1] + W] if best else b""
                        e[sd + "_kmer"] = (kmer if not best or best[2] == "+" else kmer.translate(_COMP)[::-1]).decode()
                        e[sd + "_log2_affinity"] = float(np.log2(float(total))) + log2_offset if total else float("nan")
                    e["delta_log2_affinity"] = e["alt_log2_affinity"] - e["ref_log2_affinity"]
                    rows.append(e)
    return rows


def summary_rows(rows):
    """The summary from the detail rows, one row at a time: over the named blocks of the versions >= 0
    -> {(sequence_name, position, length): dict(versions, haplotypes, haplotypes_gain, haplotypes_loss, deltas, scores)}"""
    out = {}
    for r in rows:
        if not r["named"] or r["version"] < 0:
            continue
        d = out.setdefault((r["sequence_name"], r["position"], r["length"]),
                           dict(versions=0, haplotypes=0, haplotypes_gain=0, haplotypes_loss=0, deltas=[], scores=[]))
        d["versions"] += 1
        d["haplotypes"] += r["haplotypes"]
        d["haplotypes_gain"] += r["haplotypes"] if r["effect"] == "gain" else 0
        d["haplotypes_loss"] += r["haplotypes"] if r["effect"] == "loss" else 0
        if r["delta_log2_affinity"] == r["delta_log2_affinity"]:
            d["deltas"].append(r["delta_log2_affinity"])
        if r["alt_score"] == r["alt_score"]:
            d["scores"].append(r["alt_score"])
    return out
