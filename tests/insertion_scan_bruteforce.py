"""Brute force for the insertion scan (grafimo_amd/insertion_scan.py) -- TEST INFRASTRUCTURE ONLY.

THE RULE (include/grafimo_hip.h states it for the library; grafimo_amd/insertion_scan.py for the table).  For a sequence x of
n bases, a motif of width W, a list of K inserts with K in 1 .. 16, every insert I of the list, Li its length in 1 .. 64, and
every offset o in 0 .. n - 1:
  Every insert holds A, C, G, T only.  Case is folded, as base_code does.
  The edit is the insertion of I behind x[o].  Let o' = o + 1 and y = x[:o'] + I + x[o':].
  This is gfm_graph_query_edits' rule with lr = 0, la = Li at offset o'.
    REF side (column JUNCTION): the starts s of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).
    It does not depend on the insert.  It equals the indel scan's JUNCTION column bit for bit.
    ALT side (column INS): the starts s of y with max(0, o' - W + 1) <= s <= min(o' + Li - 1, n + Li - W).
    A window that lies wholly inside the insert counts, as the query rule counts it.
  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
  A window that holds a base of x that is not A/C/G/T scores min_val on both strands.
  An insertion repairs nothing, because it removes no base.  A window that does not reach the N is clean.
  Per column, the best window by (score descending, s ascending, + before -), as the key
  ((score + 1) << 8) | ((64 - (s - o')) << 1) | plus, s - o' in -(W - 1) .. -1 for JUNCTION and in -(W - 1) .. Li - 1 for INS.
  Key 0 means the side has no window.
  Per column, the exact uint64 sum of w[score] over the side's windows and strands.
  An insertion before the first base of a sequence is not scanned, as in the indel scan.  An empty sequence has no rows.
  With the inserts ("A", "C", "G", "T") the INS columns equal the indel scan's INS_A .. INS_T bit for bit.
  A cell does not depend on the other inserts of the list or on their order.

For each (x, o, I) y is built and query_variant_bruteforce.side is called with l = 0 on x and l = Li on y, both at o + 1: every
touched window is scored from scratch -- no prefix, no H or T table is used -- and the sums are Python integers."""
import numpy as np

from mutation_scan_bruteforce import effect, key_of, region_sequences  # noqa: F401
from query_variant_bruteforce import hand_graph, side  # noqa: F401


def edited(x: bytes, o: int, insert: bytes) -> bytes:
    return x[:o + 1] + insert + x[o + 1:]


def scan(x: bytes, W: int, sm, min_val: int, wtab, forward_only: bool, inserts):
    """-> per insert, per offset o, a list of two (best or None, sum): JUNCTION, INS; a best's second field is the start minus
    o + 1, the place of the first inserted base"""
    out = []
    for ins in inserts:
        ins = ins.upper()
        out.append([[side(x, o + 1, 0, W, sm, min_val, wtab, forward_only),
                     side(edited(x, o, ins), o + 1, len(ins), W, sm, min_val, wtab, forward_only)] for o in range(len(x))])
    return out


def scan_arrays(seqs, W: int, sm, min_val: int, wtab, forward_only: bool, inserts):
    """the sequences' scans as the kernel lays them out -> (keys [n_inserts][n_bases][2], sums [n_inserts][n_bases][2]) lists
    of Python integers"""
    keys, sums = [[] for _ in inserts], [[] for _ in inserts]
    for x in seqs:
        for k, rows in enumerate(scan(x, W, sm, min_val, wtab, forward_only, inserts)):
            keys[k] += [[key_of(b) for b, _ in row] for row in rows]
            sums[k] += [[int(s) for _, s in row] for row in rows]
    return keys, sums


def reported(x: bytes, o: int, insert: bytes) -> bool:
    """the frames report a change once, at the leftmost offset that spells its y -- by the definition: no smaller offset of the
    sequence spells the same y"""
    u, ins = x.upper(), insert.upper()
    y = edited(u, o, ins)
    return all(edited(u, q, ins) != y for q in range(o))


def named(coord, o: int) -> bool:
    """coord: [(coordinate, inserted)] of a sequence -- a VCF row could name the gap behind base o: the base is non-inserted,
    and it is the sequence's last or the next base is the non-inserted base of the next coordinate"""
    p, t = coord[o]
    return not t and (o == len(coord) - 1 or coord[o + 1] == (p + 1, False))


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def detail_rows(region_names, seqs, scans, coords_of, W: int, scale: int, offset: float, ptab, log2_offset: float, threshold: float,
                inserts, every: bool = False):
    """The detail rows of all_rows as dicts, in the frame's order: regions in order, a region's versions by number, its
    reference sequence last, offsets ascending, the inserts in the list's order, without the gaps a repeat repeats (`every`:
    with them, which is what the summary is made of).  `seqs`, `scans` (this module's scan()) and coords_of as
    mutation_scan_bruteforce.detail_rows takes them; the floats are made as the table documents them."""
    rows = []
    for r, region in enumerate(seqs):
        for d, sc in zip(region, scans[r]):
            coord = coords_of(r, d)
            x = d["bases"].upper()
            for o in range(len(x)):
                for k, ins in enumerate(inserts):
                    ins = ins.upper()
                    if not (every or reported(x, o, ins)):
                        continue
                    (rb, rs), (ab, as_) = sc[k][o]
                    y = edited(x, o, ins)
                    e = dict(sequence_name=region_names[r], version=d["version"], haplotypes=d["count"], groups=list(d["group_counts"]),
                             is_reference=d["is_reference"], position=coord[o][0] + 1, inserted=coord[o][1], insert=ins.decode(),
                             length=len(ins), named=named(coord, o), effect=effect(ptab, threshold, rb, ab))
                    for sd, best, total, text in (("ref", rb, rs, x), ("alt", ab, as_, y)):
                        e[sd + "_score"] = float(best[0]) / float(scale) + float(W) * offset if best else float("nan")
                        e[sd + "_pvalue"] = float(ptab[best[0]]) if best else float("nan")
                        e[sd + "_start"] = float(best[1]) if best else float("nan")
                        e[sd + "_strand"] = best[2] if best else ""
                        kmer = text[o + 1 + best[1]:o + 1 + best[1] + W] if best else b""
                        e[sd + "_kmer"] = (kmer if not best or best[2] == "+" else kmer.translate(_COMP)[::-1]).decode()
                        e[sd + "_log2_affinity"] = float(np.log2(float(total))) + log2_offset if total else float("nan")
                    e["delta_log2_affinity"] = e["alt_log2_affinity"] - e["ref_log2_affinity"]
                    rows.append(e)
    return rows


def summary_of(every_row):
    """The summary from the detail rows made with every=True, one row at a time: over the named gaps of the versions >= 0
    -> {(sequence_name, position, insert): dict(versions, haplotypes, haplotypes_gain, haplotypes_loss, deltas, scores)}"""
    out = {}
    for r in every_row:
        if not r["named"] or r["version"] < 0:
            continue
        d = out.setdefault((r["sequence_name"], r["position"], r["insert"]),
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
