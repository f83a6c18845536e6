"""Brute force for the indel scan (grafimo_amd/indel_scan.py) -- TEST INFRASTRUCTURE ONLY.

THE RULE (include/grafimo_hip.h states it for the library; grafimo_amd/indel_scan.py for the table).  For a sequence x of
n bases, a motif of width W, and every offset o in 0 .. n - 1:
  Deletion of x[o].  y = x[:o] + x[o+1:].  This is gfm_graph_query_edits' rule with lr = 1, la = 0 at offset o.
    REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).  This is exactly the mutation
    scan's REF column.
    ALT side (column DEL): the starts of y across the junction, max(0, o - W + 1) <= s <= min(o - 1, n - 1 - W).
  Insertion of b in A, C, G, T behind x[o].  y = x[:o+1] + b + x[o+1:].  This is the query rule with lr = 0, la = 1 at offset
  o' = o + 1.
    REF side (column JUNCTION): the starts of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).
    ALT side (columns INS_A, INS_C, INS_G, INS_T): the starts of y with max(0, o' - W + 1) <= s <= min(o', n + 1 - W).
  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
  A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
  Per column, the best window by (score descending, s ascending, + before -), as the key
  ((score + 1) << 8) | ((64 - rel) << 1) | plus, rel = s - o for COVER and DEL, rel = s - (o + 1) for JUNCTION and INS_*: the
  values a gfm_edit_record_t of the same edit holds.  Key 0 means the side has no window.
  Per column, the exact uint64 sum of w[score] over the side's windows and strands.
  A deleted N can repair its windows.  An N elsewhere leaves its windows at min_val.  An insertion before the first base of a
  sequence is not scanned: every row has the base it is anchored to, as a VCF row has.  An empty sequence has no rows.

For each (x, o, change) y is built and query_variant_bruteforce.side is called with l = 1 / 0 for a deletion's sides and
0 / 1 for an insertion's: every touched window is scored from scratch -- the prefix identity is never used -- and the sums are
Python integers."""
import numpy as np

from mutation_scan_bruteforce import effect, key_of, region_sequences  # noqa: F401
from query_variant_bruteforce import hand_graph, side  # noqa: F401

TO = b"ACGT"
CHANGES = [("DEL", None)] + [("INS", b) for b in TO]             # a base's changes in the frames' order
REF_COLUMN = {"DEL": 0, "INS": 2}


def scan(x: bytes, W: int, sm, min_val: int, wtab, forward_only: bool):
    """-> per offset o a list of seven (best or None, sum): COVER, DEL, JUNCTION, INS_A, INS_C, INS_G, INS_T; a best's second
    field is the start minus o (COVER, DEL) or minus o + 1 (the others)"""
    out = []
    for o in range(len(x)):
        row = [side(x, o, 1, W, sm, min_val, wtab, forward_only),
               side(x[:o] + x[o + 1:], o, 0, W, sm, min_val, wtab, forward_only),
               side(x, o + 1, 0, W, sm, min_val, wtab, forward_only)]
        for b in TO:
            row.append(side(x[:o + 1] + bytes([b]) + x[o + 1:], o + 1, 1, W, sm, min_val, wtab, forward_only))
        out.append(row)
    return out


def scan_arrays(seqs, W: int, sm, min_val: int, wtab, forward_only: bool):
    """the sequences' scans as the kernel lays them out -> (keys [n_bases][7], sums [n_bases][7]) lists of Python integers"""
    keys, sums = [], []
    for x in seqs:
        for row in scan(x, W, sm, min_val, wtab, forward_only):
            keys.append([key_of(b) for b, _ in row])
            sums.append([int(s) for _, s in row])
    return keys, sums


def reported(x: bytes, o: int, kind: str, b) -> bool:
    """the frames report a change once, at the leftmost offset that spells its y"""
    u = x.upper()
    if o == 0:
        return True
    return u[o - 1] != u[o] if kind == "DEL" else u[o] != b


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def detail_rows(region_names, seqs, scans, coords_of, W: int, scale: int, offset: float, ptab, log2_offset: float, threshold: float):
    """The detail rows of all_rows as dicts, in the frame's order: regions in order, a region's versions by number, its
    reference sequence last, offsets ascending, the changes DEL, INS A, C, G, T, without those a homopolymer repeats.  `seqs`,
    `scans` (this module's scan()) and coords_of as mutation_scan_bruteforce.detail_rows takes them; the floats are made as
    the table documents them."""
    rows = []
    for r, region in enumerate(seqs):
        for d, sc in zip(region, scans[r]):
            coord = coords_of(r, d)
            x = d["bases"].upper()
            for o, row in enumerate(sc):
                for col, (kind, b) in zip((1, 3, 4, 5, 6), CHANGES):
                    if not reported(x, o, kind, b):
                        continue
                    (rb, rs), (ab, as_) = row[REF_COLUMN[kind]], row[col]
                    y = x[:o] + x[o + 1:] if kind == "DEL" else x[:o + 1] + bytes([b]) + x[o + 1:]
                    at = o if kind == "DEL" else o + 1
                    e = dict(sequence_name=region_names[r], version=d["version"], haplotypes=d["count"], groups=list(d["group_counts"]),
                             is_reference=d["is_reference"], position=coord[o][0] + 1, inserted=coord[o][1], type=kind,
                             base=chr(x[o]) if kind == "DEL" else chr(b), effect=effect(ptab, threshold, rb, ab))
                    for sd, best, total, text in (("ref", rb, rs, x), ("alt", ab, as_, y)):
                        e[sd + "_score"] = float(best[0]) / float(scale) + float(W) * offset if best else float("nan")
                        e[sd + "_pvalue"] = float(ptab[best[0]]) if best else float("nan")
                        e[sd + "_start"] = float(best[1]) if best else float("nan")
                        e[sd + "_strand"] = best[2] if best else ""
                        k = text[at + best[1]:at + best[1] + W] if best else b""
                        e[sd + "_kmer"] = (k if not best or best[2] == "+" else k.translate(_COMP)[::-1]).decode()
                        e[sd + "_log2_affinity"] = float(np.log2(float(total))) + log2_offset if total else float("nan")
                    e["delta_log2_affinity"] = e["alt_log2_affinity"] - e["ref_log2_affinity"]
                    rows.append(e)
    return rows


def summary_of(detail_rows):
    """The summary from the detail rows, one row at a time -> {(sequence_name, position, type, base): dict(versions, haplotypes,
    haplotypes_gain, haplotypes_loss, deltas, scores)}"""
    out = {}
    for r in detail_rows:
        if r["inserted"] or r["version"] < 0:
            continue
        d = out.setdefault((r["sequence_name"], r["position"], r["type"], r["base"]),
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
