"""Brute force for the mutation scan (grafimo_amd/mutation_scan.py) -- TEST INFRASTRUCTURE ONLY.

THE RULE (include/grafimo_hip.h states it for the library; grafimo_amd/mutation_scan.py for the table).  For a sequence x of n
bases and a motif of width W, for every offset o in 0 .. n - 1 and every base b in A, C, G, T:
  y = x with y[o] = b.
  REF side: the window starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).
  ALT side: the same starts in y.
  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY.
  A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
  Per side: the best window by (score descending, s ascending, + before -), as the key
  ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, with s - o in -(W - 1) .. 0; key 0 means the side has no window (n < W);
  and the exact uint64 sum of w[score] over the side's windows and strands.
  b equal to the folded x[o] gives ALT equal to REF.
  An x[o] that is no base has an all-min_val REF side, and each b can repair it.

For each (x, o, b) y is built and query_variant_bruteforce.side is called with l = 1 for both sides: every touched window is
scored from scratch -- the delta trick is never used -- and the sums are Python integers."""
import numpy as np

from query_variant_bruteforce import hand_graph, side, spelled  # noqa: F401
from variant_bruteforce import haplotype_classes, spell

TO = b"ACGT"


def key_of(best) -> int:
    return 0 if best is None else ((best[0] + 1) << 8) | ((64 - best[1]) << 1) | int(best[2] == "+")


def scan(x: bytes, W: int, sm, min_val: int, wtab, forward_only: bool):
    """-> per offset o a list of five (best or None, sum): REF, then y[o] = A, C, G, T"""
    out = []
    for o in range(len(x)):
        row = [side(x, o, 1, W, sm, min_val, wtab, forward_only)]
        for b in TO:
            y = x[:o] + bytes([b]) + x[o + 1:]
            row.append(side(y, o, 1, W, sm, min_val, wtab, forward_only))
        out.append(row)
    return out


def scan_arrays(seqs, W: int, sm, min_val: int, wtab, forward_only: bool):
    """the sequences' scans as the kernel lays them out -> (keys [n_bases][5], sums [n_bases][5]) lists of Python integers"""
    keys, sums = [], []
    for x in seqs:
        for row in scan(x, W, sm, min_val, wtab, forward_only):
            keys.append([key_of(b) for b, _ in row])
            sums.append([int(s) for _, s in row])
    return keys, sums


def region_sequences(idx, S: int, E: int, groups=()):
    """The sequences the table scans in the region [S, E) of the chromosome of `idx`, independent of the versions machinery:
    every haplotype class is spelled over the whole chromosome and cut to the bases with coord + inserted >= S and coord < E;
    equal bases are one version (two deletions of a repeat spell one sequence with two sets of coordinates: `coords` lists them
    all, the table holds its representative's), numbered by haplotypes descending, then smallest member; the reference sequence
    is added with count 0 and version -1 where no version equals it
    -> [dict(version, count, group_counts, is_reference, bases, coords [[(coordinate, inserted)]])] by version, the reference last"""
    L = len(idx.ref)
    S, E = min(max(S, 0), L), min(max(E, 0), L)
    reps, class_of = haplotype_classes(idx)
    found = {}
    for c, h in enumerate(np.asarray(reps).tolist()):
        seq, coord, ins, _, _ = spell(idx, h)
        cut = [(int(b), int(p), bool(t)) for b, p, t in zip(seq, coord, ins) if p + int(t) >= S and p < E]
        text = bytes(b for b, _, _ in cut)
        d = found.setdefault(text, dict(members=[], coords=[]))
        d["members"] += np.flatnonzero(class_of == c).tolist()
        if [(p, t) for _, p, t in cut] not in d["coords"]:
            d["coords"].append([(p, t) for _, p, t in cut])
    ref = bytes(np.asarray(idx.ref, dtype=np.uint8))[S:E] if E > S else b""
    out = []
    for text, d in found.items():
        m = sorted(d["members"])
        out.append(dict(count=len(m), first=m[0], group_counts=[len(set(m) & set(g)) for g in groups], is_reference=text == ref,
                        bases=text, coords=d["coords"]))
    out.sort(key=lambda d: (-d["count"], d["first"]))
    for k, d in enumerate(out):
        d["version"] = k
    if not any(d["is_reference"] for d in out):
        out.append(dict(version=-1, count=0, first=-1, group_counts=[0 for _ in groups], is_reference=True, bases=ref,
                        coords=[[(p, False) for p in range(S, max(E, S))]]))
    return out


def effect(ptab, threshold: float, ref, alt) -> str:
    pr = ref is not None and ptab[ref[0]] < threshold
    px = alt is not None and ptab[alt[0]] < threshold
    return ["none", "gain", "loss", "both"][2 * int(pr) + int(px)]


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def detail_rows(region_names, seqs, scans, coords_of, W: int, scale: int, offset: float, ptab, log2_offset: float, threshold: float):
    """The detail rows of all_rows as dicts, in the frame's order: regions in order, a region's versions by number, its
    reference sequence last, offsets ascending, to-bases A, C, G, T without the from-base.  `seqs`: per region what
    region_sequences gives; `scans`: per region, per sequence, its scan(); coords_of(r, d): the [(coordinate, inserted)] of
    sequence d of region r (one of d["coords"]).  The floats are made as the table documents them: score / scale + W offset,
    the tail table at the score, log2(sum) + log2_offset."""
    rows = []
    for r, region in enumerate(seqs):
        for d, sc in zip(region, scans[r]):
            coord = coords_of(r, d)
            x = d["bases"].upper()
            for o, row in enumerate(sc):
                for col, to in enumerate(TO, 1):
                    if x[o] == to:
                        continue
                    (rb, rs), (ab, as_) = row[0], row[col]
                    y = x[:o] + bytes([to]) + x[o + 1:]
                    e = dict(sequence_name=region_names[r], version=d["version"], haplotypes=d["count"], groups=list(d["group_counts"]),
                             is_reference=d["is_reference"], position=coord[o][0] + 1, inserted=coord[o][1], to=chr(to),
                             effect=effect(ptab, threshold, rb, ab))
                    e["from"] = chr(x[o])
                    for sd, best, total, text in (("ref", rb, rs, x), ("alt", ab, as_, y)):
                        e[sd + "_score"] = float(best[0]) / float(scale) + float(W) * offset if best else float("nan")
                        e[sd + "_pvalue"] = float(ptab[best[0]]) if best else float("nan")
                        e[sd + "_start"] = float(best[1]) if best else float("nan")
                        e[sd + "_strand"] = best[2] if best else ""
                        k = text[o + best[1]:o + best[1] + W] if best else b""
                        e[sd + "_kmer"] = (k if not best or best[2] == "+" else k.translate(_COMP)[::-1]).decode()
                        e[sd + "_log2_affinity"] = float(np.log2(float(total))) + log2_offset if total else float("nan")
                    e["delta_log2_affinity"] = e["alt_log2_affinity"] - e["ref_log2_affinity"]
                    rows.append(e)
    return rows


def summary_of(detail_rows):
    """The summary from the detail rows (dicts with sequence_name, version, haplotypes, position, inserted, from, to,
    delta_log2_affinity, effect, alt_score), one row at a time -> {(sequence_name, position, from, to): dict(versions, haplotypes,
    haplotypes_gain, haplotypes_loss, min_delta, max_delta, best_alt_score)}"""
    out = {}
    for r in detail_rows:
        if r["inserted"] or r["version"] < 0:
            continue
        d = out.setdefault((r["sequence_name"], r["position"], r["from"], r["to"]),
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
