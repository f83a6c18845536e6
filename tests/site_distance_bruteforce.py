"""Brute force for the site distance (grafimo_amd/site_distance.py) -- TEST INFRASTRUCTURE ONLY.

THE RULE (include/grafimo_hip.h states it for the library; grafimo_amd/site_distance.py for the table).
Inputs: a sequence x of n bases; a motif of width W with its integer matrix as the packed table holds it, entry t[j][b] for
the window's forward column j and base b, one table per strand; a cutoff c in 0 .. 1000 W + 1; a cap E in 1 .. 8.
Every window start s in 0 .. n - W and every strand is handled independently.
Under GFM_GRAPH_FORWARD_ONLY only the + strand is handled.  Case is folded, as base_code does.
A window that holds a column with no A/C/G/T scores min_val on both strands.  Otherwise its score is the sum of its entries.
A window's unedited score on a strand is its `own` score.  The window is a site on that strand when own >= c.
Raising (the near side).  Start from the window as spelled and repeat these steps:
  1. If the current score >= c, stop with d = picks made.
  2. If E picks are made, stop with d = E + 1.
  3. If a non-base column remains, the next pick is the leftmost such column.  It gets the column's best base: the largest
     entry on this strand.  Ties go to the first of A, C, G, T.  While any non-base column remains, the score stays min_val.
  4. Otherwise the next pick is the unpicked base column with the largest gain.  The gain is the column's largest entry minus
     its present entry.  Ties go to the leftmost column.  The column gets that best base.  Ties go to the first of A, C, G, T.
  5. If every remaining gain is 0, stop with d = E + 1.
Lowering (the fragile side).
  1. If own < c, d = 0 and there are no picks.
  2. A window with a non-base column takes no picks: d = 0 if min_val < c, otherwise d = E + 1.
  3. Otherwise pick as above, with the loss in place of the gain.  The loss is the present entry minus the column's smallest
     entry.  The worst base is the smallest entry.  Ties go to the first of A, C, G, T.  Stop when the score < c, with d = picks
     made.  Stop at E picks, or when every remaining loss is 0, with d = E + 1.
Results per (window start, strand, side): d in 0 .. E + 1; the score after the picks made; the 64-bit mask of the picked
forward columns, bit j for column j.  d and the score do not depend on the tie rules.  Only the mask does.
By the exchange argument d is the true minimum whenever it is <= E.
Columns are always forward offsets in the window.  Bases are forward-strand bases.  The - strand reads its own half of the
packed table at the same forward column.

Two things live here: THE RULE in plain Python loops, one step of the text at a time (raise_window, lower_window, scan_arrays),
and an exhaustive minimiser (exhaustive) that knows nothing of gains: it tries every set of at most E columns with every
assignment of bases.  The frames' rows (detail_rows, summary_of) are put together from the loops' picks one row at a time."""
import itertools

from mutation_scan_bruteforce import hand_graph, region_sequences  # noqa: F401

ACGT = b"ACGT"
NO_WINDOW = 0xFFFFFFFF
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def strand_tables(sm, W: int):
    """the score matrix sm[b][j] (rows A, C, G, T) -> (t+, t-): t[j][b] of the window's forward column j and forward base b; the -
    strand scores the reverse complement, so forward base b at forward column j meets the matrix at (3 - b, W - 1 - j)"""
    plus = [[int(sm[b][j]) for b in range(4)] for j in range(W)]
    minus = [[int(sm[3 - b][W - 1 - j]) for b in range(4)] for j in range(W)]
    return plus, minus


def window_codes(k: bytes):
    """per column the index of its base in ACGT, case folded; None: no base"""
    return [ACGT.index(c) if c in ACGT else None for c in k.upper()]


def score_of(codes, t, min_val: int) -> int:
    if any(c is None for c in codes):
        return min_val
    return sum(t[j][c] for j, c in enumerate(codes))


def raise_window(codes, t, min_val: int, c: int, E: int):
    """the near side of one window on one strand -> (d, score after, picks [(column, base it gets)] in the order made)"""
    codes, picks = list(codes), []
    while True:
        score = score_of(codes, t, min_val)
        if score >= c:                                           # 1
            return len(picks), score, picks
        if len(picks) == E:                                      # 2
            return E + 1, score, picks
        holes = [j for j, b in enumerate(codes) if b is None]
        if holes:                                                # 3
            j = holes[0]
        else:                                                    # 4, 5
            done = {j for j, _ in picks}
            gains = [0 if j in done else max(t[j]) - t[j][codes[j]] for j in range(len(codes))]
            if max(gains) == 0:
                return E + 1, score, picks
            j = gains.index(max(gains))
        b = t[j].index(max(t[j]))
        codes[j] = b
        picks.append((j, b))


def lower_window(codes, t, min_val: int, c: int, E: int):
    """the fragile side of one window on one strand -> (d, score after, picks)"""
    codes, picks = list(codes), []
    own = score_of(codes, t, min_val)
    if own < c:                                                  # 1
        return 0, own, picks
    if any(b is None for b in codes):                            # 2 (own = min_val >= c here)
        return E + 1, own, picks
    while True:                                                  # 3
        score = score_of(codes, t, min_val)
        if score < c:
            return len(picks), score, picks
        if len(picks) == E:
            return E + 1, score, picks
        done = {j for j, _ in picks}
        losses = [0 if j in done else t[j][codes[j]] - min(t[j]) for j in range(len(codes))]
        if max(losses) == 0:
            return E + 1, score, picks
        j = losses.index(max(losses))
        b = t[j].index(min(t[j]))
        codes[j] = b
        picks.append((j, b))


def mask_of(picks) -> int:
    return sum(1 << j for j, _ in picks)


def scan(x: bytes, W: int, sm, min_val: int, cutoff: int, E: int, fwd: bool):
    """-> per window start s in 0 .. n - W a list over the strands (+, then - unless fwd) of dict(own, near, fragile): near
    and fragile are (d, score after, picks)"""
    tabs = strand_tables(sm, W)[:1 if fwd else 2]
    out = []
    for s in range(len(x) - W + 1):
        codes = window_codes(x[s:s + W])
        out.append([dict(own=score_of(codes, t, min_val), near=raise_window(codes, t, min_val, cutoff, E),
                         fragile=lower_window(codes, t, min_val, cutoff, E)) for t in tabs])
    return out


def scan_arrays(seqs, W: int, score_matrix, min_val: int, cutoff: int, E: int, fwd: bool):
    """the sequences' scans as the kernel lays them out -> (words [n_bases][6], masks [n_bases][4]) lists of Python integers: a
    row per base, read as a window start"""
    words, masks = [], []
    for x in seqs:
        rows = scan(x, W, score_matrix, min_val, cutoff, E, fwd)
        for s in range(len(x)):
            w, m = [NO_WINDOW] * 6, [0] * 4
            if s < len(rows):
                for st, r in enumerate(rows[s]):
                    w[st] = r["own"]
                    for side, name in enumerate(("near", "fragile")):
                        d, after, picks = r[name]
                        w[2 + 2 * side + st] = (after << 4) | d
                        m[2 * side + st] = mask_of(picks)
            words.append(w)
            masks.append(m)
    return words, masks


def exhaustive(codes, t, min_val: int, c: int, E: int, lift: bool):
    """no gains, no greed: every set of at most k columns with every assignment of bases, k = 0 .. E -> (d, the extreme score
    over all edits of at most min(d, E) columns): d is the least k at which some edit puts the score on the asked side of c
    (>= c to lift, < c to lower), E + 1 when none of at most E columns does.  For W <= 5 and E <= 3."""
    W = len(codes)
    extreme = []
    for k in range(E + 1):
        best = score_of(codes, t, min_val)
        for cols in itertools.combinations(range(W), min(k, W)):
            for to in itertools.product(range(4), repeat=len(cols)):
                y = list(codes)
                for j, b in zip(cols, to):
                    y[j] = b
                sc = score_of(y, t, min_val)
                best = max(best, sc) if lift else min(best, sc)
        extreme.append(best)
    for k in range(E + 1):
        if (extreme[k] >= c) if lift else (extreme[k] < c):
            return k, extreme[k]
    return E + 1, extreme[E]


# ---------------------------------------------------------------------------------------------------------------- the frames
def detail_rows(region_names, seqs, scans, coords_of, W: int, scale: int, offset: float, ptab, cutoff: int, E: int):
    """The detail rows of all_rows as dicts, in the frame's order: regions in order, a region's versions by number, its reference
    sequence last, window starts ascending, + before -.  `seqs`: per region what region_sequences gives; `scans`: per region, per
    sequence, its scan(); coords_of(r, d): the [(coordinate, inserted)] of sequence d of region r.  The floats are made as the
    table documents them: score / scale + W offset, the tail table at the score."""
    rows = []
    number = lambda sc: float(sc) / float(scale) + float(W) * offset            # noqa: E731
    for r, region in enumerate(seqs):
        for d, sc in zip(region, scans[r]):
            coord = coords_of(r, d)
            x = d["bases"].upper()
            for s, strands in enumerate(sc):
                for st, res in enumerate(strands):
                    site = res["own"] >= cutoff
                    dist, after, picks = res["fragile"] if site else res["near"]
                    kind = "site" if site else ("near" if 1 <= dist <= E else "far")
                    k = x[s:s + W]
                    y = bytearray(k)
                    for j, b in picks:
                        y[j] = ACGT[b]
                    show = lambda t: (bytes(t) if st == 0 else bytes(t).translate(_COMP)[::-1]).decode()   # noqa: E731
                    rows.append(dict(
                        sequence_name=region_names[r], version=d["version"], haplotypes=d["count"], groups=list(d["group_counts"]),
                        is_reference=d["is_reference"], position=coord[s][0] + 1, inserted=coord[s][1], strand="+-"[st],
                        kmer=show(k), score=number(res["own"]), pvalue=float(ptab[res["own"]]), kind=kind, distance=dist,
                        reached=dist <= E, changes=",".join(f"{j + 1}:{chr(k[j])}>{chr(ACGT[b])}" for j, b in sorted(picks)),
                        edited_kmer=show(y), edited_score=number(after), edited_pvalue=float(ptab[after]),
                        near_d=res["near"][0], fragile_d=res["fragile"][0]))
    return rows


def summary_of(rows, E: int):
    """The summary from the detail rows of all_rows, one row at a time -> {(sequence_name, position, strand): dict(versions,
    haplotypes, haplotypes_site, near [E], haplotypes_far, site_distances, scores)}"""
    out = {}
    for r in rows:
        if r["inserted"] or r["version"] < 0:
            continue
        d = out.setdefault((r["sequence_name"], r["position"], r["strand"]),
                           dict(versions=0, haplotypes=0, haplotypes_site=0, near=[0] * E, haplotypes_far=0, site_distances=[], scores=[]))
        d["versions"] += 1
        d["haplotypes"] += r["haplotypes"]
        if r["kind"] == "site":
            d["haplotypes_site"] += r["haplotypes"]
            d["site_distances"].append(r["distance"])
        elif r["kind"] == "near":
            d["near"][r["distance"] - 1] += r["haplotypes"]
        else:
            d["haplotypes_far"] += r["haplotypes"]
        d["scores"].append(r["score"])
    return out
