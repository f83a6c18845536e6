"""Site distance: how far every window of every version (haplotype_sequences) the panel spells in a region, and of the
reference sequence, is from binding, and how much every site can absorb -- the least number of substitutions that lifts a
window over the score cutoff (near-sites one or two mutations from a site, and on how many haplotypes they lie), the least
number that drops a site under it (how robust a reported hit is), and the smallest edit set that does either (base-editor
design).  Where the mutation scan enumerates every single-base change and scores it, this table asks the inverse question and
enumerates nothing: for an additive PWM the answer is exact and greedy over the per-column gains.  The mutation scan is its
E = 1 corner, seen from the edit's side.

THE RULE (include/grafimo_hip.h states it for the library; tests/site_distance_bruteforce.py on the host).
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

The cutoff of the tables is the report's: a window is a site when the p-value of its score is < threshold (cutoff_of).

The hot path is HIP (grafimo_amd/csrc/gfm_graph_site_distance.hpp, gfm_sequence_site_distance): a lane per window start, the
selection in registers.  Everything from the kernel's arrays to the frames is numpy group-bys; there is no Python step per row
or per base.
"""
import ctypes
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _stream_ptr, _torch
from .graph_tables import scaled_pvalues, scaled_scores
from .sequence_scans import (_UPPER, DEFAULT_MAX_BYTES, TO_BASES, SequenceTable, _checked_sequences, chunk_step, printed_windows,
                             scan_inputs, table_writers, tables_by_width)

DETAIL_FILE = "grafimo_site_distance"
SUMMARY_FILE = "grafimo_site_distance_summary"
ENTRY = "gfm_sequence_site_distance"
WORD_COLUMNS = ("own+", "own-", "near+", "near-", "fragile+", "fragile-")           # the six columns of words
MASK_COLUMNS = ("near+", "near-", "fragile+", "fragile-")                          # the four columns of masks
NO_WINDOW = 0xFFFFFFFF
MAX_EDITS = nv.GFM_SITEDIST_MAX_EDITS
BYTES_PER_BASE = 6 * 4 + 4 * 8                           # a motif's words and masks per base
KINDS = np.array(["far", "near", "site"], dtype=object)


# ---------------------------------------------------------------------------------------------------------------- helpers
def decode_words(words) -> Tuple[np.ndarray, np.ndarray]:
    """near / fragile words -> (d int64, score_after int64); (-1, -1) where there is no window"""
    w = np.asarray(words).astype(np.int64)
    some = w != NO_WINDOW
    return np.where(some, w & 15, -1), np.where(some, w >> 4, -1)


def own_scores(words) -> np.ndarray:
    """own words -> int64 scores, -1 where there is no window"""
    w = np.asarray(words).astype(np.int64)
    return np.where(w != NO_WINDOW, w, -1)


def cutoff_of(ptable, threshold: float) -> int:
    """the smallest scaled score s with ptable[s] < threshold -- the report's strict < --, len(ptable) = 1000 W + 1 when there
    is none: a window is a site when its score is >= the cutoff"""
    below = np.flatnonzero(np.asarray(ptable, dtype=np.float64) < float(threshold))
    return int(below[0]) if len(below) else int(len(ptable))


def checked_edits(max_edits) -> int:
    if isinstance(max_edits, bool) or int(max_edits) != max_edits or not 1 <= int(max_edits) <= MAX_EDITS:
        raise ValueError(f"max_edits {max_edits!r}: an integer in 1 .. {MAX_EDITS}")
    return int(max_edits)


def strand_tables(motif) -> np.ndarray:
    """int64 [2, W, 4]: t[strand][j][b], the entry of the window's forward column j and forward base b of A, C, G, T, as the
    packed table holds it: + reads the matrix at (b, j), - at (complement of b, W - 1 - j)"""
    W = int(motif.width)
    if hasattr(motif, "dense_score_matrix"):
        sm = np.asarray(motif.dense_score_matrix(), dtype=np.int64).reshape(4, W)
    else:
        sm = np.asarray(motif.score_matrix, dtype=np.int64).reshape(4, W)
    return np.stack([sm.T, sm[::-1, ::-1].T])


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _scan(dms, seq_offsets: np.ndarray, bases: np.ndarray, cutoffs: np.ndarray, max_edits: int, forward_only: bool):
    """gfm_sequence_site_distance for leased motifs of one width -> (words uint32 [M, N, 6], masks uint64 [M, N, 4])"""
    M, N = len(dms), int(seq_offsets[-1])
    torch = _torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    d_bases = torch.from_numpy(np.array(bases, dtype=np.uint8)).to(dev)              # (a copy: the caller's may be read-only)
    words = torch.empty((M, max(N, 1), 6), dtype=torch.int32, device=dev)
    masks = torch.empty((M, max(N, 1), 4), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    nv.check(getattr(nv.lib(), ENTRY)(
        (vp * M)(*[x.handle for x in dms]), M, len(seq_offsets) - 1, seq_offsets.ctypes.data, d_bases.data_ptr(),
        cutoffs.ctypes.data, max_edits, nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0,
        (vp * M)(*[words[m].data_ptr() for m in range(M)]), (vp * M)(*[masks[m].data_ptr() for m in range(M)]),
        status.data_ptr(), _stream_ptr(None)))
    return words[:, :N].cpu().numpy().view(np.uint32), masks[:, :N].cpu().numpy().view(np.uint64)


def _scan_chunked(motifs: Sequence, seq_offsets, bases, cutoffs, threshold, max_edits, forward_only, max_bytes):
    """-> (per motif (words, masks), per motif its cutoff, per motif (scale, offset, ptable)): the motifs leased and scanned in
    chunks whose result tensors (56 bytes a base and motif) stay under max_bytes.  `cutoffs` None: cutoff_of at `threshold`.
    The library is called with no base too: it checks the widths, the cap and the cutoffs all the same."""
    from .device import DeviceMotif
    max_edits = checked_edits(max_edits)
    if cutoffs is not None and len(cutoffs) != len(motifs):
        raise ValueError(f"{len(cutoffs)} cutoffs for {len(motifs)} motifs")
    step = chunk_step(motifs, int(seq_offsets[-1]), BYTES_PER_BASE * int(seq_offsets[-1]), max_bytes, "words and masks")
    results, used, numbers = [], [], []
    for m0 in range(0, len(motifs), step):
        dms = [DeviceMotif.lease(m) for m in motifs[m0:m0 + step]]
        try:
            nums = [(dm.scale, dm.offset, dm.ptable_host()) for dm in dms]
            if cutoffs is None:
                cut = np.array([cutoff_of(p, threshold) for _, _, p in nums], dtype=np.int32)
            else:
                cut = np.ascontiguousarray(np.asarray(cutoffs[m0:m0 + step], dtype=np.int64).astype(np.int32))
                if not np.array_equal(cut, np.asarray(cutoffs[m0:m0 + step])):
                    raise ValueError("a cutoff is an integer in 0 .. 1000 W + 1")
            words, masks = _scan(dms, seq_offsets, bases, cut, max_edits, forward_only)
            results += [(words[m], masks[m]) for m in range(len(dms))]
            used += cut.tolist()
            numbers += nums
        finally:
            for dm in dms:
                dm.release()
    return results, used, numbers


def scan_sequences(motifs: Sequence, seq_offsets, bases, cutoffs, max_edits: int = 3, forward_only: bool = False,
                   max_bytes: int = DEFAULT_MAX_BYTES) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The kernel on plain arrays: sequences (`seq_offsets` int64 [V + 1] from 0, `bases` uint8) for motifs of ONE width, a
    scaled-score cutoff per motif in 0 .. 1000 W + 1 and the cap `max_edits` in 1 .. 8 -> per motif (words uint32 [n_bases, 6],
    masks uint64 [n_bases, 4]): per base, read as a window start, the words own +, own -, near +, near -, fragile +, fragile -
    (own: the score; else (score_after << 4) | d, decode_words; 0xFFFFFFFF: no window) and the masks of the picked columns
    near +, near -, fragile +, fragile -.  The motifs are taken in chunks whose result tensors stay under `max_bytes`; a single
    motif above it is a ValueError that names it.  The library refuses motifs of two widths and a cutoff out of range."""
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    return _scan_chunked(motifs, seq_offsets, bases, list(cutoffs), None, max_edits, forward_only, max_bytes)[0]


# ---------------------------------------------------------------------------------------------------------------- the table
def _group_heads(keys: Sequence[np.ndarray]):
    """rows that agree in every array of `keys` are one group -> (order, at): the rows sorted by the keys, the first the most
    significant, and where each group starts in that order"""
    n = len(keys[0])
    order = np.lexsort(tuple(np.asarray(k) for k in reversed(list(keys))))
    head = np.ones(n, dtype=bool)
    head[1:] = False
    for k in keys:
        k = np.asarray(k)[order]
        head[1:] |= k[1:] != k[:-1]
    return order, np.flatnonzero(head)


class SiteDistance(SequenceTable):
    """The table of one motif over S sequences of N bases in all (see the module's docstring).
    Per sequence [S]: seq_region, seq_version (-1: the region's reference sequence, which no haplotype spells), seq_count
    (haplotypes), seq_group_counts [S, G], seq_is_reference, seq_offsets int64 [S + 1] -- MutationScan's.
    Per base [N]: bases uint8, coord int32 (~coordinate for an inserted base), and the dense arrays words uint32 [N, 6] and masks
    uint64 [N, 4] as scan_sequences gives them, the base read as a window start.  tables int64 [2, W, 4] (strand_tables): what
    names the base a picked column gets.  cutoff: the scaled score from which a window is a site; max_edits: the cap E."""

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, tables, cutoff, max_edits, threshold, region_names,
                 group_names, seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord,
                 words, masks, all_rows=False):
        super().__init__(motif_id, motif_alt_id, width, scale, offset, ptable, threshold, region_names, group_names, seq_region,
                         seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, all_rows)
        self.tables = np.asarray(tables, dtype=np.int64)
        self.cutoff, self.max_edits = int(cutoff), checked_edits(max_edits)
        self.words, self.masks = np.asarray(words, dtype=np.uint32), np.asarray(masks, dtype=np.uint64)
        N = len(self.bases)
        if not self._fits((self.words, (N, 6)), (self.masks, (N, 4)), (self.tables, (2, self.width, 4))):
            raise ValueError("the arrays do not fit the sequences")

    def __len__(self) -> int:
        return int(self._kept()[0].size)

    # ---- per window-strand
    def _window_strands(self):
        """every (window start, strand) that has a window -> (base index n, strand 0: +, 1: -), in (n, strand) order"""
        n, st = np.nonzero(self.words[:, :2] != NO_WINDOW)
        return n.astype(np.int64), st.astype(np.int64)

    def _numbers(self, n, st):
        """of the window-strands (n, st) -> (own, site (bool), d, score_after, mask): the near side's where the window is no
        site, the fragile side's where it is one"""
        own = own_scores(self.words[n, st])
        site = own >= self.cutoff
        col = np.where(site, 2, 0) + st
        d, after = decode_words(self.words[n, 2 + col])
        return own, site, d, after, self.masks[n, col]

    def _kinds(self, site, d) -> np.ndarray:
        """int64: 2 site, 1 near (1 <= near d <= E), 0 far -- the index into KINDS"""
        return np.where(site, 2, np.where((d >= 1) & (d <= self.max_edits), 1, 0)).astype(np.int64)

    def _kept(self):
        n, st = self._window_strands()
        if self.all_rows:
            return n, st
        _, site, d, _, _ = self._numbers(n, st)
        keep = self._kinds(site, d) > 0
        return n[keep], st[keep]

    def distance_histogram(self) -> np.ndarray:
        """int64 [S, 2, E + 2]: per sequence and side (0 near, 1 fragile) the number of window-strands with d = 0 .. E + 1.  The
        near side counts every window-strand (d = 0: the sites), the fragile side the sites only."""
        S, E = len(self.seq_count), self.max_edits
        out = np.zeros((S, 2, E + 2), dtype=np.int64)
        n, st = self._window_strands()
        if not len(n):
            return out
        seq = self.base_sequence[n]
        near_d = decode_words(self.words[n, 2 + st])[0]
        frag_d = decode_words(self.words[n, 4 + st])[0]
        site = own_scores(self.words[n, st]) >= self.cutoff
        out[:, 0] = np.bincount(seq * (E + 2) + near_d, minlength=S * (E + 2)).reshape(S, E + 2)
        out[:, 1] = np.bincount(seq[site] * (E + 2) + frag_d[site], minlength=S * (E + 2)).reshape(S, E + 2)
        return out

    def _texts(self, n, st, site, mask):
        """-> (kmer, changes, edited_kmer) objects of the window-strands: the window as printed (- reverse complemented), the
        picks as offset:from>to in column order, the window with the picks applied as printed"""
        W, rows = self.width, len(n)
        if not rows:
            z = np.zeros(0, dtype=object)
            return z, z, z
        idx = np.minimum(n[:, None] + np.arange(W, dtype=np.int64)[None, :], len(self.bases) - 1)
        text = _UPPER[self.bases[idx]]                                                    # [rows, W], forward
        picked = ((mask[:, None] >> np.arange(W, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        # the base a picked column gets: the best of the strand's column for a raise, the worst for a site; first of A, C, G, T
        best, worst = self.tables.argmax(axis=2), self.tables.argmin(axis=2)             # [2, W]
        to = TO_BASES[np.where(site[:, None], worst[st], best[st])]                      # [rows, W]
        edited = np.where(picked, to, text)
        r, j = np.nonzero(picked)
        letters = np.array([chr(k) for k in range(256)], dtype="U1")
        piece = np.char.add(np.char.add(np.char.add((j + 1).astype("U2"), ":"), letters[text[r, j]]),
                            np.char.add(">", letters[to[r, j]]))
        first = np.concatenate([[0], np.cumsum(picked.sum(axis=1))])[:-1]
        rank = np.arange(len(r), dtype=np.int64) - first[r]
        changes = np.full(rows, "", dtype=f"U{7 * max(self.max_edits, 1)}")
        for k in range(int(rank.max()) + 1 if len(rank) else 0):                         # (at most E turns, not one per row)
            sel = rank == k
            changes[r[sel]] = np.char.add(changes[r[sel]], np.char.add("," if k else "", piece[sel]))
        return printed_windows(text.copy(), st == 1), changes.astype(object), printed_windows(edited.copy(), st == 1)

    def to_frame(self) -> pd.DataFrame:
        """a row per (sequence, window start, strand) that is a site or a near-site (1 <= near d <= E); all_rows keeps every
        window-strand: motif_id, motif_alt_id, sequence_name, version (-1: the reference sequence, no haplotype spells it),
        haplotypes, one haplotypes_<GROUP> per group, is_reference, position (1-based coordinate of the window's first base; an
        inserted base has its anchor's), inserted (of that base), strand, kmer (as printed: - reverse complemented), score,
        pvalue, kind (site / near / far), distance (the near d of a window that is no site, the fragile d of a site; E + 1 reads
        "more than E"), reached (distance <= E), changes (the picks as offset:from>to, comma-joined in column order: the offset
        1-based and forward in the window, the bases forward-strand), edited_kmer (as printed), edited_score, edited_pvalue.
        Rows in (sequence, window start, + before -) order, the sequences by region, then version, the reference sequence last."""
        n, st = self._kept()
        own, site, d, after, mask = self._numbers(n, st)
        data = self._leading_columns(n)
        data["strand"] = np.array(["+", "-"], dtype=object)[st]
        kmer, changes, edited = self._texts(n, st, site, mask)
        data["kmer"] = kmer
        data["score"] = scaled_scores(own, self.scale, self.offset, self.width)
        data["pvalue"] = scaled_pvalues(own, self.ptable)
        data["kind"] = KINDS[self._kinds(site, d)]
        data["distance"] = d
        data["reached"] = d <= self.max_edits
        data["changes"] = changes
        data["edited_kmer"] = edited
        data["edited_score"] = scaled_scores(after, self.scale, self.offset, self.width)
        data["edited_pvalue"] = scaled_pvalues(after, self.ptable)
        return pd.DataFrame(data)

    def summary_frame(self) -> pd.DataFrame:
        """a row per (region, non-inserted coordinate of the window's first base, strand) over the versions (not the count-0
        reference sequence) that have a window there: motif_id, motif_alt_id, sequence_name, position, strand, versions,
        haplotypes, haplotypes_site, haplotypes_near_1 .. haplotypes_near_<E> (by near d), haplotypes_far, min_site_distance (the
        smallest fragile d over the versions with a site there, E + 1: more than E, NaN: no site), best_score.  A row is kept
        when some haplotype has a site or a near-site there; all_rows keeps everything.  Rows in (region, position, + before -)
        order."""
        E = self.max_edits
        n, st = self._window_strands()
        seq = self._sequence_of(n)
        on = (self.coord[n] >= 0) & (self.seq_version[seq] >= 0)
        n, st, seq = n[on], st[on], seq[on]
        own, site, d, _, _ = self._numbers(n, st)
        kind = self._kinds(site, d)
        region, co, haps = self.seq_region[seq], self.coord[n].astype(np.int64), self.seq_count[seq]
        names = [f"haplotypes_near_{k}" for k in range(1, E + 1)]
        if not len(n):
            order, at = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        else:
            order, at = _group_heads((region, co, st))
        add = lambda v: np.add.reduceat(v[order], at) if len(at) else np.zeros(0, dtype=np.int64)   # noqa: E731
        h_site = add(np.where(kind == 2, haps, 0))
        h_near = [add(np.where((kind == 1) & (d == k), haps, 0)) for k in range(1, E + 1)]
        h_far = add(np.where(kind == 0, haps, 0))
        frag = np.where(site, d.astype(np.float64), np.inf)
        lo = np.minimum.reduceat(frag[order], at) if len(at) else np.zeros(0)
        best = np.maximum.reduceat(own[order], at) if len(at) else np.zeros(0, dtype=np.int64)
        keep = np.ones(len(at), dtype=bool) if self.all_rows else (h_site + sum(h_near, np.zeros(len(at), dtype=np.int64))) > 0
        k = np.flatnonzero(keep)
        f = order[at[k]] if len(at) else np.zeros(0, dtype=np.int64)
        data = self._motif_columns(len(k), region[f])
        data.update({"position": co[f] + 1, "strand": np.array(["+", "-"], dtype=object)[st[f]],
                     "versions": add(np.ones(len(n), dtype=np.int64))[k], "haplotypes": add(haps)[k], "haplotypes_site": h_site[k]})
        for name, h in zip(names, h_near):
            data[name] = h[k]
        data["haplotypes_far"] = h_far[k]
        data["min_site_distance"] = np.where(np.isfinite(lo[k]), lo[k], np.nan)
        data["best_score"] = scaled_scores(best[k], self.scale, self.offset, self.width)
        return pd.DataFrame(data)


def compute_site_distance_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                               haplotype_groups: Optional[Mapping] = None, max_edits: int = 3, threshold: Optional[float] = None,
                               all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> List[SiteDistance]:
    """One SiteDistance per motif, in the order of `motifs` (see the module's docstring).  `graph` / `regions` as
    compute_haplotype_sequences takes them.  The sequences are the mutation scan's: the versions of
    compute_haplotype_sequences(coordinates=True), the reference sequence of a region added where no version is the
    reference's.  One kernel call per motif width (in chunks of motifs under `max_bytes`).  args_obj: noreverse and threshold
    (`threshold` overrides it); a motif's cutoff is cutoff_of its tail table at the threshold.  `max_edits`: the cap E in
    1 .. 8.  The frames keep the sites and the near-sites; `all_rows` keeps every window-strand."""
    max_edits = checked_edits(max_edits)
    seqs, region_names, group_names, forward_only, threshold = scan_inputs(
        "the site distance", motifs, graph, regions, debug, args_obj, chrom_names, haplotype_groups, None, None, threshold)
    return tables_by_width(
        motifs, None,
        lambda ms, _: _scan_chunked(ms, seqs[5], seqs[6], None, threshold, max_edits, forward_only, max_bytes),
        lambda motif, W, numbers, cutoff, got: SiteDistance(motif.motif_id, motif.motif_name, W, *numbers, strand_tables(motif), cutoff,
                                                            max_edits, threshold, region_names, group_names, *seqs, *got, all_rows))


def compute_site_distance(motif, graph, regions, debug: bool, args_obj, chrom_names=None, haplotype_groups: Optional[Mapping] = None,
                          max_edits: int = 3, threshold: Optional[float] = None, all_rows: bool = False,
                          max_bytes: int = DEFAULT_MAX_BYTES) -> SiteDistance:
    """The site distance of `motif` (compute_site_distance_many for one motif)"""
    return compute_site_distance_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_groups, max_edits, threshold,
                                      all_rows, max_bytes)[0]


# grafimo_site_distance[_<motif_id>].tsv, grafimo_site_distance_summary[_<motif_id>].tsv (a row per (region, coordinate, strand)),
# and -f: both on stdout
write_site_distance, write_site_distance_summary, print_site_distance = table_writers(DETAIL_FILE, SUMMARY_FILE)
