"""Deletion scan: the companion of the indel scan for block deletions -- the deletion of every block of L bases, for a list of
lengths L in 1 .. 64, at every offset of every version (haplotype_sequences) the panel spells in a region, and of the
reference sequence: which tiling deletions (CRISPR deletion screens, linker-scanning mutants, MPRA deletion series) create or
destroy a site, by how much the total affinity moves, and on how many haplotypes.  A block deletion removes up to L + W - 1
windows at once and creates W - 1 junction windows whose halves were never neighbours, so it cannot be read off the one-base
scans; and as there, the bases a panel insertion spells are scanned like any other, which no VCF row can name.

THE RULE (include/grafimo_hip.h states it for the library; tests/deletion_scan_bruteforce.py on the host).  For a sequence x
of n bases, a motif of width W, a strictly ascending list of lengths L0 < L1 < .. with every L in 1 .. 64, every length L of
the list and every offset o in 0 .. n - 1:
  If o + L > n there is no edit: both keys and both sums of the cell are 0.
  Otherwise y = x[:o] + x[o+L:].  This is gfm_graph_query_edits' rule with lr = L, la = 0 at offset o.
    REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o + L - 1, n - W).
    ALT side (column DEL): the starts of y across the junction, max(0, o - W + 1) <= s <= min(o - 1, n - L - W).
  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY (--no-reverse).
  A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
  A deleted N can repair its junction windows.  An N elsewhere cannot be repaired.
  Per column, the best window by (score descending, s ascending, + before -), as the key
  ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. L - 1 for COVER and in -(W - 1) .. -1 for DEL.
  Key 0 means the side has no window.
  Per column, the exact uint64 sum of w[score] over the side's windows and strands.
  At L = 1 the two columns equal the indel scan's COVER and DEL bit for bit.
By construction a cell equals, field for field, what query_variants.score_edits returns for the deletion (coord[o],
x[o : o + L], "") applied to x, wherever coordinates can name the block.

THE FRAMES REPORT A CHANGE ONCE.  In a repeat several blocks spell the same y; the detail rows keep the leftmost offset: a
deletion of L bases at o > 0 with folded x[o - 1] == x[o + L - 1] is dropped (it is the deletion at o - 1).  The dense arrays
keep every cell, and the summary, which is about coordinates, keeps every block a coordinate can name.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_deletion_scan.hpp, gfm_sequence_deletion_scan): every window start of a
sequence is scored once for all lengths, and every junction window is put together from two stored pieces.  Everything from
the kernel's arrays to the frames is numpy group-bys; there is no Python step per row or per base.
"""
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .query_variants import decode_keys
from .sequence_scans import (_UPPER, DEFAULT_MAX_BYTES, ScanTable, _checked_sequences, _within, fixed_text, printed_windows,
                             scan_chunked, scan_inputs, table_writers, tables_by_width)

DETAIL_FILE = "grafimo_deletion_scan"
SUMMARY_FILE = "grafimo_deletion_scan_summary"
ENTRY = "gfm_sequence_deletion_scan"
COLUMNS = ("COVER", "DEL")                               # the two columns of the kernel's arrays
COVER, DEL = 0, 1
MAX_LENGTH = nv.GFM_DELSCAN_MAX_LENGTH
BYTES_PER_CELL = len(COLUMNS) * (4 + 8)                  # a motif's keys and sums per base and length: 24


def checked_lengths(lengths) -> np.ndarray:
    """int32 [n_lengths] of a strictly ascending list of integers in 1 .. 64; anything else is a ValueError"""
    got = np.asarray(lengths)
    if got.ndim != 1 or got.size == 0 or got.dtype.kind not in "iu":
        raise ValueError(f"lengths {lengths!r}: a non-empty list of integers in 1 .. {MAX_LENGTH}")
    got = got.astype(np.int64)
    if int(got.min()) < 1 or int(got.max()) > MAX_LENGTH:
        raise ValueError(f"lengths {got.tolist()}: every length lies in 1 .. {MAX_LENGTH}")
    if np.any(np.diff(got) <= 0):
        raise ValueError(f"lengths {got.tolist()}: they must strictly ascend")
    return np.ascontiguousarray(got, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _scan_chunked(motifs: Sequence, seq_offsets, bases, lengths, weights, temperature, forward_only, max_bytes,
                  entry: str = ENTRY, extra: Sequence = ()):
    """-> (per motif (keys, sums) [n_lengths, N, 2], per motif its log2 offset, per motif (scale, offset, ptable)) of a block scan
    (`entry`; `extra`: its arguments behind the lengths): the motifs leased and scanned in chunks whose result tensors (24 bytes a
    base, length and motif) stay under max_bytes"""
    K = len(lengths)
    return scan_chunked(motifs, seq_offsets, bases, weights, temperature, forward_only, max_bytes, entry, (K, len(bases), len(COLUMNS)),
                        (K, lengths.ctypes.data, *extra), f" and {K} lengths", " or lengths")


def scan_sequences(motifs: Sequence, seq_offsets, bases, lengths, weights: Optional[Sequence[np.ndarray]] = None,
                   temperature: float = 1.0, forward_only: bool = False,
                   max_bytes: int = DEFAULT_MAX_BYTES) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The kernel on plain arrays: sequences (`seq_offsets` int64 [V + 1] from 0, `bases` uint8) for motifs of ONE width and a
    strictly ascending list of `lengths` in 1 .. 64 -> per motif (keys uint32 [n_lengths, n_bases, 2], sums uint64
    [n_lengths, n_bases, 2]), the columns COVER, DEL (decode_keys reads a key; its start is relative to the block's offset).
    `weights`: a uint64 table per motif, default haplotype_affinity.default_weights at `temperature`.  The motifs are taken in
    chunks whose result tensors (24 bytes a base, length and motif) stay under `max_bytes`; a single motif above it is a
    ValueError that names it, and so are bad lengths, before the library is called.  The library refuses motifs of two widths
    and weights that can overflow a sum."""
    lengths = checked_lengths(lengths)
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    return _scan_chunked(motifs, seq_offsets, bases, lengths, weights, temperature, forward_only, max_bytes)[0]


def leftmost_deletions(seq_offsets, bases, lengths) -> np.ndarray:
    """bool [n_lengths, N]: False where o + L > n (there is no edit), and where the same edited sequence is made at the offset
    before: o > 0 in its sequence and folded x[o - 1] == x[o + L - 1] (see the module's docstring)"""
    seq_offsets, bases = np.asarray(seq_offsets, dtype=np.int64), np.asarray(bases, dtype=np.uint8)
    L = np.asarray(lengths, dtype=np.int64)
    N = len(bases)
    if N == 0:
        return np.zeros((len(L), 0), dtype=bool)
    up = _UPPER[bases]
    within, left = _within(seq_offsets, N)
    fits = L[:, None] <= left[None, :]
    last = np.minimum(np.arange(N, dtype=np.int64)[None, :] + L[:, None] - 1, N - 1)
    before = up[np.maximum(np.arange(N, dtype=np.int64) - 1, 0)]
    repeat = (within > 0)[None, :] & (before[None, :] == up[last])
    return fits & ~repeat


class DeletionScan(ScanTable):
    """The table of one motif over S sequences of N bases in all and K lengths (see the module's docstring).
    Per sequence [S]: seq_region, seq_version (-1: the region's reference sequence, which no haplotype spells), seq_count,
    seq_group_counts [S, G], seq_is_reference, seq_offsets int64 [S + 1] -- as IndelScan's.
    Per base [N]: bases uint8, coord int32 (~coordinate for an inserted base).  lengths int32 [K], strictly ascending.  The
    dense arrays keys uint32 [K, N, 2] and sums uint64 [K, N, 2] with the columns COVER, DEL: the deletion of lengths[k] bases
    from base n on compares column 1 with column 0; a block that does not fit its sequence has four zeros."""

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                 seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, lengths, keys,
                 sums, delta=None, all_rows=False):
        self.lengths = checked_lengths(lengths)
        super().__init__(motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                         seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, keys, sums,
                         delta, all_rows)

    def _shape(self):
        return (len(self.lengths), len(self.bases), 2), "the sequences and lengths"

    def named_blocks(self) -> np.ndarray:
        """bool [K, N]: the block fits its sequence, its bases are non-inserted and their coordinates consecutive -- what a
        VCF row could name"""
        N, L = len(self.bases), self.lengths.astype(np.int64)
        if N == 0:
            return np.zeros((len(L), 0), dtype=bool)
        co = self.coord.astype(np.int64)
        fits = L[:, None] <= _within(self.seq_offsets, N)[1][None, :]
        step = np.zeros(N, dtype=np.int64)                        # base i and base i + 1 do NOT follow each other by coordinate
        step[:-1] = ~((co[:-1] >= 0) & (co[1:] == co[:-1] + 1))
        breaks = np.concatenate([[0], np.cumsum(step)])           # breaks[j] - breaks[i]: among the steps i .. j - 1
        at = np.arange(N, dtype=np.int64)[None, :]
        last = np.minimum(at + L[:, None] - 1, N - 1)
        return fits & (co >= 0)[None, :] & (breaks[last] == breaks[at])

    def _cells(self, every: bool = False):
        """the (base, length) cells of the detail rows -> (base index n, length index k), in (n, k) order: those the repeat rule
        keeps; `every`: all whose block fits its sequence"""
        if every:
            N = len(self.bases)
            keep = (self.lengths.astype(np.int64)[:, None] <= _within(self.seq_offsets, N)[1][None, :]) if N else \
                np.zeros((len(self.lengths), 0), dtype=bool)
        else:
            keep = leftmost_deletions(self.seq_offsets, self.bases, self.lengths)
        n, k = np.nonzero(keep.T)
        return n.astype(np.int64), k.astype(np.int64)

    @staticmethod
    def _sides(n, k):
        return (k, n, 0), (k, n, 1)

    def _deleted(self, n, k) -> np.ndarray:
        """object: the deleted bases, upper case"""
        if not len(n):
            return np.zeros(0, dtype=object)
        L = self.lengths.astype(np.int64)[k]
        width = int(L.max())
        j = np.arange(width, dtype=np.int64)[None, :]
        text = _UPPER[self.bases[np.minimum(n[:, None] + j, len(self.bases) - 1)]]
        text[j >= L[:, None]] = 0                                 # (a fixed-width byte string drops its trailing zeros)
        return fixed_text(text)

    def _kmers(self, n, k, side: str) -> np.ndarray:
        """object: the best window of the side as printed ('-': reverse complemented), '' where there is none.  The REF side's
        is read from x, the ALT side's from the edited sequence y."""
        W = self.width
        if not len(n):
            return np.zeros(0, dtype=object)
        key = self.keys[k, n, COVER if side == "ref" else DEL]
        _, rel, strand = decode_keys(key)
        some = key > 0
        at = np.where(some, n + rel, 0)[:, None] + np.arange(W, dtype=np.int64)[None, :]
        if side == "alt":                                         # y's base i is x's i before the block, x's i + L behind it
            at = at + np.where(at >= n[:, None], self.lengths.astype(np.int64)[k][:, None], 0)
        text = _UPPER[self.bases[np.clip(at, 0, max(len(self.bases) - 1, 0))]]
        out = printed_windows(text, strand == "-")
        out[~some] = ""
        return out

    def to_frame(self) -> pd.DataFrame:
        """a row per (region, version, offset, length) the filter keeps (mutation_scan.keep_rows) and the repeat rule does not
        drop: motif_id, motif_alt_id, sequence_name, version (-1: the reference sequence, no haplotype spells it), haplotypes,
        one haplotypes_<GROUP> per group, is_reference, position (the 1-based coordinate of the first deleted base; an inserted
        base has its anchor's), inserted (of the first base), length, named (the block's bases are non-inserted and their
        coordinates consecutive: a VCF row could name it), deleted (the bases, upper case), ref_score, ref_pvalue, ref_start
        (the best window's start minus o), ref_strand, ref_kmer (read from x), alt_score .. alt_kmer (read from the edited
        sequence), ref_log2_affinity, alt_log2_affinity, delta_log2_affinity, effect -- NaN or empty where a side has no
        window.  Rows in (sequence, offset, length) order, the sequences by region, then version, the reference sequence last."""
        n, k = self._kept_cells()
        data = self._block_columns(n, k)
        data["deleted"] = self._deleted(n, k)
        return self._detail_frame(n, k, data)

    def _block_columns(self, n, k) -> dict:
        """the leading columns of the blocks (n, k), then length and named"""
        data = self._leading_columns(n)
        data["length"] = self.lengths.astype(np.int64)[k]
        data["named"] = self.named_blocks()[k, n]
        return data

    def summary_frame(self) -> pd.DataFrame:
        """a row per (region, coordinate of the first deleted base, length) over the versions (not the count-0 reference
        sequence) whose block there is `named`, the blocks a repeat drops from the detail rows included (the summary is about
        coordinates): motif_id, motif_alt_id, sequence_name, position, length, versions, haplotypes, haplotypes_gain,
        haplotypes_loss, min_delta_log2_affinity, max_delta_log2_affinity, best_alt_score.  A row is kept when some haplotype
        gains or loses, or when a delta is given and the smallest or largest delta reaches it; all_rows keeps everything.  Rows
        in (region, position, length) order."""
        n, k = self._cells(every=True)
        seq = self._sequence_of(n)
        on = (self.named_blocks()[k, n] & (self.seq_version[seq] >= 0)) if len(n) else np.zeros(0, dtype=bool)
        n, k, seq = n[on], k[on], seq[on]
        length = self.lengths.astype(np.int64)[k]
        return self._summary_frame(n, k, seq, (length,), lambda f: {"length": length[f]})


def compute_deletion_scan_many(motifs: Sequence, graph, regions, debug: bool, args_obj, lengths, chrom_names=None,
                               haplotype_groups: Optional[Mapping] = None, weights: Optional[Sequence[np.ndarray]] = None,
                               temperature: float = 1.0, threshold: Optional[float] = None, delta: Optional[float] = None,
                               all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> List[DeletionScan]:
    """One DeletionScan per motif, in the order of `motifs` (see the module's docstring).  `lengths`: strictly ascending, in
    1 .. 64.  The other arguments and the sequences are compute_indel_scan_many's: the versions of
    compute_haplotype_sequences(coordinates=True), the reference sequence of a region added where no version is the
    reference's; one kernel call per motif width (in chunks of motifs under `max_bytes`).  args_obj: noreverse and threshold
    (`threshold` overrides it).  The frames keep a row when its effect is gain or loss, or when |delta_log2_affinity| >=
    `delta` if a delta is given; `all_rows` keeps everything."""
    lengths = checked_lengths(lengths)
    seqs, region_names, group_names, forward_only, threshold = scan_inputs(
        "the deletion scan", motifs, graph, regions, debug, args_obj, chrom_names, haplotype_groups, weights, delta, threshold)
    return tables_by_width(
        motifs, weights,
        lambda ms, ws: _scan_chunked(ms, seqs[5], seqs[6], lengths, ws, temperature, forward_only, max_bytes),
        lambda motif, W, numbers, log2_offset, got: DeletionScan(motif.motif_id, motif.motif_name, W, *numbers, log2_offset, threshold,
                                                                 region_names, group_names, *seqs, lengths, *got, delta, all_rows))


def compute_deletion_scan(motif, graph, regions, debug: bool, args_obj, lengths, chrom_names=None,
                          haplotype_groups: Optional[Mapping] = None, weights: Optional[np.ndarray] = None, temperature: float = 1.0,
                          threshold: Optional[float] = None, delta: Optional[float] = None, all_rows: bool = False,
                          max_bytes: int = DEFAULT_MAX_BYTES) -> DeletionScan:
    """The deletion scan of `motif` (compute_deletion_scan_many for one motif)"""
    return compute_deletion_scan_many([motif], graph, regions, debug, args_obj, lengths, chrom_names, haplotype_groups,
                                      None if weights is None else [weights], temperature, threshold, delta, all_rows, max_bytes)[0]


# grafimo_deletion_scan[_<motif_id>].tsv, grafimo_deletion_scan_summary[_<motif_id>].tsv (a row per (region, coordinate, length)),
# and -f: both on stdout
write_deletion_scan, write_deletion_scan_summary, print_deletion_scan = table_writers(DETAIL_FILE, SUMMARY_FILE)
