"""Indel scan: the companion of the mutation scan for one-base indels -- the deletion of every base and the insertion of A, C, G
and T behind every base of every version (haplotype_sequences) the panel spells in a region, and of the reference sequence:
which indels create or destroy a site, by how much the total affinity moves, and on how many haplotypes.  An indel shifts
every downstream column of a motif, so it cannot be read off the substitution heat map; and as there, the bases a panel
insertion spells are scanned like any other, which no VCF row can name.

THE RULE (include/grafimo_hip.h states it for the library; tests/indel_scan_bruteforce.py on the host).  For a sequence x of
n bases, a motif of width W, and every offset o in 0 .. n - 1:
  Deletion of x[o].  y = x[:o] + x[o+1:].  This is gfm_graph_query_edits' rule with lr = 1, la = 0 at offset o.
    REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).  This is exactly the mutation
    scan's REF column.
    ALT side (column DEL): the starts of y across the junction, max(0, o - W + 1) <= s <= min(o - 1, n - 1 - W).
  Insertion of b in A, C, G, T behind x[o].  y = x[:o+1] + b + x[o+1:].  This is the query rule with lr = 0, la = 1 at offset
  o' = o + 1.
    REF side (column JUNCTION): the starts of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).
    ALT side (columns INS_A, INS_C, INS_G, INS_T): the starts of y with max(0, o' - W + 1) <= s <= min(o', n + 1 - W).
  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY (--no-reverse).
  A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
  Per column, the best window by (score descending, s ascending, + before -), as the key
  ((score + 1) << 8) | ((64 - rel) << 1) | plus, rel = s - o for COVER and DEL, rel = s - (o + 1) for JUNCTION and INS_*: the
  values a gfm_edit_record_t of the same edit holds.  Key 0 means the side has no window.
  Per column, the exact uint64 sum of w[score] over the side's windows and strands.
  A deleted N can repair its windows.  An N elsewhere leaves its windows at min_val.  An insertion before the first base of a
  sequence is not scanned: every row has the base it is anchored to, as a VCF row has.  An empty sequence has no rows.
By construction the columns equal, field for field, what query_variants.score_edits returns for the deletion (coord[o], x[o],
"") and the insertion (coord[o] + 1, "", b) applied to x, wherever a coordinate can name the edit.

THE FRAMES REPORT A CHANGE ONCE.  In a homopolymer several changes spell the same y; the frames keep the leftmost offset: a
deletion at o > 0 with folded x[o - 1] == x[o] is dropped, and so is an insertion of b behind x[o] with o > 0 and folded
x[o] == b (it is the insertion of b behind x[o - 1]).  The dense arrays keep every cell.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_indel_scan.hpp, gfm_sequence_indel_scan): every window start of a sequence is
scored once, and every window of the 5 n edited sequences is put together from two stored pieces.  Everything from the
kernel's arrays to the frames is numpy group-bys; there is no Python step per row or per base.
"""
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from .query_variants import decode_keys
from .sequence_scans import (_LETTERS, _UPPER, DEFAULT_MAX_BYTES, TO_BASES, ScanTable, _checked_sequences, printed_windows,
                             scan_chunked, scan_inputs, table_writers, tables_by_width)

DETAIL_FILE = "grafimo_indel_scan"
SUMMARY_FILE = "grafimo_indel_scan_summary"
ENTRY = "gfm_sequence_indel_scan"
COLUMNS = ("COVER", "DEL", "JUNCTION", "INS_A", "INS_C", "INS_G", "INS_T")       # the seven columns of the kernel's arrays
COVER, DEL, JUNCTION, INS_A = 0, 1, 2, 3
REL_ANCHOR = np.array([0, 0, 1, 1, 1, 1, 1], dtype=np.int64)      # a column's window starts at o + REL_ANCHOR + the key's rel
CHANGE_COLUMNS = np.array([1, 3, 4, 5, 6], dtype=np.int64)        # the ALT column of a base's five changes, in the frames' order
BYTES_PER_BASE = len(COLUMNS) * (4 + 8)                           # a motif's keys and sums per base: 84


def scan_sequences(motifs: Sequence, seq_offsets, bases, weights: Optional[Sequence[np.ndarray]] = None, temperature: float = 1.0,
                   forward_only: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The kernel on plain arrays: sequences (`seq_offsets` int64 [V + 1] from 0, `bases` uint8) for motifs of ONE width -> per
    motif (keys uint32 [n_bases, 7], sums uint64 [n_bases, 7]), the columns COVER, DEL, JUNCTION, INS_A, INS_C, INS_G, INS_T
    (decode_keys reads a key; REL_ANCHOR says what its start is relative to).  `weights`: a uint64 table per motif, default
    haplotype_affinity.default_weights at `temperature`.  The motifs are taken in chunks whose result tensors (84 bytes a base
    and motif) stay under `max_bytes`; a single motif above it is a ValueError that names it.  The library refuses motifs of
    two widths and weights that can overflow a sum."""
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    return scan_chunked(motifs, seq_offsets, bases, weights, temperature, forward_only, max_bytes, ENTRY,
                        (len(bases), len(COLUMNS)))[0]


def leftmost_changes(seq_offsets, bases) -> np.ndarray:
    """bool [N, 5], the changes DEL, INS A, INS C, INS G, INS T of every base: False where the same edited sequence is made at
    the offset before (see the module's docstring)"""
    seq_offsets, bases = np.asarray(seq_offsets, dtype=np.int64), np.asarray(bases, dtype=np.uint8)
    N = len(bases)
    up = _UPPER[bases]
    inner = np.ones(N, dtype=bool)                                # o > 0 in its sequence
    inner[seq_offsets[:-1][np.diff(seq_offsets) > 0]] = False
    keep = np.ones((N, 5), dtype=bool)
    if N:
        keep[1:, 0] = ~(inner[1:] & (up[1:] == up[:-1]))
        keep[:, 1:] = ~(inner[:, None] & (up[:, None] == TO_BASES[None, :]))
    return keep


class IndelScan(ScanTable):
    """The table of one motif over S sequences of N bases in all (see the module's docstring).
    Per sequence [S]: seq_region, seq_version (-1: the region's reference sequence, which no haplotype spells), seq_count,
    seq_group_counts [S, G], seq_is_reference, seq_offsets int64 [S + 1] -- as MutationScan's.
    Per base [N]: bases uint8, coord int32 (~coordinate for an inserted base), and the dense arrays keys uint32 [N, 7] and sums
    uint64 [N, 7] with the columns COVER, DEL, JUNCTION, INS_A, INS_C, INS_G, INS_T: the deletion of base n compares column 1
    with column 0, the insertion of b behind it column 3 .. 6 with column 2."""

    COLUMNS = COLUMNS

    def _cells(self):
        """every (base, change) cell the homopolymer rule keeps -> (base index n, ALT column c in 1, 3 .. 6), in (n, DEL, INS A
        C G T) order"""
        n, k = np.nonzero(leftmost_changes(self.seq_offsets, self.bases))
        return n.astype(np.int64), CHANGE_COLUMNS[k]

    @staticmethod
    def _ref_column(c):
        return np.where(c == DEL, COVER, JUNCTION)

    def _sides(self, n, c):
        return (n, self._ref_column(c)), (n, c)

    def _change_base(self, n, c) -> np.ndarray:
        """uint8: the deleted base (folded to upper case) or the inserted one"""
        return np.where(c == DEL, _UPPER[self.bases[n]], TO_BASES[np.maximum(c - INS_A, 0)])

    def _kmers(self, n, c, side: str) -> np.ndarray:
        """object: the best window of the side as printed ('-': reverse complemented), '' where there is none.  The REF side's
        is read from x, the ALT side's from the edited sequence y."""
        W = self.width
        if not len(n):
            return np.zeros(0, dtype=object)
        col = self._ref_column(c) if side == "ref" else c
        key = self.keys[n, col]
        _, rel, strand = decode_keys(key)
        some = key > 0
        start = np.where(some, n + REL_ANCHOR[col] + rel, 0)      # (in x for the REF side, in y for the ALT side)
        at = start[:, None] + np.arange(W, dtype=np.int64)[None, :]
        if side == "alt":
            # y's base i is x's i before the edit; behind it x's i + 1 (a deletion at n) or i - 1 (an insertion at n + 1)
            dele = (c == DEL)[:, None]
            at = np.where(dele, at + (at >= n[:, None]), at - (at > n[:, None] + 1))
        text = _UPPER[self.bases[np.clip(at, 0, max(len(self.bases) - 1, 0))]]
        if side == "alt":
            ins = np.flatnonzero(some & (c != DEL))
            text[ins, (-rel)[ins]] = TO_BASES[c[ins] - INS_A]
        out = printed_windows(text, strand == "-")
        out[~some] = ""
        return out

    def to_frame(self) -> pd.DataFrame:
        """a row per (region, version, offset, change) the filter keeps (mutation_scan.keep_rows) and the homopolymer rule does
        not drop: motif_id, motif_alt_id, sequence_name, version (-1: the reference sequence, no haplotype spells it),
        haplotypes, one haplotypes_<GROUP> per group, is_reference, position (the 1-based coordinate of x[o], the deleted base
        or the base the insertion goes behind; an inserted base has its anchor's), inserted, type (DEL / INS), base (the
        deleted or the inserted base), ref_score, ref_pvalue, ref_start (the best window's start minus o for a deletion, minus
        o + 1 for an insertion), ref_strand, ref_kmer (read from x), alt_score .. alt_kmer (read from the edited sequence),
        ref_log2_affinity, alt_log2_affinity, delta_log2_affinity, effect -- NaN or empty where a side has no window.  Rows in
        (sequence, offset, DEL, INS A C G T) order, the sequences by region, then version, the reference sequence last."""
        n, c = self._kept_cells()
        data = self._leading_columns(n)
        data["type"] = np.where(c == DEL, "DEL", "INS").astype(object)
        data["base"] = _LETTERS[self._change_base(n, c)]
        return self._detail_frame(n, c, data)

    def summary_frame(self) -> pd.DataFrame:
        """a row per (region, coordinate, type, base) over the versions (not the count-0 reference sequence) that carry that
        coordinate non-inserted and where the homopolymer rule keeps the change: motif_id, motif_alt_id, sequence_name,
        position, type, base, versions, haplotypes, haplotypes_gain, haplotypes_loss, min_delta_log2_affinity,
        max_delta_log2_affinity, best_alt_score.  A row is kept when some haplotype gains or loses, or when a delta is given and
        the smallest or largest delta reaches it; all_rows keeps everything.  Rows in (region, position, DEL before INS, base)
        order."""
        n, c = self._cells()
        seq = self._sequence_of(n)
        on = (self.coord[n] >= 0) & (self.seq_version[seq] >= 0)
        n, c, seq = n[on], c[on], seq[on]
        kind, base = (c != DEL).astype(np.int64), self._change_base(n, c).astype(np.int64)
        return self._summary_frame(n, c, seq, (kind, base), lambda f: {"type": np.where(kind[f] == 0, "DEL", "INS").astype(object),
                                                                       "base": _LETTERS[base[f]]})


def compute_indel_scan_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                            haplotype_groups: Optional[Mapping] = None, weights: Optional[Sequence[np.ndarray]] = None,
                            temperature: float = 1.0, threshold: Optional[float] = None, delta: Optional[float] = None,
                            all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> List[IndelScan]:
    """One IndelScan per motif, in the order of `motifs` (see the module's docstring).  The arguments and the sequences are
    compute_mutation_scan_many's: the versions of compute_haplotype_sequences(coordinates=True), the reference sequence of a
    region added where no version is the reference's; one kernel call per motif width (in chunks of motifs under
    `max_bytes`).  args_obj: noreverse and threshold (`threshold` overrides it).  The frames keep a row when its effect is gain
    or loss, or when |delta_log2_affinity| >= `delta` if a delta is given; `all_rows` keeps everything."""
    seqs, region_names, group_names, forward_only, threshold = scan_inputs(
        "the indel scan", motifs, graph, regions, debug, args_obj, chrom_names, haplotype_groups, weights, delta, threshold)
    return tables_by_width(
        motifs, weights,
        lambda ms, ws: scan_chunked(ms, seqs[5], seqs[6], ws, temperature, forward_only, max_bytes, ENTRY,
                                    (len(seqs[6]), len(COLUMNS))),
        lambda motif, W, numbers, log2_offset, got: IndelScan(motif.motif_id, motif.motif_name, W, *numbers, log2_offset, threshold,
                                                              region_names, group_names, *seqs, *got, delta, all_rows))


def compute_indel_scan(motif, graph, regions, debug: bool, args_obj, chrom_names=None, haplotype_groups: Optional[Mapping] = None,
                       weights: Optional[np.ndarray] = None, temperature: float = 1.0, threshold: Optional[float] = None,
                       delta: Optional[float] = None, all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> IndelScan:
    """The indel scan of `motif` (compute_indel_scan_many for one motif)"""
    return compute_indel_scan_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_groups,
                                   None if weights is None else [weights], temperature, threshold, delta, all_rows, max_bytes)[0]


# grafimo_indel_scan[_<motif_id>].tsv, grafimo_indel_scan_summary[_<motif_id>].tsv (a row per (region, coordinate, type, base)),
# and -f: both on stdout
write_indel_scan, write_indel_scan_summary, print_indel_scan = table_writers(DETAIL_FILE, SUMMARY_FILE)
