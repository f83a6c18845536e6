"""Substitution scan: the companion of the deletion scan for blocks replaced IN PLACE -- every block of L bases, for a list of
lengths L in 1 .. 64, at every offset of every version (haplotype_sequences) the panel spells in a region, and of the reference
sequence, replaced by its image under a base map: which tiling substitutions (MPRA tiling mutagenesis with 5 or 10 bp
transversion blocks, complement or scramble blocks, the poly-A linkers of linker-scanning mutants) create or destroy a site, by
how much the total affinity moves, and on how many haplotypes.  The length is preserved, so the spacing of the flanking sites
is kept, which no deletion does.  A block substitution changes up to W + L - 1 windows, each a mixture of old and new bases, so
it cannot be read off the single-base scan; and as there, the bases a panel insertion spells are scanned like any other.

THE RULE (include/grafimo_hip.h states it for the library; tests/substitution_scan_bruteforce.py on the host).  For a sequence
x of n bases, a motif of width W, a strictly ascending list of lengths L0 < L1 < .. with every L in 1 .. 64, a base map f
given as four codes -- the images of A, C, G, T, each in 0 .. 3 for A, C, G, T; any map is allowed: fixed points, constant
maps and the identity included --, every length L of the list and every offset o in 0 .. n - 1:
  If o + L > n there is no edit: both keys and both sums of the cell are 0.
  Otherwise y = x[:o] + f(x[o:o+L]) + x[o+L:].  f is applied base by base.  Case is folded, as base_code does.
  A base that is not A/C/G/T maps to itself: unlike a deletion, a substituted N is NOT repaired.
  This is gfm_graph_query_edits' rule with lr = la = L at offset o, the alleles not trimmed.
    REF side (column COVER): the starts s of x with max(0, o - W + 1) <= s <= min(o + L - 1, n - W).  This is bit for bit the
    deletion scan's COVER column.
    ALT side (column SUB): the same starts in y.
  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY (--no-reverse).
  A window that holds a base that is not A/C/G/T scores min_val on both strands.
  Per column, the best window by (score descending, s ascending, + before -), as the key
  ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus, s - o in -(W - 1) .. L - 1 on both sides.
  Key 0 means the side has no window.
  Per column, the exact uint64 sum of w[score] over the side's windows and strands.
  Under the identity map SUB == COVER in every cell.
  At L = 1, wherever x[o] is a base, SUB equals the mutation scan's column of the base f(x[o]), field for field.
By construction a cell equals, field for field, what query_variants.score_edits returns for the edit (coord[o], x[o : o + L],
f(x[o : o + L])) applied to x, wherever coordinates can name the block.

THE FRAMES REPORT A CHANGE ONCE.  A detail row exists only where `changed` > 0, the number of the block's bases the map moves:
a block whose every base is an N or a fixed point of the map is no edit, and the summary does not count it either.  Rows of
different lengths at one offset are kept even where their y coincide (the longer block's further bases are fixed points):
they are keyed by length, and the `changed` column says so.  The dense arrays keep every cell.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_substitution_scan.hpp, gfm_sequence_substitution_scan): every window start of
a sequence is scored once, over x and over f(x), for all lengths, and every window of every edited sequence is put together
from stored pieces.  Everything from the kernel's arrays to the frames is numpy group-bys; there is no Python step per row or
per base.
"""
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .deletion_scan import DeletionScan, _scan_chunked, checked_lengths
from .query_variants import decode_keys
from .sequence_scans import (_COLUMN_OF, _UPPER, DEFAULT_MAX_BYTES, TO_BASES, _checked_sequences, _within, fixed_text,
                             printed_windows, scan_inputs, table_writers, tables_by_width)

DETAIL_FILE = "grafimo_substitution_scan"
SUMMARY_FILE = "grafimo_substitution_scan_summary"
ENTRY = "gfm_sequence_substitution_scan"
COLUMNS = ("COVER", "SUB")                               # the two columns of the kernel's arrays
COVER, SUB = 0, 1
MAX_LENGTH = nv.GFM_SUBSCAN_MAX_LENGTH
MAPS = {"transversion": "CATG", "complement": "TGCA", "transition": "GTAC"}     # the images of A, C, G, T


def checked_map(spec) -> np.ndarray:
    """uint8 [4], the images of A, C, G, T as indices into "ACGT", of a name in MAPS or of four letters over ACGT in either
    case (a uint8 [4] this function made is taken as it is); anything else is a ValueError"""
    if isinstance(spec, np.ndarray) and spec.dtype == np.uint8 and spec.shape == (4,) and int(spec.max()) <= 3:
        return np.ascontiguousarray(spec)
    if isinstance(spec, bytes):
        spec = spec.decode("ascii", "replace")
    if not isinstance(spec, str):
        raise ValueError(f"base map {spec!r}: one of {', '.join(MAPS)}, or the images of A, C, G, T as four letters over ACGT")
    letters = MAPS.get(spec, spec).upper()
    if len(letters) != 4 or any(c not in "ACGT" for c in letters):
        raise ValueError(f"base map {spec!r}: one of {', '.join(MAPS)}, or the images of A, C, G, T as four letters over ACGT")
    return np.array(["ACGT".index(c) for c in letters], dtype=np.uint8)


def map_letters(base_map) -> str:
    """the four letters of a checked map"""
    return TO_BASES[checked_map(base_map)].tobytes().decode()


def mapped_bases(bases, base_map) -> np.ndarray:
    """uint8 [N]: f of every base, upper case; a base that is not A/C/G/T is itself, upper case"""
    up = _UPPER[np.asarray(bases, dtype=np.uint8)]
    col = _COLUMN_OF[up]
    return np.where(col > 0, TO_BASES[checked_map(base_map)][np.maximum(col, 1) - 1], up).astype(np.uint8)


def changed_bases(seq_offsets, bases, lengths, base_map) -> np.ndarray:
    """int32 [n_lengths, N]: how many bases of the block that starts at a base differ after the map; 0 where o + L > n (there
    is no edit)"""
    seq_offsets, bases = np.asarray(seq_offsets, dtype=np.int64), np.asarray(bases, dtype=np.uint8)
    L = np.asarray(lengths, dtype=np.int64)
    N = len(bases)
    if N == 0:
        return np.zeros((len(L), 0), dtype=np.int32)
    moved = np.concatenate([[0], np.cumsum(mapped_bases(bases, base_map) != _UPPER[bases])])
    at = np.arange(N, dtype=np.int64)[None, :]
    fits = L[:, None] <= _within(seq_offsets, N)[1][None, :]
    return np.where(fits, moved[np.minimum(at + L[:, None], N)] - moved[at], 0).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def scan_sequences(motifs: Sequence, seq_offsets, bases, lengths, base_map, weights: Optional[Sequence[np.ndarray]] = None,
                   temperature: float = 1.0, forward_only: bool = False,
                   max_bytes: int = DEFAULT_MAX_BYTES) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The kernel on plain arrays: sequences (`seq_offsets` int64 [V + 1] from 0, `bases` uint8) for motifs of ONE width, a
    strictly ascending list of `lengths` in 1 .. 64 and a `base_map` (checked_map: a name in MAPS or four letters) -> per motif
    (keys uint32 [n_lengths, n_bases, 2], sums uint64 [n_lengths, n_bases, 2]), the columns COVER, SUB (decode_keys reads a
    key; its start is relative to the block's offset).  `weights`: a uint64 table per motif, default
    haplotype_affinity.default_weights at `temperature`.  The motifs are taken in chunks whose result tensors (24 bytes a base,
    length and motif) stay under `max_bytes`; a single motif above it is a ValueError that names it, and so are bad lengths and
    a bad map, before the library is called.  The library refuses motifs of two widths and weights that can overflow a sum."""
    lengths, base_map = checked_lengths(lengths), checked_map(base_map)
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    return _scan_chunked(motifs, seq_offsets, bases, lengths, weights, temperature, forward_only, max_bytes, ENTRY,
                         (base_map.ctypes.data,))[0]


# ---------------------------------------------------------------------------------------------------------------- the table
class SubstitutionScan(DeletionScan):
    """The table of one motif over S sequences of N bases in all and K lengths (see the module's docstring).  The per-sequence
    and per-base arrays, the lengths and the filter are DeletionScan's; base_map uint8 [4] (checked_map).  The dense arrays keys
    uint32 [K, N, 2] and sums uint64 [K, N, 2] have the columns COVER, SUB: the substitution of lengths[k] bases from base n on
    compares column 1 with column 0; a block that does not fit its sequence has four zeros.  log2_affinity, named_blocks and the
    summary's group-by are inherited: they read the two columns by their places."""

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                 seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, lengths,
                 base_map, keys, sums, delta=None, all_rows=False):
        super().__init__(motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                         seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, lengths,
                         keys, sums, delta, all_rows)
        self.base_map = checked_map(base_map)

    def changed(self) -> np.ndarray:
        """int32 [K, N]: changed_bases of the table"""
        return changed_bases(self.seq_offsets, self.bases, self.lengths, self.base_map)

    def _cells(self, every: bool = False):
        """the (base, length) cells of the rows -> (base index n, length index k), in (n, k) order: the blocks that fit their
        sequence and change a base (`every`, the summary's: the same -- no block is another's repeat)"""
        n, k = np.nonzero(self.changed().T > 0)
        return n.astype(np.int64), k.astype(np.int64)

    def _kmers(self, n, k, side: str) -> np.ndarray:
        """object: the best window of the side as printed ('-': reverse complemented), '' where there is none.  The REF side's
        is read from x, the ALT side's from the edited sequence y."""
        W = self.width
        if not len(n):
            return np.zeros(0, dtype=object)
        key = self.keys[k, n, COVER if side == "ref" else SUB]
        _, rel, strand = decode_keys(key)
        some = key > 0
        at = np.where(some, n + rel, 0)[:, None] + np.arange(W, dtype=np.int64)[None, :]
        inside = np.clip(at, 0, max(len(self.bases) - 1, 0))
        text = _UPPER[self.bases[inside]]
        if side == "alt":                                         # y's base i is f(x[i]) inside the block, x's elsewhere
            block = (at >= n[:, None]) & (at < (n + self.lengths.astype(np.int64)[k])[:, None])
            text = np.where(block, mapped_bases(self.bases, self.base_map)[inside], text)
        out = printed_windows(text, strand == "-")
        out[~some] = ""
        return out

    def _replacement(self, n, k) -> np.ndarray:
        """object: the bases the block becomes, upper case"""
        if not len(n):
            return np.zeros(0, dtype=object)
        L = self.lengths.astype(np.int64)[k]
        width = int(L.max())
        j = np.arange(width, dtype=np.int64)[None, :]
        text = mapped_bases(self.bases, self.base_map)[np.minimum(n[:, None] + j, len(self.bases) - 1)]
        text[j >= L[:, None]] = 0                                 # (a fixed-width byte string drops its trailing zeros)
        return fixed_text(text)

    def to_frame(self) -> pd.DataFrame:
        """a row per (region, version, offset, length) the filter keeps (mutation_scan.keep_rows) whose block changes a base:
        motif_id, motif_alt_id, sequence_name, version (-1: the reference sequence, no haplotype spells it), haplotypes, one
        haplotypes_<GROUP> per group, is_reference, position (the 1-based coordinate of the block's first base; an inserted base
        has its anchor's), inserted (of the first base), length, named (the block's bases are non-inserted and their coordinates
        consecutive: a VCF row could name it), map (the images of A, C, G, T), replaced (the block's bases, upper case),
        replacement (what they become), changed (how many of them differ), ref_score, ref_pvalue, ref_start (the best window's
        start minus o), ref_strand, ref_kmer (read from x), alt_score .. alt_kmer (read from the edited sequence),
        ref_log2_affinity, alt_log2_affinity, delta_log2_affinity, effect -- NaN or empty where a side has no window.  Rows in
        (sequence, offset, length) order, the sequences by region, then version, the reference sequence last."""
        n, k = self._kept_cells()
        data = self._block_columns(n, k)
        data["map"] = np.full(len(n), map_letters(self.base_map), dtype=object)
        data["replaced"] = self._deleted(n, k)
        data["replacement"] = self._replacement(n, k)
        data["changed"] = self.changed()[k, n].astype(np.int64)
        return self._detail_frame(n, k, data)

    def summary_frame(self) -> pd.DataFrame:
        """a row per (region, coordinate of the block's first base, length) over the versions (not the count-0 reference
        sequence) whose block there is `named` and changes a base: motif_id, motif_alt_id, sequence_name, position, length,
        versions, haplotypes, haplotypes_gain, haplotypes_loss, min_delta_log2_affinity, max_delta_log2_affinity,
        best_alt_score -- the deletion summary's columns, filter and order."""
        return super().summary_frame()


def compute_substitution_scan_many(motifs: Sequence, graph, regions, debug: bool, args_obj, lengths, base_map="transversion",
                                   chrom_names=None, haplotype_groups: Optional[Mapping] = None,
                                   weights: Optional[Sequence[np.ndarray]] = None, temperature: float = 1.0,
                                   threshold: Optional[float] = None, delta: Optional[float] = None, all_rows: bool = False,
                                   max_bytes: int = DEFAULT_MAX_BYTES) -> List[SubstitutionScan]:
    """One SubstitutionScan per motif, in the order of `motifs` (see the module's docstring).  `lengths`: strictly ascending, in
    1 .. 64; `base_map`: a name in MAPS or the images of A, C, G, T as four letters.  The other arguments and the sequences are
    compute_deletion_scan_many's: the versions of compute_haplotype_sequences(coordinates=True), the reference sequence of a
    region added where no version is the reference's; one kernel call per motif width (in chunks of motifs under `max_bytes`).
    args_obj: noreverse and threshold (`threshold` overrides it).  The frames keep a row when its effect is gain or loss, or
    when |delta_log2_affinity| >= `delta` if a delta is given; `all_rows` keeps everything."""
    lengths, base_map = checked_lengths(lengths), checked_map(base_map)
    seqs, region_names, group_names, forward_only, threshold = scan_inputs(
        "the substitution scan", motifs, graph, regions, debug, args_obj, chrom_names, haplotype_groups, weights, delta, threshold)
    return tables_by_width(
        motifs, weights,
        lambda ms, ws: _scan_chunked(ms, seqs[5], seqs[6], lengths, ws, temperature, forward_only, max_bytes, ENTRY,
                                     (base_map.ctypes.data,)),
        lambda motif, W, numbers, log2_offset, got: SubstitutionScan(motif.motif_id, motif.motif_name, W, *numbers, log2_offset,
                                                                     threshold, region_names, group_names, *seqs, lengths, base_map,
                                                                     *got, delta, all_rows))


def compute_substitution_scan(motif, graph, regions, debug: bool, args_obj, lengths, base_map="transversion", chrom_names=None,
                              haplotype_groups: Optional[Mapping] = None, weights: Optional[np.ndarray] = None,
                              temperature: float = 1.0, threshold: Optional[float] = None, delta: Optional[float] = None,
                              all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> SubstitutionScan:
    """The substitution scan of `motif` (compute_substitution_scan_many for one motif)"""
    return compute_substitution_scan_many([motif], graph, regions, debug, args_obj, lengths, base_map, chrom_names, haplotype_groups,
                                          None if weights is None else [weights], temperature, threshold, delta, all_rows,
                                          max_bytes)[0]


# grafimo_substitution_scan[_<motif_id>].tsv, grafimo_substitution_scan_summary[_<motif_id>].tsv (a row per (region, coordinate,
# length)), and -f: both on stdout
write_substitution_scan, write_substitution_scan_summary, print_substitution_scan = table_writers(DETAIL_FILE, SUMMARY_FILE)
