"""Mutation scan: in-silico saturation mutagenesis -- every single-base change at every base of every version
(haplotype_sequences) the panel spells in a region, and of the reference sequence: which changes create or destroy a site, by
how much the total affinity moves, and on how many haplotypes.  Where query_variants answers "what does THIS variant do on every
background", this table answers "what does EVERY possible SNV do", also at the bases the panel's insertions spell, which no VCF
row can name.

THE RULE (include/grafimo_hip.h states it for the library; tests/mutation_scan_bruteforce.py on the host).  For a sequence x of
n bases and a motif of width W, for every offset o in 0 .. n - 1 and every base b in A, C, G, T:
  y = x with y[o] = b.
  REF side: the window starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).
  ALT side: the same starts in y.
  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY (--no-reverse).
  A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
  Per side: the best window by (score descending, s ascending, + before -), as the key
  ((score + 1) << 8) | ((64 - (s - o)) << 1) | plus -- query_variants.decode_keys' encoding, with s - o in -(W - 1) .. 0; key 0
  means the side has no window (n < W) --, and the exact uint64 sum of w[score] over the side's windows and strands.
  b equal to the folded x[o] gives ALT equal to REF.
  An x[o] that is no base has an all-min_val REF side, and each b can repair it.
By construction the result for a non-inserted o and b != x[o] is field for field what query_variants.score_edits returns for
the edit (coord[o], x[o], b) applied to x.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_mutation_scan.hpp, gfm_sequence_mutation_scan): every window of a sequence is
scored once, the 4 n changes are derived from the stored sums.  Everything from the kernel's arrays to the frames is numpy
group-bys; there is no Python step per row or per base.
"""
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from .query_variants import decode_keys
from .sequence_scans import (_COLUMN_OF, _LETTERS, _UPPER, DEFAULT_MAX_BYTES, TO_BASES, ScanTable, _checked_sequences,  # noqa: F401
                             effect_codes, group_summary, keep_rows, printed_windows, scan_chunked, scan_inputs, table_writers,
                             tables_by_width)

DETAIL_FILE = "grafimo_mutation_scan"
SUMMARY_FILE = "grafimo_mutation_scan_summary"
ENTRY = "gfm_sequence_mutation_scan"
COLUMNS = ("REF", "A", "C", "G", "T")                    # the five columns of the kernel's arrays
BYTES_PER_BASE = len(COLUMNS) * (4 + 8)                  # a motif's keys and sums per base


def scan_sequences(motifs: Sequence, seq_offsets, bases, weights: Optional[Sequence[np.ndarray]] = None, temperature: float = 1.0,
                   forward_only: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The kernel on plain arrays: sequences (`seq_offsets` int64 [V + 1] from 0, `bases` uint8) for motifs of ONE width -> per
    motif (keys uint32 [n_bases, 5], sums uint64 [n_bases, 5]), the columns REF, A, C, G, T (decode_keys reads a key).  `weights`:
    a uint64 table per motif, default haplotype_affinity.default_weights at `temperature`.  The motifs are taken in chunks whose
    result tensors stay under `max_bytes`; a single motif above it is a ValueError that names it.  The library refuses motifs
    of two widths and weights that can overflow a sum."""
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    return scan_chunked(motifs, seq_offsets, bases, weights, temperature, forward_only, max_bytes, ENTRY,
                        (len(bases), len(COLUMNS)))[0]


# ---------------------------------------------------------------------------------------------------------------- the table
class MutationScan(ScanTable):
    """The table of one motif over S sequences of N bases in all (see the module's docstring).
    Per sequence [S]: seq_region (the caller's region row), seq_version (the version's number in its region, -1: the region's
    reference sequence, which no haplotype spells), seq_count (haplotypes), seq_group_counts [S, G], seq_is_reference,
    seq_offsets int64 [S + 1].
    Per base [N]: bases uint8, coord int32 (~coordinate for an inserted base), and the dense arrays keys uint32 [N, 5] and sums
    uint64 [N, 5] with the columns REF, A, C, G, T -- a mutagenesis heat map needs nothing else:
    log2_affinity()[a:b, 1:] - log2_affinity()[a:b, :1] is the map of the sequence whose bases are a .. b - 1."""

    COLUMNS = COLUMNS

    def _cells(self):
        """every (base, to-base != from-base) cell -> (base index n, column c in 1 .. 4), in (n, c) order"""
        frm = _COLUMN_OF[self.bases]
        cell = np.arange(1, 5, dtype=np.int64)[None, :] != frm[:, None]
        n, c = np.nonzero(cell)
        return n.astype(np.int64), c.astype(np.int64) + 1

    @staticmethod
    def _sides(n, c):
        return (n, 0), (n, c)

    def _kmers(self, n, c, side: str) -> np.ndarray:
        """object: the best window of the side as printed ('-': reverse complemented), '' where there is none"""
        W = self.width
        key = self.keys[n, 0 if side == "ref" else c]
        _, rel, strand = decode_keys(key)
        some = key > 0
        if not len(n):
            return np.zeros(0, dtype=object)
        start = np.where(some, n + rel, 0)
        idx = np.minimum(start[:, None] + np.arange(W, dtype=np.int64)[None, :], max(len(self.bases) - 1, 0))
        text = _UPPER[self.bases[idx]]
        if side == "alt":
            text[np.flatnonzero(some), (-rel)[some]] = TO_BASES[c[some] - 1]
        out = printed_windows(text, strand == "-")
        out[~some] = ""
        return out

    def to_frame(self) -> pd.DataFrame:
        """a row per (region, version, offset, to-base != from-base) the filter keeps (keep_rows): motif_id, motif_alt_id,
        sequence_name, version (-1: the reference sequence, no haplotype spells it), haplotypes, one haplotypes_<GROUP> per group,
        is_reference, position (1-based coordinate; an inserted base has its anchor's), inserted, from, to, ref_score,
        ref_pvalue, ref_start (the best window's start minus the changed base's offset, -(W - 1) .. 0), ref_strand, ref_kmer,
        alt_score .. alt_kmer, ref_log2_affinity, alt_log2_affinity, delta_log2_affinity, effect -- NaN or empty where the
        sequence is shorter than the motif.  Rows in (sequence, offset, to A C G T) order, the sequences by region, then version,
        the reference sequence last."""
        n, c = self._kept_cells()
        data = self._leading_columns(n)
        data["from"] = _LETTERS[_UPPER[self.bases[n]]]
        data["to"] = _LETTERS[TO_BASES[c - 1]]
        return self._detail_frame(n, c, data)

    def summary_frame(self) -> pd.DataFrame:
        """a row per (region, coordinate, from, to) over the versions (not the count-0 reference sequence) that carry that
        coordinate non-inserted with that base: motif_id, motif_alt_id, sequence_name, position, from, to, versions, haplotypes,
        haplotypes_gain, haplotypes_loss, min_delta_log2_affinity, max_delta_log2_affinity, best_alt_score.  A row is kept when
        some haplotype gains or loses, or when a delta is given and the smallest or largest delta reaches it; all_rows keeps
        everything.  Rows in (region, position, from, to A C G T) order."""
        n, c = self._cells()
        seq = self._sequence_of(n)
        on = (self.coord[n] >= 0) & (self.seq_version[seq] >= 0)
        n, c, seq = n[on], c[on], seq[on]
        frm = _UPPER[self.bases[n]].astype(np.int64)
        return self._summary_frame(n, c, seq, (frm, c), lambda f: {"from": _LETTERS[frm[f]], "to": _LETTERS[TO_BASES[c[f] - 1]]})


def compute_mutation_scan_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                               haplotype_groups: Optional[Mapping] = None, weights: Optional[Sequence[np.ndarray]] = None,
                               temperature: float = 1.0, threshold: Optional[float] = None, delta: Optional[float] = None,
                               all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> List[MutationScan]:
    """One MutationScan per motif, in the order of `motifs` (see the module's docstring).  `graph` / `regions` as
    compute_haplotype_sequences takes them.  The versions come from compute_haplotype_sequences(coordinates=True); the reference
    sequence of a region is added where no version is the reference's.  One kernel call per motif width (in chunks of motifs
    under `max_bytes`).  args_obj: noreverse and threshold (`threshold` overrides it).  `temperature` / `weights` as
    compute_haplotype_affinity_many's.  The frames keep a row when its effect is gain or loss, or when |delta_log2_affinity| >=
    `delta` if a delta is given; `all_rows` keeps everything."""
    seqs, region_names, group_names, forward_only, threshold = scan_inputs(
        "the mutation scan", motifs, graph, regions, debug, args_obj, chrom_names, haplotype_groups, weights, delta, threshold)
    return tables_by_width(
        motifs, weights,
        lambda ms, ws: scan_chunked(ms, seqs[5], seqs[6], ws, temperature, forward_only, max_bytes, ENTRY,
                                    (len(seqs[6]), len(COLUMNS))),
        lambda motif, W, numbers, log2_offset, got: MutationScan(motif.motif_id, motif.motif_name, W, *numbers, log2_offset, threshold,
                                                                 region_names, group_names, *seqs, *got, delta, all_rows))


def compute_mutation_scan(motif, graph, regions, debug: bool, args_obj, chrom_names=None, haplotype_groups: Optional[Mapping] = None,
                          weights: Optional[np.ndarray] = None, temperature: float = 1.0, threshold: Optional[float] = None,
                          delta: Optional[float] = None, all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> MutationScan:
    """The mutation scan of `motif` (compute_mutation_scan_many for one motif)"""
    return compute_mutation_scan_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_groups,
                                      None if weights is None else [weights], temperature, threshold, delta, all_rows, max_bytes)[0]


# grafimo_mutation_scan[_<motif_id>].tsv, grafimo_mutation_scan_summary[_<motif_id>].tsv (a row per (region, coordinate, from,
# to)), and -f: both on stdout
write_mutation_scan, write_mutation_scan_summary, print_mutation_scan = table_writers(DETAIL_FILE, SUMMARY_FILE)
