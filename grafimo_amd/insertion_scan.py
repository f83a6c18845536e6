"""Insertion scan: the companion of the deletion scan for block insertions -- the insertion of every insert of a given list of
1 .. 16 blocks of 1 .. 64 bases behind every base of every version (haplotype_sequences) the panel spells in a region, and of
the reference sequence: where a knock-in of a consensus, loxP, FRT or att site, a 5 or 10 bp spacer, a linker, one more unit
of a repeat or a transposon's end creates or destroys a site, by how much the total affinity moves, and on how many
haplotypes.  An insert of Li bases makes up to W - 1 + Li windows that x never held, so it cannot be read off the one-base
indel scan; and as there, the bases a panel insertion spells are scanned like any other, which no VCF row can name.

THE RULE (include/grafimo_hip.h states it for the library; tests/insertion_scan_bruteforce.py on the host).  For a sequence x
of n bases, a motif of width W, a list of K inserts with K in 1 .. 16, every insert I of the list, Li its length in 1 .. 64,
and every offset o in 0 .. n - 1:
  Every insert holds A, C, G, T only.  Case is folded, as base_code does.
  The edit is the insertion of I behind x[o].  Let o' = o + 1 and y = x[:o'] + I + x[o':].
  This is gfm_graph_query_edits' rule with lr = 0, la = Li at offset o'.
    REF side (column JUNCTION): the starts s of x across the junction, max(0, o' - W + 1) <= s <= min(o' - 1, n - W).
    It does not depend on the insert.  It equals the indel scan's JUNCTION column bit for bit.
    ALT side (column INS): the starts s of y with max(0, o' - W + 1) <= s <= min(o' + Li - 1, n + Li - W).
    A window that lies wholly inside the insert counts, as the query rule counts it.
  Every window is scored once per strand, or + only under GFM_GRAPH_FORWARD_ONLY (--no-reverse).
  A window that holds a base of x that is not A/C/G/T scores min_val on both strands.
  An insertion repairs nothing, because it removes no base.  A window that does not reach the N is clean.
  Per column, the best window by (score descending, s ascending, + before -), as the key
  ((score + 1) << 8) | ((64 - (s - o')) << 1) | plus, s - o' in -(W - 1) .. -1 for JUNCTION and in -(W - 1) .. Li - 1 for INS.
  Key 0 means the side has no window.
  Per column, the exact uint64 sum of w[score] over the side's windows and strands.
  An insertion before the first base of a sequence is not scanned, as in the indel scan.  An empty sequence has no rows.
  With the inserts ("A", "C", "G", "T") the INS columns equal the indel scan's INS_A .. INS_T bit for bit.
  A cell does not depend on the other inserts of the list or on their order.
By construction a cell equals, field for field, what query_variants.score_edits returns for the insertion (coord[o] + 1, "",
I) applied to x, wherever coordinates can name the gap.

THE FRAMES REPORT A CHANGE ONCE.  In a repeat several gaps spell the same y.  Let r be the primitive root of the folded
insert, the shortest r with I = r^t, and p its length.  The insertion of I behind x[o] spells the same y as an insertion
further left exactly when o >= p in its sequence and folded x[o - p + 1 .. o] == r: it is then the insertion behind x[o - p].
The detail rows drop those cells and keep the leftmost offset; for one-base inserts this is the indel scan's homopolymer
rule.  The dense arrays keep every cell, and the summary, which is about coordinates, keeps every gap a coordinate can name.

A gap is NAMED when x[o] is a non-inserted base and o is the last base of its sequence, or x[o + 1] is the non-inserted base of
coordinate coord[o] + 1: what score_edits answers with GFM_EDIT_APPLIED, and what a VCF row can say.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_insertion_scan.hpp, gfm_sequence_insertion_scan): every window start of a
sequence is scored once for all inserts, and every window of every edited sequence is put together from at most three stored
pieces.  Everything from the kernel's arrays to the frames is numpy group-bys; there is no Python step per row or per base.
"""
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .query_variants import decode_keys
from .sequence_scans import (_UPPER, DEFAULT_MAX_BYTES, ScanTable, _checked_sequences, _within, printed_windows, scan_chunked,
                             scan_inputs, table_writers, tables_by_width)

DETAIL_FILE = "grafimo_insertion_scan"
SUMMARY_FILE = "grafimo_insertion_scan_summary"
ENTRY = "gfm_sequence_insertion_scan"
COLUMNS = ("JUNCTION", "INS")                            # the two columns of the kernel's arrays
JUNCTION, INS = 0, 1
MAX_LENGTH = nv.GFM_INSSCAN_MAX_LENGTH
MAX_INSERTS = nv.GFM_INSSCAN_MAX_INSERTS


def checked_inserts(inserts) -> Tuple[bytes, ...]:
    """the inserts (str or bytes each) folded to upper case; anything but a list of 1 .. 16 distinct inserts of 1 .. 64 letters of
    ACGT is a ValueError"""
    if isinstance(inserts, (str, bytes)) or not hasattr(inserts, "__len__") or len(inserts) == 0:
        raise ValueError(f"inserts {inserts!r}: a non-empty list of sequences over ACGT")
    if len(inserts) > MAX_INSERTS:
        raise ValueError(f"{len(inserts)} inserts: a list holds at most {MAX_INSERTS}")
    out = []
    for ins in inserts:
        if not isinstance(ins, (str, bytes)):
            raise ValueError(f"insert {ins!r}: a str or bytes over ACGT")
        try:
            text = (ins.encode("ascii") if isinstance(ins, str) else bytes(ins)).upper()
        except UnicodeEncodeError:
            raise ValueError(f"insert {ins!r}: every letter is one of ACGT") from None
        if not 1 <= len(text) <= MAX_LENGTH:
            raise ValueError(f"insert {ins!r}: the length {len(text)} lies outside 1 .. {MAX_LENGTH}")
        if text.strip(b"ACGT"):
            raise ValueError(f"insert {ins!r}: every letter is one of ACGT")
        if text in out:
            raise ValueError(f"insert {ins!r} repeats")
        out.append(text)
    return tuple(out)


def _packed(inserts: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """-> (insert_offsets int32 [K + 1], insert_bases uint8) as the entry reads them"""
    off = np.concatenate([[0], np.cumsum([len(i) for i in inserts])]).astype(np.int32)
    return np.ascontiguousarray(off), np.frombuffer(b"".join(inserts), dtype=np.uint8).copy()


def primitive_period(insert: bytes) -> int:
    """the length of the shortest r with insert == r^t"""
    return (insert + insert).find(insert, 1)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _scan_chunked(motifs: Sequence, seq_offsets, bases, inserts: Sequence[bytes], weights, temperature, forward_only, max_bytes):
    """-> (per motif (keys, sums) [K, N, 2], per motif its log2 offset, per motif (scale, offset, ptable)): the motifs leased and
    scanned in chunks whose result tensors (24 bytes a base, insert and motif) stay under max_bytes"""
    K = len(inserts)
    off, text = _packed(inserts)                                  # (alive until the last chunk's call has returned)
    return scan_chunked(motifs, seq_offsets, bases, weights, temperature, forward_only, max_bytes, ENTRY, (K, len(bases), len(COLUMNS)),
                        (K, off.ctypes.data, text.ctypes.data), f" and {K} inserts", " or inserts")


def scan_sequences(motifs: Sequence, seq_offsets, bases, inserts, weights: Optional[Sequence[np.ndarray]] = None,
                   temperature: float = 1.0, forward_only: bool = False,
                   max_bytes: int = DEFAULT_MAX_BYTES) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The kernel on plain arrays: sequences (`seq_offsets` int64 [V + 1] from 0, `bases` uint8) for motifs of ONE width and a
    list of `inserts` (checked_inserts) -> per motif (keys uint32 [K, n_bases, 2], sums uint64 [K, n_bases, 2]), the columns
    JUNCTION, INS (decode_keys reads a key; its start is relative to the first inserted base).  `weights`: a uint64 table per
    motif, default haplotype_affinity.default_weights at `temperature`.  The motifs are taken in chunks whose result tensors (24
    bytes a base, insert and motif) stay under `max_bytes`; a single motif above it is a ValueError that names it, and so are
    bad inserts, before the library is called.  The library refuses motifs of two widths and weights that can overflow a sum."""
    inserts = checked_inserts(inserts)
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    return _scan_chunked(motifs, seq_offsets, bases, inserts, weights, temperature, forward_only, max_bytes)[0]


def leftmost_insertions(seq_offsets, bases, inserts) -> np.ndarray:
    """bool [K, N]: False where the same edited sequence is made at a smaller offset of the sequence: o >= p and folded
    x[o - p + 1 .. o] == r, with r the insert's primitive root and p its length (see the module's docstring)"""
    seq_offsets, bases = np.asarray(seq_offsets, dtype=np.int64), np.asarray(bases, dtype=np.uint8)
    inserts = checked_inserts(inserts)
    N = len(bases)
    keep = np.ones((len(inserts), N), dtype=bool)
    if N == 0:
        return keep
    up = _UPPER[bases]
    within = _within(seq_offsets, N)[0]
    at = np.arange(N, dtype=np.int64)
    for k, ins in enumerate(inserts):
        p = primitive_period(ins)
        repeat = within >= p                                      # (so x[o - p + 1 .. o] lies in o's sequence)
        for j in range(p):
            repeat &= up[np.maximum(at - p + 1 + j, 0)] == ins[j]
        keep[k] = ~repeat
    return keep


class InsertionScan(ScanTable):
    """The table of one motif over S sequences of N bases in all and K inserts (see the module's docstring).
    Per sequence [S]: seq_region, seq_version (-1: the region's reference sequence, which no haplotype spells), seq_count,
    seq_group_counts [S, G], seq_is_reference, seq_offsets int64 [S + 1] -- as IndelScan's.
    Per base [N]: bases uint8, coord int32 (~coordinate for an inserted base).  inserts: K byte strings, upper case.  The
    dense arrays keys uint32 [K, N, 2] and sums uint64 [K, N, 2] with the columns JUNCTION, INS: the insertion of inserts[k]
    behind base n compares column 1 with column 0."""

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                 seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, inserts, keys,
                 sums, delta=None, all_rows=False):
        self.inserts = checked_inserts(inserts)
        super().__init__(motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                         seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, keys, sums,
                         delta, all_rows)

    def _shape(self):
        return (len(self.inserts), len(self.bases), 2), "the sequences and inserts"

    @property
    def lengths(self) -> np.ndarray:
        """int64 [K]: the inserts' lengths"""
        return np.array([len(i) for i in self.inserts], dtype=np.int64)

    def named_gaps(self) -> np.ndarray:
        """bool [N]: the gap behind the base is one a VCF row could name -- the base is non-inserted, and it is the last of its
        sequence or the next base is the non-inserted base of the next coordinate"""
        N = len(self.bases)
        if N == 0:
            return np.zeros(0, dtype=bool)
        co = self.coord.astype(np.int64)
        follows = np.zeros(N, dtype=bool)
        follows[:-1] = co[1:] == co[:-1] + 1                      # (co[o] >= 0 makes co[o] + 1 a non-inserted base's)
        return (co >= 0) & ((_within(self.seq_offsets, N)[1] == 1) | follows)

    def _cells(self, every: bool = False):
        """the (base, insert) cells of the detail rows -> (base index n, insert index k), in (n, k) order: those the repeat rule
        keeps; `every`: all"""
        keep = np.ones((len(self.inserts), len(self.bases)), dtype=bool) if every else \
            leftmost_insertions(self.seq_offsets, self.bases, self.inserts)
        n, k = np.nonzero(keep.T)
        return n.astype(np.int64), k.astype(np.int64)

    @staticmethod
    def _sides(n, k):
        return (k, n, 0), (k, n, 1)

    def _insert_text(self) -> np.ndarray:
        """uint8 [K, 64]: the inserts, padded with zeros"""
        text = np.zeros((len(self.inserts), MAX_LENGTH), dtype=np.uint8)
        for k, ins in enumerate(self.inserts):
            text[k, :len(ins)] = np.frombuffer(ins, dtype=np.uint8)
        return text

    def _kmers(self, n, k, side: str) -> np.ndarray:
        """object: the best window of the side as printed ('-': reverse complemented), '' where there is none.  The REF side's
        is read from x, the ALT side's from the edited sequence y."""
        W = self.width
        if not len(n):
            return np.zeros(0, dtype=object)
        key = self.keys[k, n, JUNCTION if side == "ref" else INS]
        _, rel, strand = decode_keys(key)
        some = key > 0
        gap = (n + 1)[:, None]                                    # the first inserted base's place in y
        at = np.where(some, n + 1 + rel, 0)[:, None] + np.arange(W, dtype=np.int64)[None, :]
        if side == "alt":                                         # y's base i is x's i before the gap, x's i - Li behind the insert
            li = self.lengths[k][:, None]
            inside = (at >= gap) & (at < gap + li) & some[:, None]
            src = np.where(at >= gap + li, at - li, at)
        else:
            src = at
        text = _UPPER[self.bases[np.clip(src, 0, max(len(self.bases) - 1, 0))]]
        if side == "alt":
            rows = np.nonzero(inside)[0]
            text[inside] = self._insert_text()[k[rows], (at - gap)[inside]]
        out = printed_windows(text, strand == "-")
        out[~some] = ""
        return out

    def _gap_columns(self, n, k) -> dict:
        """the leading columns of the cells (n, k), then insert, length and named"""
        data = self._leading_columns(n)
        data["insert"] = np.array([i.decode() for i in self.inserts], dtype=object)[k] if len(k) else np.zeros(0, dtype=object)
        data["length"] = self.lengths[k]
        data["named"] = self.named_gaps()[n]
        return data

    def to_frame(self) -> pd.DataFrame:
        """a row per (region, version, offset, insert) the filter keeps (mutation_scan.keep_rows) and the repeat rule does not
        drop: motif_id, motif_alt_id, sequence_name, version (-1: the reference sequence, no haplotype spells it), haplotypes,
        one haplotypes_<GROUP> per group, is_reference, position (the 1-based coordinate of the base the insert goes behind; an
        inserted base has its anchor's), inserted (of that base), insert (upper case), length, named (a VCF row could name the
        gap), ref_score, ref_pvalue, ref_start (the best window's start minus the first inserted base's place), ref_strand,
        ref_kmer (read from x), alt_score .. alt_kmer (read from the edited sequence), ref_log2_affinity, alt_log2_affinity,
        delta_log2_affinity, effect -- NaN or empty where a side has no window.  Rows in (sequence, offset, insert) order, the
        sequences by region, then version, the reference sequence last, the inserts in the list's order."""
        n, k = self._kept_cells()
        return self._detail_frame(n, k, self._gap_columns(n, k))

    def summary_frame(self) -> pd.DataFrame:
        """a row per (region, coordinate of the base the insert goes behind, insert) over the versions (not the count-0
        reference sequence) whose gap there is `named`, the gaps a repeat drops from the detail rows included (the summary is
        about coordinates): motif_id, motif_alt_id, sequence_name, position, insert, length, versions, haplotypes,
        haplotypes_gain, haplotypes_loss, min_delta_log2_affinity, max_delta_log2_affinity, best_alt_score.  A row is kept when
        some haplotype gains or loses, or when a delta is given and the smallest or largest delta reaches it; all_rows keeps
        everything.  Rows in (region, position, the list's order of the inserts) order."""
        n, k = self._cells(every=True)
        seq = self._sequence_of(n)
        on = (self.named_gaps()[n] & (self.seq_version[seq] >= 0)) if len(n) else np.zeros(0, dtype=bool)
        n, k, seq = n[on], k[on], seq[on]
        names = np.array([i.decode() for i in self.inserts], dtype=object)
        return self._summary_frame(n, k, seq, (k,), lambda f: {"insert": names[k[f]] if len(f) else np.zeros(0, dtype=object),
                                                               "length": self.lengths[k[f]]})


def compute_insertion_scan_many(motifs: Sequence, graph, regions, debug: bool, args_obj, inserts, chrom_names=None,
                                haplotype_groups: Optional[Mapping] = None, weights: Optional[Sequence[np.ndarray]] = None,
                                temperature: float = 1.0, threshold: Optional[float] = None, delta: Optional[float] = None,
                                all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> List[InsertionScan]:
    """One InsertionScan per motif, in the order of `motifs` (see the module's docstring).  `inserts`: 1 .. 16 distinct
    sequences of 1 .. 64 letters of ACGT (checked_inserts).  The other arguments and the sequences are
    compute_deletion_scan_many's: the versions of compute_haplotype_sequences(coordinates=True), the reference sequence of a
    region added where no version is the reference's; one kernel call per motif width (in chunks of motifs under
    `max_bytes`).  args_obj: noreverse and threshold (`threshold` overrides it).  The frames keep a row when its effect is gain
    or loss, or when |delta_log2_affinity| >= `delta` if a delta is given; `all_rows` keeps everything."""
    inserts = checked_inserts(inserts)
    seqs, region_names, group_names, forward_only, threshold = scan_inputs(
        "the insertion scan", motifs, graph, regions, debug, args_obj, chrom_names, haplotype_groups, weights, delta, threshold)
    return tables_by_width(
        motifs, weights,
        lambda ms, ws: _scan_chunked(ms, seqs[5], seqs[6], inserts, ws, temperature, forward_only, max_bytes),
        lambda motif, W, numbers, log2_offset, got: InsertionScan(motif.motif_id, motif.motif_name, W, *numbers, log2_offset, threshold,
                                                                  region_names, group_names, *seqs, inserts, *got, delta, all_rows))


def compute_insertion_scan(motif, graph, regions, debug: bool, args_obj, inserts, chrom_names=None,
                           haplotype_groups: Optional[Mapping] = None, weights: Optional[np.ndarray] = None, temperature: float = 1.0,
                           threshold: Optional[float] = None, delta: Optional[float] = None, all_rows: bool = False,
                           max_bytes: int = DEFAULT_MAX_BYTES) -> InsertionScan:
    """The insertion scan of `motif` (compute_insertion_scan_many for one motif)"""
    return compute_insertion_scan_many([motif], graph, regions, debug, args_obj, inserts, chrom_names, haplotype_groups,
                                       None if weights is None else [weights], temperature, threshold, delta, all_rows, max_bytes)[0]


# grafimo_insertion_scan[_<motif_id>].tsv, grafimo_insertion_scan_summary[_<motif_id>].tsv (a row per (region, coordinate,
# insert)), and -f: both on stdout
write_insertion_scan, write_insertion_scan_summary, print_insertion_scan = table_writers(DETAIL_FILE, SUMMARY_FILE)
