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
import contextlib
import ctypes
import sys
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _stream_ptr, _torch
from .graph_tables import (_haplotype_set, _matrix_rows, group_by_width, prepare_graphs, require_single_gpu, scaled_pvalues,
                           scaled_scores, table_path, write_frame)
from .mutation_scan import (_COMP, _UPPER, DEFAULT_MAX_BYTES, _checked_sequences, _leased_chunks, _with_references, effect_codes,
                            group_summary, keep_rows)
from .query_variants import EFFECTS, decode_keys

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
def _scan(dms, tables, seq_offsets: np.ndarray, bases: np.ndarray, lengths: np.ndarray, forward_only: bool):
    """gfm_sequence_deletion_scan for leased motifs of one width -> (keys uint32 [M, n_lengths, N, 2], sums uint64 of that
    shape).  The staging is this module's own: the entry takes the lengths and writes another shape than mutation_scan's."""
    M, N, K = len(dms), int(seq_offsets[-1]), len(lengths)
    if N == 0:
        return np.zeros((M, K, 0, 2), dtype=np.uint32), np.zeros((M, K, 0, 2), dtype=np.uint64)
    torch = _torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    d_bases = torch.from_numpy(np.array(bases, dtype=np.uint8)).to(dev)              # (a copy: the caller's may be read-only)
    d_tabs = [torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64)).to(dev) for t in tables]
    keys = torch.empty((M, K, N, 2), dtype=torch.int32, device=dev)
    sums = torch.empty((M, K, N, 2), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    nv.check(getattr(nv.lib(), ENTRY)(
        (vp * M)(*[x.handle for x in dms]), M, (vp * M)(*[t.data_ptr() for t in d_tabs]), max(int(t.max()) for t in tables),
        len(seq_offsets) - 1, seq_offsets.ctypes.data, d_bases.data_ptr(), K, lengths.ctypes.data,
        nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0, (vp * M)(*[keys[m].data_ptr() for m in range(M)]),
        (vp * M)(*[sums[m].data_ptr() for m in range(M)]), status.data_ptr(), _stream_ptr(None)))
    return keys.cpu().numpy().view(np.uint32), sums.cpu().numpy().view(np.uint64)


def _scan_chunked(motifs: Sequence, seq_offsets, bases, lengths, weights, temperature, forward_only, max_bytes):
    """-> (per motif (keys, sums), per motif its log2 offset, per motif (scale, offset, ptable)): the motifs leased and scanned
    in chunks whose result tensors (24 bytes a base, length and motif) stay under max_bytes"""
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    per_motif = BYTES_PER_CELL * len(lengths) * int(seq_offsets[-1])
    if per_motif > int(max_bytes):
        raise ValueError(f"{motifs[0].motif_id}: the keys and sums of one motif over {int(seq_offsets[-1])} bases and "
                         f"{len(lengths)} lengths hold {per_motif} bytes, more than max_bytes = {int(max_bytes)}: scan fewer "
                         f"sequences or lengths at a time, or raise max_bytes")
    step = max(1, int(max_bytes) // max(per_motif, 1))
    results, offsets, numbers = [], [], []
    with contextlib.closing(_leased_chunks(motifs, weights, temperature, step)) as chunks:     # (a failure gives the handles back)
        for _, dms, tables, offs, nums in chunks:
            keys, sums = _scan(dms, tables, seq_offsets, bases, lengths, forward_only)
            results += [(keys[m], sums[m]) for m in range(len(dms))]
            offsets += offs
            numbers += nums
    return results, offsets, numbers


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


def _within(seq_offsets: np.ndarray, N: int):
    """-> (the offset of every base in its sequence, the bases behind and including it) int64 [N]"""
    n = np.diff(seq_offsets)
    within = np.arange(N, dtype=np.int64) - np.repeat(seq_offsets[:-1], n)
    return within, np.repeat(n, n) - within


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


class DeletionScan:
    """The table of one motif over S sequences of N bases in all and K lengths (see the module's docstring).
    Per sequence [S]: seq_region, seq_version (-1: the region's reference sequence, which no haplotype spells), seq_count,
    seq_group_counts [S, G], seq_is_reference, seq_offsets int64 [S + 1] -- as IndelScan's.
    Per base [N]: bases uint8, coord int32 (~coordinate for an inserted base).  lengths int32 [K], strictly ascending.  The
    dense arrays keys uint32 [K, N, 2] and sums uint64 [K, N, 2] with the columns COVER, DEL: the deletion of lengths[k] bases
    from base n on compares column 1 with column 0; a block that does not fit its sequence has four zeros."""

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                 seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, lengths, keys,
                 sums, delta=None, all_rows=False):
        self.motif_id, self.motif_alt_id = motif_id, motif_alt_id
        self.width, self.scale, self.offset = int(width), int(scale), float(offset)
        self.ptable, self.log2_offset, self.threshold = np.asarray(ptable, dtype=np.float64), float(log2_offset), float(threshold)
        self.region_names, self.group_names = np.asarray(region_names, dtype=object), list(group_names)
        self.seq_region, self.seq_version = np.asarray(seq_region, dtype=np.int64), np.asarray(seq_version, dtype=np.int64)
        self.seq_count = np.asarray(seq_count, dtype=np.int64)
        self.seq_group_counts = np.asarray(seq_group_counts, dtype=np.int64).reshape(len(self.seq_count), len(self.group_names))
        self.seq_is_reference = np.asarray(seq_is_reference, dtype=bool)
        self.seq_offsets = np.asarray(seq_offsets, dtype=np.int64)
        self.bases, self.coord = np.asarray(bases, dtype=np.uint8), np.asarray(coord, dtype=np.int32)
        self.lengths = checked_lengths(lengths)
        self.keys, self.sums = np.asarray(keys, dtype=np.uint32), np.asarray(sums, dtype=np.uint64)
        N, K = len(self.bases), len(self.lengths)
        if self.keys.shape != (K, N, 2) or self.sums.shape != (K, N, 2) or len(self.coord) != N or int(self.seq_offsets[-1]) != N:
            raise ValueError("the arrays do not fit the sequences and lengths")
        self.delta = None if delta is None else float(delta)
        self.all_rows = bool(all_rows)

    def __len__(self) -> int:
        return int(self._kept_cells()[0].size)

    @property
    def base_sequence(self) -> np.ndarray:
        """int64 [N]: the sequence of every base"""
        return np.repeat(np.arange(len(self.seq_count), dtype=np.int64), np.diff(self.seq_offsets))

    def log2_affinity(self) -> np.ndarray:
        """float64 [K, N, 2]: log2(sum) + log2_offset, NaN where the side has no window"""
        out = np.full(self.sums.shape, np.nan)
        some = self.sums > 0
        out[some] = np.log2(self.sums[some].astype(np.float64)) + self.log2_offset
        return out

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

    def _numbers(self, n, k):
        """of the cells (n, k) -> (ref best, alt best (int64, -1: none), ref p, alt p, ref log2, alt log2)"""
        rb, ab = decode_keys(self.keys[k, n, COVER])[0], decode_keys(self.keys[k, n, DEL])[0]
        la = lambda s: np.where(s > 0, np.log2(np.where(s > 0, s, 1).astype(np.float64)) + self.log2_offset, np.nan)   # noqa: E731
        return (rb, ab, scaled_pvalues(rb, self.ptable), scaled_pvalues(ab, self.ptable), la(self.sums[k, n, COVER]),
                la(self.sums[k, n, DEL]))

    def _kept_cells(self):
        n, k = self._cells()
        rb, ab, rp, ap, rl, al = self._numbers(n, k)
        keep = keep_rows(effect_codes(rp, ap, self.threshold), al - rl, self.delta, self.all_rows)
        return n[keep], k[keep]

    def _deleted(self, n, k) -> np.ndarray:
        """object: the deleted bases, upper case"""
        if not len(n):
            return np.zeros(0, dtype=object)
        L = self.lengths.astype(np.int64)[k]
        width = int(L.max())
        j = np.arange(width, dtype=np.int64)[None, :]
        text = _UPPER[self.bases[np.minimum(n[:, None] + j, len(self.bases) - 1)]]
        text[j >= L[:, None]] = 0                                 # (a fixed-width byte string drops its trailing zeros)
        return np.ascontiguousarray(text).view(f"S{width}").reshape(-1).astype(f"U{width}").astype(object)

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
        minus = strand == "-"
        text[minus] = _COMP[text[minus]][:, ::-1]
        out = np.ascontiguousarray(text).view(f"S{W}").reshape(-1).astype(f"U{W}").astype(object)
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
        rows = len(n)
        seq = self.base_sequence[n] if rows else np.zeros(0, dtype=np.int64)
        data = {"motif_id": np.full(rows, self.motif_id, dtype=object), "motif_alt_id": np.full(rows, self.motif_alt_id, dtype=object),
                "sequence_name": self.region_names[self.seq_region[seq]] if rows else np.zeros(0, dtype=object),
                "version": self.seq_version[seq], "haplotypes": self.seq_count[seq]}
        for g, name in enumerate(self.group_names):
            data[f"haplotypes_{name}"] = self.seq_group_counts[seq, g]
        data["is_reference"] = self.seq_is_reference[seq]
        co = self.coord[n].astype(np.int64)
        data["position"] = np.where(co < 0, ~co, co) + 1
        data["inserted"] = co < 0
        data["length"] = self.lengths.astype(np.int64)[k]
        data["named"] = self.named_blocks()[k, n]
        data["deleted"] = self._deleted(n, k)
        rb, ab, rp, ap, rl, al = self._numbers(n, k)
        for side, best, p, col in (("ref", rb, rp, COVER), ("alt", ab, ap, DEL)):
            _, rel, strand = decode_keys(self.keys[k, n, col])
            data[f"{side}_score"] = scaled_scores(best, self.scale, self.offset, self.width)
            data[f"{side}_pvalue"] = p
            data[f"{side}_start"] = np.where(best >= 0, rel.astype(np.float64), np.nan)
            data[f"{side}_strand"] = strand
            data[f"{side}_kmer"] = self._kmers(n, k, side)
        data["ref_log2_affinity"], data["alt_log2_affinity"], data["delta_log2_affinity"] = rl, al, al - rl
        data["effect"] = EFFECTS[effect_codes(rp, ap, self.threshold)]
        return pd.DataFrame(data)

    def summary_frame(self) -> pd.DataFrame:
        """a row per (region, coordinate of the first deleted base, length) over the versions (not the count-0 reference
        sequence) whose block there is `named`, the blocks a repeat drops from the detail rows included (the summary is about
        coordinates): motif_id, motif_alt_id, sequence_name, position, length, versions, haplotypes, haplotypes_gain,
        haplotypes_loss, min_delta_log2_affinity, max_delta_log2_affinity, best_alt_score.  A row is kept when some haplotype
        gains or loses, or when a delta is given and the smallest or largest delta reaches it; all_rows keeps everything.  Rows
        in (region, position, length) order."""
        n, k = self._cells(every=True)
        seq = self.base_sequence[n] if len(n) else np.zeros(0, dtype=np.int64)
        on = (self.named_blocks()[k, n] & (self.seq_version[seq] >= 0)) if len(n) else np.zeros(0, dtype=bool)
        n, k, seq = n[on], k[on], seq[on]
        rb, ab, rp, ap, rl, al = self._numbers(n, k)
        codes = effect_codes(rp, ap, self.threshold)
        region, length = self.seq_region[seq], self.lengths.astype(np.int64)[k]
        first, versions, haps, gain, loss, lo, hi, best = group_summary((region, self.coord[n].astype(np.int64), length),
                                                                        self.seq_count[seq], codes, al - rl, ab)
        keep = np.ones(len(first), dtype=bool) if self.all_rows else (gain + loss) > 0
        if self.delta is not None and not self.all_rows:
            with np.errstate(invalid="ignore"):
                keep |= (np.abs(lo) >= self.delta) | (np.abs(hi) >= self.delta)
        j = np.flatnonzero(keep)
        f = first[j]
        rows = len(j)
        return pd.DataFrame({
            "motif_id": np.full(rows, self.motif_id, dtype=object), "motif_alt_id": np.full(rows, self.motif_alt_id, dtype=object),
            "sequence_name": self.region_names[region[f]] if rows else np.zeros(0, dtype=object),
            "position": self.coord[n[f]].astype(np.int64) + 1, "length": length[f], "versions": versions[j], "haplotypes": haps[j],
            "haplotypes_gain": gain[j], "haplotypes_loss": loss[j], "min_delta_log2_affinity": lo[j],
            "max_delta_log2_affinity": hi[j], "best_alt_score": scaled_scores(best[j], self.scale, self.offset, self.width)})


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
    from .haplotype_classes import compute_haplotype_classes
    from .haplotype_sequences import compute_haplotype_sequences
    require_single_gpu("the deletion scan", "is", "a gather of the sharded class matrices")
    lengths = checked_lengths(lengths)
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    if delta is not None and not float(delta) >= 0:
        raise ValueError(f"delta {delta}: it must be >= 0")
    prep = prepare_graphs(graph, regions, chrom_names)
    _haplotype_set(prep, None, "the deletion scan")
    rows, region_names = _matrix_rows(prep)
    hc = compute_haplotype_classes(graph, regions, debug, args_obj, chrom_names, None, haplotype_groups)
    hs = compute_haplotype_sequences(graph, regions, debug, args_obj, chrom_names, None, None, classes=hc, coordinates=True)
    seqs = _with_references(hs, prep, rows)
    seq_offsets, bases, coord = np.ascontiguousarray(seqs[5]), np.ascontiguousarray(seqs[6]), seqs[7]
    forward_only = bool(getattr(args_obj, "noreverse", False))
    threshold = float(args_obj.threshold if threshold is None else threshold)
    out: List[Optional[DeletionScan]] = [None] * len(motifs)
    for W, idxs in group_by_width(motifs).items():
        got, offsets, numbers = _scan_chunked([motifs[i] for i in idxs], seq_offsets, bases, lengths,
                                              None if weights is None else [weights[i] for i in idxs], temperature, forward_only,
                                              max_bytes)
        for m, i in enumerate(idxs):
            scale, offset, ptable = numbers[m]
            out[i] = DeletionScan(motifs[i].motif_id, motifs[i].motif_name, W, scale, offset, ptable, offsets[m], threshold,
                                  region_names, hs.group_names, *seqs[:5], seq_offsets, bases, coord, lengths, got[m][0], got[m][1],
                                  delta, all_rows)
    return out


def compute_deletion_scan(motif, graph, regions, debug: bool, args_obj, lengths, chrom_names=None,
                          haplotype_groups: Optional[Mapping] = None, weights: Optional[np.ndarray] = None, temperature: float = 1.0,
                          threshold: Optional[float] = None, delta: Optional[float] = None, all_rows: bool = False,
                          max_bytes: int = DEFAULT_MAX_BYTES) -> DeletionScan:
    """The deletion scan of `motif` (compute_deletion_scan_many for one motif)"""
    return compute_deletion_scan_many([motif], graph, regions, debug, args_obj, lengths, chrom_names, haplotype_groups,
                                      None if weights is None else [weights], temperature, threshold, delta, all_rows, max_bytes)[0]


def write_deletion_scan(table: DeletionScan, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_deletion_scan.tsv (grafimo_deletion_scan_<motif_id>.tsv for one of several motifs), the detail rows, in the
    directory write_results uses for this motif -> the path written.  `out`: a text stream to write to instead (-f: stdout)."""
    return write_frame(table.to_frame(), out if out is not None else table_path(DETAIL_FILE, args_obj, motif, motif_num))


def write_deletion_scan_summary(table: DeletionScan, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_deletion_scan_summary[_<motif_id>].tsv, a row per (region, coordinate, length), beside the detail rows"""
    return write_frame(table.summary_frame(), out if out is not None else table_path(SUMMARY_FILE, args_obj, motif, motif_num))


def print_deletion_scan(table: DeletionScan) -> None:
    """-f: the detail rows, then the summary, on stdout instead of files"""
    write_deletion_scan(table, None, 1, None, out=sys.stdout)
    write_deletion_scan_summary(table, None, 1, None, out=sys.stdout)
