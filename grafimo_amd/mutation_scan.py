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
from .query_variants import EFFECTS, _weight_tables, decode_keys

DETAIL_FILE = "grafimo_mutation_scan"
SUMMARY_FILE = "grafimo_mutation_scan_summary"
COLUMNS = ("REF", "A", "C", "G", "T")                    # the five columns of the kernel's arrays
TO_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
BYTES_PER_BASE = 5 * (4 + 8)                             # a motif's keys and sums per base
DEFAULT_MAX_BYTES = 1 << 31
_UPPER = np.arange(256, dtype=np.uint8)
_UPPER[ord("a"):ord("z") + 1] -= 32
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMP[_a] = _b
_COLUMN_OF = np.zeros(256, dtype=np.int64)               # the column of a base, 0: it is none of A, C, G, T
for _k, _c in enumerate(b"ACGT"):
    _COLUMN_OF[_c] = _COLUMN_OF[_c + 32] = _k + 1


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _stage(tables, seq_offsets: np.ndarray, bases: np.ndarray, columns: int = 5):
    """the inputs of gfm_sequence_mutation_scan on the current device and its result tensors -> (seq_offsets (host), the bases'
    tensor, the weight tables' tensors, the largest weight, keys int32 [M, N, 5], sums int64 [M, N, 5], the status word).
    `columns`: of an entry with the same arguments and another number of columns (indel_scan's 7)"""
    torch = _torch()
    M, N = len(tables), int(seq_offsets[-1])
    dev = torch.device("cuda", torch.cuda.current_device())
    d_bases = torch.from_numpy(np.array(bases, dtype=np.uint8)).to(dev)             # (a copy: the caller's may be read-only)
    d_tabs = [torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64)).to(dev) for t in tables]
    return (seq_offsets, d_bases, d_tabs, max(int(t.max()) for t in tables), torch.empty((M, N, columns), dtype=torch.int32, device=dev),
            torch.empty((M, N, columns), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))


def _enqueue(dms, staged, forward_only: bool, entry: str = "gfm_sequence_mutation_scan"):
    """gfm_sequence_mutation_scan (or `entry`, which takes the same arguments) over staged inputs (_stage): every row of the
    result tensors is written -> (keys, sums)"""
    seq_offsets, d_bases, d_tabs, max_weight, keys, sums, status = staged
    M = len(dms)
    vp = ctypes.c_void_p
    nv.check(getattr(nv.lib(), entry)(
        (vp * M)(*[x.handle for x in dms]), M, (vp * M)(*[t.data_ptr() for t in d_tabs]), max_weight, len(seq_offsets) - 1,
        seq_offsets.ctypes.data, d_bases.data_ptr(), nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0,
        (vp * M)(*[keys[m].data_ptr() for m in range(M)]), (vp * M)(*[sums[m].data_ptr() for m in range(M)]),
        status.data_ptr(), _stream_ptr(None)))
    return keys, sums


def _scan(dms, tables, seq_offsets: np.ndarray, bases: np.ndarray, forward_only: bool, entry: str = "gfm_sequence_mutation_scan",
          columns: int = 5):
    """gfm_sequence_mutation_scan for leased motifs of one width -> (keys uint32 [M, N, 5], sums uint64 [M, N, 5])"""
    M = len(dms)
    if int(seq_offsets[-1]) == 0:
        return np.zeros((M, 0, columns), dtype=np.uint32), np.zeros((M, 0, columns), dtype=np.uint64)
    keys, sums = _enqueue(dms, _stage(tables, seq_offsets, bases, columns), forward_only, entry)
    return keys.cpu().numpy().view(np.uint32), sums.cpu().numpy().view(np.uint64)


def _checked_sequences(seq_offsets, bases) -> Tuple[np.ndarray, np.ndarray]:
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    if seq_offsets.ndim != 1 or len(seq_offsets) < 1 or seq_offsets[0] != 0:
        raise ValueError("seq_offsets is int64 [n_seqs + 1] and starts at 0")
    if int(seq_offsets[-1]) != len(bases):
        raise ValueError(f"seq_offsets ends at {int(seq_offsets[-1])}, bases holds {len(bases)}")
    return seq_offsets, bases


def _leased_chunks(motifs: Sequence, weights, temperature, step: int):
    """The motifs `step` at a time, leased for as long as the caller holds the item -> (m0, the leased handles, their weight
    tables, their log2 offsets, per motif (scale, offset, ptable)) per chunk; the handles are given back when the caller asks
    for the next chunk, or fails.  What the sequence tables' chunked calls share (_scan_chunked, shuffle_null)."""
    from .device import DeviceMotif
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    for m0 in range(0, len(motifs), step):
        chunk = list(motifs[m0:m0 + step])
        dms = [DeviceMotif.lease(m) for m in chunk]
        try:
            tables, offs = _weight_tables(dms, chunk, None if weights is None else list(weights[m0:m0 + step]), temperature)
            yield m0, dms, tables, offs, [(dm.scale, dm.offset, dm.ptable_host()) for dm in dms]
        finally:
            for dm in dms:
                dm.release()


def _scan_chunked(motifs: Sequence, seq_offsets, bases, weights, temperature, forward_only, max_bytes,
                  entry: str = "gfm_sequence_mutation_scan", columns: int = 5):
    """-> (per motif (keys, sums), per motif its log2 offset, per motif (scale, offset, ptable)): the motifs leased and scanned
    in chunks whose result tensors stay under max_bytes"""
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    per_motif = columns * (4 + 8) * int(seq_offsets[-1])
    if per_motif > int(max_bytes):
        raise ValueError(f"{motifs[0].motif_id}: the keys and sums of one motif over {int(seq_offsets[-1])} bases hold {per_motif} "
                         f"bytes, more than max_bytes = {int(max_bytes)}: scan fewer sequences at a time, or raise max_bytes")
    step = max(1, int(max_bytes) // max(per_motif, 1))
    results, offsets, numbers = [], [], []
    with contextlib.closing(_leased_chunks(motifs, weights, temperature, step)) as chunks:     # (a failure gives the handles back)
        for _, dms, tables, offs, nums in chunks:
            keys, sums = _scan(dms, tables, seq_offsets, bases, forward_only, entry, columns)
            results += [(keys[m], sums[m]) for m in range(len(dms))]
            offsets += offs
            numbers += nums
    return results, offsets, numbers


def scan_sequences(motifs: Sequence, seq_offsets, bases, weights: Optional[Sequence[np.ndarray]] = None, temperature: float = 1.0,
                   forward_only: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The kernel on plain arrays: sequences (`seq_offsets` int64 [V + 1] from 0, `bases` uint8) for motifs of ONE width -> per
    motif (keys uint32 [n_bases, 5], sums uint64 [n_bases, 5]), the columns REF, A, C, G, T (decode_keys reads a key).  `weights`:
    a uint64 table per motif, default haplotype_affinity.default_weights at `temperature`.  The motifs are taken in chunks whose
    result tensors stay under `max_bytes`; a single motif above it is a ValueError that names it.  The library refuses motifs
    of two widths and weights that can overflow a sum."""
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    return _scan_chunked(motifs, seq_offsets, bases, weights, temperature, forward_only, max_bytes)[0]


# ---------------------------------------------------------------------------------------------------------------- the table
def effect_codes(ref_p: np.ndarray, alt_p: np.ndarray, threshold: float) -> np.ndarray:
    """int64: (the REF side's best window has p < threshold) * 2 + (the ALT side's has), the index into query_variants.EFFECTS;
    a side without a window (NaN) has not"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(ref_p) < threshold).astype(np.int64) * 2 + (np.asarray(alt_p) < threshold).astype(np.int64)


def keep_rows(codes: np.ndarray, delta_log2: np.ndarray, delta: Optional[float], all_rows: bool) -> np.ndarray:
    """bool: the rows the frames hold -- all_rows; else the effect is gain or loss, or |delta_log2| >= delta when a delta is given"""
    codes = np.asarray(codes)
    if all_rows:
        return np.ones(len(codes), dtype=bool)
    keep = (codes == 1) | (codes == 2)
    if delta is not None:
        with np.errstate(invalid="ignore"):
            keep |= np.abs(np.asarray(delta_log2)) >= float(delta)
    return keep


def group_summary(group_keys: Sequence[np.ndarray], haplotypes, codes, delta_log2, alt_best):
    """The summary's group-by: rows that agree in every array of `group_keys` are one group -> (first: a row of every group, the
    groups ascending by the keys, the first key the most significant; versions; haplotypes; haplotypes_gain; haplotypes_loss; the
    smallest and largest delta_log2 (NaN: none); the largest alt_best)"""
    n = len(haplotypes)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, z, np.zeros(0), np.zeros(0), z
    order = np.lexsort(tuple(np.asarray(k) for k in reversed(list(group_keys))))
    head = np.ones(n, dtype=bool)
    head[1:] = False
    for k in group_keys:
        k = np.asarray(k)[order]
        head[1:] |= k[1:] != k[:-1]
    at = np.flatnonzero(head)
    haplotypes, codes = np.asarray(haplotypes, dtype=np.int64)[order], np.asarray(codes)[order]
    d, best = np.asarray(delta_log2, dtype=np.float64)[order], np.asarray(alt_best, dtype=np.int64)[order]
    add = lambda v: np.add.reduceat(v, at)                # noqa: E731
    lo = np.minimum.reduceat(np.where(np.isnan(d), np.inf, d), at)
    hi = np.maximum.reduceat(np.where(np.isnan(d), -np.inf, d), at)
    return (order[at], add(np.ones(n, dtype=np.int64)), add(haplotypes), add(np.where(codes == 1, haplotypes, 0)),
            add(np.where(codes == 2, haplotypes, 0)), np.where(np.isfinite(lo), lo, np.nan), np.where(np.isfinite(hi), hi, np.nan),
            np.maximum.reduceat(best, at))


class MutationScan:
    """The table of one motif over S sequences of N bases in all (see the module's docstring).
    Per sequence [S]: seq_region (the caller's region row), seq_version (the version's number in its region, -1: the region's
    reference sequence, which no haplotype spells), seq_count (haplotypes), seq_group_counts [S, G], seq_is_reference,
    seq_offsets int64 [S + 1].
    Per base [N]: bases uint8, coord int32 (~coordinate for an inserted base), and the dense arrays keys uint32 [N, 5] and sums
    uint64 [N, 5] with the columns REF, A, C, G, T -- a mutagenesis heat map needs nothing else:
    log2_affinity()[a:b, 1:] - log2_affinity()[a:b, :1] is the map of the sequence whose bases are a .. b - 1."""

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                 seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, keys, sums,
                 delta=None, all_rows=False):
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
        self.keys, self.sums = np.asarray(keys, dtype=np.uint32), np.asarray(sums, dtype=np.uint64)
        N = len(self.bases)
        if self.keys.shape != (N, 5) or self.sums.shape != (N, 5) or len(self.coord) != N or int(self.seq_offsets[-1]) != N:
            raise ValueError("the arrays do not fit the sequences")
        self.delta = None if delta is None else float(delta)
        self.all_rows = bool(all_rows)

    def __len__(self) -> int:
        return int(self._kept_cells()[0].size)

    @property
    def base_sequence(self) -> np.ndarray:
        """int64 [N]: the sequence of every base"""
        return np.repeat(np.arange(len(self.seq_count), dtype=np.int64), np.diff(self.seq_offsets))

    def log2_affinity(self) -> np.ndarray:
        """float64 [N, 5]: log2(sum) + log2_offset, NaN where the side has no window"""
        out = np.full(self.sums.shape, np.nan)
        some = self.sums > 0
        out[some] = np.log2(self.sums[some].astype(np.float64)) + self.log2_offset
        return out

    def _cells(self):
        """every (base, to-base != from-base) cell -> (base index n, column c in 1 .. 4), in (n, c) order"""
        frm = _COLUMN_OF[self.bases]
        cell = np.arange(1, 5, dtype=np.int64)[None, :] != frm[:, None]
        n, c = np.nonzero(cell)
        return n.astype(np.int64), c.astype(np.int64) + 1

    def _numbers(self, n, c):
        """of the cells (n, c) -> (ref best, alt best (int64, -1: none), ref p, alt p, ref log2, alt log2)"""
        rb, ab = decode_keys(self.keys[n, 0])[0], decode_keys(self.keys[n, c])[0]
        la = lambda s: np.where(s > 0, np.log2(np.where(s > 0, s, 1).astype(np.float64)) + self.log2_offset, np.nan)   # noqa: E731
        return rb, ab, scaled_pvalues(rb, self.ptable), scaled_pvalues(ab, self.ptable), la(self.sums[n, 0]), la(self.sums[n, c])

    def _kept_cells(self):
        n, c = self._cells()
        rb, ab, rp, ap, rl, al = self._numbers(n, c)
        keep = keep_rows(effect_codes(rp, ap, self.threshold), al - rl, self.delta, self.all_rows)
        return n[keep], c[keep]

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
        minus = strand == "-"
        text[minus] = _COMP[text[minus]][:, ::-1]
        out = np.ascontiguousarray(text).view(f"S{W}").reshape(-1).astype(f"U{W}").astype(object)
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
        letters = np.array([chr(k) for k in range(256)], dtype=object)
        data["from"] = letters[_UPPER[self.bases[n]]] if rows else np.zeros(0, dtype=object)
        data["to"] = letters[TO_BASES[c - 1]] if rows else np.zeros(0, dtype=object)
        rb, ab, rp, ap, rl, al = self._numbers(n, c)
        for side, best, p, col in (("ref", rb, rp, np.zeros(rows, dtype=np.int64)), ("alt", ab, ap, c)):
            _, rel, strand = decode_keys(self.keys[n, col])
            data[f"{side}_score"] = scaled_scores(best, self.scale, self.offset, self.width)
            data[f"{side}_pvalue"] = p
            data[f"{side}_start"] = np.where(best >= 0, rel.astype(np.float64), np.nan)
            data[f"{side}_strand"] = strand
            data[f"{side}_kmer"] = self._kmers(n, c, side)
        data["ref_log2_affinity"], data["alt_log2_affinity"], data["delta_log2_affinity"] = rl, al, al - rl
        data["effect"] = EFFECTS[effect_codes(rp, ap, self.threshold)]
        return pd.DataFrame(data)

    def summary_frame(self) -> pd.DataFrame:
        """a row per (region, coordinate, from, to) over the versions (not the count-0 reference sequence) that carry that
        coordinate non-inserted with that base: motif_id, motif_alt_id, sequence_name, position, from, to, versions, haplotypes,
        haplotypes_gain, haplotypes_loss, min_delta_log2_affinity, max_delta_log2_affinity, best_alt_score.  A row is kept when
        some haplotype gains or loses, or when a delta is given and the smallest or largest delta reaches it; all_rows keeps
        everything.  Rows in (region, position, from, to A C G T) order."""
        n, c = self._cells()
        seq = self.base_sequence[n] if len(n) else np.zeros(0, dtype=np.int64)
        on = (self.coord[n] >= 0) & (self.seq_version[seq] >= 0)
        n, c, seq = n[on], c[on], seq[on]
        rb, ab, rp, ap, rl, al = self._numbers(n, c)
        codes = effect_codes(rp, ap, self.threshold)
        region, frm = self.seq_region[seq], _UPPER[self.bases[n]].astype(np.int64)
        first, versions, haps, gain, loss, lo, hi, best = group_summary((region, self.coord[n].astype(np.int64), frm, c),
                                                                        self.seq_count[seq], codes, al - rl, ab)
        keep = np.ones(len(first), dtype=bool) if self.all_rows else (gain + loss) > 0
        if self.delta is not None and not self.all_rows:
            with np.errstate(invalid="ignore"):
                keep |= (np.abs(lo) >= self.delta) | (np.abs(hi) >= self.delta)
        k = np.flatnonzero(keep)
        f = first[k]
        letters = np.array([chr(j) for j in range(256)], dtype=object)
        rows = len(k)
        return pd.DataFrame({
            "motif_id": np.full(rows, self.motif_id, dtype=object), "motif_alt_id": np.full(rows, self.motif_alt_id, dtype=object),
            "sequence_name": self.region_names[region[f]] if rows else np.zeros(0, dtype=object),
            "position": self.coord[n[f]].astype(np.int64) + 1, "from": letters[frm[f]] if rows else np.zeros(0, dtype=object),
            "to": letters[TO_BASES[c[f] - 1]] if rows else np.zeros(0, dtype=object), "versions": versions[k], "haplotypes": haps[k],
            "haplotypes_gain": gain[k], "haplotypes_loss": loss[k], "min_delta_log2_affinity": lo[k],
            "max_delta_log2_affinity": hi[k], "best_alt_score": scaled_scores(best[k], self.scale, self.offset, self.width)})


def _region_spans(prep, rows, R: int):
    """-> (graph int64 [R], S, E int64 [R]) of the caller's region rows, clipped to their chromosomes"""
    graph, S, E = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    for gi, g in enumerate(prep.graphs):
        L = len(g.index.ref)
        r = rows[gi]
        graph[r] = gi
        S[r] = np.clip(np.asarray(prep.spans[gi][0], dtype=np.int64), 0, L)
        E[r] = np.maximum(np.clip(np.asarray(prep.spans[gi][1], dtype=np.int64), 0, L), S[r])
    return graph, S, E


def _with_references(hs, prep, rows):
    """The sequences of the scan: the versions of `hs`, then the reference sequence ref[S:E] of every region where no version is
    the reference's (count 0, version -1) -> (seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference,
    seq_offsets, bases, coord)"""
    R, V, G = len(hs.n_versions), len(hs), len(hs.group_names)
    v_region = hs.version_region
    spelled = np.bincount(v_region[hs.is_reference], minlength=R) > 0 if V else np.zeros(R, dtype=bool)
    graph, S, E = _region_spans(prep, rows, R)
    extra = np.flatnonzero(~spelled)
    length = (E - S)[extra]
    x_off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    within = np.arange(int(x_off[-1]), dtype=np.int64) - np.repeat(x_off[:-1], length)
    x_coord = np.repeat(S[extra], length) + within
    x_bases = np.zeros(int(x_off[-1]), dtype=np.uint8)
    x_graph = np.repeat(graph[extra], length)
    for gi, g in enumerate(prep.graphs):
        mine = x_graph == gi
        x_bases[mine] = np.asarray(g.index.ref, dtype=np.uint8)[x_coord[mine]]
    X = len(extra)
    region = np.concatenate([v_region, extra])
    version = np.concatenate([np.arange(V, dtype=np.int64) - hs.offsets[v_region], np.full(X, -1, dtype=np.int64)])
    old_off = np.concatenate([hs.seq_offsets, hs.seq_offsets[-1] + x_off[1:]]).astype(np.int64)
    # by region, a region's versions by number, its reference sequence last
    order = np.lexsort((version < 0, region))
    n = np.diff(old_off)[order]
    new_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    take = np.repeat(old_off[:-1][order] - new_off[:-1], n) + np.arange(int(new_off[-1]), dtype=np.int64)
    return (region[order], version[order], np.concatenate([hs.count.astype(np.int64), np.zeros(X, dtype=np.int64)])[order],
            np.concatenate([hs.group_counts.astype(np.int64).reshape(V, G), np.zeros((X, G), dtype=np.int64)])[order],
            np.concatenate([hs.is_reference, np.ones(X, dtype=bool)])[order], new_off,
            np.concatenate([hs.bases, x_bases])[take], np.concatenate([hs.coord, x_coord.astype(np.int32)])[take])


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
    from .haplotype_classes import compute_haplotype_classes
    from .haplotype_sequences import compute_haplotype_sequences
    require_single_gpu("the mutation scan", "is", "a gather of the sharded class matrices")
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    if delta is not None and not float(delta) >= 0:
        raise ValueError(f"delta {delta}: it must be >= 0")
    prep = prepare_graphs(graph, regions, chrom_names)
    _haplotype_set(prep, None, "the mutation scan")
    rows, region_names = _matrix_rows(prep)
    hc = compute_haplotype_classes(graph, regions, debug, args_obj, chrom_names, None, haplotype_groups)
    hs = compute_haplotype_sequences(graph, regions, debug, args_obj, chrom_names, None, None, classes=hc, coordinates=True)
    seqs = _with_references(hs, prep, rows)
    seq_offsets, bases, coord = np.ascontiguousarray(seqs[5]), np.ascontiguousarray(seqs[6]), seqs[7]
    forward_only = bool(getattr(args_obj, "noreverse", False))
    threshold = float(args_obj.threshold if threshold is None else threshold)
    out: List[Optional[MutationScan]] = [None] * len(motifs)
    for W, idxs in group_by_width(motifs).items():
        got, offsets, numbers = _scan_chunked([motifs[i] for i in idxs], seq_offsets, bases,
                                              None if weights is None else [weights[i] for i in idxs], temperature, forward_only,
                                              max_bytes)
        for m, i in enumerate(idxs):
            scale, offset, ptable = numbers[m]
            out[i] = MutationScan(motifs[i].motif_id, motifs[i].motif_name, W, scale, offset, ptable, offsets[m], threshold,
                                  region_names, hs.group_names, *seqs[:5], seq_offsets, bases, coord, got[m][0], got[m][1], delta,
                                  all_rows)
    return out


def compute_mutation_scan(motif, graph, regions, debug: bool, args_obj, chrom_names=None, haplotype_groups: Optional[Mapping] = None,
                          weights: Optional[np.ndarray] = None, temperature: float = 1.0, threshold: Optional[float] = None,
                          delta: Optional[float] = None, all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> MutationScan:
    """The mutation scan of `motif` (compute_mutation_scan_many for one motif)"""
    return compute_mutation_scan_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_groups,
                                      None if weights is None else [weights], temperature, threshold, delta, all_rows, max_bytes)[0]


# ---------------------------------------------------------------------------------------------------------------- the writers
def write_mutation_scan(table: MutationScan, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_mutation_scan.tsv (grafimo_mutation_scan_<motif_id>.tsv for one of several motifs), the detail rows, in the
    directory write_results uses for this motif -> the path written.  `out`: a text stream to write to instead (-f: stdout)."""
    return write_frame(table.to_frame(), out if out is not None else table_path(DETAIL_FILE, args_obj, motif, motif_num))


def write_mutation_scan_summary(table: MutationScan, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_mutation_scan_summary[_<motif_id>].tsv, a row per (region, coordinate, from, to), beside the detail rows"""
    return write_frame(table.summary_frame(), out if out is not None else table_path(SUMMARY_FILE, args_obj, motif, motif_num))


def print_mutation_scan(table: MutationScan) -> None:
    """-f: the detail rows, then the summary, on stdout instead of files"""
    write_mutation_scan(table, None, 1, None, out=sys.stdout)
    write_mutation_scan_summary(table, None, 1, None, out=sys.stdout)
