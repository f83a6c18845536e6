"""Mutation profile: what every single-base change does to a whole MOTIF SET -- how many motifs gain or lose a site, the most
significant gain and loss, and the motifs whose total affinity moves most, up and down.  Where mutation_scan answers its question
for one motif at a time (a dense table per motif), this table answers it for the set: one row per change, whatever the number
of motifs.

It is built on a device-side FOLD OVER THE MOTIF AXIS (grafimo_amd/csrc/gfm_scan_fold.hpp, gfm_scan_fold): the keys and sums a
scan entry leaves per motif stay on the device and are reduced there into a running state per (row, pair of columns).

THE RULE (include/grafimo_hip.h states it for the library; tests/mutation_profile_bruteforce.py on the host).  For every
(row, pair (ref column, alt column)) and every motif, with r, a the two keys' scores (key >> 8) - 1 (-1 for key 0) and R, A the
two sums:
  A side is a site when its key is not 0 and its score >= cutoff.
  gain when a is a site and r is not.  loss when r is a site and a is not.
  counts[gain] and counts[loss] count the motifs.
  Gain champion: the gaining motif with the smallest ptable[a].  Loss champion: the losing motif with the smallest ptable[r].
  Ties go to the smaller motif id.  A score >= table_len reads entry table_len - 1.
  Up champion: among motifs with A > R, the one with the largest A / R, compared exactly: motif 1 beats motif 2 when
  A1 * R2 > A2 * R1.  Down champion: among A < R, the largest R / A by the same rule.  Ties go to the smaller id.
  The empty state is all zero bytes.  Ids are stored as id + 1.
The state is a running one: folding the motifs in any order and any split gives the same bytes, which is what lets
profile_sequences take the motifs width by width and chunk by chunk.

Everything from the state to the frames is numpy group-bys; there is no Python step per row.
"""
import contextlib
import ctypes
import sys
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .device import _stream_ptr, _torch
from .graph_tables import group_by_width, table_path, write_frame
from .mutation_scan import BYTES_PER_BASE, COLUMNS, ENTRY
from .query_variants import decode_keys
from .sequence_scans import (_COLUMN_OF, _LETTERS, _UPPER, DEFAULT_MAX_BYTES, TO_BASES, SequenceTable, _checked_sequences,
                             _leased_chunks, chunk_step, enqueue, printed_windows, scan_inputs, stage)

DETAIL_FILE = "grafimo_mutation_profile"
SUMMARY_FILE = "grafimo_mutation_profile_summary"
TAG = "mutation_profile"
PAIRS = ((0, 1), (0, 2), (0, 3), (0, 4))                 # REF against A, C, G, T of the mutation scan's five columns
STATE_NAMES = ("counts", "site_motif", "site_keys", "site_p", "aff_motif", "aff_sums")
_STATE_TAILS = ((2,), (2,), (2, 2), (2,), (2,), (2, 2))  # a (row, pair)'s shape in each array
_STATE_HOST = (np.uint32, np.uint32, np.uint32, np.float64, np.uint32, np.uint64)
STATE_BYTES = 88                                         # per (row, pair)
STATE_BYTES_PER_BASE = STATE_BYTES * len(PAIRS)          # 352


# ---------------------------------------------------------------------------------------------------------------- the state
class FoldState:
    """The fold's running state, a struct of arrays over [rows][P]: counts uint32 [.., 2] (gain, loss), site_motif uint32
    [.., 2] (id + 1; 0: none), site_keys uint32 [.., 2, 2] (ref key, alt key), site_p float64 [.., 2], aff_motif uint32 [.., 2]
    (up, down), aff_sums uint64 [.., 2, 2] (ref sum, alt sum).  On the device the unsigned arrays are torch's signed types of
    the same width; cpu() gives numpy arrays of the types named here."""

    def __init__(self, counts, site_motif, site_keys, site_p, aff_motif, aff_sums):
        self.counts, self.site_motif, self.site_keys, self.site_p = counts, site_motif, site_keys, site_p
        self.aff_motif, self.aff_sums = aff_motif, aff_sums

    @classmethod
    def zeros(cls, rows: int, n_pairs: int, device=None) -> "FoldState":
        """the empty state: all zero bytes, on `device` (default: the current one)"""
        torch = _torch()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        kinds = (torch.int32, torch.int32, torch.int32, torch.float64, torch.int32, torch.int64)
        return cls(*[torch.zeros((rows, n_pairs) + tail, dtype=k, device=dev) for tail, k in zip(_STATE_TAILS, kinds)])

    @classmethod
    def host_zeros(cls, rows: int, n_pairs: int) -> "FoldState":
        return cls(*[np.zeros((rows, n_pairs) + tail, dtype=k) for tail, k in zip(_STATE_TAILS, _STATE_HOST)])

    def arrays(self) -> Tuple:
        return tuple(getattr(self, name) for name in STATE_NAMES)

    @property
    def shape(self) -> Tuple[int, int]:
        return tuple(self.counts.shape[:2])

    def cpu(self) -> "FoldState":
        """the six arrays as numpy arrays on the host (waits for the work enqueued on them)"""
        out = []
        for a, kind in zip(self.arrays(), _STATE_HOST):
            a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
            out.append(np.ascontiguousarray(a).view(kind))
        return FoldState(*out)

    def as_dict(self) -> dict:
        return dict(zip(STATE_NAMES, self.arrays()))


def _on_device(a, kind, torch, dev):
    """a device tensor as it is, a host array staged for the call (unsigned types as torch's signed ones of the same width)"""
    if torch.is_tensor(a):
        if not a.is_cuda or not a.is_contiguous():
            raise ValueError("a tensor given to fold_columns is contiguous and on the GPU")
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype=kind).view({np.uint32: np.int32, np.uint64: np.int64}.get(kind, kind))).to(dev)


def fold_columns(keys: Sequence, sums: Sequence, motif_ids: Sequence[int], cutoffs: Sequence[int], ptables: Sequence,
                 pairs: Sequence[Tuple[int, int]], state: Optional[FoldState] = None) -> FoldState:
    """The kernel on plain arrays: per motif keys uint32 [..., C] and sums uint64 [..., C] as a scan entry leaves them (device
    tensors, or host arrays staged for the call; the leading axes are the rows), its id, its score cutoff and its tail table
    float64 [table_len]; `pairs`: (ref column, alt column) -> the state on the device, [rows][len(pairs)]: `state` with the
    motifs folded in, or a new one.  The kernels are enqueued on the current stream and not waited for; the library refuses
    what the rule does not allow."""
    torch = _torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    M = len(motif_ids)
    if not (len(keys) == len(sums) == len(cutoffs) == len(ptables) == M):
        raise ValueError(f"{len(keys)} keys, {len(sums)} sums, {len(cutoffs)} cutoffs and {len(ptables)} tail tables for {M} motif ids")
    d_keys = [_on_device(k, np.uint32, torch, dev) for k in keys]
    d_sums = [_on_device(s, np.uint64, torch, dev) for s in sums]
    d_tabs = [_on_device(t, np.float64, torch, dev) for t in ptables]
    shape = tuple(d_keys[0].shape) if M else (0, 2)
    if len(shape) < 2 or any(tuple(k.shape) != shape for k in d_keys) or any(tuple(s.shape) != shape for s in d_sums):
        raise ValueError("keys and sums of every motif have one shape [..., columns]")
    rows, C, P = int(np.prod(shape[:-1], dtype=np.int64)), int(shape[-1]), len(pairs)
    if state is None:
        state = FoldState.zeros(rows, P, dev)
    elif state.shape != (rows, P) or not all(torch.is_tensor(a) and a.is_cuda and a.is_contiguous() for a in state.arrays()):
        raise ValueError(f"the state given is on the GPU and holds [{rows}][{P}] cells")
    ids = np.ascontiguousarray(motif_ids, dtype=np.int32)
    cuts = np.ascontiguousarray(cutoffs, dtype=np.int32)
    lens = np.array([t.numel() for t in d_tabs], dtype=np.int32)
    prs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    vp = ctypes.c_void_p
    nv.check(nv.lib().gfm_scan_fold(
        M, ids.ctypes.data, cuts.ctypes.data, (vp * M)(*[t.data_ptr() for t in d_tabs]), lens.ctypes.data, rows, C, P,
        prs.ctypes.data, (vp * M)(*[k.data_ptr() for k in d_keys]), (vp * M)(*[s.data_ptr() for s in d_sums]),
        *[a.data_ptr() for a in state.arrays()], _stream_ptr(None)))
    return state


# ---------------------------------------------------------------------------------------------------------------- the sequences
def _profile(motifs: Sequence, seq_offsets, bases, threshold: float, weights, temperature, forward_only, max_bytes):
    """-> (the state on the host [n_bases][4], per motif (width, scale, offset, log2 offset)).  Per width and per chunk of
    motifs: the mutation scan's entry into result tensors that stay on the device, then the fold behind it on the same stream."""
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    torch = _torch()
    N = len(bases)
    info: List = [None] * len(motifs)
    per_motif, fixed = BYTES_PER_BASE * N, STATE_BYTES_PER_BASE * N
    if motifs and per_motif + fixed > int(max_bytes):
        raise ValueError(f"{motifs[0].motif_id}: the keys and sums of one motif and the profile's state over {N} bases hold "
                         f"{per_motif + fixed} bytes, more than max_bytes = {int(max_bytes)}: scan fewer sequences at a time, or raise "
                         "max_bytes")
    state = FoldState.zeros(N, len(PAIRS)) if N else FoldState.host_zeros(0, len(PAIRS))
    kept = None                                          # the staged inputs whose bases and result tensors every chunk reuses
    for W, idxs in group_by_width(motifs).items():
        ms = [motifs[i] for i in idxs]
        ws = None if weights is None else [weights[i] for i in idxs]
        step = min(chunk_step(ms, N, per_motif, int(max_bytes) - fixed), len(ms))
        with contextlib.closing(_leased_chunks(ms, ws, temperature, step)) as chunks:   # (a failure gives the handles back)
            for m0, dms, tables, offs, nums in chunks:
                M = len(dms)
                for k in range(M):
                    info[idxs[m0 + k]] = (W, nums[k][0], nums[k][1], offs[k])
                if N == 0:
                    continue
                if kept is None or kept[4].shape[0] < M:
                    kept = staged = stage(tables, seq_offsets, bases, (N, len(COLUMNS)))
                else:                                    # only the weights are new: the bases and the result tensors serve again
                    d_tabs = [torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64)).to(kept[1].device)
                              for t in tables]
                    staged = (seq_offsets, kept[1], d_tabs, max(int(t.max()) for t in tables), kept[4][:M], kept[5][:M], kept[6])
                keys, sums = enqueue(dms, staged, forward_only, ENTRY)
                fold_columns([keys[m] for m in range(M)], [sums[m] for m in range(M)], [idxs[m0 + k] for k in range(M)],
                             [dm.pvalue_cutoff(threshold) for dm in dms], [nums[k][2] for k in range(M)], PAIRS, state)
    return state.cpu(), info


def profile_sequences(motifs: Sequence, seq_offsets, bases, threshold: float, weights: Optional[Sequence[np.ndarray]] = None,
                      temperature: float = 1.0, forward_only: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> FoldState:
    """The profile on plain arrays: sequences (`seq_offsets` int64 [V + 1] from 0, `bases` uint8) and motifs of ANY widths -> the
    state on the host, [n_bases][4]: per base the pairs REF -> A, C, G, T.  The motif id is the index in `motifs`, the cutoff
    DeviceMotif.pvalue_cutoff(threshold), the tail table the handle's.  The dense per-motif tables never leave the device: the
    motifs are taken per width in chunks whose result tensors (60 bytes a base and motif) and the state (352 bytes a base,
    once) stay under `max_bytes`."""
    return _profile(motifs, seq_offsets, bases, float(threshold), weights, temperature, forward_only, max_bytes)[0]


# ---------------------------------------------------------------------------------------------------------------- the table
def _log2_ratio(alt: np.ndarray, ref: np.ndarray, some: np.ndarray) -> np.ndarray:
    """log2(alt) - log2(ref) of uint64 sums where `some`, NaN elsewhere; a sum of 0 gives an infinity"""
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.log2(alt.astype(np.float64)) - np.log2(ref.astype(np.float64))
    return np.where(some, d, np.nan)


class MutationProfile(SequenceTable):
    """The table of a motif set over S sequences of N bases in all (see the module's docstring).  The sequences' arrays are
    SequenceTable's.  Per motif [M], in the order of the call (a state's motif id is the index): motif_ids, motif_alt_ids,
    widths, scales, offsets, log2_offsets.  state: a FoldState on the host, [N][4]: per base the pairs REF -> A, C, G, T."""

    def __init__(self, motif_ids, motif_alt_ids, widths, scales, offsets, log2_offsets, threshold, region_names, group_names,
                 seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, state: FoldState,
                 delta=None, all_rows=False):
        super().__init__("", "", 0, 1, 0.0, np.zeros(0), threshold, region_names, group_names, seq_region, seq_version, seq_count,
                         seq_group_counts, seq_is_reference, seq_offsets, bases, coord, all_rows)
        self.motif_ids, self.motif_alt_ids = np.asarray(motif_ids, dtype=object), np.asarray(motif_alt_ids, dtype=object)
        self.widths, self.scales = np.asarray(widths, dtype=np.int64), np.asarray(scales, dtype=np.int64)
        self.offsets, self.log2_offsets = np.asarray(offsets, dtype=np.float64), np.asarray(log2_offsets, dtype=np.float64)
        self.state = state.cpu()
        N = len(self.bases)
        if not self._fits(*[(a, (N, len(PAIRS)) + tail) for a, tail in zip(self.state.arrays(), _STATE_TAILS)]):
            raise ValueError("the state does not fit the sequences")
        M = len(self.motif_ids)
        if not all(len(v) == M for v in (self.motif_alt_ids, self.widths, self.scales, self.offsets, self.log2_offsets)):
            raise ValueError("the motifs' arrays differ in length")
        if max(int(self.state.site_motif.max(initial=0)), int(self.state.aff_motif.max(initial=0))) > M:
            raise ValueError(f"the state names a motif beyond the {M} given")
        self.delta = None if delta is None else float(delta)

    def _motif_columns(self, rows: int, region) -> dict:
        """a row speaks of the whole set: the frames start with sequence_name"""
        return {"sequence_name": self.region_names[region] if rows else np.zeros(0, dtype=object)}

    def __len__(self) -> int:
        return int(self._kept_cells()[0].size)

    def _cells(self):
        """every (base, to-base != from-base) cell -> (base index n, column c in 1 .. 4), in (n, c) order; the pair is c - 1"""
        frm = _COLUMN_OF[self.bases]
        cell = np.arange(1, 5, dtype=np.int64)[None, :] != frm[:, None]
        n, c = np.nonzero(cell)
        return n.astype(np.int64), c.astype(np.int64) + 1

    def _affinity_deltas(self, n, c):
        """-> (up, down): log2(A) - log2(R) of the two affinity champions, NaN where there is none"""
        s = self.state
        sums, some = s.aff_sums[n, c - 1], s.aff_motif[n, c - 1] > 0
        return (_log2_ratio(sums[:, 0, 1], sums[:, 0, 0], some[:, 0]), _log2_ratio(sums[:, 1, 1], sums[:, 1, 0], some[:, 1]))

    def _kept_cells(self):
        n, c = self._cells()
        if self.all_rows:
            return n, c
        keep = self.state.counts[n, c - 1].sum(axis=1) > 0
        if self.delta is not None:
            up, down = self._affinity_deltas(n, c)
            with np.errstate(invalid="ignore"):
                keep |= (np.abs(up) >= self.delta) | (np.abs(down) >= self.delta)
        return n[keep], c[keep]

    def _names(self, id1: np.ndarray):
        """stored ids (id + 1, 0: none) -> (motif_id, motif_alt_id), '' for none"""
        some = id1 > 0
        m = np.where(some, id1.astype(np.int64) - 1, 0)
        if not len(self.motif_ids):
            return np.full(len(id1), "", dtype=object), np.full(len(id1), "", dtype=object)
        return np.where(some, self.motif_ids[m], ""), np.where(some, self.motif_alt_ids[m], "")

    def _kmers(self, n, c, key, W: int, alt: bool) -> np.ndarray:
        """object: the windows of width W the keys name at the bases n as printed ('-': reverse complemented), with the base of
        column c put in under `alt`; '' where the key is 0 -- MutationScan._kmers for a width per call"""
        if not len(n):
            return np.zeros(0, dtype=object)
        _, rel, strand = decode_keys(key)
        some = key > 0
        start = np.where(some, n + rel, 0)
        idx = np.minimum(start[:, None] + np.arange(W, dtype=np.int64)[None, :], max(len(self.bases) - 1, 0))
        text = _UPPER[self.bases[idx]]
        if alt:
            text[np.flatnonzero(some), (-rel)[some]] = TO_BASES[c[some] - 1]
        out = printed_windows(text, strand == "-")
        out[~some] = ""
        return out

    def _champion_columns(self, data: dict, n, c) -> None:
        s = self.state
        for side, name in enumerate(("gain", "loss")):
            id1 = s.site_motif[n, c - 1, side]
            some = id1 > 0
            m = np.where(some, id1.astype(np.int64) - 1, 0)
            kr, ka = s.site_keys[n, c - 1, side, 0], s.site_keys[n, c - 1, side, 1]
            W = self.widths[m] if len(self.widths) else np.zeros(len(n), dtype=np.int64)
            scale = self.scales[m] if len(self.scales) else np.ones(len(n), dtype=np.int64)
            offset = self.offsets[m] if len(self.offsets) else np.zeros(len(n))
            data[f"{name}_motif_id"], data[f"{name}_motif_alt_id"] = self._names(id1)
            for which, key in (("ref", kr), ("alt", ka)):
                best = np.where(some, decode_keys(key)[0], -1)
                data[f"{name}_{which}_score"] = np.where(best >= 0, best.astype(np.float64) / scale + W * offset, np.nan)
            data[f"{name}_pvalue"] = np.where(some, s.site_p[n, c - 1, side], np.nan)
            # the site itself: the ALT side's window of a gain, the REF side's of a loss
            site = np.where(some, ka if side == 0 else kr, 0).astype(np.uint32)
            _, rel, strand = decode_keys(site)
            data[f"{name}_start"] = np.where(site > 0, rel.astype(np.float64), np.nan)
            data[f"{name}_strand"] = strand
            kmer = np.full(len(n), "", dtype=object)
            for w in np.unique(W[some]).tolist():            # (a pass per width of the set, not per row)
                f = np.flatnonzero(some & (W == w))
                kmer[f] = self._kmers(n[f], c[f], site[f], int(w), side == 0)
            data[f"{name}_kmer"] = kmer

    def to_frame(self) -> pd.DataFrame:
        """a row per (sequence, offset, to-base != from-base) the filter keeps -- some motif gains or loses, or a delta is given
        and an affinity champion's |log2(A) - log2(R)| reaches it; all_rows keeps everything: sequence_name, version, haplotypes,
        one haplotypes_<GROUP> per group, is_reference, position, inserted, from, to, motifs_gain, motifs_loss; for gain_ and
        loss_ the champion's motif_id, motif_alt_id, ref_score, alt_score, pvalue, and start, strand, kmer of the site (the ALT
        side's best window of a gain, the REF side's of a loss), with the champion's own width; up_motif_id,
        up_delta_log2_affinity, down_motif_id, down_delta_log2_affinity (the motif's log2 offset cancels).  Empty / NaN where
        there is no champion.  Rows in (sequence, offset, to A C G T) order."""
        n, c = self._kept_cells()
        data = self._leading_columns(n)
        data["from"] = _LETTERS[_UPPER[self.bases[n]]]
        data["to"] = _LETTERS[TO_BASES[c - 1]]
        counts = self.state.counts[n, c - 1]
        data["motifs_gain"], data["motifs_loss"] = counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64)
        self._champion_columns(data, n, c)
        up, down = self._affinity_deltas(n, c)
        data["up_motif_id"], data["up_delta_log2_affinity"] = self._names(self.state.aff_motif[n, c - 1, 0])[0], up
        data["down_motif_id"], data["down_delta_log2_affinity"] = self._names(self.state.aff_motif[n, c - 1, 1])[0], down
        return pd.DataFrame(data)

    def summary_frame(self) -> pd.DataFrame:
        """a row per (region, coordinate, from, to) over the versions (not the count-0 reference sequence) that carry that
        coordinate non-inserted with that base: sequence_name, position, from, to, versions, haplotypes, haplotypes_gain,
        haplotypes_loss (the haplotypes of the versions where some motif gains / loses), max_motifs_gain, max_motifs_loss,
        gain_motif_id, loss_motif_id (the champion with the smallest p over the versions, the first version on ties).  A row is
        kept when haplotypes_gain + haplotypes_loss > 0; all_rows keeps everything.  Rows in (region, position, from, to A C G
        T) order."""
        n, c = self._cells()
        seq = self._sequence_of(n)
        on = (self.coord[n] >= 0) & (self.seq_version[seq] >= 0)
        n, c, seq = n[on], c[on], seq[on]
        frm = _UPPER[self.bases[n]].astype(np.int64)
        region, haps = self.seq_region[seq], self.seq_count[seq]
        counts = self.state.counts[n, c - 1].astype(np.int64)
        rows = len(n)
        order = np.lexsort((c, frm, self.coord[n].astype(np.int64), region))       # (stable: a group's versions stay in order)
        head = np.zeros(rows, dtype=bool)
        if rows:
            head[0] = True
            for k in (region, self.coord[n], frm, c):
                k = np.asarray(k)[order]
                head[1:] |= k[1:] != k[:-1]
        at = np.flatnonzero(head)
        group = np.cumsum(head) - 1                                                 # of the sorted rows
        add = lambda v: np.add.reduceat(v[order], at) if rows else np.zeros(0, dtype=np.int64)        # noqa: E731
        top = lambda v: np.maximum.reduceat(v[order], at) if rows else np.zeros(0, dtype=np.int64)    # noqa: E731
        gain, loss = add(np.where(counts[:, 0] > 0, haps, 0)), add(np.where(counts[:, 1] > 0, haps, 0))
        keep = np.ones(len(at), dtype=bool) if self.all_rows else (gain + loss) > 0
        k = np.flatnonzero(keep)
        f = order[at[k]]
        data = self._motif_columns(len(k), region[f])
        data["position"] = self.coord[n[f]].astype(np.int64) + 1
        data["from"], data["to"] = _LETTERS[frm[f]], _LETTERS[TO_BASES[c[f] - 1]]
        data.update({"versions": add(np.ones(rows, dtype=np.int64))[k], "haplotypes": add(haps)[k], "haplotypes_gain": gain[k],
                     "haplotypes_loss": loss[k], "max_motifs_gain": top(counts[:, 0])[k], "max_motifs_loss": top(counts[:, 1])[k]})
        for side, name in enumerate(("gain", "loss")):
            id1 = self.state.site_motif[n, c - 1, side][order]
            p = np.where(id1 > 0, self.state.site_p[n, c - 1, side][order], np.inf)
            best = np.lexsort((np.arange(rows), p, group))                          # per group: the smallest p, the first version
            lead = best[at] if rows else np.zeros(0, dtype=np.int64)               # (the groups are runs of equal length in both orders)
            data[f"{name}_motif_id"] = self._names(id1[lead])[0][k]
        return pd.DataFrame(data)


def compute_mutation_profile(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                             haplotype_groups: Optional[Mapping] = None, weights: Optional[Sequence[np.ndarray]] = None,
                             temperature: float = 1.0, threshold: Optional[float] = None, delta: Optional[float] = None,
                             all_rows: bool = False, max_bytes: int = DEFAULT_MAX_BYTES) -> MutationProfile:
    """The mutation profile of the motif set `motifs` (any widths) over the versions the panel spells in the regions, one table
    per call (see the module's docstring).  `graph` / `regions`, args_obj (noreverse and threshold; `threshold` overrides it),
    `temperature` / `weights` and the sequences are compute_mutation_scan_many's.  The frames keep a row when some motif gains
    or loses, or when an affinity champion's |delta| >= `delta` if a delta is given; `all_rows` keeps everything."""
    seqs, region_names, group_names, forward_only, threshold = scan_inputs(
        "the mutation profile", motifs, graph, regions, debug, args_obj, chrom_names, haplotype_groups, weights, delta, threshold)
    state, info = _profile(motifs, seqs[5], seqs[6], threshold, weights, temperature, forward_only, max_bytes)
    return MutationProfile([m.motif_id for m in motifs], [m.motif_name for m in motifs], [i[0] for i in info], [i[1] for i in info],
                           [i[2] for i in info], [i[3] for i in info], threshold, region_names, group_names, *seqs, state, delta,
                           all_rows)


# ---------------------------------------------------------------------------------------------------------------- the writers
def write_mutation_profile(table: MutationProfile, args_obj, out=None) -> Optional[str]:
    """grafimo_mutation_profile.tsv, the detail rows of the call's motif set -> the path written.  `out`: a text stream to write
    to instead (-f: stdout)."""
    return write_frame(table.to_frame(), out if out is not None else table_path(DETAIL_FILE, args_obj, tag=TAG))


def write_mutation_profile_summary(table: MutationProfile, args_obj, out=None) -> Optional[str]:
    """grafimo_mutation_profile_summary.tsv, the summary rows, beside the detail rows"""
    return write_frame(table.summary_frame(), out if out is not None else table_path(SUMMARY_FILE, args_obj, tag=TAG))


def print_mutation_profile(table: MutationProfile) -> None:
    """-f: the detail rows, then the summary, on stdout instead of files"""
    write_mutation_profile(table, None, out=sys.stdout)
    write_mutation_profile_summary(table, None, out=sys.stdout)
