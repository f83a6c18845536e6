"""Shuffle null: how unusual a sequence's best motif score and total binding affinity are, against K composition-preserving
shuffles of that very sequence -- and, over all regions of a call, which motifs are over-represented at all.  The best window's
p-value of the other tables is a per-window one and ignores that a 500-base region offers about 1 000 windows; log2_affinity has
no significance of its own.  A mononucleotide shuffle is the i.i.d. background the p-value DP already assumes, with the
sequence's own length and composition.

THE RULE (include/grafimo_hip.h states it for the library; tests/shuffle_null_bruteforce.py on the host).  All arithmetic on
64-bit words is modulo 2^64.
  G = 0x9E3779B97F4A7C15.
  mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
For a sequence x of n bases with a caller-given uint64 key k, a uint64 seed and the replicates r = 0 .. K - 1:
  s0 = mix(mix(seed + k G) + r).
  y starts as a copy of x: the bytes as they are, non-ACGT and lower case included.
  For i = n - 1 down to 1:  u = mix(s0 + i G);  j = ((u >> 32) (i + 1)) >> 32;  swap y[i] and y[j].
  The multiply-shift bias is at most n / 2^32 and is part of the rule.  The permutation depends on (seed, k, r, n) only, not on
  the motif or on anything else in the call.
Scores, for a motif of width W:
  Every window start 0 .. n - W of a sequence is scored once per strand, + only under GFM_GRAPH_FORWARD_ONLY (--no-reverse).
  A window that holds a base that is not A/C/G/T scores min_val on both strands.  Case is folded, as base_code does.
  best = the largest score over windows and strands, -1 when n < W.
  sum = the exact uint64 sum of w[score] over windows and strands, 0 when there are none.
  obs_best, obs_sum: those of x itself.
Per (motif, sequence): obs_best int32, obs_sum uint64, ge_best = #{r : best_r >= obs_best}, ge_sum = #{r : sum_r >= obs_sum},
uint32.  Ties count, which is the conservative choice.  n < W gives ge_best = ge_sum = K.
Per (motif, replicate): rep_hits[r] = the sum over the sequences v of seq_weight[v] [best_{v,r} >= cut[m]], uint64; cut[m] is a
scaled score in [0, L].
Per (motif, sequence, replicate), when asked for: the dense rep_best int32 [S, K] and rep_sum uint64 [S, K].
The result for one sequence depends on (seed, its key, its bytes, K, the motif, the weights, the flag) only.

THE RULE OF ORDER 2 (order=2, --null-order 2; include/grafimo_hip.h states it for the library; tests/doublet_null_bruteforce.py
on the host): the replicates keep x's doublets.  A mononucleotide shuffle destroys what real genomic sequence is made of -- CpG
depletion, poly-A/T runs, simple repeats -- and so inflates the significance of every motif whose consensus holds a depleted or
an enriched doublet.  mix, G, the key k, the seed and the replicates r are the order-1 rule's.
  draw(t, m) = ((mix(s0 + t G) >> 32) m) >> 32, with m < 2^31.
  Alphabet.  c[i] = base_code(x[i]): 0 .. 3 for A/C/G/T with case folded, 4 for anything else.  A replicate is a sequence of
  codes.  Scores are taken on codes, as now.
  Stream.  s0 = mix(mix(seed + k G) + r + 2^63).  The 2^63 separates the order-2 stream from the order-1 stream of the same
  (seed, key, replicate).
  Buckets.  cnt[a] = #{i < n - 1 : c[i] = a}; b[a] is the exclusive prefix sum over a = 0 .. 4.  E has length n - 1 and is the
  stable counting sort of the successors: for i = 0 .. n - 2 in order, c[i + 1] is appended to bucket c[i].  E is the same for
  all replicates of a sequence; the last entry of a bucket is x's own last exit from that symbol.
  Arborescence.  Wilson's algorithm, rooted at root = c[n - 1].  in_tree = {root}, a step counter t = 0, cap = walk_cap n.
  For u = 0 .. 4 in order, if cnt[u] > 0 and u is not in the tree: cur = u; while cur is not in the tree: if t == cap the
  replicate is capped and the stage stops; else e = b[cur] + draw(n + t, cnt[cur]), t += 1, last[cur] = e, cur = E[e].  Then
  retrace from u along E[last[.]], adding vertices to the tree.
  A capped replicate takes last[a] = b[a + 1] - 1 for every a: x's own last exits, which always form an arborescence.
  Per-bucket shuffle.  For a = 0 .. 4 with cnt[a] > 0: m = cnt[a]; if a != root, swap E[last[a]] with E[b[a + 1] - 1] and
  m -= 1; for i = m - 1 down to 1: p = b[a] + i, j = draw(p, i + 1), swap E[p] and E[b[a] + j].  The Fisher-Yates counters
  p <= n - 2 and the walk's counters >= n never meet.
  Euler walk.  y[0] = c[0], ptr[a] = b[a]; for i = 1 .. n - 1: y[i] = E[ptr[y[i - 1]]], then ptr[y[i - 1]] += 1.  For n <= 1,
  y = c.
  Everything else is as order 1: the windows, the strands, min_val for a window with code 4, best, sum, obs_*, ge_* with ties
  counting, rep_hits, rep_best, rep_sum, and n < W.
Every replicate has x's length, first and last code and all 25 doublet counts of x; uncapped replicates are uniform over such
sequences (Altschul and Erickson, with Wilson's arborescence) up to the multiply-shift bias.  The arborescence's walk is a
random loop, so it is bounded by construction: walk_cap (default 64, in [0, 1024]; not a command-line option) is far from
typical use -- a random 300-base sequence walks about 6 steps, (AC)^150 G about 300 --, and 0 caps every replicate.

THE KEYS.  content_keys gives every sequence the key mix(sum over its offsets o of mix(upper(x[o]) + 256 o), plus n): equal
sequences get equal nulls whatever call they are in, and whatever their neighbours.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_shuffle_null.hpp, gfm_sequence_shuffle_null): a wavefront takes 64 replicates of
one sequence, a lane per replicate, shuffles them once for up to 16 motifs and slides every motif's window over each.  Order 2
(gfm_sequence_shuffle_null_order) replaces the fill and the shuffle: the wave sorts the successors into the image, each lane
draws its arborescence, shuffles its buckets and walks; the scoring is the same code.
Everything from the kernel's arrays to the frames is numpy; there is no Python step per sequence, replicate or base.
"""
import contextlib
import ctypes
import sys
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _stream_ptr, _torch
from .graph_tables import scaled_pvalues, scaled_scores, table_path, write_frame
from .sequence_scans import _UPPER, DEFAULT_MAX_BYTES, _checked_sequences, _leased_chunks, scan_inputs, tables_by_width

TABLE_FILE = "grafimo_shuffle_null"
ENRICHMENT_FILE = "grafimo_motif_enrichment"
DEFAULT_REPLICATES = 1000
MAX_REPLICATES = nv.GFM_NULL_MAX_REPLICATES
DEFAULT_WALK_CAP = 64
MAX_WALK_CAP = nv.GFM_NULL_MAX_WALK_CAP
G = np.uint64(0x9E3779B97F4A7C15)
ENRICHMENT_COLUMNS = ["motif_id", "motif_alt_id", "width", "regions", "observed_hits", "null_mean_hits", "null_max_hits",
                      "enrichment_pvalue", "replicates"]


# ---------------------------------------------------------------------------------------------------------------- the keys
def mix(z) -> np.ndarray:
    """THE RULE's mix on uint64 (arrays or one number), modulo 2^64"""
    z = np.array(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def content_keys(seq_offsets, bases=None):
    """uint64 [S]: per sequence mix(sum over its offsets o of mix(upper(x[o]) + 256 o), plus n), modulo 2^64 -- the key of a
    sequence is its content's, so equal sequences get equal nulls whatever call they are in.  content_keys(x) with one argument
    takes the bytes of ONE sequence -> its key as an int."""
    if bases is None:
        x = np.frombuffer(bytes(seq_offsets), dtype=np.uint8)
        return int(content_keys(np.array([0, len(x)], dtype=np.int64), x)[0])
    if isinstance(bases, (bytes, bytearray)):
        bases = np.frombuffer(bytes(bases), dtype=np.uint8)
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    n = np.diff(seq_offsets)
    within = np.arange(len(bases), dtype=np.int64) - np.repeat(seq_offsets[:-1], n)
    with np.errstate(over="ignore"):
        each = mix(_UPPER[bases].astype(np.uint64) + np.uint64(256) * within.astype(np.uint64))
        run = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(each, dtype=np.uint64)])
        return mix(run[seq_offsets[1:]] - run[seq_offsets[:-1]] + n.astype(np.uint64))


def pvalue_cut(ptable: np.ndarray, threshold: float) -> int:
    """the smallest scaled score whose tail-table value is < threshold (the report's strict rule); L = len(ptable) if none"""
    below = np.flatnonzero(np.asarray(ptable, dtype=np.float64) < float(threshold))
    return int(below[0]) if len(below) else len(ptable)


def null_pvalues(ge: np.ndarray, replicates: int) -> np.ndarray:
    """(1 + ge) / (K + 1): the observed sequence counts as one of its own shuffles, so no p-value is 0"""
    return (1.0 + np.asarray(ge, dtype=np.float64)) / (float(replicates) + 1.0)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _result_bytes(n_seqs: int, K: int, keep: bool) -> int:
    """a motif's device result tensors over n_seqs sequences: the observed pair, the two counts, rep_hits, the dense arrays"""
    return n_seqs * (4 + 8 + 4 + 4) + 8 * K + (n_seqs * K * (4 + 8) if keep else 0)


_RESULTS = (("obs_best", np.int32), ("obs_sum", np.uint64), ("ge_best", np.uint32), ("ge_sum", np.uint32), ("rep_hits", np.uint64),
            ("rep_best", np.int32), ("rep_sum", np.uint64))


def _shape(name: str, M: int, S: int, K: int):
    return {"rep_hits": (M, K), "rep_best": (M, S, K), "rep_sum": (M, S, K)}.get(name, (M, S))


def _stage(tables, seq_offsets: np.ndarray, bases: np.ndarray, keys, seq_weights, K: int, keep: bool):
    """the inputs of gfm_sequence_shuffle_null on the current device and its result tensors, the motif first -> (seq_offsets
    (host), the tensors of the bases, the keys and the sequence weights, the weight tables' tensors, the largest weight, the
    result tensors by name -- rep_best and rep_sum only with `keep` --, the status word)"""
    torch = _torch()
    M, S = len(tables), len(seq_offsets) - 1
    dev = torch.device("cuda", torch.cuda.current_device())
    put = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)        # noqa: E731
    signed = {np.int32: torch.int32, np.uint32: torch.int32, np.uint64: torch.int64}
    res = {name: torch.empty(_shape(name, M, S, K), dtype=signed[t], device=dev) for name, t in _RESULTS[:7 if keep else 5]}
    return (seq_offsets, put(np.array(bases, dtype=np.uint8), np.uint8),                # (a copy: the caller's may be read-only)
            put(np.asarray(keys, dtype=np.uint64), np.int64), put(np.asarray(seq_weights, dtype=np.uint32), np.int32),
            [put(np.asarray(t, dtype=np.uint64), np.int64) for t in tables], max(int(t.max()) for t in tables), res,
            torch.zeros(1, dtype=torch.int32, device=dev))


def _checked_order(order, walk_cap=DEFAULT_WALK_CAP):
    if order not in (1, 2):
        raise ValueError(f"order {order}: the shuffle null is of order 1 (mononucleotide) or 2 (doublet-preserving)")
    if not 0 <= int(walk_cap) <= MAX_WALK_CAP:
        raise ValueError(f"walk_cap {walk_cap}: outside [0, {MAX_WALK_CAP}]")
    return int(order), int(walk_cap)


def _enqueue(dms, staged, K: int, seed: int, cuts, forward_only: bool, order: int = 1, walk_cap: int = DEFAULT_WALK_CAP):
    """gfm_sequence_shuffle_null (order 1) or gfm_sequence_shuffle_null_order (order 2) over staged inputs (_stage): every
    result tensor is overwritten -> the tensors by name"""
    seq_offsets, d_bases, d_keys, d_wts, d_tabs, max_weight, res, status = staged
    M = len(dms)
    vp = ctypes.c_void_p
    per_motif = lambda name: (vp * M)(*[res[name][m].data_ptr() if name in res else None for m in range(M)])     # noqa: E731
    h_cuts = np.ascontiguousarray(cuts, dtype=np.int32)
    entry, more = (nv.lib().gfm_sequence_shuffle_null, ()) if order == 1 else (nv.lib().gfm_sequence_shuffle_null_order,
                                                                               (int(order), int(walk_cap)))
    nv.check(entry(
        (vp * M)(*[x.handle for x in dms]), M, (vp * M)(*[t.data_ptr() for t in d_tabs]), max_weight, len(seq_offsets) - 1,
        seq_offsets.ctypes.data, d_bases.data_ptr(), d_keys.data_ptr(), d_wts.data_ptr(), int(K), int(seed) & (2**64 - 1), *more,
        h_cuts.ctypes.data, nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0, *[per_motif(name) for name, _ in _RESULTS],
        status.data_ptr(), _stream_ptr(None)))
    return res


def _launch(dms, tables, seq_offsets, bases, keys, seq_weights, K, seed, cuts, forward_only, keep, order=1,
            walk_cap=DEFAULT_WALK_CAP) -> Dict[str, np.ndarray]:
    """the kernel for leased motifs of one width over the sequences -> the arrays by name, each with the motif first"""
    M, S = len(dms), len(seq_offsets) - 1
    if S == 0:
        return {name: np.zeros(_shape(name, M, S, K), dtype=t) for name, t in _RESULTS[:7 if keep else 5]}
    res = _enqueue(dms, _stage(tables, seq_offsets, bases, keys, seq_weights, K, keep), K, seed, cuts, forward_only, order, walk_cap)
    return {name: res[name].cpu().numpy().view(t) for name, t in _RESULTS if name in res}


def _null_chunked(motifs: Sequence, seq_offsets, bases, replicates, seed, seq_keys, seq_weights, cuts, threshold, weights,
                  temperature, forward_only, keep, max_bytes, order=1, walk_cap=DEFAULT_WALK_CAP):
    """-> (per motif its dict of arrays (with "cut"), per motif its log2 offset, per motif (scale, offset, ptable)): the motifs
    leased (sequence_scans._leased_chunks) and the sequences taken in chunks whose device result tensors stay under max_bytes;
    rep_hits of sequence chunks are added here.  `cuts` None: pvalue_cut at `threshold`, or L without one."""
    S, K = len(seq_offsets) - 1, int(replicates)
    if not 1 <= K <= MAX_REPLICATES:
        raise ValueError(f"replicates {replicates}: outside [1, {MAX_REPLICATES}]")
    order, walk_cap = _checked_order(order, walk_cap)
    keys = content_keys(seq_offsets, bases) if seq_keys is None else np.ascontiguousarray(seq_keys, dtype=np.uint64)
    wts = np.ones(S, dtype=np.uint32) if seq_weights is None else np.ascontiguousarray(seq_weights, dtype=np.uint32)
    if keys.shape != (S,) or wts.shape != (S,):
        raise ValueError(f"{S} sequences, seq_keys of shape {keys.shape}, seq_weights of shape {wts.shape}")
    if cuts is not None and len(cuts) != len(motifs):
        raise ValueError(f"{len(cuts)} cuts for {len(motifs)} motifs")
    one = _result_bytes(1, K, keep)
    if S and one > int(max_bytes):
        raise ValueError(f"{motifs[0].motif_id}: the results of sequence 0 alone over {K} replicates hold {one} bytes, more than "
                         f"max_bytes = {int(max_bytes)}: ask for fewer replicates, drop keep_replicates, or raise max_bytes")
    per_seq = _result_bytes(1, K, keep) - 8 * K
    seq_step = max(1, min(S, (int(max_bytes) - 8 * K) // per_seq)) if S else 1
    step = max(1, int(max_bytes) // _result_bytes(S, K, keep)) if seq_step >= S else 1
    results, offsets, numbers = [], [], []
    with contextlib.closing(_leased_chunks(motifs, weights, temperature, step)) as chunks:     # (a failure gives the handles back)
        for m0, dms, tables, offs, nums in chunks:
            cut = [int(cuts[m0 + m]) if cuts is not None else (dm.L if threshold is None else pvalue_cut(nums[m][2], threshold))
                   for m, dm in enumerate(dms)]
            parts = []
            for v0 in range(0, max(S, 1), seq_step):
                v1 = min(v0 + seq_step, S)
                a, b = int(seq_offsets[v0]), int(seq_offsets[v1])
                parts.append(_launch(dms, tables, np.ascontiguousarray(seq_offsets[v0:v1 + 1] - a), bases[a:b], keys[v0:v1],
                                     wts[v0:v1], K, seed, cut, forward_only, keep, order, walk_cap))
            for m in range(len(dms)):
                got = {name: np.concatenate([p[name][m] for p in parts], axis=0) for name in parts[0] if name != "rep_hits"}
                got["rep_hits"] = np.sum([p["rep_hits"][m] for p in parts], axis=0, dtype=np.uint64)
                got["cut"] = cut[m]
                results.append(got)
            offsets += offs
            numbers += nums
    return results, offsets, numbers


def null_sequences(motifs: Sequence, seq_offsets, bases, replicates: int, seed: int = 0, seq_keys=None, seq_weights=None, cuts=None,
                   weights: Optional[Sequence[np.ndarray]] = None, temperature: float = 1.0, forward_only: bool = False,
                   keep_replicates: bool = False, max_bytes: int = DEFAULT_MAX_BYTES, order: int = 1,
                   walk_cap: int = DEFAULT_WALK_CAP) -> List[Dict[str, np.ndarray]]:
    """The kernel on plain arrays: sequences (`seq_offsets` int64 [S + 1] from 0, `bases` uint8) for motifs of ONE width -> per
    motif a dict: obs_best int32 [S], obs_sum uint64 [S], ge_best and ge_sum uint32 [S], rep_hits uint64 [K], cut (the scaled
    score rep_hits counted at), and with `keep_replicates` the dense rep_best int32 [S, K] and rep_sum uint64 [S, K].
    `seq_keys` uint64 [S], default content_keys; `seq_weights` uint32 [S], default 1; `cuts`: a scaled score in [0, L] per motif,
    default L (no replicate reaches it).  `weights`: a uint64 table per motif, default haplotype_affinity.default_weights at
    `temperature`.  Motifs and sequences are taken in chunks whose device result tensors stay under `max_bytes` (rep_hits of
    sequence chunks are added on the host; the result does not depend on the chunks); one sequence of one motif above it is a
    ValueError that names it.  `order` 1: THE RULE; 2: THE RULE OF ORDER 2, doublet-preserving replicates, whose arborescence
    walks at most `walk_cap` x n steps (in [0, 1024]; 0 caps every replicate).  The library refuses motifs of two widths,
    replicates outside [1, 2^20], a cut outside [0, L] and weights that can overflow a sum."""
    seq_offsets, bases = _checked_sequences(seq_offsets, bases)
    return _null_chunked(motifs, seq_offsets, bases, replicates, seed, seq_keys, seq_weights, cuts, None, weights, temperature,
                         forward_only, keep_replicates, max_bytes, order, walk_cap)[0]


# ---------------------------------------------------------------------------------------------------------------- the table
class ShuffleNull:
    """The table of one motif over S sequences (see the module's docstring).
    Per sequence [S]: seq_region (the caller's region row), seq_version (the version's number in its region, -1: the region's
    reference sequence, which no haplotype spells), seq_count (haplotypes), seq_group_counts [S, G], seq_is_reference,
    seq_length -- as MutationScan's --, seq_weight (what the sequence counts for in rep_hits), and the kernel's obs_best int32,
    obs_sum uint64, ge_best and ge_sum uint32.  Per replicate [K]: rep_hits uint64, counted at the scaled score `cut`.
    `order`: 1 or 2, the rule the replicates were made by."""

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                 seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_length, seq_weight, replicates, seed,
                 obs_best, obs_sum, ge_best, ge_sum, rep_hits, cut, order=1):
        self.order = _checked_order(order)[0]
        self.motif_id, self.motif_alt_id = motif_id, motif_alt_id
        self.width, self.scale, self.offset = int(width), int(scale), float(offset)
        self.ptable, self.log2_offset, self.threshold = np.asarray(ptable, dtype=np.float64), float(log2_offset), float(threshold)
        self.region_names, self.group_names = np.asarray(region_names, dtype=object), list(group_names)
        self.seq_region, self.seq_version = np.asarray(seq_region, dtype=np.int64), np.asarray(seq_version, dtype=np.int64)
        self.seq_count = np.asarray(seq_count, dtype=np.int64)
        S = len(self.seq_count)
        self.seq_group_counts = np.asarray(seq_group_counts, dtype=np.int64).reshape(S, len(self.group_names))
        self.seq_is_reference = np.asarray(seq_is_reference, dtype=bool)
        self.seq_length, self.seq_weight = np.asarray(seq_length, dtype=np.int64), np.asarray(seq_weight, dtype=np.uint32)
        self.replicates, self.seed, self.cut = int(replicates), int(seed), int(cut)
        self.obs_best, self.obs_sum = np.asarray(obs_best, dtype=np.int32), np.asarray(obs_sum, dtype=np.uint64)
        self.ge_best, self.ge_sum = np.asarray(ge_best, dtype=np.uint32), np.asarray(ge_sum, dtype=np.uint32)
        self.rep_hits = np.asarray(rep_hits, dtype=np.uint64)
        if any(len(a) != S for a in (self.seq_region, self.seq_version, self.seq_is_reference, self.seq_length, self.seq_weight,
                                     self.obs_best, self.obs_sum, self.ge_best, self.ge_sum)) or self.rep_hits.shape != (self.replicates,):
            raise ValueError("the arrays do not fit the sequences and replicates")

    def __len__(self) -> int:
        return len(self.seq_count)

    def to_frame(self) -> pd.DataFrame:
        """a row per (region, version): motif_id, motif_alt_id, sequence_name, version (-1: the reference sequence, no haplotype
        spells it), haplotypes, one haplotypes_<GROUP> per group, is_reference, length, best_score, best_pvalue (the tail
        table's per-window value at the best score), best_null_pvalue = (1 + ge_best) / (K + 1), log2_affinity,
        affinity_null_pvalue = (1 + ge_sum) / (K + 1), replicates -- NaN where the sequence is shorter than the motif --, and
        under order 2 one more last column, null_order = 2.  The sequences by region, then version, the reference sequence
        last."""
        S = len(self)
        best = self.obs_best.astype(np.int64)
        some = self.seq_length >= self.width
        data = {"motif_id": np.full(S, self.motif_id, dtype=object), "motif_alt_id": np.full(S, self.motif_alt_id, dtype=object),
                "sequence_name": self.region_names[self.seq_region] if S else np.zeros(0, dtype=object),
                "version": self.seq_version, "haplotypes": self.seq_count}
        for g, name in enumerate(self.group_names):
            data[f"haplotypes_{name}"] = self.seq_group_counts[:, g]
        data["is_reference"] = self.seq_is_reference
        data["length"] = self.seq_length
        data["best_score"] = scaled_scores(best, self.scale, self.offset, self.width)
        data["best_pvalue"] = scaled_pvalues(best, self.ptable)
        data["best_null_pvalue"] = np.where(some, null_pvalues(self.ge_best, self.replicates), np.nan)
        filled = self.obs_sum > 0
        data["log2_affinity"] = np.where(filled, np.log2(np.where(filled, self.obs_sum, 1).astype(np.float64)) + self.log2_offset, np.nan)
        data["affinity_null_pvalue"] = np.where(some, null_pvalues(self.ge_sum, self.replicates), np.nan)
        data["replicates"] = np.full(S, self.replicates, dtype=np.int64)
        if self.order != 1:
            data["null_order"] = np.full(S, self.order, dtype=np.int64)
        return pd.DataFrame(data)


def enrichment_frame(tables: Sequence[ShuffleNull]) -> pd.DataFrame:
    """One row per motif for the whole call, in the motifs' order: motif_id, motif_alt_id, width, regions (the sequences that
    count), observed_hits = the seq_weight of the sequences whose own best score reaches the cut, null_mean_hits and
    null_max_hits over the replicates' rep_hits, enrichment_pvalue = (1 + #{r : rep_hits[r] >= observed_hits}) / (K + 1),
    replicates -- and one more last column, null_order = 2, when the tables are of order 2.
    compute_shuffle_null_many gives seq_weight 1 to each region's version 0, its most frequent spelled sequence, and 0 to every
    other: a region is ONE draw.  The versions of a region are nearly the same sequence, and independent shuffles of each would
    be counted as independent regions -- the pooled count's variance would be understated and the p-value too small.
    The cut is the smallest scaled score whose tail-table value is < threshold, the report's strict rule, L if there is none."""
    rows = []
    for t in tables:
        w = t.seq_weight.astype(np.int64)
        observed = int(w[t.obs_best.astype(np.int64) >= t.cut].sum())
        hits = t.rep_hits.astype(np.float64)
        rows.append((t.motif_id, t.motif_alt_id, t.width, int((w > 0).sum()), observed, float(hits.mean()), int(t.rep_hits.max()),
                     float(null_pvalues(int((t.rep_hits >= np.uint64(observed)).sum()), t.replicates)), t.replicates))
    frame = pd.DataFrame(rows, columns=ENRICHMENT_COLUMNS).astype({"width": np.int64, "regions": np.int64, "observed_hits": np.int64,
                                                                   "null_mean_hits": np.float64, "null_max_hits": np.int64,
                                                                   "enrichment_pvalue": np.float64, "replicates": np.int64})
    if any(t.order != 1 for t in tables):
        frame["null_order"] = np.array([t.order for t in tables], dtype=np.int64)
    return frame


def compute_shuffle_null_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                              haplotype_groups: Optional[Mapping] = None, weights: Optional[Sequence[np.ndarray]] = None,
                              temperature: float = 1.0, threshold: Optional[float] = None, replicates: int = DEFAULT_REPLICATES,
                              seed: int = 0, max_bytes: int = DEFAULT_MAX_BYTES, order: int = 1) -> List[ShuffleNull]:
    """One ShuffleNull per motif, in the order of `motifs` (see the module's docstring).  The arguments and the sequences are
    compute_mutation_scan_many's: the versions of compute_haplotype_sequences(coordinates=True), the reference sequence of a
    region added with count 0 where no version is the reference's; one kernel call per motif width (in chunks under
    `max_bytes`).  The keys are content_keys; seq_weight is 1 for each region's version 0 and 0 elsewhere (enrichment_frame says
    why); the cut is pvalue_cut at the threshold.  args_obj: noreverse and threshold (`threshold` overrides it).
    `temperature` / `weights` as compute_haplotype_affinity_many's.  `order`: 1, or 2 for doublet-preserving replicates."""
    if not 1 <= int(replicates) <= MAX_REPLICATES:
        raise ValueError(f"replicates {replicates}: outside [1, {MAX_REPLICATES}]")
    order = _checked_order(order)[0]
    seqs, region_names, group_names, forward_only, threshold = scan_inputs(
        "the shuffle null", motifs, graph, regions, debug, args_obj, chrom_names, haplotype_groups, weights, None, threshold)
    seq_offsets, bases = seqs[5], seqs[6]
    seq_weight = (np.asarray(seqs[1]) == 0).astype(np.uint32)
    keys = content_keys(seq_offsets, bases)
    return tables_by_width(
        motifs, weights,
        lambda ms, ws: _null_chunked(ms, seq_offsets, bases, replicates, seed, keys, seq_weight, None, threshold, ws, temperature,
                                     forward_only, False, max_bytes, order),
        lambda motif, W, numbers, log2_offset, g: ShuffleNull(
            motif.motif_id, motif.motif_name, W, *numbers, log2_offset, threshold, region_names, group_names, *seqs[:5],
            np.diff(seq_offsets), seq_weight, replicates, seed, g["obs_best"], g["obs_sum"], g["ge_best"], g["ge_sum"], g["rep_hits"],
            g["cut"], order))


def compute_shuffle_null(motif, graph, regions, debug: bool, args_obj, chrom_names=None, haplotype_groups: Optional[Mapping] = None,
                         weights: Optional[np.ndarray] = None, temperature: float = 1.0, threshold: Optional[float] = None,
                         replicates: int = DEFAULT_REPLICATES, seed: int = 0, max_bytes: int = DEFAULT_MAX_BYTES,
                         order: int = 1) -> ShuffleNull:
    """The shuffle null of `motif` (compute_shuffle_null_many for one motif)"""
    return compute_shuffle_null_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_groups,
                                     None if weights is None else [weights], temperature, threshold, replicates, seed, max_bytes,
                                     order)[0]


# ---------------------------------------------------------------------------------------------------------------- the writers
def write_shuffle_null(table: ShuffleNull, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_shuffle_null.tsv (grafimo_shuffle_null_<motif_id>.tsv for one of several motifs), a row per (region, version),
    in the directory write_results uses for this motif -> the path written.  `out`: a text stream to write to instead (-f)."""
    return write_frame(table.to_frame(), out if out is not None else table_path(TABLE_FILE, args_obj, motif, motif_num))


def write_motif_enrichment(tables: Sequence[ShuffleNull], args_obj, out=None) -> Optional[str]:
    """grafimo_motif_enrichment.tsv, a row per motif of the call (enrichment_frame) -> the path written"""
    return write_frame(enrichment_frame(tables), out if out is not None else table_path(ENRICHMENT_FILE, args_obj, tag="enrichment"))


def print_shuffle_null(table: ShuffleNull) -> None:
    """-f: the rows of one motif on stdout instead of a file"""
    write_shuffle_null(table, None, 1, None, out=sys.stdout)


def print_motif_enrichment(tables: Sequence[ShuffleNull]) -> None:
    """-f: the enrichment rows on stdout instead of a file"""
    write_motif_enrichment(tables, None, out=sys.stdout)
