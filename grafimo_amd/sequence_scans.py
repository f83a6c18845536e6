"""What the sequence scans share: mutation_scan, indel_scan, deletion_scan, substitution_scan, insertion_scan and site_distance, and
the shuffle null where it scans the same sequences.  Each of those modules keeps its own RULE, its cells and its frames' own
columns; here is what was the same in all of them:
  the sequences   the checked plain arrays (_checked_sequences), the versions of a region with its reference sequence
                  (_with_references), and the prologue of every compute_*_many (scan_inputs);
  the kernel      the staging and the call of an entry that writes keys and sums (stage, enqueue, scan -- the probes time the
                  first two apart), the motifs leased in chunks under max_bytes (_leased_chunks, chunk_step, scan_chunked), and
                  the loop over the motif widths that makes a table per motif (tables_by_width);
  the tables      SequenceTable (the per-sequence and per-base arrays, the frames' leading columns, the printed windows) and
                  ScanTable (keys and sums of a REF and an ALT side: the filter, the ref_ / alt_ columns, the summary's group-by);
  the writers     table_writers: a module's write_X, write_X_summary and print_X from its two file names.
"""
import contextlib
import ctypes
import sys
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _stream_ptr, _torch
from .graph_tables import (_haplotype_set, _matrix_rows, group_by_width, prepare_graphs, require_single_gpu, scaled_pvalues,
                           scaled_scores, table_path, write_frame)
from .query_variants import EFFECTS, _weight_tables, decode_keys

TO_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
DEFAULT_MAX_BYTES = 1 << 31
_UPPER = np.arange(256, dtype=np.uint8)
_UPPER[ord("a"):ord("z") + 1] -= 32
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMP[_a] = _b
_COLUMN_OF = np.zeros(256, dtype=np.int64)               # the column of a base, 0: it is none of A, C, G, T
for _k, _c in enumerate(b"ACGT"):
    _COLUMN_OF[_c] = _COLUMN_OF[_c + 32] = _k + 1
_LETTERS = np.array([chr(k) for k in range(256)], dtype=object)


# ---------------------------------------------------------------------------------------------------------------- the sequences
def _checked_sequences(seq_offsets, bases) -> Tuple[np.ndarray, np.ndarray]:
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    if seq_offsets.ndim != 1 or len(seq_offsets) < 1 or seq_offsets[0] != 0:
        raise ValueError("seq_offsets is int64 [n_seqs + 1] and starts at 0")
    if int(seq_offsets[-1]) != len(bases):
        raise ValueError(f"seq_offsets ends at {int(seq_offsets[-1])}, bases holds {len(bases)}")
    return seq_offsets, bases


def _within(seq_offsets: np.ndarray, N: int):
    """-> (the offset of every base in its sequence, the bases behind and including it) int64 [N]"""
    n = np.diff(seq_offsets)
    within = np.arange(N, dtype=np.int64) - np.repeat(seq_offsets[:-1], n)
    return within, np.repeat(n, n) - within


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


def scan_inputs(what: str, motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names, haplotype_groups, weights, delta,
                threshold):
    """The prologue of every compute_*_many (`what`: "the mutation scan", as the messages name the table): the arguments checked,
    the versions of compute_haplotype_sequences(coordinates=True) with the reference sequence of a region added where no version
    is the reference's -> (seqs: _with_references' eight arrays, seq_offsets and bases contiguous; region_names; group_names;
    forward_only; threshold).  args_obj: noreverse and threshold (`threshold` overrides it)."""
    from .haplotype_classes import compute_haplotype_classes
    from .haplotype_sequences import compute_haplotype_sequences
    require_single_gpu(what, "is", "a gather of the sharded class matrices")
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    if delta is not None and not float(delta) >= 0:
        raise ValueError(f"delta {delta}: it must be >= 0")
    prep = prepare_graphs(graph, regions, chrom_names)
    _haplotype_set(prep, None, what)
    rows, region_names = _matrix_rows(prep)
    hc = compute_haplotype_classes(graph, regions, debug, args_obj, chrom_names, None, haplotype_groups)
    hs = compute_haplotype_sequences(graph, regions, debug, args_obj, chrom_names, None, None, classes=hc, coordinates=True)
    seqs = _with_references(hs, prep, rows)
    seqs = seqs[:5] + (np.ascontiguousarray(seqs[5]), np.ascontiguousarray(seqs[6]), seqs[7])
    return (seqs, region_names, hs.group_names, bool(getattr(args_obj, "noreverse", False)),
            float(args_obj.threshold if threshold is None else threshold))


# ---------------------------------------------------------------------------------------------------------------- the kernel
def stage(tables, seq_offsets: np.ndarray, bases: np.ndarray, shape: Tuple[int, ...]):
    """the inputs of an entry that writes keys and sums on the current device and its result tensors -> (seq_offsets (host), the
    bases' tensor, the weight tables' tensors, the largest weight, keys int32 [M, *shape], sums int64 [M, *shape], the status
    word).  `shape`: a motif's results, (n_bases, columns) or (n_lengths, n_bases, 2)."""
    torch = _torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    d_bases = torch.from_numpy(np.array(bases, dtype=np.uint8)).to(dev)             # (a copy: the caller's may be read-only)
    d_tabs = [torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64)).to(dev) for t in tables]
    full = (len(tables),) + tuple(shape)
    return (seq_offsets, d_bases, d_tabs, max(int(t.max()) for t in tables), torch.empty(full, dtype=torch.int32, device=dev),
            torch.empty(full, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))


def enqueue(dms, staged, forward_only: bool, entry: str, extra: Sequence = ()):
    """`entry` over staged inputs (stage): every row of the result tensors is written -> (keys, sums).  `extra`: the entry's own
    arguments between d_bases and flags (the block scans' lengths and map)."""
    seq_offsets, d_bases, d_tabs, max_weight, keys, sums, status = staged
    M = len(dms)
    vp = ctypes.c_void_p
    nv.check(getattr(nv.lib(), entry)(
        (vp * M)(*[x.handle for x in dms]), M, (vp * M)(*[t.data_ptr() for t in d_tabs]), max_weight, len(seq_offsets) - 1,
        seq_offsets.ctypes.data, d_bases.data_ptr(), *extra, nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0,
        (vp * M)(*[keys[m].data_ptr() for m in range(M)]), (vp * M)(*[sums[m].data_ptr() for m in range(M)]),
        status.data_ptr(), _stream_ptr(None)))
    return keys, sums


def scan(dms, tables, seq_offsets: np.ndarray, bases: np.ndarray, forward_only: bool, entry: str, shape: Tuple[int, ...],
         extra: Sequence = ()):
    """`entry` for leased motifs of one width -> (keys uint32 [M, *shape], sums uint64 [M, *shape]) on the host"""
    if int(seq_offsets[-1]) == 0:
        return np.zeros((len(dms),) + tuple(shape), dtype=np.uint32), np.zeros((len(dms),) + tuple(shape), dtype=np.uint64)
    keys, sums = enqueue(dms, stage(tables, seq_offsets, bases, shape), forward_only, entry, extra)
    return keys.cpu().numpy().view(np.uint32), sums.cpu().numpy().view(np.uint64)


def _leased_chunks(motifs: Sequence, weights, temperature, step: int):
    """The motifs `step` at a time, leased for as long as the caller holds the item -> (m0, the leased handles, their weight
    tables, their log2 offsets, per motif (scale, offset, ptable)) per chunk; the handles are given back when the caller asks
    for the next chunk, or fails.  What the sequence tables' chunked calls share (scan_chunked, shuffle_null)."""
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


def chunk_step(motifs: Sequence, n_bases: int, per_motif: int, max_bytes: int, what: str = "keys and sums", over: str = "",
               fewer: str = "") -> int:
    """how many motifs a chunk takes so that its result tensors (`per_motif` bytes each) stay under max_bytes; a single motif
    above it is a ValueError that names it.  `over` / `fewer`: what a block scan's message adds (" and K lengths", " or lengths")."""
    if per_motif > int(max_bytes):
        raise ValueError(f"{motifs[0].motif_id}: the {what} of one motif over {n_bases} bases{over} hold {per_motif} "
                         f"bytes, more than max_bytes = {int(max_bytes)}: scan fewer sequences{fewer} at a time, or raise max_bytes")
    return max(1, int(max_bytes) // max(per_motif, 1))


def scan_chunked(motifs: Sequence, seq_offsets, bases, weights, temperature, forward_only, max_bytes, entry: str,
                 shape: Tuple[int, ...], extra: Sequence = (), over: str = "", fewer: str = ""):
    """-> (per motif (keys, sums), per motif its log2 offset, per motif (scale, offset, ptable)): the motifs leased and scanned
    in chunks whose result tensors (12 bytes a key and sum) stay under max_bytes"""
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    step = chunk_step(motifs, int(seq_offsets[-1]), (4 + 8) * int(np.prod(shape, dtype=np.int64)), max_bytes, over=over, fewer=fewer)
    results, offsets, numbers = [], [], []
    with contextlib.closing(_leased_chunks(motifs, weights, temperature, step)) as chunks:     # (a failure gives the handles back)
        for _, dms, tables, offs, nums in chunks:
            keys, sums = scan(dms, tables, seq_offsets, bases, forward_only, entry, shape, extra)
            results += [(keys[m], sums[m]) for m in range(len(dms))]
            offsets += offs
            numbers += nums
    return results, offsets, numbers


def tables_by_width(motifs: Sequence, weights, scan_width: Callable, make: Callable) -> List:
    """The epilogue of every compute_*_many: one chunked kernel call per motif width -> a table per motif, in the order of
    `motifs`.  scan_width(the motifs of a width, their weights or None) -> (results, offsets, numbers) per motif, as scan_chunked
    gives them; make(motif, W, (scale, offset, ptable), its offset, its result) -> the table."""
    out: List = [None] * len(motifs)
    for W, idxs in group_by_width(motifs).items():
        got, offsets, numbers = scan_width([motifs[i] for i in idxs], None if weights is None else [weights[i] for i in idxs])
        for m, i in enumerate(idxs):
            out[i] = make(motifs[i], W, numbers[m], offsets[m], got[m])
    return out


# ---------------------------------------------------------------------------------------------------------------- the filter
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


# ---------------------------------------------------------------------------------------------------------------- the tables
def fixed_text(text: np.ndarray) -> np.ndarray:
    """uint8 [rows, width] -> object [rows]: each row as a string (a fixed-width byte string drops its trailing zeros)"""
    width = text.shape[1]
    return np.ascontiguousarray(text).view(f"S{width}").reshape(-1).astype(f"U{width}").astype(object)


def printed_windows(text: np.ndarray, minus: np.ndarray) -> np.ndarray:
    """uint8 [rows, W] forward windows -> object [rows] as printed: the rows of `minus` reverse complemented (`text` is changed)"""
    text[minus] = _COMP[text[minus]][:, ::-1]
    return fixed_text(text)


class SequenceTable:
    """What the tables over S sequences of N bases in all share.
    Per sequence [S]: seq_region (the caller's region row), seq_version (the version's number in its region, -1: the region's
    reference sequence, which no haplotype spells), seq_count (haplotypes), seq_group_counts [S, G], seq_is_reference,
    seq_offsets int64 [S + 1].  Per base [N]: bases uint8, coord int32 (~coordinate for an inserted base)."""

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, threshold, region_names, group_names, seq_region,
                 seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, all_rows=False):
        self.motif_id, self.motif_alt_id = motif_id, motif_alt_id
        self.width, self.scale, self.offset = int(width), int(scale), float(offset)
        self.ptable, self.threshold = np.asarray(ptable, dtype=np.float64), float(threshold)
        self.region_names, self.group_names = np.asarray(region_names, dtype=object), list(group_names)
        self.seq_region, self.seq_version = np.asarray(seq_region, dtype=np.int64), np.asarray(seq_version, dtype=np.int64)
        self.seq_count = np.asarray(seq_count, dtype=np.int64)
        self.seq_group_counts = np.asarray(seq_group_counts, dtype=np.int64).reshape(len(self.seq_count), len(self.group_names))
        self.seq_is_reference = np.asarray(seq_is_reference, dtype=bool)
        self.seq_offsets = np.asarray(seq_offsets, dtype=np.int64)
        self.bases, self.coord = np.asarray(bases, dtype=np.uint8), np.asarray(coord, dtype=np.int32)
        self.all_rows = bool(all_rows)

    def _fits(self, *arrays_and_shapes) -> bool:
        """coord and seq_offsets fit the N bases, and every (array, shape) pair given"""
        N = len(self.bases)
        return len(self.coord) == N and int(self.seq_offsets[-1]) == N and all(a.shape == s for a, s in arrays_and_shapes)

    @property
    def base_sequence(self) -> np.ndarray:
        """int64 [N]: the sequence of every base"""
        return np.repeat(np.arange(len(self.seq_count), dtype=np.int64), np.diff(self.seq_offsets))

    def _sequence_of(self, n) -> np.ndarray:
        return self.base_sequence[n] if len(n) else np.zeros(0, dtype=np.int64)

    def _motif_columns(self, rows: int, region) -> dict:
        """the columns every frame starts with: motif_id, motif_alt_id, sequence_name (of the region rows `region`)"""
        return {"motif_id": np.full(rows, self.motif_id, dtype=object), "motif_alt_id": np.full(rows, self.motif_alt_id, dtype=object),
                "sequence_name": self.region_names[region] if rows else np.zeros(0, dtype=object)}

    def _leading_columns(self, n) -> dict:
        """the detail rows' leading columns for the bases n: motif_id, motif_alt_id, sequence_name, version, haplotypes, one
        haplotypes_<GROUP> per group, is_reference, position (1-based; an inserted base has its anchor's), inserted"""
        seq = self._sequence_of(n)
        data = self._motif_columns(len(n), self.seq_region[seq])
        data["version"], data["haplotypes"] = self.seq_version[seq], self.seq_count[seq]
        for g, name in enumerate(self.group_names):
            data[f"haplotypes_{name}"] = self.seq_group_counts[seq, g]
        data["is_reference"] = self.seq_is_reference[seq]
        co = self.coord[n].astype(np.int64)
        data["position"] = np.where(co < 0, ~co, co) + 1
        data["inserted"] = co < 0
        return data


class ScanTable(SequenceTable):
    """A SequenceTable with the dense arrays keys uint32 and sums uint64 of one shape, whose cells compare an ALT side with a
    REF side.  A subclass names its cells as a pair of index arrays (n, c) and says where their two sides lie (_sides), which
    cells exist (_cells), what its arrays' shape is (_shape) and how a side's best window reads (_kmers)."""

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, region_names, group_names,
                 seq_region, seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, keys, sums,
                 delta=None, all_rows=False):
        super().__init__(motif_id, motif_alt_id, width, scale, offset, ptable, threshold, region_names, group_names, seq_region,
                         seq_version, seq_count, seq_group_counts, seq_is_reference, seq_offsets, bases, coord, all_rows)
        self.log2_offset = float(log2_offset)
        self.keys, self.sums = np.asarray(keys, dtype=np.uint32), np.asarray(sums, dtype=np.uint64)
        shape, what = self._shape()
        if not self._fits((self.keys, shape), (self.sums, shape)):
            raise ValueError(f"the arrays do not fit {what}")
        self.delta = None if delta is None else float(delta)

    def _shape(self):
        """-> (the shape of keys and of sums, what they must fit, for the message): [N, the module's COLUMNS]"""
        return (len(self.bases), len(self.COLUMNS)), "the sequences"

    def __len__(self) -> int:
        return int(self._kept_cells()[0].size)

    def log2_affinity(self) -> np.ndarray:
        """float64, the shape of sums: log2(sum) + log2_offset, NaN where the side has no window"""
        out = np.full(self.sums.shape, np.nan)
        some = self.sums > 0
        out[some] = np.log2(self.sums[some].astype(np.float64)) + self.log2_offset
        return out

    def _numbers(self, n, c):
        """of the cells (n, c) -> (ref best, alt best (int64, -1: none), ref p, alt p, ref log2, alt log2)"""
        ref, alt = self._sides(n, c)
        rb, ab = decode_keys(self.keys[ref])[0], decode_keys(self.keys[alt])[0]
        la = lambda s: np.where(s > 0, np.log2(np.where(s > 0, s, 1).astype(np.float64)) + self.log2_offset, np.nan)   # noqa: E731
        return rb, ab, scaled_pvalues(rb, self.ptable), scaled_pvalues(ab, self.ptable), la(self.sums[ref]), la(self.sums[alt])

    def _kept_cells(self):
        n, c = self._cells()
        rb, ab, rp, ap, rl, al = self._numbers(n, c)
        keep = keep_rows(effect_codes(rp, ap, self.threshold), al - rl, self.delta, self.all_rows)
        return n[keep], c[keep]

    def _detail_frame(self, n, c, data: dict) -> pd.DataFrame:
        """`data` (the leading and the table's own columns of the cells (n, c)) with the columns every detail frame ends with:
        ref_score, ref_pvalue, ref_start, ref_strand, ref_kmer, alt_score .. alt_kmer, ref_log2_affinity, alt_log2_affinity,
        delta_log2_affinity, effect"""
        rb, ab, rp, ap, rl, al = self._numbers(n, c)
        for side, best, p, at in zip(("ref", "alt"), (rb, ab), (rp, ap), self._sides(n, c)):
            _, rel, strand = decode_keys(self.keys[at])
            data[f"{side}_score"] = scaled_scores(best, self.scale, self.offset, self.width)
            data[f"{side}_pvalue"] = p
            data[f"{side}_start"] = np.where(best >= 0, rel.astype(np.float64), np.nan)
            data[f"{side}_strand"] = strand
            data[f"{side}_kmer"] = self._kmers(n, c, side)
        data["ref_log2_affinity"], data["alt_log2_affinity"], data["delta_log2_affinity"] = rl, al, al - rl
        data["effect"] = EFFECTS[effect_codes(rp, ap, self.threshold)]
        return pd.DataFrame(data)

    def _summary_frame(self, n, c, seq, group_keys: Sequence[np.ndarray], own_columns: Callable) -> pd.DataFrame:
        """The summary over the cells (n, c) of the sequences seq: a row per (region, coordinate, *group_keys) with motif_id,
        motif_alt_id, sequence_name, position, the table's own columns (own_columns(f): of the groups' first cells f), versions,
        haplotypes, haplotypes_gain, haplotypes_loss, min_delta_log2_affinity, max_delta_log2_affinity, best_alt_score.  A row
        is kept when some haplotype gains or loses, or when a delta is given and the smallest or largest delta reaches it;
        all_rows keeps everything."""
        rb, ab, rp, ap, rl, al = self._numbers(n, c)
        codes = effect_codes(rp, ap, self.threshold)
        region = self.seq_region[seq]
        first, versions, haps, gain, loss, lo, hi, best = group_summary((region, self.coord[n].astype(np.int64), *group_keys),
                                                                        self.seq_count[seq], codes, al - rl, ab)
        keep = np.ones(len(first), dtype=bool) if self.all_rows else (gain + loss) > 0
        if self.delta is not None and not self.all_rows:
            with np.errstate(invalid="ignore"):
                keep |= (np.abs(lo) >= self.delta) | (np.abs(hi) >= self.delta)
        k = np.flatnonzero(keep)
        f = first[k]
        data = self._motif_columns(len(k), region[f])
        data["position"] = self.coord[n[f]].astype(np.int64) + 1
        data.update(own_columns(f))
        data.update({"versions": versions[k], "haplotypes": haps[k], "haplotypes_gain": gain[k], "haplotypes_loss": loss[k],
                     "min_delta_log2_affinity": lo[k], "max_delta_log2_affinity": hi[k],
                     "best_alt_score": scaled_scores(best[k], self.scale, self.offset, self.width)})
        return pd.DataFrame(data)


# ---------------------------------------------------------------------------------------------------------------- the writers
def table_writers(detail_file: str, summary_file: str):
    """-> (write, write_summary, show) of a module whose tables have to_frame() and summary_frame(): the detail rows in
    <detail_file>.tsv and the summary in <summary_file>.tsv, each with _<motif_id> for one of several motifs, in the directory
    write_results uses for the motif; show prints both on stdout (-f)."""
    def write(table, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
        return write_frame(table.to_frame(), out if out is not None else table_path(detail_file, args_obj, motif, motif_num))

    def write_summary(table, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
        return write_frame(table.summary_frame(), out if out is not None else table_path(summary_file, args_obj, motif, motif_num))

    def show(table) -> None:
        write(table, None, 1, None, out=sys.stdout)
        write_summary(table, None, 1, None, out=sys.stdout)

    write.__doc__ = (f"{detail_file}.tsv ({detail_file}_<motif_id>.tsv for one of several motifs), the detail rows, in the directory "
                     "write_results uses for this motif -> the path written.  `out`: a text stream to write to instead (-f: stdout).")
    write_summary.__doc__ = f"{summary_file}[_<motif_id>].tsv, the summary rows, beside the detail rows"
    show.__doc__ = "-f: the detail rows, then the summary, on stdout instead of files"
    return write, write_summary, show
