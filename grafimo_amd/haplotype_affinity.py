"""Per-haplotype total binding affinity: for every region and every haplotype of the graph, the sum over EVERY k-mer of the
haplotype's own sequence in the region of 2^(log-odds / T) -- the number occupancy models of TF binding regress on (TRAP-style
total affinity, motif-score QTL, allele-specific binding).  Where haplotype_scores gives the single best k-mer, the sum also
moves when a variant weakens the second-best site of a cluster or an indel adds or removes windows.

Rows(r, h) are haplotype_scores' rows: the windows of W consecutive bases of h's spelled sequence under the report's region
rule, on both strands unless --no-reverse, each window once per strand.  The device sums INTEGERS: with a weight table
w uint64 [L] over the motif's scaled scores, A(r, h) = sum over Rows(r, h) of w[score(row)], exact in uint64 -- bit for bit
what a brute force gives, whatever the run / block decomposition and the order of the atomics.  A k-mer holding N scores
min_val.  The reference column is the same over the graph's reference path.  -t, -q, --qvalueT and --recomb change nothing.

The default table (default_weights) is fixed-point with F = 40 fraction bits, anchored at the best score the motif can reach,
s_best = the sum of the scaled matrix's column maxima:  w[s] = max(1, rint(2^F * 2^((min(s, s_best) - s_best) / (scale T)))),
T > 0 the temperature.  Every weight is >= 1, so A == 0 exactly where the haplotype has no row in the region.  The 40-bit
FLOOR: a k-mer 40 T bits or more of log-odds below the optimum counts as 2^-40 of it, not less.  Reported is
log2_affinity = log2(A) - F + (s_best / scale + W offset) / T, float64, NaN where A == 0: the log2 of the sum of
2^(log-odds / T), a soft maximum on the scale of haplotype_scores' best_score (divided by T).  With the caller's own tables
(`weights=`) log2_affinity is the plain log2(A).

The hot path is HIP (grafimo_amd/csrc/gfm_graph_hapaffinity.hpp, gfm_graph_haplotype_affinity).
"""
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _stream_ptr, _torch
from .graph_tables import (META_COLUMNS, _haplotype_set, _matrix_rows, group_by_width, prepare_graphs, require_single_gpu,
                           table_path, text_table, write_wide)

COLUMNS_HEAD = META_COLUMNS + ["reference"]
FRACTION_BITS = 40


def default_weights(motif, temperature: float = 1.0) -> Tuple[np.ndarray, int]:
    """The fixed-point table of a motif (a Motif, or a DeviceMotif: score_matrix [4, W] scaled, scale) at temperature T
    -> (w uint64 [L], s_best): w[s] = max(1, rint(2^40 * 2^((min(s, s_best) - s_best) / (scale * T)))), s_best the best score
    the motif can reach (NOT L - 1, which no k-mer reaches: anchoring there would throw away tens of bits of range)."""
    from .device import DeviceMotif
    from .motif import dense_score_matrix
    T = float(temperature)
    if not T > 0:
        raise ValueError(f"temperature {temperature}: it must be > 0")
    sm = motif.score_matrix if isinstance(motif, DeviceMotif) else dense_score_matrix(motif)
    sm = np.asarray(sm, dtype=np.int64)
    W = sm.shape[1]
    L = nv.RANGE * W + 1
    s_best = int(sm.max(axis=0).sum())
    s = np.minimum(np.arange(L, dtype=np.int64), s_best)
    w = np.rint(np.exp2(FRACTION_BITS + (s - s_best).astype(np.float64) / (float(motif.scale) * T)))
    return np.maximum(w, 1.0).astype(np.uint64), s_best


class HaplotypeAffinity:
    """The matrix of one motif: region_names [R], haplotype_names [H], sums uint64 [R, H] and reference_sum [R]; made on
    first use: log2_affinity float64 [R, H] and reference_log2_affinity [R] = log2(sum) + log2_offset, NaN where the sum is
    0.  log2_offset: -40 + (s_best / scale + W offset) / T for the default weights, 0 for the caller's own."""

    def __init__(self, motif_id: str, motif_alt_id: str, region_names, haplotype_names, sums: np.ndarray,
                 log2_offset: float = 0.0):
        self.motif_id, self.motif_alt_id = motif_id, motif_alt_id
        self.region_names = np.asarray(region_names, dtype=object)
        self.haplotype_names = list(haplotype_names)
        self.full = np.ascontiguousarray(sums, dtype=np.uint64)            # [R, H + 1], column H the reference
        self.log2_offset = float(log2_offset)
        H = len(self.haplotype_names)
        if self.full.shape != (len(self.region_names), H + 1):
            raise ValueError(f"sums of shape {self.full.shape} for {len(self.region_names)} regions and {H} haplotypes")
        self.sums, self.reference_sum = self.full[:, :H], self.full[:, H]
        self._cells = None

    def _by_sum(self):
        """-> (the distinct sums ascending, their log2 affinity (NaN for 0), per cell of `full` the index of its sum): a
        value is made once per DISTINCT sum, the frame and the writer share it"""
        if self._cells is None:
            vals = np.unique(self.full)
            lv = np.full(len(vals), np.nan)
            lv[vals > 0] = np.log2(vals[vals > 0].astype(np.float64)) + self.log2_offset
            self._cells = (vals, lv, np.searchsorted(vals, self.full))
        return self._cells

    def _log2(self):
        _, lv, codes = self._by_sum()
        return lv[codes]

    log2_affinity = property(lambda self: self._log2()[:, :-1])
    reference_log2_affinity = property(lambda self: self._log2()[:, -1])

    def to_frame(self) -> pd.DataFrame:
        """the wide table of the TSV: motif_id, motif_alt_id, sequence_name, reference, then one column per haplotype, each
        cell the log2 affinity (NaN where the haplotype has no row)"""
        R = len(self.region_names)
        full = self._log2()
        meta = pd.DataFrame({"motif_id": np.full(R, self.motif_id, dtype=object),
                             "motif_alt_id": np.full(R, self.motif_alt_id, dtype=object), "sequence_name": self.region_names,
                             "reference": full[:, -1]})
        return pd.concat([meta, pd.DataFrame(full[:, :-1], columns=self.haplotype_names)], axis=1)


def _scan(dg, starts: np.ndarray, stops: np.ndarray, dms, tables, forward_only: bool, H: int, windows_per_run: int,
          haplotypes_per_block: int) -> List[np.ndarray]:
    """gfm_graph_haplotype_affinity over one graph for motifs of one width -> per motif the sums uint64 [n, H + 1]"""
    import ctypes
    torch = _torch()
    M, n = len(dms), len(starts)
    vp = ctypes.c_void_p
    with torch.cuda.device(dg.device):
        sums = torch.zeros((M, n, H + 1), dtype=torch.int64, device=dg.device)
        over = torch.zeros(1, dtype=torch.int32, device=dg.device)
        d_tabs = [torch.from_numpy(t.view(np.int64)).to(dg.device) for t in tables]
        handles = (vp * M)(*[d.handle for d in dms])
        tabs_p = (vp * M)(*[t.data_ptr() for t in d_tabs])
        sums_p = (vp * M)(*[sums[m].data_ptr() for m in range(M)])
        nv.check(nv.lib().gfm_graph_haplotype_affinity(
            dg._h, handles, M, tabs_p, max(int(t.max()) for t in tables), n, nv.ptr(starts) if n else None,
            nv.ptr(stops) if n else None, nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0, sums_p, over.data_ptr(),
            int(windows_per_run), int(haplotypes_per_block), _stream_ptr(None)))
        if int(over.item()):
            raise OverflowError(f"{dg.index.chrom}: a window holds more than 2^24 walks: the per-haplotype affinities would be "
                                "incomplete (scan regions without it)")
        host = sums.cpu().numpy().view(np.uint64)
    return [host[m] for m in range(M)]


def compute_haplotype_affinity_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                                    haplotype_names: Optional[Sequence[str]] = None, temperature: float = 1.0,
                                    weights: Optional[Sequence[np.ndarray]] = None, windows_per_run: int = 0,
                                    haplotypes_per_block: int = 0) -> List[HaplotypeAffinity]:
    """compute_haplotype_affinity for every motif of a set -> one HaplotypeAffinity per motif, in the order of `motifs`.  The
    motifs of one width share one run list and one call.  `weights`: one uint64 [L] table per motif instead of
    default_weights(motif, temperature).  `windows_per_run` / `haplotypes_per_block` cut the device work (0: the library's
    defaults); the result does not depend on them."""
    from .device import DeviceMotif
    require_single_gpu("the per-haplotype affinities", "are", "a gather of the sharded matrices")
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    prep = prepare_graphs(graph, regions, chrom_names)
    H, names = _haplotype_set(prep, haplotype_names, "the per-haplotype affinity matrix")
    rows, region_names = _matrix_rows(prep)
    R = len(region_names)
    forward_only = bool(getattr(args_obj, "noreverse", False))
    out: List[Optional[HaplotypeAffinity]] = [None] * len(motifs)
    for W, idxs in group_by_width(motifs).items():
        dms = [DeviceMotif.lease(motifs[i]) for i in idxs]
        try:
            tables, offsets = [], []
            for dm, i in zip(dms, idxs):
                if weights is None:
                    w, s_best = default_weights(dm, temperature)
                    offsets.append(-FRACTION_BITS + (s_best / dm.scale + W * dm.offset) / float(temperature))
                else:
                    w = np.ascontiguousarray(weights[i], dtype=np.uint64)
                    if w.shape != (dm.L,):
                        raise ValueError(f"{motifs[i].motif_id}: a weight table of shape {w.shape}, the motif's scores need "
                                         f"({dm.L},)")
                    offsets.append(0.0)
                tables.append(w)
            one = len(prep.graphs) == 1 and np.array_equal(rows[0], np.arange(R))
            sums = None if one else [np.zeros((R, H + 1), dtype=np.uint64) for _ in idxs]
            for gi, g in enumerate(prep.graphs):
                starts = np.ascontiguousarray(prep.spans[gi][0], dtype=np.int64)
                stops = np.ascontiguousarray(prep.spans[gi][1], dtype=np.int64)
                got = _scan(g, starts, stops, dms, tables, forward_only, H, windows_per_run, haplotypes_per_block)
                if one:
                    sums = got
                    continue
                for m in range(len(idxs)):
                    sums[m][rows[gi]] = got[m]
            for m, i in enumerate(idxs):
                out[i] = HaplotypeAffinity(motifs[i].motif_id, motifs[i].motif_name, region_names, names, sums[m], offsets[m])
        finally:
            for dm in dms:
                dm.release()
    return out


def compute_haplotype_affinity(motif, graph, regions, debug: bool, args_obj, chrom_names=None,
                               haplotype_names: Optional[Sequence[str]] = None, temperature: float = 1.0,
                               weights: Optional[np.ndarray] = None, windows_per_run: int = 0,
                               haplotypes_per_block: int = 0) -> HaplotypeAffinity:
    """The per-haplotype affinity matrix of `motif` (see the module's docstring).  `graph` / `regions` as
    compute_results_from_graph takes them -- a DeviceGraph or GraphIndex with its [(S, E)] list, or lists of both, one entry
    per chromosome -- or a scan_graph manifest (read_manifest) with regions None.  args_obj: noreverse (nothing else of it
    changes the matrix).  `temperature`: T of the default weights; `weights`: the caller's uint64 [L] table instead."""
    return compute_haplotype_affinity_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_names, temperature,
                                           None if weights is None else [weights], windows_per_run, haplotypes_per_block)[0]


def _float_strings(values: np.ndarray) -> List[bytes]:
    """floats as DataFrame.to_csv writes a float column: one string per value"""
    if len(values) == 0:
        return []
    text = pd.DataFrame({"s": values}).to_csv(sep="\t", index=False, header=False, lineterminator="\n")
    return [t.encode() for t in text.split("\n")[:-1]]


def _cell_table(ha: HaplotypeAffinity) -> Tuple[np.ndarray, List[bytes]]:
    """-> (codes int64 [R, H + 1]: the reference column first, 0 for an empty cell; the text of every code) -- one string
    per distinct sum"""
    vals, lv, codes = ha._by_sum()
    zero = int(len(vals) > 0 and vals[0] == 0)                      # (the sum 0, if any cell holds it, sorts first)
    strings = [b""] + _float_strings(lv[zero:])
    codes = np.concatenate([codes[:, -1:], codes[:, :-1]], axis=1)
    return codes + (1 - zero), strings


def write_haplotype_affinity(ha: HaplotypeAffinity, motif, motif_num: int, args_obj, out=None,
                             cell_bytes: Optional[int] = None) -> Optional[str]:
    """grafimo_haplotype_affinity.tsv (grafimo_haplotype_affinity_<motif_id>.tsv for one of several motifs) in the directory
    write_results uses for this motif -> the path written.  `out`: a binary stream to write to instead (-f: stdout).
    Columns: motif_id, motif_alt_id, sequence_name, reference, one per haplotype; a cell holds the log2 affinity, written as
    DataFrame.to_csv writes a float column, and is empty where the haplotype has no row.  `cell_bytes`: write_wide's (the
    output does not depend on it)."""
    codes, strings = _cell_table(ha)
    return write_wide(out if out is not None else table_path("grafimo_haplotype_affinity", args_obj, motif, motif_num),
                      COLUMNS_HEAD + list(ha.haplotype_names), f"{ha.motif_id}\t{ha.motif_alt_id}\t", ha.region_names, codes,
                      *text_table(strings), **({} if cell_bytes is None else {"cell_bytes": cell_bytes}))


def print_haplotype_affinity(ha: HaplotypeAffinity) -> None:
    """-f: the table on stdout instead of a file"""
    sys.stdout.flush()
    write_haplotype_affinity(ha, None, 1, None, out=sys.stdout.buffer)
