"""Per-haplotype best motif score: for every region and every haplotype of the graph, the best k-mer of the haplotype's own
sequence in the region, significant or not -- the per-individual number motif-score QTL and allele-specific binding analyses
regress on.

Rows(r, h) are the report's rows of region r at threshold 1 that haplotype h carries (h is in the AND of the bitsets of the
walk's allele constraints, the set whose size is haplotype_frequency): the k-mers of h's spelled sequence under the report's
region rule, on both strands unless --no-reverse.  best(r, h) is the row of Rows(r, h) with the highest integer score; ties
go to the smallest left coordinate (the '+' row's start), then the smallest right coordinate (the '+' row's stop), then '+'
before '-'.  For that row the matrix gives the scaled score (`best`, -1 when h has no row in r), the log-odds score
(score / scale + W * offset, as the report), the p-value (the motif's tail table) and start / stop / strand as the report
prints them.  The reference column is the same over the graph's reference path (every site at its REF allele).  -t, -q,
--qvalueT and --recomb change nothing (recombinant walks have no carriers).

Rows: the regions of the caller's list in order; columns: <SAMPLE>|1, <SAMPLE>|2 per VCF sample or hap<k> (as
haplotype_hits).  The hot path is HIP (grafimo_amd/csrc/gfm_graph_hapscores.hpp, gfm_graph_haplotype_scores): the walks are
enumerated and reduced to one 64-bit key per cell on the device, with no hit list.
"""
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _stream_ptr, _torch
from .graph_tables import (META_COLUMNS, _haplotype_set, _matrix_rows, group_by_width, prepare_graphs, require_single_gpu,
                           scaled_pvalues, scaled_scores, table_path, text_table, write_wide)

COLUMNS_HEAD = META_COLUMNS + ["reference"]
# the key's fields (gfm_graph_hapscores.hpp): score << 48 | (2^28 - 1 - (left - base)) << 20 | (2^19 - 1 - (right - left)) << 1 | '+'
LEFT_BITS, SPAN_BITS = 28, 19
LEFT_MAX, SPAN_MAX = (1 << LEFT_BITS) - 1, (1 << SPAN_BITS) - 1
_STRANDS = np.array(["-", "+"], dtype=object)


def pack_key(score, left, right, plus, base):
    """the device's key of a row (numpy-broadcasting): larger is better -- score, then smaller left, smaller right, '+'"""
    score, left, right, base = (np.asarray(x, dtype=np.uint64) for x in (score, left, right, base))
    return ((score << np.uint64(48)) | ((np.uint64(LEFT_MAX) - (left - base)) << np.uint64(SPAN_BITS + 1))
            | ((np.uint64(SPAN_MAX) - (right - left)) << np.uint64(1)) | np.asarray(plus, dtype=np.uint64))


def unpack_keys(keys: np.ndarray, base: np.ndarray):
    """keys uint64 [...], base int64 broadcastable (the region's start clipped at 0) -> (best int32 (-1: none), left, right
    int64 (-1: none), plus bool)"""
    keys = np.asarray(keys, dtype=np.uint64)
    some = keys != 0
    best = np.where(some, (keys >> np.uint64(48)).astype(np.int64), -1).astype(np.int32)
    left = np.asarray(base, dtype=np.int64) + (LEFT_MAX - ((keys >> np.uint64(SPAN_BITS + 1)) & np.uint64(LEFT_MAX)).astype(np.int64))
    right = left + (SPAN_MAX - ((keys >> np.uint64(1)) & np.uint64(SPAN_MAX)).astype(np.int64))
    plus = (keys & np.uint64(1)) != 0
    return best, np.where(some, left, -1), np.where(some, right, -1), plus & some


class HaplotypeScores:
    """The matrix of one motif: region_names [R], haplotype_names [H], best (scaled score, -1 for none) int32 [R, H] and
    reference_best [R]; made on first use from the keys: best_score / best_pvalue float64 (NaN for none), start / stop int64
    (-1 for none), strand ('+', '-', '' for none) [R, H], and the same as reference_* [R]."""

    def __init__(self, motif_id: str, motif_alt_id: str, region_names, haplotype_names, keys: np.ndarray, base: np.ndarray,
                 scale: int, offset: float, width: int, ptable: np.ndarray):
        self.motif_id, self.motif_alt_id = motif_id, motif_alt_id
        self.region_names = np.asarray(region_names, dtype=object)
        self.haplotype_names = list(haplotype_names)
        self.keys = np.asarray(keys, dtype=np.uint64)              # [R, H + 1], column H the reference
        self.base = np.asarray(base, dtype=np.int64)               # [R]
        self.scale, self.offset, self.width, self.ptable = int(scale), float(offset), int(width), ptable
        H = len(self.haplotype_names)
        if self.keys.shape != (len(self.region_names), H + 1):
            raise ValueError(f"keys of shape {self.keys.shape} for {len(self.region_names)} regions and {H} haplotypes")
        full = self.keys.view(np.uint16)[..., 3::4].astype(np.int32)     # the score field (bits 48..63; little-endian)
        np.putmask(full, self.keys == 0, -1)
        self.best, self.reference_best = full[:, :H], full[:, H]
        self._coords = None
        self._score = self._pvalue = None

    def _scores(self):
        if self._score is None:
            full = np.concatenate([self.best, self.reference_best[:, None]], axis=1)
            self._score = scaled_scores(full, self.scale, self.offset, self.width)
            self._pvalue = scaled_pvalues(full, self.ptable)
        return self._score, self._pvalue

    def _coordinates(self):
        if self._coords is None:
            _, left, right, plus = unpack_keys(self.keys, self.base[:, None])
            some = self.keys != 0
            strand = np.where(some, _STRANDS[plus.astype(np.int64)], "").astype(object)
            self._coords = (np.where(plus, left, right), np.where(plus, right, left), strand)
        return self._coords

    best_score = property(lambda self: self._scores()[0][:, :-1])
    best_pvalue = property(lambda self: self._scores()[1][:, :-1])
    reference_score = property(lambda self: self._scores()[0][:, -1])
    reference_pvalue = property(lambda self: self._scores()[1][:, -1])
    start = property(lambda self: self._coordinates()[0][:, :-1])
    stop = property(lambda self: self._coordinates()[1][:, :-1])
    strand = property(lambda self: self._coordinates()[2][:, :-1])
    reference_start = property(lambda self: self._coordinates()[0][:, -1])
    reference_stop = property(lambda self: self._coordinates()[1][:, -1])
    reference_strand = property(lambda self: self._coordinates()[2][:, -1])

    def to_frame(self) -> pd.DataFrame:
        """the wide table of the TSV: motif_id, motif_alt_id, sequence_name, reference, then one column per haplotype, each
        cell the log-odds score of the best row (NaN for none)"""
        R = len(self.region_names)
        meta = pd.DataFrame({"motif_id": np.full(R, self.motif_id, dtype=object),
                             "motif_alt_id": np.full(R, self.motif_alt_id, dtype=object), "sequence_name": self.region_names,
                             "reference": self.reference_score})
        return pd.concat([meta, pd.DataFrame(self.best_score, columns=self.haplotype_names)], axis=1)


def _scan(dg, starts: np.ndarray, stops: np.ndarray, dms, forward_only: bool, H: int, windows_per_run: int,
          haplotypes_per_block: int) -> List[np.ndarray]:
    """gfm_graph_haplotype_scores over one graph for motifs of one width -> per motif the keys uint64 [n, H + 1]"""
    import ctypes
    torch = _torch()
    M, n = len(dms), len(starts)
    vp = ctypes.c_void_p
    with torch.cuda.device(dg.device):
        keys = torch.zeros((M, n, H + 1), dtype=torch.int64, device=dg.device)
        over = torch.zeros(1, dtype=torch.int32, device=dg.device)
        handles = (vp * M)(*[d.handle for d in dms])
        keys_p = (vp * M)(*[keys[m].data_ptr() for m in range(M)])
        nv.check(nv.lib().gfm_graph_haplotype_scores(
            dg._h, handles, M, n, nv.ptr(starts) if n else None, nv.ptr(stops) if n else None,
            nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0, keys_p, over.data_ptr(), int(windows_per_run),
            int(haplotypes_per_block), _stream_ptr(None)))
        if int(over.item()):
            raise OverflowError(f"{dg.index.chrom}: a window holds more than 2^24 walks: the per-haplotype best scores would be "
                                "incomplete (scan regions without it)")
        host = keys.cpu().numpy().view(np.uint64)
    return [host[m] for m in range(M)]


def compute_haplotype_scores_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                                  haplotype_names: Optional[Sequence[str]] = None, windows_per_run: int = 0,
                                  haplotypes_per_block: int = 0) -> List[HaplotypeScores]:
    """compute_haplotype_scores for every motif of a set -> one HaplotypeScores per motif, in the order of `motifs`.  The
    motifs of one width share one run list and one call.  `windows_per_run` / `haplotypes_per_block` cut the device work
    (0: the library's defaults); the result does not depend on them."""
    from .device import DeviceMotif
    require_single_gpu("the per-haplotype best scores", "are", "a gather of the sharded matrices")
    prep = prepare_graphs(graph, regions, chrom_names)
    H, names = _haplotype_set(prep, haplotype_names, "the per-haplotype best score matrix")
    rows, region_names = _matrix_rows(prep)
    R = len(region_names)
    base = np.zeros(R, dtype=np.int64)
    for gi, r in enumerate(rows):
        base[r] = np.maximum(np.asarray(prep.spans[gi][0], dtype=np.int64), 0)
    forward_only = bool(getattr(args_obj, "noreverse", False))
    out: List[Optional[HaplotypeScores]] = [None] * len(motifs)
    for W, idxs in group_by_width(motifs).items():
        dms = [DeviceMotif.lease(motifs[i]) for i in idxs]
        try:
            one = len(prep.graphs) == 1 and np.array_equal(rows[0], np.arange(R))
            keys = None if one else [np.zeros((R, H + 1), dtype=np.uint64) for _ in idxs]
            for gi, g in enumerate(prep.graphs):
                starts = np.ascontiguousarray(prep.spans[gi][0], dtype=np.int64)
                stops = np.ascontiguousarray(prep.spans[gi][1], dtype=np.int64)
                got = _scan(g, starts, stops, dms, forward_only, H, windows_per_run, haplotypes_per_block)
                if one:
                    keys = got
                    continue
                for m in range(len(idxs)):
                    keys[m][rows[gi]] = got[m]
            for m, i in enumerate(idxs):
                dm = dms[m]
                out[i] = HaplotypeScores(motifs[i].motif_id, motifs[i].motif_name, region_names, names, keys[m], base, dm.scale,
                                         dm.offset, W, dm.ptable_host())
        finally:
            for dm in dms:
                dm.release()
    return out


def compute_haplotype_scores(motif, graph, regions, debug: bool, args_obj, chrom_names=None,
                             haplotype_names: Optional[Sequence[str]] = None, windows_per_run: int = 0,
                             haplotypes_per_block: int = 0) -> HaplotypeScores:
    """The per-haplotype best score matrix of `motif` (see the module's docstring).  `graph` / `regions` as
    compute_results_from_graph takes them -- a DeviceGraph or GraphIndex with its [(S, E)] list, or lists of both, one entry
    per chromosome -- or a scan_graph manifest (read_manifest) with regions None.  args_obj: noreverse (nothing else of it
    changes the matrix).  `chrom_names`: the name printed in sequence_name per entry; `haplotype_names`: column names instead
    of the index's."""
    return compute_haplotype_scores_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_names,
                                         windows_per_run, haplotypes_per_block)[0]


def _score_strings(values: np.ndarray) -> List[bytes]:
    """the log-odds scores as DataFrame.to_csv writes a float column (the report's `score`): one string per value"""
    if len(values) == 0:
        return []
    text = pd.DataFrame({"s": values}).to_csv(sep="\t", index=False, header=False, lineterminator="\n")
    return [t.encode() for t in text.split("\n")[:-1]]


def _cell_table(hs: HaplotypeScores) -> Tuple[np.ndarray, List[bytes]]:
    """-> (codes int64 [R, H + 1]: the reference column first, 0 for an empty cell; the text of every code) -- one string
    per distinct scaled score"""
    full = np.concatenate([hs.reference_best[:, None], hs.best], axis=1).astype(np.int64)
    vals = np.unique(full[full >= 0])
    strings = [b""] + _score_strings(scaled_scores(vals, hs.scale, hs.offset, hs.width))
    return np.where(full >= 0, np.searchsorted(vals, np.maximum(full, 0)) + 1, 0), strings


def write_haplotype_scores(hs: HaplotypeScores, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_haplotype_scores.tsv (grafimo_haplotype_scores_<motif_id>.tsv for one of several motifs) in the directory
    write_results uses for this motif -> the path written.  `out`: a binary stream to write to instead (-f: stdout).
    Columns: motif_id, motif_alt_id, sequence_name, reference, one per haplotype; a cell holds the log-odds score of the
    best row, written as the report writes its score column, and is empty where there is no row."""
    codes, strings = _cell_table(hs)
    return write_wide(out if out is not None else table_path("grafimo_haplotype_scores", args_obj, motif, motif_num),
                      COLUMNS_HEAD + list(hs.haplotype_names), f"{hs.motif_id}\t{hs.motif_alt_id}\t", hs.region_names, codes,
                      *text_table(strings))


def print_haplotype_scores(hs: HaplotypeScores) -> None:
    """-f: the table on stdout instead of a file"""
    sys.stdout.flush()
    write_haplotype_scores(hs, None, 1, None, out=sys.stdout.buffer)
