"""Per-haplotype hit matrix: for every region and every haplotype of the graph, how many of the report's rows of that
region the haplotype carries, and the best of them.

Rows(r) are the rows compute_results_from_graph reports for region r under the same arguments (both strands unless
--no-reverse; kept on p < t, or on q < t with --qvalueT).  Haplotype h CARRIES a row when it is one of the haplotypes the
row's haplotype_frequency counts: h is in the AND of the bitsets of the walk's allele constraints.  Then
  counts[r, h]      = rows of Rows(r) that h carries (int32);
  best_score[r, h]  = the highest score among them as log-odds (score / scale + W * offset, as the report), NaN for none;
  best_pvalue[r, h] = the motif's tail table at that integer score, NaN for none.
So sum_h counts[r, h] is the sum of haplotype_frequency over Rows(r), and --recomb changes nothing (recombinant rows have
no carriers).  Rows of the matrix: the regions of the caller's list in the report's entry order (regions without a hit
are rows of zeros); columns: the graph's haplotypes in its bitset order, named <SAMPLE>|1, <SAMPLE>|2 per VCF sample
(GraphIndex.sample_names) or hap<k> when the index does not know its samples (vg's files, older indexes).

The selection is the report's own: the same fused pass (scoring, q-table, the hit-list capacity retry) runs, and
gfm_graph_haplotype_hits (HIP, grafimo_amd/csrc/gfm_graph_haplotypes.hpp) turns the hit entries it leaves into the matrix
on the device.
"""
import sys
from typing import List, Optional, Sequence

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _FusedPass, _stream_ptr, _torch
from .graph_tables import (META_COLUMNS, _haplotype_set, _matrix_rows, group_by_width, prepare_graphs, require_single_gpu,
                           scaled_pvalues, scaled_scores, table_path, text_table, write_wide)
from .graph_tables import haplotype_column_names  # noqa: F401  (the columns' names: importable from here as before)


class HaplotypeHits:
    """The matrix of one motif: region_names [R], haplotype_names [H], counts [R, H] int32, best (scaled score, -1 for
    none) [R, H] int32; best_score / best_pvalue [R, H] float64 made from `best` on first use."""

    def __init__(self, motif_id: str, motif_alt_id: str, region_names, haplotype_names, counts: np.ndarray, best: np.ndarray,
                 scale: int, offset: float, width: int, ptable: np.ndarray):
        self.motif_id, self.motif_alt_id = motif_id, motif_alt_id
        self.region_names = np.asarray(region_names, dtype=object)
        self.haplotype_names = list(haplotype_names)
        self.counts, self.best = counts, best
        self.scale, self.offset, self.width, self.ptable = int(scale), float(offset), int(width), ptable
        self._score = self._pvalue = None

    @property
    def best_score(self) -> np.ndarray:
        if self._score is None:
            self._score = scaled_scores(self.best, self.scale, self.offset, self.width)
        return self._score

    @property
    def best_pvalue(self) -> np.ndarray:
        if self._pvalue is None:
            self._pvalue = scaled_pvalues(self.best, self.ptable)
        return self._pvalue

    def to_frame(self) -> pd.DataFrame:
        """the wide counts table: motif_id, motif_alt_id, sequence_name, then one count column per haplotype"""
        R = len(self.region_names)
        meta = pd.DataFrame({"motif_id": np.full(R, self.motif_id, dtype=object),
                             "motif_alt_id": np.full(R, self.motif_alt_id, dtype=object), "sequence_name": self.region_names})
        return pd.concat([meta, pd.DataFrame(self.counts, columns=self.haplotype_names)], axis=1)


def compute_haplotype_hits_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                                haplotype_names: Optional[Sequence[str]] = None,
                                scratch_bytes: int = 0) -> List[HaplotypeHits]:
    """compute_haplotype_hits for every motif of a set -> one HaplotypeHits per motif, in the order of `motifs`.  The motifs
    of one width share one enumeration of the walks (as compute_results_from_graph_many).  `scratch_bytes`: the device
    budget of the carrier masks (0: the library's default, 256 MB); the result does not depend on it."""
    torch = _torch()
    require_single_gpu("the per-haplotype hit matrix", "is", "a gather of the sharded matrices")
    prep = prepare_graphs(graph, regions, chrom_names)
    H, names = _haplotype_set(prep, haplotype_names, "the per-haplotype hit matrix")
    rows, region_names = _matrix_rows(prep)
    R = len(region_names)
    out: List[Optional[HaplotypeHits]] = [None] * len(motifs)
    sp = _stream_ptr(None)
    for W, idxs in group_by_width(motifs).items():
        p = _FusedPass([motifs[i] for i in idxs], prep, debug, args_obj, None)
        try:
            p.enqueue()
            p.fetch()                                   # (a hit list that was too short is taken again here)
            one = len(prep.graphs) == 1 and np.array_equal(rows[0], np.arange(R))
            for m, i in enumerate(idxs):
                dm = p.dms[m]
                cut = p.cutoff(m)
                counts = torch.empty((R, H), dtype=torch.int32, device=p.dev)
                best = torch.empty((R, H), dtype=torch.int32, device=p.dev)
                for gi, g in enumerate(prep.graphs):
                    n_g = len(rows[gi])
                    c_g, b_g = (counts, best) if one else (torch.empty((n_g, H), dtype=torch.int32, device=p.dev),
                                                           torch.empty((n_g, H), dtype=torch.int32, device=p.dev))
                    entries, base, _cap = g.hit_list(m)
                    nv.check(nv.lib().gfm_graph_haplotype_hits(
                        g._h, entries, base, p.n_hits(m, gi), cut.data_ptr() if cut is not None else None, n_g,
                        c_g.data_ptr(), b_g.data_ptr(), int(scratch_bytes), sp))
                    if not one and n_g:
                        r_t = torch.from_numpy(rows[gi]).to(p.dev)
                        counts.index_copy_(0, r_t, c_g)
                        best.index_copy_(0, r_t, b_g)
                out[i] = HaplotypeHits(motifs[i].motif_id, motifs[i].motif_name, region_names, names, counts.cpu().numpy(),
                                       best.cpu().numpy(), dm.scale, dm.offset, W, dm.ptable_host())
        finally:
            p.close()
    return out


def compute_haplotype_hits(motif, graph, regions, debug: bool, args_obj, chrom_names=None,
                           haplotype_names: Optional[Sequence[str]] = None, scratch_bytes: int = 0) -> HaplotypeHits:
    """The per-haplotype hit matrix of `motif` (see the module's docstring).  `graph` / `regions` as
    compute_results_from_graph takes them -- a DeviceGraph or GraphIndex with its [(S, E)] list, or lists of both, one entry
    per chromosome -- or a scan_graph manifest (read_manifest) with regions None.  args_obj: threshold, noqvalue, qvalueT,
    noreverse, recomb.  `chrom_names`: the name printed in sequence_name per entry (default: the graph's own);
    `haplotype_names`: column names instead of the index's."""
    return compute_haplotype_hits_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_names, scratch_bytes)[0]


def write_haplotype_hits(hh: HaplotypeHits, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_haplotype_hits.tsv (grafimo_haplotype_hits_<motif_id>.tsv for one of several motifs) in the directory
    write_results uses for this motif -> the path written.  `out`: a binary stream to write to instead (-f: stdout)."""
    counts = np.ascontiguousarray(hh.counts)
    tab, ln = text_table([str(v).encode() for v in range(int(counts.max(initial=0)) + 1)])      # the decimal strings of 0 .. max
    return write_wide(out if out is not None else table_path("grafimo_haplotype_hits", args_obj, motif, motif_num),
                      META_COLUMNS + list(hh.haplotype_names), f"{hh.motif_id}\t{hh.motif_alt_id}\t", hh.region_names, counts, tab, ln)


def print_haplotype_hits(hh: HaplotypeHits) -> None:
    """-f: the table on stdout instead of a file"""
    sys.stdout.flush()
    write_haplotype_hits(hh, None, 1, None, out=sys.stdout.buffer)
