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
import ctypes
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import GraphIndex, _FusedPass, _manifest_prep, _prepare_entries, _stream_ptr, _torch

META_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name"]


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
            some = self.best >= 0
            self._score = np.where(some, self.best.astype(np.float64) / float(self.scale) + float(self.width) * self.offset, np.nan)
        return self._score

    @property
    def best_pvalue(self) -> np.ndarray:
        if self._pvalue is None:
            some = self.best >= 0
            self._pvalue = np.where(some, self.ptable[np.where(some, self.best, 0)], np.nan)
        return self._pvalue

    def to_frame(self) -> pd.DataFrame:
        """the wide counts table: motif_id, motif_alt_id, sequence_name, then one count column per haplotype"""
        R = len(self.region_names)
        meta = pd.DataFrame({"motif_id": np.full(R, self.motif_id, dtype=object),
                             "motif_alt_id": np.full(R, self.motif_alt_id, dtype=object), "sequence_name": self.region_names})
        return pd.concat([meta, pd.DataFrame(self.counts, columns=self.haplotype_names)], axis=1)


def haplotype_column_names(index: GraphIndex) -> List[str]:
    """<SAMPLE>|1, <SAMPLE>|2 per sample when the index knows its samples, else hap0, hap1, ..."""
    H = int(index.n_haplotypes)
    names = getattr(index, "sample_names", None)
    if names and 2 * len(names) == H:
        return [f"{s}|{k}" for s in names for k in (1, 2)]
    return [f"hap{k}" for k in range(H)]


def _caller_rows(prep) -> List[np.ndarray]:
    """-> per graph handle of the prepared call, the row of the caller's region list (entries in order, regions in order)
    that each of its regions is"""
    n_entries = 1 + max((int(e.max()) for e in prep.entry_of if len(e)), default=-1)
    sizes = np.zeros(n_entries, dtype=np.int64)
    for eo in prep.entry_of:
        sizes += np.bincount(eo, minlength=n_entries)
    first_row = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    rows = []
    for eo in prep.entry_of:
        local = np.arange(len(eo), dtype=np.int64)
        ents, first_local = np.unique(eo, return_index=True)
        start = np.zeros(n_entries, dtype=np.int64)
        start[ents] = first_local
        rows.append(first_row[eo] + local - start[eo])
    return rows


def _haplotype_set(prep, haplotype_names: Optional[Sequence[str]], what: str) -> Tuple[int, List[str]]:
    """-> (H, column names) of the prepared call's graphs; ValueError when a graph carries no haplotypes or the graphs do not
    share one haplotype set.  `what` names the result in the messages."""
    for g in prep.graphs:
        if g.index.alt_bits is None or int(g.index.n_haplotypes) <= 0:
            raise ValueError(f"{g.index.chrom}: the graph carries no haplotypes (an XG without its GBWT, or a VCF without "
                             f"samples): {what} needs them")
    H = int(prep.graphs[0].index.n_haplotypes)
    known = [g.index.sample_names for g in prep.graphs if getattr(g.index, "sample_names", None)]
    if any(int(g.index.n_haplotypes) != H for g in prep.graphs) or any(k != known[0] for k in known):
        raise ValueError("the chromosomes' graphs do not share one haplotype set (different samples or numbers of "
                         "haplotypes): one matrix needs the same columns for all of them")
    # (sample names only when every graph knows them: a graph from vg's files numbers its haplotypes instead)
    names = haplotype_column_names(prep.graphs[0].index) if len(known) == len(prep.graphs) else [f"hap{k}" for k in range(H)]
    if haplotype_names is not None:
        names = [str(x) for x in haplotype_names]
        if len(names) != H:
            raise ValueError(f"{len(names)} haplotype names for {H} haplotypes")
    return H, names


def _matrix_rows(prep) -> Tuple[List[np.ndarray], np.ndarray]:
    """-> (per graph handle the caller's rows of its regions (_caller_rows), the region names of the caller's rows)"""
    rows = _caller_rows(prep)
    R = int(sum(len(r) for r in rows))
    region_names = np.empty(R, dtype=object)
    for gi, r in enumerate(rows):
        region_names[r] = prep.labels.take(prep.region_base[gi] + np.arange(len(r), dtype=np.int64))
    return rows, region_names


def compute_haplotype_hits_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                                haplotype_names: Optional[Sequence[str]] = None,
                                scratch_bytes: int = 0) -> List[HaplotypeHits]:
    """compute_haplotype_hits for every motif of a set -> one HaplotypeHits per motif, in the order of `motifs`.  The motifs
    of one width share one enumeration of the walks (as compute_results_from_graph_many).  `scratch_bytes`: the device
    budget of the carrier masks (0: the library's default, 256 MB); the result does not depend on it."""
    torch = _torch()
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("the per-haplotype hit matrix is computed on one GPU: under a process group of more than one "
                                  "rank, call it outside the group (a gather of the sharded matrices is not built yet)")
    if graph is None:
        raise ValueError("no graph: a DeviceGraph / GraphIndex with its regions, lists of both, or a scan_graph manifest "
                         "(read_manifest gives None when scan_graph left TSV rows: GRAFIMO_SCAN_OUTPUT=manifest asks for one)")
    prep = _manifest_prep(graph) if isinstance(graph, dict) else _prepare_entries(graph, regions, chrom_names, None, False)
    H, names = _haplotype_set(prep, haplotype_names, "the per-haplotype hit matrix")
    rows, region_names = _matrix_rows(prep)
    R = len(region_names)
    out: List[Optional[HaplotypeHits]] = [None] * len(motifs)
    by_width = {}
    for i, m in enumerate(motifs):
        by_width.setdefault(int(m.width), []).append(i)
    sp = _stream_ptr(None)
    for W, idxs in by_width.items():
        p = _FusedPass([motifs[i] for i in idxs], prep, debug, args_obj, None)
        try:
            p.enqueue()
            p.fetch()                                   # (a hit list that was too short is taken again here)
            one = len(prep.graphs) == 1 and np.array_equal(rows[0], np.arange(R))
            for m, i in enumerate(idxs):
                dm = p.dms[m]
                cut = dm.fused_views(p.dev)[2] if (p.qval_t and p.works is not None) else None     # as _FusedPass.enqueue
                counts = torch.empty((R, H), dtype=torch.int32, device=p.dev)
                best = torch.empty((R, H), dtype=torch.int32, device=p.dev)
                for gi, g in enumerate(prep.graphs):
                    n_g = len(rows[gi])
                    c_g, b_g = (counts, best) if one else (torch.empty((n_g, H), dtype=torch.int32, device=p.dev),
                                                           torch.empty((n_g, H), dtype=torch.int32, device=p.dev))
                    buf, cap = g.fused_buffers(0, m)
                    base = buf.data_ptr()
                    n_hits = min(int(p.got[m][gi][0]), cap)          # known since fetch(): no batch beyond it
                    nv.check(nv.lib().gfm_graph_haplotype_hits(
                        g._h, base + 128 + 120 * cap, base, n_hits, cut.data_ptr() if cut is not None else None, n_g,
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


_ROW_CHUNK = 1024


def _count_text(counts: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """counts [n, H] -> (bytes of the n lines' count fields, tab-separated, each line ending in '\\n'; byte length per line)
    -- one table of the decimal strings of 0 .. max, then boolean selection: no Python step per cell"""
    n, H = counts.shape
    vmax = int(counts.max(initial=0))
    digits = [str(v).encode() for v in range(vmax + 1)]
    D = max(len(d) for d in digits) + 1
    tab = np.zeros((vmax + 1, D), dtype=np.uint8)
    ln = np.empty(vmax + 1, dtype=np.int64)
    for v, d in enumerate(digits):
        tab[v, :len(d)] = np.frombuffer(d, dtype=np.uint8)
        tab[v, len(d)] = ord("\t")
        ln[v] = len(d) + 1
    cells = tab[counts]                                       # [n, H, D]
    cells[:, -1, :][np.arange(D)[None, :] == ln[counts[:, -1]][:, None] - 1] = ord("\n")
    keep = np.arange(D)[None, None, :] < ln[counts][:, :, None]
    return cells[keep], ln[counts].sum(axis=1)


def write_haplotype_hits(hh: HaplotypeHits, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_haplotype_hits.tsv (grafimo_haplotype_hits_<motif_id>.tsv for one of several motifs) in the directory
    write_results uses for this motif -> the path written.  `out`: a binary stream to write to instead (-f: stdout)."""
    from .res_writer import DEFAULT_OUTDIR
    path = None
    if out is None:
        outdir = getattr(args_obj, "outdir", DEFAULT_OUTDIR)
        dirname_default = outdir == DEFAULT_OUTDIR
        if dirname_default:
            outdir = "_".join(["grafimo_out", str(os.getpid()), motif.motif_id])
        os.makedirs(outdir, exist_ok=True)
        name = "grafimo_haplotype_hits" if (dirname_default or motif_num <= 1) else "_".join(["grafimo_haplotype_hits", motif.motif_id])
        path = os.path.join(outdir, name + ".tsv")
        fh = open(path, "wb")
    else:
        fh = out
    try:
        fh.write(("\t".join(META_COLUMNS + list(hh.haplotype_names)) + "\n").encode())
        head = f"{hh.motif_id}\t{hh.motif_alt_id}\t"
        counts = np.ascontiguousarray(hh.counts)
        for r0 in range(0, counts.shape[0], _ROW_CHUNK):
            text, lens = _count_text(counts[r0:r0 + _ROW_CHUNK])
            ends = np.cumsum(lens)
            mv = memoryview(text)
            parts = []
            at = 0
            for name, e in zip(hh.region_names[r0:r0 + _ROW_CHUNK].tolist(), ends.tolist()):     # a step per ROW
                parts.append(f"{head}{name}\t".encode())
                parts.append(mv[at:e])
                at = e
            fh.writelines(parts)
    finally:
        if out is None:
            fh.close()
        else:
            fh.flush()
    return path


def print_haplotype_hits(hh: HaplotypeHits) -> None:
    """-f: the table on stdout instead of a file"""
    sys.stdout.flush()
    write_haplotype_hits(hh, None, 1, None, out=sys.stdout.buffer)
