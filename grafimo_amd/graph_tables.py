"""What the per-graph result tables share -- variant_effects, haplotype_hits, haplotype_scores, hit_alleles, hit_pairs,
hit_linkage -- and where the next one starts: the refusal under a process group (require_single_gpu), the graph intake
(prepare_graphs), the motifs of one width (group_by_width), the rows and columns of a region x haplotype matrix
(_matrix_rows, _haplotype_set), a site as the tables print it (_site_columns), scaled scores as log-odds and p-values, and
the writers: where a table's file goes (table_path), a DataFrame table (write_frame), a wide matrix (text_table, write_wide).
"""
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from .extract_regions import GraphIndex, _manifest_prep, _prepare_entries, _torch

META_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name"]


def require_single_gpu(what: str, verb: str, missing: str) -> None:
    """NotImplementedError under a process group of more than one rank: `what` `verb` ("is" / "are") computed on one GPU;
    `missing` names what a sharded run would still need"""
    dist = _torch().distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(f"{what} {verb} computed on one GPU: under a process group of more than one rank, call it "
                                  f"outside the group ({missing} is not built yet)")


def prepare_graphs(graph, regions, chrom_names):
    """`graph` / `regions` as compute_results_from_graph takes them, or a scan_graph manifest with regions None -> the
    prepared entries (extract_regions._FusedPrep) on this one GPU"""
    if graph is None:
        raise ValueError("no graph: a DeviceGraph / GraphIndex with its regions, lists of both, or a scan_graph manifest "
                         "(read_manifest gives None when scan_graph left TSV rows: GRAFIMO_SCAN_OUTPUT=manifest asks for one)")
    return _manifest_prep(graph) if isinstance(graph, dict) else _prepare_entries(graph, regions, chrom_names, None, False)


def group_by_width(motifs: Sequence) -> Dict[int, List[int]]:
    """-> {W: the indices of the motifs of width W}, widths in first-seen order: the motifs of one width share a pass"""
    by_width: Dict[int, List[int]] = {}
    for i, m in enumerate(motifs):
        by_width.setdefault(int(m.width), []).append(i)
    return by_width


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


def _site_columns(index: GraphIndex, site: np.ndarray, alt: np.ndarray):
    """for the rows (site, alt): position (1-based), REF and ALT strings, ref_haplotypes, alt_haplotypes -- made for the
    table's rows only (a chromosome holds millions of sites and thousands of haplotypes)"""
    ref = np.asarray(index.ref)
    pos = np.asarray(index.pos, dtype=np.int64)[site]
    n = len(site)
    H = int(index.n_haplotypes) if index.alt_bits is not None else 0
    alt_h = np.zeros(n, dtype=np.int64)
    ref_h = np.full(n, H, dtype=np.int64)
    if H and n:
        bits = np.asarray(index.alt_bits, dtype=np.uint64)[site]                        # [n, 3, hw]
        na = np.asarray(index.n_alts, dtype=np.int64)[site]
        used = (np.arange(3)[None, :] < na[:, None])[..., None]
        bits = np.where(used, bits, np.uint64(0))
        pc = lambda w: np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[..., :H].sum(axis=-1)    # noqa: E731
        alt_h = pc(np.ascontiguousarray(bits[np.arange(n), alt - 1])).astype(np.int64)
        ref_h = H - pc(np.ascontiguousarray(np.bitwise_or.reduce(bits, axis=1))).astype(np.int64)
    refs, alts = [], []
    for i, a, p in zip(site.tolist(), alt.tolist(), pos.tolist()):
        anchor = chr(int(ref[p]))
        if index.del_len[i] > 0:
            refs.append(bytes(ref[p:p + 1 + int(index.del_len[i])]).decode())
            alts.append(anchor)
        elif index.ins_len[i] > 0:
            o = int(index.ins_off[i])
            refs.append(anchor)
            alts.append(anchor + bytes(index.ins_bases[o:o + int(index.ins_len[i])]).decode())
        else:
            refs.append(anchor)
            alts.append(chr(int(index.alt_bases[i, a - 1])))
    return pos + 1, np.array(refs, dtype=object), np.array(alts, dtype=object), ref_h, alt_h


def scaled_scores(best: np.ndarray, scale: int, offset: float, width: int) -> np.ndarray:
    """scaled integer scores (-1: none) -> log-odds as the report prints them (score / scale + W * offset), NaN for none"""
    return np.where(best >= 0, best.astype(np.float64) / float(scale) + float(width) * offset, np.nan)


def scaled_pvalues(best: np.ndarray, ptable: np.ndarray) -> np.ndarray:
    """scaled integer scores (-1: none) -> the motif's tail table at them, NaN for none"""
    some = best >= 0
    return np.where(some, np.asarray(ptable)[np.where(some, best, 0)], np.nan)


# ---- writers
def table_path(stem: str, args_obj, motif=None, motif_num: int = 1, tag: Optional[str] = None) -> str:
    """Where a table's TSV goes, its directory made: <stem>.tsv in the directory write_results uses for `motif`
    (res_writer.output_dir), <stem>_<motif_id>.tsv for one of several motifs that share a directory the user named.
    `tag`: a table per call, not per motif -- <stem>.tsv, the default directory named after the tag."""
    from .res_writer import output_dir
    outdir, dirname_default = output_dir(args_obj, motif.motif_id if tag is None else tag)
    name = stem if (tag is not None or dirname_default or motif_num <= 1) else "_".join([stem, motif.motif_id])
    return os.path.join(outdir, name + ".tsv")


def write_frame(table, out) -> Optional[str]:
    """a DataFrame, or a table with to_frame(), as TSV to the path `out` (-> the path) or to the text stream `out`"""
    frame = table if isinstance(table, pd.DataFrame) else table.to_frame()
    if isinstance(out, str):
        frame.to_csv(out, sep="\t", index=False, encoding="utf-8")
        return out
    frame.to_csv(out, sep="\t", index=False)
    out.flush()
    return None


_CELL_BYTES = 1 << 25                                 # bytes of cell text write_wide makes at a time


def text_table(strings: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """the texts a cell can hold, by code -> (tab uint8 [V, D]: per code its text and a tab; ln int64 [V]: its length)"""
    D = max(len(s) for s in strings) + 1
    tab = np.zeros((len(strings), D), dtype=np.uint8)
    ln = np.empty(len(strings), dtype=np.int64)
    for v, t in enumerate(strings):
        tab[v, :len(t)] = np.frombuffer(t, dtype=np.uint8)
        tab[v, len(t)] = ord("\t")
        ln[v] = len(t) + 1
    return tab, ln


def write_wide(out, header: Sequence[str], head: str, region_names, codes: np.ndarray, tab: np.ndarray, ln: np.ndarray,
               cell_bytes: int = _CELL_BYTES) -> Optional[str]:
    """A wide matrix as TSV to the path `out` (-> the path) or to the binary stream `out`: the header line, then per row
    `head`, its region name and the cells codes[r, :] as text_table spells them -- selected from the table, no Python step
    per cell.  `cell_bytes` bounds the cell text made at a time; the output does not depend on it."""
    fh = open(out, "wb") if isinstance(out, str) else out
    try:
        fh.write(("\t".join(header) + "\n").encode())
        D = tab.shape[1]
        chunk = max(1, cell_bytes // max(1, codes.shape[1] * D))
        for r0 in range(0, codes.shape[0], chunk):
            c = codes[r0:r0 + chunk]
            cells = tab[c]                                            # [n, C, D]
            cells[:, -1, :][np.arange(D)[None, :] == ln[c[:, -1]][:, None] - 1] = ord("\n")     # a line ends in '\n', not a tab
            text = cells[np.arange(D)[None, None, :] < ln[c][:, :, None]]
            mv = memoryview(text)
            parts = []
            at = 0
            for name, e in zip(region_names[r0:r0 + chunk].tolist(), np.cumsum(ln[c].sum(axis=1)).tolist()):     # a step per ROW
                parts.append(f"{head}{name}\t".encode())
                parts.append(mv[at:e])
                at = e
            fh.writelines(parts)
    finally:
        if fh is out:
            fh.flush()
        else:
            fh.close()
    return out if isinstance(out, str) else None
