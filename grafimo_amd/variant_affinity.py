"""Per-variant affinity effects: for every (site, ALT allele) of the variation graph, the total binding affinity the carriers
of REF have over the allele's footprint beside the total of the carriers of ALT -- the threshold-free, per-variant number
motif-QTL and allele-specific-binding work regress on.  Where variant_effects compares the single best k-mer of each side,
the sum also moves when a variant weakens the second site of a cluster, when an indel adds or removes windows, or when ten
weaker k-mers move while the best stays put; where haplotype_affinity needs a region per variant and a genotype group-by over
a sites x haplotypes matrix, this is two numbers per variant.

An OCCURRENCE is one window of W consecutive bases of one haplotype's own spelled sequence on one strand (both strands unless
--no-reverse), held by at least one region under the report's region rule (start in [S, E), stop <= E); an occurrence several
regions hold counts once.  It qualifies for every (site s, allele a) whose footprint its bases cover -- variant_effects'
footprints; allele 0 is "none of the site's ALTs".  Per (s, a), both exact in uint64: sum = the sum of w[score] over the
qualifying occurrences, rows = their number.  w is haplotype_affinity.default_weights(motif, T) (fixed point, 40 fraction
bits) or the caller's own table; a k-mer holding N scores min_val.  -t, -q, --qvalueT and --recomb change nothing.

The table has one row per (site, ALT allele) in genome order, as variant_effects orders its rows, kept when either side has
an occurrence: motif_id, motif_alt_id, sequence_name, position, ref, alt, ref_haplotypes, alt_haplotypes (variant_effects'
columns), ref_rows, alt_rows, then x_log2_affinity = log2(sum_x) - log2(x_haplotypes) + log2_offset -- the log2 of the MEAN,
over the allele's carriers, of the total affinity over the allele's footprint; NaN where sum_x == 0 -- and
delta_log2_affinity = alt - ref (NaN if either is).  log2_offset is haplotype_affinity's: -40 + (s_best / scale + W offset) / T
for the default weights, 0 for the caller's own.  min_abs_delta > 0 keeps only the rows with a finite |delta| >= it.

A 64-bit sum that wraps is detected on the device (every add is checked) and raised as OverflowError; with the default
weights 2^40 * H * 2 * (W + indel length) stays far below 2^64.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_variant_affinity.hpp, gfm_graph_variant_affinity).
"""
import ctypes
import sys
from typing import List, Optional, Sequence

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import GraphIndex, _stream_ptr, _torch
from .graph_tables import _site_columns, group_by_width, require_single_gpu, table_path, write_frame
from .haplotype_affinity import FRACTION_BITS, default_weights
from .variant_effects import _entries

COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "ref", "alt", "ref_haplotypes", "alt_haplotypes",
           "ref_rows", "alt_rows", "ref_log2_affinity", "alt_log2_affinity", "delta_log2_affinity"]
_OVER_WALKS, _OVER_SUM = 1, 2                       # bits of the device's overflow word


def _log2_mean(sums: np.ndarray, haplotypes: np.ndarray, log2_offset: float) -> np.ndarray:
    """log2(sum) - log2(haplotypes) + log2_offset, NaN where the sum is 0"""
    out = np.full(len(sums), np.nan)
    some = sums > 0
    out[some] = np.log2(sums[some].astype(np.float64)) - np.log2(haplotypes[some].astype(np.float64)) + float(log2_offset)
    return out


class VariantAffinity:
    """The table of one motif, a row per (site, ALT allele): sequence_name, site (the site's number in its graph), allele
    (1..3), position, ref, alt, ref_haplotypes, alt_haplotypes as variant_effects prints them, and the raw uint64 ref_sum,
    alt_sum, ref_rows, alt_rows; made from them: ref_log2_affinity, alt_log2_affinity, delta_log2_affinity, to_frame()."""

    def __init__(self, motif_id: str, motif_alt_id: str, log2_offset: float = 0.0):
        self.motif_id, self.motif_alt_id, self.log2_offset = motif_id, motif_alt_id, float(log2_offset)
        self.sequence_name = np.empty(0, dtype=object)
        self.site, self.allele = np.empty(0, np.int64), np.empty(0, np.int64)
        self.position = np.empty(0, np.int64)
        self.ref, self.alt = np.empty(0, dtype=object), np.empty(0, dtype=object)
        self.ref_haplotypes, self.alt_haplotypes = np.empty(0, np.int64), np.empty(0, np.int64)
        self.ref_sum, self.alt_sum = np.empty(0, np.uint64), np.empty(0, np.uint64)
        self.ref_rows, self.alt_rows = np.empty(0, np.uint64), np.empty(0, np.uint64)

    _FIELDS = ("sequence_name", "site", "allele", "position", "ref", "alt", "ref_haplotypes", "alt_haplotypes", "ref_sum",
               "alt_sum", "ref_rows", "alt_rows")

    def __len__(self) -> int:
        return len(self.site)

    ref_log2_affinity = property(lambda self: _log2_mean(self.ref_sum, self.ref_haplotypes, self.log2_offset))
    alt_log2_affinity = property(lambda self: _log2_mean(self.alt_sum, self.alt_haplotypes, self.log2_offset))
    delta_log2_affinity = property(lambda self: self.alt_log2_affinity - self.ref_log2_affinity)

    def append(self, name: str, index: GraphIndex, sums: np.ndarray, min_abs_delta: float = 0.0) -> None:
        """the rows of one graph: `sums` uint64 [n_sites, 4, 2] -- per (site, allele) its (sum, rows) as the device leaves
        them -- -> a row per (site, ALT allele) either side of which has rows > 0, in site order"""
        sums = np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1, 4, 2)
        n_alts = np.asarray(index.n_alts, dtype=np.int64)
        if len(sums) != len(n_alts):
            raise ValueError(f"sums of {len(sums)} sites for a graph of {len(n_alts)}")
        is_alt = np.arange(1, 4)[None, :] <= n_alts[:, None]                                   # [n, 3]
        keep = is_alt & ((sums[:, :1, 1] > 0) | (sums[:, 1:, 1] > 0))
        site, a = np.nonzero(keep)                                                            # (site order, then allele)
        site, allele = site.astype(np.int64), a.astype(np.int64) + 1
        position, refs, alts, ref_h, alt_h = _site_columns(index, site, allele)
        part = dict(sequence_name=np.full(len(site), name, dtype=object), site=site, allele=allele, position=position, ref=refs,
                    alt=alts, ref_haplotypes=ref_h, alt_haplotypes=alt_h, ref_sum=sums[site, 0, 0], alt_sum=sums[site, allele, 0],
                    ref_rows=sums[site, 0, 1], alt_rows=sums[site, allele, 1])
        if min_abs_delta > 0:
            delta = (_log2_mean(part["alt_sum"], alt_h, self.log2_offset) - _log2_mean(part["ref_sum"], ref_h, self.log2_offset))
            ok = np.isfinite(delta) & (np.abs(delta) >= float(min_abs_delta))
            part = {k: v[ok] for k, v in part.items()}
        for k in self._FIELDS:
            setattr(self, k, np.concatenate([getattr(self, k), part[k]]))

    def to_frame(self) -> pd.DataFrame:
        n = len(self)
        ref_l, alt_l = self.ref_log2_affinity, self.alt_log2_affinity
        d = {"motif_id": np.full(n, self.motif_id, dtype=object), "motif_alt_id": np.full(n, self.motif_alt_id, dtype=object),
             "sequence_name": self.sequence_name, "position": self.position, "ref": self.ref, "alt": self.alt,
             "ref_haplotypes": self.ref_haplotypes, "alt_haplotypes": self.alt_haplotypes, "ref_rows": self.ref_rows,
             "alt_rows": self.alt_rows, "ref_log2_affinity": ref_l, "alt_log2_affinity": alt_l,
             "delta_log2_affinity": alt_l - ref_l}
        return pd.DataFrame(d, columns=COLUMNS)


def _scan(dg, name: str, starts: np.ndarray, stops: np.ndarray, dms, tables, forward_only: bool,
          table_entries: int) -> List[np.ndarray]:
    """gfm_graph_variant_affinity over one graph for motifs of one width -> per motif the sums uint64 [n_sites, 4, 2]"""
    torch = _torch()
    M, n_sites = len(dms), len(dg.index.pos)
    vp = ctypes.c_void_p
    with torch.cuda.device(dg.device):
        sums = torch.zeros((M, max(n_sites, 1), 4, 2), dtype=torch.int64, device=dg.device)
        over = torch.zeros(1, dtype=torch.int32, device=dg.device)
        d_tabs = [torch.from_numpy(t.view(np.int64)).to(dg.device) for t in tables]
        handles = (vp * M)(*[d.handle for d in dms])
        tabs_p = (vp * M)(*[t.data_ptr() for t in d_tabs])
        sums_p = (vp * M)(*[sums[m].data_ptr() for m in range(M)])
        nw = ctypes.c_int64()
        n = len(starts)
        nv.check(nv.lib().gfm_graph_variant_affinity(
            dg._h, handles, M, tabs_p, n, nv.ptr(starts) if n else None, nv.ptr(stops) if n else None,
            nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0, sums_p, over.data_ptr(), ctypes.byref(nw), int(table_entries),
            _stream_ptr(None)))
        flag = int(over.item())
        if flag & _OVER_WALKS:
            raise OverflowError(f"{name}: a window holds more than 2^24 walks: the variant affinity table would be incomplete "
                                "(scan regions without it)")
        if flag & _OVER_SUM:
            raise OverflowError(f"{name}: a 64-bit affinity sum wrapped: the weights are too large for this many haplotypes "
                                "and k-mers (use smaller weights)")
        host = sums.cpu().numpy().view(np.uint64)
    return [host[m, :n_sites] for m in range(M)]


def compute_variant_affinity_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                                  temperature: float = 1.0, weights: Optional[Sequence[np.ndarray]] = None,
                                  min_abs_delta: float = 0.0, table_entries: int = 0) -> List[VariantAffinity]:
    """compute_variant_affinity for every motif of a set -> one VariantAffinity per motif, in the order of `motifs`.  The
    motifs of one width share the window list of a call; the tables equal the single calls'.  `weights`: one uint64 [L] table
    per motif instead of default_weights(motif, temperature).  `table_entries` sizes the device's staging table (0: the
    library's default); the result does not depend on it."""
    from .device import DeviceMotif
    require_single_gpu("the variant affinity table", "is", "a SUM all-reduce of the slot arrays")
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    forward_only = bool(getattr(args_obj, "noreverse", False))
    entries = _entries(graph, regions, chrom_names)
    for dg, _, _, name in entries:
        if dg.index.alt_bits is None or int(dg.index.n_haplotypes) <= 0:
            raise ValueError(f"{name}: the graph carries no haplotypes (an XG without its GBWT, or a VCF without samples): the "
                             "variant affinity table needs them")
    out: List[Optional[VariantAffinity]] = [None] * len(motifs)
    for W, idxs in group_by_width(motifs).items():
        dms = [DeviceMotif.lease(motifs[i]) for i in idxs]
        try:
            tables = []
            for dm, i in zip(dms, idxs):
                if weights is None:
                    w, s_best = default_weights(dm, temperature)
                    offset = -FRACTION_BITS + (s_best / dm.scale + W * dm.offset) / float(temperature)
                else:
                    w = np.ascontiguousarray(weights[i], dtype=np.uint64)
                    if w.shape != (dm.L,):
                        raise ValueError(f"{motifs[i].motif_id}: a weight table of shape {w.shape}, the motif's scores need "
                                         f"({dm.L},)")
                    offset = 0.0
                tables.append(w)
                out[i] = VariantAffinity(motifs[i].motif_id, motifs[i].motif_name, offset)
            for dg, starts, stops, name in entries:
                got = _scan(dg, name, starts, stops, dms, tables, forward_only, table_entries)
                for m, i in enumerate(idxs):
                    out[i].append(name, dg.index, got[m], min_abs_delta)
        finally:
            for dm in dms:
                dm.release()
    return out


def compute_variant_affinity(motif, graph, regions, debug: bool, args_obj, chrom_names=None, temperature: float = 1.0,
                             weights: Optional[np.ndarray] = None, min_abs_delta: float = 0.0,
                             table_entries: int = 0) -> VariantAffinity:
    """The per-variant affinity table of `motif` (see the module's docstring).  `graph` / `regions` as
    compute_results_from_graph takes them -- a DeviceGraph or GraphIndex with its [(S, E)] list, or lists of both, one entry
    per chromosome -- or a scan_graph manifest (read_manifest) with regions None.  args_obj: noreverse (nothing else of it
    changes the table).  `temperature`: T of the default weights; `weights`: the caller's uint64 [L] table instead.
    `chrom_names`: the name printed in sequence_name per entry (default: the graph's own)."""
    return compute_variant_affinity_many([motif], graph, regions, debug, args_obj, chrom_names, temperature,
                                         None if weights is None else [weights], min_abs_delta, table_entries)[0]


def write_variant_affinity(table: VariantAffinity, motif, motif_num: int, args_obj) -> str:
    """grafimo_variant_affinity.tsv (grafimo_variant_affinity_<motif_id>.tsv for one of several motifs) in the directory
    write_results uses for this motif -> the path written."""
    return write_frame(table, table_path("grafimo_variant_affinity", args_obj, motif, motif_num))


def print_variant_affinity(table: VariantAffinity) -> None:
    """-f: the table on stdout instead of a file"""
    write_frame(table, sys.stdout)
