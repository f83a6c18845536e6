"""Per-variant motif effects: for every site of the variation graph, the best k-mer that carries its REF allele beside the
best k-mer that carries each ALT allele -- which variants create (gain) or destroy (loss) a binding site.

The unit is a graph SITE as GraphIndex holds it: a substitution site with 1-3 ALT bases, an insertion (ins_len > 0) or a
deletion (del_len > 0).  Multi-base substitutions and complex alleles appear as the sites GraphIndex.from_fasta_vcf /
vg_files decompose them into (one substitution site per mismatching base, an insertion / deletion for the rest); they are
not grouped back into their VCF record.

A k-mer QUALIFIES for (site s, allele a) when (1) it is a row the fused report would give at threshold 1 -- a walk of a
window of one of the regions under the report's region rule and --no-reverse handling, and without --recomb one that some
haplotype carries; (2) its walk takes allele a at s; (3) its bases cover the allele's footprint: SNV -- the site's base;
deletion REF -- a deleted base; deletion ALT -- the junction (the anchor and the base behind the deleted span); insertion
ALT -- an inserted base; insertion REF -- the junction (the anchor and the base behind it; a walk that reads an insertion
listed before it at the same anchor does not count for it).  Those are exactly the walks
that carry a haplotype constraint for s in the report's haplotype counting.  The BEST hit of (s, a) is the qualifying
k-mer with the highest integer score, then the smallest start, the smallest stop, '+' before '-', and the smallest k-mer
as printed for its strand.

The table has one row per (site, ALT allele) in genome order (the caller's chromosome entries, then site order):
motif_id, motif_alt_id, sequence_name, position (1-based VCF POS: the anchor + 1 for an indel), ref / alt (VCF style),
ref_haplotypes (haplotypes that carry NONE of the site's ALT alleles), alt_haplotypes (carriers of this ALT), then per side
(ref_, alt_) score (log-odds), pvalue (the motif's tail table at the integer score, as the report), start, stop, strand,
sequence of the best hit -- NaN / <NA> / "" for a side without a qualifying k-mer --, delta_score = alt_score - ref_score
and effect: gain (only the ALT side has p < threshold), loss (only the REF side), both, none (only with all_sites=True).
A row is kept when either side has p < threshold (strict, as the report) unless all_sites; a site that no region covers
does not appear.  There are no q-values in this table.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_variant.hpp, gfm_graph_variant_effects); the rows are built on the host
by gfm_variant_effect_columns.
"""
import ctypes
from typing import List, Sequence

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import GraphIndex, _stream_ptr, _torch
from .graph_tables import _site_columns, group_by_width, prepare_graphs, require_single_gpu, table_path, write_frame

VARIANT_REC_DTYPE = np.dtype([("slot", "<i4"), ("score", "<i4"), ("start", "<i8"), ("stop", "<i8"), ("strand", "u1"),
                              ("pad", "u1", (7,)), ("kmer", "u1", (nv.GFM_MAX_WIDTH,))])
assert VARIANT_REC_DTYPE.itemsize == 96
EFFECTS = np.array(["none", "gain", "loss", "both"], dtype=object)
COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "ref", "alt", "ref_haplotypes", "alt_haplotypes",
           "ref_score", "ref_pvalue", "ref_start", "ref_stop", "ref_strand", "ref_sequence",
           "alt_score", "alt_pvalue", "alt_start", "alt_stop", "alt_strand", "alt_sequence", "delta_score", "effect"]
_STRANDS = np.array(["+", "-"], dtype=object)
# records of _scan's first call per motif (0: its guess from the sites the regions reach); tests set it small to take the
# path where the call is made again with the count
_FIRST_REC_CAPACITY = 0


def _entries(graph, regions, chrom_names):
    """-> [(DeviceGraph, starts, stops, name)] in the caller's entry order, one per distinct graph handle (entries that
    share a handle are scanned as one list of regions, named after the first of them)."""
    prep = prepare_graphs(graph, regions, chrom_names)
    runs, base = prep.labels.runs, prep.labels.base             # (one run of regions per entry, with the entry's name)
    out = []
    for gi, g_ in enumerate(prep.graphs):
        s_, e_ = prep.spans[gi]
        run = int(np.searchsorted(base, prep.region_base[gi], side="right")) - 1      # the entry of the handle's first region
        out.append((g_, np.ascontiguousarray(s_, dtype=np.int64), np.ascontiguousarray(e_, dtype=np.int64),
                    runs[min(run, len(runs) - 1)][0]))
    return out


def effect_columns(ptable: np.ndarray, scale: int, offset: float, W: int, n_alts: np.ndarray, recs: np.ndarray,
                   threshold: float, all_sites: bool):
    """gfm_variant_effect_columns over one motif's records of one graph -> dict of numpy columns (rows in site order):
    site, alt, found / score / pvalue / start / stop / strand [n, 2] (side 0 REF, 1 ALT), kmers [n, 2] str, effect."""
    n_alts = np.ascontiguousarray(n_alts, dtype=np.uint8)
    recs = np.ascontiguousarray(recs, dtype=VARIANT_REC_DTYPE)
    ptable = np.ascontiguousarray(ptable, dtype=np.float64)
    cap = max(int(n_alts.astype(np.int64).sum()), 1)
    i4 = lambda *s: np.empty(s, dtype=np.int32)      # noqa: E731
    c = dict(site=i4(cap), alt=i4(cap), found=np.empty((cap, 2), np.uint8), score=np.empty((cap, 2)), pvalue=np.empty((cap, 2)),
             start=np.empty((cap, 2), np.int64), stop=np.empty((cap, 2), np.int64), strand=np.empty((cap, 2), np.uint8),
             kmers=np.empty((cap, 2, W + 1), np.uint8), effect=np.empty(cap, np.uint8))
    n_out = ctypes.c_int64()
    nv.check(nv.lib().gfm_variant_effect_columns(
        nv.ptr(ptable), len(ptable), int(scale), float(offset), int(W), len(n_alts), nv.ptr(n_alts) if len(n_alts) else None,
        recs.ctypes.data if len(recs) else None, len(recs), float(threshold), nv.GFM_VARIANT_ALL_SITES if all_sites else 0,
        ctypes.byref(n_out), nv.ptr(c["site"]), nv.ptr(c["alt"]), nv.ptr(c["found"]), nv.ptr(c["score"]), nv.ptr(c["pvalue"]),
        nv.ptr(c["start"]), nv.ptr(c["stop"]), nv.ptr(c["strand"]), nv.ptr(c["kmers"]), nv.ptr(c["effect"])))
    n = int(n_out.value)
    out = {k: v[:n] for k, v in c.items()}
    flat = out.pop("kmers").reshape(-1).tobytes().decode("ascii")
    seqs = np.array(flat.split("\n")[:-1] if n else [], dtype=object).reshape(n, 2)
    out["sequence"] = np.where(out["found"] != 0, seqs, "")
    return out


def _frame(motif, name: str, index: GraphIndex, c) -> pd.DataFrame:
    n = len(c["site"])
    site, alt = c["site"].astype(np.int64), c["alt"].astype(np.int64)
    position, refs, alts, ref_h, alt_h = _site_columns(index, site, alt)
    found = c["found"] != 0
    d = {"motif_id": np.full(n, motif.motif_id, dtype=object), "motif_alt_id": np.full(n, motif.motif_name, dtype=object),
         "sequence_name": np.full(n, name, dtype=object), "position": position,
         "ref": refs, "alt": alts, "ref_haplotypes": ref_h, "alt_haplotypes": alt_h}
    for k, side in ((0, "ref"), (1, "alt")):
        d[f"{side}_score"] = c["score"][:, k]
        d[f"{side}_pvalue"] = c["pvalue"][:, k]
        d[f"{side}_start"] = pd.array(np.where(found[:, k], c["start"][:, k], 0), dtype="Int64")
        d[f"{side}_start"][~found[:, k]] = pd.NA
        d[f"{side}_stop"] = pd.array(np.where(found[:, k], c["stop"][:, k], 0), dtype="Int64")
        d[f"{side}_stop"][~found[:, k]] = pd.NA
        d[f"{side}_strand"] = np.where(found[:, k], _STRANDS[c["strand"][:, k]], "").astype(object)
        d[f"{side}_sequence"] = c["sequence"][:, k]
    d["delta_score"] = d["alt_score"] - d["ref_score"]
    d["effect"] = EFFECTS[c["effect"]]
    return pd.DataFrame(d, columns=COLUMNS)


def _scan(dg, starts, stops, dms, forward_only: bool, recomb: bool):
    """gfm_graph_variant_effects over one graph for motifs of one width -> (records per motif, overflow flag)."""
    torch = _torch()
    M = len(dms)
    n_slots = max(4 * len(dg.index.pos), 1)
    # first guess at the records: a few per (site, allele) the regions can reach -- not per site of the chromosome (a BED of
    # a few peaks on a whole-chromosome graph); a call whose ties need more room is made again with the count as capacity
    pos = np.asarray(dg.index.pos)
    reach = int(dg.index.del_len.max(initial=0)) + int(dms[0].width) + 1
    near = int((np.searchsorted(pos, stops, side="right") - np.searchsorted(pos, starts - reach)).clip(min=0).sum())
    cap = _FIRST_REC_CAPACITY if _FIRST_REC_CAPACITY > 0 else 2 * 4 * near + 1024
    flags = (nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0) | (nv.GFM_VARIANT_KEEP_ZERO_FREQ if recomb else 0)
    vp = ctypes.c_void_p
    with torch.cuda.device(dg.device):
        while True:
            keys = torch.zeros((M, n_slots), dtype=torch.int64, device=dg.device)
            ctl = torch.zeros(M + 1, dtype=torch.int64, device=dg.device)         # record counts, then the overflow word
            recs = torch.empty((M, cap * VARIANT_REC_DTYPE.itemsize), dtype=torch.uint8, device=dg.device)
            handles = (vp * M)(*[d.handle for d in dms])
            keys_p = (vp * M)(*[keys[m].data_ptr() for m in range(M)])
            recs_p = (vp * M)(*[recs[m].data_ptr() for m in range(M)])
            caps = (ctypes.c_int64 * M)(*([cap] * M))
            cnt_p = (vp * M)(*[ctl.data_ptr() + 8 * m for m in range(M)])
            nw = ctypes.c_int64()
            nv.check(nv.lib().gfm_graph_variant_effects(dg._h, handles, M, len(starts), nv.ptr(starts), nv.ptr(stops), flags, keys_p,
                                                        recs_p, caps, cnt_p, ctl.data_ptr() + 8 * M, ctypes.byref(nw),
                                                        _stream_ptr(None)))
            got = ctl.cpu().numpy()
            counts, over = got[:M], int(got[M] & 0xffffffff)
            if int(counts.max(initial=0)) <= cap:
                break
            cap = int(counts.max())
        # only the records written come back
        out = [recs[m, :int(counts[m]) * VARIANT_REC_DTYPE.itemsize].cpu().numpy().view(VARIANT_REC_DTYPE) for m in range(M)]
    return out, over


def compute_variant_effects_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                                 all_sites: bool = False) -> List[pd.DataFrame]:
    """compute_variant_effects for every motif of a set -> one table per motif, in the order of `motifs`.  The motifs of one
    width share the window list of a call; the tables equal the single calls'."""
    from .device import DeviceMotif
    require_single_gpu("the variant effect table", "is", "a MAX all-reduce of the key arrays")
    threshold = float(args_obj.threshold)
    forward_only, recomb = bool(args_obj.noreverse), bool(args_obj.recomb)
    entries = _entries(graph, regions, chrom_names)
    parts: List[List[pd.DataFrame]] = [[] for _ in motifs]
    for W, ks in group_by_width(motifs).items():
        dms = [DeviceMotif.lease(motifs[k]) for k in ks]
        try:
            for dg, starts, stops, name in entries:
                recs, over = _scan(dg, starts, stops, dms, forward_only, recomb)
                if over:
                    raise OverflowError(f"{name}: a window holds more than 2^24 walks: the variant effect table would be "
                                        "incomplete (scan regions without it)")
                for j, k in enumerate(ks):
                    dm = dms[j]
                    c = effect_columns(dm.ptable_host(), dm.scale, dm.offset, W, dg.index.n_alts, recs[j], threshold, all_sites)
                    parts[k].append(_frame(motifs[k], name, dg.index, c))
        finally:
            for dm in dms:
                dm.release()
    return [pd.concat(p_, ignore_index=True) if p_ else pd.DataFrame(columns=COLUMNS) for p_ in parts]


def compute_variant_effects(motif, graph, regions, debug: bool, args_obj, chrom_names=None,
                            all_sites: bool = False) -> pd.DataFrame:
    """The per-variant effect table of `motif` (see the module's docstring).  `graph` / `regions` as
    compute_results_from_graph takes them -- a DeviceGraph or GraphIndex with its [(S, E)] list, or lists of both, one entry
    per chromosome -- or a scan_graph manifest (read_manifest) with regions None.  args_obj: threshold, noreverse, recomb.
    `chrom_names`: the name printed in sequence_name per entry (default: the graph's own)."""
    return compute_variant_effects_many([motif], graph, regions, debug, args_obj, chrom_names, all_sites)[0]


def write_variant_effects(table: pd.DataFrame, motif, motif_num: int, args_obj) -> str:
    """grafimo_variant_effects.tsv (grafimo_variant_effects_<motif_id>.tsv for one of several motifs) in the directory
    write_results uses for this motif -> the path written."""
    return write_frame(table, table_path("grafimo_variant_effects", args_obj, motif, motif_num))
