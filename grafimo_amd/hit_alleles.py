"""Per-hit allele table: for every row of the report, the variants that make its k-mer and the haplotypes that carry it.

One line per row of the table compute_results_from_graph gives for the same arguments, in its order, with
  its alleles: the set of (graph site, allele) constraints of the row's walk, allele 0 = REF, 1..3 = ALT -- exactly the
    constraints the haplotype counting uses: a substitution base read, an insertion read (1) or passed by (0), a deletion
    jumped (1) or whose bases the walk uses (0), a deletion that would cover the window's first base (0).  A set: sorted by
    (site, allele), no pair twice.  The sites are graph SITES as GraphIndex holds them (see variant_effects.py): they are
    not grouped back into their VCF records;
  its carriers by group: for caller-given haplotype groups (populations) how many haplotypes of each group carry the row
    -- popcount(carriers & group), carriers = the AND of the constraints' bitsets, the set whose size is the row's
    haplotype_frequency.  Groups may overlap and need not cover the haplotypes;
  the carrier set itself on request (carriers=True): uint64 [rows, ceil(H / 64)], the bits beyond H clear.

The selection is the report's own: the same fused pass (scoring, q-table, the hit-list capacity retry) runs, then
gfm_graph_hit_alleles (HIP, grafimo_amd/csrc/gfm_graph_hit_alleles.hpp) works on the hit entries it left -- one result per
ENTRY --, and gfm_graph_hit_order (the report's ordering code, csrc/hit_table.cpp) says which entry became which row.
"""
import ctypes
import sys
import warnings
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _FusedPass, _stream_ptr, _torch
from .graph_tables import (_haplotype_set, _matrix_rows, _site_columns, group_by_width, prepare_graphs, require_single_gpu,
                           table_path, write_frame)

MAX_GROUPS = 64
# room for the constraints of a call's first try, per hit entry (a walk has a handful); tests set it to 0 to take the path
# where the call is made again with the size the first one reports
_FIRST_ALLELES_PER_ENTRY = 8


class HitAlleles:
    """The table of one motif (n rows = the rows of `report`):
    report          the DataFrame compute_results_from_graph returns for the same arguments, row for row;
    allele_offsets  int64 [n + 1], CSR over the rows of allele_entry / allele_site / allele;
    allele_entry    int32: the chromosome entry (of the caller's list) whose GraphIndex allele_site indexes;
    allele_site     int32: the graph site;  allele uint8: 0 = REF, 1..3 = ALT;
    group_names     [G];  group_counts int32 [n, G];
    carrier_bits    uint64 [n, hw] or None;  haplotype_names [H] (empty for a graph without haplotypes);
    indexes         per chromosome entry its GraphIndex (None for an entry without regions);
    row_region      int64 [n] or None: the region listing of every row -- the index into the caller's flattened region list
                    (entries in order, regions in order; a region listed twice is two listings);
    row_entry       int64 [n] or None: the chromosome entry of every row (an index into `indexes`)."""

    def __init__(self, report: pd.DataFrame, allele_offsets, allele_entry, allele_site, allele, group_names, group_counts,
                 carrier_bits, haplotype_names, indexes, *, row_region=None, row_entry=None):
        self.report = report
        self.allele_offsets = np.asarray(allele_offsets, dtype=np.int64)
        self.allele_entry = np.asarray(allele_entry, dtype=np.int32)
        self.allele_site = np.asarray(allele_site, dtype=np.int32)
        self.allele = np.asarray(allele, dtype=np.uint8)
        self.group_names = [str(g) for g in group_names]
        self.group_counts = np.asarray(group_counts, dtype=np.int32).reshape(len(report), len(self.group_names))
        self.carrier_bits = carrier_bits
        self.haplotype_names = list(haplotype_names)
        self.indexes = list(indexes)
        self.row_region = None if row_region is None else np.asarray(row_region, dtype=np.int64)
        self.row_entry = None if row_entry is None else np.asarray(row_entry, dtype=np.int64)

    def __len__(self) -> int:
        return len(self.report)

    def alleles(self, row: int) -> List[Tuple[int, int, int]]:
        """-> [(entry, site, allele)] of one row"""
        a, b = int(self.allele_offsets[row]), int(self.allele_offsets[row + 1])
        return list(zip(self.allele_entry[a:b].tolist(), self.allele_site[a:b].tolist(), self.allele[a:b].tolist()))

    def carriers(self, row: int) -> List[str]:
        """the names of the haplotypes that carry the row (needs carriers=True)"""
        if self.carrier_bits is None:
            raise ValueError("the carrier sets were not asked for (carriers=True)")
        H = len(self.haplotype_names)
        bits = np.unpackbits(np.ascontiguousarray(self.carrier_bits[row]).view(np.uint8), bitorder="little")[:H]
        return [self.haplotype_names[h] for h in np.flatnonzero(bits).tolist()]

    def _allele_strings(self) -> np.ndarray:
        """one string per entry of the CSR arrays -- POS:REF>ALT for an ALT, POS:REF for a REF allele, as
        graph_tables._site_columns prints a site --, made once per distinct (entry, site, allele)"""
        n = len(self.allele)
        out = np.empty(n, dtype=object)
        if not n:
            return out
        key = (self.allele_entry.astype(np.int64) << 34) | (self.allele_site.astype(np.int64) << 2) | self.allele.astype(np.int64)
        uniq, inv = np.unique(key, return_inverse=True)
        text = np.empty(len(uniq), dtype=object)
        ent = uniq >> 34
        for e in np.unique(ent).tolist():
            sel = np.flatnonzero(ent == e)
            site = (uniq[sel] >> 2) & ((1 << 32) - 1)
            al = uniq[sel] & 3
            pos, refs, alts, _, _ = _site_columns(self.indexes[e], site, np.maximum(al, 1))
            text[sel] = [f"{p}:{r}>{x}" if a else f"{p}:{r}" for p, r, x, a in zip(pos.tolist(), refs, alts, al.tolist())]
        out[:] = text[inv]
        return out

    def to_frame(self) -> pd.DataFrame:
        """the report's columns, then alt_alleles and ref_alleles (';'-joined POS:REF>ALT resp. POS:REF in (site, allele)
        order, "" for none) and one haplotypes_<GROUP> column per group"""
        df = self.report.copy()
        n = len(df)
        text = self._allele_strings().tolist()
        is_alt = (self.allele > 0).tolist()
        alt_col = np.full(n, "", dtype=object)
        ref_col = np.full(n, "", dtype=object)
        off = self.allele_offsets.tolist()
        for r in np.flatnonzero(np.diff(self.allele_offsets) > 0).tolist():        # (rows with alleles only)
            a, b = off[r], off[r + 1]
            if b - a == 1:
                (alt_col if is_alt[a] else ref_col)[r] = text[a]
                continue
            alt_col[r] = ";".join([text[k] for k in range(a, b) if is_alt[k]])
            ref_col[r] = ";".join([text[k] for k in range(a, b) if not is_alt[k]])
        df["alt_alleles"] = alt_col
        df["ref_alleles"] = ref_col
        for g, name in enumerate(self.group_names):
            df[f"haplotypes_{name}"] = self.group_counts[:, g].astype(np.int64)
        return df


def read_haplotype_groups(path: str, haplotype_names: Sequence[str]) -> Dict[str, List[int]]:
    """A text file of `SAMPLE<white space>GROUP` lines -> {group: [haplotype columns]}, groups in the order of the file.
    Further columns are ignored, '#' lines, empty lines and a first line whose first field is `sample` skipped (the 1000
    Genomes panel file reads as is).  Both haplotypes of a sample (<SAMPLE>|1, <SAMPLE>|2) join its group; a first field
    that is itself a column name (hap<k> of a graph whose haplotypes are unnamed) names that column.  Samples the graph
    does not have are skipped, and counted in one warning."""
    col = {str(n): k for k, n in enumerate(haplotype_names)}
    groups: Dict[str, List[int]] = {}
    missing = 0
    first = True
    with open(path) as fh:
        for line in fh:
            f = line.split()
            if not f or f[0].startswith("#"):
                continue
            was_first, first = first, False
            if was_first and f[0].lower() == "sample":
                continue
            if len(f) < 2:
                raise ValueError(f"{path}: a line without a group: {line.rstrip()!r}")
            sample, group = f[0], f[1]
            cols = [col[sample]] if sample in col else [col[k] for k in (f"{sample}|1", f"{sample}|2") if k in col]
            if not cols:
                missing += 1
                continue
            have = groups.setdefault(group, [])
            have.extend(c for c in cols if c not in have)
    if missing:
        warnings.warn(f"{path}: {missing} samples are not among the graph's haplotypes and were skipped")
    return groups


def _group_bits(haplotype_groups: Optional[Mapping], names: Sequence[str], H: int) -> Tuple[List[str], np.ndarray]:
    """-> (group names, uint64 [G, hw] bitsets) of a mapping group -> haplotype column names or indices"""
    hw = (H + 63) // 64
    if not haplotype_groups:
        return [], np.zeros((0, hw), dtype=np.uint64)
    if len(haplotype_groups) > MAX_GROUPS:
        raise ValueError(f"{len(haplotype_groups)} haplotype groups: at most {MAX_GROUPS} per call")
    col = None
    member = np.zeros((len(haplotype_groups), hw * 64), dtype=bool)
    for g, (gname, who) in enumerate(haplotype_groups.items()):
        who = list(who)
        ks = np.asarray(who) if who else np.zeros(0, dtype=np.int64)
        if ks.dtype.kind not in "iu":                   # names among them: a dictionary lookup per member
            if col is None:
                col = {str(n): k for k, n in enumerate(names)}
            ks = np.empty(len(who), dtype=np.int64)
            for j, x in enumerate(who):
                if isinstance(x, (int, np.integer)):
                    ks[j] = x
                else:
                    ks[j] = col.get(str(x), -1)
                    if ks[j] < 0:
                        raise ValueError(f"group {gname}: unknown haplotype {x!r}")
        ks = ks.astype(np.int64)
        bad = ks[(ks < 0) | (ks >= H)]
        if len(bad):
            raise ValueError(f"group {gname}: haplotype index {int(bad[0])} outside 0 .. {H - 1}")
        member[g, ks] = True
    bits = np.packbits(member, axis=-1, bitorder="little").view(np.uint64).reshape(len(haplotype_groups), hw)
    return [str(k) for k in haplotype_groups], np.ascontiguousarray(bits)


def _entry_alleles(g, p, m: int, n_hits: int, cut, G: int, d_groups, want_total: bool, want_masks: bool, hw: int,
                   scratch_bytes: int, sp):
    """gfm_graph_hit_alleles over the entries motif slot m left on graph g -> (off int64 [n + 1], packed int32, group counts
    int32 [n, G], totals int32 [n] or None, masks uint64 [n, hw] or None) on the host"""
    torch = _torch()
    entries, base, _cap = g.hit_list(m)
    dev = p.dev
    off = torch.empty(n_hits + 1, dtype=torch.int64, device=dev)
    gc = torch.empty((n_hits, G), dtype=torch.int32, device=dev)
    total = torch.empty(n_hits, dtype=torch.int32, device=dev) if want_total else None
    masks = torch.empty((n_hits, hw), dtype=torch.int64, device=dev) if want_masks else None
    room = _FIRST_ALLELES_PER_ENTRY * n_hits
    while True:
        packed = torch.empty(max(room, 1), dtype=torch.int32, device=dev)
        nv.check(nv.lib().gfm_graph_hit_alleles(
            g._h, entries, base, n_hits, cut.data_ptr() if cut is not None else None, G,
            d_groups.data_ptr() if G else None, off.data_ptr(), packed.data_ptr() if room else None, room,
            gc.data_ptr() if (G and n_hits) else None, total.data_ptr() if total is not None else None,
            masks.data_ptr() if masks is not None else None, int(scratch_bytes), sp))
        h_off = off.cpu().numpy()
        need = int(h_off[-1])
        if need <= room:
            break
        room = need                                   # (the offsets say how much room to come back with)
    return (h_off, packed[:need].cpu().numpy(), gc.cpu().numpy(), total.cpu().numpy() if total is not None else None,
            masks.cpu().numpy().view(np.uint64) if masks is not None else None)


def _report_order(spec) -> Tuple[np.ndarray, np.ndarray]:
    """gfm_graph_hit_order for one motif's _hit_columns arguments -> (part int32 [n], record index int64 [n]) per report row"""
    ptable, _scale, _offset, _W, entry_of, _region_base, parts, recomb, first_per_region = spec
    if first_per_region:
        raise ValueError("the per-hit allele table is made for the whole report (no top_graphs)")
    n_parts = len(parts)
    total = int(sum(len(r) for r in parts))
    vp = ctypes.c_void_p
    parts = [np.ascontiguousarray(r) for r in parts]
    recs_p = (vp * n_parts)(*[r.ctypes.data if len(r) else None for r in parts])
    n_recs = (ctypes.c_int64 * n_parts)(*[len(r) for r in parts])
    eo_p = (vp * n_parts)(*[e.ctypes.data if len(e) else None for e in entry_of])
    o_part = np.empty(total, dtype=np.int32)
    o_index = np.empty(total, dtype=np.int64)
    n_out = ctypes.c_int64()
    nv.check(nv.lib().gfm_graph_hit_order(nv.ptr(ptable), len(ptable), n_parts, recs_p, n_recs, eo_p,
                                          0 if recomb else nv.GFM_HITS_DROP_ZERO_FREQ, ctypes.byref(n_out), nv.ptr(o_part),
                                          nv.ptr(o_index)))
    n = int(n_out.value)
    return o_part[:n], o_index[:n]


def _gather_rows(part, index, per_part, entry_of, recs, G: int, hw: int, want_masks: bool):
    """the per-entry results of every graph handle into report order -> (offsets, entry, site, allele, group counts, masks, the
    rows' entries)"""
    n = len(part)
    lens = np.zeros(n, dtype=np.int64)
    first = np.zeros(n, dtype=np.int64)
    gc = np.zeros((n, G), dtype=np.int32)
    masks = np.zeros((n, hw), dtype=np.uint64) if want_masks else None
    row_entry = np.zeros(n, dtype=np.int64)
    for gi, (off, _packed, g_gc, _tot, g_masks) in enumerate(per_part):
        rows = np.flatnonzero(part == gi)
        if not len(rows):
            continue
        idx = index[rows]
        lens[rows] = off[idx + 1] - off[idx]
        first[rows] = off[idx]
        if G:
            gc[rows] = g_gc[idx]
        if want_masks:
            masks[rows] = g_masks[idx]
        row_entry[rows] = entry_of[gi][recs[gi]["region"][idx]]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(offsets[-1])
    packed = np.empty(total, dtype=np.int32)
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    within = np.arange(total, dtype=np.int64) - offsets[row_of]
    src = first[row_of] + within
    p_of = part[row_of] if total else np.zeros(0, dtype=np.int32)
    for gi, (_off, g_packed, _gc, _tot, _m) in enumerate(per_part):
        sel = p_of == gi
        packed[sel] = g_packed[src[sel]]
    return (offsets, row_entry[row_of].astype(np.int32), (packed >> 2).astype(np.int32), (packed & 3).astype(np.uint8), gc, masks,
            row_entry)


def compute_hit_alleles_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                             haplotype_names: Optional[Sequence[str]] = None, haplotype_groups: Optional[Mapping] = None,
                             carriers: bool = False, scratch_bytes: int = 0) -> List[HitAlleles]:
    """compute_hit_alleles for every motif of a set -> one HitAlleles per motif, in the order of `motifs`.  The motifs of
    one width share one enumeration of the walks (as compute_results_from_graph_many).  `scratch_bytes`: the device budget
    of the call's staging (0: the library's default, 256 MB); the result does not depend on it."""
    torch = _torch()
    require_single_gpu("the per-hit allele table", "is", "a gather of the sharded tables")
    prep = prepare_graphs(graph, regions, chrom_names)
    with_haps = all(g.index.alt_bits is not None and int(g.index.n_haplotypes) > 0 for g in prep.graphs)
    H, names = 0, []
    if haplotype_groups or carriers:
        # (a graph without haplotypes still has alleles; groups and carrier sets need the bitsets, and one set for all graphs)
        H, names = _haplotype_set(prep, haplotype_names, "the groups and carrier sets of the per-hit allele table")
    elif with_haps:
        try:
            H, names = _haplotype_set(prep, haplotype_names, "the per-hit allele table")
        except ValueError:
            # graphs of different haplotype sets: alleles only -- nothing was asked of the sets, unless names were given
            if haplotype_names is not None:
                raise
    hw = (H + 63) // 64
    group_names, bits = _group_bits(haplotype_groups, names, H)
    G = len(group_names)
    n_entries = 1 + max((int(e.max()) for e in prep.entry_of if len(e)), default=-1)
    indexes = [None] * n_entries
    for g, eo in zip(prep.graphs, prep.entry_of):
        for e in np.unique(eo).tolist():
            indexes[int(e)] = g.index
    listing_of = _matrix_rows(prep)[0]                  # per graph handle: the caller's region listing of its regions
    out: List[Optional[HitAlleles]] = [None] * len(motifs)
    sp = _stream_ptr(None)
    for W, idxs in group_by_width(motifs).items():
        p = _FusedPass([motifs[i] for i in idxs], prep, debug, args_obj, None)
        try:
            p.enqueue()
            p.fetch()                                   # (a hit list that was too short is taken again here)
            d_groups = torch.from_numpy(bits.view(np.int64)).to(p.dev) if G else None
            per_motif = []
            for m in range(len(idxs)):
                cut = p.cutoff(m)
                per_part = []
                for gi, g in enumerate(prep.graphs):
                    per_part.append(_entry_alleles(g, p, m, p.n_hits(m, gi), cut, G, d_groups, H > 0, carriers, hw, scratch_bytes, sp))
                per_motif.append(per_part)
            specs = p._column_specs()
            orders = [_report_order(spec) for spec in specs]
            # (the kernel's own carrier count against annotate's, entry by entry: the two derive the walk separately)
            for m, per_part in enumerate(per_motif):
                for gi, (_off, _pk, _gc, tot, _mk) in enumerate(per_part):
                    recs = p.got[m][gi][3]
                    if tot is not None and len(recs) and not np.array_equal(np.where(recs["keep"] != 0, recs["freq"], 0), tot):
                        raise RuntimeError("gfm_graph_hit_alleles and gfm_graph_annotate disagree on a hit entry's carriers")
            gathered = [_gather_rows(part, index, per_motif[m], prep.entry_of, [r for _, _, _, r in p.got[m]], G, hw, carriers)
                        for m, (part, index) in enumerate(orders)]
            frames = p.tables()
            for m, i in enumerate(idxs):
                offsets, a_entry, a_site, a_allele, gc, masks, row_entry = gathered[m]
                if len(frames[m]) != len(offsets) - 1:
                    raise RuntimeError("the report and its order disagree on the number of rows")
                part, index = orders[m]
                row_region = np.zeros(len(part), dtype=np.int64)
                for gi in range(len(prep.graphs)):
                    rows = np.flatnonzero(part == gi)
                    if len(rows):
                        row_region[rows] = listing_of[gi][p.got[m][gi][3]["region"][index[rows]]]
                out[i] = HitAlleles(frames[m], offsets, a_entry, a_site, a_allele, group_names, gc, masks, names, indexes,
                                    row_region=row_region, row_entry=row_entry)
        finally:
            p.close()
    return out


def compute_hit_alleles(motif, graph, regions, debug: bool, args_obj, chrom_names=None,
                        haplotype_names: Optional[Sequence[str]] = None, haplotype_groups: Optional[Mapping] = None,
                        carriers: bool = False, scratch_bytes: int = 0) -> HitAlleles:
    """The per-hit allele table of `motif` (see the module's docstring).  `graph` / `regions` as compute_results_from_graph
    takes them -- a DeviceGraph or GraphIndex with its [(S, E)] list, or lists of both, one entry per chromosome -- or a
    scan_graph manifest (read_manifest) with regions None.  args_obj: threshold, noqvalue, qvalueT, noreverse, recomb.
    `chrom_names`: the name printed in sequence_name per entry (default: the graph's own); `haplotype_names`: names instead
    of the index's; `haplotype_groups`: a mapping group name -> haplotype names or column indices (its order = the order of
    the group columns; read_haplotype_groups reads one from a panel file), at most 64; `carriers`: keep the carrier sets."""
    return compute_hit_alleles_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_names, haplotype_groups,
                                    carriers, scratch_bytes)[0]


def write_hit_alleles(ha: HitAlleles, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_hit_alleles.tsv (grafimo_hit_alleles_<motif_id>.tsv for one of several motifs) in the directory
    write_results uses for this motif -> the path written.  `out`: a text stream to write to instead (-f: stdout)."""
    return write_frame(ha, out if out is not None else table_path("grafimo_hit_alleles", args_obj, motif, motif_num))


def print_hit_alleles(ha: HitAlleles) -> None:
    """-f: the table on stdout instead of a file"""
    write_hit_alleles(ha, None, 1, None, out=sys.stdout)
