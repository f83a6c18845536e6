"""Haplotype classes: for every region the DISTINCT versions of it the panel holds -- the haplotypes grouped by their alleles
at the sites that can change the region's rows --, each with its count, its counts per group, the alleles that make it and
what it does to a motif.  Where the haplotype matrices (haplotype_hits, haplotype_scores, haplotype_affinity) have a column
per haplotype, thousands on a cohort panel, this table has a row per version.

The sites of region [S, E) clipped to the chromosome, T(r) (region_sites): a substitution with S <= pos < E, an insertion
with S - 1 <= pos < E, a deletion of d bases with pos + 1 < E and pos + d >= S -- the report's region rule: a row starts in
[S, E) and stops <= E, and a row that starts on an inserted base has start = anchor + 1.  An empty region has no site.  The
STATE of haplotype h at a site is the tuple of its bits in the site's n_alts used slots, 0 = none of the ALTs.  Two
haplotypes are in one CLASS of r when their states agree at every site of T(r).  Classes are numbered per region by count
descending, then by smallest member; the representative of a class is its smallest member; is_reference: every state is 0.
A region without a site has one class of all haplotypes.  Haplotypes of one class spell the same rows; two classes may still
spell the same bases (a second insertion at an anchor whose first insertion is the one read, a site under a deletion the
class carries): the table groups by ALLELES.  The classes do not depend on the motif: one computation serves a motif set.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_hapclasses.hpp): a 64-bit key per (region, haplotype), a hash table per
region, and a verification of every haplotype against its representative -- the result is exact, a key shared by two allele
combinations is detected (the call is repeated with another seed, then HashCollisionError), never silently wrong.
"""
import sys
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import DeviceGraph, GraphIndex, _stream_ptr, _torch
from .grafimo_errors import HashCollisionError
from .graph_tables import (META_COLUMNS, _haplotype_set, _matrix_rows, _site_columns, prepare_graphs, require_single_gpu,
                           table_path, text_table, write_frame, write_wide)

CLASSES_FILE = "grafimo_haplotype_classes"
MEMBERS_FILE = "grafimo_haplotype_class_members"
MAX_GROUPS = 64
SEEDS_TRIED = 3
COLUMNS_HEAD = META_COLUMNS + ["class", "haplotypes", "frequency"]
COLUMNS_TAIL = ["representative", "is_reference", "alt_alleles", "best_score", "best_pvalue", "start", "stop", "strand",
                "log2_affinity", "delta_log2_affinity"]


def region_sites(index: GraphIndex, S: int, E: int) -> np.ndarray:
    """T(r): the indices of the sites of `index` that can change the rows of region [S, E) (see the module's docstring)"""
    S, E = max(int(S), 0), min(int(E), len(index.ref))
    if E <= S:
        return np.zeros(0, dtype=np.int64)
    p = np.asarray(index.pos, dtype=np.int64)
    d = np.asarray(index.del_len, dtype=np.int64)
    ins = np.asarray(index.ins_len, dtype=np.int64) > 0
    dele = d > 0
    sub = ~dele & ~ins
    keep = (sub & (p >= S) & (p < E)) | (ins & ~dele & (p >= S - 1) & (p < E)) | (dele & (p + 1 < E) & (p + d >= S))
    return np.flatnonzero(keep).astype(np.int64)


def haplotype_states(index: GraphIndex, sites: np.ndarray, haplotypes: np.ndarray) -> np.ndarray:
    """-> uint8 [len(haplotypes), len(sites)]: the state of the haplotypes at the sites (bit k: ALT k + 1)"""
    sites, haplotypes = np.asarray(sites, dtype=np.int64), np.asarray(haplotypes, dtype=np.int64)
    out = np.zeros((len(haplotypes), len(sites)), dtype=np.uint8)
    if not len(sites) or not len(haplotypes):
        return out
    bits = np.asarray(index.alt_bits, dtype=np.uint64)[sites]                           # [n, 3, hw]
    used = np.arange(bits.shape[1])[None, :] < np.asarray(index.n_alts, dtype=np.int64)[sites][:, None]
    words = bits[:, :, haplotypes >> 6]                                                 # [n, 3, m]
    on = ((words >> (haplotypes & 63).astype(np.uint64)[None, None, :]) & np.uint64(1)).astype(np.uint8) * used[..., None]
    for k in range(bits.shape[1]):
        out |= (on[:, k, :].T << k).astype(np.uint8)
    return out


def _scan(dg: DeviceGraph, starts: np.ndarray, stops: np.ndarray, d_class, d_n, seed: int, key_bits: int, table_slots: int,
          scratch_bytes: int) -> bool:
    """gfm_graph_haplotype_classes over one graph into d_class int32 [n, H] / d_n int32 [n] -> True: the classes are
    verified, False: two allele combinations shared a key"""
    torch = _torch()
    n = len(starts)
    with torch.cuda.device(dg.device):
        status = torch.zeros(1, dtype=torch.int32, device=dg.device)
        nv.check(nv.lib().gfm_graph_haplotype_classes(
            dg._h, n, nv.ptr(starts) if n else None, nv.ptr(stops) if n else None, int(seed) & ((1 << 64) - 1), int(key_bits),
            int(table_slots), d_class.data_ptr() if n else None, d_n.data_ptr() if n else None, status.data_ptr(),
            int(scratch_bytes), _stream_ptr(None)))
        return int(status.item()) == 0


def _records(d_class, d_n, H: int, group_bits: Optional[np.ndarray], dev):
    """gfm_graph_haplotype_class_records -> (offsets int64 [R + 1], count, first int32 [K], group_counts int32 [K, G]) on
    the host.  The exclusive scan of the class counts is a torch cumsum."""
    torch = _torch()
    R = int(d_n.shape[0])
    G = 0 if group_bits is None else len(group_bits)
    with torch.cuda.device(dev):
        off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
        if R:
            torch.cumsum(d_n, 0, out=off[1:])
        K = int(off[-1].item())
        count = torch.empty(K, dtype=torch.int32, device=dev)
        first = torch.empty(K, dtype=torch.int32, device=dev)
        gc = torch.empty((K, G), dtype=torch.int32, device=dev)
        d_bits = torch.from_numpy(np.ascontiguousarray(group_bits).view(np.int64)).to(dev) if G else None
        if R:
            nv.check(nv.lib().gfm_graph_haplotype_class_records(
                R, H, d_class.data_ptr(), off.data_ptr(), d_bits.data_ptr() if G else None, G, count.data_ptr(), first.data_ptr(),
                gc.data_ptr() if G else None, _stream_ptr(None)))
        return off.cpu().numpy(), count.cpu().numpy(), first.cpu().numpy(), gc.cpu().numpy().reshape(K, G)


def _check_group_bits(group_bits, H: int) -> Optional[np.ndarray]:
    if group_bits is None:
        return None
    if hasattr(group_bits, "detach"):
        group_bits = group_bits.detach().cpu().numpy()
    group_bits = np.ascontiguousarray(group_bits)
    if group_bits.dtype == np.int64:
        group_bits = group_bits.view(np.uint64)
    hw = (H + 63) // 64
    if group_bits.dtype != np.uint64 or group_bits.ndim != 2 or (len(group_bits) and group_bits.shape[1] != hw):
        raise ValueError("group_bits: uint64 [groups, words of the haplotype bitsets]")
    if len(group_bits) > MAX_GROUPS:
        raise ValueError(f"{len(group_bits)} haplotype groups: at most {MAX_GROUPS} per call")
    return group_bits


def class_rows(graph, starts, stops, seed: int = 0, key_bits: int = 64, table_slots: int = 0, scratch_bytes: int = 0,
               group_bits=None):
    """The kernels on plain arrays: `graph` a DeviceGraph (or a GraphIndex, uploaded for the call), `starts` / `stops` int64
    [n] the regions, `group_bits` uint64 [G, hw] or None -> (class_of int32 [n, H], n_classes int32 [n], offsets int64 [n + 1],
    count int32 [K], first int32 [K], group_counts int32 [K, G]).  ONE seed: HashCollisionError on the first verdict that two
    allele combinations shared a key.  `key_bits` < 64 truncates the keys (a lab knob); `table_slots` (0 or a power of two in
    [64, 2048]) and `scratch_bytes` cut the device work; the result depends on none of them."""
    torch = _torch()
    own = not isinstance(graph, DeviceGraph)
    dg = DeviceGraph(graph) if own else graph
    try:
        if dg.index.alt_bits is None or int(dg.index.n_haplotypes) <= 0:
            raise ValueError(f"{dg.index.chrom}: the graph carries no haplotypes: haplotype classes need them")
        H = int(dg.index.n_haplotypes)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        stops = np.ascontiguousarray(stops, dtype=np.int64)
        if starts.shape != stops.shape or starts.ndim != 1:
            raise ValueError("starts and stops are one value per region")
        group_bits = _check_group_bits(group_bits, H)
        n = len(starts)
        with torch.cuda.device(dg.device):
            d_class = torch.empty((n, H), dtype=torch.int32, device=dg.device)
            d_n = torch.empty(n, dtype=torch.int32, device=dg.device)
            if not _scan(dg, starts, stops, d_class, d_n, seed, key_bits, table_slots, scratch_bytes):
                raise HashCollisionError(f"{dg.index.chrom}: two allele combinations of a region share a {key_bits}-bit key under "
                                         f"seed {seed}")
            off, count, first, gc = _records(d_class, d_n, H, group_bits, dg.device)
            return d_class.cpu().numpy(), d_n.cpu().numpy(), off, count, first, gc
    finally:
        if own:
            dg.close()


class HaplotypeClasses:
    """The classes of a region list (R regions, H haplotypes, K classes in all):
    region_names [R], haplotype_names [H];
    class_of      int32 [R, H]: the class of every haplotype;  n_classes int32 [R];
    offsets       int64 [R + 1]: the classes of region r are offsets[r] .. offsets[r + 1] - 1 of count / first / is_reference /
                  group_counts, class k of r at offsets[r] + k;
    count         int32 [K];  first int32 [K]: the representative (smallest member);  is_reference bool [K];
    group_names   [G];  group_counts int32 [K, G];
    indexes       per chromosome entry its GraphIndex (None for an entry without regions);
    entry         int64 [R]: the chromosome entry of every region;  spans int64 [R, 2]: its (S, E) as given."""

    def __init__(self, region_names, haplotype_names, class_of, n_classes, offsets, count, first, group_names, group_counts,
                 indexes, entry, spans):
        self.region_names = np.asarray(region_names, dtype=object)
        self.haplotype_names = list(haplotype_names)
        self.class_of = np.asarray(class_of, dtype=np.int32)
        self.n_classes = np.asarray(n_classes, dtype=np.int32)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.count = np.asarray(count, dtype=np.int32)
        self.first = np.asarray(first, dtype=np.int32)
        self.group_names = [str(g) for g in group_names]
        self.group_counts = np.asarray(group_counts, dtype=np.int32).reshape(len(self.count), len(self.group_names))
        self.indexes = list(indexes)
        self.entry = np.asarray(entry, dtype=np.int64)
        self.spans = np.asarray(spans, dtype=np.int64).reshape(len(self.region_names), 2)
        if self.class_of.shape != (len(self.region_names), len(self.haplotype_names)):
            raise ValueError(f"class_of of shape {self.class_of.shape} for {len(self.region_names)} regions and "
                             f"{len(self.haplotype_names)} haplotypes")
        self._states = None

    def __len__(self) -> int:
        return len(self.count)

    @property
    def class_region(self) -> np.ndarray:
        """int64 [K]: the region of every class"""
        return np.repeat(np.arange(len(self.n_classes), dtype=np.int64), np.diff(self.offsets))

    def _rep_states(self):
        """per region (its sites T(r), the states uint8 [classes of r, sites] of its representatives) -- built on the host,
        for the representatives only"""
        if self._states is None:
            out = []
            for r in range(len(self.region_names)):
                idx = self.indexes[int(self.entry[r])]
                sites = region_sites(idx, *self.spans[r].tolist())
                reps = self.first[self.offsets[r]:self.offsets[r + 1]]
                out.append((sites, haplotype_states(idx, sites, reps)))
            self._states = out
        return self._states

    @property
    def is_reference(self) -> np.ndarray:
        parts = [~(st != 0).any(axis=1) for _, st in self._rep_states()]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=bool)

    def alleles(self, region: int, k: int) -> List[Tuple[int, int, int]]:
        """-> [(entry, site, allele)] of the non-zero states of class k's representative, in (site, allele) order"""
        sites, st = self._rep_states()[region]
        e = int(self.entry[region])
        return [(e, int(s), a + 1) for s, v in zip(sites.tolist(), st[k].tolist()) for a in range(3) if (v >> a) & 1]

    def allele_strings(self) -> np.ndarray:
        """object [K]: per class its alleles as POS:REF>ALT joined with ';' ("" for the reference class), a site printed as
        hit_alleles prints it (graph_tables._site_columns)"""
        out = np.full(len(self.count), "", dtype=object)
        for r, (sites, st) in enumerate(self._rep_states()):
            if not len(sites) or not st.any():
                continue
            idx = self.indexes[int(self.entry[r])]
            ks, js, als = [], [], []
            for a in range(3):
                k, j = np.nonzero((st >> a) & 1)
                ks.append(k), js.append(j), als.append(np.full(len(k), a + 1, dtype=np.int64))
            k, j, al = np.concatenate(ks), np.concatenate(js), np.concatenate(als)
            order = np.lexsort((al, j, k))
            k, j, al = k[order], j[order], al[order]
            pos, refs, alts, _, _ = _site_columns(idx, sites[j], al)
            text = [f"{p}:{a}>{b}" for p, a, b in zip(pos.tolist(), refs, alts)]
            cut = np.flatnonzero(np.diff(k)) + 1
            base = int(self.offsets[r])
            for kk, lo, hi in zip(k[np.concatenate([[0], cut])].tolist(), np.concatenate([[0], cut]).tolist(),
                                  np.concatenate([cut, [len(k)]]).tolist()):
                out[base + kk] = ";".join(text[lo:hi])
        return out


def compute_haplotype_classes(graph, regions, debug: bool, args_obj, chrom_names=None,
                              haplotype_names: Optional[Sequence[str]] = None, haplotype_groups: Optional[Mapping] = None,
                              seed: int = 0, key_bits: int = 64, table_slots: int = 0, scratch_bytes: int = 0) -> HaplotypeClasses:
    """The haplotype classes of every region (see the module's docstring).  `graph` / `regions` as compute_haplotype_scores
    takes them -- a DeviceGraph or GraphIndex with its [(S, E)] list, or lists of both, one entry per chromosome (the
    chromosomes share one haplotype set) -- or a scan_graph manifest with regions None.  `haplotype_groups`: a mapping group
    name -> haplotype names or column indices, at most 64 (hit_alleles.read_haplotype_groups reads one from a panel file).
    A verdict that two allele combinations shared a key repeats the call with seed + 1, at most three seeds, then
    HashCollisionError.  `key_bits`, `table_slots`, `scratch_bytes`: class_rows'."""
    from .hit_alleles import _group_bits
    torch = _torch()
    require_single_gpu("the haplotype classes", "are", "a gather of the sharded class matrices")
    prep = prepare_graphs(graph, regions, chrom_names)
    H, names = _haplotype_set(prep, haplotype_names, "the haplotype class table")
    rows, region_names = _matrix_rows(prep)
    R = len(region_names)
    group_names, bits = _group_bits(haplotype_groups, names, H)
    n_entries = 1 + max((int(e.max()) for e in prep.entry_of if len(e)), default=-1)
    indexes: List[Optional[GraphIndex]] = [None] * n_entries
    entry = np.zeros(R, dtype=np.int64)
    spans = np.zeros((R, 2), dtype=np.int64)
    for gi, g in enumerate(prep.graphs):
        for e in np.unique(prep.entry_of[gi]).tolist():
            indexes[int(e)] = g.index
        entry[rows[gi]] = prep.entry_of[gi]
        spans[rows[gi], 0] = np.asarray(prep.spans[gi][0], dtype=np.int64)
        spans[rows[gi], 1] = np.asarray(prep.spans[gi][1], dtype=np.int64)
    dev = prep.graphs[0].device if prep.graphs else torch.device("cuda", torch.cuda.current_device())
    one = len(prep.graphs) == 1 and np.array_equal(rows[0], np.arange(R))
    for attempt in range(SEEDS_TRIED):
        with torch.cuda.device(dev):
            d_class = torch.empty((R, H), dtype=torch.int32, device=dev)
            d_n = torch.empty(R, dtype=torch.int32, device=dev)
            good = True
            for gi, g in enumerate(prep.graphs):
                starts = np.ascontiguousarray(prep.spans[gi][0], dtype=np.int64)
                stops = np.ascontiguousarray(prep.spans[gi][1], dtype=np.int64)
                if one:
                    good = _scan(g, starts, stops, d_class, d_n, seed + attempt, key_bits, table_slots, scratch_bytes)
                    break
                n = len(starts)
                part = torch.empty((n, H), dtype=torch.int32, device=dev)
                part_n = torch.empty(n, dtype=torch.int32, device=dev)
                good = _scan(g, starts, stops, part, part_n, seed + attempt, key_bits, table_slots, scratch_bytes)
                if not good:
                    break
                at = torch.from_numpy(np.ascontiguousarray(rows[gi])).to(dev)
                d_class[at] = part
                d_n[at] = part_n
            if not good:
                continue
            off, count, first, gc = _records(d_class, d_n, H, bits if len(group_names) else None, dev)
            return HaplotypeClasses(region_names, names, d_class.cpu().numpy(), d_n.cpu().numpy(), off, count, first, group_names,
                                    gc, indexes, entry, spans)
    raise HashCollisionError(f"two allele combinations of a region share a {key_bits}-bit key under each of the seeds "
                             f"{seed} .. {seed + SEEDS_TRIED - 1}")


class HaplotypeClassTable:
    """The class table of one motif: `classes` (shared by the motifs of a call), per class of `rows` (indices into the
    classes' K records, those with count >= min_haplotypes) the representative's motif numbers."""

    def __init__(self, motif_id: str, motif_alt_id: str, classes: HaplotypeClasses, rows: np.ndarray, best_score, best_pvalue,
                 start, stop, strand, log2_affinity, delta_log2_affinity):
        self.motif_id, self.motif_alt_id = motif_id, motif_alt_id
        self.classes = classes
        self.rows = np.asarray(rows, dtype=np.int64)
        self.best_score, self.best_pvalue = np.asarray(best_score, dtype=np.float64), np.asarray(best_pvalue, dtype=np.float64)
        self.start, self.stop = np.asarray(start, dtype=np.int64), np.asarray(stop, dtype=np.int64)
        self.strand = np.asarray(strand, dtype=object)
        self.log2_affinity = np.asarray(log2_affinity, dtype=np.float64)
        self.delta_log2_affinity = np.asarray(delta_log2_affinity, dtype=np.float64)

    def __len__(self) -> int:
        return len(self.rows)

    def to_frame(self) -> pd.DataFrame:
        """motif_id, motif_alt_id, sequence_name, class, haplotypes, frequency, one haplotypes_<GROUP> per group,
        representative, is_reference, alt_alleles, best_score, best_pvalue, start, stop, strand, log2_affinity,
        delta_log2_affinity -- a row per (region, class), regions in the caller's order, classes by number"""
        hc, k = self.classes, self.rows
        n = len(k)
        region = hc.class_region[k]
        H = len(hc.haplotype_names)
        data = {"motif_id": np.full(n, self.motif_id, dtype=object), "motif_alt_id": np.full(n, self.motif_alt_id, dtype=object),
                "sequence_name": hc.region_names[region] if n else np.zeros(0, dtype=object),
                "class": k - hc.offsets[region], "haplotypes": hc.count[k].astype(np.int64),
                "frequency": hc.count[k].astype(np.float64) / float(max(H, 1))}
        for g, name in enumerate(hc.group_names):
            data[f"haplotypes_{name}"] = hc.group_counts[k, g].astype(np.int64)
        names = np.asarray(hc.haplotype_names, dtype=object)
        data["representative"] = names[hc.first[k]] if n else np.zeros(0, dtype=object)
        data["is_reference"] = hc.is_reference[k]
        data["alt_alleles"] = hc.allele_strings()[k]
        data["best_score"], data["best_pvalue"] = self.best_score, self.best_pvalue
        data["start"], data["stop"], data["strand"] = self.start, self.stop, self.strand
        data["log2_affinity"], data["delta_log2_affinity"] = self.log2_affinity, self.delta_log2_affinity
        return pd.DataFrame(data)


def class_table(motif_id: str, motif_alt_id: str, classes: HaplotypeClasses, scores, affinity,
                min_haplotypes: int = 1) -> HaplotypeClassTable:
    """The table of one motif from the classes, the motif's HaplotypeScores and HaplotypeAffinity over the same regions: a
    class takes its representative's column of both matrices"""
    k = np.flatnonzero(classes.count >= int(min_haplotypes)).astype(np.int64)
    region = classes.class_region[k]
    rep = classes.first[k].astype(np.int64)
    la = affinity.log2_affinity[region, rep]
    return HaplotypeClassTable(motif_id, motif_alt_id, classes, k, scores.best_score[region, rep], scores.best_pvalue[region, rep],
                               scores.start[region, rep], scores.stop[region, rep], scores.strand[region, rep], la,
                               la - affinity.reference_log2_affinity[region])


def compute_haplotype_class_table_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                                       haplotype_names: Optional[Sequence[str]] = None,
                                       haplotype_groups: Optional[Mapping] = None, temperature: float = 1.0,
                                       min_haplotypes: int = 1, classes: Optional[HaplotypeClasses] = None,
                                       **knobs) -> List[HaplotypeClassTable]:
    """One HaplotypeClassTable per motif, in the order of `motifs`: a row per (region, class) with count >= min_haplotypes.
    The classes are computed ONCE for the set (or taken from `classes`); a class's motif numbers are its representative's
    column of compute_haplotype_scores_many (best_score, best_pvalue, start, stop, strand) and of
    compute_haplotype_affinity_many at `temperature` (log2_affinity; delta_log2_affinity against the reference column).
    `knobs`: seed, key_bits, table_slots, scratch_bytes of compute_haplotype_classes."""
    from .haplotype_affinity import compute_haplotype_affinity_many
    from .haplotype_scores import compute_haplotype_scores_many
    if int(min_haplotypes) < 1:
        raise ValueError(f"min_haplotypes {min_haplotypes}: it must be >= 1")
    if classes is None:
        classes = compute_haplotype_classes(graph, regions, debug, args_obj, chrom_names, haplotype_names, haplotype_groups,
                                            **knobs)
    hss = compute_haplotype_scores_many(motifs, graph, regions, debug, args_obj, chrom_names, haplotype_names)
    has = compute_haplotype_affinity_many(motifs, graph, regions, debug, args_obj, chrom_names, haplotype_names, temperature)
    return [class_table(m.motif_id, m.motif_name, classes, hs, ha, min_haplotypes) for m, hs, ha in zip(motifs, hss, has)]


def compute_haplotype_class_table(motif, graph, regions, debug: bool, args_obj, chrom_names=None,
                                  haplotype_names: Optional[Sequence[str]] = None, haplotype_groups: Optional[Mapping] = None,
                                  temperature: float = 1.0, min_haplotypes: int = 1, classes: Optional[HaplotypeClasses] = None,
                                  **knobs) -> HaplotypeClassTable:
    """The class table of `motif` (compute_haplotype_class_table_many for one motif)"""
    return compute_haplotype_class_table_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_names,
                                              haplotype_groups, temperature, min_haplotypes, classes, **knobs)[0]


def write_haplotype_classes(table: HaplotypeClassTable, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_haplotype_classes.tsv (grafimo_haplotype_classes_<motif_id>.tsv for one of several motifs) in the directory
    write_results uses for this motif -> the path written.  `out`: a text stream to write to instead (-f: stdout)."""
    return write_frame(table, out if out is not None else table_path(CLASSES_FILE, args_obj, motif, motif_num))


def print_haplotype_classes(table: HaplotypeClassTable) -> None:
    """-f: the table on stdout instead of a file"""
    write_haplotype_classes(table, None, 1, None, out=sys.stdout)


def write_haplotype_class_members(classes: HaplotypeClasses, args_obj, out=None) -> Optional[str]:
    """grafimo_haplotype_class_members.tsv, one file per call (the classes do not depend on the motif): in the -o directory,
    or with the default output directory in grafimo_out_<pid>_classes -> the path written.  `out`: a binary stream to write
    to instead.  Wide: sequence_name, then one column per haplotype holding its class in the region."""
    top = int(classes.class_of.max()) if classes.class_of.size else 0
    tab, ln = text_table([str(k).encode() for k in range(top + 1)])
    return write_wide(out if out is not None else table_path(MEMBERS_FILE, args_obj, tag="classes"),
                      ["sequence_name"] + list(classes.haplotype_names), "", classes.region_names, classes.class_of, tab, ln)


def print_haplotype_class_members(classes: HaplotypeClasses) -> None:
    """-f: the matrix on stdout instead of a file"""
    sys.stdout.flush()
    write_haplotype_class_members(classes, None, out=sys.stdout.buffer)
