"""Hit-pair table: which motif hits lie close to each other on the SAME haplotypes.

The question a variation graph answers and a linear scan cannot: two report rows that each have carriers need not share
one.  For a motif set (one or more motifs, any mix of widths, a motif possibly twice), the rows are those of the reports
compute_results_from_graph gives per motif for the same arguments.  Every row has its region listing r (the index into the
caller's flattened region list; a region listed twice is two listings), its interval lo = min(start, stop),
hi = max(start, stop) in the coordinates the report prints, and its carrier set C, the set whose size is
haplotype_frequency.  For two rows
  gap = max(lo_a, lo_b) - min(hi_a, hi_b): the reference bases between them, negative when they overlap by that many.
A PAIR is two distinct rows of the same region listing -- of one motif or of two -- with min_gap <= gap <= max_gap and
joint = popcount(C_a & C_b) > 0.  Rows without carriers (--recomb rows of frequency 0) never pair.  Rows are ordered by the
key (r, lo, hi, motif index, report row index); in a pair `a` is the row of the smaller key, and the table lists its pairs
by (key(a), key(b)): the order is part of the contract.

The gap is measured in REPORT coordinates, i.e. on the reference.  Inside and across insertions and deletions it is not
the distance on the haplotype's own sequence: two rows on either side of a deletion a haplotype carries are closer on that
haplotype than their gap says, two rows around an insertion further apart.

The join runs on the GPU: gfm_hit_pairs (HIP, grafimo_amd/csrc/hit_pairs.hip), a banded, segmented self-join over the rows
sorted by (region listing, lo) with a bitset intersection per candidate.  The carrier sets come from
compute_hit_alleles_many(..., carriers=True), so the selection is the report's own.  The default gap (0, 50) --
non-overlapping sites at most 50 reference bases apart -- is a product default, not a measured quantity.
"""
import ctypes
import sys
from typing import List, Mapping, Optional, Sequence

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _stream_ptr, _torch
from .graph_tables import _haplotype_set, _matrix_rows, prepare_graphs, require_single_gpu, table_path, write_frame
from .hit_alleles import MAX_GROUPS, HitAlleles, compute_hit_alleles_many

SIDE_COLUMNS = ["motif_id", "motif_alt_id", "start", "stop", "strand", "score", "p-value", "matched_sequence",
                "haplotype_frequency"]
PAIRS_FILE = "grafimo_hit_pairs"
_COORD_LIMIT = 1 << 61


def _as_numpy(x, dtype):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def pair_rows(group, lo, hi, masks, min_gap: int, max_gap: int, group_bits=None, device=None, tie: Sequence = (),
              max_pairs: Optional[int] = None, n_haplotypes: Optional[int] = None):
    """The thin wrapper of gfm_hit_pairs.  n rows: `group` (int32: rows pair inside a group only), `lo` <= `hi` (int64),
    `masks` uint64 [n, hw] (bits beyond the last haplotype clear); `group_bits` uint64 [G, hw], G <= 64; numpy arrays or
    torch tensors, in any order.  The rows are sorted here by the key (group, lo, hi, *tie, index) -- `tie`: further
    integer key columns of the caller -- and the pairs come back in the caller's indices:
    -> (a, b, joint, group_counts): int64 [P], int64 [P], int32 [P], int32 [P, G]; key(a) < key(b), the pairs ascending by
    (key(a), key(b)).  More than `max_pairs` pairs: OverflowError naming the count, before anything is allocated for them.
    `n_haplotypes`: the number of haplotypes H the bitsets stand for, (hw - 1) * 64 < H <= hw * 64; bits beyond it are refused
    (the kernel counts every bit it is given)."""
    torch = _torch()
    group = _as_numpy(group, np.int32)
    lo, hi = _as_numpy(lo, np.int64), _as_numpy(hi, np.int64)
    n = len(group)
    if min_gap > max_gap:
        raise ValueError(f"min_gap {min_gap} > max_gap {max_gap}")
    if lo.shape != (n,) or hi.shape != (n,):
        raise ValueError("group, lo and hi are one value per row")
    masks = _as_numpy(masks, None)
    if masks.dtype == np.int64:
        masks = masks.view(np.uint64)
    if masks.dtype != np.uint64 or masks.ndim != 2 or masks.shape[0] != n or masks.shape[1] < 1:
        raise ValueError("masks: uint64 [rows, words], at least one word")
    hw = masks.shape[1]
    if n_haplotypes is not None:
        H = int(n_haplotypes)
        if not (hw - 1) * 64 < H <= hw * 64:
            raise ValueError(f"{H} haplotypes do not fill {hw} words")
        if H & 63 and n and (masks[:, -1] >> np.uint64(H & 63)).any():
            raise ValueError("a carrier set has bits beyond the last haplotype")
    if (lo > hi).any():
        raise ValueError("a row with lo > hi")
    if n and (max(abs(int(lo.min())), abs(int(hi.max()))) >= _COORD_LIMIT or max(abs(min_gap), abs(max_gap)) >= _COORD_LIMIT):
        raise ValueError("coordinates and gaps stay below 2^61")
    G = 0
    if group_bits is not None:
        group_bits = _as_numpy(group_bits, None)
        if group_bits.dtype == np.int64:
            group_bits = group_bits.view(np.uint64)
        if group_bits.dtype != np.uint64 or group_bits.ndim != 2 or (len(group_bits) and group_bits.shape[1] != hw):
            raise ValueError("group_bits: uint64 [groups, words of the masks]")
        G = len(group_bits)
        if G > MAX_GROUPS:
            raise ValueError(f"{G} haplotype groups: at most {MAX_GROUPS} per call")
    tie = [_as_numpy(t, np.int64) for t in tie]
    if any(t.shape != (n,) for t in tie):
        raise ValueError("a tie-break key is one value per row")
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros((0, G), np.int32))
    if n < 2:
        return empty
    order = np.lexsort(tuple([np.arange(n)] + tie[::-1] + [hi, lo, group]))
    if np.array_equal(order, np.arange(n)):
        order = None
    else:
        group, lo, hi, masks = group[order], lo[order], hi[order], masks[order]
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        sp = _stream_ptr(None)
        d_group = torch.from_numpy(group).to(dev)
        d_lo, d_hi = torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
        d_masks = torch.from_numpy(np.ascontiguousarray(masks).view(np.int64)).to(dev)
        d_gbits = torch.from_numpy(np.ascontiguousarray(group_bits).view(np.int64)).to(dev) if G else None
        d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        total = ctypes.c_int64()

        def call(cap, d_b, d_joint, d_gc, flags):
            nv.check(nv.lib().gfm_hit_pairs(d_group.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr(), d_masks.data_ptr(), n, hw,
                                            int(min_gap), int(max_gap), G, d_gbits.data_ptr() if G else None, d_off.data_ptr(), cap,
                                            d_b.data_ptr() if d_b is not None else None,
                                            d_joint.data_ptr() if d_joint is not None else None,
                                            d_gc.data_ptr() if d_gc is not None else None, flags, ctypes.byref(total), sp))

        call(0, None, None, None, 0)                                  # count first ...
        P = int(total.value)
        if max_pairs is not None and P > max_pairs:
            raise OverflowError(f"{P} hit pairs, more than max_pairs = {max_pairs}: narrow the gap, raise the threshold's "
                                "strictness or raise max_pairs")
        if P == 0:
            return empty
        d_b = torch.empty(P, dtype=torch.int32, device=dev)           # ... then allocate
        d_joint = torch.empty(P, dtype=torch.int32, device=dev)
        d_gc = torch.empty((P, G), dtype=torch.int32, device=dev) if G else None
        call(P, d_b, d_joint, d_gc, nv.GFM_PAIRS_HAVE_OFFSETS)
        off = d_off.cpu().numpy()
        b = d_b.cpu().numpy().astype(np.int64)
        joint = d_joint.cpu().numpy()
        gc = d_gc.cpu().numpy() if G else np.zeros((P, 0), np.int32)
    a = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    if order is not None:
        a, b = order[a], order[b]
    return a, b, joint, gc


class HitPairs:
    """The pair table of a motif set:
    tables        per motif its HitAlleles (carriers kept, row_region filled): tables[m].report is motif m's report;
    region        int64 [P]: the region listing of the pair;  region_names [R]: sequence_name per listing;
    motif_a, row_a, motif_b, row_b  int64 [P]: motif indices and row indices into the per-motif reports;
    gap           int64 [P];  co_haplotypes int32 [P];
    group_names   [G];  group_counts int32 [P, G];
    reference     bool [P]: both rows are `ref`."""

    def __init__(self, tables: Sequence[HitAlleles], region, motif_a, row_a, motif_b, row_b, gap, co_haplotypes, group_names,
                 group_counts, reference, region_names):
        self.tables = list(tables)
        self.region = np.asarray(region, dtype=np.int64)
        self.motif_a, self.row_a = np.asarray(motif_a, dtype=np.int64), np.asarray(row_a, dtype=np.int64)
        self.motif_b, self.row_b = np.asarray(motif_b, dtype=np.int64), np.asarray(row_b, dtype=np.int64)
        self.gap = np.asarray(gap, dtype=np.int64)
        self.co_haplotypes = np.asarray(co_haplotypes, dtype=np.int32)
        self.group_names = [str(g) for g in group_names]
        self.group_counts = np.asarray(group_counts, dtype=np.int32).reshape(len(self.region), len(self.group_names))
        self.reference = np.asarray(reference, dtype=bool)
        self.region_names = np.asarray(region_names, dtype=object)

    def __len__(self) -> int:
        return len(self.region)

    def _side(self, motif, row, column: str) -> np.ndarray:
        cols = [t.report[column].to_numpy() for t in self.tables]
        kind = object if any(c.dtype == object for c in cols) or not cols else np.result_type(*cols)
        out = np.empty(len(motif), dtype=kind)
        for m, c in enumerate(cols):
            sel = motif == m
            out[sel] = c[row[sel]]
        return out

    def to_frame(self) -> pd.DataFrame:
        """sequence_name; motif_id, motif_alt_id, start, stop, strand, score, p-value, matched_sequence, haplotype_frequency
        of row a (suffix _a), then of row b (_b); gap; co_haplotypes; one haplotypes_<GROUP> column per group; reference"""
        data = {"sequence_name": self.region_names[self.region] if len(self) else np.zeros(0, dtype=object)}
        for suffix, motif, row in (("_a", self.motif_a, self.row_a), ("_b", self.motif_b, self.row_b)):
            for c in SIDE_COLUMNS:
                data[c + suffix] = self._side(motif, row, c)
        data["gap"] = self.gap
        data["co_haplotypes"] = self.co_haplotypes.astype(np.int64)
        for g, name in enumerate(self.group_names):
            data[f"haplotypes_{name}"] = self.group_counts[:, g].astype(np.int64)
        data["reference"] = np.where(self.reference, "ref", "non.ref").astype(object)
        return pd.DataFrame(data)


def compute_hit_pairs(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                      haplotype_names: Optional[Sequence[str]] = None, haplotype_groups: Optional[Mapping] = None,
                      min_gap: int = 0, max_gap: int = 50, max_pairs: int = 1 << 26) -> HitPairs:
    """The hit-pair table of the motif set (see the module's docstring).  `graph` / `regions`, args_obj, `chrom_names`,
    `haplotype_names` and `haplotype_groups` as compute_hit_alleles_many takes them.  A graph without haplotype bitsets or
    graphs of different haplotype sets: ValueError; more than `max_pairs` pairs: OverflowError naming the count."""
    require_single_gpu("the hit-pair table", "is", "a gather of the sharded tables")
    if int(min_gap) > int(max_gap):
        raise ValueError(f"min_gap {min_gap} > max_gap {max_gap}")
    prep = prepare_graphs(graph, regions, chrom_names)
    _haplotype_set(prep, haplotype_names, "the hit-pair table")         # (the refusals, before any pass runs)
    region_names = _matrix_rows(prep)[1]
    tables = compute_hit_alleles_many(motifs, graph, regions, debug, args_obj, chrom_names, haplotype_names, haplotype_groups,
                                      carriers=True)
    group_names = tables[0].group_names if tables else []
    H = len(tables[0].haplotype_names) if tables else 0
    hw = (H + 63) // 64
    from .hit_alleles import _group_bits
    bits = _group_bits(haplotype_groups, tables[0].haplotype_names, H)[1] if tables else np.zeros((0, hw), np.uint64)
    motif_of, row_of, r_of, lo, hi, masks, is_ref = [], [], [], [], [], [], []
    for m, t in enumerate(tables):
        n = len(t)
        start, stop = t.report["start"].to_numpy(np.int64), t.report["stop"].to_numpy(np.int64)
        keep = np.flatnonzero(t.carrier_bits.any(axis=1)) if n else np.zeros(0, np.int64)      # rows without carriers never pair
        motif_of.append(np.full(len(keep), m, np.int64))
        row_of.append(keep.astype(np.int64))
        r_of.append(t.row_region[keep])
        lo.append(np.minimum(start, stop)[keep])
        hi.append(np.maximum(start, stop)[keep])
        masks.append(t.carrier_bits[keep].reshape(len(keep), hw))
        is_ref.append((t.report["reference"].to_numpy() == "ref")[keep])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)      # noqa: E731
    motif_of, row_of, r_of = cat(motif_of, np.int64), cat(row_of, np.int64), cat(r_of, np.int64)
    lo, hi, is_ref = cat(lo, np.int64), cat(hi, np.int64), cat(is_ref, bool)
    masks = np.concatenate(masks, axis=0) if masks else np.zeros((0, max(hw, 1)), np.uint64)
    if len(r_of) and int(r_of.max()) >= 2 ** 31:
        raise ValueError("more than 2^31 region listings")
    a, b, joint, gc = pair_rows(r_of.astype(np.int32), lo, hi, masks, int(min_gap), int(max_gap), bits if len(group_names) else None,
                                tie=(motif_of, row_of), max_pairs=max_pairs, n_haplotypes=H)
    gap = np.maximum(lo[a], lo[b]) - np.minimum(hi[a], hi[b])
    return HitPairs(tables, r_of[a], motif_of[a], row_of[a], motif_of[b], row_of[b], gap, joint, group_names, gc,
                    is_ref[a] & is_ref[b], region_names)


def write_hit_pairs(hp: HitPairs, args_obj, out=None) -> Optional[str]:
    """grafimo_hit_pairs.tsv, one file per call: in the -o directory, or with the default output directory in
    grafimo_out_<pid>_pairs -> the path written.  `out`: a text stream to write to instead (-f: stdout)."""
    return write_frame(hp, out if out is not None else table_path(PAIRS_FILE, args_obj, tag="pairs"))


def print_hit_pairs(hp: HitPairs) -> None:
    """-f: the table on stdout instead of a file"""
    write_hit_pairs(hp, None, out=sys.stdout)
