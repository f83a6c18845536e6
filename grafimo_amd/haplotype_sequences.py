"""Haplotype sequences: for every region the DISTINCT sequences the panel spells in it -- its VERSIONS --, each with its
bases, its count, its counts per group and the classes (haplotype_classes) that spell it.  Where the class table groups the
haplotypes by their ALLELES, this table groups them by their BASES: two classes are one version when their bytes are equal (a
second insertion at an anchor whose first insertion is the one read, a site under a deletion the class carries).

THE RULE (tests/variant_bruteforce.py spell; include/grafimo_hip.h states it for the library).  Haplotype h spells one
sequence over the chromosome by walking the reference: at a position the substitution it carries replaces the base; the first
insertion in site order it carries at that anchor is read behind the anchor, later ones at that anchor are not; if no
insertion was read there, the first deletion it carries at that anchor jumps over its span; every site anchored on a
jumped-over base is ignored.  Every spelled base has a coordinate -- its own reference position, or its anchor's if it was
inserted -- and an inserted flag.  The region sequence of h in [S, E) clipped to the chromosome is the contiguous stretch of
spelled bases with coord + inserted >= S and coord < E: exactly the bases a report row of the region can contain (start in
[S, E), stop <= E).  Haplotype -1 is the reference.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_hapsequences.hpp): a measure pass, a fill pass that writes the bases and a
64-bit content key per sequence, and a verification of every sequence against the one it is grouped with -- the result is
exact, a key shared by two different sequences is detected (the call is repeated with another seed, then
HashCollisionError), never silently wrong.  Only one haplotype per class is spelled, and the reference of every region.
"""
import sys
from typing import Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import DeviceGraph, _stream_ptr, _torch
from .grafimo_errors import HashCollisionError
from .graph_tables import _haplotype_set, _matrix_rows, prepare_graphs, require_single_gpu, table_path, write_frame

FASTA_FILE = "grafimo_haplotype_sequences"
VERSIONS_FILE = "grafimo_haplotype_sequence_versions"
SEEDS_TRIED = 3
_NO_FIRST = np.iinfo(np.int32).max


def _spell(dg: DeviceGraph, starts: np.ndarray, stops: np.ndarray, seq_region: np.ndarray, seq_hap: np.ndarray,
           coordinates: bool, seed: int, key_bits: int, max_bytes: Optional[int]):
    """gfm_graph_haplotype_sequences over one graph, count first, then fill -> device tensors (lengths int32 [n], offsets int64
    [n + 1], bases uint8 [total], coord int32 [total] or None, keys int64 [n] holding the uint64 keys' bits)"""
    torch = _torch()
    lib = nv.lib()
    n, R = len(seq_region), len(starts)
    with torch.cuda.device(dg.device):
        d_region = torch.from_numpy(np.ascontiguousarray(seq_region, dtype=np.int32)).to(dg.device)
        d_hap = torch.from_numpy(np.ascontiguousarray(seq_hap, dtype=np.int32)).to(dg.device)
        d_len = torch.zeros(n, dtype=torch.int32, device=dg.device)
        off = torch.zeros(n + 1, dtype=torch.int64, device=dg.device)
        keys = torch.zeros(n, dtype=torch.int64, device=dg.device)
        total = nv.c_i64(0)
        args = (dg._h, R, nv.ptr(starts) if R else None, nv.ptr(stops) if R else None, n, d_region.data_ptr() if n else None,
                d_hap.data_ptr() if n else None, d_len.data_ptr() if n else None)
        seed, stream = int(seed) & ((1 << 64) - 1), _stream_ptr(None)
        nv.check(lib.gfm_graph_haplotype_sequences(*args, None, 0, None, None, seed, int(key_bits), None, 0, total, stream))
        total = int(total.value)
        if max_bytes is not None and total > int(max_bytes):
            raise ValueError(f"{dg.index.chrom}: the sequences asked for hold {total} bases, more than max_bytes = {int(max_bytes)}: "
                             "ask for fewer regions or haplotypes at a time, or raise max_bytes")
        if n:
            torch.cumsum(d_len, 0, out=off[1:])
        # (a byte more than the total: the fill pass is asked for by a d_bases that is not NULL, also when no base is spelled)
        bases = torch.empty(total + 1, dtype=torch.uint8, device=dg.device)
        coord = torch.empty(total + 1, dtype=torch.int32, device=dg.device) if coordinates else None
        if n:
            nv.check(lib.gfm_graph_haplotype_sequences(*args, off.data_ptr(), total, bases.data_ptr(),
                                                       coord.data_ptr() if coordinates else None, seed, int(key_bits),
                                                       keys.data_ptr(), nv.GFM_SEQS_HAVE_LENGTHS, None, stream))
        return d_len, off, bases[:total], coord[:total] if coordinates else None, keys


def _check_pairs(starts, stops, seq_region, seq_hap):
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    stops = np.ascontiguousarray(stops, dtype=np.int64)
    if starts.shape != stops.shape or starts.ndim != 1:
        raise ValueError("starts and stops are one value per region")
    seq_region = np.ascontiguousarray(seq_region, dtype=np.int64)
    seq_hap = np.ascontiguousarray(seq_hap, dtype=np.int64)
    if seq_region.shape != seq_hap.shape or seq_region.ndim != 1:
        raise ValueError("seq_region and seq_hap are one value per sequence")
    for name, v in (("seq_region", seq_region), ("seq_hap", seq_hap)):
        if len(v) and (v.min() < -(1 << 31) or v.max() >= (1 << 31)):
            raise ValueError(f"{name}: values beyond int32")
    return starts, stops, seq_region.astype(np.int32), seq_hap.astype(np.int32)


def spell_rows(graph, starts, stops, seq_region, seq_hap, coordinates: bool = False, seed: int = 0, key_bits: int = 64):
    """The kernels on plain arrays, one chromosome: `graph` a DeviceGraph (or a GraphIndex, uploaded for the call), `starts` /
    `stops` int64 [R] the regions, `seq_region` / `seq_hap` [n] the (region, haplotype) pairs to spell, haplotype -1 the
    reference -> (lengths int32 [n], offsets int64 [n + 1], bases uint8 [total], coord int32 [total] or None, keys uint64 [n]).
    coord: the coordinate of every base, ~coordinate for an inserted base.  A pair out of range, a region that ends before it
    starts or key_bits outside 1 .. 64 raise; a graph without haplotypes spells haplotype -1 only."""
    own = not isinstance(graph, DeviceGraph)
    dg = DeviceGraph(graph) if own else graph
    try:
        starts, stops, seq_region, seq_hap = _check_pairs(starts, stops, seq_region, seq_hap)
        d_len, off, bases, coord, keys = _spell(dg, starts, stops, seq_region, seq_hap, coordinates, seed, key_bits, None)
        return (d_len.cpu().numpy(), off.cpu().numpy(), bases.cpu().numpy(), coord.cpu().numpy() if coord is not None else None,
                keys.cpu().numpy().view(np.uint64))
    finally:
        if own:
            dg.close()


def group_by_key(region: np.ndarray, length: np.ndarray, key: np.ndarray) -> np.ndarray:
    """-> same_as int32 [n]: per item the smallest index among the items of its region with its (length, key) -- what the
    device then verifies byte for byte"""
    region, length = np.asarray(region, dtype=np.int64), np.asarray(length, dtype=np.int64)
    key = np.asarray(key).astype(np.uint64)
    n = len(region)
    if not n:
        return np.zeros(0, dtype=np.int32)
    order = np.lexsort((np.arange(n), key, length, region))
    r, ln, k = region[order], length[order], key[order]
    head = np.concatenate([[True], (r[1:] != r[:-1]) | (ln[1:] != ln[:-1]) | (k[1:] != k[:-1])])
    same = np.empty(n, dtype=np.int32)
    same[order] = order[np.flatnonzero(head)][np.cumsum(head) - 1]      # (indices ascend inside a group: the head is the smallest)
    return same


def number_versions(same_as: np.ndarray, region: np.ndarray, count: np.ndarray, first: np.ndarray, n_regions: int):
    """The versions of grouped items: item n belongs to the group of item same_as[n] (a group's items share a region); `count`
    and `first` are an item's haplotypes and its smallest member (a reference item: count 0).  A version is a group of count > 0;
    versions are numbered per region by count descending, then by smallest member.
    -> (version_of_item int32 [n], -1 for the items of a group without haplotypes; n_versions int32 [n_regions]; head int64 [V]:
    per version, in (region, number) order, the item it is spelled by (its smallest index); v_count, v_first int64 [V])"""
    same_as, region = np.asarray(same_as, dtype=np.int64), np.asarray(region, dtype=np.int64)
    count, first = np.asarray(count, dtype=np.int64), np.asarray(first, dtype=np.int64)
    heads, inv = np.unique(same_as, return_inverse=True)
    inv = inv.reshape(-1)
    g_count = np.zeros(len(heads), dtype=np.int64)
    np.add.at(g_count, inv, count)
    g_first = np.full(len(heads), np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(g_first, inv, np.where(count > 0, first, np.iinfo(np.int64).max))
    g_region = region[heads] if len(heads) else np.zeros(0, dtype=np.int64)
    live = g_count > 0
    order = np.lexsort((g_first, -g_count, g_region))
    order = order[live[order]]
    n_versions = np.bincount(g_region[order], minlength=int(n_regions)).astype(np.int32)
    base = np.concatenate([[0], np.cumsum(n_versions)])[:-1]
    number = np.arange(len(order), dtype=np.int64) - base[g_region[order]]
    g_number = np.full(len(heads), -1, dtype=np.int64)
    g_number[order] = number
    return g_number[inv].astype(np.int32), n_versions, heads[order], g_count[order], g_first[order]


class HaplotypeSequences:
    """The versions of a region list (R regions, H haplotypes, K classes and V versions in all):
    classes            the HaplotypeClasses the versions are made of;
    version_of_class   int32 [K]: the version, in its region, of every class row;
    version_of         int32 [R, H]: the version of every haplotype;  n_versions int32 [R];
    offsets            int64 [R + 1]: the versions of region r are offsets[r] .. offsets[r + 1] - 1 of the per-version arrays,
                       version k of r at offsets[r] + k;
    count              int32 [V];  first int32 [V]: the representative (smallest member);  group_counts int32 [V, G];
    length             int32 [V];  is_reference bool [V]: its bytes equal the reference's region sequence;
    seq_offsets        int64 [V + 1], bases uint8: the bases of version v are bases[seq_offsets[v] : seq_offsets[v + 1]];
    coord              int32 like bases, or None: per base its coordinate, ~coordinate for an inserted base;
    region_names [R], haplotype_names [H], group_names [G]."""

    def __init__(self, classes, version_of_class, n_versions, offsets, count, first, group_counts, length, is_reference, seq_offsets,
                 bases, coord=None):
        self.classes = classes
        self.version_of_class = np.asarray(version_of_class, dtype=np.int32)
        self.n_versions = np.asarray(n_versions, dtype=np.int32)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.count = np.asarray(count, dtype=np.int32)
        self.first = np.asarray(first, dtype=np.int32)
        self.group_counts = np.asarray(group_counts, dtype=np.int32).reshape(len(self.count), len(classes.group_names))
        self.length = np.asarray(length, dtype=np.int32)
        self.is_reference = np.asarray(is_reference, dtype=bool)
        self.seq_offsets = np.asarray(seq_offsets, dtype=np.int64)
        self.bases = np.asarray(bases, dtype=np.uint8)
        self.coord = None if coord is None else np.asarray(coord, dtype=np.int32)
        if len(self.version_of_class) != len(classes.count) or len(self.offsets) != len(classes.region_names) + 1:
            raise ValueError("the versions do not fit the classes")
        R = len(classes.region_names)
        self.version_of = (self.version_of_class[classes.offsets[:-1, None] + classes.class_of] if R and classes.class_of.shape[1]
                           else np.zeros(classes.class_of.shape, dtype=np.int32))

    region_names = property(lambda self: self.classes.region_names)
    haplotype_names = property(lambda self: self.classes.haplotype_names)
    group_names = property(lambda self: self.classes.group_names)

    def __len__(self) -> int:
        return len(self.count)

    @property
    def version_region(self) -> np.ndarray:
        """int64 [V]: the region of every version"""
        return np.repeat(np.arange(len(self.n_versions), dtype=np.int64), np.diff(self.offsets))

    def _row(self, region: int, k: int) -> int:
        if not 0 <= k < int(self.n_versions[region]):
            raise IndexError(f"region {region} has {int(self.n_versions[region])} versions, not a version {k}")
        return int(self.offsets[region]) + k

    def sequence(self, region: int, k: int) -> bytes:
        v = self._row(region, k)
        return self.bases[self.seq_offsets[v]:self.seq_offsets[v + 1]].tobytes()

    def coordinates(self, region: int, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """-> (coordinate int64 [length], inserted bool [length]) of the version's bases (computed with coordinates=True)"""
        if self.coord is None:
            raise ValueError("the sequences were computed without coordinates (coordinates=True keeps them)")
        v = self._row(region, k)
        c = self.coord[self.seq_offsets[v]:self.seq_offsets[v + 1]].astype(np.int64)
        return np.where(c < 0, ~c, c), c < 0

    def classes_of(self, region: int, k: int) -> np.ndarray:
        """int64: the classes of the region that spell version k, ascending"""
        self._row(region, k)
        a, b = int(self.classes.offsets[region]), int(self.classes.offsets[region + 1])
        return np.flatnonzero(self.version_of_class[a:b] == k).astype(np.int64)

    def _representative_class(self) -> np.ndarray:
        """int64 [V]: the class row (of the classes' K) of every version's representative"""
        hc = self.classes
        region = self.version_region
        return hc.offsets[region] + hc.class_of[region, self.first] if len(region) else np.zeros(0, dtype=np.int64)

    def class_strings(self) -> np.ndarray:
        """object [V]: the classes of every version joined with ';'"""
        out = np.full(len(self.count), "", dtype=object)
        hc = self.classes
        for r in range(len(self.n_versions)):
            voc = self.version_of_class[hc.offsets[r]:hc.offsets[r + 1]]
            for k in range(int(self.n_versions[r])):
                out[int(self.offsets[r]) + k] = ";".join(str(c) for c in np.flatnonzero(voc == k).tolist())
        return out

    def to_frame(self) -> pd.DataFrame:
        """sequence_name, version, haplotypes, frequency, one haplotypes_<GROUP> per group, representative, is_reference, length,
        classes, alt_alleles (the representative's, a site printed as hit_alleles prints it) -- a row per (region, version),
        regions in the caller's order, versions by number"""
        hc = self.classes
        n = len(self.count)
        region = self.version_region
        H = len(hc.haplotype_names)
        data = {"sequence_name": hc.region_names[region] if n else np.zeros(0, dtype=object),
                "version": np.arange(n, dtype=np.int64) - self.offsets[region], "haplotypes": self.count.astype(np.int64),
                "frequency": self.count.astype(np.float64) / float(max(H, 1))}
        for g, name in enumerate(hc.group_names):
            data[f"haplotypes_{name}"] = self.group_counts[:, g].astype(np.int64)
        names = np.asarray(hc.haplotype_names, dtype=object)
        data["representative"] = names[self.first] if n else np.zeros(0, dtype=object)
        data["is_reference"] = self.is_reference
        data["length"] = self.length.astype(np.int64)
        data["classes"] = self.class_strings()
        data["alt_alleles"] = hc.allele_strings()[self._representative_class()] if n else np.zeros(0, dtype=object)
        return pd.DataFrame(data)


def _assemble(classes, pair_class, pair_region, lengths, offsets, bases, coord, same_as) -> HaplotypeSequences:
    """the table from the spelled pairs of all graphs (host arrays; pair_class: the class row of a pair, -1 for a region's
    reference; same_as: verified)"""
    R = len(classes.region_names)
    ref = pair_class < 0
    at = np.where(ref, 0, pair_class)
    count = np.where(ref, 0, classes.count[at]).astype(np.int64)
    first = np.where(ref, _NO_FIRST, classes.first[at]).astype(np.int64)
    version_of_item, n_versions, head, v_count, v_first = number_versions(same_as, pair_region, count, first, R)
    V = len(head)
    v_off = np.concatenate([[0], np.cumsum(n_versions)]).astype(np.int64)
    row = v_off[pair_region] + version_of_item                          # the version row of every item (where it has one)
    voc = np.full(len(classes.count), -1, dtype=np.int32)
    voc[pair_class[~ref]] = version_of_item[~ref]
    G = len(classes.group_names)
    gc = np.zeros((V, G), dtype=np.int64)
    if G and (~ref).any():
        np.add.at(gc, row[~ref], classes.group_counts[pair_class[~ref]])
    is_ref = np.zeros(V, dtype=bool)
    is_ref[row[ref & (version_of_item >= 0)]] = True
    length = lengths[head].astype(np.int64)
    seq_off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    take = np.repeat(offsets[head] - seq_off[:-1], length) + np.arange(int(seq_off[-1]), dtype=np.int64)
    return HaplotypeSequences(classes, voc, n_versions, v_off, v_count, v_first, gc, length, is_ref, seq_off, bases[take],
                              None if coord is None else coord[take])


def _class_pairs(classes, rows):
    """the pairs one graph spells: `rows` the caller's row of each of its regions -> (seq_region int32: the graph's own region
    index, seq_hap int32, pair_class int64: the class row, -1 for a reference, pair_region int64: the caller's row) -- per
    region its classes' representatives in class order, then the reference"""
    r = np.asarray(rows, dtype=np.int64)
    k = (classes.offsets[r + 1] - classes.offsets[r]).astype(np.int64)
    local = np.repeat(np.arange(len(r), dtype=np.int64), k + 1)
    within = np.arange(len(local), dtype=np.int64) - np.repeat(np.concatenate([[0], np.cumsum(k + 1)])[:-1], k + 1)
    is_ref = within == k[local]
    pair_class = np.where(is_ref, -1, classes.offsets[r[local]] + within)
    hap = np.where(is_ref, -1, classes.first[np.where(is_ref, 0, pair_class)])
    return local.astype(np.int32), hap.astype(np.int32), pair_class.astype(np.int64), r[local]


def compute_haplotype_sequences(graph, regions, debug: bool, args_obj, chrom_names=None,
                                haplotype_names: Optional[Sequence[str]] = None, haplotype_groups: Optional[Mapping] = None,
                                classes=None, coordinates: bool = False, seed: int = 0, key_bits: int = 64,
                                max_bytes: int = 1 << 31) -> HaplotypeSequences:
    """The versions of every region (see the module's docstring).  `graph` / `regions` as compute_haplotype_classes takes them
    -- a DeviceGraph or GraphIndex with its [(S, E)] list, or lists of both, one entry per chromosome, or a scan_graph manifest
    with regions None.  The classes are computed here unless `classes` (compute_haplotype_classes over the same graph and
    regions) is given; every class's representative and the reference of every region are spelled, the classes of a region are
    grouped by (length, key) on the host and the groups verified byte for byte on the device.  A failed verification repeats
    with seed + 1, at most three seeds, then HashCollisionError.  `max_bytes`: the most bases spelled per chromosome graph; a
    larger total is refused with a ValueError that names it.  `key_bits` < 64 truncates the keys (a lab knob)."""
    from .haplotype_classes import compute_haplotype_classes
    torch = _torch()
    require_single_gpu("the haplotype sequences", "are", "a gather of the sharded class matrices")
    prep = prepare_graphs(graph, regions, chrom_names)
    _haplotype_set(prep, haplotype_names, "the haplotype sequence table")
    rows, _ = _matrix_rows(prep)
    if classes is None:
        classes = compute_haplotype_classes(graph, regions, debug, args_obj, chrom_names, haplotype_names, haplotype_groups)
    R = len(classes.region_names)
    if R != int(sum(len(r) for r in rows)):
        raise ValueError(f"classes of {R} regions for {int(sum(len(r) for r in rows))} regions")
    # ---- the pairs of every graph: per region (in the graph's order) its classes' representatives, then the reference
    jobs = []
    for gi, g in enumerate(prep.graphs):
        starts = np.ascontiguousarray(prep.spans[gi][0], dtype=np.int64)
        stops = np.ascontiguousarray(prep.spans[gi][1], dtype=np.int64)
        jobs.append((g, starts, stops) + _class_pairs(classes, rows[gi]))
    for attempt in range(SEEDS_TRIED):
        parts, good, base, byte_base = [], True, 0, 0
        for g, starts, stops, local, hap, pair_class, pair_region in jobs:
            with torch.cuda.device(g.device):
                d_len, off, bases, coord, keys = _spell(g, starts, stops, local, hap, coordinates, seed + attempt, key_bits, max_bytes)
                lengths = d_len.cpu().numpy()
                same = group_by_key(pair_region, lengths, keys.cpu().numpy().view(np.uint64))
                status = torch.zeros(1, dtype=torch.int32, device=g.device)
                d_same = torch.from_numpy(same).to(g.device)
                nv.check(nv.lib().gfm_sequences_verify(len(same), off.data_ptr(), bases.data_ptr(),
                                                       d_same.data_ptr() if len(same) else None, status.data_ptr(),
                                                       _stream_ptr(None)))
                if int(status.item()) != 0:
                    good = False
                    break
                parts.append((pair_class, pair_region, lengths, off.cpu().numpy()[:-1] + byte_base, bases.cpu().numpy(),
                              coord.cpu().numpy() if coord is not None else None, same.astype(np.int64) + base))
                base += len(same)
                byte_base += int(bases.numel())
        if not good:
            continue
        cat = lambda j, dt: (np.concatenate([p[j] for p in parts]) if parts else np.zeros(0, dtype=dt))      # noqa: E731
        return _assemble(classes, cat(0, np.int64), cat(1, np.int64), cat(2, np.int32), cat(3, np.int64), cat(4, np.uint8),
                         cat(5, np.int32) if coordinates else None, cat(6, np.int64))
    raise HashCollisionError(f"two sequences of a region share a {key_bits}-bit key under each of the seeds "
                             f"{seed} .. {seed + SEEDS_TRIED - 1}")


def _fasta_lines(hs: HaplotypeSequences, width: int):
    if int(width) < 1:
        raise ValueError(f"width {width}: it must be >= 1")
    hc = hs.classes
    alleles = hc.allele_strings()[hs._representative_class()] if len(hs) else []
    region = hs.version_region
    for v in range(len(hs)):
        r = int(region[v])
        yield (f">{hc.region_names[r]}|v{v - int(hs.offsets[r])} haplotypes={int(hs.count[v])} "
               f"representative={hc.haplotype_names[int(hs.first[v])]} alt_alleles={alleles[v]}\n")
        seq = hs.bases[hs.seq_offsets[v]:hs.seq_offsets[v + 1]].tobytes().decode("ascii")
        for at in range(0, len(seq), int(width)):
            yield seq[at:at + int(width)] + "\n"


def write_haplotype_sequences_fasta(hs: HaplotypeSequences, out, width: int = 60) -> Optional[str]:
    """The versions as FASTA to the path `out` (-> the path) or to the text stream `out`: a record per (region, version) in the
    table's order, header `>{sequence_name}|v{k} haplotypes={count} representative={name} alt_alleles={...}`, the bases in
    lines of `width`; an empty sequence has a header and no line"""
    if isinstance(out, str):
        with open(out, "w", encoding="utf-8", newline="\n") as fh:
            fh.writelines(_fasta_lines(hs, width))
        return out
    out.writelines(_fasta_lines(hs, width))
    out.flush()
    return None


def write_haplotype_sequence_versions(hs: HaplotypeSequences, out) -> Optional[str]:
    """The versions table (to_frame) as TSV to the path `out` (-> the path) or to the text stream `out`"""
    return write_frame(hs, out)


def haplotype_sequence_paths(args_obj) -> Tuple[str, str]:
    """-> (the FASTA's path, the versions table's): one pair per call, where grafimo_haplotype_class_members.tsv goes -- the -o
    directory, or with the default output directory grafimo_out_<pid>_classes"""
    tsv = table_path(VERSIONS_FILE, args_obj, tag="classes")
    return tsv[:-len(VERSIONS_FILE + ".tsv")] + FASTA_FILE + ".fa", tsv


def print_haplotype_sequence_versions(hs: HaplotypeSequences) -> None:
    """-f: the versions table on stdout instead of a file"""
    write_haplotype_sequence_versions(hs, sys.stdout)
