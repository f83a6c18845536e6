"""Hit-linkage table: which variants around a motif hit are carried by the same haplotypes as the hit.

The per-hit allele table and the pair table look INSIDE the k-mer.  This one answers the opposite question: a lead variant
lies near a peak but in no motif -- which predicted binding sites travel with it?  That is linkage disequilibrium between
a report row's carrier set and the allele bitsets of the sites around it, and only a haplotype-resolved graph has both.

All coordinates are the report's: 0-based reference offsets, as GraphIndex.pos (graph_tables._site_columns prints
pos + 1).  A report ROW has lo = min(start, stop), hi = max(start, stop) and its carrier set C, n_hit = |C| = its
haplotype_frequency; H is the number of haplotypes.  An ALLELE is (site s, ALT a) of the row's chromosome entry,
1 <= a <= n_alts[s], with carrier set A = alt_bits[s, a - 1], n_allele = |A|.  REF alleles are not listed (at a biallelic
site the REF allele has the ALT's r2).  distance = max(lo - pos[s], pos[s] - (hi - 1), 0); an allele is a CANDIDATE of the
row when distance <= flank -- sites outside the row's region count, the graph is the whole chromosome.  With
n_joint = |C & A|:
  Dn  = H * n_joint - n_hit * n_allele,    den = n_hit * (H - n_hit) * n_allele * (H - n_allele)
are exact integers (H <= 32 768 keeps both inside int64; a larger H is refused).  den == 0 -- a row or an allele carried by
nobody or by everybody -- leaves the LD undefined and the candidate is never listed.  Else
  r2 = float64(Dn * Dn) / float64(den)     (one IEEE division of the converted integers, on the host, in numpy)
  r  = sign(Dn) * sqrt(r2)
  d_prime = Dn / Dmax, 0 for Dn == 0;  Dmax = min(n_hit (H - n_allele), (H - n_hit) n_allele) for Dn > 0,
                                             min(n_hit n_allele, (H - n_hit) (H - n_allele)) otherwise.
A LINK is a candidate with r2 >= min_r2 (a candidate exactly at the threshold is listed); in_hit says that (entry, s, a) is
one of the row's own alleles in the HitAlleles CSR.  The table is per motif, ascending by (report row, site, allele): the
order is part of the contract.

The product runs on the GPU: gfm_hit_linkage (HIP, grafimo_amd/csrc/hit_linkage.hip) keeps a cell when ITS fp64 r2 is
>= min_r2 - 1e-9 and returns integers only; r2 is computed here by the formula above and the final cut made here, so the
device's rounding can only add cells that are then dropped, never lose or reorder a link.  `max_links` is checked against
the device's count, i.e. with that slack.  The defaults flank = 10 000 and min_r2 = 0.8 (the customary LD-proxy cut) are
product defaults, not measured quantities.
"""
import ctypes
import sys
from typing import List, Optional, Sequence

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import _stream_ptr, _torch
from .graph_tables import _haplotype_set, _site_columns, prepare_graphs, require_single_gpu, table_path, write_frame
from .hit_alleles import HitAlleles, compute_hit_alleles_many

ROW_COLUMNS = ["sequence_name", "motif_id", "motif_alt_id", "start", "stop", "strand", "score", "p-value", "matched_sequence",
               "haplotype_frequency"]
LINKAGE_FILE = "grafimo_hit_linkage"
MAX_HAPLOTYPES = 32768
ROWS_PER_TILE = (8, 16, 32)              # what gfm_hit_linkage takes beside 0, the library's default
SLOTS_PER_CHUNK = (64, 128, 256)
_COORD_LIMIT = 1 << 61
_DEFAULT_SCRATCH = 256 << 20


def _as_numpy(x, dtype):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def _as_words(x, name):
    x = _as_numpy(x, None)
    if x.dtype == np.int64:
        x = x.view(np.uint64)
    if x.dtype != np.uint64:
        raise ValueError(f"{name}: uint64 words")
    return x


def ld_statistics(n_joint, n_hit, n_allele, n_haplotypes: int):
    """-> (Dn int64, den int64, r2, r, d_prime float64) of the module's definitions; r2, r and d_prime are nan where
    den == 0.  H <= 32 768."""
    H = int(n_haplotypes)
    nj, nh, na = (np.asarray(x).astype(np.int64) for x in (n_joint, n_hit, n_allele))
    Dn = H * nj - nh * na
    den = nh * (H - nh) * na * (H - na)
    ok = den != 0
    safe = np.where(ok, den, 1)
    r2 = np.where(ok, (Dn * Dn).astype(np.float64) / safe.astype(np.float64), np.nan)
    r = np.sign(Dn) * np.sqrt(r2)
    dmax = np.where(Dn > 0, np.minimum(nh * (H - na), (H - nh) * na), np.minimum(nh * na, (H - nh) * (H - na)))
    dp = np.where(Dn == 0, 0.0, Dn.astype(np.float64) / np.where(dmax != 0, dmax, 1).astype(np.float64))
    return Dn, den, r2, r, np.where(ok, dp, np.nan)


def link_rows(lo, hi, masks, pos, n_alts, allele_bits, flank: int, min_r2: float, n_haplotypes: int,
              max_links: Optional[int] = None, rows_per_tile: int = 0, slots_per_chunk: int = 0, scratch_bytes: int = 0,
              device=None):
    """The thin wrapper of gfm_hit_linkage.  Rows in any order: `lo` <= `hi` (int64), `masks` uint64 [rows, hw]; sites in
    ascending `pos` (equal positions allowed), `n_alts` (<= 3), `allele_bits` uint64 [sites, 3, hw] whose slots a > n_alts
    are ignored whatever they hold; numpy arrays or torch tensors.  `n_haplotypes`: H, (hw - 1) * 64 < H <= hw * 64,
    H <= 32 768; bits beyond it in a mask or a used slot are refused (the kernel counts every bit it is given).
    The rows are sorted here by (lo, hi, index) and cut into position batches whose upload -- the batch's rows and only the
    sites that lie in some row's window -- stays within `scratch_bytes` (0: 256 MB; a batch is at least one row); the
    result does not depend on the budget, nor on `rows_per_tile` / `slots_per_chunk` (0: the library's default).
    -> (row, site, allele, n_joint, n_hit, n_allele): int64 [L] the caller's row index, int64 [L] the caller's site index,
    uint8 [L] 1 .. 3, int32 [L], int32 [rows], int32 [L] -- the links with r2 >= min_r2 (the exact cut, made here),
    ascending by (row, site, allele).  More than `max_links` cells listed by the device (r2 >= min_r2 - 1e-9 there):
    OverflowError naming the count, before anything is allocated for them."""
    torch = _torch()
    lo, hi = _as_numpy(lo, np.int64), _as_numpy(hi, np.int64)
    n = len(lo)
    H = int(n_haplotypes)
    if not 1 <= H <= MAX_HAPLOTYPES:
        raise ValueError(f"{H} haplotypes: the linkage counts are exact in int64 for 1 .. {MAX_HAPLOTYPES}")
    flank = int(flank)
    if flank < 0 or flank >= _COORD_LIMIT:
        raise ValueError(f"flank {flank} outside 0 .. 2^61")
    min_r2 = float(min_r2)
    if not 0.0 <= min_r2 <= 1.0:
        raise ValueError(f"min_r2 {min_r2} outside [0, 1]")
    if rows_per_tile not in (0,) + ROWS_PER_TILE:
        raise ValueError(f"rows_per_tile {rows_per_tile}: 0 or one of {ROWS_PER_TILE}")
    if slots_per_chunk not in (0,) + SLOTS_PER_CHUNK:
        raise ValueError(f"slots_per_chunk {slots_per_chunk}: 0 or one of {SLOTS_PER_CHUNK}")
    hw = (H + 63) // 64
    masks = _as_words(masks, "masks")
    if hi.shape != (n,) or masks.shape != (n, hw):
        raise ValueError(f"lo and hi are one value per row, masks uint64 [rows, {hw}] for {H} haplotypes")
    pos, n_alts = _as_numpy(pos, np.int64), _as_numpy(n_alts, np.uint8)
    S = len(pos)
    allele_bits = _as_words(allele_bits, "allele_bits") if S else np.zeros((0, 3, hw), np.uint64)
    if n_alts.shape != (S,) or allele_bits.shape != (S, 3, hw):
        raise ValueError(f"n_alts is one value per site, allele_bits uint64 [sites, 3, {hw}]")
    if (lo > hi).any():
        raise ValueError("a row with lo > hi")
    if (n and max(abs(int(lo.min())), abs(int(hi.max()))) >= _COORD_LIMIT) or (S and max(abs(int(pos[0])), abs(int(pos[-1]))) >= _COORD_LIMIT):
        raise ValueError("coordinates stay below 2^61")
    if S and (np.diff(pos) < 0).any():
        raise ValueError("the sites are not in ascending pos order")
    if S and int(n_alts.max()) > 3:
        raise ValueError("a site with more than 3 ALTs")
    if H & 63:
        if n and (masks[:, -1] >> np.uint64(H & 63)).any():
            raise ValueError("a carrier set has bits beyond the last haplotype")
        used = np.arange(3)[None, :] < n_alts[:, None]
        if S and ((allele_bits[:, :, -1] >> np.uint64(H & 63)) != 0)[used].any():
            raise ValueError("an allele bitset has bits beyond the last haplotype")
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(n, np.int32),
             np.zeros(0, np.int32))
    if n == 0:
        return empty
    order = np.lexsort((np.arange(n), hi, lo))
    lo_s, hi_s = lo[order], hi[order]
    first = np.searchsorted(pos, lo_s - flank, side="left")             # the row's sites are first .. last - 1
    last = np.maximum(np.searchsorted(pos, hi_s - 1 + flank, side="right"), first)
    # position batches: consecutive sorted rows; the sites of rows i .. j - 1 lie in first[i] .. max(last[i .. j - 1]) - 1
    budget = int(scratch_bytes) if scratch_bytes else _DEFAULT_SCRATCH
    row_bytes, site_bytes = 8 * hw + 40, 24 * hw + 48
    reach = np.maximum.accumulate(last)
    cost = np.arange(1, n + 1, dtype=np.int64) * row_bytes + reach.astype(np.int64) * site_bytes
    cuts, i = [0], 0
    while i < n:
        j = int(np.searchsorted(cost, budget + i * row_bytes + int(first[i]) * site_bytes, side="right"))
        i = max(j, i + 1)
        cuts.append(min(i, n))
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    lib = nv.lib()

    def upload(b):
        """rows cuts[b] .. cuts[b + 1] - 1 and the sites in a window of one of them -> the call's buffers"""
        i, j = cuts[b], cuts[b + 1]
        mark = np.zeros(S + 1, np.int64)
        np.add.at(mark, first[i:j], 1)
        np.add.at(mark, last[i:j], -1)
        sites = np.flatnonzero(np.cumsum(mark[:S]) > 0)
        rows = order[i:j]
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
        return dict(n=j - i, rows=rows, sites=sites, lo=t(lo_s[i:j]), hi=t(hi_s[i:j]), masks=t(masks[rows].view(np.int64)),
                    pos=t(pos[sites]), n_alts=t(n_alts[sites]), bits=t(allele_bits[sites].view(np.int64)),
                    off=torch.empty(j - i + 1, dtype=torch.int64, device=dev), n_hit=torch.empty(j - i, dtype=torch.int32, device=dev),
                    n_allele=torch.empty((max(len(sites), 1), 3), dtype=torch.int32, device=dev))

    def call(u, cap, d_site, d_allele, d_joint, flags):
        total = ctypes.c_int64()
        p = lambda x: x.data_ptr() if x is not None and x.numel() else None      # noqa: E731
        nv.check(lib.gfm_hit_linkage(p(u["lo"]), p(u["hi"]), p(u["masks"]), u["n"], p(u["pos"]), p(u["n_alts"]), p(u["bits"]),
                                     len(u["sites"]), hw, H, flank, min_r2, u["off"].data_ptr(), cap, p(d_site), p(d_allele),
                                     p(d_joint), u["n_hit"].data_ptr(), u["n_allele"].data_ptr(), int(rows_per_tile),
                                     int(slots_per_chunk), flags, ctypes.byref(total), sp))
        return int(total.value)

    n_batches = len(cuts) - 1
    n_hit = np.zeros(n, np.int32)
    parts = []
    with torch.cuda.device(dev):
        sp = _stream_ptr(None)
        kept, offsets, listed = None, [], 0
        for b in range(n_batches):                                    # count first ...
            u = upload(b)
            listed += call(u, 0, None, None, None, 0)
            offsets.append(u["off"].cpu().numpy())
            n_hit[u["rows"]] = u["n_hit"].cpu().numpy()
            if n_batches == 1:
                kept = u
        if max_links is not None and listed > max_links:
            raise OverflowError(f"{listed} candidate links, more than max_links = {max_links}: narrow the flank, raise min_r2 "
                                "or raise max_links")
        for b in range(n_batches):                                    # ... then allocate
            L = int(offsets[b][-1])
            if not L:
                continue
            u = kept if kept is not None else upload(b)
            if kept is None:
                u["off"].copy_(torch.from_numpy(offsets[b]))
            d_site = torch.empty(L, dtype=torch.int32, device=dev)
            d_allele = torch.empty(L, dtype=torch.uint8, device=dev)
            d_joint = torch.empty(L, dtype=torch.int32, device=dev)
            call(u, L, d_site, d_allele, d_joint, nv.GFM_LINKAGE_HAVE_OFFSETS)
            site_c, allele, joint = d_site.cpu().numpy().astype(np.int64), d_allele.cpu().numpy(), d_joint.cpu().numpy()
            row_c = np.repeat(np.arange(u["n"], dtype=np.int64), np.diff(offsets[b]))
            na = u["n_allele"].cpu().numpy()[site_c, allele.astype(np.int64) - 1]
            r2 = ld_statistics(joint, n_hit[u["rows"]][row_c], na, H)[2]
            keep = r2 >= min_r2                                       # the exact cut (nan: never)
            parts.append((u["rows"][row_c[keep]], u["sites"][site_c[keep]], allele[keep], joint[keep], na[keep]))
    if not parts:
        return empty[:4] + (n_hit, empty[5])
    row, site, allele, joint, na = (np.concatenate(x) for x in zip(*parts))
    o = np.argsort(row, kind="stable")                                # (a row's links are in (site, allele) order already)
    return row[o].astype(np.int64), site[o].astype(np.int64), allele[o], joint[o].astype(np.int32), n_hit, na[o].astype(np.int32)


class HitLinkage:
    """The linkage table of one motif (L links):
    table     the motif's HitAlleles (carriers kept, row_entry filled): table.report is the motif's report;
    row       int64 [L]: the report row;  entry int32 [L]: its chromosome entry;  site int32 [L]: the graph site of
              table.indexes[entry];  allele uint8 [L]: the ALT, 1 .. 3;
    distance  int64 [L];  n_joint, n_allele, n_hit int32 [L]: |C & A|, |A|, |C|;
    r2, r, d_prime float64 [L];  in_hit bool [L]: the allele is one of the row's own."""

    def __init__(self, table: HitAlleles, row, site, allele, entry, distance, n_joint, n_allele, n_hit, r2, r, d_prime, in_hit):
        self.table = table
        self.row = np.asarray(row, dtype=np.int64)
        self.site = np.asarray(site, dtype=np.int32)
        self.allele = np.asarray(allele, dtype=np.uint8)
        self.entry = np.asarray(entry, dtype=np.int32)
        self.distance = np.asarray(distance, dtype=np.int64)
        self.n_joint = np.asarray(n_joint, dtype=np.int32)
        self.n_allele = np.asarray(n_allele, dtype=np.int32)
        self.n_hit = np.asarray(n_hit, dtype=np.int32)
        self.r2 = np.asarray(r2, dtype=np.float64)
        self.r = np.asarray(r, dtype=np.float64)
        self.d_prime = np.asarray(d_prime, dtype=np.float64)
        self.in_hit = np.asarray(in_hit, dtype=bool)

    def __len__(self) -> int:
        return len(self.row)

    def _variant_strings(self) -> np.ndarray:
        """POS:REF>ALT per link, as HitAlleles._allele_strings prints an ALT allele"""
        out = np.empty(len(self), dtype=object)
        for e in np.unique(self.entry).tolist():
            sel = np.flatnonzero(self.entry == e)
            pos, refs, alts, _, _ = _site_columns(self.table.indexes[e], self.site[sel].astype(np.int64), self.allele[sel].astype(np.int64))
            out[sel] = [f"{p}:{r}>{x}" for p, r, x in zip(pos.tolist(), refs, alts)]
        return out

    def to_frame(self) -> pd.DataFrame:
        """sequence_name, motif_id, motif_alt_id, start, stop, strand, score, p-value, matched_sequence, haplotype_frequency
        of the row; variant (POS:REF>ALT); distance; allele_haplotypes; co_haplotypes; r2; r; d_prime; in_hit"""
        rep = self.table.report
        data = {c: rep[c].to_numpy()[self.row] for c in ROW_COLUMNS}
        data["variant"] = self._variant_strings()
        data["distance"] = self.distance
        data["allele_haplotypes"] = self.n_allele.astype(np.int64)
        data["co_haplotypes"] = self.n_joint.astype(np.int64)
        data["r2"], data["r"], data["d_prime"] = self.r2, self.r, self.d_prime
        data["in_hit"] = self.in_hit
        return pd.DataFrame(data)


def _linkage_of(t: HitAlleles, H: int, flank: int, min_r2: float, max_links: Optional[int], **cuts) -> HitLinkage:
    n = len(t)
    hw = (H + 63) // 64
    start, stop = t.report["start"].to_numpy(np.int64), t.report["stop"].to_numpy(np.int64)
    lo, hi = np.minimum(start, stop), np.maximum(start, stop)
    freq = t.report["haplotype_frequency"].to_numpy(np.int64)
    row_entry = np.asarray(t.row_entry, dtype=np.int64)
    parts, listed = [], 0
    for e in np.unique(row_entry).tolist():
        rows = np.flatnonzero(row_entry == e)
        idx = t.indexes[e]
        room = None if max_links is None else max_links - listed
        row, site, allele, joint, n_hit, na = link_rows(lo[rows], hi[rows], t.carrier_bits[rows].reshape(len(rows), hw), idx.pos, idx.n_alts,
                                                        idx.alt_bits, flank, min_r2, H, max_links=room, **cuts)
        if not np.array_equal(n_hit.astype(np.int64), freq[rows]):
            raise RuntimeError("gfm_hit_linkage and the report disagree on a row's haplotype_frequency")
        listed += len(row)
        pos = np.asarray(idx.pos, dtype=np.int64)[site]
        r = rows[row]
        dist = np.maximum(np.maximum(lo[r] - pos, pos - (hi[r] - 1)), 0)
        parts.append((r, site, allele, np.full(len(r), e, np.int32), dist, joint, na, n_hit[row]))
    if parts:
        row, site, allele, entry, dist, joint, na, nh = (np.concatenate(x) for x in zip(*parts))
    else:
        row, site, dist = (np.zeros(0, np.int64) for _ in range(3))
        allele, entry, joint, na, nh = np.zeros(0, np.uint8), np.zeros(0, np.int32), *(np.zeros(0, np.int32) for _ in range(3))
    o = np.argsort(row, kind="stable")                                # (a row has one entry: its links stay in (site, allele) order)
    row, site, allele, entry, dist, joint, na, nh = (x[o] for x in (row, site, allele, entry, dist, joint, na, nh))
    _, _, r2, r, dp = ld_statistics(joint, nh, na, H)
    # in_hit: (row, site, allele) among the row's own alleles of the CSR (an allele there belongs to the row's entry)
    csr_row = np.repeat(np.arange(n, dtype=np.int64), np.diff(t.allele_offsets))
    width = 4 * (1 + max(int(t.allele_site.max()) if len(t.allele_site) else 0, int(site.max()) if len(site) else 0))
    own = csr_row * width + t.allele_site.astype(np.int64) * 4 + t.allele.astype(np.int64)
    own = own[t.allele_entry.astype(np.int64) == row_entry[csr_row]] if len(own) else own
    in_hit = np.isin(row * width + site * 4 + allele.astype(np.int64), own)
    return HitLinkage(t, row, site, allele, entry, dist, joint, na, nh, r2, r, dp, in_hit)


def compute_hit_linkage_many(motifs: Sequence, graph, regions, debug: bool, args_obj, chrom_names=None,
                             haplotype_names: Optional[Sequence[str]] = None, flank: int = 10000, min_r2: float = 0.8,
                             max_links: Optional[int] = 1 << 26, rows_per_tile: int = 0, slots_per_chunk: int = 0,
                             scratch_bytes: int = 0) -> List[HitLinkage]:
    """The hit-linkage table of every motif of a set (see the module's docstring) -> one HitLinkage per motif, in the order
    of `motifs`.  `graph` / `regions`, args_obj, `chrom_names` and `haplotype_names` as compute_hit_alleles_many takes them.
    A graph without haplotype bitsets, graphs of different haplotype sets, more than 32 768 haplotypes, flank < 0 or min_r2
    outside [0, 1]: ValueError; more than `max_links` cells listed by the device for one motif: OverflowError naming the
    count.  `rows_per_tile`, `slots_per_chunk`, `scratch_bytes` as link_rows takes them: the result does not depend on them."""
    require_single_gpu("the hit-linkage table", "is", "a gather of the sharded tables")
    if int(flank) < 0:
        raise ValueError(f"flank {flank} < 0")
    if not 0.0 <= float(min_r2) <= 1.0:
        raise ValueError(f"min_r2 {min_r2} outside [0, 1]")
    prep = prepare_graphs(graph, regions, chrom_names)
    H, _names = _haplotype_set(prep, haplotype_names, "the hit-linkage table")      # (the refusals, before any pass runs)
    if H > MAX_HAPLOTYPES:
        raise ValueError(f"{H} haplotypes: the linkage counts are exact in int64 up to {MAX_HAPLOTYPES}")
    tables = compute_hit_alleles_many(motifs, graph, regions, debug, args_obj, chrom_names, haplotype_names, None, carriers=True,
                                      scratch_bytes=scratch_bytes)
    return [_linkage_of(t, H, int(flank), float(min_r2), max_links, rows_per_tile=rows_per_tile, slots_per_chunk=slots_per_chunk,
                        scratch_bytes=scratch_bytes) for t in tables]


def compute_hit_linkage(motif, graph, regions, debug: bool, args_obj, chrom_names=None,
                        haplotype_names: Optional[Sequence[str]] = None, flank: int = 10000, min_r2: float = 0.8,
                        max_links: Optional[int] = 1 << 26, **cuts) -> HitLinkage:
    """The hit-linkage table of `motif`: compute_hit_linkage_many for a set of one."""
    return compute_hit_linkage_many([motif], graph, regions, debug, args_obj, chrom_names, haplotype_names, flank, min_r2,
                                    max_links, **cuts)[0]


def write_hit_linkage(hl: HitLinkage, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_hit_linkage.tsv (grafimo_hit_linkage_<motif_id>.tsv for one of several motifs) in the directory
    write_hit_alleles uses for this motif -> the path written.  `out`: a text stream to write to instead (-f: stdout)."""
    return write_frame(hl, out if out is not None else table_path(LINKAGE_FILE, args_obj, motif, motif_num))


def print_hit_linkage(hl: HitLinkage) -> None:
    """-f: the table on stdout instead of a file"""
    write_hit_linkage(hl, None, 1, None, out=sys.stdout)
