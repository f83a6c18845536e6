"""Query variants: variants that are NOT in the panel -- GWAS lead SNPs, rare or de-novo calls, somatic mutations -- scored on
every sequence background the panel holds.  Where a linear scanner states a variant's effect against the reference sequence,
this table states it per CONTEXT: per distinct stretch of bases the haplotypes spell around the variant, with how many
haplotypes (and how many per group) carry each.  A SNP that breaks a site on the reference may do nothing on the haplotypes
that carry a neighbouring panel variant.

THE RULE (include/grafimo_hip.h states it for the library; tests/query_variant_bruteforce.py on the host).
A query variant is (chrom, pos 1-based, id, REF, ALT), REF and ALT plain base strings.  It is normalised first (normalise): the
common prefix is stripped, then the common suffix -> pos0 (0-based position of the first remaining REF base), ref of lr >= 0 and
alt of la >= 0 bases, not both 0; lr or la above MAX_ALLELE = 64 is refused (ValueError naming the variant; the command line
skips it with a warning).
The FOOTPRINT (footprints) is the region spelled for the variant: walking left from pos0 the reference positions that are not
inside the deleted span [pos + 1, pos + del_len] of any deletion site are counted until W - 1 are counted or position 0 is
reached, the same to the right from pos0 + lr up to the chromosome's end: [pos0 - FL, pos0 + lr + FR).  Conservative: every
haplotype spells at least W - 1 bases on each side of the allele wherever the chromosome has them.  (A pure insertion's
footprint holds at least the two bases of its junction, also at W = 1.)
APPLICABILITY, with x the bases a version (haplotype_sequences) spells over the footprint and coord their coordinates.
lr > 0: o is the offset of the non-inserted base with coordinate pos0; the edit applies when x[o .. o + lr) are non-inserted, their
coordinates pos0 .. pos0 + lr - 1 in order, and they equal ref without regard to case.  lr == 0 (a pure insertion): o as above,
the edit applies when x[o - 1] is the non-inserted base with coordinate pos0 - 1; when pos0 is the chromosome's length o = len(x)
and x[o - 1] must be that base.  An edit that does not apply is `absent` -- no non-inserted base carries a needed coordinate, the
background deletes it -- or a `mismatch` -- the bases are there but differ from REF, or an inserted base lies between them: the
background carries a panel allele there.  A variant that is itself in the panel applies to its REF carriers and is a mismatch on
its ALT carriers.
WINDOWS.  y = x[:o] + alt + x[o + lr:].  REF side: the window starts s of x with s <= o + lr - 1 and s + W - 1 >= o (lr == 0: the
windows across the junction); ALT side: the same in y with la; each clipped to 0 <= s <= len - W, a side may have no window.
Every window is scored once per strand unless --no-reverse; a k-mer holding a non-ACGT base scores min_val.
RESULTS per side: the best window by (score descending, s ascending, '+' before '-'), and the exact uint64 sum over the side's
windows and strands of w[score], w the table of haplotype_affinity.default_weights or the caller's.
CONTEXTS.  The result depends on nothing but the USED CONTEXT x[max(0, o - W + 1) : min(len, o + lr + W - 1)] and o's place in it:
the applied versions of a variant whose used contexts are byte-equal are merged (counts and group counts summed, the smallest
member the representative), and numbered by haplotypes descending, then representative.  is_reference: the context is the
reference sequence's.

The hot path is HIP (grafimo_amd/csrc/gfm_graph_query_variants.hpp, gfm_graph_query_edits): a wavefront per (version, edit).
"""
import gzip
import sys
import warnings
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from . import _native as nv
from .extract_regions import GraphIndex, _stream_ptr, _torch
from .graph_tables import (group_by_width, prepare_graphs, require_single_gpu, scaled_pvalues, scaled_scores, table_path,
                           write_frame)

MAX_ALLELE = nv.GFM_QUERY_MAX_ALLELE
SUMMARY_FILE = "grafimo_query_variants"
CONTEXTS_FILE = "grafimo_query_variant_contexts"
STATUS_NAMES = ("applied", "absent", "mismatch")
EFFECTS = np.array(["none", "gain", "loss", "both"], dtype=object)          # index: (ref hit) * 2 + (alt hit)
RECORD = np.dtype([("status", np.int32), ("o", np.int32), ("ref_key", np.uint32), ("alt_key", np.uint32),
                   ("ref_sum", np.uint64), ("alt_sum", np.uint64)])
_COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")
_PLAIN = np.full(256, ord("N"), dtype=np.uint8)                               # an ALT byte that is no base scores as N
for _c in b"ACGTacgt":
    _PLAIN[_c] = _c


# ---------------------------------------------------------------------------------------------------------------- the input
def read_query_vcf(path: str) -> List[Tuple[str, int, str, str, str]]:
    """The query variants of a VCF (plain or gzip), the five fixed columns only -> [(chrom, pos, id, ref, alt)], a multi-allelic
    ALT one variant per allele; symbolic (<DEL>), '*' and breakend ALTs are left out with one warning that counts them; sample
    columns are ignored."""
    with open(path, "rb") as fh:
        gz = fh.read(2) == b"\x1f\x8b"
    out, left_out = [], 0
    with (gzip.open(path, "rt", errors="replace") if gz else open(path, "rt", errors="replace")) as fh:
        for n, line in enumerate(fh, 1):
            if line.startswith("#") or not line.strip():
                continue
            f = line.rstrip("\r\n").split("\t", 5)
            if len(f) < 5:
                raise ValueError(f"{path}:{n}: a VCF line has CHROM POS ID REF ALT, tab-separated")
            chrom, pos, vid, ref = f[0], int(f[1]), f[2], f[3]
            for alt in f[4].split(","):
                if not _plain(alt) or not _plain(ref):
                    left_out += 1
                    continue
                out.append((chrom, pos, vid, ref, alt))
    if left_out:
        warnings.warn(f"{path}: {left_out} ALT alleles that are no plain base string of A, C, G, T, N (symbolic, '*', breakends, "
                      "ambiguity codes) were left out")
    return out


def _plain(allele: str) -> bool:
    """a non-empty string of A, C, G, T, N in either case"""
    return bool(allele) and not allele.strip("ACGTNacgtn")


def unusable(chrom: str, pos: int, vid: str, ref: str, alt: str, chrom_len: Optional[int] = None) -> Optional[str]:
    """None, or why the table cannot take this variant, in words that name it: REF or ALT is no plain base string, REF equals
    ALT, an allele of more than MAX_ALLELE bases after trimming, or -- given the chromosome's length -- a REF that does not lie
    on the chromosome (POS < 1 or POS - 1 + |REF| beyond its end: a VCF of another assembly)"""
    what = f"query variant {chrom}:{pos} {vid} {ref[:20]}>{alt[:20]}"
    if not _plain(ref) or not _plain(alt):
        return f"{what}: REF and ALT are plain base strings"
    _, nref, nalt = normalise(pos, ref, alt)
    if not nref and not nalt:
        return f"{what}: REF equals ALT"
    if len(nref) > MAX_ALLELE or len(nalt) > MAX_ALLELE:
        return f"{what}: an allele of {max(len(nref), len(nalt))} bases after trimming, at most {MAX_ALLELE}"
    if chrom_len is not None and (int(pos) < 1 or int(pos) - 1 + len(ref) > int(chrom_len)):
        return f"{what}: REF lies outside the chromosome's {int(chrom_len)} bases"
    return None


def normalise(pos: int, ref: str, alt: str) -> Tuple[int, str, str]:
    """-> (pos0, ref, alt): the common prefix stripped, then the common suffix; pos0 the 0-based position of the first
    remaining REF base (of the base behind the insertion point when no REF base remains)"""
    a = 0
    while a < len(ref) and a < len(alt) and ref[a].upper() == alt[a].upper():
        a += 1
    ref, alt = ref[a:], alt[a:]
    b = 0
    while b < len(ref) and b < len(alt) and ref[-1 - b].upper() == alt[-1 - b].upper():
        b += 1
    if b:
        ref, alt = ref[:-b], alt[:-b]
    return int(pos) - 1 + a, ref, alt


def deleted_spans(index: GraphIndex) -> Tuple[np.ndarray, np.ndarray]:
    """-> (starts, stops) int64: the union of the deleted spans [pos + 1, pos + 1 + del_len) of the index's deletion sites as
    disjoint ascending intervals, clipped to the chromosome"""
    L = len(index.ref)
    d = np.asarray(index.del_len, dtype=np.int64)
    at = np.flatnonzero(d > 0)
    a = np.minimum(np.asarray(index.pos, dtype=np.int64)[at] + 1, L)
    b = np.minimum(a + d[at], L)
    a, b = a[b > a], b[b > a]
    if not len(a):
        return a, b
    order = np.argsort(a, kind="stable")
    a, b = a[order], b[order]
    reach = np.maximum.accumulate(b)
    head = np.concatenate([[True], a[1:] > reach[:-1]])
    last = np.concatenate([np.flatnonzero(head)[1:] - 1, [len(a) - 1]])
    return a[head], reach[last]


def footprints(index: GraphIndex, pos0, lr, width: int) -> Tuple[np.ndarray, np.ndarray]:
    """The footprints [S, E) of the edits (pos0, lr) at motif width `width` over `index` (see the module's docstring) -> (S, E)
    int64.  Vectorised over the edits: the kept positions -- those in no deleted span -- are counted and selected through the
    merged spans, no step per base."""
    L = len(index.ref)
    pos0 = np.asarray(pos0, dtype=np.int64)
    lr = np.asarray(lr, dtype=np.int64)
    lo = np.clip(pos0, 0, L)
    hi = np.clip(pos0 + lr, 0, L)
    a, b = deleted_spans(index)
    done = np.concatenate([[0], np.cumsum(b - a)]).astype(np.int64)         # deleted positions in the first k spans
    kept_before = a - done[:-1]                                             # kept positions before span k

    def kept_below(x):                                                      # the kept positions < x
        k = np.searchsorted(a, x, side="right")
        inside = np.where(k > 0, np.clip(x - a[np.maximum(k - 1, 0)], 0, (b - a)[np.maximum(k - 1, 0)]), 0) if len(a) else 0
        return x - (done[np.maximum(k - 1, 0)] + inside) if len(a) else x.copy()

    def kept_at(r):                                                         # the position of the kept position of rank r
        return r + done[np.searchsorted(kept_before, r, side="right")]

    n = int(width) - 1
    total = int(L - done[-1])
    if n <= 0:
        S, E = lo.copy(), hi.copy()
    else:
        left, right = kept_below(lo), kept_below(hi)
        S = np.where(left >= n, kept_at(np.maximum(left - n, 0)), 0)
        E = np.where(right + n <= total, kept_at(np.minimum(right + n - 1, max(total - 1, 0))) + 1, L) if total else np.full(len(lo), L)
    ins = lr == 0                                                           # a junction's two bases, whatever the width
    S = np.where(ins, np.minimum(S, np.maximum(lo - 1, 0)), S)
    E = np.where(ins, np.maximum(E, np.minimum(hi + 1, L)), E)
    return np.minimum(S, lo).astype(np.int64), np.maximum(E, hi).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _byte_table(strings: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """-> (offsets int32 [n + 1], bytes uint8, one spare byte so that the buffer is never empty)"""
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in strings]
    off = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
    if off[-1] >= 1 << 31:
        raise ValueError("the edits' alleles hold 2^31 bytes or more")
    return off.astype(np.int32), np.frombuffer(b"".join(raw) + b"N", dtype=np.uint8).copy()


def _stage(tables, seq_offsets, bases, coord, pos0, refs, alts, item_seq, item_edit):
    """the inputs of gfm_graph_query_edits on the current device -> (the device tensors in the entry's order, the weight
    tables' tensors, the largest weight, the counts (V, Q, N))"""
    torch = _torch()
    seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    ref_off, ref_bytes = _byte_table(refs)
    alt_off, alt_bytes = _byte_table(alts)
    alt_bytes = _PLAIN[alt_bytes]
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    pad = lambda a, dt: np.concatenate([np.asarray(a, dtype=dt), np.zeros(1, dtype=dt)])  # noqa: E731  (never an empty buffer)
    d = [up(seq_offsets, np.int64), up(pad(bases, np.uint8), np.uint8), up(pad(coord, np.int32), np.int32),
         up(pad(pos0, np.int64), np.int64), up(ref_off, np.int32), up(ref_bytes, np.uint8), up(alt_off, np.int32),
         up(alt_bytes, np.uint8), up(item_seq, np.int32), up(item_edit, np.int32)]
    return d, [up(t.view(np.int64), np.int64) for t in tables], max(int(t.max()) for t in tables), \
        (len(seq_offsets) - 1, len(pos0), len(item_seq))


def _enqueue(dms, staged, forward_only: bool, rec=None, status=None):
    """gfm_graph_query_edits over staged inputs (_stage) -> the records, a device tensor int64 [M, N, 4].  `rec`, `status`: a
    record tensor and an int32 status word to reuse, whatever they hold: the entry writes every record and clears the word."""
    import ctypes
    torch = _torch()
    d, d_tabs, max_weight, (V, Q, N) = staged
    M = len(dms)
    if rec is None:
        rec = torch.zeros((M, N, RECORD.itemsize // 8), dtype=torch.int64, device=d[0].device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=d[0].device)
    vp = ctypes.c_void_p
    nv.check(nv.lib().gfm_graph_query_edits(
        (vp * M)(*[x.handle for x in dms]), M, (vp * M)(*[t.data_ptr() for t in d_tabs]), max_weight, V, d[0].data_ptr(),
        d[1].data_ptr(), d[2].data_ptr(), Q, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(),
        N, d[8].data_ptr(), d[9].data_ptr(), nv.GFM_GRAPH_FORWARD_ONLY if forward_only else 0,
        (vp * M)(*[rec[m].data_ptr() for m in range(M)]), status.data_ptr(), _stream_ptr(None)))
    return rec


def _launch(dms, tables, seq_offsets, bases, coord, pos0, refs, alts, item_seq, item_edit, forward_only: bool) -> np.ndarray:
    """gfm_graph_query_edits for leased motifs of one width -> RECORD [M, N]"""
    M, N = len(dms), len(item_seq)
    if N == 0:
        return np.zeros((M, 0), dtype=RECORD)
    rec = _enqueue(dms, _stage(tables, seq_offsets, bases, coord, pos0, refs, alts, item_seq, item_edit), forward_only)
    return rec.cpu().numpy().view(RECORD).reshape(M, N)


def _weight_tables(dms, motifs, weights, temperature):
    """-> (per motif its uint64 [L] table, its log2 offset): haplotype_affinity's"""
    from .haplotype_affinity import FRACTION_BITS, default_weights
    tables, offsets = [], []
    for k, dm in enumerate(dms):
        if weights is None:
            w, s_best = default_weights(dm, temperature)
            offsets.append(-FRACTION_BITS + (s_best / dm.scale + dm.width * dm.offset) / float(temperature))
        else:
            w = np.ascontiguousarray(weights[k], dtype=np.uint64)
            if w.shape != (dm.L,):
                raise ValueError(f"{motifs[k].motif_id}: a weight table of shape {w.shape}, the motif's scores need ({dm.L},)")
            offsets.append(0.0)
        tables.append(w)
    return tables, offsets


def score_edits(motifs: Sequence, seq_offsets, bases, coord, pos0, refs: Sequence, alts: Sequence, item_seq, item_edit,
                weights: Optional[Sequence[np.ndarray]] = None, temperature: float = 1.0,
                forward_only: bool = False) -> List[np.ndarray]:
    """The kernel on plain arrays: sequences as HaplotypeSequences holds them (`seq_offsets` int64 [V + 1], `bases` uint8,
    `coord` int32, ~coordinate for an inserted base), edits (`pos0` [Q], `refs` / `alts`: Q byte strings, already normalised) and
    items (`item_seq`, `item_edit` [N]) for motifs of ONE width -> per motif a RECORD array [N]: status (0 applied, 1 absent,
    2 mismatch), o, ref_key / alt_key (decode_keys) and ref_sum / alt_sum.  A sequence whose last base is the base pos0 - 1 is
    taken to end its chromosome (see include/grafimo_hip.h).  The library refuses motifs of two widths, an allele longer than
    MAX_ALLELE and an item index out of range."""
    from .device import DeviceMotif
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    if len(refs) != len(pos0) or len(alts) != len(pos0):
        raise ValueError("pos0, refs and alts are one value per edit")
    if len(item_seq) != len(item_edit):
        raise ValueError("item_seq and item_edit are one value per item")
    dms = [DeviceMotif.lease(m) for m in motifs]
    try:
        tables, _ = _weight_tables(dms, motifs, weights, temperature)
        got = _launch(dms, tables, seq_offsets, bases, coord, pos0, refs, alts, item_seq, item_edit, forward_only)
        return [got[m] for m in range(len(motifs))]
    finally:
        for dm in dms:
            dm.release()


def decode_keys(key: np.ndarray):
    """a side's keys -> (score int64, -1: no window; s - o int64; strand object '+' / '-', '' for none)"""
    key = np.asarray(key, dtype=np.int64)
    some = key > 0
    score = np.where(some, (key >> 8) - 1, -1)
    rel = np.where(some, 64 - ((key >> 1) & 127), 0)
    strand = np.where(some, np.where(key & 1, "+", "-"), "").astype(object)
    return score, rel, strand


# ---------------------------------------------------------------------------------------------------------------- the table
def used_context(x: bytes, o: int, lr: int, W: int) -> Tuple[bytes, int]:
    """-> (x[max(0, o - W + 1) : min(len, o + lr + W - 1)], o's place in it): all a side's result depends on"""
    lo = max(0, o - W + 1)
    return x[lo:min(len(x), o + lr + W - 1)], o - lo


def merge_contexts(keys: Sequence, count, first, group_counts, is_reference):
    """The contexts of ONE variant from its applied versions: `keys` a hashable per version (its used context), count / first
    [n], group_counts [n, G], is_reference [n] -> (context_of int64 [n]: the context's number, by haplotypes descending, then
    representative; count, first, group_counts, is_reference of the contexts; the version each context is spelled by: the one
    holding its representative)"""
    count, first = np.asarray(count, dtype=np.int64), np.asarray(first, dtype=np.int64)
    group_counts = np.asarray(group_counts, dtype=np.int64)
    if group_counts.ndim != 2:
        group_counts = group_counts.reshape(len(count), -1) if len(count) else np.zeros((0, 0), dtype=np.int64)
    is_reference = np.asarray(is_reference, dtype=bool)
    slot = {}
    of = np.array([slot.setdefault(k, len(slot)) for k in keys], dtype=np.int64)
    C = len(slot)
    c_count = np.zeros(C, dtype=np.int64)
    np.add.at(c_count, of, count)
    c_first = np.full(C, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(c_first, of, first)
    c_groups = np.zeros((C, group_counts.shape[1]), dtype=np.int64)
    np.add.at(c_groups, of, group_counts)
    c_ref = np.zeros(C, dtype=bool)
    np.logical_or.at(c_ref, of, is_reference)
    head = np.zeros(C, dtype=np.int64)
    head[of[first == c_first[of]]] = np.flatnonzero(first == c_first[of])
    order = np.lexsort((c_first, -c_count))
    number = np.empty(C, dtype=np.int64)
    number[order] = np.arange(C)
    return number[of], c_count[order], c_first[order], c_groups[order], c_ref[order], head[order]


def _kmer(x: bytes, rel: int, o: int, strand: str, W: int) -> str:
    k = x[o + rel:o + rel + W]
    return (k if strand == "+" else k.translate(_COMP)[::-1]).decode("ascii")


class QueryVariants:
    """The table of one motif over R query variants and C contexts (see the module's docstring).
    Per variant [R]: chrom, pos, vid, ref, alt (as given), pos0 / nref / nalt (normalised), haplotypes_applied / _absent /
    _mismatch, context_offsets int64 [R + 1] (the contexts of variant r are rows context_offsets[r] .. of the per-context
    arrays, by number), reference (RECORD [R]: the edit on the reference sequence itself).
    Per context [C]: count, first, group_counts [C, G], is_reference, records (RECORD), ref_kmer / alt_kmer.
    Per spelled version [V] (what the kernel saw, before the merge): version_variant, version_count, version_records (RECORD,
    the status corrected by the chromosome's length), version_context (the context's number, -1 where the edit does not apply).
    """

    def __init__(self, motif_id, motif_alt_id, width, scale, offset, ptable, log2_offset, threshold, haplotype_names, group_names,
                 variants, normalised, hap_status, context_offsets, count, first, group_counts, is_reference, records, ref_kmer,
                 alt_kmer, reference, version_variant, version_count, version_records, version_context, all_variants=False):
        self.motif_id, self.motif_alt_id = motif_id, motif_alt_id
        self.width, self.scale, self.offset = int(width), int(scale), float(offset)
        self.ptable, self.log2_offset, self.threshold = np.asarray(ptable, dtype=np.float64), float(log2_offset), float(threshold)
        self.haplotype_names, self.group_names = list(haplotype_names), list(group_names)
        self.chrom, self.pos, self.vid, self.ref, self.alt = [np.asarray(c, dtype=object) for c in zip(*variants)] if len(variants) \
            else [np.zeros(0, dtype=object)] * 5
        self.pos = self.pos.astype(np.int64)
        self.pos0 = np.array([n[0] for n in normalised], dtype=np.int64)
        self.nref, self.nalt = [n[1] for n in normalised], [n[2] for n in normalised]
        hap_status = np.asarray(hap_status, dtype=np.int64).reshape(len(self.pos0), 3)
        self.haplotypes_applied, self.haplotypes_absent, self.haplotypes_mismatch = hap_status[:, 0], hap_status[:, 1], hap_status[:, 2]
        self.context_offsets = np.asarray(context_offsets, dtype=np.int64)
        self.count, self.first = np.asarray(count, dtype=np.int64), np.asarray(first, dtype=np.int64)
        self.group_counts = np.asarray(group_counts, dtype=np.int64).reshape(len(self.count), len(self.group_names))
        self.is_reference = np.asarray(is_reference, dtype=bool)
        self.records = np.asarray(records, dtype=RECORD)
        self.ref_kmer, self.alt_kmer = np.asarray(ref_kmer, dtype=object), np.asarray(alt_kmer, dtype=object)
        self.reference = np.asarray(reference, dtype=RECORD)
        self.version_variant = np.asarray(version_variant, dtype=np.int64)
        self.version_count = np.asarray(version_count, dtype=np.int64)
        self.version_records = np.asarray(version_records, dtype=RECORD)
        self.version_context = np.asarray(version_context, dtype=np.int64)
        self.all_variants = bool(all_variants)

    def __len__(self) -> int:
        return int(self.kept().sum())

    @property
    def context_variant(self) -> np.ndarray:
        return np.repeat(np.arange(len(self.pos0), dtype=np.int64), np.diff(self.context_offsets))

    def _side(self, recs, side: str):
        """-> (score log-odds, p-value, strand, offset float (NaN: none), integer score, log2 affinity)"""
        best, rel, strand = decode_keys(recs[side + "_key"])
        sums = recs[side + "_sum"]
        la = np.full(len(recs), np.nan)
        la[sums > 0] = np.log2(sums[sums > 0].astype(np.float64)) + self.log2_offset
        return (scaled_scores(best, self.scale, self.offset, self.width), scaled_pvalues(best, self.ptable), strand,
                np.where(best >= 0, rel.astype(np.float64), np.nan), best, la)

    def effect_codes(self, recs) -> np.ndarray:
        """int64: (the REF side's best window has p < threshold) * 2 + (the ALT side's has); a side without a window has not"""
        with np.errstate(invalid="ignore"):
            pr, px = self._side(recs, "ref")[1] < self.threshold, self._side(recs, "alt")[1] < self.threshold      # (NaN: False)
        return pr.astype(np.int64) * 2 + px.astype(np.int64)

    def effects(self, recs) -> np.ndarray:
        """none / gain / loss / both on p < threshold of the two sides' best windows"""
        return EFFECTS[self.effect_codes(recs)]

    def kept(self) -> np.ndarray:
        """bool [R]: the variants the frames hold -- all_variants, or some context has an effect other than none"""
        R = len(self.pos0)
        if self.all_variants:
            return np.ones(R, dtype=bool)
        hit = np.zeros(R, dtype=bool)
        hit[self.context_variant[self.effects(self.records) != "none"]] = True
        return hit

    def _variant_columns(self, at) -> dict:
        n = len(at)
        return {"motif_id": np.full(n, self.motif_id, dtype=object), "motif_alt_id": np.full(n, self.motif_alt_id, dtype=object),
                "chrom": self.chrom[at], "pos": self.pos[at], "id": self.vid[at], "ref": self.ref[at], "alt": self.alt[at]}

    def contexts_frame(self) -> pd.DataFrame:
        """a row per (variant, context) of the kept variants: motif_id, motif_alt_id, chrom, pos, id, ref, alt, context,
        haplotypes, frequency, one haplotypes_<GROUP> per group, representative, is_reference, ref_score, ref_pvalue, ref_strand,
        ref_offset, ref_kmer, alt_score .. alt_kmer, delta_score, ref_log2_affinity, alt_log2_affinity, delta_log2_affinity,
        effect -- the offsets are window start - o; NaN or empty where a side has no window"""
        var = self.context_variant
        rows = np.flatnonzero(self.kept()[var]) if len(var) else np.zeros(0, dtype=np.int64)
        v, recs = var[rows], self.records[rows]
        data = self._variant_columns(v)
        H = max(len(self.haplotype_names), 1)
        data["context"] = rows - self.context_offsets[v]
        data["haplotypes"] = self.count[rows]
        data["frequency"] = self.count[rows].astype(np.float64) / float(H)
        for g, name in enumerate(self.group_names):
            data[f"haplotypes_{name}"] = self.group_counts[rows, g]
        names = np.asarray(self.haplotype_names, dtype=object)
        data["representative"] = names[self.first[rows]] if len(rows) else np.zeros(0, dtype=object)
        data["is_reference"] = self.is_reference[rows]
        sides = {}
        for side, kmers in (("ref", self.ref_kmer), ("alt", self.alt_kmer)):
            sides[side] = sc, pv, strand, off, _, la = self._side(recs, side)
            data[f"{side}_score"], data[f"{side}_pvalue"], data[f"{side}_strand"] = sc, pv, strand
            data[f"{side}_offset"], data[f"{side}_kmer"] = off, kmers[rows]
        data["delta_score"] = sides["alt"][0] - sides["ref"][0]
        data["ref_log2_affinity"], data["alt_log2_affinity"] = sides["ref"][5], sides["alt"][5]
        data["delta_log2_affinity"] = sides["alt"][5] - sides["ref"][5]
        data["effect"] = self.effects(recs)
        return pd.DataFrame(data)

    def to_frame(self) -> pd.DataFrame:
        """the summary, a row per kept variant: motif_id, motif_alt_id, chrom, pos, id, ref, alt, haplotypes_applied,
        haplotypes_absent, haplotypes_mismatch, contexts, reference_effect, reference_delta_score (empty / NaN when the edit does
        not apply to the reference sequence), haplotypes_gain / _loss / _both / _none, min_delta_score, max_delta_score,
        mean_delta_log2_affinity (haplotype-weighted), background_dependent (the applied contexts do not all share one effect)"""
        R = len(self.pos0)
        at = np.flatnonzero(self.kept())
        var = self.context_variant
        eff = self.effects(self.records)
        ref_s, alt_s = self._side(self.records, "ref"), self._side(self.records, "alt")
        delta, dla = alt_s[0] - ref_s[0], alt_s[5] - ref_s[5]
        data = self._variant_columns(at)
        data["haplotypes_applied"], data["haplotypes_absent"] = self.haplotypes_applied[at], self.haplotypes_absent[at]
        data["haplotypes_mismatch"] = self.haplotypes_mismatch[at]
        data["contexts"] = np.diff(self.context_offsets)[at]
        on_ref = self.reference["status"] == nv.GFM_EDIT_APPLIED
        r_ref, r_alt = self._side(self.reference, "ref"), self._side(self.reference, "alt")
        data["reference_effect"] = np.where(on_ref, self.effects(self.reference), "").astype(object)[at]
        data["reference_delta_score"] = np.where(on_ref, r_alt[0] - r_ref[0], np.nan)[at]
        for name in ("gain", "loss", "both", "none"):
            n = np.zeros(R, dtype=np.int64)
            np.add.at(n, var[eff == name], self.count[eff == name])
            data[f"haplotypes_{name}"] = n[at]
        lo, hi = np.full(R, np.inf), np.full(R, -np.inf)
        some = ~np.isnan(delta)
        np.minimum.at(lo, var[some], delta[some])
        np.maximum.at(hi, var[some], delta[some])
        data["min_delta_score"] = np.where(np.isfinite(lo), lo, np.nan)[at]
        data["max_delta_score"] = np.where(np.isfinite(hi), hi, np.nan)[at]
        num, den = np.zeros(R), np.zeros(R)
        some = ~np.isnan(dla)
        np.add.at(num, var[some], dla[some] * self.count[some])
        np.add.at(den, var[some], self.count[some].astype(np.float64))
        data["mean_delta_log2_affinity"] = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)[at]
        kinds = np.zeros((R, 4), dtype=bool)
        kinds[var, self.effect_codes(self.records)] = True
        data["background_dependent"] = (kinds.sum(axis=1) > 1)[at]
        return pd.DataFrame(data)


def _own_chromosomes(graph, chrom_names):
    """-> [(name, DeviceGraph or GraphIndex)], one per distinct chromosome graph of `graph`"""
    if graph is None:
        raise ValueError("no graph: a DeviceGraph / GraphIndex, a list of them, or a scan_graph manifest")
    if isinstance(graph, dict):
        prep = prepare_graphs(graph, None, None)
        return [(g.index.chrom, g) for g in prep.graphs]
    entries = list(graph) if isinstance(graph, (list, tuple)) else [graph]
    names = ([chrom_names] if isinstance(chrom_names, str) else list(chrom_names)) if chrom_names is not None else \
        [(g.chrom if isinstance(g, GraphIndex) else g.index.chrom) for g in entries]
    if len(names) != len(entries):
        raise ValueError("one chromosome name per graph")
    out = []
    for name, g in zip(names, entries):
        if not any(x is g for _, x in out):
            out.append((name, g))
    return out


def _find_chromosome(chroms, name: str) -> int:
    strip = lambda s: s[3:] if s.lower().startswith("chr") else s          # noqa: E731
    for k, (c, _) in enumerate(chroms):
        if c == name or strip(c) == strip(name):
            return k
    return -1


def _sequences_and_items(hs, indexes, v_graph, S, E):
    """The sequences of one kernel call: the versions of `hs` (the footprints' haplotype sequences), then per variant the
    reference's own footprint; item n is sequence n with its variant's edit -> (seq_offsets, bases, coord, item_edit, the
    references' bases per variant)"""
    R = len(S)
    seq_offsets = np.concatenate([hs.seq_offsets, hs.seq_offsets[-1] + np.cumsum(E - S)]).astype(np.int64)
    ref_bases = [indexes[g].ref[s:e] for g, s, e in zip(v_graph.tolist(), S.tolist(), E.tolist())]
    bases = np.concatenate([hs.bases] + ref_bases) if R else hs.bases
    coord = np.concatenate([hs.coord] + [np.arange(s, e, dtype=np.int32) for s, e in zip(S.tolist(), E.tolist())]) if R else hs.coord
    return seq_offsets, bases, coord, np.concatenate([hs.version_region, np.arange(R, dtype=np.int64)]), ref_bases


def compute_query_variants_many(motifs: Sequence, graph, variants: Sequence, debug: bool, args_obj, chrom_names=None,
                                haplotype_names: Optional[Sequence[str]] = None, haplotype_groups: Optional[Mapping] = None,
                                temperature: float = 1.0, threshold: Optional[float] = None, all_variants: bool = False,
                                weights: Optional[Sequence[np.ndarray]] = None,
                                skip_unusable: bool = False) -> List[QueryVariants]:
    """One QueryVariants per motif, in the order of `motifs` (see the module's docstring).  `graph`: a DeviceGraph or GraphIndex,
    a list of them (one per chromosome, the chromosomes share one haplotype set), or a scan_graph manifest; `variants`:
    [(chrom, pos 1-based, id, ref, alt)] or what read_query_vcf returns.  A variant's chromosome is matched against the graphs'
    (`chrom_names`, default their own; a leading "chr" does not count); variants on chromosomes without a graph are skipped and
    counted in one warning.  A variant the table cannot take (unusable: an allele of more than MAX_ALLELE bases after trimming,
    REF equal to ALT, an allele that is no plain base string, a REF outside the chromosome) is a ValueError that names it; with
    `skip_unusable` such variants are skipped and counted in one warning that names the first.  args_obj: noreverse
    and threshold (`threshold` overrides it).  `haplotype_groups` as compute_haplotype_classes takes them; `temperature` / `weights` as compute_haplotype_affinity_many's.  Unless `all_variants`,
    the frames keep a variant only if some context has an effect other than none."""
    from .device import DeviceMotif
    from .graph_tables import _haplotype_set
    from .haplotype_classes import compute_haplotype_classes
    from .haplotype_sequences import compute_haplotype_sequences
    require_single_gpu("the query variants", "are", "a gather of the sharded class matrices")
    if weights is not None and len(weights) != len(motifs):
        raise ValueError(f"{len(weights)} weight tables for {len(motifs)} motifs")
    chroms = _own_chromosomes(graph, chrom_names)
    graphs = [g for _, g in chroms]
    none = [np.zeros((0, 2), dtype=np.int64)] * len(graphs)
    _, names = _haplotype_set(prepare_graphs(graphs, none, [c for c, _ in chroms]), haplotype_names, "the query variant table")
    indexes = [g if isinstance(g, GraphIndex) else g.index for g in graphs]
    # ---- the variants: on a graph's chromosome, normalised; rows in (graph, given) order
    rows, skipped, refused = [], 0, []
    for n, v in enumerate(variants):
        chrom, pos, vid, ref, alt = str(v[0]), int(v[1]), str(v[2]), str(v[3]), str(v[4])
        gi = _find_chromosome(chroms, chrom)
        if gi < 0:
            skipped += 1
            continue
        why = unusable(chrom, pos, vid, ref, alt, len(indexes[gi].ref))
        if why is not None:
            if not skip_unusable:
                raise ValueError(why)
            refused.append(why)
            continue
        pos0, nref, nalt = normalise(pos, ref, alt)
        rows.append((gi, n, (chrom, pos, vid, ref, alt), (pos0, nref.upper(), nalt.upper())))
    if skipped:
        warnings.warn(f"{skipped} query variants lie on chromosomes without a graph and were skipped")
    if refused:
        warnings.warn(f"{len(refused)} query variants were skipped, the first: {refused[0]}")
    rows.sort(key=lambda r: (r[0], r[1]))
    R = len(rows)
    given = [r[2] for r in rows]
    norm = [r[3] for r in rows]
    v_graph = np.array([r[0] for r in rows], dtype=np.int64)
    pos0 = np.array([n[0] for n in norm], dtype=np.int64)
    lr = np.array([len(n[1]) for n in norm], dtype=np.int64)
    chrom_len = np.array([len(indexes[g].ref) for g in v_graph.tolist()], dtype=np.int64)
    forward_only = bool(getattr(args_obj, "noreverse", False))
    threshold = float(args_obj.threshold if threshold is None else threshold)
    out: List[Optional[QueryVariants]] = [None] * len(motifs)
    for W, idxs in group_by_width(motifs).items():
        # ---- the footprints as regions, their classes and versions
        regions = []
        S, E = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
        for gi, index in enumerate(indexes):
            mine = np.flatnonzero(v_graph == gi)
            S[mine], E[mine] = footprints(index, pos0[mine], lr[mine], W)
            regions.append(np.stack([S[mine], E[mine]], axis=1))
        names_in = [c for c, _ in chroms]
        hc = compute_haplotype_classes(graphs, regions, debug, args_obj, names_in, names, haplotype_groups)
        hs = compute_haplotype_sequences(graphs, regions, debug, args_obj, names_in, names, None, classes=hc, coordinates=True)
        V = len(hs)
        G = len(hs.group_names)
        version_variant = hs.version_region
        seq_offsets, bases, coord, item_edit, ref_bases = _sequences_and_items(hs, indexes, v_graph, S, E)
        dms = [DeviceMotif.lease(motifs[i]) for i in idxs]
        try:
            tables, offsets = _weight_tables(dms, [motifs[i] for i in idxs], None if weights is None else [weights[i] for i in idxs],
                                             temperature)
            got = _launch(dms, tables, seq_offsets, bases, coord, pos0, [n[1] for n in norm], [n[2] for n in norm],
                          np.arange(V + R, dtype=np.int64), item_edit, forward_only)
            # the sequence's end is the chromosome's only when pos0 is its length: else the base pos0 is missing
            recs = got[0]
            at_end = (recs["o"] == np.diff(seq_offsets)) & (lr[item_edit] == 0) & (pos0[item_edit] < chrom_len[item_edit]) & \
                (recs["status"] != nv.GFM_EDIT_ABSENT)
            for m in range(len(idxs)):
                got[m]["status"][at_end] = nv.GFM_EDIT_ABSENT
                for f in ("ref_key", "alt_key", "ref_sum", "alt_sum"):
                    got[m][f][at_end] = 0
            # ---- the contexts (they do not depend on the motif: the first motif's statuses and offsets are everyone's)
            status, o = got[0]["status"][:V], got[0]["o"][:V]
            hap_status = np.zeros((R, 3), dtype=np.int64)
            np.add.at(hap_status, (version_variant, status), hs.count.astype(np.int64))
            version_context = np.full(V, -1, dtype=np.int64)
            c_off, c_count, c_first, c_groups, c_ref, c_head = [0], [], [], [], [], []
            raw = hs.bases.tobytes()
            for r in range(R):
                a, b = int(hs.offsets[r]), int(hs.offsets[r + 1])
                ok = np.flatnonzero(status[a:b] == nv.GFM_EDIT_APPLIED) + a
                keys = [used_context(raw[hs.seq_offsets[v]:hs.seq_offsets[v + 1]], int(o[v]), int(lr[r]), W) for v in ok.tolist()]
                ref_key = used_context(ref_bases[r].tobytes(), int(pos0[r] - S[r]), int(lr[r]), W)
                of, n_, f_, g_, _, h_ = merge_contexts(keys, hs.count[ok], hs.first[ok], hs.group_counts[ok],
                                                       np.zeros(len(ok), dtype=bool))
                version_context[ok] = of
                c_off.append(c_off[-1] + len(n_))
                c_count.append(n_); c_first.append(f_); c_groups.append(g_); c_head.append(ok[h_])
                c_ref.append(np.array([keys[k] == ref_key for k in h_.tolist()], dtype=bool))
            cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)      # noqa: E731
            head = cat(c_head, np.int64).astype(np.int64)
            groups = np.concatenate(c_groups) if c_groups else np.zeros((0, G), dtype=np.int64)
            head_var = version_variant[head] if len(head) else np.zeros(0, dtype=np.int64)
            for m, i in enumerate(idxs):
                dm = dms[m]
                crecs = got[m][:V][head]
                kmers = {"ref": [], "alt": []}
                for side in ("ref", "alt"):
                    _, rel, strand = decode_keys(crecs[side + "_key"])
                    for k, v in enumerate(head.tolist()):
                        if not strand[k]:
                            kmers[side].append("")
                            continue
                        r = int(head_var[k])
                        x = raw[hs.seq_offsets[v]:hs.seq_offsets[v + 1]]
                        oo = int(crecs["o"][k])
                        if side == "alt":
                            x = x[:oo] + norm[r][2].encode() + x[oo + int(lr[r]):]
                        kmers[side].append(_kmer(x, int(rel[k]), oo, strand[k], W))
                out[i] = QueryVariants(motifs[i].motif_id, motifs[i].motif_name, W, dm.scale, dm.offset, dm.ptable_host(), offsets[m],
                                       threshold, names, hs.group_names, given, norm, hap_status, c_off, cat(c_count, np.int64),
                                       cat(c_first, np.int64), groups, cat(c_ref, bool), crecs, kmers["ref"], kmers["alt"],
                                       got[m][V:], version_variant, hs.count, got[m][:V], version_context, all_variants)
        finally:
            for dm in dms:
                dm.release()
    return out


def compute_query_variants(motif, graph, variants, debug: bool, args_obj, chrom_names=None,
                           haplotype_names: Optional[Sequence[str]] = None, haplotype_groups: Optional[Mapping] = None,
                           temperature: float = 1.0, threshold: Optional[float] = None, all_variants: bool = False,
                           weights: Optional[np.ndarray] = None, skip_unusable: bool = False) -> QueryVariants:
    """The query variant table of `motif` (compute_query_variants_many for one motif)"""
    return compute_query_variants_many([motif], graph, variants, debug, args_obj, chrom_names, haplotype_names, haplotype_groups,
                                       temperature, threshold, all_variants, None if weights is None else [weights],
                                       skip_unusable)[0]


# ---------------------------------------------------------------------------------------------------------------- the writers
def write_query_variants(table: QueryVariants, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_query_variants.tsv (grafimo_query_variants_<motif_id>.tsv for one of several motifs), the summary, in the
    directory write_results uses for this motif -> the path written.  `out`: a text stream to write to instead (-f: stdout)."""
    return write_frame(table.to_frame(), out if out is not None else table_path(SUMMARY_FILE, args_obj, motif, motif_num))


def write_query_variant_contexts(table: QueryVariants, motif, motif_num: int, args_obj, out=None) -> Optional[str]:
    """grafimo_query_variant_contexts[_<motif_id>].tsv, a row per (variant, context), beside the summary"""
    return write_frame(table.contexts_frame(), out if out is not None else table_path(CONTEXTS_FILE, args_obj, motif, motif_num))


def print_query_variants(table: QueryVariants) -> None:
    """-f: the summary, then the contexts, on stdout instead of files"""
    write_query_variants(table, None, 1, None, out=sys.stdout)
    write_query_variant_contexts(table, None, 1, None, out=sys.stdout)
