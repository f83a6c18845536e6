"""The query-variant table on the GPU: the kernel through score_edits against the rule restated with numpy / Python integers
on random sequences, the table against the brute force (tests/query_variant_bruteforce.py) on the class table's fuzz graphs and on
bitset graphs of odd haplotype counts, the refusals and the command line."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_panel_cases as wp  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402
from graph_table_checks import random_bitset_index  # noqa: E402
from graph_tables_fuzz_core import make_graph  # noqa: E402
from query_variant_bruteforce import ABSENT, APPLIED, MISMATCH, side, variant_expected  # noqa: E402
from variant_bruteforce import haplotype_classes  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
SEEDS = list(range(21)) + [21, 24]                           # (test_gpu_haplotype_classes.py: every kind string occurs)
ODD_H = (63, 65, 129)
GRAPHS = [f"seed{s}" for s in SEEDS] + [f"bits{h}" for h in ODD_H]
KINDS = [(1, 1), (3, 3), (0, 1), (0, 64), (1, 0), (64, 0), (64, 64)]
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


# ------------------------------------------------------------------------------------------- the kernel through score_edits
def _kernel_locate(x: bytes, coord, pos0: int, ref: bytes):
    """the entry's rule (include/grafimo_hip.h): it has no chromosome, a sequence that ends on the base pos0 - 1 ends it"""
    at = {int(c): j for j, c in enumerate(coord) if c >= 0}
    lr = len(ref)
    if lr:
        if any(pos0 + k not in at for k in range(lr)):
            return ABSENT, at.get(pos0, -1)
        o = at[pos0]
        ok = all(at[pos0 + k] == o + k for k in range(lr)) and x[o:o + lr].upper() == ref.upper()
        return (APPLIED if ok else MISMATCH), o
    if pos0 in at:
        o = at[pos0]
        return (ABSENT if pos0 - 1 not in at else APPLIED if at[pos0 - 1] == o - 1 else MISMATCH), o
    if pos0 - 1 in at and at[pos0 - 1] == len(x) - 1:
        return APPLIED, len(x)
    if pos0 - 1 in at and int(coord[-1]) == ~(pos0 - 1):
        return MISMATCH, len(x)
    return ABSENT, -1


def _key(best):
    return 0 if best is None else ((best[0] + 1) << 8) | ((64 - best[1]) << 1) | int(best[2] == "+")


def _kernel_expected(x, coord, pos0, ref, alt, W, sm, min_val, wtab, fwd):
    status, o = _kernel_locate(x, coord, pos0, ref)
    if status != APPLIED:
        return (status, o, 0, 0, 0, 0)
    alt = bytes(c if c in b"ACGTacgt" else ord("N") for c in alt)
    rb, rs = side(x, o, len(ref), W, sm, min_val, wtab, fwd)
    ab, as_ = side(x[:o] + alt + x[o + len(ref):], o, len(alt), W, sm, min_val, wtab, fwd)
    return (status, o, _key(rb), _key(ab), rs, as_)


def _sequence(rng, start, n, inserted=(), deleted=(), n_at=()):
    """n reference coordinates from `start`, those in `deleted` left out, `inserted`: {coordinate: bases inserted behind it},
    n_at: offsets that hold an N -> (bases bytes, coord int32 list)"""
    x, c = bytearray(), []
    for p in range(start, start + n):
        if p in deleted:
            continue
        x.append(int(BASES[rng.integers(0, 4)])); c.append(p)
        for _ in range(dict(inserted).get(p, 0)):
            x.append(int(BASES[rng.integers(0, 4)])); c.append(~p)
    for j in n_at:
        if 0 <= j < len(x):
            x[j] = ord("N")
    return bytes(x), c


def _cases(W, rng):
    """-> (sequences [(bases, coord)], edits [(pos0, ref, alt)], items [(seq, edit)]) for motif width W"""
    seqs, edits, items = [], [], []

    def add(x, c, pos0, ref, alt):
        seqs.append((x, c)); edits.append((pos0, ref, alt)); items.append((len(seqs) - 1, len(edits) - 1))

    def ref_of(x, c, pos0, lr):
        at = {p: j for j, p in enumerate(c) if p >= 0}
        return bytes(x[at[pos0 + k]] for k in range(lr))

    alt_of = lambda la: bytes(BASES[rng.integers(0, 4, size=la)])          # noqa: E731
    start = int(rng.integers(0, 1000))
    for lr, la in KINDS:
        n = 2 * W + lr + 40
        for where in ("middle", "left", "right"):                          # o >= W - 1 .. ; o < W - 1; o > len - W: clipping
            x, c = _sequence(rng, start, n)
            pos0 = start + {"middle": W + 20, "left": min(W // 2, 1), "right": n - lr - min(W // 2, 1)}[where]
            add(x, c, pos0, ref_of(x, c, pos0, lr), alt_of(la))
        x, c = _sequence(rng, start, max(lr + 1, 2))                       # shorter than W (W > lr + 1): a side has no window
        add(x, c, start + 1, ref_of(x, c, start + 1, min(lr, len(x) - 1)), alt_of(la))
        x, c = _sequence(rng, start, n, n_at=(W + 19, W + 21 + lr))         # an N on each side of the edit
        add(x, c, start + W + 20, ref_of(x, c, start + W + 20, lr), alt_of(la))
        x, c = _sequence(rng, start, n)                                     # a lower-case REF, an ALT with a base that is none
        alt = alt_of(la)
        add(x, c, start + W + 20, ref_of(x, c, start + W + 20, lr).lower(), (b"R" + alt[1:]) if la else alt)
        if lr:
            x, c = _sequence(rng, start, n)                                 # REF differs: a mismatch
            ref = bytearray(ref_of(x, c, start + W + 20, lr))
            ref[-1] = ord("A") if ref[-1] != ord("A") else ord("C")
            add(x, c, start + W + 20, bytes(ref), alt_of(la))
            x, c = _sequence(rng, start, n, deleted={start + W + 20 + lr - 1})   # the last REF coordinate is deleted: absent
            add(x, c, start + W + 20, b"A" * lr, alt_of(la))
        if lr >= 3:
            x, c = _sequence(rng, start, n, inserted={start + W + 21: 2})   # an inserted base inside the REF span
            add(x, c, start + W + 20, ref_of(x, c, start + W + 20, lr), alt_of(la))
        if lr == 0:
            x, c = _sequence(rng, start, n, inserted={start + W + 19: 3})   # inserted bases in the junction: a mismatch
            add(x, c, start + W + 20, b"", alt_of(la))
            x, c = _sequence(rng, start, n)                                 # behind the last base
            add(x, c, start + n, b"", alt_of(la))
            x, c = _sequence(rng, start, n, inserted={start + n - 1: 2})    # ... which carries an insertion: a mismatch at len
            add(x, c, start + n, b"", alt_of(la))
            add(x, c, start, b"", alt_of(la))                               # before the first base: absent
    x, c = _sequence(rng, start, 10, inserted={start + 3: 70})              # (an insertion longer than a wavefront before o)
    add(x, c, start + 7, ref_of(x, c, start + 7, 1), b"G")
    add(b"", [], start, b"A", b"C")                                         # an empty sequence
    for _ in range(6):                                                      # edits on other sequences: mostly absent
        items.append((int(rng.integers(0, len(seqs))), int(rng.integers(0, len(edits)))))
    if len(items) % 4 == 0:
        items.append((0, 0))
    return seqs, edits, items


@pytest.mark.parametrize("W", [1, 5, 19, 64])
def test_kernel_against_numpy(W):
    from grafimo_amd.query_variants import score_edits
    rng = np.random.default_rng(52_000 + W)
    seqs, edits, items = _cases(W, rng)
    motifs = [SynMotif(W, seed=900 + k) for k in range(3)]
    ods = [motif_as_oracle_dict(m) for m in motifs]
    weights = [rng.integers(1, 1 << 40, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    off = np.concatenate([[0], np.cumsum([len(x) for x, _ in seqs])]).astype(np.int64)
    bases = np.frombuffer(b"".join(x for x, _ in seqs), dtype=np.uint8)
    coord = np.array([p for _, c in seqs for p in c], dtype=np.int32)
    args = (off, bases, coord, [e[0] for e in edits], [e[1] for e in edits], [e[2] for e in edits], [i[0] for i in items],
            [i[1] for i in items])
    assert len(items) % 4 != 0
    expected = {}
    for fwd in (False, True):
        got = score_edits(motifs, *args, weights=weights, forward_only=fwd)
        assert len(got) == 3 and all(g.shape == (len(items),) for g in got)
        seen = set()
        expected[fwd] = [[_kernel_expected(seqs[s][0], seqs[s][1], *edits[e], W, od["score_matrix"], od["min_val"], weights[m], fwd)
                          for s, e in items] for m, od in enumerate(ods)]
        for m in range(3):
            for n, (s, e) in enumerate(items):
                exp = expected[fwd][m][n]
                assert tuple(int(v) for v in got[m][n]) == exp, (W, fwd, m, n, len(seqs[s][0]), edits[e], got[m][n], exp)
                seen.add((exp[0], exp[2] != 0, exp[3] != 0))
        # applied with and without windows on either side, absent, mismatch
        assert {(APPLIED, True, True), (ABSENT, False, False), (MISMATCH, False, False)} <= seen, seen
        assert W == 1 or (APPLIED, False, False) in seen or (APPLIED, False, True) in seen
    _second_call_on_the_same_buffers(motifs, weights, args, items, len(seqs), expected)
    # the default weights: haplotype_affinity's
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.haplotype_affinity import default_weights
    got = score_edits(motifs[:1], *args, temperature=2.0)[0]
    dm = DeviceMotif.lease(motifs[0])
    try:
        w = default_weights(dm, 2.0)[0]
    finally:
        dm.release()
    for n, (s, e) in enumerate(items):
        exp = _kernel_expected(seqs[s][0], seqs[s][1], *edits[e], W, ods[0]["score_matrix"], ods[0]["min_val"], w, False)
        assert tuple(int(v) for v in got[n]) == exp, (W, n)


def _second_call_on_the_same_buffers(motifs, weights, args, items, n_seqs, expected):
    """The inputs staged ONCE, one record tensor and one status word for every call, both dirty before each: every record is
    written on every path (applied, absent, mismatch, invalid) and the entry clears the status word itself, also after a call
    it refused"""
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd import query_variants as qv
    from grafimo_amd.device import DeviceMotif
    N = len(items)
    dms = [DeviceMotif.lease(m) for m in motifs]
    try:
        staged = qv._stage(weights, *args)
        spoiled = qv._stage(weights, *args[:6], list(args[6][:-1]) + [n_seqs], args[7])      # the last item: no such sequence
        rec = torch.full((len(motifs), N, 4), -1, dtype=torch.int64, device="cuda")
        status = torch.full((1,), 7, dtype=torch.int32, device="cuda")

        def records():
            return rec.cpu().numpy().view(qv.RECORD).reshape(len(motifs), N)

        def check(fwd, upto):
            got = records()
            for m in range(len(motifs)):
                for n in range(upto):
                    assert tuple(int(v) for v in got[m][n]) == expected[fwd][m][n], (fwd, m, n)

        assert qv._enqueue(dms, staged, True, rec, status) is rec
        check(True, N)
        assert int(status.item()) == 0
        for again in range(2):                                # the other strand setting over the last call's records, twice
            qv._enqueue(dms, staged, False, rec, status)
            check(False, N)
        rec.fill_(0x5A5A5A5A5A5A5A5A)
        with pytest.raises(nv.NativeError, match="out of range"):
            qv._enqueue(dms, spoiled, False, rec, status)
        assert int(status.item()) != 0
        check(False, N - 1)                                   # the refused call still wrote every record: the bad item's says so
        assert (records()[:, N - 1]["status"] == nv.GFM_EDIT_INVALID).all() and (records()[:, N - 1]["ref_key"] == 0).all()
        rec.fill_(-1)
        qv._enqueue(dms, staged, True, rec, status)           # the word the refused call left set is cleared by the entry
        check(True, N)
        assert int(status.item()) == 0
    finally:
        for dm in dms:
            dm.release()


def test_seventeen_motifs_take_two_launches():
    """more motifs of one width than one launch holds (16): the second launch's tables, weights and record buffers"""
    from grafimo_amd.query_variants import score_edits
    W = 5
    rng = np.random.default_rng(53_000)
    seqs, edits, items = _cases(W, rng)
    items = items[::2]
    motifs = [SynMotif(W, seed=1200 + k) for k in range(17)]
    weights = [rng.integers(1, 1 << 40, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    off = np.concatenate([[0], np.cumsum([len(x) for x, _ in seqs])]).astype(np.int64)
    got = score_edits(motifs, off, np.frombuffer(b"".join(x for x, _ in seqs), dtype=np.uint8),
                      np.array([p for _, c in seqs for p in c], dtype=np.int32), [e[0] for e in edits], [e[1] for e in edits],
                      [e[2] for e in edits], [i[0] for i in items], [i[1] for i in items], weights=weights)
    assert len(got) == 17
    for m, motif in enumerate(motifs):
        od = motif_as_oracle_dict(motif)
        for n, (s, e) in enumerate(items):
            exp = _kernel_expected(seqs[s][0], seqs[s][1], *edits[e], W, od["score_matrix"], od["min_val"], weights[m], False)
            assert tuple(int(v) for v in got[m][n]) == exp, (m, n)
    assert len({tuple(int(v) for v in got[m][0]) for m in (0, 15, 16)}) == 3      # (three motifs, three answers)


def test_no_item_is_a_no_op_and_the_entry_refuses():
    from grafimo_amd import _native as nv
    from grafimo_amd.query_variants import score_edits
    assert nv.lib().gfm_graph_query_edits(None, 1, None, 1, 0, None, None, None, 0, None, None, None, None, None, 0, None, None, 0, None,
                                          None, None) == nv.GFM_OK
    assert nv.lib().gfm_graph_query_edits(None, 1, None, 1, 0, None, None, None, 0, None, None, None, None, None, 0, None, None, 2, None,
                                          None, None) == nv.GFM_ERR_INVALID
    assert nv.lib().gfm_graph_query_edits(None, 1, None, 1, 0, None, None, None, 0, None, None, None, None, None, 1, None, None, 0, None,
                                          None, None) == nv.GFM_ERR_INVALID           # a NULL pointer
    m5, m7 = SynMotif(5, seed=1), SynMotif(7, seed=2)
    x = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)
    seq = ([0, 12], x, np.arange(12, dtype=np.int32))
    assert [len(g) for g in score_edits([m5], *seq, [3], [b"T"], [b"A"], [], [])] == [0]
    with pytest.raises(nv.NativeError, match="one width"):
        score_edits([m5, m7], *seq, [3], [b"T"], [b"A"], [0], [0])
    with pytest.raises(nv.NativeError, match="longer than 64"):
        score_edits([m5], *seq, [3], [b"T" * 65], [b"A"], [0], [0])
    with pytest.raises(nv.NativeError, match="longer than 64"):
        score_edits([m5], *seq, [3], [b""], [b""], [0], [0])                 # (or both are empty)
    for s, e in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        with pytest.raises(nv.NativeError, match="out of range"):
            score_edits([m5], *seq, [3], [b"T"], [b"A"], [0, s], [0, e])
    with pytest.raises(nv.NativeError, match="may pass 2\\^64"):
        score_edits([m5], *seq, [3], [b"T"], [b"A"], [0], [0], weights=[np.full(5001, 1 << 63, dtype=np.uint64)])
    got = score_edits([m5], *seq, [3], [b"T"], [b"A"], [0], [0])[0]           # the handle afterwards: exact
    od = motif_as_oracle_dict(m5)
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.haplotype_affinity import default_weights
    dm = DeviceMotif.lease(m5)
    try:
        w = default_weights(dm, 1.0)[0]
    finally:
        dm.release()
    assert tuple(int(v) for v in got[0]) == _kernel_expected(x.tobytes(), seq[2], 3, b"T", b"A", 5, od["score_matrix"], od["min_val"], w, False)


# ------------------------------------------------------------------------------------------- the table against the brute force
@functools.lru_cache(maxsize=None)
def _graph(name):
    import tempfile
    if name.startswith("seed"):
        seed = int(name[4:])
        with tempfile.TemporaryDirectory() as d:
            return make_graph(seed, np.random.default_rng(70_000 + seed), d)[0]
    H = int(name[4:])
    rng = np.random.default_rng(71_500 + H)
    return random_bitset_index(H, 81_500 + H, length=int(rng.integers(150, 360)), n_sites=int(rng.integers(4, 36)))


def _variants(idx, rng):
    """query variants at and next to panel sites, inside and beside panel deletions and insertions, at both chromosome ends,
    with a REF that disagrees with the reference, and anywhere"""
    ref = bytes(np.asarray(idx.ref))
    L, p = len(ref), np.asarray(idx.pos, dtype=np.int64)
    other = lambda b: bytes([int(rng.choice([c for c in b"ACGT" if c != b]))]).decode()      # noqa: E731
    out = []

    def snv(pos0, tag):
        if 0 <= pos0 < L:
            out.append(("c", pos0 + 1, tag, chr(ref[pos0]), other(ref[pos0])))

    def ins(anchor, tag, n=2):
        if 0 <= anchor < L:
            out.append(("c", anchor + 1, tag, chr(ref[anchor]), chr(ref[anchor]) + "".join(rng.choice(list("ACGT"), size=n))))

    def dele(anchor, n, tag):
        if 0 <= anchor and anchor + n < L:
            out.append(("c", anchor + 1, tag, ref[anchor:anchor + 1 + n].decode(), chr(ref[anchor])))

    pick = lambda a, k: [int(v) for v in rng.permutation(a)[:k]]            # noqa: E731
    for i in pick(np.arange(len(p)), 4):
        for d in (-1, 0, 1):
            snv(int(p[i]) + d, f"site{i}{d:+d}")
    subs = np.flatnonzero((idx.del_len == 0) & (idx.ins_len == 0))
    for i in pick(subs, 2):                                                 # REF = a panel ALT: applies to its carriers only
        a = chr(int(idx.alt_bases[i, 0]))
        out.append(("c", int(p[i]) + 1, f"alt{i}", a, other(ord(a))))
        out.append(("c", int(p[i]) + 1, f"panel{i}", chr(ref[p[i]]), a))    # the panel's own variant
    for i in pick(np.flatnonzero(idx.del_len > 0), 3):
        d = int(idx.del_len[i])
        snv(int(p[i]) + 1 + int(rng.integers(0, d)), f"indel{i}")
        snv(int(p[i]) + d + 1, f"behind{i}")
        dele(int(p[i]) + d - 1, 2, f"overlap{i}")
        ins(int(p[i]) + int(rng.integers(0, d + 1)), f"insdel{i}")
        dele(int(p[i]), d, f"same{i}")                                      # the panel's own deletion
    for i in pick(np.flatnonzero(idx.ins_len > 0), 3):
        ins(int(p[i]), f"atins{i}")
        snv(int(p[i]), f"anchor{i}")
        snv(int(p[i]) + 1, f"next{i}")
        dele(int(p[i]) - 1, 2, f"delins{i}")
    snv(0, "first"); snv(L - 1, "last"); ins(L - 1, "end", 3); dele(L - 3, 2, "tail")
    out.append(("c", 1, "front", chr(ref[0]), "GT" + chr(ref[0])))          # before the first base: pos0 0, absent everywhere
    out.append(("c", 2, "mnv", ref[1:4].decode(), "".join(other(b) for b in ref[1:4])))
    q = int(rng.integers(5, L - 5))
    out.append(("c", q + 1, "wrong", other(ref[q]), chr(ref[q])))           # REF disagrees with the reference
    out.append(("c", q + 1, "long", chr(ref[q]), chr(ref[q]) + "ACGT" * 16))   # 64 inserted bases
    for _ in range(5):
        snv(int(rng.integers(0, L)), "any")
    return out


def _motifs(name):
    k = GRAPHS.index(name)
    widths = [(5, 19), (7, 12), (1, 30), (3, 64)][k % 4]
    ms = [SynMotif(w, seed=300 + 7 * k + j) for j, w in enumerate(widths)]
    for j, m in enumerate(ms):
        m.motif_id, m.motif_name = f"Q{j}_{m.width}", f"q{j}"
    return ms


def _setup(name):
    idx = _graph(name)
    k = GRAPHS.index(name)
    rng = np.random.default_rng(74_000 + k)
    H = int(idx.n_haplotypes)
    groups = {"a": sorted(rng.choice(H, size=int(rng.integers(0, H + 1)), replace=False).tolist()), "all": list(range(H)), "none": []}
    return idx, _variants(idx, rng), _motifs(name), groups, bool(k % 5 == 3)


THRESHOLD = 0.25


@functools.lru_cache(maxsize=None)
def _expected(name):
    """the brute force alone -> per motif, per variant its expected rows (default weights restated: haplotype_affinity's formula)"""
    from oracle import oracle as orc
    from grafimo_amd.query_variants import normalise
    idx, variants, motifs, groups, fwd = _setup(name)
    classes, cache = haplotype_classes(idx), {}
    out = []
    for m in motifs:
        od = motif_as_oracle_dict(m)
        sm = od["score_matrix"]
        s_best = int(sm.max(axis=0).sum())
        s = np.minimum(np.arange(1000 * od["width"] + 1, dtype=np.int64), s_best)
        wtab = np.maximum(np.rint(np.exp2(40 + (s - s_best).astype(np.float64) / float(od["scale"]))), 1.0).astype(np.uint64)
        memo, rows = {}, []
        for v in variants:
            pos0, r, a = normalise(v[1], v[3], v[4])
            rows.append(variant_expected(idx, pos0, r.upper().encode(), a.upper().encode(), od["width"], sm, od["min_val"], wtab, fwd,
                                         list(groups.values()), classes, cache, memo))
        out.append((od, orc.p_table(od["pmf"]), rows))
    return out


def _effect(ptab, threshold, ref, alt):
    pr = ref is not None and ptab[ref[0]] < threshold
    px = alt is not None and ptab[alt[0]] < threshold
    return ["none", "gain", "loss", "both"][2 * int(pr) + int(px)]


@pytest.mark.parametrize("name", GRAPHS)
def test_table_against_the_brute_force(name):
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.graph_tables import scaled_pvalues, scaled_scores
    from grafimo_amd.query_variants import compute_query_variants_many
    idx, variants, motifs, groups, fwd = _setup(name)
    exp = _expected(name)
    g = DeviceGraph(idx)
    try:
        tables = compute_query_variants_many(motifs, g, variants, False, wp.Args(threshold=THRESHOLD, no_reverse=fwd),
                                             haplotype_groups=groups, all_variants=True)
    finally:
        g.close()
    for t, m, (od, _, rows) in zip(tables, motifs, exp):
        W = od["width"]
        assert len(t.pos0) == len(variants) == len(rows) and t.group_names == list(groups)
        assert [tuple(x) for x in zip(t.chrom, t.pos, t.vid, t.ref, t.alt)] == variants
        frame = t.contexts_frame()
        assert len(frame) == len(t.records) == int(t.context_offsets[-1])
        at = 0
        for r, e in enumerate(rows):
            ctx = (name, m.motif_id, variants[r])
            assert (int(t.haplotypes_applied[r]), int(t.haplotypes_absent[r]), int(t.haplotypes_mismatch[r])) == e["status"], ctx
            a, b = int(t.context_offsets[r]), int(t.context_offsets[r + 1])
            assert b - a == len(e["contexts"]), ctx
            status, res = e["reference"]
            assert int(t.reference["status"][r]) == status, ctx
            if status == APPLIED:
                assert (int(t.reference["ref_key"][r]), int(t.reference["alt_key"][r]), int(t.reference["ref_sum"][r]),
                        int(t.reference["alt_sum"][r])) == (_key(res[0]), _key(res[2]), res[1], res[3]), ctx
            for k, c in enumerate(e["contexts"]):
                row = a + k
                assert (int(t.count[row]), int(t.first[row]), t.group_counts[row].tolist(), bool(t.is_reference[row])) == \
                    (c["count"], c["first"], c["group_counts"], c["is_reference"]), ctx
                rec = t.records[row]
                assert int(rec["status"]) == APPLIED
                assert (int(rec["ref_key"]), int(rec["alt_key"])) == (_key(c["ref"]), _key(c["alt"])), (ctx, k, c)
                assert (int(rec["ref_sum"]), int(rec["alt_sum"])) == (c["ref_sum"], c["alt_sum"]), (ctx, k)
                assert (t.ref_kmer[row], t.alt_kmer[row]) == (c["ref"][3] if c["ref"] else "", c["alt"][3] if c["alt"] else ""), (ctx, k)
                # the frame's columns: the integers, and the floats the shared helpers make of them
                f = frame.iloc[at + k]
                assert (f["context"], f["haplotypes"], f["representative"]) == (k, c["count"], t.haplotype_names[c["first"]])
                for sd in ("ref", "alt"):
                    best = np.array([c[sd][0] if c[sd] else -1])
                    want = (scaled_scores(best, t.scale, t.offset, W)[0], scaled_pvalues(best, t.ptable)[0],
                            c[sd][2] if c[sd] else "", float(c[sd][1]) if c[sd] else np.nan, c[sd][3] if c[sd] else "")
                    have = (f[sd + "_score"], f[sd + "_pvalue"], f[sd + "_strand"], f[sd + "_offset"], f[sd + "_kmer"])
                    assert all((x == y) or (x != x and y != y) for x, y in zip(have, want)), (ctx, k, sd, have, want)
                    la = np.log2(float(c[sd + "_sum"])) + t.log2_offset if c[sd + "_sum"] else np.nan
                    assert f[sd + "_log2_affinity"] == la or (la != la and f[sd + "_log2_affinity"] != f[sd + "_log2_affinity"])
                assert f["effect"] == _effect(t.ptable, THRESHOLD, c["ref"], c["alt"]), (ctx, k)
            at += b - a
        # the unmerged kernel records agree inside every merged group
        on = t.version_context >= 0
        assert (t.version_records["status"][on] == APPLIED).all() and (t.version_records["status"][~on] != APPLIED).all()
        row_of = t.context_offsets[t.version_variant[on]] + t.version_context[on]
        for f in ("ref_key", "alt_key", "ref_sum", "alt_sum"):
            assert np.array_equal(t.version_records[f][on], t.records[f][row_of]), (name, f)
        # the summary's counts
        s = t.to_frame()
        assert len(s) == len(variants) and s["contexts"].tolist() == [len(e["contexts"]) for e in rows]
        effects = [[_effect(t.ptable, THRESHOLD, c["ref"], c["alt"]) for c in e["contexts"]] for e in rows]
        assert s["background_dependent"].tolist() == [len(set(x)) > 1 for x in effects]
        for kind in ("gain", "loss", "both", "none"):
            assert s[f"haplotypes_{kind}"].tolist() == [sum(c["count"] for c, x in zip(e["contexts"], fx) if x == kind)
                                                        for e, fx in zip(rows, effects)]
        kept = [any(x != "none" for x in fx) for fx in effects]
        assert t.kept().tolist() == [True] * len(variants)
        t.all_variants = False
        assert t.kept().tolist() == kept and len(t.to_frame()) == sum(kept)


def test_the_fuzz_holds_every_case():
    """with the brute force alone: the seeds' variants hold a variant whose contexts differ in their effect, absent and mismatch
    haplotypes, classes merged into one context, a reference the edit does not apply to, sides without a window"""
    dependent = absent = mismatch = merged = off_ref = no_window = contexts = 0
    for name in GRAPHS:
        for od, ptab, rows in _expected(name):
            for e in rows:
                effects = {_effect(ptab, THRESHOLD, c["ref"], c["alt"]) for c in e["contexts"]}
                dependent += int(len(effects) > 1)
                absent += int(e["status"][1] > 0)
                mismatch += int(e["status"][2] > 0)
                merged += sum(int(c["classes"] > 1) for c in e["contexts"])
                off_ref += int(e["reference"][0] != APPLIED)
                no_window += sum(int(c["ref"] is None or c["alt"] is None) for c in e["contexts"])
                contexts += len(e["contexts"])
    assert dependent >= 1 and absent >= 1 and mismatch >= 1 and merged >= 1 and off_ref >= 1 and no_window >= 1, \
        (dependent, absent, mismatch, merged, off_ref, no_window, contexts)


def test_versions_merge_into_one_context_on_the_hand_made_graph():
    """the table's side of the merge, on a graph where it can be read off (query_variant_bruteforce.hand_graph): A>C at 12 with
    W = 2 has the footprint [9, 14); haplotype 1 (a SNP at 9) and haplotype 3 (GG read behind 10) spell versions of their own
    there, but the bases next to 12 are the reference's: three versions, ONE context; haplotype 2 (10 and 11 deleted) is the
    other context"""
    from grafimo_amd.query_variants import compute_query_variants
    from query_variant_bruteforce import hand_graph
    idx = hand_graph()
    m = SynMotif(2, seed=77)
    od = motif_as_oracle_dict(m)
    t = compute_query_variants(m, idx, [("c", 13, "v", "A", "C")], False, wp.Args(threshold=0.5), haplotype_groups={"g": [1, 3]},
                               all_variants=True)
    assert t.version_variant.tolist() == [0, 0, 0, 0] and sorted(t.version_count.tolist()) == [1, 1, 1, 1]
    assert sorted(t.version_context.tolist()) == [0, 0, 0, 1] and (t.version_records["status"] == APPLIED).all()
    assert t.count.tolist() == [3, 1] and t.first.tolist() == [0, 2] and t.group_counts.tolist() == [[2], [0]]
    assert t.is_reference.tolist() == [True, False] and t.context_offsets.tolist() == [0, 2]
    assert (int(t.haplotypes_applied[0]), int(t.haplotypes_absent[0]), int(t.haplotypes_mismatch[0])) == (4, 0, 0)
    s = np.minimum(np.arange(2001, dtype=np.int64), int(od["score_matrix"].max(axis=0).sum()))
    wtab = np.maximum(np.rint(np.exp2(40 + (s - s.max()).astype(np.float64) / float(od["scale"]))), 1.0).astype(np.uint64)
    e = variant_expected(idx, 12, b"A", b"C", 2, od["score_matrix"], od["min_val"], wtab, groups=[[1, 3]])
    assert [c["members"] for c in e["contexts"]] == [[0, 1, 3], [2]]
    for k, c in enumerate(e["contexts"]):
        assert (int(t.records["ref_key"][k]), int(t.records["alt_key"][k]), int(t.records["ref_sum"][k]), int(t.records["alt_sum"][k])) \
            == (_key(c["ref"]), _key(c["alt"]), c["ref_sum"], c["alt_sum"]), k
        assert (t.ref_kmer[k], t.alt_kmer[k]) == (c["ref"][3], c["alt"][3])
    for f in ("ref_key", "alt_key", "ref_sum", "alt_sum"):                   # the unmerged records agree inside the merged group
        assert len(set(t.version_records[f][t.version_context == 0].tolist())) == 1


# ------------------------------------------------------------------------------------------- refusals, call forms, command line
def test_refusals(monkeypatch):
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.query_variants import MAX_ALLELE, compute_query_variants
    idx = random_bitset_index(7, 31, length=150, n_sites=10)
    ref = bytes(np.asarray(idx.ref))
    m = SynMotif(6, seed=4)
    assert MAX_ALLELE == 64
    with pytest.raises(ValueError, match="c:11 big .* an allele of 65 bases after trimming, at most 64"):
        compute_query_variants(m, idx, [("c", 11, "big", ref[10:76].decode(), chr(ref[10]))], False, wp.Args())
    with pytest.raises(ValueError, match="REF equals ALT"):
        compute_query_variants(m, idx, [("c", 11, "same", "A", "a")], False, wp.Args())
    with pytest.raises(ValueError, match="plain base strings"):
        compute_query_variants(m, idx, [("c", 11, "sym", "A", "<DEL>")], False, wp.Args())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        t = compute_query_variants(m, idx, [("zz", 11, "far", "A", "C"), ("chrc", 11, "near", chr(ref[10]), "C" if ref[10] != 67 else "G")],
                                   False, wp.Args(), all_variants=True)
    assert any("1 query variants lie on chromosomes without a graph" in str(x.message) for x in w)
    assert t.vid.tolist() == ["near"] and int(t.haplotypes_applied[0] + t.haplotypes_absent[0] + t.haplotypes_mismatch[0]) == 7
    # a REF that does not lie on the chromosome (a VCF of another assembly): refused by name, or skipped and counted
    near = ("c", 11, "near", chr(ref[10]), "C" if ref[10] != 67 else "G")
    with pytest.raises(ValueError, match="c:151 far A>C: REF lies outside the chromosome's 150 bases"):
        compute_query_variants(m, idx, [near, ("c", 151, "far", "A", "C")], False, wp.Args())
    for pos, r in ((0, "A"), (-3, "A"), (150, ref[149:150].decode() + "A")):
        with pytest.raises(ValueError, match="lies outside"):
            compute_query_variants(m, idx, [("c", pos, "off", r, "C")], False, wp.Args())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        t = compute_query_variants(m, idx, [("c", 151, "far", "A", "C"), near, ("c", 0, "zero", "A", "C"), ("c", 5, "iupac", "A", "R")],
                                   False, wp.Args(), all_variants=True, skip_unusable=True)
    assert any("3 query variants were skipped, the first: query variant c:151 far A>C" in str(x.message) for x in w)
    assert t.vid.tolist() == ["near"] and len(t.to_frame()) == 1
    none = compute_query_variants(m, idx, [], False, wp.Args())
    assert len(none) == 0 and len(none.to_frame()) == 0 and len(none.contexts_frame()) == 0
    bare = GraphIndex("c", np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([10], np.int32), np.array([1], np.uint8),
                      np.array([[ord("A"), 0, 0]], np.uint8), None, 0)
    with pytest.raises(ValueError, match="carries no haplotypes"):
        compute_query_variants(m, bare, [("c", 11, "v", "G", "C")], False, wp.Args())
    import torch
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="the query variants are computed on one GPU"):
        compute_query_variants(m, idx, [("c", 11, "v", "G", "C")], False, wp.Args())


def test_two_chromosomes_and_the_single_motif_form():
    from grafimo_amd.query_variants import compute_query_variants, compute_query_variants_many
    H = 65
    a = random_bitset_index(H, 4601, length=200, n_sites=20, chrom="a")
    b = random_bitset_index(H, 4602, length=160, n_sites=16, chrom="b")
    ra, rb = bytes(np.asarray(a.ref)), bytes(np.asarray(b.ref))
    flip = lambda c: "C" if c != ord("C") else "G"                          # noqa: E731
    variants = [("b", 31, "b30", chr(rb[30]), flip(rb[30])), ("a", int(a.pos[3]) + 1, "a3", chr(ra[a.pos[3]]), flip(ra[a.pos[3]])),
                ("b", int(b.pos[2]) + 2, "b2", chr(rb[b.pos[2] + 1]), flip(rb[b.pos[2] + 1]))]
    m = SynMotif(9, seed=11)
    both = compute_query_variants_many([m, m], [a, b], variants, False, wp.Args(threshold=0.3), all_variants=True)
    assert both[0].vid.tolist() == ["a3", "b30", "b2"]                      # rows in (graph, given) order
    one = compute_query_variants(m, [a, b], variants, False, wp.Args(threshold=0.3), all_variants=True)
    assert one.contexts_frame().equals(both[1].contexts_frame()) and one.to_frame().equals(both[0].to_frame())
    only_b = compute_query_variants(m, b, [variants[0], variants[2]], False, wp.Args(threshold=0.3), all_variants=True)
    cols = [c for c in one.to_frame().columns]
    assert one.to_frame()[one.to_frame()["chrom"] == "b"].reset_index(drop=True)[cols].equals(only_b.to_frame()[cols])
    assert (one.haplotypes_applied + one.haplotypes_absent + one.haplotypes_mismatch == H).all()


def test_manifest_route_equals_fasta_vcf_route(tmp_path, monkeypatch):
    """`graph` a scan_graph manifest: the same table as over the FASTA + VCF graph of the same chromosome"""
    import contextlib
    import io
    import shutil
    from grafimo_amd.extract_regions import GraphIndex, read_manifest, scan_graph
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.query_variants import compute_query_variants
    from grafimo_amd.workflow import Findmotif
    genome = tmp_path / "data" / "mygenome"
    shutil.copytree(os.path.join(GOLD, "mygenome"), genome)     # (scan_graph saves x.gfmidx.npz beside x.xg)
    monkeypatch.setenv("GRAFIMO_INDEX_CACHE", str(tmp_path / "cache"))
    bed = os.path.join(tmp_path, "x.bed")
    with open(os.path.join(GOLD, "regions.bed")) as src, open(bed, "w") as dst:
        dst.writelines(line for line in src if line.startswith("chrx\t"))
    wf = Findmotif(graph_genome_dir=str(genome), bedfile=bed, cores=2, threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "example.meme"), wf, 2, True, pvalue_matrix=False)[0]
    monkeypatch.setenv("GRAFIMO_SCAN_OUTPUT", "manifest")
    with contextlib.redirect_stdout(io.StringIO()):
        loc = scan_graph({motif.width}, wf, True)
    try:
        man = read_manifest(loc)
        assert man is not None
        idx = GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), "x")
        ref = bytes(np.asarray(idx.ref))
        sites = np.asarray(idx.pos)[:5].tolist()
        variants = [("x", p + 1 + d, f"v{p}{d}", chr(ref[p + d]), "C" if ref[p + d] != 67 else "G") for p in sites for d in (0, 1)]
        variants.append(("chrx", sites[0] + 1, "ins", chr(ref[sites[0]]), chr(ref[sites[0]]) + "TT"))
        a = compute_query_variants(motif, man, variants, False, wp.Args(threshold=0.05), haplotype_names=["p", "m"], all_variants=True)
        b = compute_query_variants(motif, idx, variants, False, wp.Args(threshold=0.05), haplotype_names=["p", "m"], all_variants=True)
        assert len(a.to_frame()) == len(variants) and (a.haplotypes_applied + a.haplotypes_absent + a.haplotypes_mismatch == 2).all()
        assert a.to_frame().equals(b.to_frame()) and a.contexts_frame().equals(b.contexts_frame())
        assert (np.diff(a.context_offsets) == 2).any() or (a.haplotypes_mismatch > 0).any()      # (the two haplotypes differ somewhere)
    finally:
        shutil.rmtree(loc, ignore_errors=True)


def test_cli_writes_both_files_and_prints_them(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.query_variants import compute_query_variants_many, read_query_vcf
    from grafimo_amd.workflow import Findmotif
    fa, vcf, bedfile = os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), os.path.join(GOLD, "regions.bed")
    bed = read_bed_regions(bedfile)
    graphs = [GraphIndex.from_fasta_vcf(fa, vcf, c[3:]) for c in bed]
    q = str(tmp_path / "query.vcf")
    with open(q, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        for g in graphs:
            ref = bytes(np.asarray(g.ref))
            for k, p in enumerate(np.asarray(g.pos)[:4].tolist() + [int(g.pos[0]) + 1, 40]):
                fh.write(f"{g.chrom}\t{p + 1}\t{g.chrom}{k}\t{chr(ref[p])}\t{'C' if ref[p] != 67 else 'G'},{chr(ref[p])}TT\n")
        fh.write("zz\t5\tnowhere\tA\tC\n")
        fh.write(f"{graphs[0].chrom}\t99999999\tbeyond\tA\tC\n")
        fh.write(f"{graphs[0].chrom}\t50\tlong\tA\tA{'ACGT' * 17}\n")
    base = [sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", fa, "-v", vcf, "-b", bedfile,
            "-t", "0.05"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = str(tmp_path / "o")
    r = subprocess.run(base + ["-o", out, "--query-variants", q, "--query-all"], check=True, cwd=str(tmp_path), env=env, timeout=600,
                       capture_output=True, text=True)
    assert "query variant rows written to" in r.stdout and "query variant context rows written to" in r.stdout
    assert "1 query variants with an allele of more than 64 bases" in r.stderr
    wf = Findmotif(threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "MA0139.1.meme"), wf, 2, True, pvalue_matrix=False)[0]
    assert "1 query variants were skipped, the first: query variant" in r.stderr and "beyond A>C: REF lies outside" in r.stderr
    variants = [v for v in read_query_vcf(q) if v[2] not in ("long", "beyond")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = compute_query_variants_many([motif], graphs, variants, False, wp.Args(threshold=0.05), all_variants=True)[0]
    assert len(t.to_frame()) == 2 * 6 * len(graphs) and len(t.contexts_frame()) >= len(t.to_frame())
    for stem, frame in (("grafimo_query_variants.tsv", t.to_frame()), ("grafimo_query_variant_contexts.tsv", t.contexts_frame())):
        assert open(os.path.join(out, stem)).read() == frame.to_csv(sep="\t", index=False, lineterminator="\n"), stem
    r = subprocess.run(base + ["-o", str(tmp_path / "p"), "-f", "--query-variants", q, "--query-all"], check=True, cwd=str(tmp_path),
                       env=env, timeout=600, capture_output=True, text=True)
    assert t.to_frame().to_csv(sep="\t", index=False, lineterminator="\n") in r.stdout
    assert t.contexts_frame().to_csv(sep="\t", index=False, lineterminator="\n") in r.stdout
    assert not os.path.exists(tmp_path / "p" / "grafimo_query_variants.tsv")
