"""A workgroup's second and later tiles, and a wavefront's second item.  The six tile-based sequence scans cap their grid
(kSeqMaxBlocks = 65 536 workgroups, the insertion scan kInsMaxBlocks = 4 096) and walk on with t += gridDim.x in the LDS the
last tile left; gfm_graph_query_edits gives a wavefront its next item 131 072 items on.  The calls of
tests/many_tiles_cases.py put a longer, N-bearing or differently placed tile exactly one grid before a shorter one, for
every scan, and every row of the call -- filler included -- is compared exactly with the Python brute force of its scan, run
once over the pool of distinct sequences and gathered.  tests/test_many_tiles_host.py shows on the CPU that the caps are the
library's and that the gather is the brute force over a whole call."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import many_tiles_cases as mt  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

pytestmark = pytest.mark.gpu
T = 64
LONG = b"ACGTTGCAAGGCTTAACCGGATATCGCGTATGCATGCAAGTCCTGAGGTTCCAAGGTCAGTCAA"
INSERTS = (b"A", b"CG", LONG[:19], LONG)
assert [len(i) for i in INSERTS] == [1, 2, 19, 64]
SIXTEEN = tuple(bytes(mt.BASES[(np.arange(n) * 7 + n) % 4].tolist()) for n in (3, 63, 11, 2, 33, 5, 8, 9, 17, 4, 21, 6)) + INSERTS
assert len(set(SIXTEEN)) == 16
E = 3                                                            # the site distance's cap on the edits


def _lengths(W):
    return (1, 64) if W == 64 else (1, 2, 7, 64)


# scan -> (module, brute force, the cap it runs under, the axis of its results that runs over the bases)
SCANS = {"mutation": ("mutation_scan", "mutation_scan_bruteforce", "seq", 0),
         "indel": ("indel_scan", "indel_scan_bruteforce", "seq", 0),
         "deletion": ("deletion_scan", "deletion_scan_bruteforce", "seq", 1),
         "substitution": ("substitution_scan", "substitution_scan_bruteforce", "seq", 1),
         "insertion": ("insertion_scan", "insertion_scan_bruteforce", "insertion", 1),
         "site_distance": ("site_distance", "site_distance_bruteforce", "seq", 0)}


def _extra(scan, W, inserts=INSERTS):
    """what the scan takes between the bases and the weights, as the existing kernel tests choose it"""
    return {"deletion": (_lengths(W),), "substitution": (_lengths(W), "CATG"), "insertion": (inserts,)}.get(scan, ())


@functools.lru_cache(maxsize=None)
def _case(W, n_motifs, seed, kept=None):
    """-> (pool, motifs, their oracle dicts, weight tables in [2^40, 2^55)).  `kept`: the lengths of the pool's members that
    stay, where a brute force would take too long over all of them (coverage() is asked of what is left)"""
    rng = np.random.default_rng(seed)
    pool = [x for x in mt.pool(W, T, rng) if kept is None or len(x) in kept]
    motifs = [SynMotif(W, seed=seed + 11 * k) for k in range(n_motifs)]
    weights = [rng.integers(1 << 40, 1 << 55, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    return pool, motifs, [motif_as_oracle_dict(m) for m in motifs], weights


@functools.lru_cache(maxsize=None)
def _cutoffs(*key):
    """as test_gpu_site_distance._kernel_case chooses them, on the pool: a quantile of the windows' own scores; at W >= 19 the
    first of a few quantiles at which the brute force shows, with E = 3, every d in 0 .. 4 on both sides"""
    import test_gpu_site_distance as tsd
    W = key[0]
    pool, _, ods, _ = _case(*key)
    out = []
    for od in ods:
        own = sorted(w[c] for w in tsd._brute(pool, od, 0, 1, False)[0] for c in (0, 1) if w[c] != tsd.bf.NO_WINDOW)
        picks = [own[int(q * (len(own) - 1))] for q in (0.6, 0.5, 0.7, 0.4, 0.8, 0.3, 0.9)]
        if W >= 19:
            picks = [c for c in picks if tsd._distances(tsd._brute(pool, od, c, E, False)[0]) == (set(range(5)), set(range(5)))][:1]
            assert picks, (W, od["motif_id"])
        out.append(int(picks[0]))
    return out


def _expected(scan, key, fwd, inserts=INSERTS):
    """the brute force over the pool alone -> per motif its two arrays, as the kernel types them"""
    bf = importlib.import_module(SCANS[scan][1])
    W = key[0]
    pool, _, ods, weights = _case(*key)
    out = []
    for m, od in enumerate(ods):
        if scan == "site_distance":
            a, b = bf.scan_arrays(pool, W, od["score_matrix"], od["min_val"], _cutoffs(*key)[m], E, fwd)
        else:
            a, b = bf.scan_arrays(pool, W, od["score_matrix"], od["min_val"], weights[m], fwd, *_extra(scan, W, inserts))
        out.append((np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint64)))
    return out


def _run(scan, key, fwd, inserts, off, bases):
    """the scan through its scan_sequences -> per motif its two arrays"""
    mod = importlib.import_module("grafimo_amd." + SCANS[scan][0])
    W = key[0]
    _, motifs, _, weights = _case(*key)
    if scan == "site_distance":
        return mod.scan_sequences(motifs, off, bases, _cutoffs(*key), max_edits=E, forward_only=fwd)
    return mod.scan_sequences(motifs, off, bases, *_extra(scan, W, inserts), weights=weights, forward_only=fwd)


def _check(scan, W, fwd, n_motifs=2, seed=None, turns=2, inserts=INSERTS, kept=None):
    key = (W, n_motifs, 111_000 + W if seed is None else seed, kept)
    pool = _case(*key)[0]
    cap, axis = mt.CAPS[SCANS[scan][2]], SCANS[scan][3]
    call, pairs = mt.layout(pool, T, cap, turns=turns)
    mt.coverage(pairs, pool, W, T)
    off, bases = mt.call_arrays(pool, call)
    assert mt.tile_count(off, T) > (turns - 1) * cap and len(bases) < 100_000
    want = _expected(scan, key, fwd, inserts)
    got = _run(scan, key, fwd, inserts, off, bases)
    assert len(got) == n_motifs
    later = mt.later_turn_bases(off, T, (turns - 1) * cap)       # the rows of the last turn
    assert later.any() and not later.all()
    for m in range(n_motifs):
        for c in range(2):
            exp = mt.gather(want[m][c], pool, call, axis)
            assert got[m][c].dtype == exp.dtype and got[m][c].shape == exp.shape, (scan, W, fwd, m, c)
            assert np.array_equal(got[m][c], exp), (scan, W, fwd, m, c, np.argwhere(got[m][c] != exp)[:5].tolist())
            rows = np.compress(later, got[m][c], axis=axis)
            assert rows.any() and (scan != "site_distance" or c == 1 or (rows != 0xFFFFFFFF).any()), (scan, W, m, c)
        if scan != "site_distance":
            assert int(got[m][1].max()) > 1 << 53                 # some sum no double holds
    return got


CASES = [(s, W, False) for s in SCANS for W in (2, 19, 64)] + [(s, 19, True) for s in SCANS] + \
    [(s, 1, False) for s in ("mutation", "deletion")]


@pytest.mark.parametrize("scan,W,fwd", CASES)
def test_second_turn_against_brute_force(scan, W, fwd):
    """every row of a call of more tiles than the grid's cap, exactly, for two motifs of one width (grid.y)"""
    got = _check(scan, W, fwd)
    assert not np.array_equal(got[0][0], got[1][0])              # (two motifs, two answers)


def test_insertion_third_turn():
    """two caps and more of tiles under the insertion scan's 4 096 workgroups, sixteen inserts: a workgroup's H and T tables
    serve three tiles each.  One motif, and of the pool the lengths coverage() needs: the brute force of sixteen inserts is the
    test's time, and over the whole pool and two motifs it is five times as long."""
    W = 19
    kept = frozenset((1, 2, W - 1, W + 64, 70, 2 * T + 3, 3 * T + 1))
    got = _check("insertion", W, False, n_motifs=1, turns=3, inserts=SIXTEEN, kept=kept)
    assert got[0][0].shape[0] == 16 and len({got[0][0][k, :, 1].tobytes() for k in range(16)}) == 16


def test_seventeen_motifs_and_a_second_turn():
    """the second launch of a call (motifs 16 ..) has second turns too"""
    got = _check("mutation", 2, False, n_motifs=17, seed=112_000)
    assert len({g[1].tobytes() for g in (got[0], got[15], got[16])}) == 3


# ------------------------------------------------------------------------------------------- gfm_graph_query_edits
@pytest.mark.parametrize("W", [5, 19])
def test_query_edits_second_item_of_a_wave(W):
    """131 072 items and more: item n + 131 072 is the next item of the wavefront that did item n, in the same two LDS
    slices.  The expected record of every distinct (sequence, edit) is made once and gathered."""
    import test_gpu_query_variants as tq
    from grafimo_amd.query_variants import RECORD, score_edits
    rng = np.random.default_rng(113_000 + W)
    seqs, edits, items = tq._cases(W, rng)
    motifs = [SynMotif(W, seed=1130 + k) for k in range(3)]
    ods = [motif_as_oracle_dict(m) for m in motifs]
    weights = [rng.integers(1 << 40, 1 << 55, size=1000 * W + 1, dtype=np.uint64) for _ in motifs]
    cap, n = mt.CAPS["query_items"], len(items)
    distinct = sorted(set(items))
    number = {p: k for k, p in enumerate(distinct)}
    for fwd in (False, True):
        want = np.zeros((3, len(distinct)), dtype=RECORD)
        for m, od in enumerate(ods):
            for k, (s, e) in enumerate(distinct):
                want[m, k] = tq._kernel_expected(seqs[s][0], seqs[s][1], *edits[e], W, od["score_matrix"], od["min_val"], weights[m], fwd)
        status = {p: int(want[0, number[p]]["status"]) for p in distinct}

        def long_context(p):                                     # W - 1 bases on both sides of the REF allele
            o, lr, x = int(want[0, number[p]]["o"]), len(edits[p[1]][1]), seqs[p[0]][0]
            return status[p] == tq.APPLIED and o >= W - 1 and len(x) - o - lr >= W - 1

        def scored(p):                                           # applied, and both sides have a window
            r = want[0, number[p]]
            return status[p] == tq.APPLIED and r["ref_key"] != 0 and r["alt_key"] != 0

        def holds(pairs):
            return (any(long_context(a) and status[b] == tq.APPLIED and len(seqs[b[0]][0]) < W for a, b in pairs) and
                    any(long_context(a) and scored(b) and not long_context(b) for a, b in pairs) and
                    any(status[a] in (tq.ABSENT, tq.MISMATCH) and scored(b) for a, b in pairs) and
                    any(scored(a) and status[b] == tq.ABSENT for a, b in pairs))

        # the filler: the applied item with the shortest sequence; the rotation that lies one grid behind `items` themselves
        # is the first that shows every succession, the three others follow a quarter of the list apart
        cheap = min((p for p in distinct if status[p] == tq.APPLIED), key=lambda p: (len(seqs[p[0]][0]), p))
        first = next(s for s in range(1, n) if holds(list(zip(items, items[s:] + items[:s]))))
        entries = list(items) + [cheap] * (cap - n)
        for r in range(4):
            s = (first + r * (n // 4)) % n
            entries += items[s:] + items[:s]
        entries.append(items[0])
        N = len(entries)
        assert N == cap + 4 * n + 1 and N % 4 != 0 and entries[cap:cap + n] != list(items)
        assert holds([(entries[i], entries[i + cap]) for i in range(N - cap)])
        ids = np.array([number[p] for p in entries])
        off = np.concatenate([[0], np.cumsum([len(x) for x, _ in seqs])]).astype(np.int64)
        bases = np.frombuffer(b"".join(x for x, _ in seqs), dtype=np.uint8)
        coord = np.array([p for _, c in seqs for p in c], dtype=np.int32)
        got = score_edits(motifs, off, bases, coord, [e[0] for e in edits], [e[1] for e in edits], [e[2] for e in edits],
                          np.array([p[0] for p in entries], dtype=np.int32), np.array([p[1] for p in entries], dtype=np.int32),
                          weights=weights, forward_only=fwd)
        assert len(got) == 3
        for m in range(3):
            assert got[m].shape == (N,)
            for field in RECORD.names:
                exp = want[m][ids][field]
                assert np.array_equal(got[m][field], exp), (W, fwd, m, field, np.flatnonzero(got[m][field] != exp)[:5].tolist())
            assert got[m]["ref_key"][cap:].any() and int(got[m]["ref_sum"].max()) > 1 << 53
        assert not np.array_equal(got[0]["ref_sum"], got[1]["ref_sum"])
