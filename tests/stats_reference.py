"""Exact references and adversarial inputs for the tail-table and q-value kernels (gfm_stats_kernels.hpp).

Host only: numpy and the standard library, no torch and no native library.  The references are written from the
definitions (score_sequences.py:390-391 for the tail table, score_sequences.py:401-428 / statsmodels' fdr_bh for the
q-values), not from the kernels: every float is taken as the exact rational it is and all arithmetic is done on Python
ints and fractions.Fraction, so a reference value has NO rounding error and a tolerance only has to cover the device's
own operations.
"""
from fractions import Fraction

import numpy as np

RANGE = 1000            # scaled scores of one position lie in [0, RANGE]
SEGMENTS = 1024         # ptable_kernel: contiguous segments of the window, one per thread
QBLOCK = 256            # q_*_kernel: bins per block
WAVE = 64

ONE = Fraction(1)
ZERO = Fraction(0)


# ------------------------------------------------------------------------------------------------ exact arithmetic
def exact_ints(values):
    """floats -> (Python ints, k) with value[i] == ints[i] / 2**k exactly."""
    ratios = [float(v).as_integer_ratio() for v in values]
    k = max((d.bit_length() - 1 for _, d in ratios), default=0)
    return [n << (k - (d.bit_length() - 1)) for n, d in ratios], k


def ptable_exact(pmf, lo, hi):
    """p_table[s] = sum(pmf[max(s, lo) .. hi]) / sum(pmf[lo .. hi]) as Fractions [len(pmf)]: 1 at and below lo, 0 above hi."""
    L = len(pmf)
    if not (0 <= lo <= hi < L):
        raise ValueError("window outside the table")
    ints, _ = exact_ints(pmf[lo:hi + 1])
    if any(v < 0 for v in ints):
        raise ValueError("negative mass")
    total = sum(ints)
    if total <= 0:
        raise ValueError("the window holds no mass")
    out = [ZERO] * L
    tail, cur = 0, ZERO
    for j in range(hi, lo - 1, -1):
        if ints[j - lo]:                         # (an empty bin shares the value object of the bin above it)
            tail += ints[j - lo]
            cur = Fraction(tail, total)
        out[j] = cur
    assert tail == total
    out[:lo] = [ONE] * lo
    return out


def bh_exact(hist, ptable, lo, hi, min_val):
    """Benjamini-Hochberg q-value of every score from a histogram -> (q as Fractions [L], n).

    Rows are ranked by p-value, all rows of one score share the largest rank of their group, C(s) = #rows scoring >= s;
    raw(s) = p(s) n / C(s); the rows holding an N score min_val, rank last (rank n) and have raw = p(min_val);
    q(s) = min(1, min over occupied s' <= s of raw(s'), N rows included).  Below the window q = min(1, raw of the N rows),
    above it the last running minimum.  `ptable` floats are taken as exact."""
    L = len(hist)
    h = [int(v) for v in np.asarray(hist).tolist()]
    if min(h) < 0:
        raise ValueError("negative count")
    inside = lo <= min_val <= hi
    n_N = 0 if inside else h[min_val]
    n = sum(h[lo:hi + 1]) + n_N
    run = None                                   # running minimum of raw; None = +inf
    if n_N:
        run = Fraction(float(ptable[min_val])) * n / n
    cur = ONE if run is None else min(ONE, run)
    q = [cur] * L
    occupied = [j for j in range(lo, hi + 1) if h[j]]
    c_ge = 0
    counts = {}
    for j in reversed(occupied):
        c_ge += h[j]
        counts[j] = c_ge
    # raw(j) = P[j] n / (C(j) 2**k) with integer P: compared with the running minimum num / den in integers, and only a
    # new minimum becomes a Fraction
    P, k = exact_ints([ptable[j] for j in occupied])
    num, den = (run.numerator, run.denominator) if run is not None else (1, 0)      # 1 / 0: +inf
    at = lo
    for j, pj in zip(occupied, P):
        q[at:j] = [cur] * (j - at)
        raw_num, raw_den = pj * n, counts[j] << k
        if raw_num * den < num * raw_den:
            num, den = raw_num, raw_den
            cur = min(ONE, Fraction(num, den))
        at = j
    q[at:] = [cur] * (L - at)
    return q, n


def to_floats(fracs):
    """Correctly rounded f64 of every Fraction (runs that share one object are converted once)."""
    out = np.empty(len(fracs), dtype=np.float64)
    last, last_f = None, 0.0
    for j, e in enumerate(fracs):
        if e is not last:
            last, last_f = e, float(e)
        out[j] = last_f
    return out


def rel_violations(got, exact, bound, floor=None):
    """-> (indices j with |got[j] - exact[j]| > bound * exact[j], number of entries skipped because 0 < exact[j] < floor).
    Evaluated exactly; `bound` must be at least 2**-53 (an entry that equals the correctly rounded reference passes
    without the long arithmetic unless it lies below `floor`, where rounding to f64 is no longer relative)."""
    assert bound >= Fraction(1, 1 << 53)
    got = np.asarray(got, dtype=np.float64)
    assert len(got) == len(exact) and not np.isnan(got).any()
    normal = Fraction(1, 1 << 1022)
    bad, skipped, seen = [], 0, {}
    rounded = to_floats(exact)
    assert floor is None or floor < Fraction(1, 10 ** 260)
    tiny = rounded < 1e-250                        # only these need the exact look at `floor` and the normal range
    for j in np.nonzero(tiny | (got != rounded))[0]:
        j = int(j)
        e = exact[j]
        if tiny[j]:
            if floor is not None and 0 < e < floor:
                skipped += 1
                continue
            if got[j] == rounded[j] and (e == 0 or e >= normal):
                continue
        key = (float(got[j]), id(e))
        ok = seen.get(key)
        if ok is None:
            ok = seen[key] = abs(Fraction(float(got[j])) - e) <= bound * e
        if not ok:
            bad.append(j)
    return bad, skipped


# ------------------------------------------------------------------------------------------------ score matrices
def window_matrix(W, nb, lo, n_bin_inside):
    """int64 [4, W] score matrix, entries in [0, RANGE], global minimum 0, whose reachable window (sum of the column
    minima .. sum of the column maxima) is exactly [lo, lo + nb - 1].  n_bin_inside: lo == 0 and every column holds a 0,
    so the bin of the rows with an N (the global minimum) is bin lo; otherwise lo > 0 and that bin lies below the window."""
    hi = lo + nb - 1
    if W < 1 or nb < 1 or lo < 0 or hi > RANGE * W:
        raise ValueError("window does not fit the width")
    if n_bin_inside != (lo == 0):
        raise ValueError("the N bin is inside the window exactly when lo == 0")
    mins = [0] * W
    if lo:
        if W < 2 or lo > RANGE * (W - 1):
            raise ValueError("lo > 0 needs a column of its own for the global minimum")
        for j in range(1, W):                    # column 0 keeps the 0
            mins[j] = lo // (W - 1) + (1 if j - 1 < lo % (W - 1) else 0)
    left = nb - 1
    maxs = list(mins)
    for j in range(W):
        r = min(left, RANGE - mins[j])
        maxs[j] += r
        left -= r
    if left:
        raise ValueError("window does not fit the width")
    sm = np.zeros((4, W), dtype=np.int64)
    for j in range(W):
        m, M = mins[j], maxs[j]
        col = [m, M, m + (M - m) // 3, M - (M - m) // 4]
        for r in range(4):                       # minimum and maximum wander over the rows
            sm[(r + j) % 4, j] = col[r]
    return sm


def matrix_window(sm):
    """(lo, hi, min_val) of a score matrix from its column minima and maxima."""
    sm = np.asarray(sm)
    return int(sm.min(axis=0).sum()), int(sm.max(axis=0).sum()), int(sm.min())


# name -> (W, nb, lo).  1 / 2: the smallest windows; 1001: W = 1 with lo == min_val; 1023..1025 and 2047..2049: the
# tail table's per-thread segment grows from 1 to 2 to 3 bins and the last threads' segments become empty, the q kernels'
# last block holds 255 / 256 / 1 bins; 5003: mid-size; 64001: all of L at the largest width (251 q blocks); W = 64 with
# lo = 63: the largest window that keeps the N bin outside.
SHAPES = {
    "nb1": (1, 1, 0),
    "nb2": (1, 2, 0),
    "nb1001": (1, 1001, 0),
    "nb1023": (2, 1023, 0),
    "nb1024": (3, 1024, 7),
    "nb1025": (2, 1025, 300),
    "nb2047": (3, 2047, 0),
    "nb2048": (3, 2048, 2),
    "nb2049": (4, 2049, 1500),
    "nb5003": (6, 5003, 11),
    "nb64001": (64, 64001, 0),
    "w64lo63": (64, 63938, 63),
}
BIG = ("nb64001", "w64lo63")


def shape_matrix(name):
    W, nb, lo = SHAPES[name]
    return window_matrix(W, nb, lo, lo == 0)


def _seed(name, salt):
    return [salt] + [ord(c) for c in name]


# ------------------------------------------------------------------------------------------------ pmf families
def segment_boundaries(lo, hi):
    """The bins on each side of the tail table's segment boundaries lo + k per, k = 1, 2, 1023, inside the window."""
    nb = hi - lo + 1
    per = (nb + SEGMENTS - 1) // SEGMENTS
    out = []
    for k in (1, 2, SEGMENTS - 1):
        for j in (lo + k * per - 1, lo + k * per):
            if lo <= j <= hi and j not in out:
                out.append(j)
    return out


def integer_pmfs(name):
    """Integer-valued distributions over the shape's window (zero outside it), values in [0, 2**30] with zeros mixed
    in: every partial sum is an integer below 2**53, so the device's sums are exact and its table is one correctly
    rounded division away from the exact one.  -> {family: f64 [L]}"""
    W, nb, lo = SHAPES[name]
    hi, L = lo + nb - 1, RANGE * W + 1
    rng = np.random.default_rng(_seed(name, 1))
    fams = {}

    def one_hot(j, v):
        a = np.zeros(L)
        a[j] = v
        return a
    fams["onehot_lo"] = one_hot(lo, 3.0)
    fams["onehot_hi"] = one_hot(hi, float(1 << 30))
    for j in segment_boundaries(lo, hi):
        fams[f"onehot_{j - lo}"] = one_hot(j, float(1 + (j % 5)))
    a = np.zeros(L)
    a[lo + nb // 3] += 12345.0
    a[lo + (2 * nb) // 3] += 12345.0
    fams["two_spikes"] = a
    a = np.zeros(L)
    a[lo:hi + 1] = rng.integers(0, (1 << 30) + 1, size=nb).astype(np.float64)
    a[lo:hi + 1][rng.random(nb) < 0.1] = 0.0
    a[lo + nb // 2] = float(1 << 30)
    fams["dense"] = a
    a = np.zeros(L)
    a[lo:hi + 1] = rng.integers(1, (1 << 30) + 1, size=nb).astype(np.float64)
    a[lo:hi + 1][rng.random(nb) < 0.9] = 0.0
    a[hi] = 1.0
    fams["sparse"] = a
    return fams


def float_pmfs(name, only=None):
    """Distributions spanning hundreds of orders of magnitude over the shape's window.  -> {family: f64 [L]}"""
    W, nb, lo = SHAPES[name]
    hi, L = lo + nb - 1, RANGE * W + 1
    rng = np.random.default_rng(_seed(name, 2))
    fams = {}
    a = np.zeros(L)
    a[lo:hi + 1] = np.exp(30.0 * rng.standard_normal(nb))
    fams["lognormal30"] = a
    a = np.zeros(L)
    a[lo:hi + 1] = 10.0 ** np.linspace(0.0, -300.0, nb)
    fams["decades_down"] = a
    a = np.zeros(L)
    a[lo:hi + 1] = (10.0 ** np.linspace(0.0, -300.0, nb))[::-1]
    fams["decades_up"] = a
    a = np.zeros(L)                               # sparse, a normal entry at hi - 1 and a denormal at hi
    keep = rng.random(nb) < 0.02
    a[lo:hi + 1][keep] = np.exp(10.0 * rng.standard_normal(int(keep.sum())))
    if nb >= 2:
        a[hi - 1] = 1e-200
    a[hi] = 3 * 5e-324
    fams["sparse_denormal_top"] = a
    if only is not None:
        fams = {k: fams[k] for k in only}
    return fams


# ------------------------------------------------------------------------------------------------ histogram families
def q_boundary_bins(lo, hi):
    """Bins on the wave and block boundaries of the q kernels, inside the window: both ends, the last lane of wave 0 and
    the first of wave 1, the last bin of block 0 and the first two of block 1, the first bin of the last block and the
    last bin that block holds."""
    nb = hi - lo + 1
    nblk = (nb + QBLOCK - 1) // QBLOCK
    cand = [lo, hi, lo + WAVE - 1, lo + WAVE, lo + QBLOCK - 1, lo + QBLOCK, lo + QBLOCK + 1, lo + (nblk - 1) * QBLOCK,
            min(hi, lo + nblk * QBLOCK - 1)]
    out = []
    for j in cand:
        if lo <= j <= hi and j not in out:
            out.append(j)
    return out


def histograms(name, min_val=0):
    """Row-count histograms over the shape's window, each without and with rows that hold an N (bin min_val: below the
    window when lo > 0, bin lo itself when lo == 0).  Totals stay below 2**53, so (double)n is exact.
    -> {family: int64 [L]}"""
    W, nb, lo = SHAPES[name]
    hi, L = lo + nb - 1, RANGE * W + 1
    nblk = (nb + QBLOCK - 1) // QBLOCK
    rng = np.random.default_rng(_seed(name, 3))
    base = {}
    base["empty"] = np.zeros(L, dtype=np.int64)
    for k, j in enumerate(q_boundary_bins(lo, hi)):
        a = np.zeros(L, dtype=np.int64)
        a[j] = (1 << 33) + 5 if k % 2 else 7         # every other one holds more than 2**32 rows
        base[f"one_bin_{j - lo}"] = a
    a = np.zeros(L, dtype=np.int64)
    a[q_boundary_bins(lo, hi)] = 1
    base["boundary_rows"] = a
    a = np.zeros(L, dtype=np.int64)
    a[lo:hi + 1] = rng.integers(1, 101, size=nb)
    base["dense"] = a
    a = np.zeros(L, dtype=np.int64)                   # 1 % occupied, counts up to 2**40
    occ = rng.random(nb) < 0.01
    occ[rng.integers(0, nb)] = True
    a[lo:hi + 1][occ] = rng.integers(1, (1 << 40) + 1, size=int(occ.sum()))
    a[lo + int(np.nonzero(occ)[0][0])] = 1 << 40
    base["huge_counts"] = a

    def blocks(which):
        a = np.zeros(L, dtype=np.int64)
        for b in which:
            s, e = lo + b * QBLOCK, min(hi, lo + b * QBLOCK + QBLOCK - 1)
            v = rng.integers(1, 101, size=e - s + 1)
            v[rng.random(e - s + 1) < 0.3] = 0
            v[-1] = 3                                 # the block's last bin is occupied
            a[s:e + 1] = v
        return a
    base["every_third_block"] = blocks(range(0, nblk, 3))
    base["top_block"] = blocks([nblk - 1])
    base["bottom_block"] = blocks([0])
    out = {}
    for k, (fam, a) in enumerate(base.items()):
        out[fam] = a
        b = a.copy()
        b[min_val] += (1 << 34) + 3 if k % 3 == 0 else 1 + k
        out[fam + "+N"] = b
    assert all(0 <= int(a.sum()) < (1 << 53) for a in out.values())
    return out
