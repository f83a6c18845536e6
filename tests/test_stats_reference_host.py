"""The exact references of tests/stats_reference.py against the CPU oracle and brute force: shown right before the GPU
tests (test_gpu_stats_tables.py) lean on them.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import stats_reference as ref
from oracle import oracle as orc

U = Fraction(1, 1 << 53)         # unit roundoff of f64


def _within(got, exact, bound):
    """|got - exact| <= bound * exact, evaluated exactly."""
    return abs(Fraction(float(got)) - exact) <= bound * exact


def _float_ptable(sm, seed):
    """A tail table with rounding in it: the oracle's table of a random distribution over the matrix's window."""
    lo, hi, _ = ref.matrix_window(sm)
    rng = np.random.default_rng(seed)
    pmf = np.zeros(ref.RANGE * sm.shape[1] + 1)
    pmf[lo:hi + 1] = rng.random(hi - lo + 1) ** 8
    return orc.p_table(pmf)


@pytest.mark.parametrize("n_inside", [False, True])
def test_bh_exact_agrees_with_sorted_bh_over_rows(n_inside):
    """bh_exact works from a histogram, the oracle's fdr_bh from one p-value per row (score_sequences.py:401-428): expand
    a small histogram to shuffled rows.  The oracle rounds twice per row, rank / n and p / that, both correctly: its
    relative error is below 2 u + u^2 < 3 * 2**-53; its running minimum and clip are exact."""
    sm = ref.window_matrix(3, 700, 0 if n_inside else 40, n_inside)
    lo, hi, min_val = ref.matrix_window(sm)
    assert (lo <= min_val <= hi) == n_inside
    pt = _float_ptable(sm, 5)
    rng = np.random.default_rng(11)
    hist = np.zeros(len(pt), dtype=np.int64)
    bins = rng.choice(np.arange(lo, hi + 1), size=300, replace=False)
    hist[bins] = rng.integers(1, 40, size=300)
    hist[[lo + 255, lo + 256]] = 1
    hist[min_val] += 90                              # the rows with an N
    q, n = ref.bh_exact(hist, pt, lo, hi, min_val)
    scores = np.repeat(np.arange(len(hist)), hist)
    rng.shuffle(scores)
    assert n == len(scores) == int(hist.sum())
    q_rows = orc.fdr_bh(pt[scores])
    assert all(_within(g, q[s], 3 * U) for g, s in zip(q_rows, scores))
    # the definition, entry by entry, on this small case: raw of every occupied score, minimum over the scores below
    raws = {s: Fraction(float(pt[s])) * n / int(hist[s:].sum()) for s in range(lo, hi + 1) if hist[s]}
    if not n_inside:
        raws[min_val] = Fraction(float(pt[min_val]))
    for s in range(len(hist)):
        assert q[s] == min([Fraction(1)] + [r for t, r in raws.items() if t <= s])
    assert all(a >= b for a, b in zip(q, q[1:]))


def test_bh_exact_of_nothing_and_of_one_row():
    sm = ref.window_matrix(2, 600, 9, False)
    lo, hi, min_val = ref.matrix_window(sm)
    pt = _float_ptable(sm, 6)
    hist = np.zeros(len(pt), dtype=np.int64)
    q, n = ref.bh_exact(hist, pt, lo, hi, min_val)
    assert n == 0 and q == [Fraction(1)] * len(pt)
    hist[hi] = 1
    q, n = ref.bh_exact(hist, pt, lo, hi, min_val)
    assert n == 1 and q[hi] == Fraction(float(pt[hi])) and q[hi - 1] == 1 and q[-1] == q[hi]
    hist[min_val] = 3                                # three rows with an N: the one scored row has rank 1 of 4
    q, n = ref.bh_exact(hist, pt, lo, hi, min_val)
    assert n == 4 and q[hi] == Fraction(float(pt[hi])) * 4 and q[0] == 1


def test_ptable_exact_against_the_oracle_table():
    """orc.p_table is a sequential sum from the top and one division: a tail is a chain of at most L - 1 additions of
    non-negatives, the total another, so its relative error is at most ((1 + u)^(2 L - 1) - 1) <= (2 L + 2) u."""
    for name in ("nb1001", "nb1025", "nb2049"):
        W, nb, lo = ref.SHAPES[name]
        hi = lo + nb - 1
        for fam, pmf in ref.float_pmfs(name).items():
            exact = ref.ptable_exact(pmf, lo, hi)
            got = orc.p_table(pmf)
            bound = (2 * len(pmf) + 2) * U
            # (additions cannot underflow; the division's rounding is relative only while the quotient is a normal number)
            assert all(_within(g, e, bound) for g, e in zip(got, exact) if e >= Fraction(1, 1 << 1022)), (name, fam)
            assert exact[lo] == 1 and all(e == 1 for e in exact[:lo]) and all(e == 0 for e in exact[hi + 1:])
            assert all(a >= b for a, b in zip(exact, exact[1:]))


def test_ptable_exact_is_exact_on_integer_distributions():
    rng = np.random.default_rng(3)
    for lo, hi, L in [(0, 0, 1), (0, 9, 10), (4, 30, 41), (7, 7, 20)]:
        pmf = np.zeros(L)
        pmf[lo:hi + 1] = rng.integers(0, 1 << 30, size=hi - lo + 1)
        pmf[hi] = 5.0
        ints = [int(v) for v in pmf]
        brute = [Fraction(sum(ints[max(s, lo):hi + 1]), sum(ints[lo:hi + 1])) for s in range(L)]
        assert ref.ptable_exact(pmf, lo, hi) == brute
    # sums of integers below 2**53 are exact in f64 and the division rounds correctly: bit-equal to the oracle's table
    for name in ("nb2", "nb1024", "nb2047"):
        W, nb, lo = ref.SHAPES[name]
        for fam, pmf in ref.integer_pmfs(name).items():
            exact = ref.ptable_exact(pmf, lo, lo + nb - 1)
            assert np.array_equal(np.array([float(e) for e in exact]), orc.p_table(pmf)), (name, fam)
    tiny = Fraction(1, 1 << 1074)                    # non-integers are exact too, down to the smallest denormal
    total = Fraction(3, 4) + tiny
    assert ref.ptable_exact(np.array([0.0, 0.5, 0.25, 2.0 ** -1074, 0.0]), 1, 3) == \
        [1, 1, (Fraction(1, 4) + tiny) / total, tiny / total, 0]
    with pytest.raises(ValueError):
        ref.ptable_exact(np.zeros(5), 1, 3)


@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_window_matrix_yields_the_requested_window(name):
    W, nb, lo = ref.SHAPES[name]
    sm = ref.shape_matrix(name)
    assert sm.shape == (4, W) and sm.dtype == np.int64
    assert sm.min() == 0 and sm.max() <= ref.RANGE
    assert int(sm.min(axis=0).sum()) == lo
    assert int(sm.max(axis=0).sum()) == lo + nb - 1
    if lo == 0:
        assert (sm.min(axis=0) == 0).all()       # every column holds a 0: the N bin is bin lo
    assert ref.matrix_window(sm) == (lo, lo + nb - 1, 0)


def test_window_matrix_refuses_what_cannot_be_built():
    for args in [(1, 1002, 0, True), (1, 5, 3, False), (2, 10, 0, False), (2, 10, 4, True), (2, 1500, 600, False)]:
        with pytest.raises(ValueError):
            ref.window_matrix(*args)


def test_input_families_stay_inside_their_window():
    for name in ref.SHAPES:
        if name in ref.BIG:
            continue
        W, nb, lo = ref.SHAPES[name]
        hi = lo + nb - 1
        pmfs = {**ref.integer_pmfs(name), **ref.float_pmfs(name)}
        for fam, a in pmfs.items():
            assert a.shape == (ref.RANGE * W + 1,) and (a >= 0).all() and a[lo:hi + 1].sum() > 0, (name, fam)
            assert not a[:lo].any() and not a[hi + 1:].any(), (name, fam)
        for fam, a in ref.integer_pmfs(name).items():
            assert (a == np.floor(a)).all() and a.max() <= 1 << 30
        for fam, h in ref.histograms(name).items():
            outside = h.copy()
            outside[lo:hi + 1] = 0
            outside[0] = 0                           # the N bin
            assert not outside.any() and (h >= 0).all(), (name, fam)
    assert max(int(h.max()) for h in ref.histograms("nb5003").values()) > 1 << 32
