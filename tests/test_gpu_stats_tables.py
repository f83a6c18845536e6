"""pvalue_dp_kernel, ptable_kernel and the q_*_kernel passes (gfm_stats_kernels.hpp) on adversarial synthetic inputs.

No k-mer is scored: a DeviceMotif created with a given pmf uploads it as it is and runs ptable_kernel on it, and
DeviceMotif.qvalue_table takes any uint64 [L] histogram.  Both are compared with exact rational arithmetic
(tests/stats_reference.py, itself checked in test_stats_reference_host.py) at the window sizes and bins where a blocked
scan goes wrong: segment, wave and block boundaries, empty segments and blocks, counts above 2**32.

Tolerances (u = 2**-53; all derived, none measured):
  integer pmfs   bit for bit.  Every partial sum is an integer below 2**53, hence exact in f64 in any association order;
                 the table is one correctly rounded division of exact operands, and so is float(Fraction).
  float pmfs     (2 (ceil(nb / 1024) + 1024) + 2) u relative.  A tail is a chain of at most per + 1024 additions of
                 non-negatives (per = ceil(nb / 1024) inside a segment, at most 1024 segment totals), each within a
                 factor (1 + u); the total is another such chain; then one division: (1 + u)^(2 (per + 1024) + 1) - 1,
                 which the + 2 covers for every per here.  f64 addition cannot underflow, so this holds wherever the
                 QUOTIENT is a normal number: the accuracy is asserted down to 2**-1022 (10**-290 was asked for).
  q-values       3 u relative.  raw = p / (C / n): C and n are integers below 2**53, (double) of them exact; two
                 correctly rounded divisions, (1 + u)^2 / (1 - u) - 1 < 3 u; the minima and the clip at 1 are exact.
                 The tail tables used hold no positive entry below 10**-290 and q >= p, so no quotient is subnormal.
"""
import os
from fractions import Fraction

import numpy as np
import pytest

import stats_reference as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = Fraction(1, 1 << 53)
NORMAL = Fraction(1, 1 << 1022)
BG = np.full(4, 0.25)
SHAPE_NAMES = list(ref.SHAPES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from grafimo_amd import _native as nv
    assert os.path.exists(nv.LIB_PATH), "libgrafimo_hip.so not built"
    assert nv.device_count() >= 1
    return torch.device("cuda:0")


def _geometry(name):
    W, nb, lo = ref.SHAPES[name]
    return W, nb, lo, lo + nb - 1, ref.RANGE * W + 1


def _spec(sm, pmf):
    """(score matrix, bg, min_val, scale, offset, pmf) of a handle: the matrices of stats_reference have minimum 0."""
    return (sm, BG, 0, 1, 0.0, pmf)


def _create(name, pmfs):
    """One handle per distribution over the shape's matrix, all in ONE create_many call (one multi-job ptable_kernel
    launch); the handles' window must be the requested one."""
    from grafimo_amd.device import DeviceMotif
    W, nb, lo, hi, L = _geometry(name)
    sm = ref.shape_matrix(name)
    dms = DeviceMotif._create_many([_spec(sm, pmf) for pmf in pmfs])
    for dm in dms:
        assert (dm.score_lo, dm.score_hi, dm.L, dm.min_val) == (lo, hi, L, 0), name
    return dms


def _first_below(values, lo, hi, L, thr):
    """First j in [lo, hi] with values[j] < thr, L when there is none."""
    idx = np.nonzero(values[lo:hi + 1] < thr)[0]
    return lo + int(idx[0]) if len(idx) else L


# ------------------------------------------------------------------------------------------------ tail table
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_tail_table_of_integer_distributions_is_bit_exact(dev, name):
    from grafimo_amd.device import DeviceMotif
    W, nb, lo, hi, L = _geometry(name)
    fams = ref.integer_pmfs(name)
    dms = _create(name, list(fams.values()))
    try:
        for (fam, pmf), dm in zip(fams.items(), dms):
            got_pmf, pt = dm.tables()
            assert np.array_equal(got_pmf, pmf), (name, fam)
            want = ref.to_floats(ref.ptable_exact(pmf, lo, hi))
            diff = np.nonzero(pt != want)[0]
            assert len(diff) == 0, (name, fam, "first differing score", int(diff[0]), "of", len(diff),
                                    "window offset", int(diff[0]) - lo, float(pt[diff[0]]), float(want[diff[0]]))
        # the single constructor is the set call of one motif: the same table, bit for bit
        one = DeviceMotif(*_spec(ref.shape_matrix(name), fams["dense"]))
        assert (one.score_lo, one.score_hi) == (lo, hi)
        assert np.array_equal(one.tables()[1], dms[list(fams).index("dense")].tables()[1])
        one.close()
    finally:
        for dm in dms:
            dm.close()


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_tail_table_of_float_distributions(dev, name):
    """Exactly non-increasing, exactly 1 at and below the lowest mass, exactly 0 above the window, and within the derived
    bound of the exact table wherever that is a normal number.  Windows of at most ~5 000 bins take every family, the two
    W = 64 shapes one."""
    W, nb, lo, hi, L = _geometry(name)
    fams = ref.float_pmfs(name, only=["lognormal30"] if name in ref.BIG else None)
    per = (nb + ref.SEGMENTS - 1) // ref.SEGMENTS
    bound = (2 * (per + ref.SEGMENTS) + 2) * U
    dms = _create(name, list(fams.values()))
    try:
        for (fam, pmf), dm in zip(fams.items(), dms):
            got_pmf, pt = dm.tables()
            assert np.array_equal(got_pmf, pmf), (name, fam)
            steps_up = np.nonzero(np.diff(pt) > 0)[0]
            assert len(steps_up) == 0, (name, fam, "rises after score", int(steps_up[0]))
            lowest = int(np.nonzero(pmf)[0][0])
            assert lowest >= lo and (pt[:lowest + 1] == 1.0).all(), (name, fam)
            assert (pt[hi + 1:] == 0.0).all(), (name, fam)
            bad, skipped = ref.rel_violations(pt, ref.ptable_exact(pmf, lo, hi), bound, floor=NORMAL)
            assert not bad, (name, fam, "first score off", bad[0], "window offset", bad[0] - lo, len(bad))
            assert skipped < 0.01 * L, (name, fam, skipped)
    finally:
        for dm in dms:
            dm.close()


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_pvalue_cutoff_is_the_first_score_below_the_threshold(dev, name):
    """gfm_motif_pvalue_cutoff on tables with long plateaus (one-hot, sparse) and without: strict `<` on a threshold that
    equals a table value, the next float above it, 1.0 and 1e-300."""
    W, nb, lo, hi, L = _geometry(name)
    ints, floats = ref.integer_pmfs(name), ref.float_pmfs(name, only=["lognormal30", "sparse_denormal_top"])
    pmfs = [ints["sparse"], ints["two_spikes"], floats["lognormal30"], floats["sparse_denormal_top"]]
    dms = _create(name, pmfs)
    try:
        for k, dm in enumerate(dms):
            pt = dm.tables()[1]
            picks = {lo, hi, lo + nb // 2, lo + nb // 3, min(hi + 1, L - 1), int(np.nonzero(pmfs[k])[0][-1])}
            thresholds = [1.0, 1e-300, 0.5, 5e-324]
            for j in sorted(picks):
                thresholds += [float(pt[j]), float(np.nextafter(pt[j], np.inf))]
            for t in thresholds:
                idx = np.nonzero(pt < t)[0]
                want = int(idx[0]) if len(idx) else L
                assert dm.pvalue_cutoff(t) == want, (name, k, t)
    finally:
        for dm in dms:
            dm.close()


# ------------------------------------------------------------------------------------------------ DP kernel
def _dp_cases():
    rng = np.random.default_rng(41)
    uniform = np.full(4, 0.25)
    skew = np.array([0.1, 0.2, 0.3, 0.4])
    tiny = np.array([5e-7, 0.3, 0.3, 0.4 - 5e-7])        # products of the first component underflow at W = 64
    cases = []
    for W in (1, 2, 7, 64):
        const = np.repeat(rng.integers(0, 1001, size=(1, W)), 4, axis=0)
        cases.append((f"constant_columns_W{W}", const, skew))
        a, b = rng.integers(0, 1001, size=(2, W))
        pairs = np.stack([a, b, a, b])
        pairs[:, ::2] = pairs[[0, 0, 1, 1]][:, ::2]      # the equal pairs sit in different rows from column to column
        cases.append((f"two_equal_pairs_W{W}", pairs, skew))
    for name in ("nb1", "nb2", "nb1001"):                # W = 1
        cases.append((f"window_{name}", ref.shape_matrix(name), uniform))
    cases.append(("all_zero_W64", np.zeros((4, 64), dtype=np.int64), skew))
    cases.append(("full_range_W64", ref.shape_matrix("nb64001"), tiny))
    lone = rng.integers(0, 500, size=(4, 64))
    lone[0] = 1000                                       # the top scores are reached through the rare base alone
    cases.append(("rare_base_on_top_W64", lone, tiny))
    cases.append(("rare_base_constant_W64", np.repeat(rng.integers(0, 1001, size=(1, 64)), 4, axis=0), tiny))
    return cases


def test_dp_on_degenerate_matrices_is_bit_identical(dev):
    """comp_pval_mat on matrices whose targets collide (constant columns: all four bases add into one score; two equal
    pairs: two and two), on W = 1, and at W = 64 with a background component of 5e-7, whose products run through the
    denormals to zero so that the reference's `> 0` support test decides which targets are touched."""
    from grafimo_amd.device import comp_pval_mat_dense
    from oracle import oracle as orc
    underflowed = False
    for label, sm, bg in _dp_cases():
        want = orc.comp_pval_mat(sm, bg)
        got = comp_pval_mat_dense(sm, bg)
        diff = np.nonzero(got != want)[0]
        assert len(diff) == 0, (label, "first differing score", int(diff[0]), len(diff))
        lo, hi, _ = ref.matrix_window(sm)
        assert not got[:lo].any() and not got[hi + 1:].any() and got[lo] > 0, label
        underflowed |= bool((got[lo:hi + 1] == 0).any() and (got[got > 0] < 2.0 ** -1022).any())
    assert underflowed                                   # a case did reach the denormals and zero inside its window


# ------------------------------------------------------------------------------------------------ q-value kernels
def _q_handle(name):
    """A handle over the shape with the lognormal tail table; -> (handle, its p_table as the device holds it)."""
    dm = _create(name, [ref.float_pmfs(name, only=["lognormal30"])["lognormal30"]])[0]
    pt = dm.tables()[1]
    assert np.isfinite(pt).all() and pt[pt > 0].min() >= 1e-290                    # no quotient p / (C / n) >= p can be subnormal
    return dm, pt


def _distinct(q_ref, occupied):
    """The distinct reference q-values of the occupied bins, descending (bins of one run share the value object)."""
    out = []
    for s in occupied:
        if not out or q_ref[s] is not out[-1]:
            out.append(q_ref[s])
    return out


def _far_thresholds(distinct):
    """Thresholds that lie further than 4 u (relative) from every reference q of an occupied bin: 1e-300, and a value
    between neighbouring distinct q-values at the top, in the middle and at the bottom of their range."""
    out = [1e-300]
    gaps = [(a, b) for b, a in zip(distinct, distinct[1:]) if b > a * (1 + 64 * U)]
    for a, b in (gaps[:1] + gaps[len(gaps) // 2:len(gaps) // 2 + 1] + gaps[-1:]):
        out.append(float((a + b) / 2))
    if distinct and distinct[0] < Fraction(1, 2):
        out.append(float(distinct[0] * 2))
    return out


def _first_occupied_below(q_ref, occupied, thr):
    """Index into `occupied` of the first bin whose reference q is below thr (q_ref is non-increasing)."""
    a, b = 0, len(occupied)
    while a < b:
        mid = (a + b) // 2
        if q_ref[occupied[mid]] < thr:
            b = mid
        else:
            a = mid + 1
    return a


def _check_q_case(dm, pt, hist, dev, tag, stream=None):
    """One histogram through gfm_qvalue_table against bh_exact: row count, every q entry, monotonicity."""
    lo, hi, L = dm.score_lo, dm.score_hi, dm.L
    q_ref, n_ref = ref.bh_exact(hist, pt, lo, hi, dm.min_val)
    d_h = torch.from_numpy(hist).to(dev)
    q = torch.full((L,), float("nan"), dtype=torch.float64, device=dev)
    cut = torch.full((1,), -7, dtype=torch.int32, device=dev)
    nrows = torch.full((1,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    dm.qvalue_table(d_h, 0.5, True, q, cut, nrows, stream=stream)
    torch.cuda.synchronize()
    q_got = q.cpu().numpy()
    assert int(nrows.item()) == n_ref, (tag, int(nrows.item()), n_ref)
    bad, _ = ref.rel_violations(q_got, q_ref, 3 * U)
    assert not bad, (tag, "first score off", bad[0], "window offset", bad[0] - lo, len(bad), float(q_got[bad[0]]),
                     float(q_ref[bad[0]]))
    rises = np.nonzero(np.diff(q_got) > 0)[0]
    assert len(rises) == 0, (tag, "q rises after score", int(rises[0]))
    assert int(cut.item()) == _first_below(q_got, lo, hi, L, 0.5), tag
    assert torch.equal(d_h.cpu(), torch.from_numpy(hist)), tag      # not cleared unless asked
    return q_ref, q_got, d_h


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_qvalue_tables_of_synthetic_histograms(dev, name):
    W, nb, lo, hi, L = _geometry(name)
    dm, pt = _q_handle(name)
    cut = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch_q = torch.empty(L, dtype=torch.float64, device=dev)
    try:
        for k, (fam, hist) in enumerate(ref.histograms(name).items()):
            tag = (name, fam)
            q_ref, q_got, d_h = _check_q_case(dm, pt, hist, dev, tag)
            occupied = [int(s) for s in np.nonzero(hist[lo:hi + 1])[0] + lo]
            occ = np.array(occupied, dtype=np.int64)

            def cutoff_of(thr, on_q, with_table):
                cut.fill_(-7)
                dm.qvalue_table(d_h, thr, on_q, scratch_q if with_table else None, cut)
                torch.cuda.synchronize()
                if with_table:
                    assert np.array_equal(scratch_q.cpu().numpy(), q_got), tag     # the table does not depend on them
                return int(cut.item())

            # the cutoff is the first window score whose RETURNED value is below the threshold, strictly
            picks = sorted({float(q_got[s]) for s in occupied[:1] + occupied[len(occupied) // 2:][:1] + occupied[-1:]}
                           | {float(q_got[hi])})
            q_thresholds = [1.0, 1e-300] + picks + [float(np.nextafter(v, np.inf)) for v in picks]
            distinct = _distinct(q_ref, occupied)
            far = _far_thresholds(distinct)
            for i, thr in enumerate(q_thresholds + far):
                c = cutoff_of(thr, True, with_table=(i + k) % 2 == 0)
                assert c == _first_below(q_got, lo, hi, L, thr), (tag, "q", thr)
                near = [v for v in distinct if abs(Fraction(thr) - v) <= 4 * U * v]
                if thr in far:
                    assert not near, (tag, thr)          # built to be far: no bin is left out of the comparison
                if not near:                             # the selection is the exact reference's
                    want = occ[_first_occupied_below(q_ref, occupied, Fraction(thr)):]
                    assert np.array_equal(occ[occ >= c], want), (tag, "q selection", thr)
            p_picks = sorted({float(pt[s]) for s in (lo, hi, lo + nb // 2)})
            for i, thr in enumerate([1.0, 1e-300] + p_picks + [float(np.nextafter(v, np.inf)) for v in p_picks]):
                c = cutoff_of(thr, False, with_table=(i + k) % 2 == 1)
                assert c == _first_below(pt, lo, hi, L, thr), (tag, "p", thr)
                assert np.array_equal(occ[occ >= c], occ[pt[occ] < thr]), (tag, "p selection", thr)
            # handed back cleared: the window and the N bin
            work = d_h.clone()
            dm.qvalue_table(work, 0.5, True, None, cut, None, clear_hist=True)
            torch.cuda.synchronize()
            assert int(work.abs().sum().item()) == 0, tag
    finally:
        dm.close()


def test_qvalue_tables_of_eleven_handles_in_one_call(dev):
    """gfm_qvalue_table_multi over eleven handles, more than one group of eight; the first group mixes widths 1, 2, 3 and
    64, so its grid is sized for 251 blocks while other jobs of it use 1 to 5.  Some optional outputs are left out.
    Bit-equal to the single calls (which the test above holds against the exact reference)."""
    from grafimo_amd.device import qvalue_table_multi
    names = ["nb1", "nb2", "nb1001", "nb1023", "nb1024", "nb64001", "nb1025", "w64lo63", "nb2047", "nb2049", "nb5003"]
    assert sorted({ref.SHAPES[n][0] for n in names[:8]}) == [1, 2, 3, 64]
    fams = ["dense+N", "huge_counts", "every_third_block+N", "boundary_rows", "top_block+N", "huge_counts+N",
            "bottom_block", "every_third_block", "empty+N", "dense", "top_block"]
    dms = [_q_handle(n)[0] for n in names]
    try:
        hists = [torch.from_numpy(ref.histograms(n)[f]).to(dev) for n, f in zip(names, fams)]
        for on_q, thr in [(True, 0.05), (False, 1e-3)]:
            single = []
            for dm, h in zip(dms, hists):
                q = torch.empty(dm.L, dtype=torch.float64, device=dev)
                c = torch.zeros(1, dtype=torch.int32, device=dev)
                nr = torch.zeros(1, dtype=torch.int64, device=dev)
                dm.qvalue_table(h, thr, on_q, q, c, nr)
                single.append((q, c, nr))
            work = [h.clone() for h in hists]
            qs = [torch.full((dm.L,), float("nan"), dtype=torch.float64, device=dev) if i not in (4, 5) else None
                  for i, dm in enumerate(dms)]
            cuts = [torch.full((1,), -7, dtype=torch.int32, device=dev) for _ in dms]
            nrs = [torch.full((1,), -7, dtype=torch.int64, device=dev) if i not in (2, 9) else None for i in range(len(dms))]
            qvalue_table_multi(dms, work, thr, on_q, qs, cuts, nrs, clear_hist=True)
            torch.cuda.synchronize()
            for i, (q, c, nr) in enumerate(single):
                if qs[i] is not None:
                    assert torch.equal(qs[i], q), (names[i], on_q)
                assert int(cuts[i].item()) == int(c.item()), (names[i], on_q)
                if nrs[i] is not None:
                    assert int(nrs[i].item()) == int(nr.item()) == int(hists[i].sum().item()), (names[i], on_q)
                assert int(work[i].abs().sum().item()) == 0, (names[i], on_q)
    finally:
        for dm in dms:
            dm.close()


def test_qvalue_table_of_one_handle_from_ten_streams(dev):
    """A handle keeps one scratch set per calling stream, eight of them (kQStreams): the ninth and tenth stream take over
    the sets of the streams that called longest ago, and a first stream that comes back takes one over again.  One call
    after the other, synchronised: every table is still right."""
    name = "nb2049"
    dm, pt = _q_handle(name)
    try:
        hists = list(ref.histograms(name).items())
        streams = [torch.cuda.Stream(device=dev) for _ in range(10)]
        for i, st in enumerate(streams + streams[:2]):
            fam, hist = hists[(3 * i + 1) % len(hists)]
            _check_q_case(dm, pt, hist, dev, (name, fam, "stream", i), stream=st)
    finally:
        dm.close()
