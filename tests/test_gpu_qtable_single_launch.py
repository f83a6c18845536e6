"""gfm_qvalue_table / gfm_qvalue_table_multi around the one-launch q-table kernel (q_table_kernel, gfm_stats_kernels.hpp).

Windows of at most THREADS * K = 8192 bins take the one-launch kernel (thread t owns K consecutive bins), wider ones the
three q_*_kernel passes; both are held against exact rational arithmetic (stats_reference.bh_exact) with the method and
the bound of test_gpu_stats_tables.py: q-values within 3 u relative (two correctly rounded divisions of exact operands;
minima and the clip at 1 are exact), row counts and clears exact, the cutoff the first window score whose returned value
is below the threshold.

Window sizes: 1, 2, 7425 (CTCF), THREADS * K - 1, THREADS * K (the largest the new kernel takes) and THREADS * K + 1 (the
three-kernel path), each with the N bin inside the window (lo == 0 == min_val) and below it (lo > 0).
"""
import os
from fractions import Fraction

import numpy as np
import pytest

import stats_reference as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = Fraction(1, 1 << 53)
BG = np.full(4, 0.25)
THREADS, K, WAVE = 512, 16, 64
LIMIT = THREADS * K
SIZES = [1, 2, 7425, LIMIT - 1, LIMIT, LIMIT + 1]
GEOMETRIES = [(nb, inside) for nb in SIZES for inside in (True, False)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from grafimo_amd import _native as nv
    assert os.path.exists(nv.LIB_PATH), "libgrafimo_hip.so not built"
    return torch.device("cuda:0")


def geometry(nb, inside):
    """(W, lo) of a window of nb bins with the N bin inside (lo == 0) or below it."""
    lo = 0 if inside else 37
    W = max(1 if inside else 2, -(-(nb - 1) // ref.RANGE) + (0 if inside else 1))
    return W, lo


def handle(nb, inside):
    """A handle whose window is [lo, lo + nb - 1] and whose tail table has plateaus (30 % of the bins carry no mass, so
    neighbouring scores tie on p) -> (handle, p_table as the device holds it)."""
    from grafimo_amd.device import DeviceMotif
    W, lo = geometry(nb, inside)
    hi, L = lo + nb - 1, ref.RANGE * W + 1
    sm = ref.window_matrix(W, nb, lo, inside)
    rng = np.random.default_rng([nb, int(inside), 5])
    pmf = np.zeros(L)
    pmf[lo:hi + 1] = np.exp(30.0 * rng.standard_normal(nb))
    pmf[lo:hi + 1][rng.random(nb) < 0.3] = 0.0
    pmf[hi] = 1.0
    dm = DeviceMotif._create_many([(sm, BG, 0, 1, 0.0, pmf)])[0]
    assert (dm.score_lo, dm.score_hi, dm.L, dm.min_val) == (lo, hi, L, 0)
    pt = dm.tables()[1]
    assert np.isfinite(pt).all() and pt[pt > 0].min() >= 1e-290       # no quotient p / (C / n) >= p can be subnormal
    return dm, pt


def histograms(nb, lo, L):
    """{name: int64 [L]}: empty, one occupied bin at lo / at hi, rows on the thread and wave boundaries of the blocked
    scan, dense counts with many equal ones (ties), counts above 2**32; each without and with rows that hold an N (bin
    min_val = 0: bin lo itself when lo == 0, below the window otherwise)."""
    hi = lo + nb - 1
    rng = np.random.default_rng([nb, lo, 6])
    base = {"empty": np.zeros(L, dtype=np.int64)}
    a = np.zeros(L, dtype=np.int64)
    a[lo] = 7
    base["one_bin_lo"] = a
    a = np.zeros(L, dtype=np.int64)
    a[hi] = (1 << 33) + 5
    base["one_bin_hi"] = a
    a = np.zeros(L, dtype=np.int64)
    for j in (0, K - 1, K, WAVE * K - 1, WAVE * K, nb - K, nb - 1):
        if 0 <= j < nb:
            a[lo + j] = 1
    base["boundaries"] = a
    a = np.zeros(L, dtype=np.int64)
    a[lo:hi + 1] = rng.integers(0, 4, size=nb)
    base["ties"] = a
    a = np.zeros(L, dtype=np.int64)
    occ = rng.random(nb) < 0.02
    occ[rng.integers(0, nb)] = True
    a[lo:hi + 1][occ] = rng.integers(1, (1 << 40) + 1, size=int(occ.sum()))
    base["huge_sparse"] = a
    out = {}
    for k, (name, a) in enumerate(base.items()):
        out[name] = a
        b = a.copy()
        b[0] += (1 << 34) + 3 if k % 2 == 0 else 2 + k
        out[name + "+N"] = b
    return out


def first_below(values, lo, hi, L, thr):
    idx = np.nonzero(values[lo:hi + 1] < thr)[0]
    return lo + int(idx[0]) if len(idx) else L


def check_table(tag, q_got, n_got, hist, pt, lo, hi, min_val):
    q_ref, n_ref = ref.bh_exact(hist, pt, lo, hi, min_val)
    assert n_got == n_ref, (tag, n_got, n_ref)
    bad, _ = ref.rel_violations(q_got, q_ref, 3 * U)
    assert not bad, (tag, "first score off", bad[0], "window offset", bad[0] - lo, len(bad), float(q_got[bad[0]]),
                     float(q_ref[bad[0]]))
    rises = np.nonzero(np.diff(q_got) > 0)[0]
    assert len(rises) == 0, (tag, "q rises after score", int(rises[0]))


@pytest.mark.parametrize("nb,inside", GEOMETRIES, ids=[f"nb{nb}_{'Nin' if i else 'Nbelow'}" for nb, i in GEOMETRIES])
def test_qvalue_table_at_the_single_launch_limit(dev, nb, inside):
    dm, pt = handle(nb, inside)
    lo, hi, L = dm.score_lo, dm.score_hi, dm.L
    cut = torch.zeros(1, dtype=torch.int32, device=dev)
    nrows = torch.zeros(1, dtype=torch.int64, device=dev)
    try:
        for k, (name, hist) in enumerate(histograms(nb, lo, L).items()):
            tag = (nb, inside, name)
            d_h = torch.from_numpy(hist).to(dev)
            q = torch.full((L,), float("nan"), dtype=torch.float64, device=dev)
            cut.fill_(-7)
            nrows.fill_(-7)
            dm.qvalue_table(d_h, 0.5, True, q, cut, nrows)
            torch.cuda.synchronize()
            q_got = q.cpu().numpy()
            check_table(tag, q_got, int(nrows.item()), hist, pt, lo, hi, dm.min_val)
            assert int(cut.item()) == first_below(q_got, lo, hi, L, 0.5), tag
            assert torch.equal(d_h.cpu(), torch.from_numpy(hist)), tag              # not cleared unless asked
            # thresholds on q and on p that equal a returned value (strict <), the next float above it, 1 and 1e-300;
            # with and without a q-table, with and without the clear
            occupied = np.nonzero(hist[lo:hi + 1])[0] + lo
            picks = {float(q_got[lo]), float(q_got[hi])} | {float(q_got[s]) for s in occupied[len(occupied) // 2:][:1]}
            p_picks = {float(pt[lo]), float(pt[hi]), float(pt[lo + nb // 2])}
            cases = [(True, v) for v in sorted(picks)] + [(False, v) for v in sorted(p_picks)]
            cases += [(on_q, float(np.nextafter(v, np.inf))) for on_q, v in list(cases)]
            cases += [(True, 1.0), (True, 1e-300), (False, 1.0), (False, 1e-300)]
            for i, (on_q, thr) in enumerate(cases):
                clear = (i + k) % 2 == 0
                with_table = (i + k) % 3 != 0
                work = d_h.clone()
                q2 = torch.full((L,), float("nan"), dtype=torch.float64, device=dev) if with_table else None
                cut.fill_(-7)
                dm.qvalue_table(work, thr, on_q, q2, cut, None, clear_hist=clear)
                torch.cuda.synchronize()
                if with_table:
                    assert np.array_equal(q2.cpu().numpy(), q_got), (tag, on_q, thr)  # the table does not depend on them
                assert int(cut.item()) == first_below(q_got if on_q else pt, lo, hi, L, thr), (tag, on_q, thr)
                if clear:
                    assert int(work.abs().sum().item()) == 0, (tag, "cleared: the window and the N bin")
                else:
                    assert torch.equal(work, d_h), tag
    finally:
        dm.close()


def test_nine_handles_of_mixed_widths_in_one_call(dev):
    """gfm_qvalue_table_multi over nine handles: two groups, eight and one.  The group of eight (windows of 1 to 8193
    bins) takes the three-kernel path, the lone ninth motif (5003 bins) the one-launch kernel.  Some optional outputs
    are left out.  Every table against the exact reference."""
    from grafimo_amd.device import qvalue_table_multi
    geos = [(1, True), (LIMIT + 1, False), (2, False), (7425, False), (LIMIT, True), (LIMIT - 1, False), (100, True),
            (1025, False), (5003, True)]
    names = ["one_bin_lo+N", "ties+N", "one_bin_hi", "ties", "huge_sparse+N", "boundaries+N", "empty+N", "ties+N",
             "huge_sparse"]
    made = [handle(nb, inside) for nb, inside in geos]
    dms = [m[0] for m in made]
    assert sorted({dm.width for dm in dms})[0] == 1 and max(dm.width for dm in dms) >= 9
    try:
        hosts = [histograms(nb, dm.score_lo, dm.L)[name] for (nb, _), dm, name in zip(geos, dms, names)]
        for on_q, thr, clear in [(True, 0.05, True), (False, 1e-3, False)]:
            work = [torch.from_numpy(h).to(dev) for h in hosts]
            qs = [torch.full((dm.L,), float("nan"), dtype=torch.float64, device=dev) for dm in dms]
            cuts = [torch.full((1,), -7, dtype=torch.int32, device=dev) for _ in dms]
            nrs = [torch.full((1,), -7, dtype=torch.int64, device=dev) if i not in (2, 8) else None
                   for i in range(len(dms))]
            qvalue_table_multi(dms, work, thr, on_q, qs, cuts, nrs, clear_hist=clear)
            torch.cuda.synchronize()
            for i, ((dm, pt), hist) in enumerate(zip(made, hosts)):
                tag = (geos[i], names[i], on_q)
                lo, hi, L = dm.score_lo, dm.score_hi, dm.L
                q_got = qs[i].cpu().numpy()
                n_ref = int(hist[lo:hi + 1].sum()) + (0 if lo == 0 else int(hist[0]))
                check_table(tag, q_got, int(nrs[i].item()) if nrs[i] is not None else n_ref, hist, pt, lo, hi, dm.min_val)
                assert int(cuts[i].item()) == first_below(q_got if on_q else pt, lo, hi, L, thr), tag
                if clear:
                    assert int(work[i].abs().sum().item()) == 0, tag
                else:
                    assert torch.equal(work[i].cpu(), torch.from_numpy(hist)), tag
    finally:
        for dm in dms:
            dm.close()
