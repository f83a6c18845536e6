"""The histogram and hit booking of score_quad_kernel (book() and the ragged-end loop of gfm_score_quad.hpp).

Scores, the uint64 histogram and the hit set of gfm_score_kmers / gfm_score_kmers_multi against oracle.score_kmers_table:
the histogram must equal np.bincount of the oracle's scores and the hits the rows whose oracle score reaches the cutoff,
exactly.  The three destinations of a booked row are all driven: the in-window LDS bin, the N bin behind the window and
the global spill counter of a partial window.

Row counts (a wave takes chunks of 256 rows; the < 256 rows behind the last whole chunk go through the ragged-end loop):
255, 256, 257, 16 * 256 + 3 (one workgroup, every wave one chunk), and the smallest count at which every wave of the
grid makes at least two turns and some make three, (n_cu * 16 * 2 + 5) * 256 + 77: a chunk is booked one step late, at
the top of the wave's next turn or behind its loop, so a wave's first, middle and last chunk take different paths.
Every case runs with score arrays and without (d_scores NULL: another instantiation of the kernel).
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 256
WAVES = 16
LDS_BYTES = 160 * 1024          # per CU on gfx950


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from grafimo_amd import _native as nv
    assert os.path.exists(nv.LIB_PATH), "libgrafimo_hip.so not built"
    return torch.device("cuda:0")


def row_counts():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return [255, 256, 257, WAVES * CHUNK + 3, (n_cu * WAVES * 2 + 5) * CHUNK + 77]


COUNT_IDS = ["255", "256", "257", "one_wg", "multi_turn"]


@functools.lru_cache(maxsize=2)
def kmers(n, W, extra=None):
    """uint8 [n, W]: uniform bases, 0.5 % of the rows with an N, 5 % of the rows in lower case (lower-case n is outside the
    reference's domain and stays upper case), an N in the first and in the last row of every chunk boundary that exists
    near both ends of the batch, one of them in the last base of its row.  `extra`: rows (bytes objects) written over rows
    1.. of the batch.  Left unchanged by its users."""
    rng = np.random.default_rng([n, W])
    km = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, W))
    nn = rng.random(n) < 0.005
    pos = rng.integers(0, W, size=n)
    km[nn, pos[nn]] = ord("N")
    low = rng.random(n) < 0.05
    km[low] |= 0x20
    last_chunk = (n // CHUNK - 1) * CHUNK
    for r, p in ((0, W // 2), (CHUNK - 1, W - 1), (last_chunk, W - 1), (last_chunk + CHUNK - 1, 0), (n - 1, W - 1)):
        if 0 <= r < n:
            km[r, p] = ord("N")
    for i, row in enumerate(extra or ()):
        km[1 + i] = np.frombuffer(row, dtype=np.uint8)
    km[km == ord("n")] = ord("N")
    km.setflags(write=False)
    return km


@functools.lru_cache(maxsize=8)
def expected(key, n, W, extra=None):
    """Oracle scores of motif `key` over kmers(n, W, extra): computed once, shared by the runs with and without score arrays."""
    from oracle import oracle as orc
    sm, pt, min_val = SPECS[key]
    exp, _ = orc.score_kmers_table(kmers(n, W, extra), sm, pt, min_val)
    exp.setflags(write=False)
    return exp


SPECS = {}      # key -> (score matrix, tail table of the handle, min_val)


def run_single(dev, dm, key, n, extra=None):
    W = dm.width
    km = kmers(n, W, extra)
    exp = expected(key, n, W, extra)
    want_hist = np.bincount(exp, minlength=dm.L)
    cut = dm.pvalue_cutoff(1e-3)
    rows = np.nonzero(exp >= cut)[0]
    d_k = torch.from_numpy(km.copy()).to(dev)
    for with_scores in (True, False):
        d_sc = torch.full((n,), -3, dtype=torch.int32, device=dev) if with_scores else None
        d_hist = torch.zeros(dm.L, dtype=torch.int64, device=dev)
        hits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        dm.score(d_k, d_sc, hist=d_hist, select_cutoff=cut, row_base=7, hit_rows=hits[1:], hit_count=hits[:1],
                 reset_hits=True)
        torch.cuda.synchronize()
        tag = (key, n, with_scores)
        if with_scores:
            assert np.array_equal(d_sc.cpu().numpy(), exp), tag
        assert np.array_equal(d_hist.cpu().numpy(), want_hist), tag
        k = int(hits[0].item())
        assert k == len(rows), tag
        got = np.sort(hits[1:1 + k].cpu().numpy())
        assert np.array_equal(got >> 20, rows + 7) and np.array_equal(got & 0xFFFFF, exp[rows]), tag
    return exp


# ------------------------------------------------------------------------------------------------ CTCF: whole window
@pytest.fixture(scope="module")
def ctcf(dev):
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.motif_ops import build_motif_meme_host
    motif = build_motif_meme_host(os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"), "unfrm_dst", 0.1,
                                  False)[0]
    sm = motif.dense_score_matrix()
    dm = DeviceMotif(sm, motif.dense_bg(), motif.min_val, motif.scale, motif.offset)
    assert dm.width == 19
    SPECS["ctcf"] = (sm, dm.tables()[1], motif.min_val)
    yield dm
    dm.close()


@pytest.mark.parametrize("which", range(5), ids=COUNT_IDS)
def test_ctcf_whole_window(dev, ctcf, which):
    n = row_counts()[which]
    exp = run_single(dev, ctcf, "ctcf", n)
    assert (exp == ctcf.min_val).any()                          # the N bin is driven (it lies below CTCF's window)
    assert ctcf.min_val < ctcf.score_lo


# ------------------------------------------------------------------------------------------------ W = 40: partial window
@pytest.fixture(scope="module")
def wide(dev):
    """A W = 40 matrix with a 0 and a 1000 in every column: the reachable scores are 0 .. 40 000, 40 001 bins.  The strips
    of the 8 waves a workgroup has at least (8 x 64 lanes x 4 W bytes = 81 920 of a CU's 163 840 bytes of LDS) leave room
    for at most 20 480 bins, so the window is partial whatever the launch plan picks."""
    from grafimo_amd.device import DeviceMotif
    rng = np.random.default_rng(4040)
    sm = rng.integers(0, 1001, size=(4, 40)).astype(np.int64)
    sm[0, :] = 0
    sm[3, :] = 1000
    bg = np.full(4, 0.25)
    dm = DeviceMotif(sm, bg, 0, 100, -10.0)
    assert (dm.score_lo, dm.score_hi, dm.min_val) == (0, 40_000, 0)
    SPECS["wide"] = (sm, dm.tables()[1], 0)
    yield dm, sm
    dm.close()


# rows 1..3 of every W = 40 batch: all T (40 000, the top of the range), A with one T (1000) and A with two T (2000)
WIDE_EXTRA = (b"T" * 40, b"A" * 39 + b"T", b"A" * 38 + b"TT")


@pytest.mark.parametrize("which", range(5), ids=COUNT_IDS)
def test_wide_motif_partial_window_and_spill(dev, wide, which):
    """All three destinations, shown on the CPU from the oracle's scores and the motif's score distribution alone.  The
    window is a run of B consecutive bins holding the most background probability, 8192 <= B <= 20 480 (upper bound: see
    the fixture; lower bound: what the tables, 8 strips with their padding and the hit queues leave is more than 32 KB).
      N bin:    a row holds an N.
      outside:  two rows without N score further apart than 20 480, so no window holds both.
      inside:   the best window of B >= 8192 bins holds at least the mass M of the best 8192-bin window, and a run of
                bins of mass >= M contains every score s with P(score <= s) > 1 - M and P(score >= s) > 1 - M; a row
                without N has such a score."""
    from oracle import oracle as orc
    dm, sm = wide
    n = row_counts()[which]
    exp = run_single(dev, dm, "wide", n, WIDE_EXTRA)
    km = kmers(n, 40, WIDE_EXTRA)
    has_n = (km == ord("N")).any(axis=1)
    assert has_n.any() and (exp[has_n] == 0).all()
    clean = exp[~has_n]
    assert int(clean.max()) - int(clean[clean > 0].min()) > LDS_BYTES // 2 // 4
    pmf = orc.comp_pval_mat(sm, np.full(4, 0.25))
    pmf = pmf / pmf.sum()
    cum = np.concatenate([[0.0], np.cumsum(pmf)])
    B = 8192
    M = float((cum[B:] - cum[:-B]).max())
    assert M > 0.5
    cdf, sf = cum[1:], 1.0 - cum[:-1]
    slack = 1e-9                                                # the sums above are f64: keep clear of their rounding
    core = (cdf > 1 - M + slack) & (sf > 1 - M + slack)
    assert core[clean].any()


# ------------------------------------------------------------------------------------------------ W = 12, two and three motifs
@pytest.fixture(scope="module", params=[2, 3], ids=["MM2", "MM3"])
def batched(dev, request):
    from grafimo_amd.device import DeviceMotif, multi_plan
    MM = request.param
    rng = np.random.default_rng(1200 + MM)
    motifs, keys = [], []
    for k in range(MM):
        span = 4200 // (12 * MM)
        base = rng.integers(0, 1001 - span, size=12)
        sm = (base[None, :] + rng.integers(0, span + 1, size=(4, 12))).astype(np.int64)
        sm[rng.integers(0, 4), rng.integers(0, 12)] = 0
        dm = DeviceMotif(sm, rng.dirichlet([30, 20, 20, 30]), int(sm.min()), 40 + k, -9.0 - k)
        SPECS[f"w12_{MM}_{k}"] = (sm, dm.tables()[1], int(sm.min()))
        motifs.append(dm)
        keys.append(f"w12_{MM}_{k}")
    sizes, _ = multi_plan(motifs)
    assert list(sizes) == [MM] * MM                             # one launch of score_quad_kernel<12, MM>
    yield motifs, keys
    for m in motifs:
        m.close()


@pytest.mark.parametrize("which", range(5), ids=COUNT_IDS)
def test_batched_motifs(dev, batched, which):
    from grafimo_amd.device import score_multi
    motifs, keys = batched
    n = row_counts()[which]
    km = kmers(n, 12)
    d_k = torch.from_numpy(km.copy()).to(dev)
    cuts = [m.pvalue_cutoff(1e-3) for m in motifs]
    for with_scores in (True, False):
        scores = [torch.full((n,), -3, dtype=torch.int32, device=dev) for _ in motifs] if with_scores else None
        hists = [torch.zeros(m.L, dtype=torch.int64, device=dev) for m in motifs]
        hits = [torch.zeros(n + 1, dtype=torch.int64, device=dev) for _ in motifs]
        score_multi(motifs, d_k, scores, hists=hists, cutoffs=cuts, row_base=7, hit_rows=[h[1:] for h in hits],
                    hit_counts=[h[:1] for h in hits], reset_hits=True)
        torch.cuda.synchronize()
        for j, (m, key) in enumerate(zip(motifs, keys)):
            tag = (key, n, with_scores)
            exp = expected(key, n, 12)
            if with_scores:
                assert np.array_equal(scores[j].cpu().numpy(), exp), tag
            assert np.array_equal(hists[j].cpu().numpy(), np.bincount(exp, minlength=m.L)), tag
            rows = np.nonzero(exp >= cuts[j])[0]
            k = int(hits[j][0].item())
            assert k == len(rows), tag
            got = np.sort(hits[j][1:1 + k].cpu().numpy())
            assert np.array_equal(got >> 20, rows + 7) and np.array_equal(got & 0xFFFFF, exp[rows]), tag
            assert (exp == m.min_val).any(), tag
