"""GFM_FLAG_OVERLAP_LAUNCHES: the score kernels of consecutive KmerScanner batches go to two streams of the motif handle's
own, in turn, instead of the caller's stream, so that nothing orders kernel k+1 behind kernel k.  What must hold then:
every batch's scores, q-table, row count and hit list are what the same sequence gives in stream order
(GRAFIMO_SCORE_OVERLAP=0) and what the CPU oracle gives; a caller stream that still holds work (possibly the producer of
the k-mers) puts the call's kernel behind that work; and the cases that do not qualify -- device-paced slots, no
side stream, a second user of the handle -- never overlap, which the handle's counter of overlapped launches shows.

Row counts: a workgroup of 16 waves takes 256 rows per wave and step.  200 rows: less than one wave's step; 5 * 256 + 17:
a ragged end; 256 * 16 * 3: three whole workgroups; 1 100 017: more than one turn of a 256-CU grid (256 x 16 x 256 =
1 048 576 rows), ragged, and kernels long enough (a few microseconds) to be on the device side by side."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", np.uint8)
SIZES = [200, 5 * 256 + 17, 256 * 16 * 3, 1_100_017]
TURNS = 12
QTOL = dict(rtol=1e-12, atol=0)          # the parity tests' tolerance for q-values against orc.fdr_bh


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=1)
def ctcf_numbers():
    from grafimo_amd.motif_ops import build_motif_meme_host
    motif = build_motif_meme_host(os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"), "unfrm_dst", 0.1,
                                  False)[0]
    return motif.dense_score_matrix(), motif.dense_bg(), motif.min_val, motif.scale, motif.offset


@functools.lru_cache(maxsize=1)
def wide_numbers():
    """W = 40 with a 0 and a 1000 in every column (test_gpu_score_booking's): 40 001 reachable scores, more than any LDS
    window, so rows outside the window go to the spill counters."""
    rng = np.random.default_rng(4040)
    sm = rng.integers(0, 1001, size=(4, 40)).astype(np.int64)
    sm[0, :] = 0
    sm[3, :] = 1000
    return sm, np.full(4, 0.25), 0, 100, -10.0


def fresh_motif(numbers):
    from grafimo_amd.device import DeviceMotif
    return DeviceMotif(*numbers)


@functools.lru_cache(maxsize=2)
def tables(which):
    """(score matrix, min_val, tail table) of 'ctcf' / 'wide'; the tail table is the handle's own (the device DP is
    bit-exact to the oracle's: test_gpu_parity)."""
    numbers = ctcf_numbers() if which == "ctcf" else wide_numbers()
    dm = fresh_motif(numbers)
    pt = dm.tables()[1]
    dm.close()
    return numbers[0], numbers[2], pt


@functools.lru_cache(maxsize=16)
def batch(which, n, b):
    """Batch `b` of `n` rows: random ACGT, an N in about 1 % of the rows, and n // 200 rows that spell the motif's best
    k-mer with one random base changed (so that a q-value threshold keeps some).  -> (k-mers, oracle scores, p, q)."""
    from oracle import oracle as orc
    sm, min_val, pt = tables(which)
    W = sm.shape[1]
    rng = np.random.default_rng([n, W, b])
    km = rng.choice(ACGT, size=(n, W))
    bad = rng.random(n) < 0.01
    km[bad, rng.integers(0, W, n)[bad]] = ord("N")
    best = ACGT[np.argmax(sm, axis=0)]
    for r in rng.choice(n, size=max(1, n // 200), replace=False):
        km[r] = best
        km[r, rng.integers(0, W)] = rng.choice(ACGT)
    sc, p = orc.score_kmers_table(km, sm, pt, min_val)
    q = orc.fdr_bh(p)
    for a in (km, sc, p, q):
        a.setflags(write=False)
    return km, sc, p, q


WARM = 4        # GFM_WORKSPACE_RING


def pipeline(dev, dm, which, n, thr, on_q, turns=TURNS, collect_at=(4, 8), scanner_kw=None, sc=None, overlap_q=False):
    """`turns` enqueues of the two batches in turn without a synchronisation in between (beyond the scanner's own pacing);
    the turn two back is collected at the turns of `collect_at` while its successors are in flight, the last n_slots at
    the end.  -> {turn: (collect() result, scores)}.
    A scanner made here first runs WARM batches and drains the device, as a pipeline's warm-up does: the library honours
    the flags only once the workspace ring's worth of calls on the handle came from this scanner's stream pair, and those
    first calls sit on the caller's stream, which must be found empty for a launch to leave it.  From there on nothing is
    ever put on the caller's stream, so WHICH launches overlap is known: all of them, if the scanner passes the flag."""
    from grafimo_amd.scan import KmerScanner
    d = [torch.from_numpy(batch(which, n, b)[0].copy()).to(dev) for b in range(2)]
    if sc is None:
        sc = KmerScanner(dm, n, device=dev, **(scanner_kw or {"n_slots": 3}))
        sc.overlap_qvalue_batches = overlap_q
        for t in range(WARM):
            sc.enqueue(d[t % 2], thr, on_qvalue=on_q)
        sc.finish()
    torch.cuda.synchronize(dev)
    n_slots = len(sc.slots)
    out, slots = {}, {}

    def take(t):
        res = sc.collect(slots[t])
        out[t] = (res, slots[t].scores[:n].cpu().numpy())

    for t in range(turns):
        slots[t] = sc.enqueue(d[t % 2], thr, on_qvalue=on_q)
        if t in collect_at and n_slots >= 3:
            take(t - 2)
    for t in range(turns - n_slots, turns):
        take(t)
    return sc, out


def check_against_oracle(which, n, thr, on_q, out):
    for t, (res, scores) in out.items():
        km, sc, p, q = batch(which, n, t % 2)
        keep = np.nonzero((q if on_q else p) < thr)[0]
        assert np.array_equal(scores, sc), t
        assert res["n_scored"] == n, t
        np.testing.assert_allclose(res["qtable"][sc], q, err_msg=str(t), **QTOL)
        assert np.array_equal(res["rows"], keep), t
        assert np.array_equal(res["scaled"], sc[keep]), t


def check_same(a, b):
    assert sorted(a) == sorted(b)
    for t in a:
        (ra, sa), (rb, sb) = a[t], b[t]
        assert np.array_equal(sa, sb), t
        assert ra["n_scored"] == rb["n_scored"], t
        assert np.array_equal(ra["qtable"], rb["qtable"]), t          # one histogram, one kernel: the same bits
        assert np.array_equal(ra["rows"], rb["rows"]) and np.array_equal(ra["scaled"], rb["scaled"]), t


@pytest.mark.parametrize("n", SIZES)
def test_bit_identity_under_overlap(dev, monkeypatch, n):
    """Twelve batches, three slots: overlapped == in stream order == oracle, for the slots collected along the way and
    for those valid at the end."""
    monkeypatch.delenv("GRAFIMO_SCORE_OVERLAP", raising=False)
    dm = fresh_motif(ctcf_numbers())
    sc, over = pipeline(dev, dm, "ctcf", n, 1e-2, False)
    assert sc.overlap
    assert dm.overlapped_launches() == TURNS
    dm.close()
    monkeypatch.setenv("GRAFIMO_SCORE_OVERLAP", "0")
    dm = fresh_motif(ctcf_numbers())
    sc, plain = pipeline(dev, dm, "ctcf", n, 1e-2, False)
    assert not sc.overlap and dm.overlapped_launches() == 0
    dm.close()
    assert len(over) == 5
    check_against_oracle("ctcf", n, 1e-2, False, over)
    check_same(over, plain)


def test_library_switch_ignores_the_flag(dev, monkeypatch):
    """GRAFIMO_SCORE_OVERLAP=0 while the HANDLE is created, gone when the scanner is: the scanner passes the flag, the
    library ignores it.  No launch overlaps, results unchanged."""
    from grafimo_amd.scan import KmerScanner
    n = SIZES[1]
    monkeypatch.setenv("GRAFIMO_SCORE_OVERLAP", "0")
    dm = fresh_motif(ctcf_numbers())
    monkeypatch.delenv("GRAFIMO_SCORE_OVERLAP")
    sc = KmerScanner(dm, n, device=dev, n_slots=3)
    assert sc.overlap
    pipeline(dev, dm, "ctcf", n, 1e-2, False, turns=WARM, collect_at=(), sc=sc)
    _, out = pipeline(dev, dm, "ctcf", n, 1e-2, False, sc=sc)
    assert dm.overlapped_launches() == 0
    check_against_oracle("ctcf", n, 1e-2, False, out)
    dm.set_overlap(True)                         # ... and the same pipeline with the switch back on
    _, out = pipeline(dev, dm, "ctcf", n, 1e-2, False, sc=sc)
    assert dm.overlapped_launches() == TURNS
    check_against_oracle("ctcf", n, 1e-2, False, out)
    dm.close()


def test_busy_caller_stream_falls_back_and_stays_ordered(dev, monkeypatch):
    """The k-mers are produced on the caller's stream right before enqueue() -- behind a 2 GiB device copy that keeps the
    stream busy for the better part of a millisecond -- with no host synchronisation: the library must find the stream
    busy and order the kernel behind it, and the scores show the edit (rows 3 and 4 become the motif's best k-mer).
    Before that the pipeline's kernels had nothing in front of them, and they have again once the caller's stream has
    drained (the library asks again after three more calls)."""
    from grafimo_amd.scan import KmerScanner
    from oracle import oracle as orc
    monkeypatch.delenv("GRAFIMO_SCORE_OVERLAP", raising=False)
    n = SIZES[2]
    sm, min_val, pt = tables("ctcf")
    km0 = batch("ctcf", n, 0)[0]
    best = ACGT[np.argmax(sm, axis=0)]
    edited = km0.copy()
    edited[3] = edited[4] = best
    exp_edit, p_edit = orc.score_kmers_table(edited, sm, pt, min_val)
    assert exp_edit[3] == sm.max(axis=0).sum() != batch("ctcf", n, 0)[1][3]
    d_best = torch.from_numpy(best.copy()).to(dev)
    base = torch.from_numpy(km0.copy()).to(dev)
    big = torch.zeros(1 << 31, dtype=torch.uint8, device=dev)

    def produce():
        keep = big.clone()                       # long-running work on the current stream ...
        d = base.clone()                         # ... and behind it the producer of the k-mers
        d[3:5] = d_best
        return keep, d

    produce()                                    # once for the allocator: the second time allocates nothing
    torch.cuda.synchronize(dev)
    dm = fresh_motif(ctcf_numbers())
    sc, out = pipeline(dev, dm, "ctcf", n, 1e-2, False, turns=6, collect_at=())
    check_against_oracle("ctcf", n, 1e-2, False, out)
    before = dm.overlapped_launches()
    assert before == 6
    torch.cuda.synchronize(dev)
    keep, d = produce()
    slot = sc.enqueue(d, 1e-2)
    assert dm.overlapped_launches() == before, "the caller's stream was busy: the kernel must have waited for it"
    res = sc.collect(slot)
    assert np.array_equal(slot.scores[:n].cpu().numpy(), exp_edit)
    assert np.array_equal(res["rows"], np.nonzero(p_edit < 1e-2)[0])
    del keep
    # ... and forward again: collect() waited for that batch, so the caller's stream is empty when the library next asks
    _, out = pipeline(dev, dm, "ctcf", n, 1e-2, False, turns=8, collect_at=(4,), sc=sc)
    check_against_oracle("ctcf", n, 1e-2, False, out)
    assert dm.overlapped_launches() >= before + 4
    dm.close()


def test_partial_window_motif_counts_every_row(dev, monkeypatch):
    """W = 40, partial LDS window: the rows outside it are counted in the spill counters, which the score kernel adds
    to and the post kernel hands back zeroed.  They belong to the workspace ring (one set per call in flight), so
    overlapped kernels never share one: driven through the library as the scanner drives it (side stream, host-paced
    three back, the flags), twelve calls behind a warm-up with a histogram of their own each; every histogram equals the oracle's
    counts exactly.  Then the scanner itself over the same batches: q-table, row count and hits."""
    from grafimo_amd import _native as nv
    monkeypatch.delenv("GRAFIMO_SCORE_OVERLAP", raising=False)
    n = SIZES[1]
    dm = fresh_motif(wide_numbers())
    exp = [batch("wide", n, b) for b in range(2)]
    lo, hi = dm.score_lo, dm.score_hi
    assert any(int(e[1].max()) - int(e[1][e[1] > 0].min()) > 160 * 1024 // 2 // 4 for e in exp)      # wider than any window
    d = [torch.from_numpy(e[0].copy()).to(dev) for e in exp]
    hists = torch.zeros((WARM + TURNS, dm.L), dtype=torch.int64, device=dev)
    scores = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3)]
    side = torch.cuda.Stream(device=dev, priority=-1)
    done = [torch.cuda.Event() for _ in range(WARM + TURNS)]
    torch.cuda.synchronize(dev)
    main_p = torch.cuda.current_stream(dev).cuda_stream
    flags = nv.GFM_FLAG_CALLER_ORDERS_REUSE | nv.GFM_FLAG_OVERLAP_LAUNCHES
    for t in range(WARM + TURNS):
        if t == WARM:
            torch.cuda.synchronize(dev)          # the warm-up's fence: see pipeline()
        if t >= 3:
            done[t - 3].synchronize()
        nv.check(nv.lib().gfm_score_kmers(dm.handle, d[t % 2].data_ptr(), n, scores[t % 3].data_ptr(), hists[t].data_ptr(),
                                          nv.GFM_NO_SELECT, 0, None, 0, None, flags, main_p, side.cuda_stream))
        done[t].record(side)
    torch.cuda.synchronize(dev)
    assert dm.overlapped_launches() == TURNS
    got = hists.cpu().numpy()
    for t in range(WARM + TURNS):
        assert np.array_equal(got[t], np.bincount(exp[t % 2][1], minlength=dm.L)), t
    assert lo == 0 and hi == 40_000
    _, out = pipeline(dev, dm, "wide", n, 1e-2, False)
    check_against_oracle("wide", n, 1e-2, False, out)
    dm.close()


def test_qvalue_threshold_with_candidates(dev, monkeypatch):
    """on_qvalue=True: the score kernel collects the p < t candidates, the tail selects on q from them.  Six enqueues
    with the launches overlapped (the scanner keeps such batches in stream order unless told otherwise: their tail is
    the longest): the hit lists equal those of the scanner's default, of the run with the switch off, and the oracle's."""
    n = SIZES[3]
    monkeypatch.delenv("GRAFIMO_SCORE_OVERLAP", raising=False)
    dm = fresh_motif(ctcf_numbers())
    sc, over = pipeline(dev, dm, "ctcf", n, 0.3, True, turns=6, collect_at=(4,), overlap_q=True)
    assert sc.overlap and sc.candidates and dm.overlapped_launches() == 6
    dm.close()
    dm = fresh_motif(ctcf_numbers())
    sc, default = pipeline(dev, dm, "ctcf", n, 0.3, True, turns=6, collect_at=(4,))
    assert sc.overlap and dm.overlapped_launches() == 0
    dm.close()
    monkeypatch.setenv("GRAFIMO_SCORE_OVERLAP", "0")
    dm = fresh_motif(ctcf_numbers())
    _, plain = pipeline(dev, dm, "ctcf", n, 0.3, True, turns=6, collect_at=(4,))
    assert dm.overlapped_launches() == 0
    dm.close()
    assert all(len(r["rows"]) > 100 for r, _ in over.values())
    check_same(over, plain)
    check_same(default, plain)
    check_against_oracle("ctcf", n, 0.3, True, over)


def test_thresholds_on_p_and_on_q_in_turn(dev, monkeypatch):
    """One scanner, p-value and q-value batches alternating: the first kind overlaps, the second stays on the caller's
    stream, so every batch changes the mode (the caller's stream joins the launch streams, the next launch waits for the
    caller's stream).  Every batch equals the oracle."""
    from grafimo_amd.scan import KmerScanner
    monkeypatch.delenv("GRAFIMO_SCORE_OVERLAP", raising=False)
    n = SIZES[3]
    dm = fresh_motif(ctcf_numbers())
    sc = KmerScanner(dm, n, device=dev, n_slots=3)
    d = [torch.from_numpy(batch("ctcf", n, b)[0].copy()).to(dev) for b in range(2)]
    torch.cuda.synchronize(dev)
    plan = [(1e-2, False), (0.3, True)]
    slots = {}
    for t in range(TURNS + 1):
        slots[t] = sc.enqueue(d[t % 2], plan[t % 3 % 2][0], on_qvalue=plan[t % 3 % 2][1])
        if t >= 2:
            u = t - 2
            thr, on_q = plan[u % 3 % 2]
            res = sc.collect(slots[u])
            check_against_oracle("ctcf", n, thr, on_q, {u: (res, slots[u].scores[:n].cpu().numpy())})
    sc.finish()
    torch.cuda.synchronize(dev)
    assert dm.overlapped_launches() <= TURNS + 1 - 4 - 3        # the first four calls and the q-value batches never count
    dm.close()


@pytest.mark.parametrize("kw", [dict(n_slots=2), dict(n_slots=3, side_stream=False), dict(n_slots=5)],
                         ids=["two_slots", "no_side_stream", "five_slots"])
def test_unqualified_scanners_do_not_pass_the_flag(dev, monkeypatch, kw):
    """Device-paced slots, no side stream, more slots than the library's workspace ring: stream order is what protects
    these pipelines, the flag is not passed even when the switch asks for overlap, and no launch overlaps."""
    from grafimo_amd import _native as nv
    monkeypatch.setenv("GRAFIMO_SCORE_OVERLAP", "1")
    n = SIZES[1]
    dm = fresh_motif(ctcf_numbers())
    sc, out = pipeline(dev, dm, "ctcf", n, 1e-2, False, scanner_kw=kw)
    assert not sc.overlap and not (sc._reuse_flag & nv.GFM_FLAG_OVERLAP_LAUNCHES)
    assert dm.overlapped_launches() == 0
    check_against_oracle("ctcf", n, 1e-2, False, out)
    dm.close()


def test_two_scanners_on_one_handle_fall_back(dev, monkeypatch):
    """Two three-slot scanners take turns on ONE handle, both passing the flag: neither can promise anything about the
    handle's ring (the call four back was the other scanner's half the time), so every launch stays on the caller's
    stream; every batch equals the oracle."""
    from grafimo_amd.scan import KmerScanner
    monkeypatch.delenv("GRAFIMO_SCORE_OVERLAP", raising=False)
    n = SIZES[2]
    dm = fresh_motif(ctcf_numbers())
    a, b = KmerScanner(dm, n, device=dev, n_slots=3), KmerScanner(dm, n, device=dev, n_slots=3)
    assert a.overlap and b.overlap
    d = [torch.from_numpy(batch("ctcf", n, k)[0].copy()).to(dev) for k in range(2)]
    torch.cuda.synchronize(dev)
    for rnd in range(3):
        got = [(sc, k, sc.enqueue(d[k], 1e-2)) for sc, k in [(a, 0), (b, 1), (a, 1), (b, 0), (a, 0), (b, 1)]]
        for sc, k, slot in got:
            res = sc.collect(slot)
            check_against_oracle("ctcf", n, 1e-2, False, {k: (res, slot.scores[:n].cpu().numpy())})
    assert dm.overlapped_launches() == 0
    dm.close()


def test_timed_overlapped_launches_then_the_timer_goes_away(dev, monkeypatch):
    """Every launch timed (gfm_profile_enable): the timer's stop event is then also what a later call on the caller's
    stream waits for to get back in order behind the launch streams.  Turning the timer off destroys its events; the
    plain call that follows must not wait on one of them, and gives the oracle's scores and histogram."""
    monkeypatch.delenv("GRAFIMO_SCORE_OVERLAP", raising=False)
    n = SIZES[2]
    dm = fresh_motif(ctcf_numbers())
    sc, _ = pipeline(dev, dm, "ctcf", n, 1e-2, False, turns=WARM, collect_at=())
    dm.profile_enable(16, every=1)
    _, out = pipeline(dev, dm, "ctcf", n, 1e-2, False, turns=6, collect_at=(), sc=sc)
    assert dm.overlapped_launches() == WARM + 6
    ms = dm.profile_read()
    assert len(ms) == 6 and np.all(ms > 0)
    dm.profile_enable(0)
    km, exp, _, _ = batch("ctcf", n, 0)
    d_k = torch.from_numpy(km.copy()).to(dev)
    d_sc = torch.empty(n, dtype=torch.int32, device=dev)
    d_hist = torch.zeros(dm.L, dtype=torch.int64, device=dev)
    dm.score(d_k, d_sc, hist=d_hist)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_sc.cpu().numpy(), exp)
    assert np.array_equal(d_hist.cpu().numpy(), np.bincount(exp, minlength=dm.L))
    check_against_oracle("ctcf", n, 1e-2, False, out)
    dm.close()


def test_temporaries_as_kmers_under_allocator_pressure(dev, monkeypatch):
    """enqueue(torch.from_numpy(km).to(dev), ...): the caller drops its k-mer tensor at once.  The overlapped score kernel
    reads it from a stream torch's caching allocator knows nothing about, so the allocator would hand the block to the
    caller's next allocation of that size -- here a tensor of the same shape filled with 'N' right after every enqueue,
    which would turn the batch's scores into min_val.  The scanner keeps the tensor in the slot until the slot's next
    batch: no such allocation gets a block whose batch is still in the slot ring, and every batch equals the oracle."""
    monkeypatch.delenv("GRAFIMO_SCORE_OVERLAP", raising=False)
    n = SIZES[3]
    dm = fresh_motif(ctcf_numbers())
    sc, _ = pipeline(dev, dm, "ctcf", n, 1e-2, False, turns=WARM, collect_at=())
    kms = [batch("ctcf", n, b)[0] for b in range(2)]
    torch.cuda.synchronize(dev)
    slots, out = {}, {}
    for t in range(TURNS):
        slots[t] = sc.enqueue(torch.from_numpy(kms[t % 2].copy()).to(dev), 1e-2)
        junk = torch.full((n, 19), ord("N"), dtype=torch.uint8, device=dev)
        live = {s_.kmers.data_ptr() for s_ in sc.slots if s_.kmers is not None}
        assert len(live) == 3 and junk.data_ptr() not in live, t
        del junk
        if t in (4, 8):
            out[t - 2] = (sc.collect(slots[t - 2]), slots[t - 2].scores[:n].cpu().numpy())
    for t in range(TURNS - 3, TURNS):
        out[t] = (sc.collect(slots[t]), slots[t].scores[:n].cpu().numpy())
    assert dm.overlapped_launches() >= WARM                     # (the fill may leave the caller's stream busy at the next enqueue: those kernels wait for it)
    check_against_oracle("ctcf", n, 1e-2, False, out)
    dm.close()
