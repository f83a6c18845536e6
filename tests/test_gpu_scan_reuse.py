"""Buffer reuse of KmerScanner and SameWidthScanner with the tail stream held back (stream_hold.py): the score kernel
of a batch goes to the main stream, its tail (post kernel, all-reduce, q-table, selection, per-region best hit, gather) to
a side stream, and slots -- optionally a shorter ring of score arrays -- are reused while older tails are still
outstanding.  A hold in front of every tail keeps them outstanding for as long as the host needs to enqueue the next
batches, so a missing or misdirected wait yields a foreign batch's numbers in a slot instead of passing because the
kernels are short.  Every batch is distinct; every compared quantity comes from the oracle.

Shape of a run: holds are armed in front of every enqueue of the last two laps; the last n_slots turns are collected
and compared once all of them are enqueued.  The checked turns start half a lap into the slot ring (a lap and a half of
turns come first), so that they straddle the ring's wrap-around: that is where score arrays bound to SLOTS leave the
t - score_buffers spacing, and a reader has to be among the checked turns for its damage to be seen.

The batches: 60 000 - 7 b rows of random ACGT with 40 N each, as in test_scanner_slot_rings_under_pipelining, plus 300
rows drawn from the motif at random places.  Random rows alone never reach q < 0.3 (their smallest q-value is 0.5 - 0.96
by the oracle), and the hit lists of a q-value threshold, which is what the selection cases compare, would all be empty."""
import datetime
import socket
from types import SimpleNamespace

import numpy as np
import pytest

import stream_hold
from test_gpu_top_hits import _np_region_best

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 60_000
N_REG = 300
N_BATCHES = 20          # the longest run: 8 slots -> 12 + 8 turns
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def world(golden_motifs):
    from oracle import oracle as orc
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _, flat = golden_motifs
    g = flat["ctcf_meme_unif#0"]
    dev = torch.device("cuda:0")
    ptab = orc.p_table(g["pmf"])
    rng = np.random.default_rng(5)
    cdf = np.cumsum(g["probs"] / g["probs"].sum(0, keepdims=True), axis=0)          # [4, W]
    batches, exp = [], []
    for b in range(N_BATCHES):
        km = rng.choice(ACGT, size=(N - 7 * b, 19))
        km[rng.integers(0, len(km), 40), rng.integers(0, 19, 40)] = ord("N")
        u = rng.random((300, 19))
        km[rng.choice(len(km), 300, replace=False)] = ACGT[np.minimum((u[:, None, :] > cdf[None]).sum(1), 3)]
        sc, p = orc.score_kmers_table(km, g["score_matrix"], ptab, g["min_val"])
        batches.append(km)
        exp.append(SimpleNamespace(scores=sc, p=p, q=orc.fdr_bh(p)))
    region = (np.arange(N) * N_REG // N).astype(np.int32)
    freq = rng.integers(0, 5, N).astype(np.int64)                                   # a fifth of the rows: freq == 0
    return SimpleNamespace(g=g, dev=dev, batches=batches, exp=exp, region=region, freq=freq,
                           d_batches=[torch.from_numpy(k).to(dev) for k in batches],
                           d_region=torch.from_numpy(region).to(dev), d_freq=torch.from_numpy(freq).to(dev))


def _motif(g):
    from grafimo_amd.device import DeviceMotif
    return DeviceMotif(g["score_matrix"], g["bg"], g["min_val"], g["scale"], g["offset"], g["pmf"])


@pytest.fixture(scope="module")
def plan(world):
    """The hold's length for this device and this batch size, measured once (stream_hold.calibrate)."""
    from grafimo_amd.scan import KmerScanner
    dm = _motif(world.g)
    sc = KmerScanner(dm, N, device=world.dev, n_slots=3)
    turn = iter(range(1 << 30))
    p = stream_hold.calibrate(torch, world.dev, lambda: sc.enqueue(world.d_batches[next(turn) % N_BATCHES], 1e-2))
    sc.finish()
    torch.cuda.synchronize(world.dev)
    dm.close()
    print(f"\nstream_hold on {torch.cuda.get_device_name(0)}: {p}")
    assert p.hold_s <= stream_hold.MAX_HOLD_S
    return p


def _check(world, b, thr, on_q, res, regions=False, hits=True):
    """One collected batch against the oracle: rows, scaled scores, n_scored and best-hit keys exactly; the q-table at
    every score the batch holds (a histogram that counted two batches moves all of it)."""
    from grafimo_amd import top_hits as th
    e = world.exp[b]
    n = len(world.batches[b])
    keep = (e.q if on_q else e.p) < thr
    what = (b, thr, on_q)
    assert res["n_scored"] == n, what
    np.testing.assert_allclose(res["qtable"][e.scores], e.q, rtol=1e-12, atol=0, err_msg=str(what))
    if hits:
        rows = np.nonzero(keep)[0]
        assert len(rows) > 100, what
        assert np.array_equal(res["rows"], rows), what
        assert np.array_equal(res["scaled"], e.scores[rows]), what
    if regions:
        es, er = _np_region_best(e.scores, world.region[:n], N_REG, keep=keep & (world.freq[:n] > 0))
        s_, r_, ok = th.decode_best(res["best"])
        assert (es >= 0).sum() > N_REG // 4, what
        assert np.array_equal(s_, es) and np.array_equal(r_, er) and np.array_equal(ok, es >= 0), what


def _held_run(world, plan, sc, thresholds, hits=True, regions=False, **enqueue_kw):
    """A lap and a half of turns, then the checked lap; a hold on the tail stream in front of every enqueue of the last
    two laps.  Turn t scans batch t under thresholds[t % len].  Returns turn -> address of the score array it wrote."""
    n_slots = len(sc.slots)
    first = n_slots + n_slots // 2
    slots, wrote, prev = {}, {}, None
    for t in range(first + n_slots):
        h = stream_hold.hold(torch, sc.side, plan) if t >= first - n_slots else None
        # the precondition, not the sizing, is what the test rests on: the tail of turn t - 1 is still behind its hold now
        assert prev is None or stream_hold.still_held(prev), f"the hold of turn {t - 1} drained before turn {t} was enqueued"
        thr, on_q = thresholds[t % len(thresholds)]
        slots[t] = sc.enqueue(world.d_batches[t], thr, on_qvalue=on_q, **enqueue_kw)
        wrote[t] = slots[t].scores.data_ptr()
        prev = h
    for t in range(first, first + n_slots):
        thr, on_q = thresholds[t % len(thresholds)]
        _check(world, t, thr, on_q, sc.collect(slots[t]), regions=regions, hits=hits)
    return {t: wrote[t] for t in range(first, first + n_slots)}


@pytest.mark.parametrize("n_slots,ring", [(4, 3), (8, 3), (3, 2), (5, 2), (6, 2), (4, 2)])
def test_score_ring_with_region_best_reading_held_scores(world, plan, n_slots, ring):
    """gfm_region_best of a held tail reads the batch's scores while later score kernels run: the best-hit keys of every
    checked turn are its own.  p-value thresholds: no selection kernel reads the scores, the regions alone do."""
    from grafimo_amd.scan import KmerScanner
    dm = _motif(world.g)
    sc = KmerScanner(dm, N, device=world.dev, n_slots=n_slots, score_buffers=ring)
    sc.set_regions(world.d_region, N_REG, freq=world.d_freq)
    wrote = _held_run(world, plan, sc, [(1e-2, False), (1e-3, False)], regions=True)
    assert len(set(wrote.values())) < len(wrote), "no score array was rewritten inside the checked lap"
    dm.close()


@pytest.mark.parametrize("candidates,cap", [(False, None), (True, 2000)])
@pytest.mark.parametrize("n_slots,ring", [(4, 3), (8, 3)])
def test_score_ring_with_selection_reading_held_scores(world, plan, n_slots, ring, candidates, cap):
    """A q-value batch, whose held selection reads every score (gfm_select_hits; gfm_select_hits_from after its
    candidate list overflowed: 2000 entries for some 18 000 rows with p < 0.3, enough for the ~420 hits), followed on
    the same array by a p-value batch, whose own tail reads nothing: the reader is the EARLIER batch."""
    from grafimo_amd.scan import KmerScanner
    dm = _motif(world.g)
    sc = KmerScanner(dm, N, hit_capacity=cap, device=world.dev, n_slots=n_slots, score_buffers=ring, candidates=candidates)
    wrote = _held_run(world, plan, sc, [(1e-2, False), (0.3, True)])
    assert len(set(wrote.values())) < len(wrote)
    dm.close()


@pytest.mark.parametrize("n_slots,ring", [(4, 3), (8, 3), (3, 2)])
def test_scores_stay_valid_for_ring_minus_one_enqueues(world, n_slots, ring):
    """The documented lifetime: after turn t and score_buffers - 1 further enqueues, slot.scores of turn t are still its
    own, for every turn of two laps."""
    from grafimo_amd.scan import KmerScanner
    dm = _motif(world.g)
    sc = KmerScanner(dm, N, device=world.dev, n_slots=n_slots, score_buffers=ring)
    slots = []
    for u in range(2 * n_slots + ring - 1):
        slots.append(sc.enqueue(world.d_batches[u], 1e-2))
        t = u - (ring - 1)
        if t >= 0:
            torch.cuda.synchronize(world.dev)
            n = len(world.batches[t])
            assert np.array_equal(slots[t].scores[:n].cpu().numpy(), world.exp[t].scores), (t, u)
    dm.close()


@pytest.mark.parametrize("n_slots", [2, 3, 5])
def test_slot_reuse_with_tails_in_flight(world, plan, n_slots):
    """One score array per slot; the slot of turn t - n_slots is taken again while its tail is held.  Two slots: the
    device orders the reuse; three: the host paces it and the library is told the caller orders its workspace ring; five:
    more than that ring, which the library then orders itself.  Threshold 1.0 makes every wave flush its hit queue."""
    from grafimo_amd import _native as nv
    from grafimo_amd.scan import KmerScanner
    dm = _motif(world.g)
    sc = KmerScanner(dm, N, device=world.dev, n_slots=n_slots)
    assert sc.host_paced == (n_slots >= 3)
    assert bool(sc._reuse_flag) == (n_slots <= nv.GFM_WORKSPACE_RING)
    _held_run(world, plan, sc, [(1.0, False), (1e-2, False), (0.3, True), (1e-3, False), (0.5, True)])
    dm.close()


def test_gather_stream_behind_a_held_tail(world, plan):
    """One-rank RCCL group, the hit gather on its own stream: `done` is recorded on the gather stream, behind the held
    tail.  Once gathering the per-region keys (top_only), once the hit entries."""
    import torch.distributed as dist
    from grafimo_amd.scan import KmerScanner
    started = False
    if not dist.is_initialized():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        torch.cuda.set_device(world.dev)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                device_id=world.dev, timeout=datetime.timedelta(seconds=60))
        started = True
    dm = _motif(world.g)
    try:
        thresholds = [(1e-2, False), (0.3, True), (1e-3, False), (0.5, True)]
        for top_only in (True, False):
            sc = KmerScanner(dm, N, device=world.dev, n_slots=3, side_stream=True, always_collective=True)
            assert sc._gather_stream is not None
            if top_only:
                sc.set_regions(world.d_region, N_REG, freq=world.d_freq, top_only=True)
            _held_run(world, plan, sc, thresholds, hits=not top_only, regions=top_only, gather_hits=True)
            assert all(s_.gathered is not None for s_ in sc.slots)
    finally:
        torch.cuda.synchronize(world.dev)
        if started:
            dist.destroy_process_group()
        dm.close()


@pytest.mark.parametrize("thr,on_q", [(1e-2, False), (0.3, True)])
def test_same_width_scanner_second_enqueue_behind_a_held_tail(world, plan, golden_motifs, thr, on_q):
    """SameWidthScanner(side_stream=True) has ONE set of buffers: the score kernels of the second enqueue must wait for
    the first one's held tail.  The second batch's rows, scores and q-tables are its own, its histograms not the sum."""
    from grafimo_amd.scan import SameWidthScanner
    from oracle import oracle as orc
    _, flat = golden_motifs
    gs = [flat[k] for k in ("ctcf_meme_unif#0", "ctcf_meme_bgnt#0")]
    assert all(g["width"] == 19 for g in gs)
    dms = [_motif(g) for g in gs]
    sw = SameWidthScanner(dms, N, N, world.dev, side_stream=True)
    h = stream_hold.hold(torch, sw.side, plan)
    sw.enqueue(world.d_batches[0], thr, on_qvalue=on_q)
    assert stream_hold.still_held(h), "the hold drained before the second enqueue"
    sw.enqueue(world.d_batches[1], thr, on_qvalue=on_q)
    sw.finish()
    torch.cuda.synchronize(world.dev)
    km = world.batches[1]
    for j, g in enumerate(gs):
        sc, p = orc.score_kmers_table(km, g["score_matrix"], orc.p_table(g["pmf"]), g["min_val"])
        q = orc.fdr_bh(p)
        rows = np.nonzero((q if on_q else p) < thr)[0]
        assert len(rows) > 100
        assert np.array_equal(sw.scores[j][:len(km)].cpu().numpy(), sc), j
        assert int(sw.nrows[j].item()) == len(km), j
        np.testing.assert_allclose(sw.qtable[j].cpu().numpy()[sc], q, rtol=1e-12, atol=0)
        k = int(sw.hits[j, 0].item())
        packed = np.sort(sw.hits[j, 1:1 + k].cpu().numpy())
        assert np.array_equal(packed >> 20, rows) and np.array_equal(packed & 0xFFFFF, sc[rows]), j
    for dm in dms:
        dm.close()
