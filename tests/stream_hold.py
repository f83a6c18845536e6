"""Hold a stream back with ordinary work, so that a test of stream ordering can fail: `hold(stream, plan)` enqueues a
chain of in-place adds on a tensor of its own and returns an event recorded behind the chain.  Whatever is enqueued on
that stream afterwards starts only when the chain has run, while the other streams run ahead.  A missing wait between
the streams then shows as wrong numbers, every time, instead of passing because the kernels are short.

The chain's length is measured, not fixed: `calibrate` times one link and one step of the caller (events on the device
at hand; for the step the larger of the wall-clock and the event time) and sizes the chain to STEPS_PER_HOLD steps --
the hold must outlast the host side of two or three enqueues with certainty -- and to MAX_HOLD_S at the most, so that a
test of a few holds stays within seconds.  The sizing is not trusted either: a test asserts, through `still_held`,
that the hold it relies on had not drained when the enqueue it was meant to overtake began."""
import math
import time

STEPS_PER_HOLD = 100
MAX_HOLD_S = 0.25
LINK_ELEMS = 1 << 25        # float32: one link reads and writes 128 MiB, long against the host's cost of enqueuing it


class HoldPlan:
    def __init__(self, buf, link_s, step_s, n_links):
        self.buf, self.link_s, self.step_s, self.n_links = buf, link_s, step_s, n_links

    @property
    def hold_s(self):
        return self.n_links * self.link_s

    def __str__(self):
        return (f"chain link {self.link_s * 1e6:.1f} us, step {self.step_s * 1e6:.1f} us -> {self.n_links} links, "
                f"hold {self.hold_s * 1e3:.2f} ms")


def calibrate(torch, device, step, n_steps: int = 12, n_links: int = 50) -> HoldPlan:
    """`step()`: one enqueue + score kernel of the test's batch size, on the current stream of `device`."""
    buf = torch.zeros(LINK_ELEMS, dtype=torch.float32, device=device)
    main = torch.cuda.current_stream(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        buf.add_(1.0)
    torch.cuda.synchronize(device)
    e0.record(main)
    for _ in range(n_links):
        buf.add_(1.0)
    e1.record(main)
    torch.cuda.synchronize(device)
    link_s = e0.elapsed_time(e1) * 1e-3 / n_links
    for _ in range(n_steps):
        step()
    torch.cuda.synchronize(device)
    e0.record(main)
    t0 = time.perf_counter()
    for _ in range(n_steps):
        step()
    wall_s = (time.perf_counter() - t0) / n_steps
    e1.record(main)
    torch.cuda.synchronize(device)
    step_s = max(wall_s, e0.elapsed_time(e1) * 1e-3 / n_steps)
    want = math.ceil(STEPS_PER_HOLD * step_s / link_s)
    return HoldPlan(buf, link_s, step_s, max(1, min(want, int(MAX_HOLD_S / link_s))))


def hold(torch, stream, plan: HoldPlan):
    """Enqueue the chain on `stream`; returns the event behind it."""
    end = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for _ in range(plan.n_links):
            plan.buf.add_(1.0)
        end.record(stream)
    return end


def still_held(end) -> bool:
    """The precondition of a test that relies on `end`'s hold: the chain has not run out yet."""
    return not end.query()
