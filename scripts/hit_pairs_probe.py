"""What gfm_hit_pairs (grafimo_amd/csrc/hit_pairs.hip) does per second, on a synthetic input stated here.

Input (seeded): ROWS rows in regions of ROWS_PER_REGION rows; a row's lo uniform in [0, SPAN), its length 8 .. 20; its
carrier set the AND of k random bitsets, k = 1 .. 6 per row (a carrier frequency of 1/2 .. 1/64: common and rare rows), the
bits beyond H clear.  The gap is (0, MAX_GAP).  Run at H = 5 096 (80 words) and at H = 64 (one word).

Timed with device events after a warm-up, REPS repetitions each, median and (min .. max) printed:
  count   the counting pass alone: gfm_hit_pairs with pair capacity 0 (order check, count kernel, exclusive sum)
  fill    the writing pass alone: gfm_hit_pairs with GFM_PAIRS_HAVE_OFFSETS and room
per pass: candidates/s (rows behind a in its region with lo_b - hi_a <= MAX_GAP: what the kernel walks), pairs/s, and the
bitset bytes intersected per second (candidates that pass the full gap test x 2 bitsets x hw x 8 bytes).  The same for
the O(n^2) numpy reference of tests/hit_pair_bruteforce.py on the first SLICE_REGIONS regions: that is the baseline, not
the code under test; on the slice the two results are compared.

    python scripts/hit_pairs_probe.py [--rows 200000] [--rows-per-region 300] [--max-gap 400] [--reps 7]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPAN = 3000


def make_rows(torch, rows, per_region, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    hw = (H + 63) // 64
    group = (torch.arange(rows, device="cuda") // per_region).to(torch.int32)
    lo = torch.randint(0, SPAN, (rows,), generator=g, device="cuda", dtype=torch.int64)
    hi = lo + torch.randint(8, 21, (rows,), generator=g, device="cuda", dtype=torch.int64)
    key = (group.to(torch.int64) * (4 * SPAN) + lo) * 32 + (hi - lo)      # ascending (group, lo, hi): the reference's order too
    order = torch.argsort(key, stable=True)
    lo, hi = lo[order].contiguous(), hi[order].contiguous()
    k = torch.randint(1, 7, (rows, 1), generator=g, device="cuda")
    masks = torch.full((rows, hw), -1, dtype=torch.int64, device="cuda")
    for step in range(6):
        word = (torch.randint(0, 2 ** 32, (rows, hw), generator=g, device="cuda", dtype=torch.int64) << 32) | \
            torch.randint(0, 2 ** 32, (rows, hw), generator=g, device="cuda", dtype=torch.int64)
        masks = torch.where(k > step, masks & word, masks)
    if H & 63:
        masks[:, -1] &= (1 << (H & 63)) - 1
    return group, lo, hi, masks.contiguous()


def candidates(group, lo, hi, max_gap):
    """rows behind a in its group with lo_b - hi_a <= max_gap, summed over a (host, from the sorted arrays)"""
    base = group.astype(np.int64) * (8 * SPAN + 8 * max_gap)
    end = np.searchsorted(base + lo, base + hi + max_gap, side="right")
    return int((end - np.arange(len(lo)) - 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--rows-per-region", type=int, default=300)
    ap.add_argument("--max-gap", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slice-regions", type=int, default=4)
    a = ap.parse_args()
    import torch
    from grafimo_amd import _native as nv
    from hit_pair_bruteforce import pairs_reference
    assert torch.cuda.is_available(), "the probe measures the GPU: there is no fallback"
    lib = nv.lib()
    out = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "rows_per_region": a.rows_per_region, "gap": [0, a.max_gap],
           "reps": a.reps, "runs": []}
    for H in (5096, 64):
        hw = (H + 63) // 64
        group, lo, hi, masks = make_rows(torch, a.rows, a.rows_per_region, H, 1234 + H)
        n = a.rows
        h_group, h_lo, h_hi = group.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
        n_cand = candidates(h_group, h_lo, h_hi, a.max_gap)
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        total = ctypes.c_int64()
        sp = torch.cuda.current_stream().cuda_stream

        def call(cap, b, joint, flags):
            nv.check(lib.gfm_hit_pairs(group.data_ptr(), lo.data_ptr(), hi.data_ptr(), masks.data_ptr(), n, hw, 0, a.max_gap, 0, None,
                                       off.data_ptr(), cap, b.data_ptr() if b is not None else None,
                                       joint.data_ptr() if joint is not None else None, None, flags, ctypes.byref(total), sp))

        call(0, None, None, 0)                                            # warm-up, and the total
        P = int(total.value)
        b = torch.empty(max(P, 1), dtype=torch.int32, device="cuda")
        joint = torch.empty(max(P, 1), dtype=torch.int32, device="cuda")
        call(P, b, joint, nv.GFM_PAIRS_HAVE_OFFSETS)
        torch.cuda.synchronize()
        # candidates that pass the full gap test (their bitsets are read): from the offsets of a run whose masks are all ones
        ones = torch.ones((n, 1), dtype=torch.int64, device="cuda")
        off1 = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        t1 = ctypes.c_int64()
        nv.check(lib.gfm_hit_pairs(group.data_ptr(), lo.data_ptr(), hi.data_ptr(), ones.data_ptr(), n, 1, 0, a.max_gap, 0, None,
                                   off1.data_ptr(), 0, None, None, None, 0, ctypes.byref(t1), sp))
        tested = int(t1.value)
        times = {"count": [], "fill": []}
        for _ in range(a.reps):
            for what in ("count", "fill"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if what == "count":
                    call(0, None, None, 0)
                else:
                    call(P, b, joint, nv.GFM_PAIRS_HAVE_OFFSETS)
                e1.record()
                torch.cuda.synchronize()
                times[what].append(e0.elapsed_time(e1) * 1e-3)
        run = {"H": H, "hw": hw, "candidates": n_cand, "gap_tested": tested, "pairs": P}
        for what, ts in times.items():
            med = float(np.median(ts))
            run[what] = {"median_s": med, "min_s": min(ts), "max_s": max(ts), "candidates_per_s": n_cand / med,
                         "pairs_per_s": P / med, "bitset_bytes_per_s": tested * 2 * hw * 8 / med}
        # the numpy reference on a slice, and the comparison there
        m = min(n, a.slice_regions * a.rows_per_region)
        s_masks = masks[:m].cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        ra, rb, rj, _ = pairs_reference(h_group[:m], h_lo[:m], h_hi[:m], s_masks, 0, a.max_gap)
        dt = time.perf_counter() - t0
        h_off = off.cpu().numpy()
        k = int(h_off[m])
        assert np.array_equal(np.repeat(np.arange(m), np.diff(h_off[:m + 1])), ra), "the slice differs from the reference"
        assert np.array_equal(b[:k].cpu().numpy(), rb) and np.array_equal(joint[:k].cpu().numpy(), rj)
        s_cand = candidates(h_group[:m], h_lo[:m], h_hi[:m], a.max_gap)
        run["numpy_reference_slice"] = {"rows": m, "pairs": len(ra), "seconds": dt, "candidates_per_s": s_cand / dt,
                                        "pairs_per_s": len(ra) / dt}          # (it intersects every later row of the slice)
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))


if __name__ == "__main__":
    main()
