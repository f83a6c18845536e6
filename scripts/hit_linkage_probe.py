"""What gfm_hit_linkage (grafimo_amd/csrc/hit_linkage.hip) does per second, on a synthetic input stated here.

Input (seeded): SITES sites at ascending random positions of [0, SPAN), 80 % of them with one ALT, 15 % with two, 5 % with
three; an allele's carriers are random with a frequency of 1/2 .. 1/64 (the AND of 1 .. 6 random bitsets).  ROWS rows with lo
uniform in [0, SPAN), length 8 .. 20; four rows in five have random carriers of the same kind, one in five the carriers of the
first allele of the nearest site behind it (so that links exist); the bits beyond H are clear.  The defaults -- 10^5 rows,
10^5 sites on 4 * 10^6 bases, flank 10 000 -- give about 600 alleles per window.  Run at H = 5 096 (80 words) and H = 64 (one).

Timed with device events after a warm-up, REPS repetitions each, median and (min .. max) printed:
  count   the counting pass alone: gfm_hit_linkage with link capacity 0 (check, slot compaction, ranges, count kernel, sum)
  fill    the writing pass alone: gfm_hit_linkage with GFM_LINKAGE_HAVE_OFFSETS and room (the preparation runs again)
per pass: word intersections per second -- candidates (row, slot) x hw, what the main loop does --, candidates/s and links/s.
link_rows on the first SLICE_ROWS rows is compared with the numpy / Python reference of tests/hit_linkage_bruteforce.py: that
is the baseline, not the code under test.

    python scripts/hit_linkage_probe.py [--rows 100000] [--sites 100000] [--span 4000000] [--flank 10000] [--reps 5]
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


def random_sets(torch, g, n, hw, H):
    """n bitsets [n, hw] int64 of frequency 1/2 .. 1/64"""
    k = torch.randint(1, 7, (n, 1), generator=g, device="cuda")
    out = torch.full((n, hw), -1, dtype=torch.int64, device="cuda")
    for step in range(6):
        word = (torch.randint(0, 2 ** 32, (n, hw), generator=g, device="cuda", dtype=torch.int64) << 32) | \
            torch.randint(0, 2 ** 32, (n, hw), generator=g, device="cuda", dtype=torch.int64)
        out = torch.where(k > step, out & word, out)
    if H & 63:
        out[:, -1] &= (1 << (H & 63)) - 1
    return out


def make_input(torch, rows, sites, span, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    hw = (H + 63) // 64
    pos = torch.sort(torch.randint(0, span, (sites,), generator=g, device="cuda", dtype=torch.int64)).values
    u = torch.rand(sites, generator=g, device="cuda")
    n_alts = (1 + (u > 0.80).to(torch.uint8) + (u > 0.95).to(torch.uint8)).contiguous()
    bits = random_sets(torch, g, sites * 3, hw, H).view(sites, 3, hw).contiguous()
    lo = torch.sort(torch.randint(0, span, (rows,), generator=g, device="cuda", dtype=torch.int64)).values
    hi = lo + torch.randint(8, 21, (rows,), generator=g, device="cuda", dtype=torch.int64)
    masks = random_sets(torch, g, rows, hw, H)
    near = torch.clamp(torch.searchsorted(pos, lo), max=sites - 1)
    copy = torch.rand(rows, generator=g, device="cuda") < 0.2
    masks = torch.where(copy[:, None], bits[near, 0], masks).contiguous()
    return lo, hi, masks, pos, n_alts, bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--sites", type=int, default=100_000)
    ap.add_argument("--span", type=int, default=4_000_000)
    ap.add_argument("--flank", type=int, default=10_000)
    ap.add_argument("--min-r2", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slice-rows", type=int, default=48)
    a = ap.parse_args()
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd.hit_linkage import link_rows
    from hit_linkage_bruteforce import links_reference
    assert torch.cuda.is_available(), "the probe measures the GPU: there is no fallback"
    lib = nv.lib()
    out = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "sites": a.sites, "span": a.span, "flank": a.flank,
           "min_r2": a.min_r2, "reps": a.reps}
    for H in (5096, 64):
        hw = (H + 63) // 64
        lo, hi, masks, pos, n_alts, bits = make_input(torch, a.rows, a.sites, a.span, H, 4321 + H)
        n, S = a.rows, a.sites
        h_lo, h_hi, h_pos, h_alts = lo.cpu().numpy(), hi.cpu().numpy(), pos.cpu().numpy(), n_alts.cpu().numpy()
        slot_base = np.concatenate([[0], np.cumsum(h_alts.astype(np.int64))])
        first = np.searchsorted(h_pos, h_lo - a.flank, side="left")
        last = np.maximum(np.searchsorted(h_pos, h_hi - 1 + a.flank, side="right"), first)
        n_cand = int((slot_base[last] - slot_base[first]).sum())
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        n_hit = torch.empty(n, dtype=torch.int32, device="cuda")
        n_allele = torch.empty((S, 3), dtype=torch.int32, device="cuda")
        total = ctypes.c_int64()
        sp = torch.cuda.current_stream().cuda_stream

        def call(cap, site, allele, joint, flags):
            p = lambda x: x.data_ptr() if x is not None else None      # noqa: E731
            nv.check(lib.gfm_hit_linkage(lo.data_ptr(), hi.data_ptr(), masks.data_ptr(), n, pos.data_ptr(), n_alts.data_ptr(),
                                         bits.data_ptr(), S, hw, H, a.flank, a.min_r2, off.data_ptr(), cap, p(site), p(allele), p(joint),
                                         n_hit.data_ptr(), n_allele.data_ptr(), 0, 0, flags, ctypes.byref(total), sp))

        call(0, None, None, None, 0)                                      # warm-up, and the total
        L = int(total.value)
        site = torch.empty(max(L, 1), dtype=torch.int32, device="cuda")
        allele = torch.empty(max(L, 1), dtype=torch.uint8, device="cuda")
        joint = torch.empty(max(L, 1), dtype=torch.int32, device="cuda")
        call(L, site, allele, joint, nv.GFM_LINKAGE_HAVE_OFFSETS)
        torch.cuda.synchronize()
        times = {"count": [], "fill": []}
        for _ in range(a.reps):
            for what in ("count", "fill"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if what == "count":
                    call(0, None, None, None, 0)
                else:
                    call(L, site, allele, joint, nv.GFM_LINKAGE_HAVE_OFFSETS)
                e1.record()
                torch.cuda.synchronize()
                times[what].append(e0.elapsed_time(e1) * 1e-3)
        run = {"H": H, "hw": hw, "candidates": n_cand, "word_intersections": n_cand * hw, "device_links": L}
        for what, ts in times.items():
            med = float(np.median(ts))
            run[what] = {"median_s": med, "min_s": min(ts), "max_s": max(ts), "word_intersections_per_s": n_cand * hw / med,
                         "candidates_per_s": n_cand / med, "links_per_s": L / med}
        # the reference on a slice, and the comparison there (the sites the slice can reach)
        m = min(n, a.slice_rows)
        s0, s1 = int(first[:m].min()), int(last[:m].max())
        s_masks = masks[:m].cpu().numpy().view(np.uint64)
        s_bits = bits[s0:s1].cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        exp = links_reference(h_lo[:m], h_hi[:m], s_masks, h_pos[s0:s1], h_alts[s0:s1], s_bits, a.flank, a.min_r2, H)
        dt = time.perf_counter() - t0
        got = link_rows(h_lo[:m], h_hi[:m], s_masks, h_pos[s0:s1], h_alts[s0:s1], s_bits, a.flank, a.min_r2, H)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e), "the slice differs from the reference"
        run["reference_slice"] = {"rows": m, "links": len(exp[0]), "candidates": exp[9], "seconds": dt,
                                  "word_intersections_per_s": exp[9] * hw / dt}
        out.setdefault("runs", []).append(run)
        print(json.dumps(run), flush=True)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))


if __name__ == "__main__":
    main()
