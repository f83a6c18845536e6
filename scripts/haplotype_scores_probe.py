"""What the per-haplotype best score matrix costs on the bench's graph: synth.make_graph_index(10 000, 19) (5 096 haplotypes, a
site every 32 bases) with CTCF planted in 2 % of the regions as bench.py's config 4 plants its motif.  Times, with wall
clocks, the whole compute_haplotype_scores call; with a hipEvent pair, gfm_graph_haplotype_scores alone; the device-to-host
copy of the [R, H + 1] keys; and the TSV write.  Beside it, the route that gives the same `best` without this call:
compute_haplotype_hits at threshold 1 (the report's fused pass with a hit list of every row, then gfm_graph_haplotype_hits),
whole call wall-clocked and gfm_graph_haplotype_hits event-timed on the entries it left; the two `best` matrices are
compared.  The kernels' own times: run it under `rocprofv3 --kernel-trace --stats`.

    python scripts/haplotype_scores_probe.py [--reps 5] [--out profiles/haplotype_scores_probe.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Args:
    threshold, noreverse, recomb, noqvalue, qvalueT = 1.0, False, False, True, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import contextlib
    import io
    import numpy as np
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import DeviceGraph, _stream_ptr
    from grafimo_amd.haplotype_hits import compute_haplotype_hits
    from grafimo_amd.haplotype_scores import compute_haplotype_scores, write_haplotype_scores
    from grafimo_amd.motif_ops import build_motif_meme_host

    motif = build_motif_meme_host(os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]
    probs = np.asarray(motif.count_matrix, dtype=np.float64)
    idx, regions = synth.make_graph_index(10_000, 19, plant=(probs, 0.02))
    dg = DeviceGraph(idx)
    reg = np.asarray(regions, dtype=np.int64)
    starts, stops = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    R, H = len(regions), int(idx.n_haplotypes)
    lines = [f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {H} haplotypes, {R} regions, W = 19, CTCF planted in 2 % of "
             f"the regions, both strands, no threshold; {torch.cuda.get_device_name(0)}"]
    sink = io.StringIO()
    call, kern, d2h, tsv, hcall, hkern = [], [], [], [], [], []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tmp = tempfile.mkdtemp()

    class _Out:
        outdir = tmp

    dm = DeviceMotif.lease(motif)
    vp = ctypes.c_void_p
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        hs = compute_haplotype_scores(motif, dg, reg, False, _Args())
        t_call = time.perf_counter() - t
        # the device call alone
        keys = torch.zeros((R, H + 1), dtype=torch.int64, device=dg.device)
        over = torch.zeros(1, dtype=torch.int32, device=dg.device)
        torch.cuda.synchronize()
        ev0.record()
        nv.check(nv.lib().gfm_graph_haplotype_scores(dg._h, (vp * 1)(dm.handle), 1, R, nv.ptr(starts), nv.ptr(stops), 0,
                                                     (vp * 1)(keys.data_ptr()), over.data_ptr(), 0, 0, _stream_ptr(None)))
        ev1.record()
        torch.cuda.synchronize()
        t_kern = ev0.elapsed_time(ev1) * 1e3
        t = time.perf_counter()
        k_h = keys.cpu().numpy().view(np.uint64)
        t_d2h = time.perf_counter() - t
        assert int(over.item()) == 0 and (k_h == hs.keys).all()
        t = time.perf_counter()
        path = write_haplotype_scores(hs, motif, 1, _Out())
        t_tsv = time.perf_counter() - t
        # the route of today: threshold 1 through the hit list
        with contextlib.redirect_stdout(sink):
            torch.cuda.synchronize()
            t = time.perf_counter()
            hh = compute_haplotype_hits(motif, dg, reg, False, _Args())
            t_hcall = time.perf_counter() - t
        buf, cap = dg.fused_buffers(0, 0)
        n_hits = min(int(buf[0].item()), cap)
        counts = torch.empty((R, H), dtype=torch.int32, device=dg.device)
        best = torch.empty((R, H), dtype=torch.int32, device=dg.device)
        torch.cuda.synchronize()
        ev0.record()
        nv.check(nv.lib().gfm_graph_haplotype_hits(dg._h, *dg.hit_list(0)[:2], n_hits, None, R,
                                                   counts.data_ptr(), best.data_ptr(), 0, _stream_ptr(None)))
        ev1.record()
        torch.cuda.synchronize()
        t_hkern = ev0.elapsed_time(ev1) * 1e3
        assert (hh.best == hs.best).all()
        if rep:
            call.append(t_call * 1e3), kern.append(t_kern), d2h.append(t_d2h * 1e3), tsv.append(t_tsv * 1e3)
            hcall.append(t_hcall * 1e3), hkern.append(t_hkern)
    dm.release()
    med = statistics.median
    lines.append(f"best == compute_haplotype_hits(threshold 1).best in all {R * H} cells; threshold-1 hit entries: {n_hits}; "
                 f"cells whose best beats the reference: {int((hs.best > hs.reference_best[:, None]).sum())}")
    lines.append(f"compute_haplotype_scores, whole call, wall: median {med(call):.1f} ms (min {min(call):.1f}, {a.reps} reps)")
    lines.append(f"gfm_graph_haplotype_scores alone (run list, upload, kernel), event-timed: median {med(kern) / 1e3:.3f} ms "
                 f"(min {min(kern) / 1e3:.3f})")
    lines.append(f"device -> host copy of the keys ({8 * R * (H + 1) / 1e6:.0f} MB, pageable): median {med(d2h):.1f} ms "
                 f"({8 * R * (H + 1) / 1e6 / med(d2h):.1f} GB/s)")
    lines.append(f"TSV write ({os.path.getsize(path) / 1e6:.1f} MB): median {med(tsv):.1f} ms")
    lines.append(f"threshold-1 route, compute_haplotype_hits whole call, wall: median {med(hcall):.1f} ms (min {min(hcall):.1f})")
    lines.append(f"threshold-1 route, gfm_graph_haplotype_hits alone on its {n_hits} entries, event-timed: median "
                 f"{med(hkern) / 1e3:.3f} ms (min {min(hkern) / 1e3:.3f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
