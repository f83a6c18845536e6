"""What the per-haplotype affinity matrix costs on the bench's graph, beside the best-score matrix whose enumeration it shares:
synth.make_graph_index(10 000, 19) (5 096 haplotypes, a site every 32 bases) with CTCF planted in 2 % of the regions as
bench.py's config 4 plants its motif.  Times, with wall clocks, the whole compute_haplotype_affinity call; with a hipEvent
pair, gfm_graph_haplotype_affinity alone and, in the same process, gfm_graph_haplotype_scores alone; the device-to-host copy
of the [R, H + 1] sums; and the TSV write (--tsv: its np.unique over 51 M cells takes a while).  Checks that with the 0/1
table w[s] = (s >= the integer cutoff of -t 1e-4) the sums equal compute_haplotype_hits' counts in all cells.  The kernels'
own times: run it under `rocprofv3 --kernel-trace --stats`.

    python scripts/haplotype_affinity_probe.py [--reps 5] [--tsv] [--out profiles/haplotype_affinity_probe.txt]
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
    threshold, noreverse, recomb, noqvalue, qvalueT = 1e-4, False, False, True, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tsv", action="store_true")
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
    from grafimo_amd.haplotype_affinity import compute_haplotype_affinity, default_weights, write_haplotype_affinity
    from grafimo_amd.haplotype_hits import compute_haplotype_hits
    from grafimo_amd.motif_ops import build_motif_meme_host

    motif = build_motif_meme_host(os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]
    probs = np.asarray(motif.count_matrix, dtype=np.float64)
    idx, regions = synth.make_graph_index(10_000, 19, plant=(probs, 0.02))
    dg = DeviceGraph(idx)
    reg = np.asarray(regions, dtype=np.int64)
    starts, stops = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    R, H = len(regions), int(idx.n_haplotypes)
    lines = [f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {H} haplotypes, {R} regions, W = 19, CTCF planted in 2 % of "
             f"the regions, both strands; {torch.cuda.get_device_name(0)}"]
    call, aff, best, d2h = [], [], [], []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dm = DeviceMotif.lease(motif)
    vp = ctypes.c_void_p
    w, s_best = default_weights(dm)
    d_w = torch.from_numpy(w.view(np.int64)).to(dg.device)
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ha = compute_haplotype_affinity(motif, dg, reg, False, _Args())
        t_call = time.perf_counter() - t
        # the device call alone, and the best-score call beside it
        sums = torch.zeros((R, H + 1), dtype=torch.int64, device=dg.device)
        keys = torch.zeros((R, H + 1), dtype=torch.int64, device=dg.device)
        over = torch.zeros(1, dtype=torch.int32, device=dg.device)
        torch.cuda.synchronize()
        ev0.record()
        nv.check(nv.lib().gfm_graph_haplotype_affinity(dg._h, (vp * 1)(dm.handle), 1, (vp * 1)(d_w.data_ptr()), int(w.max()), R,
                                                       nv.ptr(starts), nv.ptr(stops), 0, (vp * 1)(sums.data_ptr()),
                                                       over.data_ptr(), 0, 0, _stream_ptr(None)))
        ev1.record()
        torch.cuda.synchronize()
        t_aff = ev0.elapsed_time(ev1)
        ev0.record()
        nv.check(nv.lib().gfm_graph_haplotype_scores(dg._h, (vp * 1)(dm.handle), 1, R, nv.ptr(starts), nv.ptr(stops), 0,
                                                     (vp * 1)(keys.data_ptr()), over.data_ptr(), 0, 0, _stream_ptr(None)))
        ev1.record()
        torch.cuda.synchronize()
        t_best = ev0.elapsed_time(ev1)
        t = time.perf_counter()
        s_h = sums.cpu().numpy().view(np.uint64)
        t_d2h = time.perf_counter() - t
        assert int(over.item()) == 0 and (s_h == ha.full).all()
        if rep:
            call.append(t_call * 1e3), aff.append(t_aff), best.append(t_best), d2h.append(t_d2h * 1e3)
    # the 0/1 table: the sums are the hit matrix's counts
    cutoff = dm.pvalue_cutoff(_Args.threshold)
    with contextlib.redirect_stdout(io.StringIO()):
        hh = compute_haplotype_hits(motif, dg, reg, False, _Args())
    zo = compute_haplotype_affinity(motif, dg, reg, False, _Args(), weights=(np.arange(dm.L) >= cutoff).astype(np.uint64))
    same = bool((zo.sums == hh.counts.astype(np.uint64)).all())
    dm.release()
    med = statistics.median
    lines.append(f"default weights: s_best = {s_best} of L - 1 = {dm.L - 1}, largest sum {int(ha.full.max())} "
                 f"(2^{np.log2(float(ha.full.max())):.1f}), cells with sum 0: {int((ha.full == 0).sum())}")
    lines.append(f"0/1 table at the cutoff of -t {_Args.threshold} ({cutoff}): sums == compute_haplotype_hits counts in all "
                 f"{R * H} cells: {same} ({int(hh.counts.sum())} counted rows)")
    lines.append(f"compute_haplotype_affinity, whole call, wall: median {med(call):.1f} ms (min {min(call):.1f}, {a.reps} reps)")
    lines.append(f"gfm_graph_haplotype_affinity alone (run list, upload, kernel), event-timed: median {med(aff):.3f} ms "
                 f"(min {min(aff):.3f})")
    lines.append(f"gfm_graph_haplotype_scores alone, same process, event-timed: median {med(best):.3f} ms (min {min(best):.3f}); "
                 f"affinity / best score = {med(aff) / med(best):.2f}")
    lines.append(f"device -> host copy of the sums ({8 * R * (H + 1) / 1e6:.0f} MB, pageable): median {med(d2h):.1f} ms "
                 f"({8 * R * (H + 1) / 1e6 / med(d2h):.1f} GB/s)")
    if a.tsv:
        tmp = tempfile.mkdtemp()

        class _Out:
            outdir = tmp

        t = time.perf_counter()
        path = write_haplotype_affinity(ha, motif, 1, _Out())
        lines.append(f"TSV write ({os.path.getsize(path) / 1e6:.1f} MB, {len(ha._by_sum()[0])} distinct sums): "
                     f"{(time.perf_counter() - t) * 1e3:.0f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    assert same


if __name__ == "__main__":
    main()
