"""What the per-haplotype hit matrix costs on the bench's graph: synth.make_graph_index(10 000, 19) (5 096 haplotypes, a site
every 32 bases) with CTCF planted in 2 % of the regions as bench.py's config 4 plants its motif, so that p < 1e-4 reports
rows.  Times, with wall clocks, the whole compute_haplotype_hits call beside compute_results_from_graph (the report, same
arguments); with a hipEvent pair, gfm_graph_haplotype_hits alone on the entries the report's pass left; the device-to-host
copy of the two [R, H] int32 arrays; and the TSV write.  The kernels' own times: run it under
`rocprofv3 --kernel-trace --stats`.

    python scripts/haplotype_hits_probe.py [--reps 5] [--out profiles/haplotype_hits_probe.txt]
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
    threshold, noreverse, recomb, noqvalue, qvalueT = 1e-4, False, False, False, False


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
    from grafimo_amd.extract_regions import DeviceGraph, _stream_ptr, compute_results_from_graph
    from grafimo_amd.haplotype_hits import compute_haplotype_hits, write_haplotype_hits
    from grafimo_amd.motif_ops import build_motif_meme_host

    motif = build_motif_meme_host(os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]
    probs = np.asarray(motif.count_matrix, dtype=np.float64)
    idx, regions = synth.make_graph_index(10_000, 19, plant=(probs, 0.02))
    dg = DeviceGraph(idx)
    reg = np.asarray(regions, dtype=np.int64)
    R, H = len(regions), int(idx.n_haplotypes)
    lines = [f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {H} haplotypes, {R} regions, W = 19, CTCF planted in 2 % of "
             f"the regions, p < 1e-4, both strands; {torch.cuda.get_device_name(0)}"]
    sink = io.StringIO()
    call, report, kern, d2h, tsv = [], [], [], [], []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tmp = tempfile.mkdtemp()

    class _Out:
        outdir = tmp

    for rep in range(a.reps + 1):
        with contextlib.redirect_stdout(sink):
            torch.cuda.synchronize()
            t = time.perf_counter()
            hh = compute_haplotype_hits(motif, dg, reg, False, _Args())
            t_call = time.perf_counter() - t
            t = time.perf_counter()
            df = compute_results_from_graph(motif, dg, reg, False, _Args())
            t_rep = time.perf_counter() - t
        # the kernel chain alone on the entries the report's pass just left (slot 0 of the graph's buffers)
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
        t_kern = ev0.elapsed_time(ev1) * 1e3
        t = time.perf_counter()
        c_h, b_h = counts.cpu().numpy(), best.cpu().numpy()
        t_d2h = time.perf_counter() - t
        assert (c_h == hh.counts).all() and (b_h == hh.best).all()
        t = time.perf_counter()
        path = write_haplotype_hits(hh, motif, 1, _Out())
        t_tsv = time.perf_counter() - t
        if rep:
            call.append(t_call * 1e3), report.append(t_rep * 1e3), kern.append(t_kern), d2h.append(t_d2h * 1e3)
            tsv.append(t_tsv * 1e3)
    med = statistics.median
    lines.append(f"report rows at p < 1e-4: {len(df)} (entries {n_hits}), sum of haplotype_frequency {int(df['haplotype_frequency'].sum())}"
                 f" = sum of the matrix {int(hh.counts.sum())}; cells with a hit {int((hh.counts > 0).sum())} of {R * H}")
    lines.append(f"compute_haplotype_hits, whole call, wall: median {med(call):.1f} ms (min {min(call):.1f}, {a.reps} reps)")
    lines.append(f"compute_results_from_graph, same arguments, wall: median {med(report):.1f} ms")
    lines.append(f"gfm_graph_haplotype_hits alone (memsets, grouping, masks, reduction, scratch), event-timed: median "
                 f"{med(kern) / 1e3:.3f} ms (min {min(kern) / 1e3:.3f})")
    lines.append(f"device -> host copy of counts + best ({2 * 4 * R * H / 1e6:.0f} MB, pageable): median {med(d2h):.1f} ms "
                 f"({2 * 4 * R * H / 1e6 / med(d2h):.1f} GB/s)")
    lines.append(f"TSV write ({os.path.getsize(path) / 1e6:.1f} MB): median {med(tsv):.1f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
