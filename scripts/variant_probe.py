"""What the per-variant effect table costs on the bench's graph: synth.make_graph_index(10 000, 19) (5 096 haplotypes, a site
every 32 bases) and CTCF.  Times, with a hipEvent pair on the stream, the whole device-facing call (_scan: buffers, the host
window list and its upload, both kernels, the count read-back, the copy of the records written) -- without and with
--recomb, which skips the haplotype presence test -- the whole compute_variant_effects call with wall clocks, and
gfm_graph_score on the same regions beside it.  The kernels' own times: run it under
`rocprofv3 --kernel-trace --stats` (with --recomb-only for the kernels without the presence test).

    python scripts/variant_probe.py [--reps 7] [--recomb-only] [--out profiles/variant_probe.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Args:
    threshold, noreverse, recomb, noqvalue, qvalueT = 1e-4, False, False, True, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--recomb-only", action="store_true", help="time the --recomb form alone (no presence test)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.motif_ops import build_motif_meme_host
    from grafimo_amd.variant_effects import _scan, compute_variant_effects

    motif = build_motif_meme_host(os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]
    idx, regions = synth.make_graph_index(10_000, 19)
    dg = DeviceGraph(idx)
    starts = np.array([s for s, _ in regions], dtype=np.int64)
    stops = np.array([e for _, e in regions], dtype=np.int64)
    lines = [f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {idx.n_haplotypes} haplotypes, {len(regions)} regions, W = 19, "
             f"{torch.cuda.get_device_name(0)}"]
    dm = DeviceMotif.lease(motif)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kern, kern_rc, call, score = [], [], [], []
    try:
        for rep in range(a.reps + 1):
            for rc_, lst in ((False, kern), (True, kern_rc)):
                if a.recomb_only and not rc_:
                    continue
                torch.cuda.synchronize()
                ev0.record()
                recs, over = _scan(dg, starts, stops, [dm], False, rc_)      # (synchronises: reads the counts back)
                ev1.record()
                torch.cuda.synchronize()
                if rep:
                    lst.append(ev0.elapsed_time(ev1) * 1e3)
            if a.recomb_only:
                continue
            t = time.perf_counter()
            df = compute_variant_effects(motif, dg, regions, False, _Args())
            if rep:
                call.append((time.perf_counter() - t) * 1e6)
            torch.cuda.synchronize()
            ev0.record()
            dg.score(dm, starts, stops, dm.pvalue_cutoff(1e-4))
            ev1.record()
            torch.cuda.synchronize()
            if rep:
                score.append(ev0.elapsed_time(ev1) * 1e3)
    finally:
        dm.release()
    med = statistics.median
    if a.recomb_only:
        lines.append(f"_scan --recomb (buffers, window list + upload, both kernels, count read-back, record copy), event-timed: "
                     f"median {med(kern_rc):.1f} us (min {min(kern_rc):.1f}, {a.reps} reps)")
    else:
        lines.append(f"records {len(recs[0])} (--recomb), overflow {over}, table rows at p < 1e-4: {len(df)} "
                     f"({dict(df['effect'].value_counts())})")
        lines.append(f"_scan (buffers, window list + upload, both kernels, count read-back, record copy), event-timed: median "
                     f"{med(kern):.1f} us (min {min(kern):.1f}, max {max(kern):.1f}, {a.reps} reps)")
        lines.append(f"_scan --recomb (the same without the presence test), event-timed: median {med(kern_rc):.1f} us "
                     f"(min {min(kern_rc):.1f})")
        lines.append(f"compute_variant_effects, whole call, wall: median {med(call):.1f} us (min {min(call):.1f})")
        lines.append(f"gfm_graph_score on the same regions (report path, the call enqueued to done), event-timed: median "
                     f"{med(score):.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
