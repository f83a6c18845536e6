"""What the per-hit allele table costs on the bench's graph: synth.make_graph_index(10 000, 19) (5 096 haplotypes, a site
every 32 bases) with CTCF planted in 2 % of the regions as bench.py's config 4 plants its motif, at p < 1e-4 and once at a
looser threshold for a table of thousands of rows, with five population-sized haplotype groups.  Times, with wall clocks, the
whole compute_hit_alleles call (groups, no carrier sets) beside compute_results_from_graph (the report, same arguments) and
the to_frame() strings; with a hipEvent pair, gfm_graph_hit_alleles alone on the entries the report's pass left.  The
kernels' own times: run it under `rocprofv3 --kernel-trace --stats`.

    python scripts/hit_alleles_probe.py [--reps 5] [--out profiles/hit_alleles_probe.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Args:
    noreverse, recomb, noqvalue, qvalueT = False, False, False, False

    def __init__(self, threshold):
        self.threshold = threshold


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
    from grafimo_amd.hit_alleles import _group_bits, compute_hit_alleles
    from grafimo_amd.motif_ops import build_motif_meme_host

    motif = build_motif_meme_host(os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]
    probs = np.asarray(motif.count_matrix, dtype=np.float64)
    idx, regions = synth.make_graph_index(10_000, 19, plant=(probs, 0.02))
    dg = DeviceGraph(idx)
    reg = np.asarray(regions, dtype=np.int64)
    R, H = len(regions), int(idx.n_haplotypes)
    hw = (H + 63) // 64
    cuts = np.linspace(0, H, 6).astype(int)
    groups = {f"POP{k}": list(range(cuts[k], cuts[k + 1])) for k in range(5)}
    names = [f"hap{k}" for k in range(H)]
    _, bits = _group_bits(groups, names, H)
    d_bits = torch.from_numpy(bits.view(np.int64)).to(dg.device)
    lines = [f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {H} haplotypes ({hw} bitset words), {R} regions, W = 19, CTCF "
             f"planted in 2 % of the regions, both strands, 5 groups of ~{H // 5} haplotypes; {torch.cuda.get_device_name(0)}"]
    sink = io.StringIO()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    med = statistics.median
    for threshold in (1e-4, 1e-3):
        call, report, kern, frame = [], [], [], []
        for rep in range(a.reps + 1):
            with contextlib.redirect_stdout(sink):
                torch.cuda.synchronize()
                t = time.perf_counter()
                ha = compute_hit_alleles(motif, dg, reg, False, _Args(threshold), haplotype_names=names, haplotype_groups=groups)
                t_call = time.perf_counter() - t
                t = time.perf_counter()
                df = compute_results_from_graph(motif, dg, reg, False, _Args(threshold))
                t_rep = time.perf_counter() - t
            t = time.perf_counter()
            table = ha.to_frame()
            t_frame = time.perf_counter() - t
            # the C call alone on the entries the report's pass just left (slot 0 of the graph's buffers)
            buf, cap = dg.fused_buffers(0, 0)
            n_hits = min(int(buf[0].item()), cap)
            off = torch.empty(n_hits + 1, dtype=torch.int64, device=dg.device)
            packed = torch.empty(8 * n_hits + 1, dtype=torch.int32, device=dg.device)
            gc = torch.empty((n_hits, 5), dtype=torch.int32, device=dg.device)
            tot = torch.empty(n_hits, dtype=torch.int32, device=dg.device)
            torch.cuda.synchronize()
            ev0.record()
            nv.check(nv.lib().gfm_graph_hit_alleles(dg._h, *dg.hit_list(0)[:2], n_hits, None, 5,
                                                    d_bits.data_ptr(), off.data_ptr(), packed.data_ptr(), 8 * n_hits, gc.data_ptr(),
                                                    tot.data_ptr(), None, 0, _stream_ptr(None)))
            ev1.record()
            torch.cuda.synchronize()
            if rep:
                call.append(t_call * 1e3), report.append(t_rep * 1e3), kern.append(ev0.elapsed_time(ev1) * 1e3)
                frame.append(t_frame * 1e3)
        assert len(df) == len(ha) and (table["haplotype_frequency"] == ha.group_counts.sum(axis=1)).all()
        lines.append(f"p < {threshold:g}: {len(df)} report rows ({n_hits} entries), {len(ha.allele)} alleles in the rows' sets "
                     f"({len(ha.allele) / max(len(ha), 1):.2f} per row, at most {int(np.diff(ha.allele_offsets).max(initial=0))}), "
                     f"{int((ha.allele > 0).sum())} of them ALT")
        lines.append(f"  compute_hit_alleles, whole call, wall: median {med(call):.2f} ms (min {min(call):.2f}, {a.reps} reps)")
        lines.append(f"  compute_results_from_graph, same arguments, wall: median {med(report):.2f} ms "
                     f"-> the table costs {med(call) / med(report):.2f}x the report alone")
        lines.append(f"  gfm_graph_hit_alleles alone (memsets, entry kernel, scan, compaction, scratch), event-timed: median "
                     f"{med(kern):.1f} us (min {min(kern):.1f})")
        lines.append(f"  to_frame() (strings per distinct allele, joins per row): median {med(frame):.2f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
