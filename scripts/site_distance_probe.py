"""What the site distance costs, beside the mutation scan on the same input in the same session: the bench's panel
(synth.make_graph_index: 5 096 haplotypes, a site every 32 bases around every region's core), every version its regions spell
and the reference sequences, three synthetic motifs of W = 19 and one of W = 64 -- the sequences and widths of
scripts/mutation_scan_probe.py.  Reported per width:
  the new entry   gfm_sequence_site_distance over the staged sequences and reused result tensors, at E = 1, 3 and 8, with the
                  cutoff of the report's threshold (p < 1e-3) and, to see what the cutoff does to the cost, at E = 3 with the
                  cutoffs 0 (every window a site: the fragile side works) and 1000 W + 1 (nothing reaches it: the near side works);
  beside it       gfm_sequence_mutation_scan over the SAME sequences,
both with two hipEvents on the stream around the entry, --warmup passes, then --reps timed ones, median / min / max (each entry
clears a word, launches, copies 4 bytes back and waits for the stream: the figure is the kernels plus some tens of
microseconds), and the ratio of the medians.  Then the wall time of the whole compute_site_distance_many call with both frames.

    python scripts/site_distance_probe.py [--regions 2000] [--reps 10] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Args:
    threshold, noreverse, recomb, noqvalue, qvalueT = 1e-3, False, False, True, False


def _timed(run, warmup, reps):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        ev[0].record()
        run()
        ev[1].record()
        torch.cuda.synchronize()
        if rep >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd import mutation_scan as ms
    from grafimo_amd import sequence_scans as ss
    from grafimo_amd import query_variants as qv
    from grafimo_amd import site_distance as sd
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import DeviceGraph, _stream_ptr
    from grafimo_amd.graph_tables import _matrix_rows, prepare_graphs
    from grafimo_amd.haplotype_classes import compute_haplotype_classes
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences

    clock = time.perf_counter
    idx, core = synth.make_graph_index(a.regions, 19)
    regions = np.array(core, dtype=np.int64)
    dg = DeviceGraph(idx)
    lines = [f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {int(idx.n_haplotypes)} haplotypes; {len(regions)} regions of "
             f"{int(regions[0, 1] - regions[0, 0])} bases; {torch.cuda.get_device_name(0)}"]
    # ---- the sequences, as compute_site_distance_many makes them
    hc = compute_haplotype_classes(dg, regions, False, _Args())
    hs = compute_haplotype_sequences(dg, regions, False, _Args(), classes=hc, coordinates=True)
    prep = prepare_graphs(dg, regions, None)
    seqs = ss._with_references(hs, prep, _matrix_rows(prep)[0])
    seq_offsets, bases = np.ascontiguousarray(seqs[5]), np.ascontiguousarray(seqs[6])
    V, N = len(seq_offsets) - 1, len(bases)
    lines.append(f"input: {len(hs)} versions + {V - len(hs)} reference sequences = {V} sequences, {N} bases")
    dev = torch.device("cuda", torch.cuda.current_device())
    d_bases = torch.from_numpy(bases).to(dev)
    vp = ctypes.c_void_p
    for W, n_motifs in ((19, 3), (64, 1)):
        motifs = [synth.motif_object(synth.synthetic_motif(W, np.random.default_rng(7 + k), np.full(4, 0.25)), f"P{W}_{k}")
                  for k in range(n_motifs)]
        dms = [DeviceMotif.lease(m) for m in motifs]
        words = torch.empty((n_motifs, N, 6), dtype=torch.int32, device=dev)
        masks = torch.empty((n_motifs, N, 4), dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        handles = (vp * n_motifs)(*[x.handle for x in dms])
        p_words = (vp * n_motifs)(*[words[m].data_ptr() for m in range(n_motifs)])
        p_masks = (vp * n_motifs)(*[masks[m].data_ptr() for m in range(n_motifs)])
        report = np.array([sd.cutoff_of(dm.ptable_host(), _Args.threshold) for dm in dms], dtype=np.int32)

        def run(cut, E):
            nv.check(nv.lib().gfm_sequence_site_distance(handles, n_motifs, V, seq_offsets.ctypes.data, d_bases.data_ptr(),
                                                         cut.ctypes.data, E, 0, p_words, p_masks, status.data_ptr(), _stream_ptr(None)))
        # the mutation scan, from the same library, over the same staged sequences
        tables, _ = qv._weight_tables(dms, motifs, None, 1.0)
        staged = ss.stage(tables, seq_offsets, bases, (N, len(ms.COLUMNS)))
        old = _timed(lambda: ss.enqueue(dms, staged, False, ms.ENTRY), a.warmup, a.reps)
        lines.append(f"W = {W}, {n_motifs} motifs, {N} bases: gfm_sequence_mutation_scan: median {old[0]:.3f} ms (min {old[1]:.3f}, max "
                     f"{old[2]:.3f}); {a.warmup} warm-ups, {a.reps} timed")
        for E in (1, 3, 8):
            new = _timed(lambda: run(report, E), a.warmup, a.reps)
            w = words.cpu().numpy().view(np.uint32)
            some = w[:, :, 0] != sd.NO_WINDOW
            near = np.bincount((w[:, :, 2:4][some] & 15).reshape(-1), minlength=E + 2)
            site = sd.own_scores(w[:, :, 0:2][some]) >= report[:, None, None].repeat(N, axis=1)[some]
            frag = np.bincount((w[:, :, 4:6][some] & 15)[site], minlength=E + 2)
            lines.append(f"  gfm_sequence_site_distance, E = {E}, cutoffs {report.tolist()} (p < {_Args.threshold}): median {new[0]:.3f} ms "
                         f"(min {new[1]:.3f}, max {new[2]:.3f}); {new[0] / old[0]:.2f}x the mutation scan; "
                         f"{2 * int(some.sum()) / new[0] / 1e6:.2f} G window-strands/s; near d counts {near.tolist()}, fragile d counts of "
                         f"the sites {frag.tolist()}")
        for name, cut in (("0", np.zeros(n_motifs, dtype=np.int32)), ("1000 W + 1", np.full(n_motifs, 1000 * W + 1, dtype=np.int32))):
            new = _timed(lambda: run(cut, 3), a.warmup, a.reps)
            lines.append(f"  gfm_sequence_site_distance, E = 3, cutoff {name}: median {new[0]:.3f} ms (min {new[1]:.3f}, max {new[2]:.3f}); "
                         f"{new[0] / old[0]:.2f}x the mutation scan")
        del words, masks, staged
        for dm in dms:
            dm.release()
    # ---- the whole call, as a user makes it
    motifs = [synth.motif_object(synth.synthetic_motif(19, np.random.default_rng(7 + k), np.full(4, 0.25)), f"P19_{k}") for k in range(3)]
    t = clock()
    tabs = sd.compute_site_distance_many(motifs, dg, regions, False, _Args(), max_edits=3)
    t_compute = clock() - t
    rows = [len(x.to_frame()) for x in tabs]
    t_detail = clock() - t - t_compute
    srows = [len(x.summary_frame()) for x in tabs]
    wall = clock() - t
    lines.append(f"compute_site_distance_many, E = 3: {t_compute:.2f} s for {N} bases x 3 motifs; to_frame {t_detail:.2f} s ({rows} rows "
                 f"kept); summary_frame {wall - t_compute - t_detail:.2f} s ({srows} rows); {wall:.2f} s wall in all")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    dg.close()


if __name__ == "__main__":
    main()
