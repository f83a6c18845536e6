"""What the indel scan costs, beside the only way the tree could produce its numbers before: the bench's panel
(synth.make_graph_index: 5 096 haplotypes, a site every 32 bases around every region's core), every version its regions spell
and the reference sequences, three synthetic motifs of W = 19 and one of W = 64 -- scripts/mutation_scan_probe.py's workload.
Reported per width:
  the new entry   gfm_sequence_indel_scan over the staged sequences and reused result tensors;
  the baseline    gfm_graph_query_edits over the SAME sequences with five items per non-inserted base -- the deletion of the
                  base and the insertion of A, C, G, T behind it, an item per (sequence, edit) --, staged once, a reused record
                  tensor.  An insertion is an item only where a coordinate can name it: the next base is the non-inserted next
                  coordinate, or the base is its sequence's last;
both with two hipEvents on the stream around the entry, --warmup passes, then --reps timed ones, median / min / max (each entry
clears a word, launches, copies 4 bytes back and waits for the stream: the figure is the kernels plus some tens of
microseconds), the ratio of the medians, whether the slowest pass of the new entry is below the fastest of the baseline, and
whether the two agree field for field on every item (compared on the device).  Then the wall time of the whole
compute_indel_scan_many call with both frames made.

    python scripts/indel_scan_probe.py [--regions 2000] [--reps 10] [--warmup 3] [--no-frames] [--out FILE]
"""
import argparse
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
    ap.add_argument("--no-frames", action="store_true", help="skip the whole call and its frames")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import indel_scan as isc
    from grafimo_amd import sequence_scans as ss
    from grafimo_amd import query_variants as qv
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.graph_tables import _matrix_rows, prepare_graphs
    from grafimo_amd.haplotype_classes import compute_haplotype_classes
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences

    clock = time.perf_counter
    idx, core = synth.make_graph_index(a.regions, 19)
    regions = np.array(core, dtype=np.int64)
    dg = DeviceGraph(idx)
    lines = [f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {int(idx.n_haplotypes)} haplotypes; {len(regions)} regions of "
             f"{int(regions[0, 1] - regions[0, 0])} bases; {torch.cuda.get_device_name(0)}"]
    # ---- the sequences, as compute_indel_scan_many makes them
    hc = compute_haplotype_classes(dg, regions, False, _Args())
    hs = compute_haplotype_sequences(dg, regions, False, _Args(), classes=hc, coordinates=True)
    prep = prepare_graphs(dg, regions, None)
    seqs = ss._with_references(hs, prep, _matrix_rows(prep)[0])
    seq_offsets, bases, coord = np.ascontiguousarray(seqs[5]), np.ascontiguousarray(seqs[6]), seqs[7]
    V, N = len(seq_offsets) - 1, len(bases)
    lines.append(f"input: {len(hs)} versions + {V - len(hs)} reference sequences = {V} sequences, {N} bases ({int((coord < 0).sum())} "
                 "inserted)")
    # ---- the baseline's items: per non-inserted base its deletion, and the four insertions behind it where a coordinate names them
    upper = ss._UPPER[bases]
    seq_of_base = np.repeat(np.arange(V, dtype=np.int64), np.diff(seq_offsets))
    last = np.zeros(N, dtype=bool)
    last[seq_offsets[1:][np.diff(seq_offsets) > 0] - 1] = True
    nxt = np.concatenate([coord[1:], [-1]]).astype(np.int64)
    dele = np.flatnonzero(coord >= 0)
    ins = np.flatnonzero((coord >= 0) & (last | (nxt == coord.astype(np.int64) + 1)))
    n_of = np.concatenate([dele, np.repeat(ins, 4)])                                   # the base of every item
    ref_col = np.concatenate([np.full(len(dele), isc.COVER), np.full(4 * len(ins), isc.JUNCTION)]).astype(np.int64)
    alt_col = np.concatenate([np.full(len(dele), isc.DEL), np.tile(np.arange(isc.INS_A, isc.INS_A + 4), len(ins))]).astype(np.int64)
    pos0 = np.concatenate([coord[dele], np.repeat(coord[ins], 4) + 1]).astype(np.int64)
    ref_off = np.concatenate([np.arange(len(dele) + 1), np.full(4 * len(ins), len(dele))]).astype(np.int32)
    alt_off = np.concatenate([np.zeros(len(dele) + 1), np.arange(1, 4 * len(ins) + 1)]).astype(np.int32)
    pad = lambda x: np.concatenate([x, np.zeros(1, dtype=x.dtype)])                    # noqa: E731  (never an empty buffer)
    Q = len(n_of)
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)      # noqa: E731
    d_edits = [up(seq_offsets, np.int64), up(bases, np.uint8), up(coord, np.int32), up(pos0, np.int64), up(ref_off, np.int32),
               up(pad(upper[dele]), np.uint8), up(alt_off, np.int32), up(pad(np.tile(ss.TO_BASES, len(ins))), np.uint8),
               up(seq_of_base[n_of], np.int32), up(np.arange(Q), np.int32)]
    lines.append(f"baseline items: {len(dele)} deletions + {4 * len(ins)} insertions = {Q} ({Q / max(N, 1):.2f} a base)")
    ok = True
    for W, n_motifs in ((19, 3), (64, 1)):
        motifs = [synth.motif_object(synth.synthetic_motif(W, np.random.default_rng(7 + k), np.full(4, 0.25)), f"P{W}_{k}")
                  for k in range(n_motifs)]
        dms = [DeviceMotif.lease(m) for m in motifs]
        tables, _ = qv._weight_tables(dms, motifs, None, 1.0)
        staged = ss.stage(tables, seq_offsets, bases, (N, len(isc.COLUMNS)))
        new = _timed(lambda: ss.enqueue(dms, staged, False, isc.ENTRY), a.warmup, a.reps)
        d_tabs = [up(t.view(np.int64), np.int64) for t in tables]
        q_staged = (d_edits, d_tabs, max(int(t.max()) for t in tables), (V, Q, Q))
        rec = torch.zeros((n_motifs, Q, 4), dtype=torch.int64, device=dev)
        old = _timed(lambda: qv._enqueue(dms, q_staged, False, rec), a.warmup, a.reps)
        keys, sums = staged[4].view(n_motifs, N * 7), staged[5].view(n_motifs, N * 7)
        d_r, d_a = up(n_of * 7 + ref_col, np.int64), up(n_of * 7 + alt_col, np.int64)
        # status applied in the low word, o above it: the deletion's o is the base's offset, the insertion's the offset behind it
        o_want = up((n_of - seq_offsets[seq_of_base[n_of]] + (alt_col != isc.DEL)) << 32, np.int64)
        same = bool((rec[:, :, 0] == o_want[None, :]).all())
        same &= bool((rec[:, :, 2] == sums[:, d_r]).all()) and bool((rec[:, :, 3] == sums[:, d_a]).all())
        packed = (keys[:, d_r].to(torch.int64) & 0xffffffff) | ((keys[:, d_a].to(torch.int64) & 0xffffffff) << 32)
        same &= bool((rec[:, :, 1] == packed).all())
        below = new[2] < old[1]
        ok &= same and below
        lines.append(f"W = {W}, {n_motifs} motifs: gfm_sequence_indel_scan over {N} bases: median {new[0]:.3f} ms (min {new[1]:.3f}, max "
                     f"{new[2]:.3f}); gfm_graph_query_edits over {Q} one-base indels of the same bases: median {old[0]:.3f} ms (min "
                     f"{old[1]:.3f}, max {old[2]:.3f}); {a.warmup} warm-ups, {a.reps} timed; ratio {old[0] / new[0]:.1f}x; the new "
                     f"entry's slowest pass is below the baseline's fastest: {below}; {N * n_motifs * 7 / new[0] / 1e6:.2f} G (base, "
                     f"column) cells/s; the two agree on every item: {same}")
        del rec, staged, q_staged
        for dm in dms:
            dm.release()
    # ---- the whole call, as a user makes it
    if not a.no_frames:
        motifs = [synth.motif_object(synth.synthetic_motif(19, np.random.default_rng(7 + k), np.full(4, 0.25)), f"P19_{k}") for k in range(3)]
        t = clock()
        tabs = isc.compute_indel_scan_many(motifs, dg, regions, False, _Args())
        t_compute = clock() - t
        rows = [len(x.to_frame()) for x in tabs]
        t_detail = clock() - t - t_compute
        srows = [len(x.summary_frame()) for x in tabs]
        wall = clock() - t
        lines.append(f"compute_indel_scan_many: {t_compute:.2f} s for {N} bases x 3 motifs; to_frame {t_detail:.2f} s ({rows} rows kept "
                     f"a motif); summary_frame {wall - t_compute - t_detail:.2f} s ({srows} rows); {wall:.2f} s wall in all")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    dg.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
