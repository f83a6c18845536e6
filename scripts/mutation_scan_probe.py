"""What the mutation scan costs, beside the only way the tree could produce its numbers before: the bench's panel
(synth.make_graph_index: 5 096 haplotypes, a site every 32 bases around every region's core), every version its regions spell
and the reference sequences, three synthetic motifs of W = 19 and one of W = 64.  Reported per width:
  the new entry   gfm_sequence_mutation_scan over the staged sequences and reused result tensors;
  the baseline    gfm_graph_query_edits over the SAME sequences with three SNVs per non-inserted base -- an item per
                  (sequence, base, to-base) --, staged once, a reused record tensor;
both with two hipEvents on the stream around the entry, --warmup passes, then --reps timed ones, median / min / max (each entry
clears a word, launches, copies 4 bytes back and waits for the stream: the figure is the kernels plus some tens of
microseconds), the ratio of the medians, and whether the two agree field for field on every item.  Then the wall time of the
whole compute_mutation_scan_many call with both frames made, and of compute_query_variants_many over a sample of the same SNVs:
of --baseline-variants / 3 random bases, those that lie on a version that is the reference's, three SNVs each.

    python scripts/mutation_scan_probe.py [--regions 2000] [--reps 10] [--warmup 3] [--baseline-variants 100000] [--out FILE]
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
    ap.add_argument("--baseline-variants", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import mutation_scan as ms
    from grafimo_amd import query_variants as qv
    from grafimo_amd import sequence_scans as ss
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
    # ---- the sequences, as compute_mutation_scan_many makes them
    t0 = clock()
    hc = compute_haplotype_classes(dg, regions, False, _Args())
    t1 = clock()
    hs = compute_haplotype_sequences(dg, regions, False, _Args(), classes=hc, coordinates=True)
    t2 = clock()
    prep = prepare_graphs(dg, regions, None)
    seqs = ss._with_references(hs, prep, _matrix_rows(prep)[0])
    seq_offsets, bases, coord = np.ascontiguousarray(seqs[5]), np.ascontiguousarray(seqs[6]), seqs[7]
    t3 = clock()
    V, N = len(seq_offsets) - 1, len(bases)
    lines.append(f"input: {len(hs)} versions + {V - len(hs)} reference sequences = {V} sequences, {N} bases ({int((coord < 0).sum())} "
                 f"inserted); classes {t1 - t0:.2f} s, sequences {t2 - t1:.2f} s, assembling {t3 - t2:.2f} s")
    # ---- the baseline's items: three SNVs per non-inserted base
    upper = ss._UPPER[bases]
    column = ss._COLUMN_OF[bases]
    at = np.flatnonzero(coord >= 0)
    n_of = np.repeat(at, 3)
    to_col = (np.tile(np.arange(3, dtype=np.int64), len(at)) + np.repeat(column[at], 3)) % 4 + 1      # the three other columns
    to_col = np.where(np.repeat(column[at], 3) == 0, np.tile(np.arange(1, 4, dtype=np.int64), len(at)), to_col)
    Q = len(n_of)
    seq_of_base = np.repeat(np.arange(V, dtype=np.int64), np.diff(seq_offsets))
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)      # noqa: E731
    one_each = np.arange(Q + 1, dtype=np.int32)
    d_edits = [up(seq_offsets, np.int64), up(bases, np.uint8), up(coord, np.int32), up(coord[n_of], np.int64), up(one_each, np.int32),
               up(upper[n_of], np.uint8), up(one_each, np.int32), up(ss.TO_BASES[to_col - 1], np.uint8),
               up(seq_of_base[n_of], np.int32), up(np.arange(Q), np.int32)]
    for W, n_motifs in ((19, 3), (64, 1)):
        motifs = [synth.motif_object(synth.synthetic_motif(W, np.random.default_rng(7 + k), np.full(4, 0.25)), f"P{W}_{k}")
                  for k in range(n_motifs)]
        dms = [DeviceMotif.lease(m) for m in motifs]
        tables, _ = qv._weight_tables(dms, motifs, None, 1.0)
        staged = ss.stage(tables, seq_offsets, bases, (N, len(ms.COLUMNS)))
        new = _timed(lambda: ss.enqueue(dms, staged, False, ms.ENTRY), a.warmup, a.reps)
        d_tabs = [up(t.view(np.int64), np.int64) for t in tables]
        q_staged = (d_edits, d_tabs, max(int(t.max()) for t in tables), (V, Q, Q))
        rec = torch.zeros((n_motifs, Q, 4), dtype=torch.int64, device=dev)
        old = _timed(lambda: qv._enqueue(dms, q_staged, False, rec), a.warmup, a.reps)
        keys, sums = staged[4].view(n_motifs, N * 5), staged[5].view(n_motifs, N * 5)
        d_n, d_c = up(n_of, np.int64), up(to_col, np.int64)
        same = bool(((rec[:, :, 0] & 0xffffffff) == 0).all())                       # status applied (o lies above it)
        same &= bool((rec[:, :, 2] == sums[:, d_n * 5]).all()) and bool((rec[:, :, 3] == sums[:, d_n * 5 + d_c]).all())
        packed = (keys[:, d_n * 5].to(torch.int64) & 0xffffffff) | ((keys[:, d_n * 5 + d_c].to(torch.int64) & 0xffffffff) << 32)
        same &= bool((rec[:, :, 1] == packed).all())
        lines.append(f"W = {W}, {n_motifs} motifs: gfm_sequence_mutation_scan over {N} bases: median {new[0]:.3f} ms (min {new[1]:.3f}, max "
                     f"{new[2]:.3f}); gfm_graph_query_edits over {Q} SNVs of the same bases: median {old[0]:.3f} ms (min {old[1]:.3f}, max "
                     f"{old[2]:.3f}); {a.warmup} warm-ups, {a.reps} timed; ratio {old[0] / new[0]:.1f}x; "
                     f"{N * n_motifs * 5 / new[0] / 1e6:.2f} G (base, column) cells/s; the two agree on every item: {same}")
        del rec, staged, q_staged
        for dm in dms:
            dm.release()
    # ---- the whole calls, as a user makes them
    motifs = [synth.motif_object(synth.synthetic_motif(19, np.random.default_rng(7 + k), np.full(4, 0.25)), f"P19_{k}") for k in range(3)]
    t = clock()
    tabs = ms.compute_mutation_scan_many(motifs, dg, regions, False, _Args())
    t_compute = clock() - t
    rows = [len(x.to_frame()) for x in tabs]
    t_detail = clock() - t - t_compute
    srows = [len(x.summary_frame()) for x in tabs]
    wall = clock() - t
    lines.append(f"compute_mutation_scan_many: {t_compute:.2f} s for {N} bases x 3 motifs; to_frame {t_detail:.2f} s ({rows} rows kept of "
                 f"{3 * N} a motif); summary_frame {wall - t_compute - t_detail:.2f} s ({srows} rows); {wall:.2f} s wall in all")
    pick = np.random.default_rng(139).permutation(len(at))[:max(a.baseline_variants // 3, 1)]
    ref_at = seqs[4][seq_of_base[at[pick]]] & (seqs[1][seq_of_base[at[pick]]] >= 0)
    pick = pick[ref_at] if ref_at.any() else pick
    variants = [(idx.chrom, int(p) + 1, f"v{k}", chr(r), b) for k, (p, r) in enumerate(zip(coord[at[pick]].tolist(), upper[at[pick]].tolist()))
                for b in "ACGT" if b != chr(r)]
    t = clock()
    qv.compute_query_variants_many(motifs, dg, variants, False, _Args(), all_variants=True)
    q_wall = clock() - t
    lines.append(f"compute_query_variants_many over {len(variants)} of these SNVs (every background of each): {q_wall:.2f} s wall -> "
                 f"{q_wall / len(variants) * 1e6:.1f} us an SNV, against {wall / (3 * N) * 1e6:.2f} us an SNV of the scan")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    dg.close()


if __name__ == "__main__":
    main()
