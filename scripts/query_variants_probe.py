"""What the query-variant table costs: a synthetic catalogue of --variants SNVs over the bench's panel (synth.make_graph_index:
5 096 haplotypes, a site every 32 bases around every region's core), three synthetic motifs of W = 19.  Reported: the kernel's
entry (gfm_graph_query_edits over the staged inputs and a reused record tensor, two hipEvents on the stream around the call,
--warmup passes, then --reps timed ones, median / min / max; the entry clears a word, launches, copies 4 bytes back and waits
for the stream, so the figure is the kernel plus some tens of microseconds: an upper bound of the kernel's own time) as items
per second -- an item is one (sequence, edit, motif) --, the host steps that prepare its input
(footprints, classes, sequences, staging), and the wall time of the whole compute_query_variants_many call.

    python scripts/query_variants_probe.py [--variants 100000] [--regions 2000] [--reps 10] [--warmup 3] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=100_000)
    ap.add_argument("--regions", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import query_variants as qv
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.haplotype_classes import compute_haplotype_classes
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences

    W = 19
    rng = np.random.default_rng(139)
    idx, core = synth.make_graph_index(a.regions, W)
    ref = np.asarray(idx.ref)
    per = (a.variants + a.regions - 1) // a.regions
    pos = np.concatenate([rng.integers(S - 20, E + 20, size=per) for S, E in core])[:a.variants]
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    alt = acgt[(np.searchsorted(acgt, ref[pos]) + rng.integers(1, 4, size=len(pos))) % 4]
    variants = [(idx.chrom, int(p) + 1, f"v{k}", chr(r), chr(x)) for k, (p, r, x) in enumerate(zip(pos.tolist(), ref[pos].tolist(), alt.tolist()))]
    motifs = [synth.motif_object(synth.synthetic_motif(W, np.random.default_rng(7 + k), np.full(4, 0.25)), f"P{k}") for k in range(3)]
    dg = DeviceGraph(idx)
    lines = [f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {int(idx.n_haplotypes)} haplotypes; {len(variants)} SNVs, "
             f"{len(motifs)} motifs of W = {W}; {torch.cuda.get_device_name(0)}"]
    # ---- the steps by hand: what the kernel's input costs, then the kernel alone
    clock = time.perf_counter
    t0 = clock()
    pos0 = pos.astype(np.int64)
    S, E = qv.footprints(idx, pos0, np.ones(len(pos0), dtype=np.int64), W)
    t1 = clock()
    regions = np.stack([S, E], axis=1)
    hc = compute_haplotype_classes(dg, regions, False, _Args())
    t2 = clock()
    hs = compute_haplotype_sequences(dg, regions, False, _Args(), classes=hc, coordinates=True)
    t3 = clock()
    seq_offsets, bases, coord, item_edit, _ = qv._sequences_and_items(hs, [idx], np.zeros(len(pos0), dtype=np.int64), S, E)
    dms = [DeviceMotif.lease(m) for m in motifs]
    tables, _ = qv._weight_tables(dms, motifs, None, 1.0)
    N = len(item_edit)
    staged = qv._stage(tables, seq_offsets, bases, coord, pos0, [chr(r) for r in ref[pos].tolist()], [chr(x) for x in alt.tolist()],
                       np.arange(N, dtype=np.int64), item_edit)
    torch.cuda.synchronize()
    t4 = clock()
    lines.append(f"input: {len(hs)} versions ({len(hs) / len(variants):.1f} a variant) + {len(variants)} references = {N} sequences of "
                 f"{len(bases) / N:.0f} bases; footprints {1e3 * (t1 - t0):.0f} ms, classes {t2 - t1:.2f} s, sequences {t3 - t2:.2f} s, "
                 f"items + staging {t4 - t3:.2f} s")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rec = torch.zeros((len(motifs), N, 4), dtype=torch.int64, device=dg.device)       # (made once, outside the events)
    ms = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        ev[0].record()
        rec = qv._enqueue(dms, staged, False, rec)
        ev[1].record()
        torch.cuda.synchronize()
        if rep >= a.warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    got = rec.cpu().numpy().view(qv.RECORD).reshape(len(motifs), N)
    applied = int((got[0]["status"] == 0).sum())
    windows = 2 * 2 * W                                  # an applied SNV: W starts a side, two sides, two strands
    med = statistics.median(ms)
    items = N * len(motifs)
    lines.append(f"kernel entry: {items} items ({applied * len(motifs)} applied, {windows} windows of {W} lookups each): median {med:.3f} ms "
                 f"(min {min(ms):.3f}, max {max(ms):.3f}; {a.warmup} warm-ups, {a.reps} timed) -> {items / med / 1e3:.1f} M items/s, "
                 f"{applied * len(motifs) * windows * W / 2 / med / 1e6:.1f} G table lookups/s")
    for dm in dms:
        dm.release()
    # ---- the whole call, as a user makes it
    t = clock()
    tabs = qv.compute_query_variants_many(motifs, dg, variants, False, _Args(), all_variants=True)
    wall = clock() - t
    lines.append(f"compute_query_variants_many: {wall:.2f} s wall for {len(variants)} variants x {len(motifs)} motifs "
                 f"({len(tabs[0].records)} contexts a motif); the kernel is {med / 1e3 / wall * 100:.2f} % of it")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    dg.close()


if __name__ == "__main__":
    main()
