"""What the shuffle null's kernel costs: --seqs random sequences of --length bases, --replicates shuffles of each, motifs of
width --width, for 1 motif and for 16 (one launch: the shuffle is made once for all of them), staged once with reused result
tensors, two hipEvents on the stream around the entry, --warmup passes, then --reps timed ones: median / min / max (the entry
clears the counters, uploads its sequence table, launches per length class, copies 4 bytes back and waits for the stream: the
figure is the kernels plus some tens of microseconds), and the ratio of the 16-motif median to the 1-motif median -- 16 if the
shuffle cost nothing, 1 if it cost everything.  Then the same for --long-length bases (the scratch path) at a tenth of the
sequences, and the LDS-instruction floor of the shape (DESIGN 3.22 derives it).  --no-reverse scores the + strand only: the same
LDS work with one weight gather a window instead of two, which shows what the gathers cost.  --order 2 makes the replicates
doublet-preserving: what is made once per launch is then the counting sort, the arborescence, the bucket shuffles
and the walk; the floor printed is order 1's.

    python scripts/null_probe.py [--seqs 2000] [--length 300] [--replicates 1024] [--width 19] [--reps 5] [--warmup 2]
                                 [--order 1] [--no-reverse] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--seqs", type=int, default=2000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--long-length", type=int, default=2000)
    ap.add_argument("--replicates", type=int, default=1024)
    ap.add_argument("--width", type=int, default=19)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--order", type=int, choices=(1, 2), default=1, help="2: doublet-preserving replicates")
    ap.add_argument("--no-reverse", action="store_true", help="+ strand only: one weight gather a window instead of two")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import shuffle_null as sn
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.haplotype_affinity import default_weights
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from extract_fuzz_core import SynMotif

    lines = [f"{torch.cuda.get_device_name(0)}: W = {a.width}, K = {a.replicates}, {'+ strand only' if a.no_reverse else 'both strands'}"
             + (f", order {a.order}" if a.order != 1 else "")]
    rng = np.random.default_rng(1)
    W, K = a.width, a.replicates
    motifs = [SynMotif(W, seed=900 + k) for k in range(16)]
    dms = [DeviceMotif.lease(m) for m in motifs]
    try:
        tables = [default_weights(dm, 1.0)[0] for dm in dms]
        for n_seqs, length in ((a.seqs, a.length), (max(a.seqs // 10, 1), a.long_length)):
            off = np.arange(n_seqs + 1, dtype=np.int64) * length
            bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n_seqs * length)]
            keys = sn.content_keys(off, bases)
            med = {}
            for M in (1, 16):
                staged = sn._stage(tables[:M], off, bases, keys, np.ones(n_seqs, dtype=np.uint32), K, False)
                run = lambda: sn._enqueue(dms[:M], staged, K, 0, [9000] * M, a.no_reverse, a.order)     # noqa: E731
                med[M], lo, hi = _timed(run, a.warmup, a.reps)
                windows = n_seqs * K * (length - W + 1)
                lines.append(f"{n_seqs} sequences of {length} bases, {M:2d} motifs: median {med[M]:9.3f} ms (min {lo:.3f}, max {hi:.3f}), "
                             f"{M * windows / med[M] / 1e6:8.1f} G windows/s")
            lines.append(f"{n_seqs} sequences of {length} bases: 16 motifs / 1 motif = {med[16] / med[1]:.2f}; a further motif "
                         f"{(med[16] - med[1]) / 15:.3f} ms, made once {med[1] - (med[16] - med[1]) / 15:.3f} ms")
            # the floor: a window column costs the lane a byte read of its code and a word read of the table row, a swap two
            # byte reads and two byte stores: wave-instructions on the LDS, at best 2 array cycles each, a CU's LDS one at a time
            waves = n_seqs * ((K + 63) // 64)
            per_motif = waves * (length - W + 1) * W * 2
            shuffle = waves * (length - 1) * 4
            cus, ghz = torch.cuda.get_device_properties(0).multi_processor_count, 2.4
            floor = lambda M: (M * per_motif + shuffle) * 2 / cus / (ghz * 1e6)          # noqa: E731
            lines.append(f"{n_seqs} sequences of {length} bases: LDS-instruction floor at {cus} CUs, {ghz} GHz, 2 cycles an instruction: "
                         f"{floor(1):.3f} ms for 1 motif, {floor(16):.3f} ms for 16 (LDS path only)")
    finally:
        for dm in dms:
            dm.release()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
