"""What the insertion scan costs, beside the only way the tree could produce its numbers before: --seqs random sequences of
--length bases (the other sequence probes' 2 000 x 300), every base non-inserted with consecutive coordinates, so that every
gap is one a coordinate can name; three synthetic motifs of W = 19.  Reported for the insert lists (A, C, G, T), one 10-mer,
and a 64-mer with a 5-mer:
  the new entry   gfm_sequence_insertion_scan over the staged sequences and reused result tensors;
  the baseline    gfm_graph_query_edits (query_variants.score_edits' entry) over the SAME sequences with one item per (insert,
                  offset) -- exactly the insertions the new entry scores --, staged once, a reused record tensor;
  the floor       for (A, C, G, T) only: gfm_sequence_indel_scan (indel_scan.scan_sequences' entry) on the same input, which
                  writes seven columns a base where the insertion scan writes two a base and insert;
each with two hipEvents on the stream around the entry, --warmup passes, then --reps timed ones, median / min / max (each entry
clears a word, launches, copies 4 bytes back and waits for the stream: the figure is the kernels plus some tens of
microseconds), the ratio of the medians, whether the slowest pass of the new entry is below the fastest of the baseline (the
run-to-run spread the probe itself sees), and whether the two agree field for field on every item (compared on the device).

    python scripts/insertion_scan_probe.py [--seqs 2000] [--length 300] [--reps 10] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEN = b"GATTACAGAT"
FIVE = b"CTGCA"
LONG = b"ACGTTGCAAGGCTTAACCGGATATCGCGTATGCATGCAAGTCCTGAGGTTCCAAGGTCAGTCAA"


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd import indel_scan as isc
    from grafimo_amd import insertion_scan as ins
    from grafimo_amd import sequence_scans as ss
    from grafimo_amd import query_variants as qv
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import _stream_ptr

    W, n_motifs = 19, 3
    rng = np.random.default_rng(23)
    V, n = a.seqs, a.length
    N = V * n
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=N)]
    seq_offsets = np.arange(V + 1, dtype=np.int64) * n
    within = np.tile(np.arange(n, dtype=np.int64), V)
    coord = within.astype(np.int32)                               # every sequence carries the coordinates 0 .. n - 1
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)      # noqa: E731
    lines = [f"input: {V} sequences of {n} bases = {N} bases, none inserted; {n_motifs} motifs of W = {W}; {torch.cuda.get_device_name(0)}"]
    motifs = [synth.motif_object(synth.synthetic_motif(W, np.random.default_rng(7 + k), np.full(4, 0.25)), f"P{W}_{k}")
              for k in range(n_motifs)]
    dms = [DeviceMotif.lease(m) for m in motifs]
    tables, _ = qv._weight_tables(dms, motifs, None, 1.0)
    d_tabs = [up(t.view(np.int64), np.int64) for t in tables]
    max_weight = max(int(t.max()) for t in tables)
    d_bases = up(bases, np.uint8)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    handles, tabs = (vp * n_motifs)(*[x.handle for x in dms]), (vp * n_motifs)(*[t.data_ptr() for t in d_tabs])
    ok = True
    for inserts in ((b"A", b"C", b"G", b"T"), (TEN,), (LONG, FIVE)):
        inserts = ins.checked_inserts(inserts)
        K = len(inserts)
        ioff, itext = ins._packed(inserts)
        keys = torch.empty((n_motifs, K, N, 2), dtype=torch.int32, device=dev)
        sums = torch.empty((n_motifs, K, N, 2), dtype=torch.int64, device=dev)
        kp = (vp * n_motifs)(*[keys[m].data_ptr() for m in range(n_motifs)])
        sp = (vp * n_motifs)(*[sums[m].data_ptr() for m in range(n_motifs)])
        new = _timed(lambda: nv.check(getattr(nv.lib(), ins.ENTRY)(handles, n_motifs, tabs, max_weight, V, seq_offsets.ctypes.data,
                                                                 d_bases.data_ptr(), K, ioff.ctypes.data, itext.ctypes.data, 0, kp, sp,
                                                                 status.data_ptr(), _stream_ptr(None))), a.warmup, a.reps)
        # ---- the baseline: an edit and an item per (insert, base), in that order; the gap behind base o is named coord + 1
        cell_k = np.repeat(np.arange(K, dtype=np.int64), N)
        cell_n = np.tile(np.arange(N, dtype=np.int64), K)
        alt_len = np.repeat(np.array([len(i) for i in inserts], dtype=np.int64), N)
        Q = len(cell_n)
        alt_off = np.concatenate([[0], np.cumsum(alt_len)])
        assert int(alt_off[-1]) < 1 << 31
        alt_bytes = np.concatenate([np.tile(np.frombuffer(i, dtype=np.uint8), N) for i in inserts])
        d_edits = [up(seq_offsets, np.int64), d_bases, up(coord, np.int32), up(within[cell_n] + 1, np.int64), up(np.zeros(Q + 1), np.int32),
                   up(np.zeros(1), np.uint8), up(alt_off, np.int32), up(alt_bytes, np.uint8), up(cell_n // n, np.int32),
                   up(np.arange(Q), np.int32)]
        q_staged = (d_edits, d_tabs, max_weight, (V, Q, Q))
        rec = torch.zeros((n_motifs, Q, 4), dtype=torch.int64, device=dev)
        old = _timed(lambda: qv._enqueue(dms, q_staged, False, rec), a.warmup, a.reps)
        # ---- field for field: status applied in the low word and o + 1 above it, the keys packed, the sums
        cell = up((cell_k * N + cell_n) * 2, np.int64)
        fk, fs = keys.view(n_motifs, -1), sums.view(n_motifs, -1)
        same = bool((rec[:, :, 0] == up((within[cell_n] + 1) << 32, np.int64)[None, :]).all())
        same &= bool((rec[:, :, 2] == fs[:, cell]).all()) and bool((rec[:, :, 3] == fs[:, cell + 1]).all())
        packed = (fk[:, cell].to(torch.int64) & 0xffffffff) | ((fk[:, cell + 1].to(torch.int64) & 0xffffffff) << 32)
        same &= bool((rec[:, :, 1] == packed).all())
        below = new[2] < old[1]
        ok &= same and below
        names = ", ".join(i.decode() if len(i) <= 10 else f"a {len(i)}-mer" for i in inserts)
        lines.append(f"inserts ({names}): gfm_sequence_insertion_scan over {N} bases: median {new[0]:.3f} ms (min {new[1]:.3f}, max "
                     f"{new[2]:.3f}); gfm_graph_query_edits over the same {Q} insertions: median {old[0]:.3f} ms (min {old[1]:.3f}, max "
                     f"{old[2]:.3f}); {a.warmup} warm-ups, {a.reps} timed; ratio {old[0] / new[0]:.1f}x; the new entry's slowest pass "
                     f"is below the baseline's fastest: {below}; {Q * n_motifs / new[0] / 1e6:.3f} G insertions/s; the two agree on "
                     f"every item: {same}")
        if K == 4:
            staged = ss.stage(tables, seq_offsets, bases, (N, len(isc.COLUMNS)))
            floor = _timed(lambda: ss.enqueue(dms, staged, False, isc.ENTRY), a.warmup, a.reps)
            equal = True
            for k in range(4):
                cols = [isc.JUNCTION, isc.INS_A + k]
                equal &= bool((staged[4][:, :, cols] == keys[:, k]).all()) and bool((staged[5][:, :, cols] == sums[:, k]).all())
            lines.append(f"inserts (A, C, G, T): gfm_sequence_indel_scan on the same input (seven columns a base): median {floor[0]:.3f} ms "
                         f"(min {floor[1]:.3f}, max {floor[2]:.3f}); its JUNCTION and INS_A .. INS_T equal the insertion scan's: {equal}")
            ok &= equal
            del staged
        del rec, q_staged, d_edits, keys, sums
    for dm in dms:
        dm.release()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
