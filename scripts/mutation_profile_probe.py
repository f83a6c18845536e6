"""What the scan fold and the mutation profile cost.
  (a) the fold kernel alone: gfm_scan_fold over --motifs synthetic motifs x --rows rows of the mutation shape (5 columns, 4
      pairs), keys and sums made on the device (sites are rare, as in a real scan: a motif gains or loses in about 0.1 % of
      the cells), two hipEvents around the call's launches (one per 16 motifs), --warmup passes, then --reps timed ones.  Its bytes are counted
      from the shapes -- per launch of 16 motifs the state's 88 B x 4 per row read and written once and 16 x 12 B x 5 of input
      per row -- and set beside the device's measured stream rate (gfm_calibrate_stream, 5 loads per store) taken in the same run.
  (b) profile_sequences end to end against the only route there was before: mutation_scan.scan_sequences to the host, then the
      same reduction in numpy (vectorised over the cells, a pass per motif; its affinity champions compare long-double ratios,
      not exact products: it is the cheaper stand-in).  The same motifs (--motifs, of widths 11, 19 and 64) and the same
      --seqs random sequences of --length bases; the two alternate, one warm-up pass, then --reps timed ones, median / min / max
      of a host clock around calls that end with the results on the host.

    python scripts/mutation_profile_probe.py [--motifs 64] [--rows 1000000] [--seqs 2000] [--length 200] [--reps 5] [--warmup 2]
                                             [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return f"median {statistics.median(v):.3f} (min {min(v):.3f}, max {max(v):.3f})"


def numpy_profile(arrays, cutoffs, ptables):
    """the fold of per-motif host arrays in numpy, the motifs in id order (a tie keeps the earlier) -> (counts [N, 4, 2], site
    champion id + 1, affinity champion id + 1)"""
    import numpy as np
    N = len(arrays[0][0])
    counts = np.zeros((N, 4, 2), dtype=np.int64)
    site_id, aff_id = np.zeros((N, 4, 2), dtype=np.int64), np.zeros((N, 4, 2), dtype=np.int64)
    site_p = np.full((N, 4, 2), np.inf)
    ratio = np.zeros((N, 4, 2), dtype=np.longdouble)
    for m, (keys, sums) in enumerate(arrays):
        pt, cutoff = ptables[m], cutoffs[m]
        score = (keys >> 8).astype(np.int64) - 1
        site = (keys != 0) & (score >= cutoff)
        p = pt[np.clip(score, 0, len(pt) - 1)]
        sides = (site[:, 1:] & ~site[:, :1], site[:, :1] & ~site[:, 1:])
        for side, (hit, pv) in enumerate(zip(sides, (p[:, 1:], np.broadcast_to(p[:, :1], (N, 4))))):
            counts[:, :, side] += hit
            better = hit & (pv < site_p[:, :, side])
            site_p[:, :, side][better] = pv[better]
            site_id[:, :, side][better] = m + 1
        R, A = sums[:, :1].astype(np.longdouble), sums[:, 1:].astype(np.longdouble)
        with np.errstate(divide="ignore", invalid="ignore"):
            for side, (num, den) in enumerate(((A, R), (R, A))):
                q = np.where(num > den, num / den, 0)
                better = q > ratio[:, :, side]
                ratio[:, :, side][better] = q[better]
                aff_id[:, :, side][better] = m + 1
    return counts, site_id, aff_id


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--motifs", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--seqs", type=int, default=2000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import mutation_profile as mp
    from grafimo_amd import mutation_scan as ms
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif, calibrate_stream
    from grafimo_amd.graph_tables import group_by_width

    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [torch.cuda.get_device_name(0)]
    # ---- (a) the kernel alone
    M, rows, C, P = a.motifs, a.rows, len(ms.COLUMNS), len(mp.PAIRS)
    gen = torch.Generator(device=dev).manual_seed(5)
    L, cutoff = 19001, 1999
    keys = [((torch.randint(0, 2000, (rows, C), generator=gen, device=dev, dtype=torch.int32) + 1) << 8) | 129 for _ in range(M)]
    sums = [torch.randint(1 << 30, 1 << 50, (rows, C), generator=gen, device=dev, dtype=torch.int64) for _ in range(M)]
    tabs = [torch.from_numpy(np.sort(np.random.default_rng(k).random(L))[::-1].copy()).to(dev) for k in range(M)]
    ids, cuts = list(range(M)), [cutoff] * M
    state = mp.FoldState.zeros(rows, P)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    msec = []
    for rep in range(a.warmup + a.reps):
        for arr in state.arrays():
            arr.zero_()
        torch.cuda.synchronize()
        ev[0].record()
        mp.fold_columns(keys, sums, ids, cuts, tabs, mp.PAIRS, state)
        ev[1].record()
        torch.cuda.synchronize()
        if rep >= a.warmup:
            msec.append(ev[0].elapsed_time(ev[1]))
    launches = -(-M // 16)
    nbytes = rows * (launches * 2 * mp.STATE_BYTES * P + M * ms.BYTES_PER_BASE)
    moved = float((state.counts.sum(dim=2) > 0).float().mean())
    us, sbytes = calibrate_stream(5, 256 << 20, False, 20)
    stream = sbytes / us / 1e3
    rate = nbytes / statistics.median(msec) / 1e6
    lines.append(f"(a) gfm_scan_fold alone, {M} motifs x {rows} rows, {C} columns, {P} pairs, {launches} launches; {moved:.3f} of the cells "
                 f"have a gain or a loss: {_stats(msec)} ms; {a.warmup} warm-ups, {a.reps} timed")
    lines.append(f"    bytes from the shapes: rows x ({launches} x 2 x {mp.STATE_BYTES} x {P} state + {M} x {ms.BYTES_PER_BASE} input) = "
                 f"{nbytes / 1e9:.3f} GB -> {rate:.0f} GB/s; the device's measured stream rate {stream:.0f} GB/s (gfm_calibrate_stream, 5 "
                 f"loads per store, {sbytes / 1e6:.0f} MB a launch): {rate / stream:.2f} of it.  No LDS-staged variant was tried.")
    del keys, sums, tabs, state
    torch.cuda.empty_cache()
    # ---- (b) end to end against scan_sequences + numpy
    rng = np.random.default_rng(11)
    widths = [(11, 19, 64, 19)[k % 4] for k in range(M)]
    motifs = [synth.motif_object(synth.synthetic_motif(W, np.random.default_rng(100 + k), np.full(4, 0.25)), f"P{k}_{W}")
              for k, W in enumerate(widths)]
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=a.seqs * a.length)]
    off = np.arange(a.seqs + 1, dtype=np.int64) * a.length
    threshold = 1e-3
    by_width = group_by_width(motifs)
    numbers = [None] * M
    for i, m in enumerate(motifs):
        dm = DeviceMotif.lease(m)
        numbers[i] = (dm.pvalue_cutoff(threshold), dm.ptable_host().copy())
        dm.release()

    def new_route():
        return mp.profile_sequences(motifs, off, bases, threshold)

    def old_route():
        arrays = [None] * M
        for W, idxs in by_width.items():
            for i, got in zip(idxs, ms.scan_sequences([motifs[i] for i in idxs], off, bases)):
                arrays[i] = got
        t_scan = time.perf_counter()
        return numpy_profile(arrays, [n[0] for n in numbers], [n[1] for n in numbers]), t_scan

    new_s, old_s, scan_s = [], [], []
    for rep in range(1 + a.reps):
        t0 = time.perf_counter()
        state = new_route()
        t1 = time.perf_counter()
        (counts, site_id, aff_id), t_scan = old_route()
        t2 = time.perf_counter()
        if rep >= 1:
            new_s.append(t1 - t0), old_s.append(t2 - t1), scan_s.append(t_scan - t1)
    agree = (np.array_equal(counts, state.counts.astype(np.int64)), np.array_equal(site_id, state.site_motif.astype(np.int64)),
             float((aff_id == state.aff_motif.astype(np.int64)).mean()))
    N = len(bases)
    lines.append(f"(b) {M} motifs of widths 11 / 19 / 64 over {a.seqs} sequences of {a.length} bases = {N} bases, threshold {threshold}; 1 "
                 f"warm-up, {a.reps} timed, the two routes alternating")
    lines.append(f"    profile_sequences (the state, {mp.STATE_BYTES_PER_BASE * N / 1e6:.0f} MB, to the host): {_stats(new_s)} s")
    lines.append(f"    scan_sequences to the host ({M * ms.BYTES_PER_BASE * N / 1e6:.0f} MB) + the reduction in numpy: {_stats(old_s)} s, of "
                 f"which the scans and their copies {_stats(scan_s)} s")
    lines.append(f"    ratio of the medians {statistics.median(old_s) / statistics.median(new_s):.1f}x; the two agree on the counts: {agree[0]}, "
                 f"on the site champions: {agree[1]}, on {agree[2]:.6f} of the affinity champions (the numpy route rounds its ratios)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
