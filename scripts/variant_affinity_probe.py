"""What the per-variant affinity table costs on the bench's graph, beside the per-variant effect table whose window list and
walk replay it shares: synth.make_graph_index(10 000, 19) (5 096 haplotypes, a site every 32 bases) with CTCF planted in 2 % of
the regions as bench.py's config 4 plants its motif.  Times, with wall clocks, the whole compute_variant_affinity call; with a
hipEvent pair after a warm-up, gfm_graph_variant_affinity alone and, in the same process on the same graph, motif and regions,
gfm_graph_variant_effects alone (both of its passes; a record buffer large enough that the call is not made twice).  Checks
that a slot has rows > 0 exactly where the effect table's key array holds a best k-mer, and that with all-ones weights
sum == rows in every slot.  The kernels' own times: run it under `rocprofv3 --kernel-trace --stats`.

    python scripts/variant_affinity_probe.py [--reps 20] [--out profiles/variant_affinity_probe.txt]
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
    threshold, noreverse, recomb, noqvalue, qvalueT = 1e-4, False, False, True, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import DeviceGraph, _stream_ptr
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.motif_ops import build_motif_meme_host
    from grafimo_amd.variant_affinity import compute_variant_affinity
    from grafimo_amd.variant_effects import VARIANT_REC_DTYPE

    motif = build_motif_meme_host(os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]
    probs = np.asarray(motif.count_matrix, dtype=np.float64)
    idx, regions = synth.make_graph_index(10_000, 19, plant=(probs, 0.02))
    dg = DeviceGraph(idx)
    reg = np.asarray(regions, dtype=np.int64)
    starts, stops = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    R, H, S = len(regions), int(idx.n_haplotypes), len(idx.pos)
    lines = [f"graph: {len(idx.ref)} bases, {S} sites, {H} haplotypes ({idx.hw} bitset words), {R} regions, W = 19, CTCF planted "
             f"in 2 % of the regions, both strands; {torch.cuda.get_device_name(0)}"]
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dm = DeviceMotif.lease(motif)
    vp = ctypes.c_void_p
    w, s_best = default_weights(dm)
    d_w = torch.from_numpy(w.view(np.int64)).to(dg.device)
    cap = 16 * S + 1024
    call, aff, eff = [], [], []
    n_aff, n_eff = ctypes.c_int64(), ctypes.c_int64()
    for rep in range(a.reps + 1):                          # (the first round is the warm-up)
        torch.cuda.synchronize()
        t = time.perf_counter()
        va = compute_variant_affinity(motif, dg, reg, False, _Args())
        t_call = time.perf_counter() - t
        sums = torch.zeros((S, 4, 2), dtype=torch.int64, device=dg.device)
        over = torch.zeros(1, dtype=torch.int32, device=dg.device)
        keys = torch.zeros(4 * S, dtype=torch.int64, device=dg.device)
        ctl = torch.zeros(2, dtype=torch.int64, device=dg.device)
        recs = torch.empty(cap * VARIANT_REC_DTYPE.itemsize, dtype=torch.uint8, device=dg.device)
        torch.cuda.synchronize()
        ev0.record()
        nv.check(nv.lib().gfm_graph_variant_affinity(dg._h, (vp * 1)(dm.handle), 1, (vp * 1)(d_w.data_ptr()), R, nv.ptr(starts),
                                                     nv.ptr(stops), 0, (vp * 1)(sums.data_ptr()), over.data_ptr(),
                                                     ctypes.byref(n_aff), 0, _stream_ptr(None)))
        ev1.record()
        torch.cuda.synchronize()
        t_aff = ev0.elapsed_time(ev1)
        ev0.record()
        nv.check(nv.lib().gfm_graph_variant_effects(dg._h, (vp * 1)(dm.handle), 1, R, nv.ptr(starts), nv.ptr(stops), 0,
                                                    (vp * 1)(keys.data_ptr()), (vp * 1)(recs.data_ptr()),
                                                    (ctypes.c_int64 * 1)(cap), (vp * 1)(ctl.data_ptr()), ctl.data_ptr() + 8,
                                                    ctypes.byref(n_eff), _stream_ptr(None)))
        ev1.record()
        torch.cuda.synchronize()
        t_eff = ev0.elapsed_time(ev1)
        assert int(over.item()) == 0 and int(ctl[1].item()) == 0 and int(ctl[0].item()) <= cap
        if rep:
            call.append(t_call * 1e3), aff.append(t_aff), eff.append(t_eff)
    s_h = sums.cpu().numpy().view(np.uint64)
    k_h = keys.cpu().numpy().reshape(S, 4)
    same_slots = bool(((s_h[:, :, 1] > 0) == (k_h != 0)).all())
    table_ok = bool((s_h[va.site, 0, 0] == va.ref_sum).all() and (s_h[va.site, va.allele, 0] == va.alt_sum).all())
    ones = compute_variant_affinity(motif, dg, reg, False, _Args(), weights=np.ones(dm.L, dtype=np.uint64))
    ones_ok = bool((ones.ref_sum == ones.ref_rows).all() and (ones.alt_sum == ones.alt_rows).all() and
                   (ones.ref_rows == va.ref_rows).all() and (ones.alt_rows == va.alt_rows).all())
    dm.release()
    med = statistics.median
    d = va.delta_log2_affinity
    lines.append(f"default weights: s_best = {s_best} of L - 1 = {dm.L - 1}; {len(va)} rows, {int(np.isfinite(d).sum())} with both "
                 f"sides, largest sum {int(s_h[:, :, 0].max())} (2^{np.log2(float(s_h[:, :, 0].max())):.1f}), most rows of a slot "
                 f"{int(s_h[:, :, 1].max())}, largest |delta_log2_affinity| {float(np.nanmax(np.abs(d))):.2f}")
    lines.append(f"rows > 0 exactly where gfm_graph_variant_effects keeps a best k-mer, all {4 * S} slots: {same_slots}; the table "
                 f"holds the device's sums: {table_ok}; all-ones weights give sum == rows and the same rows: {ones_ok}")
    lines.append(f"windows: {n_aff.value} distinct starts (variant affinity), {n_eff.value} (region, start) pairs (variant effects)")
    lines.append(f"compute_variant_affinity, whole call, wall: median {med(call):.1f} ms (min {min(call):.1f}, {a.reps} reps)")
    lines.append(f"gfm_graph_variant_affinity alone (window list, upload, one kernel), event-timed: median {med(aff):.3f} ms "
                 f"(min {min(aff):.3f})")
    lines.append(f"gfm_graph_variant_effects alone (window list, upload, two passes), same process, event-timed: median "
                 f"{med(eff):.3f} ms (min {min(eff):.3f}); affinity / effects = {med(aff) / med(eff):.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    assert same_slots and table_ok and ones_ok


if __name__ == "__main__":
    main()
