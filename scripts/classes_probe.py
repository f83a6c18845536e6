"""What the haplotype classes cost on the bench's graph, beside the best-score matrix they summarise:
synth.make_graph_index(R, 19) (5 096 haplotypes, a site every 32 bases, R regions of 200 bases).  Times, with the library's
own hipEvent pairs around every launch (gfm_graph_profile_enable), hc_key_kernel, hc_class_kernel (and the launches that redo
spilled regions) and hc_verify_kernel; with a hipEvent pair, gfm_graph_haplotype_classes and
gfm_graph_haplotype_class_records as a whole and, in the same process, gfm_graph_haplotype_scores alone over the same regions
(CTCF, W = 19, both strands); with wall clocks the whole compute_haplotype_classes call (device-to-host copies and the host
side included).  For hc_key_kernel the bytes it moves, counted from the shapes, over its time, beside the device's measured
stream rate (gfm_calibrate_stream).  One warm-up pass, then --reps timed passes, the calls alternating within a pass.

    python scripts/classes_probe.py [--regions 3000] [--reps 7] [--out profiles/classes_probe.txt]
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
    ap.add_argument("--regions", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif, calibrate_stream
    from grafimo_amd.extract_regions import DeviceGraph, _stream_ptr
    from grafimo_amd.haplotype_classes import compute_haplotype_classes, region_sites
    from grafimo_amd.motif_ops import build_motif_meme_host

    motif = build_motif_meme_host(os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]
    idx, regions = synth.make_graph_index(a.regions, 19)
    dg = DeviceGraph(idx)
    reg = np.asarray(regions, dtype=np.int64)
    starts, stops = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    R, H = len(regions), int(idx.n_haplotypes)
    hw = (H + 63) // 64
    lines = [f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {H} haplotypes ({hw} words), {R} regions of "
             f"{int(reg[0, 1] - reg[0, 0])} bases; {torch.cuda.get_device_name(0)}"]
    # the bytes of hc_key_kernel from the shapes: per region and bitset word the words of the used ALT slots of its sites, a
    # 16-byte site record per site of the index range (the range looks back by the longest deletion), an 8-byte key per haplotype
    pos = np.asarray(idx.pos, dtype=np.int64)
    max_del = int(np.asarray(idx.del_len).max()) if len(pos) else 0
    n_alts = np.asarray(idx.n_alts, dtype=np.int64)
    bit_bytes = rec_bytes = sites_total = 0
    for S, E in regions:
        t = region_sites(idx, S, E)
        sites_total += len(t)
        bit_bytes += int(n_alts[t].sum()) * 8 * hw
        lo, hi = np.searchsorted(pos, max(S, 0) - 1 - max_del), np.searchsorted(pos, min(E, len(idx.ref)))
        rec_bytes += int(hi - lo) * 16 * hw
    key_bytes = R * H * 8
    dm = DeviceMotif.lease(motif)
    vp = ctypes.c_void_p
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    d_class = torch.empty((R, H), dtype=torch.int32, device=dg.device)
    d_n = torch.empty(R, dtype=torch.int32, device=dg.device)
    status = torch.zeros(1, dtype=torch.int32, device=dg.device)
    keys = torch.zeros((R, H + 1), dtype=torch.int64, device=dg.device)
    over = torch.zeros(1, dtype=torch.int32, device=dg.device)
    t_key, t_class, t_spill, t_verify, t_entry, t_rec, t_scores, t_call = [], [], [], [], [], [], [], []
    n_spill_launches = 0
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        hc = compute_haplotype_classes(dg, reg, False, _Args())
        wall = time.perf_counter() - t
        nv.check(nv.lib().gfm_graph_profile_enable(dg._h, 1))
        torch.cuda.synchronize()
        ev[0].record()
        nv.check(nv.lib().gfm_graph_haplotype_classes(dg._h, R, nv.ptr(starts), nv.ptr(stops), 0, 64, 0, d_class.data_ptr(),
                                                      d_n.data_ptr(), status.data_ptr(), 0, _stream_ptr(None)))
        ev[1].record()
        off = torch.zeros(R + 1, dtype=torch.int64, device=dg.device)
        torch.cumsum(d_n, 0, out=off[1:])
        K = int(off[-1].item())
        count = torch.empty(K, dtype=torch.int32, device=dg.device)
        first = torch.empty(K, dtype=torch.int32, device=dg.device)
        torch.cuda.synchronize()
        ev[2].record()
        nv.check(nv.lib().gfm_graph_haplotype_class_records(R, H, d_class.data_ptr(), off.data_ptr(), None, 0, count.data_ptr(),
                                                            first.data_ptr(), None, _stream_ptr(None)))
        ev[3].record()
        torch.cuda.synchronize()
        ms = (ctypes.c_float * 64)()
        n = ctypes.c_int()
        nv.check(nv.lib().gfm_graph_profile_read(dg._h, ms, 64, ctypes.byref(n)))
        nv.check(nv.lib().gfm_graph_profile_enable(dg._h, 0))
        assert int(status.item()) == 0 and n.value >= 3 and (hc.class_of == d_class.cpu().numpy()).all()
        entry_ms, rec_ms = ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])
        ev[0].record()
        nv.check(nv.lib().gfm_graph_haplotype_scores(dg._h, (vp * 1)(dm.handle), 1, R, nv.ptr(starts), nv.ptr(stops), 0,
                                                     (vp * 1)(keys.data_ptr()), over.data_ptr(), 0, 0, _stream_ptr(None)))
        ev[1].record()
        torch.cuda.synchronize()
        if rep:                                               # (the first pass warms up: code objects, scratch, plans)
            t_key.append(ms[0]), t_class.append(ms[1]), t_verify.append(ms[n.value - 1])
            t_spill.append(sum(ms[2:n.value - 1]))
            n_spill_launches = n.value - 3
            t_entry.append(entry_ms), t_rec.append(rec_ms), t_scores.append(ev[0].elapsed_time(ev[1])), t_call.append(wall * 1e3)
    dm.release()
    us, nbytes = calibrate_stream(5, 256 << 20, False, 20)
    stream = nbytes / us / 1e3                               # GB/s
    med = statistics.median
    fmt = lambda v: f"median {med(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"     # noqa: E731
    moved = bit_bytes + rec_bytes + key_bytes
    rate = moved / med(t_key) / 1e6
    lines += [
        f"classes: {len(hc)} in all, {len(hc) / R:.1f} per region (largest {int(hc.n_classes.max())}), "
        f"{sites_total / R:.1f} sites per region; {n_spill_launches} launches for spilled regions; {a.reps} timed passes",
        f"hc_key_kernel: {fmt(t_key)}",
        f"  bytes from the shapes: {bit_bytes / 1e6:.1f} MB of bitset words + {rec_bytes / 1e6:.1f} MB of site records (scalar "
        f"loads, the same {rec_bytes // hw // 1000} kB for every word) + {key_bytes / 1e6:.1f} MB of keys written = "
        f"{moved / 1e6:.1f} MB -> {rate:.0f} GB/s, {rate / stream:.2f} of the measured stream rate "
        f"({stream:.0f} GB/s: gfm_calibrate_stream, 5 loads per store, {nbytes / 1e6:.0f} MB per launch)",
        f"hc_class_kernel: {fmt(t_class)}",
        f"hc_class_spill_kernel launches: {fmt(t_spill)}",
        f"hc_verify_kernel: {fmt(t_verify)}",
        f"gfm_graph_haplotype_classes, whole entry (host work, uploads and the wait for the spill list included): {fmt(t_entry)}",
        f"gfm_graph_haplotype_class_records: {fmt(t_rec)}",
        f"compute_haplotype_classes, whole call, wall ({4 * R * H / 1e6:.0f} MB class matrix to the host): {fmt(t_call)}",
        f"gfm_graph_haplotype_scores alone (CTCF, W = 19, both strands), same regions, same process: {fmt(t_scores)}; "
        f"classes entry / score matrix = {med(t_entry) / med(t_scores):.2f}",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
