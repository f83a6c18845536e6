"""What spelling the haplotype sequences costs: hseq_fill_kernel on the bench's panel (synth.make_graph_index: 5 096
haplotypes, a site every 32 bases around every region's core) over --regions regions of --length bases, for the pairs
compute_haplotype_sequences spells (every class's representative and the reference of every region).  Timed with the
library's own hipEvent pairs around its launches (gfm_graph_profile_enable); --warmup passes, then --reps timed ones, the
median reported.  Beside it the FLOOR, a plain device copy of the same number of bytes (torch.clone between two events), and
the BASELINE, the rate at which the tests' brute force (tests/variant_bruteforce.py spell) spells on the CPU.

    python scripts/hapseq_bench.py [--regions 1000] [--length 500] [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class _Args:
    threshold, noreverse, recomb, noqvalue, qvalueT = 1e-4, False, False, True, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-haplotypes", type=int, default=2, dest="cpu_haplotypes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd import synth
    from grafimo_amd.extract_regions import DeviceGraph, _stream_ptr
    from grafimo_amd.haplotype_classes import compute_haplotype_classes
    from variant_bruteforce import spell

    idx, core = synth.make_graph_index(a.regions, 19)
    pad = (a.length - (core[0][1] - core[0][0])) // 2
    regions = [(S - pad, S - pad + a.length) for S, _ in core]
    dg = DeviceGraph(idx)
    reg = np.asarray(regions, dtype=np.int64)
    starts, stops = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    R, H = len(regions), int(idx.n_haplotypes)
    hc = compute_haplotype_classes(dg, regions, False, _Args())
    k = np.diff(hc.offsets)
    seq_region = np.repeat(np.arange(R), k + 1).astype(np.int32)
    seq_hap = np.full(len(seq_region), -1, dtype=np.int32)
    is_ref = np.zeros(len(seq_region), dtype=bool)
    is_ref[np.cumsum(k + 1) - 1] = True
    seq_hap[~is_ref] = hc.first
    n = len(seq_region)
    dev = dg.device
    d_region, d_hap = torch.from_numpy(seq_region).to(dev), torch.from_numpy(seq_hap).to(dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    total = nv.c_i64(0)
    lib = nv.lib()
    head = (dg._h, R, nv.ptr(starts), nv.ptr(stops), n, d_region.data_ptr(), d_hap.data_ptr(), d_len.data_ptr())
    nv.check(lib.gfm_graph_haplotype_sequences(*head, None, 0, None, None, 0, 64, None, 0, total, _stream_ptr(None)))
    total = int(total.value)
    torch.cumsum(d_len, 0, out=off[1:])
    bases = torch.empty(total + 1, dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_measure, t_fill, t_copy = [], [], []
    for rep in range(a.warmup + a.reps):
        nv.check(lib.gfm_graph_profile_enable(dg._h, 1))
        nv.check(lib.gfm_graph_haplotype_sequences(*head, off.data_ptr(), total, bases.data_ptr(), None, 0, 64, keys.data_ptr(), 0,
                                                   None, _stream_ptr(None)))
        ms = (ctypes.c_float * 64)()
        got = ctypes.c_int()
        nv.check(lib.gfm_graph_profile_read(dg._h, ms, 64, ctypes.byref(got)))
        nv.check(lib.gfm_graph_profile_enable(dg._h, 0))
        assert got.value == 2, got.value
        torch.cuda.synchronize()
        ev[0].record()
        copy = bases.clone()
        ev[1].record()
        torch.cuda.synchronize()
        del copy
        if rep >= a.warmup:
            t_measure.append(ms[0]), t_fill.append(ms[1]), t_copy.append(ev[0].elapsed_time(ev[1]))
    # the baseline: the brute force spells whole chromosomes, a Python step per base
    t = time.perf_counter()
    spelt = sum(len(spell(idx, h)[0]) for h in range(min(a.cpu_haplotypes, H)))
    cpu_rate = spelt / (time.perf_counter() - t)
    med = statistics.median
    fmt = lambda v: f"median {med(v) * 1e3:.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})"     # noqa: E731
    fill_rate = total / med(t_fill) / 1e6
    lines = [
        f"graph: {len(idx.ref)} bases, {len(idx.pos)} sites, {H} haplotypes, {R} regions of {a.length} bases; "
        f"{torch.cuda.get_device_name(0)}",
        f"pairs: {n} sequences ({len(hc)} classes and {R} references), {total} bases, {total / n:.0f} per sequence; "
        f"{a.warmup} warm-ups, {a.reps} timed passes",
        f"hseq_measure_kernel: {fmt(t_measure)}",
        f"hseq_fill_kernel: {fmt(t_fill)} -> {fill_rate:.2f} GB/s of bases written",
        f"floor, torch.clone of {total} bytes: {fmt(t_copy)}; fill / floor = {med(t_fill) / med(t_copy):.1f}",
        f"baseline, the brute force's spell on the CPU: {cpu_rate / 1e6:.2f} Mbases/s over {spelt} bases; the fill kernel spells "
        f"{fill_rate * 1e9 / cpu_rate:.0f} times as fast",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    dg.close()


if __name__ == "__main__":
    main()
