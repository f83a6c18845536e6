"""Motif-set preparation one motif at a time against one device pass (GPU box).

Times, for BASELINE config 5's fifty motifs (synth.config_motifs(5), widths 8..25), with a device synchronisation at the
end of each variant:
  handles   DeviceMotif.from_motif per motif (a DP launch + a tail-table launch + a wait each)
            against DeviceMotif.create_many (one DP launch, one tail-table launch, one wait)
  pmfs      motif_processing.comp_pval_mat per motif against comp_pval_mat_many
The variants alternate, after one warm-up call of each; both sides' tables are compared byte for byte.

    python scripts/motif_set_probe.py [--reps 7] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/motif_set_probe.py --reps 3
    python scripts/motif_set_probe.py --summarize DIR     # (no GPU) the DP / tail-table dispatches of a trace by grid size

--summarize answers whether one motif's DP gets slower when the set's DPs run side by side: the one-workgroup dispatches
are the per-motif calls, the 50-workgroup ones the batches."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _motifs():
    from grafimo_amd import synth
    out = []
    for k, rec in enumerate(synth.config_motifs(5)):
        m = synth.motif_object(rec, f"C5_{k}")
        m.is_scaled = True          # what comp_pval_mat asks of a Motif
        out.append(m)
    return out


def _handles_one_by_one(motifs, torch):
    from grafimo_amd.device import DeviceMotif
    t = time.perf_counter()
    dms = [DeviceMotif.from_motif(m) for m in motifs]
    torch.cuda.synchronize()
    return time.perf_counter() - t, dms


def _handles_batched(motifs, torch):
    from grafimo_amd.device import DeviceMotif
    t = time.perf_counter()
    dms = DeviceMotif.create_many(motifs)
    torch.cuda.synchronize()
    return time.perf_counter() - t, dms


def _pmfs_one_by_one(motifs, torch):
    from grafimo_amd.motif_processing import comp_pval_mat
    t = time.perf_counter()
    out = [comp_pval_mat(m, False) for m in motifs]
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def _pmfs_batched(motifs, torch):
    from grafimo_amd.motif_processing import comp_pval_mat_many
    t = time.perf_counter()
    out = comp_pval_mat_many(motifs, False)
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def run(reps):
    import numpy as np
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    motifs = _motifs()
    variants = {"handles_one_by_one": _handles_one_by_one, "handles_batched": _handles_batched,
                "pmfs_one_by_one": _pmfs_one_by_one, "pmfs_batched": _pmfs_batched}
    samples = {k: [] for k in variants}
    for rep in range(reps + 1):                      # rep 0: warm-up, not kept
        names = list(variants) if rep % 2 == 0 else list(variants)[::-1]
        got = {}
        for name in names:
            dt, res = variants[name](motifs, torch)
            if rep:
                samples[name].append(dt * 1e3)
            got[name] = res
        a, b = got["handles_one_by_one"], got["handles_batched"]
        for x, y in zip(a, b):
            (px, tx), (py, ty) = x.tables(), y.tables()
            assert px.tobytes() == py.tobytes() and tx.tobytes() == ty.tobytes()
        for dm in a + b:
            dm.close()
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes()
                   for x, y in zip(got["pmfs_one_by_one"], got["pmfs_batched"]))
    out = dict(device=torch.cuda.get_device_name(0), motifs=len(motifs),
               widths=sorted({m.width for m in motifs}), reps=reps, tables_equal=True,
               ms={k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), all=[round(x, 3) for x in v])
                   for k, v in samples.items()})
    return out


def summarize(trace_dir):
    """per kernel (pvalue_dp_kernel, ptable_kernel) and grid size: dispatches and their durations"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    rows = {}
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r.get("Kernel_Name", "")
                kern = next((k for k in ("pvalue_dp_kernel", "ptable_kernel") if k in name), None)
                if kern is None:
                    continue
                grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
                wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 1024)
                wgs = grid // wg if grid >= wg else grid        # (work-items, or workgroups in some trace versions)
                us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                rows.setdefault((kern, wgs), []).append(us)
    lines = []
    for (kern, wgs), v in sorted(rows.items()):
        lines.append(f"{kern:18s} workgroups {wgs:4d}: {len(v):4d} dispatches, mean {statistics.mean(v):8.1f} us, "
                     f"median {statistics.median(v):8.1f}, min {min(v):8.1f}, max {max(v):8.1f}, sum {sum(v):9.1f} us")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarize", default=None, metavar="TRACE_DIR")
    a = ap.parse_args()
    if a.summarize:
        text = summarize(a.summarize)
    else:
        text = json.dumps(run(a.reps))
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
