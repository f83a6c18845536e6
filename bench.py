#!/usr/bin/env python3
"""bench.py -- scored haplotype k-mers/s of the MI355X scoring path (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--config 2|3|4|5] [--full]

A plain run does what the headline figure needs and nothing else: it sets up, warms up, times the K steps, writes
--dump-outputs if asked and prints the result line.  --full adds every side measurement and self-check listed below
(CPU baselines, the oracle slice, the other configs and paths); the blocks of the line that a plain run leaves out are null.

With N > 1 and no WORLD_SIZE in the environment this process touches no GPU: it starts the N ranks itself
(python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same flags>),
passes their output through, prints rank 0's JSON line as its own LAST line and exits with the children's code.
Launched through torch.distributed.run directly (RANK / LOCAL_RANK / WORLD_SIZE set) it is one of the ranks.

One "step" = one pass of the hot path over one batch of synthetic k-mers resident in HBM:
score kernel (+ fused p-value selection) -> histogram reduction -> [all-reduce of the score histogram
across ranks] -> BH q-value table -> [selection on q for --qvalueT] -> [gather of the hit rows to rank 0].

Workloads (BASELINE.json configs; weak scaling: every rank scores its own shard, value = all ranks'
units / max-over-ranks time):
  --config 2  (default at N=1) CTCF MA0139.1 W=19, 10 000 synthetic 200-bp regions x 2 000 haplotype
              k-mers = 2.0e7 windows per GPU, p < 1e-4, q-values on.  Two input buffers are used in
              turn (380 MB each) so that no step re-reads what the 256 MiB Infinity Cache may still hold.
  --config 3  (default at N>1) the per-GPU shard of the 1e9-window scan: 1.25e8 windows, generated on
              the device.
  --config 4  W=30 JASPAR-style motif, 50 000 regions x 2 000 = 1.0e8 windows, both strands, --qvalueT 1e-4.
  --config 5  50 JASPAR-style PWMs, widths cycling 8..25, per-motif background, 1.0e8 windows per width
              (split over the ranks); motifs of one width share each read of the k-mers
              (gfm_score_kmers_multi); unit = one (k-mer, motif) pair.

Timing: W warm-up steps, then EXACTLY K timed steps, split into `--bursts` (default 1) bursts of nearly equal
length, each burst bracketed by a barrier + torch.cuda.synchronize() on both sides and reduced with MAX over the
ranks; `ms_per_step` is the MEDIAN over the bursts of burst time / its steps.  Rank 0 prints ONE JSON line.
With --dump-outputs DIR rank 0 also writes what the last timed step computed (see dump_outputs) as DIR/<name>.npy.
Beside the contract's fields the line carries
  roofline            the score kernel alone: HIP events riding on its dispatch packets, sampled inside the timed
                      bursts; `peak` = 8 TB/s vendor, `peak_measured` = this device's bare interleaved stream of
                      the same byte mix (gfm_calibrate_stream, --full), `frac_of_measured`; `traffic` from the committed
                      PMC passes (`traffic_source` says so);
  tail_ms             post kernel + [all-reduce] + q-table [+ selection on q] [+ gather], events on the tail stream;
  rank_ms_per_step    every rank's own median ms per step; rccl_world = dist.get_world_size();
  --full only:
  config.oracle_checked_rows   a slice of the last timed step's scores checked against the CPU oracle (0 without --full);
  product_paths       N > 1 (or --force-dist), configs 2 / 3: the fused graph path and the streamed scan under the
                      run's process group (--no-extras switches it off);
  --full, N = 1, default config only (each can be switched off):
  roofline_config3    >= 10 steps of the config-3 shard (1.25e8 windows generated on the device, `nt` stores: 477 MiB
                      of scores per launch, beyond any cache) -- also the 1-GPU point of the N > 1 curve
                      (`scaling_curve_point` names the curve's workload and this N's value on it at every N);
  roofline_config4/5  12 steps each of BASELINE configs[3] (W=30, --qvalueT) and configs[4] (50 PWMs, batched launches);
  sustained           >= 5 s of back-to-back steps, k-mers/s and min/median/max ms per 100 steps;
  extract             the k-mer extraction kernels on a synthetic graph at config-2 scale + extraction -> scoring;
  pcie_inclusive      the host-buffer form of the boundary (gfm_scan_host) over the same 2e7 k-mers, H2D included;
  e2e / e2e_config2   a TSV directory through compute_results' streamed scan (2e6 rows; 2e7 rows in 10 000 files);
  cpu_baseline / cpu_baseline_table   the CPU oracle's loop over TSV text on every host core (bounded sample).
"""
import argparse
import contextlib
import ctypes
import io
import json
import multiprocessing as mp
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E vendor peak (MI355X_MICROARCH.md), GB/s


def load_ctcf():
    """CTCF MA0139.1 through the package's own motif pipeline (MEME parser -> log-odds -> scaling)."""
    from grafimo_amd.motif_ops import build_motif_meme_host
    path = os.path.join(ROOT, "tests", "golden", "ref_data", "MA0139.1.meme")
    return build_motif_meme_host(path, "unfrm_dst", 0.1, False)[0]


# ---------------------------------------------------------------------------- N > 1: start the ranks
def launch_ranks(n: int, argv) -> int:
    """The driver calls `python bench.py --gpus N ...`; the ranks are children of this process, which has made
    no GPU call.  Their stdout passes through, except that JSON lines carrying "metric" are held back and the last
    one is printed at the very end, so that it is this process's last line."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True, bufsize=1)
    line_json = None
    for line in proc.stdout:
        s = line.strip()
        if s.startswith("{") and '"metric"' in s:
            try:
                json.loads(s)
                line_json = s
                continue
            except ValueError:
                pass
        sys.stdout.write(line)
        sys.stdout.flush()
    rc = proc.wait()
    if line_json is not None:
        print(line_json, flush=True)
    elif rc == 0:
        print("bench.py: the ranks printed no result line", file=sys.stderr)
        rc = 1
    return rc


def dry_run(args, rank, world):
    """--dry-run: the launcher and process-group plumbing without a GPU (gloo): rendezvous, one all-reduce, the
    per-rank list, rank 0's line.  What the CPU test-suite drives; measures nothing."""
    import torch
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    if args.dry_run_fail_rank is not None and rank == args.dry_run_fail_rank:
        sys.exit(3)
    one = torch.ones(1, dtype=torch.int64)
    ms = torch.tensor([float(rank + 1)], dtype=torch.float64)
    per_rank = [ms.clone() for _ in range(world)]
    if world > 1:
        dist.all_reduce(one)
        dist.all_gather(per_rank, ms)
        assert dist.get_world_size() == args.gpus
    assert int(one.item()) == world
    if rank == 0:
        print(json.dumps({"metric": "scored haplotype k-mers/sec", "value": None, "unit": "k-mers/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": "int32",
                          "data": "dry run: launcher and process-group plumbing only, no GPU work",
                          "rccl_world": world, "rank_ms_per_step": [float(t.item()) for t in per_rank],
                          # what every rank would hold of the sharded product paths (product_paths at N > 1): host-side plan
                          "product_paths": shard_plan(world),
                          "config": {"workload": "none (--dry-run)"}}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


# ---------------------------------------------------------------------------- CPU baselines
def _cpu_worker(args):
    text, W, sm, tab, min_val, scale, offset, table, budget_s = args
    from oracle import oracle as orc
    t = time.perf_counter()
    n = passes = 0
    while time.perf_counter() - t < budget_s:          # a bounded amount of CPU work per worker
        n += orc.score_tsv_text(text, W, sm, tab, min_val, scale, offset, table=table)[0]
        passes += 1
    return n, passes


def cpu_quota_cores():
    """CPU time the container may use per second of wall time, in cores (cgroup v2 cpu.max / v1 cfs quota); None: no
    quota.  The GPU boxes of round 3 show 256 hardware threads and a quota of 16: more runnable threads than that only
    burst until the period's allowance is used up and are then frozen to its end (cpu.stat nr_throttled)."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            quota, period = fh.read().split()[:2]
        return None if quota == "max" else float(quota) / float(period)
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fh:
            quota = float(fh.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
            period = float(fh.read())
        return None if quota <= 0 else quota / period
    except (OSError, ValueError):
        return None


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def cpu_baselines(mot, budget_s=8.0):
    """The reference's scoring loop restated (oracle/, the checker -- kind 'port'), timed on the host
    cores of this box: per TSV line the text handling of score_seqs (score_sequences.py:273-321) and
    compute_score_seq (:331-396).  'faithful' = the reference's two O(1000 W) f64 sums per k-mer,
    'table' = one p_table lookup instead (shows how much of the GPU/CPU ratio is algorithmic).  One
    forked worker per core like the reference's mp.Process fan-out (:133-147); every worker goes over
    its sample until `budget_s` seconds have passed."""
    from grafimo_amd import synth
    from oracle import oracle as orc
    orc.build()
    W = mot["width"]
    pmf = orc.comp_pval_mat(mot["sm"], mot["bg"])
    ptab = orc.p_table(pmf)
    sample = synth.make_batch(10, 2000, W, mot["probs"], synth.seed_for(0))
    threads = os.cpu_count() or 1
    quota = cpu_quota_cores()
    # one worker per core the container may actually use (a quota of 16 on a 256-thread host: 256 workers would share
    # the same 16 cores' worth of time and only add throttling stalls)
    cores = threads if quota is None else max(1, min(threads, int(np.ceil(quota))))
    out = {}
    for name, tab, table, rows in (("cpu_baseline", pmf, False, 1000), ("cpu_baseline_table", ptab, True, 20000)):
        text = synth.tsv_text(sample, np.arange(rows))
        job = (text, W, mot["sm"], tab, mot["min_val"], mot["scale"], mot["offset"], table, budget_s)
        t = time.perf_counter()
        with mp.get_context("fork").Pool(cores) as pool:
            res = pool.map(_cpu_worker, [job] * cores)
        wall = time.perf_counter() - t
        total = sum(r[0] for r in res)
        out[name] = {
            "value": total / wall, "unit": "k-mers/s", "cores": cores, "kind": "port",
            "host_threads": threads, "cpu_quota_cores": quota, "cpu_model": cpu_model(),
            "cache_resident": True,
            "sample": f"the first {rows} TSV rows ({len(text)} bytes of text: cache resident) of a batch of the same "
                      f"synthetic recipe, passed over again and again "
                      f"for {budget_s:.0f} s per worker ({min(r[1] for r in res)}..{max(r[1] for r in res)} passes), "
                      f"{cores} forked workers, text parse + "
                      + ("p_table lookup" if table else "per-row O(1000 W) tail sums")
                      + f" (oracle/grafimo_oracle.c orc_score_tsv_text), {wall:.1f} s wall",
        }
    return out


# ---------------------------------------------------------------------------- end to end (TSV -> hits)
def _tsv_worker(job):
    out_dir, r0, count, rows_per_region, W, probs, seed = job
    from grafimo_amd import synth
    batch = synth.make_batch(count, rows_per_region, W, probs, seed + r0, region_base=r0)
    synth.write_tsv_dir(batch, out_dir, regions_per_file=1)
    return len(batch)


def make_tsv_dir(regions, rows_per_region, W, probs, workers):
    """A synthetic TSV directory (one file per region) written by forked workers -- BEFORE anything
    touches the GPU.  -> (dir, rows)."""
    from grafimo_amd import synth
    need = 3 * regions * rows_per_region * (W + 75)      # ~92 bytes of text per row at W = 19, with headroom
    base = None
    cands = ("/dev/shm", tempfile.gettempdir())
    if os.environ.get("GRAFIMO_BENCH_TSV_BASE"):                  # measurement aid: where the TSV directories go
        cands = (os.environ["GRAFIMO_BENCH_TSV_BASE"],)
    for cand in cands:
        if os.path.isdir(cand) and os.access(cand, os.W_OK) and shutil.disk_usage(cand).free > need:
            base = cand
            break
    if base is None:
        return None, 0
    tmp = tempfile.mkdtemp(prefix="grafimo_e2e_", dir=base)
    per = max(1, min(100, regions // max(1, workers)))
    jobs = [(tmp, r0, min(per, regions - r0), rows_per_region, W, probs, synth.seed_for(7)) for r0 in range(0, regions, per)]
    with mp.get_context("fork").Pool(min(workers, len(jobs))) as pool:
        n = sum(pool.map(_tsv_worker, jobs))
    return tmp, n


def e2e_block(tmp, n_expected, W, dm):
    """A TSV directory through the pipeline behind compute_results (gfm_scan_tsv): parse threads (k-mer + line offset per
    row) -> pinned chunks -> hipMemcpyAsync -> score kernel per chunk -> q-table -> hits back, their columns read from
    the files.  `total_ms` is the median of BACK-TO-BACK scans -- what a caller that scans motif after motif gets; on a
    host with a CPU quota a scan that has a quota period to itself is given beside it, labelled.  `full_parse_ms`: the
    table form of the ingest (gfm_tsv_open: every column of every row converted) on the same files with the same thread
    request -- what the scan no longer does for rows that are not hits."""
    import ctypes
    import glob
    from grafimo_amd import _native as nv
    from grafimo_amd.score_sequences import StreamScan
    files = sorted(glob.glob(os.path.join(tmp, f"width_{W}", "*.tsv")))
    nbytes = sum(os.path.getsize(f) for f in files)
    threads = os.cpu_count() or 1
    quota = cpu_quota_cores()

    def scans(count, idle):
        runs = []
        for _ in range(count):
            if idle:
                time.sleep(idle)
            t = time.perf_counter()
            sc = StreamScan(dm, files, False, threads, 1e-4, False, True)
            runs.append((sc.stats.total_s, time.perf_counter() - t, sc.stats.parse_s, sc.stats.h2d_s, sc.stats.h2d_bytes,
                         sc.stats.tail_s, sc.n, sc.n_hits, sc.stats.n_chunks, sc.stats.parse_threads))
        return runs

    scans(1, 0.0)                            # the first call sizes the buffer pool
    back = sorted(scans(5, 0.0))
    total_s, wall, parse_s, h2d_s, h2d_bytes, tail_s, n, n_hits, n_chunks, pthreads = back[len(back) // 2]
    assert n == n_expected, (n, n_expected)
    out = {
        "rows": int(n), "tsv_bytes": int(nbytes), "files": len(files), "host_threads": threads,
        "cpu_quota_cores": quota, "parse_threads": int(pthreads), "hits": int(n_hits),
        "kmers_per_s": n / total_s, "h2d_GBps": h2d_bytes / h2d_s / 1e9,
        "total_ms": total_s * 1e3, "total_ms_runs": [round(r[0] * 1e3, 3) for r in back],
        "parse_ms_inside": parse_s * 1e3, "parse_cpu_ns_per_row": parse_s * pthreads / max(n, 1) * 1e9,
        "h2d_ms": h2d_s * 1e3, "after_parse_ms": tail_s * 1e3, "chunks": int(n_chunks),
        "path": "gfm_scan_tsv (grafimo_amd.score_sequences.StreamScan, what compute_results calls); total_ms = median of "
                "five back-to-back scans",
    }
    if quota is not None and nbytes > (1 << 30):
        # a container with a CPU quota freezes every thread once a 100 ms period's allowance is used up, and a scan of
        # this size needs a good part of one: with 0.15 s of idle before it a scan is charged for its own CPU time only
        fresh = sorted(scans(3, 0.15))
        out["total_ms_with_a_quota_period_to_itself"] = fresh[len(fresh) // 2][0] * 1e3
    arr = (ctypes.c_char_p * len(files))(*[f.encode() for f in files])
    ingest = []
    for _ in range(3):
        h, n_ = ctypes.c_void_p(), ctypes.c_int64()
        t = time.perf_counter()
        nv.check(nv.lib().gfm_tsv_open(arr, len(files), W, 0, threads, ctypes.byref(h), ctypes.byref(n_)))
        ingest.append(time.perf_counter() - t)
        nv.lib().gfm_tsv_close(h)
    out["full_parse_ms"] = float(np.median(ingest)) * 1e3
    return out


# ---------------------------------------------------------------------------- extraction (N = 1)
def extract_block(ctcf, dev, n_regions=10_000):
    """The extraction kernels (what replaces `vg find -K`) on a synthetic graph at config-2 scale:
    10 000 regions x 200 bp, one site per ~32 bp of which 6 % deletions, 5096 haplotypes; W = 19.  fused_ms = the
    kernels of gfm_graph_score (every walk scored on both strands where it is enumerated; HIP events, 10 calls);
    extract_plus_score_ms = the product entry point compute_results_from_graph (fused extraction + scoring -> q-table ->
    columns of the hit rows -> table) on the same graph; emit_ms = the materialising emit kernels of one plan, kept for
    write_region_tsvs."""
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd import synth
    from grafimo_amd.extract_regions import DeviceGraph, compute_results_from_graph
    from grafimo_amd.workflow import Findmotif
    W = ctcf.width
    idx, regions = synth.make_graph_index(n_regions, W)
    g = DeviceGraph(idx, dev)
    walls = []
    rows = None
    for _ in range(4):
        t = time.perf_counter()
        rows = g.extract(regions, W)
        torch.cuda.synchronize(dev)
        walls.append(time.perf_counter() - t)
    n = len(rows)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 10
    torch.cuda.synchronize(dev)
    t_enq = time.perf_counter()
    ev0.record()
    for _ in range(reps):
        nv.check(nv.lib().gfm_graph_emit(g._h, rows.kmers.data_ptr(), rows.start.data_ptr(), rows.stop.data_ptr(),
                                         rows.strand.data_ptr(), rows.freq.data_ptr(), rows.is_ref.data_ptr(),
                                         rows.region.data_ptr(), rows.walk.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream))
    ev1.record()
    # one emit is a memset, five kernels on two streams and four event operations: if the host takes longer to ENQUEUE a call
    # than the GPU to run it, emit_ms measures the host (round 4: 0.173 ms on an idle box, 0.451 ms on the driver's)
    emit_enqueue_ms = 1e3 * (time.perf_counter() - t_enq) / reps
    torch.cuda.synchronize(dev)
    emit_ms = ev0.elapsed_time(ev1) / reps
    out_bytes = n * (W + 8 + 8 + 1 + 8 + 1 + 4 + 4)     # k-mer + start, stop, strand, freq, is_ref, region, walk
    args_obj = Findmotif(cores=1, threshold=1e-4)
    # ---- the fused path (the product's default): gfm_graph_score alone (HIP events: tile ticket reset, the two score
    # kernels, the slab reduction), then the entry point as a caller sees it -- regions as an [n, 2] array, the way a caller
    # that scans motif after motif over one BED file holds them
    from grafimo_amd.device import DeviceMotif
    dm = DeviceMotif.lease(ctcf)
    reg = np.asarray(regions, dtype=np.int64)
    starts, stops = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    hist = torch.zeros(dm.L, dtype=torch.int64, device=dev)
    cut = dm.pvalue_cutoff(1e-4)
    for _ in range(3):
        g.score(dm, starts, stops, cut, hist=hist)
    torch.cuda.synchronize(dev)
    ev0.record()
    for _ in range(reps):
        g.score(dm, starts, stops, cut, hist=hist)
    ev1.record()
    torch.cuda.synchronize(dev)
    fused_ms = ev0.elapsed_time(ev1) / reps
    fused_rows = int(g.fused_results()[1])
    # graph_score_kernel alone (HIP events on its launch stream, inside the library) against its instruction-issue floor
    fused_roofline = None
    try:
        nv.check(nv.lib().gfm_graph_profile_enable(g._h, 1))
        for _ in range(20):
            g.score(dm, starts, stops, cut, hist=hist)
        torch.cuda.synchronize(dev)
        ms = np.empty(64, dtype=np.float32)
        k_ = ctypes.c_int(0)
        nv.check(nv.lib().gfm_graph_profile_read(g._h, nv.ptr(ms), 64, ctypes.byref(k_)))
        nv.check(nv.lib().gfm_graph_profile_enable(g._h, 0))
        fused_roofline = fused_issue_roofline(float(np.median(ms[:k_.value])) * 1e3)
    except Exception as e:                       # (a side measurement: it must not take the bench line with it)
        fused_roofline = {"error": f"{type(e).__name__}: {e}"}
    dm.release()
    runs, runs_rows = [], []
    hits = 0
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(12):
            t = time.perf_counter()
            df = compute_results_from_graph(ctcf, g, reg, False, args_obj)
            runs.append(time.perf_counter() - t)
            hits = len(df)
        for _ in range(4):
            t = time.perf_counter()
            df_m = compute_results_from_graph(ctcf, g, regions, False, args_obj, fused=False)
            runs_rows.append(time.perf_counter() - t)
    same = len(df_m) == len(df) and bool((df_m["matched_sequence"].to_numpy() == df["matched_sequence"].to_numpy()).all()) \
        and bool((df_m["start"].to_numpy() == df["start"].to_numpy()).all()) \
        and bool((df_m["haplotype_frequency"].to_numpy() == df["haplotype_frequency"].to_numpy()).all())
    # ---- the reference's unchanged call sequence (grafimo.py:176-183): scan_graph, then compute_results per motif.
    # (a) our compute_results as the consumer: scan_graph leaves a manifest, no row exists anywhere; (b) GRAFIMO's own
    # compute_results as the consumer: the TSV files, written by the library's host threads (gfm_graph_write_tsvs)
    scan_e2e = None
    try:
        scan_e2e = scan_graph_block(ctcf, idx, regions, rows, g)
    except Exception as e:                       # (a side measurement: it must not take the bench line with it)
        scan_e2e = {"error": f"{type(e).__name__}: {e}"}
    g.close()
    e2e = 1e3 * float(np.median(runs[2:]))
    # ---- windows of very many walks (16 neighbouring biallelic SNPs inside one 30-mer: 2^16 walks per window): they leave
    # graph_score_kernel for graph_heavy_kernel, whose wavefronts share a window's walks (one wavefront had them all: 78 ms)
    heavy = None
    try:
        from grafimo_amd.extract_regions import GraphIndex
        rng = np.random.default_rng(3)
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        href = acgt[rng.integers(0, 4, 600)]
        hpos = np.arange(300, 316, dtype=np.int32)
        halt = np.zeros((16, 3), np.uint8)
        halt[:, 0] = np.where(href[hpos] == ord("A"), ord("C"), ord("A"))
        hg = DeviceGraph(GraphIndex("c", href, hpos, np.ones(16, np.uint8), halt, None, 0), dev)
        rec = synth.synthetic_motif(30, np.random.default_rng(5), np.full(4, 0.25))
        hdm = DeviceMotif(rec["sm"], rec["bg"], rec["min_val"], rec["scale"], rec["offset"])
        hs, he = np.array([0, 270], dtype=np.int64), np.array([200, 360], dtype=np.int64)
        hh = torch.zeros(hdm.L, dtype=torch.int64, device=dev)
        for _ in range(3):
            hg.score(hdm, hs, he, hdm.pvalue_cutoff(1e-9), hist=hh)
        torch.cuda.synchronize(dev)
        ev0.record()
        for _ in range(reps):
            hg.score(hdm, hs, he, hdm.pvalue_cutoff(1e-9), hist=hh)
        ev1.record()
        torch.cuda.synchronize(dev)
        hrows = int(hg.fused_results()[1])
        heavy = {"what": "16 neighbouring SNPs inside one 30-mer (windows of up to 2^16 walks)", "rows": hrows,
                 "fused_ms": ev0.elapsed_time(ev1) / reps, "rows_per_s": hrows / (ev0.elapsed_time(ev1) / reps * 1e-3)}
        hdm.close()
        hg.close()
    except Exception as e:                       # (a side measurement: it must not take the bench line with it)
        heavy = {"error": f"{type(e).__name__}: {e}"}
    return {
        "heavy_windows": heavy, "scan_graph_e2e": scan_e2e,
        "regions": n_regions, "region_bp": 200, "width": W, "sites": int(len(idx.pos)),
        "deletions": int((idx.del_len > 0).sum()), "haplotypes": idx.n_haplotypes, "rows": int(n),
        "fused_ms": fused_ms, "rows_per_s_fused": fused_rows / (fused_ms * 1e-3), "roofline": fused_roofline,
        "extract_plus_score_ms": e2e, "rows_per_s_extract_plus_score": n / (e2e * 1e-3), "hits_p1e-4": int(hits),
        "fused_equals_materialised": same,
        "emit_ms": emit_ms, "emit_host_enqueue_ms": emit_enqueue_ms, "rows_per_s_emit": n / (emit_ms * 1e-3),
        "written_bytes": int(out_bytes), "written_GBps": out_bytes / (emit_ms * 1e-3) / 1e9,
        "frac": out_bytes / (emit_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "peak": HBM_PEAK_GBS,
        "plan_plus_emit_wall_ms": 1e3 * float(np.median(walls[1:])),
        "extract_plus_score_materialised_ms": 1e3 * float(np.median(runs_rows[1:])),
        "path": "compute_results_from_graph = gfm_graph_score (walks scored where they are enumerated: no row reaches HBM) + "
                "q-table + gfm_graph_annotate (columns of the hit rows only) -> table; fused_ms = gfm_graph_score alone; "
                "emit_ms / written_GBps / frac = the materialising gfm_graph_emit kept for write_region_tsvs",
    }


PRODUCT_PATHS_TIMEOUT_S = 300      # process-group timeout of the bench's ranks
GRAPH_REGIONS_PER_RANK = 4000      # product_paths: regions of the synthetic chromosome per rank (weak scaling)
SCAN_REGIONS_PER_RANK = 400        # ... and TSV files (2 000 rows each) per rank


def shard_plan(world, cores_flag=0):
    """What every rank of an N-rank run holds of the two sharded product paths -- computable without a GPU (bench.py
    --dry-run prints it; tests/test_bench_launcher.py checks it): regions and site records of the graph per rank
    (extract_regions.shard_index), TSV files and parse threads per rank (distributed.shard_files / _parse_threads)."""
    from grafimo_amd import synth
    from grafimo_amd.distributed import _parse_threads, shard_bounds
    from grafimo_amd.extract_regions import shard_index
    idx, regions = synth.make_graph_index(min(GRAPH_REGIONS_PER_RANK, 500) * world, 19, with_counts=False)
    reg = np.asarray(regions, dtype=np.int64)
    sites, n_reg = [], []
    for r in range(world):
        lo, hi = shard_bounds(len(reg), world, r)
        n_reg.append(int(hi - lo))
        sites.append(int(len(shard_index(idx, reg[lo:hi, 0], reg[lo:hi, 1]).pos)) if world > 1 else int(len(idx.pos)))
    return {"graph_path": {"regions_per_rank": n_reg, "sites_per_rank": sites, "sites_total": int(len(idx.pos))},
            "streamed_scan": {"files_per_rank": [int(shard_bounds(SCAN_REGIONS_PER_RANK * world, world, r)[1] -
                                                     shard_bounds(SCAN_REGIONS_PER_RANK * world, world, r)[0]) for r in range(world)],
                              "parse_threads_per_rank": [_parse_threads(cores_flag, world)] * world,
                              "host_cores": os.cpu_count() or 1}}


def product_paths_block(ctcf, dev, rank, world):
    """N > 1: the fused graph path (one motif, a motif set) and the streamed scan under the run's process group (weak scaling:
    every rank brings GRAPH_REGIONS_PER_RANK regions / SCAN_REGIONS_PER_RANK files).  Rank 0 reports; every rank takes part.
    Three STAGES, each a sequence of collectives.  A stage that raises on this rank is caught here, and the decision to go on is
    COLLECTIVE: after every stage the ranks all-reduce(MAX) a failure flag -- a failure anywhere ends the block on
    every rank together, with the stage's error in the line, and the main bench's collectives stay in step.  (A rank that fails
    while its peers are still inside the stage's own collectives cannot be helped from here: the process group's timeout,
    PRODUCT_PATHS_TIMEOUT_S, ends the run instead of a hang.)"""
    import shutil
    import tempfile
    import torch
    import torch.distributed as dist
    from grafimo_amd import synth
    from grafimo_amd.distributed import compute_results_sharded
    from grafimo_amd.extract_regions import (_SHARD_GRAPHS, compute_results_from_graph, compute_results_from_graph_many,
                                             drop_graph_cache)
    from grafimo_amd.workflow import Findmotif
    W = ctcf.width
    out = {}
    sink = io.StringIO()
    state = {}

    def stage_graph():
        # the HOST index is handed over; a rank uploads the part of the graph its regions can meet
        idx, regions = synth.make_graph_index(GRAPH_REGIONS_PER_RANK * world, W)
        reg = np.asarray(regions, dtype=np.int64)
        wf = Findmotif(cores=1, threshold=1e-4)
        state.update(idx=idx, reg=reg, wf=wf)
        ts = []
        with contextlib.redirect_stdout(sink):
            for _ in range(8):
                dist.barrier()
                t = time.perf_counter()
                df = compute_results_from_graph(ctcf, idx, reg, False, wf)
                torch.cuda.synchronize(dev)
                ts.append(time.perf_counter() - t)
        mine = [g for g in _SHARD_GRAPHS.values() if g._source is idx]
        n_rows = torch.tensor([int(mine[0].fused_results()[1]) if mine else 0], dtype=torch.int64, device=dev)
        sites = torch.tensor([len(mine[0].index.pos) if mine else 0], dtype=torch.int64, device=dev)
        t_max = torch.tensor([float(np.median(ts[2:]))], dtype=torch.float64, device=dev)
        dist.all_reduce(n_rows)
        dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
        per_rank_sites = [torch.zeros_like(sites) for _ in range(world)]
        dist.all_gather(per_rank_sites, sites)
        state.update(df=df, n_rows=int(n_rows.item()))
        return {"regions": int(len(reg)), "rows": int(n_rows.item()), "compute_results_from_graph_ms": 1e3 * float(t_max.item()),
                "rows_per_s": int(n_rows.item()) / float(t_max.item()), "hits": int(len(df)) if df is not None else None,
                "sites_total": int(len(idx.pos)), "sites_per_rank": [int(x.item()) for x in per_rank_sites],
                "what": "compute_results_from_graph(motif, GraphIndex, regions) on every rank: regions sharded, each rank "
                        "uploads its shard of the graph (shard_index), one all-reduce of the histogram, hit rows gathered; "
                        "median of 6 calls, MAX over ranks"}

    def stage_graph_many():
        # the same graph, a motif SET: three CTCF-width motifs share one enumeration per rank, their histograms cross the
        # ranks as ONE [3, L] all-reduce
        idx, reg, wf, df = state["idx"], state["reg"], state["wf"], state["df"]
        rng = np.random.default_rng(11)
        trio = [ctcf] + [synth.motif_object(synth.synthetic_motif(W, rng, np.full(4, 0.25)), f"S{k}") for k in range(2)]
        ts = []
        with contextlib.redirect_stdout(sink):
            for _ in range(6):
                dist.barrier()
                t = time.perf_counter()
                tabs = compute_results_from_graph_many(trio, idx, reg, False, wf)
                torch.cuda.synchronize(dev)
                ts.append(time.perf_counter() - t)
        t_many = torch.tensor([float(np.median(ts[2:]))], dtype=torch.float64, device=dev)
        dist.all_reduce(t_many, op=dist.ReduceOp.MAX)
        drop_graph_cache()
        return {"motifs": 3, "regions": int(len(reg)), "compute_results_from_graph_many_ms": 1e3 * float(t_many.item()),
                "pairs_per_s": 3 * state["n_rows"] / float(t_many.item()),
                "hits": [int(len(t_)) for t_ in tabs] if tabs[0] is not None else None,
                "first_table_equals_single_call": bool(tabs[0] is None or (len(tabs[0]) == len(df) and bool(
                    (tabs[0]["matched_sequence"].to_numpy() == df["matched_sequence"].to_numpy()).all()))),
                "what": "compute_results_from_graph_many([CTCF, 2 synthetic W=19 PWMs], GraphIndex, regions) on every "
                        "rank: one enumeration of a rank's walks for the three motifs, one [3, L] all-reduce; median of 4, "
                        "MAX over ranks"}

    def stage_scan():
        # every rank writes its own files, then compute_results_sharded over the whole directory
        tmp = tempfile.mkdtemp(prefix="gfm_bench_scan_") if rank == 0 else None
        box = [tmp]
        dist.broadcast_object_list(box, src=0)
        tmp = state["tmp"] = box[0]
        batch = synth.make_batch(SCAN_REGIONS_PER_RANK, 2000, W, np.asarray(ctcf.count_matrix, dtype=np.float64), synth.seed_for(2, rank),
                                 region_base=rank * SCAN_REGIONS_PER_RANK)       # (file names are made from the region numbers)
        synth.write_tsv_dir(batch, tmp)
        dist.barrier()
        wf = Findmotif(cores=0, threshold=1e-4)
        ts = []
        with contextlib.redirect_stdout(sink):
            for _ in range(5):
                dist.barrier()
                t = time.perf_counter()
                df = compute_results_sharded(ctcf, tmp, False, wf)
                ts.append(time.perf_counter() - t)
        t_max = torch.tensor([float(np.median(ts[1:]))], dtype=torch.float64, device=dev)
        dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
        n = SCAN_REGIONS_PER_RANK * 2000 * world
        return {"files": SCAN_REGIONS_PER_RANK * world, "rows": n, "compute_results_sharded_ms": 1e3 * float(t_max.item()),
                "rows_per_s": n / float(t_max.item()), "hits": int(len(df)) if df is not None else None,
                "what": "compute_results_sharded over one directory: files split over the ranks, gfm_scan_tsv_begin per "
                        "rank, all-reduce of the histogram, gfm_scan_tsv_finish, hit rows gathered; median of 4, MAX over ranks"}

    try:
        out = run_stages_together((("graph_path", stage_graph), ("graph_path_many", stage_graph_many), ("streamed_scan", stage_scan)), dev)
    finally:
        drop_graph_cache()
        if rank == 0 and state.get("tmp"):
            shutil.rmtree(state["tmp"], ignore_errors=True)
    return out


def run_stages_together(stages, device):
    """Runs (name, function) stages on every rank of the default process group; a stage's exception is caught on the rank that
    raised it, and after EVERY stage the ranks all-reduce(MAX) a failure flag: a failure anywhere stops the sequence on every rank
    together (its stage reads {"error": ...}, "stopped_after" names it), so that whatever follows the block stays in step.
    -> {name: result}  (tests/test_bench_launcher.py drives it with two gloo ranks and a stage that fails on one of them)"""
    import torch
    import torch.distributed as dist
    out = {}
    for name, fn in stages:
        err = None
        try:
            out[name] = fn()
        except Exception as e:                   # (decided together, below)
            err = f"{type(e).__name__}: {e}"
        flag = torch.tensor([1 if err else 0], dtype=torch.int64, device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if int(flag.item()):
            out[name] = {"error": err or "another rank failed in this stage"}
            out["stopped_after"] = name
            break
    return out


def fused_issue_roofline(kernel_us):
    """graph_score_kernel is integer / LDS work that moves ~40 MB per launch: its bounds are the CU's own units, not HBM.  A
    wave64 vector instruction occupies a SIMD for two cycles (MI355X_MICROARCH.md: SIMD-32 lanes), a CU has four SIMDs, ONE
    scalar unit and ONE LDS array: floor = max(VALU x 2 / (4 x CUs), SALU / CUs, LDS-array cycles / CUs) / clock, with the
    counts of the committed rocprofv3 --pmc passes (profiles/pmc_fused.json, valid while the kernel's sources hash as they
    did; SQ_LDS_IDX_ACTIVE = all LDS-array cycles, bank conflicts included)."""
    import hashlib
    path = os.path.join(ROOT, "profiles", "pmc_fused.json")
    out = {"bound": "valu_issue", "kernel": "graph_score_kernel", "kernel_us": kernel_us, "clock_ghz": 2.4, "cus": 256}
    try:
        rec = json.load(open(path))
        src = b"".join(open(os.path.join(ROOT, f), "rb").read() for f in rec["kernel_source_files"])
        fresh = hashlib.sha256(src).hexdigest()[:16] == rec["kernel_source_sha16"]
        floors = {"valu_issue": rec["insts_valu"] * 2.0 / (4 * 256) / 2.4e3, "salu_issue": rec["insts_salu"] / 256.0 / 2.4e3,
                  "lds": (rec.get("lds_idx_active_cycles") or 0.0) / 256.0 / 2.4e3}
        bound = max(floors, key=floors.get)
        out.update({"bound": bound, "insts": {"valu": rec["insts_valu"], "salu": rec["insts_salu"], "lds": rec["insts_lds"]},
                    "lds_array_cycles": rec.get("lds_idx_active_cycles"),
                    "floor_us": floors[bound], "valu_floor_us": floors["valu_issue"], "salu_floor_us": floors["salu_issue"],
                    "lds_floor_us": floors["lds"], "frac": floors[bound] / kernel_us if kernel_us > 0 else None,
                    "counters": rec["source"] if fresh else "profiles/pmc_fused.json is STALE: the fused kernels' sources changed "
                                                              "since its counters were taken (the floor is that of the older kernel)",
                    "counters_fresh": fresh})
    except Exception as e:
        out["error"] = f"{type(e).__name__}: {e}"
    return out


def extract_config_block(cfg, dev):
    """BASELINE configs[3] / configs[4] THROUGH THE GRAPH (the fused path): 50 000 regions x 200 bp of the synthetic
    chromosome.  cfg 4: one W = 30 motif, both strands, --qvalueT 1e-4.  cfg 5: 50 PWMs of widths 8..25 -- in ONE
    compute_results_from_graph_many call (up to three motifs of a width per enumeration) against 50 single calls."""
    import torch
    from grafimo_amd import synth
    from grafimo_amd.extract_regions import DeviceGraph, compute_results_from_graph, compute_results_from_graph_many
    from grafimo_amd.workflow import Findmotif
    mots = synth.config_motifs(cfg)
    motifs = [synth.motif_object(m, f"M{i}") for i, m in enumerate(mots)]
    n_regions = 50_000
    # cfg 4: 2 % of the regions hold a sample of the motif's own PWM columns (SURVEY 8d's recipe for the resident batches), so
    # that q < 1e-4 reports rows and the call's annotate / table half has work (VERDICT r5 Weak #1 ii: hits_q1e-4 was 0)
    idx, regions = synth.make_graph_index(n_regions, max(m.width for m in motifs),
                                          plant=(mots[0]["probs"], 0.02) if cfg == 4 else None)
    g = DeviceGraph(idx, dev)
    reg = np.asarray(regions, dtype=np.int64)
    sink = io.StringIO()
    out = {"regions": n_regions, "region_bp": 200, "sites": int(len(idx.pos)), "motifs": len(motifs)}
    with contextlib.redirect_stdout(sink):
        if cfg == 4:
            wf = Findmotif(threshold=1e-4, qval_t=True)
            ts = []
            for _ in range(8):
                t = time.perf_counter()
                df = compute_results_from_graph(motifs[0], g, reg, False, wf)
                ts.append(time.perf_counter() - t)
            n_rows = int(g.fused_results()[1])
            ms = 1e3 * float(np.median(ts[2:]))
            out.update({"width": motifs[0].width, "rows": n_rows, "compute_results_from_graph_ms": ms,
                        "rows_per_s": n_rows / (ms * 1e-3), "hits_q1e-4": int(len(df)),
                        "what": "BASELINE configs[3] through the graph: W = 30, 50 000 regions, both strands, --qvalueT 1e-4"})
        else:
            wf = Findmotif(threshold=1e-4)
            ts_many, ts_single = [], []
            for _ in range(4):
                t = time.perf_counter()
                tabs = compute_results_from_graph_many(motifs, g, reg, False, wf)
                ts_many.append(time.perf_counter() - t)
            for _ in range(2):
                t = time.perf_counter()
                singles = [compute_results_from_graph(m, g, reg, False, wf) for m in motifs]
                ts_single.append(time.perf_counter() - t)
            same = all(len(a) == len(b) and bool((a["matched_sequence"].to_numpy() == b["matched_sequence"].to_numpy()).all())
                       and bool(np.array_equal(a["q-value"].to_numpy(), b["q-value"].to_numpy())) for a, b in zip(tabs, singles))
            many_ms, single_ms = 1e3 * float(np.median(ts_many[1:])), 1e3 * float(min(ts_single))
            # the DEVICE passes alone (the tables above are dominated by what the host does with 440 000 hit rows: records back,
            # 50 DataFrames): gfm_graph_score_multi per group of <= 3 motifs of a width against gfm_graph_score per motif, HIP
            # events around the enqueued calls, histograms and hit lists as in the product
            from grafimo_amd.device import DeviceMotif
            by_w = {}
            for i, m in enumerate(motifs):
                by_w.setdefault(m.width, []).append(i)
            dms = [DeviceMotif.from_motif(m) for m in motifs]
            hists = [torch.zeros(d.L, dtype=torch.int64, device=dev) for d in dms]
            cuts = [d.pvalue_cutoff(1e-4) for d in dms]
            starts, stops = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

            def pass_many():
                for w, idxs in by_w.items():
                    for c0 in range(0, len(idxs), 3):
                        sl = idxs[c0:c0 + 3]
                        g.score_many([dms[i] for i in sl], starts, stops, [cuts[i] for i in sl], [hists[i] for i in sl],
                                     slots=list(range(len(sl))))

            def pass_single():
                for w, idxs in by_w.items():
                    for i in idxs:
                        g.score(dms[i], starts, stops, cuts[i], hist=hists[i])

            for fn in (pass_many, pass_single):          # warm: plans of every width, kernels loaded
                fn()
            torch.cuda.synchronize(dev)
            ev[0].record(); pass_many(); ev[1].record()
            ev[2].record(); pass_single(); ev[3].record()
            torch.cuda.synchronize(dev)
            dev_many, dev_single = ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])
            rows_per_motif = int(g.fused_results()[1])
            for d in dms:
                d.close()
            out.update({"widths": sorted({m.width for m in motifs}), "many_ms": many_ms, "fifty_single_calls_ms": single_ms,
                        "speedup_vs_single_calls": single_ms / many_ms, "tables_equal": same, "hits": int(sum(len(t_) for t_ in tabs)),
                        "device_pass_many_ms": dev_many, "device_pass_fifty_single_ms": dev_single,
                        "device_speedup_vs_single_passes": dev_single / dev_many, "rows_last_width": rows_per_motif,
                        "what": "BASELINE configs[4] through the graph: 50 PWMs (W = 8..25), 50 000 regions; many = one "
                                "compute_results_from_graph_many call (<= 3 motifs of a width per enumeration, gfm_graph_score_multi), "
                                "against one compute_results_from_graph call per motif; device_pass_* = the scoring passes alone "
                                "(HIP events: the tile-table switches between widths included), many_ms / fifty_single_calls_ms = "
                                "whole calls with their tables (host work on ~9 000 hit rows per motif dominates both)"})
    g.close()
    return out


def scan_graph_block(ctcf, idx, regions, rows, g):
    """scan_graph(widths, workflow, debug) + compute_results(motif, loc, debug, workflow), the two calls of
    grafimo.findmotif (grafimo.py:176-179) with their reference signatures, on the extract block's graph."""
    import shutil
    import tempfile
    from grafimo_amd import extract_regions as xr
    from grafimo_amd.score_sequences import compute_results
    from grafimo_amd.workflow import Findmotif
    W = ctcf.width
    tmp = tempfile.mkdtemp(prefix="gfm_bench_scan_")
    out = {}
    old_mode = os.environ.get("GRAFIMO_SCAN_OUTPUT")
    try:
        idx.save(os.path.join(tmp, "chr22"))
        bed = os.path.join(tmp, "regions.bed")
        with open(bed, "w") as fh:
            fh.write("".join(f"chr22\t{s}\t{e}\n" for s, e in regions))
        wf = Findmotif(cores=min(32, os.cpu_count() or 1), threshold=1e-4, graph_genome_dir=tmp, bedfile=bed, chroms_prefix="chr")
        sink = io.StringIO()
        # (a) manifest: scan_graph does not touch the GPU; the first compute_results loads and uploads the graph
        os.environ["GRAFIMO_SCAN_OUTPUT"] = "manifest"
        with contextlib.redirect_stdout(sink):
            t_scans = []
            for _ in range(3):                               # (the first call of a process also imports the XG / GBWT reader)
                t = time.perf_counter()
                loc = xr.scan_graph({W}, wf, False)
                t_scans.append(time.perf_counter() - t)
                if len(t_scans) < 3:
                    shutil.rmtree(loc)
            t_scan = float(np.median(t_scans))
            calls = []
            for _ in range(24):                              # "motif after motif" over one scan_graph result
                t = time.perf_counter()
                df = compute_results(ctcf, loc, False, wf)
                calls.append(time.perf_counter() - t)
        shutil.rmtree(loc)
        xr.drop_graph_cache()
        out["manifest"] = {"scan_graph_ms": 1e3 * t_scan, "scan_graph_first_ms": 1e3 * t_scans[0], "first_compute_results_ms": 1e3 * calls[0],
                           "compute_results_ms": 1e3 * float(np.median(calls[2:])), "hits": int(len(df)), "rows_written": 0,
                           "what": "scan_graph leaves a manifest (graph index, regions, widths); compute_results runs "
                                   "compute_results_from_graph; first call = + GraphIndex.load + upload of the graph"}
        # (b) TSV files for GRAFIMO's own compute_results: extraction + native writer
        os.environ["GRAFIMO_SCAN_OUTPUT"] = "tsv"
        with contextlib.redirect_stdout(sink):
            t = time.perf_counter()
            loc = xr.scan_graph({W}, wf, False)
            t_tsv = time.perf_counter() - t
        n_files = len(os.listdir(os.path.join(loc, f"width_{W}")))
        shutil.rmtree(loc)
        # the writer alone on the extract block's rows (round 4: a Python row loop, 4 us a row)
        wr = {}
        for name, node_paths in (("with_node_paths", True), ("without_node_paths", False)):
            ts = []
            for _ in range(2):
                d = os.path.join(tmp, "w_" + name)
                t = time.perf_counter()
                xr.write_region_tsvs(idx, rows, d, node_paths=node_paths, threads=wf.cores)
                ts.append(time.perf_counter() - t)
                st = rows.write_stats
                shutil.rmtree(d)
            wr[name] = {"ms": 1e3 * min(ts), "rows_per_s": len(rows) / min(ts), "bytes": int(st.bytes), "threads": int(st.threads),
                        "format_s": float(st.format_s), "copy_wait_s": float(st.copy_s)}
        out["tsv"] = {"scan_graph_ms": 1e3 * t_tsv, "files": n_files, "rows": int(len(rows)), "rows_per_s": len(rows) / t_tsv,
                      "writer": wr, "what": "scan_graph = GraphIndex.load + upload + plan + emit + gfm_graph_write_tsvs (host "
                                            "threads format the rows from pinned chunks; node paths from the node table)"}
    finally:
        if old_mode is None:
            os.environ.pop("GRAFIMO_SCAN_OUTPUT", None)
        else:
            os.environ["GRAFIMO_SCAN_OUTPUT"] = old_mode
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def extra_config_block(cfg, dev, rank, args, side, steps=12):
    """BASELINE configs[3] / configs[4] inside the default N = 1 line (like roofline_config3): `steps` timed steps after
    two warm-up steps, the score kernels timed by HIP events on their dispatch packets, a slice of the last step's scores
    against the CPU oracle.  -> the block (roofline_config4 / roofline_config5)."""
    import torch
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.scan import KmerScanner, SameWidthScanner
    from oracle import oracle as orc
    mots = synth.config_motifs(cfg)
    dms = [DeviceMotif(m["sm"], m["bg"], m["min_val"], m["scale"], m["offset"]) for m in mots]
    n = 100_000_000

    def fence():
        torch.cuda.synchronize(dev)

    if cfg == 4:
        W = mots[0]["width"]
        d = synth.make_device_kmers(n, W, mots[0]["probs"], synth.seed_for(4, rank), dev)
        sc = KmerScanner(dms[0], n, hit_capacity=n // 64, device=dev, side_stream=side, n_slots=args.slots, score_buffers=args.score_buffers or None)
        step = lambda: sc.enqueue(d, args.threshold, on_qvalue=True, want_qvalues=True)      # noqa: E731
        units, alg = n, n * (W + 4)
        kname = f"score_quad_kernel<{W}, 1>"
        what = f"BASELINE configs[3]: synthetic JASPAR-style PWM W=30, {n} windows generated on the device, both strands, --qvalueT"
    else:
        widths = sorted({m["width"] for m in mots})
        groups = {w: [j for j, m in enumerate(mots) if m["width"] == w] for w in widths}
        bufs = {w: synth.make_device_kmers(n, w, mots[groups[w][0]]["probs"], synth.seed_for(50 + w, rank), dev) for w in widths}
        scs = {w: SameWidthScanner([dms[j] for j in groups[w]], n, max(4096, n // 64), dev) for w in widths}

        def step():
            for w in widths:
                scs[w].enqueue(bufs[w], args.threshold, on_qvalue=False, want_qvalues=True)

        units, alg = n * len(mots), sum(n * (w + 4 * len(groups[w])) for w in widths)
        kname = "score_quad_kernel<W, MM> (batched, one launch per group of <= 3 same-width motifs; summed per step)"
        what = (f"BASELINE configs[4]: 50 synthetic JASPAR-style PWMs W=8..25 (per-motif background), {n} windows per width, "
                f"same-width motifs share each k-mer read; unit = (k-mer, motif) pair")
    last = None
    for _ in range(2):
        last = step()
    fence()
    for dmx in dms:
        dmx.profile_enable(steps + 2, every=1)
    t0 = time.perf_counter()
    for _ in range(steps):
        last = step()
    fence()
    el = time.perf_counter() - t0
    per_motif = [dmx.profile_read() for dmx in dms]
    for dmx in dms:
        dmx.profile_enable(0)
    orc.build()
    if cfg == 4:
        k_ms = float(np.mean(per_motif[0]))
        timed = int(len(per_motif[0]))
        res = sc.collect(last)
        assert res["n_scored"] == n
        km = d[:1_000_000].cpu().numpy()
        _, pt = dms[0].tables()
        exp, _ = orc.score_kmers_table(km, mots[0]["sm"], pt, mots[0]["min_val"])
        assert np.array_equal(last.scores[:len(km)].cpu().numpy(), exp), "config 4: scores differ from the oracle"
        hits = int(len(res["rows"]))
    else:
        k_ms = float(sum(float(np.mean(k)) for k in per_motif if len(k)))
        timed = int(sum(len(k) for k in per_motif))
        hits = 0
        for w in widths:
            km = bufs[w][:200_000].cpu().numpy()
            for k_, j in enumerate(groups[w]):
                _, pt = dms[j].tables()
                exp, _ = orc.score_kmers_table(km, mots[j]["sm"], pt, mots[j]["min_val"])
                assert np.array_equal(scs[w].scores[k_][:len(km)].cpu().numpy(), exp), f"config 5: motif {j} (W={w}) differs from the oracle"
            hits += int(scs[w].hits[:, 0].sum().item())
    block = {"workload": what, "steps": steps, "ms_per_step": 1e3 * el / steps, "units_per_s": units * steps / el,
             "unit": "k-mers/s" if cfg == 4 else "(k-mer, motif) pairs/s", "kernel": kname, "kernel_ms_avg": k_ms,
             "kernel_launches_timed": timed, "algorithmic_bytes_per_launch": alg, "achieved": alg / (k_ms * 1e-3) / 1e9,
             "peak": HBM_PEAK_GBS, "unit_bw": "GB/s", "frac": alg / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
             "hits_last_step": hits, "oracle_checked": True}
    for dmx in dms:
        dmx.close()
    return block


# ---------------------------------------------------------------------------- --dump-outputs
DUMP_LIMIT_BYTES = 64 << 20     # all files of one dump together
DUMP_SAMPLE = 1 << 20           # rows kept of a longer output (a fixed, seeded sample)
DUMP_SAMPLE_MULTI = 1 << 14     # the same per motif of config 5 (50 motifs)


def _dump_sample(n, k, seed):
    """Ascending indices of a fixed sample of k of n rows (all n rows when n <= k): the same for every run."""
    if n <= k:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).choice(n, size=k, replace=False))


def _sampled_hits(rows, scaled, qtable, k, seed):
    """Hit rows (ascending) with their scaled scores and q-values; at most k of them, a fixed sample."""
    i = _dump_sample(len(rows), k, seed)
    return rows[i], scaled[i], qtable[scaled[i]]


def scan_outputs(res, scores):
    """What KmerScanner.collect hands its caller for the last timed step (configs 2-4), plus its score array:
    hit rows ascending with their scaled scores and q-values, the q-table, the row count, and a fixed sample of the
    int32 scores (scores_sample_rows says which rows)."""
    import torch
    idx = _dump_sample(int(scores.numel()), DUMP_SAMPLE, 1)
    rows, scaled, qv = _sampled_hits(res["rows"], res["scaled"], res["qtable"], DUMP_SAMPLE, 2)
    return {"hit_rows": rows, "hit_scaled_scores": scaled, "hit_qvalues": qv, "qtable": res["qtable"],
            "n_scored": np.array([res["n_scored"]]), "n_hits": np.array([len(res["rows"])]),
            "scores_sample_rows": idx, "scores_sample": scores[torch.from_numpy(idx).to(scores.device)].cpu().numpy()}


def multi_outputs(scanners, groups, n_motifs, n):
    """Config 5: per motif (index into the config's motif list) the hits of the last timed step (rows, scaled scores,
    q-values; at most DUMP_SAMPLE_MULTI per motif, a fixed sample), the hit and row counts, and the scores of a fixed
    sample of rows (scores_sample[motif, j] is the score of row scores_sample_rows[j])."""
    import torch
    from grafimo_amd.scan import HIT_SCORE_BITS
    idx = _dump_sample(n, DUMP_SAMPLE_MULTI, 1)
    d_idx = None
    motif, rows, scaled, qv = [], [], [], []
    n_hits, n_scored = np.zeros(n_motifs), np.zeros(n_motifs)
    sample = np.zeros((n_motifs, len(idx)))
    for w, sc in scanners.items():
        hits, qtab, nrows = sc.hits.cpu().numpy(), sc.qtable.cpu().numpy(), sc.nrows.cpu().numpy()
        for k, j in enumerate(groups[w]):
            cnt = int(hits[k, 0])
            if cnt > hits.shape[1] - 1:
                raise OverflowError(f"motif {j}: {cnt} hits exceed the {hits.shape[1] - 1} entries the scanner holds")
            packed = np.sort(hits[k, 1:1 + cnt])
            r, s_, q = _sampled_hits(packed >> HIT_SCORE_BITS, packed & ((1 << HIT_SCORE_BITS) - 1), qtab[k],
                                     DUMP_SAMPLE_MULTI, 2 + j)
            motif.append(np.full(len(r), j))
            rows.append(r)
            scaled.append(s_)
            qv.append(q)
            n_hits[j], n_scored[j] = cnt, nrows[k]
            if d_idx is None:
                d_idx = torch.from_numpy(idx).to(sc.scores[k].device)
            sample[j] = sc.scores[k][d_idx].cpu().numpy()
    return {"hit_motif": np.concatenate(motif), "hit_rows": np.concatenate(rows), "hit_scaled_scores": np.concatenate(scaled),
            "hit_qvalues": np.concatenate(qv), "n_hits": n_hits, "n_scored": n_scored,
            "scores_sample_rows": idx, "scores_sample": sample}


def dump_outputs(out_dir, arrays):
    """DIR/<name>.npy for every array, as float64 (exact for every integer output here: all are below 2**53)."""
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", type=int, choices=[2, 3, 4, 5], default=None,
                    help="BASELINE.json config (default: 2 on one GPU, 3 = its per-GPU shard on several)")
    ap.add_argument("--bursts", type=int, default=1,
                    help="split the --steps timed steps into this many bursts; the median ms per step is reported")
    ap.add_argument("--rows", type=int, default=None, help="override the rows per GPU (diagnostics)")
    ap.add_argument("--threshold", type=float, default=1e-4)
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement and self-check (CPU baselines, oracle slice, other configs and "
                         "paths); a plain run measures the headline figure only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the TSV-directory scans")
    ap.add_argument("--no-e2e-large", action="store_true", help="with --full: skip the 2e7-row / 10 000-file TSV directory")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip roofline_config3, sustained, peak_measured and extract (N=1 default config "
                         "only) and product_paths (N > 1)")
    ap.add_argument("--sustained-s", type=float, default=5.0, help="length of the sustained leg in seconds")
    ap.add_argument("--no-config45", action="store_true",
                    help="with --full: skip the roofline_config4 / roofline_config5 blocks of the default line")
    ap.add_argument("--slots", type=int, default=3,
                    help="buffer slots of the scan pipeline (2: the device waits for slot reuse; >= 3: the host does)")
    ap.add_argument("--score-buffers", type=int, default=0,
                    help="score arrays of the scan pipeline (0 = one per slot); fewer than --slots: a shorter ring (a batch's "
                         "scores stay valid for score_buffers - 1 further steps).  Measured and not the default: "
                         "profiles/r06_step_gap*.txt")
    ap.add_argument("--force-dist", action="store_true",
                    help="diagnostic: initialise torch.distributed and issue the collectives even with "
                         "one rank (exercises the N > 1 code path on a 1-GPU box)")
    ap.add_argument("--event-every", type=int, default=None,
                    help="time the score kernel of every n-th step with a hipEvent pair on its dispatch "
                         "(default: every 8th, more often when the run is short, so that at least ~6 launches are timed)")
    ap.add_argument("--no-candidates", action="store_true",
                    help="config 4: select on the q-value threshold by a pass over every score instead of "
                         "filtering the p < t candidates the score kernel collects (measurement aid)")
    ap.add_argument("--overlap", choices=["auto", "on", "off"], default="auto",
                    help="run the per-step tail (post kernel, collective, q-table, gather) on a side "
                         "stream so that it overlaps the next step's score kernel; auto = on")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / process-group plumbing only (gloo, no GPU, nothing measured): the CPU tests use it")
    ap.add_argument("--dry-run-fail-rank", type=int, default=None, help="with --dry-run: this rank exits with code 3")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float64, <= 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))       # this process never touches a GPU

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        args.gpus = world
    if args.dry_run:
        return dry_run(args, rank, world)
    cfg = args.config if args.config is not None else (2 if world == 1 else 3)

    from grafimo_amd import synth
    ctcf = load_ctcf()
    if cfg in (2, 3):
        mots = [dict(sm=ctcf.dense_score_matrix(), bg=ctcf.dense_bg(), min_val=ctcf.min_val, scale=ctcf.scale,
                     offset=float(ctcf.offset), probs=np.asarray(ctcf.count_matrix, dtype=np.float64), width=ctcf.width)]
    else:
        mots = synth.config_motifs(cfg)
    on_q = cfg == 4
    rows_default = {2: 20_000_000, 3: 125_000_000, 4: 100_000_000, 5: 100_000_000 // world}[cfg]
    n = int(args.rows) if args.rows else rows_default

    host_batch = None
    if cfg == 2 and not args.rows:
        host_batch = synth.make_batch(10_000, 2_000, mots[0]["width"], mots[0]["probs"], synth.seed_for(2, rank),
                                      region_base=rank * 10_000)
        n = len(host_batch)

    # ---- everything that forks workers comes BEFORE the first HIP call
    # default_n1: the side blocks of the default N = 1 line are run (--full only)
    default_n1 = args.full and rank == 0 and world == 1 and cfg == 2 and not args.rows
    cpu = {}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baselines(mots[0])
    tsv_dirs = {}
    try:
        if default_n1 and not args.no_e2e:
            workers = min(os.cpu_count() or 1, 128)
            probs = np.asarray(ctcf.count_matrix, dtype=np.float64)
            tsv_dirs["e2e"] = make_tsv_dir(1000, 2000, ctcf.width, probs, workers)
            if not args.no_e2e_large:
                tsv_dirs["e2e_config2"] = make_tsv_dir(10_000, 2000, ctcf.width, probs, workers)
            tsv_dirs = {k: v for k, v in tsv_dirs.items() if v[0] is not None}     # no room: that block is left out
        run_rank(args, cfg, rank, local_rank, world, mots, ctcf, n, host_batch, on_q, cpu, tsv_dirs, default_n1)
    finally:
        for d, _ in tsv_dirs.values():
            shutil.rmtree(d, ignore_errors=True)


def run_rank(args, cfg, rank, local_rank, world, mots, ctcf, n, host_batch, on_q, cpu, tsv_dirs, default_n1):
    import torch
    import torch.distributed as dist
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif, calibrate_stream
    from grafimo_amd.scan import KmerScanner, SameWidthScanner

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        import datetime
        # (a collective nobody answers ends the run after PRODUCT_PATHS_TIMEOUT_S instead of the default ten minutes)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev,
                                timeout=datetime.timedelta(seconds=PRODUCT_PATHS_TIMEOUT_S))
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)
        # RCCL's kernels need CUs of their own next to the persistent score grid: leave 16 free
        # (the score kernel is HBM-bound; 240 CUs move the same bytes, measured -1 %)
        os.environ.setdefault("GRAFIMO_RESERVE_CUS", "16")
    side = args.overlap != "off"

    dms = [DeviceMotif(m["sm"], m["bg"], m["min_val"], m["scale"], m["offset"]) for m in mots]   # DP on device
    # ---- inputs resident in HBM
    if cfg == 5:
        widths = sorted({m["width"] for m in mots})
        groups = {w: [j for j, m in enumerate(mots) if m["width"] == w] for w in widths}
        bufs = {w: [synth.make_device_kmers(n, w, mots[groups[w][0]]["probs"], synth.seed_for(50 + w, rank), dev)]
                for w in widths}
        scanners = {w: SameWidthScanner([dms[j] for j in groups[w]], n, max(4096, n // 64), dev,
                                        side_stream=args.overlap == "on")
                    for w in widths}
        units_per_step = n * len(mots)
        alg_bytes = sum(n * (w + 4 * len(groups[w])) for w in widths)

        def step(i):
            for w in widths:
                scanners[w].enqueue(bufs[w][0], args.threshold, on_qvalue=False, want_qvalues=True, row_base=rank * n)

        rotate = 1
    else:
        m0 = mots[0]
        W = m0["width"]
        if host_batch is not None:
            first = torch.from_numpy(host_batch.kmers).to(dev)
        else:
            first = synth.make_device_kmers(n, W, m0["probs"], synth.seed_for(cfg, rank), dev)
        bufs = [first]
        if first.numel() < (512 << 20):   # small enough to sit in the 256 MiB Infinity Cache in part: alternate
            bufs.append(torch.roll(first, shifts=n // 3, dims=0).contiguous())
        rotate = len(bufs)
        hit_cap = max(4096, n // 64)
        scanner = KmerScanner(dms[0], n, hit_capacity=hit_cap, device=dev, group=None, side_stream=side,
                              n_slots=args.slots, always_collective=args.force_dist,
                              candidates=not args.no_candidates, score_buffers=args.score_buffers or None)
        scanner.profile_tail = side
        units_per_step = n
        alg_bytes = n * (W + 4)

        def step(i):
            return scanner.enqueue(bufs[i % rotate], args.threshold, on_qvalue=on_q, want_qvalues=True,
                                   row_base=rank * n, gather_hits=use_dist)

    def fence():
        # the device-wide synchronize covers the side streams too: no stream-to-stream waits (finish()) in front of it
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize(dev)

    it = 0
    for _ in range(max(args.warmup, rotate)):
        step(it)
        it += 1
    fence()
    if cfg != 5 and use_dist:
        scanner.size_gather()          # the per-step gather moves what is hit, not the whole hit buffer
    every = max(1, args.event_every) if args.event_every else max(1, min(8, args.steps // 6))
    for d in dms:
        d.profile_enable(min(1024, max(16, args.steps // every + 1)), every=every)
    # the --steps timed steps, split into --bursts bursts of (nearly) equal length
    n_bursts = min(max(1, args.bursts), args.steps)
    burst_steps = [args.steps // n_bursts + (b < args.steps % n_bursts) for b in range(n_bursts)]
    burst_s, own_s = [], []           # seconds per burst (MAX over ranks) and this rank's own
    for k in burst_steps:
        fence()
        t0 = time.perf_counter()
        for _ in range(k):
            last = step(it)
            it += 1
        fence()
        own_s.append(time.perf_counter() - t0)
        el = torch.tensor([own_s[-1]], dtype=torch.float64, device=dev)
        if use_dist:
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
        burst_s.append(float(el.item()))
    step_s = float(np.median([b / k for b, k in zip(burst_s, burst_steps)]))     # seconds per timed step
    kernel_ms = [d.profile_read() for d in dms]
    tail_ms = dms[0].profile_read_tail() if cfg != 5 else np.empty(0, np.float32)
    for d in dms:
        d.profile_enable(0)
    if cfg != 5:
        scanner.profile_tail = False
    # every rank's own median ms per step -> rank 0
    mine = torch.tensor([1e3 * float(np.median([b / k for b, k in zip(own_s, burst_steps)]))], dtype=torch.float64, device=dev)
    rank_ms = [mine.clone() for _ in range(world)]
    if use_dist and world > 1:
        dist.all_gather(rank_ms, mine)
    rank_ms = [float(t.item()) for t in rank_ms]

    # outputs of the last step stay valid: self-checks outside the timed region -- the counts always, with --full also a
    # slice of the scores against the CPU oracle (the checker)
    checked_rows = 1_000_000 if args.full else 0
    if checked_rows:
        from oracle import oracle as orc
        orc.build()
    if cfg == 5:
        torch.cuda.synchronize(dev)
        for w in widths:
            nr = scanners[w].nrows.cpu().numpy()
            assert (nr == n * world).all(), (w, nr, n, world)
            if not checked_rows:
                continue
            km = bufs[w][0][:checked_rows].cpu().numpy()
            for k, j in enumerate(groups[w]):        # a slice of every motif's scores against the oracle
                _, pt = dms[j].tables()
                exp, _ = orc.score_kmers_table(km, mots[j]["sm"], pt, mots[j]["min_val"])
                got = scanners[w].scores[k][:len(km)].cpu().numpy()
                assert np.array_equal(got, exp), f"config 5: scores of motif {j} (W={w}) differ from the oracle"
        n_hits = int(sum(int(scanners[w].hits[:, 0].sum().item()) for w in widths))
    else:
        res = scanner.collect(last)
        n_hits = int(len(res["rows"]))
        assert res["n_scored"] == n * world, (res["n_scored"], n, world)
        if checked_rows:
            km = bufs[(it - 1) % rotate][:checked_rows].cpu().numpy()
            _, pt = dms[0].tables()
            exp, _ = orc.score_kmers_table(km, mots[0]["sm"], pt, mots[0]["min_val"])
            assert np.array_equal(last.scores[:len(km)].cpu().numpy(), exp), "scores differ from the oracle"
    assert n_hits > 0
    if args.dump_outputs and rank == 0:      # before the blocks below run further steps on these buffers
        dump_outputs(args.dump_outputs, multi_outputs(scanners, groups, len(mots), n) if cfg == 5
                     else scan_outputs(res, last.scores[:n]))

    extras = {}
    if args.full and use_dist and cfg in (2, 3) and not args.no_extras:
        # the two other PRODUCT paths under the same process group, so that a scaling run says something about all three: the
        # fused graph path (every rank uploads its shard of the graph) and the streamed TSV scan (every rank its files)
        #  the block decides about failures COLLECTIVELY, stage by stage: see product_paths_block
        extras["product_paths"] = product_paths_block(ctcf, dev, rank, world)
    if default_n1 and not args.no_extras:
        W = mots[0]["width"]
        # (c) what this device sustains for a bare stream of the kernel's byte mix (76 B in / 16 B out per lane-step)
        cal = {}
        for name, through in (("write_through", True), ("nt", False)):
            us, nbytes = calibrate_stream(5, n * W, through, 20)
            cal[name] = {"us_per_launch": us, "GBps": nbytes / (us * 1e-6) / 1e9, "bytes_per_launch": nbytes}
        extras["peak_measured"] = {
            "kernel": "stream_mix_kernel<5> (gfm_calibrate_stream): 5 x 16 B nt loads + one 16 B store per lane-step, "
                      "interleaved, one step prefetched; output rotating over three buffers",
            "in_bytes": n * W, **cal,
            "GBps": max(c["GBps"] for c in cal.values()), "unit": "GB/s"}
        # (c') the same launch WITHOUT the score store (d_scores == NULL: what the product's scans run -- with a threshold the
        # cutoff is known before scoring and nothing ever reads the int32 [N] array): N x W bytes instead of N x (W + 4).
        # A side block: the contract's metric counts the score store, `value` keeps it.
        try:
            hist0 = torch.zeros(dms[0].L, dtype=torch.int64, device=dev)
            rows0 = torch.empty(max(4096, n // 64), dtype=torch.int64, device=dev)
            cnt0 = torch.zeros(1, dtype=torch.int64, device=dev)
            cut0 = dms[0].pvalue_cutoff(args.threshold)
            for i_ in range(3):
                dms[0].score(bufs[i_ % rotate], None, hist=hist0, select_cutoff=cut0, hit_rows=rows0, hit_count=cnt0, reset_hits=True)
            fence()
            dms[0].profile_enable(20, every=1)
            t0 = time.perf_counter()
            for i_ in range(20):                 # (input buffers rotated like the main loop's)
                dms[0].score(bufs[i_ % rotate], None, hist=hist0, select_cutoff=cut0, hit_rows=rows0, hit_count=cnt0, reset_hits=True)
            fence()
            el0 = time.perf_counter() - t0
            k0 = dms[0].profile_read()
            dms[0].profile_enable(0)
            k0_ms = float(np.mean(k0))
            extras["roofline_noscore"] = {
                "what": "gfm_score_kmers with d_scores == NULL on the same 2e7 k-mers: histogram + hit list, no score array",
                "kernel": f"score_quad_kernel<{W}, 1>", "kernel_ms_avg": k0_ms, "ms_per_step": 1e3 * el0 / 20,
                "kmers_per_s": n * 20 / el0, "algorithmic_bytes_per_launch": n * W,
                "achieved": n * W / (k0_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": n * W / (k0_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "hits": int(cnt0.item())}
            del hist0, rows0, cnt0
        except Exception as e:                   # (a side measurement: it must not take the bench line with it)
            extras["roofline_noscore"] = {"error": f"{type(e).__name__}: {e}"}
        # (b) sustained: back-to-back steps for >= sustained_s seconds, one timing event per 100 steps
        per = 100
        blocks = max(2, int(args.sustained_s / step_s / per) + 1)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(blocks + 1)]
        fence()
        main_stream = torch.cuda.current_stream(dev)
        t0 = time.perf_counter()
        evs[0].record(main_stream)
        for b in range(blocks):
            for _ in range(per):
                step(it)
                it += 1
            evs[b + 1].record(main_stream)
        fence()
        wall = time.perf_counter() - t0
        blk = np.array([evs[b].elapsed_time(evs[b + 1]) for b in range(blocks)])
        extras["sustained"] = {"steps": blocks * per, "seconds": wall, "kmers_per_s": blocks * per * n / wall,
                               "ms_per_100_steps": {"min": float(blk.min()), "median": float(np.median(blk)),
                                                    "max": float(blk.max())},
                               "first_vs_last_block_ms": [float(blk[0]), float(blk[-1])]}
        # (a) the config-3 shard: scores beyond any cache (477 MiB per launch, nt stores); the 1-GPU point of the curve
        n3 = 125_000_000
        d3 = synth.make_device_kmers(n3, W, mots[0]["probs"], synth.seed_for(3, rank), dev)
        sc3 = KmerScanner(dms[0], n3, hit_capacity=n3 // 64, device=dev, side_stream=side, n_slots=args.slots, score_buffers=args.score_buffers or None)
        for _ in range(3):
            sc3.enqueue(d3, args.threshold, want_qvalues=True)
        fence()
        steps3 = 12
        dms[0].profile_enable(steps3, every=2)
        t0 = time.perf_counter()
        for _ in range(steps3):
            last3 = sc3.enqueue(d3, args.threshold, want_qvalues=True)
        fence()
        el3 = time.perf_counter() - t0
        k3 = dms[0].profile_read()
        dms[0].profile_enable(0)
        r3 = sc3.collect(last3)
        assert r3["n_scored"] == n3 and len(r3["rows"]) > 0
        k3_ms = float(np.mean(k3))
        extras["roofline_config3"] = {
            "workload": f"BASELINE configs[2], one GPU's shard: CTCF W=19, {n3} windows generated on the device",
            "steps": steps3, "ms_per_step": 1e3 * el3 / steps3, "kmers_per_s": n3 * steps3 / el3,
            "kernel": f"score_quad_kernel<{W}, 1>", "kernel_ms_avg": k3_ms, "kernel_launches_timed": int(len(k3)),
            "algorithmic_bytes_per_launch": n3 * (W + 4), "achieved": n3 * (W + 4) / (k3_ms * 1e-3) / 1e9,
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": n3 * (W + 4) / (k3_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "score_stores": "nt (477 MiB of scores per launch)"}
        del sc3, d3, last3
        torch.cuda.empty_cache()
        if not args.no_config45:
            # BASELINE configs[3] and configs[4], driver-timed inside the default line (their own runs: --config 4 / 5)
            extras["roofline_config4"] = extra_config_block(4, dev, rank, args, side)
            torch.cuda.empty_cache()
            extras["roofline_config5"] = extra_config_block(5, dev, rank, args, side)
            torch.cuda.empty_cache()
        extras["extract"] = extract_block(ctcf, dev)
        if not args.no_config45:
            for cfg_ in (4, 5):                  # the same two configs through the GRAPH (the fused path; motif sets in one pass)
                try:
                    extras[f"extract_config{cfg_}"] = extract_config_block(cfg_, dev)
                except Exception as e:           # (a side measurement: it must not take the bench line with it)
                    extras[f"extract_config{cfg_}"] = {"error": f"{type(e).__name__}: {e}"}
                torch.cuda.empty_cache()
        # the strand-max / per-region best-hit reductions (north_star; csrc/region_reduce.hip) over this batch's scores:
        # 10 000 regions, rows under the p-value cutoff and carried by a haplotype
        from grafimo_amd import top_hits as th
        d_region = torch.from_numpy(host_batch.region).to(dev)
        d_freq = torch.from_numpy(host_batch.freq).to(dev)
        d_start, d_stop = torch.from_numpy(host_batch.start).to(dev), torch.from_numpy(host_batch.stop).to(dev)
        cut = dms[0].pvalue_cutoff(args.threshold)
        sc_last = last.scores
        best = th.region_best(sc_last, d_region, 10_000, freq=d_freq, min_score=cut)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(10):
            th.region_best(sc_last, d_region, 10_000, freq=d_freq, min_score=cut, out=best)
        e1.record()
        for _ in range(3):
            lm = th.locus_max(sc_last, d_region, 10_000, d_start, d_stop, freq=d_freq, min_score=cut)
        e2.record()
        torch.cuda.synchronize(dev)
        s_np = sc_last.cpu().numpy()
        ok_rows = (s_np >= cut) & (host_batch.freq > 0)
        want = np.full(10_000, -1, np.int64)
        np.maximum.at(want, host_batch.region[ok_rows], s_np[ok_rows])
        got_s, _, _ = th.decode_best(best)
        extras["strand_max"] = {
            "rows": n, "regions": 10_000, "region_best_ms": e0.elapsed_time(e1) / 10,
            "region_best_read_GBps": n * 16 / (e0.elapsed_time(e1) / 10 * 1e-3) / 1e9,      # score + region id + frequency
            "locus_max_ms_all_rows_filtered": e1.elapsed_time(e2) / 3, "regions_with_a_hit": int((want >= 0).sum()),
            "equals_numpy_groupby": bool(np.array_equal(got_s, want)) and int((lm.cpu().numpy() >= 0).sum()) == int(ok_rows.sum()),
            "what": "gfm_region_best / gfm_locus_max over the last step's scores: per region the best reported hit, per "
                    "locus the both-strand maximum (rows with p < threshold and haplotype_frequency > 0)"}
        # the boundary's host-buffer form (gfm_scan_host: pageable k-mers in, hits out): the PCIe-inclusive rate --
        # never `value`
        t_host = []
        for _ in range(3):
            t0 = time.perf_counter()
            hres = dms[0].scan_host(host_batch.kmers, args.threshold, capacity=n // 16)
            t_host.append(time.perf_counter() - t0)
        extras["pcie_inclusive"] = {
            "rows": n, "ms": 1e3 * float(np.median(t_host)), "kmers_per_s": n / float(np.median(t_host)),
            "hits": int(len(hres["rows"])),
            "path": "gfm_scan_host: hipMalloc + pageable H2D of the k-mer matrix + score + q-table + D2H of the hits, one call"}

    e2e = {}
    if default_n1 and not args.no_e2e:
        for name, (tmp, rows) in tsv_dirs.items():
            e2e[name] = e2e_block(tmp, rows, ctcf.width, dms[0])

    if rank == 0:
        ms_per_step = 1e3 * step_s
        value = units_per_step * world / step_s
        if cfg == 5:      # a step launches one batched kernel per group of <= 3 same-width motifs: sum of their means
            k_ms = float(sum(float(np.mean(k)) for k in kernel_ms if len(k)))
            timed = int(sum(len(k) for k in kernel_ms))
            kname = "score_quad_kernel<W, MM> (batched, one launch per group of <= 3 same-width motifs; summed per step)"
        else:
            k_ms = float(np.mean(kernel_ms[0])) if len(kernel_ms[0]) else float("nan")
            timed = int(len(kernel_ms[0]))
            kname = f"score_quad_kernel<{mots[0]['width']}, 1>"
        achieved = alg_bytes / (k_ms * 1e-3) / 1e9
        traffic, traffic_source = None, None
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tpath) and cfg != 5:
            with open(tpath) as fh:
                tj = json.load(fh)
            if tj.get("rows_per_launch") == n and tj.get("width") == mots[0]["width"] and tj.get("kernel") == kname:
                import hashlib
                src = b"".join(open(os.path.join(ROOT, f), "rb").read() for f in tj.get("kernel_source_files", []))
                if src and hashlib.sha256(src).hexdigest()[:16] == tj.get("kernel_source_sha16"):
                    traffic = tj.get("hbm_bytes_per_launch")
                    traffic_source = ("profiles/pmc_traffic.json: committed rocprofv3 --pmc passes of this kernel at this "
                                      "size (" + str(tj.get("source", "scripts/lab_pmc.sh")) + "), NOT counters of this run; "
                                      "the kernel's sources still hash to what the counters were taken from")
                else:
                    traffic_source = ("profiles/pmc_traffic.json is STALE: the score kernel's sources changed since its counters "
                                      "were collected (scripts/lab_pmc.sh collects them again)")
        workload = {
            2: f"BASELINE configs[1] per GPU: CTCF MA0139.1 W=19, 10000 synthetic 200bp regions x 2000 haplotype "
               f"k-mers = {n} windows",
            3: f"BASELINE configs[2], one GPU's shard of the 1e9-window scan: CTCF MA0139.1 W=19, {n} windows "
               f"generated on the device",
            4: f"BASELINE configs[3]: synthetic JASPAR-style PWM W=30, 50000 regions x 2000 = {n} windows, both "
               f"strands, --qvalueT (threshold on q)",
            5: f"BASELINE configs[4]: 50 synthetic JASPAR-style PWMs W=8..25 (per-motif background), {n} windows per "
               f"width per GPU, same-width motifs share each k-mer read; unit = (k-mer, motif) pair",
        }[cfg]
        roofline = {
            "bound": "hbm",
            "kernel": kname,
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic,
            "traffic_source": traffic_source,
            "algorithmic_bytes_per_launch": alg_bytes,
            "kernel_ms_avg": k_ms,
            "kernel_launches_timed": timed,
        }
        if "peak_measured" in extras:
            roofline["peak_measured"] = extras["peak_measured"]["GBps"]
            roofline["frac_of_measured"] = achieved / extras["peak_measured"]["GBps"]
        # the fused graph path's figures as SCALARS inside `config` (the driver's record keeps `config`, `roofline` and
        # `cpu_baseline` verbatim and only the names of the other blocks: VERDICT r5 Missing #5 / next #4)
        def _pick(block, *path):
            v = extras.get(block)
            for k in path:
                v = v.get(k) if isinstance(v, dict) else None
            return float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else None

        k_us = _pick("extract", "roofline", "kernel_us")
        f_ms = _pick("extract", "fused_ms")
        fused_cfg = {
            "kernel_us": k_us, "frac": _pick("extract", "roofline", "frac"), "fused_ms": f_ms,
            "fused_minus_kernel_us": (1e3 * f_ms - k_us) if (k_us is not None and f_ms is not None) else None,
            "extract_plus_score_ms": _pick("extract", "extract_plus_score_ms"),
            "scan_graph_ms": _pick("extract", "scan_graph_e2e", "manifest", "scan_graph_ms"),
            "first_call_ms": _pick("extract", "scan_graph_e2e", "manifest", "first_compute_results_ms"),
            "compute_results_ms": _pick("extract", "scan_graph_e2e", "manifest", "compute_results_ms"),
            "many_ms": _pick("extract_config5", "many_ms"), "fifty_single_calls_ms": _pick("extract_config5", "fifty_single_calls_ms"),
            "speedup_vs_single_calls": _pick("extract_config5", "speedup_vs_single_calls"),
            "device_pass_many_ms": _pick("extract_config5", "device_pass_many_ms"),
            "device_pass_fifty_single_ms": _pick("extract_config5", "device_pass_fifty_single_ms"),
            "config4_ms": _pick("extract_config4", "compute_results_from_graph_ms"), "config4_hits": _pick("extract_config4", "hits_q1e-4"),
        } if "extract" in extras else None
        out = {
            "metric": "scored haplotype k-mers/sec",
            "value": value,
            "unit": "k-mers/s" if cfg != 5 else "(k-mer, motif) pairs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": max(args.warmup, rotate),
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            # every rank scores its own shard of fixed size (weak) -- except config 5, whose 1e8 windows per width are SPLIT
            # over the ranks (strong)
            "scaling": "strong" if cfg == 5 else "weak",
            "vs_baseline": None,
            "dtype": "int32",
            "data": "synthetic",
            # the workload a 1 -> N curve is made of: N = 1 defaults to configs[1] (the config the metric is quoted on), N > 1
            # to configs[2]'s per-GPU shard -- the curve's point for THIS N on that one workload is given here at every N
            "scaling_curve_point": (
                {"workload": "BASELINE configs[2] per-GPU shard: CTCF W=19, 1.25e8 windows per GPU", "n_gpus": world,
                 "kmers_per_s": value if cfg == 3 else (extras.get("roofline_config3") or {}).get("kmers_per_s"),
                 "source": "value" if cfg == 3 else "roofline_config3"}
                if cfg in (2, 3) else None),
            "rccl_world": dist.get_world_size() if use_dist else 1,
            "rank_ms_per_step": rank_ms,
            "tail_ms": ({"avg": float(np.mean(tail_ms)), "max": float(np.max(tail_ms)), "timed": int(len(tail_ms)),
                         "what": "post kernel" + (" + all-reduce(histogram)" if use_dist else "") + " + q-table"
                                 + (" + selection on q" if on_q else "") + (" + gather(hits)" if use_dist else "")
                                 + ", HIP events on the tail / gather stream from 'score kernel done' to the last of it"}
                        if len(tail_ms) else None),
            "config": {
                "workload": workload,
                "baseline_config": cfg,
                "threshold": args.threshold,
                "threshold_on": "q-value" if on_q else "p-value",
                "qvalues": True,
                "hits_last_step": n_hits,
                "oracle_checked_rows": checked_rows if cfg != 5 else checked_rows * len(mots),
                "full": args.full,
                "input_buffers_rotated": rotate,
                "bursts": len(burst_s),
                "burst_steps": burst_steps,
                "burst_ms": [round(1e3 * b, 4) for b in burst_s],
                "timing": "`steps` timed steps in `bursts` bursts, each burst barrier + synchronize bracketed, MAX over ranks; "
                          "ms_per_step = median over the bursts of burst time / its steps",
                "sharding": (f"regions split over {world} rank(s); all-reduce(score histogram) + gather(hit entries, "
                             f"sized from the observed hit counts) per step") if world > 1 else "single GPU",
                "fused": fused_cfg,
            },
            "roofline": roofline,
            "roofline_noscore": extras.get("roofline_noscore"),
            "roofline_config3": extras.get("roofline_config3"),
            "roofline_config4": extras.get("roofline_config4"),
            "roofline_config5": extras.get("roofline_config5"),
            "sustained": extras.get("sustained"),
            "peak_measured": extras.get("peak_measured"),
            "extract": extras.get("extract"),
            "extract_config4": extras.get("extract_config4"),
            "extract_config5": extras.get("extract_config5"),
            "product_paths": extras.get("product_paths"),
            "strand_max": extras.get("strand_max"),
            "pcie_inclusive": extras.get("pcie_inclusive"),
            "cpu_baseline": cpu.get("cpu_baseline"),
            "cpu_baseline_table": cpu.get("cpu_baseline_table"),
            "e2e": e2e.get("e2e"),
            "e2e_config2": e2e.get("e2e_config2"),
        }
        # RCCL's version banner sits in the C runtime's stdout buffer until the process ends: push it out first,
        # so that the JSON line is the last line of the run
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
