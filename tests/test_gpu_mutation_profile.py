"""The scan fold and the mutation profile on the GPU: the kernel through fold_columns on synthetic keys and sums against the
brute force (tests/mutation_profile_bruteforce.py), bit for bit, at the edges of a launch's 16 motifs and in the three shapes;
split and order independence; profile_sequences against the fold of the mutation scan's per-motif arrays; the table and both
frames against a pandas reduction over the mutation scan's per-motif frames; the command line."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mutation_profile_bruteforce as bf  # noqa: E402
import mutation_scan_bruteforce as msbf  # noqa: E402
import test_gpu_mutation_scan as mst  # noqa: E402  (its sequences at a tile's edges, its graphs, regions, motifs and groups)
import wide_panel_cases as wp  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402
from test_mutation_profile_host import COLUMNS as HOST_COLUMNS, SUMMARY_COLUMNS  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
SHAPES = {"mutation": (5, bf.MUTATION_PAIRS), "indel": (7, bf.INDEL_PAIRS), "block": (2, bf.BLOCK_PAIRS)}
ROWS = (1, 63, 64, 65, 257)


def _got(state):
    return state.cpu().as_dict()


# ------------------------------------------------------------------------------------------- the kernel through fold_columns
@pytest.mark.parametrize("M", [1, 16, 17, 33])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fold_against_brute_force(shape, M):
    """every state array, bit for bit, at 1, 63, 64, 65 and 257 rows"""
    from grafimo_amd.mutation_profile import fold_columns
    C, pairs = SHAPES[shape]
    seen = np.zeros(6, dtype=np.int64)
    for rows in ROWS:
        rng = np.random.default_rng(82_000 + 1000 * list(SHAPES).index(shape) + 10 * M + rows)
        keys, sums, ids, cutoffs, ptables = bf.random_case(rng, rows, C, M)
        want = bf.fold_all(keys, sums, ids, cutoffs, ptables, pairs)
        got = _got(fold_columns(keys, sums, ids, cutoffs, ptables, pairs))
        assert bf.same_state(got, want), (shape, M, rows, bf.first_difference(got, want))
        assert len({len(t) for t in ptables}) > 1 or M == 1                             # tables of differing lengths
        seen += [int(v) for v in (want["counts"][..., 0].sum(), want["counts"][..., 1].sum(), (want["aff_motif"][..., 0] > 0).sum(),
                                  (want["aff_motif"][..., 1] > 0).sum(), (want["aff_sums"] == 0).sum(),
                                  (want["aff_sums"] == np.uint64((1 << 64) - 1)).sum())]
    assert seen.min() > 0, seen                                                         # gains, losses, up, down, sums of 0 and 2^64 - 1


def test_fold_takes_device_tensors_and_block_scan_shapes():
    """keys and sums given as device tensors [n_lengths, n_bases, 2], the rows the leading axes; a second call into the same state"""
    import torch
    from grafimo_amd.mutation_profile import FoldState, fold_columns
    rng = np.random.default_rng(82_900)
    keys, sums, ids, cutoffs, ptables = bf.random_case(rng, 3 * 70, 2, 5)
    want = bf.fold_all(keys, sums, ids, cutoffs, ptables, bf.BLOCK_PAIRS)
    dev = torch.device("cuda", torch.cuda.current_device())
    dk = [torch.from_numpy(k.view(np.int32).reshape(3, 70, 2)).to(dev) for k in keys]
    ds = [torch.from_numpy(s.view(np.int64).reshape(3, 70, 2)).to(dev) for s in sums]
    dp = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in ptables]
    state = FoldState.zeros(210, 1)
    assert fold_columns(dk[:2], ds[:2], ids[:2], cutoffs[:2], dp[:2], bf.BLOCK_PAIRS, state) is state
    fold_columns(dk[2:], ds[2:], ids[2:], cutoffs[2:], dp[2:], bf.BLOCK_PAIRS, state)
    assert bf.same_state(_got(state), want), bf.first_difference(_got(state), want)
    with pytest.raises(ValueError, match=r"holds \[210\]\[4\] cells"):
        fold_columns(dk, ds, ids, cutoffs, dp, bf.MUTATION_PAIRS, state)


def test_split_and_order_give_one_state():
    """33 motifs in one call, one by one in reverse id order, and in chunks of 5 into one state: three byte-identical states"""
    from grafimo_amd.mutation_profile import FoldState, fold_columns
    rng = np.random.default_rng(83_000)
    rows, M = 130, 33
    case = bf.random_case(rng, rows, 5, M)
    take = lambda idx: [[v[i] for i in idx] for v in case]                              # noqa: E731
    want = bf.fold_all(*case, bf.MUTATION_PAIRS)
    whole = _got(fold_columns(*case, bf.MUTATION_PAIRS))
    one = FoldState.zeros(rows, 4)
    for i in np.argsort(case[2])[::-1].tolist():
        fold_columns(*take([i]), bf.MUTATION_PAIRS, one)
    fives = FoldState.zeros(rows, 4)
    for a in range(0, M, 5):
        fold_columns(*take(list(range(a, min(a + 5, M)))), bf.MUTATION_PAIRS, fives)
    assert bf.same_state(whole, want), bf.first_difference(whole, want)
    assert bf.same_state(_got(one), whole), bf.first_difference(_got(one), whole)
    assert bf.same_state(_got(fives), whole), bf.first_difference(_got(fives), whole)


# ------------------------------------------------------------------------------------------- profile_sequences
WIDTHS = (4, 7, 19, 64)
PROFILE_THRESHOLD = 0.1


@functools.lru_cache(maxsize=None)
def _profile_case():
    """the mutation scan's edge lengths for each of the four widths, with N and lower-case bases; two motifs per width, the
    widths interleaved: the fold visits them width by width, not in id order"""
    rng = np.random.default_rng(84_000)
    T = mst._tile()
    seqs = [x for W in WIDTHS for x in mst._sequences(W, T, rng)]
    motifs = [SynMotif(W, seed=840 + 10 * k + j) for k in range(2) for j, W in enumerate(WIDTHS)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    return seqs, motifs, off, np.frombuffer(b"".join(seqs), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _motif_numbers(fwd):
    """per motif of _profile_case, from the library: (keys, sums) of mutation_scan.scan_sequences, the cutoff, the tail table,
    the default weights"""
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.mutation_scan import scan_sequences
    from grafimo_amd.site_distance import cutoff_of
    seqs, motifs, off, bases = _profile_case()
    out = [None] * len(motifs)
    for W in WIDTHS:
        idxs = [i for i, m in enumerate(motifs) if m.width == W]
        arrays = scan_sequences([motifs[i] for i in idxs], off, bases, forward_only=fwd)
        for i, (keys, sums) in zip(idxs, arrays):
            dm = DeviceMotif.lease(motifs[i])
            try:
                ptable = dm.ptable_host().copy()
                cutoff = dm.pvalue_cutoff(PROFILE_THRESHOLD)
                assert cutoff == cutoff_of(ptable, PROFILE_THRESHOLD), (i, cutoff)
                out[i] = (keys, sums, cutoff, ptable, default_weights(dm, 1.0)[0])
            finally:
                dm.release()
    return out


@pytest.mark.parametrize("fwd", [False, True])
def test_profile_sequences_equals_the_fold_of_the_scans(fwd):
    from grafimo_amd.mutation_profile import BYTES_PER_BASE, STATE_BYTES_PER_BASE, profile_sequences
    seqs, motifs, off, bases = _profile_case()
    numbers = _motif_numbers(fwd)
    ids = list(range(len(motifs)))
    want = bf.fold_all([n[0] for n in numbers], [n[1] for n in numbers], ids, [n[2] for n in numbers], [n[3] for n in numbers],
                       bf.MUTATION_PAIRS)
    got = profile_sequences(motifs, off, bases, PROFILE_THRESHOLD, forward_only=fwd)
    assert got.counts.shape == (len(bases), 4, 2) and got.aff_sums.dtype == np.uint64 and got.site_p.dtype == np.float64
    assert bf.same_state(got.as_dict(), want), (fwd, bf.first_difference(got.as_dict(), want))
    assert want["counts"][..., 0].sum() > 0 and want["counts"][..., 1].sum() > 0
    assert len(set(want["site_motif"][want["site_motif"] > 0].tolist())) > 2 and len(set(want["aff_motif"].ravel().tolist())) > 4
    # ---- W = 4 and 7 from the mutation scan's own brute force: the chain does not rest on the scan kernel alone
    keys, sums = [n[0] for n in numbers], [n[1] for n in numbers]
    for i, m in enumerate(motifs):
        if m.width in (4, 7):
            od = motif_as_oracle_dict(m)
            k, s = msbf.scan_arrays(seqs, m.width, od["score_matrix"], od["min_val"], numbers[i][4], fwd)
            keys[i], sums[i] = np.array(k, dtype=np.uint32).reshape(-1, 5), np.array(s, dtype=np.uint64).reshape(-1, 5)
    again = bf.fold_all(keys, sums, ids, [n[2] for n in numbers], [n[3] for n in numbers], bf.MUTATION_PAIRS)
    assert bf.same_state(again, want), bf.first_difference(again, want)
    # ---- one motif per chunk: the same state; one byte less: refused
    N = len(bases)
    tight = (BYTES_PER_BASE + STATE_BYTES_PER_BASE) * N
    assert bf.same_state(profile_sequences(motifs, off, bases, PROFILE_THRESHOLD, forward_only=fwd, max_bytes=tight).as_dict(), want)
    with pytest.raises(ValueError, match=f"{tight} bytes, more than max_bytes = {tight - 1}"):
        profile_sequences(motifs, off, bases, PROFILE_THRESHOLD, forward_only=fwd, max_bytes=tight - 1)
    none = profile_sequences(motifs[:2], [0, 0], np.zeros(0, dtype=np.uint8), PROFILE_THRESHOLD)
    assert none.counts.shape == (0, 4, 2) and none.aff_sums.shape == (0, 4, 2, 2)


# ------------------------------------------------------------------------------------------- the table against pandas
def _expected_detail(frames, motifs):
    """the pandas reduction over the per-motif all_rows frames of the mutation scan (one row per cell in each, in one order)"""
    n = len(frames[0])
    df = pd.concat([f.assign(cell=np.arange(n), m=k) for k, f in enumerate(frames)], ignore_index=True)
    lead = [c for c in frames[0].columns[2:] if c in HOST_COLUMNS or c.startswith("haplotypes_")]
    out = frames[0][lead].copy()
    for name, effect, side in (("gain", "gain", "alt"), ("loss", "loss", "ref")):
        hit = df[df["effect"] == effect]
        out[f"motifs_{name}"] = hit.groupby("cell").size().reindex(range(n), fill_value=0).to_numpy()
        best = hit.sort_values(["cell", f"{side}_pvalue", "m"], kind="stable").groupby("cell").first().reindex(range(n))
        some = best["m"].notna().to_numpy()
        text = lambda c: np.where(some, best[c].to_numpy(dtype=object), "")          # noqa: E731
        out[f"{name}_motif_id"], out[f"{name}_motif_alt_id"] = text("motif_id"), text("motif_alt_id")
        out[f"{name}_ref_score"], out[f"{name}_alt_score"] = best["ref_score"].to_numpy(float), best["alt_score"].to_numpy(float)
        out[f"{name}_pvalue"], out[f"{name}_start"] = best[f"{side}_pvalue"].to_numpy(float), best[f"{side}_start"].to_numpy(float)
        out[f"{name}_strand"], out[f"{name}_kmer"] = text(f"{side}_strand"), text(f"{side}_kmer")
    d = df.pivot(index="cell", columns="m", values="delta_log2_affinity").to_numpy(float)
    ids = np.array([m.motif_id for m in motifs], dtype=object)
    up, down = np.nanmax(np.where(np.isnan(d), -np.inf, d), axis=1), np.nanmin(np.where(np.isnan(d), np.inf, d), axis=1)
    out["up_motif_id"], out["up_delta_log2_affinity"] = ids[np.argmax(np.where(np.isnan(d), -np.inf, d), axis=1)], up
    out["down_motif_id"], out["down_delta_log2_affinity"] = ids[np.argmin(np.where(np.isnan(d), np.inf, d), axis=1)], down
    return out


def _check_affinity(got, want, side, sign):
    """the affinity champions: the per-motif frames hold rounded log2 differences, the state exact sums -- the ids agree but
    where two motifs' deltas are closer than the rounding, and where no delta differs from 0 by more than it"""
    g_id, g_d = got[f"{side}_motif_id"].to_numpy(dtype=object), got[f"{side}_delta_log2_affinity"].to_numpy(float)
    w_id, w_d = want[f"{side}_motif_id"].to_numpy(dtype=object), want[f"{side}_delta_log2_affinity"].to_numpy(float)
    clear = sign * w_d > 1e-9
    assert (g_id[clear] != "").all() and np.allclose(g_d[clear], w_d[clear], rtol=0, atol=1e-9)
    none = ~(sign * w_d > -1e-9)                                    # every motif moves the other way, or has no window
    assert (g_id[none] == "").all() and np.isnan(g_d[none]).all()
    assert ((g_id == w_id) | ~clear).mean() > 0.99 and clear.sum() > 0
    return clear.sum()


@pytest.mark.parametrize("name", mst.GRAPHS)
def test_table_against_a_pandas_reduction_of_the_mutation_scan(name):
    from grafimo_amd.mutation_profile import compute_mutation_profile
    from grafimo_amd.mutation_scan import compute_mutation_scan_many
    idx, regions, motifs, groups, fwd = mst._setup(name)
    motifs = list(motifs) + [SynMotif(motifs[0].width, seed=900 + mst.GRAPHS.index(name)), SynMotif(4, seed=950)]
    for j, m in enumerate(motifs[2:], 2):
        m.motif_id, m.motif_name = f"M{j}_{m.width}", f"m{j}"
    args = wp.Args(threshold=mst.THRESHOLD, no_reverse=fwd)
    tables = compute_mutation_scan_many(motifs, idx, regions, False, args, haplotype_groups=groups, all_rows=True)
    t = compute_mutation_profile(motifs, idx, regions, False, args, haplotype_groups=groups, all_rows=True)
    _check_table(name, t, tables, motifs, ["haplotypes_a", "haplotypes_none"])


def _check_table(name, t, tables, motifs, group_columns):
    """the profile `t` against the mutation scan's per-motif tables of the same call"""
    assert t.motif_ids.tolist() == [m.motif_id for m in motifs] and t.widths.tolist() == [m.width for m in motifs]
    assert np.array_equal(t.bases, tables[0].bases) and np.array_equal(t.seq_offsets, tables[0].seq_offsets)
    # ---- the state is the brute force fold of the tables' arrays
    want = bf.fold_all([x.keys for x in tables], [x.sums for x in tables], list(range(len(motifs))),
                       [int(np.argmax(x.ptable < mst.THRESHOLD)) if (x.ptable < mst.THRESHOLD).any() else len(x.ptable) for x in tables],
                       [x.ptable for x in tables], bf.MUTATION_PAIRS)
    assert bf.same_state(t.state.as_dict(), want), (name, bf.first_difference(t.state.as_dict(), want))
    # ---- the detail frame
    expect = _expected_detail([x.to_frame() for x in tables], motifs)
    frame = t.to_frame()
    columns = [c for c in HOST_COLUMNS if c != "haplotypes_g"]
    columns[3:3] = group_columns
    assert list(frame.columns) == columns and sorted(expect.columns) == sorted(columns)
    assert len(frame) == len(expect) == 3 * len(t.bases) == len(t)
    exact = [c for c in columns if not c.startswith(("up_", "down_"))]
    for c in exact:
        g, w = frame[c].to_numpy(), expect[c].to_numpy()
        same = (g == w) | ((g != g) & (w != w))
        assert same.all(), (name, c, np.flatnonzero(~same)[:5].tolist(), g[~same][:3], w[~same][:3])
    assert (frame["motifs_gain"] > 1).any() or name == "hand"
    assert _check_affinity(frame, expect, "up", 1.0) and _check_affinity(frame, expect, "down", -1.0)
    # ---- the filters keep the stated subset
    moved = (frame["motifs_gain"] + frame["motifs_loss"] > 0).to_numpy()
    t.all_rows = False
    text = lambda f: f.to_csv(sep="\t", index=False)                                    # noqa: E731
    assert text(t.to_frame()) == text(frame[moved]) and 0 < moved.sum() < len(frame)
    t.delta = 1.0
    far = (frame["up_delta_log2_affinity"].abs() >= 1.0).to_numpy() | (frame["down_delta_log2_affinity"].abs() >= 1.0).to_numpy()
    assert text(t.to_frame()) == text(frame[moved | far]) and len(t) == (moved | far).sum()
    t.delta, t.all_rows = None, True
    # ---- the summary: a pandas group-by over the detail rows of the versions' own coordinates
    s = t.summary_frame()
    assert list(s.columns) == SUMMARY_COLUMNS
    on = frame[(frame["version"] >= 0) & ~frame["inserted"]].copy()
    on["hg"], on["hl"] = on["haplotypes"] * (on["motifs_gain"] > 0), on["haplotypes"] * (on["motifs_loss"] > 0)
    on["region"] = on["sequence_name"].map({n_: k for k, n_ in enumerate(t.region_names.tolist())})
    on["to_k"] = on["to"].map({b: k for k, b in enumerate("ACGT")})
    by = on.groupby(["region", "position", "from", "to_k"], sort=True)
    agg = by.agg(versions=("haplotypes", "size"), haplotypes=("haplotypes", "sum"), haplotypes_gain=("hg", "sum"),
                 haplotypes_loss=("hl", "sum"), max_motifs_gain=("motifs_gain", "max"), max_motifs_loss=("motifs_loss", "max")).reset_index()
    assert len(s) == len(agg)
    assert s["position"].tolist() == agg["position"].tolist() and s["from"].tolist() == agg["from"].tolist()
    assert s["to"].tolist() == ["ACGT"[k] for k in agg["to_k"]] and s["sequence_name"].tolist() == t.region_names[agg["region"]].tolist()
    for c in SUMMARY_COLUMNS[4:10]:
        assert s[c].tolist() == agg[c].tolist(), (name, c)
    for side in ("gain", "loss"):
        some = on[on[f"{side}_motif_id"] != ""]
        first = some.sort_values(["region", "position", "from", "to_k", f"{side}_pvalue"], kind="stable").groupby(
            ["region", "position", "from", "to_k"]).first()[f"{side}_motif_id"]
        want_ids = first.reindex(pd.MultiIndex.from_frame(agg[["region", "position", "from", "to_k"]])).fillna("").tolist()
        assert s[f"{side}_motif_id"].tolist() == want_ids, (name, side)
    t.all_rows = False
    kept = (s["haplotypes_gain"] + s["haplotypes_loss"] > 0).to_numpy()
    assert text(t.summary_frame()) == text(s[kept]) and 0 < kept.sum()


def test_refusals(monkeypatch):
    from grafimo_amd.mutation_profile import compute_mutation_profile, profile_sequences
    x = np.frombuffer(b"ACGTACGTACGT", dtype=np.uint8)
    m5 = SynMotif(5, seed=1)
    with pytest.raises(ValueError, match="starts at 0"):
        profile_sequences([m5], [1, 12], x, 0.1)
    with pytest.raises(ValueError, match="2 weight tables for 1 motifs"):
        profile_sequences([m5], [0, 12], x, 0.1, weights=[None, None])
    with pytest.raises(ValueError, match="delta -1"):
        compute_mutation_profile([m5], msbf.hand_graph(), [(0, 20)], False, wp.Args(), delta=-1)
    import torch
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="the mutation profile is computed on one GPU"):
        compute_mutation_profile([m5], msbf.hand_graph(), [(0, 20)], False, wp.Args())


# ------------------------------------------------------------------------------------------- the command line
def test_cli_writes_both_files_and_prints_them(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.mutation_profile import compute_mutation_profile
    from grafimo_amd.workflow import Findmotif
    fa, vcf, bedfile = os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), os.path.join(GOLD, "regions.bed")
    bed = read_bed_regions(bedfile)
    graphs = [GraphIndex.from_fasta_vcf(fa, vcf, c[3:]) for c in bed]
    out = str(tmp_path / "o")
    base = [sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", fa, "-v", vcf, "-b", bedfile, "-t", "0.05",
            "--mutation-profile", "--mutation-profile-delta", "2.5"]
    r = subprocess.run(base + ["-o", out], check=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=600,
                       capture_output=True, text=True)
    assert "mutation profile rows written to" in r.stdout and "mutation profile summary rows written to" in r.stdout
    assert "mutation scan" not in r.stdout                                               # (independent of --mutation-scan)
    wf = Findmotif(threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "MA0139.1.meme"), wf, 2, True, pvalue_matrix=False)[0]
    t = compute_mutation_profile([motif], graphs, list(bed.values()), False, wp.Args(threshold=0.05), delta=2.5)
    detail = open(os.path.join(out, "grafimo_mutation_profile.tsv")).read()
    summary = open(os.path.join(out, "grafimo_mutation_profile_summary.tsv")).read()
    assert detail.split("\n", 1)[0].split("\t") == [c for c in HOST_COLUMNS if c != "haplotypes_g"]
    assert summary.split("\n", 1)[0].split("\t") == SUMMARY_COLUMNS
    assert len(t) > 0 and detail == t.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    assert summary == t.summary_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    r = subprocess.run(base + ["-f"], check=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=600,
                       capture_output=True, text=True)
    assert detail in r.stdout and summary in r.stdout and "written to" not in r.stdout
