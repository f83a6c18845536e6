"""A motif set prepared in one device pass (gfm_comp_pval_mat_many / gfm_motif_create_many: one launch of
pvalue_dp_kernel and one of ptable_kernel for the whole set, one workgroup per motif) gives, motif for motif, what the
single-motif calls give -- byte for byte -- and what the oracle and the golden files hold; and the entry points that create
handles for a set (lease_many, create_many and their call sites) give the tables the per-motif entry points give."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from grafimo_amd import _native as nv          # noqa: E402
from grafimo_amd import synth                   # noqa: E402
from grafimo_amd.device import DeviceMotif, comp_pval_mat_dense   # noqa: E402
from oracle import oracle as orc                # noqa: E402

ACGT = {n: i for i, n in enumerate("ACGT")}


class _Scaled:
    """the members comp_pval_mat / DeviceMotif read of a scaled Motif"""

    def __init__(self, sm, bg, min_val=None, scale=1, offset=0.0, name="m"):
        self.score_matrix = np.asarray(sm, dtype=np.int64)
        self.width = int(self.score_matrix.shape[1])
        self.nucsmap = dict(ACGT)
        self.bg = {n: float(bg[i]) for i, n in enumerate("ACGT")}
        self.min_val = int(self.score_matrix.min()) if min_val is None else int(min_val)
        self.scale, self.offset = int(scale), np.double(offset)
        self.is_scaled = True
        self.motif_id, self.motif_name = name, name.lower()


def _rec_motif(rec, name="m"):
    return _Scaled(rec["sm"], rec["bg"], rec["min_val"], rec["scale"], rec["offset"], name)


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _random_set(widths, seed):
    rng = np.random.default_rng(seed)
    return [synth.synthetic_motif(int(W), rng, rng.dirichlet(np.full(4, 20.0))) for W in widths]


# ------------------------------------------------------------------------------------------------ score distributions
def test_golden_motifs_in_one_call(golden_motifs):
    from grafimo_amd.motif_processing import comp_pval_mat_many
    _, flat = golden_motifs
    keys = sorted(flat)
    assert len(keys) == 24
    got = comp_pval_mat_many([_Scaled(flat[k]["score_matrix"], flat[k]["bg"]) for k in keys], False)
    gold = np.load(os.path.join(GOLDEN, "pmf.npz"))
    for k, pmf in zip(keys, got):
        assert np.array_equal(pmf, gold[k]), k
        assert _same_bytes(pmf, gold[k]), k


@pytest.mark.parametrize("case", ["every_width", "one", "600"])
def test_random_sets_equal_the_oracle_and_the_single_call(case):
    """every width 1..64 in shuffled order with duplicates; a set of one; 600 motifs (more workgroups than the chip holds
    at once: 2 per CU), all byte for byte equal to orc_comp_pval_mat and to gfm_comp_pval_mat"""
    from grafimo_amd.motif_processing import comp_pval_mat_many
    rng = np.random.default_rng({"every_width": 11, "one": 12, "600": 13}[case])
    if case == "every_width":
        recs = _random_set(range(1, 65), 1)
        recs = recs + [recs[i] for i in rng.choice(64, 16, replace=False)]
    elif case == "one":
        recs = _random_set([23], 2)
    else:
        distinct = _random_set(np.arange(150) % 64 + 1, 3)
        recs = [distinct[i] for i in rng.integers(0, len(distinct), 600)]
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order]
    got = comp_pval_mat_many([_rec_motif(r) for r in recs], False)
    assert len(got) == len(recs)
    cache = {}
    for r, pmf in zip(recs, got):
        key = r["sm"].tobytes() + r["bg"].tobytes()
        if key not in cache:
            cache[key] = (orc.comp_pval_mat(r["sm"], r["bg"]), comp_pval_mat_dense(r["sm"], r["bg"]))
        want_orc, want_one = cache[key]
        assert len(pmf) == 1000 * r["width"] + 1
        assert _same_bytes(pmf, want_orc), r["width"]
        assert _same_bytes(pmf, want_one), r["width"]


# ------------------------------------------------------------------------------------------------ handles
def _kmers(W, n, rng):
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTN", dtype=np.uint8)
    return np.ascontiguousarray(rng.choice(alphabet, size=(n, W)))


def _score(dm, kmers):
    dev = torch.device("cuda", torch.cuda.current_device())
    d_k = torch.from_numpy(kmers).to(dev)
    scores = torch.empty(len(kmers), dtype=torch.int32, device=dev)
    hist = torch.zeros(dm.L, dtype=torch.int64, device=dev)
    dm.score(d_k, scores, hist=hist)
    torch.cuda.synchronize()
    return scores.cpu().numpy(), hist.cpu().numpy()


def _assert_same_handle(a, b, kmers):
    pa, ta = a.tables()
    pb, tb = b.tables()
    assert _same_bytes(pa, pb) and _same_bytes(ta, tb)
    assert (a.score_lo, a.score_hi) == (b.score_lo, b.score_hi)
    for t in (1.0, 1e-2, 1e-4, 1e-8):
        assert a.pvalue_cutoff(t) == b.pvalue_cutoff(t), t
    sa, ha = _score(a, kmers)
    sb, hb = _score(b, kmers)
    assert np.array_equal(sa, sb) and np.array_equal(ha, hb)


def test_create_many_with_given_and_device_distributions():
    """gfm_motif_create_many with some pmfs given (one of them NOT the motif's own DP, so that the given one must be the
    one the handle holds) and the others computed in the set's one DP launch == handles created one by one"""
    rng = np.random.default_rng(5)
    recs = _random_set([8, 19, 30, 12, 64, 1, 19, 25], 21)
    motifs = [_rec_motif(r, f"M{i}") for i, r in enumerate(recs)]
    for i in (1, 4, 6):
        motifs[i].pval_matrix = comp_pval_mat_dense(recs[i]["sm"], recs[i]["bg"])
    motifs[6].pval_matrix = orc.comp_pval_mat(recs[6]["sm"], np.array([0.1, 0.4, 0.4, 0.1]))   # not its own
    many = DeviceMotif.create_many(motifs)
    try:
        assert len(many) == len(motifs)
        for m, dm in zip(motifs, many):
            one = DeviceMotif.from_motif(m)
            try:
                _assert_same_handle(dm, one, _kmers(m.width, 5000, rng))
                if hasattr(m, "pval_matrix"):
                    assert _same_bytes(dm.tables()[0], m.pval_matrix)
            finally:
                one.close()
        # use_motif_pmf=False: every DP on the device
        for m, dm in zip(motifs, DeviceMotif.create_many(motifs, use_motif_pmf=False)):
            assert _same_bytes(dm.tables()[0], orc.comp_pval_mat(m.score_matrix, [m.bg[n] for n in "ACGT"]))
            dm.close()
    finally:
        for dm in many:
            dm.close()


def test_a_bad_motif_in_the_middle_creates_nothing():
    recs = _random_set([10, 14, 18, 22, 26], 31)
    motifs = [_rec_motif(r) for r in recs]
    motifs[2].min_val += 1
    lib = nv.lib()
    h = (ctypes.c_void_p * 5)(*([0xBEEF] * 5))
    sm = np.concatenate([m.score_matrix.ravel() for m in motifs])
    widths = np.array([m.width for m in motifs], dtype=np.int32)
    bgs = np.stack([[m.bg[n] for n in "ACGT"] for m in motifs])
    mins = np.array([m.min_val for m in motifs], dtype=np.int32)
    scales = np.array([m.scale for m in motifs], dtype=np.int32)
    offs = np.array([m.offset for m in motifs], dtype=np.float64)
    rc = lib.gfm_motif_create_many(5, nv.ptr(sm), nv.ptr(widths), nv.ptr(bgs), nv.ptr(mins), nv.ptr(scales), nv.ptr(offs),
                                   None, h)
    assert rc == nv.GFM_ERR_INVALID and b"motif 2" in lib.gfm_last_error()
    assert all(x is None for x in h)
    with pytest.raises(nv.NativeError, match="motif 2"):
        DeviceMotif.create_many(motifs)
    motifs[2].min_val -= 1
    dms = DeviceMotif.create_many(motifs)
    for m, dm in zip(motifs, dms):
        assert _same_bytes(dm.tables()[0], orc.comp_pval_mat(m.score_matrix, [m.bg[n] for n in "ACGT"]))
        dm.close()


# ------------------------------------------------------------------------------------------------ motif files
def _meme_motif_by_motif(meme, bg_file, pseudo, norev):
    """build_motif_meme's steps with process_motif_for_logodds (log-odds, scaling, the DP) run per motif"""
    from grafimo_amd.motif import Motif
    from grafimo_amd.motif_ops import _load_bg, _read_meme, norm_motif, process_motif_for_logodds
    from grafimo_amd.motif_processing import apply_pseudocount_meme
    alphabet, raws = _read_meme(meme, True)
    nucsmap = {n: i for i, n in enumerate(alphabet)}
    bgs = _load_bg(bg_file, alphabet, norev, True)
    out = []
    for raw in raws:
        width = int(raw.values.shape[1])
        probs = norm_motif(pd.DataFrame(raw.values, index=alphabet), width, alphabet, True)
        probs = apply_pseudocount_meme(probs.to_numpy(), pseudo, raw.nsites, width, bgs, alphabet, nucsmap, True)
        motif = Motif(probs, width, alphabet, raw.motif_id, raw.motif_name, nucsmap)
        motif.set_bg(bgs)
        out.append(process_motif_for_logodds(motif, True))
    return out


def test_meme_file_in_one_pass_equals_golden_and_motif_by_motif(golden_motifs, capsys):
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.workflow import Findmotif
    _, flat = golden_motifs
    meme = os.path.join(GOLDEN, "synth", "multi.meme")
    for case, bg_name, pseudo, norev in (("multi_meme_bg1", "bg_1.txt", 0.1, False), ("multi_meme_bg2_norev", "bg_2.txt", 0.5, True)):
        bg_file = os.path.join(GOLDEN, "synth", bg_name)
        wf = Findmotif(bgfile=bg_file, pseudo=pseudo, no_reverse=norev, verbose=True)
        capsys.readouterr()
        motifs = get_motif_pwm(meme, wf, 1, True)
        out = capsys.readouterr().out
        assert len(motifs) == 6
        assert out.count("processed in") == 1 and "6 motifs processed in" in out
        singles = _meme_motif_by_motif(meme, bg_file, pseudo, norev)
        capsys.readouterr()
        for k, (m, s) in enumerate(zip(motifs, singles)):
            assert _same_bytes(m.pval_matrix, flat[f"{case}#{k}"]["pmf"]), (case, k)
            assert _same_bytes(m.pval_matrix, s.pval_matrix), (case, k)
            assert np.array_equal(np.asarray(m.score_matrix), np.asarray(s.score_matrix))
            assert (m.min_val, m.scale, m.offset) == (s.min_val, s.scale, s.offset)


# ------------------------------------------------------------------------------------------------ call sites
def _config5_like():
    """twelve of config 5's motifs (two of width 8..11 each, so that widths are shared) and one of them twice"""
    recs = synth.config_motifs(5)
    picked = [0, 1, 2, 3, 4, 5, 6, 7, 18, 19, 20, 21]
    motifs = [synth.motif_object(recs[k], f"C5_{k}") for k in picked]
    return motifs + [motifs[3]], [recs[k] for k in picked] + [recs[3]]


def _assert_frames(got, want, what):
    assert got is not None and want is not None, what
    pd.testing.assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True), check_exact=True, obj=str(what))


def test_graph_motif_set_equals_motif_by_motif(tmp_path):
    from extract_helpers import make_graph_files
    from grafimo_amd.extract_regions import (DeviceGraph, GraphIndex, compute_results_from_graph,
                                             compute_results_from_graph_many)
    from grafimo_amd.workflow import Findmotif
    motifs, _ = _config5_like()
    fasta, vcf = make_graph_files(str(tmp_path), chrom="7", length=3000, n_sites=300, n_samples=30, seed=77, rich=True)
    g = DeviceGraph(GraphIndex.from_fasta_vcf(fasta, vcf, "7"))
    regions = [(0, 700), (900, 2100), (2400, 2990)]
    try:
        for kw in (dict(threshold=0.05), dict(threshold=0.3, qval_t=True, recomb=True)):
            DeviceMotif.drop_kept()
            with contextlib.redirect_stdout(io.StringIO()) as o1:
                singles = [compute_results_from_graph(m, g, regions, True, Findmotif(**kw)) for m in motifs]
            DeviceMotif.drop_kept()                      # the set's handles: made by lease_many in one pass
            with contextlib.redirect_stdout(io.StringIO()) as o2:
                many = compute_results_from_graph_many(motifs, g, regions, True, Findmotif(**kw))
            assert o1.getvalue().count("Scanned sequences:") == o2.getvalue().count("Scanned sequences:") == len(motifs)
            assert sum(len(t) for t in many) > 0
            for m, a, b in zip(motifs, many, singles):
                _assert_frames(a, b, (m.motif_id, kw))
    finally:
        g.close()
        DeviceMotif.drop_kept()


def test_tsv_motif_set_equals_motif_by_motif(tmp_path):
    from grafimo_amd.score_sequences import compute_results, compute_results_many
    from grafimo_amd.workflow import Findmotif
    motifs, recs = _config5_like()
    done = set()
    for m, r in zip(motifs, recs):
        if m.width not in done:
            synth.write_tsv_dir(synth.make_batch(3, 500, m.width, r["probs"], synth.seed_for(m.width)), str(tmp_path))
            done.add(m.width)
    for kw in (dict(threshold=1e-2), dict(threshold=0.5, qval_t=True, recomb=True)):
        wf = Findmotif(cores=2, **kw)
        DeviceMotif.drop_kept()
        with contextlib.redirect_stdout(io.StringIO()):
            singles = [compute_results(m, str(tmp_path), True, wf) for m in motifs]
        DeviceMotif.drop_kept()
        with contextlib.redirect_stdout(io.StringIO()):
            many = compute_results_many(motifs, str(tmp_path), True, wf)
        assert sum(len(t) for t in many) > 0
        for m, a, b in zip(motifs, many, singles):
            _assert_frames(a, b, (m.motif_id, kw))
    DeviceMotif.drop_kept()


def test_lease_many_reuses_kept_handles_and_creates_the_rest_in_one_call(monkeypatch):
    lib = nv.lib()
    real = lib.gfm_motif_create_many
    calls = []

    def spy(n, *args):
        calls.append(n)
        return real(n, *args)

    monkeypatch.setattr(lib, "gfm_motif_create_many", spy)
    recs = _random_set([9, 13, 13, 20, 31], 41)
    motifs = [_rec_motif(r, f"L{i}") for i, r in enumerate(recs)]
    DeviceMotif.drop_kept()
    before = DeviceMotif.lease(motifs[1])
    got = DeviceMotif.lease_many(motifs + [motifs[3]])
    try:
        assert calls == [4]                          # one call for the four misses
        assert got[1] is before                      # the kept handle
        assert got[5] is got[3]                      # the same numbers twice share a handle ...
        calls.clear()
        dist = DeviceMotif.lease_many(motifs + [motifs[3]], distinct=True)
        assert calls == [1]                          # ... unless distinct: the copy is made, the rest are kept ones
        assert all(d is g for d, g in zip(dist[:5], got[:5])) and dist[5] is not dist[3]
        _assert_same_handle(dist[5], dist[3], _kmers(20, 2000, np.random.default_rng(1)))
        for d in dist:
            d.release()
        assert dist[5].handle is None                # the distinct copy is not kept
    finally:
        for d in got:
            d.release()
        before.release()
    DeviceMotif.drop_kept()
