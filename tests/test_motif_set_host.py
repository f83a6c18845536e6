"""The checks of the motif-set entry points (gfm_comp_pval_mat_many, gfm_motif_create_many) through ctypes.  Every motif
of a set is checked before the device is touched, so these run without a GPU: each bad input returns its code, the
message names the failing motif, and no handle is handed out."""
import ctypes

import numpy as np
import pytest

from grafimo_amd import _native as nv
from grafimo_amd import synth

M = 5
K = 3          # the motif that is made bad


def _set():
    rng = np.random.default_rng(7)
    recs = [synth.synthetic_motif(W, rng, np.full(4, 0.25)) for W in (6, 12, 19, 8, 30)]
    return [dict(sm=r["sm"].copy(), bg=r["bg"].copy(), W=r["width"], min_val=r["min_val"], scale=r["scale"],
                 offset=r["offset"]) for r in recs]


def _arrays(recs):
    sm = np.ascontiguousarray(np.concatenate([r["sm"].ravel() for r in recs]), dtype=np.int64)
    widths = np.array([r["W"] for r in recs], dtype=np.int32)
    bgs = np.ascontiguousarray(np.stack([r["bg"] for r in recs]), dtype=np.float64)
    min_vals = np.array([r["min_val"] for r in recs], dtype=np.int32)
    scales = np.array([r["scale"] for r in recs], dtype=np.int32)
    offsets = np.array([r["offset"] for r in recs], dtype=np.float64)
    return sm, widths, bgs, min_vals, scales, offsets


def _sentinel_handles(n):
    return (ctypes.c_void_p * n)(*([0xDEAD] * n))


def _create(recs, n=None, **null):
    sm, widths, bgs, min_vals, scales, offsets = _arrays(recs)
    n = len(recs) if n is None else n
    out = _sentinel_handles(max(1, len(recs)))
    a = dict(sm=nv.ptr(sm), widths=nv.ptr(widths), bgs=nv.ptr(bgs), min_vals=nv.ptr(min_vals), scales=nv.ptr(scales),
             offsets=nv.ptr(offsets))
    a.update({k: None for k in null})
    rc = nv.lib().gfm_motif_create_many(n, a["sm"], a["widths"], a["bgs"], a["min_vals"], a["scales"], a["offsets"], None, out)
    return rc, nv.lib().gfm_last_error().decode(), list(out)


def _pval(recs, n=None, **null):
    sm, widths, bgs, *_ = _arrays(recs)
    out = np.zeros(int(sum(1000 * r["W"] + 1 for r in recs)) or 1)
    a = dict(sm=nv.ptr(sm), widths=nv.ptr(widths), bgs=nv.ptr(bgs), out=nv.ptr(out))
    a.update({k: None for k in null})
    rc = nv.lib().gfm_comp_pval_mat_many(len(recs) if n is None else n, a["sm"], a["widths"], a["bgs"], a["out"])
    return rc, nv.lib().gfm_last_error().decode(), out


def _bad(kind):
    """the set with motif K made bad in one way -> (recs, expected code)"""
    recs = _set()
    r = recs[K]
    if kind == "width0":
        r["W"], r["sm"] = 0, np.zeros((4, 0), dtype=np.int64)
    elif kind == "width65":
        r["W"], r["sm"], r["min_val"] = 65, np.zeros((4, 65), dtype=np.int64), 0
    elif kind == "score_neg":
        r["sm"][2, 1], r["min_val"] = -1, -1
    elif kind == "score_big":
        r["sm"][1, 3] = 1001
    elif kind == "bg0":
        r["bg"][2] = 0.0
        return recs, nv.GFM_ERR_ASSERT
    elif kind == "min_val":
        r["min_val"] = int(r["sm"].min()) + 1
    elif kind == "scale":
        r["scale"] = 0
    return recs, nv.GFM_ERR_INVALID


CREATE_KINDS = ["width0", "width65", "score_neg", "score_big", "bg0", "min_val", "scale"]
PVAL_KINDS = ["width0", "width65", "score_neg", "score_big", "bg0"]


@pytest.mark.parametrize("kind", CREATE_KINDS)
def test_create_many_refuses_a_bad_motif_and_names_it(kind):
    recs, code = _bad(kind)
    rc, msg, out = _create(recs)
    assert rc == code, (rc, msg)
    assert f"motif {K}" in msg, msg
    assert all(h is None for h in out), out


@pytest.mark.parametrize("kind", PVAL_KINDS)
def test_pval_mat_many_refuses_a_bad_motif_and_names_it(kind):
    recs, code = _bad(kind)
    rc, msg, out = _pval(recs)
    assert rc == code, (rc, msg)
    assert f"motif {K}" in msg, msg
    assert not out.any()            # nothing was written


def test_the_first_bad_motif_is_the_one_named():
    recs = _set()
    recs[1]["bg"][0] = 0.0
    recs[4]["sm"][0, 0] = 5000
    rc, msg, out = _create(recs)
    assert rc == nv.GFM_ERR_ASSERT and "motif 1" in msg and "bg > 0" in msg
    rc, msg, _ = _pval(recs)
    assert rc == nv.GFM_ERR_ASSERT and "motif 1" in msg


def test_messages_keep_the_single_calls_wording():
    recs, _ = _bad("width65")
    assert "width 65 outside [1, 64]" in _create(recs)[1]
    recs, _ = _bad("score_big")
    assert "scaled score 1001 outside [0, 1000]" in _create(recs)[1]
    recs, _ = _bad("min_val")
    assert "is not the minimum of the score matrix" in _create(recs)[1]
    recs, _ = _bad("scale")
    assert "scale must be a positive integer" in _create(recs)[1]


def test_negative_count():
    recs = _set()
    rc, msg, _ = _create(recs, n=-1)           # (out has no entries to clear)
    assert rc == nv.GFM_ERR_INVALID and "negative" in msg
    rc, msg, _ = _pval(recs, n=-1)
    assert rc == nv.GFM_ERR_INVALID and "negative" in msg


@pytest.mark.parametrize("arg", ["sm", "widths", "bgs", "min_vals", "scales", "offsets"])
def test_create_many_null_arrays(arg):
    rc, msg, out = _create(_set(), **{arg: True})
    assert rc == nv.GFM_ERR_INVALID and "NULL" in msg
    assert all(h is None for h in out)


@pytest.mark.parametrize("arg", ["sm", "widths", "bgs", "out"])
def test_pval_mat_many_null_arrays(arg):
    rc, msg, _ = _pval(_set(), **{arg: True})
    assert rc == nv.GFM_ERR_INVALID and "NULL" in msg


def test_create_many_null_out():
    sm, widths, bgs, min_vals, scales, offsets = _arrays(_set())
    rc = nv.lib().gfm_motif_create_many(M, nv.ptr(sm), nv.ptr(widths), nv.ptr(bgs), nv.ptr(min_vals), nv.ptr(scales),
                                        nv.ptr(offsets), None, None)
    assert rc == nv.GFM_ERR_INVALID


def test_an_empty_set_is_no_error_and_touches_no_device():
    out = _sentinel_handles(1)
    assert nv.lib().gfm_motif_create_many(0, None, None, None, None, None, None, None, out) == nv.GFM_OK
    assert nv.lib().gfm_comp_pval_mat_many(0, None, None, None, None) == nv.GFM_OK


def test_the_single_calls_are_the_one_motif_case():
    """gfm_motif_create / gfm_comp_pval_mat check as before, the message naming motif 0"""
    h = ctypes.c_void_p(0xDEAD)
    sm = np.zeros((4, 3), dtype=np.int64)
    bg = np.array([0.25, 0.25, 0.0, 0.5])
    assert nv.lib().gfm_motif_create(nv.ptr(sm), 3, nv.ptr(bg), 0, 1, 0.0, None, ctypes.byref(h)) == nv.GFM_ERR_ASSERT
    assert h.value is None and "motif 0" in nv.lib().gfm_last_error().decode()
    out = np.zeros(3001)
    assert nv.lib().gfm_comp_pval_mat(nv.ptr(sm), 3, nv.ptr(bg), nv.ptr(out)) == nv.GFM_ERR_ASSERT
    assert nv.lib().gfm_comp_pval_mat(nv.ptr(sm), 3, None, nv.ptr(out)) == nv.GFM_ERR_INVALID
