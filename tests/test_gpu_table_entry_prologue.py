"""What the six table entries that score with a motif set share before they launch anything -- the motif-set checks of
gfm_graph_variant_effects, gfm_graph_haplotype_scores, gfm_graph_haplotype_affinity, gfm_graph_variant_affinity,
gfm_graph_query_edits and gfm_sequence_mutation_scan --, through _native directly: two motifs of widths 4 and 5, a NULL motif
handle in the array and an unknown flag bit are each refused with GFM_ERR_INVALID and the entry's message, and no output
buffer is touched; one valid motif on the same input is GFM_OK.  The refusals are made on the host side of the entry: no
kernel sees any of these inputs."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

ENTRIES = ["gfm_graph_variant_effects", "gfm_graph_haplotype_scores", "gfm_graph_haplotype_affinity",
           "gfm_graph_variant_affinity", "gfm_graph_query_edits", "gfm_sequence_mutation_scan"]
ONE_WIDTH = "the motifs of one call have one width and live on one device"
NULL_MOTIF = "NULL motif / device buffer"
UNKNOWN_FLAG = "unknown flag"
SENTINEL = 0x5A
REF_LEN, N_HAP = 200, 4
VP = ctypes.c_void_p


def _index():
    """200 reference bases; an SNV at 50, an insertion of two bases behind 100, a deletion of three bases behind 150; four
    haplotypes: 0 carries nothing, 1 the SNV, 2 the insertion and the deletion, 3 all three"""
    from grafimo_amd.extract_regions import MAX_ALTS, GraphIndex
    rng = np.random.default_rng(12)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = acgt[rng.integers(0, 4, size=REF_LEN)]
    pos = np.array([50, 100, 150], np.int32)
    alt = np.zeros((3, MAX_ALTS), np.uint8)
    alt[0, 0] = acgt[(int(np.nonzero(acgt == ref[50])[0][0]) + 1) % 4]
    bits = np.zeros((3, MAX_ALTS, 64), dtype=bool)
    bits[0, 0, [1, 3]] = True
    bits[1, 0, [2, 3]] = True
    bits[2, 0, [2, 3]] = True
    words = np.packbits(bits, axis=-1, bitorder="little").view(np.uint64).reshape(3, MAX_ALTS, 1)
    return GraphIndex("c", ref, pos, np.array([1, 1, 1], np.uint8), alt, words, N_HAP, del_len=np.array([0, 0, 3], np.int32),
                      ins_len=np.array([0, 2, 0], np.int32), ins_off=np.array([0, 0, 2], np.int32),
                      ins_bases=np.frombuffer(b"GT", dtype=np.uint8).copy())


@pytest.fixture(scope="module")
def world():
    """the graph, a motif of width 4 and one of width 5 on the current device, a weight table that serves both widths"""
    import torch
    from grafimo_amd import synth
    from grafimo_amd.device import DeviceMotif
    from grafimo_amd.extract_regions import DeviceGraph
    g = DeviceGraph(_index())
    dms = []
    for W, seed in ((4, 0), (5, 1)):
        rec = synth.synthetic_motif(W, np.random.default_rng(4100 + seed), np.array([0.3, 0.2, 0.2, 0.3]))
        dms.append(DeviceMotif.lease(synth.motif_object(rec, f"SYN{W}_{seed}")))
    assert [dm.width for dm in dms] == [4, 5]
    weights = torch.ones(dms[1].L, dtype=torch.int64, device=g.device)
    yield g, dms, weights
    for dm in dms:
        dm.release()
    g.close()


def _call(entry, g, handles, weights, flags, fill):
    """one call of `entry` with the motif handles `handles` (None: a NULL handle) over the one region / the two sequences, every
    output buffer filled with the byte `fill` before -> (return code, the output tensors)"""
    import torch
    from grafimo_amd import _native as nv
    from grafimo_amd.device import _stream_ptr
    from grafimo_amd.variant_effects import VARIANT_REC_DTYPE
    lib, dev, M, S = nv.lib(), g.device, len(handles), 3
    buf = lambda nbytes: torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)      # noqa: E731
    arr = lambda ts: (VP * M)(*[t.data_ptr() for t in ts])                              # noqa: E731
    motifs, w = (VP * M)(*handles), (VP * M)(*[weights.data_ptr()] * M)
    starts, stops = np.array([0], np.int64), np.array([REF_LEN], np.int64)
    over, n_win, st = buf(4), ctypes.c_int64(), _stream_ptr(None)
    if entry == "gfm_graph_variant_effects":
        cap = 64
        keys, recs, cnt = [buf(8 * 4 * S) for _ in handles], [buf(cap * VARIANT_REC_DTYPE.itemsize) for _ in handles], \
            [buf(8) for _ in handles]
        rc = lib.gfm_graph_variant_effects(g._h, motifs, M, 1, nv.ptr(starts), nv.ptr(stops), flags, arr(keys), arr(recs),
                                           (ctypes.c_int64 * M)(*[cap] * M), arr(cnt), over.data_ptr(), ctypes.byref(n_win), st)
        outs = keys + recs + cnt + [over]
    elif entry == "gfm_graph_haplotype_scores":
        keys = [buf(8 * (N_HAP + 1)) for _ in handles]
        rc = lib.gfm_graph_haplotype_scores(g._h, motifs, M, 1, nv.ptr(starts), nv.ptr(stops), flags, arr(keys), over.data_ptr(),
                                            0, 0, st)
        outs = keys + [over]
    elif entry == "gfm_graph_haplotype_affinity":
        sums = [buf(8 * (N_HAP + 1)) for _ in handles]
        rc = lib.gfm_graph_haplotype_affinity(g._h, motifs, M, w, 1, 1, nv.ptr(starts), nv.ptr(stops), flags, arr(sums),
                                              over.data_ptr(), 0, 0, st)
        outs = sums + [over]
    elif entry == "gfm_graph_variant_affinity":
        sums = [buf(8 * S * 4 * 2) for _ in handles]
        rc = lib.gfm_graph_variant_affinity(g._h, motifs, M, w, 1, nv.ptr(starts), nv.ptr(stops), flags, arr(sums),
                                            over.data_ptr(), ctypes.byref(n_win), 0, st)
        outs = sums + [over]
    else:
        # two sequences of 10 and 3 bases, without inserted bases: coordinates 20 .. 29 and 40 .. 42
        x = np.frombuffer(b"ACGTTGCAAC" + b"GAT", dtype=np.uint8)
        seq_off = np.array([0, 10, 13], np.int64)
        up = lambda a: torch.from_numpy(np.array(a)).to(dev)                            # noqa: E731  (a writable copy)
        d_x = up(x)
        if entry == "gfm_graph_query_edits":
            coord = np.concatenate([np.arange(20, 30), np.arange(40, 43)]).astype(np.int32)
            # one edit, G -> T at 22 (the first sequence's third base), on both sequences (absent from the second)
            ins = [up(seq_off), d_x, up(coord), up(np.array([22], np.int64)), up(np.array([0, 1], np.int32)), up(x[2:3].copy()),
                   up(np.array([0, 1], np.int32)), up(np.frombuffer(b"T", dtype=np.uint8).copy()), up(np.array([0, 1], np.int32)),
                   up(np.array([0, 0], np.int32))]
            recs = [buf(2 * 32) for _ in handles]
            rc = lib.gfm_graph_query_edits(motifs, M, w, 1, 2, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), 1,
                                           ins[3].data_ptr(), ins[4].data_ptr(), ins[5].data_ptr(), ins[6].data_ptr(),
                                           ins[7].data_ptr(), 2, ins[8].data_ptr(), ins[9].data_ptr(), flags, arr(recs),
                                           over.data_ptr(), st)
            outs = recs + [over]
        else:
            assert entry == "gfm_sequence_mutation_scan"
            keys, sums = [buf(4 * 13 * 5) for _ in handles], [buf(8 * 13 * 5) for _ in handles]
            rc = lib.gfm_sequence_mutation_scan(motifs, M, w, 1, 2, nv.ptr(seq_off), d_x.data_ptr(), flags, arr(keys), arr(sums),
                                                over.data_ptr(), st)
            outs = keys + sums + [over]
    torch.cuda.synchronize()
    return rc, outs


def _refused(entry, world, handles, flags, message):
    from grafimo_amd import _native as nv
    g, _, weights = world
    rc, outs = _call(entry, g, handles, weights, flags, SENTINEL)
    assert rc == nv.GFM_ERR_INVALID
    assert nv.lib().gfm_last_error().decode() == message
    for t in outs:                                         # nothing was launched, cleared or copied
        assert bool((t == SENTINEL).all())


@pytest.mark.parametrize("entry", ENTRIES)
def test_two_widths_are_refused(world, entry):
    dms = world[1]
    _refused(entry, world, [dms[0].handle, dms[1].handle], 0, ONE_WIDTH)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_motif_handle_is_refused(world, entry):
    dms = world[1]
    _refused(entry, world, [dms[0].handle, None], 0, NULL_MOTIF)


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_unknown_flag_bit_is_refused(world, entry):
    dms = world[1]
    _refused(entry, world, [dms[0].handle], 1 << 7, UNKNOWN_FLAG)


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_valid_motif_is_accepted(world, entry):
    import torch
    from grafimo_amd import _native as nv
    g, dms, weights = world
    rc, outs = _call(entry, g, [dms[0].handle], weights, 0, 0)
    assert rc == nv.GFM_OK, nv.lib().gfm_last_error().decode()
    assert int(outs[-1].view(torch.int32).item()) == 0     # neither an overflow nor a bad item / tile
