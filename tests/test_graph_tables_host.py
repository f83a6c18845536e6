"""The graph-table fuzz's pieces without a GPU: the brute forces' haplotype-class memo against the plain brute forces, and the
random-bitset GraphIndex builder (odd haplotype counts) against GraphIndex and the library's graph checks."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict  # noqa: E402
from graph_table_checks import random_bitset_index  # noqa: E402
from haplotype_bruteforce import haplotype_matrix  # noqa: E402
from haplotype_score_bruteforce import haplotype_score_keys  # noqa: E402
from variant_bruteforce import best_hits, haplotype_classes, spell  # noqa: E402


def _motif(W, seed):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(4100 + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


def _few_site_index(n_hap, seed):
    """few sites, many haplotypes: most haplotypes share their alleles with others"""
    return random_bitset_index(n_hap, seed, length=90, n_sites=4)


@pytest.mark.parametrize("make", ["vcf", "bits", "few"])
@pytest.mark.parametrize("W,no_reverse", [(1, False), (5, True), (9, False)])
def test_memo_equals_plain_brute_forces(tmp_path, monkeypatch, make, W, no_reverse):
    """memo=True spells one haplotype per class (counted at each brute force's spell) and gives the plain result"""
    import haplotype_bruteforce
    import haplotype_score_bruteforce
    import variant_bruteforce
    from grafimo_amd.extract_regions import GraphIndex
    if make == "vcf":
        fa, vcf = make_consistent_graph_files(str(tmp_path), length=160, n_samples=5, seed=W, kinds="sidmDOc")
        idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    elif make == "bits":
        idx = random_bitset_index(67, 10 + W, length=150, n_sites=16)
    else:
        idx = _few_site_index(150, W)
    H = idx.n_haplotypes
    first, cls = haplotype_classes(idx)
    assert len(cls) == H and (cls[first] == np.arange(len(first))).all()
    if make == "few":
        assert len(first) < H // 4
    for h in range(H):                                    # a class spells one sequence
        assert spell(idx, h)[0] == spell(idx, int(first[cls[h]]))[0]
    calls = []
    for mod in (haplotype_bruteforce, haplotype_score_bruteforce, variant_bruteforce):
        monkeypatch.setattr(mod, "spell", lambda index, h: calls.append(h) or spell(index, h))

    def spelled(f, *a, **kw):
        calls.clear()
        out = f(*a, **kw)
        return out, len(calls)

    od = motif_as_oracle_dict(_motif(W, W))
    sm, mv = od["score_matrix"], od["min_val"]
    regions = [(0, 100), (40, 200), (-5, 30), (7, 7), (60, 61)]
    (a, na), (b, nb) = (spelled(best_hits, idx, regions, W, sm, mv, no_reverse, memo=m) for m in (True, False))
    assert a == b and (na, nb) == (len(first), H)
    (a, na), (b, nb) = (spelled(haplotype_score_keys, idx, regions, W, sm, mv, no_reverse, memo=m) for m in (True, False))
    assert (a == b).all() and (na, nb) == (len(first) + 1, H + 1)      # (+ the reference path)
    cut = int(sm.min(0).sum() + sm.max(0).sum()) // 2               # about half the rows count
    (a, na), (b, nb) = (spelled(haplotype_matrix, idx, regions, W, sm, mv, cut, no_reverse, memo=m) for m in (True, False))
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (na, nb) == (len(first), H)
    assert b[0].sum() > 0


def test_classes_of_a_graph_without_sites():
    from grafimo_amd.extract_regions import GraphIndex
    idx = GraphIndex("c", np.frombuffer(b"ACGT" * 10, dtype=np.uint8), np.zeros(0, np.int32), np.zeros(0, np.uint8),
                     np.zeros((0, 3), np.uint8), np.zeros((0, 3, 1), np.uint64), 5)
    first, cls = haplotype_classes(idx)
    assert first.tolist() == [0] and cls.tolist() == [0] * 5


@pytest.mark.parametrize("n_hap", [1, 63, 64, 65, 127, 129, 150])
def test_random_bitset_index_is_a_valid_graph(n_hap):
    """the builder's indexes: the shapes GraphIndex keeps, tail bits beyond H clear, one allele per haplotype and site, no site
    inside a deletion, and the checks DeviceGraph's gfm_graph_create makes pass (gfm_graph_validate: on the host only)"""
    from grafimo_amd import _native as nv
    idx = random_bitset_index(n_hap, 500 + n_hap, length=240, n_sites=30)
    hw = (n_hap + 63) // 64
    S = len(idx.pos)
    assert idx.n_haplotypes == n_hap and idx.hw == hw and idx.alt_bits.shape == (S, 3, hw) and S > 5
    assert (np.diff(idx.pos) > 0).all() and idx.pos[-1] < len(idx.ref)
    bits = np.unpackbits(idx.alt_bits.view(np.uint8), axis=-1, bitorder="little")          # [S, 3, 64 hw]
    assert not bits[..., n_hap:].any()
    assert (bits.sum(axis=1) <= 1).all()
    for k in range(3):
        assert not bits[idx.n_alts <= k, k].any()
    for i in np.nonzero(idx.del_len)[0]:
        assert i + 1 == S or idx.pos[i + 1] > idx.pos[i] + idx.del_len[i]
        assert idx.pos[i] + idx.del_len[i] < len(idx.ref)
    assert ((idx.del_len > 0) | (idx.ins_len > 0) <= (idx.n_alts == 1)).all()
    for i in np.nonzero((idx.del_len == 0) & (idx.ins_len == 0))[0]:
        alts = idx.alt_bases[i, :idx.n_alts[i]].tolist()
        assert len(set(alts)) == len(alts) and idx.ref[idx.pos[i]] not in alts and set(alts) <= set(b"ACGT")

    def validate(pos):
        return nv.lib().gfm_graph_validate(
            nv.ptr(idx.ref), len(idx.ref), S, nv.ptr(pos), nv.ptr(idx.n_alts), nv.ptr(idx.alt_bases), nv.ptr(idx.del_len),
            nv.ptr(idx.ins_len), nv.ptr(idx.ins_off), nv.ptr(idx.ins_bases) if len(idx.ins_bases) else None, len(idx.ins_bases),
            n_hap)

    assert validate(idx.pos) == 0, nv.lib().gfm_last_error()
    swapped = idx.pos.copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    assert validate(swapped) == nv.GFM_ERR_INVALID and b"ascending" in nv.lib().gfm_last_error()
