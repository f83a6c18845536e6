"""The scan fold and the mutation profile without a GPU: the brute force (tests/mutation_profile_bruteforce.py) on hand-made
cases whose answers are written out here, its split and order independence, every refusal of gfm_scan_fold (host pointers only:
each is made before any device work), the frames of a table built from a hand-made state, the command line's refusals."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mutation_profile_bruteforce as bf  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
PT = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.25, 0.25, 0.1]     # a tail table of 9 entries, two of them equal
U64 = (1 << 64) - 1


def key(score, rel=0, plus=1):
    return ((score + 1) << 8) | ((64 - rel) << 1) | plus


def _one_cell(motifs, pairs=((0, 1),)):
    """motifs: (id, cutoff, ptable, (ref key, alt key), (ref sum, alt sum)) over one row of two columns -> the state's cell"""
    st = bf.fold_all([[list(m[3])] for m in motifs], [[list(m[4])] for m in motifs], [m[0] for m in motifs], [m[1] for m in motifs],
                     [m[2] for m in motifs], list(pairs))
    return {k: v[0, 0].tolist() for k, v in st.items()}


# ------------------------------------------------------------------------------------------- the rule on hand-made cases
def test_a_p_tie_goes_to_the_smaller_id():
    # both gain with p = 0.25 (scores 6 and 7): id 1 wins whatever the order; its keys and its p are kept
    a, b = (3, 5, PT, (key(2), key(6)), (1, 1)), (1, 5, PT, (0, key(7)), (1, 1))
    for order in ((a, b), (b, a)):
        c = _one_cell(order)
        assert c["counts"] == [2, 0] and c["site_motif"] == [2, 0] and c["site_p"] == [0.25, 0.0]
        assert c["site_keys"] == [[0, key(7)], [0, 0]] and c["aff_motif"] == [0, 0] and c["aff_sums"] == [[0, 0], [0, 0]]
    # a smaller p beats a smaller id
    c = _one_cell([a, (0, 5, PT, (key(1), key(5)), (1, 1)), (7, 5, PT, (key(4), key(8)), (1, 1))])
    assert c["counts"] == [3, 0] and c["site_motif"] == [8, 0] and c["site_p"] == [0.1, 0.0] and c["site_keys"][0] == [key(4), key(8)]


def test_equal_ratios_tie_and_go_to_the_smaller_id():
    # down: 4 -> 2 against 2 -> 1, both R / A = 2
    a, b = (0, 5, PT, (0, 0), (4, 2)), (1, 5, PT, (0, 0), (2, 1))
    for order in ((a, b), (b, a)):
        c = _one_cell(order)
        assert c["aff_motif"] == [0, 1] and c["aff_sums"] == [[0, 0], [4, 2]] and c["counts"] == [0, 0]
    # the larger ratio wins against the smaller id: 2 -> 5 (x 2.5) against 4 -> 9 (x 2.25)
    c = _one_cell([(0, 5, PT, (0, 0), (4, 9)), (6, 5, PT, (0, 0), (2, 5))])
    assert c["aff_motif"] == [7, 0] and c["aff_sums"] == [[2, 5], [0, 0]]


def test_a_reference_sum_of_zero_is_an_infinite_ratio():
    inf5, fin2, inf4 = (5, 5, PT, (0, 0), (0, 1)), (2, 5, PT, (0, 0), (1, 1000)), (4, 5, PT, (0, 0), (0, 99))
    for order in itertools.permutations((inf5, fin2)):
        c = _one_cell(order)
        assert c["aff_motif"] == [6, 0] and c["aff_sums"] == [[0, 1], [0, 0]]               # infinite beats finite
    for order in itertools.permutations((inf5, fin2, inf4)):
        c = _one_cell(order)
        assert c["aff_motif"] == [5, 0] and c["aff_sums"] == [[0, 99], [0, 0]]              # two infinite ones tie: id 4
    # and downwards: an ALT sum of 0
    c = _one_cell([(3, 5, PT, (0, 0), (1000, 1)), (9, 5, PT, (0, 0), (7, 0))])
    assert c["aff_motif"] == [0, 10] and c["aff_sums"] == [[0, 0], [7, 0]]


def test_key_zero_on_either_side():
    c = _one_cell([(0, 3, PT, (0, key(3)), (0, 5))])
    assert c["counts"] == [1, 0] and c["site_motif"] == [1, 0] and c["site_keys"][0] == [0, key(3)] and c["site_p"][0] == 0.7
    c = _one_cell([(0, 3, PT, (key(4), 0), (5, 0))])
    assert c["counts"] == [0, 1] and c["site_motif"] == [0, 1] and c["site_keys"][1] == [key(4), 0] and c["site_p"][1] == 0.6
    c = _one_cell([(0, 3, PT, (0, 0), (0, 0))])
    assert c == {"counts": [0, 0], "site_motif": [0, 0], "site_keys": [[0, 0], [0, 0]], "site_p": [0.0, 0.0], "aff_motif": [0, 0],
                 "aff_sums": [[0, 0], [0, 0]]}
    # both sides are sites, or neither: no gain and no loss
    assert _one_cell([(0, 3, PT, (key(3), key(8)), (1, 1))])["counts"] == [0, 0]
    assert _one_cell([(0, 3, PT, (key(2), key(1)), (1, 1))])["counts"] == [0, 0]


def test_cutoff_zero_and_cutoff_at_the_table_length():
    # cutoff 0: every key but 0 is a site
    c = _one_cell([(0, 0, PT, (key(0), 0), (1, 1))])
    assert c["counts"] == [0, 1] and c["site_p"] == [0.0, 1.0]
    assert _one_cell([(0, 0, PT, (key(0), key(8)), (1, 1))])["counts"] == [0, 0]
    # cutoff = table_len: no score of the table is a site; a score beyond it is, and reads the last entry
    assert _one_cell([(0, 9, PT, (key(0), key(8)), (1, 1))])["counts"] == [0, 0]
    c = _one_cell([(0, 9, PT, (key(8), key(12)), (1, 1))])
    assert c["counts"] == [1, 0] and c["site_p"] == [0.1, 0.0] and c["site_keys"][0] == [key(8), key(12)]


def test_sums_where_64_bit_products_wrap():
    # up: (2^64 - 1) / (2^64 - 2) against 2^63 / (2^63 - 1): the second is larger; modulo 2^64 the products say the opposite
    a, b = (0, 5, PT, (0, 0), (U64 - 1, U64)), (1, 5, PT, (0, 0), ((1 << 63) - 1, 1 << 63))
    assert (U64 * ((1 << 63) - 1)) % (1 << 64) > ((1 << 63) * (U64 - 1)) % (1 << 64)
    for order in ((a, b), (b, a)):
        c = _one_cell(order)
        assert c["aff_motif"] == [2, 0] and c["aff_sums"] == [[(1 << 63) - 1, 1 << 63], [0, 0]]
    # both sums 2^64 - 1: neither up nor down
    assert _one_cell([(0, 5, PT, (0, 0), (U64, U64))])["aff_motif"] == [0, 0]
    # down with the largest sums
    c = _one_cell([(4, 5, PT, (0, 0), (U64, U64 - 1)), (2, 5, PT, (0, 0), (U64, 1))])
    assert c["aff_motif"] == [0, 3] and c["aff_sums"] == [[0, 0], [U64, 1]]


def test_pairs_read_their_own_columns():
    keys, sums = [[key(1), key(6), 0, key(7), key(2), 0, key(8)]], [[5, 6, 7, 1, 7, 9, 0]]
    st = bf.fold_all([keys], [sums], [11], [5], [PT], bf.INDEL_PAIRS)
    assert st["counts"][0].tolist() == [[1, 0], [1, 0], [0, 0], [0, 0], [1, 0]]
    assert st["site_p"][0, :, 0].tolist() == [0.25, 0.25, 0.0, 0.0, 0.1]
    assert st["aff_motif"][0].tolist() == [[12, 0], [0, 12], [0, 0], [12, 0], [0, 12]]
    assert st["aff_sums"][0, 1].tolist() == [[0, 0], [7, 1]] and st["aff_sums"][0, 3].tolist() == [[7, 9], [0, 0]]


def test_the_brute_force_does_not_depend_on_split_or_order():
    rng = np.random.default_rng(81_000)
    keys, sums, ids, cutoffs, ptables = bf.random_case(rng, 23, 5, 9)
    whole = bf.fold_all(keys, sums, ids, cutoffs, ptables, bf.MUTATION_PAIRS)
    assert whole["counts"].sum() > 0 and (whole["site_motif"] > 0).any() and (whole["aff_motif"] > 0).any(axis=(0, 1)).all()
    take = lambda idx: [[v[i] for i in idx] for v in (keys, sums, ids, cutoffs, ptables)]    # noqa: E731
    for order in (list(range(9))[::-1], rng.permutation(9).tolist()):
        assert bf.same_state(bf.fold_all(*take(order), bf.MUTATION_PAIRS), whole), bf.first_difference(bf.fold_all(*take(order), bf.MUTATION_PAIRS), whole)
        st = bf.empty_state(23, 4)
        for a in range(0, 9, 4):
            st = bf.fold(st, *take(order[a:a + 4]), bf.MUTATION_PAIRS)
        assert bf.same_state(st, whole)
    by_id = np.argsort(ids).tolist()
    one = bf.empty_state(23, 4)
    for i in by_id[::-1]:
        one = bf.fold(one, *take([i]), bf.MUTATION_PAIRS)
    assert bf.same_state(one, whole)


# ------------------------------------------------------------------------------------------- the library's refusals
def _fold_args(**over):
    """a call gfm_scan_fold would accept, the `device` buffers on the host (no call that passes the checks is ever made)"""
    M, rows, C, P = 2, 4, 5, 4
    hold = dict(ids=np.array([4, 0], dtype=np.int32), cutoffs=np.array([3, 9], dtype=np.int32), lens=np.array([9, 9], dtype=np.int32),
                pt=[np.array(PT), np.array(PT)], pairs=np.array(bf.MUTATION_PAIRS, dtype=np.int32),
                keys=[np.zeros((rows, C), dtype=np.uint32) for _ in range(M)], sums=[np.zeros((rows, C), dtype=np.uint64) for _ in range(M)],
                state=[v for v in bf.empty_state(rows, P).values()], n_motifs=M, n_rows=rows, C=C, P=P)
    hold.update(over)
    return hold


def _fold(h):
    import ctypes
    from grafimo_amd import _native as nv
    vp = ctypes.c_void_p
    arr = lambda v: None if v is None else (vp * len(v))(*[nv.ptr(x) for x in v])               # noqa: E731
    st = h["state"]
    rc = nv.lib().gfm_scan_fold(h["n_motifs"], nv.ptr(h["ids"]), nv.ptr(h["cutoffs"]), arr(h["pt"]), nv.ptr(h["lens"]), h["n_rows"],
                                h["C"], h["P"], nv.ptr(h["pairs"]), arr(h["keys"]), arr(h["sums"]), *[nv.ptr(a) for a in st], None)
    return rc, nv.lib().gfm_last_error().decode()


REFUSALS = [
    ("no motif", dict(n_motifs=0), "n_motifs < 1"),
    ("negative rows", dict(n_rows=-1), "n_rows"),
    ("one column", dict(C=1), "n_columns 1 is outside 2 .. 8"),
    ("nine columns", dict(C=9), "n_columns 9 is outside 2 .. 8"),
    ("no pair", dict(P=0), "n_pairs 0 is outside 1 .. 8"),
    ("nine pairs", dict(P=9), "n_pairs 9 is outside 1 .. 8"),
    ("NULL ids", dict(ids=None), "NULL argument"),
    ("NULL cutoffs", dict(cutoffs=None), "NULL argument"),
    ("NULL tables", dict(pt=None), "NULL argument"),
    ("NULL lengths", dict(lens=None), "NULL argument"),
    ("NULL pairs", dict(pairs=None), "NULL argument"),
    ("NULL keys", dict(keys=None), "NULL argument"),
    ("NULL sums", dict(sums=None), "NULL argument"),
    ("a pair beyond the columns", dict(pairs=np.array([[0, 1], [0, 5], [0, 3], [0, 4]], dtype=np.int32)), "pair 1 (0, 5)"),
    ("a negative column", dict(pairs=np.array([[0, 1], [0, 2], [-1, 3], [0, 4]], dtype=np.int32)), "pair 2 (-1, 3)"),
    ("ref == alt", dict(pairs=np.array([[0, 1], [0, 2], [0, 3], [4, 4]], dtype=np.int32)), "pair 3 (4, 4)"),
    ("a negative id", dict(ids=np.array([4, -2], dtype=np.int32)), "motif id -2 is negative"),
    ("a repeated id", dict(ids=np.array([4, 4], dtype=np.int32)), "motif id 4 is repeated"),
    ("an empty table", dict(lens=np.array([9, 0], dtype=np.int32), cutoffs=np.array([3, 0], dtype=np.int32)), "table_len 0 of motif 1"),
    ("a negative cutoff", dict(cutoffs=np.array([-1, 9], dtype=np.int32)), "cutoff -1 of motif 0 is outside 0 .. 9"),
    ("a cutoff beyond the table", dict(cutoffs=np.array([3, 10], dtype=np.int32)), "cutoff 10 of motif 1 is outside 0 .. 9"),
]


@pytest.mark.parametrize("what,over,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_library_refuses(what, over, message):
    from grafimo_amd import _native as nv
    rc, said = _fold(_fold_args(**over))
    assert rc == nv.GFM_ERR_INVALID and "gfm_scan_fold" in said and message in said, said


def test_the_library_refuses_null_and_misaligned_buffers():
    from grafimo_amd import _native as nv
    for name in range(6):                                                      # each of the six state pointers
        h = _fold_args()
        h["state"][name] = None
        rc, said = _fold(h)
        assert rc == nv.GFM_ERR_INVALID and "gfm_scan_fold: NULL argument" in said, (name, said)
    for field in ("keys", "sums", "pt"):                                       # a motif's own buffer
        h = _fold_args()
        h[field] = [h[field][0], None]
        rc, said = _fold(h)
        assert rc == nv.GFM_ERR_INVALID and "gfm_scan_fold: NULL device buffer of motif 1" in said, (field, said)
    odd = np.zeros(4 * 5 * 2 + 1, dtype=np.uint32)                             # 4 bytes past an 8-byte boundary
    h = _fold_args()
    h["sums"] = [h["sums"][0], odd[1:].ctypes.data if odd.ctypes.data % 8 == 0 else odd.ctypes.data]
    rc, said = _fold(h)
    assert rc == nv.GFM_ERR_INVALID and "gfm_scan_fold: d_sums[m]" in said and "8-byte aligned" in said, said
    for name in (3, 5):                                                        # site_p, aff_sums
        h = _fold_args()
        h["state"][name] = odd[1:].ctypes.data if odd.ctypes.data % 8 == 0 else odd.ctypes.data
        rc, said = _fold(h)
        assert rc == nv.GFM_ERR_INVALID and "gfm_scan_fold: site_p and aff_sums are 8-byte aligned" in said, said


def test_no_row_is_a_no_op_and_the_abi_is_still_12():
    from grafimo_amd import _native as nv
    lib = nv.lib()
    assert lib.gfm_abi_version() == nv.ABI_VERSION == 12
    name = "gfm_scan_fold"
    assert name in nv.PROTOTYPES and hasattr(lib, name) and len(nv.PROTOTYPES[name][1]) == 18
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert f"int {name}(" in header and "does NOT wait for the stream" in header
    assert lib.gfm_scan_fold(1, None, None, None, None, 0, 5, 4, None, None, None, None, None, None, None, None, None, None) == nv.GFM_OK
    # the counts are looked at first, with no row too
    assert lib.gfm_scan_fold(0, None, None, None, None, 0, 5, 4, None, None, None, None, None, None, None, None, None, None) == nv.GFM_ERR_INVALID
    assert lib.gfm_scan_fold(1, None, None, None, None, 0, 9, 4, None, None, None, None, None, None, None, None, None, None) == nv.GFM_ERR_INVALID


def test_header_module_and_brute_force_state_one_rule():
    from grafimo_amd import mutation_profile
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    squeeze = lambda s: " ".join(s.replace("*", " ").split())                   # noqa: E731
    texts = [squeeze(header), squeeze(mutation_profile.__doc__), squeeze(bf.__doc__)]
    for line in ("A side is a site when its key is not 0 and its score >= cutoff",
                 "gain when a is a site and r is not. loss when r is a site and a is not.",
                 "counts[gain] and counts[loss] count the motifs.",
                 "Gain champion: the gaining motif with the smallest ptable[a].",
                 "Loss champion: the losing motif with the smallest ptable[r].",
                 "A score >= table_len reads entry table_len - 1",
                 "A1 R2 > A2 R1",
                 "The empty state is all zero bytes. Ids are stored as id + 1"):
        for text in texts:
            assert line in text, line
    assert mutation_profile.STATE_BYTES == sum(np.dtype(v.dtype).itemsize * v[0, 0].size for v in bf.empty_state(1, 1).values()) == 88
    assert mutation_profile.STATE_BYTES_PER_BASE == 352 and list(mutation_profile.PAIRS) == bf.MUTATION_PAIRS
    assert mutation_profile.STATE_NAMES == bf.NAMES


# ------------------------------------------------------------------------------------------- the frames of a hand-made state
COLUMNS = ["sequence_name", "version", "haplotypes", "haplotypes_g", "is_reference", "position", "inserted", "from", "to", "motifs_gain",
           "motifs_loss"] + \
    [f"{side}_{c}" for side in ("gain", "loss") for c in ("motif_id", "motif_alt_id", "ref_score", "alt_score", "pvalue", "start", "strand",
                                                           "kmer")] + \
    ["up_motif_id", "up_delta_log2_affinity", "down_motif_id", "down_delta_log2_affinity"]
SUMMARY_COLUMNS = ["sequence_name", "position", "from", "to", "versions", "haplotypes", "haplotypes_gain", "haplotypes_loss",
                   "max_motifs_gain", "max_motifs_loss", "gain_motif_id", "loss_motif_id"]


def _hand_profile(**kw):
    """Region c:10-15 in three sequences: version 0 (3 haplotypes) ACGTAC with an inserted G behind coordinate 11, version 1 (1
    haplotype) ATTAC, and the count-0 reference ACTAC.  Two motifs: MA of width 3, MB of width 5.  Seven cells of the state are
    set by hand."""
    from grafimo_amd.mutation_profile import FoldState, MutationProfile
    bases = np.frombuffer(b"ACGTAC" + b"ATTAC" + b"ACTAC", dtype=np.uint8)
    coord = [10, 11, ~11, 12, 13, 14] + [10, 11, 12, 13, 14] + [10, 11, 12, 13, 14]
    st = FoldState.host_zeros(16, 4)
    A, C, G, T = 0, 1, 2, 3                                                        # the pair of a to-base
    # version 0, offset 1 (C at 11) -> T: two motifs gain; MB's site on - from offset 0; MA's affinity x 8
    st.counts[1, T] = [2, 0]; st.site_motif[1, T, 0] = 2; st.site_keys[1, T, 0] = [key(40, -1, 1), key(480, -1, 0)]
    st.site_p[1, T, 0] = 0.001; st.aff_motif[1, T, 0] = 1; st.aff_sums[1, T, 0] = [4, 32]
    # version 0, offset 2 (the inserted G) -> A: MA loses its site at offsets 0 .. 2; MB's affinity / 4
    st.counts[2, A] = [0, 1]; st.site_motif[2, A, 1] = 1; st.site_keys[2, A, 1] = [key(25, -2, 1), key(3, 0, 1)]
    st.site_p[2, A, 1] = 0.01; st.aff_motif[2, A, 1] = 2; st.aff_sums[2, A, 1] = [64, 16]
    # version 0, offset 0 (A at 10) -> T: three gain, MB the champion with p = 0.03
    st.counts[0, T] = [3, 0]; st.site_motif[0, T, 0] = 2; st.site_keys[0, T, 0] = [key(100, 0, 1), key(450, 0, 1)]; st.site_p[0, T, 0] = 0.03
    # version 1, offset 0 (A at 10) -> T: MA gains with the same p = 0.03
    st.counts[6, T] = [1, 0]; st.site_motif[6, T, 0] = 1; st.site_keys[6, T, 0] = [key(5, 0, 1), key(20, 0, 1)]; st.site_p[6, T, 0] = 0.03
    # the reference, offset 1 (C at 11) -> G: MA gains
    st.counts[12, G] = [1, 0]; st.site_motif[12, G, 0] = 1; st.site_keys[12, G, 0] = [0, key(30, 0, 1)]; st.site_p[12, G, 0] = 0.02
    # version 0, offset 4 (A at 13) -> C: MB's affinity rises from 0; offset 5 (C at 14) -> A: MA's x 1.5
    st.aff_motif[4, C, 0] = 2; st.aff_sums[4, C, 0] = [0, 8]
    st.aff_motif[5, A, 0] = 1; st.aff_sums[5, A, 0] = [8, 12]
    return MutationProfile(["MA", "MB"], ["a", "b"], [3, 5], [10, 100], [0.5, -0.25], [1.0, 2.0], 0.05, ["c:10-15"], ["g"], [0, 0, 0],
                           [0, 1, -1], [3, 1, 0], [[2], [0], [0]], [False, False, True], [0, 6, 11, 16], bases, coord, st, **kw)


def _same(x, y):
    return x == y or (x != x and y != y)


def test_frames_of_a_hand_made_state():
    nan = float("nan")
    t = _hand_profile()
    f = t.to_frame()
    assert list(f.columns) == COLUMNS and len(f) == len(t) == 5
    rows = f.to_dict("records")
    # (sequence, offset, to A C G T) order
    assert [(r["version"], r["position"], r["inserted"], r["from"], r["to"]) for r in rows] == \
        [(0, 11, False, "A", "T"), (0, 12, False, "C", "T"), (0, 12, True, "G", "A"), (1, 11, False, "A", "T"), (-1, 12, False, "C", "G")]
    want = {"sequence_name": "c:10-15", "version": 0, "haplotypes": 3, "haplotypes_g": 2, "is_reference": False, "position": 12,
            "inserted": False, "from": "C", "to": "T", "motifs_gain": 2, "motifs_loss": 0, "gain_motif_id": "MB", "gain_motif_alt_id": "b",
            "gain_ref_score": 40 / 100 + 5 * -0.25, "gain_alt_score": 480 / 100 + 5 * -0.25, "gain_pvalue": 0.001, "gain_start": -1.0,
            "gain_strand": "-", "gain_kmer": "TACAT",                        # ACGTA with T at its offset 1, reverse complemented
            "loss_motif_id": "", "loss_motif_alt_id": "", "loss_ref_score": nan, "loss_alt_score": nan, "loss_pvalue": nan,
            "loss_start": nan, "loss_strand": "", "loss_kmer": "", "up_motif_id": "MA", "up_delta_log2_affinity": 3.0,
            "down_motif_id": "", "down_delta_log2_affinity": nan}
    assert set(want) == set(COLUMNS)
    for c in COLUMNS:
        assert _same(rows[1][c], want[c]), (c, rows[1][c], want[c])
    # the inserted base: its anchor's position; the loss champion MA prints the REF side's window of ITS width, 3
    r = rows[2]
    assert (r["motifs_gain"], r["motifs_loss"], r["loss_motif_id"], r["loss_motif_alt_id"], r["loss_kmer"], r["loss_strand"], r["loss_start"]) == \
        (0, 1, "MA", "a", "ACG", "+", -2.0)
    assert (r["loss_ref_score"], r["loss_alt_score"], r["loss_pvalue"]) == (25 / 10 + 3 * 0.5, 3 / 10 + 3 * 0.5, 0.01)
    assert (r["gain_motif_id"], r["gain_kmer"], r["down_motif_id"], r["down_delta_log2_affinity"], r["up_motif_id"]) == ("", "", "MB", -2.0, "")
    # champions of two widths print k-mers of their own width
    assert (rows[0]["gain_motif_id"], rows[0]["gain_kmer"]) == ("MB", "TCGTA") and (rows[3]["gain_motif_id"], rows[3]["gain_kmer"]) == ("MA", "TTT")
    # the count-0 reference sequence has detail rows
    assert (rows[4]["haplotypes"], rows[4]["is_reference"], rows[4]["gain_kmer"], rows[4]["gain_ref_score"] != rows[4]["gain_ref_score"]) == \
        (0, True, "GTA", True)
    # ---- the filter: a delta adds the rows whose up or down champion reaches it; an infinite delta reaches every delta
    t.delta = 1.0
    assert [(r["version"], r["position"], r["to"]) for r in t.to_frame().to_dict("records")] == \
        [(0, 11, "T"), (0, 12, "T"), (0, 12, "A"), (0, 14, "C"), (1, 11, "T"), (-1, 12, "G")]
    r = t.to_frame().to_dict("records")[3]
    assert (r["up_motif_id"], r["up_delta_log2_affinity"], r["motifs_gain"], r["gain_motif_id"]) == ("MB", float("inf"), 0, "")
    t.delta = 0.58
    assert len(t.to_frame()) == len(t) == 7 and t.to_frame().to_dict("records")[4]["up_delta_log2_affinity"] == np.log2(12) - np.log2(8)
    t.delta = 0.59
    assert len(t.to_frame()) == 6
    t.delta, t.all_rows = None, True
    f = t.to_frame()
    assert len(f) == 3 * 16 and list(f.columns) == COLUMNS and (f["motifs_gain"] + f["motifs_loss"] > 0).sum() == 5
    assert f["to"].tolist()[:6] == ["C", "G", "T", "A", "G", "T"]
    # ---- the summary: the versions, not the reference; not the inserted base
    t.all_rows = False
    s = t.summary_frame()
    assert list(s.columns) == SUMMARY_COLUMNS
    assert s.to_dict("records") == [
        # A at 10 in both versions: 3 + 1 haplotypes gain; the champions tie at p = 0.03: the first version's
        {"sequence_name": "c:10-15", "position": 11, "from": "A", "to": "T", "versions": 2, "haplotypes": 4, "haplotypes_gain": 4,
         "haplotypes_loss": 0, "max_motifs_gain": 3, "max_motifs_loss": 0, "gain_motif_id": "MB", "loss_motif_id": ""},
        # C at 11 in version 0 alone (version 1 reads T there)
        {"sequence_name": "c:10-15", "position": 12, "from": "C", "to": "T", "versions": 1, "haplotypes": 3, "haplotypes_gain": 3,
         "haplotypes_loss": 0, "max_motifs_gain": 2, "max_motifs_loss": 0, "gain_motif_id": "MB", "loss_motif_id": ""}]
    t.all_rows = True
    s = t.summary_frame()
    assert len(s) == 18 and s["versions"].tolist() == [2] * 3 + [1] * 6 + [2] * 9 and set(s["haplotypes"]) == {4, 3, 1}
    keys = [(r["position"], r["from"], "ACGT".index(r["to"])) for r in s.to_dict("records")]
    assert keys == sorted(keys) and (s["loss_motif_id"] == "").all()
    # a smaller p in a later version wins
    t.state.site_p[6, 3, 0] = 0.02
    assert t.summary_frame().to_dict("records")[2]["gain_motif_id"] == "MA"


def test_a_table_refuses_arrays_that_do_not_fit():
    from grafimo_amd.mutation_profile import FoldState
    t = _hand_profile()
    with pytest.raises(ValueError, match="does not fit"):
        type(t)(["MA"], ["a"], [3], [10], [0.5], [1.0], 0.05, ["r"], [], [0], [0], [1], np.zeros((1, 0)), [True], [0, 3],
                np.frombuffer(b"ACG", dtype=np.uint8), [0, 1, 2], FoldState.host_zeros(4, 4))
    st = FoldState.host_zeros(3, 4)
    st.aff_motif[0, 0, 0] = 2
    with pytest.raises(ValueError, match="names a motif beyond"):
        type(t)(["MA"], ["a"], [3], [10], [0.5], [1.0], 0.05, ["r"], [], [0], [0], [1], np.zeros((1, 0)), [True], [0, 3],
                np.frombuffer(b"ACG", dtype=np.uint8), [0, 1, 2], st)
    empty = type(t)([], [], [], [], [], [], 0.05, [], [], [], [], [], np.zeros((0, 0)), [], [0], np.zeros(0, dtype=np.uint8), [],
                    FoldState.host_zeros(0, 4), all_rows=True)
    assert len(empty.to_frame()) == 0 and list(empty.summary_frame().columns) == SUMMARY_COLUMNS


# ------------------------------------------------------------------------------------------- the command line
def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(flags),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, "-s", str(tmp_path), "--mutation-profile")
    assert r.returncode != 0 and "--mutation-profile needs the graph" in r.stderr
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--mutation-profile-all")
    assert r.returncode != 0 and "--mutation-profile-all goes with --mutation-profile" in r.stderr
    r = _cli(tmp_path, *graph, "--mutation-profile-delta", "1.5")
    assert r.returncode != 0 and "--mutation-profile-delta goes with --mutation-profile" in r.stderr
    r = _cli(tmp_path, *graph, "--mutation-profile", "--mutation-profile-delta", "-1")
    assert r.returncode != 0 and "--mutation-profile-delta -1.0 is not >= 0" in r.stderr
    r = _cli(tmp_path, *graph, "--mutation-all", "--mutation-profile")
    assert r.returncode != 0 and "--mutation-all goes with --mutation-scan" in r.stderr          # (the two are independent)
