"""The shuffle null without a GPU: the rule's pinned permutations, mix values and content keys, the frames of tables made from
hand-made arrays, the cut rule, the export, the header and the command line's refusals."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shuffle_null_bruteforce as bf  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_g", "is_reference", "length",
           "best_score", "best_pvalue", "best_null_pvalue", "log2_affinity", "affinity_null_pvalue", "replicates"]
ENRICHMENT_COLUMNS = ["motif_id", "motif_alt_id", "width", "regions", "observed_hits", "null_mean_hits", "null_max_hits",
                      "enrichment_pvalue", "replicates"]


# ------------------------------------------------------------------------------------------- the rule
def test_mix_values():
    from grafimo_amd.shuffle_null import G, mix
    assert bf.mix(1) == 0x5692161d100b05e5 and bf.mix(0) == 0
    assert int(mix(1)) == 0x5692161d100b05e5 and int(mix(0)) == 0
    assert int(G) == bf.G == 0x9E3779B97F4A7C15
    z = np.random.default_rng(1).integers(0, 1 << 64, size=100, dtype=np.uint64)
    assert mix(z).tolist() == bf.mix_words(z).tolist() == [bf.mix(int(v)) for v in z]


def test_pinned_permutations():
    """seed 7, key 3, n 8, x = ACGTNacg: the bytes travel as they are, non-ACGT and lower case included"""
    x = b"ACGTNacg"
    perm = bf.permutations(8, 3, 7, 3)
    assert perm.tolist() == [[6, 7, 5, 0, 4, 3, 2, 1], [5, 1, 7, 0, 4, 3, 2, 6], [5, 4, 6, 2, 1, 3, 0, 7]]
    assert bf.shuffles(x, 3, 7, 3) == [b"cgaANTGC", b"aCgANTGc", b"aNcGCTAg"]
    # replicate r does not depend on K, and r0 names the first one
    assert bf.permutations(8, 3, 7, 1, r0=2).tolist() == [perm[2].tolist()]
    # the key and the seed both matter
    assert bf.permutations(8, 4, 7, 1).tolist() != perm[:1].tolist() and bf.permutations(8, 3, 8, 1).tolist() != perm[:1].tolist()


@pytest.mark.parametrize("n", [0, 1, 2, 7, 64, 65, 300])
def test_every_replicate_is_a_permutation(n):
    perm = bf.permutations(n, 0xFFFFFFFFFFFFFFFF, (1 << 64) - 3, 130)
    assert perm.shape == (130, n)
    assert (np.sort(perm, axis=1) == np.arange(n)[None, :]).all()
    if n >= 64:
        assert len({p.tobytes() for p in perm}) == 130


def test_the_shuffle_is_uniform_at_eight_positions():
    """over 80 000 replicates element 0 lands in each of the eight positions between 9 811 and 10 190 times (10 000 +- 2 sigma
    of a binomial is 9 813 .. 10 187; the counts were computed with this restatement of the rule when the rule was written)"""
    perm = bf.permutations(8, 3, 7, 80_000)
    landed = np.bincount(np.argmax(perm == 0, axis=1), minlength=8)
    assert landed.sum() == 80_000 and landed.min() >= 9_811 and landed.max() <= 10_190, landed.tolist()


def test_content_keys():
    from grafimo_amd.shuffle_null import content_keys
    assert content_keys(b"") == 0 and content_keys(b"A") == 0xcc799cabe4be9717
    assert content_keys(b"ACGT") == content_keys(b"acgt") == 0x38a9e524dbd0154a
    assert content_keys(b"TGCA") == 0x6d895e9eaac00bb9
    # many at once, empty sequences between others: a sequence's key is its content's, wherever it stands
    seqs = [b"", b"A", b"ACGT", b"", b"acgt", b"TGCA", b"ACGTNNNNacgtn" * 9, b""]
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    keys = content_keys(off, np.frombuffer(b"".join(seqs), dtype=np.uint8))
    assert keys.dtype == np.uint64 and keys.tolist() == [bf.content_key(x) for x in seqs]
    assert keys.tolist()[:6] == [0, 0xcc799cabe4be9717, 0x38a9e524dbd0154a, 0, 0x38a9e524dbd0154a, 0x6d895e9eaac00bb9]
    assert content_keys(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint8)).shape == (0,)
    with pytest.raises(ValueError, match="starts at 0"):
        content_keys([1, 2], b"AC")


def test_the_brute_force_follows_the_rule_on_a_sequence_read_by_hand():
    """W = 2, w[s] = s + 1: ACN has the windows AC and CN; CN holds an N and scores min_val on both strands"""
    sm = np.array([[1, 2], [3, 4], [5, 6], [7, 8]])              # rows A, C, G, T
    w = np.arange(100, dtype=np.uint64) + 1
    assert bf.pair(b"ACN", 2, sm, 0, w, True) == (5, 6 + 1)      # AC: 1 + 4; CN: 0
    assert bf.pair(b"ACN", 2, sm, 0, w, False) == (13, 6 + 14 + 1 + 1)      # the other strand of AC reads GT: 5 + 8
    assert bf.pair(b"A", 2, sm, 0, w, False) == (-1, 0) and bf.pair(b"", 2, sm, 0, w, False) == (-1, 0)
    ys = np.frombuffer(b"ACNacn", dtype=np.uint8).reshape(2, 3)
    assert bf.pairs(ys, 2, sm, 0, w, False) == [(13, 22), (13, 22)]          # case is folded
    assert bf.pairs(ys[:, :1], 2, sm, 0, w, False) == [(-1, 0), (-1, 0)]
    # counts: ties count; a sequence shorter than W has ge = K
    reps = dict(obs_best=[5, -1], obs_sum=[7, 0], rep_best=[[5, 4, 9], [-1, -1, -1]], rep_sum=[[7, 8, 6], [0, 0, 0]])
    got = bf.counts(reps, 3, 5, [2, 3])
    assert got["ge_best"] == [2, 3] and got["ge_sum"] == [2, 3] and got["rep_hits"] == [2, 0, 2]
    assert bf.counts(reps, 2, 0, None)["rep_hits"] == [1, 1] and bf.counts(reps, 2, 0, None)["ge_best"] == [1, 2]


# ------------------------------------------------------------------------------------------- the table from hand-made arrays
def _table(**over):
    from grafimo_amd.shuffle_null import ShuffleNull
    ptable = np.array([1.0, 0.5, 0.5, 0.2, 0.2, 0.01])           # (a frame indexes it by the scaled score and needs no more of it)
    a = dict(motif_id="M1", motif_alt_id="m1", width=3, scale=2, offset=-1.5, ptable=ptable, log2_offset=-40.0, threshold=0.5,
             region_names=["c:0-9", "c:20-22"], group_names=["g"], seq_region=[0, 0, 1, 1], seq_version=[0, 1, 0, -1],
             seq_count=[5, 1, 6, 0], seq_group_counts=[[2], [0], [3], [0]], seq_is_reference=[False, True, False, True],
             seq_length=[9, 10, 2, 2], seq_weight=[1, 0, 1, 0], replicates=9, seed=4, obs_best=[4, 3, -1, -1],
             obs_sum=[1 << 60, 12, 0, 0], ge_best=[0, 9, 9, 9], ge_sum=[4, 1, 9, 9], rep_hits=[0, 1, 2, 0, 1, 1, 0, 2, 1], cut=3)
    a.update(over)
    return ShuffleNull(**a)


def test_frame_from_hand_made_arrays():
    t = _table()
    f = t.to_frame()
    assert list(f.columns) == COLUMNS and len(f) == len(t) == 4
    assert f["sequence_name"].tolist() == ["c:0-9", "c:0-9", "c:20-22", "c:20-22"] and f["version"].tolist() == [0, 1, 0, -1]
    assert f["haplotypes"].tolist() == [5, 1, 6, 0] and f["haplotypes_g"].tolist() == [2, 0, 3, 0]
    assert f["is_reference"].tolist() == [False, True, False, True] and f["length"].tolist() == [9, 10, 2, 2]
    assert f["replicates"].tolist() == [9] * 4 and set(f["motif_id"]) == {"M1"} and set(f["motif_alt_id"]) == {"m1"}
    # the p-value formula: (1 + ge) / (K + 1) -- never 0, and 1 when every replicate ties or beats
    assert f["best_null_pvalue"].tolist()[:2] == [1 / 10, 10 / 10] and f["affinity_null_pvalue"].tolist()[:2] == [5 / 10, 2 / 10]
    assert f["best_score"].tolist()[:2] == [4 / 2 + 3 * -1.5, 3 / 2 + 3 * -1.5] and f["best_pvalue"].tolist()[:2] == [0.2, 0.2]
    assert f["log2_affinity"].tolist()[:2] == [60.0 - 40.0, float(np.log2(12.0)) - 40.0]
    # NaN below W: everywhere
    for c in ("best_score", "best_pvalue", "best_null_pvalue", "log2_affinity", "affinity_null_pvalue"):
        assert f[c].isna().tolist() == [False, False, True, True], c
    with pytest.raises(ValueError, match="do not fit"):
        _table(rep_hits=[0] * 8)
    with pytest.raises(ValueError, match="do not fit"):
        _table(ge_sum=[0] * 3)


def test_enrichment_frame_from_hand_made_arrays():
    from grafimo_amd.shuffle_null import enrichment_frame
    a = _table()                                                  # weights 1, 0, 1, 0; obs_best 4, 3, -1, -1 at cut 3
    b = _table(motif_id="M2", motif_alt_id="m2", cut=5, rep_hits=[0] * 9)
    c = _table(motif_id="M0", motif_alt_id="m0", cut=0, seq_weight=[1, 1, 1, 1], rep_hits=[2, 2, 2, 2, 2, 2, 2, 2, 3])
    e = enrichment_frame([a, b, c])
    assert list(e.columns) == ENRICHMENT_COLUMNS and e["motif_id"].tolist() == ["M1", "M2", "M0"]       # the motifs' order
    assert e["width"].tolist() == [3, 3, 3] and e["regions"].tolist() == [2, 2, 4] and e["replicates"].tolist() == [9, 9, 9]
    # a: version 0 of region 0 reaches the cut (the weight-0 version 1 does too and is not counted); 6 replicates hold >= 1 hit
    assert e["observed_hits"].tolist() == [1, 0, 2]
    assert e["null_mean_hits"].tolist() == [8 / 9, 0.0, 19 / 9] and e["null_max_hits"].tolist() == [2, 0, 3]
    assert e["enrichment_pvalue"].tolist() == [(1 + 6) / 10, (1 + 9) / 10, (1 + 9) / 10]
    assert enrichment_frame([]).columns.tolist() == ENRICHMENT_COLUMNS


def test_the_cut_is_strict_at_a_tie_of_the_tail_table():
    from grafimo_amd.shuffle_null import null_pvalues, pvalue_cut
    ptable = np.array([1.0, 0.5, 0.5, 0.2, 0.2, 0.01])
    assert pvalue_cut(ptable, 0.5) == 3                           # 0.5 is not < 0.5: the scores 1 and 2 do not count
    assert pvalue_cut(ptable, 0.50001) == 1 and pvalue_cut(ptable, 0.2) == 5 and pvalue_cut(ptable, 1.5) == 0
    assert pvalue_cut(ptable, 0.01) == 6 == len(ptable)           # none: L
    assert null_pvalues(np.array([0, 999, 1000]), 1000).tolist() == [1 / 1001, 1000 / 1001, 1.0]


# ------------------------------------------------------------------------------------------- the export, the header, the CLI
N_ARGS = 22


def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    name = "gfm_sequence_shuffle_null"
    assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == N_ARGS
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert f"int {name}(" in header
    decl = header[header.index(f"int {name}("):]
    assert decl[:decl.index(";")].count(",") == N_ARGS - 1
    # before a device is touched: no sequence is a no-op; an unknown flag, replicates out of range and offsets that descend
    # are refused
    fn = nv.lib().gfm_sequence_shuffle_null
    def call(n_seqs, off, K, flags):
        return fn(None, 1, None, 1, n_seqs, off, None, None, None, K, 0, None, flags, *([None] * 9))
    assert call(0, None, 1, 0) == nv.GFM_OK
    assert call(0, None, 1, 2) == nv.GFM_ERR_INVALID and b"unknown flag" in nv.lib().gfm_last_error()
    for K in (0, -1, (1 << 20) + 1):
        assert call(0, None, K, 0) == nv.GFM_ERR_INVALID and b"outside [1, 2^20]" in nv.lib().gfm_last_error()
    assert call(0, None, 1 << 20, 0) == nv.GFM_OK
    off = np.array([0, 5, 3], dtype=np.int64)
    assert call(2, off.ctypes.data, 1, 0) == nv.GFM_ERR_INVALID and b"descends" in nv.lib().gfm_last_error()
    off = np.array([0, 1 << 31], dtype=np.int64)
    assert call(1, off.ctypes.data, 1, 0) == nv.GFM_ERR_INVALID and b"2^31" in nv.lib().gfm_last_error()
    off = np.array([0, 4], dtype=np.int64)
    assert call(1, off.ctypes.data, 1, 0) == nv.GFM_ERR_INVALID and b"NULL argument" in nv.lib().gfm_last_error()
    assert call(1, None, 1, 0) == nv.GFM_ERR_INVALID and b"NULL argument" in nv.lib().gfm_last_error()


def test_header_defines_the_cap_and_states_the_rule():
    from grafimo_amd import _native as nv
    from grafimo_amd import shuffle_null
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    m = re.search(r"#define GFM_NULL_LDS_BASES (\d+)", header)
    assert m and int(m.group(1)) == nv.GFM_NULL_LDS_BASES
    # a workgroup's image (64 bytes a base) and the motif's table fit 64 KiB, so two workgroups fit a CU's 160 KiB
    assert 64 * nv.GFM_NULL_LDS_BASES + 2048 <= 64 * 1024
    assert shuffle_null.MAX_REPLICATES == 1 << 20
    squeeze = lambda s: " ".join(s.replace("*", " ").split())                   # noqa: E731
    texts = [squeeze(header), squeeze(shuffle_null.__doc__), squeeze(bf.__doc__)]
    for line in ("G = 0x9E3779B97F4A7C15.",
                 "mix(z): z ^= z >> 30; z = 0xBF58476D1CE4E5B9; z ^= z >> 27; z = 0x94D049BB133111EB; z ^= z >> 31.",
                 "s0 = mix(mix(seed + k G) + r).",
                 "y starts as a copy of x: the bytes as they are, non-ACGT and lower case included.",
                 "For i = n - 1 down to 1: u = mix(s0 + i G); j = ((u >> 32) (i + 1)) >> 32; swap y[i] and y[j]."):
        for text in texts:
            assert line in text, line
    for line in ("A window that holds a base that is not A/C/G/T scores min_val on both strands.",
                 "Case is folded, as base_code does.",
                 "Ties count", "The permutation depends on (seed, k, r, n) only"):
        for text in texts[:2]:
            assert line in text, line


def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(flags),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, "-s", str(tmp_path), "--shuffle-null")
    assert r.returncode != 0 and "--shuffle-null needs the graph" in r.stderr
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--null-seed", "5")
    assert r.returncode != 0 and "--null-seed goes with --shuffle-null" in r.stderr
    r = _cli(tmp_path, *graph, "--shuffle-null", "0")
    assert r.returncode != 0 and "--shuffle-null 0 outside [1, 2^20]" in r.stderr
    r = _cli(tmp_path, *graph, "--shuffle-null", "--null-seed", "-1")
    assert r.returncode != 0 and "--null-seed -1 outside" in r.stderr
    r = _cli(tmp_path, "--help")
    assert r.returncode == 0 and r.stdout.count("--shuffle-null") >= 5          # its own options and the two lists it joined


def test_parser_defaults():
    from grafimo_amd.__main__ import get_parser
    p = get_parser()
    assert p.parse_args(["-m", "x"]).shuffle_null is None and p.parse_args(["-m", "x"]).null_seed is None
    assert p.parse_args(["-m", "x", "--shuffle-null"]).shuffle_null == 1000
    a = p.parse_args(["-m", "x", "--shuffle-null", "250", "--null-seed", "9"])
    assert (a.shuffle_null, a.null_seed) == (250, 9)
