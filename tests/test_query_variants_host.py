"""Query-variant table without a GPU: the VCF reader, the trimming, the footprint helper against a per-base loop, the brute
force's rule on a hand-made graph, the context merge and its numbering, the frames and writers on a hand-made result, the CLI's
refusals and the library's export."""
import gzip
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from graph_table_checks import random_bitset_index  # noqa: E402
from haplotype_sequence_cases import chained_graph  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
VCF = ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"
       "x\t10\trs1\tA\tG\t.\t.\t.\tGT\t0|1\n"
       "x\t20\trs2\tAT\tA,ATT,<DEL>\t.\t.\t.\tGT\t0|1\n"
       "y\t5\t.\tC\t*\n"
       "y\t7\tbnd\tG\tG]y:9]\n"
       "\n"
       "y\t9\trs3\tc\tt\textra\n")


def test_read_query_vcf_plain_and_gzip(tmp_path):
    from grafimo_amd.query_variants import read_query_vcf
    plain, packed = str(tmp_path / "q.vcf"), str(tmp_path / "q.vcf.gz")
    open(plain, "w").write(VCF)
    with gzip.open(packed, "wt") as fh:
        fh.write(VCF)
    want = [("x", 10, "rs1", "A", "G"), ("x", 20, "rs2", "AT", "A"), ("x", 20, "rs2", "AT", "ATT"), ("y", 9, "rs3", "c", "t")]
    for path in (plain, packed):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert read_query_vcf(path) == want
        assert len(w) == 1 and "3 ALT alleles" in str(w[0].message)
    open(plain, "w").write("x\t10\trs1\tA\n")
    with pytest.raises(ValueError, match="CHROM POS ID REF ALT"):
        read_query_vcf(plain)


def test_normalise_strips_the_prefix_then_the_suffix():
    from grafimo_amd.query_variants import normalise
    assert normalise(10, "A", "G") == (9, "A", "G")
    assert normalise(10, "AT", "A") == (10, "T", "")                  # a deletion behind its anchor
    assert normalise(10, "A", "ATT") == (10, "", "TT")                # an insertion behind its anchor
    assert normalise(10, "ACGT", "ATGT") == (10, "C", "T")
    assert normalise(10, "ATTT", "AT") == (11, "TT", "")              # prefix first: AT, then nothing is left to strip
    assert normalise(10, "TA", "A") == (9, "T", "")                   # no common prefix: the suffix goes
    assert normalise(10, "acg", "AtG") == (10, "c", "t")              # without regard to case, the bases as given
    assert normalise(1, "A", "TA") == (0, "", "T")                    # before the first base
    assert normalise(10, "AC", "AC") == (11, "", "")


def _footprint_loop(idx, pos0, lr, W):
    L = len(idx.ref)
    gone = np.zeros(L, dtype=bool)
    for p, d in zip(idx.pos.tolist(), idx.del_len.tolist()):
        if d > 0:
            gone[p + 1:p + 1 + d] = True
    lo, hi = min(max(pos0, 0), L), min(max(pos0 + lr, 0), L)
    S, n = lo, 0
    while n < W - 1 and S > 0:
        S -= 1
        n += 0 if gone[S] else 1
    E, n = hi, 0
    while n < W - 1 and E < L:
        n += 0 if gone[E] else 1
        E += 1
    if lr == 0:
        S, E = min(S, max(lo - 1, 0)), max(E, min(hi + 1, L))
    return S, E


def _with_deletions(rng, L, n):
    """a GraphIndex whose deletions overlap, chain (an anchor inside another's span), touch and reach the chromosome's end"""
    from grafimo_amd.extract_regions import GraphIndex
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)]
    pos = np.sort(rng.choice(L - 1, size=n, replace=False)).astype(np.int32)
    dl = np.array([min(int(rng.integers(1, 12)), L - 1 - p) if rng.random() < 0.7 else 0 for p in pos.tolist()], dtype=np.int32)
    alt = np.zeros((n, 3), dtype=np.uint8)
    alt[dl == 0, 0] = ord("A")
    return GraphIndex("c", ref, pos, np.ones(n, dtype=np.uint8), alt, None, 0, del_len=dl)


def test_footprints_equal_a_per_base_loop():
    from grafimo_amd.query_variants import deleted_spans, footprints
    seen_chain = clipped = 0
    for seed in range(40):
        rng = np.random.default_rng(91_000 + seed)
        L = int(rng.integers(30, 200))
        idx = _with_deletions(rng, L, int(rng.integers(1, min(L - 1, 40)))) if seed else chained_graph()[0]
        L = len(idx.ref)
        a, b = deleted_spans(idx)
        assert (a[1:] > b[:-1]).all() and (b > a).all()
        gone = np.zeros(L, dtype=bool)
        for x, y in zip(a.tolist(), b.tolist()):
            gone[x:y] = True
        d = np.flatnonzero(idx.del_len > 0)
        seen_chain += int(any(gone[idx.pos[i]] for i in d.tolist()))
        pos0 = np.concatenate([rng.integers(0, L + 1, size=60), [0, 0, L - 1, L, L, L + 3]])
        lr = np.concatenate([rng.integers(0, 9, size=60), [0, 1, 1, 0, 2, 1]])
        for W in (1, 2, 5, 19, 64):
            S, E = footprints(idx, pos0, lr, W)
            assert S.dtype == np.int64 and E.dtype == np.int64
            for k in range(len(pos0)):
                assert (int(S[k]), int(E[k])) == _footprint_loop(idx, int(pos0[k]), int(lr[k]), W), (seed, W, int(pos0[k]), int(lr[k]))
            clipped += int((S == 0).sum() + (E == L).sum())
    assert seen_chain >= 5 and clipped > 100
    idx = random_bitset_index(5, 3, length=80, n_sites=6, indels=False)           # no deletion at all
    S, E = footprints(idx, [10, 0, 79], [1, 1, 1], 5)
    assert S.tolist() == [6, 0, 75] and E.tolist() == [15, 5, 80]
    assert [len(x) for x in footprints(idx, [], [], 5)] == [0, 0]


def test_the_rule_on_a_hand_made_graph():
    """the brute force itself (test infrastructure), where the answer can be read off: a panel SNP next to the query, a panel
    deletion over it, a panel insertion in its REF span -- and the module's own trimming, footprint, used context and refusals
    on the same graph"""
    from grafimo_amd import query_variants as qv
    from query_variant_bruteforce import (ABSENT, APPLIED, MISMATCH, hand_graph, locate, side, spelled, used_context,
                                          variant_expected)
    idx = hand_graph()
    ref = np.asarray(idx.ref)
    L = len(ref)
    got = [locate(*spelled(idx, h)[:2], L, 10, b"GT") for h in (0, 1, 2, 3, -1)]
    assert got == [(APPLIED, 10), (APPLIED, 10), (ABSENT, -1), (MISMATCH, 10), (APPLIED, 10)]
    assert locate(*spelled(idx, 0)[:2], L, 10, b"CT")[0] == MISMATCH
    assert locate(*spelled(idx, 0)[:2], L, 11, b"")[0] == APPLIED and locate(*spelled(idx, 3)[:2], L, 11, b"")[0] == MISMATCH
    assert locate(*spelled(idx, 0)[:2], L, L, b"") == (APPLIED, L) and locate(*spelled(idx, 0)[:2], L, 0, b"")[0] == ABSENT
    sm = np.arange(12, dtype=np.int64).reshape(4, 3) * 10
    wtab = np.arange(3001, dtype=np.uint64) + 1
    best, total = side(b"ACGTACGT", 3, 1, 3, sm, 0, wtab, True)
    assert best == (max(30 + 70 + 110, 60 + 100 + 20, 90 + 10 + 50), -2, "+", "CGT") and total == 210 + 180 + 150 + 3
    assert side(b"ACGTACGT", 3, 0, 3, sm, 0, wtab, True)[1] == 210 + 180 + 2        # the two windows across the junction
    assert side(b"AC", 1, 1, 3, sm, 0, wtab, False) == (None, 0)
    e = variant_expected(idx, 10, b"G", b"A", 3, sm, 0, wtab, groups=[[0, 1], [3]])
    # the SNP at 10 applies to all but the haplotype that deletes it; the inserted GG behind 10 is a context of its own
    assert e["status"] == (3, 1, 0) and [c["count"] for c in e["contexts"]] == [1, 1, 1]
    assert [c["first"] for c in e["contexts"]] == [0, 1, 3] and [c["is_reference"] for c in e["contexts"]] == [True, False, False]
    assert [c["group_counts"] for c in e["contexts"]] == [[1, 0], [1, 0], [0, 1]] and e["reference"][0] == APPLIED
    # W = 2 at 12: the SNP at 9 and the insertion behind 10 are out of reach, the deletion of 10, 11 is not
    one = variant_expected(idx, 12, b"A", b"C", 2, sm[:, :2], 0, wtab)
    assert one["status"] == (4, 0, 0) and [c["members"] for c in one["contexts"]] == [[0, 1, 3], [2]]
    # the module under test states the same rule: its trimming, its used context and its footprint on this graph
    # (the footprint counts kept positions: 10 and 11 lie in the deletion's span, so W - 1 = 1 to the left of 12 reaches 9)
    assert qv.normalise(13, "A", "C") == (12, "A", "C") and [v.tolist() for v in qv.footprints(idx, [12], [1], 2)] == [[9], [14]]
    for h in (0, 2, 3, -1):
        x = spelled(idx, h)[0]
        o = locate(*spelled(idx, h)[:2], L, 12, b"A")[1]
        assert qv.used_context(x, o, 1, 2) == used_context(x, o, 1, 2) == ((b"TAC", 1) if h != 2 else (b"CAC", 1))
    assert [v.tolist() for v in qv.footprints(idx, [10], [1], 3)] == [[8], [14]]
    assert qv.unusable("c", 21, "v", "A", "C", L) == "query variant c:21 v A>C: REF lies outside the chromosome's 20 bases"
    assert qv.unusable("c", 0, "v", "A", "C", L) is not None and qv.unusable("c", 20, "v", "T", "TA", L) is None
    assert qv.unusable("c", 20, "v", "TA", "T", L) is not None and qv.unusable("c", 5, "v", "R", "A") is not None
    assert qv.unusable("c", 5, "v", "A", "É") == "query variant c:5 v A>É: REF and ALT are plain base strings"


def test_merge_contexts_sums_and_numbers():
    from grafimo_amd.query_variants import merge_contexts, used_context
    assert used_context(b"ACGTACGTAC", 4, 1, 3) == (b"GTACG", 2) and used_context(b"ACGT", 0, 0, 3) == (b"AC", 0)
    assert used_context(b"ACGT", 4, 0, 3) == (b"GT", 2)
    keys = ["b", "a", "b", "c", "a", "a"]
    count, first = [5, 1, 2, 7, 1, 1], [9, 3, 4, 0, 8, 1]
    groups = [[1, 0], [0, 1], [1, 1], [2, 2], [0, 0], [1, 0]]
    of, n, f, g, ref, head = merge_contexts(keys, count, first, groups, [False, False, True, False, False, False])
    # the contexts: c (7 haplotypes), b (7, representative 4), a (3)
    assert n.tolist() == [7, 7, 3] and f.tolist() == [0, 4, 1] and of.tolist() == [1, 2, 1, 0, 2, 2]
    assert g.tolist() == [[2, 2], [2, 1], [1, 1]] and ref.tolist() == [False, True, False] and head.tolist() == [3, 2, 5]
    empty = merge_contexts([], [], [], np.zeros((0, 2)), [])
    assert [len(x) for x in empty] == [0] * 6


def _hand_made(all_variants=False):
    """two variants, motif of W = 2: variant 0 has two contexts with different effects and a reference that applies,
    variant 1 one context without any hit and a reference the edit does not apply to"""
    from grafimo_amd.query_variants import RECORD, QueryVariants
    key = lambda score, rel, plus: ((score + 1) << 8) | ((64 - rel) << 1) | int(plus)      # noqa: E731
    recs = np.zeros(3, dtype=RECORD)
    recs[0] = (0, 5, key(90, -1, True), key(10, 0, False), 1 << 40, 1 << 38)       # loss
    recs[1] = (0, 5, key(10, 0, True), key(10, 0, True), 1 << 38, 1 << 38)         # none
    recs[2] = (0, 1, 0, key(20, 0, True), 0, 1 << 30)                              # no REF window; none
    reference = np.zeros(2, dtype=RECORD)
    reference[0] = recs[0]
    reference[1]["status"] = 2
    ptable = np.linspace(1.0, 0.0, 2001)
    return QueryVariants("M1", "m1", 2, 10, -1.5, ptable, -40.0, 0.5, ["h0", "h1", "h2", "h3"], ["g"],
                         [("x", 10, "rs1", "A", "G"), ("x", 20, ".", "AT", "A")], [(9, "A", "G"), (20, "T", "")],
                         [[3, 1, 0], [2, 0, 2]], [0, 2, 3], [2, 1, 2], [0, 2, 1], [[1], [1], [0]], [True, False, False], recs,
                         ["AC", "GT", ""], ["TG", "GT", "CA"], reference, [0, 0, 1], [2, 1, 2], recs, [0, 1, 0], all_variants)


def test_frames_on_a_hand_made_result(tmp_path):
    from grafimo_amd.query_variants import (print_query_variants, write_query_variant_contexts, write_query_variants)
    t = _hand_made(True)
    c, s = t.contexts_frame(), t.to_frame()
    assert list(c.columns) == ["motif_id", "motif_alt_id", "chrom", "pos", "id", "ref", "alt", "context", "haplotypes", "frequency",
                               "haplotypes_g", "representative", "is_reference", "ref_score", "ref_pvalue", "ref_strand", "ref_offset",
                               "ref_kmer", "alt_score", "alt_pvalue", "alt_strand", "alt_offset", "alt_kmer", "delta_score",
                               "ref_log2_affinity", "alt_log2_affinity", "delta_log2_affinity", "effect"]
    assert list(s.columns) == ["motif_id", "motif_alt_id", "chrom", "pos", "id", "ref", "alt", "haplotypes_applied",
                               "haplotypes_absent", "haplotypes_mismatch", "contexts", "reference_effect", "reference_delta_score",
                               "haplotypes_gain", "haplotypes_loss", "haplotypes_both", "haplotypes_none", "min_delta_score",
                               "max_delta_score", "mean_delta_log2_affinity", "background_dependent"]
    assert c["context"].tolist() == [0, 1, 0] and c["haplotypes"].tolist() == [2, 1, 2] and c["frequency"].tolist() == [0.5, 0.25, 0.5]
    assert c["representative"].tolist() == ["h0", "h2", "h1"] and c["is_reference"].tolist() == [True, False, False]
    assert c["ref_score"].tolist()[:2] == [90 / 10 - 3.0, 10 / 10 - 3.0] and np.isnan(c["ref_score"][2])
    assert c["ref_pvalue"].tolist()[:2] == [t.ptable[90], t.ptable[10]] and c["alt_pvalue"].tolist() == [t.ptable[10]] * 2 + [t.ptable[20]]
    assert c["ref_strand"].tolist() == ["+", "+", ""] and c["alt_strand"].tolist() == ["-", "+", "+"]
    assert c["ref_offset"].tolist()[:2] == [-1.0, 0.0] and np.isnan(c["ref_offset"][2]) and c["ref_kmer"].tolist() == ["AC", "GT", ""]
    assert c["delta_score"].tolist()[:2] == [-8.0, 0.0] and np.isnan(c["delta_score"][2])
    assert c["ref_log2_affinity"].tolist()[:2] == [0.0, -2.0] and c["delta_log2_affinity"].tolist()[:2] == [-2.0, 0.0]
    assert np.isnan(c["ref_log2_affinity"][2]) and c["alt_log2_affinity"][2] == -10.0
    assert c["effect"].tolist() == ["none"] * 3 and not s["background_dependent"].any()      # (no p-value is below 0.5)
    t2 = _hand_made(True)
    t2.threshold = 0.96                                                     # ptable[90] = 0.955 < 0.96 <= ptable[10]
    assert t2.contexts_frame()["effect"].tolist() == ["loss", "none", "none"]
    assert s["haplotypes_applied"].tolist() == [3, 2] and s["haplotypes_absent"].tolist() == [1, 0] and s["contexts"].tolist() == [2, 1]
    s2 = t2.to_frame()
    assert s2["reference_effect"].tolist() == ["loss", ""] and s2["reference_delta_score"].tolist()[0] == -8.0
    assert np.isnan(s2["reference_delta_score"][1])
    assert s2["haplotypes_loss"].tolist() == [2, 0] and s2["haplotypes_none"].tolist() == [1, 2] and s2["haplotypes_gain"].tolist() == [0, 0]
    assert s2["min_delta_score"].tolist()[0] == -8.0 and s2["max_delta_score"].tolist()[0] == 0.0 and np.isnan(s2["min_delta_score"][1])
    assert s2["mean_delta_log2_affinity"].tolist()[0] == (-2.0 * 2 + 0.0) / 3 and np.isnan(s2["mean_delta_log2_affinity"][1])
    assert s2["background_dependent"].tolist() == [True, False]
    # without all_variants only the variant with an effect stays, its context rows with it
    t3 = _hand_made(False)
    t3.threshold = 0.96
    assert len(t3) == 1 and t3.to_frame()["id"].tolist() == ["rs1"] and t3.contexts_frame()["id"].tolist() == ["rs1", "rs1"]

    class _Out:
        outdir = str(tmp_path / "o")

    class _Motif:
        motif_id = "M1"

    a, b = write_query_variants(t2, _Motif(), 1, _Out()), write_query_variant_contexts(t2, _Motif(), 2, _Out())
    assert os.path.basename(a) == "grafimo_query_variants.tsv" and os.path.basename(b) == "grafimo_query_variant_contexts_M1.tsv"
    assert open(a, "rb").read() == s2.to_csv(sep="\t", index=False, lineterminator="\n").encode()
    assert open(b, "rb").read() == t2.contexts_frame().to_csv(sep="\t", index=False, lineterminator="\n").encode()
    old, sys.stdout = sys.stdout, io.StringIO()
    try:
        print_query_variants(t2)
        text = sys.stdout.getvalue()
    finally:
        sys.stdout = old
    assert text == open(a).read() + open(b).read()


def test_decode_keys():
    from grafimo_amd.query_variants import decode_keys
    key = np.array([0, (1 << 8) | (64 << 1) | 1, (65536 << 8) | (127 << 1), (6 << 8) | (1 << 1) | 1], dtype=np.uint32)
    score, rel, strand = decode_keys(key)
    assert score.tolist() == [-1, 0, 65535, 5] and rel.tolist() == [0, 0, -63, 63] and strand.tolist() == ["", "+", "-", "+"]


def _cli(tmp_path, *args):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(args),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    q = str(tmp_path / "q.vcf")
    open(q, "w").write(VCF)
    r = _cli(tmp_path, "-s", str(tmp_path), "--query-variants", q)
    assert r.returncode != 0 and "--query-variants needs the graph (-g / -d with -b, or -l -v -b): the rows of -s carry no haplotypes" in r.stderr
    r = _cli(tmp_path, "-s", str(tmp_path), "--query-all")
    assert r.returncode != 0 and "--query-all goes with --query-variants" in r.stderr
    r = _cli(tmp_path, "-s", str(tmp_path), "--query-variants", str(tmp_path / "missing.vcf"))
    assert r.returncode != 0 and "Unable to locate" in r.stderr
    # the two options the new flag also takes: refused without a table that reads them, in the words they always had
    r = _cli(tmp_path, "-s", str(tmp_path), "--affinity-temperature", "2")
    assert r.returncode != 0 and r.stderr.strip().endswith(
        "ERROR: --affinity-temperature goes with --haplotype-affinity or --variant-affinity or --haplotype-classes")
    r = _cli(tmp_path, "-s", str(tmp_path), "--haplotype-groups", q)
    assert r.returncode != 0 and "--haplotype-groups goes with --hit-alleles or --hit-pairs or --haplotype-classes or" in r.stderr
    # ... and accepted with it: the refusal is then the graph's, not theirs
    r = _cli(tmp_path, "-s", str(tmp_path), "--query-variants", q, "--affinity-temperature", "2", "--haplotype-groups", q)
    assert r.returncode != 0 and "--query-variants needs the graph" in r.stderr


def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    from grafimo_amd.query_variants import MAX_ALLELE, RECORD
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert "gfm_graph_query_edits" in nv.PROTOTYPES and hasattr(nv.lib(), "gfm_graph_query_edits")
    assert len(nv.PROTOTYPES["gfm_graph_query_edits"][1]) == 21
    proto = header[header.index("int gfm_graph_query_edits("):]
    assert proto[:proto.index(";")].count(",") == 20
    assert "#define GFM_ABI_VERSION 12" in header and f"#define GFM_QUERY_MAX_ALLELE {MAX_ALLELE}" in header and MAX_ALLELE == 64
    assert RECORD.itemsize == 32 and "} gfm_edit_record_t;" in header
