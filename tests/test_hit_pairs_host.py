"""The host half of the hit-pair table, no GPU: the expected sides against each other (the haplotype brute force against the
walk enumerator through pairs_reference), pairs_reference on hand-written cases, a hand-made HitPairs against the exact TSV
text, and the command line's argument errors."""
import io
import os

import numpy as np
import pandas as pd
import pytest

from graph_table_checks import random_bitset_index
from hit_allele_bruteforce import report_cutoff
from hit_pair_bruteforce import enumerator_pairs, haplotype_pairs, pack, pairs_reference


class _Args:
    def __init__(self, threshold=1e-4, no_reverse=False, recomb=False, qvalue_t=False, no_qvalue=True):
        self.threshold, self.noreverse, self.recomb = threshold, no_reverse, recomb
        self.noqvalue, self.qvalueT = no_qvalue, qvalue_t


def _motif(W, seed=0):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(900 + 13 * W + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


# ---- the expected side checks itself: sum of joint popcounts over walk-level row pairs = instance pairs per haplotype

@pytest.mark.parametrize("seed,H,widths,threshold,gap,no_reverse", [
    (1, 63, (4, 9, 13), 0.05, (0, 20), False), (2, 65, (5, 5, 11), 0.1, (-64, 10), False), (3, 130, (6, 12), 0.05, (0, 0), True),
    (4, 65, (4, 13, 7), 0.02, (-3, 50), False), (5, 63, (8,), 0.1, (-3, 50), False)])
def test_the_haplotype_brute_force_equals_the_walk_enumerator(seed, H, widths, threshold, gap, no_reverse):
    idx = random_bitset_index(H, 700 + seed, length=140, n_sites=22)
    regions = [(0, 140), (30, 95), (-5, 40), (100, 400), (50, 50), (30, 95)]
    motifs = [_motif(W, seed + k) for k, W in enumerate(widths)]
    if len(widths) == 3 and widths[0] == widths[1]:
        motifs[1] = motifs[0]                                              # one motif twice
    args = _Args(threshold=threshold, no_reverse=no_reverse)
    cutoffs = [report_cutoff(m, args) for m in motifs]
    entries = [(idx, regions)]
    exp = haplotype_pairs(entries, motifs, cutoffs, gap[0], gap[1], no_reverse)
    got, n_pairs = enumerator_pairs(entries, motifs, cutoffs, gap[0], gap[1], no_reverse)
    assert n_pairs >= 5 and sum(exp.values()) > 0
    assert got == exp
    # the region listed twice: its pairs under both listings
    assert {k[1:] for k in exp if k[0] == 1} == {k[1:] for k in exp if k[0] == 5}


# ---- pairs_reference on hand-written cases

def _ref(rows, min_gap, max_gap, **kw):
    """rows: [(group, lo, hi, carriers as a bit string, haplotype 0 first)]"""
    H = len(rows[0][3])
    masks = pack(np.array([[c == "1" for c in r[3]] for r in rows]))
    a, b, j, gc = pairs_reference([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], masks, min_gap, max_gap, **kw)
    return list(zip(a.tolist(), b.tolist(), j.tolist())), gc, H


def test_reference_nested_intervals_and_equal_lo():
    rows = [(0, 10, 50, "1110"), (0, 20, 30, "0110"), (0, 10, 18, "1000"), (0, 10, 50, "0011")]
    # order: (10,18) row 2, (10,50) row 0, (10,50) row 3, (20,30) row 1
    got, _, _ = _ref(rows, -100, 100)
    assert got == [(2, 0, 1), (0, 3, 1), (0, 1, 2), (3, 1, 1)]
    # nested: gap = 20 - 30 = -10; the equal intervals overlap by 40; (10,18) and (20,30) are 2 apart but share nobody
    got, _, _ = _ref(rows, -10, -10)
    assert got == [(0, 1, 2), (3, 1, 1)]
    got, _, _ = _ref(rows, -40, -40)
    assert got == [(0, 3, 1)]
    assert _ref(rows, 2, 2)[0] == []


def test_reference_gap_bounds_are_inclusive():
    rows = [(0, 0, 10, "11"), (0, 15, 25, "01"), (0, 30, 40, "11")]
    assert _ref(rows, 5, 5)[0] == [(0, 1, 1), (1, 2, 1)]
    assert _ref(rows, 6, 19)[0] == []
    assert _ref(rows, 5, 20)[0] == [(0, 1, 1), (0, 2, 2), (1, 2, 1)]
    assert _ref(rows, 20, 20)[0] == [(0, 2, 2)]
    assert _ref(rows, 0, 4)[0] == []


def test_reference_same_interval_on_both_strands_and_tie_keys():
    # two rows of one interval (the '+' and the '-' row of a palindromic site): one pair, `a` by the tie-break keys
    rows = [(3, 7, 15, "101"), (3, 7, 15, "100")]
    assert _ref(rows, -8, -8)[0] == [(0, 1, 1)]
    assert _ref(rows, -8, -8, tie=([1, 0],))[0] == [(1, 0, 1)]
    assert _ref(rows, 0, 50)[0] == []
    # groups never mix
    rows = [(0, 7, 15, "1"), (1, 7, 15, "1")]
    assert _ref(rows, -100, 100)[0] == []


def test_reference_row_without_carriers_never_pairs_and_group_counts():
    rows = [(0, 0, 5, "1111"), (0, 6, 9, "0000"), (0, 10, 15, "0111")]
    gb = pack(np.array([[True, True, False, False], [False, False, False, True], [False, False, False, False]]))
    got, gc, _ = _ref(rows, 0, 50, group_bits=gb)
    assert got == [(0, 2, 3)]
    assert gc.tolist() == [[1, 1, 0]] and gc.dtype == np.int32


# ---- a hand-made table

def _hand_made():
    from grafimo_amd.hit_alleles import HitAlleles
    from grafimo_amd.hit_pairs import HitPairs

    def table(mid, alt, starts, stops, strands, seqs, freqs, refs, bits):
        n = len(starts)
        rep = pd.DataFrame({"motif_id": [mid] * n, "motif_alt_id": [alt] * n, "sequence_name": ["c:0-60"] * n, "start": starts,
                            "stop": stops, "strand": strands, "score": [1.5 - 0.25 * k for k in range(n)],
                            "p-value": [1e-5 * (k + 1) for k in range(n)], "matched_sequence": seqs,
                            "haplotype_frequency": freqs, "reference": refs})
        return HitAlleles(rep, [0] * (n + 1), [], [], [], ["EUR"], np.zeros((n, 1), np.int32), np.array(bits, np.uint64).reshape(n, 1),
                          [f"h{k}" for k in range(4)], [None], row_region=[0] * n)

    t0 = table("MA1.1", "ONE", [2, 30], [8, 24], ["+", "-"], ["ACGTAC", "TTGACA"], [3, 2], ["ref", "non.ref"], [0b0111, 0b0110])
    t1 = table("MA2.1", "TWO", [12], [16], ["+"], ["GGCC"], [4], ["ref"], [0b1111])
    hp = HitPairs([t0, t1], region=[0, 0, 0], motif_a=[0, 0, 1], row_a=[0, 0, 0], motif_b=[1, 0, 0], row_b=[0, 1, 1],
                  gap=[4, 16, 8], co_haplotypes=[3, 2, 2], group_names=["EUR"], group_counts=[[2], [1], [1]],
                  reference=[True, False, False], region_names=["c:0-60"])
    return hp


TSV = ("sequence_name\tmotif_id_a\tmotif_alt_id_a\tstart_a\tstop_a\tstrand_a\tscore_a\tp-value_a\tmatched_sequence_a\t"
       "haplotype_frequency_a\tmotif_id_b\tmotif_alt_id_b\tstart_b\tstop_b\tstrand_b\tscore_b\tp-value_b\tmatched_sequence_b\t"
       "haplotype_frequency_b\tgap\tco_haplotypes\thaplotypes_EUR\treference\n"
       "c:0-60\tMA1.1\tONE\t2\t8\t+\t1.5\t1e-05\tACGTAC\t3\tMA2.1\tTWO\t12\t16\t+\t1.5\t1e-05\tGGCC\t4\t4\t3\t2\tref\n"
       "c:0-60\tMA1.1\tONE\t2\t8\t+\t1.5\t1e-05\tACGTAC\t3\tMA1.1\tONE\t30\t24\t-\t1.25\t2e-05\tTTGACA\t2\t16\t2\t1\tnon.ref\n"
       "c:0-60\tMA2.1\tTWO\t12\t16\t+\t1.5\t1e-05\tGGCC\t4\tMA1.1\tONE\t30\t24\t-\t1.25\t2e-05\tTTGACA\t2\t8\t2\t1\tnon.ref\n")


class _Out:
    def __init__(self, outdir):
        self.outdir = outdir


def test_to_frame_and_the_writer_give_the_exact_text(tmp_path, capsys, monkeypatch):
    from grafimo_amd import hit_pairs as hpm
    from grafimo_amd.res_writer import DEFAULT_OUTDIR
    hp = _hand_made()
    assert len(hp) == 3
    df = hp.to_frame()
    assert list(df.columns) == TSV.split("\n")[0].split("\t")
    buf = io.StringIO()
    assert hpm.write_hit_pairs(hp, None, out=buf) is None and buf.getvalue() == TSV
    path = hpm.write_hit_pairs(hp, _Out(str(tmp_path / "o")))
    assert path == str(tmp_path / "o" / "grafimo_hit_pairs.tsv") and open(path).read() == TSV
    monkeypatch.chdir(tmp_path)
    dflt = hpm.write_hit_pairs(hp, _Out(DEFAULT_OUTDIR))
    assert dflt == os.path.join(f"grafimo_out_{os.getpid()}_pairs", "grafimo_hit_pairs.tsv") and open(dflt).read() == TSV
    capsys.readouterr()
    hpm.print_hit_pairs(hp)
    assert capsys.readouterr().out == TSV
    back = pd.read_csv(path, sep="\t", keep_default_na=False)
    pd.testing.assert_frame_equal(back, df, check_dtype=False)


def test_an_empty_pair_table_has_the_columns():
    from grafimo_amd.hit_pairs import HitPairs
    hp = _hand_made()
    empty = HitPairs(hp.tables, [], [], [], [], [], [], [], ["EUR"], np.zeros((0, 1), np.int32), [], hp.region_names)
    df = empty.to_frame()
    assert len(df) == 0 and list(df.columns) == TSV.split("\n")[0].split("\t")


def test_hit_alleles_still_constructs_without_row_region():
    from grafimo_amd.hit_alleles import HitAlleles
    rep = pd.DataFrame({"motif_id": ["M"], "start": [1], "stop": [5]})
    ha = HitAlleles(rep, [0, 0], [], [], [], [], np.zeros((1, 0), np.int32), None, [], [None])
    assert ha.row_region is None and len(ha) == 1
    with pytest.raises(TypeError):
        HitAlleles(rep, [0, 0], [], [], [], [], np.zeros((1, 0), np.int32), None, [], [None], [0])     # keyword-only
    ha = HitAlleles(rep, [0, 0], [], [], [], [], np.zeros((1, 0), np.int32), None, [], [None], row_region=[3])
    assert ha.row_region.dtype == np.int64 and ha.row_region.tolist() == [3]


def test_the_binding_knows_the_export():
    from grafimo_amd import _native as nv
    assert "gfm_hit_pairs" in nv.PROTOTYPES and hasattr(nv.lib(), "gfm_hit_pairs")
    assert nv.lib().gfm_hit_pairs(None, None, None, None, 0, 0, 0, 0, 0, None, None, 0, None, None, None, 0, None, None) == nv.GFM_ERR_INVALID
    assert nv.lib().gfm_abi_version() == 12


def test_pair_rows_refuses_bad_rows_before_any_device_work():
    from grafimo_amd.hit_pairs import pair_rows
    one = np.ones((2, 1), np.uint64)
    with pytest.raises(ValueError, match="min_gap"):
        pair_rows([0, 0], [0, 5], [3, 9], one, 5, 4)
    with pytest.raises(ValueError, match="lo > hi"):
        pair_rows([0, 0], [4, 5], [3, 9], one, 0, 4)
    with pytest.raises(ValueError, match="beyond the last haplotype"):
        pair_rows([0, 0], [0, 5], [3, 9], np.full((2, 1), 8, np.uint64), 0, 4, n_haplotypes=3)
    with pytest.raises(ValueError, match="do not fill"):
        pair_rows([0, 0], [0, 5], [3, 9], one, 0, 4, n_haplotypes=65)
    with pytest.raises(ValueError, match="at most 64"):
        pair_rows([0, 0], [0, 5], [3, 9], one, 0, 4, group_bits=np.zeros((65, 1), np.uint64))
    a, b, j, gc = pair_rows([0], [0], [3], one[:1], 0, 4, group_bits=np.zeros((2, 1), np.uint64))       # one row: no pair, no device
    assert len(a) == len(b) == len(j) == 0 and gc.shape == (0, 2)


# ---- the command line

@pytest.mark.parametrize("argv,word", [
    (["-m", "x.meme", "-l", "a.fa", "-v", "a.vcf", "-b", "a.bed", "--haplotype-groups", "panel.txt"], "--haplotype-groups goes with"),
    (["-m", "x.meme", "-s", "dir", "--hit-pairs"], "--hit-pairs needs the graph"),
    (["-m", "x.meme", "-s", "dir", "--hit-pairs", "--haplotype-groups", "panel.txt"], "--hit-pairs needs the graph"),
    (["-m", "x.meme", "-l", "a.fa", "-v", "a.vcf", "-b", "a.bed", "--pair-gap", "0", "10"], "--pair-gap goes with --hit-pairs"),
    (["-m", "x.meme", "-l", "a.fa", "-v", "a.vcf", "-b", "a.bed", "--hit-pairs", "--pair-gap", "10", "0"], "--pair-gap MIN MAX"),
])
def test_the_command_line_refuses_the_flags_where_they_mean_nothing(argv, word, monkeypatch):
    from grafimo_amd import __main__ as cli
    monkeypatch.setattr(cli, "_Workflow", lambda a: pytest.fail("arguments must be refused before anything is set up"))
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert word in str(e.value)


def test_the_parser_takes_the_flags_and_negative_gaps():
    from grafimo_amd.__main__ import get_parser
    a = get_parser().parse_args(["-m", "x.meme", "--hit-pairs", "--pair-gap", "-5", "30", "--haplotype-groups", "p.txt"])
    assert a.hit_pairs and a.pair_gap == [-5, 30] and a.haplotype_groups == "p.txt"
    a = get_parser().parse_args(["-m", "x.meme", "--hit-pairs"])
    assert a.hit_pairs and a.pair_gap is None
