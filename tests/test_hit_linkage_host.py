"""Hit-linkage table without a GPU: the reference (tests/hit_linkage_bruteforce.py) against first principles, the host
statistics of grafimo_amd.hit_linkage against the reference, the exact tie, the undefined cases, the writer and the CLI."""
import io
import os
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grafimo_amd.hit_linkage import ld_statistics  # noqa: E402
from hit_linkage_bruteforce import ld_of_counts, links_reference, synthetic_input, unpack_bits  # noqa: E402
from hit_pair_bruteforce import pack  # noqa: E402


# ---- the reference against first principles

@pytest.mark.parametrize("H", [2, 7, 64, 65, 300])
def test_reference_equals_corrcoef_and_d_prime_stays_in_its_bounds(H):
    rng = np.random.default_rng(H)
    seen = 0
    for _ in range(200):
        c, a = rng.random(H) < rng.random(), rng.random(H) < rng.random()
        ld = ld_of_counts(H, c.sum(), a.sum(), (c & a).sum())
        if c.all() or a.all() or not c.any() or not a.any():
            assert ld is None
            continue
        r2, r, dp = ld
        cc = np.corrcoef(c.astype(float), a.astype(float))[0, 1]
        assert abs(cc * cc - r2) <= 1e-12 and abs(cc - r) <= 1e-12
        assert 0.0 <= r2 <= 1.0 and -1.0 <= dp <= 1.0 and (dp > 0) == (r > 0) and (dp == 0) == (r == 0)
        # |D'| == 1 exactly when one of the four haplotype classes is empty
        empty = min((c & a).sum(), (c & ~a).sum(), (~c & a).sum(), (~c & ~a).sum()) == 0
        assert (abs(dp) == 1.0) == bool(empty)
        seen += 1
    assert seen > (10 if H == 2 else 100)          # (two haplotypes are seldom both mixed)


def test_the_host_statistics_equal_the_reference():
    rng = np.random.default_rng(3)
    for H in (1, 2, 8, 5096, 32768):
        nh, na = rng.integers(0, H + 1, 500), rng.integers(0, H + 1, 500)
        nj = np.array([rng.integers(max(0, h + a - H), min(h, a) + 1) for h, a in zip(nh, na)])
        Dn, den, r2, r, dp = ld_statistics(nj, nh, na, H)
        for k in range(500):
            ld = ld_of_counts(H, nh[k], na[k], nj[k])
            assert int(Dn[k]) == H * int(nj[k]) - int(nh[k]) * int(na[k])
            assert int(den[k]) == int(nh[k]) * (H - int(nh[k])) * int(na[k]) * (H - int(na[k]))
            if ld is None:
                assert np.isnan(r2[k]) and np.isnan(r[k]) and np.isnan(dp[k])
            else:
                assert (r2[k], r[k], dp[k]) == ld


def _tie():
    """H = 8, n_hit = 4, n_allele = 4, n_joint = 3: Dn = 8, den = 256, r2 == 0.25"""
    row = pack(np.array([[1, 1, 1, 1, 0, 0, 0, 0]], bool))
    allele = np.zeros((1, 3, 1), np.uint64)
    allele[0, 0] = pack(np.array([[1, 1, 1, 0, 1, 0, 0, 0]], bool))[0]
    return [10], [14], row, [12], [1], allele


def test_the_exact_tie_is_listed_at_its_threshold_and_not_above():
    assert ld_of_counts(8, 4, 4, 3) == (0.25, 0.5, 0.5)
    at = links_reference(*_tie(), 0, 0.25, 8)
    assert at[0].tolist() == [0] and at[1].tolist() == [0] and at[2].tolist() == [1] and at[3].tolist() == [3] and at[6].tolist() == [0.25]
    assert len(links_reference(*_tie(), 0, np.nextafter(0.25, 1), 8)[0]) == 0


def test_the_undefined_cases_are_never_listed():
    H = 6
    vec = {"none": [0] * 6, "all": [1] * 6, "some": [1, 0, 1, 0, 0, 0]}
    for rname, aname in (("none", "some"), ("all", "some"), ("some", "none"), ("some", "all"), ("none", "none"), ("all", "all")):
        row = pack(np.array([vec[rname]], bool))
        allele = np.zeros((1, 3, 1), np.uint64)
        allele[0, 0] = pack(np.array([vec[aname]], bool))[0]
        got = links_reference([5], [9], row, [6], [1], allele, 0, 0.0, H)
        assert len(got[0]) == 0 and got[9] == 1, (rname, aname)
    # H = 1: every row and every allele is carried by nobody or by everybody
    lo, hi, masks, pos, n_alts, bits = synthetic_input(5, 1, n_rows=40, n_sites=60, span=300)
    got = links_reference(lo, hi, masks, pos, n_alts, bits, 60, 0.0, 1)
    assert len(got[0]) == 0 and got[9] > 100


def test_distance_counts_from_the_interval_and_unused_slots_are_ignored():
    H = 8
    row = pack(np.array([[1, 1, 0, 0, 0, 0, 0, 0]], bool))
    same = pack(np.array([[1, 1, 0, 0, 0, 0, 0, 0]], bool))[0]
    pos = [94, 95, 100, 109, 114, 115]                       # lo = 100, hi = 110, flank 5: 95 .. 114
    bits = np.zeros((6, 3, 1), np.uint64)
    bits[:, 0] = same
    bits[:, 1:] = same                                       # garbage in the unused slots: a perfect link if it were read
    got = links_reference([100], [110], row, pos, [1] * 6, bits, 5, 1.0, H)
    assert got[1].tolist() == [1, 2, 3, 4] and got[2].tolist() == [1] * 4 and got[9] == 4
    assert got[6].tolist() == [1.0] * 4 and got[8].tolist() == [1.0] * 4


def test_the_synthetic_input_has_links_and_mostly_candidates_that_are_none():
    """the figures the GPU tests' floors come from: at (flank 60, min_r2 0.2) every H >= 63 gives at least 40 links among
    some thousand candidates, fewer than a tenth of them"""
    for H in (63, 64, 65, 200):
        lo, hi, masks, pos, n_alts, bits = synthetic_input(100 + H, H)
        got = links_reference(lo, hi, masks, pos, n_alts, bits, 60, 0.2, H)
        L, cand = len(got[0]), got[9]
        assert 40 <= L < 0.1 * cand and 3000 <= cand <= 12000, (H, L, cand)
        used = unpack_bits(bits, H)[np.arange(3)[None, :] < np.asarray(n_alts)[:, None]]
        assert (~used.any(axis=1)).sum() >= 20                # sites carried by nobody


# ---- a hand-made table

class _Index:
    """what variant_effects._site_columns reads of a GraphIndex"""

    def __init__(self):
        self.ref = np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8)
        self.pos = np.array([3, 9, 15], np.int32)
        self.n_alts = np.array([1, 2, 1], np.uint8)
        self.alt_bases = np.array([[ord("A"), 0, 0], [ord("G"), ord("T"), 0], [0, 0, 0]], np.uint8)
        self.del_len = np.array([0, 0, 2], np.int32)
        self.ins_len = np.array([0, 0, 0], np.int32)
        self.ins_off = np.zeros(3, np.int32)
        self.ins_bases = np.zeros(0, np.uint8)
        self.n_haplotypes = 4
        self.alt_bits = np.zeros((3, 3, 1), np.uint64)


def _hand_made():
    from grafimo_amd.hit_alleles import HitAlleles
    from grafimo_amd.hit_linkage import HitLinkage
    rep = pd.DataFrame({"motif_id": ["MA1.1"] * 2, "motif_alt_id": ["ONE"] * 2, "sequence_name": ["c:0-20"] * 2, "start": [2, 14],
                        "stop": [8, 10], "strand": ["+", "-"], "score": [1.5, 1.25], "p-value": [1e-5, 2e-5],
                        "matched_sequence": ["GTACGT", "TACG"], "haplotype_frequency": [2, 1], "reference": ["non.ref", "ref"]})
    t = HitAlleles(rep, [0, 1, 1], [0], [0], [1], [], np.zeros((2, 0), np.int32), np.array([[0b0011], [0b0100]], np.uint64),
                   [f"h{k}" for k in range(4)], [_Index()], row_region=[0, 0], row_entry=[0, 0])
    return HitLinkage(t, row=[0, 0, 1], site=[0, 1, 2], allele=[1, 2, 1], entry=[0, 0, 0], distance=[0, 2, 2], n_joint=[2, 0, 1],
                      n_allele=[2, 2, 1], n_hit=[2, 2, 1], r2=[1.0, 1.0, 1.0], r=[1.0, -1.0, 1.0], d_prime=[1.0, -1.0, 1.0],
                      in_hit=[True, False, False])


TSV = ("sequence_name\tmotif_id\tmotif_alt_id\tstart\tstop\tstrand\tscore\tp-value\tmatched_sequence\thaplotype_frequency\t"
       "variant\tdistance\tallele_haplotypes\tco_haplotypes\tr2\tr\td_prime\tin_hit\n"
       "c:0-20\tMA1.1\tONE\t2\t8\t+\t1.5\t1e-05\tGTACGT\t2\t4:T>A\t0\t2\t2\t1.0\t1.0\t1.0\tTrue\n"
       "c:0-20\tMA1.1\tONE\t2\t8\t+\t1.5\t1e-05\tGTACGT\t2\t10:C>T\t2\t2\t0\t1.0\t-1.0\t-1.0\tFalse\n"
       "c:0-20\tMA1.1\tONE\t14\t10\t-\t1.25\t2e-05\tTACG\t1\t16:TAC>T\t2\t1\t1\t1.0\t1.0\t1.0\tFalse\n")


class _Out:
    def __init__(self, outdir):
        self.outdir = outdir


class _Motif:
    motif_id = "MA1.1"


def test_to_frame_and_the_writer_give_the_exact_text(tmp_path, capsys, monkeypatch):
    from grafimo_amd import hit_linkage as hlm
    from grafimo_amd.res_writer import DEFAULT_OUTDIR
    hl = _hand_made()
    assert len(hl) == 3
    df = hl.to_frame()
    assert list(df.columns) == TSV.split("\n")[0].split("\t")
    buf = io.StringIO()
    assert hlm.write_hit_linkage(hl, _Motif(), 1, None, out=buf) is None and buf.getvalue() == TSV
    path = hlm.write_hit_linkage(hl, _Motif(), 1, _Out(str(tmp_path / "o")))
    assert path == str(tmp_path / "o" / "grafimo_hit_linkage.tsv") and open(path).read() == TSV
    path = hlm.write_hit_linkage(hl, _Motif(), 2, _Out(str(tmp_path / "o")))
    assert path == str(tmp_path / "o" / "grafimo_hit_linkage_MA1.1.tsv") and open(path).read() == TSV
    monkeypatch.chdir(tmp_path)
    dflt = hlm.write_hit_linkage(hl, _Motif(), 2, _Out(DEFAULT_OUTDIR))
    assert dflt == os.path.join(f"grafimo_out_{os.getpid()}_MA1.1", "grafimo_hit_linkage.tsv") and open(dflt).read() == TSV
    capsys.readouterr()
    hlm.print_hit_linkage(hl)
    assert capsys.readouterr().out == TSV
    back = pd.read_csv(path, sep="\t", keep_default_na=False)
    pd.testing.assert_frame_equal(back, df, check_dtype=False)


def test_an_empty_table_has_the_columns():
    from grafimo_amd.hit_linkage import HitLinkage
    hl = _hand_made()
    empty = HitLinkage(hl.table, *([[]] * 12))
    df = empty.to_frame()
    assert len(empty) == 0 and len(df) == 0 and list(df.columns) == TSV.split("\n")[0].split("\t")


def test_hit_alleles_still_constructs_without_row_entry():
    from grafimo_amd.hit_alleles import HitAlleles
    rep = pd.DataFrame({"motif_id": ["M"], "start": [1], "stop": [5]})
    ha = HitAlleles(rep, [0, 0], [], [], [], [], np.zeros((1, 0), np.int32), None, [], [None])
    assert ha.row_entry is None and ha.row_region is None
    ha = HitAlleles(rep, [0, 0], [], [], [], [], np.zeros((1, 0), np.int32), None, [], [None], row_entry=[2])
    assert ha.row_entry.dtype == np.int64 and ha.row_entry.tolist() == [2]


def test_the_binding_knows_the_export():
    from grafimo_amd import _native as nv
    assert "gfm_hit_linkage" in nv.PROTOTYPES and hasattr(nv.lib(), "gfm_hit_linkage")
    total = nv.c_i64(-1)
    off = np.zeros(1, np.int64)
    good = [None, None, None, 0, None, None, None, 0, 1, 8, 0, 0.5, off.ctypes.data, 0, None, None, None, None, None, 0, 0, 0, total, None]

    def bad(k):
        """the call with the arguments k replaced: every one below is refused on its arguments, before any device work"""
        return nv.lib().gfm_hit_linkage(*[k.get(i, v) for i, v in enumerate(good)])

    for k in ({8: 2}, {9: 0}, {9: 32769, 8: 513}, {10: -1}, {11: 1.5}, {11: float("nan")}, {19: 7}, {19: 64}, {20: 32}, {20: 512},
              {21: 2}, {12: None}, {3: -1}, {7: -1}):
        assert bad(k) == nv.GFM_ERR_INVALID, k
        assert b"gfm_hit_linkage" in nv.lib().gfm_last_error()
    assert nv.lib().gfm_abi_version() == 12


def test_link_rows_refuses_bad_input_before_any_device_work():
    from grafimo_amd.hit_linkage import link_rows
    one = np.ones((2, 1), np.uint64)
    bits = np.ones((2, 3, 1), np.uint64)
    ok = dict(lo=[0, 5], hi=[3, 9], masks=one, pos=[1, 4], n_alts=[1, 1], allele_bits=bits, flank=5, min_r2=0.5, n_haplotypes=8)
    def refused(match, **k):
        with pytest.raises(ValueError, match=match):
            link_rows(**{**ok, **k})

    refused("haplotypes", n_haplotypes=32769, masks=np.ones((2, 513), np.uint64), allele_bits=np.ones((2, 3, 513), np.uint64))
    refused("haplotypes", n_haplotypes=0)
    refused("flank", flank=-1)
    refused("min_r2", min_r2=1.01)
    refused("min_r2", min_r2=-0.1)
    refused("rows_per_tile", rows_per_tile=12)
    refused("slots_per_chunk", slots_per_chunk=100)
    refused("lo > hi", lo=[4, 5])
    refused("ascending pos", pos=[4, 1])
    refused("more than 3", n_alts=[1, 4])
    refused("masks uint64", masks=np.ones((2, 2), np.uint64))
    refused("allele_bits uint64", allele_bits=np.ones((2, 2, 1), np.uint64))
    refused("carrier set has bits beyond", n_haplotypes=3, masks=np.full((2, 1), 8, np.uint64))
    refused("allele bitset has bits beyond", n_haplotypes=3, allele_bits=np.full((2, 3, 1), 8, np.uint64))
    got = link_rows([], [], np.zeros((0, 1), np.uint64), [1, 4], [1, 1], bits, 5, 0.5, 8)         # no rows: no device
    assert [len(x) for x in got] == [0] * 6 and got[2].dtype == np.uint8


# ---- the command line

GRAPH = ["-m", "x.meme", "-l", "a.fa", "-v", "a.vcf", "-b", "a.bed"]


@pytest.mark.parametrize("argv,word", [
    (["-m", "x.meme", "-s", "dir", "--hit-linkage"], "--hit-linkage needs the graph"),
    (GRAPH + ["--linkage-flank", "100"], "go with --hit-linkage"),
    (GRAPH + ["--linkage-r2", "0.5"], "go with --hit-linkage"),
    (GRAPH + ["--hit-linkage", "--linkage-flank", "-1"], "--linkage-flank -1 < 0"),
    (GRAPH + ["--hit-linkage", "--linkage-r2", "1.5"], "--linkage-r2 1.5 outside"),
])
def test_the_command_line_refuses_the_flags_where_they_mean_nothing(argv, word, monkeypatch):
    from grafimo_amd import __main__ as cli
    monkeypatch.setattr(cli, "_Workflow", lambda a: pytest.fail("arguments must be refused before anything is set up"))
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert word in str(e.value)


def test_the_parser_takes_the_flags():
    from grafimo_amd.__main__ import get_parser
    a = get_parser().parse_args(["-m", "x.meme", "--hit-linkage", "--linkage-flank", "250", "--linkage-r2", "0.5"])
    assert a.hit_linkage and a.linkage_flank == 250 and a.linkage_r2 == 0.5
    a = get_parser().parse_args(["-m", "x.meme", "--hit-linkage"])
    assert a.hit_linkage and a.linkage_flank is None and a.linkage_r2 is None
    assert not get_parser().parse_args(["-m", "x.meme"]).hit_linkage
