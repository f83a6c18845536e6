"""The host half of the per-hit allele table, no GPU: gfm_graph_hit_order (csrc/hit_table.cpp) against the columns
gfm_graph_hit_columns makes from the same records, the haplotype group readers, the strings and files of a hand-made
HitAlleles, and the command line's argument errors."""
import ctypes
import io
import os
import warnings

import numpy as np
import pandas as pd
import pytest

from grafimo_amd import _native as nv
from grafimo_amd import extract_regions as xr
from grafimo_amd import hit_alleles as hal
from grafimo_amd.graph_tables import _site_columns
from test_hit_table_host import _records, _reference_columns


def _ptable(rng, W):
    L = 1000 * W + 1
    pmf = rng.random(L)
    ptable = np.minimum.accumulate(np.cumsum(pmf[::-1])[::-1] / pmf.sum())
    ptable[L // 2 + 10:L // 2 + 20] = ptable[L // 2 + 10]          # different scores, one p-value: row order decides
    return ptable


def _check_order(ptable, W, parts, entry_of, region_base, recomb):
    spec = (ptable, 37, -12.0, W, entry_of, region_base, parts, recomb, False)
    part, index = hal._report_order(spec)
    assert part.dtype == np.int32 and index.dtype == np.int64 and len(part) == len(index)
    pairs = set(zip(part.tolist(), index.tolist()))
    assert len(pairs) == len(part)                                   # no record twice
    got = xr._hit_columns(*spec)
    want = _reference_columns(ptable, 37, -12.0, W, parts, entry_of, region_base, recomb, False)
    assert len(part) == len(got["start"]) == len(want["start"])
    # the records gathered by (part, index), made into columns as gfm_graph_hit_columns' emit step makes them
    recs = np.empty(len(part), dtype=xr.HIT_DTYPE)
    for p_ in range(len(parts)):
        sel = part == p_
        assert (index[sel] >= 0).all() and (index[sel] < len(parts[p_])).all()
        recs[sel] = parts[p_][index[sel]]
    gid = recs["region"].astype(np.int64) + np.asarray(region_base)[part]
    mine = dict(start=recs["start"], stop=recs["stop"], freq=recs["freq"], region=gid,
                logodds=recs["score"].astype(np.float64) / 37.0 + float(W) * -12.0, pvalue=ptable[recs["score"]],
                qvalue=recs["qvalue"], strand=(recs["strand"] == ord("-")).astype(np.uint8),
                ref=((recs["is_ref"] != 0) & (np.abs(recs["stop"] - recs["start"]) == W)).astype(np.uint8),
                kmers=np.concatenate([recs["kmer"][:, :W], np.full((len(recs), 1), 10, np.uint8)], axis=1))
    assert set(mine) == set(got) == set(want)
    for k in got:
        assert np.array_equal(mine[k], got[k]), k
        assert np.array_equal(mine[k], want[k]), k
    return len(part)


@pytest.mark.parametrize("W,n_parts,dup", [(19, 1, True), (8, 3, True), (64, 2, False), (1, 1, True)])
@pytest.mark.parametrize("recomb", [True, False])
def test_the_order_entry_point_names_the_record_of_every_row(W, n_parts, dup, recomb):
    rng = np.random.default_rng(2000 * W + n_parts + 2 * recomb)
    ptable = _ptable(rng, W)
    n_regions = [int(rng.integers(1, 400)) for _ in range(n_parts)]
    parts = [_records(rng, int(rng.integers(1, 3000)), W, nr, dup_scores=dup) for nr in n_regions]
    if n_parts == 3:
        parts[1] = parts[1][:0]                                       # a handle without a hit
    entry_of = [np.sort(rng.integers(10 * p, 10 * p + 3, nr)).astype(np.int64) for p, nr in enumerate(n_regions)]
    region_base = np.cumsum([0] + n_regions).astype(np.int64)
    _check_order(ptable, W, parts, entry_of, region_base, recomb)


@pytest.mark.parametrize("recomb", [True, False])
def test_the_order_of_a_large_table_built_by_several_threads(recomb):
    rng = np.random.default_rng(23 + recomb)
    for n, dup in ((30_000, True), (4_300, False)):
        W = 19
        ptable = _ptable(rng, W)
        n_regions = [700, 900]
        parts = [_records(rng, n, W, n_regions[0], n_win=40_000, dup_scores=dup),
                 _records(rng, n // 3, W, n_regions[1], n_win=40_000, dup_scores=dup)]
        parts[0]["keep"] = 1                                          # (>= 4 096 rows stay whatever the filters drop)
        parts[0]["freq"] = np.maximum(parts[0]["freq"], 1)
        entry_of = [np.sort(rng.integers(10 * p, 10 * p + 3, nr)).astype(np.int64) for p, nr in enumerate(n_regions)]
        region_base = np.cumsum([0] + n_regions).astype(np.int64)
        assert _check_order(ptable, W, parts, entry_of, region_base, recomb) >= 4096


def test_order_arguments_and_empty_input():
    pt = np.ones(19001)
    part, index = hal._report_order((pt, 62, -14.0, 19, [np.zeros(0, np.int64)], np.zeros(2, np.int64),
                                     [np.empty(0, xr.HIT_DTYPE)], True, False))
    assert len(part) == 0 and len(index) == 0
    n_out = ctypes.c_int64()
    assert nv.lib().gfm_graph_hit_order(None, 1, 0, None, None, None, 0, n_out, None, None) == nv.GFM_ERR_INVALID
    rec = np.zeros(1, dtype=xr.HIT_DTYPE)
    rec["keep"], rec["freq"] = 1, 1
    recs_p = (ctypes.c_void_p * 1)(rec.ctypes.data)
    n_recs = (ctypes.c_int64 * 1)(1)
    o_part, o_index = np.empty(1, np.int32), np.empty(1, np.int64)
    rc = nv.lib().gfm_graph_hit_order(nv.ptr(pt), len(pt), 1, recs_p, n_recs, None, nv.GFM_HITS_FIRST_PER_REGION, n_out,
                                      nv.ptr(o_part), nv.ptr(o_index))
    assert rc == nv.GFM_ERR_INVALID and b"FIRST_PER_REGION" in nv.lib().gfm_last_error()
    assert nv.lib().gfm_graph_hit_order(nv.ptr(pt), len(pt), 1, recs_p, n_recs, None, 0, n_out, nv.ptr(o_part),
                                        nv.ptr(o_index)) == nv.GFM_OK
    assert n_out.value == 1 and o_part[0] == 0 and o_index[0] == 0
    with pytest.raises(ValueError):
        hal._report_order((pt, 62, -14.0, 19, [np.zeros(1, np.int64)], np.zeros(2, np.int64), [rec], True, True))


# ---- haplotype groups

PANEL = """sample\tpop\tsuper_pop\tgender
# a comment
HG001\tGBR\tEUR\tmale
HG002\tFIN\tEUR\tfemale

NA999\tYRI\tAFR\tfemale
HG003\tGBR\tEUR\tfemale
NA998\tYRI\tAFR\tmale
"""


def test_read_haplotype_groups_reads_a_panel_file(tmp_path):
    path = tmp_path / "panel.txt"
    path.write_text(PANEL)
    names = [f"{s}|{k}" for s in ("HG001", "HG002", "HG003", "HG004") for k in (1, 2)]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        groups = hal.read_haplotype_groups(str(path), names)
    assert list(groups) == ["GBR", "FIN"]                              # the file's order; YRI has no sample of the graph
    assert groups == {"GBR": [0, 1, 4, 5], "FIN": [2, 3]}
    assert len(w) == 1 and "2 samples" in str(w[0].message)


def test_read_haplotype_groups_of_an_unnamed_graph(tmp_path):
    path = tmp_path / "groups.txt"
    path.write_text("hap0 A\nhap2 A extra\nhap1 B\nhap7 B\n")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        groups = hal.read_haplotype_groups(str(path), [f"hap{k}" for k in range(5)])
    assert groups == {"A": [0, 2], "B": [1]} and len(w) == 1
    path.write_text("hap0\n")
    with pytest.raises(ValueError):
        hal.read_haplotype_groups(str(path), ["hap0"])


def test_group_bitsets_of_the_mapping_form():
    names = [f"s{k}" for k in range(70)]
    gnames, bits = hal._group_bits({"low": ["s0", "s1", 65], "both": [1, "s69"], "none": []}, names, 70)
    assert gnames == ["low", "both", "none"] and bits.shape == (3, 2) and bits.dtype == np.uint64
    assert bits[0].tolist() == [3, 2] and bits[1].tolist() == [2, 1 << 5] and bits[2].tolist() == [0, 0]   # overlapping groups
    assert hal._group_bits(None, names, 70)[1].shape == (0, 2)
    with pytest.raises(ValueError, match="unknown haplotype"):
        hal._group_bits({"g": ["nobody"]}, names, 70)
    with pytest.raises(ValueError, match="outside"):
        hal._group_bits({"g": [70]}, names, 70)
    with pytest.raises(ValueError, match="at most 64"):
        hal._group_bits({f"g{k}": [0] for k in range(65)}, names, 70)


# ---- a hand-made table

class _M:
    motif_id, motif_name = "MA0000.1", "TEST"


def _hand_made():
    from grafimo_amd.extract_regions import MAX_ALTS, GraphIndex
    ref = np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8)
    pos = np.array([3, 6, 9, 12], np.int32)                 # SNV, SNV with two ALTs, insertion, deletion
    n_alts = np.array([1, 2, 1, 1], np.uint8)
    alt = np.zeros((4, MAX_ALTS), np.uint8)
    alt[0, 0], alt[1, 0], alt[1, 1] = ord("A"), ord("A"), ord("C")
    H = 6
    bits = np.zeros((4, MAX_ALTS, 1), np.uint64)
    bits[0, 0, 0], bits[1, 0, 0], bits[1, 1, 0], bits[2, 0, 0], bits[3, 0, 0] = 0b000011, 0b000100, 0b011000, 0b100001, 0b000010
    idx = GraphIndex("c", ref, pos, n_alts, alt, bits, H, del_len=np.array([0, 0, 0, 3], np.int32),
                     ins_len=np.array([0, 0, 2, 0], np.int32), ins_off=np.array([0, 0, 0, 2], np.int32),
                     ins_bases=np.frombuffer(b"GG", dtype=np.uint8))
    report = pd.DataFrame({"motif_id": ["MA0000.1"] * 4, "motif_alt_id": ["TEST"] * 4, "sequence_name": ["c:0-20"] * 4,
                           "start": [1, 5, 8, 0], "stop": [5, 9, 14, 4], "strand": ["+", "-", "+", "+"],
                           "score": [1.0, 0.5, 0.25, 0.1], "p-value": [1e-5, 2e-5, 3e-5, 4e-5],
                           "matched_sequence": ["CGAA", "TGCG", "CGGT", "ACGT"], "haplotype_frequency": [2, 2, 1, 6],
                           "reference": ["non.ref", "non.ref", "non.ref", "ref"]})
    # row 0: SNV ALT; row 1: the multi-allelic SNV's second ALT beside the first SNV's REF; row 2: insertion read, deletion
    # jumped and the second SNV's REF; row 3: nothing
    offsets = [0, 1, 3, 6, 6]
    site = [0, 0, 1, 1, 2, 3]
    allele = [1, 0, 2, 0, 1, 1]
    ha = hal.HitAlleles(report, offsets, [0] * 6, site, allele, ["EUR", "AFR"], [[2, 0], [1, 1], [0, 1], [3, 3]],
                        np.array([[0b000011], [0b011000], [0b000001], [0b111111]], np.uint64),
                        [f"S{k // 2}|{k % 2 + 1}" for k in range(H)], [idx])
    return idx, ha


def test_to_frame_prints_the_alleles_as_the_variant_table_prints_its_sites():
    idx, ha = _hand_made()
    df = ha.to_frame()
    assert list(df.columns) == list(ha.report.columns) + ["alt_alleles", "ref_alleles", "haplotypes_EUR", "haplotypes_AFR"]
    pd.testing.assert_frame_equal(df[list(ha.report.columns)], ha.report)
    pos, refs, alts, _, _ = _site_columns(idx, np.array([0, 1, 2, 3]), np.array([1, 2, 1, 1]))
    s = lambda i: f"{pos[i]}:{refs[i]}>{alts[i]}"      # noqa: E731
    r = lambda i: f"{pos[i]}:{refs[i]}"                # noqa: E731
    assert (s(0), s(1), s(2), s(3)) == ("4:T>A", "7:G>C", "10:C>CGG", "13:ACGT>A")      # (what _site_columns prints)
    assert df["alt_alleles"].tolist() == [s(0), s(1), s(2) + ";" + s(3), ""]
    assert df["ref_alleles"].tolist() == ["", r(0), r(1), ""]
    assert df["haplotypes_EUR"].tolist() == [2, 1, 0, 3] and df["haplotypes_AFR"].tolist() == [0, 1, 1, 3]
    assert ha.alleles(2) == [(0, 1, 0), (0, 2, 1), (0, 3, 1)] and ha.alleles(3) == []
    assert ha.carriers(0) == ["S0|1", "S0|2"] and ha.carriers(1) == ["S1|2", "S2|1"] and len(ha.carriers(3)) == 6
    assert len(ha) == 4


class _Args:
    def __init__(self, outdir):
        self.outdir = outdir


def test_the_writer_names_its_files_as_the_other_tables_do(tmp_path, capsys, monkeypatch):
    _, ha = _hand_made()
    one = hal.write_hit_alleles(ha, _M, 1, _Args(str(tmp_path / "one")))
    assert one == str(tmp_path / "one" / "grafimo_hit_alleles.tsv")
    many = hal.write_hit_alleles(ha, _M, 3, _Args(str(tmp_path / "many")))
    assert many == str(tmp_path / "many" / "grafimo_hit_alleles_MA0000.1.tsv")
    back = pd.read_csv(one, sep="\t", keep_default_na=False)
    assert list(back.columns) == list(ha.to_frame().columns) and len(back) == 4
    assert back["alt_alleles"].tolist() == ha.to_frame()["alt_alleles"].tolist()
    assert open(one).read() == open(many).read()
    monkeypatch.chdir(tmp_path)
    from grafimo_amd.res_writer import DEFAULT_OUTDIR
    dflt = hal.write_hit_alleles(ha, _M, 3, _Args(DEFAULT_OUTDIR))
    assert dflt == os.path.join(f"grafimo_out_{os.getpid()}_MA0000.1", "grafimo_hit_alleles.tsv")
    # -f: the same bytes on stdout, no file
    before = sorted(os.listdir(tmp_path))
    capsys.readouterr()
    hal.print_hit_alleles(ha)
    assert capsys.readouterr().out == open(one).read()
    assert sorted(os.listdir(tmp_path)) == before
    buf = io.StringIO()
    assert hal.write_hit_alleles(ha, None, 1, None, out=buf) is None and buf.getvalue() == open(one).read()


def test_an_empty_table_has_the_columns():
    _, ha = _hand_made()
    empty = hal.HitAlleles(ha.report.iloc[:0].reset_index(drop=True), [0], [], [], [], ["EUR"], np.zeros((0, 1), np.int32), None,
                           ha.haplotype_names, ha.indexes)
    df = empty.to_frame()
    assert len(df) == 0 and list(df.columns) == list(ha.report.columns) + ["alt_alleles", "ref_alleles", "haplotypes_EUR"]
    with pytest.raises(ValueError):
        empty.carriers(0)


@pytest.mark.parametrize("argv,word", [
    (["-m", "x.meme", "-l", "a.fa", "-v", "a.vcf", "-b", "a.bed", "--haplotype-groups", "panel.txt"], "--haplotype-groups goes with"),
    (["-m", "x.meme", "-s", "dir", "--hit-alleles"], "--hit-alleles needs the graph"),
    (["-m", "x.meme", "-s", "dir", "--hit-alleles", "--haplotype-groups", "panel.txt"], "--hit-alleles needs the graph"),
    (["-m", "x.meme", "-s", "dir", "--haplotype-groups", "panel.txt"], "--haplotype-groups goes with"),
])
def test_the_command_line_refuses_the_flags_where_they_mean_nothing(argv, word, monkeypatch):
    from grafimo_amd import __main__ as cli
    monkeypatch.setattr(cli, "_Workflow", lambda a: pytest.fail("arguments must be refused before anything is set up"))
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert word in str(e.value)
