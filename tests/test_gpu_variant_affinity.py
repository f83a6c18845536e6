"""Per-variant affinity table on the GPU (gfm_graph_variant_affinity -> grafimo_amd.variant_affinity): the four arrays -- ref_sum,
alt_sum, ref_rows, alt_rows -- equal, AS INTEGERS, the brute force of tests/variant_affinity_bruteforce.py; they depend neither on
how many regions hold an occurrence nor on the size of the device's staging table; the variant-effect table finds a side
exactly where a side has rows; the refusals, the call variants, the manifest route and the CLI.  No tolerance on a sum or a
count: the device adds 64-bit integers."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_helpers import make_consistent_graph_files, motif_as_oracle_dict  # noqa: E402
from variant_affinity_bruteforce import expected_rows, variant_affinity_sums  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")


class _Args:
    def __init__(self, threshold=1e-4, no_reverse=False, recomb=False, qvalue_t=False, no_qvalue=True):
        self.threshold, self.noreverse, self.recomb = threshold, no_reverse, recomb
        self.noqvalue, self.qvalueT = no_qvalue, qvalue_t


def _motif(W, seed=0):
    from grafimo_amd import synth
    rec = synth.synthetic_motif(W, np.random.default_rng(6100 + 17 * W + seed), np.array([0.3, 0.2, 0.2, 0.3]))
    return synth.motif_object(rec, f"SYN{W}")


def _ctcf():
    from grafimo_amd.motif_ops import build_motif_meme_host
    return build_motif_meme_host(os.path.join(GOLD, "MA0139.1.meme"), "unfrm_dst", 0.1, False)[0]


def _expected(idx, regions, motif, weights, no_reverse, memo=False):
    od = motif_as_oracle_dict(motif)
    sums, rows = variant_affinity_sums(idx, regions, od["width"], od["score_matrix"], od["min_val"], weights,
                                       forward_only=no_reverse, memo=memo)
    assert all(v < (1 << 64) for v in sums.values())
    return expected_rows(idx, sums, rows)


def _arrays(va):
    return [tuple(int(x) for x in r) for r in zip(va.site, va.allele, va.ref_sum, va.alt_sum, va.ref_rows, va.alt_rows)]


def _check(va, idx, regions, motif, no_reverse, temperature=1.0, weights=None, exp=None, memo=False):
    """the table's rows and their four integers against the brute force, and what the table makes of them -> the expected rows"""
    from grafimo_amd.graph_tables import _site_columns
    from grafimo_amd.haplotype_affinity import FRACTION_BITS, default_weights
    off = 0.0
    if weights is None:
        weights, s_best = default_weights(motif, temperature)
        off = -FRACTION_BITS + (s_best / motif.scale + motif.width * motif.offset) / temperature
    if exp is None:
        exp = _expected(idx, regions, motif, weights, no_reverse, memo)
    for name in ("ref_sum", "alt_sum", "ref_rows", "alt_rows"):
        assert getattr(va, name).dtype == np.uint64
    got = _arrays(va)
    assert got == exp, [(g, e) for g, e in zip(got, exp) if g != e][:5] + [len(got), len(exp)]
    assert va.log2_offset == off
    f = va.to_frame()
    assert len(f) == len(exp)
    if not exp:
        return exp
    site, allele = np.array([e[0] for e in exp]), np.array([e[1] for e in exp])
    position, refs, alts, ref_h, alt_h = _site_columns(idx, site, allele)
    assert f["position"].tolist() == position.tolist() and f["ref"].tolist() == refs.tolist() and f["alt"].tolist() == alts.tolist()
    assert f["ref_haplotypes"].tolist() == ref_h.tolist() and f["alt_haplotypes"].tolist() == alt_h.tolist()
    assert f["ref_rows"].tolist() == [e[4] for e in exp] and f["alt_rows"].tolist() == [e[5] for e in exp]
    for k, side, hap in ((2, "ref", ref_h), (3, "alt", alt_h)):
        s = np.array([e[k] for e in exp], dtype=np.uint64)
        col = f[f"{side}_log2_affinity"].to_numpy()
        assert (np.isnan(col) == (s == 0)).all()
        some = s > 0
        # (float64 log2 of the same integers made in another array: equal to an ulp or two of values below 100)
        want = np.log2(s[some].astype(np.float64)) - np.log2(hap[some].astype(np.float64)) + off
        assert np.allclose(col[some], want, rtol=0, atol=1e-12)
    d = f["delta_log2_affinity"].to_numpy()
    both = ~np.isnan(f["ref_log2_affinity"].to_numpy()) & ~np.isnan(f["alt_log2_affinity"].to_numpy())
    assert (np.isnan(d) == ~both).all()
    assert np.array_equal(d[both], (f["alt_log2_affinity"].to_numpy() - f["ref_log2_affinity"].to_numpy())[both])
    return exp


def _regions(idx, W, length=400):
    """overlapping, nested, the whole chromosome, shorter than W, starting / ending on a site, out of range"""
    p = idx.pos
    return [(0, int(p[len(p) // 3]) + 1), (int(p[len(p) // 3]) - 2, int(p[2 * len(p) // 3])), (int(p[-3]), length), (0, length),
            (3, 4), (int(p[len(p) // 2]), int(p[len(p) // 2]) + W + 3), (-10, length + 100)]


@pytest.mark.parametrize("W", [5, 8, 19, 30, 64])
@pytest.mark.parametrize("no_reverse", [False, True])
def test_bruteforce_parity(tmp_path, W, no_reverse):
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.variant_affinity import compute_variant_affinity
    seed = W + int(no_reverse)
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=seed, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = _regions(idx, W)
    assert (0, 400) in regions and (-10, 500) in regions          # (an occurrence counts once however many regions hold it)
    motif = _motif(W, seed)
    g = DeviceGraph(idx)
    va = compute_variant_affinity(motif, g, regions, False, _Args(no_reverse=no_reverse))
    exp = _check(va, idx, regions, motif, no_reverse)
    assert len(exp) > 10 and any(e[4] and e[5] for e in exp)
    assert (va.sequence_name == "c").all()
    # the whole chromosome alone holds every occurrence the list holds
    whole = compute_variant_affinity(motif, g, [(0, 400)], False, _Args(no_reverse=no_reverse))
    assert _arrays(whole) == exp
    if W == 8:                                           # once at another temperature, once with a filter
        cold = compute_variant_affinity(motif, g, regions, False, _Args(no_reverse=no_reverse), temperature=0.5)
        assert [e[2:4] for e in _check(cold, idx, regions, motif, no_reverse, temperature=0.5)] != [e[2:4] for e in exp]
        d = va.delta_log2_affinity
        cut = float(np.nanmedian(np.abs(d)))
        kept = compute_variant_affinity(motif, g, regions, False, _Args(no_reverse=no_reverse), min_abs_delta=cut)
        ok = np.isfinite(d) & (np.abs(d) >= cut)
        assert 0 < len(kept) < len(va) and _arrays(kept) == [r for r, k in zip(exp, ok) if k]
    g.close()


@pytest.mark.parametrize("n_samples,W,no_reverse", [(33, 8, False), (40, 12, True)])
def test_popcount_crosses_bitset_words(tmp_path, n_samples, W, no_reverse):
    """66 and 80 haplotypes: two bitset words, the second one partly used -- a walk's carriers are counted over both"""
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.variant_affinity import compute_variant_affinity
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=n_samples, seed=50 + n_samples, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    assert idx.hw == 2
    regions = [(0, 250), (200, 400), (-5, 1000)]
    motif = _motif(W, n_samples)
    va = compute_variant_affinity(motif, idx, regions, False, _Args(no_reverse=no_reverse))
    exp = _check(va, idx, regions, motif, no_reverse, memo=True)
    # (the precondition: alleles with carriers in the second word, and rows on both sides of some of them)
    second = {(i, k + 1) for i, k in zip(*np.nonzero(np.asarray(idx.alt_bits)[:, :, 1]))}
    assert sum(1 for e in exp if (e[0], e[1]) in second and e[4] and e[5]) > 5


def _dense_snv_graph(n_hap, seed=5, length=120, first=40, n_sites=12):
    """biallelic SNVs every 2 bases: a window of 19 bases holds up to 10 of them -- 2^10 walks on one layout"""
    from grafimo_amd.extract_regions import GraphIndex
    rng = np.random.default_rng(seed)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)]
    pos = np.arange(first, first + 2 * n_sites, 2, dtype=np.int32)
    alt = np.zeros((len(pos), 3), np.uint8)
    alt[:, 0] = np.where(ref[pos] == ord("A"), ord("C"), ord("A"))
    hw = (n_hap + 63) // 64
    carry = rng.random((len(pos), n_hap)) < 0.4
    bits = np.zeros((len(pos), 3, hw), np.uint64)
    for h in range(n_hap):
        bits[:, 0, h >> 6] |= carry[:, h].astype(np.uint64) << np.uint64(h & 63)
    return GraphIndex("c", ref, pos, np.ones(len(pos), np.uint8), alt, bits, n_hap)


def test_more_than_64_walks_on_a_layout():
    """the lanes take a layout's walks 64 at a time: a window of 2^10 walks goes round sixteen times.  70 haplotypes with
    random alleles: most walks are carried by nobody or by one"""
    from grafimo_amd.variant_affinity import compute_variant_affinity
    idx = _dense_snv_graph(70)
    W = 19
    walks = [sum(1 for _ in idx.window_walks(p, W)) for p in range(30, 70)]
    assert max(walks) == 1 << 10 and sum(n > 64 for n in walks) > 10          # the precondition, from the host enumerator
    motif = _ctcf()
    for regions, fwd in (([(0, 120)], False), ([(20, 80), (50, 120), (60, 64)], True)):
        va = compute_variant_affinity(motif, idx, regions, False, _Args(no_reverse=fwd))
        exp = _check(va, idx, regions, motif, fwd, memo=True)
        assert len(exp) == len(idx.pos)


def test_result_does_not_depend_on_the_staging_table(tmp_path):
    """a staging table of 1, 2 or 4 entries under windows that meet many more slots: the adds that find it full go to global
    memory, the result is the same"""
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.variant_affinity import compute_variant_affinity
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=77, kinds="sidmDOc")
    motif = _motif(19, 7)
    for idx, regions, memo in ((GraphIndex.from_fasta_vcf(fa, vcf, "c"), [(0, 400), (100, 300)], False),
                               (_dense_snv_graph(70), [(0, 120)], True)):
        # a window of 19 bases over k sites meets at least 2 k slots
        assert int(np.diff(np.searchsorted(idx.pos, [[p, p + 19] for p in range(len(idx.ref))]), axis=1).max()) >= 3
        g = DeviceGraph(idx)
        ref = compute_variant_affinity(motif, g, regions, False, _Args())
        exp = _check(ref, idx, regions, motif, False, memo=memo)
        for entries in (1, 2, 4, 64):
            got = compute_variant_affinity(motif, g, regions, False, _Args(), table_entries=entries)
            assert _arrays(got) == exp, entries
        g.close()


@pytest.mark.parametrize("seed,W,no_reverse", [(21, 8, False), (22, 19, True)])
def test_rows_exactly_where_variant_effects_finds_a_side(tmp_path, seed, W, no_reverse):
    """a product cross-route: with all_sites the variant-effect table has a row where either allele has a qualifying k-mer, and
    a side's best hit where that side has one -- the rows and the sides with rows > 0 here"""
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.variant_affinity import compute_variant_affinity
    from grafimo_amd.variant_effects import compute_variant_effects
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=seed, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = _regions(idx, W)[:3]
    motif = _motif(W, seed)
    args = _Args(threshold=1e-4, no_reverse=no_reverse)
    va = compute_variant_affinity(motif, idx, regions, False, args).to_frame()
    ve = compute_variant_effects(motif, idx, regions, False, args, all_sites=True)
    key = ["sequence_name", "position", "ref", "alt", "ref_haplotypes", "alt_haplotypes"]
    assert len(va) > 0 and va[key].values.tolist() == ve[key].values.tolist()
    assert ((va["ref_rows"] > 0).to_numpy() == (ve["ref_sequence"] != "").to_numpy()).all()
    assert ((va["alt_rows"] > 0).to_numpy() == (ve["alt_sequence"] != "").to_numpy()).all()


def test_zero_one_table_counts_the_occurrences_above_the_cutoff(tmp_path):
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.variant_affinity import compute_variant_affinity
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=13, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = [(0, 250), (200, 400)]
    W = 8
    motif = _motif(W, 13)
    od = motif_as_oracle_dict(motif)
    L = 1000 * W + 1
    g = DeviceGraph(idx)
    ones = compute_variant_affinity(motif, g, regions, False, _Args(), weights=np.ones(L, dtype=np.uint64))
    assert len(ones) > 0 and (ones.ref_sum == ones.ref_rows).all() and (ones.alt_sum == ones.alt_rows).all()
    assert ones.log2_offset == 0.0
    cutoff = int(np.median(od["score_matrix"].max(axis=0))) * W // 2
    w = (np.arange(L) >= cutoff).astype(np.uint64)
    va = compute_variant_affinity(motif, g, regions, False, _Args(), weights=w)
    exp = _check(va, idx, regions, motif, False, weights=w)
    # the rows are the table's whatever the weights; the sums count the occurrences at or above the cutoff: fewer
    assert _arrays(va) != _arrays(ones) and [e[:2] + e[4:] for e in exp] == [r[:2] + r[4:] for r in _arrays(ones)]
    assert (va.ref_sum <= va.ref_rows).all() and (va.alt_sum <= va.alt_rows).all() and int(va.ref_sum.sum()) > 0
    with pytest.raises(ValueError, match="weight table of shape"):
        compute_variant_affinity(motif, g, regions, False, _Args(), weights=w[:-1])
    g.close()


def test_flags_many_and_refusals(tmp_path):
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.variant_affinity import compute_variant_affinity, compute_variant_affinity_many
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=400, n_samples=12, seed=29, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    regions = [(0, 300), (200, 400)]
    m = _motif(8, 1)
    ref = compute_variant_affinity(m, idx, regions, False, _Args())
    exp = _check(ref, idx, regions, m, False)
    # --recomb, -t, -q, --qvalueT change nothing
    for args in (_Args(recomb=True), _Args(threshold=1e-8), _Args(threshold=0.5, qvalue_t=True, no_qvalue=False)):
        assert _arrays(compute_variant_affinity(m, idx, regions, False, args)) == exp
    motifs = [_motif(8, 1), _motif(12, 2), _motif(8, 3), _motif(12, 4)]
    many = compute_variant_affinity_many(motifs, idx, regions, False, _Args())
    for mo, t in zip(motifs, many):
        one = compute_variant_affinity(mo, idx, regions, False, _Args())
        assert t.motif_id == mo.motif_id and t.log2_offset == one.log2_offset and _arrays(t) == _arrays(one)
        pd.testing.assert_frame_equal(t.to_frame(), one.to_frame())
    assert _arrays(many[0]) == exp and _arrays(many[1]) != exp
    # two entries (chromosomes): the rows of the first, then the second's, named as the caller names them
    fa2, vcf2 = make_consistent_graph_files(str(tmp_path), length=300, n_samples=12, seed=30, kinds="sidmDOc")
    idx2 = GraphIndex.from_fasta_vcf(fa2, vcf2, "c")
    two = compute_variant_affinity(m, [idx2, idx], [[(0, 300)], regions], False, _Args(), chrom_names=["a", "b"])
    first = compute_variant_affinity(m, idx2, [(0, 300)], False, _Args())
    assert len(first) > 0 and _arrays(two) == _arrays(first) + exp
    assert two.sequence_name.tolist() == ["a"] * len(first) + ["b"] * len(exp)
    bare = GraphIndex("c", np.frombuffer(b"ACGT" * 25, dtype=np.uint8), np.array([10], np.int32), np.array([1], np.uint8),
                      np.array([[ord("A"), 0, 0]], np.uint8), None, 0)
    with pytest.raises(ValueError, match="carries no haplotypes"):
        compute_variant_affinity(m, bare, [(0, 100)], False, _Args())
    # a region shorter than the motif: an empty table with the columns
    from grafimo_amd.variant_affinity import COLUMNS
    none = compute_variant_affinity(m, idx, [(3, 4)], False, _Args())
    assert _check(none, idx, [(3, 4)], m, False) == [] and list(none.to_frame().columns) == COLUMNS


@pytest.mark.parametrize("no_reverse", [False, True])
def test_a_wrapped_sum_is_an_error(tmp_path, no_reverse):
    """weights of 2^63: two strands, or two carriers, or two occurrences of a slot wrap the 64-bit sum -- detected on the
    device, at whichever add it happens; the largest weights that fit are summed exactly"""
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.variant_affinity import compute_variant_affinity
    fa, vcf = make_consistent_graph_files(str(tmp_path), length=300, n_samples=6, seed=41, kinds="sidmDOc")
    idx = GraphIndex.from_fasta_vcf(fa, vcf, "c")
    motif = _motif(8, 4)
    L = 1000 * 8 + 1
    regions = [(10, 200), (0, 300)]
    g = DeviceGraph(idx)
    with pytest.raises(OverflowError, match="^c: a 64-bit affinity sum wrapped"):
        compute_variant_affinity(motif, g, regions, False, _Args(no_reverse=no_reverse), weights=np.full(L, 1 << 63, dtype=np.uint64))
    ones = compute_variant_affinity(motif, g, regions, False, _Args(no_reverse=no_reverse), weights=np.ones(L, dtype=np.uint64))
    most = int(max(ones.ref_rows.max(), ones.alt_rows.max()))
    fits = ((1 << 64) - 1) // most
    w = np.full(L, fits, dtype=np.uint64)
    va = compute_variant_affinity(motif, g, regions, False, _Args(no_reverse=no_reverse), weights=w)
    exp = _check(va, idx, regions, motif, no_reverse, weights=w)
    assert max(max(e[2], e[3]) for e in exp) > 1 << 63
    with pytest.raises(OverflowError, match="sum wrapped"):          # one more and the fullest slot wraps
        compute_variant_affinity(motif, g, regions, False, _Args(no_reverse=no_reverse),
                                 weights=np.full(L, ((1 << 64) - 1) // most + 1, dtype=np.uint64))
    g.close()


def test_walk_overflow_is_an_error():
    from grafimo_amd.extract_regions import GraphIndex
    from grafimo_amd.variant_affinity import compute_variant_affinity
    ref = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    pos = np.arange(20, 33, dtype=np.int32)          # 13 sites of 3 ALTs in one window of 19: 4^13 walks
    alt = np.array([[c for c in b"ACGT" if c != ref[q]] for q in pos], dtype=np.uint8)
    idx = GraphIndex("c", ref, pos, np.full(13, 3, np.uint8), alt, np.ones((13, 3, 1), np.uint64), 2)
    # (only windows that see all 13 sites: a window of exactly 4^12 = 2^24 walks would be replayed)
    with pytest.raises(OverflowError, match="more than 2\\^24 walks"):
        compute_variant_affinity(_motif(19), idx, [(14, 39)], False, _Args())


@pytest.fixture()
def mygenome(tmp_path, monkeypatch):
    import shutil
    g = tmp_path / "data" / "mygenome"
    shutil.copytree(os.path.join(GOLD, "mygenome"), g)     # (scan_graph saves x.gfmidx.npz beside x.xg)
    monkeypatch.setenv("GRAFIMO_INDEX_CACHE", str(tmp_path / "cache"))
    monkeypatch.delenv("GRAFIMO_SCAN_OUTPUT", raising=False)
    return str(g)


def test_manifest_route_equals_graph_route(tmp_path, mygenome, monkeypatch):
    import shutil
    from grafimo_amd.extract_regions import cached_host_index, read_manifest, scan_graph
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.variant_affinity import compute_variant_affinity
    from grafimo_amd.workflow import Findmotif
    wf = Findmotif(graph_genome_dir=mygenome, bedfile=os.path.join(GOLD, "regions.bed"), cores=2, threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "example.meme"), wf, 2, True, pvalue_matrix=False)[0]
    monkeypatch.setenv("GRAFIMO_SCAN_OUTPUT", "manifest")     # (this caller holds no compute_results to be recognised by)
    with contextlib.redirect_stdout(io.StringIO()):
        loc = scan_graph({motif.width}, wf, True)
    try:
        man = read_manifest(loc)
        assert man is not None
        a = compute_variant_affinity(motif, man, None, False, _Args())
        names = [e["chrom"] for e in man["entries"]]
        assert len(names) == 2 and list(dict.fromkeys(a.sequence_name.tolist())) == names      # entry order
        graphs = [cached_host_index(e["index"]) for e in man["entries"]]
        regs = [[tuple(int(v) for v in r) for r in e["regions"]] for e in man["entries"]]
        b = compute_variant_affinity(motif, graphs, regs, False, _Args(), chrom_names=names)
        assert len(a) > 0 and _arrays(a) == _arrays(b)
        pd.testing.assert_frame_equal(a.to_frame(), b.to_frame())
        for name, idx, rg in zip(names, graphs, regs):      # and each chromosome against the brute force
            part = compute_variant_affinity(motif, idx, rg, False, _Args())
            _check(part, idx, rg, motif, False)
            assert _arrays(part) == [r for r, n in zip(_arrays(a), a.sequence_name.tolist()) if n == name]
    finally:
        shutil.rmtree(loc, ignore_errors=True)


def test_cli_writes_table_and_leaves_report_alone(tmp_path):
    base = [sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", os.path.join(GOLD, "xy.fa"),
            "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed"), "-t", "0.05"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run(base + ["-o", a], check=True, cwd=str(tmp_path), env=env, timeout=600)
    r = subprocess.run(base + ["-o", b, "--variant-affinity", "--affinity-temperature", "2"], check=True, cwd=str(tmp_path), env=env,
                       timeout=600, capture_output=True, text=True)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fb == sorted(fa + ["grafimo_variant_affinity.tsv"])
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert "variant affinity rows written to" in r.stdout
    path = os.path.join(b, "grafimo_variant_affinity.tsv")
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    from grafimo_amd.variant_affinity import COLUMNS, compute_variant_affinity_many
    motif = _ctcf()
    bed = read_bed_regions(os.path.join(GOLD, "regions.bed"))
    graphs = [GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), c[3:]) for c in bed]
    va = compute_variant_affinity_many([motif], graphs, [bed[c] for c in bed], False, _Args(threshold=0.05), temperature=2.0)[0]
    assert len(va) > 0
    assert open(path).read() == va.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    pd.testing.assert_frame_equal(pd.read_csv(path, sep="\t"), va.to_frame(), check_dtype=False)
    r = subprocess.run(base + ["-o", str(tmp_path / "c"), "-f", "--variant-affinity", "--variant-affinity-delta", "0.25"],
                       check=True, cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    assert "\t".join(COLUMNS) + "\n" in r.stdout and not os.path.exists(tmp_path / "c" / "grafimo_variant_affinity.tsv")
    kept = compute_variant_affinity_many([motif], graphs, [bed[c] for c in bed], False, _Args(), min_abs_delta=0.25)[0]
    assert kept.to_frame().to_csv(sep="\t", index=False, lineterminator="\n") in r.stdout
