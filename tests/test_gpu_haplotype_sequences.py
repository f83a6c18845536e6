"""The haplotype sequence table on the GPU against the brute force (tests/haplotype_sequence_bruteforce.py): a fuzz over the
class table's graphs and regions, a hand-made graph of every alignment and edge of the region rule, chained deletions upstream
of a region, merging classes, cohort-size panels, the verification under truncated keys, the refusals, the call forms and the
command line."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_panel_cases as wp  # noqa: E402
from extract_fuzz_core import KINDS  # noqa: E402
from graph_table_checks import random_bitset_index  # noqa: E402
from graph_tables_fuzz_core import ODD_H, Args, make_graph, make_regions  # noqa: E402
from haplotype_class_bruteforce import region_classes  # noqa: E402
from haplotype_sequence_bruteforce import check_versions, content_key, region_sequence, region_versions  # noqa: E402
from haplotype_sequence_cases import LONG_INS, chained_graph, edge_graph  # noqa: E402
from variant_bruteforce import haplotype_classes  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
SEEDS = list(range(21)) + [21, 24]                           # (test_gpu_haplotype_classes.py: every kind string occurs)


@pytest.fixture(scope="module")
def fuzz_graphs(tmp_path_factory):
    """[(what, GraphIndex, regions)]: the class table's fuzz graphs -- the seeds' graphs, then a bitset graph of every odd
    haplotype count"""
    tmp = tmp_path_factory.mktemp("sequences")
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(70_000 + seed)
        d = tmp / f"g{seed}"
        d.mkdir()
        idx, what = make_graph(seed, rng, str(d))
        out.append((f"seed {seed}: {what}", idx, make_regions(rng, idx)))
    for k, H in enumerate(ODD_H):
        rng = np.random.default_rng(71_000 + k)
        idx = random_bitset_index(H, 81_000 + k, length=int(rng.integers(150, 360)), n_sites=int(rng.integers(4, 36)))
        out.append((f"bits H={H}", idx, make_regions(rng, idx)))
    kinds = {w.split()[3] for w, _, _ in out if " vcf " in w}
    assert kinds == set(KINDS), sorted(set(KINDS) - kinds)
    return out


def _groups(H, rng):
    g = {f"g{k}": sorted(rng.choice(H, size=int(rng.integers(0, H + 1)), replace=False).tolist()) for k in range(2)}
    g["none"], g["all"] = [], list(range(H))
    return g


def _check_spelled(got, idx, regions, pairs, cache, ctx, seed=0, key_bits=64):
    """spell_rows' result over `pairs` [(region, haplotype)] against the brute force: lengths, offsets, bases, coordinates,
    inserted flags and keys"""
    lengths, offsets, bases, coord, keys = got
    assert lengths.dtype == np.int32 and offsets.dtype == np.int64 and bases.dtype == np.uint8 and keys.dtype == np.uint64
    assert len(lengths) == len(pairs) == len(keys) and len(offsets) == len(pairs) + 1
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(lengths.astype(np.int64))])) and len(bases) == offsets[-1]
    for n, (r, h) in enumerate(pairs):
        seq, c, ins = region_sequence(idx, h, *regions[r], cache)
        a, b = int(offsets[n]), int(offsets[n + 1])
        assert bases[a:b].tobytes() == seq, (ctx, regions[r], h, bases[a:b].tobytes(), seq)
        if coord is not None:
            assert coord[a:b].tolist() == [~x if t else x for x, t in zip(c, ins)], (ctx, regions[r], h)
        assert int(keys[n]) == content_key(seq, seed, key_bits), (ctx, regions[r], h)


def test_fuzz_against_the_brute_force(fuzz_graphs):
    """merging -- a region with fewer versions than classes -- is covered HERE (asserted below: the seeds' graphs hold such a
    region) and again by the hand-made graphs of test_chained_deletions_upstream_and_merging"""
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences, spell_rows
    versions = n_regions = merged = 0
    for k, (what, idx, regions) in enumerate(fuzz_graphs):
        H = int(idx.n_haplotypes)
        groups = _groups(H, np.random.default_rng(73_000 + k))
        cache = {}
        exp = [region_versions(idx, S, E, groups=list(groups.values()), classes=haplotype_classes(idx), cache=cache) for S, E in regions]
        starts, stops = [S for S, _ in regions], [E for _, E in regions]
        g = DeviceGraph(idx)
        try:
            if H <= 130:
                pairs = [(r, h) for r in range(len(regions)) for h in list(range(H)) + [-1]]
                for again in range(2):                       # (again on the same handle: the scratch is reused)
                    got = spell_rows(g, starts, stops, [p[0] for p in pairs], [p[1] for p in pairs], coordinates=True, seed=again)
                    _check_spelled(got, idx, regions, pairs, cache, (what, again), seed=again)
            for again in range(2):
                hs = compute_haplotype_sequences(g, regions, False, Args(), haplotype_groups=groups, seed=k + again,
                                                 coordinates=bool(again))
                check_versions(hs, exp, (what, regions, again))
                assert hs.group_names == list(groups) and hs.version_of.shape == (len(regions), H)
        finally:
            g.close()
        versions += len(hs)
        n_regions += len(regions)
        merged += int((hs.n_versions < hs.classes.n_classes).sum())
    assert versions > n_regions and merged >= 1, (versions, n_regions, merged)


def test_alignment_and_edges():
    """one call over the hand-made graph: every residue of output offset and source position, several strides, an insertion
    longer than a wavefront, the edges of the region rule"""
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences, spell_rows
    idx, regions, _ = edge_graph()
    pairs = [(r, h) for r in range(len(regions)) for h in (0, 1, 2, -1)]
    cache = {}
    starts, stops = [S for S, _ in regions], [E for _, E in regions]
    got = spell_rows(idx, starts, stops, [p[0] for p in pairs], [p[1] for p in pairs], coordinates=True, seed=3)
    _check_spelled(got, idx, regions, pairs, cache, "edges", seed=3)
    lengths, offsets = got[0], got[1]
    assert {0, 1, 2, 3} <= set(lengths.tolist()) and lengths.max() > 256
    assert {int(o) % 16 for o in offsets[:-1]} == set(range(16))                   # (every alignment of the output)
    short = regions.index((395, 405))
    assert lengths[4 * short] == 10 + LONG_INS and lengths[4 * short + 2] == 10    # (the region is shorter than its insertion)
    # the pairs in another order and without coordinates: other offsets, the same sequences
    back = pairs[::-1][::3]
    got = spell_rows(idx, starts, stops, [p[0] for p in back], [p[1] for p in back])
    assert got[3] is None
    _check_spelled(got, idx, regions, back, cache, "edges, reversed")
    hs = compute_haplotype_sequences(idx, regions, False, Args())
    check_versions(hs, [region_versions(idx, S, E, cache=cache) for S, E in regions], "edges")


def test_chained_deletions_upstream_and_merging():
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences, spell_rows
    idx, regions = chained_graph()
    pairs = [(r, h) for r in range(len(regions)) for h in (0, 1, 2, 3, -1)]
    cache = {}
    got = spell_rows(idx, [S for S, _ in regions], [E for _, E in regions], [p[0] for p in pairs], [p[1] for p in pairs],
                     coordinates=True)
    _check_spelled(got, idx, regions, pairs, cache, "chained")
    assert got[0][:4].tolist() == [42, 29, 40, 40]           # (A and B: B is not made; B only: 90 .. 100 are gone)
    # (the VERSIONS of this graph are not compared: they are made of the class table's classes, whose sites T(r) hold B but not
    # A -- haplotypes 0 and 1 are one class of (95, 100) and spell differently; the class table's rule is not this table's to change)
    idx, regions, merging = edge_graph()
    regions = [regions[r] for r in merging]
    hs = compute_haplotype_sequences(idx, regions, False, Args(), haplotype_groups={"a": [0], "b": [1, 2]})
    assert (hs.n_versions < hs.classes.n_classes).all() and hs.n_versions.tolist() == [2, 2]
    check_versions(hs, [region_versions(idx, S, E, groups=[[0], [1, 2]]) for S, E in regions], "merging")
    assert [c.tolist() for c in (hs.classes_of(0, 0), hs.classes_of(0, 1))] == [[0, 1], [2]]


def _wide(idx, regions, groups):
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences
    cls = haplotype_classes(idx)
    cache = {}
    exp = [region_versions(idx, S, E, groups=list(groups.values()), classes=cls, cache=cache) for S, E in regions]
    hs = compute_haplotype_sequences(idx, regions, False, wp.Args(), haplotype_groups=groups)
    check_versions(hs, exp, int(idx.n_haplotypes))
    return hs


def test_wide_panels():
    """carrier words beyond index 64: 4 200 haplotypes, and the 5 096-haplotype panel"""
    H = 4200
    hs = _wide(random_bitset_index(H, 4401, length=220, n_sites=16, chrom="a"), [(0, 220), (50, 120), (90, 90)],
               dict(wp.groups(H), late=list(range(64 * 64 + 3, H))))
    assert hs.n_versions[2] == 1 and hs.count[hs.offsets[2]] == H and hs.first.max() >= 64 * 64
    H, seed, _, regions = wp.CASES[4]
    assert H == 5096
    hs = _wide(wp.graph(H, seed), list(regions), wp.groups(H))
    assert hs.n_versions.max() > 1000


def test_truncated_keys_are_caught_never_silently_wrong():
    from grafimo_amd.extract_regions import DeviceGraph
    from grafimo_amd.grafimo_errors import HashCollisionError
    from grafimo_amd.haplotype_sequences import SEEDS_TRIED, compute_haplotype_sequences
    H, seed, _, regions = wp.CASES[1]                        # 1 025 haplotypes
    idx = wp.graph(H, seed)
    regions = list(regions)
    cls, cache = haplotype_classes(idx), {}
    exp = [region_versions(idx, S, E, classes=cls, cache=cache) for S, E in regions]
    assert all(len(e["count"]) > 8 for e in exp)

    def collides(r, s, bits):
        """the brute force's verdict: two different sequences of region r (the reference's among them) share (length, key)"""
        seqs = set(exp[r]["sequences"]) | {region_sequence(idx, -1, *regions[r], cache)[0]}
        return len({(len(q), content_key(q, s, bits)) for q in seqs}) < len(seqs)

    g = DeviceGraph(idx)
    try:
        hc = None
        for r in range(len(regions)):                        # more than 8 sequences under 8 keys: two of one length share one?
            assert all(collides(r, s, 3) for s in range(5, 5 + SEEDS_TRIED))
            with pytest.raises(HashCollisionError, match="seeds 5 .. 7"):
                compute_haplotype_sequences(g, regions[r:r + 1], False, wp.Args(), seed=5, key_bits=3)
        caught = clean = 0
        for bits in (8, 16):
            for s in range(8):
                for r in (2, 3):
                    foretold = all(collides(r, s + a, bits) for a in range(SEEDS_TRIED))
                    try:
                        hs = compute_haplotype_sequences(g, regions[r:r + 1], False, wp.Args(), seed=s, key_bits=bits)
                    except HashCollisionError:
                        caught += 1
                        assert foretold, (bits, s, r)
                        continue
                    clean += 1
                    assert not foretold, (bits, s, r)
                    check_versions(hs, exp[r:r + 1], (bits, s, r))
        assert caught > 0 and clean > 0, (caught, clean)
        # the same handle afterwards: exact again
        check_versions(compute_haplotype_sequences(g, regions, False, wp.Args(), classes=hc), exp)
    finally:
        g.close()


def test_refusals():
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences, spell_rows
    idx = random_bitset_index(7, 31, length=150, n_sites=10)
    g = DeviceGraph(idx)
    try:
        with pytest.raises(Exception, match="out of range"):
            spell_rows(g, [0], [100], [0], [7])              # haplotype >= H
        with pytest.raises(Exception, match="out of range"):
            spell_rows(g, [0], [100], [0], [-2])
        with pytest.raises(Exception, match="out of range"):
            spell_rows(g, [0], [100], [1], [0])              # region index
        with pytest.raises(Exception, match="ends before it starts"):
            spell_rows(g, [10], [5], [0], [0])
        with pytest.raises(Exception, match="key_bits"):
            spell_rows(g, [0], [100], [0], [0], key_bits=65)
        spelt = region_classes(idx, 0, 100)["first"].tolist() + [-1]       # (the classes' representatives and the reference)
        need = sum(len(region_sequence(idx, h, 0, 100)[0]) for h in spelt)
        with pytest.raises(ValueError, match=f"hold {need} bases"):
            compute_haplotype_sequences(g, [(0, 100)], False, Args(), max_bytes=need - 1)
        assert len(compute_haplotype_sequences(g, [(0, 100)], False, Args(), max_bytes=need)) >= 1
        total = sum(len(region_sequence(idx, h, 0, 100)[0]) for h in (0, 6, -1))
        got = spell_rows(g, [0], [100], [0, 0, 0], [0, 6, -1])         # the handle afterwards: exact
        assert int(got[1][-1]) == total
        _check_spelled(got, idx, [(0, 100)], [(0, 0), (0, 6), (0, -1)], {}, "after the refusals")
        assert [len(x) for x in spell_rows(g, [0], [100], [], [])[:3]] == [0, 1, 0]
    finally:
        g.close()
    ref = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    bare = GraphIndex("c", ref, np.array([10], np.int32), np.array([1], np.uint8), np.array([[ord("A"), 0, 0]], np.uint8), None, 0)
    with pytest.raises(ValueError, match="carries no haplotypes"):
        compute_haplotype_sequences(bare, [(0, 100)], False, Args())
    with pytest.raises(Exception, match="carries no haplotypes"):
        spell_rows(bare, [0], [100], [0], [0])
    got = spell_rows(bare, [0, 90], [100, 200], [0, 1], [-1, -1], coordinates=True)    # the reference alone still works
    assert got[2].tobytes() == ref.tobytes() + ref.tobytes()[90:] and got[3].tolist() == list(range(100)) + list(range(90, 100))


def test_call_forms():
    from grafimo_amd.haplotype_classes import compute_haplotype_classes
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences
    H = 130
    a = random_bitset_index(H, 4501, length=220, n_sites=24, chrom="a")
    b = random_bitset_index(H, 4502, length=180, n_sites=18, chrom="b")
    ra, rb = [(0, 220), (50, 120), (90, 90)], [(-5, 60), (30, 180)]
    names = [f"n{k}" for k in range(H)]
    groups = {"x": ["n0", "n129", 7], "y": list(range(64, 130))}
    members = [[0, 129, 7], list(range(64, 130))]
    hs = compute_haplotype_sequences([a, b], [ra, rb], False, Args(), chrom_names=["a", "b"], haplotype_names=names,
                                     haplotype_groups=groups)
    exp = [region_versions(a, S, E, groups=members) for S, E in ra] + [region_versions(b, S, E, groups=members) for S, E in rb]
    check_versions(hs, exp)
    assert hs.haplotype_names == names and hs.group_names == ["x", "y"] and len(hs.region_names) == 5
    assert all(n.startswith("a:") for n in hs.region_names[:3]) and hs.n_versions[2] == 1 and hs.length[hs.offsets[2]] == 0
    # entries that share one graph: rows in the caller's entry order; the classes handed in
    forms = ([a, b, a], [[ra[1]], rb, [ra[0]]])
    hc = compute_haplotype_classes(*forms, False, Args(), chrom_names=["a", "b", "a"], haplotype_names=names, haplotype_groups=groups)
    split = compute_haplotype_sequences(*forms, False, Args(), chrom_names=["a", "b", "a"], classes=hc, coordinates=True)
    check_versions(split, [exp[r] for r in (1, 3, 4, 0)])
    assert split.classes is hc and split.coord is not None and len(split.coord) == len(split.bases)
    assert list(split.to_frame().columns)[:6] == ["sequence_name", "version", "haplotypes", "frequency", "haplotypes_x", "haplotypes_y"]


def test_manifest_route_equals_fasta_vcf_route(tmp_path, monkeypatch):
    import shutil
    from grafimo_amd.extract_regions import DeviceGraph, GraphIndex, read_bed_regions, read_manifest, scan_graph
    from grafimo_amd.haplotype_sequences import compute_haplotype_sequences
    from grafimo_amd.motif_ops import get_motif_pwm
    from grafimo_amd.workflow import Findmotif
    genome = tmp_path / "data" / "mygenome"
    shutil.copytree(os.path.join(GOLD, "mygenome"), genome)     # (scan_graph saves x.gfmidx.npz beside x.xg)
    monkeypatch.setenv("GRAFIMO_INDEX_CACHE", str(tmp_path / "cache"))
    bed = os.path.join(tmp_path, "x.bed")
    with open(os.path.join(GOLD, "regions.bed")) as src, open(bed, "w") as dst:
        dst.writelines(line for line in src if line.startswith("chrx\t"))
    wf = Findmotif(graph_genome_dir=str(genome), bedfile=bed, cores=2, threshold=0.05)
    motif = get_motif_pwm(os.path.join(GOLD, "example.meme"), wf, 2, True, pvalue_matrix=False)[0]
    monkeypatch.setenv("GRAFIMO_SCAN_OUTPUT", "manifest")
    with contextlib.redirect_stdout(io.StringIO()):
        loc = scan_graph({motif.width}, wf, True)
    try:
        man = read_manifest(loc)
        assert man is not None
        a = compute_haplotype_sequences(man, None, False, wp.Args())
        idx = GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), "x")
        regions = read_bed_regions(bed)["chrx"]
        b = compute_haplotype_sequences(DeviceGraph(idx), regions, False, wp.Args())
        assert a.haplotype_names == ["hap0", "hap1"] and b.haplotype_names == ["1|1", "1|2"]
        assert a.region_names.tolist() == b.region_names.tolist()
        for name in ("version_of_class", "version_of", "n_versions", "offsets", "count", "first", "length", "is_reference",
                     "seq_offsets", "bases"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        check_versions(b, [region_versions(idx, S, E) for S, E in regions])
        assert (b.n_versions == 2).any()
    finally:
        shutil.rmtree(loc, ignore_errors=True)


def test_cli_writes_both_files_and_leaves_the_report_alone(tmp_path):
    base = [sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-l", os.path.join(GOLD, "xy.fa"),
            "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed"), "-t", "0.05"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run(base + ["-o", a], check=True, cwd=str(tmp_path), env=env, timeout=600)
    r = subprocess.run(base + ["-o", b, "--haplotype-sequences"], check=True, cwd=str(tmp_path), env=env, timeout=600,
                       capture_output=True, text=True)
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fb == sorted(fa + ["grafimo_haplotype_sequences.fa", "grafimo_haplotype_sequence_versions.tsv"])
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert "haplotype sequences written to" in r.stdout and "haplotype sequence versions written to" in r.stdout
    from grafimo_amd.extract_regions import GraphIndex, read_bed_regions
    from grafimo_amd.haplotype_sequences import (compute_haplotype_sequences, write_haplotype_sequence_versions,
                                                 write_haplotype_sequences_fasta)
    bed = read_bed_regions(os.path.join(GOLD, "regions.bed"))
    graphs = [GraphIndex.from_fasta_vcf(os.path.join(GOLD, "xy.fa"), os.path.join(GOLD, "xy2.vcf.gz"), c[3:]) for c in bed]
    hs = compute_haplotype_sequences(graphs, [bed[c] for c in bed], False, wp.Args(threshold=0.05))
    assert (hs.n_versions == 2).any()
    text = io.StringIO()
    write_haplotype_sequences_fasta(hs, text)
    assert open(os.path.join(b, "grafimo_haplotype_sequences.fa")).read() == text.getvalue()
    text = io.StringIO()
    write_haplotype_sequence_versions(hs, text)
    assert open(os.path.join(b, "grafimo_haplotype_sequence_versions.tsv")).read() == text.getvalue()
    assert text.getvalue() == hs.to_frame().to_csv(sep="\t", index=False, lineterminator="\n")
    r = subprocess.run(base + ["-o", str(tmp_path / "c"), "-f", "--haplotype-sequences"], check=True, cwd=str(tmp_path), env=env,
                       timeout=600, capture_output=True, text=True)
    assert "\t".join(hs.to_frame().columns) + "\n" in r.stdout
    assert not os.path.exists(tmp_path / "c" / "grafimo_haplotype_sequences.fa")
    assert not os.path.exists(tmp_path / "c" / "grafimo_haplotype_sequence_versions.tsv")
    r = subprocess.run(base[:5] + ["-s", str(tmp_path), "--haplotype-sequences"], cwd=str(tmp_path), env=env, timeout=600,
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--haplotype-sequences needs the graph" in r.stderr
