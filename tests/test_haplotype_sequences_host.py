"""Haplotype sequence table without a GPU: the base-set rule of the region sequence against the rows the report's region rule
admits (tests/variant_bruteforce.py spell), the host's grouping and numbering of versions, the table's assembly from spelled
pairs, the frame, the FASTA writer, the CLI's refusal and the library's exports."""
import io
import os
import subprocess
import sys
import zlib

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from graph_table_checks import random_bitset_index  # noqa: E402
from graph_tables_fuzz_core import make_regions  # noqa: E402
from haplotype_class_bruteforce import region_classes  # noqa: E402
from haplotype_sequence_bruteforce import check_versions, cut, region_sequence, region_versions, spelled  # noqa: E402
from haplotype_sequence_cases import chained_graph, edge_graph  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
ODD_H = (1, 3, 7, 63, 65)


def _windows(sp, W, S, E, L):
    """the rows of a spelled chromosome in the clipped region under the report's rule: {(start, stop, k-mer)}"""
    seq, coord, ins = sp
    S, E = max(S, 0), min(E, L)
    out = set()
    for o in range(len(seq) - W + 1):
        start, stop = int(coord[o]) + (1 if ins[o] else 0), int(coord[o + W - 1]) + 1
        if S <= start < E and stop <= E:
            out.add((start, stop, seq[o:o + W]))
    return out


def test_region_sequence_holds_exactly_the_rows_of_the_region_rule():
    rows = 0
    for seed in range(15):
        rng = np.random.default_rng(61_000 + seed)
        H = ODD_H[seed % len(ODD_H)]
        idx = random_bitset_index(H, 62_000 + seed, length=int(rng.integers(150, 360)), n_sites=int(rng.integers(4, 36)))
        L = len(idx.ref)
        regions = make_regions(rng, idx) + [(5, 5), (L - 1, L + 4), (-3, 1)]
        for h in list(range(min(H, 6))) + [-1]:
            sp = spelled(idx, h)
            for S, E in regions:
                seq, coord, ins = cut(sp, L, S, E)
                Ec = min(E, L)
                for W in (1, 8, 20):
                    admitted = _windows(sp, W, S, E, L)
                    mine = {}
                    for o in range(len(seq) - W + 1):
                        mine[(coord[o] + (1 if ins[o] else 0), coord[o + W - 1] + 1, seq[o:o + W])] = (coord[o], ins[o])
                    # every admitted row is a window of the region sequence ...
                    assert admitted <= set(mine), (seed, h, S, E, W)
                    # ... and every window is an admitted row, unless it starts on a base inserted behind E - 1
                    for row, (c, t) in mine.items():
                        assert row in admitted or (t and c == Ec - 1), (seed, h, S, E, W, row)
                    rows += len(admitted)
    assert rows > 20_000


def test_hand_made_graphs_spell_what_their_comments_say():
    idx, regions = chained_graph()
    # haplotype 0 carries A and B: B's anchor lies under A, B is not made; 1 carries B only: 90 .. 100 are gone
    ref = bytes(np.asarray(idx.ref))
    assert region_sequence(idx, 0, 90, 130)[0] == ref[90:121] + b"GG" + ref[121:130]
    assert region_sequence(idx, 1, 90, 130)[0] == ref[101:130] and region_sequence(idx, 2, 90, 130)[0] == ref[90:130]
    assert region_sequence(idx, 1, 95, 100) == (b"", [], [])
    idx, regions, merging = edge_graph()
    assert len(idx.ref) == 1400 and int(idx.n_haplotypes) == 3
    for r in merging:                                        # alleles differ, bases do not
        assert len(region_versions(idx, *regions[r])["count"]) < len(region_classes(idx, *regions[r])["count"])
    at = regions.index((800, 810))                           # wholly under haplotype 2's deletion: nothing; the insertion is jumped
    assert region_sequence(idx, 2, *regions[at])[0] == b"" and len(region_sequence(idx, 0, *regions[at])[0]) == 15
    assert region_sequence(idx, 0, 500, 520)[2][:3] == [True] * 3 and region_sequence(idx, 0, 500, 520)[1][:4] == [499] * 3 + [500]
    assert region_sequence(idx, 1, 500, 520)[1][-6:] == [519] * 6 and region_sequence(idx, 1, 500, 520)[2][-6:] == [False] + [True] * 5


def test_grouping_and_numbering_by_hand():
    from grafimo_amd.haplotype_sequences import group_by_key, number_versions
    #        item:   0   1   2   3   4   5   6   7    8 (the reference of region 0)   9  10 (reference of region 1)
    region = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1])
    length = np.array([5, 5, 5, 6, 5, 7, 7, 9, 5, 5, 5])
    key = np.array([11, 12, 11, 11, 12, 40, 41, 2 ** 64 - 1, 12, 11, 13], dtype=np.uint64)
    count = np.array([2, 3, 1, 3, 0, 4, 4, 1, 0, 6, 0])
    first = np.array([4, 0, 9, 1, 2 ** 31 - 1, 7, 3, 30, 2 ** 31 - 1, 0, 2 ** 31 - 1])
    same = group_by_key(region, length, key)
    # equal keys of different lengths (0 and 3) stay apart; equal (length, key) in another region (9) stays apart
    assert same.dtype == np.int32 and same.tolist() == [0, 1, 0, 3, 1, 5, 6, 7, 1, 9, 10]
    version, n_versions, head, v_count, v_first = number_versions(same, region, count, first, 3)
    # region 0: {5, 6} tie at 4 -> the smaller first (item 6) first; then {0, 2} = 3 first 4, {1, 4, 8} = 3 first 0, {3} = 3 first 1
    assert n_versions.tolist() == [6, 1, 0] and head.tolist() == [6, 5, 1, 3, 0, 7, 9]
    assert v_count.tolist() == [4, 4, 3, 3, 3, 1, 6] and v_first.tolist() == [3, 7, 0, 1, 4, 30, 0]
    assert version.tolist() == [4, 2, 4, 3, 2, 1, 0, 5, 2, 0, -1]     # (the reference of region 1 equals no haplotype: no version)
    assert group_by_key(region[:0], length[:0], key[:0]).tolist() == []
    version, n_versions, head, _, _ = number_versions(np.zeros(0, np.int32), region[:0], count[:0], first[:0], 2)
    assert version.tolist() == [] and n_versions.tolist() == [0, 0] and head.tolist() == []


def _host_sequences(idx, regions, groups=None, coordinates=False):
    """a HaplotypeSequences made on the host: the classes from the class brute force, the pairs spelled by the sequence brute
    force, keyed by a checksum, grouped and assembled by the module's own host code"""
    from grafimo_amd.haplotype_classes import HaplotypeClasses
    from grafimo_amd.haplotype_sequences import _assemble, group_by_key
    groups = groups or {}
    per = [region_classes(idx, S, E, groups=list(groups.values())) for S, E in regions]
    H = int(idx.n_haplotypes)
    n = np.array([len(p["count"]) for p in per])
    hc = HaplotypeClasses([f"c:{S}-{E}" for S, E in regions], [f"hap{k}" for k in range(H)], np.stack([p["class_of"] for p in per]),
                          n, np.concatenate([[0], np.cumsum(n)]), np.concatenate([p["count"] for p in per]),
                          np.concatenate([p["first"] for p in per]), list(groups),
                          np.concatenate([p["group_counts"] for p in per]), [idx], np.zeros(len(regions), np.int64), regions)
    pair_class, pair_region, seqs, coords = [], [], [], []
    for r, (S, E) in enumerate(regions):
        for k in list(range(int(n[r]))) + [-1]:
            h = -1 if k < 0 else int(hc.first[hc.offsets[r] + k])
            s, c, t = region_sequence(idx, h, S, E)
            pair_class.append(-1 if k < 0 else int(hc.offsets[r]) + k), pair_region.append(r), seqs.append(s)
            coords.append(np.array([~x if i else x for x, i in zip(c, t)], dtype=np.int32))
    lengths = np.array([len(s) for s in seqs], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths)])[:-1].astype(np.int64)
    keys = np.array([zlib.crc32(s) for s in seqs], dtype=np.uint64)
    same = group_by_key(np.array(pair_region), lengths, keys)
    for a, b in enumerate(same.tolist()):
        assert seqs[a] == seqs[b]                            # (what the device verifies)
    return _assemble(hc, np.array(pair_class, dtype=np.int64), np.array(pair_region, dtype=np.int64), lengths, offsets,
                     np.frombuffer(b"".join(seqs), dtype=np.uint8), np.concatenate(coords) if coordinates else None,
                     same.astype(np.int64))


def test_assembly_equals_the_brute_force():
    groups = {"a": [0, 1], "b": [2], "none": []}
    idx, regions, merging = edge_graph()
    regions = regions[::9] + regions[-14:]
    hs = _host_sequences(idx, regions, groups, coordinates=True)
    check_versions(hs, [region_versions(idx, S, E, groups=list(groups.values())) for S, E in regions])
    assert (hs.n_versions < hs.classes.n_classes).sum() >= 2 and hs.group_names == list(groups)
    for r, (S, E) in enumerate(regions):
        for k in range(int(hs.n_versions[r])):
            c, t = hs.coordinates(r, k)
            _, ec, et = region_sequence(idx, int(hs.first[hs.offsets[r] + k]), S, E)
            assert c.tolist() == ec and t.tolist() == et
    rng = np.random.default_rng(9)
    idx = random_bitset_index(65, 93, length=240, n_sites=30)
    regions = make_regions(rng, idx) + [(10, 10), (0, 240)]
    hs = _host_sequences(idx, regions)
    check_versions(hs, [region_versions(idx, S, E) for S, E in regions])
    with pytest.raises(ValueError, match="without coordinates"):
        hs.coordinates(0, 0)
    with pytest.raises(IndexError):
        hs.sequence(0, int(hs.n_versions[0]))


def test_the_pairs_a_graph_spells():
    from grafimo_amd.haplotype_sequences import _class_pairs
    idx, regions, _ = edge_graph()
    hs = _host_sequences(idx, [(890, 910), (300, 300), (940, 970), (100, 140)])
    hc = hs.classes
    assert hc.n_classes.tolist() == [3, 1, 3, 3]
    # a graph that holds the caller's rows 2 and 0, in this order
    region, hap, pair_class, pair_region = _class_pairs(hc, [2, 0])
    assert region.dtype == hap.dtype == np.int32 and region.tolist() == [0] * 4 + [1] * 4
    assert hap.tolist() == hc.first[4:7].tolist() + [-1] + hc.first[0:3].tolist() + [-1]
    assert pair_class.tolist() == [4, 5, 6, -1, 0, 1, 2, -1] and pair_region.tolist() == [2] * 4 + [0] * 4
    assert [len(x) for x in _class_pairs(hc, [])] == [0] * 4


def test_frame_and_fasta_writer(tmp_path):
    from grafimo_amd.haplotype_sequences import (haplotype_sequence_paths, write_haplotype_sequence_versions,
                                                 write_haplotype_sequences_fasta)
    idx, regions, merging = edge_graph()
    names = [(890, 910), (940, 970), (800, 810), (300, 300), (395, 405)]
    hs = _host_sequences(idx, names, {"g": [0, 2]})
    f = hs.to_frame()
    assert list(f.columns) == ["sequence_name", "version", "haplotypes", "frequency", "haplotypes_g", "representative",
                               "is_reference", "length", "classes", "alt_alleles"]
    # (890, 910): haplotypes 0 (both insertions) and 1 (the first) spell AC behind 900, haplotype 2 GGT
    assert f["sequence_name"].tolist()[:2] == ["c:890-910"] * 2 and f["version"].tolist()[:4] == [0, 1, 0, 1]
    assert f["haplotypes"].tolist()[:2] == [2, 1] and f["representative"].tolist()[:2] == ["hap0", "hap2"]
    assert f["frequency"].tolist()[:2] == [2 / 3, 1 / 3] and f["haplotypes_g"].tolist()[:2] == [1, 1]
    assert f["classes"].tolist()[:2] == ["0;1", "2"] and f["length"].tolist()[:2] == [22, 23]
    assert f["alt_alleles"].tolist()[:2] == [f"901:{chr(idx.ref[900])}>{chr(idx.ref[900])}AC;901:{chr(idx.ref[900])}>{chr(idx.ref[900])}GGT",
                                             f"901:{chr(idx.ref[900])}>{chr(idx.ref[900])}GGT"]
    assert not f["is_reference"].tolist()[0] and f["is_reference"].dtype == bool and f["version"].dtype == np.int64
    empty = f[f["sequence_name"] == "c:300-300"]
    assert empty["length"].tolist() == [0] and empty["haplotypes"].tolist() == [3] and empty["is_reference"].tolist() == [True]
    assert 0 in f[f["sequence_name"] == "c:800-810"]["length"].tolist()
    for width in (60, 7):
        buf = io.StringIO()
        write_haplotype_sequences_fasta(hs, buf, width=width)
        lines = buf.getvalue().split("\n")
        assert lines[-1] == ""
        heads = [k for k, ln in enumerate(lines[:-1]) if ln.startswith(">")]
        assert len(heads) == len(hs)
        for v, k in enumerate(heads):
            r = int(hs.version_region[v])
            assert lines[k] == (f">{f['sequence_name'][v]}|v{f['version'][v]} haplotypes={f['haplotypes'][v]} "
                                f"representative={f['representative'][v]} alt_alleles={f['alt_alleles'][v]}")
            body = lines[k + 1:(heads[v + 1] if v + 1 < len(heads) else len(lines) - 1)]
            seq = hs.sequence(r, int(f["version"][v]))
            assert "".join(body).encode() == seq
            assert all(len(b) == width for b in body[:-1]) and all(0 < len(b) <= width for b in body[-1:])
            assert len(body) == (len(seq) + width - 1) // width          # (an empty sequence: a header and no line)
    assert any(len(hs.sequence(int(hs.version_region[v]), int(f["version"][v]))) > 60 for v in range(len(hs)))

    class _Out:
        outdir = str(tmp_path / "o")

    fasta, tsv = haplotype_sequence_paths(_Out())
    assert (os.path.basename(fasta), os.path.basename(tsv)) == ("grafimo_haplotype_sequences.fa",
                                                                "grafimo_haplotype_sequence_versions.tsv")
    assert os.path.dirname(fasta) == os.path.dirname(tsv) == _Out.outdir
    assert write_haplotype_sequences_fasta(hs, fasta, width=7) == fasta and open(fasta).read() == buf.getvalue()
    assert write_haplotype_sequence_versions(hs, tsv) == tsv
    assert open(tsv, "rb").read() == f.to_csv(sep="\t", index=False, lineterminator="\n").encode()
    back = pd.read_csv(tsv, sep="\t", keep_default_na=False, dtype={"alt_alleles": str, "classes": str})
    assert back["classes"].tolist() == f["classes"].tolist()
    with pytest.raises(ValueError, match="width"):
        write_haplotype_sequences_fasta(hs, io.StringIO(), width=0)


def test_cli_refuses_the_rows_of_s(tmp_path):
    r = subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme"), "-s", str(tmp_path),
                        "--haplotype-sequences"], capture_output=True, text=True, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert r.returncode != 0 and "--haplotype-sequences needs the graph" in r.stderr


def test_library_exports_both_entries_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    for name, n_args in (("gfm_graph_haplotype_sequences", 18), ("gfm_sequences_verify", 6)):
        assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == n_args
        assert f"int {name}(" in header
    assert "#define GFM_SEQS_HAVE_LENGTHS 1u" in header and nv.GFM_SEQS_HAVE_LENGTHS == 1
    assert nv.lib().gfm_graph_haplotype_sequences(None, 0, None, None, 0, None, None, None, None, 0, None, None, 0, 64, None, 0, None,
                                                  None) == nv.GFM_ERR_INVALID
    assert nv.lib().gfm_sequences_verify(-1, None, None, None, None, None) == nv.GFM_ERR_INVALID
    assert nv.lib().gfm_sequences_verify(1, None, None, None, None, None) == nv.GFM_ERR_INVALID
