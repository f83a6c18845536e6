"""The mutation scan without a GPU: the key encoding, the effect codes and the filter, the summary's group-by, the frames of a
table whose arrays the brute force made (tests/mutation_scan_bruteforce.py), the command line's refusals, the export and the
header."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mutation_scan_bruteforce as bf  # noqa: E402
from extract_fuzz_core import SynMotif  # noqa: E402
from extract_helpers import motif_as_oracle_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "ref_data")
COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "version", "haplotypes", "haplotypes_g", "is_reference", "position", "inserted",
           "from", "to", "ref_score", "ref_pvalue", "ref_start", "ref_strand", "ref_kmer", "alt_score", "alt_pvalue", "alt_start",
           "alt_strand", "alt_kmer", "ref_log2_affinity", "alt_log2_affinity", "delta_log2_affinity", "effect"]
SUMMARY_COLUMNS = ["motif_id", "motif_alt_id", "sequence_name", "position", "from", "to", "versions", "haplotypes", "haplotypes_gain",
                   "haplotypes_loss", "min_delta_log2_affinity", "max_delta_log2_affinity", "best_alt_score"]


def _same(x, y):
    return x == y or (x != x and y != y)


def test_keys_decode_for_every_start_of_a_side():
    from grafimo_amd.query_variants import decode_keys
    for W in (1, 2, 19, 64):
        rel = np.arange(-(W - 1), 1)
        for plus in (0, 1):
            for score in (0, 7, 64_000):
                key = ((score + 1) << 8) | ((64 - rel) << 1) | plus
                assert key.max() < 1 << 25
                s, r, strand = decode_keys(key)
                assert s.tolist() == [score] * W and r.tolist() == rel.tolist() and set(strand) == {"+" if plus else "-"}
                assert [bf.key_of((score, int(q), "+" if plus else "-")) for q in rel] == key.tolist()
        # the order of the keys is the rule's: score descending, start ascending, + before -
        order = sorted([(5, -1, "+"), (5, -1, "-"), (5, 0, "+"), (6, 0, "-"), (4, -(W - 1), "+")], key=bf.key_of, reverse=True)
        assert order == [(6, 0, "-"), (5, -1, "+"), (5, -1, "-"), (5, 0, "+"), (4, -(W - 1), "+")]
    assert decode_keys(np.array([0]))[0].tolist() == [-1] and bf.key_of(None) == 0


def test_effect_codes_and_the_filter():
    from grafimo_amd.mutation_scan import effect_codes, keep_rows
    from grafimo_amd.query_variants import EFFECTS
    nan = np.nan
    ref_p = np.array([0.5, 0.5, 0.01, 0.01, 0.05, nan, 0.01, nan])
    alt_p = np.array([0.5, 0.01, 0.5, 0.01, 0.01, 0.01, nan, nan])
    codes = effect_codes(ref_p, alt_p, 0.05)
    # strict <: a p-value AT the threshold is no hit; a side without a window has none
    assert EFFECTS[codes].tolist() == ["none", "gain", "loss", "both", "gain", "gain", "loss", "none"]
    delta = np.array([3.0, 0.1, -0.1, -4.0, 0.0, nan, nan, nan])
    assert keep_rows(codes, delta, None, False).tolist() == [False, True, True, False, True, True, True, False]
    assert keep_rows(codes, delta, 3.0, False).tolist() == [True, True, True, True, True, True, True, False]
    assert keep_rows(codes, delta, 3.5, False).tolist() == [False, True, True, True, True, True, True, False]
    assert keep_rows(codes, delta, None, True).all() and keep_rows(codes[:0], delta[:0], 1.0, False).shape == (0,)


def test_summary_groups_against_a_loop():
    from grafimo_amd.mutation_scan import group_summary
    rng = np.random.default_rng(5)
    n = 400
    region, coord = rng.integers(0, 3, size=n), rng.integers(0, 6, size=n)
    frm, to = rng.integers(65, 69, size=n), rng.integers(1, 5, size=n)
    haps, codes = rng.integers(0, 9, size=n), rng.integers(0, 4, size=n)
    delta = np.where(rng.random(n) < 0.2, np.nan, rng.normal(size=n))
    best = rng.integers(-1, 500, size=n)
    first, versions, total, gain, loss, lo, hi, top = group_summary((region, coord, frm, to), haps, codes, delta, best)
    want = {}
    for k in range(n):
        d = want.setdefault((int(region[k]), int(coord[k]), int(frm[k]), int(to[k])), dict(v=0, h=0, g=0, l=0, d=[], b=[]))
        d["v"] += 1
        d["h"] += int(haps[k])
        d["g"] += int(haps[k]) if codes[k] == 1 else 0
        d["l"] += int(haps[k]) if codes[k] == 2 else 0
        d["b"].append(int(best[k]))
        if delta[k] == delta[k]:
            d["d"].append(float(delta[k]))
    keys = [(int(region[f]), int(coord[f]), int(frm[f]), int(to[f])) for f in first]
    assert keys == sorted(want) and len(set(keys)) == len(keys)
    for j, q in enumerate(keys):
        d = want[q]
        assert (versions[j], total[j], gain[j], loss[j], top[j]) == (d["v"], d["h"], d["g"], d["l"], max(d["b"])), q
        assert _same(lo[j], min(d["d"]) if d["d"] else np.nan) and _same(hi[j], max(d["d"]) if d["d"] else np.nan), q
    assert any(not d["d"] for d in want.values()) and any(d["v"] > 3 for d in want.values())
    assert [len(x) for x in group_summary((region[:0], coord[:0]), haps[:0], codes[:0], delta[:0], best[:0])] == [0] * 8


def _hand_table(W=3, threshold=0.5, fwd=False, **kw):
    """a MutationScan over query_variant_bruteforce.hand_graph's regions whose arrays the brute force made -> (the table, the
    brute force's rows of all_rows)"""
    from oracle import oracle as orc
    from grafimo_amd.haplotype_affinity import default_weights
    from grafimo_amd.mutation_scan import MutationScan
    idx = bf.hand_graph()
    regions = [(8, 14), (0, 20), (18, 20)]
    names = [f"c:{s}-{e}" for s, e in regions]
    m = SynMotif(W, seed=5)
    od = motif_as_oracle_dict(m)
    w, s_best = default_weights(m)
    log2_offset = -40 + (s_best / float(od["scale"]) + W * od["offset"])
    ptab = orc.p_table(od["pmf"])
    seqs = [bf.region_sequences(idx, s, e, [[1, 3]]) for s, e in regions]
    scans = [[bf.scan(d["bases"], W, od["score_matrix"], od["min_val"], w, fwd) for d in region] for region in seqs]
    flat = [(r, d, sc) for r, (region, rs) in enumerate(zip(seqs, scans)) for d, sc in zip(region, rs)]
    coord = [~p if t else p for _, d, _ in flat for p, t in d["coords"][0]]
    t = MutationScan("M", "m", W, od["scale"], od["offset"], ptab, log2_offset, threshold, names, ["g"], [r for r, _, _ in flat],
                     [d["version"] for _, d, _ in flat], [d["count"] for _, d, _ in flat], [d["group_counts"] for _, d, _ in flat],
                     [d["is_reference"] for _, d, _ in flat], np.concatenate([[0], np.cumsum([len(d["bases"]) for _, d, _ in flat])]),
                     np.frombuffer(b"".join(d["bases"] for _, d, _ in flat), dtype=np.uint8), coord,
                     np.array([[bf.key_of(b) for b, _ in row] for _, _, sc in flat for row in sc], dtype=np.uint32).reshape(-1, 5),
                     np.array([[s for _, s in row] for _, _, sc in flat for row in sc], dtype=np.uint64).reshape(-1, 5), **kw)
    rows = bf.detail_rows(names, seqs, scans, lambda r, d: d["coords"][0], W, od["scale"], od["offset"], ptab, log2_offset, threshold)
    return t, rows


@pytest.mark.parametrize("W,fwd", [(3, False), (2, True), (7, False)])
def test_frames_of_a_table_the_brute_force_filled(W, fwd):
    t, rows = _hand_table(W, fwd=fwd, all_rows=True)
    frame = t.to_frame()
    assert list(frame.columns) == COLUMNS
    assert len(frame) == len(rows) == 3 * len(t.bases) == len(t)
    for k, (f, e) in enumerate(zip(frame.to_dict("records"), rows)):
        assert [f["haplotypes_g"]] == e["groups"]
        for c in COLUMNS[2:5] + COLUMNS[6:]:
            assert _same(f[c], e[c]), (k, c, f[c], e[c])
    assert frame["inserted"].any() and frame["is_reference"].any() and not frame["is_reference"].all()
    effects = set(frame["effect"])
    assert W != 3 or {"gain", "loss"} <= effects, effects
    if W == 7:                                                                          # [18, 20) is shorter than W
        short = frame[frame["sequence_name"] == "c:18-20"]
        assert short["ref_score"].isna().all() and (short["ref_kmer"] == "").all() and (short["effect"] == "none").all()
    # ---- the filter
    t.all_rows = False
    kept = [e for e in rows if e["effect"] in ("gain", "loss")]
    assert [(f["sequence_name"], f["version"], f["position"], f["from"], f["to"]) for f in t.to_frame().to_dict("records")] == \
        [(e["sequence_name"], e["version"], e["position"], e["from"], e["to"]) for e in kept]
    t.delta = 0.75
    assert len(t.to_frame()) == len([e for e in rows if e["effect"] in ("gain", "loss") or abs(e["delta_log2_affinity"]) >= 0.75])
    # ---- the summary against a loop over the detail rows
    t.delta, t.all_rows = None, True
    want = bf.summary_of(frame.to_dict("records"))
    s = t.summary_frame()
    assert list(s.columns) == SUMMARY_COLUMNS and len(s) == len(want)
    for f in s.to_dict("records"):
        w = want[(f["sequence_name"], f["position"], f["from"], f["to"])]
        assert (f["versions"], f["haplotypes"], f["haplotypes_gain"], f["haplotypes_loss"]) == \
            (w["versions"], w["haplotypes"], w["haplotypes_gain"], w["haplotypes_loss"]), f
        assert _same(f["min_delta_log2_affinity"], min(w["deltas"]) if w["deltas"] else np.nan)
        assert _same(f["max_delta_log2_affinity"], max(w["deltas"]) if w["deltas"] else np.nan)
        assert _same(f["best_alt_score"], max(w["scores"]) if w["scores"] else np.nan)
    keys = [(f["sequence_name"], f["position"], f["from"], "ACGT".index(f["to"])) for f in s.to_dict("records")]
    assert keys == sorted(keys, key=lambda q: (t.region_names.tolist().index(q[0]),) + q[1:])
    t.all_rows = False
    assert len(t.summary_frame()) == sum(1 for w in want.values() if w["haplotypes_gain"] + w["haplotypes_loss"] > 0)
    # ---- the dense arrays draw the map: a sequence's delta per offset and to-base
    a, b = int(t.seq_offsets[0]), int(t.seq_offsets[1])
    heat = t.log2_affinity()[a:b, 1:] - t.log2_affinity()[a:b, :1]
    assert heat.shape == (b - a, 4)
    if W <= b - a:
        assert (np.nan_to_num(heat[np.arange(b - a), [b"ACGT".index(c) for c in t.bases[a:b].tobytes()]]) == 0).all()


def test_the_reference_row_where_no_haplotype_spells_it():
    """hand_graph's [8, 14) is spelled as the reference by haplotype 0 (no extra row); a graph where every haplotype carries the
    SNP has none: the brute force adds the count-0 row"""
    from grafimo_amd.extract_regions import GraphIndex
    seqs = bf.region_sequences(bf.hand_graph(), 8, 14)
    assert [d["version"] for d in seqs] == [0, 1, 2, 3] and [d["is_reference"] for d in seqs] == [True, False, False, False]
    bits = np.zeros((1, 3, 1), dtype=np.uint64)
    bits[0, 0, 0] = 0b11
    idx = GraphIndex("c", np.frombuffer(b"ACGTACGTAC", dtype=np.uint8), np.array([4], np.int32), np.array([1], np.uint8),
                     np.array([[ord("T"), 0, 0]], np.uint8), bits, 2)
    seqs = bf.region_sequences(idx, 2, 8)
    assert [(d["version"], d["count"], d["is_reference"], d["bases"]) for d in seqs] == [(0, 2, False, b"GTTCGT"), (-1, 0, True, b"GTACGT")]


def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, "-m", "grafimo_amd", "-m", os.path.join(GOLD, "MA0139.1.meme")] + list(flags),
                          capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)


def test_cli_refusals(tmp_path):
    r = _cli(tmp_path, "-s", str(tmp_path), "--mutation-scan")
    assert r.returncode != 0 and "--mutation-scan needs the graph" in r.stderr
    graph = ["-l", os.path.join(GOLD, "xy.fa"), "-v", os.path.join(GOLD, "xy2.vcf.gz"), "-b", os.path.join(GOLD, "regions.bed")]
    r = _cli(tmp_path, *graph, "--mutation-all")
    assert r.returncode != 0 and "--mutation-all goes with --mutation-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--mutation-delta", "1.5")
    assert r.returncode != 0 and "--mutation-delta goes with --mutation-scan" in r.stderr
    r = _cli(tmp_path, *graph, "--mutation-scan", "--mutation-delta", "-1")
    assert r.returncode != 0 and "--mutation-delta -1.0 is not >= 0" in r.stderr


def test_library_exports_the_entry_at_abi_12():
    from grafimo_amd import _native as nv
    assert nv.lib().gfm_abi_version() == nv.ABI_VERSION == 12
    name = "gfm_sequence_mutation_scan"
    assert name in nv.PROTOTYPES and hasattr(nv.lib(), name) and len(nv.PROTOTYPES[name][1]) == 12
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    assert f"int {name}(" in header
    # before a device is touched: no sequence is a no-op, an unknown flag and descending offsets are refused
    lib = nv.lib()
    assert lib.gfm_sequence_mutation_scan(None, 1, None, 1, 0, None, None, 0, None, None, None, None) == nv.GFM_OK
    assert lib.gfm_sequence_mutation_scan(None, 1, None, 1, 0, None, None, 2, None, None, None, None) == nv.GFM_ERR_INVALID
    off = np.array([0, 5, 3], dtype=np.int64)
    assert lib.gfm_sequence_mutation_scan(None, 1, None, 1, 2, off.ctypes.data, None, 0, None, None, None, None) == nv.GFM_ERR_INVALID
    assert b"descends" in lib.gfm_last_error()


def test_header_defines_the_tile_and_states_the_rule():
    import re
    from grafimo_amd import _native as nv
    from grafimo_amd import mutation_scan
    header = open(os.path.join(ROOT, "include", "grafimo_hip.h")).read()
    m = re.search(r"#define GFM_MUTSCAN_TILE (\d+)", header)
    assert m and int(m.group(1)) == nv.GFM_MUTSCAN_TILE and 1 <= nv.GFM_MUTSCAN_TILE
    squeeze = lambda s: " ".join(s.replace("*", " ").split())                   # noqa: E731
    texts = [squeeze(header), squeeze(mutation_scan.__doc__), squeeze(bf.__doc__)]
    for line in ("y = x with y[o] = b.",
                 "REF side: the window starts s of x with max(0, o - W + 1) <= s <= min(o, n - W).",
                 "ALT side: the same starts in y.",
                 "A window that holds a base that is not A/C/G/T scores min_val on both strands.",
                 "Case is folded, as base_code does.",
                 "((score + 1) << 8) | ((64 - (s - o)) << 1) | plus",
                 "b equal to the folded x[o] gives ALT equal to REF.",
                 "An x[o] that is no base has an all-min_val REF side, and each b can repair it."):
        for text in texts:
            assert line in text, line
