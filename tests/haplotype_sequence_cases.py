"""Hand-made graphs for the haplotype sequence tests -- TEST INFRASTRUCTURE ONLY (numpy and GraphIndex, no GPU)."""
import numpy as np


def _index(chrom, ref, sites, H):
    """sites: [(pos, kind, payload, carriers)] in site order -- kind "snv": payload the ALT bases (one string of 1 .. 3), carriers a
    list per ALT; "ins": payload the inserted bases; "del": payload the number of deleted bases; carriers a list of haplotypes"""
    from grafimo_amd.extract_regions import GraphIndex
    n, hw = len(sites), (H + 63) // 64
    pos = np.array([s[0] for s in sites], np.int32)
    n_alts, alt = np.ones(n, np.uint8), np.zeros((n, 3), np.uint8)
    bits = np.zeros((n, 3, hw), np.uint64)
    del_len, ins_len, ins_off = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    pool = bytearray()
    for i, (_, kind, payload, who) in enumerate(sites):
        if kind == "snv":
            n_alts[i] = len(payload)
            alt[i, :len(payload)] = np.frombuffer(payload.encode(), np.uint8)
            who = who if isinstance(who[0], (list, tuple)) else [who]
        elif kind == "ins":
            ins_len[i], ins_off[i] = len(payload), len(pool)
            pool += payload.encode()
            who = [who]
        else:
            del_len[i] = int(payload)
            who = [who]
        for k, hs in enumerate(who):
            for h in hs:
                bits[i, k, h >> 6] |= np.uint64(1) << np.uint64(h & 63)
    return GraphIndex(chrom, np.frombuffer(ref, np.uint8), pos, n_alts, alt, bits, H, del_len=del_len, ins_len=ins_len,
                      ins_off=ins_off, ins_bases=np.frombuffer(bytes(pool) or b"A", np.uint8))


def _bases(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


EDGE_S = 100
LONG_INS = 70


def edge_graph():
    """-> (GraphIndex of 1 400 bases and 3 haplotypes, regions, the indices of the two regions whose classes merge): every
    alignment of output offset and source position, a region of several strides, an insertion longer than a wavefront, the
    region rule's edges, carried deletions over a region's start, end and whole, two insertions at one anchor, a substitution
    under a carried deletion, regions beyond both ends of the chromosome, an empty region"""
    rng = np.random.default_rng(4242)
    L = 1400
    ref = _bases(rng, L)
    other = lambda p: "ACGT"[("ACGT".index(chr(ref[p])) + 1) % 4]      # noqa: E731
    sites = [
        (2, "snv", other(2), [1]),
        (103, "snv", other(103), [0]), (110, "ins", "TTG", [1]), (120, "del", 5, [2]), (130, "snv", other(130), [0, 1]),
        (150, "ins", "C", [0, 2]), (163, "del", 2, [1]),
        (250, "snv", other(250) + "ACGT"[("ACGT".index(chr(ref[250])) + 2) % 4], [[0], [2]]),
        (400, "ins", _bases(rng, LONG_INS).decode(), [0, 1]),
        (499, "ins", "GAT", [0]), (519, "ins", "CCCCA", [1, 2]),
        (600, "del", 30, [1]),
        (690, "del", 15, [0]), (735, "del", 10, [1]),
        (795, "del", 20, [2]), (805, "ins", "ACGTA", [0, 2]),
        (900, "ins", "AC", [0, 1]), (900, "ins", "GGT", [0, 2]),
        (950, "del", 6, [0, 1]), (953, "snv", other(953), [0, 2]),
        (1200, "snv", other(1200), [1]),
        (L - 1, "snv", other(L - 1), [2]), (L - 1, "ins", "TT", [0]),
    ]
    idx = _index("e", ref, sites, 3)
    regions = [(EDGE_S + k, EDGE_S + k + n) for k in range(4) for n in range(71)]
    merging = [len(regions) + 7, len(regions) + 8]
    regions += [(200, 1300),                                 # 1 100 bases: several strides, the long insertion, a deletion
                (395, 405),                                  # shorter than the insertion it holds
                (500, 520),                                  # insertions anchored at S - 1 and at E - 1
                (700, 740),                                  # a carried deletion over the start, another over the end
                (800, 810),                                  # wholly under a carried deletion; an insertion inside, read or jumped
                (796, 816), (795, 806),
                (890, 910),                                  # two insertions at one anchor, carried together and alone
                (940, 970),                                  # a substitution under a carried deletion
                (-5, 30), (1380, L + 20), (L - 1, L), (L, L + 5),
                (300, 300)]
    return idx, regions, merging


def chained_graph():
    """-> (GraphIndex, regions): A = a deletion of 20 bases at 50 (its span ends at 70), B = a deletion of 40 bases anchored at 60,
    inside A's span, that reaches to 100 -- into the regions, which start at 90 and later.  Haplotype 0 carries A and B (B's
    anchor is jumped over: B is not made), 1 B only, 2 A only, 3 none."""
    rng = np.random.default_rng(77)
    ref = _bases(rng, 300)
    sites = [(50, "del", 20, [0, 2]), (60, "del", 40, [0, 1]), (120, "ins", "GG", [0])]
    return _index("c", ref, sites, 4), [(90, 130), (101, 140), (95, 100), (71, 90), (40, 200)]
