"""Calls that give a workgroup of the tile-based sequence scans a second and a third tile -- TEST INFRASTRUCTURE ONLY, no test.

The six scans walk the tile table with `for (t = blockIdx.x; t < n_tiles; t += gridDim.x)` under a capped grid (CAPS), and a
turn of that loop works in the LDS the turn before it left.  The tile count of a call depends on the NUMBER of its sequences:
a pool of a few distinct sequences (pool), repeated around a filler of one- and two-base sequences (layout), puts chosen
tiles exactly `cap` tiles apart -- tile t + cap is the next turn of the workgroup that did tile t -- in a call of under
100 000 bases, and the brute force runs over the pool alone (gather).  coverage says which successions the call must hold.
tests/test_many_tiles_host.py holds this module to the library's caps; tests/test_gpu_scan_many_tiles.py uses it."""
import numpy as np

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
# the grids' caps: kSeqMaxBlocks (gfm_sequence_tiles.hpp), kInsMaxBlocks (gfm_graph_insertion_scan.hpp) and the 1 << 15
# workgroups of kQvWaves = 4 wavefronts, an item each, of gfm_graph_query_edits (gfm_graph_query_variants.hpp)
CAPS = {"seq": 65536, "insertion": 4096, "query_items": 32768 * 4}


def sizes(W, T):
    out = []
    for n in [1, 2, W - 1, W, W + 1, 63, 64, 65, W + 63, W + 64, T + W - 1, 2 * T + 3, 3 * T + 1]:
        if n > 0 and n not in out:
            out.append(n)
    return out


def pool(W, T, rng):
    """Distinct sequences of `sizes` -- test_gpu_deletion_scan._sequences' family with 2 and 3 T + 1 -- with lower-case bases
    and an N at offset 0 and at the last offset (T + 1: the second tile's only base, just behind the edge), just behind a tile
    edge (T + W - 1, when it is that long), just before a tile edge and at the last offset (2 T + 3), inside the second tile's
    right halo (3 T + 1, at 2 T + 9: its first two tiles hold none) and at offset 0 of W + 1 bases; then A, c, N, GT and
    70 x N.  W - 1, W, 63, 64, W + 63 and W + 64 bases hold no N at all (where no other size coincides)."""
    seqs = []
    for n in sizes(W, T):
        x = bytearray(BASES[rng.integers(0, 4, size=n)].tobytes())
        for j in np.flatnonzero(rng.random(n) < 0.15).tolist():
            x[j] |= 0x20
        if n == T + 1:
            x[0] = ord("N")
            x[n - 1] = ord("n")
        if n == T + W - 1 and n > T:
            x[T] = ord("N")
        if n == 2 * T + 3:
            x[T - 1] = ord("N")
            x[n - 1] = ord("N")
        if n == 3 * T + 1:
            x[2 * T + 9] = ord("n")
        if n == W + 1:
            x[0] = ord("N")
        seqs.append(bytes(x))
    seqs += [b"A", b"c", b"N", b"GT", b"N" * 70]
    out = []
    for x in seqs:
        if x not in out:
            out.append(x)
    assert any(c in b"acgt" for x in out for c in x)
    return out


def _shift(k, r, P, rotations):
    """how far the reversed pool is rotated in copy r of block k >= 1: a different start in every copy of a block, and another
    set in the third block than in the second"""
    return ((2 * r + 1) * P // (2 * rotations) + 3 * (k - 1)) % P


def layout(pool_, T, cap, turns=2, rotations=4):
    """-> (call, pairs).  call: the pool index of every sequence, in order -- `rotations` copies of the pool in order; one- and
    two-base pool members until tile number `cap` exactly; `rotations` copies of the pool, each in another rotation of the
    reversed order; with turns = 3 filler again, and a third block from tile 2 cap on.  pairs: (kind of tile t, kind of tile
    t + cap) for every t that has a tile t + cap, a kind being (pool index, tile start): the two successive turns of one
    workgroup, as long as the grid is `cap` workgroups."""
    P = len(pool_)
    small = [i for i, x in enumerate(pool_) if len(x) <= 2]
    assert len({len(pool_[i]) for i in small}) == 2 and all(len(x) > 0 for x in pool_)
    call, kinds = [], []

    def put(i):
        call.append(i)
        kinds.extend((i, s) for s in range(0, len(pool_[i]), T))

    for k in range(turns):
        j = k                                                    # (a filler tile's next turn is another filler member)
        assert len(kinds) <= k * cap, "a block of the pool's copies holds more tiles than the cap"
        while len(kinds) < k * cap:
            put(small[j % len(small)])
            j += 1
        for r in range(rotations):
            order = list(range(P))
            if k > 0:
                s = _shift(k, r, P, rotations)
                order = order[::-1][s:] + order[::-1][:s]
            for i in order:
                put(i)
    return call, [(kinds[t], kinds[t + cap]) for t in range(len(kinds) - cap)]


def coverage(pairs, pool_, W, T):
    """asserts that the successions a stale LDS value would show in are among the pairs -> how many of each"""
    def nt(k):
        return min(T, len(pool_[k[0]]) - k[1])

    def holds_n(k):
        return any(c in b"Nn" for c in pool_[k[0]][k[1]:k[1] + nt(k)])

    def clean(k):                                                # no N in anything a kernel stages for the tile
        return not any(c in b"Nn" for c in pool_[k[0]][max(0, k[1] - T):k[1] + 3 * T])

    def one(k):
        return len(pool_[k[0]]) == 1

    def tail(k):                                                 # a longer sequence's last, partial tile
        return k[1] > 0 and nt(k) < T

    def middle(k):
        return len(pool_[k[0]]) == 3 * T + 1 and 0 < k[1] and k[1] + T < len(pool_[k[0]])

    count = dict(
        full_then_one=sum(1 for a, b in pairs if nt(a) == T and one(b)),
        one_then_full=sum(1 for a, b in pairs if one(a) and nt(b) == T),
        n_then_none=sum(1 for a, b in pairs if holds_n(a) and clean(b)),
        none_then_n=sum(1 for a, b in pairs if clean(a) and holds_n(b)),
        middle_then_tail=sum(1 for a, b in pairs if middle(a) and tail(b)),
        same=sum(1 for a, b in pairs if a == b))
    if W > 1:
        count["long_then_short"] = sum(1 for a, b in pairs if len(pool_[a[0]]) >= W + 64 and len(pool_[b[0]]) < W)
    assert pairs and all(v > 0 for k, v in count.items() if k != "same"), count
    assert 10 * count["same"] <= len(pairs), count
    return count


def call_arrays(pool_, call):
    """-> (seq_offsets int64 [len(call) + 1], bases uint8) of the call"""
    off = np.concatenate([[0], np.cumsum([len(pool_[i]) for i in call])]).astype(np.int64)
    return off, np.frombuffer(b"".join(pool_[i] for i in call), dtype=np.uint8)


def tile_count(seq_offsets, T):
    """as seq_tiles counts them: a tile per T offsets of every sequence, none for an empty one"""
    return int(((np.diff(seq_offsets) + T - 1) // T).sum())


def later_turn_bases(seq_offsets, T, cap):
    """-> bool [n_bases]: the base lies in a tile numbered `cap` or higher"""
    n = np.diff(seq_offsets)
    first = np.concatenate([[0], np.cumsum((n + T - 1) // T)])[:-1]                   # a sequence's first tile
    within = np.arange(int(seq_offsets[-1]), dtype=np.int64) - np.repeat(seq_offsets[:-1], n)
    return np.repeat(first, n) + within // T >= cap


def gather(pool_result, pool_, call, axis):
    """The rows of the pool's brute force (`pool_result`: an array whose `axis` runs over the pool's bases, sequence after
    sequence) in the call's row order, by ONE index array: every row of the call, filler included."""
    lens = np.array([len(x) for x in pool_], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(lens)])[:-1]
    call = np.asarray(call, dtype=np.int64)
    n = lens[call]
    at = np.concatenate([[0], np.cumsum(n)])[:-1]                # where a sequence of the call begins in the call
    index = np.repeat(start[call] - at, n) + np.arange(int(n.sum()), dtype=np.int64)
    pool_result = np.asarray(pool_result)
    assert pool_result.shape[axis] == int(lens.sum())
    return np.take(pool_result, index, axis=axis)
