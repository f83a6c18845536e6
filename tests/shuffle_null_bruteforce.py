"""Brute force for the shuffle null (grafimo_amd/shuffle_null.py) -- TEST INFRASTRUCTURE ONLY.

THE RULE (include/grafimo_hip.h states it for the library; grafimo_amd/shuffle_null.py for the table).  All arithmetic on 64-bit
words is modulo 2^64.
  G = 0x9E3779B97F4A7C15.
  mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
For a sequence x of n bases with a caller-given uint64 key k, a uint64 seed and the replicates r = 0 .. K - 1:
  s0 = mix(mix(seed + k G) + r).
  y starts as a copy of x: the bytes as they are, non-ACGT and lower case included.
  For i = n - 1 down to 1:  u = mix(s0 + i G);  j = ((u >> 32) (i + 1)) >> 32;  swap y[i] and y[j].
Scores, for a motif of width W: every window start 0 .. n - W is scored once per strand, + only when forward_only; a window that
holds a base that is not A/C/G/T scores min_val on both strands; case is folded.  best = the largest score over windows and
strands, -1 when n < W; sum = the exact sum of w[score] over windows and strands, 0 when there are none.  obs_best, obs_sum: those
of x itself.  ge_best = #{r : best_r >= obs_best}, ge_sum = #{r : sum_r >= obs_sum}; rep_hits[r] = the sum over the sequences v of
seq_weight[v] [best_{v,r} >= cut].

The Fisher-Yates walk is vectorised over the replicates with one Python step per position; the mixing is done on Python-checked
uint64 numpy words (MASK keeps every product modulo 2^64 explicit); every window of every shuffle is scored from scratch with
variant_bruteforce.int_score, and the sums are Python integers."""
import numpy as np

from variant_bruteforce import int_score, revcomp

MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def mix(z: int) -> int:
    """on one Python integer"""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mix_words(z: np.ndarray) -> np.ndarray:
    """mix on a uint64 array (numpy wraps modulo 2^64)"""
    z = np.array(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def permutations(n: int, key: int, seed: int, K: int, r0: int = 0) -> np.ndarray:
    """int64 [K, n]: row r - r0 holds the positions of x that replicate r = r0 .. r0 + K - 1 takes, y[p] = x[row[p]]"""
    s0 = np.array([mix(mix(seed + key * G) + r) for r in range(r0, r0 + K)], dtype=np.uint64)
    perm = np.tile(np.arange(n, dtype=np.int64), (K, 1))
    rows = np.arange(K)
    for i in range(n - 1, 0, -1):
        with np.errstate(over="ignore"):
            u = mix_words(s0 + np.uint64((i * G) & MASK))
        j = (((u >> np.uint64(32)) * np.uint64(i + 1)) >> np.uint64(32)).astype(np.int64)     # ((u >> 32) (i + 1)) < 2^63
        a, b = perm[rows, i].copy(), perm[rows, j].copy()
        perm[rows, i], perm[rows, j] = b, a
    return perm


def shuffles(x: bytes, key: int, seed: int, K: int):
    """the K shuffles of x as bytes"""
    xs = np.frombuffer(x, dtype=np.uint8)
    return [xs[p].tobytes() for p in permutations(len(x), key, seed, K)]


def pair(y: bytes, W: int, sm, min_val: int, wtab, forward_only: bool):
    """-> (best, sum) of one sequence: every window from scratch"""
    best, total = -1, 0
    for s in range(len(y) - W + 1):
        k = y[s:s + W]
        scores = [int_score(k, sm, min_val)] + ([] if forward_only else [int_score(revcomp(k), sm, min_val)])
        for sc in scores:
            best = max(best, sc)
            total += int(wtab[sc])
    return best, total


_CODE = np.full(256, -1, dtype=np.int64)                 # rows of the score matrix: A, C, G, T
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c + 32] = _k


def pairs(ys: np.ndarray, W: int, sm, min_val: int, wtab, forward_only: bool):
    """pair() for the rows of ys uint8 [K, n] at once -> [(best, sum)] of Python integers: every window of every row is gathered
    from the score matrix column by column -- no running sum, nothing shared between windows --, the weights are added as two
    32-bit halves so that no numpy sum can wrap"""
    K, n = ys.shape
    if n < W:
        return [(-1, 0)] * K
    sm = np.asarray(sm, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(_CODE[ys], W, axis=1)                  # [K, n - W + 1, W]
    bad = (win < 0).any(axis=-1)
    cols = np.arange(W)
    strands = [np.where(bad, min_val, sm[np.maximum(win, 0), cols].sum(axis=-1))]
    if not forward_only:
        strands.append(np.where(bad, min_val, sm[3 - np.maximum(win[..., ::-1], 0), cols].sum(axis=-1)))
    scores = np.concatenate(strands, axis=1)                                              # [K, windows x strands]
    w = np.asarray(wtab, dtype=np.uint64)[scores]
    lo, hi = (w & np.uint64(0xFFFFFFFF)).sum(axis=1, dtype=np.uint64), (w >> np.uint64(32)).sum(axis=1, dtype=np.uint64)
    return [(int(b), (int(h) << 32) + int(l)) for b, h, l in zip(scores.max(axis=1), hi, lo)]


def replicates(seqs, keys, seed: int, K: int, W: int, sm, min_val: int, wtab, forward_only: bool):
    """-> dict of lists of Python integers: obs_best, obs_sum [S], rep_best, rep_sum [S][K].  The observed pair is made by
    pair(), one window at a time, and must be what pairs() gives for x."""
    out = dict(obs_best=[], obs_sum=[], rep_best=[], rep_sum=[])
    for v, x in enumerate(seqs):
        xs = np.frombuffer(x, dtype=np.uint8)
        ob, os_ = pair(x, W, sm, min_val, wtab, forward_only)
        assert pairs(xs[None, :], W, sm, min_val, wtab, forward_only) == [(ob, os_)]
        reps = pairs(xs[permutations(len(x), int(keys[v]), seed, K)], W, sm, min_val, wtab, forward_only)
        out["obs_best"].append(ob)
        out["obs_sum"].append(os_)
        out["rep_best"].append([b for b, _ in reps])
        out["rep_sum"].append([t for _, t in reps])
    return out


def counts(reps: dict, K: int, cut: int, seq_weights=None) -> dict:
    """What the kernel returns for the first K replicates of replicates() (replicate r does not depend on K), one comparison
    at a time -> dict of lists of Python integers: obs_best, obs_sum, ge_best, ge_sum [S], rep_hits [K], rep_best, rep_sum [S][K]"""
    S = len(reps["obs_best"])
    seq_weights = [1] * S if seq_weights is None else [int(w) for w in seq_weights]
    out = dict(obs_best=list(reps["obs_best"]), obs_sum=list(reps["obs_sum"]), ge_best=[], ge_sum=[], rep_hits=[0] * K,
               rep_best=[row[:K] for row in reps["rep_best"]], rep_sum=[row[:K] for row in reps["rep_sum"]])
    for v in range(S):
        assert len(out["rep_best"][v]) == K
        out["ge_best"].append(sum(int(b >= out["obs_best"][v]) for b in out["rep_best"][v]))
        out["ge_sum"].append(sum(int(t >= out["obs_sum"][v]) for t in out["rep_sum"][v]))
        for r, b in enumerate(out["rep_best"][v]):
            out["rep_hits"][r] += seq_weights[v] * int(b >= cut)
    return out


def null(seqs, keys, seed: int, K: int, W: int, sm, min_val: int, wtab, forward_only: bool, cut: int, seq_weights=None) -> dict:
    """counts() of replicates()"""
    return counts(replicates(seqs, keys, seed, K, W, sm, min_val, wtab, forward_only), K, cut, seq_weights)


def content_key(x: bytes) -> int:
    """mix(sum over the offsets o of mix(upper(x[o]) + 256 o), plus n), one Python step per base"""
    total = 0
    for o, c in enumerate(x.upper()):
        total = (total + mix(c + 256 * o)) & MASK
    return mix(total + len(x))
