"""The scan fold and the mutation profile on the host, restated with Python integers and plain loops over (row, pair, motif):
what tests/test_mutation_profile_host.py and tests/test_gpu_mutation_profile.py hold the kernel and the frames against.

THE RULE (include/grafimo_hip.h states it for the library).  For every (row, pair (ref column, alt column)) and every motif, with
r, a the two keys' scores (key >> 8) - 1 (-1 for key 0) and R, A the two sums:
  A side is a site when its key is not 0 and its score >= cutoff.
  gain when a is a site and r is not.  loss when r is a site and a is not.
  counts[gain] and counts[loss] count the motifs.
  Gain champion: the gaining motif with the smallest ptable[a].  Loss champion: the losing motif with the smallest ptable[r].
  Ties go to the smaller motif id.  A score >= table_len reads entry table_len - 1.
  Up champion: among motifs with A > R, the one with the largest A / R, compared exactly: motif 1 beats motif 2 when
  A1 * R2 > A2 * R1.  Down champion: among A < R, the largest R / A by the same rule.  Ties go to the smaller id.
  The empty state is all zero bytes.  Ids are stored as id + 1.
Python's integers have no width: the products below are exact whatever the sums are.
"""
import numpy as np

NAMES = ("counts", "site_motif", "site_keys", "site_p", "aff_motif", "aff_sums")
MUTATION_PAIRS = [(0, 1), (0, 2), (0, 3), (0, 4)]
INDEL_PAIRS = [(0, 1), (2, 3), (2, 4), (2, 5), (2, 6)]
BLOCK_PAIRS = [(0, 1)]


def empty_state(rows, P):
    return {"counts": np.zeros((rows, P, 2), dtype=np.uint32), "site_motif": np.zeros((rows, P, 2), dtype=np.uint32),
            "site_keys": np.zeros((rows, P, 2, 2), dtype=np.uint32), "site_p": np.zeros((rows, P, 2), dtype=np.float64),
            "aff_motif": np.zeros((rows, P, 2), dtype=np.uint32), "aff_sums": np.zeros((rows, P, 2, 2), dtype=np.uint64)}


def score_of(key):
    return (key >> 8) - 1 if key else -1


def is_site(key, cutoff):
    return key != 0 and score_of(key) >= cutoff


def fold(state, keys, sums, motif_ids, cutoffs, ptables, pairs):
    """one call: the motifs in the order given, into `state` (a dict of NAMES; not changed) -> the new state"""
    lists = {k: np.asarray(v).tolist() for k, v in state.items()}
    counts, site_motif, site_keys, site_p = lists["counts"], lists["site_motif"], lists["site_keys"], lists["site_p"]
    aff_motif, aff_sums = lists["aff_motif"], lists["aff_sums"]
    for m, mid in enumerate(motif_ids):
        K, S = np.asarray(keys[m]).tolist(), np.asarray(sums[m], dtype=np.uint64).tolist()
        pt, cutoff, mid = [float(v) for v in np.asarray(ptables[m])], int(cutoffs[m]), int(mid)
        for row in range(len(K)):
            for p, (rc, ac) in enumerate(pairs):
                kr, ka, R, A = int(K[row][rc]), int(K[row][ac]), int(S[row][rc]), int(S[row][ac])
                rs, als = is_site(kr, cutoff), is_site(ka, cutoff)
                side = 0 if (als and not rs) else 1 if (rs and not als) else None
                if side is not None:
                    counts[row][p][side] += 1
                    pv = pt[min(score_of(ka if side == 0 else kr), len(pt) - 1)]
                    cur = site_motif[row][p][side]
                    if cur == 0 or pv < site_p[row][p][side] or (pv == site_p[row][p][side] and mid + 1 < cur):
                        site_motif[row][p][side], site_keys[row][p][side], site_p[row][p][side] = mid + 1, [kr, ka], pv
                if A == R:
                    continue
                side = 0 if A > R else 1
                num, den = (A, R) if side == 0 else (R, A)
                cur = aff_motif[row][p][side]
                cur_ref, cur_alt = aff_sums[row][p][side]
                cur_num, cur_den = (cur_alt, cur_ref) if side == 0 else (cur_ref, cur_alt)
                if cur == 0 or num * cur_den > cur_num * den or (num * cur_den == cur_num * den and mid + 1 < cur):
                    aff_motif[row][p][side], aff_sums[row][p][side] = mid + 1, [R, A]
    return {k: np.array(lists[k], dtype=state[k].dtype).reshape(state[k].shape) for k in NAMES}


def fold_all(keys, sums, motif_ids, cutoffs, ptables, pairs):
    rows = len(keys[0])
    return fold(empty_state(rows, len(pairs)), keys, sums, motif_ids, cutoffs, ptables, pairs)


def random_case(rng, rows, C, M):
    """synthetic inputs of a fold in which the rare branches are common -> (keys, sums, ids, cutoffs, ptables) per motif: tables
    of differing lengths with runs of equal values, cutoffs anywhere in 0 .. table_len, scores within +- 2 of the cutoff (so
    some lie beyond the table) and keys of 0, sums drawn from {0, 1, 2^63, 2^64 - 1} mixed with random ones, ids shuffled"""
    lens = rng.integers(4, 12, size=M)
    ptables = [np.sort(rng.integers(1, 5, size=n))[::-1] / 8.0 for n in lens]
    cutoffs = [int(rng.integers(0, n + 1)) for n in lens]
    keys = [np.where(rng.random((rows, C)) < 0.15, 0,
                     ((np.clip(cutoffs[m] + rng.integers(-2, 3, size=(rows, C)), 0, None) + 1) << 8) | 129).astype(np.uint32)
            for m in range(M)]
    special = np.array([0, 1, 1 << 63, (1 << 64) - 1], dtype=np.uint64)
    sums = [np.where(rng.random((rows, C)) < 0.6, special[rng.integers(0, 4, size=(rows, C))],
                     rng.integers(0, 1 << 62, size=(rows, C)).astype(np.uint64)) for _ in range(M)]
    ids = rng.permutation(3 * M)[:M].tolist()
    return keys, sums, ids, cutoffs, ptables


def same_state(a, b):
    """byte for byte, every array"""
    return all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).shape == np.asarray(b[k]).shape
               and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in NAMES)


def first_difference(a, b):
    for k in NAMES:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return k, x.shape, y.shape, x.dtype, y.dtype
        if x.tobytes() != y.tobytes():
            bad = [i for i in np.ndindex(x.shape) if x[i].tobytes() != y[i].tobytes()][:3]
            return k, bad, [x[i].tolist() for i in bad], [y[i].tolist() for i in bad]
    return None
