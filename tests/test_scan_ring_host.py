"""grafimo_amd.scan.score_ring_step -- which score array a turn of KmerScanner writes and which earlier batch its score
kernel must wait for when the score arrays form a shorter ring than the slots -- against a brute-force model that knows
only which array each turn wrote and which tails read their scores.  Every pair of ring lengths up to nine slots, seven
laps, read flags all-true, all-false, alternating and seeded random.  The model is shown to have teeth on the rule the
scanner followed before (array bound to the slot, wait for turn t - nb and only if the CURRENT tail reads)."""
import numpy as np
import pytest

from grafimo_amd.scan import score_ring_step

LAPS = 7
PAIRS = [(s, nb) for s in range(1, 10) for nb in range(1, s + 1)]

# pairs for which the previous rule waited for a batch older than the array's last writer (n_slots % nb != 0)
OLD_RULE_STALE = {(3, 2), (4, 3), (5, 2), (5, 3), (5, 4), (6, 4), (6, 5), (7, 2), (7, 3), (7, 4), (7, 5), (7, 6), (8, 3),
                  (8, 5), (8, 6), (8, 7), (9, 2), (9, 4), (9, 5), (9, 6), (9, 7), (9, 8)}


def _patterns(n_turns, n_slots, nb):
    """name -> read flag per turn"""
    out = {"all": [True] * n_turns, "none": [False] * n_turns, "alternating": [t % 2 == 0 for t in range(n_turns)]}
    for seed in range(4):
        rng = np.random.default_rng(1000 * n_slots + 10 * nb + seed)
        out[f"random{seed}"] = [bool(x) for x in rng.random(n_turns) < (0.25, 0.5, 0.5, 0.75)[seed]]
    return out


def _new_rule(turn, n_slots, nb, reads):
    return score_ring_step(turn, n_slots, nb, reads.__getitem__)


def _old_rule(turn, n_slots, nb, reads):
    """What KmerScanner.enqueue did before: slot k owns array k % nb; wait for turn t - nb if this turn's tail reads."""
    wait = turn - nb if (nb < n_slots and reads[turn] and turn >= nb) else None
    return (turn % n_slots) % nb, wait


def _violations(rule, n_slots, nb, reads):
    """Walk the turns; returns the broken properties as (property, turn, detail)."""
    bad = []
    writers = {}                                    # array -> turns that wrote it, in order
    for t in range(len(reads)):
        a, wait = rule(t, n_slots, nb, reads)
        if not (0 <= a < nb):
            bad.append(("array", t, a))
        if wait is not None and not (0 <= wait < t):
            bad.append(("wait-range", t, wait))
        earlier = writers.get(a, [])
        # done events are recorded in turn order on one stream: waiting for turn w covers every turn <= w
        covered = max(t - n_slots, -1 if wait is None else wait)
        for w in earlier:
            if reads[w] and w > covered:
                bad.append(("safety", t, w))
        if wait is not None:
            if not earlier or wait > earlier[-1]:
                bad.append(("over-wait-young", t, wait))
            if not any(reads[w] for w in earlier):
                bad.append(("over-wait-none", t, wait))
        if earlier and t - earlier[-1] < nb:
            bad.append(("lifetime", t, earlier[-1]))
        writers.setdefault(a, []).append(t)
    return bad


@pytest.mark.parametrize("n_slots,nb", PAIRS)
def test_rule_is_safe_never_over_waits_and_keeps_the_lifetime(n_slots, nb):
    n_turns = LAPS * n_slots
    for name, reads in _patterns(n_turns, n_slots, nb).items():
        assert _violations(_new_rule, n_slots, nb, reads) == [], (n_slots, nb, name)
    # no reader anywhere (a p-value scan without regions): slot pacing only
    assert all(_new_rule(t, n_slots, nb, [False] * n_turns)[1] is None for t in range(n_turns))
    # a full ring is ordered by the slot-reuse wait alone, whatever the tails read
    assert all(_new_rule(t, n_slots, n_slots, [True] * n_turns)[1] is None for t in range(n_turns))


@pytest.mark.parametrize("n_slots,nb", PAIRS)
def test_first_lap_binds_exactly_nb_arrays(n_slots, nb):
    """The turns of one lap -- the slots after construction -- reference exactly nb distinct arrays, every lap."""
    for lap in range(LAPS):
        arrays = {score_ring_step(t, n_slots, nb, lambda w: False)[0] for t in range(lap * n_slots, (lap + 1) * n_slots)}
        assert arrays == set(range(nb))


def test_documented_pairs_by_hand():
    """(4,3): turn 4 writes the array of turn 1, not the one turn 3 just wrote (turn 3 took turn 0's, while slot 3 was
    still new: no slot wait covers it); (8,3): turn 8 follows turn 5."""
    reads = [True] * 32
    assert [_new_rule(t, 4, 3, reads) for t in range(6)] == [(0, None), (1, None), (2, None), (0, 0), (1, 1), (2, 2)]
    assert _new_rule(8, 8, 3, reads) == (2, 5) and _new_rule(6, 8, 3, reads) == (0, 3)
    # the youngest READING writer inside the slot window is named; older ones are implied by it
    reads = [True] * 32
    reads[5] = False
    assert _new_rule(8, 8, 3, reads) == (2, 2)
    reads[2] = False
    assert _new_rule(8, 8, 3, reads) == (2, None)


def test_model_rejects_the_previous_rule():
    """Teeth: the rule before (wait for t - nb, only if the current tail reads; array bound to the slot) breaks safety
    with every tail reading exactly where n_slots % nb != 0, breaks the lifetime for the same pairs, and leaves a reader
    followed by a non-reading writer unguarded for every shorter ring."""
    stale, short_lived, unguarded = set(), set(), set()
    for n_slots, nb in PAIRS:
        n_turns = LAPS * n_slots
        pats = _patterns(n_turns, n_slots, nb)
        kinds = {k for k, _, _ in _violations(_old_rule, n_slots, nb, pats["all"])}
        if "safety" in kinds:
            stale.add((n_slots, nb))
        if "lifetime" in kinds:
            short_lived.add((n_slots, nb))
        for name, reads in pats.items():
            if name not in ("all", "none") and any(k == "safety" and not reads[t]
                                                   for k, t, _ in _violations(_old_rule, n_slots, nb, reads)):
                unguarded.add((n_slots, nb))
    assert stale == OLD_RULE_STALE
    assert short_lived == OLD_RULE_STALE
    assert unguarded == {(s, nb) for s, nb in PAIRS if nb < s}
