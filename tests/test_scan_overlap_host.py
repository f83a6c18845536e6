"""grafimo_amd.scan.overlap_launches -- when a KmerScanner passes GFM_FLAG_OVERLAP_LAUNCHES -- over every combination of
its inputs.  The flag takes a batch's score kernel off the caller's stream, so it may be passed only where nothing relies
on that stream's order: host-paced slots, a side stream that orders the consumers, no process group, no more slots than
the library's workspace ring.  The environment switch chooses among those cases and never adds one."""
import itertools

import pytest

from grafimo_amd import _native as nv
from grafimo_amd import scan

ENVS = [None, "", "0", "1", " 1 ", "yes", "2"]


def _qualifies(host_paced, side, collective, n_slots):
    return host_paced and side and not collective and n_slots <= nv.GFM_WORKSPACE_RING


@pytest.mark.parametrize("env", ENVS)
def test_every_combination(env):
    for host_paced, side, collective, n_slots in itertools.product((False, True), (False, True), (False, True), range(1, 10)):
        got = scan.overlap_launches(host_paced, side, collective, n_slots, env)
        assert isinstance(got, bool)
        if not _qualifies(host_paced, side, collective, n_slots):
            assert got is False, (host_paced, side, collective, n_slots, env)
        elif env is not None and env.strip() == "0":
            assert got is False
        elif env is not None and env.strip() == "1":
            assert got is True
        else:
            assert got is scan.OVERLAP_LAUNCHES_DEFAULT


def test_the_flag_is_a_bit_of_its_own():
    flags = [nv.GFM_FLAG_RESET_HITS, nv.GFM_FLAG_CLEAR_HIST, nv.GFM_FLAG_CALLER_ORDERS_REUSE, nv.GFM_FLAG_OVERLAP_LAUNCHES]
    assert all(f and f & (f - 1) == 0 for f in flags) and len(set(flags)) == len(flags)
    assert "gfm_overlapped_launches" in nv.PROTOTYPES


def test_the_default_pipeline_qualifies_and_its_neighbours_do_not():
    """bench.py's resident pipeline: three slots (host-paced), a side stream, one process."""
    assert scan.overlap_launches(True, True, False, 3, "1") is True
    assert scan.overlap_launches(True, True, False, 4, "1") is True
    assert scan.overlap_launches(True, True, False, 5, "1") is False      # the library orders the ring itself there
    assert scan.overlap_launches(False, True, False, 2, "1") is False     # two slots: the device paces slot reuse
    assert scan.overlap_launches(True, False, False, 3, "1") is False     # no side stream: consumers follow the caller's stream
    assert scan.overlap_launches(True, True, True, 3, "1") is False       # collectives beside the grid
