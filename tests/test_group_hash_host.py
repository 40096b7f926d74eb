"""The sized group table without a GPU: obx_gpu_group_hash_host_model runs
the inline sizing and find-or-insert functions of csrc/obx_grouphash.h, the
ones the kernels run, over host memory. Expected values come from numpy and
from the sizing rule stated there:

    slots = max(2^13, pow2ceil(2 * min(max_groups, n_keys) + in_flight))

The longest probe sequence is printed, not asserted: there is no derived
bound for it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oceanbase_amd import abi, engine  # noqa: E402

CAP0 = abi.GROUP_CAP_DEFAULT


def pow2ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def want_slots(max_groups, n_keys, in_flight):
    return max(abi.GROUP_HASH_MIN_SLOTS,
               pow2ceil(2 * min(max_groups, n_keys) + in_flight))


def _sequential():
    return np.arange(20_000, dtype=np.uint64)


def _high_bits_only():
    # char << 32 under a constant int32: the keys differ only above bit 32
    return (np.arange(6_000, dtype=np.uint64) << np.uint64(32)) | np.uint64(7)


def _one_repeated():
    return np.full(10_000, 0x1234_5678_9ABC, dtype=np.uint64)


def _random():
    rng = np.random.default_rng(11)
    return rng.integers(0, 2**56, 70_000, dtype=np.uint64)


KEYSETS = {"sequential": _sequential, "high_bits": _high_bits_only,
           "one_repeated": _one_repeated, "random70k": _random}


@pytest.mark.parametrize("name", sorted(KEYSETS))
@pytest.mark.parametrize("in_flight", [0, 40_000])
def test_model_against_numpy(name, in_flight):
    keys = KEYSETS[name]()
    live = len(np.unique(keys))
    cap = max(live, CAP0)
    m = engine.group_hash_host_model(keys, cap, in_flight)
    print(f"{name} in_flight={in_flight}: slots={m['slots']} live={m['live']} "
          f"longest probe={m['max_probe']}")
    assert m["rc"] == abi.OBX_SUCCESS
    assert m["found"] == len(keys)          # every key is found again
    assert m["live"] == live
    assert m["slots"] == want_slots(cap, len(keys), in_flight)
    assert m["bytes"] == m["slots"] * (16 + 32 * 2)


@pytest.mark.parametrize("name", ["sequential", "high_bits", "random70k"])
@pytest.mark.parametrize("in_flight", [0, 40_000])
def test_cap_is_exact(name, in_flight):
    keys = KEYSETS[name]()
    live = len(np.unique(keys))
    assert live - 1 >= CAP0
    ok = engine.group_hash_host_model(keys, live, in_flight)
    assert ok["rc"] == abi.OBX_SUCCESS and ok["live"] == live
    no = engine.group_hash_host_model(keys, live - 1, in_flight)
    print(f"{name} in_flight={in_flight}: refused at live={no['live']} of "
          f"{no['slots']} slots, longest probe={no['max_probe']}")
    assert no["rc"] == abi.OBX_BUF_NOT_ENOUGH
    assert no["slots"] == want_slots(live - 1, len(keys), in_flight)
    # a refused scan stops within in_flight keys of the grant, so the table
    # never fills: the sizing leaves the granted slots free
    assert live - 1 < no["live"] <= live - 1 + max(in_flight, 1)
    assert no["live"] < no["slots"]


def test_raised_cap_on_few_keys_gives_the_floor():
    keys = np.arange(300, dtype=np.uint64)
    for cap in (CAP0, 1 << 20, abi.GROUP_CAP_MAX):
        m = engine.group_hash_host_model(keys, cap, 0)
        assert m["rc"] == abi.OBX_SUCCESS
        assert (m["slots"], m["live"], m["found"]) == (1 << 13, 300, 300)


def test_record_bytes_follow_the_plan():
    keys = np.arange(10, dtype=np.uint64)
    for n_aggs in (0, 1, 2, 8):
        m = engine.group_hash_host_model(keys, CAP0, 0, n_aggs)
        assert m["bytes"] == (1 << 13) * (16 + 32 * n_aggs)


def test_empty_input():
    m = engine.group_hash_host_model(np.zeros(0, dtype=np.uint64), CAP0, 0)
    assert (m["rc"], m["live"], m["slots"]) == (0, 0, 1 << 13)


def test_cap_range():
    keys = np.arange(10, dtype=np.uint64)
    with pytest.raises(engine.GroupCapError) as e:
        engine.group_hash_host_model(keys, CAP0 - 1, 0)
    assert e.value.rc == abi.OBX_INVALID_ARGUMENT
    with pytest.raises(engine.GroupCapError) as e:
        engine.group_hash_host_model(keys, abi.GROUP_CAP_MAX + 1, 0)
    assert e.value.rc == abi.OBX_NOT_SUPPORTED
