"""Key sets without a GPU: obx_gpu_keyset_host_model builds the table in host
memory with the inline hash / insert / probe / sizing functions the device
kernels run (csrc/obx_keyset.h) and probes it. Expected values come from
numpy (np.isin, np.unique) and from the sizing rules stated in include/obx.h.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oceanbase_amd import abi, engine  # noqa: E402

I64 = np.iinfo(np.int64)
HASH, BITMAP = abi.KS_HASH, abi.KS_BITMAP
SPAN_CAP = 1 << 33


def _pow2(x):
    return x > 0 and x & (x - 1) == 0


def test_extreme_keys_hash_form():
    """every int64 can be a key, the empty-slot bit pattern (-1) included"""
    distinct = [I64.min, I64.max, -1, 0, 1]
    keys = distinct + [0, -1, I64.min, 1, 1, I64.max]
    neighbours = [I64.min + 1, I64.max - 1, -2, 2, 1 << 40, -(1 << 40)]
    hit, info = engine.keyset_host_model(keys, distinct + neighbours, HASH)
    assert hit[:5].all()
    assert not hit[5:].any()
    assert info.kind == HASH
    assert info.n_keys_in == len(keys)
    assert info.n_distinct == 5
    assert (info.min, info.max) == (I64.min, I64.max)


def test_marker_key_alone_and_absent():
    hit, info = engine.keyset_host_model([-1, -1], [-1, 0, -2], HASH)
    assert list(hit) == [True, False, False] and info.n_distinct == 1
    hit, _ = engine.keyset_host_model([0, -2], [-1, 0, -2], HASH)
    assert list(hit) == [False, True, True]


def test_auto_picks_bitmap_for_a_dense_range():
    rng = np.random.default_rng(1)
    keys = rng.integers(10**9, 10**9 + 4096, 1000)
    _, info = engine.keyset_host_model(keys)
    assert info.kind == BITMAP
    assert info.slots_or_bits == int(keys.max()) - int(keys.min()) + 1
    assert info.bytes == (info.slots_or_bits + 63) // 64 * 8
    # no larger than the hash table of max(64, pow2ceil(2 n)) u64 slots
    assert info.slots_or_bits <= 64 * 2048
    assert info.n_distinct == len(np.unique(keys))


def test_auto_picks_hash_for_a_sparse_range():
    rng = np.random.default_rng(2)
    keys = rng.integers(0, 1 << 40, 1000)
    _, info = engine.keyset_host_model(keys)
    assert info.kind == HASH
    assert info.slots_or_bits == 2048 and info.bytes == 2048 * 8
    assert info.n_distinct == len(np.unique(keys))


def test_auto_selection_boundary():
    """span <= 64 * slots picks the bitmap, one more bit the hash table;
    n = 40 keys -> slots = max(64, pow2ceil(80)) = 128"""
    n, slots = 40, 128
    for span, want in ((64 * slots, BITMAP), (64 * slots + 1, HASH)):
        keys = list(range(n - 1)) + [span - 1]
        _, info = engine.keyset_host_model(keys)
        assert info.kind == want, span
        assert info.slots_or_bits == (span if want == BITMAP else slots)


def test_forced_bitmap_past_the_cap_is_refused():
    with pytest.raises(engine.KeysetError) as e:
        engine.keyset_host_model([0, SPAN_CAP], [], BITMAP)
    assert e.value.rc == abi.OBX_NOT_SUPPORTED
    # auto never picks a bitmap there either
    _, info = engine.keyset_host_model([0, SPAN_CAP])
    assert info.kind == HASH


def test_span_overflowing_int64_picks_hash():
    hit, info = engine.keyset_host_model(
        [I64.min, I64.max], [I64.min, I64.max, 0, -1, 1, I64.min + 1])
    assert info.kind == HASH
    assert list(hit) == [True, True, False, False, False, False]
    assert info.n_distinct == 2
    with pytest.raises(engine.KeysetError) as e:
        engine.keyset_host_model([I64.min, I64.max], [], BITMAP)
    assert e.value.rc == abi.OBX_NOT_SUPPORTED


@pytest.mark.parametrize("kind", [abi.KS_AUTO, HASH, BITMAP])
def test_empty_set(kind):
    hit, info = engine.keyset_host_model([], [0, 1, -1, I64.min], kind)
    assert not hit.any()
    assert info.min > info.max and (info.min, info.max) == (1, -1)
    assert info.n_keys_in == 0 and info.n_distinct == 0
    assert info.kind == (BITMAP if kind == BITMAP else HASH)


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 1000, 4096, 4097, 70000])
def test_hash_sizing(n):
    keys = np.arange(n, dtype=np.int64) * 1000003
    _, info = engine.keyset_host_model(keys, [], HASH)
    s = info.slots_or_bits
    assert s >= 2 * n and s >= 64 and _pow2(s)
    assert s < 4 * n or s == 64  # the smallest such power of two
    assert info.bytes == 8 * s


@pytest.mark.parametrize("kind", [HASH, BITMAP])
def test_probe_equals_isin(kind):
    rng = np.random.default_rng(7 + kind)
    keys = rng.integers(-50000, 50000, 30000)
    probe = rng.integers(-60000, 60000, 10000)
    hit, info = engine.keyset_host_model(keys, probe, kind)
    assert info.kind == kind
    assert (hit == np.isin(probe, keys)).all()
    assert 0 < hit.sum() < len(probe)
    assert info.n_distinct == len(np.unique(keys))
    assert (info.min, info.max) == (int(keys.min()), int(keys.max()))


def test_probe_equals_isin_wide_hash():
    rng = np.random.default_rng(9)
    keys = rng.integers(I64.min, I64.max, 5000)
    probe = np.concatenate([keys[::2], rng.integers(I64.min, I64.max, 7500)])
    hit, _ = engine.keyset_host_model(keys, probe)
    assert (hit == np.isin(probe, keys)).all()


def test_bitmap_rejects_values_below_min_by_wrap():
    """idx = v - min wraps for v < min and must land past the span, at the
    far ends of the int64 range too"""
    keys = [I64.max - 3, I64.max]
    probe = [I64.max, I64.max - 3, I64.max - 2, I64.max - 4, I64.min, 0, -1]
    hit, info = engine.keyset_host_model(keys, probe, BITMAP)
    assert info.kind == BITMAP and info.slots_or_bits == 4
    assert list(hit) == [True, True, False, False, False, False, False]
    keys = [I64.min, I64.min + 2]
    probe = [I64.min, I64.min + 2, I64.min + 1, I64.min + 3, I64.max, 0, -1]
    hit, _ = engine.keyset_host_model(keys, probe, BITMAP)
    assert list(hit) == [True, True, False, False, False, False, False]


def test_make_filter_round_trips_a_set_leaf():
    assert abi.OP_IN_SET == 11
    f = abi.make_filter([dict(col=3, op=abi.OP_IN_SET, set=17),
                         dict(col=1, op=abi.OP_LT, lo=9)])
    assert f.n_leaves == 2
    assert (f.leaves[0].col, f.leaves[0].op, f.leaves[0].lo) == (3, 11, 17)
    assert f.leaves[0].n_in == 0
    assert (f.leaves[1].op, f.leaves[1].lo) == (abi.OP_LT, 9)


def test_jit_dump_renders_nothing_for_a_set_leaf():
    """obx_jit_dump_src has no context to resolve a set id"""
    import ctypes as C
    from oceanbase_amd import oracle
    lib = engine.lib()
    lib.obx_jit_dump_src.restype = C.c_int64
    schema = oracle.make_schema([(abi.T_INT, 0, 19, 8)])
    f = abi.make_filter([dict(col=0, op=abi.OP_IN_SET, set=0)])
    flags = (C.c_uint8 * 1)(16 | 4)
    mn, mx = (C.c_int64 * 1)(0), (C.c_int64 * 1)(100)
    cnt, w = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(64)
    rc = lib.obx_jit_dump_src(C.byref(f), None, schema, C.c_uint16(1), flags,
                              mn, mx, cnt, w, C.c_uint32(1000), 0, None,
                              C.c_int64(0))
    assert rc == 0
    f.leaves[0].op = 12  # past the last op: refused, not a silent no-match
    rc = lib.obx_jit_dump_src(C.byref(f), None, schema, C.c_uint16(1), flags,
                              mn, mx, cnt, w, C.c_uint32(1000), 0, None,
                              C.c_int64(0))
    assert rc == abi.OBX_INVALID_ARGUMENT
