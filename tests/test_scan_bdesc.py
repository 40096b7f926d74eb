"""GPU parity of the persistent scan kernel's packed block descriptors.

The kernel reads per-block geometry from a 128-byte record per block (built
once per handle and ordered column list, cached on the handle) and takes its
leaf tests as whole words. The block sets here differ from block to block in
row count, packed widths and stream offsets, so a stale, shifted or skipped
record changes the result. OBX_JIT_SGRID caps the grid so that a workgroup
sweeps several blocks. Every case compares `abi.result_rows` exactly against
the CPU oracle and asserts that the persistent (v2) kernel ran.
"""
import ctypes as Ct

import numpy as np
import pytest

from oceanbase_amd import abi, oracle

from test_scan_flush import _manual_blockset, _q1_descs

pytestmark = pytest.mark.gpu

N_BLOCKS = 10
_G = np.frombuffer(b"NPZ", dtype=np.uint8)
_D = np.array([-7, -3, 0, 2, 5], dtype=np.int64)
_B = np.array([0, 4, 10], dtype=np.int64)
_C = np.array([0, 2, 8], dtype=np.int64)
# per-block maximum of column w: its bit-packed width goes 2, 10, 5, 17, 1,
# 7, 13, 3, 20, 9 bits, which also shifts every later column's offset
_WMAX = [3, 1000, 20, 100000, 1, 100, 5000, 7, 1000000, 300]


@pytest.fixture(scope="module")
def eng():
    from oceanbase_amd.engine import GpuEngine
    e = GpuEngine(0)
    yield e
    e.close()


def _mixed_blocks(n_blocks=N_BLOCKS, seed=11):
    """cols: 0 grp CHAR dict, 1 w RAW int in [0, _WMAX[blk]] (bit-packed,
    width differs per block), 2 d signed dict, 3 r raw int64 (8-byte RAW),
    4 b dict dec(2), 5 c dict dec(2), 6 k RAW int == block index.
    Rows per block differ (700..1300); every block holds every dict value,
    so the dicts are byte-identical and the persistent kernel is eligible."""
    rng = np.random.default_rng(seed)
    schema = oracle.make_schema([
        (abi.T_CHAR, 0, 0, 1), (abi.T_INT, 0, 19, 8), (abi.T_INT, 0, 19, 8),
        (abi.T_INT, 0, 19, 8), (abi.T_DECIMAL_INT, 2, 15, 8),
        (abi.T_DECIMAL_INT, 2, 15, 8), (abi.T_INT, 0, 19, 8)])
    blocks, total = [], 0
    for blk in range(n_blocks):
        rows = 700 + (blk * 367) % 601          # 700..1300, all different
        g = rng.choice(_G, rows)
        w = rng.integers(0, _WMAX[blk % len(_WMAX)] + 1, rows)
        w[0] = _WMAX[blk % len(_WMAX)]          # pin the width
        d = rng.choice(_D, rows)
        r = rng.integers(-(1 << 30), 1 << 30, rows)
        r[1] = -5                               # keeps r an 8-byte RAW
        b = rng.choice(_B, rows)
        c = rng.choice(_C, rows)
        g[:3], d[:5], b[:3], c[:3] = _G, _D, _B, _C
        k = np.full(rows, blk, dtype=np.int64)
        cols = [g.astype(np.uint8)] + [
            a.astype(np.int64).view(np.uint8) for a in (w, d, r, b, c, k)]
        blocks.append(oracle.encode_block(
            schema, cols, [abi.ENC_DICT, abi.ENC_RAW, abi.ENC_DICT,
                           abi.ENC_RAW, abi.ENC_DICT, abi.ENC_DICT,
                           abi.ENC_RAW]))
        total += rows
    return _manual_blockset(schema, blocks, total)


@pytest.fixture(scope="module")
def mixed(eng):
    bs = _mixed_blocks()
    h = eng.load(bs)
    yield bs, h
    eng.free(h)


_ORACLE = {}


def _want(bs, key, filt, agg, n_aggs):
    """oracle result, computed once per (block set, plan)"""
    if key not in _ORACLE:
        res = oracle.scan_filter_agg(bs, filt, agg)
        _ORACLE[key] = (res.rows_passed, abi.result_rows(res, n_aggs))
    return _ORACLE[key]


def _check(eng, h, bs, key, filt, agg, n_aggs, bdesc=1):
    res = eng.scan_filter_agg(h, filt, agg)
    assert eng._lib.obx_gpu_last_jit(eng._ctx) == 2
    assert eng._lib.obx_gpu_last_bdesc(eng._ctx) == bdesc
    passed, rows = _want(bs, key, filt, agg, n_aggs)
    assert res.rows_passed == passed
    assert abi.result_rows(res, n_aggs) == rows
    return res


def _sgrid(monkeypatch, n):
    if n is None:
        monkeypatch.delenv("OBX_JIT_SGRID", raising=False)
    else:
        monkeypatch.setenv("OBX_JIT_SGRID", str(n))


_AGG6 = [dict(kind=abi.AGG_COUNT),
         dict(kind=abi.AGG_SUM, col_a=2),
         dict(kind=abi.AGG_SUM, col_a=3),
         dict(kind=abi.AGG_SUM_PROD2, col_a=3, col_b=4),
         dict(kind=abi.AGG_SUM_PROD3, col_a=3, col_b=4, col_c=5),
         dict(kind=abi.AGG_SUM, col_a=4)]

# filters on the block-index column k. With OBX_JIT_SGRID=3 workgroup 0
# sweeps blocks 0 3 6 9, workgroup 1 blocks 1 4 7, workgroup 2 blocks 2 5 8;
# with =1 one workgroup sweeps all ten.
_K_FILTERS = {
    "none": None,
    "first": [dict(col=6, op=abi.OP_GE, lo=1)],            # block 0 pruned
    "middle": [dict(col=6, op=abi.OP_NE, lo=4)],           # block 4
    "last": [dict(col=6, op=abi.OP_LE, lo=8)],             # block 9
    "consecutive": [dict(col=6, op=abi.OP_GE, lo=7)],      # 0 3 6 | 1 4 | 2 5
    "whole_workgroup": [dict(col=6, op=abi.OP_EQ, lo=1)],  # all but block 1
    # NL = 2: a range leaf on the width-changing column and a dict-ref-mask
    # leaf, so bleaves is indexed blk * 2 + i
    "two_leaf": [dict(col=1, op=abi.OP_BT, lo=1, hi=150),
                 dict(col=2, op=abi.OP_GE, lo=-3)],
}


@pytest.mark.parametrize("sgrid", [3, 1])
@pytest.mark.parametrize("name", sorted(_K_FILTERS))
def test_blocks_that_differ(eng, mixed, monkeypatch, name, sgrid):
    bs, h = mixed
    _sgrid(monkeypatch, sgrid)
    leaves = _K_FILTERS[name]
    filt = abi.make_filter(leaves) if leaves else None
    agg = abi.make_agg([0], _AGG6)
    res = _check(eng, h, bs, ("mixed", name), filt, agg, 6)
    assert eng._lib.obx_gpu_last_grid(eng._ctx) == sgrid
    if name == "whole_workgroup":
        assert res.rows_passed == 700 + 367     # block 1 alone
    if name == "none":
        assert res.rows_passed == bs.total_rows


@pytest.mark.parametrize("sgrid", [None, 1, 2])
@pytest.mark.parametrize("rows,n_blocks", [(1000, 1), (3500, 3)])
def test_q1_lineitem(eng, monkeypatch, rows, n_blocks, sgrid):
    _sgrid(monkeypatch, sgrid)
    li = oracle.Lineitem(4, rows, seed=5)
    assert li.n_blocks == n_blocks
    h = eng.load(li.bs)
    filt, agg = _q1_descs()
    _check(eng, h, li.bs, ("li", rows), filt, agg, 6)
    assert eng._lib.obx_gpu_last_grid(eng._ctx) == min(
        n_blocks, sgrid or n_blocks)
    eng.free(h)


def _builds(eng, h):
    eng._lib.obx_gpu_bdesc_builds.restype = Ct.c_int64
    return eng._lib.obx_gpu_bdesc_builds(eng._ctx, h)


def test_descriptor_cache_reuse_eviction_and_free(eng, monkeypatch):
    """One array per ordered column list: built by the first query that
    needs it, reused afterwards, at most four kept, gone with the handle."""
    _sgrid(monkeypatch, 3)
    bs = _mixed_blocks()
    h = eng.load(bs)
    assert _builds(eng, h) == 0

    def plan(cols):
        return abi.make_agg([0], [dict(kind=abi.AGG_COUNT)] + [
            dict(kind=abi.AGG_SUM, col_a=c) for c in cols])

    def run(cols):
        _check(eng, h, bs, ("cache", tuple(cols)), None, plan(cols),
               1 + len(cols))
        return _builds(eng, h)

    A, B = [2], [3]
    assert run(A) == 1
    assert run(B) == 2
    assert run(A) == 2                      # served from the handle
    n = 2
    for cols in ([4], [5], [2, 3], [3, 2], [4, 5]):   # five new lists
        n += 1
        assert run(cols) == n
    assert run([4, 5]) == n                 # the newest is still there
    assert run(A) == n + 1                  # A was evicted: rebuilt
    eng.free(h)
    assert _builds(eng, h) == -1
    # another table behind the next handle
    li = oracle.Lineitem(4, 3500, seed=5)
    h2 = eng.load(li.bs)
    filt, agg = _q1_descs()
    _check(eng, h2, li.bs, ("li", 3500), filt, agg, 6)
    assert _builds(eng, h2) == 1
    eng.free(h2)


@pytest.mark.parametrize("sgrid", [3, 1])
def test_ctx_column_that_needs_a_full_context(eng, mixed, monkeypatch, sgrid):
    """SUM over the bit-packed RAW column: not an aligned 8-byte stream, so
    its col_ctx is still built from dev_block while everything else comes
    from the record."""
    bs, h = mixed
    _sgrid(monkeypatch, sgrid)
    agg = abi.make_agg([0], [dict(kind=abi.AGG_COUNT),
                             dict(kind=abi.AGG_SUM, col_a=1),
                             dict(kind=abi.AGG_SUM, col_a=3)])
    filt = abi.make_filter([dict(col=6, op=abi.OP_GE, lo=2)])
    _check(eng, h, bs, ("mixed", "ctx"), filt, agg, 3)


def test_packed_path_off(eng, mixed, monkeypatch):
    """OBX_JIT_BDESC=0: the kernel reads dev_block as before. That is the
    path a handle takes when a count or width does not fit a slot; no plan
    eligible for this kernel can carry such a column (its dict counts stay
    under 64 and its streams under 64 bits), so the knob stands in for it."""
    bs, h = mixed
    _sgrid(monkeypatch, 3)
    monkeypatch.setenv("OBX_JIT_BDESC", "0")
    filt = abi.make_filter(_K_FILTERS["two_leaf"])
    agg = abi.make_agg([0], _AGG6)
    _check(eng, h, bs, ("mixed", "two_leaf"), filt, agg, 6, bdesc=0)
