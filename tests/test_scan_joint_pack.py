"""GPU parity of the persistent scan kernel's packed joint cells.

A row adds `weight + (1 << S)` into one 64-bit joint cell (group cell x dict
ref of one or two factor columns), so the cell carries the weight sum in its
low S bits and the row count above them; COUNT(*), the weighted products and
the sums over the factor columns all come out of that table at flush. Every
case compares `abi.result_rows` exactly with the CPU oracle and asserts the
form the kernel took (`GpuEngine.last_joint`): 2 = one axis with the packed
count, 3 = two axes with the packed count (only where the two-axis table
stays under 2 KB: past that it costs an occupancy step and measured slower,
profiles/r10_q1_joint_pack.md), 1 = the weighted table without the count
(OBX_JIT_JPACK=0). OBX_JIT_SGRID caps the grid so that one workgroup sweeps
many blocks and the cells accumulate across them.
"""
import numpy as np
import pytest

from oceanbase_amd import abi, oracle

from test_scan_flush import _manual_blockset, _q1_descs

pytestmark = pytest.mark.gpu

_KNOBS = ("OBX_JIT_JPACK", "OBX_JIT_JWS", "OBX_JIT_SGRID")


@pytest.fixture(scope="module")
def eng():
    from oceanbase_amd.engine import GpuEngine
    e = GpuEngine(0)
    yield e
    e.close()


_ORACLE = {}


def _want(key, bs, filt, agg, n_aggs):
    """oracle result, computed once per (table, plan)"""
    if key not in _ORACLE:
        res = oracle.scan_filter_agg(bs, filt, agg)
        _ORACLE[key] = (res.rows_passed, abi.result_rows(res, n_aggs))
    return _ORACLE[key]


def _env(monkeypatch, sgrid, pack=True):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    if not pack:
        monkeypatch.setenv("OBX_JIT_JPACK", "0")
    if sgrid:
        monkeypatch.setenv("OBX_JIT_SGRID", str(sgrid))


def _check(eng, h, key, bs, filt, agg, n_aggs, form):
    res = eng.scan_filter_agg(h, filt, agg)
    assert eng._lib.obx_gpu_last_jit(eng._ctx) == 2     # persistent kernel
    if form is not None:
        assert eng.last_joint() == form
    passed, rows = _want(key, bs, filt, agg, n_aggs)
    assert res.rows_passed == passed
    assert abi.result_rows(res, n_aggs) == rows
    return res


# ---- 1. the Q1 plan on generated lineitem ---------------------------------

# 12 group cells x 12 disc x 10 tax refs would be 11.5 KB of joint cells:
# Q1 keeps one axis (disc); the count rides on it, PROD3 keeps its window
_LI_ROWS = 60000


@pytest.fixture(scope="module")
def lineitem(eng):
    li = oracle.Lineitem(4, _LI_ROWS, seed=9)
    assert 40 <= li.n_blocks <= 60
    h = eng.load(li.bs)
    yield li, h
    eng.free(h)


@pytest.mark.parametrize("sgrid", [1, 3, None])
@pytest.mark.parametrize("form", [2, 1])
def test_q1_plan(eng, lineitem, monkeypatch, form, sgrid):
    li, h = lineitem
    _env(monkeypatch, sgrid, pack=form == 2)
    filt, agg = _q1_descs()
    _check(eng, h, "q1", li.bs, filt, agg, 6, form)
    assert eng._lib.obx_gpu_last_grid(eng._ctx) == (sgrid or li.n_blocks)


@pytest.mark.parametrize("sgrid", [1, 3])
@pytest.mark.parametrize("form", [3, 1])
def test_q1_plan_without_groups_takes_both_axes(eng, lineitem, monkeypatch,
                                                form, sgrid):
    """No group column: 12 x 10 joint cells are 960 B, both axes stay."""
    li, h = lineitem
    _env(monkeypatch, sgrid, pack=form == 3)
    filt, _ = _q1_descs()
    agg = abi.make_agg([], [
        dict(kind=abi.AGG_COUNT), dict(kind=abi.AGG_SUM, col_a=0),
        dict(kind=abi.AGG_SUM, col_a=1),
        dict(kind=abi.AGG_SUM_PROD2, col_a=1, col_b=2),
        dict(kind=abi.AGG_SUM_PROD3, col_a=1, col_b=2, col_c=3),
        dict(kind=abi.AGG_SUM, col_a=2), dict(kind=abi.AGG_SUM, col_a=3),
        dict(kind=abi.AGG_MIN, col_a=3)])
    _check(eng, h, "q1_nogroup", li.bs, filt, agg, 8, form)


# ---- hand-built tables ----------------------------------------------------

_SCHEMA = [(abi.T_CHAR, 0, 0, 1),           # 0 group
           (abi.T_INT, 0, 19, 8),           # 1 price (the weight)
           (abi.T_DECIMAL_INT, 2, 15, 8),   # 2 disc
           (abi.T_DECIMAL_INT, 2, 15, 8),   # 3 tax
           (abi.T_INT, 0, 19, 8),           # 4 day
           (abi.T_CHAR, 0, 0, 1)]           # 5 second group column
_ENC = [abi.ENC_DICT, abi.ENC_RAW, abi.ENC_DICT, abi.ENC_DICT, abi.ENC_RAW,
        abi.ENC_DICT]

_PLAN = [dict(kind=abi.AGG_COUNT),
         dict(kind=abi.AGG_SUM, col_a=1),
         dict(kind=abi.AGG_SUM_PROD2, col_a=1, col_b=2),
         dict(kind=abi.AGG_SUM_PROD3, col_a=1, col_b=2, col_c=3),
         dict(kind=abi.AGG_SUM, col_a=2),
         dict(kind=abi.AGG_SUM, col_a=3),
         dict(kind=abi.AGG_COUNT, col_a=3),
         dict(kind=abi.AGG_MAX, col_a=2)]


def _bitmap(mask):
    return np.packbits(mask.astype(np.uint8), bitorder="little")


def _encode(cols, nulls=None, schema=_SCHEMA):
    """cols: group bytes, price, disc, tax, day, group2 bytes"""
    g, price, disc, tax, day, g2 = cols
    arrays = [g.astype(np.uint8), price.astype(np.int64).view(np.uint8),
              disc.astype(np.int64).view(np.uint8),
              tax.astype(np.int64).view(np.uint8),
              day.astype(np.int64).view(np.uint8), g2.astype(np.uint8)]
    return oracle.encode_block(oracle.make_schema(schema), arrays, list(_ENC),
                               nulls)


def _blockset(blocks, total, schema=_SCHEMA):
    return _manual_blockset(oracle.make_schema(schema), blocks, total)


# ---- 2. the boundary between the weight field and the count ---------------

# factor columns of scale 0: the products are price x (1 - 1) x (1 + 1), so
# the i64 window bound (largest term x rows per workgroup < 2^62) is far off
# and the packing bound alone decides
_SCHEMA0 = [c if i not in (2, 3) else (abi.T_INT, 0, 19, 8)
            for i, c in enumerate(_SCHEMA)]


def _constant_table(price):
    rows, n_blocks = 512, 8
    one = np.ones(rows, dtype=np.int64)
    blk = _encode([np.full(rows, 65), one * price, one, one, one * 0,
                   np.full(rows, 70)], schema=_SCHEMA0)
    return _blockset([blk] * n_blocks, rows * n_blocks, _SCHEMA0)


@pytest.mark.parametrize("over", [0, 1])
def test_weight_field_boundary(eng, monkeypatch, over):
    """8 blocks x 512 rows under one workgroup: 4,096 rows take 13 bits, the
    weight sum the other 51, so the largest admissible price is 2^39 - 1
    (4,096 x 2^39 = 2^51). One more and the count must not be packed."""
    _env(monkeypatch, 1)
    price = (1 << 39) - 1 + over
    bs = _constant_table(price)
    h = eng.load(bs)
    agg = abi.make_agg([0], _PLAN[:6])
    res = _check(eng, h, ("const", over), bs, None, agg, 6, None)
    rows = abi.result_rows(res, 6)
    assert res.rows_passed == 4096 and len(rows) == 1
    if over:
        assert eng.last_joint() <= 1
    else:
        assert eng.last_joint() >= 2
    eng.free(h)


# ---- 3. dict NULLs on both axes and in a group column ---------------------

_G = np.frombuffer(b"ANR", dtype=np.uint8)
_G2 = np.frombuffer(b"FO", dtype=np.uint8)
_DISC = np.arange(7, dtype=np.int64)            # 0.00 .. 0.06
_TAX = np.arange(7, dtype=np.int64) * 2         # 0.00 .. 0.12
_BLK_ROWS, _N_BLOCKS = 800, 24


def _random_block(rng, rows, day_lo=0, day_hi=1000):
    g = rng.choice(_G, rows)
    g2 = rng.choice(_G2, rows)
    price = rng.integers(90000, 10500000, rows)
    disc = rng.choice(_DISC, rows)
    tax = rng.choice(_TAX, rows)
    day = rng.integers(day_lo, day_hi, rows)
    # every block holds every dict value, in one order: stable dicts
    g[:3], g2[:2], disc[:7], tax[:7] = _G, _G2, _DISC, _TAX
    return [g, price, disc, tax, day, g2]


@pytest.fixture(scope="module")
def null_table(eng):
    """NULLs (dict ref == count) in disc every 7th row, in tax every 5th
    and in the group column every 11th, never in the pinned first rows.
    4 group cells x 8 x 8 refs (7 values and the NULL bucket each) = 256
    joint cells, 2 KB: the largest table that keeps both axes. Grouped by
    both group columns it is 12 cells x 8 x 8 and folds to one axis."""
    rng = np.random.default_rng(77)
    blocks = []
    r = np.arange(_BLK_ROWS)
    for _ in range(_N_BLOCKS):
        cols = _random_block(rng, _BLK_ROWS)
        nulls = [_bitmap((r >= 8) & (r % 11 == 0)), None,
                 _bitmap((r >= 8) & (r % 7 == 0)),
                 _bitmap((r >= 8) & (r % 5 == 0)), None, None]
        blocks.append(_encode(cols, nulls))
    bs = _blockset(blocks, _BLK_ROWS * _N_BLOCKS)
    h = eng.load(bs)
    yield bs, h
    eng.free(h)


@pytest.mark.parametrize("sgrid", [1, 3])
@pytest.mark.parametrize("form", [3, 2, 1])
def test_dict_nulls(eng, null_table, monkeypatch, form, sgrid):
    """COUNT(*) counts the NULL rows; SUM(disc), SUM(tax), COUNT(tax),
    MAX(disc) and both products leave them out, as the oracle does."""
    bs, h = null_table
    _env(monkeypatch, sgrid, pack=form != 1)
    groups = [0, 5] if form == 2 else [0]
    agg = abi.make_agg(groups, _PLAN)
    want = 1 if form == 1 else form
    res = _check(eng, h, ("nulls", len(groups)), bs, None, agg, 8, want)
    assert res.rows_passed == bs.total_rows


# ---- 4. a row filter, with a pruned block and an all-pass block -----------

@pytest.fixture(scope="module")
def filter_table(eng):
    """day <= 499 passes about half the rows of most blocks; block 5 holds
    only days above it (verdict none, skipped), block 9 only days below
    (verdict all: the rows are not tested)."""
    rng = np.random.default_rng(78)
    blocks = []
    for blk in range(_N_BLOCKS):
        lo, hi = {5: (600, 1000), 9: (0, 400)}.get(blk, (0, 1000))
        blocks.append(_encode(_random_block(rng, _BLK_ROWS, lo, hi)))
    bs = _blockset(blocks, _BLK_ROWS * _N_BLOCKS)
    h = eng.load(bs)
    yield bs, h
    eng.free(h)


@pytest.mark.parametrize("sgrid", [1, 3])
def test_mixed_filter(eng, filter_table, monkeypatch, sgrid):
    bs, h = filter_table
    _env(monkeypatch, sgrid)
    filt = abi.make_filter([dict(col=4, op=abi.OP_LE, lo=499)])
    agg = abi.make_agg([0], _PLAN)
    res = _check(eng, h, "filter", bs, filt, agg, 8, 3)
    assert 0.4 * bs.total_rows < res.rows_passed < 0.6 * bs.total_rows


# ---- 5. block tails -------------------------------------------------------

@pytest.mark.parametrize("sgrid", [1, 3])
def test_block_tails(eng, monkeypatch, sgrid):
    """Blocks of 1, 1,023 and 1,025 rows: one below and one above the 1,024
    rows a workgroup covers per sweep iteration. (A one-row block holds one
    dict value per column, and the dicts must be the same in every block,
    so the dict columns are constant here; the prices differ.)"""
    _env(monkeypatch, sgrid)
    rng = np.random.default_rng(79)
    blocks, total = [], 0
    for rows in (1, 1023, 1025, 1025, 1, 1023):
        one = np.ones(rows, dtype=np.int64)
        blocks.append(_encode([
            np.full(rows, 82), rng.integers(1, 1 << 20, rows), one * 4,
            one * 6, one * 0, np.full(rows, 79)]))
        total += rows
    bs = _blockset(blocks, total)
    h = eng.load(bs)
    agg = abi.make_agg([0, 5], _PLAN)
    res = _check(eng, h, ("tails", 0), bs, None, agg, 8, 3)
    assert res.rows_passed == total
    eng.free(h)
