"""A full global group table with no workgroup past its LDS table.

Each workgroup of the fused scan kernels keeps a 16-slot LDS group table and
flushes it once, at its end, into the 256-slot global table. Tables whose
blocks are clustered by group key (sorted or partitioned on the group column)
can hold more than 256 groups while no block holds more than 16: no LDS table
overflows, and the flush itself has to report the full global table
(counters[1]) so that the host takes the growth path.

The tables: three int64 value columns (column 0 RAW and NULL in every 11th
row) and two 1-byte dict group columns. Block b has one constant g0 and a g1
that cycles over k_b chars, so the group sets of two blocks are disjoint and
the table has sum(k_b) groups. One workgroup scans one block (the launch grid
is the block count up to 4096).
  n255 .. n320   128-row blocks of 8 groups (31x8+7, 32x8, 32x8+1, 40x8):
                 2 x 9 = 18 group cells per block, so no generated kernel
  v256 .. v280   blocks of 7 groups (36x7+4, 36x7+5, 40x7): 2 x 8 = 16 cells,
                 the v1 generated kernel (g0's dict differs from block to
                 block, so the persistent v2 kernel declines)
  wide320        40 x 8 groups, 2400 rows of full-range int64 per block: past
                 the stage buffer, the unstaged kernels
  big            65 g0 chars x 8 windows of 8 g1 chars, one 64-row block per
                 (g0, window): 520 blocks, 4160 groups, past the growth path
The CPU tests pin these preconditions; every GPU result is compared with
oracle.scan_filter_agg_paged on the same blockset, bit for bit.

The join scan has the same flush: its tables give every block a key subset of
its own, which the map sends to payload values of that block's own.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oceanbase_amd import abi, oracle
from test_engine_host import DICT_STABLE, GRP16_EVERY, SLOW_ANY, _probe
from test_generic_paths import (CNT, FILTERS, PLAN_KINDS, SPECS, _every_11th,
                                _mul, _p2, _p3)
from test_group_capacity import _blockset
from test_keymap import (CH, DENSE, HASH, INT4, J, K, MIXED_AGGS, OR_LEAVES,
                         OR_PROG, PAY, Case, check_join, oracle_rows)
from test_scan_flush_source import _lib as _dump_lib

LTABLE_SLOTS, GTABLE_SLOTS, STAGE_BYTES = 16, 256, 17408


# ---- the clustered tables -------------------------------------------------

def _per_block(ks):
    """block b: g0 = chr(33 + b), g1 cycles over k_b chars from 'a'"""
    return [(33 + b, [97 + j for j in range(k)]) for b, k in enumerate(ks)]


def _big_blocks():
    return [(33 + a, [33 + 8 * w + j for j in range(8)])
            for a in range(65) for w in range(8)]


def _build(blocks, rows=128, wide=False, seed=5):
    """-> (blockset, g0 and g1 of every row, rows per block). The rows of the
    second and third g1 cycle of a block pass every filter used here unless
    column 0 is NULL there, which it is in at most one of a group's two."""
    rng = np.random.default_rng(seed)
    schema = oracle.make_schema(SPECS)
    enc = [abi.ENC_RAW] * 3 + [abi.ENC_DICT] * 2
    out, g0s, g1s = [], [], []
    r = np.arange(rows)
    for g0c, g1cs in blocks:
        k = len(g1cs)
        assert 3 * k <= rows and k % 11
        if wide:
            v0 = rng.integers(-2**62, 2**62, rows).astype(np.int64)
        else:
            v0 = rng.integers(1000, 5000, rows).astype(np.int64)
        v1 = rng.integers(0, 50, rows).astype(np.int64)
        v2 = rng.integers(0, 9, rows).astype(np.int64)
        sure = (r >= k) & (r < 3 * k)
        v0[sure] = 2000 + r[sure]
        v1[sure] = 3
        v2[sure] = 7
        g0 = np.full(rows, g0c, dtype=np.uint8)
        g1 = np.asarray(g1cs, dtype=np.uint8)[r % k]
        out.append(oracle.encode_block(
            schema, [v0.view(np.uint8), v1.view(np.uint8), v2.view(np.uint8),
                     g0, g1], enc, [_every_11th(rows), None, None, None, None]))
        g0s.append(g0)
        g1s.append(g1)
    bs = _blockset(schema, out, rows * len(blocks))
    return bs, np.concatenate(g0s), np.concatenate(g1s), rows


# name -> (groups per block or the block list, builder arguments, staged)
TABLES = {
    "n255": ([8] * 31 + [7], {}, 1),
    "n256": ([8] * 32, {}, 1),
    "n257": ([8] * 32 + [1], {}, 1),
    "n320": ([8] * 40, {}, 1),
    "v256": ([7] * 36 + [4], {}, 1),
    "v257": ([7] * 36 + [5], {}, 1),
    "v280": ([7] * 40, {}, 1),
    "wide320": ([8] * 40, dict(rows=2400, wide=True), 0),
    "big": (None, dict(rows=64), 1),
}
N_GROUPS = dict(n255=255, n256=256, n257=257, n320=320, v256=256, v257=257,
                v280=280, wide320=320, big=4160)


@functools.lru_cache(maxsize=None)
def _table(name):
    ks, kw, _staged = TABLES[name]
    return _build(_big_blocks() if ks is None else _per_block(ks), **kw)


AND = abi.make_filter([dict(col=1, op=abi.OP_LT, lo=40)])
V1_KINDS = [CNT, dict(kind=abi.AGG_COUNT, col_a=0),
            dict(kind=abi.AGG_SUM, col_a=0), _p2(0, 2), _p3(0, 2, 1),
            _mul(0, 1)]
PLANS = {"kinds": PLAN_KINDS, "v1": V1_KINDS,
         "small": [CNT, dict(kind=abi.AGG_SUM, col_a=0)]}


def _filter(name):
    return AND if name == "and" else FILTERS[name]()


def _agg(plan):
    return abi.make_agg([3, 4], PLANS[plan])


@functools.lru_cache(maxsize=None)
def _oracle(table, plan, filt):
    """-> (n_groups, rows_passed, group row tuples), computed once"""
    res, rows = oracle.scan_filter_agg_paged(_table(table)[0], _filter(filt),
                                             _agg(plan))
    assert res.n_groups == len(rows)
    return (res.n_groups, res.rows_passed,
            abi.group_row_tuples(rows, len(PLANS[plan])))


# ---------------------------------------------------------------- CPU ----

@pytest.mark.parametrize("table", sorted(TABLES))
def test_blocks_fit_the_lds_table_and_the_total_is_exact(table):
    _bs, g0, g1, rows = _table(table)
    pair = g0.astype(np.uint32) << 8 | g1
    per_block = [len(np.unique(pair[r0:r0 + rows]))
                 for r0 in range(0, len(pair), rows)]
    assert max(per_block) <= LTABLE_SLOTS
    assert len(np.unique(pair)) == sum(per_block) == N_GROUPS[table]
    filters = ("and",) if table in ("wide320", "big") else ("and", "or")
    plan = "small" if table == "big" else "kinds"
    for filt in filters:
        n_groups, passed, tuples = _oracle(table, plan, filt)
        assert n_groups == N_GROUPS[table]
        assert 0 < passed < len(pair)
        assert sum(t[1] for t in tuples) == passed


@pytest.mark.parametrize("table", sorted(TABLES))
def test_load_facts_pick_the_kernel(table):
    bs = _table(table)[0]
    hf, cols = _probe(bs)
    assert hf["lds_ok"] == TABLES[table][2]
    if table == "wide320":
        assert hf["max_block_len"] > STAGE_BYTES
    for c in (3, 4):
        assert cols[c][0] & GRP16_EVERY
    # g0's one dict entry differs from block to block: no persistent kernel
    assert not cols[3][0] & DICT_STABLE and cols[3][3] == 1
    for c in (0, 1, 2):
        assert not cols[c][0] & SLOW_ANY
    cells = (cols[3][3] + 1) * (cols[4][3] + 1)
    if table.startswith("v"):
        assert cells <= 16        # jit_pair_cells_max: v1 takes the plan
    else:
        assert cells > 16         # no generated kernel


def _v1_source():
    """the v1 generator's text for a plan of the v tables' shape"""
    n = 5
    cols = (abi.ColSchema * n)()
    for c in range(n):
        cols[c].obj_type = abi.T_INT
        cols[c].len = 8 if c < 3 else 1
    # 1 dict in every block, 2 may be NULL, 4 bounds known, 8 aligned 8-byte
    # RAW, 16 packed-range family
    flags = (C.c_uint8 * n)(2 | 4 | 8, 4 | 16, 4 | 16, 1 | 4, 1 | 4)
    cmin = (C.c_int64 * n)(1000, 0, 0, 33, 97)
    cmax = (C.c_int64 * n)(5000, 49, 8, 73, 103)
    maxcnt = (C.c_uint32 * n)(0, 0, 0, 1, 7)
    maxw = (C.c_uint32 * n)(64, 6, 4, 1, 3)
    buf = C.create_string_buffer(1 << 20)
    agg = _agg("v1")
    sz = _dump_lib().obx_jit_dump_src_ex(
        C.byref(AND), C.byref(agg), cols, n, flags, cmin, cmax, maxcnt, maxw,
        128, 1, 40, 0, None, buf, len(buf))
    assert sz > 0
    return buf.raw[:sz].decode()


def test_v1_final_flush_reports_a_full_table():
    src = _v1_source()
    assert "jtab_t" in src                     # the v1 kernel
    mark = "/* flush the LDS table to the global table */"
    assert src.count(mark) == 1
    flush = src[src.index(mark):]
    assert "atomicAdd(&counters[1]" in flush
    # a slot without a place in the global table accumulates nowhere
    assert flush.index("atomicAdd(&counters[1]") < flush.index(
        "atomicAdd(&gtable[idx].count")


# ---------------------------------------------------------------- GPU ----

@pytest.fixture(scope="module")
def eng():
    from oceanbase_amd.engine import GpuEngine
    e = GpuEngine(0)
    e.handles = {}
    yield e
    e.close()


def _handle(eng, table):
    if table not in eng.handles:
        eng.handles[table] = eng.load(_table(table)[0])
    return eng.handles[table]


def _scan(eng, table, plan, filt):
    """-> (status, AggResult); the rows stay behind obx_gpu_agg_fetch"""
    res = abi.AggResult()
    f, a = _filter(filt), _agg(plan)
    rc = eng._lib.obx_gpu_scan_filter_agg(eng._ctx, _handle(eng, table),
                                          C.byref(f), C.byref(a), C.byref(res))
    return rc, res


def _check_equal(eng, table, plan, filt, jit):
    rc, res = _scan(eng, table, plan, filt)
    assert eng._lib.obx_gpu_last_jit(eng._ctx) == jit
    n_groups, passed, tuples = _oracle(table, plan, filt)
    got = abi.group_row_tuples(eng.agg_fetch_all(_handle(eng, table)),
                               len(PLANS[plan]))
    print(f"{table} {plan} {filt}: rc={rc} n_groups={res.n_groups} "
          f"(oracle {n_groups}) rows_passed={res.rows_passed} "
          f"(oracle {passed}) fetched={len(got)}")
    assert rc == abi.OBX_BUF_NOT_ENOUGH      # more than the 64 inline rows
    assert res.n_groups == n_groups
    assert res.rows_passed == passed
    assert got == tuples


def _check_refused(eng, table, plan, filt):
    """a clean capacity error, nothing to fetch, and the handle still works"""
    rc, _res = _scan(eng, table, plan, filt)
    h = _handle(eng, table)
    fetched = eng.agg_fetch_all(h)
    print(f"{table} {plan} {filt}: rc={rc} fetched={len(fetched)}")
    assert rc == abi.OBX_BUF_NOT_ENOUGH
    assert fetched == []
    res = eng.scan_filter_agg(h, _filter(filt), abi.make_agg([], [CNT]))
    assert res.rows_passed == _oracle(
        table, "small" if table == "big" else "kinds", filt)[1]
    assert abi.result_rows(res, 1) == [(b"", res.rows_passed,
                                        [res.rows_passed])]


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["n255", "n256", "n257", "n320"])
def test_fused_generic_staged(eng, monkeypatch, table):
    """k_scan_filter_agg_lds, every aggregate kind"""
    monkeypatch.setenv("OBX_JIT", "0")
    _check_equal(eng, table, "kinds", "and", jit=0)


@pytest.mark.gpu
def test_fused_generic_unstaged(eng, monkeypatch):
    """k_scan_filter_agg: blocks past the stage buffer"""
    monkeypatch.setenv("OBX_JIT", "0")
    _check_equal(eng, "wide320", "kinds", "and", jit=0)


@pytest.mark.gpu
def test_combine_program_table_just_full(eng, monkeypatch):
    """k_scan_filter_agg_prog_lds: 256 groups fill the table, none is left"""
    monkeypatch.setenv("OBX_JIT", "0")
    _check_equal(eng, "n256", "kinds", "or", jit=0)


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["n257", "n320"])
def test_combine_program_past_the_table(eng, monkeypatch, table):
    """the growth path is AND-only: a combine program keeps the capacity
    error"""
    monkeypatch.setenv("OBX_JIT", "0")
    _check_refused(eng, table, "kinds", "or")


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["n255", "n256", "n320"])
def test_kernel_dag(eng, monkeypatch, table):
    """k_filter -> k_group_pass -> k_agg_pass: slot 255 does not fit the u8
    row map, so 256 groups already take the growth path"""
    monkeypatch.setenv("OBX_PIPELINE_AGG", "1")
    _check_equal(eng, table, "kinds", "and", jit=0)


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["v256", "v257", "v280"])
def test_v1_generated_kernel(eng, table):
    _check_equal(eng, table, "v1", "and", jit=1)


@pytest.mark.gpu
def test_more_than_4096_clustered_groups(eng, monkeypatch):
    """4160 groups, 8 per block: past the growth path's table as well"""
    monkeypatch.setenv("OBX_JIT", "0")
    _check_refused(eng, "big", "small", "and")


# ---- the join scan --------------------------------------------------------

JOIN_BLOCKS = 40
JOIN_AGGS = MIXED_AGGS + [dict(kind=abi.AGG_SUM, col_a=J),
                          dict(kind=abi.AGG_MAX, col_a=J)]


def _clustered_join(per_block):
    """block b draws its probe keys from 100 keys of its own; 60 of them are
    map keys, sent to per_block payload values of that block's own. The first
    60 rows of a block hold its map keys once each, under the chars x, y, z
    in turn: every (payload, char) pair of the block joins."""
    def edit(cs, cols, block_rows):
        rng = np.random.default_rng(23)
        dom = 10**9 + np.arange(50_000)
        keys, pays, r0 = [], [], 0
        for b, rows in enumerate(block_rows):
            own = dom[100 * b:100 * b + 100]
            keys.append(own[:60])
            pays.append(per_block * b + np.arange(60) % per_block)
            cols[K][r0:r0 + rows] = rng.choice(own, rows)
            cols[K][r0:r0 + 60] = own[:60]
            cols[CH][r0:r0 + 60, 0] = np.frombuffer(b"xyz", np.uint8)[
                np.arange(60) % 3]
            r0 += rows
        cs.map_keys = np.concatenate(keys).astype(np.int64)
        cs.spec = INT4
        cs.map_pay = np.concatenate(pays).astype(np.int32)
    return edit


@functools.lru_cache(maxsize=None)
def _join_case(per_block):
    c = Case((128,) * JOIN_BLOCKS, seed=14, edit=_clustered_join(per_block))
    assert max(c.block_bytes()) <= STAGE_BYTES
    return c


def _join_groups_per_block(c, with_char):
    pay = c.table.columns[PAY][2].astype(np.int64)
    key = pay * 256 + (c.cols[CH][:, 0] if with_char else 0)
    out, r0 = [], 0
    for rows in c.table.block_rows:
        out.append(len(np.unique(key[r0:r0 + rows][c.hit[r0:r0 + rows]])))
        r0 += rows
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("per_block,group,kind", [
    (8, [J], HASH), (8, [J], DENSE), (5, [J, CH], HASH)])
def test_join_scan_clustered_payloads(eng, per_block, group, kind):
    c = _join_case(per_block)
    per = _join_groups_per_block(c, len(group) == 2)
    n = JOIN_BLOCKS * per_block * (3 if len(group) == 2 else 1)
    assert max(per) <= LTABLE_SLOTS and sum(per) == n > GTABLE_SLOTS
    h = eng.load(c.table.bs)
    mid = c.create(eng, kind)
    try:
        assert eng.keymap_info(mid).kind == kind
        check_join(eng, h, c, mid, group, JOIN_AGGS, groups=(n, n))
    finally:
        eng.keymap_free(mid)
        eng.free(h)


@pytest.mark.gpu
def test_join_scan_combine_program_past_the_table(eng):
    c = _join_case(8)
    _want, rows = oracle_rows(c, OR_LEAVES, OR_PROG, [J], JOIN_AGGS)
    assert GTABLE_SLOTS < len(rows) <= 8 * JOIN_BLOCKS
    h = eng.load(c.table.bs)
    mid = c.create(eng, HASH)
    try:
        rc, _ = eng._scan_join_agg(h, abi.make_filter(OR_LEAVES, OR_PROG),
                                   mid, K, abi.make_agg([J], JOIN_AGGS))
        fetched = eng.agg_fetch_all(h)
        print(f"join or: rc={rc} fetched={len(fetched)} oracle={len(rows)}")
        assert rc == abi.OBX_BUF_NOT_ENOUGH
        assert fetched == []
        # a small plan on the same handle still succeeds
        check_join(eng, h, c, mid, [CH], MIXED_AGGS, groups=(3, 3))
    finally:
        eng.keymap_free(mid)
        eng.free(h)
