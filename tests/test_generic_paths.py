"""The precompiled generic kernels, variant by variant, against the oracle.

Every JIT-ineligible plan runs these kernels: the fused scan (staged or
unstaged, AND leaves or a combine program), the OBX_PIPELINE_AGG kernel DAG
(k_filter -> k_group_pass -> k_agg_pass), the direct-global growth kernel,
the filter verb's bitmap / row-id kernels and the get_rows decode kernels.

Tables (three int64 value columns, column 0 NULL in every 11th row, and two
1-byte dict group columns with 3 x 2 groups):
  A  6 blocks x 512 rows, RAW values: staged through LDS
  B  4 blocks x 6000 rows, RAW values (the encoder bit-packs them: about
     20 KB per block, past the 17 KB stage buffer): unstaged, three windows
  C  blocks of 2048, 2049 and 4000 rows (the edges of the 2048-row window),
     narrow dict values: staged
  D  as A / B with a 4-byte column, for the decode kernels' 4-byte store
The CPU test pins which of them the engine stages (obx_probe_load_facts), so
the GPU tests know which kernel variant they hit.
"""
import functools

import numpy as np
import pytest

from oceanbase_amd import abi, oracle
from test_engine_host import _probe
from test_group_capacity import _blockset, _make_null_groups

SPECS = [(abi.T_INT, 0, 0, 8)] * 3 + [(abi.T_CHAR, 0, 0, 1)] * 2
D_SPECS = [(abi.T_INT, 0, 0, 8), (abi.T_DATE, 0, 0, 4), (abi.T_CHAR, 0, 0, 1)]


def _every_11th(rows):
    nulls = np.zeros((rows + 7) // 8, dtype=np.uint8)
    for r in range(0, rows, 11):
        nulls[r >> 3] |= 1 << (r & 7)
    return nulls


def _make_windows(block_rows=(2048, 2049, 4000), seed=17):
    rng = np.random.default_rng(seed)
    schema = oracle.make_schema(SPECS)
    blocks = []
    for rows in block_rows:
        cols = [rng.integers(1000, 1016, rows).astype(np.int64).view(np.uint8),
                rng.integers(0, 50, rows).astype(np.int64).view(np.uint8),
                rng.integers(0, 9, rows).astype(np.int64).view(np.uint8),
                (65 + rng.integers(0, 3, rows)).astype(np.uint8),
                (97 + rng.integers(0, 2, rows)).astype(np.uint8)]
        blocks.append(oracle.encode_block(
            schema, cols, [abi.ENC_DICT] * 5,
            [_every_11th(rows), None, None, None, None]))
    return _blockset(schema, blocks, sum(block_rows))


def _make_len4(rows_per_block, n_blocks, seed=19):
    rng = np.random.default_rng(seed)
    schema = oracle.make_schema(D_SPECS)
    blocks = []
    for _ in range(n_blocks):
        rows = rows_per_block
        cols = [rng.integers(-2**40, 2**40, rows).astype(np.int64)
                .view(np.uint8),
                rng.integers(-2**30, 2**30, rows).astype(np.int32)
                .view(np.uint8),
                (65 + rng.integers(0, 5, rows)).astype(np.uint8)]
        blocks.append(oracle.encode_block(
            schema, cols, [abi.ENC_RAW, abi.ENC_RAW, abi.ENC_DICT],
            [_every_11th(rows), _every_11th(rows), None]))
    return _blockset(schema, blocks, rows_per_block * n_blocks)


# name -> (builder, column specs, staged through LDS)
TABLES = {
    "A": (lambda: _make_null_groups(rows_per_block=512, n_blocks=6,
                                    d0=3, d1=2), SPECS, 1),
    "B": (lambda: _make_null_groups(rows_per_block=6000, n_blocks=4,
                                    d0=3, d1=2), SPECS, 0),
    "C": (_make_windows, SPECS, 1),
    "D_staged": (lambda: _make_len4(300, 3), D_SPECS, 1),
    "D_unstaged": (lambda: _make_len4(2400, 2), D_SPECS, 0),
}


@functools.lru_cache(maxsize=None)
def _table(name):
    return TABLES[name][0]()


def _block_bytes(bs, b):
    data, offs = bs._keep
    return bytes(data[int(offs[b]):int(offs[b + 1])]) + b"\x00" * 16


def _block_rows(blk):
    return int(np.frombuffer(blk[16:20], dtype=np.uint32)[0])


CNT = dict(kind=abi.AGG_COUNT)


def _p2(a, b):
    return dict(kind=abi.AGG_SUM_PROD2, col_a=a, col_b=b)


def _p3(a, b, c):
    return dict(kind=abi.AGG_SUM_PROD3, col_a=a, col_b=b, col_c=c)


def _mul(a, b):
    return dict(kind=abi.AGG_SUM_MUL, col_a=a, col_b=b)


# every aggregate kind; the PROD2 + PROD3 pair over the same a and b is fused
PLAN_KINDS = [CNT, dict(kind=abi.AGG_COUNT, col_a=0),
              dict(kind=abi.AGG_SUM, col_a=0), dict(kind=abi.AGG_MIN, col_a=0),
              dict(kind=abi.AGG_MAX, col_a=0), _p2(0, 2), _p3(0, 2, 1),
              _mul(0, 1)]
# a PROD3 with no PROD2 before it, then a PROD2 whose neighbour PROD3 has
# another b: adjacent, not fused
PLAN_PRODS = [CNT, _p3(0, 2, 1), _p2(0, 2), _p3(0, 1, 2), _mul(1, 2),
              dict(kind=abi.AGG_SUM, col_a=1)]
PLANS = {"kinds": PLAN_KINDS, "prods": PLAN_PRODS}


def _agg(plan):
    return abi.make_agg([3, 4], PLANS[plan])


# column 1 holds [0, 50), column 2 [0, 9), column 0 at least 1000 or NULL
FILTERS = {
    "and2": lambda: abi.make_filter([dict(col=1, op=abi.OP_LT, lo=40),
                                     dict(col=2, op=abi.OP_GE, lo=2)]),
    "or": lambda: abi.make_filter(
        [dict(col=1, op=abi.OP_LT, lo=10), dict(col=2, op=abi.OP_GE, lo=6),
         dict(col=0, op=abi.OP_GT, lo=1007)],
        prog=[0, 1, abi.TOK_OR, 2, abi.TOK_AND]),
    # the stored min/max of every block proves these two
    "all": lambda: abi.make_filter([dict(col=1, op=abi.OP_GE, lo=0)]),
    "none": lambda: abi.make_filter([dict(col=1, op=abi.OP_GT, lo=1000)]),
    # ALL by the bounds, but the column's NULL rows still fail
    "all_nullable": lambda: abi.make_filter([dict(col=0, op=abi.OP_GE,
                                                  lo=0)]),
}


@functools.lru_cache(maxsize=None)
def _oracle_agg(table, plan, filt):
    res = oracle.scan_filter_agg(_table(table), FILTERS[filt](), _agg(plan))
    return res.rows_passed, abi.result_rows(res, len(PLANS[plan]))


@functools.lru_cache(maxsize=None)
def _oracle_filter(table, filt):
    """-> (survivor bits over the table's rows, per-block survivor counts,
    per-block ordered block-local row ids)"""
    bs = _table(table)
    schema = oracle.make_schema(TABLES[table][1])
    fd = FILTERS[filt]()
    bits, counts, ids = [], [], []
    for b in range(bs.n_blocks):
        blk = _block_bytes(bs, b)
        bm, pc = oracle.filter_block(schema, bs.n_cols, blk, fd)
        bb = np.unpackbits(bm, bitorder="little")[:_block_rows(blk)]
        assert int(bb.sum()) == pc
        bits.append(bb)
        counts.append(pc)
        ids.append(np.flatnonzero(bb).astype(np.int32))
    return np.concatenate(bits), np.array(counts, dtype=np.uint32), ids


# ---------------------------------------------------------------- CPU ----

@pytest.mark.parametrize("table", sorted(TABLES))
def test_tables_stage_as_the_gpu_tests_assume(table):
    hf, _cols = _probe(_table(table))
    assert hf["lds_ok"] == TABLES[table][2]
    if table == "C":
        assert hf["max_block_rows"] == 4000


def test_oracle_none_filter_has_no_groups():
    for table in "ABC":
        passed, rows = _oracle_agg(table, "kinds", "none")
        assert passed == 0 and rows == []
        passed, rows = _oracle_agg(table, "kinds", "and2")
        assert passed > 0 and len(rows) == 6


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
        eng.handles[table] = eng.load(_table(table))
    return eng.handles[table]


def _check_agg(eng, table, plan, filt):
    res = eng.scan_filter_agg(_handle(eng, table), FILTERS[filt](),
                              _agg(plan))
    assert eng._lib.obx_gpu_last_jit(eng._ctx) == 0
    passed, rows = _oracle_agg(table, plan, filt)
    assert res.rows_passed == passed
    assert abi.result_rows(res, len(PLANS[plan])) == rows
    if filt == "none":
        assert res.rows_passed == 0 and res.n_groups == 0


@pytest.mark.gpu
@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("table", ["A", "B", "C"])
def test_fused_generic_scan(eng, monkeypatch, table, plan, filt):
    """k_scan_filter_agg{,_prog}{,_lds}: A and C staged, B unstaged; the
    "or" filter takes the combine-program kernels."""
    monkeypatch.setenv("OBX_JIT", "0")
    _check_agg(eng, table, plan, filt)


@pytest.mark.gpu
@pytest.mark.parametrize("filt", ["and2", "or"])
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("table", ["A", "B"])
def test_kernel_dag(eng, monkeypatch, table, plan, filt):
    """k_filter -> k_group_pass -> one k_agg_pass per aggregate or fused
    pair."""
    monkeypatch.setenv("OBX_PIPELINE_AGG", "1")
    _check_agg(eng, table, plan, filt)


@pytest.mark.gpu
def test_growth_path_every_kind(eng, monkeypatch):
    """306 groups overflow the LDS table: k_scan_agg_direct, every aggregate
    kind with SUM_MUL and a PROD3 of its own next to the adjacent pair."""
    monkeypatch.setenv("OBX_JIT", "0")
    bs = _make_null_groups()
    filt = abi.make_filter([dict(col=1, op=abi.OP_LT, lo=40)])
    aggs = [dict(kind=abi.AGG_COUNT, col_a=0),
            dict(kind=abi.AGG_SUM, col_a=0), dict(kind=abi.AGG_MAX, col_a=0),
            dict(kind=abi.AGG_MIN, col_a=0), _p2(0, 2), _p3(0, 2, 1),
            _mul(0, 1), _p3(1, 2, 0)]
    agg = abi.make_agg([3, 4], aggs)
    h = eng.load(bs)
    res, rows = eng.scan_filter_agg_paged(h, filt, agg)
    cres, crows = oracle.scan_filter_agg_paged(bs, filt, agg)
    assert res.n_groups == cres.n_groups > 64
    assert res.rows_passed == cres.rows_passed
    assert abi.group_row_tuples(rows, 8) == abi.group_row_tuples(crows, 8)
    eng.free(h)


@pytest.mark.gpu
@pytest.mark.parametrize("want_row_ids", [False, True])
@pytest.mark.parametrize("table", ["A", "B", "C"])
def test_filter_verb_generic(eng, monkeypatch, table, want_row_ids):
    """k_filter{,_prog}{,_lds}: survivor count and bitmap, and with row ids
    the ordered block-local ids and per-block counts. "none" runs after a
    filter with survivors on the same handle: its counts must all be zero."""
    monkeypatch.setenv("OBX_JIT", "0")
    h = _handle(eng, table)
    bs = _table(table)
    rows_of = [_block_rows(_block_bytes(bs, b)) for b in range(bs.n_blocks)]
    starts = np.concatenate([[0], np.cumsum(rows_of)])
    for filt in ("and2", "or", "all", "all_nullable", "and2", "none"):
        bits, counts, ids = _oracle_filter(table, filt)
        got = eng.filter(h, FILTERS[filt](), want_row_ids=want_row_ids)
        assert eng._lib.obx_gpu_last_jit(eng._ctx) == 0
        assert got == int(counts.sum()), filt
        bm = np.unpackbits(eng.fetch_bitmap(h), bitorder="little")
        assert np.array_equal(bm[:bits.size], bits), filt
        if not want_row_ids:
            continue
        got_counts = eng.fetch_blk_counts(h, bs.n_blocks)
        assert np.array_equal(got_counts, counts), filt
        row_ids, _n = eng.fetch_row_ids(h)
        for b in range(bs.n_blocks):
            got_ids = row_ids[starts[b]:starts[b] + counts[b]]
            assert np.array_equal(got_ids, ids[b]), (filt, b)
        if filt == "none":
            assert got == 0 and not got_counts.any()


def _check_decode(eng, table, cols, together):
    """obx_gpu_decode of cols (one call, or one call per column) against the
    oracle's decode_block: datum bytes of non-NULL rows equal, of NULL rows
    zero."""
    bs = _table(table)
    specs = TABLES[table][1]
    schema = oracle.make_schema(specs)
    h = _handle(eng, table)
    if together:
        eng.decode(h, cols)
    for c in cols:
        if not together:
            eng.decode(h, [c])
        ln = specs[c][3]
        gpu = eng.fetch_col(h, c, ln).reshape(-1, ln)
        off = 0
        for b in range(bs.n_blocks):
            rows, outs, nbs = oracle.decode_block(schema, bs.n_cols,
                                                  _block_bytes(bs, b), [c])
            isnull = np.unpackbits(nbs[0], bitorder="little")[:rows] != 0
            got = gpu[off:off + rows]
            want = outs[0].reshape(-1, ln)
            assert np.array_equal(got[~isnull], want[~isnull]), (c, b)
            assert not got[isnull].any(), (c, b)
            off += rows
        assert off == gpu.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("table,cols,together", [
    ("A", [0, 3], False),           # k_decode_lds, datum lengths 8 and 1
    ("B", [0, 3], False),           # k_decode
    ("A", [0, 1, 3, 4], True),      # k_decode_multi
    ("C", [0, 2, 4], True),         # k_decode_multi, 4000-row blocks
    ("D_staged", [1], False),       # 4-byte store, k_decode_lds
    ("D_staged", [0, 1, 2], True),  # 4-byte store, k_decode_multi
    ("D_unstaged", [1, 0], False),  # 4-byte store, k_decode
])
def test_decode_kernels(eng, table, cols, together):
    _check_decode(eng, table, cols, together)
