"""Host engine: load-time column facts and handle lifetime.

CPU half: obx_probe_load_facts runs only the host half of a loader (parse +
the per-block fold of descriptors into column facts, no HIP call) and
reports what every plan / JIT eligibility decision later rests on. The
blocks come from the oracle encoder and the CS block writer, so the expected
facts follow from the encodings requested.

GPU half: a freed handle id is refused by every verb while its neighbours
keep working, and a CS handle keeps the kernel kind and launch grid it had
before the loaders shared their finish step.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oceanbase_amd import abi, cs as obx_cs, oracle  # noqa: E402
from test_cs_block import (  # noqa: E402
    _enc as cs_enc, _int_col as cs_int_col, _str_col as cs_str_col)
from test_gpu_parity import _manual_blockset  # noqa: E402

_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "oceanbase_amd", "libobx.so")

OBX_INVALID_ARGUMENT = -4002

# flag word of a column record (obx_probe_load_facts)
DICT_EVERY, DICT_ANY, DICT_STABLE, GRP16_EVERY = 1, 2, 4, 8
RAW8_EVERY, RANGEFAM_EVERY, EXT_ANY, SLOW_ANY, SPAN_ANY = 16, 32, 64, 128, 256

INT8 = (abi.T_INT, 0, 19, 8)


def _probe(bs, is_cs=False):
    """-> (handle facts dict, [(flags, maxcnt, maxw, cnt_max) per column])"""
    lib = C.CDLL(_SO)
    lib.obx_probe_load_facts.restype = C.c_int
    lib.obx_probe_load_facts.argtypes = [
        C.POINTER(abi.BlockSet), C.c_int, C.POINTER(C.c_uint64),
        C.POINTER(C.c_uint32)]
    hf = (C.c_uint64 * 7)()
    cf = (C.c_uint32 * (4 * bs.n_cols))()
    rc = lib.obx_probe_load_facts(C.byref(bs), 1 if is_cs else 0, hf, cf)
    assert rc == 0, rc
    names = ("n_blocks", "n_cols", "total_rows", "total_bytes", "lds_ok",
             "max_block_rows", "max_block_len")
    return (dict(zip(names, hf)),
            [tuple(cf[4 * c:4 * c + 4]) for c in range(bs.n_cols)])


def _pax(specs, blocks_cols, encs, nulls=None):
    """blocks_cols: per block, one numpy array per column"""
    schema = oracle.make_schema(specs)
    blocks = [oracle.encode_block(schema,
                                  [np.ascontiguousarray(a).view(np.uint8)
                                   for a in cols], encs,
                                  nulls[b] if nulls else None)
              for b, cols in enumerate(blocks_cols)]
    bs = _manual_blockset(schema, blocks)
    bs._schema = schema
    return bs


ROWS = (256, 192, 64)  # three blocks


def _dict3(vals_per_block):
    rng = np.random.default_rng(7)
    out = []
    for rows, vals in zip(ROWS, vals_per_block):
        a = rng.choice(np.asarray(vals, dtype=np.int64), rows)
        a[:len(vals)] = vals  # every value present in every block
        out.append([a])
    return out


def test_facts_stable_numeric_dict():
    bs = _pax([INT8], _dict3([(3, 17, 99)] * 3), [abi.ENC_DICT])
    hf, cols = _probe(bs)
    assert hf["n_blocks"] == 3 and hf["n_cols"] == 1
    assert hf["total_rows"] == sum(ROWS) and hf["max_block_rows"] == 256
    assert hf["total_bytes"] == bs.block_offsets[3]
    assert hf["lds_ok"] == 1
    flags, maxcnt, maxw, cnt_max = cols[0]
    assert flags == DICT_EVERY | DICT_ANY | DICT_STABLE | GRP16_EVERY
    assert maxcnt == 3 and cnt_max == 3
    assert maxw == 2  # three refs bit-pack into two bits


def test_facts_dict_payload_differs_in_one_block():
    bs = _pax([INT8], _dict3([(3, 17, 99), (3, 17, 100), (3, 17, 99)]),
              [abi.ENC_DICT])
    _hf, cols = _probe(bs)
    flags, maxcnt, _maxw, cnt_max = cols[0]
    assert flags == DICT_EVERY | DICT_ANY | GRP16_EVERY  # not DICT_STABLE
    assert maxcnt == 3 and cnt_max == 3


def test_facts_raw8_and_intdiff():
    rng = np.random.default_rng(8)
    blocks = [[rng.integers(-2**62, 2**62, rows, dtype=np.int64),
               rng.integers(1000, 5000, rows, dtype=np.int64)]
              for rows in ROWS]
    bs = _pax([INT8, INT8], blocks, [abi.ENC_RAW, abi.ENC_INT_DIFF])
    _hf, cols = _probe(bs)
    assert cols[0][0] == RAW8_EVERY | RANGEFAM_EVERY
    assert cols[0][2] == 64
    assert cols[1][0] == RANGEFAM_EVERY
    assert cols[1][1] == 0 and cols[1][3] == 0


def test_facts_string_dict():
    rng = np.random.default_rng(9)
    blocks = [[rng.choice(np.frombuffer(b"ANR", dtype=np.uint8), rows)]
              for rows in ROWS]
    bs = _pax([(abi.T_CHAR, 0, 0, 1)], blocks, [abi.ENC_DICT])
    _hf, cols = _probe(bs)
    flags = cols[0][0]
    assert flags & DICT_ANY and flags & SLOW_ANY
    assert not flags & DICT_EVERY
    assert not flags & (RAW8_EVERY | RANGEFAM_EVERY | SPAN_ANY)


def test_facts_column_equal_is_span():
    rng = np.random.default_rng(10)
    blocks = []
    for rows in ROWS:
        a = rng.integers(-2**62, 2**62, rows, dtype=np.int64)
        b = a.copy()
        b[::17] += 1  # exceptions
        blocks.append([a, b])
    bs = _pax([INT8, INT8], blocks, [abi.ENC_RAW, abi.ENC_COLUMN_EQUAL])
    _hf, cols = _probe(bs)
    assert not cols[0][0] & SPAN_ANY
    assert cols[1][0] & SPAN_ANY and cols[1][0] & SLOW_ANY
    assert not cols[1][0] & (DICT_ANY | RAW8_EVERY | RANGEFAM_EVERY)


def test_facts_cs_classes_as_pax():
    """The same integer data as a PAX and as a CS blockset: 8-byte raw, dict
    and an all-null (CONST) column fold to the same classes; only dict
    stability is PAX-only (CS dict payloads exist on the device alone)."""
    rng = np.random.default_rng(11)
    pax_blocks, pax_nulls, cs_blocks = [], [], []
    for rows in ROWS:
        d = rng.choice(np.array([3, 17, 99], dtype=np.int64), rows)
        d[:3] = (3, 17, 99)
        raw = rng.integers(-2**62, 2**62, rows, dtype=np.int64)
        nul = np.zeros(rows, dtype=np.int64)
        pax_blocks.append([raw, d, nul])
        pax_nulls.append([None, None,
                          np.full((rows + 7) // 8, 0xFF, dtype=np.uint8)])
        cs_blocks.append(cs_enc(rows, [
            cs_int_col(raw, enc=1), cs_int_col(d, dict_=True),
            cs_int_col(nul, null_rows=list(range(rows)), dict_=True)]))
    pax = _pax([INT8] * 3, pax_blocks,
               [abi.ENC_RAW, abi.ENC_DICT, abi.ENC_CONST], pax_nulls)
    _hp, pc = _probe(pax)
    schema = oracle.make_schema([INT8] * 3)
    csbs, _keep = obx_cs.make_blockset(cs_blocks, schema)
    hc, cc = _probe(csbs, is_cs=True)
    assert hc["n_blocks"] == 3 and hc["total_rows"] == sum(ROWS)
    assert hc["lds_ok"] == 1 and hc["max_block_rows"] == 256
    assert pc[0][0] == RAW8_EVERY | RANGEFAM_EVERY
    assert pc[1][0] == DICT_EVERY | DICT_ANY | DICT_STABLE | GRP16_EVERY
    assert pc[2][0] == 0 and pc[2][2] == 255  # CONST: no packed stream
    for c in range(3):
        assert cc[c][0] == pc[c][0] & ~DICT_STABLE, c
        assert cc[c][1] == pc[c][1] and cc[c][3] == pc[c][3], c
    assert [c[1] for c in cc] == [0, 3, 0]  # the true maximum on CS too


# ---- GPU ------------------------------------------------------------------

@pytest.fixture
def eng():
    from oceanbase_amd.engine import GpuEngine
    e = GpuEngine(0)
    yield e
    e.close()


def _small_pax():
    rng = np.random.default_rng(12)
    blocks = []
    for _ in range(2):
        g = rng.choice(np.array([3, 17, 99], dtype=np.int64), 256)
        g[:3] = (3, 17, 99)
        blocks.append([g, rng.integers(1, 1000, 256, dtype=np.int64)])
    bs = _pax([INT8, INT8], blocks, [abi.ENC_DICT, abi.ENC_RAW])
    bs.total_rows = 512
    return bs


@pytest.mark.gpu
def test_freed_handle_is_refused(eng):
    bs = _small_pax()
    filt = abi.make_filter([dict(col=1, op=abi.OP_LT, lo=700)])
    agg = abi.make_agg([0], [dict(kind=abi.AGG_COUNT),
                             dict(kind=abi.AGG_SUM, col_a=1)])
    h0, h1 = eng.load(bs), eng.load(bs)
    assert (h0, h1) == (0, 1)
    lib, ctx = eng._lib, eng._ctx
    assert lib.obx_gpu_free_blocks(ctx, h0) == 0

    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    n64, n32 = C.c_uint64(), C.c_uint32()
    res = abi.AggResult()
    row = (abi.GroupRow * 1)()
    proj = (C.c_uint16 * 1)(0)
    lib.obx_gpu_agg_fetch.restype = C.c_int
    lib.obx_gpu_agg_fetch.argtypes = [
        C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p,
        C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    verbs = dict(
        free=lambda: lib.obx_gpu_free_blocks(ctx, h0),
        filter=lambda: lib.obx_gpu_filter(ctx, h0, C.byref(filt), 0),
        filter_rid=lambda: lib.obx_gpu_filter(ctx, h0, C.byref(filt), 1),
        fetch_bitmap=lambda: lib.obx_gpu_fetch_bitmap(ctx, h0, p, 4096),
        fetch_row_ids=lambda: lib.obx_gpu_fetch_row_ids(ctx, h0, p, 1024,
                                                        C.byref(n64)),
        fetch_blk_counts=lambda: lib.obx_gpu_fetch_blk_counts(ctx, h0, p, 2),
        decode=lambda: lib.obx_gpu_decode(ctx, h0, proj, 1),
        fetch_col=lambda: lib.obx_gpu_fetch_col(ctx, h0, 0, p, 4096),
        scan=lambda: lib.obx_gpu_scan_filter_agg(
            ctx, h0, C.byref(filt), C.byref(agg), C.byref(res)),
        agg_fetch=lambda: lib.obx_gpu_agg_fetch(ctx, h0, 0, 1, row,
                                                C.byref(n32), C.byref(n64)),
    )
    for name, call in verbs.items():
        assert call() == OBX_INVALID_ARGUMENT, name
    for getter in ("obx_gpu_total_rows", "obx_gpu_total_bytes",
                   "obx_gpu_last_survivors"):
        assert getattr(lib, getter)(ctx, h0) == 0, getter

    # the neighbour is untouched, and ids are never reused
    res_gpu = eng.scan_filter_agg(h1, filt, agg)
    res_cpu = oracle.scan_filter_agg(bs, filt, agg)
    assert res_gpu.rows_passed == res_cpu.rows_passed
    assert abi.result_rows(res_gpu, 2) == abi.result_rows(res_cpu, 2)
    assert len(abi.result_rows(res_gpu, 2)) == 3
    assert eng.load(bs) == 2


def _cs_pin_table():
    """2 CS blocks x 256 rows: char dict flag and status (a 2-byte group
    key), qty, price, ship date -> (blocks, load specs)"""
    rng = np.random.default_rng(13)
    blocks = []
    for _ in range(2):
        flag = [b"ANR"[x:x + 1] for x in rng.integers(0, 3, 256)]
        flag[:3] = [b"A", b"N", b"R"]
        status = [b"FO"[x:x + 1] for x in rng.integers(0, 2, 256)]
        status[:2] = [b"F", b"O"]
        blocks.append(cs_enc(256, [
            cs_str_col(flag, dict_=True),
            cs_str_col(status, dict_=True),
            cs_int_col(rng.integers(1, 51, 256).astype(np.int64), enc=6),
            cs_int_col(rng.integers(90000, 10**7, 256).astype(np.int64),
                       enc=1),
            cs_int_col(rng.integers(8000, 10600, 256).astype(np.int64),
                       enc=5),
        ]))
    specs = [(abi.T_CHAR, 0, 0, 1)] * 2 + [INT8] * 3
    return blocks, specs


def _cs_pin_plans():
    """-> {name: (filter, agg, n_aggs)}"""
    grouped = (
        abi.make_filter([dict(col=4, op=abi.OP_LE, lo=10471)]),
        abi.make_agg([0, 1], [
            dict(kind=abi.AGG_COUNT),
            dict(kind=abi.AGG_SUM, col_a=2),
            dict(kind=abi.AGG_SUM, col_a=3),
            dict(kind=abi.AGG_SUM_PROD2, col_a=3, col_b=2)]), 4)
    range_sum = (
        abi.make_filter([dict(col=4, op=abi.OP_GE, lo=8500),
                         dict(col=4, op=abi.OP_LT, lo=9500)]),
        abi.make_agg([], [dict(kind=abi.AGG_SUM, col_a=3)]), 1)
    return dict(grouped=grouped, range_sum=range_sum)


# (obx_gpu_last_jit, obx_gpu_last_grid) of a CS handle, read on the commit
# before the loaders shared one finish step. CS group dicts are never
# host-verified stable, so the grouped plan takes the v1 generator (1) on
# the fixed grid (one workgroup per block); the ungrouped sum needs no
# stable dict and takes the persistent kernel (2), never more workgroups
# than blocks.
CS_PINS = dict(grouped=(1, 2), range_sum=(2, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["grouped", "range_sum"])
def test_cs_handle_kernel_choice_pinned(eng, plan):
    import cs_oracle_util as csu
    blocks, specs = _cs_pin_table()
    h = eng.load_cs(blocks, oracle.make_schema(specs))
    filt, agg, n_aggs = _cs_pin_plans()[plan]
    res_gpu = eng.scan_filter_agg(h, filt, agg)
    lib, ctx = eng._lib, eng._ctx
    lib.obx_gpu_last_grid.restype = C.c_uint32
    lib.obx_gpu_last_grid.argtypes = [C.c_void_p]
    got = (lib.obx_gpu_last_jit(ctx), lib.obx_gpu_last_grid(ctx))
    print(f"cs pin {plan}: last_jit={got[0]} last_grid={got[1]}")
    assert got == CS_PINS[plan]
    schema2, pax = csu.to_pax_blocks(blocks, declared_specs=specs)
    res_cpu = oracle.scan_filter_agg(_manual_blockset(schema2, pax), filt, agg)
    assert res_gpu.rows_passed == res_cpu.rows_passed
    assert sorted(abi.result_rows(res_gpu, n_aggs)) == sorted(
        abi.result_rows(res_cpu, n_aggs))
