"""Filtered projection: obx_gpu_scan_project decodes only the filter's
survivors into dense vectors (get_rows(row_ids) for a whole scan range), and
obx_gpu_fetch_proj / obx_gpu_fetch_proj_row_nos page the result out.

Reference: per block, oracle.filter_block gives the survivor bits and
oracle.decode_block the datums and LSB-first null bitmaps; the survivors are
concatenated in table order and the datum bytes of NULL rows zeroed. Every
comparison is bit-exact: datums, null bits, row numbers, n_rows.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oceanbase_amd import abi, oracle  # noqa: E402
import pymodel  # noqa: E402
from test_cs_block import (  # noqa: E402
    _enc as cs_enc, _dec as cs_dec, _get_int as cs_get_int,
    _int_col as cs_int_col, CA_HAS_NULL_BITMAP)
from test_gpu_parity import _manual_blockset  # noqa: E402

_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "oceanbase_amd", "libobx.so")

OBX_INVALID_ARGUMENT = -4002
OBX_BUF_NOT_ENOUGH = -4009

INT8 = (abi.T_INT, 0, 19, 8)
DATE4 = (abi.T_DATE, 0, 0, 4)


# ---- reference ------------------------------------------------------------

def _bits(packed, n):
    """LSB-first packed bytes -> bool array of n"""
    return np.unpackbits(np.asarray(packed, dtype=np.uint8),
                         bitorder="little")[:n].astype(bool)


def _pack(flags):
    return np.packbits(np.asarray(flags, dtype=np.uint8), bitorder="little")


class Ref:
    """n_rows, row_nos (uint64), and per column c: datums[c] (n_rows x len
    uint8, NULL rows zeroed), nulls[c] (bool)"""


def reference(schema, blocks, filt, cols):
    n_cols = len(schema)
    cols = sorted(set(cols))
    datums = {c: [] for c in cols}
    nulls = {c: [] for c in cols}
    row_nos, row0 = [], 0
    for blk in blocks:
        rows, outs, nbs = oracle.decode_block(schema, n_cols, blk, cols)
        if filt is None:
            keep = np.ones(rows, dtype=bool)
        else:
            bits, passed = oracle.filter_block(schema, n_cols, blk, filt)
            keep = _bits(bits, rows)
            assert int(keep.sum()) == passed
        for c, o, nb in zip(cols, outs, nbs):
            isn = _bits(nb, rows)
            d = o.reshape(rows, schema[c].len).copy()
            d[isn] = 0
            datums[c].append(d[keep])
            nulls[c].append(isn[keep])
        row_nos.append(row0 + np.nonzero(keep)[0].astype(np.uint64))
        row0 += rows
    ref = Ref()
    ref.row_nos = np.concatenate(row_nos)
    ref.n_rows = len(ref.row_nos)
    ref.total_rows = row0
    ref.datums = {c: np.concatenate(datums[c]) for c in cols}
    ref.nulls = {c: np.concatenate(nulls[c]) for c in cols}
    return ref


# ---- the boundary table ---------------------------------------------------

B_ROWS = [1, 63, 64, 65, 257, 1000, 1500, 1024, 700]
B_SPECS = [INT8, DATE4, (abi.T_CHAR, 0, 0, 3), INT8]
B_ENCS = [abi.ENC_RAW, abi.ENC_INT_DIFF, abi.ENC_DICT, abi.ENC_RAW]
B_WORDS = np.array([b"abc", b"abd", b"xyz", b"q  ", b"ZZZ"], dtype="S3")


def _null_every_5th(rows):
    """rows 4, 9, ...: a one-row block keeps a value, which the INT_DIFF
    writer needs"""
    return np.arange(rows) % 5 == 4


def _mixed_block(rng, rows, key):
    """source arrays of one block of the 4-column layout:
    -> ([key, date, char3, big], [null flags or None per column])"""
    date = (9000 + rng.integers(0, 2000, rows)).astype(np.int32)
    word = rng.choice(B_WORDS, rows)
    big = rng.integers(-2**40, 2**40, rows).astype(np.int64)
    nul = _null_every_5th(rows)
    return [key.astype(np.int64), date, word, big], [None, nul, None, nul]


def _encode(specs, encs, src_blocks):
    schema = oracle.make_schema(specs)
    blocks = []
    for arrays, nulls in src_blocks:
        raw = [np.ascontiguousarray(a).view(np.uint8).reshape(-1)
               for a in arrays]
        nbs = [None if n is None else _pack(n) for n in nulls]
        blocks.append(oracle.encode_block(schema, raw, encs, nbs))
    return schema, blocks


class Table:
    def __init__(self, specs, encs, src_blocks):
        self.specs, self.src = specs, src_blocks
        self.schema, self.blocks = _encode(specs, encs, src_blocks)
        self.bs = _manual_blockset(self.schema, self.blocks)
        self.bs.total_rows = sum(len(a[0][0]) for a in src_blocks)

    def len(self, c):
        return self.specs[c][3]


def _boundary_src():
    rng = np.random.default_rng(5)
    src = []
    for b, rows in enumerate(B_ROWS):
        if b in (0, 3, 6):
            key = 100000 + rng.integers(0, 1000, rows)
        elif b == 4:
            key = np.full(rows, 5)
        else:
            key = rng.integers(0, 1000, rows)
        src.append(_mixed_block(rng, rows, key))
    return src


_cache = {}


def boundary():
    """(Table, filter key < 500, its reference over columns 1, 2, 3),
    built once and shared; nothing changes them"""
    if "b" not in _cache:
        t = Table(B_SPECS, B_ENCS, _boundary_src())
        filt = abi.make_filter([dict(col=0, op=abi.OP_LT, lo=500)])
        _cache["b"] = (t, filt, reference(t.schema, t.blocks, filt,
                                          [0, 1, 2, 3]))
    return _cache["b"]


# ---- the encoding tables --------------------------------------------------

E_ROWS = [700, 1300, 257]
EI_SPECS = [INT8] * 6
EI_ENCS = [abi.ENC_RAW, abi.ENC_DICT, abi.ENC_RLE, abi.ENC_CONST,
           abi.ENC_INT_DIFF, abi.ENC_COLUMN_EQUAL]
# a span column refers to a plain one (one level only): both the substring
# (column 4) and the equal column (5) refer to the prefix column (3)
EC_SPECS = ([(abi.T_CHAR, 0, 0, 4)] * 4 +
            [(abi.T_CHAR, 0, 0, 2), (abi.T_CHAR, 0, 0, 4), INT8])
EC_ENCS = [abi.ENC_RAW, abi.ENC_SDIFF, abi.ENC_HEX, abi.ENC_STRING_PREFIX,
           abi.ENC_COLUMN_SUBSTR, abi.ENC_COLUMN_EQUAL, abi.ENC_RAW]


def _int_enc_src():
    rng = np.random.default_rng(21)
    src = []
    for rows in E_ROWS:
        r = np.arange(rows)
        raw = rng.integers(0, 1000, rows)               # bit-packs to 10 bits
        dic = rng.choice(np.array([3, -11, 42, 2**41]), rows)
        rle = np.repeat(rng.integers(-50, 50, rows // 40 + 1), 40)[:rows]
        con = np.full(rows, 777)
        exc = rng.choice(rows, rows // 20, replace=False)
        con[exc] = rng.integers(-1000, 1000, len(exc))
        con_null = np.zeros(rows, dtype=bool)
        con_null[exc[::3]] = True                       # NULL exceptions
        dif = 10**12 + rng.integers(0, 5000, rows)
        dif_null = r % 7 == 3
        equ = dif.copy()
        equ[::17] += 1                                  # value exceptions
        equ_null = dif_null.copy()
        equ_null[5::29] ^= True                         # null-ness exceptions
        src.append(([a.astype(np.int64) for a in
                     (raw, dic, rle, con, dif, equ)],
                    [r % 11 == 0, r % 6 == 1, r % 9 == 2, con_null, dif_null,
                     equ_null]))
    return src


def _char4(rng, rows):
    a = np.empty((rows, 4), dtype=np.uint8)
    a[:, 0], a[:, 2] = ord("A"), ord("B")
    a[:, 1] = rng.choice(np.frombuffer(b"abcdefgh", dtype=np.uint8), rows)
    a[:, 3] = rng.choice(np.frombuffer(b"0123", dtype=np.uint8), rows)
    return a


def _char_enc_src():
    rng = np.random.default_rng(22)
    src = []
    for rows in E_ROWS:
        r = np.arange(rows)
        base, sdiff, hexp, pref = (_char4(rng, rows) for _ in range(4))
        pref_null = r % 8 == 5
        equ = pref.copy()
        equ[::19, 1] = ord("z")                         # value exceptions
        equ_null = pref_null.copy()
        equ_null[3::31] ^= True
        sub = pref[:, 1:3].copy()                       # slice [1, 3) of pref
        sub[::23, 0] = ord("Q")
        sub_null = pref_null.copy()
        sub_null[7::37] ^= True
        key = rng.integers(0, 1000, rows).astype(np.int64)
        src.append(([base, sdiff, hexp, pref, sub, equ, key],
                    [None, r % 10 == 0, r % 12 == 7, pref_null, sub_null,
                     equ_null, None]))
    return src


def _src_expect(table, keep_blocks, c):
    """the reference's output for column c recomputed from the source
    arrays alone: (datums n x len, nulls)"""
    ds, ns = [], []
    for (arrays, nulls), keep in zip(table.src, keep_blocks):
        rows = len(keep)
        d = np.ascontiguousarray(arrays[c]).view(np.uint8).reshape(
            rows, table.len(c)).copy()
        isn = (np.zeros(rows, dtype=bool) if nulls[c] is None
               else np.asarray(nulls[c]))
        d[isn] = 0
        ds.append(d[keep])
        ns.append(isn[keep])
    return np.concatenate(ds), np.concatenate(ns)


# ---- CPU tests ------------------------------------------------------------

def test_exports_and_bindings():
    lib = C.CDLL(_SO)
    for name in ("obx_gpu_scan_project", "obx_gpu_fetch_proj",
                 "obx_gpu_fetch_proj_row_nos"):
        assert getattr(lib, name, None) is not None, name
    from oceanbase_amd.engine import GpuEngine
    for name in ("scan_project", "fetch_proj", "fetch_proj_row_nos"):
        assert callable(getattr(GpuEngine, name, None)), name


def test_reference_matches_numpy_on_boundary_table():
    t, _filt, ref = boundary()
    keeps = [np.asarray(arrays[0]) < 500 for arrays, _ in t.src]
    want_nos = np.nonzero(np.concatenate(keeps))[0].astype(np.uint64)
    assert ref.total_rows == sum(B_ROWS)
    assert ref.n_rows == len(want_nos) and 0 < ref.n_rows < ref.total_rows
    assert np.array_equal(ref.row_nos, want_nos)
    for c in range(4):
        d, isn = _src_expect(t, keeps, c)
        assert np.array_equal(ref.datums[c], d), c
        assert np.array_equal(ref.nulls[c], isn), c
    assert ref.nulls[1].any() and ref.nulls[3].any()
    per_block = [int(k.sum()) for k in keeps]
    assert sum(1 for n in per_block if n == 0) >= 2 and per_block[0] == 0
    assert any(n == rows for n, rows in zip(per_block, B_ROWS))


@pytest.mark.parametrize("which", ["int", "char"])
def test_encoding_tables_carry_the_requested_encodings(which):
    """The every-encoding GPU test means what it says only if the writer
    kept each requested encoding; and the reference over those blocks
    equals the source arrays."""
    specs, encs, src = ((EI_SPECS, EI_ENCS, _int_enc_src()) if which == "int"
                        else (EC_SPECS, EC_ENCS, _char_enc_src()))
    t = Table(specs, encs, src)
    for blk in t.blocks:
        hdrs = pymodel.Block(blk[:-16], specs).col_headers
        assert [h["type"] for h in hdrs] == encs
        if which == "int":
            assert hdrs[0]["attr"] & 0x4  # RAW column is bit-packed
    ref = reference(t.schema, t.blocks, None, list(range(len(specs))))
    keeps = [np.ones(len(a[0][0]), dtype=bool) for a in src]
    for c in range(len(specs)):
        d, isn = _src_expect(t, keeps, c)
        assert np.array_equal(ref.datums[c], d), c
        assert np.array_equal(ref.nulls[c], isn), c


# ---- GPU tests ------------------------------------------------------------

@pytest.fixture(scope="module")
def eng():
    from oceanbase_amd.engine import GpuEngine
    e = GpuEngine(0)
    yield e
    e.close()


def _check_window(eng, h, t, ref, cols, start, count):
    """every projected position's window against the reference slice"""
    end = min(ref.n_rows, start + count) if count is not None else ref.n_rows
    n = max(0, end - start)
    for p, c in enumerate(cols):
        got, got_nulls = eng.fetch_proj(h, p, t.len(c), start, count)
        assert got.size == n * t.len(c), (p, c, start, count)
        assert np.array_equal(got.reshape(n, t.len(c)),
                              ref.datums[c][start:start + n]), (p, c, start)
        assert np.array_equal(got_nulls, _pack(ref.nulls[c][start:start + n])
                              ), (p, c, start)


def _check(eng, h, t, filt, cols, ref=None, row_nos=False):
    ref = ref or reference(t.schema, t.blocks, filt, cols)
    n = eng.scan_project(h, filt, cols, want_row_nos=row_nos)
    assert n == ref.n_rows
    _check_window(eng, h, t, ref, cols, 0, None)
    if row_nos:
        assert np.array_equal(eng.fetch_proj_row_nos(h), ref.row_nos)
    return ref


@pytest.fixture(scope="module")
def btable(eng):
    t, filt, ref = boundary()
    h = eng.load(t.bs)
    yield t, filt, ref, h
    eng.free(h)


@pytest.mark.gpu
def test_boundary_table_whole_and_windows(eng, btable):
    t, filt, ref, h = btable
    cols = [1, 2, 3]
    n = eng.scan_project(h, filt, cols, want_row_nos=True)
    print(f"boundary table: {n} survivors of {ref.total_rows}")
    assert n == ref.n_rows
    _check_window(eng, h, t, ref, cols, 0, None)
    # windows off a byte boundary, across block boundaries, a short last one
    start = 5
    for count in (77, 3, 1000, 64, 1 << 40):
        _check_window(eng, h, t, ref, cols, start, count)
        start += min(count, max(0, n - start))
    assert start == n
    _check_window(eng, h, t, ref, cols, n - 3, 77)   # short last window
    _check_window(eng, h, t, ref, cols, n, 10)       # at the end: nothing
    _check_window(eng, h, t, ref, cols, n + 99, 10)
    nos = eng.fetch_proj_row_nos(h)
    assert np.all(np.diff(nos.astype(np.int64)) > 0)
    assert np.array_equal(nos, ref.row_nos)
    assert np.array_equal(eng.fetch_proj_row_nos(h, 5, 77),
                          ref.row_nos[5:82])
    assert eng.fetch_proj_row_nos(h, n, 4).size == 0


@pytest.mark.gpu
def test_buffer_and_argument_refusals(eng, btable):
    t, filt, ref, h = btable
    lib, ctx = eng._lib, eng._ctx
    assert eng.scan_project(h, filt, [1, 3]) == ref.n_rows
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    n64 = C.c_uint64()
    fetch = lib.obx_gpu_fetch_proj
    # 10 date datums need 40 bytes and 2 bytes of null bits
    assert fetch(ctx, h, 0, 0, 10, p, 39, p, 2, C.byref(n64)) == \
        OBX_BUF_NOT_ENOUGH
    assert fetch(ctx, h, 0, 0, 10, p, 40, p, 1, C.byref(n64)) == \
        OBX_BUF_NOT_ENOUGH
    assert fetch(ctx, h, 0, 0, 10, p, 40, p, 2, C.byref(n64)) == 0
    assert n64.value == 10
    assert fetch(ctx, h, 2, 0, 10, p, 4096, p, 4096, C.byref(n64)) == \
        OBX_INVALID_ARGUMENT  # proj_idx >= n_proj
    # row numbers were not requested
    assert lib.obx_gpu_fetch_proj_row_nos(ctx, h, 0, 10, p, 10,
                                          C.byref(n64)) == OBX_INVALID_ARGUMENT
    arr = (C.c_uint16 * 9)(*([1] * 9))
    scan = lib.obx_gpu_scan_project
    for bad_n in (0, 9):
        assert scan(ctx, h, C.byref(filt), arr, bad_n, 0, C.byref(n64)) == \
            OBX_INVALID_ARGUMENT
    assert eng.scan_project(h, filt, [1, 3], want_row_nos=True) == ref.n_rows
    assert lib.obx_gpu_fetch_proj_row_nos(ctx, h, 0, 10, p, 9,
                                          C.byref(n64)) == OBX_BUF_NOT_ENOUGH


@pytest.mark.gpu
def test_no_filter_equals_full_decode_and_adds_null_bits(eng, btable):
    t, _filt, _ref, h = btable
    cols = [1, 2, 3, 0]
    ref = _check(eng, h, t, None, cols, row_nos=True)
    assert ref.n_rows == ref.total_rows
    eng.decode(h, cols)
    for p, c in enumerate(cols):
        got, _ = eng.fetch_proj(h, p, t.len(c))
        assert np.array_equal(got, eng.fetch_col(h, c, t.len(c))), c


ROUTES = {
    # name: (leaves, prog, expected last_jit or None)
    "and3_jit": ([dict(col=0, op=abi.OP_LT, lo=500),
                  dict(col=2, op=abi.OP_NE,
                       lo=int.from_bytes(b"xyz", "little")),
                  dict(col=2, op=abi.OP_GE,
                       lo=int.from_bytes(b"abd", "little"))], None, True),
    "or_prog": ([dict(col=0, op=abi.OP_LT, lo=100),
                 dict(col=3, op=abi.OP_GT, lo=2**39)],
                [0, 1, abi.TOK_OR], False),
    "black": ([dict(op=abi.OP_BLACK, bcols=[0, 3], bconst=[2**38],
                    bprog=[abi.BX_COL | 0, abi.BX_COL | 1, abi.BX_ADD,
                           abi.BX_CONST | 0, abi.BX_LT])], None, False),
    "in_list": ([dict(col=0, op=abi.OP_IN,
                      in_list=[5, 17, 250, 251, 999, 100123])], None, False),
    "leaf_on_projected": ([dict(col=1, op=abi.OP_LE, lo=9700)], None, False),
    "zero_survivors": ([dict(col=0, op=abi.OP_LT, lo=-1)], None, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_filter_route(eng, btable, route):
    t, _filt, _ref, h = btable
    leaves, prog, jit = ROUTES[route]
    filt = abi.make_filter(leaves, prog)
    cols = [1, 2, 3]
    ref = _check(eng, h, t, filt, cols, row_nos=True)
    print(f"route {route}: {ref.n_rows} survivors, last_jit={eng.last_jit()}")
    if jit is not None:
        assert eng.last_jit() == jit
    if route == "zero_survivors":
        assert ref.n_rows == 0
        for p, c in enumerate(cols):
            for start, count in ((0, None), (0, 10), (7, 1)):
                got, nulls = eng.fetch_proj(h, p, t.len(c), start, count)
                assert got.size == 0 and nulls.size == 0
        assert eng.fetch_proj_row_nos(h).size == 0
    else:
        assert 0 < ref.n_rows < ref.total_rows


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["int", "char"])
def test_every_encoding(eng, which):
    if which == "int":
        t = Table(EI_SPECS, EI_ENCS, _int_enc_src())
        filt = abi.make_filter([dict(col=0, op=abi.OP_LT, lo=500)])
        cols = [0, 1, 2, 3, 4, 5]
    else:
        t = Table(EC_SPECS, EC_ENCS, _char_enc_src())
        filt = abi.make_filter([dict(col=6, op=abi.OP_LT, lo=500)])
        cols = [0, 1, 2, 3, 4, 5]
    h = eng.load(t.bs)
    ref = _check(eng, h, t, filt, cols, row_nos=True)
    assert 0 < ref.n_rows < ref.total_rows
    for c in cols[1:]:
        assert ref.nulls[c].any(), c
    _check_window(eng, h, t, ref, cols, 13, 601)
    eng.free(h)


@pytest.mark.gpu
def test_blocks_too_large_for_lds(eng):
    from types import SimpleNamespace
    li = oracle.Lineitem(4, 30000, block_bytes=65536)
    T = SimpleNamespace(schema=li.schema,
                        blocks=[li.block(i) for i in range(li.n_blocks)],
                        len=lambda c: li.schema[c].len)
    filt = abi.make_filter(
        [dict(col=6, op=abi.OP_LE, lo=oracle.date_days(1998, 9, 2))])
    h = eng.load(li.bs)
    cols = [4, 1, 6]
    ref = _check(eng, h, T, filt, cols, row_nos=True)
    assert 0 < ref.n_rows < li.total_rows
    _check_window(eng, h, T, ref, cols, 4097, 5003)
    eng.free(h)


@pytest.mark.gpu
def test_cs_loaded_handle(eng):
    """integer nulls in both CS forms: a replace value (col 0) and the null
    bitmap a full-range column is forced to (col 1); col 2 is the key"""
    rng = np.random.default_rng(33)
    blobs, want = [], {0: [], 1: []}
    keys = []
    for rows in (1200, 900):
        small = rng.integers(-1000, 1000, rows).astype(np.int64)
        wide = rng.integers(-2**62, 2**62, rows).astype(np.int64)
        wide[0], wide[1] = np.iinfo(np.int64).min, np.iinfo(np.int64).max
        key = rng.integers(0, 1000, rows).astype(np.int64)
        n0 = sorted(rng.choice(rows, 60, replace=False).tolist())
        n1 = sorted(rng.choice(np.arange(2, rows), 45, replace=False).tolist())
        blob = cs_enc(rows, [cs_int_col(small, null_rows=n0, enc=1),
                             cs_int_col(wide, null_rows=n1, enc=1),
                             cs_int_col(key, enc=1)])
        v = cs_dec(blob)
        assert not v.col[0].attrs & CA_HAS_NULL_BITMAP  # replace value
        assert v.col[1].attrs & CA_HAS_NULL_BITMAP
        for c, nr in ((0, n0), (1, n1)):
            vals, nulls = cs_get_int(v, c)
            assert nulls == set(nr)
            isn = np.zeros(rows, dtype=bool)
            isn[nr] = True
            vals = vals.copy()
            vals[isn] = 0
            want[c].append((vals, isn))
        kv, kn = cs_get_int(v, 2)
        assert not kn
        keys.append(kv)
        blobs.append(blob)
    h = eng.load_cs(blobs, oracle.make_schema([INT8] * 3))
    filt = abi.make_filter([dict(col=2, op=abi.OP_LT, lo=500)])
    keep = np.concatenate(keys) < 500
    n = eng.scan_project(h, filt, [0, 1], want_row_nos=True)
    assert n == int(keep.sum()) and 0 < n < len(keep)
    for p in (0, 1):
        vals = np.concatenate([w[0] for w in want[p]])[keep]
        isn = np.concatenate([w[1] for w in want[p]])[keep]
        got, got_nulls = eng.fetch_proj(h, p, 8)
        assert np.array_equal(got.view(np.int64), vals), p
        assert np.array_equal(got_nulls, _pack(isn)), p
        assert isn.any()
    assert np.array_equal(eng.fetch_proj_row_nos(h),
                          np.nonzero(keep)[0].astype(np.uint64))
    eng.free(h)


@pytest.mark.gpu
def test_state_and_lifetime(eng):
    t, filt, ref = boundary()
    h = eng.load(t.bs)
    lib, ctx = eng._lib, eng._ctx
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    n64 = C.c_uint64()
    arr = (C.c_uint16 * 2)(1, 3)

    def fetch_rc():
        return lib.obx_gpu_fetch_proj(ctx, h, 0, 0, 4, p, 4096, p, 4096,
                                      C.byref(n64))

    # a fetch before any scan_project is refused
    assert fetch_rc() == OBX_INVALID_ARGUMENT
    assert lib.obx_gpu_fetch_proj_row_nos(
        ctx, h, 0, 4, p, 512, C.byref(n64)) == OBX_INVALID_ARGUMENT

    # large, small, large: each exact, no stale tail
    small = abi.make_filter([dict(col=0, op=abi.OP_LT, lo=3)])
    r_large = _check(eng, h, t, None, [3, 1, 3], row_nos=True)
    r_small = _check(eng, h, t, small, [1, 3], row_nos=True)
    assert 0 < r_small.n_rows < ref.n_rows < r_large.n_rows
    got, nulls = eng.fetch_proj(h, 0, 4, 0, 1 << 40)
    assert got.size == 4 * r_small.n_rows
    assert nulls.size == (r_small.n_rows + 7) // 8
    _check(eng, h, t, filt, [3, 2, 1, 0], ref=ref, row_nos=True)

    # a failed call (bad column) leaves fetch refusing
    bad = (C.c_uint16 * 2)(1, 4)
    assert lib.obx_gpu_scan_project(ctx, h, C.byref(filt), bad, 2, 0,
                                    C.byref(n64)) == OBX_INVALID_ARGUMENT
    assert fetch_rc() == OBX_INVALID_ARGUMENT

    # the filter verb after a scan_project still matches the oracle, and a
    # scan_project leaves the filter state obx_gpu_filter would
    assert eng.scan_project(h, filt, [1]) == ref.n_rows

    def filter_state():
        rid, n = eng.fetch_row_ids(h)
        return (n, eng.fetch_blk_counts(h, len(t.blocks)),
                eng.fetch_bitmap(h), rid)

    after_project = filter_state()
    assert eng.filter(h, filt, want_row_ids=True) == ref.n_rows
    after_filter = filter_state()
    row0 = np.concatenate([[0], np.cumsum(B_ROWS)])
    for n, counts, bitmap, rid in (after_project, after_filter):
        assert n == ref.n_rows
        keep = np.zeros(ref.total_rows, dtype=bool)
        keep[ref.row_nos.astype(np.int64)] = True
        assert np.array_equal(_bits(bitmap, ref.total_rows), keep)
        for b in range(len(B_ROWS)):
            k = np.nonzero(keep[row0[b]:row0[b + 1]])[0]
            assert counts[b] == len(k)
            assert np.array_equal(rid[row0[b]:row0[b] + len(k)], k)

    # a freed handle refuses all three verbs
    eng.free(h)
    assert lib.obx_gpu_scan_project(ctx, h, C.byref(filt), arr, 2, 0,
                                    C.byref(n64)) == OBX_INVALID_ARGUMENT
    assert fetch_rc() == OBX_INVALID_ARGUMENT
    assert lib.obx_gpu_fetch_proj_row_nos(
        ctx, h, 0, 4, p, 512, C.byref(n64)) == OBX_INVALID_ARGUMENT


def _fuzz_case(seed):
    rng = np.random.default_rng(1000 + seed)
    n_blocks = int(rng.integers(1, 9))
    src = []
    for _ in range(n_blocks):
        rows = int(rng.integers(1, 3001))
        src.append(_mixed_block(rng, rows, rng.integers(0, 1000, rows)))
    leaves = [dict(col=0, op=int(rng.choice([abi.OP_LT, abi.OP_GE])),
                   lo=int(rng.integers(0, 1001)))]
    if rng.integers(0, 2):
        leaves.append(dict(col=1, op=int(rng.choice([abi.OP_LE, abi.OP_GT])),
                           lo=int(rng.integers(8900, 11100))))
    cols = [int(c) for c in rng.integers(0, 4, int(rng.integers(1, 9)))]
    return src, leaves, cols


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(20))
def test_seeded_fuzz(eng, seed):
    src, leaves, cols = _fuzz_case(seed)
    t = Table(B_SPECS, B_ENCS, src)
    h = eng.load(t.bs)
    ref = _check(eng, h, t, abi.make_filter(leaves), cols, row_nos=True)
    print(f"fuzz {seed}: {len(src)} blocks, {ref.total_rows} rows, "
          f"{ref.n_rows} survivors, cols {cols}")
    if ref.n_rows > 9:
        _check_window(eng, h, t, ref, cols, 3, ref.n_rows - 7)
    eng.free(h)
