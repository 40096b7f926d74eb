"""Key-set filter leaves (OBX_OP_IN_SET) on the GPU: a device-resident set of
join build keys tested per row by obx_gpu_filter, obx_gpu_scan_project and
obx_gpu_scan_filter_agg, alone and mixed with other leaves, on PAX- and
CS-loaded handles.

Expected values come from the arrays this file generates (np.isin, Python-int
sums), never from the engine. Where a set has at most 8 keys the same
predicate as OBX_OP_IN through the CPU oracle must give the identical bitmap.
Bitmaps, ordered row ids and per-block counts are compared bit-exactly.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oceanbase_amd import abi, engine, oracle  # noqa: E402
import cs_oracle_util as csu  # noqa: E402
from test_cs_block import _enc as cs_enc, _int_col as cs_int_col  # noqa: E402
from test_gpu_parity import _manual_blockset  # noqa: E402

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
INT8 = (abi.T_INT, 0, 19, 8)
CHAR2 = (abi.T_CHAR, 0, 0, 2)
HASH, BITMAP = abi.KS_HASH, abi.KS_BITMAP
JIT_FILTER = 2  # what obx_gpu_last_jit reports for the filter JIT
BLOCK_ROWS = [1000, 1500, 2000, 1024, 1237]
# a CONST block holds at most 255 exceptions (uint8 count in the format) and
# its NULLs are exceptions: with a NULL every 7th row, at most 1785 rows
CONST_BLOCK_ROWS = [1000, 1500, 1700, 1024, 1237]


@pytest.fixture(scope="module")
def eng():
    e = engine.GpuEngine(0)
    yield e
    e.close()


# ---- tables ---------------------------------------------------------------

class Table:
    """columns[c] = (spec, encoding, values, nulls or None); values is an
    int64 array, or an (n, len) uint8 array for char; split into blocks of
    block_rows"""

    def __init__(self, columns, block_rows):
        self.columns, self.block_rows = columns, block_rows
        self.schema = oracle.make_schema([c[0] for c in columns])
        encs = [c[1] for c in columns]
        self.blocks, r0 = [], 0
        for rows in block_rows:
            raw, nbs = [], []
            for _, _, vals, nulls in columns:
                raw.append(np.ascontiguousarray(vals[r0:r0 + rows])
                           .view(np.uint8).reshape(-1))
                nbs.append(None if nulls is None else np.packbits(
                    nulls[r0:r0 + rows].astype(np.uint8), bitorder="little"))
            self.blocks.append(oracle.encode_block(self.schema, raw, encs, nbs))
            r0 += rows
        self.total_rows = r0
        self.bs = _manual_blockset(self.schema, self.blocks)
        self.bs.total_rows = r0

    def key_values(self, c):
        """column c as the int64 keys a set holds (char: zero-extended
        little-endian datum bytes) and its null flags"""
        spec, _, vals, nulls = self.columns[c]
        if spec[0] == abi.T_CHAR:
            v = np.zeros(len(vals), dtype=np.int64)
            for k in range(spec[3]):
                v |= vals[:, k].astype(np.int64) << (8 * k)
            vals = v
        if nulls is None:
            nulls = np.zeros(len(vals), dtype=bool)
        return vals, nulls


def every_7th(n):
    return np.arange(n) % 7 == 3


def check_filter(eng, h, table, filt, keep):
    """bitmap, ordered row ids, per-block counts and the survivor count of
    obx_gpu_filter(want_row_ids) against the bool array keep"""
    n = eng.filter(h, filt, want_row_ids=True)
    assert n == int(keep.sum())
    bm = np.unpackbits(eng.fetch_bitmap(h), bitorder="little")
    assert (bm[:table.total_rows].astype(bool) == keep).all()
    ids, n_ids = eng.fetch_row_ids(h)
    assert n_ids == n
    counts = eng.fetch_blk_counts(h, len(table.block_rows))
    r0 = 0
    for b, rows in enumerate(table.block_rows):
        want = np.nonzero(keep[r0:r0 + rows])[0]
        assert counts[b] == len(want), b
        assert (ids[r0:r0 + len(want)] == want).all(), b
        r0 += rows


def oracle_in_bits(table, col, keys):
    """the same predicate as OBX_OP_IN (<= 8 operands) through the oracle"""
    assert len(keys) <= 8
    f = abi.make_filter([dict(col=col, op=abi.OP_IN,
                              in_list=[int(k) for k in keys])])
    out = []
    for blk, rows in zip(table.blocks, table.block_rows):
        bits, _ = oracle.filter_block(table.schema, len(table.columns), blk, f)
        out.append(np.unpackbits(bits, bitorder="little")[:rows])
    return np.concatenate(out).astype(bool)


# ---- encodings x forms x JIT ----------------------------------------------

def _enc_column(name, n, nulls):
    """(spec, enc, values, nulls) of one encoding under test; every value
    lies within +-2^21 so a forced bitmap stays small"""
    rng = np.random.default_rng(11 + ENCODINGS.index(name))
    if name == "raw_fixed":      # negatives: no bit packing
        return INT8, abi.ENC_RAW, rng.integers(-10**6, 10**6, n), nulls
    if name == "raw_packed":     # 10-bit fields
        return INT8, abi.ENC_RAW, rng.integers(0, 1000, n), nulls
    if name == "intdiff_negbase":
        return (INT8, abi.ENC_INT_DIFF,
                -2 * 10**6 + rng.integers(0, 5000, n), nulls)
    if name == "dict10":
        d = np.array([3, -11, 42, 2**20, -2**20, 0, -1, 7, 1000, 999])
        return INT8, abi.ENC_DICT, rng.choice(d, n), nulls
    if name == "dict200":
        d = rng.choice(np.arange(-50000, 50000), 200, replace=False)
        return INT8, abi.ENC_DICT, rng.choice(d, n), nulls
    if name == "rle":
        v = np.repeat(rng.integers(-50, 50, n // 40 + 1), 40)[:n]
        return INT8, abi.ENC_RLE, v, nulls
    if name == "const":          # one value per block; NULLs are exceptions
        v = np.concatenate([np.full(r, 700 + 3 * b)
                            for b, r in enumerate(CONST_BLOCK_ROWS)])
        return INT8, abi.ENC_CONST, v, nulls
    if name == "char2":
        words = np.frombuffer(b"abacxyzzQ q 09", dtype=np.uint8).reshape(-1, 2)
        return CHAR2, abi.ENC_AUTO, words[rng.integers(0, len(words), n)], nulls
    raise KeyError(name)


ENCODINGS = ["raw_fixed", "raw_packed", "intdiff_negbase", "dict10",
             "dict200", "rle", "const", "char2"]
_tables = {}


def enc_table(name, with_nulls):
    """built once per (encoding, nulls) and shared; nothing changes it"""
    key = (name, with_nulls)
    if key not in _tables:
        block_rows = CONST_BLOCK_ROWS if name == "const" else BLOCK_ROWS
        n = sum(block_rows)
        col = _enc_column(name, n, every_7th(n) if with_nulls else None)
        col = (col[0], col[1],
               col[2] if col[0] == CHAR2 else col[2].astype(np.int64), col[3])
        _tables[key] = Table([col], block_rows)
    return _tables[key]


def member_keys(vals, rng, n_absent=50):
    """about a third of the column's distinct values (every other one for a
    handful), plus values of the same range the column does not hold, with
    duplicates"""
    u = np.unique(vals)
    take = u[::2] if len(u) <= 20 else rng.choice(u, len(u) // 3, replace=False)
    absent = np.setdiff1d(rng.integers(u.min() - 5, u.max() + 5, n_absent), u)
    keys = np.concatenate([take, absent, take[:3]])
    rng.shuffle(keys)
    return keys


@pytest.mark.parametrize("jit", ["default", "off"])
@pytest.mark.parametrize("form", [HASH, BITMAP])
@pytest.mark.parametrize("name", ENCODINGS)
def test_encodings_with_nulls(eng, monkeypatch, name, form, jit):
    if jit == "off":
        monkeypatch.setenv("OBX_JIT", "0")
    t = enc_table(name, True)
    vals, nulls = t.key_values(0)
    keys = member_keys(vals[~nulls], np.random.default_rng(5))
    if form == HASH:  # any int64 can be a key of a hash set
        keys = np.concatenate([keys, [I64.min, I64.max, -1]])
    h = eng.load(t.bs)
    sid = eng.keyset_create(keys, form)
    try:
        info = eng.keyset_info(sid)
        assert info.kind == form
        assert info.n_distinct == len(np.unique(keys))
        keep = np.isin(vals, keys) & ~nulls
        assert 0 < keep.sum() < (~nulls).sum()
        filt = abi.make_filter([dict(col=0, op=abi.OP_IN_SET, set=sid)])
        check_filter(eng, h, t, filt, keep)
        ran = eng._lib.obx_gpu_last_jit(eng._ctx)
        if name == "dict10":  # <= 63 entries: lowered to a ref mask per block
            assert ran == (JIT_FILTER if jit == "default" else 0)
        if jit == "off":
            assert ran == 0
    finally:
        eng.keyset_free(sid)
        eng.free(h)


@pytest.mark.parametrize("jit", ["default", "off"])
@pytest.mark.parametrize("form", [HASH, BITMAP])
@pytest.mark.parametrize("name", ["raw_fixed", "raw_packed",
                                  "intdiff_negbase", "const"])
def test_encodings_without_nulls(eng, monkeypatch, name, form, jit):
    """no ext bits: the packed-range family is what the staged filter JIT
    takes (SET_BITS / SET_HASH per field), a const block folds to ALL/NONE"""
    if jit == "off":
        monkeypatch.setenv("OBX_JIT", "0")
    t = enc_table(name, False)
    vals, _ = t.key_values(0)
    keys = member_keys(vals, np.random.default_rng(6))
    h = eng.load(t.bs)
    sid = eng.keyset_create(keys, form)
    try:
        keep = np.isin(vals, keys)
        assert 0 < keep.sum() < len(vals)
        filt = abi.make_filter([dict(col=0, op=abi.OP_IN_SET, set=sid)])
        check_filter(eng, h, t, filt, keep)
        ran = eng._lib.obx_gpu_last_jit(eng._ctx)
        # the packed-range family takes the staged filter JIT (leaf kind 3)
        staged = name != "const" and jit == "default"
        assert ran == (JIT_FILTER if staged else 0)
        # bitmap only (no row ids) takes its own kernel variant
        assert eng.filter(h, filt) == int(keep.sum())
        bm = np.unpackbits(eng.fetch_bitmap(h), bitorder="little")
        assert (bm[:t.total_rows].astype(bool) == keep).all()
    finally:
        eng.keyset_free(sid)
        eng.free(h)


@pytest.mark.parametrize("form", [HASH, BITMAP])
@pytest.mark.parametrize("name", ENCODINGS)
def test_small_set_equals_oracle_in(eng, name, form):
    """<= 8 keys: the bitmap is the oracle's for OBX_OP_IN on the same keys"""
    t = enc_table(name, True)
    vals, nulls = t.key_values(0)
    u = np.unique(vals[~nulls])
    keys = list(u[:: max(1, len(u) // 4)][:4]) + [int(u.max()) + 1]
    want = oracle_in_bits(t, 0, keys)
    assert (want == (np.isin(vals, keys) & ~nulls)).all()
    assert want.any()
    h = eng.load(t.bs)
    sid = eng.keyset_create(keys, form)
    try:
        check_filter(eng, h, t, abi.make_filter(
            [dict(col=0, op=abi.OP_IN_SET, set=sid)]), want)
    finally:
        eng.keyset_free(sid)
        eng.free(h)


def test_fixed_width_signed_fields(eng):
    """4-byte date fields (sign bit inside the stored bytes) against keys on
    both sides of zero, in both forms"""
    rng = np.random.default_rng(8)
    n = sum(BLOCK_ROWS)
    vals = rng.integers(-3000, 3000, n).astype(np.int32)
    t = Table([((abi.T_DATE, 0, 0, 4), abi.ENC_RAW, vals, None)], BLOCK_ROWS)
    keys = member_keys(vals.astype(np.int64), rng)
    keep = np.isin(vals, keys)
    h = eng.load(t.bs)
    for form in (HASH, BITMAP):
        sid = eng.keyset_create(keys, form)
        check_filter(eng, h, t, abi.make_filter(
            [dict(col=0, op=abi.OP_IN_SET, set=sid)]), keep)
        eng.keyset_free(sid)
    eng.free(h)


# ---- build races ------------------------------------------------------------

@pytest.mark.parametrize("form,hi", [(HASH, 1 << 50), (BITMAP, 200000)])
def test_build_races(eng, form, hi):
    """70 000 input keys, about half of them duplicates, inserted by
    thousands of threads at once: exact distinct count and bounds, and the
    device set answers 10 000 probes as the host model does"""
    rng = np.random.default_rng(13)
    base = rng.integers(-hi, hi, 35000)
    keys = np.concatenate([base, rng.choice(base, 35000)])
    rng.shuffle(keys)
    probe = np.concatenate([rng.choice(base, 5000), rng.integers(-hi, hi, 5000)])
    rng.shuffle(probe)
    hit, model = engine.keyset_host_model(keys, probe)  # auto
    assert model.kind == form
    assert (hit == np.isin(probe, keys)).all()

    t = Table([(INT8, abi.ENC_RAW, probe.astype(np.int64), None)], [2000] * 5)
    h = eng.load(t.bs)
    sid = eng.keyset_create(keys)
    info = eng.keyset_info(sid)
    assert info.kind == form
    assert info.n_keys_in == 70000
    assert info.n_distinct == len(np.unique(keys)) == model.n_distinct
    assert (info.min, info.max) == (int(keys.min()), int(keys.max()))
    assert (info.slots_or_bits, info.bytes) == (model.slots_or_bits,
                                                model.bytes)
    check_filter(eng, h, t, abi.make_filter(
        [dict(col=0, op=abi.OP_IN_SET, set=sid)]), hit)
    eng.keyset_free(sid)
    eng.free(h)


# ---- skip index -------------------------------------------------------------

def _disjoint_table():
    rng = np.random.default_rng(17)
    vals = np.concatenate([b * 10000 + rng.integers(0, 5000, 1000)
                           for b in range(8)]).astype(np.int64)
    return Table([(INT8, abi.ENC_RAW, vals, every_7th(8000))], [1000] * 8), vals


@pytest.mark.parametrize("form", [HASH, BITMAP])
@pytest.mark.parametrize("which", ["inside_block_3", "empty", "outside"])
def test_skip_index(eng, which, form):
    t, vals = _disjoint_table()
    nulls = every_7th(8000)
    if which == "inside_block_3":
        keys = np.unique(vals[3000:4000][~nulls[3000:4000]])[::3]
    elif which == "empty":
        keys = np.zeros(0, dtype=np.int64)
    else:
        keys = np.array([-5, 5500, 79999, 10**6])
    keep = np.isin(vals, keys) & ~nulls
    if which == "inside_block_3":
        assert keep[3000:4000].any() and not keep[:3000].any()
    else:
        assert not keep.any()
    h = eng.load(t.bs)
    sid = eng.keyset_create(keys, form)
    info = eng.keyset_info(sid)
    if which == "empty":
        assert info.min > info.max and info.n_distinct == 0
    check_filter(eng, h, t, abi.make_filter(
        [dict(col=0, op=abi.OP_IN_SET, set=sid)]), keep)
    eng.keyset_free(sid)
    eng.free(h)


# ---- composition ------------------------------------------------------------

def _two_col_table(with_nulls):
    rng = np.random.default_rng(19)
    n = sum(BLOCK_ROWS)
    a = rng.integers(-20000, 20000, n).astype(np.int64)
    b = rng.integers(0, 1000, n).astype(np.int64)
    na = every_7th(n) if with_nulls else None
    nb = (np.arange(n) % 11 == 5) if with_nulls else None
    return Table([(INT8, abi.ENC_RAW, a, na), (INT8, abi.ENC_RAW, b, nb)],
                 BLOCK_ROWS)


@pytest.mark.parametrize("jit", ["default", "off"])
@pytest.mark.parametrize("form", [HASH, BITMAP])
@pytest.mark.parametrize("with_nulls", [True, False])
def test_composition(eng, monkeypatch, with_nulls, form, jit):
    if jit == "off":
        monkeypatch.setenv("OBX_JIT", "0")
    t = _two_col_table(with_nulls)
    (a, na), (b, nb) = t.key_values(0), t.key_values(1)
    rng = np.random.default_rng(23)
    ka, kb = member_keys(a[~na], rng), member_keys(b[~nb], rng)
    in_a, in_b = np.isin(a, ka) & ~na, np.isin(b, kb) & ~nb
    h = eng.load(t.bs)
    sa, sb = eng.keyset_create(ka, form), eng.keyset_create(kb, form)
    leaf_a = dict(col=0, op=abi.OP_IN_SET, set=sa)
    leaf_b = dict(col=1, op=abi.OP_IN_SET, set=sb)
    try:
        # IN_SET AND col < k
        check_filter(eng, h, t, abi.make_filter(
            [leaf_a, dict(col=1, op=abi.OP_LT, lo=400)]),
            in_a & (b < 400) & ~nb)
        # (IN_SET | NU) & other, three-valued: a NULL a passes the OR
        check_filter(eng, h, t, abi.make_filter(
            [leaf_a, dict(col=0, op=abi.OP_NU),
             dict(col=1, op=abi.OP_GE, lo=300)],
            prog=[0, 1, abi.TOK_OR, 2, abi.TOK_AND]),
            (in_a | na) & (b >= 300) & ~nb)
        # two set leaves on two columns, AND and OR
        check_filter(eng, h, t, abi.make_filter([leaf_a, leaf_b]), in_a & in_b)
        check_filter(eng, h, t, abi.make_filter(
            [leaf_a, leaf_b], prog=[0, 1, abi.TOK_OR]), in_a | in_b)
        if jit == "off":
            assert eng._lib.obx_gpu_last_jit(eng._ctx) == 0
    finally:
        eng.keyset_free(sa)
        eng.keyset_free(sb)
        eng.free(h)


# ---- semi-join end to end ---------------------------------------------------

N_ORDERS, N_ITEMS = 6000, 8000
ITEM_BLOCKS = [2000] * 4


def _orders():
    rng = np.random.default_rng(29)
    key = rng.permutation(np.arange(1, 3 * N_ORDERS, 3))[:N_ORDERS]
    key = key.astype(np.int64) - 4000  # some negative
    key_null = np.arange(N_ORDERS) % 13 == 6
    flag = rng.integers(0, 4, N_ORDERS).astype(np.int64)
    t = Table([(INT8, abi.ENC_RAW, key, key_null),
               (INT8, abi.ENC_DICT, flag, None)], [1500] * 4)
    return t, key, key_null, flag


def _items():
    rng = np.random.default_rng(31)
    okey = (rng.integers(0, 3 * N_ORDERS, N_ITEMS) - 4000).astype(np.int64)
    okey_null = np.arange(N_ITEMS) % 17 == 9
    grp = rng.integers(0, 3, N_ITEMS).astype(np.int64)
    qty = rng.integers(-500, 500, N_ITEMS).astype(np.int64)
    return okey, okey_null, grp, qty


def _expected_groups(keep, grp, qty):
    out = []
    for g in range(3):
        m = keep & (grp == g)
        if m.any():
            q = [int(x) for x in qty[m]]
            out.append((int(g).to_bytes(8, "little", signed=True), len(q),
                        [len(q), sum(q), min(q)]))
    return out


def _semi_join(eng, h_items, items, form):
    okey, okey_null, grp, qty = items
    orders, key, key_null, flag = _orders()
    h_orders = eng.load(orders.bs)
    try:
        n_build = eng.scan_project(
            h_orders, abi.make_filter([dict(col=1, op=abi.OP_EQ, lo=2)]),
            [0, 1])
        assert n_build == int((flag == 2).sum())
        before = [eng.fetch_proj(h_orders, p, 8) for p in (0, 1)]
        sid = eng.keyset_from_proj(h_orders, 0, form)
        build = key[(flag == 2) & ~key_null]
        info = eng.keyset_info(sid)
        assert info.kind == form
        assert info.n_keys_in == len(build)  # NULL keys skipped
        assert info.n_distinct == len(np.unique(build))
        assert (info.min, info.max) == (int(build.min()), int(build.max()))

        keep = np.isin(okey, build) & ~okey_null
        assert 0 < keep.sum() < N_ITEMS
        filt = abi.make_filter([dict(col=0, op=abi.OP_IN_SET, set=sid)])
        agg = abi.make_agg([1], [dict(kind=abi.AGG_COUNT),
                                 dict(kind=abi.AGG_SUM, col_a=2),
                                 dict(kind=abi.AGG_MIN, col_a=2)])
        res = eng.scan_filter_agg(h_items, filt, agg)
        assert res.rows_passed == int(keep.sum())
        want = _expected_groups(keep, grp, qty)
        assert abi.result_rows(res, 3) == want
        # without MIN the plan may take the scan JIT's non-inline route
        res = eng.scan_filter_agg(h_items, filt, abi.make_agg(
            [1], [dict(kind=abi.AGG_COUNT), dict(kind=abi.AGG_SUM, col_a=2)]))
        assert abi.result_rows(res, 2) == [(k, n, c[:2]) for k, n, c in want]

        n = eng.scan_project(h_items, filt, [2, 0])
        assert n == int(keep.sum())
        got_qty, qn = eng.fetch_proj(h_items, 0, 8)
        got_key, kn = eng.fetch_proj(h_items, 1, 8)
        assert (got_qty.view(np.int64) == qty[keep]).all()
        assert (got_key.view(np.int64) == okey[keep]).all()
        assert not qn.any() and not kn.any()

        # the build side's projection result is still there, unchanged
        after = [eng.fetch_proj(h_orders, p, 8) for p in (0, 1)]
        for (d0, n0), (d1, n1) in zip(before, after):
            assert (d0 == d1).all() and (n0 == n1).all()
        # the set outlives only the calls that name it
        eng.keyset_free(sid)
    finally:
        eng.free(h_orders)


@pytest.mark.parametrize("form", [HASH, BITMAP])
def test_semi_join_pax(eng, form):
    items = _items()
    okey, okey_null, grp, qty = items
    t = Table([(INT8, abi.ENC_RAW, okey, okey_null),
               (INT8, abi.ENC_DICT, grp, None),
               (INT8, abi.ENC_RAW, qty, None)], ITEM_BLOCKS)
    h = eng.load(t.bs)
    try:
        _semi_join(eng, h, items, form)
    finally:
        eng.free(h)


@pytest.mark.parametrize("form", [HASH, BITMAP])
def test_semi_join_cs(eng, form):
    """the probe side loaded from CS blocks (device-side transform)"""
    items = _items()
    okey, okey_null, grp, qty = items
    blobs, r0 = [], 0
    for rows in ITEM_BLOCKS:
        s = slice(r0, r0 + rows)
        nul = [int(r) for r in np.nonzero(okey_null[s])[0]]
        blob = cs_enc(rows, [
            cs_int_col([int(x) for x in okey[s]], enc=2, null_rows=nul),
            cs_int_col([int(x) for x in grp[s]], dict_=True),
            cs_int_col([int(x) for x in qty[s]], enc=2)])
        got_rows, cols = csu.decode_block(blob)  # the blocks hold the arrays
        assert got_rows == rows
        assert (cols[0]["nulls"] == okey_null[s]).all()
        assert (cols[0]["values"][~okey_null[s]] == okey[s][~okey_null[s]]).all()
        assert (cols[2]["values"] == qty[s]).all()
        blobs.append(blob)
        r0 += rows
    h = eng.load_cs(blobs, oracle.make_schema([INT8] * 3))
    try:
        _semi_join(eng, h, items, form)
    finally:
        eng.free(h)


@pytest.mark.parametrize("jit", ["default", "off"])
@pytest.mark.parametrize("form", [HASH, BITMAP])
def test_dict_set_leaf_in_the_scan_jit(eng, monkeypatch, form, jit):
    """a set leaf on a small-dict column lowers to a ref mask per block, so
    the Q1-shaped scan keeps its plan-specialized kernel; five keys, so the
    oracle's OBX_OP_IN scan is the reference"""
    if jit == "off":
        monkeypatch.setenv("OBX_JIT", "0")
    li = oracle.Lineitem(4, 50000, seed=42, block_bytes=8192)
    keys = [100, 700, 2500, 5000, 12345]  # l_quantity, scale 2; one absent
    agg = abi.make_agg([4, 5], [dict(kind=abi.AGG_COUNT),
                                dict(kind=abi.AGG_SUM, col_a=1),
                                dict(kind=abi.AGG_SUM_PROD2, col_a=1, col_b=2),
                                dict(kind=abi.AGG_MIN, col_a=1)])
    date = dict(col=6, op=abi.OP_LE, lo=oracle.date_days(1998, 9, 2))
    want = oracle.scan_filter_agg(li.bs, abi.make_filter(
        [dict(col=0, op=abi.OP_IN, in_list=keys), date]), agg)
    assert 0 < want.rows_passed < li.total_rows // 5
    h = eng.load(li.bs)
    sid = eng.keyset_create(keys, form)
    try:
        got = eng.scan_filter_agg(h, abi.make_filter(
            [dict(col=0, op=abi.OP_IN_SET, set=sid), date]), agg)
        assert got.rows_passed == want.rows_passed
        assert abi.result_rows(got, 4) == abi.result_rows(want, 4)
        assert eng.last_jit() == (jit == "default")
    finally:
        eng.keyset_free(sid)
        eng.free(h)


# ---- lifetime and errors ----------------------------------------------------

def _rc_filter(eng, h, filt):
    return eng._lib.obx_gpu_filter(eng._ctx, h, C.byref(filt), 1)


def test_lifetime_and_errors(eng):
    t = enc_table("raw_fixed", True)
    vals, nulls = t.key_values(0)
    h = eng.load(t.bs)
    bad = abi.OBX_INVALID_ARGUMENT
    try:
        # from_proj before any projection
        with pytest.raises(engine.KeysetError) as e:
            eng.keyset_from_proj(h, 0)
        assert e.value.rc == bad

        u = np.unique(vals[~nulls])
        k1, k2 = u[::2], u[1::2]
        s1 = eng.keyset_create(k1)
        leaf = lambda sid: abi.make_filter(  # noqa: E731
            [dict(col=0, op=abi.OP_IN_SET, set=sid)])
        keep1 = np.isin(vals, k1) & ~nulls
        check_filter(eng, h, t, leaf(s1), keep1)

        # unknown, negative and freed ids; an op past the last one
        assert _rc_filter(eng, h, leaf(s1 + 1000)) == bad
        assert _rc_filter(eng, h, leaf(-1)) == bad
        assert _rc_filter(eng, h, leaf(1 << 40)) == bad
        eng.keyset_free(s1)
        assert _rc_filter(eng, h, leaf(s1)) == bad
        with pytest.raises(engine.KeysetError) as e:
            eng.keyset_free(s1)
        assert e.value.rc == bad
        with pytest.raises(engine.KeysetError) as e:
            eng.keyset_info(s1)
        assert e.value.rc == bad
        f12 = abi.make_filter([dict(col=0, op=12, lo=0)])
        assert _rc_filter(eng, h, f12) == bad
        # the other verbs refuse the same way
        res = abi.AggResult()
        agg = abi.make_agg([], [dict(kind=abi.AGG_COUNT)])
        f = leaf(s1)
        assert eng._lib.obx_gpu_scan_filter_agg(
            eng._ctx, h, C.byref(f), C.byref(agg), C.byref(res)) == bad
        with pytest.raises(RuntimeError):
            eng.scan_project(h, f, [0])

        # the engine still answers a plain query
        check_filter(eng, h, t, abi.make_filter(
            [dict(col=0, op=abi.OP_LT, lo=0)]), (vals < 0) & ~nulls)

        # freed after its query; a new set gives the new set's result
        s2 = eng.keyset_create(k2)
        assert s2 > s1
        check_filter(eng, h, t, leaf(s2), np.isin(vals, k2) & ~nulls)
        eng.keyset_free(s2)

        # ids never repeat
        ids = [eng.keyset_create([i, i + 1]) for i in range(40)]
        assert ids == list(range(s2 + 1, s2 + 41))
        for sid in ids:
            eng.keyset_free(sid)
        s3 = eng.keyset_create(k1)
        assert s3 == s2 + 41
        check_filter(eng, h, t, leaf(s3), keep1)
        eng.keyset_free(s3)

        # a forced bitmap past the span cap
        with pytest.raises(engine.KeysetError) as e:
            eng.keyset_create([0, 1 << 33], BITMAP)
        assert e.value.rc == abi.OBX_NOT_SUPPORTED
    finally:
        eng.free(h)
