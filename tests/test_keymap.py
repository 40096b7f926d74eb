"""Key maps and the join scan (obx_gpu_scan_join_agg) on the GPU.

Every case builds one wide table: the fact columns (probe key, value columns,
a dict char) plus two columns the GPU never names, `pay` (the payload the
row's key maps to, 0 where it has none) and `hit` (1 iff the key is a map
key). The GPU joins the fact columns with a device key map; the CPU oracle
scans the same blockset as the denormalised table, with `hit = 1` AND-ed onto
the filter and `pay` in place of OBX_COL_JOINED. A join with a unique-key
build side gives the same groups, so n_groups, rows_passed and every group
row must be equal. Each test asserts its own precondition (hit share, group
count) on the oracle's result.
"""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oceanbase_amd import abi, engine, oracle  # noqa: E402
from test_cs_block import _enc as cs_enc, _int_col as cs_int_col  # noqa: E402
from test_keyset import Table  # noqa: E402

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
INT8 = (abi.T_INT, 0, 19, 8)
INT4 = (abi.T_INT32, 0, 10, 4)
DATE = (abi.T_DATE, 0, 0, 4)
CHAR1 = (abi.T_CHAR, 0, 0, 1)
HASH, DENSE, AUTO = abi.KM_HASH, abi.KM_DENSE, abi.KM_AUTO
J = abi.COL_JOINED
STAGE_BYTES = 17408
# columns of the wide table
K, V, N, D, CH, O, PAY, HIT = range(8)
STAGED_BLOCKS = [2100, 64, 1, 777]   # 2100: a partial second 2048-row window
UNSTAGED_BLOCKS = [3000, 3000]


@pytest.fixture(scope="module")
def eng():
    e = engine.GpuEngine(0)
    yield e
    e.close()


# ---- tables -----------------------------------------------------------------

def key_domain(kind, rng):
    """(the values a fact key is drawn from, its encoding)"""
    if kind == "intdiff":      # packs narrow: 16-bit diffs
        return 10**9 + np.arange(50_000), abi.ENC_INT_DIFF
    if kind == "raw_packed":   # non-negative: a bit-packed RAW stream
        return np.arange(60_000), abi.ENC_RAW
    if kind == "raw_fixed":    # the full int64 range: 8-byte fields
        d = rng.integers(I64.min, I64.max, 4000)
        return np.unique(np.concatenate([d, [-1, I64.min, I64.max, 0]])), \
            abi.ENC_RAW
    if kind == "dict":
        return np.unique(rng.integers(-10**6, 10**6, 200)), abi.ENC_DICT
    raise KeyError(kind)


def payloads(kind, n, rng):
    """(spec, n payload values: an integer array of the column's dtype, or
    (n, 1) uint8 for char)"""
    if kind == "int32":        # <= 5 values, a negative one among them
        return INT4, rng.choice([-7, -1, 0, 3, 100_000], n).astype(np.int32)
    if kind == "int32_15":
        return INT4, rng.integers(-7, 8, n).astype(np.int32)
    if kind == "int32_300":
        return INT4, rng.integers(-150, 150, n).astype(np.int32)
    if kind == "int32_unique":
        return INT4, (np.arange(n) - 7).astype(np.int32)
    if kind == "date":
        return DATE, (oracle.date_days(1995, 3, 1) +
                      rng.integers(0, 9, n)).astype(np.int32)
    if kind == "char1":
        return CHAR1, rng.choice(np.frombuffer(b"ABCDE", np.uint8),
                                 n).reshape(-1, 1)
    if kind == "int8":         # 8-byte payloads: aggregate inputs only
        vals = np.random.default_rng(99).integers(-10**17, 10**17, 40)
        return INT8, rng.choice(vals, n).astype(np.int64)
    if kind == "int8_wide":
        return INT8, rng.integers(-10**17, 10**17, n).astype(np.int64)
    raise KeyError(kind)


class Case:
    """one wide table with its map (map_keys -> map_pay)"""

    def __init__(self, block_rows, key_kind="intdiff", pay_kind="int32",
                 key_nulls=False, ch_nulls=False, share=0.5, seed=1,
                 edit=None):
        """edit(self, cols, block_rows) may change the fact columns and
        self.map_keys, and may set self.spec / self.map_pay itself"""
        rng = np.random.default_rng(seed)
        n = sum(block_rows)
        dom, key_enc = key_domain(key_kind, rng)
        n_map = int(round(len(dom) * share))
        self.map_keys = rng.choice(dom, n_map, replace=False).astype(np.int64)
        self.map_pay = None
        cols = {
            K: rng.choice(dom, n).astype(np.int64),
            V: rng.choice(np.arange(-500, 501, 25), n),   # a 41-entry dict
            N: rng.integers(0, 100, n),
            D: rng.integers(0, 11, n),
            CH: rng.choice(np.frombuffer(b"xyz", np.uint8), n).reshape(-1, 1),
            O: rng.integers(0, 20, n),
        }
        self.key_null = (np.arange(n) % 5 == 2) if key_nulls else None
        self.n_null = np.arange(n) % 9 == 4
        if edit:
            edit(self, cols, block_rows)
        if self.map_pay is None:
            self.spec, self.map_pay = payloads(pay_kind, len(self.map_keys),
                                               rng)
        assert len(np.unique(self.map_keys)) == len(self.map_keys)
        # the denormalised columns
        order = np.argsort(self.map_keys)
        sk = self.map_keys[order]
        pos = np.clip(np.searchsorted(sk, cols[K]), 0, max(len(sk) - 1, 0))
        hit = (sk[pos] == cols[K]) if len(sk) else np.zeros(n, dtype=bool)
        if self.key_null is not None:
            hit &= ~self.key_null
        pay = np.zeros((n,) + self.map_pay.shape[1:], self.map_pay.dtype)
        if len(sk):
            pay[hit] = self.map_pay[order][pos[hit]]
        self.hit = hit
        num = abi.ENC_INT_DIFF
        self.table = Table([
            (INT8, key_enc, cols[K], self.key_null),
            (INT8, abi.ENC_DICT, cols[V].astype(np.int64), None),
            (INT8, abi.ENC_AUTO, cols[N].astype(np.int64), self.n_null),
            (INT8, num, cols[D].astype(np.int64), None),
            (CHAR1, abi.ENC_DICT, cols[CH],
             (np.arange(n) % 6 == 1) if ch_nulls else None),
            (INT8, num, cols[O].astype(np.int64), None),
            # a dict keeps negative payloads narrow enough for the stage
            (self.spec, abi.ENC_DICT if len(np.unique(pay)) <= 512
             else abi.ENC_AUTO, pay, None),
            (INT8, abi.ENC_AUTO, hit.astype(np.int64), None),
        ], block_rows)
        self.cols = cols

    def block_bytes(self):
        return [len(b) - 16 for b in self.table.blocks]

    def create(self, eng, kind=AUTO):
        return eng.keymap_create(self.map_keys, self.map_pay, self.spec, kind)


_cases = {}


def case(*a, **kw):
    """built once per argument list and shared; nothing changes it"""
    key = (a, tuple(sorted((k, v) for k, v in kw.items())))
    if key not in _cases:
        _cases[key] = Case(*a, **kw)
    return _cases[key]


def staged(**kw):
    c = case(tuple(STAGED_BLOCKS), **kw)
    assert max(c.block_bytes()) <= STAGE_BYTES
    return c


# ---- the comparison ---------------------------------------------------------

def _subst(x):
    return PAY if x == J else x


def oracle_rows(c, leaves, prog, group, aggs):
    """the denormalised scan: hit = 1 AND-ed on, pay for OBX_COL_JOINED"""
    hit_leaf = dict(col=HIT, op=abi.OP_EQ, lo=1)
    if prog:
        o_prog = list(prog) + [len(leaves), abi.TOK_AND]
    else:
        o_prog = None
    filt = abi.make_filter(list(leaves) + [hit_leaf], o_prog)
    agg = abi.make_agg(
        [_subst(g) for g in group],
        [dict(a, col_a=_subst(a["col_a"])) if "col_a" in a else a
         for a in aggs])
    return oracle.scan_filter_agg_paged(c.table.bs, filt, agg)


def check_join(eng, h, c, mid, group, aggs, leaves=(), prog=None,
               gpu_leaves=None, groups=(1, 15), share=(0.0, 1.0)):
    """GPU join scan == oracle scan of the denormalised table. groups: the
    inclusive range the oracle's group count must lie in; share: the
    exclusive range of joined rows / table rows (None: not checked).
    gpu_leaves: the GPU's leaves where they differ (an IN_SET leaf)."""
    want, want_rows = oracle_rows(c, leaves, prog, group, aggs)
    assert groups[0] <= len(want_rows) <= groups[1], len(want_rows)
    if share is not None:
        s = want.rows_passed / c.table.total_rows
        assert share[0] < s < share[1], s
    filt = abi.make_filter(list(leaves if gpu_leaves is None else gpu_leaves),
                           prog)
    got, got_rows = eng.scan_join_agg_paged(h, filt, mid, K,
                                            abi.make_agg(group, aggs))
    assert eng.last_jit() is False
    assert got.rows_passed == want.rows_passed
    assert got.rows_scanned == c.table.total_rows
    assert got.n_groups == want.n_groups == len(want_rows)
    assert (abi.group_row_tuples(got_rows, len(aggs)) ==
            abi.group_row_tuples(want_rows, len(aggs)))
    return want


MIXED_AGGS = [dict(kind=abi.AGG_COUNT),
              dict(kind=abi.AGG_SUM, col_a=V),
              dict(kind=abi.AGG_SUM_PROD2, col_a=V, col_b=D),
              dict(kind=abi.AGG_MIN, col_a=N),
              dict(kind=abi.AGG_COUNT, col_a=N)]


# every kind through the join scan's aggregate passes and its growth path,
# OBX_DEV_MAX_AGGS cells: a PROD2 + PROD3 pair over the same a and b (one
# fused pass; N holds NULLs, so a NULL c drops only the PROD3 half), a PROD3
# that runs alone, SUM_MUL, MAX and COUNT of the column with NULLs, and one
# payload aggregate of the join step's own
ALL_KIND_AGGS = [dict(kind=abi.AGG_COUNT),
                 dict(kind=abi.AGG_SUM_PROD2, col_a=V, col_b=D),
                 dict(kind=abi.AGG_SUM_PROD3, col_a=V, col_b=D, col_c=N),
                 dict(kind=abi.AGG_SUM_PROD3, col_a=V, col_b=N, col_c=D),
                 dict(kind=abi.AGG_SUM_MUL, col_a=V, col_b=N),
                 dict(kind=abi.AGG_MAX, col_a=N),
                 dict(kind=abi.AGG_COUNT, col_a=N),
                 dict(kind=abi.AGG_SUM, col_a=J)]
assert len(ALL_KIND_AGGS) == 8   # OBX_DEV_MAX_AGGS
ALL_KIND_OR = dict(leaves=[dict(col=O, op=abi.OP_LT, lo=5),
                           dict(col=D, op=abi.OP_GE, lo=6)],
                   prog=[0, 1, abi.TOK_OR])


def run(eng, c, kind, group, aggs, **kw):
    h = eng.load(c.table.bs)
    mid = c.create(eng, kind)
    try:
        info = eng.keymap_info(mid)
        if kind != AUTO and len(c.map_keys):
            assert info.kind == kind
        assert info.n_keys == len(c.map_keys)
        return check_join(eng, h, c, mid, group, aggs, **kw)
    finally:
        eng.keymap_free(mid)
        eng.free(h)


# ---- group by the payload ---------------------------------------------------

@pytest.mark.parametrize("kind", [HASH, DENSE, AUTO])
@pytest.mark.parametrize("pay_kind", ["int32_15", "date", "char1"])
def test_group_by_payload_alone(eng, pay_kind, kind):
    run(eng, staged(pay_kind=pay_kind), kind, [J], MIXED_AGGS, groups=(5, 15))


@pytest.mark.parametrize("kind", [HASH, DENSE])
@pytest.mark.parametrize("group", [[CH, J], [J, CH]])
@pytest.mark.parametrize("pay_kind", ["int32", "char1"])
def test_group_by_payload_and_dict_char(eng, pay_kind, group, kind):
    run(eng, staged(pay_kind=pay_kind), kind, group, MIXED_AGGS,
        groups=(10, 15))


@pytest.mark.parametrize("group", [[CH, J], [J, CH]])
def test_null_flag_of_the_other_group_column(eng, group):
    """the dict char holds NULLs: its NULL flag keeps the bit of its
    position whichever side of the payload it stands on"""
    c = staged(pay_kind="int32", ch_nulls=True, seed=5)
    run(eng, c, HASH, group, MIXED_AGGS, groups=(16, 20))


@pytest.mark.parametrize("kind", [HASH, DENSE])
def test_payload_aggregates_without_groups(eng, kind):
    """an 8-byte payload is fine as an aggregate input"""
    aggs = [dict(kind=abi.AGG_SUM, col_a=J), dict(kind=abi.AGG_MIN, col_a=J),
            dict(kind=abi.AGG_MAX, col_a=J), dict(kind=abi.AGG_COUNT, col_a=J),
            dict(kind=abi.AGG_COUNT), dict(kind=abi.AGG_SUM, col_a=V),
            dict(kind=abi.AGG_SUM_PROD2, col_a=V, col_b=D),
            dict(kind=abi.AGG_MIN, col_a=N)]
    run(eng, staged(pay_kind="int8"), kind, [], aggs, groups=(1, 1))


def test_payload_aggregates_per_real_group(eng):
    aggs = [dict(kind=abi.AGG_MAX, col_a=J), dict(kind=abi.AGG_SUM, col_a=V),
            dict(kind=abi.AGG_SUM, col_a=J), dict(kind=abi.AGG_COUNT)]
    c = case((1000, 700), pay_kind="int8_wide", seed=13)
    run(eng, c, AUTO, [CH], aggs, groups=(3, 3))
    # 20 groups: past the LDS table, so the direct kernel sums the payloads
    run(eng, c, AUTO, [O], aggs, groups=(20, 20))


# ---- every aggregate kind through the join scan -------------------------------

@pytest.mark.parametrize("kind", [HASH, DENSE])
@pytest.mark.parametrize("filt,joined", [({}, 1482), (ALL_KIND_OR, 891)],
                         ids=["and", "or_prog"])
def test_all_kinds_staged(eng, filt, joined, kind):
    """k_scan_join_agg_lds / k_scan_join_agg_prog_lds"""
    c = staged(pay_kind="int32")
    assert c.table.total_rows == 2942
    want = run(eng, c, kind, [CH, J], ALL_KIND_AGGS, groups=(15, 15), **filt)
    assert want.rows_passed == joined


@pytest.mark.parametrize("kind", [HASH, DENSE])
def test_all_kinds_direct_kernel(eng, kind):
    """20 groups overflow the LDS table: k_scan_join_agg_direct"""
    want = run(eng, staged(pay_kind="int32"), kind, [O], ALL_KIND_AGGS,
               groups=(20, 20))
    assert want.rows_passed == 1482


@pytest.mark.parametrize("kind", [HASH, AUTO])
@pytest.mark.parametrize("filt,joined", [({}, 2975), (ALL_KIND_OR, 1806)],
                         ids=["and", "or_prog"])
def test_all_kinds_unstaged(eng, filt, joined, kind):
    """k_scan_join_agg / k_scan_join_agg_prog; a dense map cannot span the
    int64 range"""
    c = case(tuple(UNSTAGED_BLOCKS), key_kind="raw_fixed", seed=2)
    assert c.table.total_rows == 6000
    assert min(c.block_bytes()) > STAGE_BYTES
    want = run(eng, c, kind, [CH, J], ALL_KIND_AGGS, groups=(15, 15), **filt)
    assert want.rows_passed == joined


# ---- handles, encodings, block verdicts ---------------------------------------

def _extreme_keys(cs, cols, block_rows):
    """-1, INT64_MIN and INT64_MAX in the table; the first two are map keys"""
    cols[K][::50] = -1
    cols[K][1::50] = I64.min
    cols[K][2::50] = I64.max
    keep = cs.map_keys[~np.isin(cs.map_keys, [-1, I64.min, I64.max])]
    cs.map_keys = np.concatenate([keep, [-1, I64.min]]).astype(np.int64)


@pytest.mark.parametrize("kind", [HASH, AUTO])
def test_unstaged_handle_full_range_keys(eng, kind):
    c = case(tuple(UNSTAGED_BLOCKS), key_kind="raw_fixed", seed=2,
             edit=_extreme_keys)
    assert min(c.block_bytes()) > STAGE_BYTES
    for k in (-1, I64.min, I64.max):   # in the table; -1 and MIN are map keys
        assert (c.cols[K] == k).any()
    assert {-1, I64.min} <= set(c.map_keys.tolist())
    run(eng, c, kind, [CH, J], MIXED_AGGS, groups=(10, 15))


@pytest.mark.parametrize("key_nulls", [False, True])
@pytest.mark.parametrize("key_kind", ["raw_fixed", "raw_packed", "intdiff",
                                      "dict"])
def test_probe_column_encodings(eng, key_kind, key_nulls):
    """a NULL key never joins (hit is 0 for it in the reference)"""
    c = case((1000, 700), key_kind=key_kind, key_nulls=key_nulls, seed=3,
             edit=_extreme_keys if key_kind == "raw_fixed" else None)
    if key_nulls:   # rows whose key would have joined, were it not NULL
        assert np.isin(c.cols[K][c.key_null], c.map_keys).any()
    run(eng, c, HASH, [J], MIXED_AGGS, groups=(3, 5))
    if key_kind != "raw_fixed":  # a dense map cannot span the int64 range
        run(eng, c, DENSE, [J], MIXED_AGGS, groups=(3, 5))


def test_block_verdicts(eng):
    """block 1: no key is a map key; block 2: the filter's verdict (O < 20
    against a block of 99s) skips it before the probe"""
    def edit(cs, cols, block_rows):
        absent = np.setdiff1d(10**9 + np.arange(50_000), cs.map_keys)
        cols[K][500:1000] = absent[:500]
        cols[O][1000:1500] = 99
    c = case((500, 500, 500, 500), seed=4, edit=edit)
    assert not c.hit[500:1000].any() and c.hit[1000:1500].any()
    leaves = [dict(col=O, op=abi.OP_LT, lo=20)]
    for kind in (HASH, DENSE):
        run(eng, c, kind, [J, CH], MIXED_AGGS, leaves=leaves, groups=(10, 15))


def test_cs_handle(eng):
    """the fact table loaded from CS blocks (device-side transform); the
    reference scans the same arrays as a PAX blockset"""
    c = case((900, 600), pay_kind="int8_wide", seed=6)
    blobs, r0 = [], 0
    t = c.table
    for rows in t.block_rows:
        s = slice(r0, r0 + rows)
        cs_cols = []
        for ci in range(8):
            spec, _, vals, nulls = t.columns[ci]
            v = vals[s].reshape(-1) if spec == CHAR1 else vals[s]
            cs_cols.append(cs_int_col(
                [int(x) for x in v], enc=2,
                null_rows=None if nulls is None else
                [int(r) for r in np.nonzero(nulls[s])[0]]))
        blobs.append(cs_enc(rows, cs_cols))
        r0 += rows
    # every column as an 8-byte int on both sides
    wide = types.SimpleNamespace()
    wide.table = Table([(INT8, abi.ENC_AUTO,
                         (col[2].reshape(-1) if col[0] == CHAR1
                          else col[2]).astype(np.int64), col[3])
                        for col in t.columns], t.block_rows)
    h = eng.load_cs(blobs, oracle.make_schema([INT8] * 8))
    mid = c.create(eng)
    try:
        aggs = [dict(kind=abi.AGG_SUM, col_a=J), dict(kind=abi.AGG_COUNT),
                dict(kind=abi.AGG_SUM, col_a=V), dict(kind=abi.AGG_MIN, col_a=N)]
        check_join(eng, h, wide, mid, [O], aggs, groups=(20, 20))
    finally:
        eng.keymap_free(mid)
        eng.free(h)


# ---- group counts -------------------------------------------------------------

def test_overflow_to_the_direct_kernel(eng):
    """300 payload values inside one block: past the 16-slot LDS table and
    the 64-row inline result"""
    c = staged(pay_kind="int32_300", seed=7)
    aggs = MIXED_AGGS + [dict(kind=abi.AGG_SUM, col_a=J),
                         dict(kind=abi.AGG_MAX, col_a=J)]
    run(eng, c, HASH, [J], aggs, groups=(250, 300))
    run(eng, c, DENSE, [J, CH], aggs, groups=(600, 900))


def test_more_than_4096_groups(eng):
    c = case((3000, 3000, 3000), pay_kind="int32_unique", share=1.0, seed=8)
    assert len(np.unique(c.cols[K])) > 4096
    h = eng.load(c.table.bs)
    mid = c.create(eng)
    try:
        rc, _ = eng._scan_join_agg(h, abi.make_filter([]), mid, K,
                                   abi.make_agg([J], MIXED_AGGS))
        assert rc == abi.OBX_BUF_NOT_ENOUGH
        assert eng.agg_fetch_all(h) == []
        # a small plan on the same handle still succeeds
        check_join(eng, h, c, mid, [CH], MIXED_AGGS, groups=(3, 3),
                   share=None)
    finally:
        eng.keymap_free(mid)
        eng.free(h)


# ---- maps that join nothing, or everything ------------------------------------

@pytest.mark.parametrize("kind", [HASH, DENSE, AUTO])
def test_empty_map(eng, kind):
    c = case((700, 300), share=0.0)
    want = run(eng, c, kind, [J], MIXED_AGGS, groups=(0, 0), share=None)
    assert want.rows_passed == 0


@pytest.mark.parametrize("kind", [HASH, DENSE])
def test_map_none_of_whose_keys_occur(eng, kind):
    def edit(cs, cols, block_rows):
        cs.map_keys = cs.map_keys + 10**6   # off the key domain
    c = case((700, 300), seed=9, edit=edit)
    want = run(eng, c, kind, [J], MIXED_AGGS, groups=(0, 0), share=None)
    assert want.rows_passed == 0


@pytest.mark.parametrize("kind", [HASH, DENSE])
def test_every_row_hits(eng, kind):
    c = case((700, 300), share=1.0, seed=10)
    want = run(eng, c, kind, [J], MIXED_AGGS, groups=(5, 5), share=None)
    assert want.rows_passed == c.table.total_rows


# ---- filters ------------------------------------------------------------------

def test_and_leaves_with_a_set_leaf(eng):
    c = staged(pay_kind="int32", seed=11)
    h = eng.load(c.table.bs)
    mid = c.create(eng)
    sid = eng.keyset_create([3, 5, 8, 13])
    try:
        leaves = [dict(col=V, op=abi.OP_GE, lo=-300),
                  dict(col=O, op=abi.OP_IN, in_list=[3, 5, 8, 13]),
                  dict(col=N, op=abi.OP_LT, lo=80)]
        gpu_leaves = [leaves[0], dict(col=O, op=abi.OP_IN_SET, set=sid),
                      leaves[2]]
        check_join(eng, h, c, mid, [J, CH], MIXED_AGGS, leaves=leaves,
                   gpu_leaves=gpu_leaves, groups=(10, 15), share=(0.0, 0.2))
    finally:
        eng.keyset_free(sid)
        eng.keymap_free(mid)
        eng.free(h)


OR_LEAVES = [dict(col=V, op=abi.OP_LT, lo=-200),
             dict(col=O, op=abi.OP_EQ, lo=7),
             dict(col=N, op=abi.OP_GE, lo=10)]
OR_PROG = [0, 1, abi.TOK_OR, 2, abi.TOK_AND]


@pytest.mark.parametrize("blocks", [STAGED_BLOCKS, UNSTAGED_BLOCKS])
def test_or_program_few_groups(eng, blocks):
    if blocks is UNSTAGED_BLOCKS:
        c = case(tuple(blocks), key_kind="raw_fixed", seed=2,
                 edit=_extreme_keys)
        assert min(c.block_bytes()) > STAGE_BYTES
    else:
        c = staged(pay_kind="int32", seed=11)
    run(eng, c, HASH, [CH, J], MIXED_AGGS, leaves=OR_LEAVES, prog=OR_PROG,
        groups=(10, 15))


def test_or_program_with_overflow(eng):
    """an LDS-table overflow under a combine program keeps the capacity
    error: the growth path is AND-only"""
    c = staged(pay_kind="int32_300", seed=7)
    want, rows = oracle_rows(c, OR_LEAVES, OR_PROG, [J], MIXED_AGGS)
    assert len(rows) > 64
    h = eng.load(c.table.bs)
    mid = c.create(eng)
    try:
        rc, _ = eng._scan_join_agg(h, abi.make_filter(OR_LEAVES, OR_PROG),
                                   mid, K, abi.make_agg([J], MIXED_AGGS))
        assert rc == abi.OBX_BUF_NOT_ENOUGH
    finally:
        eng.keymap_free(mid)
        eng.free(h)


# ---- keymap_from_proj -----------------------------------------------------------

def _dimension(c, null_attr=False):
    """the build side as a table: key (NULL in some extra rows), attribute,
    and a flag the projection filters on (flag = 0 rows hold keys that are
    not map keys)"""
    rng = np.random.default_rng(21)
    n_map = len(c.map_keys)
    extra = np.setdiff1d(10**9 + np.arange(50_000), c.map_keys)[:400]
    keys = np.concatenate([c.map_keys, extra, np.full(100, 10**9 + 1)])
    attr = np.concatenate([c.map_pay, np.zeros(500, np.int32)])
    flag = np.concatenate([np.ones(n_map), np.zeros(400), np.ones(100)])
    key_null = np.concatenate([np.zeros(n_map + 400, bool), np.ones(100, bool)])
    attr_null = np.zeros(len(keys), bool)
    if null_attr:
        attr_null[7] = True
    perm = rng.permutation(len(keys))
    rows = len(keys)
    return Table([(INT8, abi.ENC_AUTO, keys[perm].astype(np.int64),
                   key_null[perm]),
                  (INT4, abi.ENC_AUTO, attr[perm].astype(np.int32),
                   attr_null[perm] if null_attr else None),
                  (INT8, abi.ENC_AUTO, flag[perm].astype(np.int64), None)],
                 [rows // 2, rows - rows // 2])


@pytest.mark.parametrize("kind", [HASH, DENSE])
def test_from_proj(eng, kind):
    c = staged(pay_kind="int32", seed=11)
    dim = _dimension(c)
    h = eng.load(c.table.bs)
    hd = eng.load(dim.bs)
    mids = []
    try:
        with pytest.raises(engine.KeymapError) as e:  # no result yet
            eng.keymap_from_proj(hd, 0, 1, kind)
        assert e.value.rc == abi.OBX_INVALID_ARGUMENT
        flt = abi.make_filter([dict(col=2, op=abi.OP_EQ, lo=1)])
        n = eng.scan_project(hd, flt, [0, 1])
        assert n == len(c.map_keys) + 100
        mids.append(eng.keymap_from_proj(hd, 0, 1, kind))
        info = eng.keymap_info(mids[0])
        assert info.n_keys == len(c.map_keys) and info.kind == kind
        assert (info.payload_len, info.payload_type) == (4, abi.T_INT32)
        # the same rows fetched to the host
        kb, knull = eng.fetch_proj(hd, 0, 8)
        ab, _ = eng.fetch_proj(hd, 1, 4)
        live = ~np.unpackbits(knull, bitorder="little")[:n].astype(bool)
        mids.append(eng.keymap_create(kb.view(np.int64)[live],
                                      ab.view(np.int32)[live], INT4, kind))
        got = []
        for mid in mids:
            check_join(eng, h, c, mid, [CH, J], MIXED_AGGS, groups=(10, 15))
            got.append(abi.group_row_tuples(eng.agg_fetch_all(h),
                                            len(MIXED_AGGS)))
        assert got[0] == got[1]
    finally:
        for mid in mids:
            eng.keymap_free(mid)
        eng.free(hd)
        eng.free(h)


def test_from_proj_null_payload(eng):
    c = staged(pay_kind="int32", seed=11)
    dim = _dimension(c, null_attr=True)
    hd = eng.load(dim.bs)
    try:
        eng.scan_project(hd, None, [0, 1])
        with pytest.raises(engine.KeymapError) as e:
            eng.keymap_from_proj(hd, 0, 1)
        assert e.value.rc == abi.OBX_NOT_SUPPORTED
    finally:
        eng.free(hd)


# ---- build races ----------------------------------------------------------------

def test_build_races(eng):
    """65 536 distinct keys that are multiples of 2^20: thousands of threads
    insert into shared home slots at once; every key keeps its own payload"""
    def edit(cs, cols, block_rows):
        rng = np.random.default_rng(31)
        keys = (np.arange(65_536, dtype=np.int64) - 30_000) << 20
        cs.map_keys = rng.permutation(keys)
        cs.spec = INT4
        cs.map_pay = ((cs.map_keys >> 20) % 11 - 5).astype(np.int32)
        n = len(cols[K])
        cols[K] = np.where(rng.random(n) < 0.6, rng.choice(keys, n),
                           rng.choice(keys, n) + rng.integers(1, 1 << 20, n))
    c = case((3000, 3000), key_kind="raw_fixed", seed=12, edit=edit)
    h = eng.load(c.table.bs)
    mid = c.create(eng)
    try:
        info = eng.keymap_info(mid)
        assert info.kind == HASH and info.n_keys == 65_536
        assert info.slots_or_span == 131_072 and info.bytes == 16 * 131_072
        check_join(eng, h, c, mid, [J], MIXED_AGGS, groups=(11, 11),
                   share=(0.5, 0.7))
    finally:
        eng.keymap_free(mid)
        eng.free(h)


# ---- lifetime and errors --------------------------------------------------------

def test_lifetime_and_errors(eng):
    c = staged(pay_kind="int32", seed=11)
    h = eng.load(c.table.bs)
    mid = c.create(eng)
    mid8 = eng.keymap_create([1, 2], [5, 6], INT8)
    agg = abi.make_agg([J], [dict(kind=abi.AGG_COUNT)])
    nofilt = abi.make_filter([])

    def rc_of(filt, m, a):
        return eng._scan_join_agg(h, filt, m, K, a)[0]
    try:
        assert rc_of(nofilt, mid, agg) == 0
        # OBX_COL_JOINED where it may not stand
        bad = [abi.make_agg([J], [dict(kind=abi.AGG_SUM_MUL, col_a=V, col_b=J)]),
               abi.make_agg([J], [dict(kind=abi.AGG_SUM_PROD2, col_a=J,
                                       col_b=D)]),
               abi.make_agg([J], [dict(kind=abi.AGG_SUM_PROD3, col_a=V,
                                       col_b=D, col_c=J)]),
               abi.make_agg([J, J], [dict(kind=abi.AGG_COUNT)])]
        for a in bad:
            assert rc_of(nofilt, mid, a) == abi.OBX_INVALID_ARGUMENT
        leaf = abi.make_filter([dict(col=J, op=abi.OP_EQ, lo=3)])
        assert rc_of(leaf, mid, agg) == abi.OBX_INVALID_ARGUMENT
        # the 7-byte group key: 4 + 8 bytes, and an 8-byte payload alone
        assert rc_of(nofilt, mid, abi.make_agg([J, V], [])) == \
            abi.OBX_NOT_SUPPORTED
        assert rc_of(nofilt, mid8, agg) == abi.OBX_NOT_SUPPORTED
        # unknown and freed ids
        assert rc_of(nofilt, 10_000, agg) == abi.OBX_INVALID_ARGUMENT
        assert rc_of(nofilt, -1, agg) == abi.OBX_INVALID_ARGUMENT
        eng.keymap_free(mid8)
        assert rc_of(nofilt, mid8, agg) == abi.OBX_INVALID_ARGUMENT
        for f in (eng.keymap_free, eng.keymap_info):
            with pytest.raises(engine.KeymapError) as e:
                f(mid8)
            assert e.value.rc == abi.OBX_INVALID_ARGUMENT
        # duplicate keys on the device, equal or different payloads
        for pay in ([1, 2, 1], [1, 2, 3]):
            with pytest.raises(engine.KeymapError) as e:
                eng.keymap_create([10, 20, 10], pay, INT4)
            assert e.value.rc == abi.OBX_INVALID_ARGUMENT
        # ids are never reused
        again = eng.keymap_create([1], [1], INT4)
        assert again > mid8
        eng.keymap_free(again)
        # the map still answers after all that
        check_join(eng, h, c, mid, [J], MIXED_AGGS, groups=(3, 5))
    finally:
        eng.keymap_free(mid)
        eng.free(h)
