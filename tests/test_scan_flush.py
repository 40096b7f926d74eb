"""GPU parity of the persistent scan kernel's flush and launch grid, and of
the per-call state the engine keeps across queries (load-time column
summaries, device-side table init, pinned result buffer).

The kernel reduces histogram- and joint-cell-weighted aggregates inside the
workgroup (exact int128 in LDS) and sends one global accumulate per (cell,
aggregate); its grid is the resident set, CUs x workgroups-per-CU. Every
case compares `abi.result_rows` exactly against the CPU oracle and asserts
that the specialized kernel ran.
"""
import ctypes as Ct

import numpy as np
import pytest

from oceanbase_amd import abi, oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from oceanbase_amd.engine import GpuEngine
    e = GpuEngine(0)
    yield e
    e.close()


def _v2(eng):
    """The persistent (v2) generator ran, not v1 or the generic kernels."""
    return eng._lib.obx_gpu_last_jit(eng._ctx) == 2


def _manual_blockset(schema, blocks_bytes, total_rows):
    """Build a BlockSet over concatenated (16-B aligned) encoded blocks."""
    aligned = []
    offs = [0]
    for b in blocks_bytes:
        body = b[:-16]  # strip the slack suffix encode_block appends
        pad = (-len(body)) % 16
        aligned.append(body + b"\x00" * pad)
        offs.append(offs[-1] + len(body) + pad)
    data = np.frombuffer(b"".join(aligned) + b"\x00" * 16, dtype=np.uint8)
    offarr = np.array(offs, dtype=np.uint64)
    bs = abi.BlockSet()
    bs.data = data.ctypes.data_as(Ct.POINTER(Ct.c_uint8))
    bs.block_offsets = offarr.ctypes.data_as(Ct.POINTER(Ct.c_uint64))
    bs.n_blocks = len(blocks_bytes)
    bs.n_cols = len(schema)
    bs.cols = Ct.cast(schema, Ct.POINTER(abi.ColSchema))
    bs.total_rows = total_rows
    bs._keep = (data, offarr, schema)  # keep alive
    return bs


def _q1_descs():
    filt = abi.make_filter([
        dict(col=6, op=abi.OP_LE, lo=oracle.date_days(1998, 9, 2))])
    agg = abi.make_agg([4, 5], [
        dict(kind=abi.AGG_COUNT),
        dict(kind=abi.AGG_SUM, col_a=0),
        dict(kind=abi.AGG_SUM, col_a=1),
        dict(kind=abi.AGG_SUM_PROD2, col_a=1, col_b=2),
        dict(kind=abi.AGG_SUM_PROD3, col_a=1, col_b=2, col_c=3),
        dict(kind=abi.AGG_SUM, col_a=2),
    ])
    return filt, agg


def _check(eng, h, bs, filt, agg, n_aggs, v2=True):
    res_gpu = eng.scan_filter_agg(h, filt, agg)
    assert eng.last_jit()
    if v2:
        assert _v2(eng)
    res_cpu = oracle.scan_filter_agg(bs, filt, agg)
    assert res_gpu.rows_passed == res_cpu.rows_passed
    rows = abi.result_rows(res_gpu, n_aggs)
    assert rows == abi.result_rows(res_cpu, n_aggs)
    return res_gpu, rows


# ---- block counts around the grid ---------------------------------------

@pytest.mark.parametrize("n_blocks,rows", [(1, 1000), (3, 3500)])
def test_q1_few_blocks(eng, n_blocks, rows):
    """Fewer blocks than workgroup slots: the grid is the block count."""
    li = oracle.Lineitem(4, rows, seed=5)
    assert li.n_blocks == n_blocks
    h = eng.load(li.bs)
    filt, agg = _q1_descs()
    _check(eng, h, li.bs, filt, agg, 6)
    eng.free(h)


def _resident(eng):
    import torch
    # Q1 keeps 7 workgroups per CU (LDS-bound)
    return torch.cuda.get_device_properties(0).multi_processor_count * 7


def _q1_with_blocks(n_blocks):
    probe = oracle.Lineitem(4, 200_000, seed=42)
    return oracle.Lineitem(4, int(n_blocks * 200_000 / probe.n_blocks),
                           seed=42)


def test_q1_blocks_just_above_resident_set(eng):
    """A block count just above CUs x workgroups-per-CU: one block per
    workgroup and more workgroups than are resident at once."""
    res_set = _resident(eng)
    li = _q1_with_blocks(res_set + 60)
    assert res_set < li.n_blocks < 2 * res_set, (res_set, li.n_blocks)
    h = eng.load(li.bs)
    filt, agg = _q1_descs()
    res, rows = _check(eng, h, li.bs, filt, agg, 6)
    assert sum(rc for _, rc, _ in rows) == res.rows_passed
    eng.free(h)


def test_q1_blocks_just_above_launch_grid(eng):
    """A block count just above the launch grid (8 x the resident set; the
    engine reports the grid it launched): some workgroups sweep two blocks
    and the others one."""
    li = _q1_with_blocks(8 * _resident(eng) + 80)
    h = eng.load(li.bs)
    filt, agg = _q1_descs()
    res, rows = _check(eng, h, li.bs, filt, agg, 6)
    grid = eng._lib.obx_gpu_last_grid(eng._ctx)
    assert grid < li.n_blocks < 2 * grid, (grid, li.n_blocks)
    assert sum(rc for _, rc, _ in rows) == res.rows_passed
    eng.free(h)


# ---- hand-made block sets -------------------------------------------------

_G = np.frombuffer(b"NPZ", dtype=np.uint8)   # group key bytes
_D = np.array([-7, -3, 0, 2, 5], dtype=np.int64)        # signed dict (+ -5)
_B = np.array([0, 4, 10], dtype=np.int64)               # "discount" dict
_C = np.array([0, 2, 8], dtype=np.int64)                # "tax" dict


def _signed_blocks(n_blocks=5, rows_pb=1100, seed=3):
    """cols: 0 grp CHAR dict, 1 d signed dict, 2 r raw int64 (negatives),
    3 b dict dec(2), 4 c dict dec(2), 5 k raw int64 == block index.

    Group Z sums to exactly 0 in d, r and every product (paired rows
    +v / -v with equal b, c); group N is all-negative; group P is mixed.
    Every block holds every dict value, so the dicts are byte-identical.
    |r| < 2^30 keeps |r| x 110 x 108 x rows-per-workgroup under the 2^62
    bound of the i64 window accumulators, so the persistent kernel runs."""
    rng = np.random.default_rng(seed)
    schema = oracle.make_schema([
        (abi.T_CHAR, 0, 0, 1), (abi.T_INT, 0, 19, 8), (abi.T_INT, 0, 19, 8),
        (abi.T_DECIMAL_INT, 2, 15, 8), (abi.T_DECIMAL_INT, 2, 15, 8),
        (abi.T_INT, 0, 19, 8)])
    blocks = []
    for blk in range(n_blocks):
        nz = 2 * int(rng.integers(20, 60))      # even: +/- pairs
        nn = int(rng.integers(100, 300))
        npz = rows_pb - nz - nn
        g = np.concatenate([np.full(nz, _G[2]), np.full(nn, _G[0]),
                            np.full(npz, _G[1])])
        zb = np.repeat(rng.choice(_B, nz // 2), 2)
        zc = np.repeat(rng.choice(_C, nz // 2), 2)
        d = np.concatenate([np.tile(np.array([5, -5]), nz // 2),
                            rng.choice(_D[:2], nn), rng.choice(_D, npz)])
        zmag = rng.integers(1, 1 << 30, nz // 2)
        r = np.concatenate([np.stack([zmag, -zmag], 1).reshape(-1),
                            -rng.integers(1, 1 << 30, nn),
                            rng.integers(-(1 << 30), 1 << 30, npz)])
        b = np.concatenate([zb, rng.choice(_B, nn), rng.choice(_B, npz)])
        c = np.concatenate([zc, rng.choice(_C, nn), rng.choice(_C, npz)])
        # force every dict value into the block (tail of group P)
        dvals = np.array([-7, -5, -3, 0, 2, 5], dtype=np.int64)
        d[-len(dvals):] = dvals
        b[-3:] = _B
        c[-3:] = _C
        k = np.full(rows_pb, blk, dtype=np.int64)
        cols = [g.astype(np.uint8), d.astype(np.int64).view(np.uint8),
                r.astype(np.int64).view(np.uint8),
                b.astype(np.int64).view(np.uint8),
                c.astype(np.int64).view(np.uint8), k.view(np.uint8)]
        blocks.append(oracle.encode_block(
            schema, cols, [abi.ENC_DICT, abi.ENC_DICT, abi.ENC_RAW,
                           abi.ENC_DICT, abi.ENC_DICT, abi.ENC_RAW]))
    return _manual_blockset(schema, blocks, n_blocks * rows_pb)


@pytest.fixture(scope="module")
def signed(eng):
    bs = _signed_blocks()
    h = eng.load(bs)
    yield bs, h
    eng.free(h)


def _group(rows, byte):
    hit = [r for r in rows if bytes(r[0])[:1] == byte]
    assert len(hit) == 1, rows
    return hit[0]


def test_signed_hist_and_window_sums(eng, signed):
    """Negative dict entries under a histogram SUM and negative RAW values
    under the i64 window SUM (one candidate only: no joint cells)."""
    bs, h = signed
    agg = abi.make_agg([0], [dict(kind=abi.AGG_COUNT),
                             dict(kind=abi.AGG_SUM, col_a=1),
                             dict(kind=abi.AGG_SUM, col_a=2),
                             dict(kind=abi.AGG_COUNT, col_a=1)])
    _, rows = _check(eng, h, bs, None, agg, 4)
    z = _group(rows, b"Z")
    assert z[1] > 0 and z[2][1] == 0 and z[2][2] == 0  # zero sums, shown
    n = _group(rows, b"N")
    assert n[2][1] < 0 and n[2][2] < 0                 # sign-extended cells


def test_signed_joint_cells_products(eng, signed):
    """SUM / PROD2 / PROD3 over one negative RAW weight column fold into
    the joint weighted cells; their flush goes through the in-workgroup
    int128 reduce into the 256-bit cells."""
    bs, h = signed
    agg = abi.make_agg([0], [dict(kind=abi.AGG_SUM, col_a=2),
                             dict(kind=abi.AGG_SUM_PROD2, col_a=2, col_b=3),
                             dict(kind=abi.AGG_SUM_PROD3, col_a=2, col_b=3,
                                  col_c=4),
                             dict(kind=abi.AGG_SUM, col_a=1)])
    _, rows = _check(eng, h, bs, None, agg, 4)
    z = _group(rows, b"Z")
    assert z[1] > 0 and list(z[2]) == [0, 0, 0, 0]
    n = _group(rows, b"N")
    assert all(v < 0 for v in n[2])


def test_no_row_survives(eng, signed):
    bs, h = signed
    agg = abi.make_agg([0], [dict(kind=abi.AGG_COUNT),
                             dict(kind=abi.AGG_SUM, col_a=1)])
    filt = abi.make_filter([dict(col=5, op=abi.OP_LT, lo=-1)])
    res, rows = _check(eng, h, bs, filt, agg, 2)
    assert res.rows_passed == 0 and res.n_groups == 0 and rows == []


def test_whole_blocks_without_survivors(eng, signed):
    """Only blocks 0 and 1 hold survivors: the other workgroups flush
    nothing."""
    bs, h = signed
    agg = abi.make_agg([0], [dict(kind=abi.AGG_COUNT),
                             dict(kind=abi.AGG_SUM, col_a=1),
                             dict(kind=abi.AGG_SUM, col_a=2)])
    filt = abi.make_filter([dict(col=5, op=abi.OP_LE, lo=1)])
    res, _ = _check(eng, h, bs, filt, agg, 3)
    assert res.rows_passed == 2 * 1100


def _null_blocks(n_blocks=4, rows_pb=900, seed=9):
    """cols: 0 grp CHAR dict, 1 dict value col with NULLs (ref == count),
    2 RAW value col with NULLs."""
    rng = np.random.default_rng(seed)
    schema = oracle.make_schema([(abi.T_CHAR, 0, 0, 1),
                                 (abi.T_INT, 0, 19, 8),
                                 (abi.T_INT, 0, 19, 8)])
    dv = np.array([-40, -1, 6, 33], dtype=np.int64)
    blocks = []
    for _ in range(n_blocks):
        g = rng.choice(np.frombuffer(b"XY", dtype=np.uint8), rows_pb)
        d = rng.choice(dv, rows_pb)
        d[:4] = dv
        g[:2] = np.frombuffer(b"XY", dtype=np.uint8)
        r = rng.integers(-10**9, 10**9, rows_pb).astype(np.int64)
        n1 = np.zeros((rows_pb + 7) // 8, dtype=np.uint8)
        n2 = np.zeros((rows_pb + 7) // 8, dtype=np.uint8)
        for i in range(5, rows_pb, 7):
            n1[i >> 3] |= 1 << (i & 7)
        for i in range(6, rows_pb, 11):
            n2[i >> 3] |= 1 << (i & 7)
        blocks.append(oracle.encode_block(
            schema, [g, d.view(np.uint8), r.view(np.uint8)],
            [abi.ENC_DICT, abi.ENC_DICT, abi.ENC_RAW], [None, n1, n2]))
    return _manual_blockset(schema, blocks, n_blocks * rows_pb)


def test_dict_nulls_sum_count_min_max(eng):
    """NULLs in a dict value column (null bucket excluded from SUM,
    COUNT(col), MIN, MAX at flush) and MIN/MAX of a nullable RAW column
    through the LDS CAS cells."""
    bs = _null_blocks()
    h = eng.load(bs)
    agg = abi.make_agg([0], [dict(kind=abi.AGG_COUNT),
                             dict(kind=abi.AGG_SUM, col_a=1),
                             dict(kind=abi.AGG_COUNT, col_a=1),
                             dict(kind=abi.AGG_MIN, col_a=1),   # histogram
                             dict(kind=abi.AGG_MAX, col_a=1),
                             dict(kind=abi.AGG_MIN, col_a=2),   # CAS cells
                             dict(kind=abi.AGG_MAX, col_a=2)])
    _, rows = _check(eng, h, bs, None, agg, 7)
    for _, rc, cells in rows:
        assert cells[2] < rc               # some rows are NULL
        assert cells[3] == -40 and cells[4] == 33
    eng.free(h)


# ---- state carried from call to call ----------------------------------------

def test_filter_x_y_x_on_one_handle(eng, signed):
    """MIN/MAX sentinels, counters and the result buffer are rebuilt per
    call: X, then Y with other aggregate kinds in the same slots, then X."""
    bs, h = signed
    agg_x = abi.make_agg([0], [dict(kind=abi.AGG_MIN, col_a=1),
                               dict(kind=abi.AGG_MAX, col_a=2),
                               dict(kind=abi.AGG_SUM, col_a=1)])
    agg_y = abi.make_agg([0], [dict(kind=abi.AGG_SUM, col_a=2),
                               dict(kind=abi.AGG_COUNT),
                               dict(kind=abi.AGG_MAX, col_a=1)])
    fx = abi.make_filter([dict(col=5, op=abi.OP_GE, lo=2)])
    fy = abi.make_filter([dict(col=5, op=abi.OP_LE, lo=3)])
    r1, rows1 = _check(eng, h, bs, fx, agg_x, 3)
    _check(eng, h, bs, fy, agg_y, 3)
    r3, rows3 = _check(eng, h, bs, fx, agg_x, 3)
    assert rows1 == rows3 and r1.rows_passed == r3.rows_passed


def test_alternating_handles_jit_and_generic(eng, signed):
    """A JIT-eligible handle and one that is not (RAW group column),
    queried in turn: the path taken follows the handle every time."""
    bs, h = signed
    rng = np.random.default_rng(12)
    schema = oracle.make_schema([(abi.T_INT, 0, 19, 8),
                                 (abi.T_INT, 0, 19, 8)])
    blocks = []
    for _ in range(3):
        g = rng.integers(0, 3, 800).astype(np.int64)
        v = rng.integers(-50, 50, 800).astype(np.int64)
        blocks.append(oracle.encode_block(
            schema, [g.view(np.uint8), v.view(np.uint8)],
            [abi.ENC_RAW, abi.ENC_RAW]))
    bs2 = _manual_blockset(schema, blocks, 2400)
    h2 = eng.load(bs2)
    agg = abi.make_agg([0], [dict(kind=abi.AGG_COUNT),
                             dict(kind=abi.AGG_SUM, col_a=1)])
    want1 = abi.result_rows(oracle.scan_filter_agg(bs, None, agg), 2)
    want2 = abi.result_rows(oracle.scan_filter_agg(bs2, None, agg), 2)
    for _ in range(3):
        got = eng.scan_filter_agg(h, None, agg)
        assert eng.last_jit() and _v2(eng)
        assert abi.result_rows(got, 2) == want1
        got = eng.scan_filter_agg(h2, None, agg)
        assert not eng.last_jit()
        assert abi.result_rows(got, 2) == want2
    eng.free(h2)
