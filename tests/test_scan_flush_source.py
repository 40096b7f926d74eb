"""CPU checks of the persistent scan kernel's flush codegen, of the launch
grid behind its i64 accumulator bound, and of the per-column summaries that
replace the per-query walks over every block (no GPU needed: codegen,
strategy selection and plan building are host code)."""
import ctypes as C
import os

import numpy as np

from oceanbase_amd import abi, oracle

OBX_NOT_SUPPORTED = -4007


def _lib():
    lib = C.CDLL(os.path.join(os.path.dirname(abi.__file__), "libobx.so"))
    lib.obx_jit_dump_src_ex.restype = C.c_int64
    lib.obx_jit_probe_blocks.restype = C.c_int
    return lib


def _lineitem_summaries(price_max=10500000):
    """Load-time summaries of the Q1 lineitem shape (test_jit_source.py)."""
    n = 7
    cols = (abi.ColSchema * n)()
    for c in range(n):
        cols[c].obj_type = abi.T_INT
    return dict(
        n=n, cols=cols,
        flags=(C.c_uint8 * n)(*[37, 12, 37, 37, 37, 37, 20]),
        cmin=(C.c_int64 * n)(*[0, 90000, 0, 0, 0, 0, 8000]),
        cmax=(C.c_int64 * n)(*[50, price_max, 10, 8, 2, 1, 11000]),
        maxcnt=(C.c_uint32 * n)(*[50, 0, 11, 9, 3, 2, 0]),
        maxw=(C.c_uint32 * n)(*[6, 64, 4, 4, 2, 1, 13]))


def _dump(lib, filt, agg, s, n_blocks=1, n_cus=0, rows_pb=1365):
    buf = C.create_string_buffer(1 << 20)
    grid = C.c_uint32(0)
    sz = lib.obx_jit_dump_src_ex(
        C.byref(filt), C.byref(agg), s["cols"], s["n"], s["flags"],
        s["cmin"], s["cmax"], s["maxcnt"], s["maxw"], rows_pb, 0,
        n_blocks, n_cus, C.byref(grid), buf, len(buf))
    assert sz > 0
    return buf.raw[:sz].decode(), grid.value


def _q1():
    filt = abi.make_filter([dict(col=6, op=abi.OP_LE,
                                 lo=oracle.date_days(1998, 9, 2))])
    agg = abi.make_agg([4, 5], [
        dict(kind=abi.AGG_COUNT),
        dict(kind=abi.AGG_SUM, col_a=0),
        dict(kind=abi.AGG_SUM, col_a=1),
        dict(kind=abi.AGG_SUM_PROD2, col_a=1, col_b=2),
        dict(kind=abi.AGG_SUM_PROD3, col_a=1, col_b=2, col_c=3),
        dict(kind=abi.AGG_SUM, col_a=2)])
    return filt, agg


def test_q1_flush_has_no_per_ref_global_accumulate():
    """Passes 2 (per dict ref) and 3 (per joint-cell slice) accumulate into
    the workgroup's LDS partials; only pass 4 touches the global cells,
    once per (cell, aggregate)."""
    filt, agg = _q1()
    src, _ = _dump(_lib(), filt, agg, _lineitem_summaries())
    p2 = src.index("flush pass 2")
    p4 = src.index("flush pass 4")
    per_ref = src[p2:p4]
    assert "for (uint32_t idx = tid; idx < fcells * 51u" in per_ref
    assert "g_acc_i128" not in per_ref
    assert "cas_minmax(&gtable" not in per_ref
    assert per_ref.count("lds_acc_i128(facc[cell]") == 4   # qty, disc, 2 JWS
    tail = src[p4:]
    assert tail.count("g_acc_i128(gtable[ce].cells[a], lo, hi)") == 1
    assert "idx < fcells * NAGGS" in tail
    # the partials reuse the idle stage buffer: no new LDS array
    assert "(unsigned long long (*)[NAGGS][2])lds_blk" in src
    assert "__shared__ unsigned long long facc" not in src


def test_minmax_flush_reduces_in_workgroup_first():
    """Histogram MIN/MAX: CAS into the LDS partial per ref, one global CAS
    per (cell, aggregate)."""
    filt, _ = _q1()
    agg = abi.make_agg([4, 5], [dict(kind=abi.AGG_COUNT),
                                dict(kind=abi.AGG_MIN, col_a=0),
                                dict(kind=abi.AGG_MAX, col_a=2)])
    src, _ = _dump(_lib(), filt, agg, _lineitem_summaries())
    per_ref = src[src.index("flush pass 2"):src.index("flush pass 4")]
    assert per_ref.count("cas_minmax(&facc[cell]") == 2
    assert "gtable" not in per_ref
    assert "cas_minmax(&gtable[ce].cells[a][0]" in src[src.index(
        "flush pass 4"):]


def test_i64_bound_follows_the_launch_grid():
    """The i64 window bound is max|term| x rows-per-workgroup, and rows per
    workgroup come from the launch grid min(n_blocks, CUs x wpb): the same
    plan over the same blocks keeps the v2 kernel on a wide device and
    loses it (v1 generator) where fewer workgroups share the blocks."""
    lib = _lib()
    filt = abi.make_filter([dict(col=6, op=abi.OP_LE, lo=10500)])
    agg = abi.make_agg([4, 5], [dict(kind=abi.AGG_COUNT),
                                dict(kind=abi.AGG_SUM, col_a=1)])
    s = _lineitem_summaries(price_max=1 << 39)
    n_blocks, rows_pb = 1_000_000, 1365
    src, grid = _dump(lib, filt, agg, s, n_blocks, 256, rows_pb)
    assert "wacc64" in src                       # persistent v2 kernel
    assert grid and grid % 256 == 0
    per_cu = grid // 256          # workgroups the grid gives each CU
    # 2^39 x ceil(1e6 / grid) x 1365 rows < 2^62 there ...
    assert (1 << 39) * -(-n_blocks // grid) * rows_pb < 1 << 62
    # ... and not on a 1-CU device, whose grid is per_cu workgroups
    assert (1 << 39) * -(-n_blocks // per_cu) * rows_pb >= 1 << 62
    src1, grid1 = _dump(lib, filt, agg, s, n_blocks, 1, rows_pb)
    assert "wacc64" not in src1 and "jtab_t" in src1 and grid1 == 0
    # never more workgroups than blocks
    _, grid3 = _dump(lib, filt, agg, s, 3, 256, rows_pb)
    assert grid3 == 3


def test_sweep_narrowing_engages_only_when_proven():
    """32-bit extraction for streams with R x W <= 32; the PROD3 term as one
    u32 x u32 multiply against the combined factor table only when the
    stored bounds prove price in [0, 2^32) and both factors >= 0."""
    lib = _lib()
    filt, agg = _q1()
    s = _lineitem_summaries()
    s["cols"][2].scale = s["cols"][3].scale = 2      # one = 100
    src, _ = _dump(lib, filt, agg, s)
    assert "uint32_t wgr0 = jit_bread32(bv.base, go0 + rbase * gW0);" in src
    assert "uint32_t wx0 = jit_bread32(" in src      # qty: 4 x 6 bits
    assert "uint64_t wl0 = jit_bread(" in src        # date: 4 x 13 bits
    assert "__shared__ uint32_t vtc[12u * 10u];" in src
    assert "(unsigned long long)(uint32_t)v1 *" in src
    assert "vt0[x2] * vt1[x3]" not in src
    # a negative price bound: back to the two-table 64-bit product
    s["cmin"][1] = -5
    src, _ = _dump(lib, filt, agg, s)
    assert "vtc" not in src and "(long long)v1 * vt" in src
    # scale 0: (1 - d) can be negative for d up to 10
    s = _lineitem_summaries()
    src, _ = _dump(lib, filt, agg, s)
    assert "vtc" not in src


# ---- per-column summaries vs the per-block loops they replace -------------

def _old_decision(cls, cnt, gcols, vcols):
    """The walks over every block that build_plan and jit_blocks_ok did
    per query before the summaries."""
    for g in gcols:
        for b in range(cls.shape[0]):
            if (cls[b, g] & 0xF) == 5:
                return OBX_NOT_SUPPORTED
    for b in range(cls.shape[0]):
        cells = 1
        for g in gcols:
            if (cls[b, g] & 0xF) != 1 or cnt[b, g] >= 16:
                return 0
            cells *= int(cnt[b, g]) + 1
        if cells > 16:
            return 0
        for v in vcols:
            if (cls[b, v] & 0xF) > 3 or (cls[b, v] & 0x10):
                return 0
    return 1


def _probe(lib, cls, cnt):
    n = cls.shape[1]
    cols = oracle.make_schema([(abi.T_INT, 0, 19, 8)] * n)
    agg = abi.make_agg([0, 1], [dict(kind=abi.AGG_COUNT),
                                dict(kind=abi.AGG_SUM, col_a=2),
                                dict(kind=abi.AGG_SUM, col_a=3)])
    cls = np.ascontiguousarray(cls, dtype=np.uint8)
    cnt = np.ascontiguousarray(cnt, dtype=np.uint8)
    got = lib.obx_jit_probe_blocks(
        None, C.byref(agg), cols, n,
        cls.ctypes.data_as(C.POINTER(C.c_uint8)),
        cnt.ctypes.data_as(C.POINTER(C.c_uint8)), cls.shape[0])
    assert got == _old_decision(cls, cnt, [0, 1], [2, 3]), (cls, cnt)
    return got


def _base(n_blocks=40):
    cls = np.zeros((n_blocks, 4), dtype=np.uint8)
    cnt = np.zeros((n_blocks, 4), dtype=np.uint8)
    cls[:, 0] = cls[:, 1] = 1          # dict group columns
    cnt[:, 0], cnt[:, 1] = 3, 2        # 4 x 3 = 12 cells
    cls[:, 2], cls[:, 3] = 0, 2        # raw + intdiff value columns
    return cls, cnt


def test_summaries_match_block_walk_named_cases():
    lib = _lib()
    cls, cnt = _base()
    assert _probe(lib, cls, cnt) == 1
    # a span-encoded (class 5) group column in one late block
    c2, n2 = _base()
    c2[37, 1] = 5
    assert _probe(lib, c2, n2) == OBX_NOT_SUPPORTED
    # a group dict count >= 16 in one block
    c2, n2 = _base()
    n2[21, 0] = 16
    assert _probe(lib, c2, n2) == 0
    # a slow value column in one block; a string value column in one block
    c2, n2 = _base()
    c2[39, 3] = 4
    assert _probe(lib, c2, n2) == 0
    c2, n2 = _base()
    c2[0, 2] = 0x10
    assert _probe(lib, c2, n2) == 0
    # a non-dict group column in one block
    c2, n2 = _base()
    c2[5, 0] = 0
    assert _probe(lib, c2, n2) == 0
    # more than 16 cells in one block only
    c2, n2 = _base()
    n2[8, 0], n2[8, 1] = 5, 2
    assert _probe(lib, c2, n2) == 0
    # the column maxima sit in different blocks: their product (8 x 8)
    # exceeds 16 but no block does -- still eligible, as the walk decided
    c2, n2 = _base()
    n2[3, 0], n2[3, 1] = 7, 1
    n2[30, 0], n2[30, 1] = 1, 7
    assert _probe(lib, c2, n2) == 1
    n2[31, 0], n2[31, 1] = 7, 2
    assert _probe(lib, c2, n2) == 0


def test_summaries_match_block_walk_random():
    lib = _lib()
    rng = np.random.default_rng(7)
    seen = set()
    for _ in range(300):
        cls, cnt = _base(int(rng.integers(1, 30)))
        cnt[:, 0] = rng.integers(0, 6, cls.shape[0])
        cnt[:, 1] = rng.integers(0, 4, cls.shape[0])
        for _ in range(int(rng.integers(0, 3))):
            b, c = int(rng.integers(cls.shape[0])), int(rng.integers(4))
            if rng.integers(2):
                cls[b, c] = rng.choice([0, 1, 2, 3, 4, 5, 0x11])
            else:
                cnt[b, c] = rng.choice([0, 7, 15, 16, 255])
        seen.add(_probe(lib, cls, cnt))
    assert seen == {OBX_NOT_SUPPORTED, 0, 1}
