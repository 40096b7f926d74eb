"""CPU checks of the persistent scan kernel's packed block descriptor
(obx_bdesc): the field packing against dev_block input, through the host
probe that calls the very function k_pack_bdesc runs, and the shape of the
generated block loop -- geometry from the record, loaded once per block
before the stage (no GPU needed: packing and codegen are host code)."""
import ctypes as C

import numpy as np

from oceanbase_amd import abi, oracle

from test_scan_flush_source import _dump, _lib, _lineitem_summaries, _q1

MAX_COLS, MAX_NEED = 8, 12
DF_BITPACK, DF_HAS_EXT, DF_SIGNED, DF_STRING = 1, 2, 4, 8


class DevCol(C.Structure):
    _fields_ = [("data_bit", C.c_uint64), ("ext_bit", C.c_uint64),
                ("dict_byte", C.c_uint64), ("aux_byte", C.c_uint64),
                ("base", C.c_int64), ("count", C.c_uint32),
                ("runs", C.c_uint32), ("enc", C.c_uint8),
                ("flags", C.c_uint8), ("width", C.c_uint8),
                ("entry_len", C.c_uint8), ("rib", C.c_uint8),
                ("rfb", C.c_uint8), ("datum_len", C.c_uint8),
                ("ext_width", C.c_uint8), ("tss", C.c_uint8),
                ("pad", C.c_uint8 * 7)]


class DevBlock(C.Structure):
    _fields_ = [("row_start_lo", C.c_uint32), ("row_start_hi", C.c_uint32),
                ("row_count", C.c_uint32), ("block_len", C.c_uint32),
                ("block_byte", C.c_uint64), ("cols", DevCol * MAX_COLS)]


class BDesc(C.Structure):
    _fields_ = [("block_byte", C.c_uint64), ("block_len", C.c_uint32),
                ("row_count", C.c_uint32), ("slot", C.c_uint64 * MAX_NEED),
                ("pad", C.c_uint64 * 2)]


def test_struct_sizes():
    assert C.sizeof(DevCol) == 64 and C.sizeof(DevBlock) == 536
    assert C.sizeof(BDesc) == 128


def _pack(lib, blk, cols):
    out = BDesc()
    arr = (C.c_uint16 * len(cols))(*cols)
    lib.obx_bdesc_probe.restype = C.c_int
    fits = lib.obx_bdesc_probe(C.byref(blk), arr, len(cols), C.byref(out))
    assert fits in (0, 1), fits
    return fits, out


def _fields(slot):
    """(offset bits, count, width bits, flags) of a slot"""
    return (slot & 0xFFFFFFFF, (slot >> 32) & 0xFFFF, (slot >> 48) & 0xFF,
            slot >> 56)


def _block(block_byte=0x1234560, rows=1322, block_len=16384):
    b = DevBlock()
    b.block_byte, b.row_count, b.block_len = block_byte, rows, block_len
    return b


def _col(b, c, rel_bit, width, flags, count=0):
    b.cols[c].data_bit = b.block_byte * 8 + rel_bit
    b.cols[c].width, b.cols[c].flags, b.cols[c].count = width, flags, count


def _expect(b, c):
    dc = b.cols[c]
    w = dc.width if dc.flags & DF_BITPACK else dc.width * 8
    return ((dc.data_bit - b.block_byte * 8) & 0xFFFFFFFF, dc.count, w,
            dc.flags)


def test_pack_named_cases():
    lib = _lib()
    b = _block()
    _col(b, 0, 1000, 6, DF_BITPACK, count=50)            # bit-packed dict
    _col(b, 1, 8 * 4096, 8, DF_SIGNED)                   # 8-byte RAW
    _col(b, 2, 77, 13, DF_BITPACK | DF_HAS_EXT | DF_SIGNED)
    _col(b, 3, 139263, 1, DF_STRING, count=0)            # 1-byte refs, 0
    _col(b, 4, 5, 255, DF_BITPACK, count=0xFFFF)         # largest that fit
    _col(b, 5, 8, 31, 0, count=1)                        # 31 bytes = 248 bits
    order = [4, 0, 5, 1, 3, 2]                           # the plan's order
    fits, out = _pack(lib, b, order)
    assert fits == 1
    assert (out.block_byte, out.block_len, out.row_count) == (
        b.block_byte, b.block_len, b.row_count)
    for i, c in enumerate(order):
        assert _fields(out.slot[i]) == _expect(b, c), (i, c)
    assert list(out.slot[len(order):]) == [0] * (MAX_NEED - len(order))
    assert list(out.pad) == [0, 0]
    # what the kernel derives from a slot equals what it derived before
    assert _fields(out.slot[3])[0] >> 3 == (
        (b.cols[1].data_bit >> 3) - b.block_byte)        # vb of a raw8 col


def test_first_values_that_do_not_fit_turn_the_path_off():
    lib = _lib()
    for width, flags, count, fits in [
            (255, DF_BITPACK, 0xFFFF, 1),
            (255, DF_BITPACK, 0x10000, 0),    # count needs 17 bits
            (31, 0, 7, 1),
            (32, 0, 7, 0),                    # 32 bytes = 256 bits
            (0, 0, 0, 1)]:
        b = _block()
        _col(b, 0, 64, 6, DF_BITPACK, count=3)
        _col(b, 1, 640, width, flags, count=count)
        got, out = _pack(lib, b, [0, 1])
        assert got == fits, (width, flags, count)
        assert _fields(out.slot[0]) == _expect(b, 0)
        # a column that is not listed does not matter
        assert _pack(lib, b, [0])[0] == 1
    # the handle keeps that verdict per column: a plan that reads it stays
    # on dev_block (no packed record in the generated source)
    filt, agg = _q1()
    s = _lineitem_summaries()
    src, _ = _dump(lib, filt, agg, s)
    assert "bdesc[blk]" in src and "cur.cols[" not in src
    s["maxcnt"][1] = 0x10000
    src, _ = _dump(lib, filt, agg, s)
    assert "bdesc[blk]" not in src and "cur.cols[1].data_bit" in src
    assert "stage2(buf, cur, lds_blk);" in src


def test_pack_random():
    lib = _lib()
    rng = np.random.default_rng(5)
    for _ in range(300):
        b = _block(block_byte=int(rng.integers(0, 1 << 40)) * 16,
                   rows=int(rng.integers(1, 4097)),
                   block_len=int(rng.integers(64, 17408)))
        fit_all = True
        for c in range(MAX_COLS):
            bp = int(rng.integers(2))
            width = int(rng.choice([0, 1, 2, 8, 13, 31, 32, 64, 255]))
            count = int(rng.choice([0, 1, 63, 255, 0xFFFF, 0x10000, 1 << 31]))
            _col(b, c, int(rng.integers(0, 17408 * 8)), width,
                 (DF_BITPACK if bp else 0) | int(rng.integers(8)) << 1,
                 count=count)
        n = int(rng.integers(0, MAX_COLS + 1))
        order = [int(c) for c in rng.permutation(MAX_COLS)[:n]]
        fits, out = _pack(lib, b, order)
        for i, c in enumerate(order):
            want = _expect(b, c)
            ok = want[1] <= 0xFFFF and want[2] <= 0xFF
            fit_all &= ok
            if ok:
                assert _fields(out.slot[i]) == want
        assert fits == int(fit_all)


def test_load_facts_report_a_column_that_does_not_fit():
    """A 40-byte RAW char column (320 bits per value) next to one that
    fits: the load-time fold flags the wide one only."""
    from test_engine_host import _probe
    from test_scan_flush import _manual_blockset
    schema = oracle.make_schema([(abi.T_INT, 0, 19, 8),
                                 (abi.T_CHAR, 0, 0, 40)])
    rng = np.random.default_rng(1)
    v = rng.integers(0, 100, 50).astype(np.int64)
    t = rng.integers(65, 91, 50 * 40).astype(np.uint8)
    blk = oracle.encode_block(schema, [v.view(np.uint8), t],
                              [abi.ENC_RAW, abi.ENC_RAW])
    _, cols = _probe(_manual_blockset(schema, [blk], 50))
    assert not cols[0][0] & 512 and cols[1][0] & 512


# ---- generated block loop --------------------------------------------------

def _q1_loop():
    filt, agg = _q1()
    s = _lineitem_summaries()
    s["cols"][2].scale = s["cols"][3].scale = 2
    src, _ = _dump(_lib(), filt, agg, s, 453858, 256)
    loop = src[src.index("for (uint32_t blk = blockIdx.x"):
               src.index("/* blocks */")]
    return src, loop


def test_q1_block_loop_reads_the_record_only():
    src, loop = _q1_loop()
    assert "#define NBS 7" in src        # 2 group + 4 value + 1 leaf column
    assert "const obx_bdesc *__restrict__ bdesc" in src
    load = "jit_load_meta(cm, bdesc, bleaves, blk);"
    assert loop.count("jit_load_meta(") == loop.count(load) == 1
    for bad in ("cur.cols[", "blocks[blk]", "bl[", "bleaves", "PW("):
        assert bad not in loop.replace(load, ""), bad
    # the names the sweep uses, now from slots
    for name in ("go0", "gW0", "gn0", "go1", "gW1", "gn1", "xo0", "xW0",
                 "xn0", "vb1", "xo2", "xo3", "l0o", "l0W"):
        assert f"const uint32_t {name} = OBX_BD_" in loop, name
    assert "const uint32_t rows = cm.rows;" in loop
    assert "stage2(buf, cm.byte, cm.len, lds_blk);" in loop
    assert "const blk_leaf lb0 = jit_leaf_of(cm.lf[0]);" in loop
    # the one-time builds and the flush still read block 0's dev_block
    assert "const dev_block &b0 = blocks[0];" in src[:src.index(loop[:40])]
    assert "const dev_block &b0 = blocks[0];" in src[src.index("/* blocks */"):]


def test_q1_metadata_is_loaded_once_before_the_stage():
    """One batch of loads at the top of the iteration: the verdict, the
    stage and the sweep preamble all read registers, and nothing is loaded
    between the stage wait and the sweep. (Loading the record one block
    ahead, behind the stage DMA, measured slower than this and was taken
    out again: profiles/r05_scan_bdesc.md.)"""
    _, loop = _q1_loop()
    load = loop.index("jit_load_meta(cm, bdesc, bleaves, blk);")
    verdict = loop.index("blk_verdict")
    stage = loop.index("stage2(")
    wait = loop.index('asm volatile("s_waitcnt vmcnt(0)"')
    assert load < verdict < stage < wait
    assert "jit_load_meta" not in loop[wait:]
    assert "if (blk_verdict == 0) continue;" in loop[verdict:stage]


def test_full_context_column_keeps_its_dev_col():
    """SUM over a CTX column that is not an aligned 8-byte RAW stream: its
    col_ctx alone is still made from dev_block."""
    filt, _ = _q1()
    agg = abi.make_agg([4, 5], [dict(kind=abi.AGG_COUNT),
                                dict(kind=abi.AGG_SUM, col_a=6),
                                dict(kind=abi.AGG_SUM, col_a=1)])
    src, _ = _dump(_lib(), filt, agg, _lineitem_summaries())
    loop = src[src.index("for (uint32_t blk = blockIdx.x"):
               src.index("/* blocks */")]
    assert loop.count("blocks[blk].cols[") == 1
    assert "make_col_ctx(blocks[blk].cols[6], blk_bit);" in loop
    assert "const uint32_t vb1 = OBX_BD_OFF(" in loop


def test_sgrid_caps_the_launch_grid(monkeypatch):
    filt, agg = _q1()
    s = _lineitem_summaries()
    lib = _lib()
    _, grid = _dump(lib, filt, agg, s, 100000, 256)
    assert grid == 256 * 7 * 8
    monkeypatch.setenv("OBX_JIT_SGRID", "3")
    _, grid = _dump(lib, filt, agg, s, 100000, 256)
    assert grid == 3
    _, grid = _dump(lib, filt, agg, s, 2, 256)
    assert grid == 2                       # never more than blocks
    monkeypatch.setenv("OBX_JIT_SGRID", "0")   # not a grid: ignored
    _, grid = _dump(lib, filt, agg, s, 100000, 256)
    assert grid == 256 * 7 * 8
