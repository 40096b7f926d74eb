"""CPU checks of the persistent scan kernel's packed joint cells: which form
the strategy picks, and what the generated sweep and flush then hold (no GPU
needed: strategy selection and codegen are host code)."""
import re

from oceanbase_amd import abi

from test_scan_flush_source import _dump, _lib, _lineitem_summaries, _q1

KNOBS = ("OBX_JIT_JPACK", "OBX_JIT_SGRID")


def _clean(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _q1_sf100(s=None):
    """the benchmarked kernel: Q1, scale 2, 453,858 blocks, 256 CUs"""
    filt, agg = _q1()
    s = s or _lineitem_summaries()
    s["cols"][2].scale = s["cols"][3].scale = 2
    return _dump(_lib(), filt, agg, s, 453858, 256, 1322)


def _sweep(src):
    return src[src.index("for (uint32_t it = 0; it < itersR"):
               src.index("/* row sweep */")]


def _lds_bytes(src):
    """bytes of the __shared__ arrays the source declares"""
    env = {m.group(1): int(m.group(2))
           for m in re.finditer(r"#define (\w+) (\d+)$", src, re.M)}
    size = {"uint8_t": 1, "uint32_t": 4, "int": 4, "uint64_t": 8,
            "unsigned long long": 8, "long long": 8}
    total = 0
    for m in re.finditer(r"__shared__ (?:__attribute__\(\(aligned\(16\)\)\) )?"
                         r"([a-z0-9_ ]+?)\s+\w+((?:\[[^\]]+\])+);",
                         src.replace("\n      ", " ")):
        n = 1
        for dim in re.findall(r"\[([^\]]+)\]", m.group(2)):
            n *= eval(re.sub(r"(\d+)u", r"\1", dim), {}, env)
        total += n * size[m.group(1).strip()]
    return total


def test_q1_at_sf100_packs_the_count_into_one_axis(monkeypatch):
    _clean(monkeypatch)
    src, grid = _q1_sf100()
    sweep = _sweep(src)
    # three adds per live row where there were four: the disc histogram is
    # gone, the count rides on the price add; PROD3 keeps its window slot
    # (both axes would be 11.5 KB of cells and an occupancy step)
    assert sweep.count("atomicAdd(") == 3
    assert "atomicAdd(&hist[0u + cell * 51u + x0], 1u);" in sweep
    assert "atomicAdd(&jws[cell * 12u + (x2 < 12u ? x2 : 11u)]," in sweep
    assert "(1ull << 48));" in sweep
    assert "(unsigned long long)(uint32_t)v1 *" in sweep
    assert "__shared__ unsigned long long jws[12u * 12u * 1u];" in src
    assert "#define HTOT 612" in src and "hist[612u" not in src
    assert "wcnt" not in src
    # 32 blocks x 1,322 rows = 42,304 rows take 16 bits; 48 are the weight's
    assert 1 << 15 <= -(-453858 // grid) * 1322 < 1 << 16
    # the occupancy the strategy declares is what its LDS allows
    wpb = int(re.search(r"__launch_bounds__\(256, (\d+)\)", src).group(1))
    lds = _lds_bytes(src)
    assert 16384 + 612 * 4 + 1152 < lds < 23248
    assert wpb == 163840 // (lds + 64) == 7
    assert grid == 256 * 7 * 8
    # the flush splits the cell, and SUM(disc) reads the counts
    flush = src[src.index("flush pass 2"):src.index("flush pass 4")]
    assert "const unsigned long long c = jc >> 48;" in flush
    assert "(__int128)vt3[d0] * (long long)n_pl" in flush
    assert "if (d0 < hc0) { /* excl. null bucket */" in flush
    assert flush.count("lds_acc_i128(facc[cell]") == 4
    # a single block: 1,365 rows take 11 bits
    filt, agg = _q1()
    one_block, _ = _dump(_lib(), filt, agg, _lineitem_summaries())
    assert "(1ull << 53));" in _sweep(one_block)


def test_two_axes_only_under_the_cap(monkeypatch):
    """Without group columns 12 x 10 joint cells are 960 B: both axes stay,
    every member and the count ride on one add, no window slot is left."""
    _clean(monkeypatch)
    filt, _ = _q1()
    agg = abi.make_agg([], [
        dict(kind=abi.AGG_COUNT), dict(kind=abi.AGG_SUM, col_a=1),
        dict(kind=abi.AGG_SUM_PROD2, col_a=1, col_b=2),
        dict(kind=abi.AGG_SUM_PROD3, col_a=1, col_b=2, col_c=3),
        dict(kind=abi.AGG_SUM, col_a=2)])
    s = _lineitem_summaries()
    s["cols"][2].scale = s["cols"][3].scale = 2
    src, _ = _dump(_lib(), filt, agg, s, 453858, 256, 1322)
    sweep = _sweep(src)
    assert sweep.count("atomicAdd(") == 1
    assert "atomicAdd(&jws[cell * 120u + " in sweep
    assert "wacc64[" not in src and "vtc" not in src and "wcnt" not in src
    assert "cnt2 += jws[cell * 120u + j2] >> " in src


def test_knob_off_is_the_unpacked_kernel(monkeypatch):
    _clean(monkeypatch)
    monkeypatch.setenv("OBX_JIT_JPACK", "0")
    src, grid = _q1_sf100()
    sweep = _sweep(src)
    assert sweep.count("atomicAdd(") == 4
    assert "atomicAdd(&hist[612u + cell * 12u + x2], 1u);" in sweep
    assert "if (!nu1)\n            atomicAdd(&jws[cell * 12u + " in sweep
    assert "1ull <<" not in sweep and "jc >>" not in src
    assert "__shared__ uint32_t vtc[12u * 10u];" in src
    assert "#define HTOT 756" in src and grid == 256 * 7 * 8


def _unpacked(monkeypatch, s):
    monkeypatch.setenv("OBX_JIT_JPACK", "0")
    src, grid = _q1_sf100(s)
    monkeypatch.delenv("OBX_JIT_JPACK")
    return src, grid


def test_a_failed_precondition_leaves_the_unpacked_form(monkeypatch):
    _clean(monkeypatch)

    def summaries(**over):
        s = _lineitem_summaries()
        for k, (c, v) in over.items():
            s[k][c] = v
        return s
    assert "1ull << 48" in _q1_sf100(summaries())[0]
    for over in (dict(cmin=(1, -1)),        # a negative weight
                 dict(flags=(1, 12 | 2)),   # the weight can be NULL
                 dict(flags=(1, 8))):       # its bounds are not known
        got = _q1_sf100(summaries(**over))
        want = _unpacked(monkeypatch, summaries(**over))
        assert got == want, over
        if "jtab_t" in got[0]:      # unknown bounds: not this kernel at all
            assert "flags" in over and over["flags"][1] == 8
        else:
            assert "1ull <<" not in _sweep(got[0])


def test_packing_bound_follows_the_launch_grid(monkeypatch):
    """The count takes the bits of the rows one workgroup can sweep at the
    launched grid, the weight sum the rest: the largest price maximum that
    still packs is computed from the grid the dump reports."""
    _clean(monkeypatch)
    lib = _lib()
    filt = abi.make_filter([dict(col=6, op=abi.OP_LE, lo=10500)])
    agg = abi.make_agg([4, 5], [dict(kind=abi.AGG_COUNT),
                                dict(kind=abi.AGG_SUM, col_a=1),
                                dict(kind=abi.AGG_SUM_PROD2, col_a=1,
                                     col_b=2)])
    n_blocks, rows_pb = 1_000_000, 1365
    _, grid = _dump(lib, filt, agg, _lineitem_summaries(), n_blocks, 256,
                    rows_pb)
    maxrows = -(-n_blocks // grid) * rows_pb
    shift = 64 - maxrows.bit_length()
    top = ((1 << shift) - 1) // maxrows       # top * maxrows < 2^shift
    assert (top + 1) * maxrows >= 1 << shift
    src, g2 = _dump(lib, filt, agg, _lineitem_summaries(price_max=top),
                    n_blocks, 256, rows_pb)
    assert g2 == grid and f"(1ull << {shift}));" in _sweep(src)
    assert "wcnt" not in src                  # COUNT(*) from the joint cells
    assert f"cnt2 += jws[cell * 12u + j2] >> {shift};" in src
    src, g2 = _dump(lib, filt, agg, _lineitem_summaries(price_max=top + 1),
                    n_blocks, 256, rows_pb)
    assert g2 == grid and "1ull <<" not in _sweep(src)
    assert "atomicAdd(&wcnt[cell][stripe], 1u);" in _sweep(src)
    assert "wacc64" in src                    # still the persistent kernel
    # a grid cap gives the workgroup more rows, the count more bits and the
    # weight fewer: the lineitem price no longer fits, a small one does
    monkeypatch.setenv("OBX_JIT_SGRID", "64")
    big = -(-n_blocks // 64) * rows_pb
    shift = 64 - big.bit_length()
    assert 10500000 * big >= 1 << shift > 1000 * big
    src, g3 = _dump(lib, filt, agg, _lineitem_summaries(), n_blocks, 256,
                    rows_pb)
    assert g3 == 64 and "1ull <<" not in _sweep(src)
    s = _lineitem_summaries(price_max=1000)
    s["cmin"][1] = 0
    src, g3 = _dump(lib, filt, agg, s, n_blocks, 256, rows_pb)
    assert g3 == 64 and f"(1ull << {shift}));" in _sweep(src)


def test_axis_aggregates_read_the_counts_of_their_axis(monkeypatch):
    """COUNT(col), SUM and MIN/MAX over both axis columns, no group column:
    no histogram is left, and the row count comes from the joint cells."""
    _clean(monkeypatch)
    filt, _ = _q1()
    agg = abi.make_agg([], [
        dict(kind=abi.AGG_COUNT), dict(kind=abi.AGG_SUM, col_a=1),
        dict(kind=abi.AGG_SUM_PROD3, col_a=1, col_b=2, col_c=3),
        dict(kind=abi.AGG_SUM, col_a=3), dict(kind=abi.AGG_COUNT, col_a=3),
        dict(kind=abi.AGG_MIN, col_a=3), dict(kind=abi.AGG_MAX, col_a=2),
        dict(kind=abi.AGG_COUNT, col_a=2)])
    src, _ = _dump(_lib(), filt, agg, _lineitem_summaries())
    assert "#define HTOT 1\n" in src and "atomicAdd(&hist[" not in src
    assert _sweep(src).count("atomicAdd(") == 1
    flush = src[src.index("flush pass 2"):src.index("flush pass 4")]
    for text in ("h1_3 += (__int128)vt", "h1_4 += c;",
                 "cas_minmax(&facc[cell][5][0],",
                 "cas_minmax(&facc[cell][6][0],",
                 "atomicAdd(&facc[cell][7][0], n_pl);",
                 "if (d1 < hc1) { /* excl. null bucket */"):
        assert text in flush, text
