"""Hash group-by past 4096 groups: the sized table (csrc/obx_grouphash.h)
under a raised cap (obx_gpu_set_max_groups).

Two tables (built from numpy through oracle.encode_block, 16.8 M rows by
default, 1024-row blocks so every block is LDS-staged), no filter: four int32
key columns drawn from d = 4 000, 65 536, 1 000 000 and 4 000 000 values and
an int64 value `val`.
  random   every key drawn uniformly
  runs4    key = (row // 4) % d: sorted in runs of 4 adjacent rows, the
           l_orderkey shape
Per table and d: GROUP BY the key column, COUNT(*) + SUM(val), cap =
max(d, 8192), through the generic kernels (OBX_JIT=0). Reported per point,
median (min-max) of --steps runs after --warmup:
  hash ms   device time of the sized-table kernel alone
            (obx_gpu_last_group_ms)
  first ms  device time of the first scan, whose LDS tables overflow
            (obx_gpu_last_kernel_ms)
  verb ms   wall time of the whole verb: two scans, compaction, the copy of
            the live records, the host's sort and row build
The group count, the survivor count and the first page of rows are checked
against numpy at every point.

At d = 4 000 the 4096-slot path (the default cap) is measured too, as the
wall time of the verb (the engine does not time that path's second kernel):
with this build and, given --direct-so PATH, with another build of the
library (the parent commit's), both on the same table, alternating inside
one loop.

--so PATH runs everything on another build of the current library (an A/B
of a kernel variant).

Run on a GPU box:  python tools/bench_group_hash.py
Prints one JSON object per measured point and markdown tables at the end.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from oceanbase_amd import abi, engine, oracle  # noqa: E402

INT8 = (abi.T_INT, 0, 19, 8)
INT4 = (abi.T_INT32, 0, 10, 4)
BLOCK_ROWS = 1024
DOMAINS = (4_000, 65_536, 1_000_000, 4_000_000)
VAL = len(DOMAINS)
AGGS = [dict(kind=abi.AGG_COUNT), dict(kind=abi.AGG_SUM, col_a=VAL)]


def build_table(rows, shape, seed=7):
    """-> (blockset, the key columns, val, bytes of the largest block)"""
    rng = np.random.default_rng(seed)
    if shape == "random":
        keys = [rng.integers(0, d, rows).astype(np.int32) for d in DOMAINS]
    else:
        keys = [((np.arange(rows) // 4) % d).astype(np.int32)
                for d in DOMAINS]
    val = rng.integers(-50_000, 50_000, rows).astype(np.int64)
    cols = keys + [val]
    specs = [INT4] * len(DOMAINS) + [INT8]
    schema = oracle.make_schema(specs)
    encs = [abi.ENC_AUTO] * len(specs)
    blocks = []
    for r0 in range(0, rows, BLOCK_ROWS):
        raw = [np.ascontiguousarray(c[r0:r0 + BLOCK_ROWS]).view(np.uint8)
               .reshape(-1) for c in cols]
        blocks.append(oracle.encode_block(schema, raw, encs))
    parts, offs = [], [0]
    for blk in blocks:
        body = blk[:-16]
        parts.append(body + b"\x00" * ((-len(body)) % 16))
        offs.append(offs[-1] + len(parts[-1]))
    data = np.frombuffer(b"".join(parts) + b"\x00" * 16, dtype=np.uint8)
    offarr = np.array(offs, dtype=np.uint64)
    bs = abi.BlockSet()
    bs.data = data.ctypes.data_as(C.POINTER(C.c_uint8))
    bs.block_offsets = offarr.ctypes.data_as(C.POINTER(C.c_uint64))
    bs.n_blocks, bs.n_cols = len(blocks), len(specs)
    bs.cols = C.cast(schema, C.POINTER(abi.ColSchema))
    bs.total_rows = rows
    bs._keep = (data, offarr, schema)
    return bs, keys, val, max(len(blk) - 16 for blk in blocks)


class PlainEngine:
    """the few verbs the 4096-slot comparison needs, bound by hand: a build
    of the library from before the cap has no obx_gpu_set_max_groups, which
    engine.GpuEngine insists on"""

    def __init__(self, path):
        lib = C.CDLL(path)
        lib.obx_gpu_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.obx_gpu_close.argtypes = [C.c_void_p]
        lib.obx_gpu_load_blocks.argtypes = [C.c_void_p,
                                            C.POINTER(abi.BlockSet)]
        lib.obx_gpu_free_blocks.argtypes = [C.c_void_p, C.c_int]
        lib.obx_gpu_scan_filter_agg.argtypes = [
            C.c_void_p, C.c_int, C.POINTER(abi.FilterDesc),
            C.POINTER(abi.AggDesc), C.POINTER(abi.AggResult)]
        lib.obx_gpu_agg_fetch.argtypes = [
            C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p,
            C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        self._lib, self._ctx = lib, C.c_void_p()
        rc = lib.obx_gpu_open(0, C.byref(self._ctx))
        assert rc == 0, rc

    def load(self, bs):
        h = self._lib.obx_gpu_load_blocks(self._ctx, C.byref(bs))
        assert h >= 0, h
        return h

    def close(self):
        self._lib.obx_gpu_close(self._ctx)


def scan(eng, h, agg):
    """-> (status, AggResult, wall ms)"""
    res = abi.AggResult()
    t0 = time.perf_counter()
    rc = eng._lib.obx_gpu_scan_filter_agg(eng._ctx, h, None, C.byref(agg),
                                          C.byref(res))
    return rc, res, (time.perf_counter() - t0) * 1e3


def first_page(eng, h, n=256):
    buf = (abi.GroupRow * n)()
    n_out, total = C.c_uint32(), C.c_uint64()
    rc = eng._lib.obx_gpu_agg_fetch(eng._ctx, h, 0, n, buf, C.byref(n_out),
                                    C.byref(total))
    assert rc == 0, rc
    return abi.group_row_tuples(list(buf[:n_out.value]), len(AGGS)), \
        total.value


def want_first_page(key, val, n=256):
    """the first n groups in key-byte order: little-endian int32 bytes"""
    uniq = np.unique(key)
    first = uniq[np.argsort(uniq.astype(np.uint32).byteswap(),
                            kind="stable")[:n]]
    by_value = np.sort(first)
    m = np.isin(key, by_value)
    idx = np.searchsorted(by_value, key[m])
    cnt = np.bincount(idx, minlength=len(by_value))
    sums = np.zeros(len(by_value), dtype=np.int64)
    np.add.at(sums, idx, val[m])
    out = []
    for k in first.tolist():
        i = int(np.searchsorted(by_value, k))
        out.append((int(k).to_bytes(4, "little"), int(cnt[i]),
                    [int(cnt[i]), int(sums[i])]))
    return out, len(uniq)


def mmm(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3),
            round(max(xs), 3)]


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_400 * BLOCK_ROWS)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", nargs="+", default=["random", "runs4"])
    ap.add_argument("--domains", type=int, nargs="+", default=list(DOMAINS),
                    help="measure only these d")
    ap.add_argument("--so", help="run on this build of the library")
    ap.add_argument("--direct-so", help="a second build to measure the "
                    "4096-slot path with, at d = 4000")
    args = ap.parse_args()
    os.environ["OBX_JIT"] = "0"   # like for like: the generic kernels
    if args.so:
        engine._SO = os.path.abspath(args.so)
    print(json.dumps(dict(so=engine._SO, direct_so=args.direct_so)),
          flush=True)

    sized, direct = [], []
    for shape in args.shapes:
        t0 = time.perf_counter()
        bs, keys, val, max_block = build_table(args.rows, shape)
        assert max_block <= 17408, max_block
        eng = engine.GpuEngine(0)
        h = eng.load(bs)
        print(json.dumps(dict(shape=shape, rows=args.rows,
                              bytes=eng.total_bytes(h),
                              max_block_bytes=max_block,
                              gen_seconds=round(time.perf_counter() - t0,
                                                1))), flush=True)
        for col, d in enumerate(DOMAINS):
            if d not in args.domains:
                continue
            agg = abi.make_agg([col], AGGS)
            want, n_groups = want_first_page(keys[col], val)
            eng.set_max_groups(max(d, 8192))
            hash_ms, first_ms, verb_ms = [], [], []
            for i in range(args.warmup + args.steps):
                rc, res, wall = scan(eng, h, agg)
                assert rc == abi.OBX_BUF_NOT_ENOUGH, rc
                assert res.n_groups == n_groups, (res.n_groups, n_groups)
                assert res.rows_passed == args.rows
                if i == 0:
                    got, total = first_page(eng, h)
                    assert total == n_groups and got == want, (shape, d)
                if i >= args.warmup:
                    hash_ms.append(eng.last_group_ms())
                    first_ms.append(eng.last_kernel_ms())
                    verb_ms.append(wall)
            rec = dict(shape=shape, d=d, groups=n_groups,
                       slots=eng.last_group_slots(), hash_ms=mmm(hash_ms),
                       first_ms=mmm(first_ms), verb_ms=mmm(verb_ms),
                       mrows_per_s=round(args.rows / 1e3 /
                                         statistics.median(hash_ms), 1))
            print(json.dumps(rec), flush=True)
            sized.append(f"| {shape} | {d} | {n_groups} | {rec['slots']} | "
                         f"{fmt(rec['hash_ms'])} | {rec['mrows_per_s']} | "
                         f"{fmt(rec['first_ms'])} | {fmt(rec['verb_ms'])} |")

        if DOMAINS[0] not in args.domains:
            eng.free(h)
            eng.close()
            continue
        # the 4096-slot path at d = 4000: the default cap
        eng.set_max_groups(abi.GROUP_CAP_DEFAULT)
        agg = abi.make_agg([0], AGGS)
        want, n_groups = want_first_page(keys[0], val)
        runs = {"this build": (eng, h)}
        if args.direct_so:
            other = PlainEngine(os.path.abspath(args.direct_so))
            runs["--direct-so"] = (other, other.load(bs))
        ms = {k: [] for k in runs}
        for i in range(args.warmup + args.steps):
            for name, (e, hh) in runs.items():
                rc, res, wall = scan(e, hh, agg)
                assert rc == abi.OBX_BUF_NOT_ENOUGH and \
                    res.n_groups == n_groups == 4000
                if i == 0:
                    assert first_page(e, hh)[0] == want
                if i >= args.warmup:
                    ms[name].append(wall)
        assert eng.last_group_slots() == 0
        for name in runs:
            rec = dict(shape=shape, d=4000, path="4096-slot", build=name,
                       verb_ms=mmm(ms[name]),
                       runs=[round(x, 3) for x in ms[name]])
            print(json.dumps(rec), flush=True)
            direct.append(f"| {shape} | {name} | {fmt(rec['verb_ms'])} | "
                          + " ".join(f"{x:.2f}" for x in ms[name]) + " |")
        if args.direct_so:
            other.close()
        eng.free(h)
        eng.close()

    print("\n| shape | d | groups | slots | hash ms (min-max) | M rows/s | "
          "first scan ms | verb wall ms |")
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(sized))
    print("\n| shape | build | 4096-slot verb wall ms (min-max) | the runs |")
    print("|---|---|---|---|")
    print("\n".join(direct))


if __name__ == "__main__":
    main()
