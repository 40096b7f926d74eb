"""Key-set filter leaf (OBX_OP_IN_SET) throughput on one raw int64 column.

Workload: obx_gen_lineitem config 2 (one RAW fixed 8-byte column, values
1..50, 100 M rows by default). Sets are drawn from the column's own values:
the keys 1..k, so that `col BETWEEN 1 AND k` (an OBX_OP_BT leaf) keeps exactly
the same rows. That leaf reads the same bytes with no probe and is the floor.
The column has 50 equally likely values, so one key keeps 2 % of the rows:
the "1 %" point of the sweep is that single key.

For each survivor share and each form (hash, bitmap) the filter runs through
the staged filter JIT and with the JIT off (OBX_JIT=0, the generic kernels),
alternating the two inside one loop. --pad adds that many absent keys spread
over 2^40 to the hash sets, so that the table no longer fits a cache.

Times are device milliseconds of the filter kernel (obx_gpu_last_kernel_ms,
HIP events on the context's stream): median, min and max of --steps runs
after --warmup. Set build time is host wall time around obx_gpu_keyset_create
(which ends in a stream synchronise), first build excluded as warm-up.
"first call ms" is the host wall time of a plan's first filter call: it holds
the hipRTC build of the plan's kernel when that was not cached yet.

Run on a GPU box:  python tools/bench_keyset.py
Prints one JSON object per measured point and a markdown table at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from oceanbase_amd import abi, oracle  # noqa: E402
from oceanbase_amd.engine import GpuEngine  # noqa: E402

FORMS = {"hash": abi.KS_HASH, "bitmap": abi.KS_BITMAP}


def timed(eng, h, filt, jit):
    """one filter run -> (device ms, survivors, last_jit)"""
    if jit:
        os.environ.pop("OBX_JIT", None)
    else:
        os.environ["OBX_JIT"] = "0"
    n = eng.filter(h, filt)
    return (eng.last_kernel_ms(), n,
            int(eng._lib.obx_gpu_last_jit(eng._ctx)))


def measure(eng, h, filt, warmup, steps):
    """alternate JIT / generic; -> {path: (median, min, max, survivors, jit)}
    and "first_ms": host wall time of the first call through the JIT, which
    holds the hipRTC build when the plan's kernel was not cached yet"""
    out = {}
    ms = {True: [], False: []}
    seen = {}
    t0 = time.perf_counter()
    timed(eng, h, filt, True)
    out["first_ms"] = (time.perf_counter() - t0) * 1e3
    for i in range(warmup + steps):
        for jit in (True, False):
            t, n, ran = timed(eng, h, filt, jit)
            seen[jit] = (n, ran)
            if i >= warmup:
                ms[jit].append(t)
    for jit in (True, False):
        out["jit" if jit else "generic"] = (
            statistics.median(ms[jit]), min(ms[jit]), max(ms[jit]),
            seen[jit][0], seen[jit][1])
    os.environ.pop("OBX_JIT", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pad", type=int, default=1 << 20,
                    help="absent keys added to the padded hash sets")
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("--steps must be at least 5")

    t0 = time.perf_counter()
    li = oracle.Lineitem(2, args.rows, seed=42, block_bytes=16384)
    gen_s = time.perf_counter() - t0
    rng = np.random.default_rng(3)
    pad = (1 << 20) + rng.integers(0, 1 << 40, args.pad).astype(np.int64)

    eng = GpuEngine(0)
    h = eng.load(li.bs)
    total_bytes = eng.total_bytes(h)
    rows = eng.total_rows(h)
    results, table = [], []

    def report(name, share, form, pad_n, info, build_ms, m):
        for path in ("jit", "generic"):
            med, lo, hi, n, ran = m[path]
            rec = dict(leaf=name, keys=share, form=form, pad=pad_n, path=path,
                       last_jit=ran, ms_median=round(med, 4),
                       ms_min=round(lo, 4), ms_max=round(hi, 4),
                       survivors=n, share=round(n / rows, 4),
                       GBps=round(total_bytes / med / 1e6, 1),
                       set_bytes=info.bytes if info else 0,
                       set_build_ms=round(build_ms, 3),
                       first_call_ms=round(m["first_ms"], 1))
            results.append(rec)
            print(json.dumps(rec), flush=True)
            table.append(
                f"| {name} | {share} | {form} | {pad_n} | {path} | {ran} | "
                f"{med:.3f} | {lo:.3f} | {hi:.3f} | {rec['GBps']} | "
                f"{rec['share']:.3f} | {rec['set_bytes']} | "
                f"{rec['set_build_ms']} | {rec['first_call_ms']} |")

    eng.keyset_free(eng.keyset_create([1, 2, 3]))  # warm the build kernels
    for k in (1, 5, 25):  # 2 %, 10 %, 50 % of the rows
        bt = abi.make_filter([dict(col=0, op=abi.OP_BT, lo=1, hi=k)])
        m = measure(eng, h, bt, args.warmup, args.steps)
        want = m["jit"][3]
        assert m["generic"][3] == want
        report("BT", k, "-", 0, None, 0.0, m)
        members = np.arange(1, k + 1, dtype=np.int64)
        for form, kind in FORMS.items():
            for pad_n in ((0, args.pad) if form == "hash" else (0,)):
                keys = np.concatenate([members, pad[:pad_n]])
                t1 = time.perf_counter()
                sid = eng.keyset_create(keys, kind)
                build_ms = (time.perf_counter() - t1) * 1e3
                info = eng.keyset_info(sid)
                f = abi.make_filter([dict(col=0, op=abi.OP_IN_SET, set=sid)])
                m = measure(eng, h, f, args.warmup, args.steps)
                # the same rows as the BETWEEN leaf, on both paths
                assert m["jit"][3] == want and m["generic"][3] == want, \
                    (m, want)
                report("IN_SET", k, form, pad_n, info, build_ms, m)
                eng.keyset_free(sid)

    print(json.dumps(dict(rows=rows, bytes=total_bytes,
                          gen_seconds=round(gen_s, 2), steps=args.steps,
                          warmup=args.warmup)))
    print("\n| leaf | keys | form | pad keys | path | last_jit | median ms | "
          "min | max | GB/s | survivors | set bytes | build ms | "
          "first call ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(table))
    eng.free(h)
    eng.close()


if __name__ == "__main__":
    main()
