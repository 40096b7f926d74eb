"""Lifetime of the JIT compile cache across contexts.

The cache of compiled kernels belongs to the process, not to a context: a
second context on the same device hits the entry the first one compiled, and
the entry stays good after the context that compiled it is closed. Two
contexts on device 0 scan the same Q1-shaped table (3 blocks, so the
persistent kernel runs): A, B, close A, B again. Every result equals the CPU
oracle's and every scan reports the persistent (v2) generated kernel.

Single-threaded on purpose: the lock and the device ordinal in the cache key
are for review, not for a test that would have to race to see them.
"""
import pytest

from oceanbase_amd import abi, oracle

pytestmark = pytest.mark.gpu


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


def test_entry_outlives_the_context_that_compiled_it():
    from oceanbase_amd.engine import GpuEngine

    li = oracle.Lineitem(4, 3500, seed=5)
    assert li.n_blocks == 3
    filt, agg = _q1_descs()
    res_cpu = oracle.scan_filter_agg(li.bs, filt, agg)
    want = abi.result_rows(res_cpu, 6)

    def scan(eng, h):
        res = eng.scan_filter_agg(h, filt, agg)
        assert eng._lib.obx_gpu_last_jit(eng._ctx) == 2
        assert res.rows_passed == res_cpu.rows_passed
        assert abi.result_rows(res, 6) == want

    a, b = GpuEngine(0), GpuEngine(0)
    try:
        ha, hb = a.load(li.bs), b.load(li.bs)
        scan(a, ha)  # compiles
        scan(b, hb)  # hits A's entry
        a.close()
        scan(b, hb)  # the entry outlived A
    finally:
        a.close()  # a second close is a no-op
        b.close()
