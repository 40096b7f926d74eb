"""Unit tests for bench.py's cross-rank result merge (the distributed
2-phase group-by merge: sum-family adds, MIN/MAX folds)."""
import ctypes as C
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pytest

from oceanbase_amd import abi
import bench


def _blob(key, cnt, cells):
    r = abi.AggResult()
    r.n_groups = 1
    r.rows_scanned = cnt
    r.rows_passed = cnt
    g = r.groups[0]
    g.key[0] = key
    g.key_len = 1
    g.row_count = cnt
    for i, v in enumerate(cells):
        g.cells[i].limb[0] = v & ((1 << 64) - 1)
        s = ~0 if v < 0 else 0
        for l in (1, 2, 3):
            g.cells[i].limb[l] = s & ((1 << 64) - 1)
    return bytes(r)


def test_merge_sums_and_minmax():
    kinds = [abi.AGG_SUM, abi.AGG_MIN, abi.AGG_MAX]
    b1 = _blob(65, 10, [100, -5, 7])
    b2 = _blob(65, 3, [-40, -9, 2])
    groups, scanned, passed = bench.merge_results([b1, b2], 3, kinds)
    assert scanned == 13 and passed == 13
    (key, (cnt, s, mn, mx)), = [(k, tuple(v)) for k, v in groups.items()]
    assert key == b"A" and cnt == 13
    assert s == 60 and mn == -9 and mx == 7


def test_merge_rejects_unmergeable_kind():
    blob = _blob(66, 1, [1])
    with pytest.raises(AssertionError):
        bench.merge_results([blob], 1, [99])


def _limbs_to_int(limbs):
    u = sum(int(v) << (32 * j) for j, v in enumerate(limbs))
    return u - (1 << 256) if u >> 255 else u


def test_dump_outputs_agg_table_is_exact(tmp_path):
    """--dump-outputs writes the result table as float64 arrays; the
    32-bit limbs carry wide cells exactly, for a single result and for the
    merged multi-rank table alike."""
    import numpy as np
    big = (1 << 62) + 12345  # past float64's 53-bit mantissa
    blob = _blob(65, 10, [big, -5])
    res = abi.AggResult.from_buffer_copy(blob)
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "merged")
    bench.dump_outputs(d1, res, 2, seed=42)
    bench.dump_outputs(d2, bench.merge_results([blob], 2), 2, seed=42)
    for d in (d1, d2):
        arrs = {n: np.load(os.path.join(d, n + ".npy"))
                for n in ("rows_scanned_passed", "group_keys",
                          "group_row_counts", "agg_values", "agg_limbs32")}
        assert all(a.dtype == np.float64 for a in arrs.values())
        assert arrs["rows_scanned_passed"].tolist() == [10.0, 10.0]
        assert arrs["group_keys"].tolist() == [[65.0]]
        assert arrs["group_row_counts"].tolist() == [10.0]
        assert arrs["agg_values"][0].tolist() == [float(big), -5.0]
        assert _limbs_to_int(arrs["agg_limbs32"][0, 0]) == big
        assert _limbs_to_int(arrs["agg_limbs32"][0, 1]) == -5


def test_dump_outputs_bitmap_is_capped_and_seeded(tmp_path, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 16)
    bm = np.arange(203, dtype=np.uint8)
    outs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        bench.dump_outputs(d, 77, 0, seed=42, bitmap=bm)
        assert np.load(os.path.join(d, "survivors.npy")).tolist() == [77.0]
        outs.append(np.load(os.path.join(d, "bitmap_words32.npy")))
    assert outs[0].dtype == np.float64 and outs[0].size == 16
    assert np.array_equal(outs[0], outs[1])
    words = np.concatenate([bm, np.zeros(1, np.uint8)]).view("<u4")
    assert set(outs[0].tolist()) <= set(words.astype(np.float64).tolist())
