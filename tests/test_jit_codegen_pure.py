"""CPU check that the generated source follows the knobs its cache key
covers (no GPU needed: codegen and strategy selection are host code)."""
from test_scan_flush_source import _dump, _lib, _lineitem_summaries, _q1


def _wpb_line(src):
    lines = [ln for ln in src.splitlines()
             if ln.startswith("#define OBX_JIT_WPB ")]
    assert len(lines) == 1
    return lines[0]


def test_v1_source_follows_wpb(monkeypatch):
    """The v1 kernel's OBX_JIT_WPB reaches its generator as an argument (and
    through it the cache key): two dumps of one plan under two settings
    differ in that line, and only there."""
    filt, agg = _q1()
    monkeypatch.setenv("OBX_JIT_V2", "0")
    srcs = {}
    for wpb in ("3", "5"):
        monkeypatch.setenv("OBX_JIT_WPB", wpb)
        srcs[wpb], grid = _dump(_lib(), filt, agg, _lineitem_summaries())
        assert "jtab_t" in srcs[wpb] and grid == 0      # the v1 kernel
        assert _wpb_line(srcs[wpb]) == "#define OBX_JIT_WPB " + wpb
    a, b = srcs["3"].splitlines(), srcs["5"].splitlines()
    assert len(a) == len(b)
    assert [x for x, y in zip(a, b) if x != y] == ["#define OBX_JIT_WPB 3"]
    monkeypatch.delenv("OBX_JIT_WPB")
    src, _ = _dump(_lib(), filt, agg, _lineitem_summaries())
    assert _wpb_line(src) == "#define OBX_JIT_WPB 7"    # the default
