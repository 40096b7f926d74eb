#!/usr/bin/env python3
"""Writes the hipRTC source the JIT generators emit for a corpus of plans,
strategies and env knobs, one file per case, into the directory given on the
command line. No GPU needed: the generators are host code behind
obx_jit_dump_src_ex.

A generator refactor is checked by running this on the commit before it and
on the commit after it (each built in its own copy of the tree) and comparing
the two directories with `diff -r`: same text, same kernels.

A case the engine would not JIT-compile is written as the line NOJIT, so a
changed eligibility decision shows up as well.
"""
import ctypes as C
import os
import sys

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)
sys.path.insert(0, os.path.join(_REPO, "tests"))

from oceanbase_amd import abi  # noqa: E402
from test_scan_flush_source import _lib, _lineitem_summaries, _q1  # noqa: E402

KNOBS = ("OBX_JIT_R", "OBX_JIT_STRIPES", "OBX_JIT_M32", "OBX_JIT_CTAB",
         "OBX_JIT_JWS", "OBX_JIT_BDESC", "OBX_JIT_WPB", "OBX_JIT_V2",
         "OBX_JIT_FSTAGE", "OBX_JIT_FR", "OBX_JIT_FU", "OBX_JIT_FSL",
         "OBX_DUMP_RID", "OBX_JIT_SGRID", "OBX_JIT_JPACK")

# column facts of obx_jit_dump_src_ex: 1 dict in every block, 2 may be NULL,
# 4 bounds known, 8 aligned 8-byte RAW, 16 packed-range family, 32 dict stable
DICT, EXT, KNOWN, RAW8, RANGE, STABLE = 1, 2, 4, 8, 16, 32


def summaries(cols):
    """cols: list of dicts {f, lo, hi, cnt, w, len?, scale?}."""
    n = len(cols)
    sch = (abi.ColSchema * n)()
    for c, d in enumerate(cols):
        sch[c].obj_type = abi.T_INT
        sch[c].len = d.get("len", 0)
        sch[c].scale = d.get("scale", 0)
    return dict(
        n=n, cols=sch,
        flags=(C.c_uint8 * n)(*[d["f"] for d in cols]),
        cmin=(C.c_int64 * n)(*[d["lo"] for d in cols]),
        cmax=(C.c_int64 * n)(*[d["hi"] for d in cols]),
        maxcnt=(C.c_uint32 * n)(*[d["cnt"] for d in cols]),
        maxw=(C.c_uint32 * n)(*[d["w"] for d in cols]))


D = DICT | KNOWN | STABLE


def table(**over):
    """0 qty, 2 disc, 3 tax: dict values; 1 price: raw8; 4, 5: dict group
    keys; 6 date: packed range; 7: nullable packed range."""
    cols = [dict(f=D, lo=0, hi=50, cnt=50, w=6),
            dict(f=KNOWN | RAW8, lo=90000, hi=10500000, cnt=0, w=64),
            dict(f=D, lo=0, hi=10, cnt=11, w=4, scale=2),
            dict(f=D, lo=0, hi=8, cnt=9, w=4, scale=2),
            dict(f=D, lo=0, hi=2, cnt=3, w=2, len=8),
            dict(f=D, lo=0, hi=1, cnt=2, w=1, len=1),
            dict(f=KNOWN | RANGE, lo=8000, hi=11000, cnt=0, w=13),
            dict(f=KNOWN | RANGE | EXT, lo=-500, hi=70000, cnt=0, w=20)]
    for k, v in over.items():
        cols[int(k[1:])].update(v)
    return summaries(cols)


def dump(lib, filt, agg, s, n_blocks=1, n_cus=0, rows_pb=1365, force_v1=0):
    buf = C.create_string_buffer(1 << 21)
    grid = C.c_uint32(0)
    sz = lib.obx_jit_dump_src_ex(
        C.byref(filt) if filt is not None else None,
        C.byref(agg) if agg is not None else None, s["cols"], s["n"],
        s["flags"], s["cmin"], s["cmax"], s["maxcnt"], s["maxw"], rows_pb,
        force_v1, n_blocks, n_cus, C.byref(grid), buf, len(buf))
    if sz <= 0:
        return "NOJIT %d\n" % sz
    return "/* grid %u */\n" % grid.value + buf.raw[:sz].decode()


A = abi
CNT = dict(kind=A.AGG_COUNT)


def SUM(a):
    return dict(kind=A.AGG_SUM, col_a=a)


def P2(a, b):
    return dict(kind=A.AGG_SUM_PROD2, col_a=a, col_b=b)


def P3(a, b, c):
    return dict(kind=A.AGG_SUM_PROD3, col_a=a, col_b=b, col_c=c)


def MUL(a, b):
    return dict(kind=A.AGG_SUM_MUL, col_a=a, col_b=b)


RNG = [dict(col=6, op=A.OP_LE, lo=10561), dict(col=7, op=A.OP_GT, lo=5),
       dict(col=6, op=A.OP_NE, lo=9000), dict(col=7, op=A.OP_BT, lo=1, hi=9)]
MSK = [dict(col=2, op=A.OP_BT, lo=5, hi=7), dict(col=0, op=A.OP_LT, lo=24),
       dict(col=3, op=A.OP_IN, in_list=[1, 4]), dict(col=4, op=A.OP_NN)]


def scan_cases():
    q1f, q1a = _q1()
    li = _lineitem_summaries
    li2 = li()
    li2["cols"][2].scale = li2["cols"][3].scale = 2
    yield "q1", q1f, q1a, li(), {}, {}
    yield "q1_scale2", q1f, q1a, li2, {}, {}
    yield "q1_grid", q1f, q1a, li2, dict(n_blocks=453858, n_cus=256), {}
    for r in "1248":
        yield "q1_r" + r, q1f, q1a, li2, {}, dict(OBX_JIT_R=r)
    for k, v in (("STRIPES", "1"), ("STRIPES", "16"), ("M32", "0"),
                 ("CTAB", "0"), ("JWS", "0"), ("BDESC", "0"), ("WPB", "3"),
                 ("V2", "0")):
        yield "q1_%s%s" % (k.lower(), v), q1f, q1a, li2, {}, {"OBX_JIT_" + k: v}
    # joint-table forms: one axis with the packed row count (q1_grid), the
    # same without it, both axes with it (q1_nogroup: 12 x 10 cells) and
    # without; a workgroup with so many rows that the count cannot be packed
    yield "q1_grid_jpack0", q1f, q1a, li2, dict(n_blocks=453858, n_cus=256), \
        dict(OBX_JIT_JPACK="0")
    yield "q1_grid_sgrid64", q1f, q1a, li2, dict(n_blocks=453858, n_cus=256), \
        dict(OBX_JIT_SGRID="64")
    yield "q1_nogroup_jpack0", q1f, A.make_agg([], [
        CNT, SUM(0), SUM(1), P2(1, 2), P3(1, 2, 3), SUM(2)]), table(), {}, \
        dict(OBX_JIT_JPACK="0")
    yield "q1_v1_wpb5", q1f, q1a, li(), {}, dict(OBX_JIT_V2="0",
                                                 OBX_JIT_WPB="5")
    yield "q1_force_v1", q1f, q1a, li(), dict(force_v1=1), {}
    yield "q1_force_v1_wpb3", q1f, q1a, li(), dict(force_v1=1), dict(
        OBX_JIT_WPB="3")
    s = li()
    s["maxcnt"][1] = 0x10000
    yield "q1_bdesc_unfit", q1f, q1a, s, {}, {}
    # a negative price bound: no combined factor table
    yield "q1_neg_price", q1f, q1a, table(c1=dict(lo=-5)), {}, {}
    # a two-axis joint histogram: no group cells, 12 x 10 factor cells
    yield "q1_nogroup", q1f, A.make_agg([], [
        CNT, SUM(0), SUM(1), P2(1, 2), P3(1, 2, 3), SUM(2)]), table(), {}, {}
    yield "q1_nogroup_jws0", q1f, A.make_agg([], [
        CNT, SUM(1), P2(1, 2), P3(1, 2, 3)]), table(), {}, dict(OBX_JIT_JWS="0")
    # bounds that lose the persistent kernel
    wide = li(price_max=1 << 39)
    a2 = A.make_agg([4, 5], [CNT, SUM(1)])
    f2 = A.make_filter([dict(col=6, op=A.OP_LE, lo=10500)])
    yield "bound_v2", f2, a2, wide, dict(n_blocks=10**6, n_cus=256), {}
    yield "bound_v1", f2, a2, wide, dict(n_blocks=10**6, n_cus=1), {}
    # Q6: no group columns, SUM_MUL, date range merged into one BT leaf
    q6f = A.make_filter([dict(col=6, op=A.OP_GE, lo=8766),
                         dict(col=6, op=A.OP_LT, lo=9131),
                         dict(col=2, op=A.OP_BT, lo=5, hi=7),
                         dict(col=0, op=A.OP_LT, lo=24)])
    q6a = A.make_agg([], [MUL(1, 2)])
    yield "q6", q6f, q6a, table(), {}, {}
    yield "q6_grid", q6f, q6a, table(), dict(n_blocks=453858, n_cus=256), {}
    for k, v in (("R", "1"), ("R", "8"), ("M32", "0"), ("BDESC", "0"),
                 ("V2", "0"), ("WPB", "2")):
        yield "q6_%s%s" % (k.lower(), v), q6f, q6a, table(), {}, {
            "OBX_JIT_" + k: v}
    yield "q6_force_v1", q6f, q6a, table(), dict(force_v1=1), {}
    # group columns: none, one, two; key lengths 8, 1 and 0
    for name, g in (("g0", []), ("g1_len8", [4]), ("g1_len1", [5]),
                    ("g2", [4, 5]), ("g2_swapped", [5, 4])):
        agg = A.make_agg(g, [CNT, SUM(1), SUM(0)])
        yield "grp_" + name, f2, agg, table(), {}, {}
        yield "grp_" + name + "_v1", f2, agg, table(), dict(force_v1=1), {}
        yield "grp_" + name + "_r1", f2, agg, table(), {}, dict(OBX_JIT_R="1")
    # 0 to 4 leaves of each kind, and mixed
    agg = A.make_agg([4], [CNT, SUM(1)])
    for nl in range(5):
        for kind, pool in (("range", RNG), ("mask", MSK)):
            filt = A.make_filter(pool[:nl])
            for env in ({}, dict(OBX_JIT_R="1"), dict(OBX_JIT_M32="0"),
                        dict(OBX_JIT_BDESC="0"), dict(OBX_JIT_V2="0")):
                tag = "".join("_%s%s" % (k[8:].lower(), v)
                              for k, v in env.items())
                yield "leaf%d_%s%s" % (nl, kind, tag), filt, agg, table(), {}, env
    yield ("leaf_mixed", A.make_filter([RNG[0], MSK[0], RNG[1], MSK[1]]), agg,
           table(), {}, {})
    yield ("leaf_wide", A.make_filter([dict(col=1, op=A.OP_GT, lo=100000)]),
           agg, table(c1=dict(f=KNOWN | RAW8 | RANGE)), {}, {})
    yield ("leaf_wide_r8", A.make_filter([RNG[0], RNG[1]]), agg, table(), {},
           dict(OBX_JIT_R="8"))
    # aggregate strategies
    shapes = dict(
        minmax_ctx=[CNT, dict(kind=A.AGG_MIN, col_a=1),
                    dict(kind=A.AGG_MAX, col_a=7)],
        minmax_dict=[CNT, dict(kind=A.AGG_MIN, col_a=0),
                     dict(kind=A.AGG_MAX, col_a=2)],
        minmax_both=[dict(kind=A.AGG_MAX, col_a=1), SUM(0),
                     dict(kind=A.AGG_MIN, col_a=0)],
        count_cols=[dict(kind=A.AGG_COUNT, col_a=7),
                    dict(kind=A.AGG_COUNT, col_a=1),
                    dict(kind=A.AGG_COUNT, col_a=0)],
        count_only=[CNT],
        sum_ctx_not_raw8=[CNT, SUM(6), SUM(1), SUM(7)],
        prod2=[P2(1, 2)], prod3=[P3(1, 2, 3)], prod23=[P2(1, 2), P3(1, 2, 3)],
        prod23_sum=[SUM(1), P2(1, 2), P3(1, 2, 3)],
        prod2_ctx=[P2(1, 7)], prod3_ctx=[P3(1, 7, 6)],
        prod3_ctx_b=[P3(1, 7, 3)], prod3_ctx_c=[P3(1, 2, 6)],
        prod23_ctx=[P2(1, 2), P3(1, 2, 6)],
        prod23_ctx_b=[P2(1, 7), P3(1, 7, 3)],
        prod_ref_a=[P2(0, 2), P3(0, 2, 3), MUL(0, 3)],
        mul_ctx=[MUL(1, 7), MUL(7, 6)], mul_ref=[MUL(1, 2), MUL(0, 1)],
        hist_many=[SUM(0), SUM(2), SUM(3), dict(kind=A.AGG_COUNT, col_a=2)],
        jws_axis1_only=[SUM(1), P2(1, 2), MUL(1, 3)],
        eight=[CNT, SUM(0), SUM(1), P2(1, 2), P3(1, 2, 3), SUM(2), SUM(3),
               dict(kind=A.AGG_COUNT, col_a=1)])
    for name, aggs in shapes.items():
        for gname, g in (("g2", [4, 5]), ("g0", [])):
            agg = A.make_agg(g, aggs)
            base = "agg_%s_%s" % (name, gname)
            yield base, f2, agg, table(), {}, {}
            yield base + "_nofilter", None, agg, table(), {}, {}
            yield base + "_v1", f2, agg, table(), dict(force_v1=1), {}
            for k, v in (("JWS", "0"), ("CTAB", "0"), ("R", "1"), ("R", "2"),
                         ("BDESC", "0"), ("STRIPES", "2")):
                yield (base + "_%s%s" % (k.lower(), v), f2, agg, table(), {},
                       {"OBX_JIT_" + k: v})
    # scale 0 factors: (1 - d) may be negative, no combined table
    yield ("agg_prod3_scale0", f2, A.make_agg([4], [P3(1, 2, 3)]),
           table(c2=dict(scale=0), c3=dict(scale=0)), {}, {})
    # tiny blocks: the stage buffer is sized by the flush partials
    yield ("tiny_blocks", f2, A.make_agg([4, 5], shapes["eight"]), table(),
           dict(rows_pb=8), {})


def filter_cases():
    def t(*w):
        return summaries([dict(f=KNOWN | RANGE, lo=0, hi=30000, cnt=0, w=x)
                          for x in w])
    dmix = summaries([dict(f=KNOWN | RANGE, lo=0, hi=30000, cnt=0, w=13),
                      dict(f=D, lo=0, hi=10, cnt=11, w=4),
                      dict(f=KNOWN | RANGE | EXT, lo=0, hi=99, cnt=0, w=8),
                      dict(f=D, lo=0, hi=50, cnt=50, w=6)])
    L = [dict(col=0, op=A.OP_LE, lo=10561), dict(col=1, op=A.OP_GT, lo=5),
         dict(col=2, op=A.OP_EQ, lo=3), dict(col=3, op=A.OP_BT, lo=2, hi=30)]
    M = [dict(col=1, op=A.OP_IN, in_list=[1, 4]), dict(col=3, op=A.OP_NE, lo=7),
         dict(col=1, op=A.OP_NU), dict(col=3, op=A.OP_LT, lo=9)]
    envs = [{}, dict(OBX_JIT_FSTAGE="0"), dict(OBX_DUMP_RID="1")]
    envs += [dict(OBX_JIT_FR=r) for r in "124"]
    envs += [dict(OBX_JIT_FR=r, OBX_JIT_FSTAGE="0") for r in "124"]
    envs += [dict(OBX_JIT_FU=u, OBX_JIT_FSTAGE="0") for u in "128"]
    envs += [dict(OBX_JIT_FSL="3", OBX_JIT_FSTAGE="0"), dict(OBX_JIT_FSL="3"),
             dict(OBX_JIT_V2="0")]

    def tag(env):
        return "".join("_%s%s" % (k.split("_")[-1].lower(), v)
                       for k, v in env.items())
    for nl in range(1, 5):
        for env in envs:
            yield ("f_range%d%s" % (nl, tag(env)), A.make_filter(L[:nl]),
                   t(13, 8, 6, 20), dict(rows_pb=4000), env)
            yield ("f_mask%d%s" % (nl, tag(env)), A.make_filter(M[:nl]), dmix,
                   dict(rows_pb=4000), env)
    mixed = [L[0], M[0], L[2], M[1]]
    progs = dict(
        and_or=(L[:3], [0, 1, A.TOK_AND, 2, A.TOK_OR], t(13, 8, 6, 20)),
        or_and=(mixed, [0, 1, A.TOK_OR, 2, 3, A.TOK_OR, A.TOK_AND], dmix),
        or2=([M[0], L[0]], [0, 1, A.TOK_OR], dmix))
    for env in envs:
        yield ("f_mixed" + tag(env), A.make_filter(mixed), dmix,
               dict(rows_pb=4000), env)
        for name, (lv, prog, tab) in progs.items():
            yield ("f_prog_%s%s" % (name, tag(env)),
                   A.make_filter(lv, prog=prog), tab, dict(rows_pb=4000), env)
    # a 64-bit-wide leaf column, alone and next to a narrow one
    for env in envs:
        yield ("f_wide" + tag(env), A.make_filter(L[:1]), t(64, 64, 64, 64),
               dict(rows_pb=2048), env)
        yield ("f_wide_narrow" + tag(env), A.make_filter(L[:2]), t(40, 13),
               dict(rows_pb=1024), env)
        yield ("f_wide_prog" + tag(env),
               A.make_filter(L[:2], prog=[0, 1, A.TOK_OR]), t(40, 13),
               dict(rows_pb=1024), env)
    # a dict leaf too wide for a packed read of FR fields, next to one that
    # fits
    dwide = summaries([dict(f=D, lo=0, hi=10, cnt=11, w=20),
                       dict(f=D, lo=0, hi=50, cnt=50, w=6)])
    two = [dict(col=0, op=A.OP_IN, in_list=[1, 4]), dict(col=1, op=A.OP_NE, lo=7)]
    for env in (dict(OBX_JIT_FR="4"), dict(OBX_JIT_FR="4", OBX_JIT_FSTAGE="0"),
                dict(OBX_JIT_FR="2")):
        yield ("f_mask_wide" + tag(env), A.make_filter(two), dwide,
               dict(rows_pb=2000), env)
        yield ("f_mask_wide_prog" + tag(env),
               A.make_filter(two, prog=[0, 1, A.TOK_OR]), dwide,
               dict(rows_pb=2000), env)
    yield ("f_many_blocks", A.make_filter(L[:2]), t(13, 8),
           dict(rows_pb=4000, n_blocks=100000), {})
    yield ("f_too_big_for_lds", A.make_filter(L[:2]), t(64, 64),
           dict(rows_pb=4096), {})


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: jit_src_corpus.py OUT_DIR")
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    lib = _lib()
    cases = [(n, f, a, s, kw, env) for n, f, a, s, kw, env in scan_cases()]
    cases += [(n, f, None, s, kw, env) for n, f, s, kw, env in filter_cases()]
    seen = set()
    for name, filt, agg, s, kw, env in cases:
        assert name not in seen, name
        seen.add(name)
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        with open(os.path.join(out, name + ".hip"), "w") as f:
            f.write(dump(lib, filt, agg, s, **kw))
    for k in KNOBS:
        os.environ.pop(k, None)
    print("%d cases -> %s" % (len(cases), out))


if __name__ == "__main__":
    main()
