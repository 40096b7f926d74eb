"""Join scan (obx_gpu_scan_join_agg) against its two floors.

Table (built from numpy through oracle.encode_block, 16 M rows by default,
1024-row blocks so every block is LDS-staged): three orderkey-like sparse
int64 key columns k0 / k1 / k2 drawn from domains of --keys distinct keys
each (multiples of 32, so a dense map spends 32 entries per key), a dict
char `ch`, an int64 value `val`, and two columns only the floor reads: `pay`
(the payload the row's key maps to) and `rank` in [0, 100). Every key encodes
its own rank and payload, key = 32 * (u * 500 + rank * 5 + pay) with pay in
[0, 5): 15 groups with the three chars, inside the 16-slot LDS group table.
So one table serves every hit share: the map for share s holds the domain's
keys of rank < s with their payloads, padded with absent keys (key + 16,
rank >= s) to the full domain size, so the map's size does not change with
the share.

Per map size, form (hash, dense) and hit share (1, 10, 50, 100 %) three scans
alternate inside one loop, all through the generic kernels (OBX_JIT=0):
  join    scan_join_agg, GROUP BY (ch, payload), COUNT(*), SUM(val)
  denorm  scan_filter_agg over the same table with the leaf rank < s (the
          one-leaf test on a materialised column that `hit = 1` is) and
          GROUP BY (ch, pay): what the join costs nothing over if the probe
          were free
  in_set  scan_filter_agg with an OBX_OP_IN_SET leaf on the key column, a key
          set of the same keys and form, GROUP BY ch: the semi-join half
The join's group rows must equal the denormalised scan's at every point.

Times are device milliseconds (obx_gpu_last_kernel_ms): median, min and max
of --steps runs after --warmup.

Run on a GPU box:  python tools/bench_keymap.py
Prints one JSON object per measured point and a markdown table at the end.
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

from oceanbase_amd import abi, oracle  # noqa: E402
from oceanbase_amd.engine import GpuEngine  # noqa: E402

INT8 = (abi.T_INT, 0, 19, 8)
INT4 = (abi.T_INT32, 0, 10, 4)
CHAR1 = (abi.T_CHAR, 0, 0, 1)
CH, VAL, PAY, RANK = 3, 4, 5, 6     # after the three key columns
BLOCK_ROWS = 1024
FORMS = {"hash": (abi.KM_HASH, abi.KS_HASH),
         "dense": (abi.KM_DENSE, abi.KS_BITMAP)}
SHARES = (1, 10, 50, 100)


def make_key(u, rank, pay):
    return 32 * (u * 500 + rank * 5 + pay)


def build_table(rows, domains, seed=7):
    """-> (blockset, bytes of the largest block)"""
    rng = np.random.default_rng(seed)
    rank = rng.integers(0, 100, rows)
    pay = rng.integers(0, 5, rows)
    cols = [make_key(rng.integers(0, d // 500, rows), rank, pay)
            .astype(np.int64) for d in domains]
    cols += [rng.choice(np.frombuffer(b"ANR", np.uint8), rows),
             rng.integers(0, 50_000, rows).astype(np.int64),
             pay.astype(np.int32), rank.astype(np.int64)]
    specs = [INT8] * 3 + [CHAR1, INT8, INT4, INT8]
    schema = oracle.make_schema(specs)
    encs = [abi.ENC_AUTO] * len(specs)
    blocks = []
    for r0 in range(0, rows, BLOCK_ROWS):
        raw = [np.ascontiguousarray(c[r0:r0 + BLOCK_ROWS]).view(np.uint8)
               .reshape(-1) for c in cols]
        blocks.append(oracle.encode_block(schema, raw, encs))
    # concatenate the blocks 16-byte aligned (encode_block appends 16 bytes
    # of read slack to each)
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
    return bs, max(len(blk) - 16 for blk in blocks)


def map_of(domain, share):
    """keys and payloads of the build side for one hit share, padded to the
    domain's size with keys no row holds"""
    u, r, p = np.meshgrid(np.arange(domain // 500), np.arange(100),
                          np.arange(5), indexing="ij")
    keys = make_key(u, r, p) + np.where(r < share, 0, 16)
    return (keys.reshape(-1).astype(np.int64),
            p.reshape(-1).astype(np.int32))


def tuples(res, rows, n_aggs):
    return res.rows_passed, abi.group_row_tuples(rows, n_aggs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16 * 1024 * 1024)
    ap.add_argument("--keys", type=int, nargs=3,
                    default=[32_000, 256_000, 2_048_000],
                    help="distinct keys of the three key columns "
                         "(multiples of 500)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    os.environ["OBX_JIT"] = "0"   # like for like: the generic kernels

    t0 = time.perf_counter()
    bs, max_block = build_table(args.rows, args.keys)
    gen_s = time.perf_counter() - t0
    assert max_block <= 17408, max_block
    eng = GpuEngine(0)
    h = eng.load(bs)
    total_bytes = eng.total_bytes(h)
    aggs = [dict(kind=abi.AGG_COUNT), dict(kind=abi.AGG_SUM, col_a=VAL)]
    table = []
    print(json.dumps(dict(rows=args.rows, bytes=total_bytes,
                          max_block_bytes=max_block,
                          gen_seconds=round(gen_s, 1))), flush=True)

    for kcol, domain in enumerate(args.keys):
        for share in SHARES:
            keys, pays = map_of(domain, share)
            f_denorm = abi.make_filter([dict(col=RANK, op=abi.OP_LT,
                                             lo=share)])
            for form, (km_kind, ks_kind) in FORMS.items():
                mid = eng.keymap_create(keys, pays, INT4, km_kind)
                sid = eng.keyset_create(keys, ks_kind)
                info = eng.keymap_info(mid)
                f_set = abi.make_filter([dict(col=kcol, op=abi.OP_IN_SET,
                                              set=sid)])
                scans = {
                    "join": lambda: tuples(*eng.scan_join_agg_paged(
                        h, None, mid, kcol,
                        abi.make_agg([CH, abi.COL_JOINED], aggs)), 2),
                    "denorm": lambda: tuples(*eng.scan_filter_agg_paged(
                        h, f_denorm, abi.make_agg([CH, PAY], aggs)), 2),
                    "in_set": lambda: tuples(*eng.scan_filter_agg_paged(
                        h, f_set, abi.make_agg([CH], aggs)), 2),
                }
                ms = {k: [] for k in scans}
                out = {}
                for i in range(args.warmup + args.steps):
                    for name, fn in scans.items():
                        out[name] = fn()
                        assert not eng.last_jit()
                        if i >= args.warmup:
                            ms[name].append(eng.last_kernel_ms())
                assert out["join"] == out["denorm"], (domain, share, form)
                assert out["in_set"][0] == out["join"][0]
                hit = out["join"][0] / args.rows
                rec = dict(keys=int(info.n_keys), form=form, share=share,
                           hit=round(hit, 4), map_bytes=int(info.bytes),
                           groups=len(out["join"][1]))
                for name in scans:
                    rec[name] = [round(statistics.median(ms[name]), 4),
                                 round(min(ms[name]), 4),
                                 round(max(ms[name]), 4)]
                j, d, s = (rec[n][0] for n in ("join", "denorm", "in_set"))
                rec["join_over_denorm"] = round(j / d, 3)
                rec["join_over_in_set"] = round(j / s, 3)
                print(json.dumps(rec), flush=True)
                table.append(
                    f"| {rec['keys']} | {form} | {rec['map_bytes'] >> 10} | "
                    f"{share} | {rec['hit']:.3f} | "
                    + " | ".join(f"{rec[n][0]:.3f} ({rec[n][1]:.3f}-"
                                 f"{rec[n][2]:.3f})" for n in scans)
                    + f" | {rec['join_over_denorm']} | "
                    f"{rec['join_over_in_set']} |")
                eng.keymap_free(mid)
                eng.keyset_free(sid)

    print("\n| map keys | form | map KiB | share % | joined | join ms "
          "(min-max) | denorm ms | in_set ms | join/denorm | join/in_set |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(table))
    eng.free(h)
    eng.close()


if __name__ == "__main__":
    main()
