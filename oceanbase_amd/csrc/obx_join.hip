/*
 * obx_join.hip — the join scan kernels of obx_gpu_scan_join_agg: the fused
 * scan -> filter -> aggregate of obx_kernels.hip with one more step between
 * the filter and the aggregates, the probe of a key map (obx_keymap.h). The
 * probe side of the reference's ObHashJoinVecOp (sql/engine/join/hash_join)
 * followed by its hash group-by, in one pass over the encoded blocks.
 *
 * This file holds the join step, two assemblies of the steps of obx_steps.h
 * and the entry points:
 *   join_scan_body = lds_table_init + per window (open + filter_window +
 *                    JOIN STEP + agg_passes) + lds_table_flush
 *   k_scan_join_agg_direct = scan_direct_body(direct_join), the growth path
 * The join step, per row the filter passed: decode the probe column
 * (opnd_value, so every encoding works), probe the map, clear the pass bit on
 * a miss; on a hit resolve the group (group_row with the payload spliced
 * into the key, obx_join_key), and accumulate the payload aggregates while
 * the payload is in a register. No per-row payload is stored: the
 * per-aggregate passes that follow read only real columns, through the
 * rewritten pass bitmap and row_slot. Unlike the plain scan, which counts
 * the passed rows after the filter and groups in a loop of its own, the join
 * step does both inside the probe loop. direct_join is the same step for the
 * growth path, one row at a time into global cells.
 *
 * The plan (dev_plan_hdr) does not know the payload: the host removed it
 * from the group columns and put COUNT(*) where a payload aggregate stands.
 * dev_join says where the payload goes in the key and which cells are the
 * join step's (own_mask), and holds every cell's true kind.
 *
 * A translation unit of its own, so the kernels of obx_kernels.hip keep
 * their code and register allocation.
 */
#include "obx_steps.h"
#include "obx_keymap.h"

template <bool STAGE, bool PROG>
__device__ __forceinline__ void join_scan_body(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr &ph,
    const dev_join &dj, gslot *__restrict__ gtable,
    unsigned long long *__restrict__ counters, uint8_t *lds_blk) {
  __shared__ lds_table tab;
  __shared__ uint64_t pass_bm[OBX_MAX_BLOCK_ROWS / 64];
  /* leaf_bm (phase 1, combine programs only) and row_slot (from the join
     step on) are live in disjoint phases, as in scan_filter_agg_body */
  __shared__ union {
    uint64_t leaf_bm[8][OBX_MAX_BLOCK_ROWS / 64];
    uint8_t row_slot[OBX_MAX_BLOCK_ROWS];
  } u;
  __shared__ uint8_t cell_slot[64];
  __shared__ unsigned long long wg_passed;

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63;
  const uint32_t wv = tid >> 6;
  const uint32_t stripe = lane & (OBX_STRIPES - 1);
  const auto kind_of = [&](uint32_t a) { return dj.kind[a]; };

  lds_table_init(&tab, ph.n_aggs, kind_of);
  if (tid == 0) wg_passed = 0;
  __syncthreads();

  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const dev_block &cur = blocks[b];
    const blk_leaf *bl = bleaves + (uint64_t)b * ph.n_leaves;
    const uint8_t blk_verdict = fold_prog3(ph, cur, plan_leaves, bl);
    if (blk_verdict == 0) continue;
    const blk_view bv = blk_open<STAGE>(buf, cur, lds_blk);
    const uint64_t blk_bit = cur.block_byte * 8;

    const uint32_t all_rows = cur.row_count;
    for (uint32_t w0 = 0; w0 < all_rows; w0 += OBX_MAX_BLOCK_ROWS) {
    const uint32_t rows = (all_rows - w0 < OBX_MAX_BLOCK_ROWS)
                              ? all_rows - w0 : OBX_MAX_BLOCK_ROWS;
    const uint32_t iters = (rows + WG - 1) / WG;

    /* ---- phase 1: filter into the LDS pass bitmap ---- */
    filter_window<PROG>(bv, cur, plan_leaves, bl, ph, blk_verdict, blk_bit,
                        rows, w0, pass_bm, &u.leaf_bm[0][0]);
    __syncthreads(); /* leaf_bm fully read before row_slot is written */

    /* ---- the join step: probe, regroup, payload aggregates. A wave reads
       and rewrites only its own pass-bitmap words. ---- */
    {
      group_ctx g = group_open(ph, cur, blk_bit);
      /* the ref -> slot cache maps a cell of real group columns to one
         slot: not so once the payload is part of the key */
      if (dj.pay_group) g.ref_fast = false;
      if (g.ref_fast) {
        for (uint32_t i = tid; i < 64; i += WG) cell_slot[i] = 254;
        __syncthreads();
      }
      const agg_opnd okey = opnd_open(ph, cur, dj.probe_idx, blk_bit);
      for (uint32_t it = 0; it < iters; it++) {
        const uint32_t rr = it * WG + tid;
        const uint64_t m = pass_bm[it * WAVES + wv];
        if (!m) { if (rr < rows) u.row_slot[rr] = 255; continue; }
        uint8_t slot8 = 255;
        bool hit = false;
        if ((m >> lane) & 1) {
          bool isn = false;
          const int64_t kv = opnd_value(bv, cur, okey, w0 + rr, isn);
          uint64_t pv = 0;
          hit = !isn && obx_keymap_probe(dj.km, kv, &pv);
          if (hit && ph.n_aggs) {
            slot8 = group_row(
                bv, ph, g, cell_slot, w0 + rr, counters,
                [&](uint64_t rk) {
                  return lds_slot(&tab, obx_join_key(dj, rk, pv));
                },
                [&](uint8_t s) { atomicAdd(&tab.count[s][stripe], 1ull); });
            if (slot8 != 255 && dj.own_mask)
              for (uint32_t a = 0; a < ph.n_aggs; a++)
                if ((dj.own_mask >> a) & 1)
                  agg_term(dj.kind[a], false, 0, 0, (int64_t)pv, false, 0,
                           false, 0, false,
                           lds_sink{tab.cell[slot8][a][stripe], nullptr});
          }
        }
        const uint64_t joined = __ballot(hit);
        if (lane == 0) {
          pass_bm[it * WAVES + wv] = joined;
          if (joined)
            atomicAdd(&wg_passed, (unsigned long long)__popcll(joined));
        }
        if (rr < rows) u.row_slot[rr] = slot8;
      }
    }
    __syncthreads();

    /* ---- one pass per real-column aggregate (payload aggregates and
       COUNT(*) need none) ---- */
    agg_passes(bv, cur, ph, blk_bit, rows, w0, pass_bm, u.row_slot, &tab);
    __syncthreads(); /* pass_bm reuse across windows */
    } /* window loop */
  }
  __syncthreads();

  lds_table_flush(&tab, &wg_passed, ph, kind_of, gtable, counters);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_join_agg(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    const dev_join dj, gslot *__restrict__ gtable,
    unsigned long long *__restrict__ counters) {
  join_scan_body<false, false>(buf, blocks, n_blocks, plan_leaves, bleaves,
                               ph, dj, gtable, counters, nullptr);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_join_agg_prog(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    const dev_join dj, gslot *__restrict__ gtable,
    unsigned long long *__restrict__ counters) {
  join_scan_body<false, true>(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                              dj, gtable, counters, nullptr);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_join_agg_lds(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    const dev_join dj, gslot *__restrict__ gtable,
    unsigned long long *__restrict__ counters) {
  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];
  join_scan_body<true, false>(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                              dj, gtable, counters, lds_blk);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_join_agg_prog_lds(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    const dev_join dj, gslot *__restrict__ gtable,
    unsigned long long *__restrict__ counters) {
  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];
  join_scan_body<true, true>(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                             dj, gtable, counters, lds_blk);
}

/* ---------------- the growth path ----------------------------------------
 * k_scan_agg_direct with the probe: when a workgroup's LDS table overflowed
 * (counters[1]), the host reruns the scan here. direct_join is what the join
 * puts between scan_direct_body's filter and its table: a row takes part
 * when its probe key (col_value2, every encoding) is a map key, the payload
 * is spliced into the group key, and the cells of own_mask accumulate the
 * payload (through the sink the body hands in). */
struct direct_join {
  const dev_join &dj;
  __device__ __forceinline__ bool admit(const blk_view &bv,
                                        const dev_block &cur,
                                        const dev_plan_hdr &ph, uint32_t r,
                                        uint64_t &pv) const {
    bool isn = false;
    const int64_t kv = col_value2(
        bv, cur, cur.cols[ph.need_cols[dj.probe_idx]], r, isn);
    return !isn && obx_keymap_probe(dj.km, kv, &pv);
  }
  __device__ __forceinline__ uint64_t key(uint64_t rk, uint64_t pv) const {
    return obx_join_key(dj, rk, pv);
  }
  template <class SINK>
  __device__ __forceinline__ bool own(uint32_t a, uint64_t pv,
                                      const SINK sink) const {
    if (!((dj.own_mask >> a) & 1)) return false;
    agg_term(dj.kind[a], false, 0, 0, (int64_t)pv, false, 0, false, 0, false,
             sink);
    return true;
  }
};

extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_join_agg_direct(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    const dev_join dj, gslot *__restrict__ gtable,
    unsigned long long *__restrict__ counters) {
  scan_direct_body(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                   gslot_table{gtable}, counters, direct_join{dj});
}

/* the same on the sized table (k_scan_agg_hash, obx_kernels.hip) */
extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_join_agg_hash(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    const dev_join dj, const obx_gh_dev table, uint64_t max_groups,
    unsigned long long *__restrict__ counters) {
  scan_direct_body(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                   sized_table{table, max_groups}, counters, direct_join{dj});
}
