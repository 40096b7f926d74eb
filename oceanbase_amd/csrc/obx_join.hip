/*
 * obx_join.hip — the join scan kernels of obx_gpu_scan_join_agg: the fused
 * scan -> filter -> aggregate of obx_kernels.hip with one more step between
 * the filter and the aggregates, the probe of a key map (obx_keymap.h). The
 * probe side of the reference's ObHashJoinVecOp (sql/engine/join/hash_join)
 * followed by its hash group-by, in one pass over the encoded blocks.
 *
 * Assembled from the steps of obx_steps.h:
 *   join_scan_body = open + filter_window + JOIN STEP + agg_row(lds_sink) +
 *                    flush_cells
 *   k_scan_join_agg_direct = open + leaf_match + probe + gtable_slot +
 *                    agg_term(gcell_sink), the growth path
 * The join step, per row the filter passed: decode the probe column
 * (opnd_value, so every encoding works), probe the map, clear the pass bit on
 * a miss; on a hit resolve the group (group_row with the payload spliced
 * into the key, obx_join_key), and accumulate the payload aggregates while
 * the payload is in a register. No per-row payload is stored: the
 * per-aggregate passes that follow read only real columns, through the
 * rewritten pass bitmap and row_slot.
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

  for (uint32_t s = tid; s < OBX_LTABLE_SLOTS; s += WG) {
    tab.key[s] = OBX_KEY_EMPTY;
    for (uint32_t st = 0; st < OBX_STRIPES; st++) {
      tab.count[s][st] = 0;
      for (uint32_t a = 0; a < ph.n_aggs; a++) {
        const uint8_t k = dj.kind[a];
        tab.cell[s][a][st][0] = (k == 2) ? (unsigned long long)INT64_MAX
                                : (k == 3) ? (unsigned long long)INT64_MIN
                                           : 0ull;
        tab.cell[s][a][st][1] = 0;
      }
    }
  }
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

    /* ---- one pass per real-column aggregate, as scan_filter_agg_body's
       phase 3 (payload aggregates and COUNT(*) need none) ---- */
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      const dev_agg ag = ph.aggs[a];
      if (ag.kind == 0 && ag.ia == 0xFF) continue;
      const bool fuse_p3 = obx_fuse_p3(ph.aggs, ph.n_aggs, a);
      const dev_agg ag2 = fuse_p3 ? ph.aggs[a + 1] : ag;
      const agg_opnd oa = opnd_open(ph, cur, ag.ia, blk_bit);
      const agg_opnd ob = opnd_open(ph, cur, ag.ib, blk_bit);
      const agg_opnd oc = opnd_open(ph, cur, ag2.ic, blk_bit);
      auto rows_of = [&](auto kind, auto fuse) {
        for (uint32_t it = 0; it < iters; it++) {
          uint32_t rr = it * WG + tid;
          uint64_t m = pass_bm[it * WAVES + wv];
          if (!m) continue;
          bool pass = (m >> lane) & 1;
          uint8_t slot8 = pass && rr < rows ? u.row_slot[rr] : 255;
          if (slot8 == 255) continue;
          agg_row(bv, cur, kind.v, fuse.v != 0, ag, ag2, oa, ob, oc, w0 + rr,
                  lds_sink{tab.cell[slot8][a][stripe],
                           fuse.v ? tab.cell[slot8][a + 1][stripe] : nullptr});
        }
      };
      switch (ag.kind) {
        case 0: rows_of(kc<0>{}, kc<0>{}); break; /* COUNT(col) */
        case 1: rows_of(kc<1>{}, kc<0>{}); break; /* SUM */
        case 2: rows_of(kc<2>{}, kc<0>{}); break; /* MIN */
        case 3: rows_of(kc<3>{}, kc<0>{}); break; /* MAX */
        case 4: /* SUM_PROD2, optionally with its PROD3 mate */
          if (fuse_p3) rows_of(kc<4>{}, kc<1>{});
          else rows_of(kc<4>{}, kc<0>{});
          break;
        case 5: rows_of(kc<5>{}, kc<0>{}); break; /* SUM_PROD3 alone */
        case 6: rows_of(kc<6>{}, kc<0>{}); break; /* SUM_MUL */
        default: break;
      }
      if (fuse_p3) a++; /* consumed the PROD3 mate */
    }
    __syncthreads(); /* pass_bm reuse across windows */
    } /* window loop */
  }
  __syncthreads();

  /* flush LDS table to the global table (merge lane stripes) */
  if (tid == 0 && wg_passed) atomicAdd(&counters[0], wg_passed);
  for (uint32_t s = tid; s < OBX_LTABLE_SLOTS; s += WG) {
    uint64_t key = tab.key[s];
    if (key == OBX_KEY_EMPTY) continue;
    unsigned long long cnt = 0;
    for (uint32_t st = 0; st < OBX_STRIPES; st++) cnt += tab.count[s][st];
    /* a full global table: the growth path, as in scan_filter_agg_body */
    const int gi = gtable_slot<OBX_GTABLE_SHIFT>(gtable, key);
    if (gi < 0) {
      atomicAdd(&counters[1], cnt);
      continue;
    }
    const uint32_t idx = (uint32_t)gi;
    atomicAdd(&gtable[idx].count, cnt);
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      const bool own = (dj.own_mask >> a) & 1;
      const uint8_t kind = dj.kind[a];
      if (!own && kind == 0 && ph.aggs[a].ia == 0xFF) /* COUNT(*) */
        g_acc_i128(gtable[idx].cells[a], cnt, 0);
      else
        flush_cells<OBX_STRIPES>(tab.cell[s][a], kind, gtable[idx].cells[a]);
    }
  }
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
 * (counters[1]), the host reruns the scan here. Every joined row resolves
 * its key in the OBX_GTABLE_BIG table and accumulates with global atomics.
 * AND-combined leaves only. A full table is surfaced as counters[2]. */
extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_join_agg_direct(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    const dev_join dj, gslot *__restrict__ gtable,
    unsigned long long *__restrict__ counters) {
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63, wv = tid >> 6;
  unsigned long long lane_cnt = 0;
  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const dev_block &cur = blocks[b];
    const blk_leaf *bl = bleaves + (size_t)b * ph.n_leaves;
    bool skip = false;
    for (uint32_t i = 0; i < ph.n_leaves; i++)
      if (leaf_class(cur, plan_leaves[i], bl[i]) == 0) { skip = true; break; }
    if (skip) continue;
    const blk_view bv = blk_open<false>(buf, cur, nullptr);
    const dev_col *gd0 = nullptr, *gd1 = nullptr;
    if (ph.n_group_cols > 0) gd0 = &cur.cols[ph.need_cols[ph.group_idx[0]]];
    if (ph.n_group_cols > 1) gd1 = &cur.cols[ph.need_cols[ph.group_idx[1]]];
    const uint32_t kl0 = ph.group_len[0], kl1 = ph.group_len[1];
    const dev_col &kc0 = cur.cols[ph.need_cols[dj.probe_idx]];
    const uint32_t rows = cur.row_count;
    for (uint32_t r = tid; r < rows; r += WG) {
      bool live = true;
      for (uint32_t i = 0; live && i < ph.n_leaves; i++)
        live = leaf_match(bv, cur, plan_leaves[i], bl[i], r);
      if (!live) continue;
      bool isn = false;
      const int64_t kv = col_value2(bv, cur, kc0, r, isn);
      uint64_t pv = 0;
      if (isn || !obx_keymap_probe(dj.km, kv, &pv)) continue;
      lane_cnt++;
      const uint64_t key = obx_join_key(
          dj, build_group_key(bv, ph.n_group_cols, gd0, gd1, kl0, kl1, r), pv);
      int gi = gtable_slot<OBX_GTABLE_BIG_SHIFT>(gtable, key);
      if (gi < 0) { /* global table full: surfaced as counters[2] */
        atomicAdd(&counters[2], 1ull);
        continue;
      }
      atomicAdd(&gtable[gi].count, 1ull);
      for (uint32_t a = 0; a < ph.n_aggs; a++) {
        if ((dj.own_mask >> a) & 1) { /* a payload aggregate */
          agg_term(dj.kind[a], false, 0, 0, (int64_t)pv, false, 0, false,
                   0, false, gcell_sink{gtable[gi].cells[a]});
          continue;
        }
        const dev_agg ag = ph.aggs[a];
        if (ag.kind == 0 && ag.ia == 0xFF) continue; /* COUNT(*): count */
        bool na = false, nb = false, nc = false;
        int64_t va = 0, vb = 0, vc = 0;
        if (ag.ia != 0xFF)
          va = col_value2(bv, cur, cur.cols[ph.need_cols[ag.ia]], r, na);
        if (ag.kind >= 4 && ag.ib != 0xFF)
          vb = col_value2(bv, cur, cur.cols[ph.need_cols[ag.ib]], r, nb);
        if (ag.kind == 5 && ag.ic != 0xFF)
          vc = col_value2(bv, cur, cur.cols[ph.need_cols[ag.ic]], r, nc);
        agg_term(ag.kind, false, ag.one_b, ag.one_c, va, na, vb, nb, vc, nc,
                 gcell_sink{gtable[gi].cells[a]});
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1)
    lane_cnt += (unsigned long long)__shfl_xor((long long)lane_cnt, off, 64);
  if (lane == 0 && lane_cnt)
    atomicAdd(&counters[8 + ((blockIdx.x * WAVES + wv) & 7)], lane_cnt);
}
