/*
 * obx_kernels.hip — gfx950 (MI355X/CDNA4) kernels for the OLAP hot path:
 * microblock decode -> pushdown filter -> hash group-by aggregate.
 *
 * Design (MI355X-first, not a translation of the reference's AVX loops):
 *  - one 256-thread workgroup processes whole microblocks from a grid-stride
 *    loop; each block's encoded bytes are STAGED THROUGH LDS with coalesced
 *    dwordx4 copies (HBM sees exactly the encoded column pages, read once,
 *    fully coalesced), then all bit-granular decode reads hit LDS
 *    (~16 KB block << 160 KB LDS/CU). Blocks larger than
 *    OBX_LDS_STAGE_BYTES take a generic global-memory path.
 *  - white filters arrive pre-lowered per block (obx_dev.h): dict-domain
 *    64-bit ref masks or packed-domain unsigned ranges, so the inner loop is
 *    unpack + mask/range test + __ballot (cf. the reference's AVX512
 *    compares, ob_raw_decoder_simd.cpp, and dict-domain filters,
 *    ob_dict_decoder.cpp:810-886)
 *  - selection vectors are built with wavefront ballot + mbcnt prefix sums
 *    (the get_row_ids bitmap->row_ids compaction,
 *    ob_block_batched_row_store.cpp:107)
 *  - group-by: per-row group key -> wave-level cell clustering (ballot +
 *    64-wide shfl reductions of int128 partials) -> per-workgroup LDS table
 *    (int128 cells, carry-propagating u64 atomics) -> one global open-
 *    addressing table flush per workgroup (256-bit cells). Mirrors
 *    ObExtendHashTableVec + aggregate::Processor semantics
 *    (ob_exec_hash_struct_vec.h:1718, share/aggregate/sum.h) with exact
 *    integer arithmetic.
 *  - no MFMA anywhere: this path is memory-bound integer work.
 *
 * These are the GENERIC kernels: what every plan the JIT does not specialise
 * runs (MIN/MAX without a v2 strategy, OR programs, slow encodings, more
 * than 4 value columns, OBX_JIT=0, the growth path, the OBX_PIPELINE_AGG
 * kernel DAG) plus the get_rows decode kernels. Each step exists once
 * (obx_steps.h, which the join scan of obx_join.hip assembles too) and the
 * kernels are assembled from the steps:
 *   blk_open<STAGE>      open a block, staged or not      (obx_blk.h)
 *   filter_window<PROG>  phase 1: a row window -> LDS pass bitmap
 *   group_open/group_row a surviving row -> group-table slot; the table's
 *                        find-or-insert and the row-count sink are arguments
 *   opnd_open/opnd_value an aggregate operand: ctx fast path or col_value2
 *   agg_term / agg_row   a kind's term and null rule, into an lds_sink or a
 *                        gcell_sink
 *   flush_cells<NST>     LDS cell stripes -> global cell
 *   gtable_slot<SHIFT>   global table find-or-insert
 *   cell_init            a cell's start value for its kind
 *   lds_table_init / agg_passes / lds_table_flush
 *                        the fused bodies' LDS group table: start state,
 *                        phase 3 of a row window (agg_row(lds_sink) per
 *                        aggregate), the flush (gtable_slot + flush_cells)
 *   scan_direct_body     the growth path: open + leaf_match + gtable_slot +
 *                        agg_term(gcell_sink); what a join adds is an argument
 *   store_datum          one VEC_FIXED datum                (obx_blk.h)
 * scan_filter_agg_body = lds_table_init + per window (open + filter_window +
 * its row count + group_row(lds_slot) + agg_passes) + lds_table_flush;
 * filter_body = open + filter_window + bitmap / row-id output; k_group_pass =
 * open + group_row(gtable_slot); k_agg_pass = cell_init + open +
 * agg_row(lds_sink) + flush_cells; k_scan_agg_direct =
 * scan_direct_body(no_join); the decode kernels = open + decode_rows.
 */
#include "obx_steps.h"

/* ---------------- fused scan->filter->aggregate kernel ------------------ */
template <bool STAGE, bool PROG>
__device__ void scan_filter_agg_body(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr &ph,
    gslot *__restrict__ gtable, unsigned long long *__restrict__ counters,
    uint8_t *lds_blk) {
  __shared__ lds_table tab;
  __shared__ uint64_t pass_bm[OBX_MAX_BLOCK_ROWS / 64];
  /* leaf_bm (phase 1, combine programs only) and row_slot (phases 2-3) are
     live in disjoint phases — share the same 2 KB of LDS */
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
  const auto kind_of = [&](uint32_t a) { return ph.aggs[a].kind; };

  lds_table_init(&tab, ph.n_aggs, kind_of);
  if (tid == 0) wg_passed = 0;
  __syncthreads();

  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const dev_block &cur = blocks[b];
    const blk_leaf *bl = bleaves + (uint64_t)b * ph.n_leaves;
    /* constant-result short-circuit: fold the combine program over the
       lowered leaf classes — a FALSE block is skipped before staging (cf.
       the reference's filter constant results / skip-index pruning) */
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
    /* rows-passed count (lane 0 of each wave over its own words) */
    for (uint32_t it = 0; it < iters; it++) {
      if (lane == 0) {
        uint64_t m = pass_bm[it * WAVES + wv];
        if (m) atomicAdd(&wg_passed, (unsigned long long)__popcll(m));
      }
    }
    __syncthreads();

    if (ph.n_aggs) {
      /* ---- phase 2: group rows to LDS-table slots (row_slot map) ---- */
      const group_ctx g = group_open(ph, cur, blk_bit);
      if (g.ref_fast) {
        for (uint32_t i = tid; i < 64; i += WG) cell_slot[i] = 254;
        __syncthreads();
      }
      for (uint32_t it = 0; it < iters; it++) {
        uint32_t rr = it * WG + tid;
        uint64_t m = pass_bm[it * WAVES + wv];
        if (!m) { if (rr < rows) u.row_slot[rr] = 255; continue; }
        uint8_t slot8 = 255;
        if ((m >> lane) & 1)
          slot8 = group_row(
              bv, ph, g, cell_slot, w0 + rr, counters,
              [&](uint64_t key) { return lds_slot(&tab, key); },
              [&](uint8_t s) { atomicAdd(&tab.count[s][stripe], 1ull); });
        if (rr < rows) u.row_slot[rr] = slot8;
      }
      __syncthreads();

      /* ---- phase 3: one pass per aggregate ---- */
      agg_passes(bv, cur, ph, blk_bit, rows, w0, pass_bm, u.row_slot, &tab);
    }
    __syncthreads(); /* pass_bm reuse across windows */
    } /* window loop */
  }
  __syncthreads();

  lds_table_flush(&tab, &wg_passed, ph, kind_of, gtable, counters);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_filter_agg(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    gslot *__restrict__ gtable, unsigned long long *__restrict__ counters) {
  scan_filter_agg_body<false, false>(buf, blocks, n_blocks, plan_leaves,
                                     bleaves, ph, gtable, counters, nullptr);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_filter_agg_prog(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    gslot *__restrict__ gtable, unsigned long long *__restrict__ counters) {
  scan_filter_agg_body<false, true>(buf, blocks, n_blocks, plan_leaves,
                                    bleaves, ph, gtable, counters, nullptr);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_filter_agg_lds(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    gslot *__restrict__ gtable, unsigned long long *__restrict__ counters) {
  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];
  scan_filter_agg_body<true, false>(buf, blocks, n_blocks, plan_leaves,
                                    bleaves, ph, gtable, counters, lds_blk);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_filter_agg_prog_lds(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    gslot *__restrict__ gtable, unsigned long long *__restrict__ counters) {
  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];
  scan_filter_agg_body<true, true>(buf, blocks, n_blocks, plan_leaves,
                                   bleaves, ph, gtable, counters, lds_blk);
}

/* ---------------- filter-only kernel (bitmap + selection vectors) ------- */
template <bool STAGE, bool PROG>
__device__ void filter_body(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr &ph,
    uint64_t *__restrict__ bitmap, int32_t *__restrict__ row_ids,
    uint32_t *__restrict__ blk_counts,
    unsigned long long *__restrict__ counters, uint8_t *lds_blk) {
  __shared__ uint32_t wv_cnt[WAVES];
  __shared__ uint32_t wv_scan[WAVES];
  __shared__ uint32_t blk_written;
  __shared__ unsigned long long wg_passed;
  __shared__ uint64_t pass_bm[OBX_MAX_BLOCK_ROWS / 64];
  __shared__ uint64_t leaf_bm[8][OBX_MAX_BLOCK_ROWS / 64];

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63;
  const uint32_t wv = tid >> 6;
  if (tid == 0) wg_passed = 0;
  __syncthreads();

  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const dev_block &cur = blocks[b];
    const blk_leaf *bl = bleaves + (uint64_t)b * ph.n_leaves;
    /* constant-result short-circuit (see scan_filter_agg_body) */
    const uint8_t blk_verdict = fold_prog3(ph, cur, plan_leaves, bl);
    if (blk_verdict == 0) {
      if (row_ids && tid == 0) blk_counts[b] = 0;
      continue; /* bitmap is pre-zeroed */
    }
    if (tid == 0) blk_written = 0;
    const blk_view bv = blk_open<STAGE>(buf, cur, lds_blk);
    if (!STAGE) __syncthreads(); /* blk_written reset */
    const uint64_t blk_bit = cur.block_byte * 8;

    const uint32_t all_rows = cur.row_count;
    const uint64_t row_start = dev_block_row_start(&cur);
    for (uint32_t w0 = 0; w0 < all_rows; w0 += OBX_MAX_BLOCK_ROWS) {
    const uint32_t rows = (all_rows - w0 < OBX_MAX_BLOCK_ROWS)
                              ? all_rows - w0 : OBX_MAX_BLOCK_ROWS;
    const uint32_t iters = (rows + WG - 1) / WG;

    filter_window<PROG>(bv, cur, plan_leaves, bl, ph, blk_verdict, blk_bit,
                        rows, w0, pass_bm, &leaf_bm[0][0]);

    /* output: global bitmap words, pass counts, selection vectors */
    for (uint32_t it = 0; it < iters; it++) {
      uint64_t m = pass_bm[it * WAVES + wv];
      if (bitmap && lane == 0 && m) {
        uint64_t gbit = row_start + w0 + (uint64_t)it * WG +
                        (uint64_t)wv * 64;
        uint64_t widx = gbit >> 6;
        uint32_t sh = (uint32_t)(gbit & 63);
        atomicOr((unsigned long long *)&bitmap[widx],
                 (unsigned long long)(m << sh));
        if (sh && (m >> (64 - sh)))
          atomicOr((unsigned long long *)&bitmap[widx + 1],
                   (unsigned long long)(m >> (64 - sh)));
      }
      if (row_ids) {
        if (lane == 0) wv_cnt[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        if (tid == 0) {
          uint32_t acc = blk_written;
          for (uint32_t w = 0; w < WAVES; w++) {
            wv_scan[w] = acc;
            acc += wv_cnt[w];
          }
          blk_written = acc;
        }
        __syncthreads();
        uint32_t r = w0 + it * WG + tid;
        bool pass = (m >> lane) & 1;
        if (pass) {
          uint32_t below = __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0);
          below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), below);
          row_ids[row_start + wv_scan[wv] + below] = (int32_t)r;
        }
        __syncthreads();
      } else if (lane == 0 && m) {
        atomicAdd(&wg_passed, (unsigned long long)__popcll(m));
      }
    }
    __syncthreads(); /* pass_bm reuse across windows */
    } /* window loop */
    if (row_ids) {
      __syncthreads();
      if (tid == 0) {
        blk_counts[b] = blk_written;
        atomicAdd(&wg_passed, (unsigned long long)blk_written);
      }
    }
    __syncthreads();
  }
  if (tid == 0 && wg_passed) atomicAdd(&counters[0], wg_passed);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_filter(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    uint64_t *__restrict__ bitmap, int32_t *__restrict__ row_ids,
    uint32_t *__restrict__ blk_counts,
    unsigned long long *__restrict__ counters) {
  filter_body<false, false>(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                            bitmap, row_ids, blk_counts, counters, nullptr);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_filter_prog(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    uint64_t *__restrict__ bitmap, int32_t *__restrict__ row_ids,
    uint32_t *__restrict__ blk_counts,
    unsigned long long *__restrict__ counters) {
  filter_body<false, true>(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                           bitmap, row_ids, blk_counts, counters, nullptr);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_filter_lds(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    uint64_t *__restrict__ bitmap, int32_t *__restrict__ row_ids,
    uint32_t *__restrict__ blk_counts,
    unsigned long long *__restrict__ counters) {
  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];
  filter_body<true, false>(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                           bitmap, row_ids, blk_counts, counters, lds_blk);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_filter_prog_lds(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    uint64_t *__restrict__ bitmap, int32_t *__restrict__ row_ids,
    uint32_t *__restrict__ blk_counts,
    unsigned long long *__restrict__ counters) {
  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];
  filter_body<true, true>(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                          bitmap, row_ids, blk_counts, counters, lds_blk);
}

/* ---------------- decode kernels (get_rows equivalent, parity) ---------- */
/* every row of one column of an open block -> datums and null bytes */
__device__ __forceinline__ void decode_rows(const blk_view &bv,
                                            const dev_block &cur,
                                            uint32_t col, uint32_t datum_len,
                                            uint8_t *__restrict__ out,
                                            uint8_t *__restrict__ out_null) {
  const uint32_t rows = cur.row_count;
  const uint64_t row_start = dev_block_row_start(&cur);
  for (uint32_t r = threadIdx.x; r < rows; r += WG) {
    bool isn;
    int64_t v = col_value2(bv, cur, cur.cols[col], r, isn);
    store_datum(out + (row_start + r) * datum_len, isn ? 0 : (uint64_t)v,
                datum_len);
    if (out_null) out_null[row_start + r] = isn ? 1 : 0;
  }
}

template <bool STAGE>
__device__ __forceinline__ void decode_body(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, uint32_t col, uint32_t datum_len,
    uint8_t *__restrict__ out, uint8_t *__restrict__ out_null,
    uint8_t *lds_blk) {
  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const dev_block &cur = blocks[b];
    const blk_view bv = blk_open<STAGE>(buf, cur, lds_blk);
    decode_rows(bv, cur, col, datum_len, out, out_null);
  }
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_decode(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, uint32_t col, uint32_t datum_len,
    uint8_t *__restrict__ out, uint8_t *__restrict__ out_null) {
  decode_body<false>(buf, blocks, n_blocks, col, datum_len, out, out_null,
                     nullptr);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_decode_lds(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, uint32_t col, uint32_t datum_len,
    uint8_t *__restrict__ out, uint8_t *__restrict__ out_null) {
  /* staged get_rows: per-lane bit-granular reads hit LDS instead of L2
     (the global-read variant measured ~0.8 TB/s; staging reads the
     encoded bytes once, coalesced) */
  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];
  decode_body<true>(buf, blocks, n_blocks, col, datum_len, out, out_null,
                    lds_blk);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_decode_multi(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const uint16_t *__restrict__ proj,
    const uint8_t *__restrict__ lens, uint32_t n_proj,
    uint8_t *const *__restrict__ outs, uint8_t *const *__restrict__ onulls) {
  /* one stage per block, ALL projected columns decoded from LDS — the
     per-column variant re-reads every block once per column */
  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];
  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const dev_block &cur = blocks[b];
    const blk_view bv = blk_open<true>(buf, cur, lds_blk);
    for (uint32_t p = 0; p < n_proj; p++)
      decode_rows(bv, cur, proj[p], lens[p], outs[p],
                  onulls ? onulls[p] : nullptr);
  }
}

/* ---------------- device-side filter lowering ---------------------------
 * One thread per (block, leaf): translate the leaf into the block's packed
 * domain (the reference evaluates dict-domain filters once per dict entry,
 * ob_dict_decoder.cpp:810-886,1481-1561; and maps raw compares to its
 * fast SIMD paths, ob_raw_decoder.cpp:707-790). */
__device__ __forceinline__ void lower_range(__int128 D, __int128 D2,
                                            uint8_t op, uint64_t dmax,
                                            blk_leaf &out) {
  /* unsigned packed domain: v in [0, dmax]; D/D2 are the operands already
     mapped into that domain (may lie outside [0, dmax]) */
  out.invert = 0;
  switch (op) {
    case 0: /* EQ */
      if (D < 0 || D > (__int128)dmax) { out.mode = OBX_LEAF_NONE; return; }
      out.mode = OBX_LEAF_RANGE; out.lo = (uint64_t)D; out.hi = (uint64_t)D;
      return;
    case 5: /* NE */
      if (D < 0 || D > (__int128)dmax) { out.mode = OBX_LEAF_ALL; return; }
      out.mode = OBX_LEAF_RANGE; out.lo = (uint64_t)D; out.hi = (uint64_t)D;
      out.invert = 1;
      return;
    case 1: /* LE */
      if (D < 0) { out.mode = OBX_LEAF_NONE; return; }
      if (D >= (__int128)dmax) { out.mode = OBX_LEAF_ALL; return; }
      out.mode = OBX_LEAF_RANGE; out.lo = 0; out.hi = (uint64_t)D;
      return;
    case 2: /* LT */
      if (D <= 0) { out.mode = OBX_LEAF_NONE; return; }
      if (D > (__int128)dmax) { out.mode = OBX_LEAF_ALL; return; }
      out.mode = OBX_LEAF_RANGE; out.lo = 0; out.hi = (uint64_t)(D - 1);
      return;
    case 3: /* GE */
      if (D <= 0) { out.mode = OBX_LEAF_ALL; return; }
      if (D > (__int128)dmax) { out.mode = OBX_LEAF_NONE; return; }
      out.mode = OBX_LEAF_RANGE; out.lo = (uint64_t)D; out.hi = dmax;
      return;
    case 4: /* GT */
      if (D < 0) { out.mode = OBX_LEAF_ALL; return; }
      if (D >= (__int128)dmax) { out.mode = OBX_LEAF_NONE; return; }
      out.mode = OBX_LEAF_RANGE; out.lo = (uint64_t)(D + 1); out.hi = dmax;
      return;
    case 6: { /* BT */
      __int128 lo = D < 0 ? 0 : D;
      __int128 hi = D2 > (__int128)dmax ? (__int128)dmax : D2;
      if (lo > hi) { out.mode = OBX_LEAF_NONE; return; }
      out.mode = OBX_LEAF_RANGE; out.lo = (uint64_t)lo; out.hi = (uint64_t)hi;
      return;
    }
    default:
      out.mode = OBX_LEAF_VALUE;
      return;
  }
}

extern "C" __global__ void k_lower_leaves(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ pl, uint32_t n_leaves,
    uint32_t n_cols, const int64_t *__restrict__ minmax,
    blk_leaf *__restrict__ out) {
  uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t total = (uint64_t)n_blocks * n_leaves;
  if (idx >= total) return;
  uint32_t b = (uint32_t)(idx / n_leaves);
  uint32_t i = (uint32_t)(idx % n_leaves);
  const dev_leaf &lf = pl[i];
  const dev_col &c = blocks[b].cols[lf.col];
  blk_view bv; bv.base = buf; bv.bit_bias = 0; bv.rbase_bit = 0;
  blk_leaf o;
  o.mask = 0; o.lo = 0; o.hi = 0; o.mode = OBX_LEAF_VALUE; o.invert = 0;

  /* black (generic-expression) leaves: the filter-on-dict trick — a
     single-column program over a small dict evaluates ONCE PER ENTRY
     into a ref mask (ob_dict_decoder.cpp:1481-1561); a const column
     folds to ALL/NONE; anything else evaluates per row (VALUE mode,
     black_match). */
  if (lf.op == 10) {
    const dev_col &bc = blocks[b].cols[lf.bcols[0]];
    if (lf.n_bcols == 1 &&
        (bc.enc == OBX_D_DICT || bc.enc == OBX_D_RLE) && bc.count < 64) {
      for (uint32_t e = 0; e < bc.count; e++) {
        int64_t v = dict_entry(bv, bc, e);
        bool nu0 = false;
        if (black_eval_vals(lf, &v, &nu0)) o.mask |= 1ull << e;
      }
      o.mode = (o.mask == 0) ? OBX_LEAF_NONE : OBX_LEAF_REF_MASK;
    } else if (lf.n_bcols == 1 && bc.enc == OBX_D_CONST && bc.runs == 0) {
      int64_t v = bc.base;
      bool nu0 = (bc.count == 0);
      o.mode = black_eval_vals(lf, &v, &nu0) ? OBX_LEAF_ALL : OBX_LEAF_NONE;
    } else {
      o.mode = OBX_LEAF_VALUE;
    }
    out[idx] = o;
    return;
  }

  /* NOT const-with-exceptions: REF_MASK row evaluation reads a per-row
     ref (packed stream or RLE runs), which CONST does not have — its
     refs live in the exception list, so it takes the VALUE slow path
     (col_value2 walks the exceptions). */
  const bool is_dict = (c.enc == OBX_D_DICT || c.enc == OBX_D_RLE);

  /* key-set membership (IN_SET): a small dict is probed once per entry
     into a ref mask (the filter-on-dict path; the null ref stays unset); a
     const column folds to ALL/NONE; the packed-range family tests
     value = (packed ^ mask) + delta per row against the bitmap or the hash
     table; everything else probes the decoded value (VALUE mode). The
     stored min/max only ever proves NONE here, never ALL. */
  if (lf.op == 11) {
    const obx_keyset_dev ks = obx_leaf_keyset(lf);
    uint64_t delta = 0;
    bool packed_dom = false;
    if (ks.form == OBX_KS_EMPTY) {
      o.mode = OBX_LEAF_NONE;
    } else if (is_dict && c.count < 64) {
      for (uint32_t e = 0; e < c.count; e++)
        if (obx_keyset_probe(ks, dict_entry(bv, c, e))) o.mask |= 1ull << e;
      o.mode = (o.mask == 0) ? OBX_LEAF_NONE : OBX_LEAF_REF_MASK;
    } else if (c.enc == OBX_D_CONST && c.runs == 0) {
      o.mode = (c.count != 0 && obx_keyset_probe(ks, c.base)) ? OBX_LEAF_ALL
                                                              : OBX_LEAF_NONE;
    } else if (c.enc == OBX_D_RAW && (c.flags & OBX_DF_BITPACK)) {
      packed_dom = true; /* zero-extended field */
    } else if (c.enc == OBX_D_RAW && !(c.flags & OBX_DF_STRING)) {
      /* fixed width: a signed k-byte field is (packed ^ bias) - bias, the
         order map of the RANGE lowering below */
      const uint32_t kbits = (uint32_t)c.width * 8;
      const bool signed_dom =
          ((c.flags & OBX_DF_SIGNED) && c.width >= c.tss) ||
          (!(c.flags & OBX_DF_SIGNED) && c.width == 8);
      if (signed_dom && kbits >= 8 && kbits <= 64) {
        o.mask = 1ull << (kbits - 1);
        delta = 0 - o.mask;
      }
      packed_dom = true;
    } else if (c.enc == OBX_D_INTDIFF) {
      delta = (uint64_t)c.base;
      packed_dom = true;
    } else {
      o.mode = OBX_LEAF_VALUE;
    }
    if (packed_dom) {
      if (ks.form == OBX_KS_BITMAP) {
        o.mode = OBX_LEAF_SET_BITS;
        o.lo = delta - (uint64_t)ks.min;
        o.hi = ks.hi;
      } else {
        o.mode = OBX_LEAF_SET_HASH;
        o.lo = delta;
      }
    }
    if (minmax && !(c.flags & OBX_DF_STRING) &&
        (o.mode == OBX_LEAF_SET_BITS || o.mode == OBX_LEAF_SET_HASH ||
         o.mode == OBX_LEAF_VALUE)) {
      int64_t mn = minmax[2 * ((uint64_t)b * n_cols + lf.col)];
      int64_t mx = minmax[2 * ((uint64_t)b * n_cols + lf.col) + 1];
      if (!(mn == INT64_MIN && mx == INT64_MAX) &&
          (mn > mx || mx < ks.min || mn > ks.max))
        o.mode = OBX_LEAF_NONE;
    }
    out[idx] = o;
    return;
  }

  if (is_dict && c.count < 64) {
    if (lf.op == 8) {
      o.mask = 1ull << c.count;
    } else if (lf.op == 9) {
      o.mask = (c.count == 0) ? 0 : ((1ull << c.count) - 1);
    } else {
      for (uint32_t e = 0; e < c.count; e++) {
        int64_t v = dict_entry(bv, c, e);
        if (leaf_value_match(lf, v, false)) o.mask |= 1ull << e;
      }
    }
    o.mode = (o.mask == 0) ? OBX_LEAF_NONE : OBX_LEAF_REF_MASK;
  } else if (c.enc == OBX_D_RAW && (c.flags & OBX_DF_BITPACK) && lf.op <= 6) {
    uint64_t dmax = (c.width >= 64) ? ~0ull : ((1ull << c.width) - 1);
    lower_range((__int128)lf.vlo, (__int128)lf.vhi, lf.op, dmax, o);
  } else if (c.enc == OBX_D_RAW && !(c.flags & OBX_DF_BITPACK) &&
             !(c.flags & OBX_DF_STRING) && lf.op <= 6 && lf.op != 7 /* IN */) {
    /* fixed-width RAW numeric: k-byte domain. Signed iff the sign bit lives
       inside the stored bytes (INT class with width==tss, or DECIMAL);
       order-map signed domains to unsigned with an xor bias. */
    uint32_t kbits = (uint32_t)c.width * 8;
    uint64_t dmax = (kbits >= 64) ? ~0ull : ((1ull << kbits) - 1);
    bool signed_dom = ((c.flags & OBX_DF_SIGNED) && c.width >= c.tss) ||
                      (!(c.flags & OBX_DF_SIGNED) && c.width == 8);
    if (signed_dom) {
      uint64_t bias = 1ull << (kbits - 1);
      __int128 smin = -(__int128)bias, smax = (__int128)bias - 1;
      auto biasmap = [&](int64_t x) -> __int128 {
        __int128 v = x;
        if (v < smin) return (__int128)-1;          /* below domain */
        if (v > smax) return (__int128)dmax + 1;    /* above domain */
        return v + (__int128)bias;                  /* in [0, dmax] */
      };
      lower_range(biasmap(lf.vlo), biasmap(lf.vhi), lf.op, dmax, o);
      if (o.mode == OBX_LEAF_RANGE) o.mask = bias;
    } else {
      lower_range((__int128)lf.vlo, (__int128)lf.vhi, lf.op, dmax, o);
    }
  } else if (c.enc == OBX_D_INTDIFF && lf.op <= 6) {
    uint32_t kbits = (c.flags & OBX_DF_BITPACK) ? c.width : c.width * 8;
    uint64_t dmax = (kbits >= 64) ? ~0ull : ((1ull << kbits) - 1);
    lower_range((__int128)lf.vlo - c.base, (__int128)lf.vhi - c.base, lf.op,
                dmax, o);
  } else if ((c.enc == OBX_D_RAW || c.enc == OBX_D_INTDIFF) &&
             (lf.op == 8 || lf.op == 9)) {
    if (c.flags & OBX_DF_HAS_EXT) {
      o.mode = OBX_LEAF_NULL;
      o.invert = (lf.op == 9);
    } else {
      o.mode = (lf.op == 8) ? OBX_LEAF_NONE : OBX_LEAF_ALL;
    }
  } else if (c.enc == OBX_D_CONST && c.runs == 0) {
    bool isn = (c.count == 0);
    bool m = leaf_value_match(lf, c.base, isn);
    o.mode = m ? OBX_LEAF_ALL : OBX_LEAF_NONE;
  } else {
    o.mode = OBX_LEAF_VALUE;
  }

  /* Stored min/max skip-index refinement (the rebuild of the reference's
   * ObSSTableIndexFilter micro-block pruning,
   * /root/reference/src/storage/access/ob_sstable_index_filter.cpp: skip
   * a micro block whose [min,max] cannot satisfy the predicate, or mark
   * it all-pass). The per-(block,col) bounds are captured once at load
   * by k_col_minmax (the analogue of the skip index written at encode
   * time); strings are excluded (VALUE-mode compares map char through
   * char_key order, which the raw-LE bounds do not follow). */
  if (minmax && lf.op <= 6 && !(c.flags & OBX_DF_STRING) &&
      (o.mode == OBX_LEAF_RANGE || o.mode == OBX_LEAF_VALUE)) {
    int64_t mn = minmax[2 * ((uint64_t)b * n_cols + lf.col)];
    int64_t mx = minmax[2 * ((uint64_t)b * n_cols + lf.col) + 1];
    if (!(mn == INT64_MIN && mx == INT64_MAX)) { /* known bounds */
      bool none = false, all = false;
      if (mn > mx) { /* no non-null values in the block */
        none = true;
      } else {
        const int64_t lo = lf.vlo, hi = lf.vhi;
        switch (lf.op) {
          case 0: none = lo < mn || lo > mx; all = (mn == mx && mn == lo);
                  break;
          case 1: none = mn > lo; all = mx <= lo; break; /* LE */
          case 2: none = mn >= lo; all = mx < lo; break; /* LT */
          case 3: none = mx < lo; all = mn >= lo; break; /* GE */
          case 4: none = mx <= lo; all = mn > lo; break; /* GT */
          case 5: none = (mn == mx && mn == lo); all = lo < mn || lo > mx;
                  break;
          case 6: none = mx < lo || mn > hi; all = mn >= lo && mx <= hi;
                  break;
        }
      }
      if (none) o.mode = OBX_LEAF_NONE;
      else if (all) o.mode = OBX_LEAF_ALL; /* non-null rows all pass; ext
                                              nulls still excluded by the
                                              kernels' ALL handling */
    }
  }
  out[idx] = o;
}

/* Empty group table, written on the device before every scan: one u64 word
 * per thread over n_slots gslots plus tail_words zeroed counter words that
 * sit behind the table. Slot layout: key, count, cells[a][4]; MIN/MAX cells
 * start at their sentinel in limb 0 (bit a of min_mask / max_mask). */
extern "C" __global__ void k_gtable_init(
    unsigned long long *__restrict__ words, uint32_t n_slots,
    uint32_t tail_words, uint32_t min_mask, uint32_t max_mask) {
  const uint32_t SW = (uint32_t)(sizeof(gslot) / 8);
  const uint32_t total = n_slots * SW + tail_words;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  unsigned long long v = 0;
  if (i < n_slots * SW) {
    const uint32_t w = i % SW;
    if (w == 0) {
      v = OBX_KEY_EMPTY;
    } else if (w >= 2 && ((w - 2) & 3) == 0) {
      const uint32_t a = (w - 2) >> 2;
      if ((min_mask >> a) & 1) v = (unsigned long long)INT64_MAX;
      else if ((max_mask >> a) & 1) v = (unsigned long long)INT64_MIN;
    }
  }
  words[i] = v;
}

/* Packed per-block descriptors of the persistent scan JIT (obx_bdesc,
 * obx_dev.h), built once per (handle, column list): one thread per u64 word
 * of a record, so the 128-byte records are written coalesced. Words 0-1 are
 * the block header, 2-13 the column slots (obx_bdesc_pack_col, the function
 * the host probe checks), 14-15 padding. */
extern "C" __global__ void k_pack_bdesc(
    const dev_block *__restrict__ blocks, uint32_t n_blocks,
    const obx_bdesc_cols cols, obx_bdesc *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t blk = (uint32_t)(i >> 4), w = (uint32_t)i & 15;
  if (blk >= n_blocks) return;
  const dev_block &b = blocks[blk];
  uint64_t v = 0;
  if (w == 0) v = b.block_byte;
  else if (w == 1) v = (uint64_t)b.block_len | ((uint64_t)b.row_count << 32);
  else if (w - 2 < cols.n)
    (void)obx_bdesc_pack_col(&b.cols[cols.c[w - 2]], b.block_byte, &v);
  ((uint64_t *)out)[i] = v;
}

/* Per-(block,column) min/max of the NON-NULL decoded values, captured once
 * at load time — the engine's stored skip index (the reference writes
 * ObSkipIndex min/max rows at encode time, storage/blocksstable/index_block;
 * our container has no index block, so the bounds are derived from the
 * encoded data at load, outside every timed region). One wave per
 * (block,col). Output: out[2*(b*n_cols+c)] = {min, max};
 * {INT64_MIN, INT64_MAX} = unknown (strings/span encodings);
 * min > max = no non-null values. */
extern "C" __global__ void k_col_minmax(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, uint32_t n_cols, int64_t *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = threadIdx.x >> 6;
  uint64_t total = (uint64_t)n_blocks * n_cols;
  for (uint64_t wid = (uint64_t)blockIdx.x * WAVES + wv; wid < total;
       wid += (uint64_t)gridDim.x * WAVES) {
    uint32_t b = (uint32_t)(wid / n_cols), c = (uint32_t)(wid % n_cols);
    const dev_block &blk = blocks[b];
    const dev_col &dc = blk.cols[c];
    blk_view bv;
    bv.base = buf;
    bv.bit_bias = 0;
    bv.rbase_bit = 0;
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    bool known = true;
    if (dc.flags & OBX_DF_STRING) {
      known = false;
    } else {
      switch (dc.enc) {
        case OBX_D_DICT:
        case OBX_D_RLE:
          for (uint32_t e = lane; e < dc.count; e += 64) {
            int64_t v = dict_entry(bv, dc, e);
            if (v < mn) mn = v;
            if (v > mx) mx = v;
          }
          break;
        case OBX_D_CONST:
          if (dc.runs == 0) {
            if (lane == 0 && dc.count) mn = mx = dc.base;
          } else {
            for (uint32_t e = lane; e < dc.count; e += 64) {
              int64_t v = dict_entry(bv, dc, e);
              if (v < mn) mn = v;
              if (v > mx) mx = v;
            }
          }
          break;
        case OBX_D_RAW:
        case OBX_D_INTDIFF:
          for (uint32_t r = lane; r < blk.row_count; r += 64) {
            bool isn;
            int64_t v = col_value(bv, dc, r, isn);
            if (!isn) {
              if (v < mn) mn = v;
              if (v > mx) mx = v;
            }
          }
          break;
        default:
          known = false;
          break;
      }
    }
    if (!known) {
      mn = INT64_MIN;
      mx = INT64_MAX;
    }
    for (int off = 32; off > 0; off >>= 1) {
      int64_t omn = (int64_t)shflxor64((uint64_t)mn, off);
      int64_t omx = (int64_t)shflxor64((uint64_t)mx, off);
      if (known) { /* unknown is wave-uniform (depends only on dc) */
        if (omn < mn) mn = omn;
        if (omx > mx) mx = omx;
      }
    }
    if (lane == 0) {
      out[2 * wid] = mn;
      out[2 * wid + 1] = mx;
    }
  }
}

/* ======================================================================
 * Pass-pipeline aggregation (round-1 final design).
 *
 * The one-kernel fused design pays SGPR-spill scratch traffic and staging
 * barriers (profiles/r01_q1_sf100.md). The query instead runs as a short
 * kernel DAG — each pass small and register-lean, reading only its own
 * column streams directly from HBM (consecutive rows of one column are
 * contiguous -> coalesced; dict payloads stay hot in L1/L2):
 *
 *   k_filter(_lds)  -> survivor bitmap (1 bit/row)   [existing kernel]
 *   k_group_pass    -> row_slot[] (u8/row), global group keys + counts
 *   k_agg_pass x P  -> one aggregate (or a fused PROD2+PROD3 pair) per
 *                      pass; per-slot LDS cells, one global flush per WG
 *
 * Kernel boundaries are the inter-pass synchronization (~1.5 us each).
 * Slots are indices into the global group table (gslot); row_slot stores
 * them as u8 (255 = filtered out or table overflow; overflow counted).
 * ====================================================================== */

/* this row's bit from the global survivor bitmap */
__device__ __forceinline__ bool pass_bit(const uint64_t *__restrict__ bitmap,
                                         uint64_t grow) {
  return (bitmap[grow >> 6] >> (grow & 63)) & 1;
}

/* ---- group pass: map each surviving row to a global-table slot ---- */
extern "C" __global__ __launch_bounds__(WG, 2) void k_group_pass(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_plan_hdr ph,
    const uint64_t *__restrict__ bitmap, uint8_t *__restrict__ row_slot,
    gslot *__restrict__ gtable, unsigned long long *__restrict__ counters) {
  __shared__ uint8_t cell_slot[64];
  __shared__ unsigned long long cnt[OBX_GTABLE_SLOTS][4]; /* lane-striped */
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63;

  for (uint32_t i = tid; i < OBX_GTABLE_SLOTS; i += WG) {
    cnt[i][0] = 0; cnt[i][1] = 0; cnt[i][2] = 0; cnt[i][3] = 0;
  }
  __syncthreads();

  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const dev_block &cur = blocks[b];
    const blk_view bv = blk_open<false>(buf, cur, nullptr);
    const uint32_t rows = cur.row_count;
    const uint64_t row_start = dev_block_row_start(&cur);
    const group_ctx g = group_open(ph, cur, cur.block_byte * 8);
    if (g.ref_fast) {
      __syncthreads(); /* previous block's cell reads drain */
      for (uint32_t i = tid; i < 64; i += WG) cell_slot[i] = 254;
      __syncthreads();
    }

    const uint32_t iters = (rows + WG - 1) / WG;
    for (uint32_t it = 0; it < iters; it++) {
      uint32_t r = it * WG + tid;
      bool in = r < rows;
      uint8_t slot8 = 255;
      if (in && pass_bit(bitmap, row_start + r))
        slot8 = group_row(
            bv, ph, g, cell_slot, r, counters,
            [&](uint64_t key) {
              return gtable_slot<OBX_GTABLE_SHIFT>(gtable, key);
            },
            [&](uint8_t s) { atomicAdd(&cnt[s][lane & 3], 1ull); });
      if (in) row_slot[row_start + r] = slot8;
    }
  }
  __syncthreads();
  for (uint32_t s = tid; s < OBX_GTABLE_SLOTS; s += WG) {
    unsigned long long c = cnt[s][0] + cnt[s][1] + cnt[s][2] + cnt[s][3];
    if (c) atomicAdd(&gtable[s].count, c);
  }
}

/* ---- aggregate pass: one aggregate (or a fused PROD2+PROD3 pair) ---- */
extern "C" __global__ __launch_bounds__(WG, 2) void k_agg_pass(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_plan_hdr ph, uint32_t a,
    const uint64_t *__restrict__ bitmap, const uint8_t *__restrict__ row_slot,
    gslot *__restrict__ gtable) {
  /* per-slot LDS cells for this pass's aggregate(s): [slot][stripe][2] */
  __shared__ unsigned long long cells[2][OBX_GTABLE_SLOTS][4][2];
  const uint32_t tid = threadIdx.x;
  const uint32_t stripe = tid & 3;

  const dev_agg ag = ph.aggs[a];
  const bool fuse_p3 = obx_fuse_p3(ph.aggs, ph.n_aggs, a);
  const dev_agg ag2 = fuse_p3 ? ph.aggs[a + 1] : ag;

  for (uint32_t s = tid; s < OBX_GTABLE_SLOTS; s += WG) {
    for (uint32_t f = 0; f < 2; f++) {
      for (uint32_t st = 0; st < 4; st++) {
        cells[f][s][st][0] = cell_init(ag.kind);
        cells[f][s][st][1] = 0;
      }
    }
  }
  __syncthreads();

  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const dev_block &cur = blocks[b];
    const blk_view bv = blk_open<false>(buf, cur, nullptr);
    const uint64_t blk_bit = cur.block_byte * 8;
    const uint32_t rows = cur.row_count;
    const uint64_t row_start = dev_block_row_start(&cur);
    const agg_opnd oa = opnd_open(ph, cur, ag.ia, blk_bit);
    const agg_opnd ob = opnd_open(ph, cur, ag.ib, blk_bit);
    const agg_opnd oc = opnd_open(ph, cur, ag2.ic, blk_bit);

    for (uint32_t r = tid; r < rows; r += WG) {
      uint8_t slot8 = row_slot[row_start + r];
      if (slot8 == 255) continue;
      agg_row(bv, cur, ag.kind, fuse_p3, ag, ag2, oa, ob, oc, r,
              lds_sink{cells[0][slot8][stripe], cells[1][slot8][stripe]});
    }
  }
  __syncthreads();

  /* flush: merge the lane stripes, one global accumulate per slot */
  for (uint32_t s = tid; s < OBX_GTABLE_SLOTS; s += WG)
    for (uint32_t f = 0; f < (fuse_p3 ? 2u : 1u); f++)
      flush_cells<4>(cells[f][s], ph.aggs[a + f].kind,
                     gtable[s].cells[a + f]);
}

/* ---------------- high-cardinality direct-global scan --------------------
 * Growth path past the per-workgroup LDS group table (the reference's
 * ObHashGroupByOp hash table grows unboundedly,
 * ob_exec_hash_struct_vec.h:1718): when the generic kernel reports an LDS
 * table overflow, the host reruns the scan with this kernel
 * (scan_direct_body, obx_steps.h, with nothing between the filter and the
 * table). Correctness-first slow path — plans that fit the LDS table never
 * take it. AND-combined leaves only (the host keeps OBX_BUF_NOT_ENOUGH for
 * OR-programs). */
extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_agg_direct(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    gslot *__restrict__ gtable, unsigned long long *__restrict__ counters) {
  scan_direct_body(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                   gslot_table{gtable}, counters, no_join{});
}

/* ---------------- the sized group table (obx_grouphash.h) ----------------
 * Past OBX_GTABLE_BIG groups, under a cap the caller granted
 * (obx_gpu_set_max_groups): the same body on a hash table in device memory
 * sized from the cap. It counts its CAS winners and starts no further block
 * once they pass max_groups, so a grant that is too small costs a bounded
 * number of short probe sequences, never a table filled to the brim. The
 * host refuses the scan iff winners > max_groups or counters[2] != 0. */
extern "C" __global__ __launch_bounds__(WG, 2) void k_scan_agg_hash(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr ph,
    const obx_gh_dev table, uint64_t max_groups,
    unsigned long long *__restrict__ counters) {
  scan_direct_body(buf, blocks, n_blocks, plan_leaves, bleaves, ph,
                   sized_table{table, max_groups}, counters, no_join{});
}

/* Empty sized table and its zeroed counter block: one u64 word per thread
 * and step over the three arrays (EMPTY keys, zero counts, cells at zero
 * with limb 0 of a MIN / MAX cell at its sentinel, bit a of the masks as in
 * k_gtable_init). 64-bit word indices: the cell array alone passes 2^32
 * bytes long before the largest cap. */
extern "C" __global__ void k_group_hash_init(
    const obx_gh_dev table, unsigned long long *__restrict__ counters,
    uint32_t min_mask, uint32_t max_mask) {
  const uint64_t slots = obx_gh_n_slots(table);
  const uint64_t cell_words = slots * table.n_aggs * 4;
  const uint64_t total = 2 * slots + cell_words;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t0 < OBX_GH_COUNTER_WORDS) counters[t0] = 0;
  unsigned long long *keys = obx_gh_keys(table);
  unsigned long long *counts = obx_gh_count(table, 0);
  unsigned long long *cells = obx_gh_cell(table, 0, 0);
  for (uint64_t i = t0; i < total; i += step) {
    if (i < slots) {
      keys[i] = OBX_KEY_EMPTY;
    } else if (i < 2 * slots) {
      counts[i - slots] = 0;
    } else {
      const uint64_t w = i - 2 * slots;
      unsigned long long v = 0;
      if ((w & 3) == 0) {
        const uint32_t a = (uint32_t)((w >> 2) % table.n_aggs);
        if ((min_mask >> a) & 1) v = (unsigned long long)INT64_MAX;
        else if ((max_mask >> a) & 1) v = (unsigned long long)INT64_MIN;
      }
      cells[w] = v;
    }
  }
}

/* Live slots of a sized table -> dense records of 16 + 32 * n_aggs bytes
 * {key, count, cells}, so the host copies n_live records and not `slots`.
 * Every wave takes 64 slots at a time (slots is a multiple of 64): a ballot
 * of the live lanes, one add of its popcount into the cursor by lane 0 for
 * the wave's base, each live lane at base + its prefix. Record order is
 * whatever the adds make it; the host sorts. out holds `cap` records: the
 * host sized it from the winner count, and the test keeps a wrong count
 * from writing past it. */
extern "C" __global__ void k_group_compact(
    const obx_gh_dev table, unsigned long long *__restrict__ cursor,
    unsigned long long *__restrict__ out, uint64_t cap) {
  const uint64_t slots = obx_gh_n_slots(table);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t rec_words = 2 + 4 * table.n_aggs;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const unsigned long long *keys = obx_gh_keys(table);
  for (uint64_t s0 = wave * 64; s0 < slots; s0 += n_waves * 64) {
    const uint64_t s = s0 + lane;
    const unsigned long long key = keys[s];
    const bool live = key != OBX_KEY_EMPTY;
    const uint64_t m = __ballot(live);
    if (!m) continue;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
    base = (unsigned long long)__shfl((long long)base, 0, 64);
    if (!live) continue;
    const uint64_t at = base + __popcll(m & ((1ull << lane) - 1));
    if (at >= cap) continue;
    unsigned long long *rec = out + at * rec_words;
    rec[0] = key;
    rec[1] = *obx_gh_count(table, s);
    const unsigned long long *c = obx_gh_cell(table, s, 0);
    for (uint32_t w = 0; w < 4 * table.n_aggs; w++) rec[2 + w] = c[w];
  }
}
