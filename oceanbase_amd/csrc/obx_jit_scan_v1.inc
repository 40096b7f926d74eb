/*
 * obx_jit_scan_v1.inc — first-generation scan codegen (included by
 * obx_jit.inc): the fallback for plans whose bounds the persistent kernel
 * (obx_jit_scan.inc) cannot prove, or under OBX_JIT_V2=0.
 *
 * Eligible plans: AND-only filter, SUM-family aggregates over <= 4 distinct
 * fast-decodable columns, dict-ref grouping with <= 16 cells, every block
 * LDS-stageable. The whole aggregate program is emitted as literals —
 * column indices, scale constants, pass slots. Sums are exact int128,
 * accumulated per window as four 32-bit-digit sums (returnless LDS atomics,
 * reconstructed exactly at the window merge) and merged per block.
 */

static void jit_emit_agg_program(std::string &s, const dev_plan_hdr &ph,
                                 const jit_shape &js) {
  char buf2[512];
  auto reg_of = [&](uint8_t need_idx) -> int {
    uint8_t col = ph.need_cols[need_idx];
    for (int j = 0; j < js.n_vc; j++)
      if (js.vcol[j] == col) return j;
    return 0;
  };
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg &g = ph.aggs[a];
    if (js.agg_wa[a] == 0xFF) continue;
    int wa = js.agg_wa[a];
    switch (g.kind) {
      case OBX_AGG_COUNT: /* COUNT(col) */
        snprintf(buf2, sizeof buf2,
                 "          if (!nu%d) atomicAdd(&wacc[%d][cell][0], 1ull);\n",
                 reg_of(g.ia), wa);
        s += buf2;
        break;
      case OBX_AGG_SUM:
        snprintf(buf2, sizeof buf2,
                 "          if (!nu%d && v%d)\n"
                 "            ACC4(%d, i128_from_i64(v%d));\n",
                 reg_of(g.ia), reg_of(g.ia), wa, reg_of(g.ia));
        s += buf2;
        break;
      case OBX_AGG_SUM_PROD2: {
        bool f2 = (js.agg_f2 >> a) & 1;
        const dev_agg &g3 = f2 ? ph.aggs[a + 1] : g;
        snprintf(buf2, sizeof buf2,
                 "          if (!nu%d && !nu%d) {\n"
                 "            i128v p2 = i128_mul_i64(v%d, %lldll - v%d);\n"
                 "            if (p2.lo | p2.hi) ACC4(%d, p2);\n",
                 reg_of(g.ia), reg_of(g.ib), reg_of(g.ia),
                 (long long)g.one_b, reg_of(g.ib), wa);
        s += buf2;
        if (f2) {
          snprintf(buf2, sizeof buf2,
                   "            if (!nu%d) {\n"
                   "              i128v p3 = i128_mul_pos_i64(p2, %lldll + "
                   "v%d);\n"
                   "              if (p3.lo | p3.hi) ACC4(%d, p3);\n"
                   "            }\n",
                   reg_of(g3.ic), (long long)g3.one_c, reg_of(g3.ic), wa + 1);
          s += buf2;
          a++;
        }
        s += "          }\n";
        break;
      }
      case OBX_AGG_SUM_PROD3:
        snprintf(buf2, sizeof buf2,
                 "          if (!nu%d && !nu%d && !nu%d) {\n"
                 "            i128v p3 = i128_mul_pos_i64(\n"
                 "                i128_mul_i64(v%d, %lldll - v%d), %lldll + "
                 "v%d);\n"
                 "            if (p3.lo | p3.hi) ACC4(%d, p3);\n"
                 "          }\n",
                 reg_of(g.ia), reg_of(g.ib), reg_of(g.ic), reg_of(g.ia),
                 (long long)g.one_b, reg_of(g.ib), (long long)g.one_c,
                 reg_of(g.ic), wa);
        s += buf2;
        break;
      case OBX_AGG_SUM_MUL:
        snprintf(buf2, sizeof buf2,
                 "          if (!nu%d && !nu%d) {\n"
                 "            i128v p = i128_mul_i64(v%d, v%d);\n"
                 "            if (p.lo | p.hi) ACC4(%d, p);\n"
                 "          }\n",
                 reg_of(g.ia), reg_of(g.ib), reg_of(g.ia), reg_of(g.ib), wa);
        s += buf2;
        break;
      default:
        break;
    }
  }
}

static std::string jit_gen_source(const dev_plan_hdr &ph,
                                  const jit_shape &js) {
  const int NG = ph.n_group_cols;
  const int NL = ph.n_leaves;
  char b[1024];
  std::string s;
  s += "#define OBX_PIPELINE 0\n#include \"obx_dev_common.h\"\n\n";
  /* waves-per-block floor for the specialized kernel: 7 WGs/CU measured
     best for the Q1/Q6 shapes (LDS ~22 KB, ~72 VGPRs); OBX_JIT_WPB
     overrides for experiments */
  const char *wpb = getenv("OBX_JIT_WPB");
  s += std::string("#define OBX_JIT_WPB ") + (wpb ? wpb : "7") + "\n";
  snprintf(b, sizeof b,
           "#define NL %d\n#define NG %d\n#define NWA %d\n"
           "#define ACC4(WA, PV)                                          \\\n"
           "  do {                                                        \\\n"
           "    unsigned long long *w_ = wacc[WA][cell];                  \\\n"
           "    atomicAdd(&w_[0], (unsigned long long)(uint32_t)(PV).lo); \\\n"
           "    if ((uint32_t)((PV).lo >> 32))                            \\\n"
           "      atomicAdd(&w_[1],                                       \\\n"
           "                (unsigned long long)(uint32_t)((PV).lo >> 32)); \\\n"
           "    if ((uint32_t)(PV).hi)                                    \\\n"
           "      atomicAdd(&w_[2], (unsigned long long)(uint32_t)(PV).hi); \\\n"
           "    if ((uint32_t)((PV).hi >> 32))                            \\\n"
           "      atomicAdd(&w_[3], (unsigned long long)(int64_t)(int32_t)( \\\n"
           "                            (PV).hi >> 32));                  \\\n"
           "  } while (0)\n\n",
           NL, NG, js.n_wa > 0 ? js.n_wa : 1);
  s += b;
  snprintf(b, sizeof b,
           "#define GD0P %s\n#define GD1P %s\n"
           "#define KL0V %u\n#define KL1V %u\n\n",
           NG > 0 ? "gd0" : "(const dev_col *)nullptr",
           NG > 1 ? "gd1" : "(const dev_col *)nullptr",
           (unsigned)ph.group_len[0], (unsigned)ph.group_len[1]);
  s += b;
  snprintf(b, sizeof b,
           "/* right-sized LDS group table: the JIT kernel writes one\n"
           "   stripe and exactly n_aggs cells, cutting LDS for occupancy\n"
           "   (the generic lds_table is 16x8x2 cells) */\n"
           "struct jtab_t {\n"
           "  unsigned long long key[OBX_LTABLE_SLOTS];\n"
           "  unsigned long long count[OBX_LTABLE_SLOTS];\n"
           "  unsigned long long cell[OBX_LTABLE_SLOTS][%u][2];\n"
           "};\n"
           "__device__ __forceinline__ int jit_slot(jtab_t *t, uint64_t "
           "key) {\n"
           "  uint32_t idx = key_hash(key);\n"
           "  for (int probe = 0; probe < OBX_LTABLE_SLOTS; probe++) {\n"
           "    unsigned long long k = t->key[idx];\n"
           "    if (k == key) return (int)idx;\n"
           "    if (k == OBX_KEY_EMPTY) {\n"
           "      unsigned long long cur = atomicCAS(&t->key[idx], "
           "OBX_KEY_EMPTY,\n"
           "                                         (unsigned long "
           "long)key);\n"
           "      if (cur == OBX_KEY_EMPTY || cur == key) return "
           "(int)idx;\n"
           "    }\n"
           "    idx = (idx + 1) & (OBX_LTABLE_SLOTS - 1);\n"
           "  }\n"
           "  return -1;\n"
           "}\n\n",
           (unsigned)ph.n_aggs);
  s += b;
  s +=
      "extern \"C\" __global__ __launch_bounds__(256, OBX_JIT_WPB) void k_jit_scan(\n"
      "    const uint8_t *__restrict__ buf, const dev_block *__restrict__ "
      "blocks,\n"
      "    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,\n"
      "    const blk_leaf *__restrict__ bleaves, gslot *__restrict__ "
      "gtable,\n"
      "    unsigned long long *__restrict__ counters) {\n"
      "  __shared__ jtab_t tab;\n"
      "  __shared__ uint64_t pass_bm[OBX_MAX_BLOCK_ROWS / 64];\n"
      "  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];\n"
      "  __shared__ unsigned long long wacc[NWA][16][4];\n"
      "  __shared__ unsigned long long wcnt[16];\n"
      "  __shared__ uint32_t rep_row[16];\n"
      "  __shared__ unsigned long long wg_passed;\n"
      "  __shared__ uint16_t spill_list[16];\n"
      "  __shared__ uint32_t spill_cnt;\n"
      "  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;\n"
      "\n"
      "  for (uint32_t s = tid; s < OBX_LTABLE_SLOTS; s += WG) {\n"
      "    tab.key[s] = OBX_KEY_EMPTY;\n"
      "    tab.count[s] = 0;\n";
  snprintf(b, sizeof b,
           "    for (uint32_t a = 0; a < %u; a++) {\n"
           "      tab.cell[s][a][0] = 0;\n"
           "      tab.cell[s][a][1] = 0;\n"
           "    }\n"
           "  }\n"
           "  if (tid == 0) wg_passed = 0;\n"
           "  __syncthreads();\n\n",
           (unsigned)ph.n_aggs);
  s += b;
  s +=
      "  for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) "
      "{\n"
      "    const dev_block &cur = blocks[blk];\n"
      "    const blk_leaf *bl = bleaves + (uint64_t)blk * (NL ? NL : 1);\n"
      "    uint8_t blk_verdict = 1;\n"
      "    for (uint32_t i = 0; i < NL; i++) {\n"
      "      uint8_t c = leaf_class(cur, plan_leaves[i], bl[i]);\n"
      "      if (c == 0) { blk_verdict = 0; break; }\n"
      "      if (c == 2) blk_verdict = 2;\n"
      "    }\n"
      "    if (blk_verdict == 0) continue;\n"
      "    __syncthreads(); /* drain previous block's reads */\n"
      "    stage_issue(buf, cur, lds_blk);\n"
      "    stage_wait();\n"
      "    const uint64_t blk_bit = cur.block_byte * 8;\n"
      "    blk_view bv;\n"
      "    bv.base = lds_blk;\n"
      "    bv.bit_bias = blk_bit;\n"
      "    bv.rbase_bit = 0;\n"
      "\n"
      "    const uint32_t all_rows = cur.row_count;\n"
      "    for (uint32_t w0 = 0; w0 < all_rows; w0 += OBX_MAX_BLOCK_ROWS) "
      "{\n"
      "      const uint32_t rows = (all_rows - w0 < OBX_MAX_BLOCK_ROWS)\n"
      "                                ? all_rows - w0 : "
      "OBX_MAX_BLOCK_ROWS;\n"
      "      const uint32_t iters = (rows + WG - 1) / WG;\n"
      "\n";
  if (NL > 1) {
    s +=
      "      /* phase 1: AND-fission filter into the LDS pass bitmap (same\n"
      "         structure as the generic kernel) */\n"
      "      if (blk_verdict == 1) {\n"
      "        for (uint32_t it = 0; it < iters; it++) {\n"
      "          uint32_t rr = it * WG + tid;\n"
      "          uint64_t m = __ballot(rr < rows);\n"
      "          if (lane == 0) pass_bm[it * WAVES + wv] = m;\n"
      "        }\n"
      "      } else {\n"
      "        bool first = true;\n"
      "        for (uint32_t i = 0; i < NL; i++) {\n"
      "          const blk_leaf lfb = bl[i];\n"
      "          if (lfb.mode == OBX_LEAF_ALL &&\n"
      "              !(cur.cols[plan_leaves[i].col].flags & "
      "OBX_DF_HAS_EXT))\n"
      "            continue;\n"
      "          leaf_ctx lc = make_leaf_ctx(cur, plan_leaves[i], bl[i], "
      "blk_bit);\n"
      "          const bool slow = lc.slow;\n"
      "          for (uint32_t it = 0; it < iters; it++) {\n"
      "            uint64_t prev = first ? ~0ull : pass_bm[it * WAVES + "
      "wv];\n"
      "            if (!prev) {\n"
      "              if (first && lane == 0) pass_bm[it * WAVES + wv] = 0;\n"
      "              continue;\n"
      "            }\n"
      "            uint32_t rr = it * WG + tid;\n"
      "            uint32_t r = w0 + rr;\n"
      "            bool pass = rr < rows && ((prev >> lane) & 1);\n"
      "            if (pass)\n"
      "              pass = slow ? leaf_match(bv, cur, plan_leaves[i], "
      "bl[i], r)\n"
      "                          : leaf_ctx_match(bv, lc, plan_leaves[i], "
      "r);\n"
      "            uint64_t m = __ballot(pass);\n"
      "            if (lane == 0) pass_bm[it * WAVES + wv] = m;\n"
      "          }\n"
      "          first = false;\n"
      "        }\n"
      "        if (first) {\n"
      "          for (uint32_t it = 0; it < iters; it++) {\n"
      "            uint32_t rr = it * WG + tid;\n"
      "            uint64_t m = __ballot(rr < rows);\n"
      "            if (lane == 0) pass_bm[it * WAVES + wv] = m;\n"
      "          }\n"
      "        }\n"
      "      }\n"
      "      for (uint32_t it = 0; it < iters; it++) {\n"
      "        if (lane == 0) {\n"
      "          uint64_t m = pass_bm[it * WAVES + wv];\n"
      "          if (m) atomicAdd(&wg_passed, (unsigned long "
      "long)__popcll(m));\n"
      "        }\n"
      "      }\n"
      "      __syncthreads();\n"
      "\n";
  } else if (NL == 1) {
    /* single leaf: evaluated inline in the sweep below — no bitmap, no
       separate pass, one less barrier */
    s += "      leaf_ctx lc0 = make_leaf_ctx(cur, plan_leaves[0], bl[0], "
         "blk_bit);\n"
         "      const bool leaf_live =\n"
         "          blk_verdict != 1 &&\n"
         "          !(bl[0].mode == OBX_LEAF_ALL &&\n"
         "            !(cur.cols[plan_leaves[0].col].flags & "
         "OBX_DF_HAS_EXT));\n"
         "      unsigned long long my_cnt = 0;\n";
  } else {
    s += "      unsigned long long my_cnt = 0;\n";
  }
  /* group contexts + window accumulator zero */
  if (NG > 0) {
    snprintf(b, sizeof b,
             "      const dev_col *gd0 = &cur.cols[%u];\n"
             "      col_ctx g0 = make_col_ctx(*gd0, blk_bit);\n"
             "      const uint32_t dim0 = g0.count + 1;\n",
             (unsigned)ph.need_cols[ph.group_idx[0]]);
    s += b;
  }
  if (NG > 1) {
    snprintf(b, sizeof b,
             "      const dev_col *gd1 = &cur.cols[%u];\n"
             "      col_ctx g1 = make_col_ctx(*gd1, blk_bit);\n"
             "      const uint32_t dim1 = g1.count + 1;\n",
             (unsigned)ph.need_cols[ph.group_idx[1]]);
    s += b;
  }
  s += NG == 0 ? "      const uint32_t n_cells = 1;\n"
      : NG == 1 ? "      const uint32_t n_cells = dim0;\n"
                : "      const uint32_t n_cells = dim0 * dim1;\n";
  snprintf(b, sizeof b,
           "      for (uint32_t i = tid; i < NWA * 16 * 4; i += WG)\n"
           "        (&wacc[0][0][0])[i] = 0;\n"
           "      for (uint32_t i = tid; i < 16; i += WG) wcnt[i] = 0;\n"
           "      if (tid == 0) spill_cnt = 0;\n"
           "      __syncthreads();\n");
  s += b;
  /* value-column contexts (registers: the specialized kernel carries no
     plan machinery, so the uniform budget allows it) */
  for (int j = 0; j < js.n_vc; j++) {
    snprintf(b, sizeof b,
             "      const col_ctx c%d = make_col_ctx(cur.cols[%u], "
             "blk_bit);\n",
             j, (unsigned)js.vcol[j]);
    s += b;
  }
  s += "\n"
       "      for (uint32_t it = 0; it < iters; it++) {\n"
       "        uint32_t rr = it * WG + tid;\n";
  if (NL > 1) {
    s += "        uint64_t m = pass_bm[it * WAVES + wv];\n"
         "        if (!m) continue; /* wave-uniform skip */\n"
         "        const bool live = ((m >> lane) & 1) && rr < rows;\n"
         "        const uint32_t r = w0 + (rr < rows ? rr : 0);\n";
  } else {
    s += "        const uint32_t r = w0 + (rr < rows ? rr : 0);\n";
    if (NL == 1)
      s += "        bool live = rr < rows;\n"
           "        if (live && leaf_live)\n"
           "          live = lc0.slow\n"
           "                     ? leaf_match(bv, cur, plan_leaves[0], "
           "bl[0], r)\n"
           "                     : leaf_ctx_match(bv, lc0, plan_leaves[0], "
           "r);\n";
    else
      s += "        const bool live = rr < rows;\n";
    s += "        {\n"
         "          uint64_t pm = __ballot(live);\n"
         "          if (lane == 0) my_cnt += __popcll(pm);\n"
         "        }\n";
  }
  if (NG > 0)
    s += "        uint32_t ref0 = (uint32_t)bit_read_at(\n"
         "            bv.base, bv.rbase_bit + (uint32_t)(gd0->data_bit - "
         "blk_bit) +\n"
         "                         (uint64_t)r * g0.W, g0.W);\n"
         "        if (ref0 > g0.count) ref0 = g0.count;\n"
         "        uint32_t cell = ref0;\n";
  if (NG > 1)
    s += "        uint32_t ref1 = (uint32_t)bit_read_at(\n"
         "            bv.base, bv.rbase_bit + (uint32_t)(gd1->data_bit - "
         "blk_bit) +\n"
         "                         (uint64_t)r * g1.W, g1.W);\n"
         "        if (ref1 > g1.count) ref1 = g1.count;\n"
         "        cell += ref1 * dim0;\n";
  if (NG == 0) s += "        const uint32_t cell = 0;\n";
  s += "        if (live) {\n"
       "          rep_row[cell] = r;\n"
       "          atomicAdd(&wcnt[cell], 1ull);\n"
       "        }\n";
  for (int j = 0; j < js.n_vc; j++) {
    snprintf(b, sizeof b,
             "        bool nu%d;\n"
             "        int64_t v%d = ctx_value(bv, c%d, r, nu%d);\n",
             j, j, j, j);
    s += b;
  }
  s += "        if (live) {\n";
  jit_emit_agg_program(s, ph, js);
  s += "        }\n"
       "      }\n";
  if (NL <= 1)
    s += "      if (lane == 0 && my_cnt) atomicAdd(&wg_passed, my_cnt);\n";
  s += "      __syncthreads();\n"
       "\n"
       "      /* merge the window accumulators into the group table */\n"
       "      for (uint32_t cell = tid; cell < n_cells; cell += WG) {\n"
       "        unsigned long long cnt2 = wcnt[cell];\n"
       "        if (!cnt2) continue;\n";
  snprintf(b, sizeof b,
           "        uint64_t key = build_group_key(bv, NG, %s, %s, %u, %u,\n"
           "                                       rep_row[cell]);\n",
           NG > 0 ? "gd0" : "(const dev_col *)nullptr",
           NG > 1 ? "gd1" : "(const dev_col *)nullptr",
           (unsigned)ph.group_len[0], (unsigned)ph.group_len[1]);
  s += b;
  s += "        int s2 = jit_slot(&tab, key);\n"
       "        if (s2 < 0) {\n"
       "          /* WG-local table full: queue the cell for the cold\n"
       "             global-table spill pass below */\n"
       "          uint32_t si = atomicAdd(&spill_cnt, 1u);\n"
       "          if (si < 16) spill_list[si] = (uint16_t)cell;\n"
       "          else atomicAdd(&counters[1], cnt2);\n"
       "          continue;\n"
       "        }\n"
       "        atomicAdd(&tab.count[s2], cnt2);\n";
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (js.agg_wa[a] == 0xFF) continue;
    snprintf(b, sizeof b,
             "        {\n"
             "          uint64_t d0 = wacc[%d][cell][0], d1 = "
             "wacc[%d][cell][1];\n"
             "          uint64_t d2 = wacc[%d][cell][2], d3 = "
             "wacc[%d][cell][3];\n"
             "          unsigned __int128 tot =\n"
             "              ((unsigned __int128)d3 << 96) +\n"
             "              ((unsigned __int128)d2 << 64) +\n"
             "              ((unsigned __int128)d1 << 32) + d0;\n"
             "          if (tot) {\n"
             "            i128v pv = {(uint64_t)tot, (uint64_t)(tot >> "
             "64)};\n"
             "            lds_acc_i128(tab.cell[s2][%u], pv);\n"
             "          }\n"
             "        }\n",
             js.agg_wa[a], js.agg_wa[a], js.agg_wa[a], js.agg_wa[a],
             (unsigned)a);
    s += b;
  }
  s += "      }\n"
       "      __syncthreads(); /* spill list ready */\n"
       "      for (uint32_t i = tid; i < spill_cnt && i < 16; i += WG) {\n"
       "        uint32_t cell = spill_list[i];\n"
       "        unsigned long long cnt2 = wcnt[cell];\n"
       "        uint64_t key = build_group_key(bv, NG, "
       "GD0P, GD1P, KL0V, KL1V, rep_row[cell]);\n"
       "        uint32_t gidx = (uint32_t)((key * 0x9E3779B97F4A7C15ull) "
       ">> (64 - OBX_GTABLE_SHIFT)) &\n"
       "                       (OBX_GTABLE_SLOTS - 1);\n"
       "        int found = 0;\n"
       "        for (int probe = 0; probe < OBX_GTABLE_SLOTS; probe++) {\n"
       "          unsigned long long ck = atomicCAS(&gtable[gidx].key,\n"
       "                                            OBX_KEY_EMPTY,\n"
       "                                            (unsigned long "
       "long)key);\n"
       "          if (ck == OBX_KEY_EMPTY || ck == key) { found = 1; "
       "break; }\n"
       "          gidx = (gidx + 1) & (OBX_GTABLE_SLOTS - 1);\n"
       "        }\n"
       "        if (!found) { atomicAdd(&counters[1], cnt2); continue; }\n"
       "        atomicAdd(&gtable[gidx].count, cnt2);\n";
  for (uint32_t a2 = 0; a2 < ph.n_aggs; a2++) {
    if (js.agg_wa[a2] == 0xFF) {
      snprintf(b, sizeof b,
               "        g_acc_i128(gtable[gidx].cells[%u], cnt2, 0);\n",
               (unsigned)a2);
    } else {
      snprintf(b, sizeof b,
               "        {\n"
               "          uint64_t d0 = wacc[%d][cell][0], d1 = "
               "wacc[%d][cell][1];\n"
               "          uint64_t d2 = wacc[%d][cell][2], d3 = "
               "wacc[%d][cell][3];\n"
               "          unsigned __int128 tot = ((unsigned __int128)d3 "
               "<< 96) +\n"
               "              ((unsigned __int128)d2 << 64) +\n"
               "              ((unsigned __int128)d1 << 32) + d0;\n"
               "          if (tot)\n"
               "            g_acc_i128(gtable[gidx].cells[%u], "
               "(uint64_t)tot,\n"
               "                       (uint64_t)(tot >> 64));\n"
               "        }\n",
               js.agg_wa[a2], js.agg_wa[a2], js.agg_wa[a2], js.agg_wa[a2],
               (unsigned)a2);
    }
    s += b;
  }
  s += "      }\n"
       "      __syncthreads(); /* pass_bm / accumulator reuse */\n"
       "    } /* windows */\n"
       "  } /* blocks */\n"
       "  __syncthreads();\n"
       "\n"
       "  /* flush the LDS table to the global table */\n"
       "  if (tid == 0 && wg_passed) atomicAdd(&counters[0], wg_passed);\n"
       "  for (uint32_t s = tid; s < OBX_LTABLE_SLOTS; s += WG) {\n"
       "    uint64_t key = tab.key[s];\n"
       "    if (key == OBX_KEY_EMPTY) continue;\n"
       "    uint32_t idx = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - OBX_GTABLE_SHIFT)) "
       "&\n"
       "                   (OBX_GTABLE_SLOTS - 1);\n"
       "    for (int probe = 0; probe < OBX_GTABLE_SLOTS; probe++) {\n"
       "      unsigned long long cur_k = atomicCAS(&gtable[idx].key, "
       "OBX_KEY_EMPTY,\n"
       "                                           (unsigned long "
       "long)key);\n"
       "      if (cur_k == OBX_KEY_EMPTY || cur_k == key) break;\n"
       "      idx = (idx + 1) & (OBX_GTABLE_SLOTS - 1);\n"
       "    }\n"
       "    unsigned long long cnt = tab.count[s];\n"
       "    atomicAdd(&gtable[idx].count, cnt);\n";
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (js.agg_wa[a] == 0xFF) {
      snprintf(b, sizeof b,
               "    g_acc_i128(gtable[idx].cells[%u], cnt, 0); /* COUNT(*) "
               "*/\n",
               (unsigned)a);
    } else {
      snprintf(b, sizeof b,
               "    g_acc_i128(gtable[idx].cells[%u], tab.cell[s][%u][0],\n"
               "               tab.cell[s][%u][1]);\n",
               (unsigned)a, (unsigned)a, (unsigned)a);
    }
    s += b;
  }
  s += "  }\n"
       "}\n";
  return s;
}

static std::string jit_plan_sig(const dev_plan_hdr &ph) {
  /* everything the generated SOURCE depends on (operand VALUES live in the
     uploaded leaf/bleaf arrays, so they are not part of the key) */
  std::string k;
  char b[64];
  snprintf(b, sizeof b, "L%dG%dA%d|", ph.n_leaves, ph.n_group_cols,
           ph.n_aggs);
  k += b;
  for (uint32_t g = 0; g < ph.n_group_cols; g++) {
    snprintf(b, sizeof b, "g%u:%u:%u|", g,
             (unsigned)ph.need_cols[ph.group_idx[g]],
             (unsigned)ph.group_len[g]);
    k += b;
  }
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg &g = ph.aggs[a];
    snprintf(b, sizeof b, "a%u:%u:%u:%u:%u:%lld:%lld|", a, (unsigned)g.kind,
             (unsigned)(g.ia == 0xFF ? 255 : ph.need_cols[g.ia]),
             (unsigned)(g.ib == 0xFF ? 255 : ph.need_cols[g.ib]),
             (unsigned)(g.ic == 0xFF ? 255 : ph.need_cols[g.ic]),
             (long long)g.one_b, (long long)g.one_c);
    k += b;
  }
  return k;
}
