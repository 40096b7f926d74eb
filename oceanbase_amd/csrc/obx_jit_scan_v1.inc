/*
 * obx_jit_scan_v1.inc — first-generation scan codegen (included by
 * obx_jit_gen.cpp): the fallback for plans whose bounds the persistent kernel
 * (obx_jit_scan.inc) cannot prove, or under OBX_JIT_V2=0.
 *
 * Eligible plans: AND-only filter, SUM-family aggregates over <= 4 distinct
 * fast-decodable columns, dict-ref grouping with <= 16 cells, every block
 * LDS-stageable. The whole aggregate program is emitted as literals —
 * column indices, scale constants, pass slots. Sums are exact int128,
 * accumulated per window as four 32-bit-digit sums (returnless LDS atomics,
 * reconstructed exactly at the window merge) and merged per block.
 *
 * jit_gen_source lists the kernel's phases: header, per-block preamble,
 * sweep, merge. Each takes (plan, shape, strategy, out).
 */

static std::string jit_v1_sig(const jit_v1_strategy &st) {
  return "V1|p" + st.wpb + "|";
}

/* the null-pointer or named group dev_col argument of build_group_key */
static const char *jit_v1_gd(int NG, int g) {
  return NG > g ? (g ? "gd1" : "gd0") : "(const dev_col *)nullptr";
}

/* exact total of a window's four digit sums, into `tot` */
static void jit_v1_emit_digits(std::string &s, int wa, const char *brk) {
  jit_emit(s,
           "        {\n"
           "          uint64_t d0 = wacc[%1$d][cell][0], d1 = "
           "wacc[%1$d][cell][1];\n"
           "          uint64_t d2 = wacc[%1$d][cell][2], d3 = "
           "wacc[%1$d][cell][3];\n"
           "          unsigned __int128 tot =%2$s((unsigned __int128)d3 << 96) "
           "+\n"
           "              ((unsigned __int128)d2 << 64) +\n"
           "              ((unsigned __int128)d1 << 32) + d0;\n",
           wa, brk);
}

static void jit_v1_header(const dev_plan_hdr &ph, const jit_shape &js,
                          const jit_v1_strategy &st, std::string &s) {
  const int NG = ph.n_group_cols;
  s += "#include \"obx_dev_common.h\"\n\n";
  jit_emit(s, "#define OBX_JIT_WPB %s\n", st.wpb.c_str());
  jit_emit(s,
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
           (int)ph.n_leaves, NG, js.n_wa > 0 ? js.n_wa : 1);
  jit_emit(s,
           "#define GD0P %s\n#define GD1P %s\n"
           "#define KL0V %u\n#define KL1V %u\n\n",
           jit_v1_gd(NG, 0), jit_v1_gd(NG, 1), (unsigned)ph.group_len[0],
           (unsigned)ph.group_len[1]);
  jit_emit(s,
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
  jit_emit(s,
           "    for (uint32_t a = 0; a < %u; a++) {\n"
           "      tab.cell[s][a][0] = 0;\n"
           "      tab.cell[s][a][1] = 0;\n"
           "    }\n"
           "  }\n"
           "  if (tid == 0) wg_passed = 0;\n"
           "  __syncthreads();\n\n",
           (unsigned)ph.n_aggs);
}

/* block loop head: verdict, stage, the window loop, the filter (pass
   bitmap for several leaves, inline context for one), group and value
   contexts, window accumulator zero */
static void jit_v1_block_preamble(const dev_plan_hdr &ph, const jit_shape &js,
                                  const jit_v1_strategy &, std::string &s) {
  const int NG = ph.n_group_cols;
  const int NL = ph.n_leaves;
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
  for (int g = 0; g < NG; g++)
    jit_emit(s,
             "      const dev_col *gd%1$d = &cur.cols[%2$u];\n"
             "      col_ctx g%1$d = make_col_ctx(*gd%1$d, blk_bit);\n"
             "      const uint32_t dim%1$d = g%1$d.count + 1;\n",
             g, (unsigned)ph.need_cols[ph.group_idx[g]]);
  s += NG == 0 ? "      const uint32_t n_cells = 1;\n"
      : NG == 1 ? "      const uint32_t n_cells = dim0;\n"
                : "      const uint32_t n_cells = dim0 * dim1;\n";
  s += "      for (uint32_t i = tid; i < NWA * 16 * 4; i += WG)\n"
       "        (&wacc[0][0][0])[i] = 0;\n"
       "      for (uint32_t i = tid; i < 16; i += WG) wcnt[i] = 0;\n"
       "      if (tid == 0) spill_cnt = 0;\n"
       "      __syncthreads();\n";
  /* value-column contexts (registers: the specialized kernel carries no
     plan machinery, so the uniform budget allows it) */
  for (int j = 0; j < js.n_vc; j++)
    jit_emit(s,
             "      const col_ctx c%d = make_col_ctx(cur.cols[%u], "
             "blk_bit);\n",
             j, (unsigned)js.vcol[j]);
}

/* the aggregate program over one live row's decoded values */
static void jit_v1_agg_program(const dev_plan_hdr &ph, const jit_shape &js,
                               const jit_v1_strategy &, std::string &s) {
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg &g = ph.aggs[a];
    if (js.agg_wa[a] == 0xFF) continue;
    const int wa = js.agg_wa[a];
    const int ja = js.slot(ph, g.ia), jb = js.slot(ph, g.ib),
              jc = js.slot(ph, g.ic);
    switch (g.kind) {
      case OBX_AGG_COUNT: /* COUNT(col) */
        jit_emit(s,
                 "          if (!nu%d) atomicAdd(&wacc[%d][cell][0], 1ull);\n",
                 ja, wa);
        break;
      case OBX_AGG_SUM:
        jit_emit(s,
                 "          if (!nu%1$d && v%1$d)\n"
                 "            ACC4(%2$d, i128_from_i64(v%1$d));\n",
                 ja, wa);
        break;
      case OBX_AGG_SUM_PROD2: {
        jit_emit(s,
                 "          if (!nu%1$d && !nu%2$d) {\n"
                 "            i128v p2 = i128_mul_i64(v%1$d, %3$lldll - "
                 "v%2$d);\n"
                 "            if (p2.lo | p2.hi) ACC4(%4$d, p2);\n",
                 ja, jb, (long long)g.one_b, wa);
        if ((js.agg_f2 >> a) & 1) {
          const dev_agg &g3 = ph.aggs[a + 1];
          jit_emit(s,
                   "            if (!nu%1$d) {\n"
                   "              i128v p3 = i128_mul_pos_i64(p2, %2$lldll + "
                   "v%1$d);\n"
                   "              if (p3.lo | p3.hi) ACC4(%3$d, p3);\n"
                   "            }\n",
                   js.slot(ph, g3.ic), (long long)g3.one_c, wa + 1);
          a++;
        }
        s += "          }\n";
        break;
      }
      case OBX_AGG_SUM_PROD3:
        jit_emit(s,
                 "          if (!nu%1$d && !nu%2$d && !nu%3$d) {\n"
                 "            i128v p3 = i128_mul_pos_i64(\n"
                 "                i128_mul_i64(v%1$d, %4$lldll - v%2$d), "
                 "%5$lldll + v%3$d);\n"
                 "            if (p3.lo | p3.hi) ACC4(%6$d, p3);\n"
                 "          }\n",
                 ja, jb, jc, (long long)g.one_b, (long long)g.one_c, wa);
        break;
      case OBX_AGG_SUM_MUL:
        jit_emit(s,
                 "          if (!nu%1$d && !nu%2$d) {\n"
                 "            i128v p = i128_mul_i64(v%1$d, v%2$d);\n"
                 "            if (p.lo | p.hi) ACC4(%3$d, p);\n"
                 "          }\n",
                 ja, jb, wa);
        break;
      default:
        break;
    }
  }
}

static void jit_v1_sweep(const dev_plan_hdr &ph, const jit_shape &js,
                         const jit_v1_strategy &st, std::string &s) {
  const int NG = ph.n_group_cols;
  const int NL = ph.n_leaves;
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
  for (int g = 0; g < NG; g++) {
    jit_emit(s,
             "        uint32_t ref%1$d = (uint32_t)bit_read_at(\n"
             "            bv.base, bv.rbase_bit + (uint32_t)(gd%1$d->data_bit - "
             "blk_bit) +\n"
             "                         (uint64_t)r * g%1$d.W, g%1$d.W);\n"
             "        if (ref%1$d > g%1$d.count) ref%1$d = g%1$d.count;\n",
             g);
    s += g ? "        cell += ref1 * dim0;\n" : "        uint32_t cell = ref0;\n";
  }
  if (NG == 0) s += "        const uint32_t cell = 0;\n";
  s += "        if (live) {\n"
       "          rep_row[cell] = r;\n"
       "          atomicAdd(&wcnt[cell], 1ull);\n"
       "        }\n";
  for (int j = 0; j < js.n_vc; j++)
    jit_emit(s,
             "        bool nu%1$d;\n"
             "        int64_t v%1$d = ctx_value(bv, c%1$d, r, nu%1$d);\n",
             j);
  s += "        if (live) {\n";
  jit_v1_agg_program(ph, js, st, s);
  s += "        }\n"
       "      }\n";
  if (NL <= 1)
    s += "      if (lane == 0 && my_cnt) atomicAdd(&wg_passed, my_cnt);\n";
}

/* window merge into the workgroup's LDS table (full table: spill to the
   global one), then the LDS table's flush at the end of the kernel */
static void jit_v1_merge(const dev_plan_hdr &ph, const jit_shape &js,
                         const jit_v1_strategy &, std::string &s) {
  const int NG = ph.n_group_cols;
  s += "      __syncthreads();\n"
       "\n"
       "      /* merge the window accumulators into the group table */\n"
       "      for (uint32_t cell = tid; cell < n_cells; cell += WG) {\n"
       "        unsigned long long cnt2 = wcnt[cell];\n"
       "        if (!cnt2) continue;\n";
  jit_emit(s,
           "        uint64_t key = build_group_key(bv, NG, %s, %s, %u, %u,\n"
           "                                       rep_row[cell]);\n",
           jit_v1_gd(NG, 0), jit_v1_gd(NG, 1), (unsigned)ph.group_len[0],
           (unsigned)ph.group_len[1]);
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
    jit_v1_emit_digits(s, js.agg_wa[a], "\n              ");
    jit_emit(s,
             "          if (tot) {\n"
             "            i128v pv = {(uint64_t)tot, (uint64_t)(tot >> "
             "64)};\n"
             "            lds_acc_i128(tab.cell[s2][%u], pv);\n"
             "          }\n"
             "        }\n",
             (unsigned)a);
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
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (js.agg_wa[a] == 0xFF) {
      jit_emit(s, "        g_acc_i128(gtable[gidx].cells[%u], cnt2, 0);\n",
               (unsigned)a);
      continue;
    }
    jit_v1_emit_digits(s, js.agg_wa[a], " ");
    jit_emit(s,
             "          if (tot)\n"
             "            g_acc_i128(gtable[gidx].cells[%u], "
             "(uint64_t)tot,\n"
             "                       (uint64_t)(tot >> 64));\n"
             "        }\n",
             (unsigned)a);
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
       "    int found = 0;\n"
       "    for (int probe = 0; probe < OBX_GTABLE_SLOTS; probe++) {\n"
       "      unsigned long long cur_k = atomicCAS(&gtable[idx].key, "
       "OBX_KEY_EMPTY,\n"
       "                                           (unsigned long "
       "long)key);\n"
       "      if (cur_k == OBX_KEY_EMPTY || cur_k == key) { found = 1; "
       "break; }\n"
       "      idx = (idx + 1) & (OBX_GTABLE_SLOTS - 1);\n"
       "    }\n"
       "    unsigned long long cnt = tab.count[s];\n"
       "    /* global table full: the growth path, as the spill pass */\n"
       "    if (!found) { atomicAdd(&counters[1], cnt); continue; }\n"
       "    atomicAdd(&gtable[idx].count, cnt);\n";
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (js.agg_wa[a] == 0xFF)
      jit_emit(s,
               "    g_acc_i128(gtable[idx].cells[%u], cnt, 0); /* COUNT(*) "
               "*/\n",
               (unsigned)a);
    else
      jit_emit(s,
               "    g_acc_i128(gtable[idx].cells[%1$u], tab.cell[s][%1$u][0],\n"
               "               tab.cell[s][%1$u][1]);\n",
               (unsigned)a);
  }
  s += "  }\n"
       "}\n";
}

static std::string jit_gen_source(const dev_plan_hdr &ph, const jit_shape &js,
                                  const jit_v1_strategy &st) {
  std::string s;
  jit_v1_header(ph, js, st, s);
  jit_v1_block_preamble(ph, js, st, s);
  jit_v1_sweep(ph, js, st, s);
  jit_v1_merge(ph, js, st, s);
  return s;
}

static std::string jit_plan_sig(const dev_plan_hdr &ph) {
  /* everything the generated SOURCE depends on (operand VALUES live in the
     uploaded leaf/bleaf arrays, so they are not part of the key) */
  std::string k;
  jit_emit(k, "L%dG%dA%d|", (int)ph.n_leaves, (int)ph.n_group_cols,
           (int)ph.n_aggs);
  for (uint32_t g = 0; g < ph.n_group_cols; g++)
    jit_emit(k, "g%u:%u:%u|", g, (unsigned)ph.need_cols[ph.group_idx[g]],
             (unsigned)ph.group_len[g]);
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg &g = ph.aggs[a];
    jit_emit(k, "a%u:%u:%u:%u:%u:%lld:%lld|", a, (unsigned)g.kind,
             (unsigned)(g.ia == 0xFF ? 255 : ph.need_cols[g.ia]),
             (unsigned)(g.ib == 0xFF ? 255 : ph.need_cols[g.ib]),
             (unsigned)(g.ic == 0xFF ? 255 : ph.need_cols[g.ic]),
             (long long)g.one_b, (long long)g.one_c);
  }
  return k;
}
