/*
 * obx_jit.inc — hipRTC-specialized scan kernels (included by obx_engine.cpp).
 *
 * The precompiled kernels are plan-generic: the aggregate program is data
 * (dev_plan_hdr), so every row pays descriptor loads, operand-select chains
 * and a pass per aggregate. PMC profiling (DESIGN.md round-1 findings) shows
 * the Q1 kernel near issue saturation — the ceiling is instructions per row,
 * and plan-generic machinery is most of them. This mirrors the reference's
 * own answer (vectorized expression codegen over the pushdown aggregate
 * plan, share/aggregate): specialize the kernel to the PLAN at runtime.
 *
 * For an eligible plan (AND-only filter, SUM-family aggregates over <=4
 * distinct fast-decodable columns, dict-ref grouping with <=16 cells, every
 * block LDS-stageable) the engine generates a HIP kernel with the whole
 * aggregate program as literals — column indices, scale constants, pass
 * slots — compiles it once with hipRTC (cached by plan signature), and
 * launches it instead of the generic kernels. Results are bit-identical:
 * the same decode helpers (obx_dev_common.h) and the same exact int128
 * arithmetic, accumulated as four 32-bit-digit sums (returnless LDS
 * atomics, reconstructed exactly at the window merge).
 *
 * OBX_JIT=0 disables; OBX_JIT_DUMP=1 writes the generated source to
 * gpurun_out/ (or /tmp) for offline inspection.
 */
#include <hip/hiprtc.h>

#include <map>
#include <string>

static const char *OBX_JIT_SRC_DEV_H =
#include "obx_embed_dev_h.inc"
    ;
static const char *OBX_JIT_SRC_COMMON_H =
#include "obx_embed_common_h.inc"
    ;

struct jit_entry {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  int wpb = 0; /* v2: workgroups per CU the launch grid is sized to */
};

static std::map<std::string, jit_entry> g_jit_cache;
static int g_jit_kind = 0; /* 1 = v1 generator, 2 = v2 (persistent) */

struct jit_shape {
  int n_vc = 0;
  uint8_t vcol[4] = {0xFF, 0xFF, 0xFF, 0xFF}; /* schema column indices */
  int n_wa = 0;
  uint8_t agg_wa[OBX_DEV_MAX_AGGS];  /* 0xFF = COUNT(*) */
  uint8_t agg_f2 = 0;                /* bit a: PROD2 fused with PROD3 mate */
  bool has_mm = false;               /* MIN/MAX present: v2-only (the v1
                                        generator has no CAS cells) */
};

/* plan-shape eligibility + operand mapping (schema column indices, so the
   generated source carries cur.cols[<literal>]) */
static bool jit_plan_shape(const dev_plan_hdr &ph, jit_shape &js) {
  if (ph.n_prog || ph.n_aggs == 0) return false;
  auto vc_add = [&](uint8_t need_idx) -> bool {
    if (need_idx == 0xFF) return true;
    uint8_t col = ph.need_cols[need_idx];
    for (int j = 0; j < js.n_vc; j++)
      if (js.vcol[j] == col) return true;
    if (js.n_vc >= 4) return false;
    js.vcol[js.n_vc++] = col;
    return true;
  };
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg &g = ph.aggs[a];
    js.agg_wa[a] = 0xFF;
    if (g.kind == OBX_AGG_COUNT && g.ia == 0xFF) continue;
    if (g.kind == OBX_AGG_MIN || g.kind == OBX_AGG_MAX) {
      js.has_mm = true;
      if (!vc_add(g.ia)) return false;
      continue; /* no window-accumulator slot */
    }
    if (g.kind != OBX_AGG_COUNT && g.kind != OBX_AGG_SUM &&
        g.kind != OBX_AGG_SUM_PROD2 && g.kind != OBX_AGG_SUM_PROD3 &&
        g.kind != OBX_AGG_SUM_MUL)
      return false;
    bool f2 = (g.kind == OBX_AGG_SUM_PROD2 && a + 1 < ph.n_aggs &&
               ph.aggs[a + 1].kind == OBX_AGG_SUM_PROD3 &&
               ph.aggs[a + 1].ia == g.ia && ph.aggs[a + 1].ib == g.ib);
    js.agg_wa[a] = (uint8_t)js.n_wa;
    if (!vc_add(g.ia) || !vc_add(g.ib) ||
        !vc_add(f2 ? ph.aggs[a + 1].ic : g.ic))
      return false;
    if (f2) {
      js.agg_f2 |= (uint8_t)(1u << a);
      js.agg_wa[a + 1] = (uint8_t)(js.n_wa + 1);
      a++;
    }
    js.n_wa += f2 ? 2 : 1;
  }
  return js.n_wa <= 8;
}

/* largest per-block group-cell product of a two-column grouping: walked
   once per (handle, column pair), then served from the handle */
static uint32_t jit_pair_cells_max(const obx_handle &h, uint8_t c0,
                                   uint8_t c1) {
  const uint32_t key = ((uint32_t)c0 << 16) | c1;
  auto it = h.pair_cells_max.find(key);
  if (it != h.pair_cells_max.end()) return it->second;
  const uint32_t nc = h.n_cols;
  uint32_t mx = 0;
  for (uint32_t b = 0; b < h.n_blocks; b++) {
    const uint8_t *cnt = &h.col_cnt[(size_t)b * nc];
    uint32_t cells = ((uint32_t)cnt[c0] + 1) * ((uint32_t)cnt[c1] + 1);
    if (cells > mx) mx = cells;
  }
  h.pair_cells_max[key] = mx;
  return mx;
}

/* eligibility over the whole handle (host-side: the encodings were
   captured at load time; the JIT kernel then assumes every block is fast —
   no in-kernel plan machinery, which is the whole point). Reads the
   per-column folds of the per-block arrays (summarize_col_classes); the
   decisions are those of a walk over every block: group columns dict with
   count < 16 and at most 16 cells per block, value columns neither slow
   nor string. */
static bool jit_blocks_ok(const obx_handle &h, const dev_plan_hdr &ph,
                          const jit_shape &js) {
  if (!h.lds_ok || h.col_class.empty()) return false;
  uint8_t gcol[2] = {0xFF, 0xFF};
  uint32_t cells = 1; /* product of the column maxima: an upper bound */
  for (uint32_t g = 0; g < ph.n_group_cols; g++) {
    gcol[g] = ph.need_cols[ph.group_idx[g]];
    if (!h.col_grp16_every[gcol[g]]) return false;
    cells *= h.col_cnt_max[gcol[g]] + 1;
  }
  /* the maxima may sit in different blocks: only then is the bound loose,
     and the exact per-block maximum decides */
  if (cells > 16 && (ph.n_group_cols < 2 ||
                     jit_pair_cells_max(h, gcol[0], gcol[1]) > 16))
    return false;
  for (int j = 0; j < js.n_vc; j++)
    if (h.col_slow_any[js.vcol[j]]) return false;
  return true;
}

#include "obx_jit_v2.inc"

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
    if (js.agg_f2 & (1u << a)) { /* handled with its PROD2 head */
    }
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

/* compile (or fetch) the specialized kernel; returns nullptr on any
   failure (caller falls back to the precompiled kernels) */
static jit_entry *jit_get(const dev_plan_hdr &ph, const jit_shape &js,
                          const jit_strategy &st) {
  std::string key = jit_plan_sig(ph);
  key += st.ok ? jit_strategy_sig(st) : "V1|";
  g_jit_kind = st.ok ? 2 : 1;
  auto it = g_jit_cache.find(key);
  if (it != g_jit_cache.end())
    return it->second.fn ? &it->second : nullptr;
  jit_entry ent; /* cache negative results too */
  ent.wpb = st.ok ? st.wpb : 0;
  g_jit_kind = st.ok ? 2 : 1;
  std::string src = st.ok ? jit_gen_source_v2(ph, js, st)
                          : jit_gen_source(ph, js);
  if (getenv("OBX_JIT_DUMP")) {
    FILE *f = fopen("gpurun_out/obx_jit_src.hip", "w");
    if (!f) f = fopen("/tmp/obx_jit_src.hip", "w");
    if (f) { fwrite(src.data(), 1, src.size(), f); fclose(f); }
  }
  hiprtcProgram prog;
  const char *hdrs[2] = {OBX_JIT_SRC_COMMON_H, OBX_JIT_SRC_DEV_H};
  const char *hdr_names[2] = {"obx_dev_common.h", "obx_dev.h"};
  if (hiprtcCreateProgram(&prog, src.c_str(), "obx_jit.hip", 2, hdrs,
                          hdr_names) != HIPRTC_SUCCESS) {
    g_jit_cache[key] = ent;
    return nullptr;
  }
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-DOBX_HIPRTC=1"};
  hiprtcResult cr = hiprtcCompileProgram(prog, 4, opts);
  if (cr != HIPRTC_SUCCESS) {
    size_t lsz = 0;
    hiprtcGetProgramLogSize(prog, &lsz);
    if (lsz > 1) {
      std::string log(lsz, '\0');
      hiprtcGetProgramLog(prog, &log[0]);
      fprintf(stderr, "obx: JIT compile failed:\n%s\n", log.c_str());
    }
    hiprtcDestroyProgram(&prog);
    g_jit_cache[key] = ent;
    return nullptr;
  }
  size_t csz = 0;
  hiprtcGetCodeSize(prog, &csz);
  std::string code(csz, '\0');
  hiprtcGetCode(prog, &code[0]);
  hiprtcDestroyProgram(&prog);
  if (hipModuleLoadData(&ent.mod, code.data()) != hipSuccess ||
      hipModuleGetFunction(&ent.fn, ent.mod, "k_jit_scan") != hipSuccess) {
    fprintf(stderr, "obx: JIT module load failed\n");
    ent.fn = nullptr;
    g_jit_cache[key] = ent;
    return nullptr;
  }
  auto r = g_jit_cache.emplace(key, ent);
  return &r.first->second;
}

/* prepare (compile/lookup) before the timed region; nullptr = use the
   precompiled kernels */
static jit_entry *jit_prepare(const obx_handle &h, const dev_plan_hdr &ph,
                              const dev_leaf *pl) {
  const char *e = getenv("OBX_JIT");
  if (e && e[0] == '0') return nullptr;
  jit_shape js;
  if (!jit_plan_shape(ph, js)) return nullptr;
  if (!jit_blocks_ok(h, ph, js)) return nullptr;
  jit_strategy st;
  jit_build_strategy(h, ph, js, pl, st); /* !ok -> v1 generator */
  if (!st.ok && js.has_mm) return nullptr; /* v1 cannot do MIN/MAX */
  return jit_get(ph, js, st);
}

static int jit_launch(jit_entry *je, obx_handle &h, hipStream_t stream,
                      uint32_t *grid_out) {
  /* v2 keeps its accumulators for the kernel's lifetime and flushes once
     per workgroup: its grid is a multiple of the resident set (the grid
     the strategy proved its i64 bound for); v1 merges per block and keeps
     the fixed grid */
  const uint32_t grid = je->wpb ? jit_grid_for(h.n_blocks, h.n_cus, je->wpb)
                                : grid_for(h.n_blocks);
  *grid_out = grid;
  void *args[7] = {&h.d_buf,     &h.d_blocks, &h.n_blocks, &h.d_pleaves,
                   &h.d_bleaves, &h.d_gtable, &h.d_counters};
  return hipModuleLaunchKernel(je->fn, grid, 1, 1, OBX_WG_HOST, 1, 1, 0,
                               stream, args, nullptr) == hipSuccess
             ? 0
             : -1;
}
