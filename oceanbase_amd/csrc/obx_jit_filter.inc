/*
 * obx_jit_filter.inc — filter-only codegen (obx_gpu_filter): strategy,
 * strategy signature, source (included by obx_jit_gen.cpp).
 *
 * Eligibility: one to four leaves, each packed-range or dict-mask (the
 * classes of the scan kernel's inline filter), or a key-set leaf (IN_SET) on
 * a packed-range-family column (staged mode only: per field the SET_BITS /
 * SET_HASH row test of k_lower_leaves against the set's bitmap or hash
 * table, the set's view loaded once per block). A filter touches only its
 * leaf streams, so neither mode stages whole blocks:
 *  - staged (default when the leaf streams of one block fit 18 KB of LDS;
 *    OBX_JIT_FSTAGE=0 forces the other): workgroup per block, each leaf's
 *    packed stream DMA'd to LDS with global_load_lds and evaluated from
 *    there. AND/OR combine programs and ordered row ids need this mode.
 *  - direct: wave per block slice, no barriers — each wave streams its
 *    leaf bytes through L1/L2, FU tiles of packed loads in flight.
 * Both strip-mine FR rows per lane when FR * width <= 64, assemble the
 * survivor mask in LDS and write the bitmap with two atomicOr per 64 rows.
 * OBX_JIT_FSL / OBX_JIT_FR / OBX_JIT_FU override slices, FR and FU.
 *
 * Layout: jit_build_fstrategy (the only place that reads the environment),
 * jit_fstrategy_sig, the fragments both modes share (combine-program fold,
 * stream and operand names per mode; the row tests themselves are in
 * obx_jit_gen.cpp), then the phases (plan, strategy, out): prologue; staged
 * parameters, sweep and kernel; direct kernel. jit_gen_source_filter lists
 * them.
 */

bool jit_build_fstrategy(const obx_table_facts &h, const dev_plan_hdr &ph,
                         const dev_leaf *pl, jit_fstrategy &st) {
  const char *e = getenv("OBX_JIT_V2");
  if (e && e[0] == '0') return false;
  if (ph.n_leaves == 0 || ph.n_leaves > 4) return false;
  /* AND/OR combine programs fold at CODEGEN: the postfix program is part
     of the plan signature, so the kernel gets a single boolean
     expression (the executor tree's shape, ob_pushdown_filter.cpp:1559,
     evaluated branch-free per row) */
  /* slice big blocks across waves so few-large-block sets still fill the
     chip (16K wave slots at 8 WGs/CU) */
  {
    uint32_t want = 3u * 16384u;
    uint32_t sl = h.n_blocks ? (want + h.n_blocks - 1) / h.n_blocks : 1;
    const char *se = getenv("OBX_JIT_FSL");
    if (se) sl = (uint32_t)atoi(se);
    if (sl < 1) sl = 1;
    if (sl > 16) sl = 16;
    st.nslice = (uint8_t)sl;
  }
  uint32_t wmax = 0;
  bool has_set = false;
  for (uint32_t i = 0; i < ph.n_leaves; i++) {
    const uint16_t col = pl[i].col;
    st.leaf_kind[i] = jit_leaf_kind(h, pl[i]);
    if (st.leaf_kind[i] == JL_NONE) return false;
    if (st.leaf_kind[i] == JL_SET) {
      /* every block lowers to SET_BITS / SET_HASH (by the set's form) or
         NONE */
      st.leaf_form[i] = obx_leaf_keyset(pl[i]).form;
      has_set = true;
    }
    st.leaf_cols[i] = col;
    if (h.col_maxw[col] > wmax) wmax = h.col_maxw[col];
  }
  /* strip-mine R rows per lane: one packed read covers R fields when
     R * max_width <= 64; narrow streams (dict refs, diff-coded dates)
     would otherwise leave the kernel iteration-rate-bound */
  {
    const char *re = getenv("OBX_JIT_FR");
    int r = re ? atoi(re) : (wmax && wmax * 4 <= 64 ? 4
                             : wmax && wmax * 2 <= 64 ? 2 : 1);
    if (r != 1 && r != 2 && r != 4) r = 1;
    st.r = (uint8_t)r;
    if (st.r > 1)
      for (uint32_t i = 0; i < ph.n_leaves; i++)
        st.leaf_multi[i] =
            h.col_maxw[st.leaf_cols[i]] * st.r <= 64 ? 1 : 0;
    /* software pipeline: hoist fu tiles' packed loads per superiteration
       so each wave keeps several HBM fetches in flight (the PMC profile
       shows the one-load-per-wave version is latency-bound at ~96% L2
       miss with waves waiting ~41k cycles) */
    const char *ue = getenv("OBX_JIT_FU");
    int u = ue ? atoi(ue) : 4;
    if (u < 1 || u > 8) u = 4;
    st.fu = (uint8_t)u;
  }
  /* staged mode: DMA each leaf's packed stream into LDS with
     global_load_lds (the same engine the persistent scan kernel uses to
     stream blocks at 3.4-4.5 TB/s) and evaluate from LDS -- plain
     per-lane global loads of thin streams measured only 0.43-2.5 TB/s
     (loads-only probe, profiles/r02) */
  {
    uint32_t total = 0;
    for (uint32_t i = 0; i < ph.n_leaves; i++) {
      /* stream bytes + align-down slack(15) + jit_bread overread(8),
         16-aligned */
      uint64_t bits = (uint64_t)h.col_maxw[st.leaf_cols[i]] *
                      (h.max_block_rows ? h.max_block_rows : 4096);
      uint64_t seg = (((bits + 7) / 8) + 48) & ~15ull;
      if (seg > 0xffffffffull) { total = 0xffffffffu; break; }
      st.fseg[i] = (uint32_t)seg;
      total += st.fseg[i];
    }
    const char *ge = getenv("OBX_JIT_FSTAGE");
    bool want = !ge || ge[0] != '0';
    if (want && total > 0 && total <= 18u * 1024u) st.fstage = 1;
  }
  /* combine programs are codegen-folded in the staged kernel only, and
     only it probes key sets */
  if ((ph.n_prog || has_set) && !st.fstage) return false;
  return true;
}

std::string jit_fstrategy_sig(const dev_plan_hdr &ph, const jit_fstrategy &st) {
  std::string k = "F|";
  jit_emit(k, "s%d|r%d|u%d|g%d:%u:%u:%u:%u|i%d:%u|", st.nslice, st.r, st.fu,
           st.fstage, st.fseg[0], st.fseg[1], st.fseg[2], st.fseg[3], st.frid,
           (unsigned)st.fnch);
  k += "P";
  for (uint32_t p2 = 0; p2 < ph.n_prog; p2++) jit_emit(k, "%u.", ph.prog[p2]);
  k += "|";
  for (uint32_t i = 0; i < ph.n_leaves; i++)
    jit_emit(k, "L%d:%u:m%d:k%d|", st.leaf_kind[i], st.leaf_cols[i],
             st.leaf_multi[i], st.leaf_form[i]);
  return k;
}

/* ---- fragments the phases share ---- */

/* Codegen fold of the postfix combine program (plan data, so the kernel
   gets one closed-form expression) over the items <name><leaf>: boolean
   (&&, ||) for the row test, three-valued (f3and, f3or) for the block
   verdict. No program = AND of all leaves. */
static std::string jit_f_fold_prog(const dev_plan_hdr &ph, const char *name,
                                   bool boolean) {
  auto item = [&](int i) { return name + std::to_string(i); };
  if (ph.n_prog == 0) {
    std::string e = boolean ? "(" : "";
    for (int i = 0; i < (int)ph.n_leaves; i++) {
      if (boolean) {
        if (i) e += " && ";
        e += item(i);
      } else {
        e = i == 0 ? item(i) : ("f3and(" + e + ", " + item(i) + ")");
      }
    }
    if (boolean) e += ")";
    return e;
  }
  std::string stk[16];
  int sp = 0;
  for (uint32_t p2 = 0; p2 < ph.n_prog; p2++) {
    const uint8_t tok = ph.prog[p2];
    if (tok < ph.n_leaves) {
      stk[sp++] = item(tok);
      continue;
    }
    const std::string b2 = stk[--sp], a2 = stk[sp - 1];
    if (boolean)
      stk[sp - 1] = "(" + a2 + (tok == 128 ? " && " : " || ") + b2 + ")";
    else
      stk[sp - 1] = (tok == 128 ? "f3and(" : "f3or(") + a2 + ", " + b2 + ")";
  }
  return stk[0];
}

/* staged mode: byte offset of leaf i's segment in the LDS buffer */
static uint32_t jit_f_seg_off(const jit_fstrategy &st, int i) {
  uint32_t off = 0;
  for (int q = 0; q < i; q++) off += st.fseg[q];
  return off;
}

/* leaf i's packed stream and lowered operands, as each mode names them:
   staged reads its LDS segment and the blkp in registers, direct reads the
   block in global memory and the blk_leaf (sfx: the pipelined tile) */
static jit_stream jit_f_staged_stream(const jit_fstrategy &st, int i) {
  return {jit_fmt("wl%d", i), jit_fmt("cur.W[%d]", i), jit_fmt("lmk%d", i),
          jit_fmt("seg + %uu", jit_f_seg_off(st, i)),
          jit_fmt("cur.bit[%d]", i)};
}
static jit_leaf_ops jit_f_staged_ops(int i) {
  return {i,
          jit_fmt("cur.lmask[%d]", i),
          jit_fmt("cur.llo[%d]", i),
          jit_fmt("cur.lhi[%d]", i),
          jit_fmt("cur.linv[%d]", i),
          jit_fmt("cur.lnone[%d]", i)};
}
static jit_stream jit_f_direct_stream(int i, const char *sfx) {
  return {jit_fmt("wl%d%s", i, sfx), jit_fmt("l%dW", i), jit_fmt("lmk%d", i),
          "bp", jit_fmt("l%do", i)};
}
static jit_leaf_ops jit_f_direct_ops(int i) {
  return {i,
          jit_fmt("lb%d.mask", i),
          jit_fmt("lb%d.lo", i),
          jit_fmt("lb%d.hi", i),
          jit_fmt("lb%d.invert", i),
          ""};
}

/* key-set leaf i (JL_SET) over one packed field: the SET_BITS or SET_HASH
   row test, as `const bool lf<i> = ...` for a combine program or as a step
   of the AND chain */
static std::string jit_f_set_test(const jit_fstrategy &st, int i,
                                  const std::string &field, bool chain) {
  const std::string n = std::to_string(i);
  const std::string v = "((" + field + " ^ cur.lmask[" + n +
                        "]) + (uint64_t)cur.llo[" + n + "])";
  std::string e;
  if (st.leaf_form[i] == OBX_KS_BITMAP)
    e = "!cur.lnone[" + n + "] &&\n              obx_ks_bit_test(cur.kw[" +
        n + "], " + v + ",\n              (uint64_t)cur.lhi[" + n + "])";
  else if (st.leaf_form[i] == OBX_KS_HASH)
    e = "!cur.lnone[" + n + "] &&\n              obx_ks_hash_test(cur.kw[" +
        n + "], cur.khi[" + n + "], cur.kshift[" + n + "],\n"
        "              cur.kmark[" + n + "], " + v + ")";
  else
    e = "false"; /* the empty set */
  return chain ? "          if (live)\n            live = " + e + ";\n"
               : "          const bool lf" + n + " = " + e + ";\n";
}

/* staged mode: every leaf's test of row r (field k of the packed words
   when `packed`), narrowing `live`; a combine program evaluates all leaves
   and folds them */
static void jit_f_staged_tests(const dev_plan_hdr &ph,
                               const jit_fstrategy &st, int pad, bool packed,
                               std::string &s) {
  const bool chain = ph.n_prog == 0;
  const std::string in(pad, ' ');
  if (!chain) s += in + "if (live) {\n";
  for (int i = 0; i < (int)ph.n_leaves; i++) {
    const std::string f =
        jit_f_staged_stream(st, i).field(packed && st.leaf_multi[i]);
    if (st.leaf_kind[i] == JL_SET)
      s += jit_f_set_test(st, i, f, chain);
    else if (st.leaf_kind[i] == JL_RANGE)
      jit_emit_range_test(s, pad, jit_f_staged_ops(i), f, chain);
    else
      jit_emit_mask_test(s, pad, jit_f_staged_ops(i), f, chain);
  }
  if (!chain)
    s += in + "live = " + jit_f_fold_prog(ph, "lf", true) + ";\n" + in +
         "}\n";
}

/* direct mode: the AND chain over row r */
static void jit_f_direct_tests(const dev_plan_hdr &ph,
                               const jit_fstrategy &st, int pad,
                               const char *sfx, bool packed, std::string &s) {
  for (int i = 0; i < (int)ph.n_leaves; i++) {
    const std::string f =
        jit_f_direct_stream(i, sfx).field(packed && st.leaf_multi[i]);
    if (st.leaf_kind[i] == JL_RANGE)
      jit_emit_range_test(s, pad, jit_f_direct_ops(i), f, true);
    else
      jit_emit_mask_test(s, pad, jit_f_direct_ops(i), f, true);
  }
}

/* ---- kernel phases ---- */

static void jit_f_prologue(const dev_plan_hdr &ph, const jit_fstrategy &st,
                           std::string &s) {
  s += "#include \"obx_dev_common.h\"\n"
       "#include \"obx_jit_dev.h\"\n\n";
  jit_emit(s,
           "#define NL %d\n#define FSL %d\n#define FR %d\n"
           "#define RID %d\n#define NCH %u\n",
           (int)ph.n_leaves, st.nslice > 0 ? st.nslice : 1,
           st.r > 0 ? st.r : 1, st.frid ? 1 : 0,
           (unsigned)(st.fnch ? st.fnch : 1));
}

/* staged mode: per-block parameters in registers (blkp, load_params) and
   the LDS DMA of the leaf streams (issue_stage). One LDS buffer: the
   LDS-DMA destination stays uniform + lane-linear. */
static void jit_f_staged_params(const dev_plan_hdr &ph,
                                const jit_fstrategy &st, std::string &s) {
  const int NL = ph.n_leaves;
  jit_emit(s, "#define SEGSZ %uu\n", jit_f_seg_off(st, NL));
  s += "struct blkp {\n"
       "  const uint8_t *bp;\n"
       "  uint64_t row0;\n"
       "  uint32_t blk, rows;\n";
  jit_emit(s,
           "  uint32_t W[%1$d], bit[%1$d], lo[%1$d], len[%1$d];\n"
           "  /* leaf payload in registers: loaded once per block, so\n"
           "     the sweep issues no global load of its own */\n"
           "  unsigned long long lmask[%1$d];\n"
           "  long long llo[%1$d], lhi[%1$d];\n"
           "  uint8_t linv[%1$d], lall[%1$d], lnone[%1$d];\n"
           "  /* key-set leaves: the set's view */\n"
           "  const uint64_t *kw[%1$d];\n"
           "  uint64_t khi[%1$d];\n"
           "  uint32_t kshift[%1$d], kmark[%1$d];\n"
           "};\n",
           NL);
  s += "__device__ __forceinline__ bool load_params(\n"
       "    const uint8_t *__restrict__ buf,\n"
       "    const dev_block *__restrict__ blocks,\n"
       "    const dev_leaf *__restrict__ plan_leaves,\n"
       "    const blk_leaf *__restrict__ bleaves, uint32_t blk,\n"
       "    blkp &p) {\n"
       "  const dev_block &cur = blocks[blk];\n"
       "  const blk_leaf *bl = bleaves + (size_t)blk * NL;\n";
  for (int i = 0; i < NL; i++)
    jit_emit(s,
             "  const uint8_t c%1$d = leaf_class(cur, plan_leaves[%1$d], "
             "bl[%1$d]);\n",
             i);
  s += "  if ((" + jit_f_fold_prog(ph, "c", false) + ") == 0) return false;\n";
  s += "  p.blk = blk;\n"
       "  p.rows = cur.row_count;\n"
       "  p.row0 = dev_block_row_start(&cur);\n"
       "  p.bp = buf + cur.block_byte;\n"
       "  const uint64_t blk_bit = cur.block_byte * 8;\n";
  for (int i = 0; i < NL; i++)
    jit_emit(s,
             "  {\n"
             "    const uint32_t o = (uint32_t)(cur.cols[%1$u].data_bit - "
             "blk_bit);\n"
             "    const uint32_t W = PW(cur.cols[%1$u]);\n"
             "    const uint32_t lo = (o >> 3) & ~15u;\n"
             "    p.W[%2$d] = W;\n"
             "    p.lo[%2$d] = lo;\n"
             "    p.bit[%2$d] = o - lo * 8;\n"
             "    p.len[%2$d] = ((((o + p.rows * W + 7) >> 3) - lo) + 15) & "
             "~15u;\n"
             "  }\n",
             (unsigned)st.leaf_cols[i], i);
  for (int i = 0; i < NL; i++) {
    jit_emit(s,
             "  p.lmask[%1$d] = bl[%1$d].mask;\n"
             "  p.llo[%1$d] = bl[%1$d].lo;\n"
             "  p.lhi[%1$d] = bl[%1$d].hi;\n"
             "  p.linv[%1$d] = bl[%1$d].invert;\n"
             "  p.lall[%1$d] = bl[%1$d].mode == OBX_LEAF_ALL ? 1 : 0;\n"
             "  p.lnone[%1$d] = bl[%1$d].mode == OBX_LEAF_NONE ? 1 : 0;\n",
             i);
    if (st.leaf_kind[i] == JL_SET)
      jit_emit(s,
               "  {\n"
               "    const obx_keyset_dev ks = "
               "obx_leaf_keyset(plan_leaves[%1$d]);\n"
               "    p.kw[%1$d] = ks.words;\n"
               "    p.khi[%1$d] = ks.hi;\n"
               "    p.kshift[%1$d] = ks.shift;\n"
               "    p.kmark[%1$d] = ks.has_marker;\n"
               "  }\n",
               i);
  }
  s += "  return true;\n"
       "}\n"
       "__device__ __forceinline__ void issue_stage(\n"
       "    const blkp &p, uint8_t *dst, uint32_t tid) {\n";
  for (int i = 0; i < NL; i++)
    jit_emit(s,
             "  for (uint32_t i2 = tid; i2 * 16 < p.len[%1$d]; i2 += WG)\n"
             "    __builtin_amdgcn_global_load_lds(\n"
             "        (const __attribute__((address_space(1))) uint32_t\n"
             "             *)(p.bp + p.lo[%1$d] + (size_t)i2 * 16),\n"
             "        (__attribute__((address_space(3))) uint32_t\n"
             "             *)(dst + %2$uu + (size_t)i2 * 16),\n"
             "        16, 0, 0);\n",
             i, jit_f_seg_off(st, i));
  s += "}\n";
}

/* staged mode: sweep of one staged block (emitted inside the block loop) */
static void jit_f_staged_sweep(const dev_plan_hdr &ph,
                               const jit_fstrategy &st, std::string &s) {
  const int NL = ph.n_leaves;
  const int SR = st.r > 1 ? st.r : 1;
  s += "      {\n";
  for (int i = 0; i < NL; i++)
    if (st.leaf_kind[i] == JL_RANGE)
      jit_emit(s, "      const bool l%1$d_all = cur.lall[%1$d] != 0;\n", i);
  if (SR > 1) {
    /* strip-mined LDS sweep: one packed ds_read covers SR fields, mask
       assembled via wave-synchronous LDS ORs (as direct mode) */
    for (int i = 0; i < NL; i++)
      if (st.leaf_multi[i])
        jit_emit(s,
                 "      const uint64_t lmk%1$d =\n"
                 "          ((uint64_t)1 << cur.W[%1$d]) - 1;\n",
                 i);
    s += "      const uint32_t rows = cur.rows;\n"
         "      const uint64_t row0 = cur.row0;\n"
         "      const uint32_t tiles = (rows + 64 * FR - 1) / (64 * "
         "FR);\n"
         "      for (uint32_t t = wv; t < tiles; t += WAVES) {\n"
         "        const uint32_t rt = t * 64 * FR + lane * FR;\n"
         "        if (lane < FR) fm[wv][lane] = 0;\n";
    for (int i = 0; i < NL; i++)
      if (st.leaf_multi[i])
        jit_emit(s,
                 "        uint64_t wl%1$d = (rt < rows)\n"
                 "            ? jit_bread(seg + %2$uu, cur.bit[%1$d] + rt * "
                 "cur.W[%1$d], FR * cur.W[%1$d])\n"
                 "            : 0;\n",
                 i, jit_f_seg_off(st, i));
    s += "        uint32_t pm = 0;\n"
         "#pragma unroll\n"
         "        for (uint32_t k = 0; k < FR; k++) {\n"
         "          const uint32_t r = rt + k;\n"
         "          bool live = r < rows;\n";
    jit_f_staged_tests(ph, st, 10, true, s);
    jit_emit(s,
             "          pm |= live ? (1u << k) : 0u;\n"
             "        }\n"
             "        lane_cnt += (uint32_t)__builtin_popcount(pm);\n"
             "        if (pm)\n"
             "          atomicOr(&fm[wv][lane >> %d],\n"
             "                   (unsigned long long)pm << ((lane & %uu) "
             "* FR));\n"
             "#if RID\n"
             "        if (lane < FR && t * FR + lane < NCH)\n"
             "          cmask[t * FR + lane] = fm[wv][lane];\n"
             "#endif\n"
             "        if (lane < FR) {\n"
             "          unsigned long long m = fm[wv][lane];\n"
             "          if (m) {\n"
             "            const uint64_t pos =\n"
             "                row0 + (uint64_t)t * (64 * FR) + lane * "
             "64;\n"
             "            const uint64_t w0 = pos >> 6;\n"
             "            const uint32_t sh = (uint32_t)(pos & 63);\n"
             "            atomicOr(&bitmap[w0], m << sh);\n"
             "            if (sh && (m >> (64 - sh)))\n"
             "              atomicOr(&bitmap[w0 + 1], m >> (64 - "
             "sh));\n"
             "          }\n"
             "        }\n"
             "      }\n"
             "      }\n",
             SR == 4 ? 4 : 5, SR == 4 ? 15u : 31u);
  } else {
    s += "      const uint32_t rows = cur.rows;\n"
         "      const uint64_t row0 = cur.row0;\n"
         "      const uint32_t n64 = (rows + 63) >> 6;\n"
         "      for (uint32_t it = wv; it < n64; it += WAVES) {\n"
         "        const uint32_t r = it * 64 + lane;\n"
         "        bool live = r < rows;\n";
    jit_f_staged_tests(ph, st, 8, false, s);
    s += "        uint64_t m = __ballot(live);\n"
         "#if RID\n"
         "        if (lane == 0 && it < NCH) cmask[it] = m;\n"
         "#endif\n"
         "        lane_cnt += live ? 1u : 0u;\n"
         "        if (lane == 0 && m) {\n"
         "          const uint64_t pos = row0 + (uint64_t)it * 64;\n"
         "          const uint64_t w0 = pos >> 6;\n"
         "          const uint32_t sh = (uint32_t)(pos & 63);\n"
         "          atomicOr(&bitmap[w0], m << sh);\n"
         "          if (sh && (m >> (64 - sh)))\n"
         "            atomicOr(&bitmap[w0 + 1], m >> (64 - sh));\n"
         "        }\n"
         "      }\n"
         "      }\n";
  }
  if (st.frid)
    s += "#if RID\n"
         "      /* ordered selection vectors from the captured chunk\n"
         "         masks (get_row_ids shape: block-local int32 row ids\n"
         "         at the block's absolute row offset) */\n"
         "      __syncthreads();\n"
         "      if (tid == 0) {\n"
         "        const uint32_t n64r = (cur.rows + 63) >> 6;\n"
         "        uint32_t acc = 0;\n"
         "        for (uint32_t c2 = 0; c2 < n64r; c2++) {\n"
         "          cpre[c2] = acc;\n"
         "          acc += (uint32_t)__popcll(cmask[c2]);\n"
         "        }\n"
         "        blk_counts[cur.blk] = acc;\n"
         "      }\n"
         "      __syncthreads();\n"
         "      {\n"
         "        const uint32_t n64r = (cur.rows + 63) >> 6;\n"
         "        for (uint32_t c2 = wv; c2 < n64r; c2 += WAVES) {\n"
         "          const unsigned long long m2 = cmask[c2];\n"
         "          if ((m2 >> lane) & 1) {\n"
         "            const uint32_t pos = cpre[c2] +\n"
         "                (uint32_t)__popcll(m2 &\n"
         "                    (((unsigned long long)1 << lane) - 1));\n"
         "            row_ids[cur.row0 + pos] = (int32_t)(c2 * 64 + "
         "lane);\n"
         "          }\n"
         "        }\n"
         "      }\n"
         "#endif\n";
}

/* staged mode: the kernel — workgroup per block, next passing block,
   stage, sweep; survivor count at the end */
static void jit_f_staged_kernel(const dev_plan_hdr &ph,
                                const jit_fstrategy &st, std::string &s) {
  s += "extern \"C\" __global__ __launch_bounds__(256, 8) void "
       "k_jit_filter(\n"
       "    const uint8_t *__restrict__ buf, const dev_block "
       "*__restrict__ blocks,\n"
       "    uint32_t n_blocks, const dev_leaf *__restrict__ "
       "plan_leaves,\n"
       "    const blk_leaf *__restrict__ bleaves,\n"
       "    unsigned long long *__restrict__ bitmap,\n"
       "    int32_t *__restrict__ row_ids,\n"
       "    uint32_t *__restrict__ blk_counts,\n"
       "    unsigned long long *__restrict__ counters) {\n"
       "  const uint32_t tid = threadIdx.x;\n"
       "  const uint32_t lane = tid & 63, wv = tid >> 6;\n"
       "  uint32_t lane_cnt = 0;\n"
       "  __shared__ uint8_t seg[SEGSZ];\n"
       "#if FR > 1\n"
       "  __shared__ unsigned long long fm[WAVES][FR];\n"
       "#endif\n"
       "#if RID\n"
       "  __shared__ unsigned long long cmask[NCH];\n"
       "  __shared__ uint32_t cpre[NCH];\n"
       "#endif\n"
       "  __shared__ unsigned long long wsum;\n"
       "  if (tid == 0) wsum = 0;\n"
       "  uint32_t bi = blockIdx.x;\n"
       "  const uint32_t gstep = gridDim.x;\n"
       "  for (;;) {\n"
       "    /* next block of this workgroup's stride that any row can pass */\n"
       "    bool v0 = false;\n"
       "    blkp cur;\n"
       "    while (bi < n_blocks) {\n"
       "      bool ok = load_params(buf, blocks, plan_leaves, "
       "bleaves, bi, cur);\n"
       "      bi += gstep;\n"
       "      if (ok) { v0 = true; break; }\n"
       "    }\n"
       "    if (!v0) break;\n"
       "    __syncthreads(); /* drain previous sweep's LDS reads */\n"
       "    issue_stage(cur, seg, tid);\n"
       "    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n"
       "    __syncthreads();\n";
  jit_f_staged_sweep(ph, st, s);
  s += "  }\n"
       "  /* one global atomic per WG into a slot striped by blockIdx:\n"
       "     16k same-address atomics serialized ~0.2 ms at L2 */\n"
       "  for (int off2 = 32; off2 > 0; off2 >>= 1)\n"
       "    lane_cnt += (uint32_t)__shfl_xor((int)lane_cnt, off2, 64);\n"
       "  __syncthreads();\n"
       "  if (lane == 0 && lane_cnt)\n"
       "    atomicAdd(&wsum, (unsigned long long)lane_cnt);\n"
       "  __syncthreads();\n"
       "  if (tid == 0 && wsum)\n"
       "    atomicAdd(&counters[8 + (blockIdx.x & 7)], wsum);\n"
       "}\n";
}

/* direct mode, strip-mined: a tile is 64*FR rows per wave. The packed
   loads of tile `itx`, into names suffixed sfx ... */
static void jit_f_direct_loads(const dev_plan_hdr &ph,
                               const jit_fstrategy &st, const char *sfx,
                               const char *itx, std::string &s) {
  jit_emit(s,
           "      const uint32_t rt%s = rbeg + (%s) * 64 * FR + lane * "
           "FR;\n",
           sfx, itx);
  for (int i = 0; i < (int)ph.n_leaves; i++)
    if (st.leaf_multi[i])
      jit_emit(s,
               "      uint64_t wl%1$d%2$s = (rt%2$s < rend)\n"
               "          ? jit_bread(bp, l%1$do + rt%2$s * l%1$dW, FR * "
               "l%1$dW)\n"
               "          : 0;\n",
               i, sfx);
}

/* ... and the tile body that consumes them */
static void jit_f_direct_tile(const dev_plan_hdr &ph,
                              const jit_fstrategy &st, const char *sfx,
                              const char *itx, std::string &s) {
  s += "      if (lane < FR) fm[wv][lane] = 0;\n"
       "      {\n"
       "      uint32_t pm = 0;\n"
       "#pragma unroll\n"
       "      for (uint32_t k = 0; k < FR; k++) {\n";
  jit_emit(s,
           "        const uint32_t r = rt%s + k;\n"
           "        bool live = r < rend;\n",
           sfx);
  jit_f_direct_tests(ph, st, 8, sfx, true, s);
  jit_emit(s,
           "        pm |= live ? (1u << k) : 0u;\n"
           "      }\n"
           "      lane_cnt += (uint32_t)__builtin_popcount(pm);\n"
           "      /* wave-synchronous LDS mask assembly: DS ops of one\n"
           "         wave execute in program order (lockstep wave64), "
           "so\n"
           "         the read below sees every lane's OR, barrier-free "
           "*/\n"
           "      if (pm)\n"
           "        atomicOr(&fm[wv][lane >> %d],\n"
           "                 (unsigned long long)pm << ((lane & %uu) * "
           "FR));\n"
           "      if (lane < FR) {\n"
           "        unsigned long long m = fm[wv][lane];\n"
           "        if (m) {\n"
           "          const uint64_t pos =\n"
           "              row0 + (uint64_t)(%s) * (64 * FR) + lane * "
           "64;\n"
           "          const uint64_t w0 = pos >> 6;\n"
           "          const uint32_t sh = (uint32_t)(pos & 63);\n"
           "          atomicOr(&bitmap[w0], m << sh);\n"
           "          if (sh && (m >> (64 - sh)))\n"
           "            atomicOr(&bitmap[w0 + 1], m >> (64 - sh));\n"
           "        }\n"
           "      }\n"
           "      }\n",
           st.r == 4 ? 4 : 5, st.r == 4 ? 15u : 31u, itx);
}

/* direct mode: the kernel — wave per block slice, no barriers */
static void jit_f_direct_kernel(const dev_plan_hdr &ph,
                                const jit_fstrategy &st, std::string &s) {
  const int NL = ph.n_leaves;
  s += "extern \"C\" __global__ __launch_bounds__(256, 8) void "
       "k_jit_filter(\n"
       "    const uint8_t *__restrict__ buf, const dev_block *__restrict__ "
       "blocks,\n"
       "    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,\n"
       "    const blk_leaf *__restrict__ bleaves,\n"
       "    unsigned long long *__restrict__ bitmap,\n"
       "    int32_t *__restrict__ row_ids,\n"
       "    uint32_t *__restrict__ blk_counts,\n"
       "    unsigned long long *__restrict__ counters) {\n"
       "  const uint32_t tid = threadIdx.x;\n"
       "  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;\n"
       "  uint32_t lane_cnt = 0;\n"
       "  __shared__ unsigned long long wsum;\n"
       "  if (tid == 0) wsum = 0;\n"
       "#if FR > 1\n"
       "  __shared__ unsigned long long fm[WAVES][FR];\n"
       "#endif\n"
       "  const uint64_t n_work = (uint64_t)n_blocks * FSL;\n"
       "  for (uint64_t w = (uint64_t)blockIdx.x * WAVES + wv;\n"
       "       w < n_work; w += (uint64_t)gridDim.x * WAVES) {\n"
       "    const uint64_t blk = w / FSL;\n"
       "    const uint32_t sl = (uint32_t)(w % FSL);\n"
       "    const dev_block &cur = blocks[blk];\n"
       "    const blk_leaf *bl = bleaves + blk * NL;\n"
       "    uint8_t blk_verdict = 1;\n"
       "    for (uint32_t i = 0; i < NL; i++) {\n"
       "      uint8_t c = leaf_class(cur, plan_leaves[i], bl[i]);\n"
       "      if (c == 0) { blk_verdict = 0; break; }\n"
       "      if (c == 2) blk_verdict = 2;\n"
       "    }\n"
       "    if (blk_verdict == 0) continue;\n"
       "    const uint8_t *bp = buf + cur.block_byte;\n"
       "    const uint64_t blk_bit = cur.block_byte * 8;\n"
       "    const uint32_t all_rows = cur.row_count;\n"
       "    /* 64-aligned row slice of this block */\n"
       "    const uint32_t chunk =\n"
       "        ((all_rows + FSL * 64 - 1) / (FSL * 64)) * 64;\n"
       "    const uint32_t rbeg = sl * chunk;\n"
       "    if (rbeg >= all_rows) continue;\n"
       "    const uint32_t rend =\n"
       "        (rbeg + chunk < all_rows) ? rbeg + chunk : all_rows;\n"
       "    const uint64_t row0 = dev_block_row_start(&cur) + rbeg;\n";
  for (int i = 0; i < NL; i++) {
    jit_emit(s,
             "    const blk_leaf lb%1$d = bl[%1$d];\n"
             "    const uint32_t l%1$do =\n"
             "        (uint32_t)(cur.cols[%2$u].data_bit - blk_bit);\n"
             "    const uint32_t l%1$dW = PW(cur.cols[%2$u]);\n",
             i, (unsigned)st.leaf_cols[i]);
    if (st.leaf_kind[i] == JL_RANGE)
      jit_emit(s,
               "    const bool l%1$d_all = lb%1$d.mode == OBX_LEAF_ALL;\n", i);
  }
  if (st.r > 1) {
    for (int i = 0; i < NL; i++)
      if (st.leaf_multi[i])
        jit_emit(s,
                 "    const uint64_t lmk%1$d = ((uint64_t)1 << l%1$dW) - 1;\n",
                 i);
    /* the superiteration emits FU tiles' loads before any tile body, so
       each wave keeps FU independent HBM fetches in flight (in-order vmcnt
       retirement pipelines them) */
    const int FU = st.fu > 0 ? st.fu : 1;
    s += "    const uint32_t nr = rend - rbeg;\n"
         "    const uint32_t iters = (nr + 64 * FR - 1) / (64 * FR);\n"
         "    uint32_t it = 0;\n";
    if (FU > 1) {
      jit_emit(s, "    for (; it + %1$d <= iters; it += %1$d) {\n", FU);
      for (int u = 0; u < FU; u++)
        jit_f_direct_loads(ph, st, jit_fmt("_%d", u).c_str(),
                           jit_fmt("it + %d", u).c_str(), s);
      for (int u = 0; u < FU; u++)
        jit_f_direct_tile(ph, st, jit_fmt("_%d", u).c_str(),
                          jit_fmt("it + %d", u).c_str(), s);
      s += "    }\n";
    }
    s += "    for (; it < iters; it++) {\n";
    jit_f_direct_loads(ph, st, "", "it", s);
    jit_f_direct_tile(ph, st, "", "it", s);
    s += "    }\n"
         "  }\n";
  } else {
    s += "    const uint32_t nr = rend - rbeg;\n"
         "    const uint32_t iters = (nr + 63) / 64;\n"
         "    for (uint32_t it = 0; it < iters; it++) {\n"
         "      const uint32_t r = rbeg + it * 64 + lane;\n"
         "      bool live = r < rend;\n";
    jit_f_direct_tests(ph, st, 6, "", false, s);
    s += "      uint64_t m = __ballot(live);\n"
         "      lane_cnt += live ? 1u : 0u;\n"
         "      if (lane == 0 && m) {\n"
         "        const uint64_t pos = row0 + (uint64_t)it * 64;\n"
         "        const uint64_t w0 = pos >> 6;\n"
         "        const uint32_t sh = (uint32_t)(pos & 63);\n"
         "        atomicOr(&bitmap[w0], m << sh);\n"
         "        if (sh && (m >> (64 - sh)))\n"
         "          atomicOr(&bitmap[w0 + 1], m >> (64 - sh));\n"
         "      }\n"
         "    }\n"
         "  }\n";
  }
  s += "  for (int off = 32; off > 0; off >>= 1)\n"
       "    lane_cnt += (uint32_t)__shfl_xor((int)lane_cnt, off, 64);\n"
       "  __syncthreads();\n"
       "  if (lane == 0 && lane_cnt)\n"
       "    atomicAdd(&wsum, (unsigned long long)lane_cnt);\n"
       "  __syncthreads();\n"
       "  if (tid == 0 && wsum)\n"
       "    atomicAdd(&counters[8 + (blockIdx.x & 7)], wsum);\n"
       "}\n";
}

std::string jit_gen_source_filter(const dev_plan_hdr &ph,
                                  const jit_fstrategy &st) {
  std::string s;
  jit_f_prologue(ph, st, s);
  if (st.fstage) {
    jit_f_staged_params(ph, st, s);
    jit_f_staged_kernel(ph, st, s); /* holds jit_f_staged_sweep */
  } else {
    jit_f_direct_kernel(ph, st, s);
  }
  return s;
}

