/*
 * obx_jit_filter.inc — filter-only codegen (obx_gpu_filter): strategy,
 * strategy signature, source (included by obx_jit.inc).
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
 */

struct jit_fstrategy {
  uint8_t leaf_kind[4] = {};  /* 1 = packed range, 2 = dict ref mask,
                                 3 = key set on a packed-range column */
  uint8_t leaf_form[4] = {};  /* kind 3: OBX_KS_* form of the set */
  uint16_t leaf_cols[4] = {};
  uint8_t leaf_multi[4] = {}; /* r entries per packed read */
  uint8_t r = 1;              /* rows per lane (strip mining) */
  uint8_t nslice = 1;         /* direct mode: row slices per block */
  uint8_t fu = 4;             /* direct mode: pipelined tiles */
  uint8_t fstage = 0;         /* LDS-DMA stage the leaf streams */
  uint8_t frid = 0;           /* emit ordered selection vectors */
  uint16_t fnch = 64;         /* chunk capacity for the mask capture */
  uint32_t fseg[4] = {};      /* per-leaf LDS segment bytes (staged mode) */
};

static bool jit_build_fstrategy(const obx_handle &h, const dev_plan_hdr &ph,
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
    uint16_t col = pl[i].col;
    bool mask_ok = pl[i].op != 10 || pl[i].n_bcols == 1;
    if (h.col_dict_any[col] && mask_ok) st.leaf_kind[i] = 2;
    else if (pl[i].op <= 6 && h.col_rangefam_every[col])
      st.leaf_kind[i] = 1;
    else if (pl[i].op == 11 && h.col_rangefam_every[col]) {
      /* every block lowers to SET_BITS / SET_HASH (by the set's form) or
         NONE */
      st.leaf_kind[i] = 3;
      st.leaf_form[i] = obx_leaf_keyset(pl[i]).form;
      has_set = true;
    }
    else return false;
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

static std::string jit_fstrategy_sig(const dev_plan_hdr &ph,
                                     const jit_fstrategy &st) {
  char b[128];
  std::string k = "F|";
  snprintf(b, sizeof b, "s%d|r%d|u%d|g%d:%u:%u:%u:%u|i%d:%u|", st.nslice,
           st.r, st.fu, st.fstage, st.fseg[0], st.fseg[1], st.fseg[2],
           st.fseg[3], st.frid, (unsigned)st.fnch);
  k += b;
  k += "P";
  for (uint32_t p2 = 0; p2 < ph.n_prog; p2++) {
    snprintf(b, sizeof b, "%u.", ph.prog[p2]);
    k += b;
  }
  k += "|";
  for (uint32_t i = 0; i < ph.n_leaves; i++) {
    snprintf(b, sizeof b, "L%d:%u:m%d:k%d|", st.leaf_kind[i], st.leaf_cols[i],
             st.leaf_multi[i], st.leaf_form[i]);
    k += b;
  }
  return k;
}

static std::string jit_gen_source_filter(const dev_plan_hdr &ph,
                                         const jit_fstrategy &st) {
  const int NL = ph.n_leaves;
  char b[1024];
  std::string s;
  s += "#define OBX_PIPELINE 0\n#include \"obx_dev_common.h\"\n"
       "#include \"obx_jit_dev.h\"\n\n";
  snprintf(b, sizeof b,
           "#define NL %d\n#define FSL %d\n#define FR %d\n"
           "#define RID %d\n#define NCH %u\n",
           NL, st.nslice > 0 ? st.nslice : 1, st.r > 0 ? st.r : 1,
           st.frid ? 1 : 0, (unsigned)(st.fnch ? st.fnch : 1));
  s += b;
  /* codegen folds of the postfix combine program (plan data, so the
     kernel gets one closed-form expression) */
  auto fold_prog = [&](const char *item_fmt, bool boolean) {
    char t[96];
    if (ph.n_prog == 0) {
      std::string e = boolean ? "(" : "";
      for (int i2 = 0; i2 < NL; i2++) {
        snprintf(t, sizeof t, item_fmt, i2);
        if (boolean) {
          if (i2) e += " && ";
          e += t;
        } else {
          e = i2 == 0 ? t : ("f3and(" + e + ", " + t + ")");
        }
      }
      if (boolean) e += ")";
      return e;
    }
    std::string stk[16];
    int sp = 0;
    for (uint32_t p2 = 0; p2 < ph.n_prog; p2++) {
      uint8_t tok = ph.prog[p2];
      if (tok < ph.n_leaves) {
        snprintf(t, sizeof t, item_fmt, (int)tok);
        stk[sp++] = t;
      } else {
        std::string b2 = stk[--sp], a2 = stk[sp - 1];
        if (boolean)
          stk[sp - 1] =
              "(" + a2 + (tok == 128 ? " && " : " || ") + b2 + ")";
        else
          stk[sp - 1] = (tok == 128 ? "f3and(" : "f3or(") + a2 + ", " +
                        b2 + ")";
      }
    }
    return stk[0];
  };
  if (st.fstage) {
    /* ---- staged mode: WG per block, leaf streams DMA'd to one LDS
       buffer (the LDS-DMA destination stays uniform + lane-linear) ---- */
    uint32_t off[4] = {}, total = 0;
    for (int i = 0; i < NL; i++) { off[i] = total; total += st.fseg[i]; }
    snprintf(b, sizeof b, "#define SEGSZ %uu\n", total);
    s += b;
    s += "struct blkp {\n"
         "  const uint8_t *bp;\n"
         "  uint64_t row0;\n"
         "  uint32_t blk, rows;\n";
    snprintf(b, sizeof b,
             "  uint32_t W[%d], bit[%d], lo[%d], len[%d];\n"
             "  /* leaf payload in registers: loaded once per block, so\n"
             "     the sweep issues no global load of its own */\n"
             "  unsigned long long lmask[%d];\n"
             "  long long llo[%d], lhi[%d];\n"
             "  uint8_t linv[%d], lall[%d], lnone[%d];\n"
             "  /* key-set leaves: the set's view */\n"
             "  const uint64_t *kw[%d];\n"
             "  uint64_t khi[%d];\n"
             "  uint32_t kshift[%d], kmark[%d];\n"
             "};\n",
             NL, NL, NL, NL, NL, NL, NL, NL, NL, NL, NL, NL, NL, NL);
    s += b;
    s += "__device__ __forceinline__ bool load_params(\n"
         "    const uint8_t *__restrict__ buf,\n"
         "    const dev_block *__restrict__ blocks,\n"
         "    const dev_leaf *__restrict__ plan_leaves,\n"
         "    const blk_leaf *__restrict__ bleaves, uint32_t blk,\n"
         "    blkp &p) {\n"
         "  const dev_block &cur = blocks[blk];\n"
         "  const blk_leaf *bl = bleaves + (size_t)blk * NL;\n";
    for (int i = 0; i < NL; i++) {
      snprintf(b, sizeof b,
               "  const uint8_t c%d = leaf_class(cur, plan_leaves[%d], "
               "bl[%d]);\n",
               i, i, i);
      s += b;
    }
    s += "  if ((" + fold_prog("c%d", false) + ") == 0) return false;\n";
    s += ""
         "  p.blk = blk;\n"
         "  p.rows = cur.row_count;\n"
         "  p.row0 = dev_block_row_start(&cur);\n"
         "  p.bp = buf + cur.block_byte;\n"
         "  const uint64_t blk_bit = cur.block_byte * 8;\n";
    for (int i = 0; i < NL; i++) {
      snprintf(b, sizeof b,
               "  {\n"
               "    const uint32_t o = (uint32_t)(cur.cols[%u].data_bit - "
               "blk_bit);\n"
               "    const uint32_t W = PW(cur.cols[%u]);\n"
               "    const uint32_t lo = (o >> 3) & ~15u;\n"
               "    p.W[%d] = W;\n"
               "    p.lo[%d] = lo;\n"
               "    p.bit[%d] = o - lo * 8;\n"
               "    p.len[%d] = ((((o + p.rows * W + 7) >> 3) - lo) + 15) & "
               "~15u;\n"
               "  }\n",
               (unsigned)st.leaf_cols[i], (unsigned)st.leaf_cols[i], i, i,
               i, i);
      s += b;
    }
    for (int i = 0; i < NL; i++) {
      snprintf(b, sizeof b,
               "  p.lmask[%d] = bl[%d].mask;\n"
               "  p.llo[%d] = bl[%d].lo;\n"
               "  p.lhi[%d] = bl[%d].hi;\n"
               "  p.linv[%d] = bl[%d].invert;\n"
               "  p.lall[%d] = bl[%d].mode == OBX_LEAF_ALL ? 1 : 0;\n"
               "  p.lnone[%d] = bl[%d].mode == OBX_LEAF_NONE ? 1 : 0;\n",
               i, i, i, i, i, i, i, i, i, i, i, i);
      s += b;
      if (st.leaf_kind[i] == 3) {
        snprintf(b, sizeof b,
                 "  {\n"
                 "    const obx_keyset_dev ks = "
                 "obx_leaf_keyset(plan_leaves[%d]);\n"
                 "    p.kw[%d] = ks.words;\n"
                 "    p.khi[%d] = ks.hi;\n"
                 "    p.kshift[%d] = ks.shift;\n"
                 "    p.kmark[%d] = ks.has_marker;\n"
                 "  }\n",
                 i, i, i, i, i);
        s += b;
      }
    }
    s += "  return true;\n"
         "}\n"
         "__device__ __forceinline__ void issue_stage(\n"
         "    const blkp &p, uint8_t *dst, uint32_t tid) {\n";
    for (int i = 0; i < NL; i++) {
      snprintf(b, sizeof b,
               "  for (uint32_t i2 = tid; i2 * 16 < p.len[%d]; i2 += WG)\n"
               "    __builtin_amdgcn_global_load_lds(\n"
               "        (const __attribute__((address_space(1))) uint32_t\n"
               "             *)(p.bp + p.lo[%d] + (size_t)i2 * 16),\n"
               "        (__attribute__((address_space(3))) uint32_t\n"
               "             *)(dst + %uu + (size_t)i2 * 16),\n"
               "        16, 0, 0);\n",
               i, i, off[i]);
      s += b;
    }
    s += "}\n";
    /* key-set leaf i (kind 3) over one packed field: the SET_BITS or
       SET_HASH row test, as `const bool lf<i> = ...` for a combine program
       or as a step of the AND chain */
    auto set_stmt = [&](int i, bool multi, bool as_bool) {
      char t[256];
      if (multi)
        snprintf(t, sizeof t, "((wl%d >> (k * cur.W[%d])) & lmk%d)", i, i, i);
      else
        snprintf(t, sizeof t,
                 "jit_bread(seg + %uu, cur.bit[%d] + r * cur.W[%d], "
                 "cur.W[%d])",
                 off[i], i, i, i);
      const std::string n = std::to_string(i);
      const std::string v = "((" + std::string(t) + " ^ cur.lmask[" + n +
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
      return as_bool ? "          const bool lf" + n + " = " + e + ";\n"
                     : "          if (live)\n            live = " + e + ";\n";
    };
    /* sweep of one staged block (emitted inside the block loop below) */
    std::string sweep;
    sweep += "      {\n";
    for (int i = 0; i < NL; i++) {
      if (st.leaf_kind[i] == 1) {
        snprintf(b, sizeof b,
                 "      const bool l%d_all = cur.lall[%d] != 0;\n", i, i);
        sweep += b;
      }
    }
    const int SR = st.r > 1 ? st.r : 1;
    if (SR > 1) {
      /* strip-mined LDS sweep: one packed ds_read covers SR fields,
         mask assembled via wave-synchronous LDS ORs (as direct mode) */
      for (int i = 0; i < NL; i++)
        if (st.leaf_multi[i]) {
          snprintf(b, sizeof b,
                   "      const uint64_t lmk%d =\n"
                   "          ((uint64_t)1 << cur.W[%d]) - 1;\n",
                   i, i);
          sweep += b;
        }
      sweep +=
          "      const uint32_t rows = cur.rows;\n"
          "      const uint64_t row0 = cur.row0;\n"
          "      const uint32_t tiles = (rows + 64 * FR - 1) / (64 * "
          "FR);\n"
          "      for (uint32_t t = wv; t < tiles; t += WAVES) {\n"
          "        const uint32_t rt = t * 64 * FR + lane * FR;\n"
          "        if (lane < FR) fm[wv][lane] = 0;\n";
      for (int i = 0; i < NL; i++)
        if (st.leaf_multi[i]) {
          snprintf(b, sizeof b,
                   "        uint64_t wl%d = (rt < rows)\n"
                   "            ? jit_bread(seg + %uu, cur.bit[%d] + rt * "
                   "cur.W[%d], FR * cur.W[%d])\n"
                   "            : 0;\n",
                   i, off[i], i, i, i);
          sweep += b;
        }
      sweep += "        uint32_t pm = 0;\n"
               "#pragma unroll\n"
               "        for (uint32_t k = 0; k < FR; k++) {\n"
               "          const uint32_t r = rt + k;\n"
               "          bool live = r < rows;\n";
      if (ph.n_prog) {
        sweep += "          if (live) {\n";
        for (int i = 0; i < NL; i++) {
          if (st.leaf_kind[i] == 3) {
            sweep += set_stmt(i, st.leaf_multi[i] != 0, true);
            continue;
          }
          if (st.leaf_kind[i] == 1) {
            if (st.leaf_multi[i])
              snprintf(b, sizeof b,
                       "          uint64_t v%d = ((wl%d >> (k * cur.W[%d]))"
                       " & lmk%d) ^ cur.lmask[%d];\n"
                       "          const bool lf%d = !cur.lnone[%d] &&\n"
                       "              (l%d_all || (((v%d - cur.llo[%d]) <= "
                       "(cur.lhi[%d] - cur.llo[%d])) != "
                       "(bool)cur.linv[%d]));\n",
                       i, i, i, i, i, i, i, i, i, i, i, i, i);
            else
              snprintf(b, sizeof b,
                       "          uint64_t v%d = jit_bread(seg + %uu, "
                       "cur.bit[%d] + r * cur.W[%d], cur.W[%d]) ^ "
                       "cur.lmask[%d];\n"
                       "          const bool lf%d = !cur.lnone[%d] &&\n"
                       "              (l%d_all || (((v%d - cur.llo[%d]) <= "
                       "(cur.lhi[%d] - cur.llo[%d])) != "
                       "(bool)cur.linv[%d]));\n",
                       i, off[i], i, i, i, i, i, i, i, i, i, i, i, i);
          } else {
            if (st.leaf_multi[i])
              snprintf(b, sizeof b,
                       "          const bool lf%d = (cur.lmask[%d] >>\n"
                       "              (uint32_t)((wl%d >> (k * cur.W[%d])) "
                       "& lmk%d)) & 1;\n",
                       i, i, i, i, i);
            else
              snprintf(b, sizeof b,
                       "          const bool lf%d = (cur.lmask[%d] >>\n"
                       "              (uint32_t)jit_bread(seg + %uu, "
                       "cur.bit[%d] + r * cur.W[%d], cur.W[%d])) & 1;\n",
                       i, i, off[i], i, i, i);
          }
          sweep += b;
        }
        sweep += "          live = " + fold_prog("lf%d", true) + ";\n"
                 "          }\n";
      } else {
      for (int i = 0; i < NL; i++) {
        if (st.leaf_kind[i] == 3) {
          sweep += set_stmt(i, st.leaf_multi[i] != 0, false);
          continue;
        }
        if (st.leaf_kind[i] == 1) {
          if (st.leaf_multi[i])
            snprintf(b, sizeof b,
                     "          if (live && !l%d_all) {\n"
                     "            uint64_t v = ((wl%d >> (k * cur.W[%d])) "
                     "& lmk%d) ^ cur.lmask[%d];\n"
                     "            live = ((v - cur.llo[%d]) <= (cur.lhi[%d] - "
                     "cur.llo[%d])) != (bool)cur.linv[%d];\n"
                     "          }\n",
                     i, i, i, i, i, i, i, i, i);
          else
            snprintf(b, sizeof b,
                     "          if (live && !l%d_all) {\n"
                     "            uint64_t v = jit_bread(seg + %uu, "
                     "cur.bit[%d] + r * cur.W[%d], cur.W[%d]) ^ "
                     "cur.lmask[%d];\n"
                     "            live = ((v - cur.llo[%d]) <= (cur.lhi[%d] - "
                     "cur.llo[%d])) != (bool)cur.linv[%d];\n"
                     "          }\n",
                     i, off[i], i, i, i, i, i, i, i, i);
        } else {
          if (st.leaf_multi[i])
            snprintf(b, sizeof b,
                     "          if (live)\n"
                     "            live = (cur.lmask[%d] >>\n"
                     "                    (uint32_t)((wl%d >> (k * "
                     "cur.W[%d])) & lmk%d)) & 1;\n",
                     i, i, i, i);
          else
            snprintf(b, sizeof b,
                     "          if (live)\n"
                     "            live = (cur.lmask[%d] >>\n"
                     "                    (uint32_t)jit_bread(seg + %uu, "
                     "cur.bit[%d] + r * cur.W[%d], cur.W[%d])) & 1;\n",
                     i, off[i], i, i, i);
        }
        sweep += b;
      }
      }
      snprintf(b, sizeof b,
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
      sweep += b;
    } else {
    sweep += "      const uint32_t rows = cur.rows;\n"
             "      const uint64_t row0 = cur.row0;\n"
             "      const uint32_t n64 = (rows + 63) >> 6;\n"
             "      for (uint32_t it = wv; it < n64; it += WAVES) {\n"
             "        const uint32_t r = it * 64 + lane;\n"
             "        bool live = r < rows;\n";
    if (ph.n_prog) {
      sweep += "        if (live) {\n";
      for (int i = 0; i < NL; i++) {
        if (st.leaf_kind[i] == 3) {
          sweep += set_stmt(i, false, true);
          continue;
        }
        if (st.leaf_kind[i] == 1)
          snprintf(b, sizeof b,
                   "        uint64_t v%d = jit_bread(seg + %uu, cur.bit[%d]"
                   " + r * cur.W[%d], cur.W[%d]) ^ cur.lmask[%d];\n"
                   "        const bool lf%d = !cur.lnone[%d] &&\n"
                   "            (l%d_all || (((v%d - cur.llo[%d]) <= "
                   "(cur.lhi[%d] - cur.llo[%d])) != "
                   "(bool)cur.linv[%d]));\n",
                   i, off[i], i, i, i, i, i, i, i, i, i, i, i, i);
        else
          snprintf(b, sizeof b,
                   "        const bool lf%d = (cur.lmask[%d] >>\n"
                   "            (uint32_t)jit_bread(seg + %uu, cur.bit[%d] "
                   "+ r * cur.W[%d], cur.W[%d])) & 1;\n",
                   i, i, off[i], i, i, i);
        sweep += b;
      }
      sweep += "        live = " + fold_prog("lf%d", true) + ";\n"
               "        }\n";
    } else {
    for (int i = 0; i < NL; i++) {
      if (st.leaf_kind[i] == 3) {
        sweep += set_stmt(i, false, false);
        continue;
      }
      if (st.leaf_kind[i] == 1)
        snprintf(b, sizeof b,
                 "        if (live && !l%d_all) {\n"
                 "          uint64_t v = jit_bread(seg + %uu, cur.bit[%d] + "
                 "r * cur.W[%d], cur.W[%d]) ^ cur.lmask[%d];\n"
                 "          live = ((v - cur.llo[%d]) <= (cur.lhi[%d] - "
                 "cur.llo[%d])) != (bool)cur.linv[%d];\n"
                 "        }\n",
                 i, off[i], i, i, i, i, i, i, i, i);
      else
        snprintf(b, sizeof b,
                 "        if (live)\n"
                 "          live = (cur.lmask[%d] >>\n"
                 "                  (uint32_t)jit_bread(seg + %uu, "
                 "cur.bit[%d] + r * cur.W[%d], cur.W[%d])) & 1;\n",
                 i, off[i], i, i, i);
      sweep += b;
    }
    }
    sweep += "        uint64_t m = __ballot(live);\n"
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
    if (st.frid) {
      sweep +=
          "#if RID\n"
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
    s += sweep;
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
    return s;
  }
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
    snprintf(b, sizeof b,
             "    const blk_leaf lb%d = bl[%d];\n"
             "    const uint32_t l%do =\n"
             "        (uint32_t)(cur.cols[%u].data_bit - blk_bit);\n"
             "    const uint32_t l%dW = PW(cur.cols[%u]);\n",
             i, i, i, (unsigned)st.leaf_cols[i], i,
             (unsigned)st.leaf_cols[i]);
    s += b;
    if (st.leaf_kind[i] == 1) {
      snprintf(b, sizeof b,
               "    const bool l%d_all = lb%d.mode == OBX_LEAF_ALL;\n", i, i);
      s += b;
    }
  }
  const int R = st.r > 1 ? st.r : 1;
  if (R > 1) {
    for (int i = 0; i < NL; i++)
      if (st.leaf_multi[i]) {
        snprintf(b, sizeof b,
                 "    const uint64_t lmk%d = ((uint64_t)1 << l%dW) - 1;\n",
                 i, i);
        s += b;
      }
    const int FU = st.fu > 0 ? st.fu : 1;
    /* tile = 64*FR rows per wave; `emit_pre` issues the tile's packed
       loads, `emit_tile` consumes them — the superiteration emits FU
       pre-blocks before any tile body so each wave keeps FU independent
       HBM fetches in flight (in-order vmcnt retirement pipelines them) */
    auto emit_pre = [&](const std::string &sfx, const std::string &itx) {
      std::string o;
      char bb[512];
      snprintf(bb, sizeof bb,
               "      const uint32_t rt%s = rbeg + (%s) * 64 * FR + lane * "
               "FR;\n",
               sfx.c_str(), itx.c_str());
      o += bb;
      for (int i = 0; i < NL; i++)
        if (st.leaf_multi[i]) {
          snprintf(bb, sizeof bb,
                   "      uint64_t wl%d%s = (rt%s < rend)\n"
                   "          ? jit_bread(bp, l%do + rt%s * l%dW, FR * "
                   "l%dW)\n"
                   "          : 0;\n",
                   i, sfx.c_str(), sfx.c_str(), i, sfx.c_str(), i, i);
          o += bb;
        }
      return o;
    };
    auto emit_tile = [&](const std::string &sfx, const std::string &itx) {
      std::string o;
      char bb[1024];
      o += "      if (lane < FR) fm[wv][lane] = 0;\n"
           "      {\n"
           "      uint32_t pm = 0;\n"
           "#pragma unroll\n"
           "      for (uint32_t k = 0; k < FR; k++) {\n";
      snprintf(bb, sizeof bb,
               "        const uint32_t r = rt%s + k;\n"
               "        bool live = r < rend;\n",
               sfx.c_str());
      o += bb;
      for (int i = 0; i < NL; i++) {
        if (st.leaf_kind[i] == 1) {
          if (st.leaf_multi[i])
            snprintf(bb, sizeof bb,
                     "        if (live && !l%d_all) {\n"
                     "          uint64_t v = ((wl%d%s >> (k * l%dW)) & "
                     "lmk%d) ^ lb%d.mask;\n"
                     "          live = ((v - lb%d.lo) <= (lb%d.hi - "
                     "lb%d.lo)) != (bool)lb%d.invert;\n"
                     "        }\n",
                     i, i, sfx.c_str(), i, i, i, i, i, i, i);
          else
            snprintf(bb, sizeof bb,
                     "        if (live && !l%d_all) {\n"
                     "          uint64_t v = jit_bread(bp, l%do + r * "
                     "l%dW, l%dW) ^ lb%d.mask;\n"
                     "          live = ((v - lb%d.lo) <= (lb%d.hi - "
                     "lb%d.lo)) != (bool)lb%d.invert;\n"
                     "        }\n",
                     i, i, i, i, i, i, i, i, i);
        } else {
          if (st.leaf_multi[i])
            snprintf(bb, sizeof bb,
                     "        if (live)\n"
                     "          live = (lb%d.mask >>\n"
                     "                  (uint32_t)((wl%d%s >> (k * l%dW)) "
                     "& lmk%d)) & 1;\n",
                     i, i, sfx.c_str(), i, i);
          else
            snprintf(bb, sizeof bb,
                     "        if (live)\n"
                     "          live = (lb%d.mask >>\n"
                     "                  (uint32_t)jit_bread(bp, l%do + r "
                     "* l%dW, l%dW)) & 1;\n",
                     i, i, i, i);
        }
        o += bb;
      }
      snprintf(bb, sizeof bb,
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
               R == 4 ? 4 : 5, R == 4 ? 15u : 31u, itx.c_str());
      o += bb;
      return o;
    };
    s += "    const uint32_t nr = rend - rbeg;\n"
         "    const uint32_t iters = (nr + 64 * FR - 1) / (64 * FR);\n"
         "    uint32_t it = 0;\n";
    if (FU > 1) {
      snprintf(b, sizeof b, "    for (; it + %d <= iters; it += %d) {\n",
               FU, FU);
      s += b;
      for (int u = 0; u < FU; u++) {
        char sfx[8], itx[16];
        snprintf(sfx, sizeof sfx, "_%d", u);
        snprintf(itx, sizeof itx, "it + %d", u);
        s += emit_pre(sfx, itx);
      }
      for (int u = 0; u < FU; u++) {
        char sfx[8], itx[16];
        snprintf(sfx, sizeof sfx, "_%d", u);
        snprintf(itx, sizeof itx, "it + %d", u);
        s += emit_tile(sfx, itx);
      }
      s += "    }\n";
    }
    s += "    for (; it < iters; it++) {\n";
    s += emit_pre("", "it");
    s += emit_tile("", "it");
    s += "    }\n"
         "  }\n";
  } else {
  s += "    const uint32_t nr = rend - rbeg;\n"
       "    const uint32_t iters = (nr + 63) / 64;\n"
       "    for (uint32_t it = 0; it < iters; it++) {\n"
       "      const uint32_t r = rbeg + it * 64 + lane;\n"
       "      bool live = r < rend;\n";
  for (int i = 0; i < NL; i++) {
    if (st.leaf_kind[i] == 1) {
      snprintf(b, sizeof b,
               "      if (live && !l%d_all) {\n"
               "        uint64_t v = jit_bread(bp, l%do + r * l%dW, l%dW) ^ "
               "lb%d.mask;\n"
               "        live = ((v - lb%d.lo) <= (lb%d.hi - lb%d.lo)) != "
               "(bool)lb%d.invert;\n"
               "      }\n",
               i, i, i, i, i, i, i, i, i);
    } else {
      snprintf(b, sizeof b,
               "      if (live)\n"
               "        live = (lb%d.mask >>\n"
               "                (uint32_t)jit_bread(bp, l%do + r * l%dW, "
               "l%dW)) & 1;\n",
               i, i, i, i);
    }
    s += b;
  }
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
  return s;
}
