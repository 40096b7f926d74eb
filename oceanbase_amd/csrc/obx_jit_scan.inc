/*
 * obx_jit_scan.inc — second-generation (persistent-accumulator) scan
 * codegen: strategy, strategy signature, source (included by
 * obx_jit_gen.cpp; the strategy struct itself is in obx_jit.h).
 *
 * Defaults, all measured best (profiles/r02_*, profiles/r03_q1_flush.md):
 * R=4 strip mining, 4 accumulator stripes, single-axis joint histogram
 * unless two axes stay under 2 KB, the row count packed into the joint cell
 * where the weight's bounds allow it (profiles/r10_q1_joint_pack.md;
 * OBX_JIT_JPACK=0 keeps the count in a histogram of its own), jcells-sized
 * LDS, striped counter slots,
 * in-workgroup flush reduction, launch grid 8x the resident set
 * (jit_grid_for, obx_jit_gen.cpp — also the grid of the i64 window bound),
 * 32-bit extraction of packed streams with r * width <= 32 (OBX_JIT_M32=0
 * restores the 64-bit reads), one multiply against a combined u32 factor
 * table for a PROD3 term whose operands are proven to fit (OBX_JIT_CTAB=0
 * restores the two-table product), per-block geometry from the packed
 * descriptor (obx_bdesc, obx_dev.h; OBX_JIT_BDESC=0 restores the reads of
 * dev_block). OBX_JIT_R, OBX_JIT_STRIPES, OBX_JIT_WPB and OBX_JIT_JWS=0
 * override the rest; OBX_JIT_SGRID=n caps the launch grid.
 *
 * Per block (profiles/r05_scan_bdesc.md): what the loop reads of a block --
 * its byte offset, length and row count, and per column the stream offset,
 * count, packed width and flags -- is one 128-byte record of an array built
 * once per (handle, ordered column list) by k_pack_bdesc and cached on the
 * handle (bdesc_get, obx_engine.cpp); the lowered leaf tests are read as
 * whole words. The loop head is scalar loads of two cache lines, then the
 * stage DMA, where dev_block cost four dependent round trips over up to
 * six lines. Only a CTX value column that needs a full col_ctx still reads
 * its dev_col; blocks[0] serves the one-time table and key builds and the
 * flush. Loading the record one block ahead, behind the stage DMA, was
 * measured and is not carried: two records live across the sweep spill
 * SGPRs, and it ran slower than loading at the top of the iteration.
 *
 * Experiments that measured neutral or worse are no longer carried here:
 * the scan's overlapped two-phase block loop, the per-workgroup start
 * skew and the forced two-axis fold, and the filter kernel's double
 * buffer, block batching and perf probes. Their measurements are in
 * profiles/r02_q1.md and profiles/r02_filter_jit.md, under the env knob
 * names they had; their code is in git at commit 6ddb15c and before.
 *
 * Round-1 PMC profiling showed the specialized kernel ISSUE-bound: the
 * per-row cost was dominated by the exact-int128 digit-split LDS atomics
 * (4 atomics + guards per aggregate per row) and per-row dict-entry
 * lookups. V2 removes both, using the load-time column summaries (min/max
 * skip index, dict-everywhere flags — obx_table_facts, obx_facts.h):
 *
 *  - i64 window accumulators: when the per-block sum provably fits int64
 *    (max|term| x max_block_rows < 2^62, bounds from the stored min/max),
 *    each aggregate is ONE wrapping 64-bit LDS atomicAdd per row; the
 *    per-block merge widens to the exact int128/256 cells. Bit-exact:
 *    int64 arithmetic is exact below the bound.
 *  - histogram aggregation: SUM/COUNT over a dict-encoded column never
 *    reads the dict per row — it counts (cell, ref) pairs in a u32 LDS
 *    histogram and multiplies counts by entries once per block (the
 *    storage group-by-pushdown design, ObVectorStore::do_group_by /
 *    read_distinct, generalized to value columns).
 *  - per-block value tables: product operands on dict columns read a
 *    per-block LDS table vt[ref] = (one -/+ entry) built once from the
 *    dict (the filter-on-dict trick applied to arithmetic,
 *    ob_dict_decoder.cpp:1481-1561); the null ref slot holds 0, so NULL
 *    operands zero the term with no branch (SUM of 0 == skip).
 *  - whole-block windows (row_count <= 4096 guaranteed by lds_ok): one
 *    merge per block, parallelized over (cell, item) pairs; group keys
 *    come from a per-block LDS key table (one dict walk per block), so
 *    the merges touch no decode helpers.
 *
 * Register discipline (round-1 lesson: plan state in literals, per-block
 * state minimal — scratch spills cost 3-6x): per-column context is a
 * {u32 offset, u32 width, u32 count} trio, not a col_ctx; address math is
 * 32-bit (blocks are <= 17 KB); the only full col_ctx paths left are
 * non-raw8 CTX value columns and generic (non-range-family) filters.
 *
 * Anything outside these bounds falls back to the v1 generator (exact
 * digit-split path) or the precompiled kernels. OBX_JIT_V2=0 forces v1.
 *
 * Layout: jit_build_strategy (the only place that reads the environment;
 * knob -> field list in obx_jit_gen.cpp), jit_strategy_sig, the fragments the
 * phases share (packed read, mask, field, product operand, one copy each),
 * then one function per kernel phase; jit_gen_source_v2 at the end lists
 * them in kernel order.
 */

enum { JV_CTX = 0, JV_REF = 1 };
enum {
  JA_COUNT_STAR = 0, /* from the per-cell count */
  JA_I64 = 1,        /* i64 window accumulator */
  JA_HIST = 2,       /* histogram-weighted (SUM over dict col) */
  JA_HCOUNT = 3,     /* histogram non-null count (COUNT(col), dict col) */
  JA_I64_COUNT = 4,  /* i64 accumulator of !null (COUNT(col), ext col) */
  JA_MM = 5,         /* LDS CAS min/max (CTX value col) */
  JA_HISTMM = 6,     /* min/max over dict entries with live hist counts */
};

/* slot of a schema column in the strategy's descriptor list (it is there:
   jit_build_strategy lists every column the block loop reads) */
static int jit_bd_slot(const jit_strategy &st, uint16_t col) {
  for (uint32_t i = 0; i < st.bd_cols.n; i++)
    if (st.bd_cols.c[i] == col) return (int)i;
  return -1;
}

/* max |value| of a column from the stored bounds; false if unknown */
static bool jit_col_maxabs(const obx_table_facts &h, uint16_t col, uint64_t *out) {
  if (!h.col_known[col]) return false;
  if (h.col_min[col] > h.col_max[col]) { *out = 0; return true; } /* empty */
  uint64_t a = h.col_min[col] == INT64_MIN
                   ? (uint64_t)INT64_MAX + 1
                   : (uint64_t)(h.col_min[col] < 0 ? -h.col_min[col]
                                                   : h.col_min[col]);
  uint64_t b2 = (uint64_t)(h.col_max[col] < 0 ? -h.col_max[col]
                                              : h.col_max[col]);
  *out = a > b2 ? a : b2;
  return true;
}

/* |a|*|b| with saturation at 2^63 */
static uint64_t jit_sat_mul(uint64_t a, uint64_t b2) {
  if (a == 0 || b2 == 0) return 0;
  unsigned __int128 p = (unsigned __int128)a * b2;
  const uint64_t SAT = 1ull << 63;
  return p > SAT ? SAT : (uint64_t)p;
}

static int jit_tab_get(jit_strategy &st, uint8_t vc, uint8_t kind,
                       int64_t one, uint32_t dim) {
  for (int t = 0; t < st.n_tab; t++)
    if (st.tabs[t].vc == vc && st.tabs[t].kind == kind &&
        st.tabs[t].one == one)
      return t;
  if (st.n_tab >= 6) return -1;
  st.tabs[st.n_tab] = {vc, kind, one, dim};
  return st.n_tab++;
}

static int jit_hist_get(jit_strategy &st, uint8_t vc, uint32_t dim) {
  for (int t = 0; t < st.n_hist; t++)
    if (st.hist_vc[t] == vc) return t;
  if (st.n_hist >= 4) return -1;
  st.hist_vc[st.n_hist] = vc;
  st.hist_off[st.n_hist] = st.hist_total;
  st.hist_tab[st.n_hist] = -1;
  st.hist_total += st.jcells * dim;
  return st.n_hist++;
}

/* what building a strategy for one joint-table form answered; want_pack =
   with the row count packed into the joint cell (jit_build_strategy tries
   that first) */
enum { JB_OK = 0, JB_NO_V2 = 1, JB_PACK_REFUSED = 2 };

static int jit_build_strategy_form(const obx_table_facts &h,
                                   const dev_plan_hdr &ph,
                                   const jit_shape &js, const dev_leaf *pl,
                                   bool want_pack, jit_strategy &st) {
  const char *e = getenv("OBX_JIT_V2");
  if (e && e[0] == '0') return JB_NO_V2;
  /* inline filter: every leaf must be a packed-range-family column
     (k_lower_leaves yields only NONE/ALL/RANGE) or a dict-everywhere
     column (REF_MASK/NONE for every op incl. IN and NU/NN); the whole
     AND chain then runs in the sweep — no pass-bitmap phase */
  if (pl && ph.n_leaves >= 1 && ph.n_leaves <= 4) {
    st.leaf_inline = 1;
    for (uint32_t i = 0; i < ph.n_leaves; i++) {
      const uint8_t kind = jit_leaf_kind(h, pl[i]);
      if (kind != JL_RANGE && kind != JL_MASK) { st.leaf_inline = 0; break; }
      st.leaf_kind[i] = kind;
      st.leaf_cols[i] = pl[i].col;
    }
    if (!st.leaf_inline)
      for (uint32_t i = 0; i < 8; i++) st.leaf_kind[i] = 0;
  }
  /* i64 accumulators persist across every block a workgroup scans, so
     their safety bound needs the launch grid, and that needs wpb: the
     largest |term| is collected here and tested once wpb is known (end) */
  uint64_t max_term = 0;
  const uint64_t BOUND = 1ull << 62;

  /* group-cell count: per-cell LDS arrays are sized to the real
     (maxcnt+1) product, not the 16-slot ceiling -- at 16 KB stage
     buffers every KB of shared accumulators costs occupancy */
  {
    uint32_t cells = 1;
    for (uint32_t g2 = 0; g2 < ph.n_group_cols; g2++)
      cells *= h.col_maxcnt[ph.need_cols[ph.group_idx[g2]]] + 1;
    if (cells < 1) cells = 1;
    if (cells > 16) cells = 16;
    st.jcells = cells;
  }

  /* classify value columns (REF = persistent global-dict histograms and
     value tables, so the dict must be byte-identical in every block) */
  for (int j = 0; j < js.n_vc; j++) {
    uint16_t col = js.vcol[j];
    if (h.col_dict_stable[col] && h.col_dict_every[col]) {
      st.vmode[j] = JV_REF;
      st.vdim[j] = h.col_maxcnt[col] + 1; /* + null bucket */
    } else {
      st.vmode[j] = JV_CTX;
      st.vext[j] = h.col_ext_any[col] ? 1 : 0;
      st.vraw8[j] = h.col_raw8_every[col] ? 1 : 0;
    }
  }
  /* persistent group cells need stable group dicts */
  for (uint32_t g2 = 0; g2 < ph.n_group_cols; g2++)
    if (!h.col_dict_stable[ph.need_cols[ph.group_idx[g2]]]) return JB_NO_V2;
  auto maxabs_of = [&](uint8_t need_idx, uint64_t *out) -> bool {
    if (need_idx == 0xFF) return false;
    return jit_col_maxabs(h, ph.need_cols[need_idx], out);
  };

  /* choose per-aggregate strategies (everything must fit or v2 is off) */
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg &g = ph.aggs[a];
    const int ja = js.slot(ph, g.ia), jb = js.slot(ph, g.ib),
              jc = js.slot(ph, g.ic);
    uint64_t ma = 0, mb = 0, mc = 0;
    switch (g.kind) {
      case OBX_AGG_COUNT:
        if (g.ia == 0xFF) { st.astrat[a] = JA_COUNT_STAR; break; }
        if (ja >= 0 && st.vmode[ja] == JV_REF) {
          int hid = jit_hist_get(st, (uint8_t)ja, st.vdim[ja]);
          if (hid < 0) return JB_NO_V2;
          st.astrat[a] = JA_HCOUNT;
          st.ahist[a] = (int8_t)hid;
        } else if (ja >= 0 && !st.vext[ja]) {
          st.astrat[a] = JA_COUNT_STAR; /* never NULL -> row count */
        } else if (ja >= 0) {
          st.astrat[a] = JA_I64_COUNT;
          st.wa64[a] = (int8_t)st.n_w64++;
          st.aval_a[a] = (int8_t)ja;
        } else {
          return JB_NO_V2;
        }
        break;
      case OBX_AGG_SUM:
        if (ja < 0) return JB_NO_V2;
        if (st.vmode[ja] == JV_REF) {
          int hid = jit_hist_get(st, (uint8_t)ja, st.vdim[ja]);
          if (hid < 0) return JB_NO_V2;
          st.astrat[a] = JA_HIST; /* merge multiplies in int128: no bound */
          st.ahist[a] = (int8_t)hid;
        } else {
          if (!maxabs_of(g.ia, &ma)) return JB_NO_V2;
          if (ma > max_term) max_term = ma;
          st.astrat[a] = JA_I64;
          st.wa64[a] = (int8_t)st.n_w64++;
          st.aval_a[a] = (int8_t)ja;
        }
        break;
      case OBX_AGG_SUM_PROD2:
      case OBX_AGG_SUM_PROD3:
      case OBX_AGG_SUM_MUL: {
        if (ja < 0 || jb < 0) return JB_NO_V2;
        if (!maxabs_of(g.ia, &ma) || !maxabs_of(g.ib, &mb)) return JB_NO_V2;
        uint64_t oneb = (uint64_t)(g.one_b < 0 ? -g.one_b : g.one_b);
        uint64_t onec = (uint64_t)(g.one_c < 0 ? -g.one_c : g.one_c);
        uint64_t term;
        if (g.kind == OBX_AGG_SUM_MUL) {
          term = jit_sat_mul(ma, mb);
        } else {
          term = jit_sat_mul(ma, oneb + mb);
          if (g.kind == OBX_AGG_SUM_PROD3) {
            if (jc < 0 || !maxabs_of(g.ic, &mc)) return JB_NO_V2;
            term = jit_sat_mul(term, onec + mc);
          }
        }
        if (term > max_term) max_term = term;
        st.astrat[a] = JA_I64;
        st.wa64[a] = (int8_t)st.n_w64++;
        st.aval_a[a] = (int8_t)ja;
        /* a operand: CTX value, or ident table when the col is dict */
        if (st.vmode[ja] == JV_REF) {
          int t = jit_tab_get(st, (uint8_t)ja, 0, 0, st.vdim[ja]);
          if (t < 0) return JB_NO_V2;
          st.atab_a[a] = (int8_t)t;
        }
        /* b operand */
        if (st.vmode[jb] == JV_REF) {
          uint8_t kind = (g.kind == OBX_AGG_SUM_MUL) ? 0 : 1;
          int t = jit_tab_get(st, (uint8_t)jb, kind,
                              kind ? g.one_b : 0, st.vdim[jb]);
          if (t < 0) return JB_NO_V2;
          st.atab_b[a] = (int8_t)t;
        }
        if (g.kind == OBX_AGG_SUM_PROD3 && st.vmode[jc] == JV_REF) {
          int t = jit_tab_get(st, (uint8_t)jc, 2, g.one_c, st.vdim[jc]);
          if (t < 0) return JB_NO_V2;
          st.atab_c[a] = (int8_t)t;
        }
        break;
      }
      case OBX_AGG_MIN:
      case OBX_AGG_MAX:
        if (ja < 0) return JB_NO_V2;
        if (st.vmode[ja] == JV_REF) {
          /* min/max of a dict column: any live entry bounds it — read it
             off the histogram at flush through the ident table */
          int hid = jit_hist_get(st, (uint8_t)ja, st.vdim[ja]);
          if (hid < 0) return JB_NO_V2;
          st.astrat[a] = JA_HISTMM;
          st.ahist[a] = (int8_t)hid;
          int tt = jit_tab_get(st, (uint8_t)ja, 0, 0, st.vdim[ja]);
          if (tt < 0) return JB_NO_V2;
          st.atab_a[a] = (int8_t)tt;
        } else {
          st.astrat[a] = JA_MM;
          st.amm[a] = (int8_t)st.n_mm++;
          st.aval_a[a] = (int8_t)ja;
        }
        break;
      default:
        return JB_NO_V2;
    }
    if (st.n_w64 > 8 || st.n_mm > 8) return JB_NO_V2;
  }

  /* histogram SUMs read entry weights from an ident table at merge */
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.astrat[a] != JA_HIST) continue;
    int t2 = st.ahist[a];
    if (st.hist_tab[t2] < 0) {
      int tt = jit_tab_get(st, st.hist_vc[t2], 0, 0,
                           st.vdim[st.hist_vc[t2]]);
      if (tt < 0) return JB_NO_V2;
      st.hist_tab[t2] = (int8_t)tt;
    }
  }

  /* weighted joint histogram detection: members are JA_I64 aggregates
     whose weight operand is the same CTX column and whose other operands
     are dict-REF columns spanning at most two axes */
  {
    const char *je = getenv("OBX_JIT_JWS");
    bool allow = !je || je[0] != '0';
    int8_t axes[2] = {-1, -1};
    uint8_t cand[OBX_DEV_MAX_AGGS] = {};
    int n_cand = 0, n_axed = 0;
    int8_t wja = -1;
    bool ok2 = true;
    for (uint32_t a = 0; allow && a < ph.n_aggs; a++) {
      if (st.astrat[a] != JA_I64 || st.aval_a[a] < 0 || st.atab_a[a] >= 0)
        continue;
      const dev_agg &g = ph.aggs[a];
      bool m = false;
      if (g.kind == OBX_AGG_SUM) m = true;
      else if (g.kind == OBX_AGG_SUM_MUL || g.kind == OBX_AGG_SUM_PROD2)
        m = st.atab_b[a] >= 0;
      else if (g.kind == OBX_AGG_SUM_PROD3)
        m = st.atab_b[a] >= 0 && st.atab_c[a] >= 0;
      if (!m) continue;
      if (wja < 0) wja = st.aval_a[a];
      else if (wja != st.aval_a[a]) continue; /* different weight col */
      cand[a] = 1;
      n_cand++;
      int8_t tb[2] = {st.atab_b[a], g.kind == OBX_AGG_SUM_PROD3
                                        ? st.atab_c[a] : (int8_t)-1};
      for (int q = 0; q < 2; q++) {
        if (tb[q] < 0) continue;
        int8_t vc = (int8_t)st.tabs[tb[q]].vc;
        if (axes[0] < 0) axes[0] = vc;
        else if (axes[0] != vc && axes[1] < 0) axes[1] = vc;
        else if (axes[0] != vc && axes[1] != vc) ok2 = false;
      }
      if (tb[0] >= 0 || tb[1] >= 0) n_axed++;
    }
    /* packed row count: the preconditions that do not need the grid (the
       weight is a CTX column here, so vext says whether it can be NULL) */
    if (want_pack) {
      bool pack_ok = allow && ok2 && wja >= 0 && !st.vext[wja];
      if (pack_ok) {
        const uint16_t wc = js.vcol[wja];
        pack_ok = h.col_known[wc] && h.col_min[wc] >= 0 &&
                  h.col_min[wc] <= h.col_max[wc];
      }
      if (!pack_ok) return JB_PACK_REFUSED;
    }
    /* two-axis joint cells cost d0*d1 LDS rows; unless that stays
       trivial (<2 KB) fold to a single axis: members whose factors need
       the second axis keep their i64 window slot, one more LDS add per
       row. Measured on Q1 SF=100 with the row count packed in, where the
       two-axis table (11.5 KB, 5 workgroups per CU against 7) leaves two
       LDS atomics per row against three: 2.38 ms per step against 2.26,
       and the one-axis kernel held to 5 workgroups per CU runs the same
       2.37 -- the occupancy step costs what the shorter row saves and
       more (profiles/r10_q1_joint_pack.md) */
    if (allow && axes[1] >= 0) {
      auto adim = [&](int8_t vc) {
        uint32_t d = st.vdim[vc];
        return d ? d : 1;
      };
      const uint32_t cells0 = st.jcells;
      if ((uint64_t)cells0 * adim(axes[0]) * adim(axes[1]) * 8 > 2048) {
        /* count members per axis, keep the busier one */
        int use[2] = {0, 0};
        for (uint32_t a = 0; a < ph.n_aggs; a++) {
          if (!cand[a]) continue;
          const dev_agg &g = ph.aggs[a];
          int8_t tb2[2] = {st.atab_b[a], g.kind == OBX_AGG_SUM_PROD3
                                             ? st.atab_c[a] : (int8_t)-1};
          bool on[2] = {false, false};
          for (int q = 0; q < 2; q++)
            if (tb2[q] >= 0)
              on[(int8_t)st.tabs[tb2[q]].vc == axes[1] ? 1 : 0] = true;
          if (on[0] && !on[1]) use[0]++;
          if (on[1] && !on[0]) use[1]++;
        }
        int8_t keep = use[1] > use[0] ? axes[1] : axes[0];
        /* drop members needing the other axis */
        n_cand = 0; n_axed = 0;
        for (uint32_t a = 0; a < ph.n_aggs; a++) {
          if (!cand[a]) continue;
          const dev_agg &g = ph.aggs[a];
          int8_t tb2[2] = {st.atab_b[a], g.kind == OBX_AGG_SUM_PROD3
                                             ? st.atab_c[a] : (int8_t)-1};
          bool ok3 = true, axed = false;
          for (int q = 0; q < 2; q++) {
            if (tb2[q] < 0) continue;
            if ((int8_t)st.tabs[tb2[q]].vc != keep) ok3 = false;
            else axed = true;
          }
          if (!ok3) { cand[a] = 0; continue; }
          n_cand++;
          if (axed) n_axed++;
        }
        axes[0] = keep;
        axes[1] = -1;
      }
    }
    if (allow && ok2 && n_cand >= 2 && n_axed >= 1 && axes[0] >= 0) {
      /* the null bucket stays: dict columns encode NULL as ref==count
         WITHOUT the ext flag, so the bucket is reachable even on
         "non-nullable" columns (caught by the null-factor-axis test) */
      auto axis_dim = [&](int8_t vc) -> uint32_t {
        uint32_t d = st.vdim[vc];
        return d ? d : 1;
      };
      uint32_t d0 = axis_dim(axes[0]);
      uint32_t d1 = axes[1] >= 0 ? axis_dim(axes[1]) : 1;
      const uint32_t cells = st.jcells;
      /* LDS for wsum cells; generous cap, rechecked by the budget below */
      if ((uint64_t)cells * d0 * d1 * 8 <= 24u * 1024u) {
        st.jws_on = 1;
        st.jws_ja = wja;
        st.jws_a0 = axes[0];
        st.jws_a1 = axes[1];
        st.jws_d0 = d0;
        st.jws_d1 = d1;
        st.jws_cells = cells;
        for (uint32_t a = 0; a < ph.n_aggs; a++) {
          if (!cand[a]) continue;
          st.jws_member[a] = 1;
          const dev_agg &g = ph.aggs[a];
          int8_t tb2[2] = {st.atab_b[a], g.kind == OBX_AGG_SUM_PROD3
                                             ? st.atab_c[a] : (int8_t)-1};
          for (int q = 0; q < 2; q++) {
            if (tb2[q] < 0) continue;
            if ((int8_t)st.tabs[tb2[q]].vc == st.jws_a0)
              st.jws_f0[a] = tb2[q];
            else
              st.jws_f1[a] = tb2[q];
          }
        }
        /* members no longer need i64 window slots: compact the rest */
        int nn = 0;
        for (uint32_t a = 0; a < ph.n_aggs; a++) {
          if (st.jws_member[a]) { st.wa64[a] = -1; continue; }
          if (st.wa64[a] >= 0) st.wa64[a] = (int8_t)nn++;
        }
        st.n_w64 = nn;
      }
    }
    if (want_pack && !st.jws_on) return JB_PACK_REFUSED;
    if (want_pack) {
      /* a joint-axis column's histogram is a marginal of the packed
         counts: drop it, and point its aggregates at their axis */
      st.jws_pack = 1;
      uint8_t old_vc[4];
      int8_t old_tab[4], remap[4];
      const int old_n = st.n_hist;
      for (int t = 0; t < 4; t++) {
        old_vc[t] = st.hist_vc[t];
        old_tab[t] = st.hist_tab[t];
        remap[t] = -1;
      }
      st.n_hist = 0;
      st.hist_total = 0;
      for (int t = 0; t < old_n; t++) {
        if ((int8_t)old_vc[t] == st.jws_a0 || (int8_t)old_vc[t] == st.jws_a1)
          continue;
        remap[t] = (int8_t)st.n_hist;
        st.hist_vc[st.n_hist] = old_vc[t];
        st.hist_tab[st.n_hist] = old_tab[t];
        st.hist_off[st.n_hist] = st.hist_total;
        st.hist_total += st.jcells * st.vdim[old_vc[t]];
        st.n_hist++;
      }
      for (int t = st.n_hist; t < 4; t++) {
        st.hist_vc[t] = 0;
        st.hist_tab[t] = 0;
        st.hist_off[t] = 0;
      }
      for (uint32_t a = 0; a < ph.n_aggs; a++) {
        const int t = st.ahist[a];
        if (t < 0) continue;
        st.ahist[a] = remap[t];
        if (remap[t] >= 0) continue;
        st.jws_cax[a] = (int8_t)old_vc[t] == st.jws_a0 ? 0 : 1;
        st.jws_ctab[a] =
            st.astrat[a] == JA_HISTMM ? st.atab_a[a] : old_tab[t];
      }
    }
  }

  /* product narrowing (first eligible PROD3 that kept its window slot) */
  {
    const char *ce = getenv("OBX_JIT_CTAB");
    const bool allow = !ce || ce[0] != '0';
    for (uint32_t a = 0; allow && a < ph.n_aggs && st.ctab_agg < 0; a++) {
      const dev_agg &g = ph.aggs[a];
      if (g.kind != OBX_AGG_SUM_PROD3 || st.astrat[a] != JA_I64 ||
          st.jws_member[a] || st.wa64[a] < 0 || st.atab_a[a] >= 0 ||
          st.atab_b[a] < 0 || st.atab_c[a] < 0)
        continue;
      /* the PROD2 head, when it runs per row, shares p2 with this agg */
      if (a > 0 && (js.agg_f2 & (1u << (a - 1))) && !st.jws_member[a - 1])
        continue;
      const uint16_t ca = ph.need_cols[g.ia], cb = ph.need_cols[g.ib],
                     cc = ph.need_cols[g.ic];
      if (!h.col_known[ca] || !h.col_known[cb] || !h.col_known[cc]) continue;
      const bool empty_b = h.col_min[cb] > h.col_max[cb],
                 empty_c = h.col_min[cc] > h.col_max[cc];
      if (h.col_min[ca] > h.col_max[ca] || empty_b || empty_c) continue;
      if (h.col_min[ca] < 0 || h.col_max[ca] > (int64_t)0xffffffffll)
        continue;
      /* factor ranges over every dict entry (the stored bounds of a dict
         column cover its whole dict): one_b - e and one_c + e */
      const __int128 fb_lo = (__int128)g.one_b - h.col_max[cb],
                     fb_hi = (__int128)g.one_b - h.col_min[cb],
                     fc_lo = (__int128)g.one_c + h.col_min[cc],
                     fc_hi = (__int128)g.one_c + h.col_max[cc];
      if (fb_lo < 0 || fc_lo < 0 || fb_hi > 0xffffffffll ||
          fc_hi > 0xffffffffll || fb_hi * fc_hi > 0xffffffffll)
        continue;
      const uint32_t db = st.tabs[st.atab_b[a]].dim,
                     dc = st.tabs[st.atab_c[a]].dim;
      if ((uint64_t)db * dc > 1024) continue;
      st.ctab_agg = (int8_t)a;
      st.ctab_db = db;
      st.ctab_dc = dc;
    }
  }

  /* strip mining: r rows per lane when the filter is inline (or absent);
     a packed stream is read r-entries-at-once when r * max_width <= 64 */
  if (st.leaf_inline || ph.n_leaves == 0) {
    const char *re = getenv("OBX_JIT_R");
    int r = re ? atoi(re) : 4;
    if (r != 1 && r != 2 && r != 4 && r != 8) r = 4;
    st.r = (uint8_t)r;
    if (st.r > 1) {
      const char *ne = getenv("OBX_JIT_M32");
      const uint32_t w32 = (ne && ne[0] == '0') ? 0 : 32;
      for (uint32_t i = 0; i < ph.n_leaves; i++) {
        const uint32_t rw = h.col_maxw[st.leaf_cols[i]] * st.r;
        st.leaf_multi[i] = rw <= 64 ? 1 : 0;
        st.leaf_m32[i] = rw <= w32 ? 1 : 0;
      }
      for (uint32_t g2 = 0; g2 < ph.n_group_cols; g2++) {
        const uint32_t rw =
            h.col_maxw[ph.need_cols[ph.group_idx[g2]]] * st.r;
        st.g_multi[g2] = rw <= 64 ? 1 : 0;
        st.g_m32[g2] = rw <= w32 ? 1 : 0;
      }
      for (int j = 0; j < js.n_vc; j++) {
        const uint32_t rw = h.col_maxw[js.vcol[j]] * st.r;
        st.v_multi[j] = (st.vmode[j] == JV_REF && rw <= 64) ? 1 : 0;
        st.v_m32[j] = (st.vmode[j] == JV_REF && rw <= w32) ? 1 : 0;
      }
    }
  }
  /* any full histogram records every live row (nulls in the clamp
     bucket), so the per-cell count comes from the smallest one at flush */
  for (int t = 0; t < st.n_hist; t++)
    if (st.cnt_hist < 0 ||
        st.vdim[st.hist_vc[t]] < st.vdim[st.hist_vc[st.cnt_hist]])
      st.cnt_hist = (int8_t)t;

  /* the persistent-accumulator kernel has no per-block merge: a filter
     that cannot be inlined falls back to the v1 generator */
  if (ph.n_leaves > 0 && !st.leaf_inline) return JB_NO_V2;

  /* LDS budget: stage buffer (sized to the handle's largest block) +
     persistent shared accumulators */
  {
    const char *se = getenv("OBX_JIT_STRIPES");
    int sn = se ? atoi(se) : 4;
    if (sn != 1 && sn != 2 && sn != 4 && sn != 8 && sn != 16) sn = 4;
    st.stripes = (uint8_t)sn;
  }
  st.stage_bytes = ((h.max_block_len + 24 + 63) / 64) * 64;
  if (st.stage_bytes > OBX_LDS_STAGE_BYTES + 32)
    st.stage_bytes = OBX_LDS_STAGE_BYTES + 32;
  /* the flush reuses the stage buffer for its per-(cell, aggregate)
     partials (16 B each): tiny blocks must not undersize it */
  if (st.stage_bytes < st.jcells * ph.n_aggs * 16)
    st.stage_bytes = ((st.jcells * ph.n_aggs * 16 + 63) / 64) * 64;
  /* (a double-buffered stage was tried and reverted: 2x stage LDS
     halves occupancy, which outweighs the DMA overlap, and the LDS-DMA
     destination must stay uniform+lane-linear) */
  uint32_t lds = st.stage_bytes;
  lds += (uint32_t)st.n_w64 * st.jcells * 8 * st.stripes;
  lds += (uint32_t)st.n_mm * st.jcells * 16; /* wmm val + valid */
  lds += st.hist_total * 4;                      /* histograms */
  for (int t = 0; t < st.n_tab; t++) lds += st.tabs[t].dim * 8;
  if (st.ctab_agg >= 0) lds += st.ctab_db * st.ctab_dc * 4;
  lds += 16 * 8 + 16 * 4;                        /* keytab + cslot */
  if (st.jws_on)
    lds += st.jws_cells * st.jws_d0 * st.jws_d1 * 8; /* joint wsum */
  if (st.cnt_hist < 0 && !st.jws_pack)
    lds += st.jcells * 4 * st.stripes; /* wcnt */
  lds += 64;
  st.lds_bytes = lds;
  st.wpb = (int)(163840 / (lds > 1 ? lds : 1));
  if (st.wpb > 8) st.wpb = 8;
  const char *we = getenv("OBX_JIT_WPB");
  if (we) {
    int w = atoi(we);
    if (w >= 2 && w <= 8 && w < st.wpb) st.wpb = w;
  }
  if (st.wpb < 2) return JB_NO_V2;
  /* i64 window bound over the rows one workgroup sweeps at the launched
     grid (jit_grid_for is what jit_launch uses) */
  {
    const uint32_t grid = jit_grid_for(h.n_blocks, h.n_cus, st.wpb);
    const uint64_t maxrows = jit_wg_rows(h, grid);
    if (jit_sat_mul(max_term, maxrows) >= BOUND) return JB_NO_V2;
    /* packed count, over the same rows: the count takes the C bits of
       maxrows, the weight sum the S = 64 - C below them */
    if (st.jws_pack) {
      uint32_t cbits = 0;
      while (cbits < 64 && (maxrows >> cbits)) cbits++;
      if (cbits < 1 || cbits > 56) return JB_PACK_REFUSED;
      const uint32_t sh = 64 - cbits;
      const unsigned __int128 wsum =
          (unsigned __int128)(uint64_t)h.col_max[js.vcol[st.jws_ja]] * maxrows;
      if (wsum >= ((unsigned __int128)1 << sh)) return JB_PACK_REFUSED;
      st.jws_shift = (uint8_t)sh;
    }
  }
  /* packed descriptor: off when the column list outgrows the record or a
     listed column has a count or width that does not fit its slot */
  {
    const char *be = getenv("OBX_JIT_BDESC");
    bool on = !be || be[0] != '0';
    obx_bdesc_cols bc = {};
    auto add = [&](uint16_t col) {
      for (uint32_t i = 0; i < bc.n; i++)
        if (bc.c[i] == col) return;
      if (bc.n >= OBX_DEV_MAX_NEED || h.col_bdesc_unfit[col]) {
        on = false;
        return;
      }
      bc.c[bc.n++] = col;
    };
    for (uint32_t i = 0; on && i < ph.n_need; i++) add(ph.need_cols[i]);
    for (uint32_t i = 0; on && i < ph.n_leaves; i++) add(st.leaf_cols[i]);
    if (on) {
      st.bdesc = 1;
      st.bd_cols = bc;
    }
  }
  st.ok = true;
  return JB_OK;
}

/* The strategy of a plan: with the row count packed into the joint cells
   where that can be proven, else without. A refused form leaves nothing
   behind: the other is built from scratch, so it is exactly the strategy
   OBX_JIT_JPACK=0 gives directly. */
static bool jit_build_strategy(const obx_table_facts &h, const dev_plan_hdr &ph,
                               const jit_shape &js, const dev_leaf *pl,
                               jit_strategy &st) {
  const char *pe = getenv("OBX_JIT_JPACK");
  bool pack = !pe || pe[0] != '0';
  for (;;) {
    st = jit_strategy();
    const int rc = jit_build_strategy_form(h, ph, js, pl, pack, st);
    if (rc == JB_OK) return true;
    if (rc != JB_PACK_REFUSED || !pack) break;
    pack = false;
  }
  st = jit_strategy();
  return false;
}

/* what obx_gpu_last_joint reports of a strategy */
int jit_joint_form_of(const jit_strategy &st) {
  if (!st.jws_on) return 0;
  if (!st.jws_pack) return 1;
  return st.jws_a1 >= 0 ? 3 : 2;
}

/* every strategy field the generated text reads; per-aggregate entries
   only for the plan's aggregates (the plan signature in front fixes their
   number, so the key stays injective) */
static std::string jit_strategy_sig(const dev_plan_hdr &ph,
                                    const jit_strategy &st) {
  std::string k = "V2|";
  jit_emit(k, "w%dh%dt%dp%dli%dr%dch%ds%du%uc%um%d|", st.n_w64, st.n_hist,
           st.n_tab, st.wpb, st.leaf_inline, st.r, st.cnt_hist, st.stripes,
           st.stage_bytes, st.jcells, st.n_mm);
  for (int i = 0; i < 8; i++)
    jit_emit(k, "m%d%d%d|", st.leaf_multi[i] + 2 * st.leaf_m32[i],
             i < 2 ? st.g_multi[i] + 2 * st.g_m32[i] : 0,
             i < 4 ? st.v_multi[i] + 2 * st.v_m32[i] : 0);
  for (int i = 0; i < 8; i++)
    jit_emit(k, "L%d:%u|", st.leaf_kind[i], st.leaf_cols[i]);
  for (int j = 0; j < 4; j++)
    jit_emit(k, "v%d:%u:%u:%u|", st.vmode[j], st.vdim[j], st.vext[j],
             st.vraw8[j]);
  for (uint32_t a = 0; a < ph.n_aggs; a++)
    jit_emit(k, "a%d:%d:%d:%d:%d:%d:%d:%d|", st.astrat[a], st.wa64[a],
             st.ahist[a], st.atab_b[a], st.atab_c[a], st.atab_a[a],
             st.amm[a], st.aval_a[a]);
  for (int t = 0; t < st.n_tab; t++)
    jit_emit(k, "T%u:%u:%lld:%u|", st.tabs[t].vc, st.tabs[t].kind,
             (long long)st.tabs[t].one, st.tabs[t].dim);
  for (int t = 0; t < st.n_hist; t++)
    jit_emit(k, "H%u:%d:%u|", st.hist_vc[t], st.hist_tab[t], st.hist_off[t]);
  jit_emit(k, "C%d:%u:%u|", st.ctab_agg, st.ctab_db, st.ctab_dc);
  jit_emit(k, "B%d", st.bdesc);
  for (uint32_t i = 0; i < st.bd_cols.n; i++)
    jit_emit(k, ":%u", st.bd_cols.c[i]);
  k += "|";
  if (st.jws_on) {
    jit_emit(k, "J%d:%d:%d:%u:%u:%u|", st.jws_ja, st.jws_a0, st.jws_a1,
             st.jws_d0, st.jws_d1, st.jws_cells);
    for (uint32_t a = 0; a < ph.n_aggs; a++)
      jit_emit(k, "j%d:%d:%d|", st.jws_member[a], st.jws_f0[a],
               st.jws_f1[a]);
    if (st.jws_pack) {
      jit_emit(k, "P%u|", st.jws_shift);
      for (uint32_t a = 0; a < ph.n_aggs; a++)
        jit_emit(k, "p%d:%d|", st.jws_cax[a], st.jws_ctab[a]);
    }
  }
  return k;
}

/* ---- fragments the phases share ---- */

/* the three kinds of packed stream the sweep reads */
static jit_stream jit_v2_leaf_stream(int i) {
  return {jit_fmt("wl%d", i), jit_fmt("l%dW", i), jit_fmt("lm%d", i),
          "bv.base", jit_fmt("l%do", i)};
}
static jit_stream jit_v2_group_stream(int g) {
  return {jit_fmt("wgr%d", g), jit_fmt("gW%d", g), jit_fmt("gm%d", g),
          "bv.base", jit_fmt("go%d", g)};
}
static jit_stream jit_v2_value_stream(int j) {
  return {jit_fmt("wx%d", j), jit_fmt("xW%d", j), jit_fmt("xm%d", j),
          "bv.base", jit_fmt("xo%d", j)};
}

/* per-block field mask of a stream read r entries at once */
static void jit_v2_emit_mask(std::string &s, const jit_stream &sm, bool m32) {
  jit_emit(s,
           m32 ? "    const uint32_t %s = (1u << %s) - 1;\n"
               : "    const uint64_t %s = (1ull << %s) - 1;\n",
           sm.m.c_str(), sm.W.c_str());
}

/* the lane's R packed fields of a stream, in one read */
static void jit_v2_emit_packed_read(std::string &s, const jit_stream &sm,
                                    bool m32, int R) {
  if (m32)
    jit_emit(s,
             "      uint32_t %s = jit_bread32(bv.base, %s + rbase * %s);\n",
             sm.w.c_str(), sm.off.c_str(), sm.W.c_str());
  else
    jit_emit(s,
             "      uint64_t %1$s = jit_bread(bv.base, %2$s + rbase * %3$s, "
             "%4$d * %3$s);\n",
             sm.w.c_str(), sm.off.c_str(), sm.W.c_str(), R);
}

/* row k's dict ref of a stream, clamped to the null bucket */
static void jit_v2_emit_ref(std::string &s, const std::string &name,
                            const std::string &count, const jit_stream &sm,
                            bool packed) {
  jit_emit(s,
           "        uint32_t %1$s = (uint32_t)%2$s;\n"
           "        if (%1$s > %3$s) %1$s = %3$s;\n",
           name.c_str(), sm.field(packed).c_str(), count.c_str());
}

/* per-row text of a product's b or c operand on value slot j: its value
   table's entry when the column is dict-REF (the table holds one -/+ e and
   0 for NULL), else the CTX value with NULL as 0. sign '-' / '+' folds
   `one` in; 0 takes the value as it is. */
static std::string jit_v2_operand(int tab, int j, char sign, int64_t one) {
  if (tab >= 0) return jit_fmt("vt%d[x%d]", tab, j);
  if (!sign) return jit_fmt("(nu%1$d ? 0ll : v%1$d)", j);
  return jit_fmt("(nu%1$d ? 0ll : (%2$lldll %3$c v%1$d))", j, (long long)one,
                 sign);
}

static const char *jit_v2_is_min(const dev_agg &g) {
  return g.kind == OBX_AGG_MIN ? "true" : "false";
}

/* aggregates the flush reduces in the workgroup first (facc), as bit sets */
struct jit_v2_facc {
  uint32_t sum = 0, min = 0, max = 0;
  bool any() const { return (sum | min | max) != 0; }
};
static jit_v2_facc jit_v2_facc_of(const dev_plan_hdr &ph,
                                  const jit_strategy &st) {
  jit_v2_facc f;
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.astrat[a] == JA_HIST || st.astrat[a] == JA_HCOUNT ||
        (st.jws_on && st.jws_member[a]))
      f.sum |= 1u << a;
    else if (st.astrat[a] == JA_HISTMM)
      (ph.aggs[a].kind == OBX_AGG_MIN ? f.min : f.max) |= 1u << a;
  }
  return f;
}

/* ---- kernel phases, in kernel order ---- */

static void jit_v2_prologue(const dev_plan_hdr &ph, const jit_shape &,
                            const jit_strategy &st, std::string &s) {
  s += "#include \"obx_dev_common.h\"\n"
       "#include \"obx_jit_dev.h\"\n\n";
  jit_emit(s,
           "#define NL %d\n#define NG %d\n#define NW64 %d\n"
           "#define NAGGS %u\n#define HTOT %u\n#define NSTRIPE %u\n"
           "#define JSTAGE %u\n#define JC %u\n\n",
           (int)ph.n_leaves, (int)ph.n_group_cols,
           st.n_w64 > 0 ? st.n_w64 : 1, (unsigned)ph.n_aggs,
           st.hist_total > 0 ? st.hist_total : 1, (unsigned)st.stripes,
           (unsigned)st.stage_bytes, st.jcells);
  if (st.bdesc)
    jit_emit(s,
             "#define NBS %u\n"
             "/* what the block loop needs of one block, in registers: the\n"
             "   packed descriptor's header and column slots, and the\n"
             "   block's lowered leaf tests. Wave-uniform, whole words:\n"
             "   scalar loads. */\n"
             "struct jmeta {\n"
             "  uint64_t byte;\n"
             "  uint32_t len, rows;\n"
             "  uint64_t s[NBS];\n"
             "  jit_leafw lf[NL ? NL : 1];\n"
             "};\n"
             "__device__ __forceinline__ void jit_load_meta(\n"
             "    jmeta &m, const obx_bdesc *__restrict__ bdesc,\n"
             "    const blk_leaf *__restrict__ bleaves, uint32_t blk) {\n"
             "  const obx_bdesc &d = bdesc[blk];\n"
             "  m.byte = d.block_byte;\n"
             "  m.len = d.block_len;\n"
             "  m.rows = d.row_count;\n"
             "#pragma unroll\n"
             "  for (uint32_t i = 0; i < NBS; i++) m.s[i] = d.slot[i];\n"
             "#pragma unroll\n"
             "  for (uint32_t i = 0; i < NL; i++)\n"
             "    m.lf[i] = jit_load_leafw(bleaves + (uint64_t)blk * NL + "
             "i);\n"
             "}\n\n",
             st.bd_cols.n);
  jit_emit(s,
           "/* Persistent-accumulator scan (the whole-kernel generalization\n"
           "   of the storage group-by pushdown, ObVectorStore::do_group_by):\n"
           "   the dicts are byte-identical in every micro block (verified\n"
           "   at load), so histograms, value tables and group keys are\n"
           "   global-dict-keyed, live in LDS for the kernel's lifetime,\n"
           "   and merge into the global table exactly once. Per block:\n"
           "   stage to LDS, sweep rows, nothing else. */\n"
           "extern \"C\" __global__ __launch_bounds__(256, %d) void "
           "k_jit_scan(\n"
           "    const uint8_t *__restrict__ buf, const dev_block "
           "*__restrict__ blocks,\n"
           "    uint32_t n_blocks, const dev_leaf *__restrict__ "
           "plan_leaves,\n"
           "    const blk_leaf *__restrict__ bleaves, gslot *__restrict__ "
           "gtable,\n"
           "    unsigned long long *__restrict__ counters,\n"
           "    const obx_bdesc *__restrict__ bdesc) {\n",
           st.wpb);
}

/* LDS declarations and their zeroing */
static void jit_v2_lds(const dev_plan_hdr &ph, const jit_shape &,
                       const jit_strategy &st, std::string &s) {
  /* (the packed joint form declares no window array it has no slot for;
     the other forms keep the one-slot placeholder they always had) */
  const bool has_w64 = st.n_w64 > 0 || !st.jws_pack;
  const bool has_wcnt = st.cnt_hist < 0 && !st.jws_pack;
  s += "  __shared__ __attribute__((aligned(16))) uint8_t "
       "lds_blk[JSTAGE];\n";
  if (has_w64)
    s += "  __shared__ unsigned long long wacc64[NW64][JC][NSTRIPE];\n";
  s += "  __shared__ uint32_t hist[HTOT];\n";
  if (st.n_mm > 0)
    jit_emit(s,
             "  /* CAS min/max cells: [slot][cell][val, valid] */\n"
             "  __shared__ unsigned long long wmm[%d][JC][2];\n",
             st.n_mm);
  s += "  __shared__ uint64_t keytab[16];\n"
       "  __shared__ int cslot[16];\n";
  if (st.jws_on)
    jit_emit(s, "  __shared__ unsigned long long jws[%uu * %uu * %uu];\n",
             st.jws_cells, st.jws_d0, st.jws_d1);
  if (has_wcnt)
    s += "  __shared__ uint32_t wcnt[JC][NSTRIPE];\n";
  for (int t = 0; t < st.n_tab; t++)
    jit_emit(s, "  __shared__ long long vt%d[%u];\n", t, st.tabs[t].dim);
  if (st.ctab_agg >= 0)
    jit_emit(s,
             "  /* combined factor table [xb][xc] of the narrowed PROD3 */\n"
             "  __shared__ uint32_t vtc[%uu * %uu];\n",
             st.ctab_db, st.ctab_dc);
  s += "  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> "
       "6;\n"
       "  uint32_t lane_cnt = 0;\n"
       "  const uint32_t stripe = lane & (NSTRIPE - 1);\n"
       "\n";
  if (has_w64)
    s += "  for (uint32_t i = tid; i < NW64 * JC * NSTRIPE; i += WG)\n"
         "    (&wacc64[0][0][0])[i] = 0;\n";
  /* val slot gets the is_min/is_max sentinel; valid slot 0.  The per-agg
     sentinel depends on kind, so init per (slot,cell). */
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.amm[a] < 0) continue;
    jit_emit(s,
             "  for (uint32_t i = tid; i < JC; i += WG) {\n"
             "    wmm[%1$d][i][0] = (unsigned long long)%2$s;\n"
             "    wmm[%1$d][i][1] = 0;\n"
             "  }\n",
             st.amm[a],
             ph.aggs[a].kind == OBX_AGG_MIN ? "INT64_MAX" : "INT64_MIN");
  }
  s += "  for (uint32_t i = tid; i < HTOT; i += WG) hist[i] = 0;\n";
  if (st.jws_on)
    jit_emit(s,
             "  for (uint32_t i = tid; i < %uu * %uu * %uu; i += WG)\n"
             "    jws[i] = 0;\n",
             st.jws_cells, st.jws_d0, st.jws_d1);
  if (has_wcnt)
    s += "  for (uint32_t i = tid; i < JC * NSTRIPE; i += WG)\n"
         "    (&wcnt[0][0])[i] = 0;\n";
}

/* key of a group cell: column g's part, from its dict entry */
static void jit_v2_emit_key_part(const dev_plan_hdr &ph, int g,
                                 std::string &s) {
  const std::string keep =
      ph.group_len[g] >= 8
          ? "~0ull"
          : jit_fmt("((1ull << (8 * %u)) - 1)", (unsigned)ph.group_len[g]);
  if (g == 0)
    jit_emit(s,
             "    for (uint32_t cell = tid; cell < fcells; cell += WG) {\n"
             "      uint32_t r0 = %s;\n"
             "      uint64_t key = 0;\n"
             "      if (r0 >= gb0->count) key |= 1ull << 56;\n"
             "      else {\n"
             "        int64_t kv = dict_entry(bv0, *gb0, r0);\n"
             "        key |= (uint64_t)kv & %s;\n"
             "      }\n",
             ph.n_group_cols > 1 ? "cell % fdim0" : "cell", keep.c_str());
  else
    jit_emit(s,
             "      uint32_t r1 = cell / fdim0;\n"
             "      if (r1 >= gb1->count) key |= 1ull << 57;\n"
             "      else {\n"
             "        int64_t kv1 = dict_entry(bv0, *gb1, r1);\n"
             "        key |= ((uint64_t)kv1 & %s) << (8 * %u);\n"
             "      }\n",
             keep.c_str(), (unsigned)ph.group_len[0]);
}

/* one-time value tables and key table, from block 0 (dicts are identical) */
static void jit_v2_tables(const dev_plan_hdr &ph, const jit_shape &js,
                          const jit_strategy &st, std::string &s) {
  const int NG = ph.n_group_cols;
  s += "  {\n"
       "    const dev_block &b0 = blocks[0];\n"
       "    blk_view bv0;\n"
       "    bv0.base = buf + b0.block_byte;\n"
       "    bv0.bit_bias = b0.block_byte * 8;\n"
       "    bv0.rbase_bit = 0;\n";
  for (int t = 0; t < st.n_tab; t++) {
    const jit_vtab &vt = st.tabs[t];
    const std::string ex =
        vt.kind == 0 ? "e2"
                     : jit_fmt("%lldll %c e2", (long long)vt.one,
                               vt.kind == 1 ? '-' : '+');
    jit_emit(s,
             "    {\n"
             "      const dev_col *tb = &b0.cols[%u];\n"
             "      for (uint32_t e = tid; e <= tb->count && e < %uu; e += "
             "WG) {\n"
             "        long long v2 = 0;\n"
             "        if (e < tb->count) {\n"
             "          long long e2 = dict_entry(bv0, *tb, e);\n"
             "          v2 = %s;\n"
             "        }\n"
             "        vt%d[e] = v2;\n"
             "      }\n"
             "    }\n",
             (unsigned)js.vcol[vt.vc], vt.dim, ex.c_str(), t);
  }
  if (st.ctab_agg >= 0) {
    const dev_agg &g = ph.aggs[st.ctab_agg];
    jit_emit(s,
             "    {\n"
             "      const dev_col *tb = &b0.cols[%1$u], *tc = &b0.cols[%2$u];\n"
             "      for (uint32_t e = tid; e < %3$uu * %4$uu; e += WG) {\n"
             "        const uint32_t eb = e / %4$uu, ec = e %% %4$uu;\n"
             "        long long fb = 0, fc = 0; /* null slots: factor 0 */\n"
             "        if (eb < tb->count) fb = %5$lldll - dict_entry(bv0, *tb, "
             "eb);\n"
             "        if (ec < tc->count) fc = %6$lldll + dict_entry(bv0, *tc, "
             "ec);\n"
             "        vtc[e] = (uint32_t)(fb * fc);\n"
             "      }\n"
             "    }\n",
             (unsigned)ph.need_cols[g.ib], (unsigned)ph.need_cols[g.ic],
             st.ctab_db, st.ctab_dc, (long long)g.one_b, (long long)g.one_c);
  }
  if (NG > 0) {
    jit_emit(s,
             "    const dev_col *gb0 = &b0.cols[%u];\n"
             "    const uint32_t fdim0 = gb0->count + 1;\n",
             (unsigned)ph.need_cols[ph.group_idx[0]]);
    if (NG > 1)
      jit_emit(s,
               "    const dev_col *gb1 = &b0.cols[%u];\n"
               "    const uint32_t fdim1 = gb1->count + 1;\n"
               "    const uint32_t fcells = fdim0 * fdim1;\n",
               (unsigned)ph.need_cols[ph.group_idx[1]]);
    else
      s += "    const uint32_t fcells = fdim0;\n";
    for (int g = 0; g < NG; g++) jit_v2_emit_key_part(ph, g, s);
    s += "      keytab[cell] = key;\n"
         "    }\n";
  } else {
    s += "    if (tid == 0) keytab[0] = 0;\n";
  }
  s += "  }\n"
       "  __syncthreads();\n"
       "\n";
}

/* Block-loop head when the strategy reads the packed descriptor (st.bdesc):
   verdict, stage and per-block geometry come from a jmeta in registers,
   never from blocks[blk] -- except a CTX value column that needs a full
   col_ctx (not raw8), which reads its dev_col as before. The jmeta is
   loaded at the top of the iteration: scalar loads from two cache lines
   (leaf tests, record), then the stage DMA, where dev_block cost four
   dependent round trips over up to six lines. Loading it one block ahead,
   behind the stage DMA, measured slower and is not carried
   (profiles/r05_scan_bdesc.md). */
static void jit_v2_block_head_bdesc(const dev_plan_hdr &ph,
                                    const jit_shape &js,
                                    const jit_strategy &st, std::string &s) {
  const int NG = ph.n_group_cols;
  const int NL = ph.n_leaves;
  s += "  for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += "
       "gridDim.x) {\n"
       "    jmeta cm;\n"
       "    jit_load_meta(cm, bdesc, bleaves, blk);\n"
       "    uint8_t blk_verdict = 1;\n";
  for (int i = 0; i < NL; i++)
    jit_emit(s,
             "    {\n"
             "      const uint8_t c = jit_leaf_class(\n"
             "          cm.lf[%d], OBX_BD_FLAGS(cm.s[%d]));\n"
             "      if (c == 0) blk_verdict = 0;\n"
             "      else if (c == 2 && blk_verdict) blk_verdict = 2;\n"
             "    }\n",
             i, jit_bd_slot(st, st.leaf_cols[i]));
  s += "    if (blk_verdict == 0) continue;\n"
       "    __syncthreads(); /* drain previous block's LDS reads */\n"
       "    stage2(buf, cm.byte, cm.len, lds_blk);\n"
       "    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n"
       "    __syncthreads();\n"
       "    const uint64_t blk_bit = cm.byte * 8;\n"
       "    blk_view bv;\n"
       "    bv.base = lds_blk;\n"
       "    bv.bit_bias = blk_bit;\n"
       "    bv.rbase_bit = 0;\n"
       "    const uint32_t rows = cm.rows;\n"
       "\n";
  for (int g = 0; g < NG && g < 2; g++)
    jit_emit(s,
             "    const uint32_t go%1$d = OBX_BD_OFF(cm.s[%2$d]);\n"
             "    const uint32_t gW%1$d = OBX_BD_WIDTH(cm.s[%2$d]);\n"
             "    const uint32_t gn%1$d = OBX_BD_COUNT(cm.s[%2$d]);\n",
             g, jit_bd_slot(st, ph.need_cols[ph.group_idx[g]]));
  if (NG > 1) s += "    const uint32_t dim0 = gn0 + 1;\n";
  for (int j = 0; j < js.n_vc; j++) {
    const int k = jit_bd_slot(st, js.vcol[j]);
    if (st.vmode[j] == JV_REF)
      jit_emit(s,
               "    const uint32_t xo%1$d = OBX_BD_OFF(cm.s[%2$d]);\n"
               "    const uint32_t xW%1$d = OBX_BD_WIDTH(cm.s[%2$d]);\n"
               "    const uint32_t xn%1$d = OBX_BD_COUNT(cm.s[%2$d]);\n",
               j, k);
    else if (st.vraw8[j])
      jit_emit(s, "    const uint32_t vb%d = OBX_BD_OFF(cm.s[%d]) >> 3;\n", j,
               k);
    else
      jit_emit(s,
               "    const col_ctx c%d =\n"
               "        make_col_ctx(blocks[blk].cols[%u], blk_bit);\n",
               j, (unsigned)js.vcol[j]);
  }
}

/* block-loop head when the strategy reads dev_block */
static void jit_v2_block_head_blocks(const dev_plan_hdr &ph,
                                     const jit_shape &js,
                                     const jit_strategy &st, std::string &s) {
  const int NG = ph.n_group_cols;
  s += "  for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += "
       "gridDim.x) {\n"
       "    const dev_block &cur = blocks[blk];\n"
       "    const blk_leaf *bl = bleaves + (uint64_t)blk * (NL ? NL : "
       "1);\n"
       "    uint8_t blk_verdict = 1;\n"
       "    for (uint32_t i = 0; i < NL; i++) {\n"
       "      uint8_t c = leaf_class(cur, plan_leaves[i], bl[i]);\n"
       "      if (c == 0) { blk_verdict = 0; break; }\n"
       "      if (c == 2) blk_verdict = 2;\n"
       "    }\n"
       "    if (blk_verdict == 0) continue;\n"
       "    __syncthreads(); /* drain previous block's LDS reads */\n"
       "    stage2(buf, cur, lds_blk);\n"
       "    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n"
       "    __syncthreads();\n"
       "    const uint64_t blk_bit = cur.block_byte * 8;\n"
       "    blk_view bv;\n"
       "    bv.base = lds_blk;\n"
       "    bv.bit_bias = blk_bit;\n"
       "    bv.rbase_bit = 0;\n"
       "    const uint32_t rows = cur.row_count;\n"
       "\n";
  for (int g = 0; g < NG && g < 2; g++) {
    jit_emit(s,
             "    const dev_col *gd%1$d = &cur.cols[%2$u];\n"
             "    const uint32_t go%1$d = (uint32_t)(gd%1$d->data_bit - "
             "blk_bit);\n"
             "    const uint32_t gW%1$d = PW(*gd%1$d);\n"
             "    const uint32_t gn%1$d = gd%1$d->count;\n",
             g, (unsigned)ph.need_cols[ph.group_idx[g]]);
    if (g == 1) s += "    const uint32_t dim0 = gn0 + 1;\n";
  }
  for (int j = 0; j < js.n_vc; j++) {
    const unsigned col = js.vcol[j];
    if (st.vmode[j] == JV_REF)
      jit_emit(s,
               "    const uint32_t xo%1$d =\n"
               "        (uint32_t)(cur.cols[%2$u].data_bit - blk_bit);\n"
               "    const uint32_t xW%1$d = PW(cur.cols[%2$u]);\n"
               "    const uint32_t xn%1$d = cur.cols[%2$u].count;\n",
               j, col);
    else if (st.vraw8[j])
      jit_emit(s,
               "    const uint32_t vb%d =\n"
               "        (uint32_t)((cur.cols[%u].data_bit >> 3) - "
               "cur.block_byte);\n",
               j, col);
    else
      jit_emit(s,
               "    const col_ctx c%d = make_col_ctx(cur.cols[%u], "
               "blk_bit);\n",
               j, col);
  }
}

/* per-block leaf operands, and the field masks of every stream that is
   read r entries at once */
static void jit_v2_leaf_preambles(const dev_plan_hdr &ph, const jit_shape &js,
                                  const jit_strategy &st, std::string &s) {
  const int NG = ph.n_group_cols;
  for (int i = 0; i < (int)ph.n_leaves; i++) {
    if (st.bdesc)
      jit_emit(s,
               "    const blk_leaf lb%1$d = jit_leaf_of(cm.lf[%1$d]);\n"
               "    const uint32_t l%1$do = OBX_BD_OFF(cm.s[%2$d]);\n"
               "    const uint32_t l%1$dW = OBX_BD_WIDTH(cm.s[%2$d]);\n",
               i, jit_bd_slot(st, st.leaf_cols[i]));
    else
      jit_emit(s,
               "    const blk_leaf lb%1$d = bl[%1$d];\n"
               "    const uint32_t l%1$do =\n"
               "        (uint32_t)(cur.cols[%2$u].data_bit - blk_bit);\n"
               "    const uint32_t l%1$dW = PW(cur.cols[%2$u]);\n",
               i, (unsigned)st.leaf_cols[i]);
    if (st.leaf_kind[i] == JL_RANGE)
      jit_emit(s,
               "    const bool l%1$d_all = lb%1$d.mode == OBX_LEAF_ALL;\n", i);
    if (st.r > 1 && st.leaf_multi[i])
      jit_v2_emit_mask(s, jit_v2_leaf_stream(i), st.leaf_m32[i]);
  }
  if (st.r <= 1) return;
  for (int g = 0; g < NG && g < 2; g++)
    if (st.g_multi[g])
      jit_v2_emit_mask(s, jit_v2_group_stream(g), st.g_m32[g]);
  for (int j = 0; j < js.n_vc; j++)
    if (st.v_multi[j])
      jit_v2_emit_mask(s, jit_v2_value_stream(j), st.v_m32[j]);
}

/* accumulate body: what one row adds, inside the sweep's k loop */
static void jit_v2_accumulate(const dev_plan_hdr &ph, const jit_shape &js,
                              const jit_strategy &st, std::string &s) {
  s += "        lane_cnt += live ? 1u : 0u;\n"
       "        if (live) {\n";
  if (st.cnt_hist < 0 && !st.jws_pack)
    s += "          atomicAdd(&wcnt[cell][stripe], 1u);\n";
  for (int t = 0; t < st.n_hist; t++) {
    const int j = st.hist_vc[t];
    jit_emit(s, "          atomicAdd(&hist[%uu + cell * %uu + x%d], 1u);\n",
             st.hist_off[t], st.vdim[j], j);
  }
  if (st.jws_on) {
    /* x is clamped to the null bucket already; when that bucket was
       dropped (non-nullable axis) clamp to the last real entry -- the
       branch is unreachable for checksum-valid refs */
    auto axis = [](int j, uint32_t d) {
      return jit_fmt("(x%1$d < %2$uu ? x%1$d : %3$uu)", j, d, d - 1);
    };
    const std::string idx =
        st.jws_a1 >= 0
            ? jit_fmt("cell * %uu + %s * %uu + %s", st.jws_d0 * st.jws_d1,
                      axis(st.jws_a0, st.jws_d0).c_str(), st.jws_d1,
                      axis(st.jws_a1, st.jws_d1).c_str())
            : jit_fmt("cell * %uu + %s", st.jws_d0,
                      axis(st.jws_a0, st.jws_d0).c_str());
    if (st.jws_pack)
      /* weight and row count in one add (the strategy proved the weight
         sum stays below bit %3$u and the weight is never NULL) */
      jit_emit(s,
               "          atomicAdd(&jws[%2$s],\n"
               "                    (nu%1$d ? 0ull : (unsigned long long)v%1$d) +\n"
               "                        (1ull << %3$u));\n",
               st.jws_ja, idx.c_str(), (unsigned)st.jws_shift);
    else
      jit_emit(s,
               "          if (!nu%1$d)\n"
               "            atomicAdd(&jws[%2$s],\n"
               "                      (unsigned long long)v%1$d);\n",
               st.jws_ja, idx.c_str());
  }
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg &g = ph.aggs[a];
    if (st.jws_member[a]) continue; /* folded into the joint wsum */
    if (st.astrat[a] == JA_I64_COUNT) {
      jit_emit(s,
               "          if (!nu%d)\n"
               "            atomicAdd(&wacc64[%d][cell][stripe], 1ull);\n",
               st.aval_a[a], st.wa64[a]);
      continue;
    }
    if (st.astrat[a] == JA_MM) {
      jit_emit(s,
               "          if (!nu%1$d) {\n"
               "            cas_minmax(&wmm[%2$d][cell][0], v%1$d, %3$s);\n"
               "            wmm[%2$d][cell][1] = 1;\n"
               "          }\n",
               st.aval_a[a], st.amm[a], jit_v2_is_min(g));
      continue;
    }
    if (st.astrat[a] != JA_I64) continue;
    const int ja = st.aval_a[a], jb = js.slot(ph, g.ib),
              jc = js.slot(ph, g.ic);
    const std::string va = st.atab_a[a] >= 0
                               ? jit_fmt("vt%d[x%d]", st.atab_a[a], ja)
                               : jit_fmt("v%d", ja);
    switch (g.kind) {
      case OBX_AGG_SUM:
        jit_emit(s,
                 "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                 "                    (unsigned long long)%s);\n",
                 st.wa64[a], va.c_str());
        break;
      case OBX_AGG_SUM_MUL:
        jit_emit(s,
                 "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                 "                    (unsigned long long)((long long)%s * "
                 "%s));\n",
                 st.wa64[a], va.c_str(),
                 jit_v2_operand(st.atab_b[a], jb, 0, 0).c_str());
        break;
      case OBX_AGG_SUM_PROD2:
        jit_emit(s,
                 "          long long p2_%1$u = (long long)%2$s * %3$s;\n"
                 "          atomicAdd(&wacc64[%4$d][cell][stripe],\n"
                 "                    (unsigned long long)p2_%1$u);\n",
                 a, va.c_str(),
                 jit_v2_operand(st.atab_b[a], jb, '-', g.one_b).c_str(),
                 st.wa64[a]);
        if ((js.agg_f2 & (1u << a)) && !st.jws_member[a + 1]) {
          const dev_agg &g3 = ph.aggs[a + 1];
          jit_emit(s,
                   "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                   "                    (unsigned long long)(p2_%u * "
                   "%s));\n",
                   st.wa64[a + 1], a,
                   jit_v2_operand(st.atab_c[a + 1], js.slot(ph, g3.ic), '+',
                                  g3.one_c)
                       .c_str());
        }
        break;
      case OBX_AGG_SUM_PROD3:
        /* fused into the preceding PROD2's emission — unless that agg
           became a JWS member and skipped its per-row code entirely */
        if (a > 0 && (js.agg_f2 & (1u << (a - 1))) && !st.jws_member[a - 1])
          break;
        if (st.ctab_agg == (int)a) {
          jit_emit(s,
                   "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                   "                    (unsigned long long)(uint32_t)v%d *\n"
                   "                        (unsigned long long)vtc[x%d * %uu "
                   "+ x%d]);\n",
                   st.wa64[a], ja, jb, st.ctab_dc, jc);
          break;
        }
        jit_emit(s,
                 "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                 "                    (unsigned long long)((long long)%s * "
                 "%s * %s));\n",
                 st.wa64[a], va.c_str(),
                 jit_v2_operand(st.atab_b[a], jb, '-', g.one_b).c_str(),
                 jit_v2_operand(st.atab_c[a], jc, '+', g.one_c).c_str());
        break;
    }
  }
  s += "        }\n";
}

/* row sweep (strip-mined; whole WG over the block), to the end of the
   block loop */
static void jit_v2_sweep(const dev_plan_hdr &ph, const jit_shape &js,
                         const jit_strategy &st, std::string &s) {
  const int NG = ph.n_group_cols;
  const int NL = ph.n_leaves;
  const int R = st.r > 0 ? st.r : 1;
  jit_emit(s,
           "    const uint32_t itersR = (rows + WG * %1$d - 1) / (WG * %1$d);\n"
           "    for (uint32_t it = 0; it < itersR; it++) {\n"
           "      const uint32_t rbase = (it * WG + tid) * %1$d;\n",
           R);
  for (int i = 0; i < NL; i++)
    if (st.leaf_multi[i])
      jit_v2_emit_packed_read(s, jit_v2_leaf_stream(i), st.leaf_m32[i], R);
  for (int g = 0; g < NG && g < 2; g++)
    if (st.g_multi[g])
      jit_v2_emit_packed_read(s, jit_v2_group_stream(g), st.g_m32[g], R);
  for (int j = 0; j < js.n_vc; j++)
    if (st.v_multi[j])
      jit_v2_emit_packed_read(s, jit_v2_value_stream(j), st.v_m32[j], R);
  for (int j = 0; j < js.n_vc; j++)
    if (st.vmode[j] == JV_CTX && st.vraw8[j])
      jit_emit(s,
               "      const uint8_t *ep%1$d = bv.base + vb%1$d + (rbase << "
               "3);\n",
               j);
  jit_emit(s,
           "#pragma unroll\n"
           "      for (uint32_t k = 0; k < %du; k++) {\n"
           "        const uint32_t r = rbase + k;\n"
           "        bool live = r < rows;\n",
           R);
  for (int i = 0; i < NL; i++) {
    const jit_leaf_ops lb = {i,
                             jit_fmt("lb%d.mask", i),
                             jit_fmt("lb%d.lo", i),
                             jit_fmt("lb%d.hi", i),
                             jit_fmt("lb%d.invert", i),
                             ""};
    const std::string f = jit_v2_leaf_stream(i).field(st.leaf_multi[i] != 0);
    if (st.leaf_kind[i] == JL_RANGE) jit_emit_range_test(s, 8, lb, f, true);
    else jit_emit_mask_test(s, 8, lb, f, true);
  }
  for (int g = 0; g < NG && g < 2; g++) {
    jit_v2_emit_ref(s, jit_fmt("ref%d", g), jit_fmt("gn%d", g),
                    jit_v2_group_stream(g), st.r > 1 && st.g_multi[g]);
    s += g ? "        cell += ref1 * dim0;\n" : "        uint32_t cell = ref0;\n";
  }
  if (NG == 0) s += "        const uint32_t cell = 0;\n";
  for (int j = 0; j < js.n_vc; j++) {
    if (st.vmode[j] == JV_REF)
      jit_v2_emit_ref(s, jit_fmt("x%d", j), jit_fmt("xn%d", j),
                      jit_v2_value_stream(j), st.v_multi[j] != 0);
    else if (st.vraw8[j])
      jit_emit(s,
               "        int64_t v%1$d = *(const int64_t *)(ep%1$d + (k << "
               "3));\n"
               "        const bool nu%1$d = false;\n"
               "        (void)nu%1$d;\n",
               j);
    else
      jit_emit(s,
               "        bool nu%1$d;\n"
               "        int64_t v%1$d = ctx_value(bv, c%1$d, r, nu%1$d);\n"
               "        (void)nu%1$d;\n",
               j);
  }
  jit_v2_accumulate(ph, js, st, s);
  s += "      }\n"
       "    } /* row sweep */\n"
       "  } /* blocks */\n";
}

/* Hierarchical flush: everything summed over dict refs or joint-cell
   slices (passes 2 and 3) is first reduced inside the workgroup, in exact
   int128 in LDS, so each workgroup sends ONE global accumulate per (cell,
   aggregate) instead of one per ref -- the per-ref form put ~87
   same-address L2 atomics per live cell per workgroup on four slots. The
   partials live in the stage buffer, which is idle by now. */
static void jit_v2_flush_head(const dev_plan_hdr &ph, const jit_shape &,
                              const jit_strategy &st, std::string &s) {
  const int NG = ph.n_group_cols;
  s += "\n"
       "\n"
       "  /* survivor count: wave-reduce, then stripe the global atomic\n"
       "     over 8 slots (same-address atomics serialize at L2) */\n"
       "  for (int off = 32; off > 0; off >>= 1)\n"
       "    lane_cnt += (uint32_t)__shfl_xor((int)lane_cnt, off, 64);\n"
       "  if (lane == 0 && lane_cnt)\n"
       "    atomicAdd(&counters[8 + ((blockIdx.x * WAVES + wv) & 7)],\n"
       "              (unsigned long long)lane_cnt);\n"
       "  __syncthreads(); /* all accumulators final: flush once */\n"
       "\n"
       "  const dev_block &b0 = blocks[0];\n";
  if (NG > 0)
    jit_emit(s, "  const uint32_t fdim0 = b0.cols[%u].count + 1;\n",
             (unsigned)ph.need_cols[ph.group_idx[0]]);
  if (NG > 1)
    jit_emit(s, "  const uint32_t fcells = fdim0 * (b0.cols[%u].count + 1);\n",
             (unsigned)ph.need_cols[ph.group_idx[1]]);
  else
    s += NG == 1 ? "  const uint32_t fcells = fdim0;\n"
                 : "  const uint32_t fcells = 1;\n";
  const jit_v2_facc f = jit_v2_facc_of(ph, st);
  if (f.any())
    jit_emit(s,
             "  /* workgroup partials [cell][agg]: {lo, hi} of an int128\n"
             "     sum, or {value, valid} of a min/max */\n"
             "  unsigned long long (*facc)[NAGGS][2] =\n"
             "      (unsigned long long (*)[NAGGS][2])lds_blk;\n"
             "  for (uint32_t i = tid; i < JC * NAGGS; i += WG) {\n"
             "    const uint32_t a = i %% NAGGS;\n"
             "    facc[i / NAGGS][a][0] =\n"
             "        ((0x%xu >> a) & 1)   ? (unsigned long long)INT64_MAX\n"
             "        : ((0x%xu >> a) & 1) ? (unsigned long long)INT64_MIN\n"
             "                             : 0ull;\n"
             "    facc[i / NAGGS][a][1] = 0;\n"
             "  }\n",
             f.min, f.max);
}

/* flush pass 1: per-cell counts, keys -> global slots, and everything
   that is one value per cell (COUNT(*), i64 windows, CAS min/max) */
static void jit_v2_flush_cells(const dev_plan_hdr &ph, const jit_shape &,
                               const jit_strategy &st, std::string &s) {
  s += "  /* flush pass 1: per-cell counts, keys -> global slots */\n"
       "  for (uint32_t cell = tid; cell < fcells; cell += WG) {\n"
       "    int ce = -1;\n";
  if (st.cnt_hist >= 0) {
    const int j = st.hist_vc[st.cnt_hist];
    jit_emit(s,
             "    unsigned long long cnt2 = 0;\n"
             "    for (uint32_t ref = 0; ref < %1$uu; ref++)\n"
             "      cnt2 += hist[%2$uu + cell * %1$uu + ref];\n",
             st.vdim[j], st.hist_off[st.cnt_hist]);
  } else if (st.jws_pack) {
    /* every live row is in exactly one joint cell of its group cell */
    jit_emit(s,
             "    unsigned long long cnt2 = 0;\n"
             "    for (uint32_t j2 = 0; j2 < %1$uu; j2++)\n"
             "      cnt2 += jws[cell * %1$uu + j2] >> %2$u;\n",
             st.jws_d0 * st.jws_d1, (unsigned)st.jws_shift);
  } else {
    s += "    unsigned long long cnt2 = 0;\n"
         "    for (uint32_t s2 = 0; s2 < NSTRIPE; s2++)\n"
         "      cnt2 += wcnt[cell][s2];\n";
  }
  s += "    if (cnt2) {\n"
       "      int gi = jit_gslot(gtable, keytab[cell]);\n"
       "      if (gi >= 0) {\n"
       "        atomicAdd(&gtable[gi].count, cnt2);\n"
       "        ce = gi;\n";
  for (uint32_t a = 0; a < ph.n_aggs; a++)
    if (st.astrat[a] == JA_COUNT_STAR)
      jit_emit(s, "        g_acc_i128(gtable[gi].cells[%u], cnt2, 0);\n",
               (unsigned)a);
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.wa64[a] < 0) continue;
    jit_emit(s,
             "        {\n"
             "          unsigned long long t64 = 0;\n"
             "          for (uint32_t s2 = 0; s2 < NSTRIPE; s2++)\n"
             "            t64 += wacc64[%d][cell][s2];\n"
             "          int64_t v64 = (int64_t)t64;\n"
             "          if (v64)\n"
             "            g_acc_i128(gtable[gi].cells[%u], (uint64_t)v64,\n"
             "                       (uint64_t)(v64 >> 63));\n"
             "        }\n",
             st.wa64[a], (unsigned)a);
  }
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.amm[a] < 0) continue;
    jit_emit(s,
             "        if (wmm[%1$d][cell][1]) {\n"
             "          cas_minmax(&gtable[gi].cells[%2$u][0],\n"
             "                     (int64_t)wmm[%1$d][cell][0], %3$s);\n"
             "          gtable[gi].cells[%2$u][1] = 1;\n"
             "        }\n",
             st.amm[a], (unsigned)a, jit_v2_is_min(ph.aggs[a]));
  }
  s += "      } else {\n"
       "        atomicAdd(&counters[1], cnt2);\n"
       "      }\n"
       "    }\n"
       "    cslot[cell] = ce;\n"
       "  }\n"
       "  __syncthreads();\n";
}

/* flush pass 2: histogram-weighted aggregates over (cell, ref) */
static void jit_v2_flush_hists(const dev_plan_hdr &ph, const jit_shape &js,
                               const jit_strategy &st, std::string &s) {
  s += "  /* flush pass 2: histogram-weighted aggregates over (cell, ref) "
       "*/\n";
  for (int t = 0; t < st.n_hist; t++) {
    const int j = st.hist_vc[t];
    bool any = false, need_entry = false;
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      if (st.ahist[a] != t) continue;
      if (st.astrat[a] == JA_HIST || st.astrat[a] == JA_HCOUNT ||
          st.astrat[a] == JA_HISTMM)
        any = true;
      if (st.astrat[a] == JA_HIST) need_entry = true;
    }
    if (!any) continue;
    jit_emit(s,
             "  {\n"
             "    const uint32_t hcnt = b0.cols[%1$u].count;\n"
             "    for (uint32_t idx = tid; idx < fcells * %2$uu; idx += WG) "
             "{\n"
             "      uint32_t cell = idx / %2$uu, ref = idx %% %2$uu;\n"
             "      int ce = cslot[cell];\n"
             "      if (ce < 0 || ref >= hcnt) continue; /* excl. null "
             "bucket */\n"
             "      uint32_t c2 = hist[%3$uu + cell * %2$uu + ref];\n"
             "      if (!c2) continue;\n",
             (unsigned)js.vcol[j], st.vdim[j], st.hist_off[t]);
    if (need_entry)
      jit_emit(s, "      long long ev = vt%d[ref];\n", st.hist_tab[t]);
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      if (st.ahist[a] != t) continue;
      if (st.astrat[a] == JA_HIST)
        jit_emit(s,
                 "      {\n"
                 "        __int128 p = (__int128)ev * (long long)c2;\n"
                 "        i128v pv = {(uint64_t)p,\n"
                 "                    (uint64_t)((unsigned __int128)p >> "
                 "64)};\n"
                 "        lds_acc_i128(facc[cell][%u], pv);\n"
                 "      }\n",
                 (unsigned)a);
      else if (st.astrat[a] == JA_HISTMM) /* any live entry bounds it */
        jit_emit(s,
                 "      {\n"
                 "        cas_minmax(&facc[cell][%1$u][0],\n"
                 "                   (int64_t)vt%2$d[ref], %3$s);\n"
                 "        facc[cell][%1$u][1] = 1;\n"
                 "      }\n",
                 (unsigned)a, st.atab_a[a], jit_v2_is_min(ph.aggs[a]));
      else /* JA_HCOUNT */
        jit_emit(s,
                 "      atomicAdd(&facc[cell][%u][0], (unsigned long "
                 "long)c2);\n",
                 (unsigned)a);
    }
    s += "    }\n"
         "  }\n";
  }
}

/* an exact int128 product or sum into a workgroup partial */
static void jit_v2_emit_facc_i128(std::string &s, int pad,
                                  const std::string &expr, uint32_t a) {
  const std::string in(pad, ' ');
  jit_emit(s,
           "%1$s{\n"
           "%1$s  __int128 p = %2$s;\n"
           "%1$s  if (p != 0) {\n"
           "%1$s    i128v pv = {(uint64_t)p,\n"
           "%1$s                (uint64_t)((unsigned __int128)p >> 64)};\n"
           "%1$s    lds_acc_i128(facc[cell][%3$u], pv);\n"
           "%1$s  }\n"
           "%1$s}\n",
           in.c_str(), expr.c_str(), (unsigned)a);
}

/* what the two forms of flush pass 3 share: the distinct axis-1 factor
   tables among the members (each gets an s_c<tab> sum over the d1 ring),
   and the members' products of a (cell, d0) slice into the partials */
static int jit_v2_joint_ctabs(const dev_plan_hdr &ph, const jit_strategy &st,
                              int *c_tabs) {
  int n_ct = 0;
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (!st.jws_member[a] || st.jws_f1[a] < 0) continue;
    bool seen = false;
    for (int q = 0; q < n_ct; q++) seen |= c_tabs[q] == st.jws_f1[a];
    if (!seen) c_tabs[n_ct++] = st.jws_f1[a];
  }
  return n_ct;
}

static void jit_v2_emit_joint_members(const dev_plan_hdr &ph,
                                      const jit_strategy &st,
                                      std::string &s) {
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (!st.jws_member[a]) continue;
    const int f0 = st.jws_f0[a], f1 = st.jws_f1[a];
    const std::string sum = f1 >= 0 ? jit_fmt("s_c%d", f1) : "s_pl";
    jit_v2_emit_facc_i128(
        s, 6,
        f0 >= 0   ? jit_fmt("(__int128)vt%d[d0] * %s", f0, sum.c_str())
        : f1 >= 0 ? sum
                  : "(__int128)s_pl",
        a);
  }
}

/* flush pass 3 when the joint cells carry the row count (st.jws_pack): a
   cell splits into its weight sum (low jws_shift bits) and its count. The
   members take the weights as in the plain form; the aggregates of a
   joint-axis column (jws_cax) take the counts along their axis, the null
   bucket excluded as in pass 2. */
static void jit_v2_flush_joint_packed(const dev_plan_hdr &ph,
                                      const jit_shape &js,
                                      const jit_strategy &st,
                                      std::string &s) {
  bool ax[2] = {false, false};
  for (uint32_t a = 0; a < ph.n_aggs; a++)
    if (st.jws_cax[a] >= 0) ax[st.jws_cax[a]] = true;
  s += "  {\n";
  if (ax[0])
    jit_emit(s, "    const uint32_t hc0 = b0.cols[%u].count;\n",
             (unsigned)js.vcol[st.jws_a0]);
  if (ax[1])
    jit_emit(s, "    const uint32_t hc1 = b0.cols[%u].count;\n",
             (unsigned)js.vcol[st.jws_a1]);
  jit_emit(s,
           "    for (uint32_t idx = tid; idx < fcells * %1$uu; idx += WG) {\n"
           "      uint32_t cell = idx / %1$uu, d0 = idx %% %1$uu;\n"
           "      int ce = cslot[cell];\n"
           "      if (ce < 0) continue;\n"
           "      long long s_pl = 0;\n"
           "      unsigned long long n_pl = 0;\n",
           st.jws_d0);
  int c_tabs[OBX_DEV_MAX_AGGS];
  const int n_ct = jit_v2_joint_ctabs(ph, st, c_tabs);
  for (int q = 0; q < n_ct; q++)
    jit_emit(s, "      __int128 s_c%d = 0;\n", c_tabs[q]);
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.jws_cax[a] != 1) continue;
    if (st.astrat[a] == JA_HIST)
      jit_emit(s, "      __int128 h1_%u = 0;\n", (unsigned)a);
    else if (st.astrat[a] == JA_HCOUNT)
      jit_emit(s, "      unsigned long long h1_%u = 0;\n", (unsigned)a);
  }
  jit_emit(s,
           "      for (uint32_t d1 = 0; d1 < %1$uu; d1++) {\n"
           "        const unsigned long long jc =\n"
           "            jws[cell * %2$uu + d0 * %1$uu + d1];\n"
           "        if (!jc) continue;\n"
           "        const long long w = (long long)(jc & ((1ull << %3$u) - 1));\n"
           "        const unsigned long long c = jc >> %3$u;\n"
           "        s_pl += w;\n"
           "        n_pl += c;\n",
           st.jws_d1, st.jws_d0 * st.jws_d1, (unsigned)st.jws_shift);
  for (int q = 0; q < n_ct; q++)
    jit_emit(s, "        s_c%1$d += (__int128)vt%1$d[d1] * w;\n", c_tabs[q]);
  if (ax[1]) {
    s += "        if (d1 < hc1) { /* excl. null bucket */\n";
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      if (st.jws_cax[a] != 1) continue;
      if (st.astrat[a] == JA_HIST)
        jit_emit(s, "          h1_%u += (__int128)vt%d[d1] * (long long)c;\n",
                 (unsigned)a, st.jws_ctab[a]);
      else if (st.astrat[a] == JA_HCOUNT)
        jit_emit(s, "          h1_%u += c;\n", (unsigned)a);
      else /* JA_HISTMM: any live entry bounds it */
        jit_emit(s,
                 "          cas_minmax(&facc[cell][%1$u][0],\n"
                 "                     (int64_t)vt%2$d[d1], %3$s);\n"
                 "          facc[cell][%1$u][1] = 1;\n",
                 (unsigned)a, st.jws_ctab[a], jit_v2_is_min(ph.aggs[a]));
    }
    s += "        }\n";
  }
  s += "      }\n"
       "      if (!n_pl) continue;\n";
  jit_v2_emit_joint_members(ph, st, s);
  if (ax[0]) {
    s += "      if (d0 < hc0) { /* excl. null bucket */\n";
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      if (st.jws_cax[a] != 0) continue;
      if (st.astrat[a] == JA_HIST)
        jit_v2_emit_facc_i128(
            s, 8,
            jit_fmt("(__int128)vt%d[d0] * (long long)n_pl", st.jws_ctab[a]),
            a);
      else if (st.astrat[a] == JA_HCOUNT)
        jit_emit(s, "        atomicAdd(&facc[cell][%u][0], n_pl);\n",
                 (unsigned)a);
      else
        jit_emit(s,
                 "        cas_minmax(&facc[cell][%1$u][0],\n"
                 "                   (int64_t)vt%2$d[d0], %3$s);\n"
                 "        facc[cell][%1$u][1] = 1;\n",
                 (unsigned)a, st.jws_ctab[a], jit_v2_is_min(ph.aggs[a]));
    }
    s += "      }\n";
  }
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.jws_cax[a] != 1) continue;
    if (st.astrat[a] == JA_HIST)
      jit_v2_emit_facc_i128(s, 6, jit_fmt("h1_%u", (unsigned)a), a);
    else if (st.astrat[a] == JA_HCOUNT)
      jit_emit(s,
               "      if (h1_%1$u) atomicAdd(&facc[cell][%1$u][0], h1_%1$u);\n",
               (unsigned)a);
  }
  s += "    }\n"
       "  }\n";
}

/* flush pass 3: joint weighted cells -> member aggregates. One (cell, d0)
   slice per thread; the d1 ring is reduced in registers, factor products
   applied in int128 (exact: the per-cell i64 bound is enforced at strategy
   build). */
static void jit_v2_flush_joint(const dev_plan_hdr &ph, const jit_shape &js,
                               const jit_strategy &st, std::string &s) {
  if (!st.jws_on) return;
  if (st.jws_pack) {
    jit_v2_flush_joint_packed(ph, js, st, s);
    return;
  }
  jit_emit(s,
           "  for (uint32_t idx = tid; idx < fcells * %1$uu; idx += WG) "
           "{\n"
           "    uint32_t cell = idx / %1$uu, d0 = idx %% %1$uu;\n"
           "    int ce = cslot[cell];\n"
           "    if (ce < 0) continue;\n"
           "    long long s_pl = 0;\n",
           st.jws_d0);
  int c_tabs[OBX_DEV_MAX_AGGS];
  const int n_ct = jit_v2_joint_ctabs(ph, st, c_tabs);
  for (int q = 0; q < n_ct; q++)
    jit_emit(s, "    __int128 s_c%d = 0;\n", c_tabs[q]);
  jit_emit(s,
           "    for (uint32_t d1 = 0; d1 < %1$uu; d1++) {\n"
           "      long long w = (long long)jws[cell * %2$uu + d0 * %1$uu + "
           "d1];\n"
           "      if (!w) continue;\n"
           "      s_pl += w;\n",
           st.jws_d1, st.jws_d0 * st.jws_d1);
  for (int q = 0; q < n_ct; q++)
    jit_emit(s, "      s_c%1$d += (__int128)vt%1$d[d1] * w;\n", c_tabs[q]);
  s += "    }\n"
       "    if (s_pl";
  for (int q = 0; q < n_ct; q++) jit_emit(s, " || s_c%d != 0", c_tabs[q]);
  s += ") {\n";
  jit_v2_emit_joint_members(ph, st, s);
  s += "    }\n"
       "  }\n";
}

/* flush pass 4: the workgroup partials -> global cells */
static void jit_v2_flush_partials(const dev_plan_hdr &ph, const jit_shape &,
                                  const jit_strategy &st, std::string &s) {
  const jit_v2_facc f = jit_v2_facc_of(ph, st);
  if (f.any())
    jit_emit(s,
             "  __syncthreads();\n"
             "  /* flush pass 4: one global accumulate per (cell, aggregate) "
             "*/\n"
             "  for (uint32_t idx = tid; idx < fcells * NAGGS; idx += WG) {\n"
             "    const uint32_t cell = idx / NAGGS, a = idx %% NAGGS;\n"
             "    const int ce = cslot[cell];\n"
             "    if (ce < 0) continue;\n"
             "    const unsigned long long lo = facc[cell][a][0],\n"
             "                             hi = facc[cell][a][1];\n"
             "    if ((0x%xu >> a) & 1) {\n"
             "      if (lo | hi) g_acc_i128(gtable[ce].cells[a], lo, hi);\n"
             "    } else if (((0x%xu >> a) & 1) && hi) {\n"
             "      cas_minmax(&gtable[ce].cells[a][0], (int64_t)lo,\n"
             "                 (0x%xu >> a) & 1);\n"
             "      gtable[ce].cells[a][1] = 1;\n"
             "    }\n"
             "  }\n",
             f.sum, f.min | f.max, f.min);
  s += "}\n";
}

static std::string jit_gen_source_v2(const dev_plan_hdr &ph,
                                     const jit_shape &js,
                                     const jit_strategy &st) {
  std::string s;
  jit_v2_prologue(ph, js, st, s);
  jit_v2_lds(ph, js, st, s);
  jit_v2_tables(ph, js, st, s);
  if (st.bdesc) jit_v2_block_head_bdesc(ph, js, st, s);
  else jit_v2_block_head_blocks(ph, js, st, s);
  jit_v2_leaf_preambles(ph, js, st, s);
  jit_v2_sweep(ph, js, st, s); /* holds jit_v2_accumulate */
  jit_v2_flush_head(ph, js, st, s);
  jit_v2_flush_cells(ph, js, st, s);    /* pass 1 */
  jit_v2_flush_hists(ph, js, st, s);    /* pass 2 */
  jit_v2_flush_joint(ph, js, st, s);    /* pass 3 */
  jit_v2_flush_partials(ph, js, st, s); /* pass 4 */
  return s;
}

