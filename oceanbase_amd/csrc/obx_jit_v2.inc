/*
 * obx_jit_v2.inc — second-generation hipRTC query codegen (included by
 * obx_jit.inc).
 *
 * Round-2 note — env knobs and their measured status (profiles/r02_*):
 *   defaults (all measured best):  R=4 strip mining, stripes=4,
 *     single-axis JWS, jcells-sized LDS, striped counter slots,
 *     staged filter (FSTAGE=1) with grid n_blocks/8 in [512,2048].
 *   A/B'd neutral-or-worse, kept env-gated OFF for reproducibility:
 *     OBX_JIT_FDB2 (filter double-buffer: ISA-verified glds span,
 *     measured neutral — strided-stage ceiling), OBX_JIT_FNB (block
 *     batching: LDS vs occupancy), OBX_JIT_SDB (scan 2-phase overlap:
 *     span dies at the sweep's LDS atomics), OBX_JIT_SKEW (convoy
 *     de-phasing: no convoy exists), OBX_JIT_FPROBE (perf probes),
 *     OBX_JIT_JWS=2 (two-axis fold: occupancy step).
 *
 * After round 2 (profiles/r03_q1_flush.md), all measured wins and on by
 * default: the flush reduces per (cell, aggregate) inside the workgroup
 * before any global atomic; the launch grid is 8x the resident set
 * (jit_grid_for, obx_engine.cpp — also the grid of the i64 window bound);
 * packed streams with r * width <= 32 are extracted with 32-bit ops
 * (OBX_JIT_M32=0 restores the 64-bit reads); a PROD3 term whose operands
 * are proven to fit multiplies once against a combined u32 factor table
 * (OBX_JIT_CTAB=0 restores the two-table product).
 *
 * Round-1 PMC profiling showed the specialized kernel ISSUE-bound: the
 * per-row cost was dominated by the exact-int128 digit-split LDS atomics
 * (4 atomics + guards per aggregate per row) and per-row dict-entry
 * lookups. V2 removes both, using the load-time column summaries (min/max
 * skip index, dict-everywhere flags — obx_engine.cpp):
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

struct jit_vtab {          /* per-block LDS value table over dict refs */
  uint8_t vc;              /* value-col slot (js.vcol index) */
  uint8_t kind;            /* 0 ident, 1 (one - e), 2 (one + e) */
  int64_t one;
  uint32_t dim;            /* maxcnt + 1 */
};

struct jit_strategy {
  bool ok = false;
  uint8_t vmode[4] = {};     /* JV_CTX / JV_REF per value col */
  uint8_t vext[4] = {};      /* CTX col can be NULL (ext) in some block */
  uint8_t vraw8[4] = {};     /* CTX col is aligned 8-B RAW in every block */
  uint32_t vdim[4] = {};     /* REF: maxcnt+1 */
  uint8_t astrat[OBX_DEV_MAX_AGGS] = {};
  int8_t wa64[OBX_DEV_MAX_AGGS];    /* JA_I64*: wacc64 slot */
  int8_t amm[OBX_DEV_MAX_AGGS];     /* JA_MM: wmm slot */
  int n_mm = 0;
  int8_t ahist[OBX_DEV_MAX_AGGS];   /* JA_HIST/HCOUNT: hist id */
  int8_t atab_b[OBX_DEV_MAX_AGGS];  /* product b operand: table id or -1 */
  int8_t atab_c[OBX_DEV_MAX_AGGS];  /* product c operand: table id or -1 */
  int8_t aval_a[OBX_DEV_MAX_AGGS];  /* a operand: value-col slot or -1 */
  int8_t atab_a[OBX_DEV_MAX_AGGS];  /* a operand via ident table: id or -1 */
  int n_w64 = 0;
  int n_hist = 0;
  uint8_t hist_vc[4] = {};   /* hist id -> value-col slot */
  int8_t hist_tab[4] = {};   /* hist id -> ident table id (entry weights) */
  uint32_t hist_off[4] = {}; /* u32 offsets into the shared hist array */
  uint32_t hist_total = 0;   /* total u32 slots */
  int n_tab = 0;
  jit_vtab tabs[6];
  uint8_t leaf_inline = 0;   /* ALL leaves inline-evaluable in the sweep */
  uint8_t leaf_kind[8] = {}; /* 1 = packed range, 2 = dict ref mask */
  uint16_t leaf_cols[8] = {};
  uint8_t r = 1;             /* rows per lane (strip mining) */
  uint8_t stripes = 4;       /* i64 accumulator lane stripes */
  uint8_t fu = 4;            /* filter kernel: pipelined tiles */
  uint8_t sdb = 0;           /* scan kernel: overlapped 2-phase stage */
  uint8_t skew = 0;          /* per-WG start skew (us) to break the
                                stage/sweep convoy across co-resident WGs */
  uint8_t fprobe = 0;        /* perf probe: 1 no-flush, 2 loads-only */
  uint8_t fstage = 0;        /* filter: LDS-DMA stage leaf streams */
  uint8_t frid = 0;          /* filter: emit ordered selection vectors */
  uint16_t fnch = 64;        /* chunk capacity for the mask capture */
  uint32_t fseg[4] = {};     /* per-leaf LDS segment bytes (staged mode) */
  uint32_t stage_bytes = OBX_LDS_STAGE_BYTES + 32;
  uint8_t leaf_multi[8] = {}; /* r entries per packed read */
  uint8_t g_multi[2] = {};
  uint8_t v_multi[4] = {};
  /* ... and that read fits 32 bits (r * max_width <= 32): one
     v_alignbit_b32 over two dwords, 32-bit shifts and masks per field */
  uint8_t leaf_m32[8] = {};
  uint8_t g_m32[2] = {};
  uint8_t v_m32[4] = {};
  int8_t cnt_hist = -1;      /* cell counts derived from this hist (drops
                                the per-row wcnt atomic) */
  uint32_t jcells = 16;      /* group-cell rows actually possible */
  /* weighted joint histogram: SUM / SUM_PROD* family sharing one CTX
     weight column with small-dict REF factors collapses to a single
     per-row LDS add into wsum[cell][d0][d1]; the factor products are
     applied at flush (generalizes ObVectorStore::do_group_by's
     count-only dict pushdown to value-weighted cells) */
  uint8_t jws_on = 0;
  int8_t jws_ja = -1;                       /* weight value-col slot */
  int8_t jws_a0 = -1, jws_a1 = -1;          /* axis value-col slots */
  uint32_t jws_d0 = 1, jws_d1 = 1;          /* axis dims */
  uint32_t jws_cells = 16;                  /* group-cell rows */
  uint8_t jws_member[OBX_DEV_MAX_AGGS] = {};
  int8_t jws_f0[OBX_DEV_MAX_AGGS];          /* flush factor tab / axis0 */
  int8_t jws_f1[OBX_DEV_MAX_AGGS];          /* flush factor tab / axis1 */
  /* narrowed PROD3: when the weight is a CTX column proven in [0, 2^32)
     and both dict factors are proven non-negative with a product below
     2^32, the per-row term is ONE u32 x u32 -> u64 multiply against a
     combined LDS table vtc[xb][xc] = (one_b - eb) * (one_c + ec), instead
     of two 64 x 64 multiplies over two table reads */
  int8_t ctab_agg = -1;
  uint32_t ctab_db = 0, ctab_dc = 0;
  uint32_t lds_bytes = 0;
  int wpb = 7;
};

/* max |value| of a column from the stored bounds; false if unknown */
static bool jit_col_maxabs(const obx_handle &h, uint16_t col, uint64_t *out) {
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

static bool jit_build_strategy(const obx_handle &h, const dev_plan_hdr &ph,
                               const jit_shape &js, const dev_leaf *pl,
                               jit_strategy &st) {
  const char *e = getenv("OBX_JIT_V2");
  if (e && e[0] == '0') return false;
  /* inline filter: every leaf must be a packed-range-family column
     (k_lower_leaves yields only NONE/ALL/RANGE) or a dict-everywhere
     column (REF_MASK/NONE for every op incl. IN and NU/NN); the whole
     AND chain then runs in the sweep — no pass-bitmap phase */
  if (pl && ph.n_leaves >= 1 && ph.n_leaves <= 4) {
    st.leaf_inline = 1;
    for (uint32_t i = 0; i < ph.n_leaves; i++) {
      uint16_t col = pl[i].col;
      /* multi-column black programs cannot lower to a ref mask */
      bool mask_ok = pl[i].op != 10 || pl[i].n_bcols == 1;
      if (h.col_dict_any[col] && mask_ok) st.leaf_kind[i] = 2;
      else if (pl[i].op <= 6 && h.col_rangefam_every[col])
        st.leaf_kind[i] = 1;
      else { st.leaf_inline = 0; break; }
      st.leaf_cols[i] = col;
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
    if (!h.col_dict_stable[ph.need_cols[ph.group_idx[g2]]]) return false;
  auto slot_of = [&](uint8_t need_idx) -> int {
    if (need_idx == 0xFF) return -1;
    uint16_t col = ph.need_cols[need_idx];
    for (int j = 0; j < js.n_vc; j++)
      if (js.vcol[j] == col) return j;
    return -1;
  };
  auto maxabs_of = [&](uint8_t need_idx, uint64_t *out) -> bool {
    if (need_idx == 0xFF) return false;
    return jit_col_maxabs(h, ph.need_cols[need_idx], out);
  };

  /* choose per-aggregate strategies (everything must fit or v2 is off) */
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg &g = ph.aggs[a];
    st.wa64[a] = st.ahist[a] = st.atab_b[a] = st.atab_c[a] = -1;
    st.aval_a[a] = st.atab_a[a] = -1;
    st.amm[a] = -1;
    int ja = slot_of(g.ia), jb = slot_of(g.ib), jc = slot_of(g.ic);
    uint64_t ma = 0, mb = 0, mc = 0;
    switch (g.kind) {
      case OBX_AGG_COUNT:
        if (g.ia == 0xFF) { st.astrat[a] = JA_COUNT_STAR; break; }
        if (ja >= 0 && st.vmode[ja] == JV_REF) {
          int hid = jit_hist_get(st, (uint8_t)ja, st.vdim[ja]);
          if (hid < 0) return false;
          st.astrat[a] = JA_HCOUNT;
          st.ahist[a] = (int8_t)hid;
        } else if (ja >= 0 && !st.vext[ja]) {
          st.astrat[a] = JA_COUNT_STAR; /* never NULL -> row count */
        } else if (ja >= 0) {
          st.astrat[a] = JA_I64_COUNT;
          st.wa64[a] = (int8_t)st.n_w64++;
          st.aval_a[a] = (int8_t)ja;
        } else {
          return false;
        }
        break;
      case OBX_AGG_SUM:
        if (ja < 0) return false;
        if (st.vmode[ja] == JV_REF) {
          int hid = jit_hist_get(st, (uint8_t)ja, st.vdim[ja]);
          if (hid < 0) return false;
          st.astrat[a] = JA_HIST; /* merge multiplies in int128: no bound */
          st.ahist[a] = (int8_t)hid;
        } else {
          if (!maxabs_of(g.ia, &ma)) return false;
          if (ma > max_term) max_term = ma;
          st.astrat[a] = JA_I64;
          st.wa64[a] = (int8_t)st.n_w64++;
          st.aval_a[a] = (int8_t)ja;
        }
        break;
      case OBX_AGG_SUM_PROD2:
      case OBX_AGG_SUM_PROD3:
      case OBX_AGG_SUM_MUL: {
        if (ja < 0 || jb < 0) return false;
        if (!maxabs_of(g.ia, &ma) || !maxabs_of(g.ib, &mb)) return false;
        uint64_t oneb = (uint64_t)(g.one_b < 0 ? -g.one_b : g.one_b);
        uint64_t onec = (uint64_t)(g.one_c < 0 ? -g.one_c : g.one_c);
        uint64_t term;
        if (g.kind == OBX_AGG_SUM_MUL) {
          term = jit_sat_mul(ma, mb);
        } else {
          term = jit_sat_mul(ma, oneb + mb);
          if (g.kind == OBX_AGG_SUM_PROD3) {
            if (jc < 0 || !maxabs_of(g.ic, &mc)) return false;
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
          if (t < 0) return false;
          st.atab_a[a] = (int8_t)t;
        }
        /* b operand */
        if (st.vmode[jb] == JV_REF) {
          uint8_t kind = (g.kind == OBX_AGG_SUM_MUL) ? 0 : 1;
          int t = jit_tab_get(st, (uint8_t)jb, kind,
                              kind ? g.one_b : 0, st.vdim[jb]);
          if (t < 0) return false;
          st.atab_b[a] = (int8_t)t;
        }
        if (g.kind == OBX_AGG_SUM_PROD3 && st.vmode[jc] == JV_REF) {
          int t = jit_tab_get(st, (uint8_t)jc, 2, g.one_c, st.vdim[jc]);
          if (t < 0) return false;
          st.atab_c[a] = (int8_t)t;
        }
        break;
      }
      case OBX_AGG_MIN:
      case OBX_AGG_MAX:
        if (ja < 0) return false;
        if (st.vmode[ja] == JV_REF) {
          /* min/max of a dict column: any live entry bounds it — read it
             off the histogram at flush through the ident table */
          int hid = jit_hist_get(st, (uint8_t)ja, st.vdim[ja]);
          if (hid < 0) return false;
          st.astrat[a] = JA_HISTMM;
          st.ahist[a] = (int8_t)hid;
          int tt = jit_tab_get(st, (uint8_t)ja, 0, 0, st.vdim[ja]);
          if (tt < 0) return false;
          st.atab_a[a] = (int8_t)tt;
        } else {
          st.astrat[a] = JA_MM;
          st.amm[a] = (int8_t)st.n_mm++;
          st.aval_a[a] = (int8_t)ja;
        }
        break;
      default:
        return false;
    }
    if (st.n_w64 > 8 || st.n_mm > 8) return false;
  }

  /* histogram SUMs read entry weights from an ident table at merge */
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.astrat[a] != JA_HIST) continue;
    int t2 = st.ahist[a];
    if (st.hist_tab[t2] < 0) {
      int tt = jit_tab_get(st, st.hist_vc[t2], 0, 0,
                           st.vdim[st.hist_vc[t2]]);
      if (tt < 0) return false;
      st.hist_tab[t2] = (int8_t)tt;
    }
  }

  /* weighted joint histogram detection: members are JA_I64 aggregates
     whose weight operand is the same CTX column and whose other operands
     are dict-REF columns spanning at most two axes */
  for (uint32_t a = 0; a < OBX_DEV_MAX_AGGS; a++)
    st.jws_f0[a] = st.jws_f1[a] = -1;
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
    /* two-axis joint cells cost d0*d1 LDS rows; unless that stays
       trivial (<2 KB) a single-axis fold is the better trade: members
       whose factors need the second axis keep their i64 window slot,
       costing one LDS add per row but a whole occupancy step less */
    if (allow && axes[1] >= 0) {
      auto adim = [&](int8_t vc) {
        uint32_t d = st.vdim[vc];
        return d ? d : 1;
      };
      const uint32_t cells0 = st.jcells;
      const char *me = getenv("OBX_JIT_JWS");
      bool force2 = me && me[0] == '2';
      if (!force2 &&
          (uint64_t)cells0 * adim(axes[0]) * adim(axes[1]) * 8 > 2048) {
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
  if (ph.n_leaves > 0 && !st.leaf_inline) return false;

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
  {
    const char *sde = getenv("OBX_JIT_SDB");
    st.sdb = sde && sde[0] == '1' ? 1 : 0;
    const char *ske = getenv("OBX_JIT_SKEW");
    st.skew = ske ? (uint8_t)atoi(ske) : 0;
  }
  uint32_t lds = st.stage_bytes * (st.sdb ? 2 : 1);
  lds += (uint32_t)st.n_w64 * st.jcells * 8 * st.stripes;
  lds += (uint32_t)st.n_mm * st.jcells * 16; /* wmm val + valid */
  lds += st.hist_total * 4;                      /* histograms */
  for (int t = 0; t < st.n_tab; t++) lds += st.tabs[t].dim * 8;
  if (st.ctab_agg >= 0) lds += st.ctab_db * st.ctab_dc * 4;
  lds += 16 * 8 + 16 * 4;                        /* keytab + cslot */
  if (st.jws_on)
    lds += st.jws_cells * st.jws_d0 * st.jws_d1 * 8; /* joint wsum */
  if (st.cnt_hist < 0) lds += st.jcells * 4 * st.stripes; /* wcnt */
  lds += 64;
  st.lds_bytes = lds;
  st.wpb = (int)(163840 / (lds > 1 ? lds : 1));
  if (st.wpb > 8) st.wpb = 8;
  const char *we = getenv("OBX_JIT_WPB");
  if (we) {
    int w = atoi(we);
    if (w >= 2 && w <= 8 && w < st.wpb) st.wpb = w;
  }
  if (st.wpb < 2) return false;
  /* i64 window bound over the rows one workgroup sweeps at the launched
     grid (jit_grid_for is what jit_launch uses) */
  {
    const uint32_t grid = jit_grid_for(h.n_blocks, h.n_cus, st.wpb);
    const uint64_t maxrows =
        (uint64_t)((h.n_blocks + grid - 1) / grid) *
        (h.max_block_rows ? h.max_block_rows : 4096);
    if (jit_sat_mul(max_term, maxrows) >= BOUND) return false;
  }
  st.ok = true;
  return true;
}

static std::string jit_strategy_sig(const jit_strategy &st) {
  char b[256];
  std::string k = "V2|";
  snprintf(b, sizeof b, "w%dh%dt%dp%dli%dr%dch%ds%du%uc%ub%dm%d|",
           st.n_w64, st.n_hist, st.n_tab, st.wpb, st.leaf_inline, st.r,
           st.cnt_hist, st.stripes, st.stage_bytes, st.jcells,
           st.sdb + 10 * st.skew, st.n_mm);
  k += b;
  for (int i = 0; i < 8; i++) {
    snprintf(b, sizeof b, "m%d%d%d|",
             i < 8 ? st.leaf_multi[i] + 2 * st.leaf_m32[i] : 0,
             i < 2 ? st.g_multi[i] + 2 * st.g_m32[i] : 0,
             i < 4 ? st.v_multi[i] + 2 * st.v_m32[i] : 0);
    k += b;
  }
  for (int i = 0; i < 8; i++) {
    snprintf(b, sizeof b, "L%d:%u|", st.leaf_kind[i], st.leaf_cols[i]);
    k += b;
  }
  for (int j = 0; j < 4; j++) {
    snprintf(b, sizeof b, "v%d:%u:%u:%u|", st.vmode[j], st.vdim[j],
             st.vext[j], st.vraw8[j]);
    k += b;
  }
  for (int a = 0; a < OBX_DEV_MAX_AGGS; a++) {
    snprintf(b, sizeof b, "a%d:%d:%d:%d:%d:%d:%d|", st.astrat[a],
             st.wa64[a], st.ahist[a], st.atab_b[a], st.atab_c[a],
             st.atab_a[a], st.amm[a]);
    k += b;
  }
  for (int t = 0; t < st.n_tab; t++) {
    snprintf(b, sizeof b, "T%u:%u:%lld:%u|", st.tabs[t].vc, st.tabs[t].kind,
             (long long)st.tabs[t].one, st.tabs[t].dim);
    k += b;
  }
  snprintf(b, sizeof b, "C%d:%u:%u|", st.ctab_agg, st.ctab_db, st.ctab_dc);
  k += b;
  if (st.jws_on) {
    snprintf(b, sizeof b, "J%d:%d:%d:%u:%u:%u|", st.jws_ja, st.jws_a0,
             st.jws_a1, st.jws_d0, st.jws_d1, st.jws_cells);
    k += b;
    for (uint32_t a = 0; a < OBX_DEV_MAX_AGGS; a++) {
      snprintf(b, sizeof b, "j%d:%d:%d|", st.jws_member[a], st.jws_f0[a],
               st.jws_f1[a]);
      k += b;
    }
  }
  return k;
}

static std::string jit_gen_source_v2(const dev_plan_hdr &ph,
                                     const jit_shape &js,
                                     const jit_strategy &st) {
  const int NG = ph.n_group_cols;
  const int NL = ph.n_leaves;
  char b[1024];
  std::string s;
  s += "#define OBX_PIPELINE 0\n#include \"obx_dev_common.h\"\n\n";
  snprintf(b, sizeof b,
           "#define NL %d\n#define NG %d\n#define NW64 %d\n"
           "#define NAGGS %u\n#define HTOT %u\n#define NSTRIPE %u\n"
           "#define JSTAGE %u\n#define JC %u\n"
           "#define PW(dc)                                              \\\n"
           "  (((dc).flags & OBX_DF_BITPACK) ? (uint32_t)(dc).width     \\\n"
           "                                 : (uint32_t)(dc).width * 8u)\n\n",
           NL, NG, st.n_w64 > 0 ? st.n_w64 : 1, (unsigned)ph.n_aggs,
           st.hist_total > 0 ? st.hist_total : 1, (unsigned)st.stripes,
           (unsigned)st.stage_bytes, st.jcells);
  s += b;
  s += "/* LDS-DMA stage of one block; the partial tail chunk is handled\n"
       "   by the exec mask (the LDS destination must stay uniform +\n"
       "   lane-linear for global_load_lds addressing) */\n"
       "__device__ __forceinline__ void stage2(\n"
       "    const uint8_t *__restrict__ buf, const dev_block &blk,\n"
       "    uint8_t *dst) {\n"
       "  const uint32_t n16 = (blk.block_len + 15) >> 4;\n"
       "  const uint8_t *src = buf + blk.block_byte;\n"
       "  for (uint32_t i = threadIdx.x; i < n16; i += WG) {\n"
       "    __builtin_amdgcn_global_load_lds(\n"
       "        (const __attribute__((address_space(1))) uint32_t\n"
       "             *)(src + (size_t)i * 16),\n"
       "        (__attribute__((address_space(3))) uint32_t\n"
       "             *)(dst + (size_t)i * 16),\n"
       "        16, 0, 0);\n"
       "  }\n"
       "}\n"
       "/* 32-bit-offset packed read from an 8-B-aligned base */\n"
       "__device__ __forceinline__ uint64_t jit_bread(\n"
       "    const uint8_t *__restrict__ b, uint32_t bitpos, uint32_t k) {\n"
       "  const uint64_t *w = (const uint64_t *)b;\n"
       "  uint32_t widx = bitpos >> 6, sh = bitpos & 63;\n"
       "  uint64_t v = w[widx] >> sh;\n"
       "  if (sh + k > 64) v |= w[widx + 1] << (64 - sh);\n"
       "  if (k < 64) v &= (((uint64_t)1 << k) - 1);\n"
       "  return v;\n"
       "}\n"
       "/* the 32 bits at bitpos from a 4-B-aligned base (callers mask\n"
       "   their fields out of it) */\n"
       "__device__ __forceinline__ uint32_t jit_bread32(\n"
       "    const uint8_t *__restrict__ b, uint32_t bitpos) {\n"
       "  const uint32_t *w = (const uint32_t *)b;\n"
       "  const uint32_t widx = bitpos >> 5;\n"
       "  return __builtin_amdgcn_alignbit(w[widx + 1], w[widx], bitpos & "
       "31);\n"
       "}\n"
      "__device__ __forceinline__ int jit_gslot(gslot *gt, uint64_t key) {\n"
      "  uint32_t idx = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - OBX_GTABLE_SHIFT)) &\n"
      "                 (OBX_GTABLE_SLOTS - 1);\n"
      "  for (int probe = 0; probe < OBX_GTABLE_SLOTS; probe++) {\n"
      "    unsigned long long ck = atomicCAS(&gt[idx].key, OBX_KEY_EMPTY,\n"
      "                                      (unsigned long long)key);\n"
      "    if (ck == OBX_KEY_EMPTY || ck == key) return (int)idx;\n"
      "    idx = (idx + 1) & (OBX_GTABLE_SLOTS - 1);\n"
      "  }\n"
      "  return -1;\n"
      "}\n\n";
  snprintf(b, sizeof b,
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
           "    unsigned long long *__restrict__ counters) {\n",
           st.wpb);
  s += b;
  const int sdb = st.sdb ? 1 : 0;
  if (sdb)
    s += "  __shared__ __attribute__((aligned(16))) uint8_t sega[JSTAGE],\n"
         "      segb[JSTAGE];\n";
  else
    s += "  __shared__ __attribute__((aligned(16))) uint8_t "
         "lds_blk[JSTAGE];\n";
  s += ""
       "  __shared__ unsigned long long wacc64[NW64][JC][NSTRIPE];\n"
       "  __shared__ uint32_t hist[HTOT];\n";
  if (st.n_mm > 0) {
    snprintf(b, sizeof b,
             "  /* CAS min/max cells: [slot][cell][val, valid] */\n"
             "  __shared__ unsigned long long wmm[%d][JC][2];\n",
             st.n_mm);
    s += b;
  }
  s += ""
       "  __shared__ uint64_t keytab[16];\n"
       "  __shared__ int cslot[16];\n";
  if (st.jws_on) {
    snprintf(b, sizeof b,
             "  __shared__ unsigned long long jws[%uu * %uu * %uu];\n",
             st.jws_cells, st.jws_d0, st.jws_d1);
    s += b;
  }
  if (st.cnt_hist < 0)
    s += "  __shared__ uint32_t wcnt[JC][NSTRIPE];\n";
  for (int t = 0; t < st.n_tab; t++) {
    snprintf(b, sizeof b, "  __shared__ long long vt%d[%u];\n", t,
             st.tabs[t].dim);
    s += b;
  }
  if (st.ctab_agg >= 0) {
    snprintf(b, sizeof b,
             "  /* combined factor table [xb][xc] of the narrowed PROD3 */\n"
             "  __shared__ uint32_t vtc[%uu * %uu];\n",
             st.ctab_db, st.ctab_dc);
    s += b;
  }
  s += "  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> "
       "6;\n"
       "  uint32_t lane_cnt = 0;\n"
       "  const uint32_t stripe = lane & (NSTRIPE - 1);\n"
       "\n"
       "  for (uint32_t i = tid; i < NW64 * JC * NSTRIPE; i += WG)\n"
       "    (&wacc64[0][0][0])[i] = 0;\n";
  if (st.n_mm > 0) {
    /* val slot gets the is_min/is_max sentinel; valid slot 0.  The
       per-agg sentinel depends on kind, so init per (slot,cell). */
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      if (st.amm[a] < 0) continue;
      snprintf(b, sizeof b,
               "  for (uint32_t i = tid; i < JC; i += WG) {\n"
               "    wmm[%d][i][0] = (unsigned long long)%s;\n"
               "    wmm[%d][i][1] = 0;\n"
               "  }\n",
               st.amm[a],
               ph.aggs[a].kind == OBX_AGG_MIN ? "INT64_MAX" : "INT64_MIN",
               st.amm[a]);
      s += b;
    }
  }
  s += ""
       "  for (uint32_t i = tid; i < HTOT; i += WG) hist[i] = 0;\n";
  if (st.jws_on) {
    snprintf(b, sizeof b,
             "  for (uint32_t i = tid; i < %uu * %uu * %uu; i += WG)\n"
             "    jws[i] = 0;\n",
             st.jws_cells, st.jws_d0, st.jws_d1);
    s += b;
  }
  if (st.cnt_hist < 0)
    s += "  for (uint32_t i = tid; i < JC * NSTRIPE; i += WG)\n"
         "    (&wcnt[0][0])[i] = 0;\n";
  /* one-time table + key builds from block 0 (dicts are identical) */
  s += "  {\n"
       "    const dev_block &b0 = blocks[0];\n"
       "    blk_view bv0;\n"
       "    bv0.base = buf + b0.block_byte;\n"
       "    bv0.bit_bias = b0.block_byte * 8;\n"
       "    bv0.rbase_bit = 0;\n";
  for (int t = 0; t < st.n_tab; t++) {
    const jit_vtab &vt = st.tabs[t];
    char ex[64];
    if (vt.kind == 0) snprintf(ex, sizeof ex, "e2");
    else if (vt.kind == 1)
      snprintf(ex, sizeof ex, "%lldll - e2", (long long)vt.one);
    else
      snprintf(ex, sizeof ex, "%lldll + e2", (long long)vt.one);
    snprintf(b, sizeof b,
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
             (unsigned)js.vcol[st.tabs[t].vc], st.tabs[t].dim, ex, t);
    s += b;
  }
  if (st.ctab_agg >= 0) {
    const dev_agg &g = ph.aggs[st.ctab_agg];
    snprintf(b, sizeof b,
             "    {\n"
             "      const dev_col *tb = &b0.cols[%u], *tc = &b0.cols[%u];\n"
             "      for (uint32_t e = tid; e < %uu * %uu; e += WG) {\n"
             "        const uint32_t eb = e / %uu, ec = e %% %uu;\n"
             "        long long fb = 0, fc = 0; /* null slots: factor 0 */\n"
             "        if (eb < tb->count) fb = %lldll - dict_entry(bv0, *tb, "
             "eb);\n"
             "        if (ec < tc->count) fc = %lldll + dict_entry(bv0, *tc, "
             "ec);\n"
             "        vtc[e] = (uint32_t)(fb * fc);\n"
             "      }\n"
             "    }\n",
             (unsigned)ph.need_cols[g.ib], (unsigned)ph.need_cols[g.ic],
             st.ctab_db, st.ctab_dc, st.ctab_dc, st.ctab_dc,
             (long long)g.one_b, (long long)g.one_c);
    s += b;
  }
  if (NG > 0) {
    snprintf(b, sizeof b,
             "    const dev_col *gb0 = &b0.cols[%u];\n"
             "    const uint32_t fdim0 = gb0->count + 1;\n",
             (unsigned)ph.need_cols[ph.group_idx[0]]);
    s += b;
    if (NG > 1) {
      snprintf(b, sizeof b,
               "    const dev_col *gb1 = &b0.cols[%u];\n"
               "    const uint32_t fdim1 = gb1->count + 1;\n"
               "    const uint32_t fcells = fdim0 * fdim1;\n",
               (unsigned)ph.need_cols[ph.group_idx[1]]);
      s += b;
    } else {
      s += "    const uint32_t fcells = fdim0;\n";
    }
    snprintf(b, sizeof b,
             "    for (uint32_t cell = tid; cell < fcells; cell += WG) {\n"
             "      uint32_t r0 = %s;\n"
             "      uint64_t key = 0;\n"
             "      if (r0 >= gb0->count) key |= 1ull << 56;\n"
             "      else {\n"
             "        int64_t kv = dict_entry(bv0, *gb0, r0);\n"
             "        key |= (uint64_t)kv & %s;\n"
             "      }\n",
             NG > 1 ? "cell % fdim0" : "cell",
             ph.group_len[0] >= 8 ? "~0ull"
                                  : "((1ull << (8 * KL0)) - 1)");
    std::string t1(b);
    char kl[16];
    snprintf(kl, sizeof kl, "%u", (unsigned)ph.group_len[0]);
    size_t p;
    while ((p = t1.find("KL0")) != std::string::npos) t1.replace(p, 3, kl);
    s += t1;
    if (NG > 1) {
      snprintf(b, sizeof b,
               "      uint32_t r1 = cell / fdim0;\n"
               "      if (r1 >= gb1->count) key |= 1ull << 57;\n"
               "      else {\n"
               "        int64_t kv1 = dict_entry(bv0, *gb1, r1);\n"
               "        key |= ((uint64_t)kv1 & %s) << (8 * %u);\n"
               "      }\n",
               ph.group_len[1] >= 8 ? "~0ull" : "((1ull << (8 * KL1)) - 1)",
               (unsigned)ph.group_len[0]);
      std::string t2(b);
      snprintf(kl, sizeof kl, "%u", (unsigned)ph.group_len[1]);
      while ((p = t2.find("KL1")) != std::string::npos) t2.replace(p, 3, kl);
      s += t2;
    }
    s += "      keytab[cell] = key;\n"
         "    }\n";
  } else {
    s += "    if (tid == 0) keytab[0] = 0;\n";
  }
  s += "  }\n"
       "  __syncthreads();\n"
       "\n";
  if (st.skew) {
    snprintf(b, sizeof b,
             "  /* stagger co-resident WGs (~%u us apart) so their DMA\n"
             "     and sweep phases interleave instead of convoying */\n"
             "  for (uint32_t j2 = 0;\n"
             "       j2 < ((blockIdx.x >> 8) & 7) * %uu; j2++)\n"
             "    __builtin_amdgcn_s_sleep(15);\n",
             (unsigned)st.skew, (unsigned)(st.skew * 3));
    s += b;
  }
  /* ---- block loop ---- */
  std::string body; /* per-block preamble + row sweep (emitted once for
                       the single-buffer loop, twice for the overlapped
                       2-phase loop) */
  body += "    const uint64_t blk_bit = cur.block_byte * 8;\n"
       "    blk_view bv;\n"
       "    bv.base = stg;\n"
       "    bv.bit_bias = blk_bit;\n"
       "    bv.rbase_bit = 0;\n"
       "    const uint32_t rows = cur.row_count;\n"
       "\n";
  if (NG > 0) {
    snprintf(b, sizeof b,
             "    const dev_col *gd0 = &cur.cols[%u];\n"
             "    const uint32_t go0 = (uint32_t)(gd0->data_bit - blk_bit);\n"
             "    const uint32_t gW0 = PW(*gd0);\n"
             "    const uint32_t gn0 = gd0->count;\n",
             (unsigned)ph.need_cols[ph.group_idx[0]]);
    body += b;
  }
  if (NG > 1) {
    snprintf(b, sizeof b,
             "    const dev_col *gd1 = &cur.cols[%u];\n"
             "    const uint32_t go1 = (uint32_t)(gd1->data_bit - blk_bit);\n"
             "    const uint32_t gW1 = PW(*gd1);\n"
             "    const uint32_t gn1 = gd1->count;\n"
             "    const uint32_t dim0 = gn0 + 1;\n",
             (unsigned)ph.need_cols[ph.group_idx[1]]);
    body += b;
  }
  for (int j = 0; j < js.n_vc; j++) {
    if (st.vmode[j] == JV_REF) {
      snprintf(b, sizeof b,
               "    const uint32_t xo%d =\n"
               "        (uint32_t)(cur.cols[%u].data_bit - blk_bit);\n"
               "    const uint32_t xW%d = PW(cur.cols[%u]);\n"
               "    const uint32_t xn%d = cur.cols[%u].count;\n",
               j, (unsigned)js.vcol[j], j, (unsigned)js.vcol[j], j,
               (unsigned)js.vcol[j]);
      body += b;
    } else if (st.vraw8[j]) {
      snprintf(b, sizeof b,
               "    const uint32_t vb%d =\n"
               "        (uint32_t)((cur.cols[%u].data_bit >> 3) - "
               "cur.block_byte);\n",
               j, (unsigned)js.vcol[j]);
      body += b;
    } else {
      snprintf(b, sizeof b,
               "    const col_ctx c%d = make_col_ctx(cur.cols[%u], "
               "blk_bit);\n",
               j, (unsigned)js.vcol[j]);
      body += b;
    }
  }
  /* filter leaf preambles (always inline in v2) */
  for (int i = 0; i < NL; i++) {
    snprintf(b, sizeof b,
             "    const blk_leaf lb%d = bl[%d];\n"
             "    const uint32_t l%do =\n"
             "        (uint32_t)(cur.cols[%u].data_bit - blk_bit);\n"
             "    const uint32_t l%dW = PW(cur.cols[%u]);\n",
             i, i, i, (unsigned)st.leaf_cols[i], i,
             (unsigned)st.leaf_cols[i]);
    body += b;
    if (st.leaf_kind[i] == 1) {
      snprintf(b, sizeof b,
               "    const bool l%d_all = lb%d.mode == OBX_LEAF_ALL;\n", i,
               i);
      body += b;
    }
    if (st.r > 1 && st.leaf_multi[i]) {
      if (st.leaf_m32[i])
        snprintf(b, sizeof b,
                 "    const uint32_t lm%d = (1u << l%dW) - 1;\n", i, i);
      else
        snprintf(b, sizeof b,
                 "    const uint64_t lm%d = (1ull << l%dW) - 1;\n", i, i);
      body += b;
    }
  }
  if (st.r > 1) {
    if (NG > 0 && st.g_multi[0])
      body += st.g_m32[0] ? "    const uint32_t gm0 = (1u << gW0) - 1;\n"
                          : "    const uint64_t gm0 = (1ull << gW0) - 1;\n";
    if (NG > 1 && st.g_multi[1])
      body += st.g_m32[1] ? "    const uint32_t gm1 = (1u << gW1) - 1;\n"
                          : "    const uint64_t gm1 = (1ull << gW1) - 1;\n";
    for (int j = 0; j < js.n_vc; j++)
      if (st.v_multi[j]) {
        if (st.v_m32[j])
          snprintf(b, sizeof b,
                   "    const uint32_t xm%d = (1u << xW%d) - 1;\n", j, j);
        else
          snprintf(b, sizeof b,
                   "    const uint64_t xm%d = (1ull << xW%d) - 1;\n", j, j);
        body += b;
      }
  }

  /* ---- accumulate body ---- */
  std::string acc;
  acc += "        lane_cnt += live ? 1u : 0u;\n";
  acc += "        if (live) {\n";
  if (st.cnt_hist < 0)
    acc += "          atomicAdd(&wcnt[cell][stripe], 1u);\n";
  for (int t = 0; t < st.n_hist; t++) {
    int j = st.hist_vc[t];
    snprintf(b, sizeof b,
             "          atomicAdd(&hist[%uu + cell * %uu + x%d], 1u);\n",
             st.hist_off[t], st.vdim[j], j);
    acc += b;
  }
  if (st.jws_on) {
    char idx[224];
    /* x is clamped to the null bucket already; when that bucket was
       dropped (non-nullable axis) clamp to the last real entry -- the
       branch is unreachable for checksum-valid refs */
    if (st.jws_a1 >= 0)
      snprintf(idx, sizeof idx,
               "cell * %uu + (x%d < %uu ? x%d : %uu) * %uu + (x%d < %uu ? "
               "x%d : %uu)",
               st.jws_d0 * st.jws_d1, st.jws_a0, st.jws_d0, st.jws_a0,
               st.jws_d0 - 1, st.jws_d1, st.jws_a1, st.jws_d1, st.jws_a1,
               st.jws_d1 - 1);
    else
      snprintf(idx, sizeof idx, "cell * %uu + (x%d < %uu ? x%d : %uu)",
               st.jws_d0, st.jws_a0, st.jws_d0, st.jws_a0, st.jws_d0 - 1);
    snprintf(b, sizeof b,
             "          if (!nu%d)\n"
             "            atomicAdd(&jws[%s],\n"
             "                      (unsigned long long)v%d);\n",
             st.jws_ja, idx, st.jws_ja);
    acc += b;
  }
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg &g = ph.aggs[a];
    if (st.jws_member[a]) continue; /* folded into the joint wsum */
    if (st.astrat[a] == JA_I64_COUNT) {
      snprintf(b, sizeof b,
               "          if (!nu%d)\n"
               "            atomicAdd(&wacc64[%d][cell][stripe], 1ull);\n",
               st.aval_a[a], st.wa64[a]);
      acc += b;
      continue;
    }
    if (st.astrat[a] == JA_MM) {
      snprintf(b, sizeof b,
               "          if (!nu%d) {\n"
               "            cas_minmax(&wmm[%d][cell][0], v%d, %s);\n"
               "            wmm[%d][cell][1] = 1;\n"
               "          }\n",
               st.aval_a[a], st.amm[a], st.aval_a[a],
               g.kind == OBX_AGG_MIN ? "true" : "false", st.amm[a]);
      acc += b;
      continue;
    }
    if (st.astrat[a] != JA_I64) continue;
    int ja = st.aval_a[a];
    char va[64];
    if (st.atab_a[a] >= 0)
      snprintf(va, sizeof va, "vt%d[x%d]", st.atab_a[a], ja);
    else
      snprintf(va, sizeof va, "v%d", ja);
    auto slot_lookup = [&](uint8_t need_idx) -> int {
      for (int j2 = 0; j2 < js.n_vc; j2++)
        if (js.vcol[j2] == ph.need_cols[need_idx]) return j2;
      return -1;
    };
    switch (g.kind) {
      case OBX_AGG_SUM:
        snprintf(b, sizeof b,
                 "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                 "                    (unsigned long long)%s);\n",
                 st.wa64[a], va);
        acc += b;
        break;
      case OBX_AGG_SUM_MUL: {
        int jb = slot_lookup(g.ib);
        char vb[64];
        if (st.atab_b[a] >= 0)
          snprintf(vb, sizeof vb, "vt%d[x%d]", st.atab_b[a], jb);
        else
          snprintf(vb, sizeof vb, "(nu%d ? 0ll : v%d)", jb, jb);
        snprintf(b, sizeof b,
                 "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                 "                    (unsigned long long)((long long)%s * "
                 "%s));\n",
                 st.wa64[a], va, vb);
        acc += b;
        break;
      }
      case OBX_AGG_SUM_PROD2: {
        int jb = slot_lookup(g.ib);
        char vb[64];
        if (st.atab_b[a] >= 0)
          snprintf(vb, sizeof vb, "vt%d[x%d]", st.atab_b[a], jb);
        else
          snprintf(vb, sizeof vb, "(nu%d ? 0ll : (%lldll - v%d))", jb,
                   (long long)g.one_b, jb);
        snprintf(b, sizeof b,
                 "          long long p2_%u = (long long)%s * %s;\n"
                 "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                 "                    (unsigned long long)p2_%u);\n",
                 a, va, vb, st.wa64[a], a);
        acc += b;
        if ((js.agg_f2 & (1u << a)) && !st.jws_member[a + 1]) {
          const dev_agg &g3 = ph.aggs[a + 1];
          int jc = slot_lookup(g3.ic);
          char vc[64];
          if (st.atab_c[a + 1] >= 0)
            snprintf(vc, sizeof vc, "vt%d[x%d]", st.atab_c[a + 1], jc);
          else
            snprintf(vc, sizeof vc, "(nu%d ? 0ll : (%lldll + v%d))", jc,
                     (long long)g3.one_c, jc);
          snprintf(b, sizeof b,
                   "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                   "                    (unsigned long long)(p2_%u * "
                   "%s));\n",
                   st.wa64[a + 1], a, vc);
          acc += b;
        }
        break;
      }
      case OBX_AGG_SUM_PROD3: {
        /* fused into the preceding PROD2's emission — unless that agg
           became a JWS member and skipped its per-row code entirely */
        if (a > 0 && (js.agg_f2 & (1u << (a - 1))) &&
            !st.jws_member[a - 1])
          break;
        int jb = slot_lookup(g.ib), jc = slot_lookup(g.ic);
        if (st.ctab_agg == (int)a) {
          snprintf(b, sizeof b,
                   "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                   "                    (unsigned long long)(uint32_t)v%d *\n"
                   "                        (unsigned long long)vtc[x%d * %uu "
                   "+ x%d]);\n",
                   st.wa64[a], ja, jb, st.ctab_dc, jc);
          acc += b;
          break;
        }
        char vb[64], vc[64];
        if (st.atab_b[a] >= 0)
          snprintf(vb, sizeof vb, "vt%d[x%d]", st.atab_b[a], jb);
        else
          snprintf(vb, sizeof vb, "(nu%d ? 0ll : (%lldll - v%d))", jb,
                   (long long)g.one_b, jb);
        if (st.atab_c[a] >= 0)
          snprintf(vc, sizeof vc, "vt%d[x%d]", st.atab_c[a], jc);
        else
          snprintf(vc, sizeof vc, "(nu%d ? 0ll : (%lldll + v%d))", jc,
                   (long long)g.one_c, jc);
        snprintf(b, sizeof b,
                 "          atomicAdd(&wacc64[%d][cell][stripe],\n"
                 "                    (unsigned long long)((long long)%s * "
                 "%s * %s));\n",
                 st.wa64[a], va, vb, vc);
        acc += b;
        break;
      }
    }
  }
  acc += "        }\n";

  /* ---- row sweep (strip-mined; whole WG over the block) ---- */
  std::string sweep2; /* emitted after the next block's DMA issue so the
                         glds spans the whole row sweep */
  int R = st.r > 0 ? st.r : 1;
  snprintf(b, sizeof b,
           "    const uint32_t itersR = (rows + WG * %d - 1) / (WG * %d);\n"
           "    for (uint32_t it = 0; it < itersR; it++) {\n"
           "      const uint32_t rbase = (it * WG + tid) * %d;\n",
           R, R, R);
  sweep2 += b;
  for (int i = 0; i < NL; i++)
    if (st.leaf_multi[i]) {
      if (st.leaf_m32[i])
        snprintf(b, sizeof b,
                 "      uint32_t wl%d = jit_bread32(bv.base, l%do + rbase * "
                 "l%dW);\n",
                 i, i, i);
      else
        snprintf(b, sizeof b,
                 "      uint64_t wl%d = jit_bread(bv.base, l%do + rbase * "
                 "l%dW, %d * l%dW);\n",
                 i, i, i, R, i);
      sweep2 += b;
    }
  for (int g2 = 0; g2 < NG && g2 < 2; g2++) {
    if (!st.g_multi[g2]) continue;
    if (st.g_m32[g2])
      snprintf(b, sizeof b,
               "      uint32_t wgr%d = jit_bread32(bv.base, go%d + rbase * "
               "gW%d);\n",
               g2, g2, g2);
    else
      snprintf(b, sizeof b,
               "      uint64_t wgr%d = jit_bread(bv.base, go%d + rbase * "
               "gW%d, %d * gW%d);\n",
               g2, g2, g2, R, g2);
    sweep2 += b;
  }
  for (int j = 0; j < js.n_vc; j++)
    if (st.v_multi[j]) {
      if (st.v_m32[j])
        snprintf(b, sizeof b,
                 "      uint32_t wx%d = jit_bread32(bv.base, xo%d + rbase * "
                 "xW%d);\n",
                 j, j, j);
      else
        snprintf(b, sizeof b,
                 "      uint64_t wx%d = jit_bread(bv.base, xo%d + rbase * "
                 "xW%d, %d * xW%d);\n",
                 j, j, j, R, j);
      sweep2 += b;
    }
  for (int j = 0; j < js.n_vc; j++)
    if (st.vmode[j] == JV_CTX && st.vraw8[j]) {
      snprintf(b, sizeof b,
               "      const uint8_t *ep%d = bv.base + vb%d + (rbase << "
               "3);\n",
               j, j);
      sweep2 += b;
    }
  snprintf(b, sizeof b,
           "#pragma unroll\n"
           "      for (uint32_t k = 0; k < %du; k++) {\n"
           "        const uint32_t r = rbase + k;\n"
           "        bool live = r < rows;\n",
           R);
  sweep2 += b;
  for (int i = 0; i < NL; i++) {
    if (st.leaf_kind[i] == 1) {
      if (st.leaf_multi[i])
        snprintf(b, sizeof b,
                 "        if (live && !l%d_all) {\n"
                 "          uint64_t v = ((wl%d >> (k * l%dW)) & lm%d) ^ "
                 "lb%d.mask;\n"
                 "          live = ((v - lb%d.lo) <= (lb%d.hi - lb%d.lo)) "
                 "!= (bool)lb%d.invert;\n"
                 "        }\n",
                 i, i, i, i, i, i, i, i, i);
      else
        snprintf(b, sizeof b,
                 "        if (live && !l%d_all) {\n"
                 "          uint64_t v = jit_bread(bv.base, l%do + r * "
                 "l%dW, l%dW) ^ lb%d.mask;\n"
                 "          live = ((v - lb%d.lo) <= (lb%d.hi - lb%d.lo)) "
                 "!= (bool)lb%d.invert;\n"
                 "        }\n",
                 i, i, i, i, i, i, i, i, i);
    } else {
      if (st.leaf_multi[i])
        snprintf(b, sizeof b,
                 "        if (live)\n"
                 "          live = (lb%d.mask >>\n"
                 "                  (uint32_t)((wl%d >> (k * l%dW)) & "
                 "lm%d)) & 1;\n",
                 i, i, i, i);
      else
        snprintf(b, sizeof b,
                 "        if (live)\n"
                 "          live = (lb%d.mask >>\n"
                 "                  (uint32_t)jit_bread(bv.base, l%do + r "
                 "* l%dW, l%dW)) & 1;\n",
                 i, i, i, i);
    }
    sweep2 += b;
  }
  if (NG > 0) {
    if (st.r > 1 && st.g_multi[0])
      sweep2 += "        uint32_t ref0 = (uint32_t)((wgr0 >> (k * gW0)) & "
           "gm0);\n";
    else
      sweep2 += "        uint32_t ref0 = (uint32_t)jit_bread(bv.base, go0 + r * "
           "gW0, gW0);\n";
    sweep2 += "        if (ref0 > gn0) ref0 = gn0;\n"
         "        uint32_t cell = ref0;\n";
  }
  if (NG > 1) {
    if (st.r > 1 && st.g_multi[1])
      sweep2 += "        uint32_t ref1 = (uint32_t)((wgr1 >> (k * gW1)) & "
           "gm1);\n";
    else
      sweep2 += "        uint32_t ref1 = (uint32_t)jit_bread(bv.base, go1 + r * "
           "gW1, gW1);\n";
    sweep2 += "        if (ref1 > gn1) ref1 = gn1;\n"
         "        cell += ref1 * dim0;\n";
  }
  if (NG == 0) s += "        const uint32_t cell = 0;\n";
  for (int j = 0; j < js.n_vc; j++) {
    if (st.vmode[j] == JV_REF) {
      if (st.v_multi[j])
        snprintf(b, sizeof b,
                 "        uint32_t x%d = (uint32_t)((wx%d >> (k * xW%d)) & "
                 "xm%d);\n"
                 "        if (x%d > xn%d) x%d = xn%d;\n",
                 j, j, j, j, j, j, j, j);
      else
        snprintf(b, sizeof b,
                 "        uint32_t x%d = (uint32_t)jit_bread(bv.base, xo%d "
                 "+ r * xW%d, xW%d);\n"
                 "        if (x%d > xn%d) x%d = xn%d;\n",
                 j, j, j, j, j, j, j, j);
      sweep2 += b;
    } else if (st.vraw8[j]) {
      snprintf(b, sizeof b,
               "        int64_t v%d = *(const int64_t *)(ep%d + (k << "
               "3));\n"
               "        const bool nu%d = false;\n"
               "        (void)nu%d;\n",
               j, j, j, j);
      sweep2 += b;
    } else {
      snprintf(b, sizeof b,
               "        bool nu%d;\n"
               "        int64_t v%d = ctx_value(bv, c%d, r, nu%d);\n"
               "        (void)nu%d;\n",
               j, j, j, j, j);
      sweep2 += b;
    }
  }
  sweep2 += acc;
  sweep2 += "      }\n"
       "    } /* row sweep */\n";
  if (sdb) {
    /* overlapped 2-phase loop: next block's LDS-DMA spans this block's
       sweep (raw lgkm-only barriers; two distinct stage buffers --
       hipcc drains glds to vmcnt(0) at __syncthreads and at aliased
       LDS reads, see the filter JIT) */
    s += "  uint32_t blkA = blockIdx.x;\n"
         "  {\n"
         "  uint8_t vA = 0;\n"
         "  while (blkA < n_blocks) {\n"
         "    const dev_block &nb = blocks[blkA];\n"
         "    const blk_leaf *nbl = bleaves + (uint64_t)blkA * (NL ? NL : "
         "1);\n"
         "    vA = 1;\n"
         "    for (uint32_t i = 0; i < NL; i++)\n"
         "      if (leaf_class(nb, plan_leaves[i], nbl[i]) == 0) { vA = 0; "
         "break; }\n"
         "    if (vA) break;\n"
         "    blkA += gridDim.x;\n"
         "  }\n"
         "  if (blkA < n_blocks) {\n"
         "    stage2(buf, blocks[blkA], sega);\n"
         "    for (;;) {\n";
    const char *bufs2[2] = {"sega", "segb"};
    for (int ph2 = 0; ph2 < 2; ph2++) {
      snprintf(b, sizeof b,
               "      {\n"
               "      uint32_t blkN = blkA + gridDim.x;\n"
               "      while (blkN < n_blocks) {\n"
               "        const dev_block &nb = blocks[blkN];\n"
               "        const blk_leaf *nbl = bleaves + (uint64_t)blkN * "
               "(NL ? NL : 1);\n"
               "        uint8_t v2 = 1;\n"
               "        for (uint32_t i = 0; i < NL; i++)\n"
               "          if (leaf_class(nb, plan_leaves[i], nbl[i]) == 0) "
               "{ v2 = 0; break; }\n"
               "        if (v2) break;\n"
               "        blkN += gridDim.x;\n"
               "      }\n"
               "      asm volatile(\"s_waitcnt vmcnt(0)\" ::: "
               "\"memory\");\n"
               "      asm volatile(\"s_waitcnt lgkmcnt(0)\" ::: "
               "\"memory\");\n"
               "      __builtin_amdgcn_s_barrier();\n"
               "      const uint32_t blk = blkA;\n"
               "      const dev_block &cur = blocks[blk];\n"
               "      const blk_leaf *bl = bleaves + (uint64_t)blk * (NL ? "
               "NL : 1);\n"
               "      uint8_t blk_verdict = 1;\n"
               "      for (uint32_t i = 0; i < NL; i++) {\n"
               "        uint8_t c = leaf_class(cur, plan_leaves[i], "
               "bl[i]);\n"
               "        if (c == 2) { blk_verdict = 2; break; }\n"
               "      }\n"
               "      uint8_t *stg = %s;\n",
               bufs2[ph2]);
      s += b;
      s += body; /* preamble: ordinary loads BEFORE the next issue */
      snprintf(b, sizeof b,
               "      if (blkN < n_blocks) stage2(buf, blocks[blkN], "
               "%s);\n",
               bufs2[ph2 ^ 1]);
      s += b;
      s += sweep2; /* ds-only row sweep: the glds spans it */
      s += "      asm volatile(\"s_waitcnt lgkmcnt(0)\" ::: "
           "\"memory\");\n"
           "      __builtin_amdgcn_s_barrier();\n"
           "      if (blkN >= n_blocks) { blkA = n_blocks; break; }\n"
           "      blkA = blkN;\n"
           "      }\n";
    }
    s += "    }\n"
         "  }\n"
         "  }\n";
  } else {
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
       "    uint8_t *stg = lds_blk;\n";
  s += body;
  s += sweep2;
  s += "  } /* blocks */\n";
  }
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
  if (NG > 0) {
    snprintf(b, sizeof b,
             "  const uint32_t fdim0 = b0.cols[%u].count + 1;\n",
             (unsigned)ph.need_cols[ph.group_idx[0]]);
    s += b;
  }
  if (NG > 1) {
    snprintf(b, sizeof b,
             "  const uint32_t fcells = fdim0 * (b0.cols[%u].count + 1);\n",
             (unsigned)ph.need_cols[ph.group_idx[1]]);
    s += b;
  } else if (NG == 1) {
    s += "  const uint32_t fcells = fdim0;\n";
  } else {
    s += "  const uint32_t fcells = 1;\n";
  }
  /* Hierarchical flush: everything summed over dict refs or joint-cell
     slices (passes 2 and 3) is first reduced inside the workgroup, in
     exact int128 in LDS, so each workgroup sends ONE global accumulate per
     (cell, aggregate) instead of one per ref -- the per-ref form put ~87
     same-address L2 atomics per live cell per workgroup on four slots.
     The partials live in the stage buffer, which is idle by now. */
  uint32_t f_sum = 0, f_min = 0, f_max = 0; /* aggregates going via facc */
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.astrat[a] == JA_HIST || st.astrat[a] == JA_HCOUNT ||
        (st.jws_on && st.jws_member[a]))
      f_sum |= 1u << a;
    else if (st.astrat[a] == JA_HISTMM)
      (ph.aggs[a].kind == OBX_AGG_MIN ? f_min : f_max) |= 1u << a;
  }
  const bool f_any = (f_sum | f_min | f_max) != 0;
  if (f_any) {
    snprintf(b, sizeof b,
             "  /* workgroup partials [cell][agg]: {lo, hi} of an int128\n"
             "     sum, or {value, valid} of a min/max */\n"
             "  unsigned long long (*facc)[NAGGS][2] =\n"
             "      (unsigned long long (*)[NAGGS][2])%s;\n"
             "  for (uint32_t i = tid; i < JC * NAGGS; i += WG) {\n"
             "    const uint32_t a = i %% NAGGS;\n"
             "    facc[i / NAGGS][a][0] =\n"
             "        ((0x%xu >> a) & 1)   ? (unsigned long long)INT64_MAX\n"
             "        : ((0x%xu >> a) & 1) ? (unsigned long long)INT64_MIN\n"
             "                             : 0ull;\n"
             "    facc[i / NAGGS][a][1] = 0;\n"
             "  }\n",
             sdb ? "sega" : "lds_blk", f_min, f_max);
    s += b;
  }
  s += "  /* flush pass 1: per-cell counts, keys -> global slots */\n"
       "  for (uint32_t cell = tid; cell < fcells; cell += WG) {\n"
       "    int ce = -1;\n";
  if (st.cnt_hist >= 0) {
    int j = st.hist_vc[st.cnt_hist];
    snprintf(b, sizeof b,
             "    unsigned long long cnt2 = 0;\n"
             "    for (uint32_t ref = 0; ref < %uu; ref++)\n"
             "      cnt2 += hist[%uu + cell * %uu + ref];\n",
             st.vdim[j], st.hist_off[st.cnt_hist], st.vdim[j]);
    s += b;
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
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.astrat[a] == JA_COUNT_STAR) {
      snprintf(b, sizeof b,
               "        g_acc_i128(gtable[gi].cells[%u], cnt2, 0);\n",
               (unsigned)a);
      s += b;
    }
  }
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.wa64[a] < 0) continue;
    snprintf(b, sizeof b,
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
    s += b;
  }
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    if (st.amm[a] < 0) continue;
    snprintf(b, sizeof b,
             "        if (wmm[%d][cell][1]) {\n"
             "          cas_minmax(&gtable[gi].cells[%u][0],\n"
             "                     (int64_t)wmm[%d][cell][0], %s);\n"
             "          gtable[gi].cells[%u][1] = 1;\n"
             "        }\n",
             st.amm[a], (unsigned)a, st.amm[a],
             ph.aggs[a].kind == OBX_AGG_MIN ? "true" : "false",
             (unsigned)a);
    s += b;
  }
  s += "      } else {\n"
       "        atomicAdd(&counters[1], cnt2);\n"
       "      }\n"
       "    }\n"
       "    cslot[cell] = ce;\n"
       "  }\n"
       "  __syncthreads();\n"
       "  /* flush pass 2: histogram-weighted aggregates over (cell, ref) "
       "*/\n";
  for (int t = 0; t < st.n_hist; t++) {
    int j = st.hist_vc[t];
    bool any = false;
    for (uint32_t a = 0; a < ph.n_aggs; a++)
      if (st.ahist[a] == t &&
          (st.astrat[a] == JA_HIST || st.astrat[a] == JA_HCOUNT ||
           st.astrat[a] == JA_HISTMM))
        any = true;
    if (!any) continue;
    snprintf(b, sizeof b,
             "  {\n"
             "    const uint32_t hcnt = b0.cols[%u].count;\n"
             "    for (uint32_t idx = tid; idx < fcells * %uu; idx += WG) "
             "{\n"
             "      uint32_t cell = idx / %uu, ref = idx %% %uu;\n"
             "      int ce = cslot[cell];\n"
             "      if (ce < 0 || ref >= hcnt) continue; /* excl. null "
             "bucket */\n"
             "      uint32_t c2 = hist[%uu + cell * %uu + ref];\n"
             "      if (!c2) continue;\n",
             (unsigned)js.vcol[j], st.vdim[j], st.vdim[j], st.vdim[j],
             st.hist_off[t], st.vdim[j]);
    s += b;
    bool need_entry = false;
    for (uint32_t a = 0; a < ph.n_aggs; a++)
      if (st.ahist[a] == t && st.astrat[a] == JA_HIST) need_entry = true;
    if (need_entry) {
      snprintf(b, sizeof b, "      long long ev = vt%d[ref];\n",
               st.hist_tab[t]);
      s += b;
    }
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      if (st.ahist[a] != t) continue;
      if (st.astrat[a] == JA_HIST) {
        snprintf(b, sizeof b,
                 "      {\n"
                 "        __int128 p = (__int128)ev * (long long)c2;\n"
                 "        i128v pv = {(uint64_t)p,\n"
                 "                    (uint64_t)((unsigned __int128)p >> "
                 "64)};\n"
                 "        lds_acc_i128(facc[cell][%u], pv);\n"
                 "      }\n",
                 (unsigned)a);
        s += b;
      } else if (st.astrat[a] == JA_HISTMM) {
        /* any live dict entry bounds the min/max */
        snprintf(b, sizeof b,
                 "      {\n"
                 "        cas_minmax(&facc[cell][%u][0],\n"
                 "                   (int64_t)vt%d[ref], %s);\n"
                 "        facc[cell][%u][1] = 1;\n"
                 "      }\n",
                 (unsigned)a, st.atab_a[a],
                 ph.aggs[a].kind == OBX_AGG_MIN ? "true" : "false",
                 (unsigned)a);
        s += b;
      } else { /* JA_HCOUNT */
        snprintf(b, sizeof b,
                 "      atomicAdd(&facc[cell][%u][0], (unsigned long "
                 "long)c2);\n",
                 (unsigned)a);
        s += b;
      }
    }
    s += "    }\n"
         "  }\n";
  }
  /* flush pass 3: joint weighted cells -> member aggregates.
     One (cell, d0) slice per thread; the d1 ring is reduced in
     registers, factor products applied in int128 (exact: the per-cell
     i64 bound is enforced at strategy build). */
  if (st.jws_on) {
    snprintf(b, sizeof b,
             "  for (uint32_t idx = tid; idx < fcells * %uu; idx += WG) "
             "{\n"
             "    uint32_t cell = idx / %uu, d0 = idx %% %uu;\n"
             "    int ce = cslot[cell];\n"
             "    if (ce < 0) continue;\n"
             "    long long s_pl = 0;\n",
             st.jws_d0, st.jws_d0, st.jws_d0);
    s += b;
    /* distinct axis-1 factor tables among members */
    int c_tabs[OBX_DEV_MAX_AGGS], n_ct = 0;
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      if (!st.jws_member[a] || st.jws_f1[a] < 0) continue;
      bool seen = false;
      for (int q = 0; q < n_ct; q++) seen |= c_tabs[q] == st.jws_f1[a];
      if (!seen) c_tabs[n_ct++] = st.jws_f1[a];
    }
    for (int q = 0; q < n_ct; q++) {
      snprintf(b, sizeof b, "    __int128 s_c%d = 0;\n", c_tabs[q]);
      s += b;
    }
    snprintf(b, sizeof b,
             "    for (uint32_t d1 = 0; d1 < %uu; d1++) {\n"
             "      long long w = (long long)jws[cell * %uu + d0 * %uu + "
             "d1];\n"
             "      if (!w) continue;\n"
             "      s_pl += w;\n",
             st.jws_d1, st.jws_d0 * st.jws_d1, st.jws_d1);
    s += b;
    for (int q = 0; q < n_ct; q++) {
      snprintf(b, sizeof b,
               "      s_c%d += (__int128)vt%d[d1] * w;\n", c_tabs[q],
               c_tabs[q]);
      s += b;
    }
    s += "    }\n"
         "    if (s_pl";
    for (int q = 0; q < n_ct; q++) {
      snprintf(b, sizeof b, " || s_c%d != 0", c_tabs[q]);
      s += b;
    }
    s += ") {\n";
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      if (!st.jws_member[a]) continue;
      char expr[128];
      if (st.jws_f0[a] >= 0 && st.jws_f1[a] >= 0)
        snprintf(expr, sizeof expr, "(__int128)vt%d[d0] * s_c%d",
                 st.jws_f0[a], st.jws_f1[a]);
      else if (st.jws_f0[a] >= 0)
        snprintf(expr, sizeof expr, "(__int128)vt%d[d0] * s_pl",
                 st.jws_f0[a]);
      else if (st.jws_f1[a] >= 0)
        snprintf(expr, sizeof expr, "s_c%d", st.jws_f1[a]);
      else
        snprintf(expr, sizeof expr, "(__int128)s_pl");
      snprintf(b, sizeof b,
               "      {\n"
               "        __int128 p = %s;\n"
               "        if (p != 0) {\n"
               "          i128v pv = {(uint64_t)p,\n"
               "                      (uint64_t)((unsigned __int128)p >> "
               "64)};\n"
               "          lds_acc_i128(facc[cell][%u], pv);\n"
               "        }\n"
               "      }\n",
               expr, (unsigned)a);
      s += b;
    }
    s += "    }\n"
         "  }\n";
  }
  if (f_any) {
    snprintf(b, sizeof b,
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
             f_sum, f_min | f_max, f_min);
    s += b;
  }
  s += "}\n";
  return s;
}

/* ======================================================================
 * Filter-only JIT (obx_gpu_filter with want_row_ids == 0): wave-per-block
 * with NO LDS and NO barriers — each wave streams its block's FILTER
 * column bytes straight through L1/L2 (a filter touches only the leaf
 * streams, so staging whole blocks would read bytes nobody needs),
 * evaluates the inline leaf chain and writes the survivor bitmap with
 * two atomicOr per 64 rows. Eligibility: every leaf packed-range or
 * dict-mask (same classes as the scan kernel's inline filter).
 * ==================================================================== */

static bool jit_build_fstrategy(const obx_handle &h, const dev_plan_hdr &ph,
                                const dev_leaf *pl, jit_strategy &st) {
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
    st.stripes = (uint8_t)sl; /* slice count for filter kernels */
  }
  uint32_t wmax = 0;
  for (uint32_t i = 0; i < ph.n_leaves; i++) {
    uint16_t col = pl[i].col;
    bool mask_ok = pl[i].op != 10 || pl[i].n_bcols == 1;
    if (h.col_dict_any[col] && mask_ok) st.leaf_kind[i] = 2;
    else if (pl[i].op <= 6 && h.col_rangefam_every[col])
      st.leaf_kind[i] = 1;
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
    const char *pe = getenv("OBX_JIT_FPROBE");
    st.fprobe = pe ? (uint8_t)atoi(pe) : 0;
    const char *ske = getenv("OBX_JIT_SKEW");
    st.skew = ske ? (uint8_t)atoi(ske) : 0;
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
  /* combine programs are codegen-folded in the staged kernel only */
  if (ph.n_prog && !st.fstage) return false;
  st.leaf_inline = 1;
  st.ok = true;
  return true;
}

static std::string jit_fstrategy_sig(const dev_plan_hdr &ph,
                                     const jit_strategy &st) {
  char b[128];
  std::string k = "F|";
  const char *fnbe = getenv("OBX_JIT_FNB");
  snprintf(b, sizeof b, "s%d|r%d|u%d|p%d|g%d:%u:%u:%u:%u|n%s|k%d|i%d|",
           st.stripes, st.r, st.fu, st.fprobe, st.fstage, st.fseg[0],
           st.fseg[1], st.fseg[2], st.fseg[3], fnbe ? fnbe : "-", st.skew,
           st.frid);
  k += b;
  k += "P";
  for (uint32_t p2 = 0; p2 < ph.n_prog; p2++) {
    snprintf(b, sizeof b, "%u.", ph.prog[p2]);
    k += b;
  }
  k += "|";
  b[0] = 0;
  k += b;
  for (uint32_t i = 0; i < ph.n_leaves; i++) {
    snprintf(b, sizeof b, "L%d:%u:m%d|", st.leaf_kind[i], st.leaf_cols[i],
             st.leaf_multi[i]);
    k += b;
  }
  return k;
}

static std::string jit_gen_source_filter(const dev_plan_hdr &ph,
                                         const jit_strategy &st) {
  const int NL = ph.n_leaves;
  char b[1024];
  std::string s;
  s += "#define OBX_PIPELINE 0\n#include \"obx_dev_common.h\"\n\n";
  snprintf(b, sizeof b,
           "#define NL %d\n#define FSL %d\n#define FR %d\n"
           "#define RID %d\n#define NCH %u\n"
           "#define PW(dc)                                              \\\n"
           "  (((dc).flags & OBX_DF_BITPACK) ? (uint32_t)(dc).width     \\\n"
           "                                 : (uint32_t)(dc).width * 8u)\n",
           NL, st.stripes > 0 ? st.stripes : 1, st.r > 0 ? st.r : 1,
           st.frid ? 1 : 0, (unsigned)(st.fnch ? st.fnch : 1));
  s += b;
  s += "__device__ __forceinline__ uint64_t jit_bread(\n"
       "    const uint8_t *__restrict__ b, uint32_t bitpos, uint32_t k) {\n"
       "  const uint64_t *w = (const uint64_t *)b;\n"
       "  uint32_t widx = bitpos >> 6, sh = bitpos & 63;\n"
       "  uint64_t v = w[widx] >> sh;\n"
       "  if (sh + k > 64) v |= w[widx + 1] << (64 - sh);\n"
       "  if (k < 64) v &= (((uint64_t)1 << k) - 1);\n"
       "  return v;\n"
       "}\n"
       "__device__ __forceinline__ uint8_t f3and(uint8_t a, uint8_t b) {\n"
       "  return (a == 0 || b == 0) ? 0 : ((a == 1 && b == 1) ? 1 : 2);\n"
       "}\n"
       "__device__ __forceinline__ uint8_t f3or(uint8_t a, uint8_t b) {\n"
       "  return (a == 1 || b == 1) ? 1 : ((a == 0 && b == 0) ? 0 : 2);\n"
       "}\n";
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
    /* ---- staged mode: WG per block, leaf streams DMA'd to LDS; when
       two buffers fit the LDS budget the next block's DMA overlaps the
       current block's sweep (uniform buffer parity: the LDS-DMA
       destination stays uniform + lane-linear) ---- */
    uint32_t off[4] = {}, total = 0;
    for (int i = 0; i < NL; i++) { off[i] = total; total += st.fseg[i]; }
    /* batch NB blocks per stage round: amortizes the per-block
       vmcnt(0) drain + barriers that serialize WGs into convoys (the
       per-block wall time measured constant ~7.5us regardless of block
       bytes) */
    int NB = 1; /* batching A/B'd worse: LDS growth costs occupancy */
    if (const char *ne = getenv("OBX_JIT_FNB")) {
      int v = atoi(ne);
      if (v >= 1 && v <= 8 && (uint32_t)v * total <= 64u * 1024u) NB = v;
    }
    /* double-buffer with RAW s_barrier: hipcc drains every in-flight
       global_load_lds to vmcnt(0) before a __syncthreads(), so the naive
       double-buffer overlapped nothing (measured identical); with
       lgkmcnt-only barriers the next block's DMA spans the sweep */
    /* measured: even with the glds span achieved in ISA, overlap buys
       nothing here — the strided stage pattern caps at ~2.4 TB/s with
       or without it (profiles/r02) — so default off */
    int DB2 = 0;
    if (const char *de2 = getenv("OBX_JIT_FDB2")) DB2 = atoi(de2) ? 1 : 0;
    if (DB2 && (NB > 1 || 2u * total > 64u * 1024u)) DB2 = 0;
    if (DB2 && 2u * total > 64u * 1024u) DB2 = 0;
    snprintf(b, sizeof b,
             "#define SEGSZ %uu\n#define FNB %d\n#define FDB2 %d\n",
             total, DB2 ? 1 : NB, DB2);
    s += b;
    s += "struct blkp {\n"
         "  const uint8_t *bp;\n"
         "  uint64_t row0;\n"
         "  uint32_t blk, rows;\n";
    snprintf(b, sizeof b,
             "  uint32_t W[%d], bit[%d], lo[%d], len[%d];\n"
             "  /* leaf payload in registers: the sweep must issue no\n"
             "     ordinary global load while the next block'\''s LDS-DMA\n"
             "     is in flight (its first use would drain vmcnt to 0) */\n"
             "  unsigned long long lmask[%d];\n"
             "  long long llo[%d], lhi[%d];\n"
             "  uint8_t linv[%d], lall[%d], lnone[%d];\n"
             "};\n",
             NL, NL, NL, NL, NL, NL, NL, NL, NL, NL);
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
    /* sweep of one staged block, as a string emitted twice (db/sb) */
    std::string sweep;
    if (st.fprobe == 2) {
      /* stage-only probe: consume one staged byte so DMA isn't dead */
      sweep = "      lane_cnt += SGB[lane] & 1;\n";
    } else {
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
                   "            ? jit_bread(SGB + %uu, cur.bit[%d] + rt * "
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
                       "          uint64_t v%d = jit_bread(SGB + %uu, "
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
                       "              (uint32_t)jit_bread(SGB + %uu, "
                       "cur.bit[%d] + r * cur.W[%d], cur.W[%d])) & 1;\n",
                       i, i, off[i], i, i, i);
          }
          sweep += b;
        }
        sweep += "          live = " + fold_prog("lf%d", true) + ";\n"
                 "          }\n";
      } else {
      for (int i = 0; i < NL; i++) {
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
                     "            uint64_t v = jit_bread(SGB + %uu, "
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
                     "                    (uint32_t)jit_bread(SGB + %uu, "
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
        if (st.leaf_kind[i] == 1)
          snprintf(b, sizeof b,
                   "        uint64_t v%d = jit_bread(SGB + %uu, cur.bit[%d]"
                   " + r * cur.W[%d], cur.W[%d]) ^ cur.lmask[%d];\n"
                   "        const bool lf%d = !cur.lnone[%d] &&\n"
                   "            (l%d_all || (((v%d - cur.llo[%d]) <= "
                   "(cur.lhi[%d] - cur.llo[%d])) != "
                   "(bool)cur.linv[%d]));\n",
                   i, off[i], i, i, i, i, i, i, i, i, i, i, i, i);
        else
          snprintf(b, sizeof b,
                   "        const bool lf%d = (cur.lmask[%d] >>\n"
                   "            (uint32_t)jit_bread(SGB + %uu, cur.bit[%d] "
                   "+ r * cur.W[%d], cur.W[%d])) & 1;\n",
                   i, i, off[i], i, i, i);
        sweep += b;
      }
      sweep += "        live = " + fold_prog("lf%d", true) + ";\n"
               "        }\n";
    } else {
    for (int i = 0; i < NL; i++) {
      if (st.leaf_kind[i] == 1)
        snprintf(b, sizeof b,
                 "        if (live && !l%d_all) {\n"
                 "          uint64_t v = jit_bread(SGB + %uu, cur.bit[%d] + "
                 "r * cur.W[%d], cur.W[%d]) ^ cur.lmask[%d];\n"
                 "          live = ((v - cur.llo[%d]) <= (cur.lhi[%d] - "
                 "cur.llo[%d])) != (bool)cur.linv[%d];\n"
                 "        }\n",
                 i, off[i], i, i, i, i, i, i, i, i);
      else
        snprintf(b, sizeof b,
                 "        if (live)\n"
                 "          live = (cur.lmask[%d] >>\n"
                 "                  (uint32_t)jit_bread(SGB + %uu, "
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
    }
    auto stage_with = [&](const char *pv, const char *bufname) {
      std::string o;
      char bb[512];
      for (int i = 0; i < NL; i++) {
        snprintf(bb, sizeof bb,
                 "      for (uint32_t i2 = tid; i2 * 16 < %s.len[%d]; i2 "
                 "+= WG)\n"
                 "        __builtin_amdgcn_global_load_lds(\n"
                 "            (const __attribute__((address_space(1))) "
                 "uint32_t\n"
                 "                 *)(%s.bp + %s.lo[%d] + (size_t)i2 * "
                 "16),\n"
                 "            (__attribute__((address_space(3))) "
                 "uint32_t\n"
                 "                 *)(%s + %uu + (size_t)i2 * 16),\n"
                 "            16, 0, 0);\n",
                 pv, i, pv, pv, i, bufname, off[i]);
        o += bb;
      }
      return o;
    };
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
    auto sweep_with = [&](const char *bufname) {
      std::string t = sweep;
      size_t p2 = 0;
      while ((p2 = t.find("SGB", p2)) != std::string::npos) {
        t.replace(p2, 3, bufname);
        p2 += strlen(bufname);
      }
      return t;
    };
    if (st.fprobe == 1) {
      /* no-flush probe: strip the global bitmap atomics */
      std::string t; size_t p0 = 0;
      while (p0 < sweep.size()) {
        size_t p1 = sweep.find("atomicOr(&bitmap", p0);
        if (p1 == std::string::npos) { t += sweep.substr(p0); break; }
        size_t p2 = sweep.find(";\n", p1);
        t += sweep.substr(p0, p1 - p0);
        t += "(void)0;\n";
        p0 = p2 + 2;
      }
      sweep = t;
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
         "#if FDB2\n"
         "  __shared__ uint8_t segA[SEGSZ], segB[SEGSZ];\n"
         "#else\n"
         "  __shared__ uint8_t seg[SEGSZ * FNB];\n"
         "#endif\n"
         "#if FR > 1\n"
         "  __shared__ unsigned long long fm[WAVES][FR];\n"
         "#endif\n"
         "#if RID\n"
         "  __shared__ unsigned long long cmask[NCH];\n"
         "  __shared__ uint32_t cpre[NCH];\n"
         "#endif\n"
         "  __shared__ unsigned long long wsum;\n"
         "  if (tid == 0) wsum = 0;\n";
  if (st.skew) {
    snprintf(b, sizeof b,
             "  for (uint32_t j2 = 0;\n"
             "       j2 < ((blockIdx.x >> 8) & 7) * %uu; j2++)\n"
             "    __builtin_amdgcn_s_sleep(15);\n",
             (unsigned)(st.skew * 3));
    s += b;
  }
  s += "  uint32_t bi = blockIdx.x;\n"
         "  const uint32_t gstep = gridDim.x;\n";
    if (DB2) {
      /* two distinct LDS arrays + a 2-phase unrolled loop: a runtime
         buffer-parity pointer defeats alias analysis, and hipcc then
         orders the sweep's ds_reads after the in-flight glds with a
         vmcnt(0) (seen in ISA) — static array references let the DMA
         truly span the sweep */
      s += "  blkp cur;\n"
           "  while (bi < n_blocks &&\n"
           "         !load_params(buf, blocks, plan_leaves, bleaves, bi, "
           "cur))\n"
           "    bi += gstep;\n"
           "  if (bi < n_blocks) {\n";
    {
      std::string t = stage_with("cur", "segA");
      /* top-level indentation: staged pre-loop */
      s += t;
    }
    s += "    for (;;) {\n";
      const char *bufs[2] = {"segA", "segB"};
      for (int ph2 = 0; ph2 < 2; ph2++) {
        snprintf(b, sizeof b,
                 "      {\n"
                 "      uint32_t bj = bi + gstep;\n"
                 "      blkp nxt;\n"
                 "      while (bj < n_blocks &&\n"
                 "             !load_params(buf, blocks, plan_leaves, "
                 "bleaves, bj, nxt))\n"
                 "        bj += gstep;\n"
                 "      asm volatile(\"s_waitcnt vmcnt(0)\" ::: "
                 "\"memory\");\n"
                 "      asm volatile(\"s_waitcnt lgkmcnt(0)\" ::: "
                 "\"memory\");\n"
                 "      __builtin_amdgcn_s_barrier();\n"
                 "      if (bj < n_blocks) {\n");
        s += b;
        s += stage_with("nxt", bufs[ph2 ^ 1]);
        s += "      }\n";
        s += sweep_with(bufs[ph2]);
        s += "      asm volatile(\"s_waitcnt lgkmcnt(0)\" ::: "
             "\"memory\");\n"
             "      __builtin_amdgcn_s_barrier();\n"
             "      if (bj >= n_blocks) break;\n"
             "      cur = nxt;\n"
             "      bi = bj;\n"
             "      }\n";
      }
      s += "    }\n"
           "  }\n";
    } else {
    s += "  for (;;) {\n";
    for (int j = 0; j < NB; j++) {
      snprintf(b, sizeof b,
               "    bool v%d = false;\n"
               "    blkp pb%d;\n"
               "    while (bi < n_blocks) {\n"
               "      bool ok = load_params(buf, blocks, plan_leaves, "
               "bleaves, bi, pb%d);\n"
               "      bi += gstep;\n"
               "      if (ok) { v%d = true; break; }\n"
               "    }\n",
               j, j, j, j);
      s += b;
    }
    s += "    if (!v0) break;\n"
         "    __syncthreads(); /* drain previous sweep's LDS reads */\n";
    for (int j = 0; j < NB; j++) {
      snprintf(b, sizeof b,
               "    if (v%d) issue_stage(pb%d, seg + %d * SEGSZ, tid);\n",
               j, j, j);
      s += b;
    }
    s += "    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n"
         "    __syncthreads();\n";
    for (int j = 0; j < NB; j++) {
      snprintf(b, sizeof b,
               "    if (v%d) {\n"
               "      const blkp &cur = pb%d;\n"
               "      uint8_t *sg = seg + %d * SEGSZ;\n",
               j, j, j);
      s += b;
      s += sweep_with("sg");
      s += "    }\n";
    }
    snprintf(b, sizeof b, "    if (!v%d) break;\n", NB - 1);
    s += b;
    s += "  }\n";
    }
    s += ""
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
      if (st.fprobe == 2) {
        /* loads-only probe: defeat DCE by folding the words into
           lane_cnt; measures the achievable thin-stream read rate */
        o += "        pm |= live ? (1u << k) : 0u;\n"
             "      }\n";
        for (int i = 0; i < NL; i++)
          if (st.leaf_multi[i]) {
            snprintf(bb, sizeof bb,
                     "      lane_cnt += (uint32_t)(wl%d%s ^ (wl%d%s >> "
                     "32));\n",
                     i, sfx.c_str(), i, sfx.c_str());
            o += bb;
          }
        o += "      lane_cnt += pm;\n"
             "      }\n";
        return o;
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
      if (st.fprobe == 1) { /* no-flush probe: eval but skip bitmap */
        o += "        pm |= live ? (1u << k) : 0u;\n"
             "      }\n"
             "      lane_cnt += (uint32_t)__builtin_popcount(pm);\n"
             "      }\n";
        return o;
      }
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

/* compile-or-fetch for the filter kernel */
static jit_entry *jit_get_filter(const dev_plan_hdr &ph,
                                 const jit_strategy &st) {
  std::string key = jit_fstrategy_sig(ph, st);
  auto it = g_jit_cache.find(key);
  if (it != g_jit_cache.end())
    return it->second.fn ? &it->second : nullptr;
  jit_entry ent;
  std::string src = jit_gen_source_filter(ph, st);
  if (getenv("OBX_JIT_DUMP")) {
    FILE *f = fopen("gpurun_out/obx_jit_filter_src.hip", "w");
    if (!f) f = fopen("/tmp/obx_jit_filter_src.hip", "w");
    if (f) { fwrite(src.data(), 1, src.size(), f); fclose(f); }
  }
  hiprtcProgram prog;
  const char *hdrs[2] = {OBX_JIT_SRC_COMMON_H, OBX_JIT_SRC_DEV_H};
  const char *hdr_names[2] = {"obx_dev_common.h", "obx_dev.h"};
  if (hiprtcCreateProgram(&prog, src.c_str(), "obx_jit_filter.hip", 2, hdrs,
                          hdr_names) != HIPRTC_SUCCESS) {
    g_jit_cache[key] = ent;
    return nullptr;
  }
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-DOBX_HIPRTC=1"};
  if (hiprtcCompileProgram(prog, 4, opts) != HIPRTC_SUCCESS) {
    size_t lsz = 0;
    hiprtcGetProgramLogSize(prog, &lsz);
    if (lsz > 1) {
      std::string log(lsz, '\0');
      hiprtcGetProgramLog(prog, &log[0]);
      fprintf(stderr, "obx: filter JIT compile failed:\n%s\n", log.c_str());
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
      hipModuleGetFunction(&ent.fn, ent.mod, "k_jit_filter") != hipSuccess) {
    ent.fn = nullptr;
    g_jit_cache[key] = ent;
    return nullptr;
  }
  auto r = g_jit_cache.emplace(key, ent);
  return &r.first->second;
}

static jit_entry *jit_prepare_filter(const obx_handle &h,
                                     const dev_plan_hdr &ph,
                                     const dev_leaf *pl, int want_row_ids) {
  const char *e = getenv("OBX_JIT");
  if (e && e[0] == '0') return nullptr;
  jit_strategy st;
  if (!jit_build_fstrategy(h, ph, pl, st)) return nullptr;
  if (want_row_ids) {
    /* ordered selection vectors need the per-block mask capture of the
       staged kernel and a bounded chunk count for the LDS mask array */
    uint32_t nch = ((h.max_block_rows ? h.max_block_rows : 4096) + 63) / 64;
    if (!st.fstage || st.fprobe || nch > 256) return nullptr;
    st.frid = 1;
    st.fnch = (uint16_t)nch;
  }
  return jit_get_filter(ph, st);
}
