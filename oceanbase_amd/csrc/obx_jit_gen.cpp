/*
 * obx_jit_gen.cpp — hipRTC-specialized kernels: the generators and what
 * they share. No HIP header and no device pointer: a table is its
 * obx_table_facts. Declarations for the other units are in obx_jit.h.
 *
 * The precompiled kernels are plan-generic: the aggregate program is data
 * (dev_plan_hdr), so every row pays descriptor loads, operand-select chains
 * and a pass per aggregate. PMC profiling (DESIGN.md round-1 findings) shows
 * the Q1 kernel near issue saturation — the ceiling is instructions per row,
 * and plan-generic machinery is most of them. This mirrors the reference's
 * own answer (vectorized expression codegen over the pushdown aggregate
 * plan, share/aggregate): specialize the kernel to the PLAN at runtime.
 *
 * For an eligible plan the engine generates a HIP kernel with the whole
 * plan as literals, compiles it once with hipRTC (cached by plan + strategy
 * signature), and launches it instead of the generic kernels. Results are
 * bit-identical: the same decode helpers (obx_dev_common.h) and the same
 * exact int128 arithmetic.
 *
 * This file holds what the generators share: the source emitter, the
 * packed-stream and leaf-test fragments, plan-shape and block eligibility,
 * the launch grid, and choose / key / source of the scan kernel. The embedded
 * device headers, the compile cache and prepare / launch are the hipRTC half,
 * obx_jit_rt.cpp. The generators themselves, one file per kernel, included
 * below:
 *   obx_jit_scan_v1.inc  scan, digit-split window accumulators (fallback
 *                        when the persistent kernel's bounds cannot be proven)
 *   obx_jit_scan.inc     scan, persistent accumulators (the Q1/Q6 hot path)
 *   obx_jit_filter.inc   bitmap / row-id filter
 * Device text that does not depend on the plan is in obx_jit_dev.h.
 *
 * Layout of a generator: one function per kernel phase, each with the
 * signature (plan, shape, strategy, out), and a top-level jit_gen_* that is
 * the list of those calls in kernel order. All text goes through jit_emit /
 * jit_fmt, which size their own storage: a fragment cannot be truncated.
 *
 * Generators are pure: their text depends only on their arguments, and the
 * cache key (plan signature + strategy signature) prints every argument
 * field the text reads. No jit_gen_* function reads the environment. The
 * environment is read where a strategy is built, and every knob lands in a
 * strategy field that the signature prints:
 *   jit_build_strategy   OBX_JIT_V2 (ok), OBX_JIT_JWS (jws_on, jws_member,
 *                        wa64), OBX_JIT_JPACK (jws_pack, jws_shift, jws_cax,
 *                        hists),
 *                        OBX_JIT_CTAB (ctab_agg), OBX_JIT_R (r),
 *                        OBX_JIT_M32 (*_m32), OBX_JIT_STRIPES (stripes),
 *                        OBX_JIT_WPB (wpb), OBX_JIT_BDESC (bdesc),
 *                        OBX_JIT_SGRID via jit_grid_for (decides ok only)
 *   jit_build_fstrategy  OBX_JIT_V2 (eligibility), OBX_JIT_FSL (nslice),
 *                        OBX_JIT_FR (r, leaf_multi), OBX_JIT_FU (fu),
 *                        OBX_JIT_FSTAGE (fstage)
 *   jit_scan_choose      OBX_JIT_WPB for the v1 kernel (jit_v1_strategy.wpb)
 *
 * OBX_JIT=0 disables; OBX_JIT_DUMP=<dir> writes the generated source
 * (obx_jit_src.hip, obx_jit_filter_src.hip) into that directory for offline
 * inspection, or into /tmp when it cannot be opened there (OBX_JIT_DUMP=1);
 * both are read in obx_jit_rt.cpp.
 */
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "obx_jit.h"

/* The source emitter: printf onto the end of a std::string. Two passes of
   vsnprintf, so the text is never cut; the format attribute keeps argument
   mistakes compile-time warnings. A value that a fragment repeats is passed
   once and named by position (%1$d). */
__attribute__((format(printf, 2, 0))) static void jit_vemit(std::string &s,
                                                            const char *fmt,
                                                            va_list ap) {
  va_list ap2;
  va_copy(ap2, ap);
  const int n = vsnprintf(nullptr, 0, fmt, ap2);
  va_end(ap2);
  if (n <= 0) return;
  const size_t at = s.size();
  s.resize(at + (size_t)n + 1);
  vsnprintf(&s[at], (size_t)n + 1, fmt, ap);
  s.resize(at + (size_t)n);
}

__attribute__((format(printf, 2, 3))) static void jit_emit(std::string &s,
                                                           const char *fmt,
                                                           ...) {
  va_list ap;
  va_start(ap, fmt);
  jit_vemit(s, fmt, ap);
  va_end(ap);
}

/* the same, as a value: for text that another fragment embeds */
__attribute__((format(printf, 1, 2))) static std::string jit_fmt(
    const char *fmt, ...) {
  std::string s;
  va_list ap;
  va_start(ap, fmt);
  jit_vemit(s, fmt, ap);
  va_end(ap);
  return s;
}

/* how a filter leaf is evaluated inline, from the load-time column facts;
   the scan kernel takes the first two, the filter kernel all three */
enum { JL_NONE = 0, JL_RANGE = 1, JL_MASK = 2, JL_SET = 3 };
static uint8_t jit_leaf_kind(const obx_table_facts &h, const dev_leaf &lf) {
  /* multi-column black programs cannot lower to a ref mask */
  const bool mask_ok = lf.op != OBX_OP_BLACK || lf.n_bcols == 1;
  if (h.col_dict_any[lf.col] && mask_ok) return JL_MASK;
  if (!h.col_rangefam_every[lf.col]) return JL_NONE;
  if (lf.op <= OBX_OP_BT) return JL_RANGE;
  return lf.op == OBX_OP_IN_SET ? JL_SET : JL_NONE;
}

/* A bit-packed stream as the generated code names it: the word that holds
   the lane's packed fields (w), the width (W) and field mask (m), and for a
   field read on its own the base pointer and bit offset. */
struct jit_stream {
  std::string w, W, m, base, off;
  /* field k of the lane's strip: cut from the packed word, or read alone */
  std::string field(bool packed) const {
    return packed ? jit_fmt("((%s >> (k * %s)) & %s)", w.c_str(), W.c_str(),
                            m.c_str())
                  : jit_fmt("jit_bread(%1$s, %2$s + r * %3$s, %3$s)",
                            base.c_str(), off.c_str(), W.c_str());
  }
};

/* names of a lowered leaf's operands, and the two row tests over a field.
   `pad` is the statement's indent. The chain form narrows `live`; the
   value form (combine programs) defines `lf<i>`. */
struct jit_leaf_ops {
  int i;
  std::string mask, lo, hi, inv, none;
};

static void jit_emit_range_test(std::string &s, int pad,
                                const jit_leaf_ops &o,
                                const std::string &field, bool chain) {
  const std::string in(pad, ' ');
  if (chain)
    jit_emit(s,
             "%1$sif (live && !l%2$d_all) {\n"
             "%1$s  uint64_t v = %3$s ^ %4$s;\n"
             "%1$s  live = ((v - %5$s) <= (%6$s - %5$s)) != (bool)%7$s;\n"
             "%1$s}\n",
             in.c_str(), o.i, field.c_str(), o.mask.c_str(), o.lo.c_str(),
             o.hi.c_str(), o.inv.c_str());
  else
    jit_emit(s,
             "%1$suint64_t v%2$d = %3$s ^ %4$s;\n"
             "%1$sconst bool lf%2$d = !%8$s &&\n"
             "%1$s    (l%2$d_all || (((v%2$d - %5$s) <= (%6$s - %5$s)) != "
             "(bool)%7$s));\n",
             in.c_str(), o.i, field.c_str(), o.mask.c_str(), o.lo.c_str(),
             o.hi.c_str(), o.inv.c_str(), o.none.c_str());
}

static void jit_emit_mask_test(std::string &s, int pad, const jit_leaf_ops &o,
                               const std::string &field, bool chain) {
  const std::string in(pad, ' ');
  if (chain)
    jit_emit(s,
             "%1$sif (live)\n"
             "%1$s  live = (%2$s >>\n"
             "%1$s          (uint32_t)%3$s) & 1;\n",
             in.c_str(), o.mask.c_str(), field.c_str());
  else
    jit_emit(s,
             "%1$sconst bool lf%4$d = (%2$s >>\n"
             "%1$s    (uint32_t)%3$s) & 1;\n",
             in.c_str(), o.mask.c_str(), field.c_str(), o.i);
}

/* grid of the persistent scan JIT (obx_jit_scan.inc): OBX_JIT_GRID_WAVES
   times what is resident at wpb workgroups per CU, and never more
   workgroups than blocks. Each workgroup flushes once, a handful of global
   atomics per live cell, so the grid is free to be finer than the resident
   set: the dispatcher then evens out CU-to-CU differences and the tail
   shrinks to one short workgroup. Measured on Q1 SF=100 (profiles/
   r03_q1_flush.md): 1x 3.00 ms, 2x 2.90, 4x 2.80, 8x 2.76, 12x 2.78,
   16x 2.82, 32x 3.70; 1.5x (a half-empty second wave) 3.22. The one
   source of that grid: the strategy proves its i64 accumulator bound for
   it and the launch uses it. OBX_JIT_SGRID=n caps it at n workgroups (the
   scan-side sibling of OBX_JIT_FGRID): small tables then give a workgroup
   several blocks, which the block loop's tests and A/B runs need. */
#define OBX_JIT_GRID_WAVES 8
uint32_t jit_grid_for(uint32_t n_blocks, uint32_t n_cus, int wpb) {
  uint64_t g = (uint64_t)(n_cus ? n_cus : 1) * (uint32_t)(wpb > 0 ? wpb : 1) *
               OBX_JIT_GRID_WAVES;
  if (const char *sg = getenv("OBX_JIT_SGRID")) {
    const long v = atol(sg);
    if (v >= 1 && (uint64_t)v < g) g = (uint64_t)v;
  }
  if (g > n_blocks) g = n_blocks;
  return g ? (uint32_t)g : 1;
}

/* Rows one workgroup of that grid can sweep: its share of the blocks times
   the rows of the largest block. The bound behind the i64 windows and the
   row count packed into the joint cells. */
static uint64_t jit_wg_rows(const obx_table_facts &h, uint32_t grid) {
  if (!grid) grid = 1;
  return (uint64_t)((h.n_blocks + grid - 1) / grid) *
         (h.max_block_rows ? h.max_block_rows : 4096);
}

/* the generators: (plan, strategy) -> strategy signature and HIP source */
#include "obx_jit_scan_v1.inc"
#include "obx_jit_scan.inc"
#include "obx_jit_filter.inc"

/* plan-shape eligibility + operand mapping (schema column indices, so the
   generated source carries cur.cols[<literal>]) */
bool jit_plan_shape(const dev_plan_hdr &ph, jit_shape &js) {
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
static uint32_t jit_pair_cells_max(const obx_table_facts &h, uint8_t c0,
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
bool jit_blocks_ok(const obx_table_facts &h, const dev_plan_hdr &ph,
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

int jit_scan_choose(const obx_table_facts &h, const dev_plan_hdr &ph,
                    const dev_leaf *pl, bool force_v1, jit_scan_choice &c) {
  if (!jit_plan_shape(ph, c.js) || !jit_blocks_ok(h, ph, c.js)) return 0;
  if (!force_v1) jit_build_strategy(h, ph, c.js, pl, c.st); /* !ok -> v1 */
  if (!c.st.ok && c.js.has_mm) return 0; /* v1 cannot do MIN/MAX */
  if (!c.st.ok)
    if (const char *w = getenv("OBX_JIT_WPB")) c.v1.wpb = w;
  return c.kind = c.st.ok ? 2 : 1;
}

std::string jit_scan_key(const dev_plan_hdr &ph, const jit_scan_choice &c) {
  return jit_plan_sig(ph) +
         (c.kind == 2 ? jit_strategy_sig(ph, c.st) : jit_v1_sig(c.v1));
}

std::string jit_scan_source(const dev_plan_hdr &ph, const jit_scan_choice &c) {
  return c.kind == 2 ? jit_gen_source_v2(ph, c.js, c.st)
                     : jit_gen_source(ph, c.js, c.v1);
}
