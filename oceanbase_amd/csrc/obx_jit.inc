
/*
 * obx_jit.inc — hipRTC-specialized kernels: shared infrastructure (included
 * by obx_engine.cpp).
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
 * packed-stream and leaf-test fragments, the embedded device headers, the
 * compile cache, plan-shape and block eligibility, compile-and-cache, and
 * choose / prepare / launch. The generators themselves, one file per kernel:
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
 * inspection, or into /tmp when it cannot be opened there (OBX_JIT_DUMP=1).
 */
#include <hip/hiprtc.h>

#include <cstdarg>
#include <map>
#include <string>

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

struct jit_entry {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  int wpb = 0; /* v2: workgroups per CU the launch grid is sized to */
  bool bdesc = false;        /* v2: reads the packed block descriptors ... */
  obx_bdesc_cols bd_cols = {}; /* ... of this ordered column list */
  int joint = 0;             /* v2: joint-table form (obx_gpu_last_joint) */
};

struct jit_shape {
  int n_vc = 0;
  uint8_t vcol[4] = {0xFF, 0xFF, 0xFF, 0xFF}; /* schema column indices */
  int n_wa = 0;
  uint8_t agg_wa[OBX_DEV_MAX_AGGS];  /* 0xFF = COUNT(*) */
  uint8_t agg_f2 = 0;                /* bit a: PROD2 fused with PROD3 mate */
  bool has_mm = false;               /* MIN/MAX present: v2-only (the v1
                                        generator has no CAS cells) */
  /* value slot (vcol index) of a plan need index; -1 when there is none */
  int slot(const dev_plan_hdr &ph, uint8_t need_idx) const {
    if (need_idx == 0xFF) return -1;
    for (int j = 0; j < n_vc; j++)
      if (vcol[j] == ph.need_cols[need_idx]) return j;
    return -1;
  }
};

/* how a filter leaf is evaluated inline, from the load-time column facts;
   the scan kernel takes the first two, the filter kernel all three */
enum { JL_NONE = 0, JL_RANGE = 1, JL_MASK = 2, JL_SET = 3 };
static uint8_t jit_leaf_kind(const obx_handle &h, const dev_leaf &lf) {
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

/* the generators: (plan, strategy) -> strategy signature and HIP source */
#include "obx_jit_scan_v1.inc"
#include "obx_jit_scan.inc"
#include "obx_jit_filter.inc"

static const char *OBX_JIT_SRC_DEV_H =
#include "obx_embed_dev_h.inc"
    ;
static const char *OBX_JIT_SRC_COMMON_H =
#include "obx_embed_common_h.inc"
    ;
static const char *OBX_JIT_SRC_JIT_DEV_H =
#include "obx_embed_jit_dev_h.inc"
    ;
static const char *OBX_JIT_SRC_KEYSET_H =
#include "obx_embed_keyset_h.inc"
    ;

static std::map<std::string, jit_entry> g_jit_cache;
static int g_jit_kind = 0; /* 1 = v1 generator, 2 = v2 (persistent) */

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

/* compile (or fetch) a generated kernel; nullptr on any failure (the caller
   falls back to the precompiled kernels). gen_src() builds the source and
   runs only on a cache miss; failures are cached too, so a plan that does
   not compile costs one attempt. dump_name is the OBX_JIT_DUMP file and the
   file name in the compile log. */
template <class GenSrc>
static jit_entry *jit_get(const std::string &key, GenSrc &&gen_src,
                          const char *kernel, const char *dump_name,
                          int wpb) {
  auto it = g_jit_cache.find(key);
  if (it != g_jit_cache.end())
    return it->second.fn ? &it->second : nullptr;
  jit_entry &ent = g_jit_cache[key]; /* fn stays null unless all succeeds */
  ent.wpb = wpb;
  const std::string src = gen_src();
  if (const char *dump_dir = getenv("OBX_JIT_DUMP")) {
    FILE *f = fopen((std::string(dump_dir) + "/" + dump_name).c_str(), "w");
    if (!f) f = fopen((std::string("/tmp/") + dump_name).c_str(), "w");
    if (f) { fwrite(src.data(), 1, src.size(), f); fclose(f); }
  }
  hiprtcProgram prog;
  const char *hdrs[4] = {OBX_JIT_SRC_COMMON_H, OBX_JIT_SRC_DEV_H,
                         OBX_JIT_SRC_JIT_DEV_H, OBX_JIT_SRC_KEYSET_H};
  const char *hdr_names[4] = {"obx_dev_common.h", "obx_dev.h",
                              "obx_jit_dev.h", "obx_keyset.h"};
  if (hiprtcCreateProgram(&prog, src.c_str(), dump_name, 4, hdrs,
                          hdr_names) != HIPRTC_SUCCESS)
    return nullptr;
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-DOBX_HIPRTC=1"};
  if (hiprtcCompileProgram(prog, 4, opts) != HIPRTC_SUCCESS) {
    size_t lsz = 0;
    hiprtcGetProgramLogSize(prog, &lsz);
    if (lsz > 1) {
      std::string log(lsz, '\0');
      hiprtcGetProgramLog(prog, &log[0]);
      fprintf(stderr, "obx: JIT compile failed (%s):\n%s\n", kernel,
              log.c_str());
    }
    hiprtcDestroyProgram(&prog);
    return nullptr;
  }
  size_t csz = 0;
  hiprtcGetCodeSize(prog, &csz);
  std::string code(csz, '\0');
  hiprtcGetCode(prog, &code[0]);
  hiprtcDestroyProgram(&prog);
  if (hipModuleLoadData(&ent.mod, code.data()) != hipSuccess ||
      hipModuleGetFunction(&ent.fn, ent.mod, kernel) != hipSuccess) {
    fprintf(stderr, "obx: JIT module load failed (%s)\n", kernel);
    ent.fn = nullptr;
    return nullptr;
  }
  return &ent;
}

/* Which scan kernel a plan gets, and everything its generator takes: the
   one sequence shape -> blocks -> strategy -> v1 or v2 behind both
   jit_prepare and the dump probe (obx_jit_dump_src_ex). */
struct jit_scan_choice {
  int kind = 0; /* 0 = no generated kernel, 1 = v1, 2 = v2 (persistent) */
  jit_shape js;
  jit_strategy st;    /* kind 2 */
  jit_v1_strategy v1; /* kind 1 */
};

static int jit_scan_choose(const obx_handle &h, const dev_plan_hdr &ph,
                           const dev_leaf *pl, bool force_v1,
                           jit_scan_choice &c) {
  if (!jit_plan_shape(ph, c.js) || !jit_blocks_ok(h, ph, c.js)) return 0;
  if (!force_v1) jit_build_strategy(h, ph, c.js, pl, c.st); /* !ok -> v1 */
  if (!c.st.ok && c.js.has_mm) return 0; /* v1 cannot do MIN/MAX */
  if (!c.st.ok)
    if (const char *w = getenv("OBX_JIT_WPB")) c.v1.wpb = w;
  return c.kind = c.st.ok ? 2 : 1;
}

static std::string jit_scan_key(const dev_plan_hdr &ph,
                                const jit_scan_choice &c) {
  return jit_plan_sig(ph) +
         (c.kind == 2 ? jit_strategy_sig(ph, c.st) : jit_v1_sig(c.v1));
}

static std::string jit_scan_source(const dev_plan_hdr &ph,
                                   const jit_scan_choice &c) {
  return c.kind == 2 ? jit_gen_source_v2(ph, c.js, c.st)
                     : jit_gen_source(ph, c.js, c.v1);
}

/* prepare (compile/lookup) before the timed region; nullptr = use the
   precompiled kernels */
static jit_entry *jit_prepare(const obx_handle &h, const dev_plan_hdr &ph,
                              const dev_leaf *pl) {
  const char *e = getenv("OBX_JIT");
  if (e && e[0] == '0') return nullptr;
  jit_scan_choice c;
  if (!jit_scan_choose(h, ph, pl, false, c)) return nullptr;
  g_jit_kind = c.kind;
  jit_entry *je = jit_get(
      jit_scan_key(ph, c), [&] { return jit_scan_source(ph, c); },
      "k_jit_scan", "obx_jit_src.hip", c.kind == 2 ? c.st.wpb : 0);
  if (je && c.kind == 2) { /* the signature carries both: same for every hit */
    je->bdesc = c.st.bdesc != 0;
    je->bd_cols = c.st.bd_cols;
    je->joint = jit_joint_form_of(c.st);
  }
  return je;
}

static jit_entry *jit_prepare_filter(const obx_handle &h,
                                     const dev_plan_hdr &ph,
                                     const dev_leaf *pl, int want_row_ids) {
  const char *e = getenv("OBX_JIT");
  if (e && e[0] == '0') return nullptr;
  jit_fstrategy st;
  if (!jit_build_fstrategy(h, ph, pl, st)) return nullptr;
  if (want_row_ids) {
    /* ordered selection vectors need the per-block mask capture of the
       staged kernel and a bounded chunk count for the LDS mask array */
    uint32_t nch = ((h.max_block_rows ? h.max_block_rows : 4096) + 63) / 64;
    if (!st.fstage || nch > 256) return nullptr;
    st.frid = 1;
    st.fnch = (uint16_t)nch;
  }
  return jit_get(
      jit_fstrategy_sig(ph, st), [&] { return jit_gen_source_filter(ph, st); },
      "k_jit_filter", "obx_jit_filter_src.hip", 0);
}

static int jit_launch(jit_entry *je, obx_handle &h, const obx_bdesc *bd,
                      hipStream_t stream, uint32_t *grid_out) {
  /* v2 keeps its accumulators for the kernel's lifetime and flushes once
     per workgroup: its grid is a multiple of the resident set (the grid
     the strategy proved its i64 bound for); v1 merges per block and keeps
     the fixed grid */
  const uint32_t grid = je->wpb ? jit_grid_for(h.n_blocks, h.n_cus, je->wpb)
                                : grid_for(h.n_blocks);
  *grid_out = grid;
  /* the v2 kernel takes the descriptor array last (null when its strategy
     reads dev_block); v1 has no such parameter and ignores the entry */
  void *args[8] = {&h.d_buf,     &h.d_blocks, &h.n_blocks,   &h.d_pleaves,
                   &h.d_bleaves, &h.d_gtable, &h.d_counters, &bd};
  return hipModuleLaunchKernel(je->fn, grid, 1, 1, OBX_WG_HOST, 1, 1, 0,
                               stream, args, nullptr) == hipSuccess
             ? 0
             : -1;
}
