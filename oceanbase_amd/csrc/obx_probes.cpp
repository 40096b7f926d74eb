/*
 * obx_probes.cpp — debug/test-only exports that run the plan builder and the
 * JIT generators against synthetic table facts, without a GPU. No HIP
 * header: a probe fills an obx_table_facts and never builds a handle.
 */
#include <cstdlib>
#include <cstring>
#include <string>

#include "obx_jit.h"

/* Debug/test-only: generate the hipRTC source the JIT would compile for a
 * plan against synthetic load-time column summaries, without a GPU (the
 * container has no device; tests hipcc-compile the dump offline).
 * col_flags bits: 1 = dict-everywhere, 2 = ext-any, 4 = bounds known.
 * Returns the source length (>= 0) or a negative status; 0 = the plan
 * would not take the JIT path. The _ex form also takes the block count and
 * the device's CU count (0 = default), which size the launch grid and with
 * it the i64 accumulator bound; a v2 source reports that grid in
 * *grid_out. */
extern "C" int64_t obx_jit_dump_src_ex(
    const obx_filter_desc *filter, const obx_agg_desc *agg,
    const obx_col_schema *cols, uint16_t n_cols, const uint8_t *col_flags,
    const int64_t *col_min, const int64_t *col_max,
    const uint32_t *col_maxcnt, const uint32_t *col_maxw,
    uint32_t max_block_rows, int force_v1, uint32_t n_blocks, uint32_t n_cus,
    uint32_t *grid_out, char *out, int64_t cap) {
  if (!cols || n_cols > OBX_DEV_MAX_COLS) return OBX_INVALID_ARGUMENT;
  if (grid_out) *grid_out = 0;
  /* no context here to resolve a set id: such a plan renders nothing */
  for (uint16_t i = 0; filter && i < filter->n_leaves && i < 8; i++)
    if (filter->leaves[i].op == OBX_OP_IN_SET) return 0;
  obx_table_facts h;
  h.n_cols = n_cols;
  h.n_blocks = n_blocks ? n_blocks : 1;
  if (n_cus) h.n_cus = n_cus;
  h.max_block_rows = max_block_rows ? max_block_rows : 4096;
  h.max_block_len = OBX_LDS_STAGE_BYTES - 32;
  memcpy(h.cols, cols, sizeof(obx_col_schema) * n_cols);
  for (uint16_t c = 0; c < n_cols; c++) {
    h.col_dict_every[c] = (col_flags[c] & 1) != 0;
    h.col_ext_any[c] = (col_flags[c] & 2) != 0;
    h.col_known[c] = (col_flags[c] & 4) != 0;
    h.col_raw8_every[c] = (col_flags[c] & 8) != 0;
    h.col_rangefam_every[c] = (col_flags[c] & 16) != 0;
    h.col_dict_any[c] = h.col_dict_every[c] ||
        (obx_store_class(cols[c].obj_type) == OBX_SC_STRING &&
         (col_flags[c] & 1));
    h.col_dict_stable[c] = (col_flags[c] & 32) != 0 && h.col_dict_any[c];
    h.col_min[c] = col_min[c];
    h.col_max[c] = col_max[c];
    h.col_maxcnt[c] = col_maxcnt[c];
    h.col_maxw[c] = col_maxw ? col_maxw[c] : 255;
    /* a maximum count past an obx_bdesc slot: some block does not fit */
    h.col_bdesc_unfit[c] = col_maxcnt[c] > 0xFFFFu;
    uint8_t cls = h.col_dict_every[c] ? 1 : 0;
    if (obx_store_class(cols[c].obj_type) == OBX_SC_STRING) cls |= 0x10;
    h.col_class.push_back(cls);
    h.col_cnt.push_back(
        (uint8_t)(h.col_maxcnt[c] > 254 ? 255 : h.col_maxcnt[c]));
  }
  summarize_col_classes(h); /* one synthetic block stands for all */
  dev_plan_hdr ph;
  dev_leaf pl[OBX_DEV_MAX_LEAVES];
  int rc = build_plan(nullptr, nullptr, h, filter, agg, ph, pl);
  if (rc != OBX_SUCCESS) return rc;
  if (!agg) { /* bitmap-filter path: dump the wave-per-block filter JIT */
    jit_fstrategy fst;
    if (!jit_build_fstrategy(h, ph, pl, fst)) return 0;
    if (getenv("OBX_DUMP_RID") && fst.fstage) { /* test hook */
      fst.frid = 1;
      fst.fnch = (uint16_t)((h.max_block_rows + 63) / 64);
    }
    std::string fsrc = jit_gen_source_filter(ph, fst);
    if (out && cap > (int64_t)fsrc.size()) {
      memcpy(out, fsrc.data(), fsrc.size());
      out[fsrc.size()] = 0;
    }
    return (int64_t)fsrc.size();
  }
  jit_scan_choice c;
  if (!jit_scan_choose(h, ph, pl, force_v1 != 0, c)) return 0;
  if (c.kind == 2 && grid_out)
    *grid_out = jit_grid_for(h.n_blocks, h.n_cus, c.st.wpb);
  std::string src = jit_scan_source(ph, c);
  if (out && cap > (int64_t)src.size()) {
    memcpy(out, src.data(), src.size());
    out[src.size()] = 0;
  }
  return (int64_t)src.size();
}

extern "C" int64_t obx_jit_dump_src(
    const obx_filter_desc *filter, const obx_agg_desc *agg,
    const obx_col_schema *cols, uint16_t n_cols, const uint8_t *col_flags,
    const int64_t *col_min, const int64_t *col_max,
    const uint32_t *col_maxcnt, const uint32_t *col_maxw,
    uint32_t max_block_rows, int force_v1,
    char *out, int64_t cap) {
  return obx_jit_dump_src_ex(filter, agg, cols, n_cols, col_flags, col_min,
                             col_max, col_maxcnt, col_maxw, max_block_rows,
                             force_v1, 1, 0, nullptr, out, cap);
}

/* Debug/test-only: the plan and JIT-eligibility decisions for synthetic
 * per-(block,col) class / dict-count arrays (n_blocks x n_cols, the layout
 * of obx_table_facts::col_class / col_cnt), without a GPU. Returns
 * build_plan's status when it is not OBX_SUCCESS, else 1 if the plan passes
 * jit_plan_shape + jit_blocks_ok and 0 if not. */
extern "C" int obx_jit_probe_blocks(
    const obx_filter_desc *filter, const obx_agg_desc *agg,
    const obx_col_schema *cols, uint16_t n_cols, const uint8_t *col_class,
    const uint8_t *col_cnt, uint32_t n_blocks) {
  if (!cols || !col_class || !col_cnt || n_cols > OBX_DEV_MAX_COLS)
    return OBX_INVALID_ARGUMENT;
  obx_table_facts h;
  h.n_cols = n_cols;
  h.n_blocks = n_blocks;
  memcpy(h.cols, cols, sizeof(obx_col_schema) * n_cols);
  for (size_t b = 0; b < n_blocks; b++) {
    h.col_class.insert(h.col_class.end(), col_class + b * n_cols,
                       col_class + (b + 1) * n_cols);
    h.col_cnt.insert(h.col_cnt.end(), col_cnt + b * n_cols,
                     col_cnt + (b + 1) * n_cols);
    summarize_col_classes(h);
  }
  dev_plan_hdr ph;
  dev_leaf pl[OBX_DEV_MAX_LEAVES];
  int rc = build_plan(nullptr, nullptr, h, filter, agg, ph, pl);
  if (rc != OBX_SUCCESS) return rc;
  jit_shape js;
  return jit_plan_shape(ph, js) && jit_blocks_ok(h, ph, js) ? 1 : 0;
}
