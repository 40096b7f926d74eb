/*
 * obx_facts.h — the load-time facts of one table, and the plan builder that
 * reads them. No HIP header: this is all that plan building (obx_plan.cpp),
 * the JIT generators (obx_jit_gen.cpp) and the GPU-free probes
 * (obx_probes.cpp) know of a loaded table. obx_handle (obx_host.h) derives
 * from obx_table_facts and adds the device resources and results.
 */
#ifndef OBX_FACTS_H_
#define OBX_FACTS_H_

#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#include "obx_dev.h"
#include "obx_keyset.h"

#include "../../include/obx.h"
#include "../../oracle/obx_format.h"

struct obx_table_facts {
  uint32_t n_blocks = 0;
  uint16_t n_cols = 0;
  uint64_t total_rows = 0;
  uint64_t total_bytes = 0;
  obx_col_schema cols[OBX_DEV_MAX_COLS] = {};
  uint32_t n_cus = 256; /* compute units of the owning device */

  /* ---- load-time facts (obx_fold_block, once per block) ---------------
     everything the per-query plan and JIT eligibility tests ask of the
     blocks, so a query costs O(columns), not O(blocks) */
  bool lds_ok = true;    /* all blocks 16-B aligned and <= LDS stage size */
  uint32_t max_block_rows = 0;
  uint32_t max_block_len = 0;
  /* per-(block,col) encoding summary: low nibble = decode class (0 raw,
     1 dict, 2 intdiff, 3 const, 4 slow, 5 span), bit4 = string; col_cnt =
     dict count capped at 255. Kept for the exact per-block cell product of
     a two-column grouping (jit_pair_cells_max, obx_jit_gen.cpp) */
  std::vector<uint8_t> col_class, col_cnt;
  bool col_span_any[OBX_DEV_MAX_COLS] = {};    /* class 5 in any block */
  bool col_grp16_every[OBX_DEV_MAX_COLS] = {}; /* class 1 and count < 16 in
                                                  every block */
  bool col_slow_any[OBX_DEV_MAX_COLS] = {};    /* class > 3 or string in
                                                  any block */
  uint32_t col_cnt_max[OBX_DEV_MAX_COLS] = {}; /* max of col_cnt */
  /* max over blocks of (cnt[c0]+1)*(cnt[c1]+1), filled on the first query
     that groups by (c0, c1) and whose product of column maxima exceeds the
     16-cell limit (key = c0 << 16 | c1) */
  mutable std::map<uint32_t, uint32_t> pair_cells_max;
  bool col_dict_every[OBX_DEV_MAX_COLS] = {}; /* class==1, not string, and
                                                 count<=63 in every block */
  bool col_dict_any[OBX_DEV_MAX_COLS] = {};   /* dict (incl. char) with
                                                 count<=63 in every block */
  bool col_dict_stable[OBX_DEV_MAX_COLS] = {}; /* dict_any AND the dict
                                                  payload is byte-identical
                                                  in every block (group/ref
                                                  persistence; numeric-only
                                                  uses additionally require
                                                  col_dict_every). PAX only */
  bool col_ext_any[OBX_DEV_MAX_COLS] = {};  /* HAS_EXT in any block */
  bool col_raw8_every[OBX_DEV_MAX_COLS] = {}; /* 8-B RAW, 64-bit-aligned,
                                                 no ext, in every block */
  bool col_rangefam_every[OBX_DEV_MAX_COLS] = {}; /* RAW numeric / INTDIFF
                                                     (packed-range lowerable)
                                                     in every block */
  uint32_t col_maxcnt[OBX_DEV_MAX_COLS] = {}; /* max dict count, uncapped */
  uint32_t col_maxw[OBX_DEV_MAX_COLS] = {};   /* max packed width (bits)
                                                 across blocks; 255 = no
                                                 packed stream (slow enc) */
  bool col_bdesc_unfit[OBX_DEV_MAX_COLS] = {}; /* a count or width of some
                                                  block does not fit an
                                                  obx_bdesc slot: plans that
                                                  read the column keep the
                                                  dev_block path */

  /* host summary of the stored skip index (obx_finish_load reduces the
     per-(block,col) [min,max] that k_col_minmax captured): feeds the JIT's
     i64-accumulator range eligibility, obx_jit_scan.inc */
  int64_t col_min[OBX_DEV_MAX_COLS] = {};   /* global over blocks */
  int64_t col_max[OBX_DEV_MAX_COLS] = {};
  bool col_known[OBX_DEV_MAX_COLS] = {};    /* bounds known in EVERY block */
};

/* ---- the plan builder (obx_plan.cpp) ------------------------------------ */

/* fold one parsed block into every per-column and per-table fact */
void obx_fold_block(obx_table_facts &h, const dev_block &db);

/* fold the newest block's row of col_class / col_cnt into the per-column
   facts build_plan and jit_blocks_ok test. obx_fold_block appends that row
   from a parsed block; the GPU-free probes append synthetic ones. */
void summarize_col_classes(obx_table_facts &h);

/* how build_plan turns the set id of an OBX_OP_IN_SET leaf into the set's
   device view: null = no such set. The engine looks the id up in its
   context (arg); the GPU-free probes have no sets and pass a null resolver,
   and such a leaf is then an unknown id. */
typedef const obx_keyset_dev *(*obx_set_resolver)(const void *arg,
                                                  int64_t set_id);

/* build plan header + device leaves (pure: no HIP calls) */
int build_plan(obx_set_resolver resolve, const void *resolve_arg,
               const obx_table_facts &h, const obx_filter_desc *filter,
               const obx_agg_desc *agg, dev_plan_hdr &ph,
               dev_leaf pl[OBX_DEV_MAX_LEAVES]);

#endif /* OBX_FACTS_H_ */
