/*
 * obx_jit.h — what the engine (obx_jit_rt.cpp) and the GPU-free probes
 * (obx_probes.cpp) call of the JIT generators (obx_jit_gen.cpp): the plan
 * shape, the strategies a generator takes, and choose / key / source per
 * kernel. No HIP header; everything here reads a table through
 * obx_table_facts. The compiled side (jit_entry, jit_prepare, jit_launch) is
 * in obx_host.h.
 */
#ifndef OBX_JIT_H_
#define OBX_JIT_H_

#include <string>

#include "obx_facts.h"

struct jit_shape {
  int n_vc = 0;
  uint8_t vcol[4] = {0xFF, 0xFF, 0xFF, 0xFF}; /* schema column indices */
  int n_wa = 0;
  uint8_t agg_wa[OBX_DEV_MAX_AGGS] = {}; /* 0xFF = COUNT(*) */
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

/* all the v1 kernel takes beyond the plan: the waves-per-block floor. 7
   WGs/CU measured best for the Q1/Q6 shapes (LDS ~22 KB, ~72 VGPRs);
   OBX_JIT_WPB overrides for experiments (read by jit_scan_choose, pasted
   as given) */
struct jit_v1_strategy {
  std::string wpb = "7";
};

struct jit_vtab {          /* per-block LDS value table over dict refs */
  uint8_t vc = 0;          /* value-col slot (js.vcol index) */
  uint8_t kind = 0;        /* 0 ident, 1 (one - e), 2 (one + e) */
  int64_t one = 0;
  uint32_t dim = 0;        /* maxcnt + 1 */
};

/* per-aggregate slot ids of a strategy: -1 = none */
struct jit_agg_ids {
  int8_t v[OBX_DEV_MAX_AGGS];
  jit_agg_ids() { for (int8_t &x : v) x = -1; }
  int8_t &operator[](size_t a) { return v[a]; }
  const int8_t &operator[](size_t a) const { return v[a]; }
};

struct jit_strategy {
  bool ok = false;
  uint8_t vmode[4] = {};     /* JV_CTX / JV_REF per value col */
  uint8_t vext[4] = {};      /* CTX col can be NULL (ext) in some block */
  uint8_t vraw8[4] = {};     /* CTX col is aligned 8-B RAW in every block */
  uint32_t vdim[4] = {};     /* REF: maxcnt+1 */
  uint8_t astrat[OBX_DEV_MAX_AGGS] = {};
  jit_agg_ids wa64;    /* JA_I64*: wacc64 slot */
  jit_agg_ids amm;     /* JA_MM: wmm slot */
  int n_mm = 0;
  jit_agg_ids ahist;   /* JA_HIST/HCOUNT: hist id */
  jit_agg_ids atab_b;  /* product b operand: table id or -1 */
  jit_agg_ids atab_c;  /* product c operand: table id or -1 */
  jit_agg_ids aval_a;  /* a operand: value-col slot or -1 */
  jit_agg_ids atab_a;  /* a operand via ident table: id or -1 */
  int n_w64 = 0;
  int n_hist = 0;
  uint8_t hist_vc[4] = {};   /* hist id -> value-col slot */
  int8_t hist_tab[4] = {};   /* hist id -> ident table id (entry weights) */
  uint32_t hist_off[4] = {}; /* u32 offsets into the shared hist array */
  uint32_t hist_total = 0;   /* total u32 slots */
  int n_tab = 0;
  jit_vtab tabs[6] = {};
  uint8_t leaf_inline = 0;   /* ALL leaves inline-evaluable in the sweep */
  uint8_t leaf_kind[8] = {}; /* JL_RANGE or JL_MASK */
  uint16_t leaf_cols[8] = {};
  uint8_t r = 1;             /* rows per lane (strip mining) */
  uint8_t stripes = 4;       /* i64 accumulator lane stripes */
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
  jit_agg_ids jws_f0;                       /* flush factor tab / axis0 */
  jit_agg_ids jws_f1;                       /* flush factor tab / axis1 */
  /* row count packed into the joint cell: when the weight is proven
     non-negative, never NULL, and its sum over the rows one workgroup can
     sweep stays below 2^jws_shift, each row adds weight + (1 << jws_shift),
     so a cell carries its row count above the weight sum. A joint-axis
     column then needs no histogram of its own: the aggregates that read
     one (SUM, COUNT(col), MIN/MAX) take the counts of their axis
     (jws_cax) at flush, weighted through the ident table jws_ctab */
  uint8_t jws_pack = 0;
  uint8_t jws_shift = 0;
  jit_agg_ids jws_cax;                      /* 0 / 1: counts along that axis */
  jit_agg_ids jws_ctab;                     /* ident table of that axis col */
  /* narrowed PROD3: when the weight is a CTX column proven in [0, 2^32)
     and both dict factors are proven non-negative with a product below
     2^32, the per-row term is ONE u32 x u32 -> u64 multiply against a
     combined LDS table vtc[xb][xc] = (one_b - eb) * (one_c + ec), instead
     of two 64 x 64 multiplies over two table reads */
  int8_t ctab_agg = -1;
  uint32_t ctab_db = 0, ctab_dc = 0;
  uint32_t lds_bytes = 0;
  int wpb = 7;
  /* per-block geometry from the packed descriptor (obx_bdesc) instead of
     dev_block; bd_cols is the descriptor's column list, need_cols then the
     leaf columns not among them */
  uint8_t bdesc = 0;
  obx_bdesc_cols bd_cols = {};
};

struct jit_fstrategy {
  uint8_t leaf_kind[4] = {};  /* JL_RANGE, JL_MASK, or JL_SET: key set on a
                                 packed-range column */
  uint8_t leaf_form[4] = {};  /* JL_SET: OBX_KS_* form of the set */
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

/* Which scan kernel a plan gets, and everything its generator takes: the
   one sequence shape -> blocks -> strategy -> v1 or v2 behind both
   jit_prepare and the dump probe (obx_jit_dump_src_ex). */
struct jit_scan_choice {
  int kind = 0; /* 0 = no generated kernel, 1 = v1, 2 = v2 (persistent) */
  jit_shape js;
  jit_strategy st;    /* kind 2 */
  jit_v1_strategy v1; /* kind 1 */
};

/* ---- eligibility and launch geometry ------------------------------------ */
bool jit_plan_shape(const dev_plan_hdr &ph, jit_shape &js);
bool jit_blocks_ok(const obx_table_facts &h, const dev_plan_hdr &ph,
                   const jit_shape &js);
uint32_t jit_grid_for(uint32_t n_blocks, uint32_t n_cus, int wpb);

/* ---- the scan kernel: choice, cache key, source -------------------------- */
int jit_scan_choose(const obx_table_facts &h, const dev_plan_hdr &ph,
                    const dev_leaf *pl, bool force_v1, jit_scan_choice &c);
std::string jit_scan_key(const dev_plan_hdr &ph, const jit_scan_choice &c);
std::string jit_scan_source(const dev_plan_hdr &ph, const jit_scan_choice &c);
int jit_joint_form_of(const jit_strategy &st);

/* ---- the filter kernel: strategy, cache key, source ---------------------- */
bool jit_build_fstrategy(const obx_table_facts &h, const dev_plan_hdr &ph,
                         const dev_leaf *pl, jit_fstrategy &st);
std::string jit_fstrategy_sig(const dev_plan_hdr &ph, const jit_fstrategy &st);
std::string jit_gen_source_filter(const dev_plan_hdr &ph,
                                  const jit_fstrategy &st);

#endif /* OBX_JIT_H_ */
