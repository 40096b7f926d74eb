/*
 * obx_host.h — what the host translation units that call HIP share
 * (obx_engine.cpp, obx_pax_load.cpp, obx_cs_load.cpp, obx_jit_rt.cpp and the
 * host halves of the .hip files): the kernel entry points, the loaded-table
 * handle and its context, the load steps both loaders run, and the hipRTC
 * half of the JIT. The HIP-free units (obx_plan.cpp, obx_jit_gen.cpp,
 * obx_probes.cpp) see obx_facts.h and obx_jit.h only. Private to csrc/; the
 * public C-ABI is include/obx.h.
 */
#ifndef OBX_HOST_H_
#define OBX_HOST_H_

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <map>
#include <memory>
#include <vector>

#include "obx_dev.h"
#include "obx_facts.h"
#include "obx_grouphash.h"
#include "obx_keymap.h"
#include "obx_keyset.h"
#include "obx_project.h"

#define OBX_WG_HOST 256 /* must match the kernels' WG */

#include "../../include/obx.h"
#include "../../oracle/obx_format.h"

/* kernels (obx_kernels.hip) */
extern "C" __global__ void k_decode_lds(
    const uint8_t *, const dev_block *, uint32_t, uint32_t, uint32_t,
    uint8_t *, uint8_t *);
extern "C" __global__ void k_decode_multi(
    const uint8_t *, const dev_block *, uint32_t, const uint16_t *,
    const uint8_t *, uint32_t, uint8_t *const *, uint8_t *const *);
extern "C" __global__ void k_scan_agg_direct(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, gslot *, unsigned long long *);
extern "C" __global__ void k_scan_filter_agg(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, gslot *, unsigned long long *);
extern "C" __global__ void k_scan_filter_agg_lds(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, gslot *, unsigned long long *);
extern "C" __global__ void k_filter(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, uint64_t *, int32_t *, uint32_t *,
    unsigned long long *);
extern "C" __global__ void k_filter_lds(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, uint64_t *, int32_t *, uint32_t *,
    unsigned long long *);
/* _prog variants: compiled with the postfix AND/OR combine-program path
   (reference: ObPushdownFilterExecutor AND/OR trees); separate entry points
   so the AND-only fast path keeps its lean register budget. */
extern "C" __global__ void k_scan_filter_agg_prog(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, gslot *, unsigned long long *);
extern "C" __global__ void k_scan_filter_agg_prog_lds(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, gslot *, unsigned long long *);
extern "C" __global__ void k_filter_prog(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, uint64_t *, int32_t *, uint32_t *,
    unsigned long long *);
extern "C" __global__ void k_filter_prog_lds(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, uint64_t *, int32_t *, uint32_t *,
    unsigned long long *);
extern "C" __global__ void k_decode(
    const uint8_t *, const dev_block *, uint32_t, uint32_t, uint32_t,
    uint8_t *, uint8_t *);
extern "C" __global__ void k_group_pass(
    const uint8_t *, const dev_block *, uint32_t, const dev_plan_hdr,
    const uint64_t *, uint8_t *, gslot *, unsigned long long *);
extern "C" __global__ void k_agg_pass(
    const uint8_t *, const dev_block *, uint32_t, const dev_plan_hdr,
    uint32_t, const uint64_t *, const uint8_t *, gslot *);
extern "C" __global__ void k_lower_leaves(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *, uint32_t,
    uint32_t, const int64_t *, blk_leaf *);
extern "C" __global__ void k_col_minmax(
    const uint8_t *, const dev_block *, uint32_t, uint32_t, int64_t *);
extern "C" __global__ void k_gtable_init(
    unsigned long long *, uint32_t, uint32_t, uint32_t, uint32_t);
extern "C" __global__ void k_pack_bdesc(const dev_block *, uint32_t,
                                        const obx_bdesc_cols, obx_bdesc *);
static_assert(sizeof(obx_bdesc) == 128 && alignof(obx_bdesc) == 128 &&
                  offsetof(obx_bdesc, slot) == 16,
              "k_pack_bdesc writes obx_bdesc as 16 u64 words");

/* filtered projection (obx_project.hip) */
extern "C" __global__ void k_project_tile_sums(const uint32_t *, uint32_t,
                                               uint64_t *);
extern "C" __global__ void k_project_offsets(const uint32_t *, uint32_t,
                                             const uint64_t *, uint64_t *);
extern "C" __global__ void k_project_sel(
    const uint8_t *, const dev_block *, uint32_t, const int32_t *,
    const uint32_t *, const uint64_t *, const proj_args, uint8_t *,
    uint64_t *, uint64_t);
extern "C" __global__ void k_project_sel_lds(
    const uint8_t *, const dev_block *, uint32_t, const int32_t *,
    const uint32_t *, const uint64_t *, const proj_args, uint8_t *,
    uint64_t *, uint64_t);
extern "C" __global__ void k_project_pack_nulls(const uint8_t *, uint64_t,
                                                uint64_t, uint32_t, uint8_t *);

/* key-set and key-map build (obx_keys.hip): one minmax body and one insert
   body behind two entries each. Keys are the non-null datums of a dense
   vector of len-byte datums; nulls == nullptr = none are null. Both builds
   use one scratch of 7 words; a set's kernels touch the first five: 0 min,
   1 max, 2 non-null keys, 3 distinct keys, 4 hash marker flag. */
extern "C" __global__ void k_keyset_minmax(
    const uint8_t *, uint32_t, uint32_t, const uint8_t *, uint32_t, uint64_t,
    unsigned long long *);
extern "C" __global__ void k_keyset_insert(
    const uint8_t *, uint32_t, uint32_t, const uint8_t *, uint32_t, uint64_t,
    uint64_t *, uint64_t, int64_t, uint32_t, uint32_t, unsigned long long *);

/* the map's entries: a payload vector next to the key vector. A row whose
   key is NULL (bit key_bit of its nulls byte) is skipped. Its scratch words
   go on: 5 the marker's payload, 6 non-null keys whose payload is NULL (bit
   pay_bit). */
extern "C" __global__ void k_keymap_minmax(
    const uint8_t *, uint32_t, uint32_t, const uint8_t *, uint32_t, uint32_t,
    uint64_t, unsigned long long *);
extern "C" __global__ void k_keymap_insert(
    const uint8_t *, uint32_t, uint32_t, const uint8_t *, uint32_t, uint32_t,
    const uint8_t *, uint32_t, uint64_t, uint64_t *, uint64_t *, uint64_t,
    int64_t, uint32_t, uint32_t, unsigned long long *);

/* join scan (obx_join.hip): the fused scan kernels with the probe step */
extern "C" __global__ void k_scan_join_agg(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, const dev_join, gslot *,
    unsigned long long *);
extern "C" __global__ void k_scan_join_agg_lds(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, const dev_join, gslot *,
    unsigned long long *);
extern "C" __global__ void k_scan_join_agg_prog(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, const dev_join, gslot *,
    unsigned long long *);
extern "C" __global__ void k_scan_join_agg_prog_lds(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, const dev_join, gslot *,
    unsigned long long *);
extern "C" __global__ void k_scan_join_agg_direct(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, const dev_join, gslot *,
    unsigned long long *);

/* the sized group table (obx_grouphash.h): the growth-path body on it, its
   init, and the compaction of its live slots into records */
extern "C" __global__ void k_scan_agg_hash(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, const obx_gh_dev, uint64_t,
    unsigned long long *);
extern "C" __global__ void k_scan_join_agg_hash(
    const uint8_t *, const dev_block *, uint32_t, const dev_leaf *,
    const blk_leaf *, const dev_plan_hdr, const dev_join, const obx_gh_dev,
    uint64_t, unsigned long long *);
extern "C" __global__ void k_group_hash_init(const obx_gh_dev,
                                             unsigned long long *, uint32_t,
                                             uint32_t);
extern "C" __global__ void k_group_compact(const obx_gh_dev,
                                           unsigned long long *,
                                           unsigned long long *, uint64_t);

#define HIP_TRY(x)                                        \
  do {                                                    \
    hipError_t _e = (x);                                  \
    if (_e != hipSuccess) {                               \
      fprintf(stderr, "obx: HIP error %s at %s:%d\n",     \
              hipGetErrorString(_e), __FILE__, __LINE__); \
      return OBX_INTERNAL_ERROR;                          \
    }                                                     \
  } while (0)

/* device memory that lives no longer than its scope (loader staging) */
template <class T>
struct dev_tmp {
  T *p = nullptr;
  dev_tmp() = default;
  dev_tmp(const dev_tmp &) = delete;
  dev_tmp &operator=(const dev_tmp &) = delete;
  ~dev_tmp() { if (p) (void)hipFree(p); }
};

/* One loaded table: its load-time facts (obx_facts.h; all the plan builder
   and the JIT generators see of it) and, below, its device resources and
   results. Owns every device pointer below: ~obx_handle is the one place
   they are released, so a handle is never copied and lives behind a
   unique_ptr from the loader's first allocation to free / close. */
struct obx_handle : obx_table_facts {
  obx_handle() = default;
  obx_handle(const obx_handle &) = delete;
  obx_handle &operator=(const obx_handle &) = delete;
  ~obx_handle();

  uint8_t *d_buf = nullptr;
  dev_block *d_blocks = nullptr;
  /* query scratch */
  blk_leaf *d_bleaves = nullptr;
  uint32_t bleaves_cap = 0; /* in (block,leaf) entries */
  dev_leaf *d_pleaves = nullptr;
  gslot *d_gtable = nullptr;
  unsigned long long *d_counters = nullptr; /* tail of d_gtable */
  uint64_t *d_bitmap = nullptr;
  int32_t *d_row_ids = nullptr;
  uint32_t *d_blk_counts = nullptr;
  uint8_t *d_row_slot = nullptr;
  uint8_t *d_decode_out[OBX_DEV_MAX_COLS] = {};
  uint64_t last_survivors = 0;
  gslot *d_gtable_big = nullptr; /* high-cardinality direct kernel table */
  /* the sized group table of a scan past OBX_GTABLE_BIG groups: its counter
     block (OBX_GH_COUNTER_WORDS) then the table, in one allocation that
     grows only when a scan needs more; the compacted records next to it,
     and where they land on the host. Pageable, not pinned: the copy is
     followed at once by a sort of the same records that costs more, and a
     grant of 2^24 groups would otherwise pin gigabytes. */
  uint8_t *d_ghash = nullptr;
  uint64_t ghash_cap = 0; /* bytes */
  uint8_t *d_grecs = nullptr;
  uint64_t grecs_cap = 0; /* bytes */
  std::vector<unsigned long long> h_grecs;
  void *d_proj_scratch = nullptr; /* k_decode_multi proj/len/out arrays */
  /* result of the last obx_gpu_scan_project: dense vectors per projected
     position, one byte of null flags per row (bit p = position p), row
     numbers if asked. The buffers grow only when a result needs more and
     are kept across calls; sel_n_proj == 0 = no result to fetch. */
  uint8_t *d_sel_out[OBX_DEV_MAX_COLS] = {};
  uint64_t sel_out_cap[OBX_DEV_MAX_COLS] = {}; /* bytes */
  uint8_t *d_sel_nulls = nullptr;
  uint64_t *d_sel_row_nos = nullptr;
  uint64_t sel_nulls_cap = 0, sel_row_nos_cap = 0; /* rows */
  uint64_t *d_blk_off = nullptr;   /* n_blocks + 1 exclusive block offsets */
  uint64_t *d_tile_sums = nullptr; /* per-tile sums of that scan */
  uint8_t *d_sel_bits = nullptr;   /* a fetch window's packed null bits */
  uint64_t sel_bits_cap = 0;       /* bytes */
  uint16_t sel_cols[OBX_DEV_MAX_COLS] = {};
  uint16_t sel_n_proj = 0;
  bool sel_has_row_nos = false;
  uint64_t sel_rows = 0;
  std::vector<obx_group_row> last_rows; /* full sorted group rows of the
                                           last scan (obx_gpu_agg_fetch) */

  /* packed per-block descriptors of the persistent scan JIT, one array of
     n_blocks records per ordered column list, built by the first query
     that needs the list (bdesc_get, obx_engine.cpp). At most
     OBX_BDESC_SETS arrays; the oldest is evicted. */
#define OBX_BDESC_SETS 4
  struct bdesc_set {
    obx_bdesc_cols cols = {};
    obx_bdesc *d = nullptr;
    uint64_t born = 0; /* build order: the smallest is evicted */
  } bdesc[OBX_BDESC_SETS];
  uint64_t bdesc_builds = 0;

  /* stored skip index: per-(block,col) [min,max] of non-null decoded
     values, captured by k_col_minmax at load (feeds k_lower_leaves pruning;
     its host summary is obx_table_facts::col_min / col_max / col_known) */
  int64_t *d_minmax = nullptr;
};

/* One device-resident key set (obx_keyset.h). Owns its table; lives behind a
   unique_ptr in the context from build to free / close, like a handle. */
struct obx_keyset {
  obx_keyset() = default;
  obx_keyset(const obx_keyset &) = delete;
  obx_keyset &operator=(const obx_keyset &) = delete;
  ~obx_keyset() { if (d_words) (void)hipFree(d_words); }

  uint64_t *d_words = nullptr;
  obx_keyset_dev view = {};  /* what a set leaf carries to the kernels */
  obx_keyset_info info = {};
};

/* One device-resident key map (obx_keymap.h): the table and, for the dense
   form, the presence bitmap behind it in one allocation. Same lifetime rule
   as a key set. */
struct obx_keymap {
  obx_keymap() = default;
  obx_keymap(const obx_keymap &) = delete;
  obx_keymap &operator=(const obx_keymap &) = delete;
  ~obx_keymap() { if (d_table) (void)hipFree(d_table); }

  uint64_t *d_table = nullptr;
  obx_keymap_dev view = {}; /* what a join scan carries to the kernels */
  obx_keymap_info info = {};
};

struct obx_gpu_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  hipEvent_t ev_p0 = nullptr, ev_p1 = nullptr;
  hipEvent_t ev_mid = nullptr; /* scan_project: offsets done, gather next */
  hipEvent_t ev_b0 = nullptr, ev_b1 = nullptr; /* around a k_pack_bdesc */
  bool bdesc_built = false;   /* the running scan queued that build */
  double last_ms = 0.0;
  double last_prep_ms = 0.0;  /* plan upload + per-block filter lowering */
  int last_jit = 0;           /* last scan used the specialized kernel */
  int last_bdesc = 0;         /* ... and it read the packed descriptors */
  int last_joint = 0;         /* ... and its joint-table form (0 = none) */
  /* device times of the last scan_project: filter, block offsets, gather */
  double last_proj_ms[3] = {0.0, 0.0, 0.0};
  uint32_t last_grid = 0;     /* workgroups that kernel was launched with */
  /* most distinct groups a scan may produce (obx_gpu_set_max_groups) */
  uint64_t max_groups = OBX_GTABLE_BIG;
  uint64_t last_group_slots = 0; /* sized table of the last scan, 0 = none */
  double last_group_ms = 0.0;    /* device time of that table's scan kernel */
  uint32_t n_cus = 256;
  /* pinned landing buffer for the group table + counters of a scan (sized
     for the growth-path table) */
  uint8_t *h_result = nullptr;
  /* a handle's id is its index here: never reused, null once freed */
  std::vector<std::unique_ptr<obx_handle>> handles;
  /* key sets, same rule: a set's id is its index, null once freed */
  std::vector<std::unique_ptr<obx_keyset>> keysets;
  /* key maps, same rule */
  std::vector<std::unique_ptr<obx_keymap>> keymaps;
};

/* every use of a set id resolves it here (obx_keys.hip): null for a null
   context, an id out of range, or a freed set. No HIP call. */
const obx_keyset *obx_keyset_lookup(const obx_gpu_ctx *ctx, int64_t set_id);
/* the same for a map id */
const obx_keymap *obx_keymap_lookup(const obx_gpu_ctx *ctx, int64_t map_id);
/* every verb resolves its handle id here (obx_engine.cpp): null for a null
   context, an id out of range, or a freed handle */
obx_handle *obx_handle_lookup(obx_gpu_ctx *ctx, int handle);

static inline uint32_t grid_for(uint32_t n_blocks) {
  uint32_t g = n_blocks < 4096u ? n_blocks : 4096u;
  return g ? g : 1;
}

/* ---- loading: host half, arena upload, finish ---------------------------
   A loader (obx_pax_load.cpp, obx_cs_load.cpp) parses its format into
   dev_blocks without a HIP call, folding each into the handle's facts
   (obx_fold_block, obx_plan.cpp); uploads h->d_buf in its own way (PAX: a
   copy, CS: k_cs_decode); and hands the handle to obx_finish_load
   (obx_engine.cpp). */

/* upload the descriptors, allocate the query scratch, capture the min/max
   skip index, and publish the handle: returns its id, or a negative status
   (the handle and all it holds are then released) */
int obx_finish_load(obx_gpu_ctx *ctx, std::unique_ptr<obx_handle> h,
                    const std::vector<dev_block> &blocks);

/* the loaders' host halves: schema checks + parse + fold, no HIP call */
int obx_pax_host_load(const obx_blockset *bs, obx_table_facts &h,
                      std::vector<dev_block> &blocks);
struct obx_cs_plan; /* device decode tasks (obx_cs_load.cpp) */
int obx_cs_host_load(const obx_blockset *bs, obx_table_facts &h,
                     std::vector<dev_block> &blocks,
                     obx_cs_plan *plan /* null: facts only */);

/* ---- the hipRTC half of the JIT (obx_jit_rt.cpp) ------------------------
   What a verb holds of a generated kernel. Entries belong to the process-wide
   compile cache and are never changed or released once made, so the pointer
   stays good for the life of the process. The generators and everything
   HIP-free about them are in obx_jit.h. */
struct jit_entry {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  int kind = 0; /* scan: 1 = v1 generator, 2 = v2 (persistent) */
  int wpb = 0; /* v2: workgroups per CU the launch grid is sized to */
  bool bdesc = false;        /* v2: reads the packed block descriptors ... */
  obx_bdesc_cols bd_cols = {}; /* ... of this ordered column list */
  int joint = 0;             /* v2: joint-table form (obx_gpu_last_joint) */
};

/* prepare (compile/lookup) before the timed region, for the device the
   caller made current; nullptr = use the precompiled kernels */
const jit_entry *jit_prepare(int device, const obx_table_facts &h,
                             const dev_plan_hdr &ph, const dev_leaf *pl);
const jit_entry *jit_prepare_filter(int device, const obx_table_facts &h,
                                    const dev_plan_hdr &ph, const dev_leaf *pl,
                                    int want_row_ids);
int jit_launch(const jit_entry *je, obx_handle &h, const obx_bdesc *bd,
               hipStream_t stream, uint32_t *grid_out);

#endif /* OBX_HOST_H_ */
