/*
 * obx_engine.cpp — MI355X product engine host side (C-ABI of include/obx.h).
 *
 * Replaces the reference's scan driver around the microblock reader
 * (ObSSTableRowScanner / ObMicroBlockRowScanner / ObVectorStore,
 * /root/reference/src/storage/access/ob_sstable_row_scanner.cpp:557-598,
 * ob_vector_store.cpp:329-389): microblocks are staged to HBM once, block
 * headers are parsed ONCE into flat device descriptors (the reference caches
 * per-column decoders the same way, ob_micro_block_decoder.cpp:440-480), and
 * the per-query work is pure GPU kernels (obx_kernels.hip).
 *
 * This is the PRODUCT path: it fails loudly (OBX_NO_GPU) when no HIP device
 * is present — it never falls back to the CPU oracle.
 */
#include <cstdlib>
#include <cstring>
#include <algorithm>

#include "obx_host.h"

/* device words after the group table that hold the 16 scan counters: one
   allocation, so one copy fetches both */
#define OBX_RESULT_BYTES(slots) (sizeof(gslot) * (slots) + 16 * 8)

extern "C" int obx_gpu_open(int device, obx_gpu_ctx **out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= device) return OBX_NO_GPU;
  auto *ctx = new obx_gpu_ctx();
  ctx->device = device;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&ctx->stream));
  HIP_TRY(hipEventCreate(&ctx->ev_start));
  HIP_TRY(hipEventCreate(&ctx->ev_stop));
  HIP_TRY(hipEventCreate(&ctx->ev_p0));
  HIP_TRY(hipEventCreate(&ctx->ev_p1));
  HIP_TRY(hipEventCreate(&ctx->ev_mid));
  HIP_TRY(hipEventCreate(&ctx->ev_b0));
  HIP_TRY(hipEventCreate(&ctx->ev_b1));
  {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (prop.multiProcessorCount > 0)
      ctx->n_cus = (uint32_t)prop.multiProcessorCount;
  }
  HIP_TRY(hipHostMalloc((void **)&ctx->h_result,
                        OBX_RESULT_BYTES(OBX_GTABLE_BIG), hipHostMallocDefault));
  *out = ctx;
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_close(obx_gpu_ctx *ctx) {
  if (!ctx) return OBX_SUCCESS;
  (void)hipSetDevice(ctx->device);
  ctx->handles.clear(); /* ~obx_handle, while the device is current */
  ctx->keysets.clear();
  ctx->keymaps.clear();
  (void)hipStreamDestroy(ctx->stream);
  for (hipEvent_t ev : {ctx->ev_start, ctx->ev_stop, ctx->ev_p0, ctx->ev_p1,
                        ctx->ev_mid, ctx->ev_b0, ctx->ev_b1})
    (void)hipEventDestroy(ev);
  (void)hipHostFree(ctx->h_result);
  delete ctx;
  return OBX_SUCCESS;
}

/* the one place a handle's device memory is released (d_counters is the
   tail of d_gtable). A handle whose load failed early holds only nulls and
   makes no HIP call. */
obx_handle::~obx_handle() {
  void *owned[] = {d_buf, d_blocks, d_bleaves, d_pleaves, d_gtable,
                   d_gtable_big, d_ghash, d_grecs, d_proj_scratch, d_bitmap, d_row_ids,
                   d_blk_counts, d_row_slot, d_minmax, d_sel_nulls,
                   d_sel_row_nos, d_blk_off, d_tile_sums, d_sel_bits};
  for (void *p : owned)
    if (p) (void)hipFree(p);
  for (uint8_t *p : d_decode_out)
    if (p) (void)hipFree(p);
  for (uint8_t *p : d_sel_out)
    if (p) (void)hipFree(p);
  for (bdesc_set &s : bdesc)
    if (s.d) (void)hipFree(s.d);
}

/* every verb resolves its handle id here: null for a null context, an id
   out of range, or a freed handle */
obx_handle *obx_handle_lookup(obx_gpu_ctx *ctx, int handle) {
  if (!ctx || handle < 0 || handle >= (int)ctx->handles.size()) return nullptr;
  return ctx->handles[handle].get();
}

/* device-side fill of an empty group table (EMPTY keys, zero cells, MIN/MAX
   sentinels by aggregate mask) and of the tail_words counters behind it */
static void gtable_init(gslot *gt, uint32_t n_slots, uint32_t tail_words,
                        uint32_t min_mask, uint32_t max_mask,
                        hipStream_t stream) {
  const uint32_t words =
      n_slots * (uint32_t)(sizeof(gslot) / 8) + tail_words;
  hipLaunchKernelGGL(k_gtable_init, dim3((words + OBX_WG_HOST - 1) / OBX_WG_HOST),
                     dim3(OBX_WG_HOST), 0, stream, (unsigned long long *)gt,
                     n_slots, tail_words, min_mask, max_mask);
}

int obx_finish_load(obx_gpu_ctx *ctx, std::unique_ptr<obx_handle> h,
                    const std::vector<dev_block> &blocks) {
  h->n_cus = ctx->n_cus;
  HIP_TRY(hipMalloc(&h->d_blocks, sizeof(dev_block) * blocks.size()));
  HIP_TRY(hipMemcpy(h->d_blocks, blocks.data(),
                    sizeof(dev_block) * blocks.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&h->d_gtable, OBX_RESULT_BYTES(OBX_GTABLE_SLOTS)));
  h->d_counters = (unsigned long long *)(h->d_gtable + OBX_GTABLE_SLOTS);
  HIP_TRY(hipMalloc(&h->d_pleaves, sizeof(dev_leaf) * OBX_DEV_MAX_LEAVES));

  /* stored skip index: capture per-(block,col) min/max once at load
     (k_col_minmax; outside every timed region) and summarize per column
     for the JIT's range eligibility */
  const uint32_t nb = h->n_blocks, nc = h->n_cols;
  const uint64_t nmm = (uint64_t)nb * nc * 2;
  HIP_TRY(hipMalloc(&h->d_minmax, nmm * sizeof(int64_t)));
  hipLaunchKernelGGL(k_col_minmax, dim3(grid_for(nb)), dim3(OBX_WG_HOST), 0,
                     nullptr, h->d_buf, h->d_blocks, nb, nc, h->d_minmax);
  std::vector<int64_t> mm(nmm);
  HIP_TRY(hipMemcpy(mm.data(), h->d_minmax, nmm * sizeof(int64_t),
                    hipMemcpyDeviceToHost));
  for (uint32_t c = 0; c < nc; c++) {
    int64_t gmin = INT64_MAX, gmax = INT64_MIN;
    bool known = true;
    for (uint32_t b = 0; b < nb; b++) {
      int64_t mn = mm[2 * ((uint64_t)b * nc + c)];
      int64_t mx = mm[2 * ((uint64_t)b * nc + c) + 1];
      if (mn == INT64_MIN && mx == INT64_MAX) { known = false; break; }
      if (mn <= mx) { /* empty (all-null) blocks don't widen */
        if (mn < gmin) gmin = mn;
        if (mx > gmax) gmax = mx;
      }
    }
    h->col_known[c] = known;
    h->col_min[c] = gmin;
    h->col_max[c] = gmax;
  }
  ctx->handles.push_back(std::move(h));
  return (int)ctx->handles.size() - 1;
}

extern "C" int obx_gpu_free_blocks(obx_gpu_ctx *ctx, int handle) {
  if (!obx_handle_lookup(ctx, handle)) return OBX_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->handles[handle].reset();
  return OBX_SUCCESS;
}

/* build_plan's resolver: the device view of one of the context's key sets */
static const obx_keyset_dev *set_view_of(const void *ctx, int64_t set_id) {
  const obx_keyset *ks = obx_keyset_lookup((const obx_gpu_ctx *)ctx, set_id);
  return ks ? &ks->view : nullptr;
}

/* build the plan + upload leaves + lower per-block tests on device */
static int prep_query(obx_gpu_ctx *ctx, obx_handle &h,
                      const obx_filter_desc *filter, const obx_agg_desc *agg,
                      dev_plan_hdr &ph, dev_leaf *pl_out = nullptr) {
  dev_leaf pl[OBX_DEV_MAX_LEAVES];
  int rc = build_plan(set_view_of, ctx, h, filter, agg, ph, pl);
  if (pl_out) memcpy(pl_out, pl, sizeof(pl));
  if (rc != OBX_SUCCESS) return rc;
  uint16_t nl = ph.n_leaves;
  /* upload plan leaves + lower per-block tests on device */
  HIP_TRY(hipEventRecord(ctx->ev_p0, ctx->stream));
  HIP_TRY(hipMemcpyAsync(h.d_pleaves, pl, sizeof(pl), hipMemcpyHostToDevice,
                         ctx->stream));
  if (nl > 0) {
    uint64_t needed = (uint64_t)h.n_blocks * nl;
    if (h.bleaves_cap < needed) {
      (void)hipFree(h.d_bleaves);
      h.d_bleaves = nullptr; /* a failed hipMalloc must leave no stale pair */
      h.bleaves_cap = 0;
      HIP_TRY(hipMalloc(&h.d_bleaves, needed * sizeof(blk_leaf)));
      h.bleaves_cap = needed;
    }
    uint32_t total = (uint32_t)needed;
    uint32_t grid = (total + OBX_WG_HOST - 1) / OBX_WG_HOST;
    hipLaunchKernelGGL(k_lower_leaves, dim3(grid), dim3(OBX_WG_HOST), 0, ctx->stream,
                       h.d_buf, h.d_blocks, h.n_blocks, h.d_pleaves, nl,
                       (uint32_t)h.n_cols, (const int64_t *)h.d_minmax,
                       h.d_bleaves);
  }
  HIP_TRY(hipEventRecord(ctx->ev_p1, ctx->stream));
  return OBX_SUCCESS;
}

/* the handle's packed descriptor array for one ordered column list (the
   persistent scan JIT's per-block metadata, obx_bdesc): served from the
   handle, or built on the stream by k_pack_bdesc into the slot of the
   oldest of OBX_BDESC_SETS arrays. The evicted array is freed with hipFree,
   which waits for the device, so no earlier scan still reads it. *built
   says whether this call queued the build. nullptr = allocation failed. */
static const obx_bdesc *bdesc_get(obx_handle &h, const obx_bdesc_cols &cols,
                                  hipStream_t stream, bool *built) {
  *built = false;
  obx_handle::bdesc_set *victim = nullptr; /* a free slot, else the oldest */
  for (obx_handle::bdesc_set &s : h.bdesc) {
    if (s.d && s.cols.n == cols.n &&
        memcmp(s.cols.c, cols.c, cols.n * sizeof(cols.c[0])) == 0)
      return s.d;
    if (!victim || (victim->d && (!s.d || s.born < victim->born)))
      victim = &s;
  }
  if (victim->d) {
    (void)hipFree(victim->d);
    victim->d = nullptr;
  }
  const uint64_t nb = h.n_blocks ? h.n_blocks : 1;
  if (hipMalloc(&victim->d, nb * sizeof(obx_bdesc)) != hipSuccess) {
    victim->d = nullptr;
    return nullptr;
  }
  victim->cols = cols;
  victim->born = ++h.bdesc_builds;
  const uint64_t words = (uint64_t)h.n_blocks * 16;
  hipLaunchKernelGGL(k_pack_bdesc,
                     dim3((uint32_t)((words + OBX_WG_HOST - 1) / OBX_WG_HOST)),
                     dim3(OBX_WG_HOST), 0, stream, h.d_blocks, h.n_blocks,
                     cols, victim->d);
  *built = true;
  return victim->d;
}

/* the plan-generic filter kernel: LDS-staged when every block fits the
   stage, the _prog build when the plan carries a combine program */
static decltype(&k_filter) generic_filter_kernel(const obx_handle &h,
                                                 const dev_plan_hdr &ph) {
  return h.lds_ok ? (ph.n_prog ? k_filter_prog_lds : k_filter_lds)
                  : (ph.n_prog ? k_filter_prog : k_filter);
}

/* close a verb's timed region: ev_stop, the optional copy of a result into
   the pinned buffer (queued before the sync, so one wait serves both), the
   sync, and the device times of the kernel and, after prep_query, the prep */
static int end_timed(obx_gpu_ctx *ctx, bool prep, const void *result = nullptr,
                     size_t result_bytes = 0) {
  HIP_TRY(hipEventRecord(ctx->ev_stop, ctx->stream));
  if (result)
    HIP_TRY(hipMemcpyAsync(ctx->h_result, result, result_bytes,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
  ctx->last_ms = ms; /* per-operator monitoring */
  if (prep) {
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_p0, ctx->ev_p1));
    ctx->last_prep_ms = ms;
    if (ctx->bdesc_built) { /* this query built a descriptor array */
      ctx->bdesc_built = false;
      HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_b0, ctx->ev_b1));
      ctx->last_prep_ms += ms;
    }
  }
  return OBX_SUCCESS;
}

/* the filter verb on a resolved handle: obx_gpu_filter, and the first step
   of obx_gpu_scan_project (with row ids) */
static int run_filter(obx_gpu_ctx *ctx, obx_handle &h,
                      const obx_filter_desc *filter, int want_row_ids) {
  HIP_TRY(hipSetDevice(ctx->device));
  dev_plan_hdr ph;
  dev_leaf plv[OBX_DEV_MAX_LEAVES];
  int rc = prep_query(ctx, h, filter, nullptr, ph, plv);
  if (rc != OBX_SUCCESS) return rc;
  ctx->last_jit = 0;
  uint64_t bm_words = (h.total_rows + 63) / 64 + 1;
  if (!h.d_bitmap) HIP_TRY(hipMalloc(&h.d_bitmap, bm_words * 8));
  HIP_TRY(hipMemsetAsync(h.d_bitmap, 0, bm_words * 8, ctx->stream));
  const bool no_bitmap = getenv("OBX_NO_BITMAP") != nullptr; /* perf A/B */
  if (want_row_ids) {
    if (!h.d_row_ids)
      HIP_TRY(hipMalloc(&h.d_row_ids, h.total_rows * sizeof(int32_t)));
    if (!h.d_blk_counts)
      HIP_TRY(hipMalloc(&h.d_blk_counts, h.n_blocks * sizeof(uint32_t)));
    /* skipped blocks (NONE verdict) write nothing: stale counts from a
       previous filter would survive (caught by the zero-survivor edge
       test) */
    HIP_TRY(hipMemsetAsync(h.d_blk_counts, 0,
                           h.n_blocks * sizeof(uint32_t), ctx->stream));
  }
  HIP_TRY(hipMemsetAsync(h.d_counters, 0, 16 * 8, ctx->stream));
  /* bitmap-only filters take the specialized wave-per-block kernel
     (direct global reads of just the leaf streams; obx_jit_filter.inc) */
  const jit_entry *fje =
      jit_prepare_filter(ctx->device, h, ph, plv, want_row_ids);
  ctx->last_jit = fje ? 2 : 0;
  HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
  if (fje) {
    /* ~1-2k WGs measured optimal: larger grids thrash concurrent DMA
       streams, and the striped-counter tail scales with grid anyway */
    uint32_t fgrid = h.n_blocks / 8;
    if (fgrid < 512) fgrid = h.n_blocks < 512 ? (h.n_blocks ? h.n_blocks : 1)
                                              : 512;
    if (fgrid > 2048) fgrid = 2048;
    if (const char *fg = getenv("OBX_JIT_FGRID")) {
      int g = atoi(fg);
      if (g > 0 && g <= 65535) fgrid = (uint32_t)g;
    }
    void *rid = want_row_ids ? (void *)h.d_row_ids : nullptr;
    void *bcn = want_row_ids ? (void *)h.d_blk_counts : nullptr;
    void *args[9] = {&h.d_buf, &h.d_blocks, &h.n_blocks, &h.d_pleaves,
                     &h.d_bleaves, &h.d_bitmap, &rid, &bcn, &h.d_counters};
    if (hipModuleLaunchKernel(fje->fn, fgrid, 1, 1,
                              OBX_WG_HOST, 1, 1, 0, ctx->stream, args,
                              nullptr) != hipSuccess)
      return OBX_INTERNAL_ERROR;
  } else {
    hipLaunchKernelGGL(generic_filter_kernel(h, ph),
                       dim3(grid_for(h.n_blocks)), dim3(OBX_WG_HOST), 0,
                       ctx->stream, h.d_buf, h.d_blocks, h.n_blocks,
                       h.d_pleaves, h.d_bleaves, ph,
                       (h.lds_ok && no_bitmap) ? nullptr : h.d_bitmap,
                       want_row_ids ? h.d_row_ids : nullptr,
                       want_row_ids ? h.d_blk_counts : nullptr, h.d_counters);
  }
  rc = end_timed(ctx, true);
  if (rc != OBX_SUCCESS) return rc;
  unsigned long long cnt[16];
  HIP_TRY(hipMemcpy(cnt, h.d_counters, 16 * 8, hipMemcpyDeviceToHost));
  /* slot 0: legacy kernels; slots 8..15: JIT filter's striped WG sums */
  h.last_survivors = cnt[0];
  for (int i2 = 8; i2 < 16; i2++) h.last_survivors += cnt[i2];
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_filter(obx_gpu_ctx *ctx, int handle,
                              const obx_filter_desc *filter,
                              int want_row_ids) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  return run_filter(ctx, *hp, filter, want_row_ids);
}

extern "C" int obx_gpu_fetch_bitmap(obx_gpu_ctx *ctx, int handle, uint8_t *out,
                                    int64_t cap) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  if (!h.d_bitmap) return OBX_INVALID_ARGUMENT;
  int64_t bytes = (int64_t)((h.total_rows + 7) / 8);
  if (cap < bytes) return OBX_BUF_NOT_ENOUGH;
  HIP_TRY(hipMemcpy(out, h.d_bitmap, bytes, hipMemcpyDeviceToHost));
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_fetch_row_ids(obx_gpu_ctx *ctx, int handle,
                                     int32_t *out, int64_t cap,
                                     uint64_t *n_out) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  if (!h.d_row_ids) return OBX_INVALID_ARGUMENT;
  if (n_out) *n_out = h.last_survivors;
  if (out) {
    if (cap < (int64_t)h.total_rows) return OBX_BUF_NOT_ENOUGH;
    HIP_TRY(hipMemcpy(out, h.d_row_ids, h.total_rows * sizeof(int32_t),
                      hipMemcpyDeviceToHost));
  }
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_fetch_blk_counts(obx_gpu_ctx *ctx, int handle,
                                        uint32_t *out, int64_t cap) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  if (!h.d_blk_counts) return OBX_INVALID_ARGUMENT;
  if (cap < (int64_t)h.n_blocks) return OBX_BUF_NOT_ENOUGH;
  HIP_TRY(hipMemcpy(out, h.d_blk_counts, h.n_blocks * 4,
                    hipMemcpyDeviceToHost));
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_decode(obx_gpu_ctx *ctx, int handle,
                              const uint16_t *proj_cols, uint16_t n_proj) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
  if (h.lds_ok && n_proj > 1 && n_proj <= OBX_DEV_MAX_COLS) {
    /* one block stage serves every projected column */
    uint16_t pc[OBX_DEV_MAX_COLS];
    uint8_t ln[OBX_DEV_MAX_COLS];
    uint8_t *po[OBX_DEV_MAX_COLS];
    for (uint16_t i = 0; i < n_proj; i++) {
      uint16_t c = proj_cols[i];
      if (c >= h.n_cols) return OBX_INVALID_ARGUMENT;
      if (!h.d_decode_out[c])
        HIP_TRY(hipMalloc(&h.d_decode_out[c], h.total_rows * h.cols[c].len));
      pc[i] = c;
      ln[i] = (uint8_t)h.cols[c].len;
      po[i] = h.d_decode_out[c];
    }
    if (!h.d_proj_scratch)
      HIP_TRY(hipMalloc(&h.d_proj_scratch,
                        OBX_DEV_MAX_COLS * (8 + 2 + 1) + 16));
    /* pointers first (8-aligned base), then u16 cols, then u8 lens */
    uint8_t *base = (uint8_t *)h.d_proj_scratch;
    uint8_t *outp = base;
    uint8_t *pcp = base + OBX_DEV_MAX_COLS * 8;
    uint8_t *lnp = pcp + OBX_DEV_MAX_COLS * 2;
    /* synchronous copies: the sources are stack arrays */
    HIP_TRY(hipMemcpy(outp, po, sizeof(void *) * n_proj,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pcp, pc, sizeof(uint16_t) * n_proj,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lnp, ln, n_proj, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_decode_multi, dim3(grid_for(h.n_blocks)),
                       dim3(OBX_WG_HOST), 0, ctx->stream, h.d_buf,
                       h.d_blocks, h.n_blocks, (const uint16_t *)pcp,
                       lnp, (uint32_t)n_proj, (uint8_t *const *)outp,
                       (uint8_t *const *)nullptr);
  } else {
    for (uint16_t i = 0; i < n_proj; i++) {
      uint16_t c = proj_cols[i];
      if (c >= h.n_cols) return OBX_INVALID_ARGUMENT;
      if (!h.d_decode_out[c])
        HIP_TRY(hipMalloc(&h.d_decode_out[c], h.total_rows * h.cols[c].len));
      auto kfn = h.lds_ok ? k_decode_lds : k_decode;
      hipLaunchKernelGGL(kfn, dim3(grid_for(h.n_blocks)), dim3(OBX_WG_HOST), 0,
                         ctx->stream, h.d_buf, h.d_blocks, h.n_blocks,
                         (uint32_t)c, (uint32_t)h.cols[c].len,
                         h.d_decode_out[c], (uint8_t *)nullptr);
    }
  }
  return end_timed(ctx, false);
}

extern "C" int obx_gpu_fetch_col(obx_gpu_ctx *ctx, int handle, uint16_t col,
                                 uint8_t *out, int64_t cap) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  if (col >= h.n_cols || !h.d_decode_out[col]) return OBX_INVALID_ARGUMENT;
  int64_t bytes = (int64_t)h.total_rows * h.cols[col].len;
  if (cap < bytes) return OBX_BUF_NOT_ENOUGH;
  HIP_TRY(hipMemcpy(out, h.d_decode_out[col], bytes, hipMemcpyDeviceToHost));
  return OBX_SUCCESS;
}

/* grow-only device buffer: reallocates when `need` units exceed `cap`; a
   failed hipMalloc leaves no stale pair */
template <class T>
static int grow(T *&p, uint64_t &cap, uint64_t need, size_t unit) {
  if (need <= cap) return OBX_SUCCESS;
  (void)hipFree(p);
  p = nullptr;
  cap = 0;
  HIP_TRY(hipMalloc(&p, need * unit));
  cap = need;
  return OBX_SUCCESS;
}

/* get_rows(row_ids) for a whole scan range: filter (with row ids), block
   offsets, gather-decode of the survivors (obx_project.hip). The only host
   wait between device steps is the filter's own, whose survivor count sizes
   the outputs; the offset scan and the gather follow each other on the
   stream. */
extern "C" int obx_gpu_scan_project(obx_gpu_ctx *ctx, int handle,
                                    const obx_filter_desc *filter,
                                    const uint16_t *proj_cols, uint16_t n_proj,
                                    int want_row_nos, uint64_t *n_rows) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  h.sel_n_proj = 0; /* a failed call leaves no result behind */
  if (!proj_cols || n_proj == 0 || n_proj > OBX_DEV_MAX_COLS)
    return OBX_INVALID_ARGUMENT;
  for (uint16_t i = 0; i < n_proj; i++)
    if (proj_cols[i] >= h.n_cols) return OBX_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(ctx->device));

  const bool filtered = filter && filter->n_leaves;
  uint64_t total = h.total_rows;
  ctx->last_proj_ms[0] = ctx->last_proj_ms[1] = ctx->last_proj_ms[2] = 0.0;
  if (filtered) {
    int rc = run_filter(ctx, h, filter, 1);
    if (rc != OBX_SUCCESS) return rc;
    ctx->last_proj_ms[0] = ctx->last_ms;
    total = h.last_survivors;
  } else {
    ctx->last_jit = 0; /* no filter stage ran */
  }

  if (total > 0) {
    proj_args pa;
    memset(&pa, 0, sizeof(pa));
    pa.n_proj = n_proj;
    for (uint16_t i = 0; i < n_proj; i++) {
      const uint16_t c = proj_cols[i];
      int rc = grow(h.d_sel_out[i], h.sel_out_cap[i], total * h.cols[c].len, 1);
      if (rc != OBX_SUCCESS) return rc;
      pa.out[i] = h.d_sel_out[i];
      pa.col[i] = c;
      pa.len[i] = h.cols[c].len;
    }
    int rc = grow(h.d_sel_nulls, h.sel_nulls_cap, total, 1);
    if (rc != OBX_SUCCESS) return rc;
    if (want_row_nos) {
      rc = grow(h.d_sel_row_nos, h.sel_row_nos_cap, total, sizeof(uint64_t));
      if (rc != OBX_SUCCESS) return rc;
    }
    const uint32_t n_tiles = (h.n_blocks + OBX_PROJ_TILE - 1) / OBX_PROJ_TILE;
    if (filtered && !h.d_blk_off) {
      HIP_TRY(hipMalloc(&h.d_blk_off, ((uint64_t)h.n_blocks + 1) * 8));
      HIP_TRY(hipMalloc(&h.d_tile_sums, (uint64_t)n_tiles * 8));
    }

    HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
    if (filtered) {
      hipLaunchKernelGGL(k_project_tile_sums, dim3(n_tiles), dim3(OBX_WG_HOST),
                         0, ctx->stream, h.d_blk_counts, h.n_blocks,
                         h.d_tile_sums);
      hipLaunchKernelGGL(k_project_offsets, dim3(n_tiles), dim3(OBX_WG_HOST),
                         0, ctx->stream, h.d_blk_counts, h.n_blocks,
                         h.d_tile_sums, h.d_blk_off);
    }
    HIP_TRY(hipEventRecord(ctx->ev_mid, ctx->stream));
    hipLaunchKernelGGL(h.lds_ok ? k_project_sel_lds : k_project_sel,
                       dim3(grid_for(h.n_blocks)), dim3(OBX_WG_HOST), 0,
                       ctx->stream, h.d_buf, h.d_blocks, h.n_blocks,
                       filtered ? h.d_row_ids : (const int32_t *)nullptr,
                       filtered ? h.d_blk_counts : (const uint32_t *)nullptr,
                       filtered ? h.d_blk_off : (const uint64_t *)nullptr, pa,
                       h.d_sel_nulls,
                       want_row_nos ? h.d_sel_row_nos : (uint64_t *)nullptr,
                       total);
    rc = end_timed(ctx, false);
    if (rc != OBX_SUCCESS) return rc;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_mid));
    ctx->last_proj_ms[1] = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_mid, ctx->ev_stop));
    ctx->last_proj_ms[2] = ms;
  }
  /* filter + offset scan + gather together */
  ctx->last_ms = ctx->last_proj_ms[0] + ctx->last_proj_ms[1] +
                 ctx->last_proj_ms[2];

  memcpy(h.sel_cols, proj_cols, sizeof(uint16_t) * n_proj);
  h.sel_has_row_nos = want_row_nos != 0;
  h.sel_rows = total;
  h.sel_n_proj = n_proj;
  if (n_rows) *n_rows = total;
  return OBX_SUCCESS;
}

/* the rows of [start, start + count) that the result holds */
static uint64_t sel_window(const obx_handle &h, uint64_t start,
                           uint64_t count) {
  if (start >= h.sel_rows) return 0;
  return count < h.sel_rows - start ? count : h.sel_rows - start;
}

extern "C" int obx_gpu_fetch_proj(obx_gpu_ctx *ctx, int handle,
                                  uint16_t proj_idx, uint64_t start,
                                  uint64_t count, uint8_t *out, int64_t cap,
                                  uint8_t *out_nulls, int64_t nulls_cap,
                                  uint64_t *n_out) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  if (proj_idx >= h.sel_n_proj) return OBX_INVALID_ARGUMENT;
  const uint64_t n = sel_window(h, start, count);
  if (n_out) *n_out = n;
  if (n == 0) return OBX_SUCCESS;
  const uint64_t len = h.cols[h.sel_cols[proj_idx]].len;
  const uint64_t null_bytes = (n + 7) / 8;
  if (out && (cap < 0 || (uint64_t)cap < n * len)) return OBX_BUF_NOT_ENOUGH;
  if (out_nulls && (nulls_cap < 0 || (uint64_t)nulls_cap < null_bytes))
    return OBX_BUF_NOT_ENOUGH;
  HIP_TRY(hipSetDevice(ctx->device));
  if (out)
    HIP_TRY(hipMemcpyAsync(out, h.d_sel_out[proj_idx] + start * len, n * len,
                           hipMemcpyDeviceToHost, ctx->stream));
  if (out_nulls) {
    int rc = grow(h.d_sel_bits, h.sel_bits_cap, null_bytes, 1);
    if (rc != OBX_SUCCESS) return rc;
    uint64_t g = (null_bytes + OBX_WG_HOST - 1) / OBX_WG_HOST;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_project_pack_nulls, dim3((uint32_t)g),
                       dim3(OBX_WG_HOST), 0, ctx->stream, h.d_sel_nulls,
                       start, n, (uint32_t)proj_idx, h.d_sel_bits);
    HIP_TRY(hipMemcpyAsync(out_nulls, h.d_sel_bits, null_bytes,
                           hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_fetch_proj_row_nos(obx_gpu_ctx *ctx, int handle,
                                          uint64_t start, uint64_t count,
                                          uint64_t *out, int64_t cap,
                                          uint64_t *n_out) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  if (!h.sel_n_proj || !h.sel_has_row_nos) return OBX_INVALID_ARGUMENT;
  const uint64_t n = sel_window(h, start, count);
  if (n_out) *n_out = n;
  if (n == 0 || !out) return OBX_SUCCESS;
  if (cap < 0 || (uint64_t)cap < n) return OBX_BUF_NOT_ENOUGH;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(out, h.d_sel_row_nos + start, n * sizeof(uint64_t),
                         hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return OBX_SUCCESS;
}

/* device time of one stage of the last scan_project: 0 filter, 1 block
   offsets, 2 gather-decode (their sum is obx_gpu_last_kernel_ms) */
extern "C" double obx_gpu_last_proj_stage_ms(obx_gpu_ctx *ctx, int stage) {
  return ctx && stage >= 0 && stage < 3 ? ctx->last_proj_ms[stage] : -1.0;
}

/* one live group as either table hands it over: a gslot of the fixed
   tables, or a compacted record of the sized one. cells = n_aggs x 4 limbs */
struct live_group {
  uint64_t key, count;
  const unsigned long long *cells;
};

/* one group -> its result row: COUNT(*) from the row count, MIN/MAX sign
   extension and the "no value seen" rule, everything else limb by limb */
static void group_to_row(const live_group &lg, uint8_t key_len,
                         const obx_agg_desc *agg, obx_group_row *g) {
  memcpy(g->key, &lg.key, 8);
  g->key_len = key_len;
  g->row_count = lg.count;
  uint32_t na = agg ? agg->n_aggs : 0;
  for (uint32_t a = 0; a < na; a++) {
    const unsigned long long *cell = lg.cells + 4 * a;
    uint8_t kind = agg->aggs[a].kind;
    if (kind == OBX_AGG_COUNT && agg->aggs[a].col_a == UINT16_MAX) {
      /* COUNT(*) = the group's row count (group pass) */
      g->cells[a].limb[0] = lg.count;
      g->cells[a].limb[1] = g->cells[a].limb[2] = g->cells[a].limb[3] = 0;
    } else if (kind == OBX_AGG_MIN || kind == OBX_AGG_MAX) {
      /* sign-extend the int64 min/max into the 256-bit cell; a group
         with NO non-null values keeps the init sentinel and its valid
         flag (cell[1]) unset — report 0, matching the oracle's
         empty-MIN/MAX convention (SQL NULL surfaces via row_count /
         COUNT(col) at the caller) */
      int64_t v = cell[1] ? (int64_t)cell[0] : 0;
      g->cells[a].limb[0] = (uint64_t)v;
      uint64_t s = v < 0 ? ~0ull : 0ull;
      g->cells[a].limb[1] = g->cells[a].limb[2] = g->cells[a].limb[3] = s;
    } else {
      for (int l = 0; l < 4; l++) g->cells[a].limb[l] = cell[l];
    }
  }
}

/* the tail of both aggregate scan verbs: the live groups (in any order) and
   the scan's 16 counters at cnt -> the handle's full sorted group rows
   (obx_gpu_agg_fetch pages them) and the inline result. key_len is the sum of
   the group columns' datum lengths. */
static int groups_to_rows(obx_handle &h, std::vector<live_group> &live,
                          const unsigned long long *cnt, uint8_t key_len,
                          const obx_agg_desc *agg, obx_agg_result *out) {
  /* slots 8..15: striped per-wave survivor sums */
  unsigned long long passed = cnt[0];
  for (int i2 = 8; i2 < 16; i2++) passed += cnt[i2];

  memset(out, 0, sizeof(*out));
  out->rows_scanned = h.total_rows;
  out->rows_passed = passed;
  std::sort(live.begin(), live.end(),
            [](const live_group &a, const live_group &b) {
    /* little-endian packed keys -> compare as memcmp on key bytes */
    uint8_t ka[8], kb[8];
    memcpy(ka, &a.key, 8);
    memcpy(kb, &b.key, 8);
    return memcmp(ka, kb, 8) < 0;
  });
  /* materialize ALL rows (the growth path's pagination source), then
     surface the inline result when it fits */
  h.last_rows.assign(live.size(), obx_group_row());
  for (size_t i = 0; i < live.size(); i++)
    group_to_row(live[i], key_len, agg, &h.last_rows[i]);
  if (h.last_rows.size() > OBX_MAX_GROUPS) {
    /* more groups than the inline result holds: rows stay paged behind
       obx_gpu_agg_fetch (the ObHashGroupByOp growth path) */
    out->n_groups = (uint32_t)h.last_rows.size();
    return OBX_BUF_NOT_ENOUGH;
  }
  out->n_groups = (uint32_t)h.last_rows.size();
  for (size_t i = 0; i < h.last_rows.size(); i++)
    out->groups[i] = h.last_rows[i];
  return OBX_SUCCESS;
}

/* ... from a fetched table of n_gt gslots */
static int table_to_rows(obx_handle &h, const gslot *gt, size_t n_gt,
                         const unsigned long long *cnt, uint8_t key_len,
                         const obx_agg_desc *agg, obx_agg_result *out) {
  std::vector<live_group> live;
  for (size_t i = 0; i < n_gt; i++)
    if (gt[i].key != OBX_KEY_EMPTY)
      live.push_back({gt[i].key, gt[i].count, &gt[i].cells[0][0]});
  return groups_to_rows(h, live, cnt, key_len, agg, out);
}

/* the growth path of both aggregate scan verbs: an LDS group table
   overflowed (counters[1]), so the scan runs again through a direct-global
   kernel on the OBX_GTABLE_BIG table, which lands in the pinned buffer in
   place of the small one. launch(table, counters) queues that kernel.
   AND-only filters: OR-programs keep the capacity error, as do more than
   OBX_GTABLE_BIG distinct groups (counters[2]). */
template <class LAUNCH>
static int rerun_direct(obx_gpu_ctx *ctx, obx_handle &h,
                        const dev_plan_hdr &ph, uint32_t min_mask,
                        uint32_t max_mask, size_t *n_gt,
                        unsigned long long cnt[16], LAUNCH launch) {
  if (ph.n_prog != 0) return OBX_BUF_NOT_ENOUGH;
  if (!h.d_gtable_big)
    HIP_TRY(hipMalloc(&h.d_gtable_big, OBX_RESULT_BYTES(OBX_GTABLE_BIG)));
  /* same layout as the small table: counters behind the slots */
  unsigned long long *big_counters =
      (unsigned long long *)(h.d_gtable_big + OBX_GTABLE_BIG);
  gtable_init(h.d_gtable_big, OBX_GTABLE_BIG, 16, min_mask, max_mask,
              ctx->stream);
  launch(h.d_gtable_big, big_counters);
  HIP_TRY(hipMemcpyAsync(ctx->h_result, h.d_gtable_big,
                         OBX_RESULT_BYTES(OBX_GTABLE_BIG),
                         hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *n_gt = OBX_GTABLE_BIG;
  memcpy(cnt, (const gslot *)ctx->h_result + OBX_GTABLE_BIG,
         16 * sizeof(cnt[0]));
  if (cnt[2] != 0) return OBX_BUF_NOT_ENOUGH; /* >4096 distinct groups */
  return OBX_SUCCESS;
}

/* ---- what both aggregate scan verbs run around their own launch ---------- */

/* rows all workgroups of a sized-table scan together may insert between two
   looks at the stop word: each looks once per block */
static uint64_t group_hash_in_flight(const obx_handle &h) {
  return (uint64_t)grid_for(h.n_blocks) *
         (h.max_block_rows ? h.max_block_rows : 4096);
}

/* the growth path under a raised cap (obx_gpu_set_max_groups): an LDS group
   table overflowed (counters[1]), so the scan runs again on a hash table in
   device memory sized from the cap (obx_grouphash.h); launch(table,
   max_groups, counters) queues that kernel. The bound on the survivors is
   the table's row count: the first kernel's counters are not a count of
   survivors once a table overflowed. The counter block comes back first:
   its winner words are the live keys, which decide the refusal and size the
   compacted records; then k_group_compact and one copy of exactly those
   records. A refused scan has not seen every row, so nothing of it is
   reported. */
template <class LAUNCH>
static int rerun_hash(obx_gpu_ctx *ctx, obx_handle &h, const dev_plan_hdr &ph,
                      uint32_t min_mask, uint32_t max_mask, uint8_t key_len,
                      const obx_agg_desc *agg, obx_agg_result *out,
                      LAUNCH launch) {
  if (ph.n_prog != 0) return OBX_BUF_NOT_ENOUGH;
  const uint64_t slots =
      obx_gh_slots(ctx->max_groups, h.total_rows, group_hash_in_flight(h));
  const uint64_t head = OBX_GH_COUNTER_WORDS * 8;
  int rc = grow(h.d_ghash, h.ghash_cap,
                head + obx_gh_table_bytes(slots, ph.n_aggs), 1);
  if (rc != OBX_SUCCESS) return rc;
  unsigned long long *counters = (unsigned long long *)h.d_ghash;
  const obx_gh_dev view = obx_gh_view(h.d_ghash + head, slots, ph.n_aggs);
  ctx->last_group_slots = slots;
  const uint64_t words = slots * (2 + 4 * (uint64_t)ph.n_aggs);
  uint64_t g = (words + OBX_WG_HOST - 1) / OBX_WG_HOST;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(k_group_hash_init, dim3((uint32_t)g), dim3(OBX_WG_HOST),
                     0, ctx->stream, view, counters, min_mask, max_mask);
  HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
  launch(view, ctx->max_groups, counters);
  HIP_TRY(hipEventRecord(ctx->ev_stop, ctx->stream));
  unsigned long long cnt[OBX_GH_COUNTER_WORDS];
  HIP_TRY(hipMemcpyAsync(ctx->h_result, counters, sizeof(cnt),
                         hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  memcpy(cnt, ctx->h_result, sizeof(cnt));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
  ctx->last_group_ms = ms;
  uint64_t n_live = 0;
  for (int i = 0; i < 8; i++) n_live += cnt[OBX_GH_WINNERS + i];
  if (obx_gh_refused(n_live, cnt[2], ctx->max_groups))
    return OBX_BUF_NOT_ENOUGH;

  const uint32_t rec_words = 2 + 4 * ph.n_aggs;
  rc = grow(h.d_grecs, h.grecs_cap, n_live * rec_words * 8, 1);
  if (rc != OBX_SUCCESS) return rc;
  if (n_live) {
    g = slots / OBX_WG_HOST;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_group_compact, dim3((uint32_t)g), dim3(OBX_WG_HOST),
                       0, ctx->stream, view, counters + OBX_GH_CURSOR,
                       (unsigned long long *)h.d_grecs, n_live);
    h.h_grecs.resize(n_live * rec_words);
    HIP_TRY(hipMemcpyAsync(h.h_grecs.data(), h.d_grecs,
                           n_live * rec_words * 8, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  std::vector<live_group> live(n_live);
  for (uint64_t i = 0; i < n_live; i++) {
    const unsigned long long *rec = h.h_grecs.data() + i * rec_words;
    live[i] = {rec[0], rec[1], rec + 2};
  }
  return groups_to_rows(h, live, cnt, key_len, agg, out);
}

/* bit a: cell a is a MIN / a MAX, so the empty group table starts it at its
   sentinel (k_gtable_init). kind_of(a) is the cell's kind, as in the kernels */
struct minmax_masks { uint32_t min = 0, max = 0; };
template <class KIND_OF>
static minmax_masks agg_minmax_masks(uint32_t n_aggs, KIND_OF kind_of) {
  minmax_masks m;
  for (uint32_t a = 0; a < n_aggs; a++) {
    if (kind_of(a) == OBX_AGG_MIN) m.min |= 1u << a;
    else if (kind_of(a) == OBX_AGG_MAX) m.max |= 1u << a;
  }
  return m;
}

/* a new scan: what the context reports of the last one starts over */
static void reset_last_scan(obx_gpu_ctx *ctx) {
  ctx->last_jit = 0;
  ctx->last_grid = 0;
  ctx->last_bdesc = 0;
  ctx->last_joint = 0;
  ctx->bdesc_built = false;
  ctx->last_group_slots = 0;
  ctx->last_group_ms = 0.0;
}

/* the tail, after the scan kernel is queued: close the timed region with
   the copy of table + counters (one allocation, one copy into the pinned
   buffer), take the growth path when an LDS table overflowed or the global
   table was full (counters[1]; launch_direct as rerun_direct's launch, or,
   under a cap above OBX_GTABLE_BIG, launch_hash as rerun_hash's: straight to
   the sized table, two scans and not three), and turn the table into rows */
template <class LAUNCH, class LAUNCH_HASH>
static int finish_agg_scan(obx_gpu_ctx *ctx, obx_handle &h,
                           const dev_plan_hdr &ph, minmax_masks mm,
                           uint8_t key_len, const obx_agg_desc *agg,
                           obx_agg_result *out, LAUNCH launch_direct,
                           LAUNCH_HASH launch_hash) {
  int rc = end_timed(ctx, true, h.d_gtable,
                     OBX_RESULT_BYTES(OBX_GTABLE_SLOTS));
  if (rc != OBX_SUCCESS) return rc;
  const gslot *gt = (const gslot *)ctx->h_result;
  size_t n_gt = OBX_GTABLE_SLOTS;
  unsigned long long cnt[16];
  memcpy(cnt, gt + OBX_GTABLE_SLOTS, sizeof(cnt));
  if (cnt[1] != 0) {
    if (ctx->max_groups > OBX_GTABLE_BIG)
      return rerun_hash(ctx, h, ph, mm.min, mm.max, key_len, agg, out,
                        launch_hash);
    rc = rerun_direct(ctx, h, ph, mm.min, mm.max, &n_gt, cnt, launch_direct);
    if (rc != OBX_SUCCESS) return rc;
  }
  return table_to_rows(h, gt, n_gt, cnt, key_len, agg, out);
}

extern "C" int obx_gpu_scan_filter_agg(obx_gpu_ctx *ctx, int handle,
                                       const obx_filter_desc *filter,
                                       const obx_agg_desc *agg,
                                       obx_agg_result *out) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp || !out) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  HIP_TRY(hipSetDevice(ctx->device));
  h.last_rows.clear(); /* no stale pagination after a failed scan */
  dev_plan_hdr ph;
  dev_leaf plv[OBX_DEV_MAX_LEAVES];
  int rc = prep_query(ctx, h, filter, agg, ph, plv);
  if (rc != OBX_SUCCESS) return rc;
  reset_last_scan(ctx);

  /* init global table + counters on the device (min/max cells need
     INT64_MAX/MIN) */
  const minmax_masks mm = agg_minmax_masks(
      ph.n_aggs, [&](uint32_t a) { return ph.aggs[a].kind; });
  gtable_init(h.d_gtable, OBX_GTABLE_SLOTS, 16, mm.min, mm.max, ctx->stream);

  /* Default: the fused single-kernel path (measured fastest in round 1).
     OBX_PIPELINE_AGG=1 switches to the filter->group->agg-pass kernel DAG
     (cleaner structure, currently slower — round-2 exploration; both paths
     are parity-tested). */
  const bool use_pipeline = getenv("OBX_PIPELINE_AGG") != nullptr;
  if (use_pipeline) {
    uint64_t bm_words = (h.total_rows + 63) / 64 + 1;
    if (!h.d_bitmap) HIP_TRY(hipMalloc(&h.d_bitmap, bm_words * 8));
    HIP_TRY(hipMemsetAsync(h.d_bitmap, 0, bm_words * 8, ctx->stream));
    if (!h.d_row_slot) HIP_TRY(hipMalloc(&h.d_row_slot, h.total_rows + 1));

    HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
    hipLaunchKernelGGL(generic_filter_kernel(h, ph),
                       dim3(grid_for(h.n_blocks)), dim3(OBX_WG_HOST), 0,
                       ctx->stream, h.d_buf, h.d_blocks, h.n_blocks,
                       h.d_pleaves, h.d_bleaves, ph, h.d_bitmap,
                       (int32_t *)nullptr, (uint32_t *)nullptr, h.d_counters);
    hipLaunchKernelGGL(k_group_pass, dim3(grid_for(h.n_blocks)),
                       dim3(OBX_WG_HOST), 0, ctx->stream, h.d_buf, h.d_blocks,
                       h.n_blocks, ph, h.d_bitmap, h.d_row_slot, h.d_gtable,
                       h.d_counters);
    for (uint32_t a = 0; a < ph.n_aggs;) {
      const dev_agg &ag = ph.aggs[a];
      if (ag.kind == OBX_AGG_COUNT && ag.ia == 0xFF) { a++; continue; }
      const bool fuse = obx_fuse_p3(ph.aggs, ph.n_aggs, a);
      hipLaunchKernelGGL(k_agg_pass, dim3(grid_for(h.n_blocks)),
                         dim3(OBX_WG_HOST), 0, ctx->stream, h.d_buf,
                         h.d_blocks, h.n_blocks, ph, a, h.d_bitmap,
                         h.d_row_slot, h.d_gtable);
      a += fuse ? 2 : 1;
    }
  } else {
    /* plan-specialized JIT kernel when eligible (compiled once per plan
       signature, before the timed region; obx_jit_rt.cpp) */
    const jit_entry *je = jit_prepare(ctx->device, h, ph, plv);
    ctx->last_jit = je ? je->kind : 0; /* 2 = persistent v2, 1 = v1 */
    const obx_bdesc *bd = nullptr;
    if (je && je->bdesc) {
      /* the first query with this column list pays the build: its device
         time is added to that query's prep time (end_timed) */
      HIP_TRY(hipEventRecord(ctx->ev_b0, ctx->stream));
      bd = bdesc_get(h, je->bd_cols, ctx->stream, &ctx->bdesc_built);
      if (!bd) return OBX_INTERNAL_ERROR;
      HIP_TRY(hipEventRecord(ctx->ev_b1, ctx->stream));
    }
    ctx->last_bdesc = bd != nullptr;
    ctx->last_joint = je ? je->joint : 0;
    HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
    if (je) {
      if (jit_launch(je, h, bd, ctx->stream, &ctx->last_grid) != 0)
        return OBX_INTERNAL_ERROR;
    } else {
      auto kfn = h.lds_ok
                     ? (ph.n_prog ? k_scan_filter_agg_prog_lds
                                  : k_scan_filter_agg_lds)
                     : (ph.n_prog ? k_scan_filter_agg_prog : k_scan_filter_agg);
      hipLaunchKernelGGL(kfn, dim3(grid_for(h.n_blocks)), dim3(OBX_WG_HOST), 0,
                         ctx->stream, h.d_buf, h.d_blocks, h.n_blocks,
                         h.d_pleaves, h.d_bleaves, ph, h.d_gtable,
                         h.d_counters);
    }
  }
  uint8_t key_len = 0;
  if (agg)
    for (int g = 0; g < agg->n_group_cols; g++)
      key_len += h.cols[agg->group_cols[g]].len;
  /* the growth path: the direct-global high-cardinality kernel */
  return finish_agg_scan(
      ctx, h, ph, mm, key_len, agg, out,
      [&](gslot *big, unsigned long long *big_counters) {
        hipLaunchKernelGGL(k_scan_agg_direct, dim3(grid_for(h.n_blocks)),
                           dim3(OBX_WG_HOST), 0, ctx->stream, h.d_buf,
                           h.d_blocks, h.n_blocks, h.d_pleaves, h.d_bleaves,
                           ph, big, big_counters);
      },
      [&](const obx_gh_dev &table, uint64_t max_groups,
          unsigned long long *counters) {
        hipLaunchKernelGGL(k_scan_agg_hash, dim3(grid_for(h.n_blocks)),
                           dim3(OBX_WG_HOST), 0, ctx->stream, h.d_buf,
                           h.d_blocks, h.n_blocks, h.d_pleaves, h.d_bleaves,
                           ph, table, max_groups, counters);
      });
}

/* The join scan: obx_gpu_scan_filter_agg with a key-map probe between the
   filter and the aggregates (obx_join.hip). The plan never sees
   OBX_COL_JOINED: prep_query gets the aggregate descriptor with the payload
   group column removed and COUNT(*) where a payload aggregate stands, and
   dev_join tells the kernels where the payload goes. */
extern "C" int obx_gpu_scan_join_agg(obx_gpu_ctx *ctx, int handle,
                                     const obx_filter_desc *filter,
                                     const obx_join_desc *join,
                                     const obx_agg_desc *agg,
                                     obx_agg_result *out) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp || !out || !join) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  h.last_rows.clear(); /* no stale pagination after a failed scan */
  const obx_keymap *km = obx_keymap_lookup(ctx, join->map_id);
  if (!km || join->probe_col >= h.n_cols) return OBX_INVALID_ARGUMENT;
  const uint8_t probe_len = h.cols[join->probe_col].len;
  if (probe_len == 0 || probe_len > 8) return OBX_NOT_SUPPORTED;

  dev_join dj;
  memset(&dj, 0, sizeof(dj));
  dj.km = km->view;
  dj.pay_len = km->info.payload_len;
  /* plan: what prep_query sees; eff: what the result rows are read by
     (COUNT(payload) is COUNT(*), a payload is never NULL) */
  obx_agg_desc plan, eff;
  memset(&plan, 0, sizeof(plan));
  memset(&eff, 0, sizeof(eff));
  uint8_t key_len = 0;
  if (agg) {
    if (agg->n_group_cols > 2 || agg->n_aggs > OBX_DEV_MAX_AGGS)
      return OBX_INVALID_ARGUMENT;
    eff = *agg;
    for (int g = 0; g < agg->n_group_cols; g++) {
      if (agg->group_cols[g] == OBX_COL_JOINED) {
        if (dj.pay_group) return OBX_INVALID_ARGUMENT; /* named twice */
        dj.pay_group = 1;
        dj.pay_pos = (uint8_t)g;
        key_len += dj.pay_len;
      } else {
        if (agg->group_cols[g] >= h.n_cols) return OBX_INVALID_ARGUMENT;
        plan.group_cols[plan.n_group_cols++] = agg->group_cols[g];
        key_len += h.cols[agg->group_cols[g]].len;
      }
    }
    if (dj.pay_group) {
      dj.real_len = plan.n_group_cols ? h.cols[plan.group_cols[0]].len : 0;
      if (dj.pay_len + dj.real_len > 7) return OBX_NOT_SUPPORTED;
    }
    plan.n_aggs = agg->n_aggs;
    for (int a = 0; a < agg->n_aggs; a++) {
      const obx_agg_expr &e = agg->aggs[a];
      plan.aggs[a] = e;
      const bool prod = e.kind == OBX_AGG_SUM_PROD2 ||
                        e.kind == OBX_AGG_SUM_PROD3 ||
                        e.kind == OBX_AGG_SUM_MUL;
      if (e.col_b == OBX_COL_JOINED || e.col_c == OBX_COL_JOINED)
        return OBX_INVALID_ARGUMENT;
      if (e.col_a != OBX_COL_JOINED) continue;
      if (prod || e.kind > OBX_AGG_SUM_MUL) return OBX_INVALID_ARGUMENT;
      plan.aggs[a].kind = OBX_AGG_COUNT; /* neutral: no pass, no operand */
      plan.aggs[a].col_a = UINT16_MAX;
      if (e.kind == OBX_AGG_COUNT) {
        eff.aggs[a].col_a = UINT16_MAX;
      } else {
        dj.own_mask |= (uint8_t)(1u << a);
      }
    }
  }

  HIP_TRY(hipSetDevice(ctx->device));
  dev_plan_hdr ph;
  int rc = prep_query(ctx, h, filter, &plan, ph);
  if (rc != OBX_SUCCESS) return rc;
  /* the probe column rides in the plan's need slots, so opnd_open reads it
     like any aggregate operand */
  uint32_t pi = 0;
  while (pi < ph.n_need && ph.need_cols[pi] != join->probe_col) pi++;
  if (pi == ph.n_need) {
    if (ph.n_need >= OBX_DEV_MAX_NEED) return OBX_NOT_SUPPORTED;
    ph.need_cols[ph.n_need++] = join->probe_col;
  }
  dj.probe_idx = (uint8_t)pi;
  for (uint32_t a = 0; a < ph.n_aggs; a++)
    dj.kind[a] = ((dj.own_mask >> a) & 1) ? agg->aggs[a].kind : ph.aggs[a].kind;
  reset_last_scan(ctx);

  /* by every cell's true kind: the plan holds COUNT(*) for the join's own */
  const minmax_masks mm = agg_minmax_masks(
      ph.n_aggs, [&](uint32_t a) { return dj.kind[a]; });
  gtable_init(h.d_gtable, OBX_GTABLE_SLOTS, 16, mm.min, mm.max, ctx->stream);
  HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
  auto kfn = h.lds_ok
                 ? (ph.n_prog ? k_scan_join_agg_prog_lds : k_scan_join_agg_lds)
                 : (ph.n_prog ? k_scan_join_agg_prog : k_scan_join_agg);
  hipLaunchKernelGGL(kfn, dim3(grid_for(h.n_blocks)), dim3(OBX_WG_HOST), 0,
                     ctx->stream, h.d_buf, h.d_blocks, h.n_blocks, h.d_pleaves,
                     h.d_bleaves, ph, dj, h.d_gtable, h.d_counters);
  /* the growth path, with the probe */
  return finish_agg_scan(
      ctx, h, ph, mm, key_len, agg ? &eff : nullptr, out,
      [&](gslot *big, unsigned long long *big_counters) {
        hipLaunchKernelGGL(k_scan_join_agg_direct, dim3(grid_for(h.n_blocks)),
                           dim3(OBX_WG_HOST), 0, ctx->stream, h.d_buf,
                           h.d_blocks, h.n_blocks, h.d_pleaves, h.d_bleaves,
                           ph, dj, big, big_counters);
      },
      [&](const obx_gh_dev &table, uint64_t max_groups,
          unsigned long long *counters) {
        hipLaunchKernelGGL(k_scan_join_agg_hash, dim3(grid_for(h.n_blocks)),
                           dim3(OBX_WG_HOST), 0, ctx->stream, h.d_buf,
                           h.d_blocks, h.n_blocks, h.d_pleaves, h.d_bleaves,
                           ph, dj, table, max_groups, counters);
      });
}

/* ---- the cap on a scan's distinct groups (obx.h) ------------------------ */
extern "C" int obx_gpu_set_max_groups(obx_gpu_ctx *ctx, uint64_t max_groups) {
  if (!ctx || max_groups < OBX_GTABLE_BIG) return OBX_INVALID_ARGUMENT;
  if (max_groups > OBX_GH_MAX_GROUPS) return OBX_NOT_SUPPORTED;
  ctx->max_groups = max_groups;
  return OBX_SUCCESS;
}

extern "C" uint64_t obx_gpu_max_groups(obx_gpu_ctx *ctx) {
  return ctx ? ctx->max_groups : 0;
}

extern "C" uint64_t obx_gpu_last_group_slots(obx_gpu_ctx *ctx) {
  return ctx ? ctx->last_group_slots : 0;
}

extern "C" double obx_gpu_last_group_ms(obx_gpu_ctx *ctx) {
  return ctx ? ctx->last_group_ms : -1.0;
}

/* TEST INFRASTRUCTURE: the sized table over host memory, by the sizing and
   insert functions the kernels run. No HIP call. Keys go in one by one, in
   order; the stop word is looked at before the first key and then after
   every in_flight keys (before every key when in_flight is 0), as a grid
   that inserts in_flight rows between two looks would. *found = keys of the
   input that a lookup finds afterwards (all of them, unless the scan
   stopped). */
extern "C" int obx_gpu_group_hash_host_model(
    const uint64_t *keys, uint64_t n, uint64_t max_groups, uint64_t in_flight,
    uint32_t n_aggs, uint64_t *slots_out, uint64_t *live_out,
    uint64_t *max_probe_out, uint64_t *found_out, uint64_t *bytes_out) {
  if ((n && !keys) || n_aggs > OBX_DEV_MAX_AGGS ||
      max_groups < OBX_GTABLE_BIG)
    return OBX_INVALID_ARGUMENT;
  if (max_groups > OBX_GH_MAX_GROUPS) return OBX_NOT_SUPPORTED;
  const uint64_t slots = obx_gh_slots(max_groups, n, in_flight);
  /* the model needs the keys only: counts and cells are never touched */
  std::vector<unsigned long long> store(slots, OBX_KEY_EMPTY);
  const obx_gh_dev v = obx_gh_view(store.data(), slots, n_aggs);
  uint64_t live = 0, full = 0, max_probe = 0;
  for (uint64_t i = 0; i < n; i++) {
    if ((in_flight == 0 || i % in_flight == 0) &&
        (live > max_groups || full))
      break;
    bool won = false;
    uint64_t steps = 0;
    if (obx_gh_find_or_insert(v, keys[i], &won, &steps) < 0) full++;
    live += won;
    if (steps > max_probe) max_probe = steps;
  }
  uint64_t found = 0;
  for (uint64_t i = 0; i < n; i++) found += obx_gh_find(v, keys[i]) >= 0;
  if (slots_out) *slots_out = slots;
  if (live_out) *live_out = live;
  if (max_probe_out) *max_probe_out = max_probe;
  if (found_out) *found_out = found;
  if (bytes_out) *bytes_out = obx_gh_table_bytes(slots, n_aggs);
  return obx_gh_refused(live, full, max_groups) ? OBX_BUF_NOT_ENOUGH
                                                : OBX_SUCCESS;
}

/* Debug/test-only: the load-time facts of a blockset, without a GPU. Runs
 * only the host half of the PAX (is_cs == 0) or CS loader, then writes
 * handle_out[7] = n_blocks, n_cols, total_rows, total_bytes, lds_ok,
 * max_block_rows, max_block_len, and per column four words into col_out:
 * a flag word (1 dict_every, 2 dict_any, 4 dict_stable, 8 grp16_every,
 * 16 raw8_every, 32 rangefam_every, 64 ext_any, 128 slow_any, 256 span_any,
 * 512 bdesc_unfit), col_maxcnt, col_maxw, col_cnt_max. Returns the loader's status. */
extern "C" int obx_probe_load_facts(const obx_blockset *bs, int is_cs,
                                    uint64_t *handle_out, uint32_t *col_out) {
  if (!bs || !handle_out || !col_out) return OBX_INVALID_ARGUMENT;
  obx_table_facts h;
  std::vector<dev_block> blocks;
  int rc = is_cs ? obx_cs_host_load(bs, h, blocks, nullptr)
                 : obx_pax_host_load(bs, h, blocks);
  if (rc != OBX_SUCCESS) return rc;
  const uint64_t hf[7] = {h.n_blocks, h.n_cols, h.total_rows, h.total_bytes,
                          h.lds_ok, h.max_block_rows, h.max_block_len};
  memcpy(handle_out, hf, sizeof(hf));
  for (uint16_t c = 0; c < h.n_cols; c++) {
    const bool f[10] = {h.col_dict_every[c], h.col_dict_any[c],
                        h.col_dict_stable[c], h.col_grp16_every[c],
                        h.col_raw8_every[c], h.col_rangefam_every[c],
                        h.col_ext_any[c], h.col_slow_any[c], h.col_span_any[c],
                        h.col_bdesc_unfit[c]};
    uint32_t *o = col_out + 4 * c;
    o[0] = 0;
    for (int i = 0; i < 10; i++) o[0] |= (uint32_t)f[i] << i;
    o[1] = h.col_maxcnt[c];
    o[2] = h.col_maxw[c];
    o[3] = h.col_cnt_max[c];
  }
  return OBX_SUCCESS;
}

extern "C" double obx_gpu_last_kernel_ms(obx_gpu_ctx *ctx) {
  return ctx ? ctx->last_ms : -1.0;
}

/* per-query monitoring (the rebuild of the reference's per-operator
 * sql_plan_monitor / NG_TRACE stats): device times of the
 * last query's prep (plan upload + k_lower_leaves) and main kernel. */
extern "C" double obx_gpu_last_prep_ms(obx_gpu_ctx *ctx) {
  return ctx ? ctx->last_prep_ms : -1.0;
}

extern "C" int obx_gpu_last_jit(obx_gpu_ctx *ctx) {
  return ctx ? ctx->last_jit : 0;
}

/* 1 if the last scan's specialized kernel read the packed block descriptors
   (obx_bdesc), 0 if it read dev_block */
extern "C" int obx_gpu_last_bdesc(obx_gpu_ctx *ctx) {
  return ctx ? ctx->last_bdesc : 0;
}

/* joint-table form of the last scan's specialized kernel (obx_jit_scan.inc):
   0 none, 1 weights only, 2 one axis with the row count packed into the
   cell, 3 two axes (a table under 2 KB) with the row count packed in */
extern "C" int obx_gpu_last_joint(obx_gpu_ctx *ctx) {
  return ctx ? ctx->last_joint : 0;
}

/* how many descriptor arrays this handle has built so far (cache misses) */
extern "C" int64_t obx_gpu_bdesc_builds(obx_gpu_ctx *ctx, int handle) {
  obx_handle *h = obx_handle_lookup(ctx, handle);
  return h ? (int64_t)h->bdesc_builds : -1;
}

/* Debug/test-only: the packed descriptor of one dev_block for an ordered
 * column list, by the function k_pack_bdesc runs (obx_bdesc_pack_col),
 * without a GPU. Returns 1 if every listed count and width fits its slot,
 * 0 if not (the handle then keeps the dev_block path for that column). */
extern "C" int obx_bdesc_probe(const dev_block *blk, const uint16_t *cols,
                               uint32_t n_cols, obx_bdesc *out) {
  if (!blk || !cols || !out || n_cols > OBX_DEV_MAX_NEED)
    return OBX_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < n_cols; i++)
    if (cols[i] >= OBX_DEV_MAX_COLS) return OBX_INVALID_ARGUMENT;
  return obx_bdesc_pack(blk, cols, n_cols, out);
}

/* launch grid of the last scan's specialized kernel (0 = generic kernels) */
extern "C" uint32_t obx_gpu_last_grid(obx_gpu_ctx *ctx) {
  return ctx ? ctx->last_grid : 0;
}

extern "C" uint64_t obx_gpu_total_rows(obx_gpu_ctx *ctx, int handle) {
  const obx_handle *h = obx_handle_lookup(ctx, handle);
  return h ? h->total_rows : 0;
}
extern "C" uint64_t obx_gpu_total_bytes(obx_gpu_ctx *ctx, int handle) {
  const obx_handle *h = obx_handle_lookup(ctx, handle);
  return h ? h->total_bytes : 0;
}
extern "C" uint64_t obx_gpu_last_survivors(obx_gpu_ctx *ctx, int handle) {
  const obx_handle *h = obx_handle_lookup(ctx, handle);
  return h ? h->last_survivors : 0;
}

/* paged access to the last scan's full (sorted) group rows — the result
 * surface for > OBX_MAX_GROUPS groups (the reference's hash group-by
 * grows unboundedly, ob_exec_hash_struct_vec.h:1718; our device table
 * holds OBX_GTABLE_SLOTS groups and the host pages them out). */
extern "C" int obx_gpu_agg_fetch(obx_gpu_ctx *ctx, int handle,
                                 uint32_t start, uint32_t count,
                                 obx_group_row *out, uint32_t *n_out,
                                 uint64_t *n_total) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp || !out) return OBX_INVALID_ARGUMENT;
  obx_handle &h = *hp;
  uint64_t total = h.last_rows.size();
  if (n_total) *n_total = total;
  uint32_t n = 0;
  for (; n < count && start + n < total; n++) out[n] = h.last_rows[start + n];
  if (n_out) *n_out = n;
  return OBX_SUCCESS;
}
