/*
 * obx_keyset.hip — device-resident key sets: the build kernels and the
 * obx_gpu_keyset_* verbs (include/obx.h). Layout, sizing, insert and probe
 * are the inline functions of obx_keyset.h.
 *
 * A set is the build side of a hash join handed to the probe side's table
 * scan (the reference ships ObRFInFilterVecMsg / ObRFRangeFilterVecMsg /
 * ObRFBloomFilterMsg from the join to the scan, sql/engine/px/p2p_datahub,
 * and evaluates them in ObExprJoinFilter). Here the build keys are already in
 * device memory (obx_gpu_scan_project leaves them there), so the set is
 * built where they are, in three steps on the context's stream:
 *   k_keyset_minmax   per-workgroup reduce, one atomic min / max / count per
 *                     workgroup
 *   host              reads min and max, chooses the form (obx_ks_choose)
 *   k_keyset_insert   atomicCAS into the hash table or atomicOr into the
 *                     bitmap; the CAS winners / first setters of a bit are
 *                     the distinct keys, summed per workgroup before one
 *                     atomicAdd
 *
 * A translation unit of its own, so the scan kernels of obx_kernels.hip keep
 * their code and register allocation.
 */
#include <cstring>
#include <vector>

#include "obx_blk.h"
#include "obx_host.h"

static_assert(sizeof(((dev_leaf *)nullptr)->in_list) >= 5 * sizeof(int64_t),
              "a set leaf's view travels in dev_leaf.in_list");

enum { KS_MIN = 0, KS_MAX = 1, KS_COUNT = 2, KS_DISTINCT = 3, KS_MARKER = 4,
       KS_WORDS = 5 };

extern "C" __global__ __launch_bounds__(WG) void k_keyset_minmax(
    const uint8_t *__restrict__ src, uint32_t len, uint32_t sign,
    const uint8_t *__restrict__ nulls, uint32_t null_bit, uint64_t n,
    unsigned long long *__restrict__ scr) {
  __shared__ int64_t smn[WAVES], smx[WAVES];
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  uint64_t cnt = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * WG) {
    if (nulls && ((nulls[i] >> null_bit) & 1)) continue;
    const int64_t v = obx_ks_load_key(src, len, sign, i);
    if (v < mn) mn = v;
    if (v > mx) mx = v;
    cnt++;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t omn = (int64_t)shflxor64((uint64_t)mn, off);
    const int64_t omx = (int64_t)shflxor64((uint64_t)mx, off);
    if (omn < mn) mn = omn;
    if (omx > mx) mx = omx;
  }
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = mn;
    smx[threadIdx.x >> 6] = mx;
  }
  const uint64_t total = wg_sum(cnt); /* its barriers publish smn / smx */
  if (threadIdx.x == 0 && total) {
    for (uint32_t w = 0; w < WAVES; w++) {
      if (smn[w] < mn) mn = smn[w];
      if (smx[w] > mx) mx = smx[w];
    }
    cas_minmax(&scr[KS_MIN], mn, true);
    cas_minmax(&scr[KS_MAX], mx, false);
    atomicAdd(&scr[KS_COUNT], (unsigned long long)total);
  }
}

extern "C" __global__ __launch_bounds__(WG) void k_keyset_insert(
    const uint8_t *__restrict__ src, uint32_t len, uint32_t sign,
    const uint8_t *__restrict__ nulls, uint32_t null_bit, uint64_t n,
    uint64_t *__restrict__ words, uint64_t hi, int64_t mn, uint32_t form,
    uint32_t shift, unsigned long long *__restrict__ scr) {
  uint64_t won = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * WG) {
    if (nulls && ((nulls[i] >> null_bit) & 1)) continue;
    won += obx_ks_insert(words, hi, mn, form, shift,
                         (uint64_t *)&scr[KS_MARKER],
                         obx_ks_load_key(src, len, sign, i));
  }
  const uint64_t total = wg_sum(won);
  if (threadIdx.x == 0 && total)
    atomicAdd(&scr[KS_DISTINCT], (unsigned long long)total);
}

/* ---- host ---------------------------------------------------------------- */

const obx_keyset *obx_keyset_lookup(const obx_gpu_ctx *ctx, int64_t set_id) {
  if (!ctx || set_id < 0 || set_id >= (int64_t)ctx->keysets.size())
    return nullptr;
  return ctx->keysets[(size_t)set_id].get();
}

/* info of a chosen form; min / max read 1 / -1 when there is no key */
static void keyset_fill_info(obx_keyset_info *info, uint64_t n_in,
                             uint64_t n_distinct, uint8_t form, uint64_t size,
                             uint64_t n_words, int64_t mn, int64_t mx) {
  memset(info, 0, sizeof(*info));
  info->n_keys_in = n_in;
  info->n_distinct = n_distinct;
  info->slots_or_bits = size;
  info->bytes = n_words * 8;
  info->min = n_in ? mn : 1;
  info->max = n_in ? mx : -1;
  info->kind = form;
}

/* table words of a chosen form (at least one, so there is always memory to
   point at) */
static uint64_t keyset_words(uint8_t form, uint64_t size) {
  const uint64_t w = form == OBX_KS_BITMAP ? (size + 63) / 64 : size;
  return w ? w : 1;
}

static obx_keyset_dev keyset_view(const uint64_t *words, uint8_t form,
                                  uint64_t size, uint64_t n_in, int64_t mn,
                                  int64_t mx, bool marker) {
  obx_keyset_dev v;
  memset(&v, 0, sizeof(v));
  v.words = words;
  v.min = n_in ? mn : 1;
  v.max = n_in ? mx : -1;
  if (n_in == 0) {
    v.form = OBX_KS_EMPTY;
    return v;
  }
  v.form = form;
  v.hi = size - 1;
  v.has_marker = marker ? 1 : 0;
  v.shift = form == OBX_KS_HASH ? (uint8_t)(64 - obx_ks_log2(size)) : 0;
  return v;
}

static uint32_t keyset_grid(uint64_t n) {
  const uint64_t g = (n + OBX_WG_HOST - 1) / OBX_WG_HOST;
  return g > 4096 ? 4096u : (g ? (uint32_t)g : 1u);
}

/* the set of the non-null datums of a dense device vector */
static int keyset_build(obx_gpu_ctx *ctx, const uint8_t *d_src, uint32_t len,
                        uint32_t sign, const uint8_t *d_nulls,
                        uint32_t null_bit, uint64_t n, int kind) {
  if (kind < 0 || kind > 2 || n > OBX_KS_MAX_KEYS) return OBX_INVALID_ARGUMENT;
  dev_tmp<unsigned long long> scr;
  unsigned long long hs[KS_WORDS] = {(unsigned long long)INT64_MAX,
                                     (unsigned long long)INT64_MIN, 0, 0, 0};
  HIP_TRY(hipMalloc(&scr.p, sizeof(hs)));
  HIP_TRY(hipMemcpyAsync(scr.p, hs, sizeof(hs), hipMemcpyHostToDevice,
                         ctx->stream));
  if (n)
    hipLaunchKernelGGL(k_keyset_minmax, dim3(keyset_grid(n)),
                       dim3(OBX_WG_HOST), 0, ctx->stream, d_src, len, sign,
                       d_nulls, null_bit, n, scr.p);
  HIP_TRY(hipMemcpyAsync(hs, scr.p, sizeof(hs), hipMemcpyDeviceToHost,
                         ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const uint64_t n_in = hs[KS_COUNT];
  const int64_t mn = (int64_t)hs[KS_MIN], mx = (int64_t)hs[KS_MAX];

  uint8_t form;
  uint64_t size;
  if (obx_ks_choose(n_in, mn, mx, kind, &form, &size))
    return OBX_NOT_SUPPORTED;
  auto ks = std::make_unique<obx_keyset>();
  const uint64_t n_words = keyset_words(form, size);
  HIP_TRY(hipMalloc(&ks->d_words, n_words * 8));
  HIP_TRY(hipMemsetAsync(ks->d_words, form == OBX_KS_HASH ? 0xFF : 0,
                         n_words * 8, ctx->stream));
  if (n_in) {
    const obx_keyset_dev v = keyset_view(ks->d_words, form, size, n_in, mn, mx,
                                         false);
    hipLaunchKernelGGL(k_keyset_insert, dim3(keyset_grid(n)),
                       dim3(OBX_WG_HOST), 0, ctx->stream, d_src, len, sign,
                       d_nulls, null_bit, n, ks->d_words, v.hi, v.min,
                       (uint32_t)v.form, (uint32_t)v.shift, scr.p);
    HIP_TRY(hipMemcpyAsync(hs, scr.p, sizeof(hs), hipMemcpyDeviceToHost,
                           ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ks->view = keyset_view(ks->d_words, form, size, n_in, mn, mx,
                         hs[KS_MARKER] != 0);
  keyset_fill_info(&ks->info, n_in, hs[KS_DISTINCT], form, size, n_words, mn,
                   mx);
  ctx->keysets.push_back(std::move(ks));
  return (int)ctx->keysets.size() - 1;
}

extern "C" int obx_gpu_keyset_create(obx_gpu_ctx *ctx, const int64_t *keys,
                                     uint64_t n, int kind) {
  if (!ctx || (n && !keys)) return OBX_INVALID_ARGUMENT;
  if (n > OBX_KS_MAX_KEYS) return OBX_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(ctx->device));
  dev_tmp<uint8_t> d_keys;
  if (n) {
    HIP_TRY(hipMalloc(&d_keys.p, n * 8));
    HIP_TRY(hipMemcpy(d_keys.p, keys, n * 8, hipMemcpyHostToDevice));
  }
  return keyset_build(ctx, d_keys.p, 8, 1, nullptr, 0, n, kind);
}

extern "C" int obx_gpu_keyset_from_proj(obx_gpu_ctx *ctx, int handle,
                                        uint16_t proj_idx, int kind) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  const obx_handle &h = *hp;
  if (proj_idx >= h.sel_n_proj) return OBX_INVALID_ARGUMENT; /* no result */
  const obx_col_schema &cs = h.cols[h.sel_cols[proj_idx]];
  if (cs.len == 0 || cs.len > 8) return OBX_NOT_SUPPORTED;
  HIP_TRY(hipSetDevice(ctx->device));
  const uint32_t sign =
      obx_store_class(cs.obj_type) == OBX_SC_STRING ? 0u : 1u;
  return keyset_build(ctx, h.d_sel_out[proj_idx], cs.len, sign, h.d_sel_nulls,
                      proj_idx, h.sel_rows, kind);
}

extern "C" int obx_gpu_keyset_free(obx_gpu_ctx *ctx, int set_id) {
  if (!obx_keyset_lookup(ctx, set_id)) return OBX_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->keysets[(size_t)set_id].reset();
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_keyset_info(obx_gpu_ctx *ctx, int set_id,
                                   obx_keyset_info *out) {
  const obx_keyset *ks = obx_keyset_lookup(ctx, set_id);
  if (!ks || !out) return OBX_INVALID_ARGUMENT;
  *out = ks->info;
  return OBX_SUCCESS;
}

/* TEST INFRASTRUCTURE: the build and the probe over host memory, by the
   functions the kernels above and the filter kernels run. No HIP call. */
extern "C" int obx_gpu_keyset_host_model(const int64_t *keys, uint64_t n,
                                         int kind, const int64_t *probe,
                                         uint64_t m, uint8_t *hit,
                                         obx_keyset_info *info) {
  if ((n && !keys) || (m && (!probe || !hit)) || kind < 0 || kind > 2 ||
      n > OBX_KS_MAX_KEYS)
    return OBX_INVALID_ARGUMENT;
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  for (uint64_t i = 0; i < n; i++) {
    const int64_t v = obx_ks_load_key((const uint8_t *)keys, 8, 1, i);
    if (v < mn) mn = v;
    if (v > mx) mx = v;
  }
  uint8_t form;
  uint64_t size;
  if (obx_ks_choose(n, mn, mx, kind, &form, &size)) return OBX_NOT_SUPPORTED;
  const uint64_t n_words = keyset_words(form, size);
  std::vector<uint64_t> words(n_words,
                              form == OBX_KS_HASH ? OBX_KS_SLOT_EMPTY : 0);
  obx_keyset_dev v = keyset_view(words.data(), form, size, n, mn, mx, false);
  uint64_t marker = 0, distinct = 0;
  for (uint64_t i = 0; i < n; i++)
    distinct += obx_ks_insert(words.data(), v.hi, v.min, form, v.shift,
                              &marker,
                              obx_ks_load_key((const uint8_t *)keys, 8, 1, i));
  v = keyset_view(words.data(), form, size, n, mn, mx, marker != 0);
  for (uint64_t i = 0; i < m; i++)
    hit[i] = obx_keyset_probe(v, probe[i]) ? 1 : 0;
  if (info) keyset_fill_info(info, n, distinct, form, size, n_words, mn, mx);
  return OBX_SUCCESS;
}
