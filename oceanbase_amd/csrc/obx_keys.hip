/*
 * obx_keys.hip — device-resident key sets and key maps: the build kernels
 * and the obx_gpu_keyset_* / obx_gpu_keymap_* verbs (include/obx.h). Layout,
 * sizing, insert and probe are the inline functions of obx_keyset.h and
 * obx_keymap.h: two different tables, one build.
 *
 * A set is the build side of a hash join handed to the probe side's table
 * scan (the reference ships ObRFInFilterVecMsg / ObRFRangeFilterVecMsg /
 * ObRFBloomFilterMsg from the join to the scan, sql/engine/px/p2p_datahub,
 * and evaluates them in ObExprJoinFilter); a map is that build side with its
 * payload column (the reference's ObHashJoinVecOp build phase,
 * sql/engine/join/hash_join). The build columns are already in device memory
 * (obx_gpu_scan_project leaves them there), so either is built where they
 * are, in three steps on the context's stream:
 *   k_key*_minmax   per-workgroup reduce, one atomic min / max / count per
 *                   workgroup; a map also counts the non-null keys with a
 *                   NULL payload
 *   host            reads them, chooses the form (obx_ks_choose /
 *                   obx_km_choose)
 *   k_key*_insert   atomicCAS into the hash table or atomicOr into the
 *                   bitmap; the CAS winners / first setters of a bit are
 *                   the distinct keys, summed per workgroup before one
 *                   atomicAdd. A map's winner stores its payload, and fewer
 *                   winners than keys read means a duplicate: the build
 *                   fails.
 * What both builds run exists once: the two kernel bodies (templated on
 * "has a payload"), keys_grid, the scratch words, keys_minmax (the first
 * step), view_common and host_minmax.
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
static_assert(OBX_KM_EMPTY == OBX_KS_EMPTY && OBX_KM_HASH == OBX_KS_HASH,
              "view_common sets either view's form");

/* the scratch words of a build; a map's extend a set's */
enum { KS_MIN = 0, KS_MAX = 1, KS_COUNT = 2, KS_DISTINCT = 3, KS_MARKER = 4,
       KM_MARKER_PAYLOAD = 5, KM_NULL_PAYLOADS = 6, KEY_WORDS = 7 };
static_assert(KM_MARKER_PAYLOAD == KS_MARKER + 1,
              "obx_km_insert takes the marker flag and payload as one pair");

/* ---- kernels ------------------------------------------------------------- */

template <bool PAY>
__device__ __forceinline__ void minmax_body(
    const uint8_t *__restrict__ src, uint32_t len, uint32_t sign,
    const uint8_t *__restrict__ nulls, uint32_t key_bit, uint32_t pay_bit,
    uint64_t n, unsigned long long *__restrict__ scr) {
  __shared__ int64_t smn[WAVES], smx[WAVES];
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  uint64_t cnt = 0, null_pay = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * WG) {
    if (nulls) {
      const uint8_t f = nulls[i];
      if ((f >> key_bit) & 1) continue;
      if constexpr (PAY) null_pay += (f >> pay_bit) & 1;
    }
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
  uint64_t total_np = 0;
  if constexpr (PAY) total_np = wg_sum(null_pay);
  if (threadIdx.x == 0 && total) {
    for (uint32_t w = 0; w < WAVES; w++) {
      if (smn[w] < mn) mn = smn[w];
      if (smx[w] > mx) mx = smx[w];
    }
    cas_minmax(&scr[KS_MIN], mn, true);
    cas_minmax(&scr[KS_MAX], mx, false);
    atomicAdd(&scr[KS_COUNT], (unsigned long long)total);
    if (total_np)
      atomicAdd(&scr[KM_NULL_PAYLOADS], (unsigned long long)total_np);
  }
}

template <bool PAY>
__device__ __forceinline__ void insert_body(
    const uint8_t *__restrict__ src, uint32_t len, uint32_t sign,
    const uint8_t *__restrict__ pay, uint32_t pay_len, uint32_t pay_sign,
    const uint8_t *__restrict__ nulls, uint32_t key_bit, uint64_t n,
    uint64_t *__restrict__ table, uint64_t *__restrict__ bits, uint64_t hi,
    int64_t mn, uint32_t form, uint32_t shift,
    unsigned long long *__restrict__ scr) {
  uint64_t won = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * WG) {
    if (nulls && ((nulls[i] >> key_bit) & 1)) continue;
    const int64_t key = obx_ks_load_key(src, len, sign, i);
    if constexpr (PAY)
      won += obx_km_insert(
          table, bits, hi, mn, form, shift, (uint64_t *)&scr[KS_MARKER], key,
          (uint64_t)obx_ks_load_key(pay, pay_len, pay_sign, i));
    else
      won += obx_ks_insert(table, hi, mn, form, shift,
                           (uint64_t *)&scr[KS_MARKER], key);
  }
  const uint64_t total = wg_sum(won);
  if (threadIdx.x == 0 && total)
    atomicAdd(&scr[KS_DISTINCT], (unsigned long long)total);
}

extern "C" __global__ __launch_bounds__(WG) void k_keyset_minmax(
    const uint8_t *__restrict__ src, uint32_t len, uint32_t sign,
    const uint8_t *__restrict__ nulls, uint32_t null_bit, uint64_t n,
    unsigned long long *__restrict__ scr) {
  minmax_body<false>(src, len, sign, nulls, null_bit, 0, n, scr);
}

extern "C" __global__ __launch_bounds__(WG) void k_keyset_insert(
    const uint8_t *__restrict__ src, uint32_t len, uint32_t sign,
    const uint8_t *__restrict__ nulls, uint32_t null_bit, uint64_t n,
    uint64_t *__restrict__ words, uint64_t hi, int64_t mn, uint32_t form,
    uint32_t shift, unsigned long long *__restrict__ scr) {
  insert_body<false>(src, len, sign, nullptr, 0, 0, nulls, null_bit, n, words,
                     nullptr, hi, mn, form, shift, scr);
}

extern "C" __global__ __launch_bounds__(WG) void k_keymap_minmax(
    const uint8_t *__restrict__ src, uint32_t len, uint32_t sign,
    const uint8_t *__restrict__ nulls, uint32_t key_bit, uint32_t pay_bit,
    uint64_t n, unsigned long long *__restrict__ scr) {
  minmax_body<true>(src, len, sign, nulls, key_bit, pay_bit, n, scr);
}

extern "C" __global__ __launch_bounds__(WG) void k_keymap_insert(
    const uint8_t *__restrict__ src, uint32_t len, uint32_t sign,
    const uint8_t *__restrict__ pay, uint32_t pay_len, uint32_t pay_sign,
    const uint8_t *__restrict__ nulls, uint32_t key_bit, uint64_t n,
    uint64_t *__restrict__ table, uint64_t *__restrict__ bits, uint64_t hi,
    int64_t mn, uint32_t form, uint32_t shift,
    unsigned long long *__restrict__ scr) {
  insert_body<true>(src, len, sign, pay, pay_len, pay_sign, nulls, key_bit, n,
                    table, bits, hi, mn, form, shift, scr);
}

/* ---- host: what both builds run ------------------------------------------- */

static uint32_t keys_grid(uint64_t n) {
  const uint64_t g = (n + OBX_WG_HOST - 1) / OBX_WG_HOST;
  return g > 4096 ? 4096u : (g ? (uint32_t)g : 1u);
}

/* what the first step of a build finds in a dense device vector of keys */
struct key_stats {
  uint64_t n_in;          /* non-null keys */
  int64_t mn, mx;         /* of those; INT64_MAX / INT64_MIN when none */
  uint64_t null_payloads; /* has_pay: non-null keys whose payload is NULL */
};

/* the first step of a build: allocate the scratch words and set them to
   their start values, run the minmax kernel (the map's when has_pay), read
   the words back into hs and wait. scr stays allocated for the insert. */
static int keys_minmax(obx_gpu_ctx *ctx, dev_tmp<unsigned long long> &scr,
                       unsigned long long hs[KEY_WORDS], const uint8_t *d_src,
                       uint32_t len, uint32_t sign, const uint8_t *d_nulls,
                       uint32_t key_bit, bool has_pay, uint32_t pay_bit,
                       uint64_t n, key_stats *out) {
  memset(hs, 0, KEY_WORDS * sizeof(hs[0]));
  hs[KS_MIN] = (unsigned long long)INT64_MAX;
  hs[KS_MAX] = (unsigned long long)INT64_MIN;
  const size_t bytes = KEY_WORDS * sizeof(hs[0]);
  HIP_TRY(hipMalloc(&scr.p, bytes));
  HIP_TRY(hipMemcpyAsync(scr.p, hs, bytes, hipMemcpyHostToDevice,
                         ctx->stream));
  if (n && has_pay)
    hipLaunchKernelGGL(k_keymap_minmax, dim3(keys_grid(n)), dim3(OBX_WG_HOST),
                       0, ctx->stream, d_src, len, sign, d_nulls, key_bit,
                       pay_bit, n, scr.p);
  else if (n)
    hipLaunchKernelGGL(k_keyset_minmax, dim3(keys_grid(n)), dim3(OBX_WG_HOST),
                       0, ctx->stream, d_src, len, sign, d_nulls, key_bit, n,
                       scr.p);
  HIP_TRY(hipMemcpyAsync(hs, scr.p, bytes, hipMemcpyDeviceToHost,
                         ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  out->n_in = hs[KS_COUNT];
  out->mn = (int64_t)hs[KS_MIN];
  out->mx = (int64_t)hs[KS_MAX];
  out->null_payloads = hs[KM_NULL_PAYLOADS];
  return OBX_SUCCESS;
}

/* what a set's and a map's view share (the fields have the same names):
   everything but the table pointers. min / max read 1 / -1 and the form is
   empty when there is no key. */
template <class VIEW>
static void view_common(VIEW *v, uint8_t form, uint64_t size, uint64_t n_in,
                        int64_t mn, int64_t mx, bool marker) {
  memset(v, 0, sizeof(*v));
  v->min = n_in ? mn : 1;
  v->max = n_in ? mx : -1;
  if (n_in == 0) {
    v->form = OBX_KS_EMPTY;
    return;
  }
  v->form = form;
  v->hi = size - 1;
  v->has_marker = marker ? 1 : 0;
  v->shift = form == OBX_KS_HASH ? (uint8_t)(64 - obx_ks_log2(size)) : 0;
}

/* min and max of the host models' keys */
static void host_minmax(const int64_t *keys, uint64_t n, int64_t *mn,
                        int64_t *mx) {
  *mn = INT64_MAX;
  *mx = INT64_MIN;
  for (uint64_t i = 0; i < n; i++) {
    const int64_t v = obx_ks_load_key((const uint8_t *)keys, 8, 1, i);
    if (v < *mn) *mn = v;
    if (v > *mx) *mx = v;
  }
}

/* ---- key sets ------------------------------------------------------------ */

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
  view_common(&v, form, size, n_in, mn, mx, marker);
  v.words = words;
  return v;
}

/* the set of the non-null datums of a dense device vector */
static int keyset_build(obx_gpu_ctx *ctx, const uint8_t *d_src, uint32_t len,
                        uint32_t sign, const uint8_t *d_nulls,
                        uint32_t null_bit, uint64_t n, int kind) {
  if (kind < 0 || kind > 2 || n > OBX_KS_MAX_KEYS) return OBX_INVALID_ARGUMENT;
  dev_tmp<unsigned long long> scr;
  unsigned long long hs[KEY_WORDS];
  key_stats st;
  int rc = keys_minmax(ctx, scr, hs, d_src, len, sign, d_nulls, null_bit,
                       false, 0, n, &st);
  if (rc != OBX_SUCCESS) return rc;

  uint8_t form;
  uint64_t size;
  if (obx_ks_choose(st.n_in, st.mn, st.mx, kind, &form, &size))
    return OBX_NOT_SUPPORTED;
  auto ks = std::make_unique<obx_keyset>();
  const uint64_t n_words = keyset_words(form, size);
  HIP_TRY(hipMalloc(&ks->d_words, n_words * 8));
  HIP_TRY(hipMemsetAsync(ks->d_words, form == OBX_KS_HASH ? 0xFF : 0,
                         n_words * 8, ctx->stream));
  if (st.n_in) {
    const obx_keyset_dev v = keyset_view(ks->d_words, form, size, st.n_in,
                                         st.mn, st.mx, false);
    hipLaunchKernelGGL(k_keyset_insert, dim3(keys_grid(n)), dim3(OBX_WG_HOST),
                       0, ctx->stream, d_src, len, sign, d_nulls, null_bit, n,
                       ks->d_words, v.hi, v.min, (uint32_t)v.form,
                       (uint32_t)v.shift, scr.p);
    HIP_TRY(hipMemcpyAsync(hs, scr.p, sizeof(hs), hipMemcpyDeviceToHost,
                           ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ks->view = keyset_view(ks->d_words, form, size, st.n_in, st.mn, st.mx,
                         hs[KS_MARKER] != 0);
  keyset_fill_info(&ks->info, st.n_in, hs[KS_DISTINCT], form, size, n_words,
                   st.mn, st.mx);
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
  int64_t mn, mx;
  host_minmax(keys, n, &mn, &mx);
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

/* ---- key maps ------------------------------------------------------------ */

const obx_keymap *obx_keymap_lookup(const obx_gpu_ctx *ctx, int64_t map_id) {
  if (!ctx || map_id < 0 || map_id >= (int64_t)ctx->keymaps.size())
    return nullptr;
  return ctx->keymaps[(size_t)map_id].get();
}

static uint32_t payload_sign(const obx_col_schema &cs) {
  return obx_store_class(cs.obj_type) == OBX_SC_STRING ? 0u : 1u;
}

/* info of a chosen form; min / max read 1 / -1 when there is no key */
static void keymap_fill_info(obx_keymap_info *info, uint64_t n, uint8_t form,
                             uint64_t size, int64_t mn, int64_t mx,
                             const obx_col_schema &pay) {
  memset(info, 0, sizeof(*info));
  info->n_keys = n;
  info->slots_or_span = size;
  info->bytes =
      8 * (obx_km_table_words(form, size) + obx_km_bit_words(form, size));
  info->min = n ? mn : 1;
  info->max = n ? mx : -1;
  info->kind = form;
  info->payload_len = pay.len;
  info->payload_type = pay.obj_type;
}

/* the view over a table of obx_km_table_words words followed by the bitmap */
static obx_keymap_dev keymap_view(const uint64_t *words, uint8_t form,
                                  uint64_t size, uint64_t n, int64_t mn,
                                  int64_t mx, bool marker,
                                  uint64_t marker_payload) {
  obx_keymap_dev v;
  view_common(&v, form, size, n, mn, mx, marker);
  v.table = words;
  v.bits = words + obx_km_table_words(form, size);
  v.marker_payload = v.has_marker ? marker_payload : 0;
  return v;
}

/* the map from the non-null datums of one dense device vector to the datums
   of another; d_nulls == nullptr = nothing is null */
static int keymap_build(obx_gpu_ctx *ctx, const uint8_t *d_keys, uint32_t len,
                        uint32_t sign, const uint8_t *d_pay,
                        const obx_col_schema &pay, const uint8_t *d_nulls,
                        uint32_t key_bit, uint32_t pay_bit, uint64_t n,
                        int kind) {
  if (kind < 0 || kind > 2 || n > OBX_KM_MAX_KEYS) return OBX_INVALID_ARGUMENT;
  const uint32_t psign = payload_sign(pay);
  dev_tmp<unsigned long long> scr;
  unsigned long long hs[KEY_WORDS];
  key_stats st;
  int rc = keys_minmax(ctx, scr, hs, d_keys, len, sign, d_nulls, key_bit,
                       true, pay_bit, n, &st);
  if (rc != OBX_SUCCESS) return rc;
  if (st.null_payloads != 0) return OBX_NOT_SUPPORTED;

  uint8_t form;
  uint64_t size;
  if (obx_km_choose(st.n_in, st.mn, st.mx, kind, &form, &size))
    return OBX_NOT_SUPPORTED;
  auto km = std::make_unique<obx_keymap>();
  const uint64_t t_words = obx_km_table_words(form, size);
  const uint64_t b_words = obx_km_bit_words(form, size);
  /* at least one slot, so there is always memory to point at */
  HIP_TRY(hipMalloc(&km->d_table, (t_words + b_words + 2) * 8));
  if (form == OBX_KM_HASH)
    HIP_TRY(hipMemsetAsync(km->d_table, 0xFF, t_words * 8, ctx->stream));
  else if (b_words)
    HIP_TRY(hipMemsetAsync(km->d_table + t_words, 0, b_words * 8,
                           ctx->stream));
  if (st.n_in) {
    const obx_keymap_dev v = keymap_view(km->d_table, form, size, st.n_in,
                                         st.mn, st.mx, false, 0);
    hipLaunchKernelGGL(k_keymap_insert, dim3(keys_grid(n)), dim3(OBX_WG_HOST),
                       0, ctx->stream, d_keys, len, sign, d_pay,
                       (uint32_t)pay.len, psign, d_nulls, key_bit, n,
                       km->d_table, km->d_table + t_words, v.hi, v.min,
                       (uint32_t)v.form, (uint32_t)v.shift, scr.p);
    HIP_TRY(hipMemcpyAsync(hs, scr.p, sizeof(hs), hipMemcpyDeviceToHost,
                           ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (hs[KS_DISTINCT] != st.n_in) return OBX_INVALID_ARGUMENT; /* duplicate */
  km->view = keymap_view(km->d_table, form, size, st.n_in, st.mn, st.mx,
                         hs[KS_MARKER] != 0, hs[KM_MARKER_PAYLOAD]);
  keymap_fill_info(&km->info, st.n_in, form, size, st.mn, st.mx, pay);
  ctx->keymaps.push_back(std::move(km));
  return (int)ctx->keymaps.size() - 1;
}

static int payload_check(const obx_col_schema *pay) {
  if (!pay) return OBX_INVALID_ARGUMENT;
  if (pay->len == 0 || pay->len > 8) return OBX_NOT_SUPPORTED;
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_keymap_create(obx_gpu_ctx *ctx, const int64_t *keys,
                                     const uint8_t *payloads, uint64_t n,
                                     const obx_col_schema *payload, int kind) {
  if (!ctx || (n && (!keys || !payloads))) return OBX_INVALID_ARGUMENT;
  int rc = payload_check(payload);
  if (rc != OBX_SUCCESS) return rc;
  if (n > OBX_KM_MAX_KEYS) return OBX_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(ctx->device));
  dev_tmp<uint8_t> d_keys, d_pay;
  if (n) {
    HIP_TRY(hipMalloc(&d_keys.p, n * 8));
    HIP_TRY(hipMemcpy(d_keys.p, keys, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&d_pay.p, n * payload->len));
    HIP_TRY(hipMemcpy(d_pay.p, payloads, n * payload->len,
                      hipMemcpyHostToDevice));
  }
  return keymap_build(ctx, d_keys.p, 8, 1, d_pay.p, *payload, nullptr, 0, 0,
                      n, kind);
}

extern "C" int obx_gpu_keymap_from_proj(obx_gpu_ctx *ctx, int handle,
                                        uint16_t key_idx,
                                        uint16_t payload_idx, int kind) {
  obx_handle *hp = obx_handle_lookup(ctx, handle);
  if (!hp) return OBX_INVALID_ARGUMENT;
  const obx_handle &h = *hp;
  if (key_idx >= h.sel_n_proj || payload_idx >= h.sel_n_proj)
    return OBX_INVALID_ARGUMENT; /* no result */
  const obx_col_schema &ks = h.cols[h.sel_cols[key_idx]];
  const obx_col_schema &ps = h.cols[h.sel_cols[payload_idx]];
  if (ks.len == 0 || ks.len > 8) return OBX_NOT_SUPPORTED;
  int rc = payload_check(&ps);
  if (rc != OBX_SUCCESS) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return keymap_build(ctx, h.d_sel_out[key_idx], ks.len, payload_sign(ks),
                      h.d_sel_out[payload_idx], ps, h.d_sel_nulls, key_idx,
                      payload_idx, h.sel_rows, kind);
}

extern "C" int obx_gpu_keymap_free(obx_gpu_ctx *ctx, int map_id) {
  if (!obx_keymap_lookup(ctx, map_id)) return OBX_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->keymaps[(size_t)map_id].reset();
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_keymap_info(obx_gpu_ctx *ctx, int map_id,
                                   obx_keymap_info *out) {
  const obx_keymap *km = obx_keymap_lookup(ctx, map_id);
  if (!km || !out) return OBX_INVALID_ARGUMENT;
  *out = km->info;
  return OBX_SUCCESS;
}

/* TEST INFRASTRUCTURE: the build and the probe over host memory, by the
   functions the kernels above and the join kernels run. No HIP call. */
extern "C" int obx_gpu_keymap_host_model(
    const int64_t *keys, const uint8_t *payloads, uint64_t n,
    const obx_col_schema *payload, int kind, const int64_t *probe, uint64_t m,
    uint8_t *hit, uint64_t *out_payload, obx_keymap_info *info) {
  if ((n && (!keys || !payloads)) || (m && !probe) || kind < 0 || kind > 2 ||
      n > OBX_KM_MAX_KEYS)
    return OBX_INVALID_ARGUMENT;
  int rc = payload_check(payload);
  if (rc != OBX_SUCCESS) return rc;
  const uint32_t psign = payload_sign(*payload);
  int64_t mn, mx;
  host_minmax(keys, n, &mn, &mx);
  uint8_t form;
  uint64_t size;
  if (obx_km_choose(n, mn, mx, kind, &form, &size)) return OBX_NOT_SUPPORTED;
  const uint64_t t_words = obx_km_table_words(form, size);
  const uint64_t b_words = obx_km_bit_words(form, size);
  /* held as slots, so the hash form's 16-byte loads are aligned */
  const uint64_t fill = form == OBX_KM_HASH ? OBX_KS_SLOT_EMPTY : 0;
  std::vector<obx_km_slot> store((t_words + b_words + 3) / 2,
                                 obx_km_slot{fill, fill});
  uint64_t *const table = &store[0].key;
  obx_keymap_dev v = keymap_view(table, form, size, n, mn, mx, false, 0);
  uint64_t marker[2] = {0, 0}, distinct = 0;
  for (uint64_t i = 0; i < n; i++)
    distinct += obx_km_insert(
        table, table + t_words, v.hi, v.min, form, v.shift,
        marker, obx_ks_load_key((const uint8_t *)keys, 8, 1, i),
        (uint64_t)obx_ks_load_key(payloads, payload->len, psign, i));
  if (distinct != n) return OBX_INVALID_ARGUMENT; /* a duplicate */
  v = keymap_view(table, form, size, n, mn, mx, marker[0] != 0, marker[1]);
  for (uint64_t i = 0; i < m; i++) {
    uint64_t pv = 0;
    const bool found = obx_keymap_probe(v, probe[i], &pv);
    if (hit) hit[i] = found ? 1 : 0;
    if (out_payload) out_payload[i] = found ? pv : 0;
  }
  if (info) keymap_fill_info(info, n, form, size, mn, mx, *payload);
  return OBX_SUCCESS;
}
