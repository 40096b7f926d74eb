/*
 * obx_keyset.h — device-resident key set: layout and the inline functions
 * that size, fill and probe it. Shared by the host engine, the precompiled
 * kernels and the hipRTC-generated kernels (build.sh embeds this file next
 * to obx_dev.h), and by obx_gpu_keyset_host_model, which runs the very same
 * functions over host memory.
 *
 * The set is what a hash join's build side pushes into the probe side's
 * table scan: the exact forms of the reference's runtime filters
 * (ObRFInFilterVecMsg / ObRFRangeFilterVecMsg under
 * sql/engine/px/p2p_datahub, evaluated by ObExprJoinFilter) and of the white
 * IN filter's parameter hash set (ObWhiteFilterExecutor with
 * ObWhiteFilterParamHashSet, ob_pushdown_filter.h). Two forms:
 *   bitmap  bit (v - min) per key v, u64 words, LSB-first. Chosen when it
 *           is no larger than the hash table would be.
 *   hash    open addressing over slots = max(64, pow2ceil(2 n)) u64 keys
 *           (fill <= 50 %), multiplicative hash, linear probe bounded by
 *           slots. The all-ones word marks an empty slot, so the key with
 *           that bit pattern (-1) is never stored: a flag in the header
 *           says whether the set holds it.
 */
#ifndef OBX_KEYSET_H_
#define OBX_KEYSET_H_

#include "obx_dev.h"

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define OBX_KS_FN __host__ __device__ static inline
#else
#define OBX_KS_FN static inline
#endif

enum {
  OBX_KS_EMPTY = 0,  /* no key: nothing passes */
  OBX_KS_HASH = 1,
  OBX_KS_BITMAP = 2,
};

#define OBX_KS_SLOT_EMPTY 0xFFFFFFFFFFFFFFFFull
#define OBX_KS_MIN_SLOTS 64ull
/* hard cap of a bitmap's span in bits (1 GiB of words) */
#define OBX_KS_MAX_SPAN (1ull << 33)
/* most keys one set is built from */
#define OBX_KS_MAX_KEYS (1ull << 31)

/* what a probe needs; travels in a set leaf's dev_leaf.in_list words */
typedef struct obx_keyset_dev {
  const uint64_t *words; /* hash slots or bitmap words (device memory) */
  uint64_t hi;           /* hash: slots - 1; bitmap: span - 1 */
  int64_t min, max;      /* of the keys; min > max = empty */
  uint8_t form;          /* OBX_KS_* */
  uint8_t has_marker;    /* hash: the set holds the key -1 */
  uint8_t shift;         /* hash: 64 - log2(slots) */
} obx_keyset_dev;

/* ---- sizing ------------------------------------------------------------- */
OBX_KS_FN uint64_t obx_ks_pow2ceil(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

OBX_KS_FN uint64_t obx_ks_hash_slots(uint64_t n) {
  const uint64_t s = obx_ks_pow2ceil(2 * n);
  return s < OBX_KS_MIN_SLOTS ? OBX_KS_MIN_SLOTS : s;
}

OBX_KS_FN uint32_t obx_ks_log2(uint64_t pow2) {
  uint32_t l = 0;
  while ((1ull << l) < pow2) l++;
  return l;
}

/* form and size of the set of n keys in [mn, mx]. kind: 0 auto, 1 hash,
   2 bitmap. *size = hash slots or bitmap bits. Returns 0, or 1 when a
   bitmap is asked for (kind 2) over a span past OBX_KS_MAX_SPAN. The span
   is kept as span - 1 in unsigned arithmetic: max - min + 1 itself
   overflows for {INT64_MIN, INT64_MAX}. */
OBX_KS_FN int obx_ks_choose(uint64_t n, int64_t mn, int64_t mx, int kind,
                            uint8_t *form, uint64_t *size) {
  const uint64_t slots = obx_ks_hash_slots(n);
  if (n == 0) { /* empty: no span */
    *form = kind == 2 ? OBX_KS_BITMAP : OBX_KS_HASH;
    *size = kind == 2 ? 0 : slots;
    return 0;
  }
  const uint64_t span_m1 = (uint64_t)mx - (uint64_t)mn;
  const int fits_cap = span_m1 < OBX_KS_MAX_SPAN;
  if (kind == 2 && !fits_cap) return 1;
  /* auto: a bitmap no larger than the hash table (span <= 64 * slots) */
  if (kind == 2 || (kind == 0 && fits_cap && span_m1 < 64 * slots)) {
    *form = OBX_KS_BITMAP;
    *size = span_m1 + 1;
    return 0;
  }
  *form = OBX_KS_HASH;
  *size = slots;
  return 0;
}

/* ---- the table ---------------------------------------------------------- */
OBX_KS_FN uint64_t obx_ks_hash(uint64_t key, uint32_t shift) {
  return (key * 0x9E3779B97F4A7C15ull) >> shift;
}

/* compare-and-swap / or of one table word: atomics on the device, plain
   code in the single-threaded host model. Both return the old word. */
OBX_KS_FN uint64_t obx_ks_cas(uint64_t *p, uint64_t expect, uint64_t val) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint64_t)atomicCAS((unsigned long long *)p,
                             (unsigned long long)expect,
                             (unsigned long long)val);
#else
  const uint64_t old = *p;
  if (old == expect) *p = val;
  return old;
#endif
}
OBX_KS_FN uint64_t obx_ks_or(uint64_t *p, uint64_t val) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint64_t)atomicOr((unsigned long long *)p, (unsigned long long)val);
#else
  const uint64_t old = *p;
  *p = old | val;
  return old;
#endif
}

/* insert one key; returns 1 if this call made the key a member (the CAS
   winner, or the first setter of the bit), 0 if it already was one. The
   key -1 of a hash set goes to *marker instead of a slot. */
OBX_KS_FN uint32_t obx_ks_insert(uint64_t *words, uint64_t hi, int64_t mn,
                                 uint32_t form, uint32_t shift,
                                 uint64_t *marker, int64_t key) {
  if (form == OBX_KS_BITMAP) {
    const uint64_t idx = (uint64_t)key - (uint64_t)mn;
    if (idx > hi) return 0;
    const uint64_t bit = 1ull << (idx & 63);
    return (obx_ks_or(&words[idx >> 6], bit) & bit) ? 0u : 1u;
  }
  const uint64_t k = (uint64_t)key;
  if (k == OBX_KS_SLOT_EMPTY) return obx_ks_or(marker, 1) ? 0u : 1u;
  uint64_t s = obx_ks_hash(k, shift) & hi;
  for (uint64_t i = 0; i <= hi; i++) {
    const uint64_t old = obx_ks_cas(&words[s], OBX_KS_SLOT_EMPTY, k);
    if (old == OBX_KS_SLOT_EMPTY) return 1;
    if (old == k) return 0;
    s = (s + 1) & hi;
  }
  return 0; /* unreachable at <= 50 % fill */
}

/* bitmap row test on idx = value - min (mod 2^64): a value below min wraps
   past hi and is rejected by the same compare */
OBX_KS_FN bool obx_ks_bit_test(const uint64_t *words, uint64_t idx,
                               uint64_t hi) {
  return idx <= hi && ((words[idx >> 6] >> (idx & 63)) & 1);
}

OBX_KS_FN bool obx_ks_hash_test(const uint64_t *words, uint64_t hi,
                                uint32_t shift, uint32_t has_marker,
                                uint64_t key) {
  if (key == OBX_KS_SLOT_EMPTY) return has_marker != 0;
  uint64_t s = obx_ks_hash(key, shift) & hi;
  for (uint64_t i = 0; i <= hi; i++) {
    const uint64_t k = words[s];
    if (k == key) return true;
    if (k == OBX_KS_SLOT_EMPTY) return false;
    s = (s + 1) & hi;
  }
  return false;
}

/* the membership test every filter path calls */
OBX_KS_FN bool obx_keyset_probe(const obx_keyset_dev &ks, int64_t v) {
  if (ks.form == OBX_KS_BITMAP)
    return obx_ks_bit_test(ks.words, (uint64_t)v - (uint64_t)ks.min, ks.hi);
  if (ks.form == OBX_KS_HASH)
    return obx_ks_hash_test(ks.words, ks.hi, ks.shift, ks.has_marker,
                            (uint64_t)v);
  return false;
}

/* ---- a set leaf's view, in the leaf's in_list words --------------------- */
OBX_KS_FN void obx_keyset_to_leaf(const obx_keyset_dev &ks, int64_t w[8]) {
  w[0] = (int64_t)(uint64_t)ks.words;
  w[1] = (int64_t)ks.hi;
  w[2] = ks.min;
  w[3] = ks.max;
  w[4] = (int64_t)((uint64_t)ks.form | ((uint64_t)ks.has_marker << 8) |
                   ((uint64_t)ks.shift << 16));
  w[5] = w[6] = w[7] = 0;
}

OBX_KS_FN obx_keyset_dev obx_leaf_keyset(const dev_leaf &lf) {
  obx_keyset_dev ks;
  ks.words = (const uint64_t *)(uint64_t)lf.in_list[0];
  ks.hi = (uint64_t)lf.in_list[1];
  ks.min = lf.in_list[2];
  ks.max = lf.in_list[3];
  const uint64_t f = (uint64_t)lf.in_list[4];
  ks.form = (uint8_t)f;
  ks.has_marker = (uint8_t)(f >> 8);
  ks.shift = (uint8_t)(f >> 16);
  return ks;
}

/* ---- build input: datum i of a dense vector of len-byte datums, widened
   to int64 (sign-extended for numeric types as col_value2 does,
   zero-extended for char) ------------------------------------------------- */
OBX_KS_FN int64_t obx_ks_load_key(const uint8_t *src, uint32_t len,
                                  uint32_t sign, uint64_t i) {
  const uint8_t *p = src + i * len;
  uint64_t v = 0;
  for (uint32_t k = 0; k < len && k < 8; k++) v |= (uint64_t)p[k] << (8 * k);
  if (sign && len < 8) {
    const uint32_t sh = 64 - 8 * len;
    return ((int64_t)(v << sh)) >> sh;
  }
  return (int64_t)v;
}

#endif /* OBX_KEYSET_H_ */
