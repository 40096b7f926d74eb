/*
 * obx_keymap.h — device-resident key map: layout and the inline functions
 * that size, fill and probe it, and what a join scan carries to its kernels.
 * Shared by the host engine, the precompiled kernels (obx_keys.hip,
 * obx_join.hip) and obx_gpu_keymap_host_model, which runs the very same
 * functions over host memory. No JIT source reads it, so build.sh does not
 * embed it.
 *
 * A map is the build side of a hash join with its payload column: the
 * reference's ObHashJoinVecOp builds a hash table over the build rows and
 * probes it per probe row (sql/engine/join/hash_join, ob_hash_join_vec_op.cpp
 * and its hash_table/ directory); here the table is built once, where
 * obx_gpu_scan_project left the build columns, and probed inside the probe
 * side's table scan. It reuses the key set's hash, CAS / OR, sizing and
 * empty-slot conventions (obx_keyset.h). Keys are distinct; the payload is
 * one datum of 1..8 bytes kept widened to 64 bits by obx_ks_load_key's rule.
 * Two exact forms:
 *   hash    open addressing over slots = obx_ks_hash_slots(n) slots of 16
 *           bytes {key, payload}: one 16-byte load answers a probe step.
 *           Linear probe bounded by slots. The all-ones key word marks an
 *           empty slot, so the key -1 is never stored: the header holds a
 *           marker flag and the marker's payload.
 *   dense   payload[key - min] as u64 plus a presence bitmap (u64 words,
 *           LSB-first). Chosen when span - 1 < 2 * slots, i.e. when it is
 *           about the size of the hash table; never past OBX_KM_MAX_SPAN.
 */
#ifndef OBX_KEYMAP_H_
#define OBX_KEYMAP_H_

#include "obx_keyset.h"

/* the probe-side functions are inlined into the scan kernels, so the
   by-value dev_join stays in kernel-argument memory */
#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define OBX_KM_FN __host__ __device__ static __forceinline__
#else
#define OBX_KM_FN static inline
#endif

enum {
  OBX_KM_EMPTY = 0, /* no key: nothing joins */
  OBX_KM_HASH = 1,
  OBX_KM_DENSE = 2,
};

/* hard cap of a dense map's span in entries (2 GiB of payloads) */
#define OBX_KM_MAX_SPAN (1ull << 28)
/* most keys one map is built from */
#define OBX_KM_MAX_KEYS (1ull << 27)

/* one hash slot; 16-byte aligned so a probe step is one load */
typedef struct __attribute__((aligned(16))) obx_km_slot {
  uint64_t key, payload;
} obx_km_slot;

/* what a probe needs; travels to the join kernels by value in dev_join */
typedef struct obx_keymap_dev {
  const uint64_t *table;   /* hash: the slots; dense: the payloads */
  const uint64_t *bits;    /* dense: presence bitmap */
  uint64_t hi;             /* hash: slots - 1; dense: span - 1 */
  int64_t min, max;        /* of the keys; min > max = empty */
  uint64_t marker_payload; /* hash: payload of the key -1 */
  uint8_t form;            /* OBX_KM_* */
  uint8_t has_marker;      /* hash: the map holds the key -1 */
  uint8_t shift;           /* hash: 64 - log2(slots) */
} obx_keymap_dev;

/* form and size of the map of n keys in [mn, mx]. kind: 0 auto, 1 hash,
   2 dense. *size = hash slots or dense entries. Returns 0, or 1 when dense
   is asked for (kind 2) over a span past OBX_KM_MAX_SPAN. The span is kept
   as span - 1 in unsigned arithmetic, as in obx_ks_choose. */
OBX_KS_FN int obx_km_choose(uint64_t n, int64_t mn, int64_t mx, int kind,
                            uint8_t *form, uint64_t *size) {
  const uint64_t slots = obx_ks_hash_slots(n);
  if (n == 0) { /* empty: no span */
    *form = kind == 2 ? OBX_KM_DENSE : OBX_KM_HASH;
    *size = kind == 2 ? 0 : slots;
    return 0;
  }
  const uint64_t span_m1 = (uint64_t)mx - (uint64_t)mn;
  const int fits_cap = span_m1 < OBX_KM_MAX_SPAN;
  if (kind == 2 && !fits_cap) return 1;
  if (kind == 2 || (kind == 0 && fits_cap && span_m1 < 2 * slots)) {
    *form = OBX_KM_DENSE;
    *size = span_m1 + 1;
    return 0;
  }
  *form = OBX_KM_HASH;
  *size = slots;
  return 0;
}

/* u64 words of the table and of the dense bitmap */
OBX_KS_FN uint64_t obx_km_table_words(uint8_t form, uint64_t size) {
  return form == OBX_KM_HASH ? 2 * size : size;
}
OBX_KS_FN uint64_t obx_km_bit_words(uint8_t form, uint64_t size) {
  return form == OBX_KM_DENSE ? (size + 63) / 64 : 0;
}

/* insert one key with its payload; returns 1 if this call made the key a
   member (the CAS winner, or the first setter of the presence bit), 0 if it
   already was one. Only the winner stores its payload, with a plain store:
   probes run in later kernels. marker[0] is the flag of the key -1 of a
   hash map, marker[1] its payload. */
OBX_KS_FN uint32_t obx_km_insert(uint64_t *table, uint64_t *bits, uint64_t hi,
                                 int64_t mn, uint32_t form, uint32_t shift,
                                 uint64_t *marker, int64_t key,
                                 uint64_t payload) {
  if (form == OBX_KM_DENSE) {
    const uint64_t idx = (uint64_t)key - (uint64_t)mn;
    if (idx > hi) return 0;
    const uint64_t bit = 1ull << (idx & 63);
    if (obx_ks_or(&bits[idx >> 6], bit) & bit) return 0;
    table[idx] = payload;
    return 1;
  }
  const uint64_t k = (uint64_t)key;
  if (k == OBX_KS_SLOT_EMPTY) {
    if (obx_ks_or(&marker[0], 1)) return 0;
    marker[1] = payload;
    return 1;
  }
  uint64_t s = obx_ks_hash(k, shift) & hi;
  for (uint64_t i = 0; i <= hi; i++) {
    const uint64_t old = obx_ks_cas(&table[2 * s], OBX_KS_SLOT_EMPTY, k);
    if (old == OBX_KS_SLOT_EMPTY) {
      table[2 * s + 1] = payload;
      return 1;
    }
    if (old == k) return 0;
    s = (s + 1) & hi;
  }
  return 0; /* unreachable at <= 50 % fill */
}

/* the probe every join path calls: true and *payload (widened) iff v is a
   key. Dense tests idx = v - min (mod 2^64) by the key set's bitmap rule: a
   value below min wraps past hi and is rejected by the same compare. */
OBX_KM_FN bool obx_keymap_probe(const obx_keymap_dev &km, int64_t v,
                                uint64_t *payload) {
  if (km.form == OBX_KM_DENSE) {
    const uint64_t idx = (uint64_t)v - (uint64_t)km.min;
    if (!obx_ks_bit_test(km.bits, idx, km.hi)) return false;
    *payload = km.table[idx];
    return true;
  }
  if (km.form == OBX_KM_HASH) {
    const uint64_t key = (uint64_t)v;
    if (key == OBX_KS_SLOT_EMPTY) {
      *payload = km.marker_payload;
      return km.has_marker != 0;
    }
    const obx_km_slot *slots = (const obx_km_slot *)km.table;
    uint64_t s = obx_ks_hash(key, km.shift) & km.hi;
    for (uint64_t i = 0; i <= km.hi; i++) {
      const obx_km_slot e = slots[s];
      if (e.key == key) {
        *payload = e.payload;
        return true;
      }
      if (e.key == OBX_KS_SLOT_EMPTY) return false;
      s = (s + 1) & km.hi;
    }
  }
  return false;
}

/* ---- what obx_gpu_scan_join_agg hands its kernels, by value ------------- */
typedef struct dev_join {
  obx_keymap_dev km;
  uint8_t probe_idx; /* need slot (dev_plan_hdr.need_cols) of the probe col */
  uint8_t pay_len;   /* payload datum bytes */
  uint8_t pay_group; /* 1: the payload is a group column */
  uint8_t pay_pos;   /* ... at this position of the group key (0 or 1) */
  uint8_t real_len;  /* datum bytes of the other group column, 0 = none */
  uint8_t own_mask;  /* bit a: cell a is a payload aggregate, accumulated by
                        the join step; the plan holds COUNT(*) in its place */
  uint8_t kind[OBX_DEV_MAX_AGGS]; /* what every cell holds: the payload
                                     aggregate's kind for a cell of own_mask,
                                     else the plan's */
} dev_join;

/* the group key of a joined row: rk is the key of the real group columns as
   the plan (which does not know the payload) builds it, i.e. at most one
   column at position 0 with its NULL flag in bit 56. The payload's bytes go
   to their position; a real column that moves to position 1 takes its NULL
   flag to bit 57. pay_len + real_len <= 7 keeps the flag byte free. */
OBX_KM_FN uint64_t obx_join_key(const dev_join &dj, uint64_t rk, uint64_t pv) {
  if (!dj.pay_group) return rk;
  pv &= (1ull << (8 * dj.pay_len)) - 1;
  if (dj.pay_pos != 0) return rk | (pv << (8 * dj.real_len));
  const uint64_t data = rk & ((1ull << (8 * dj.real_len)) - 1);
  return pv | (data << (8 * dj.pay_len)) | (((rk >> 56) & 1) << 57);
}

#endif /* OBX_KEYMAP_H_ */
