/*
 * obx_grouphash.h — the sized group table: the hash group-by's table past
 * OBX_GTABLE_BIG groups, in device memory, sized per scan from the cap the
 * caller grants (obx_gpu_set_max_groups). Layout, sizing and the inline
 * find-or-insert, shared by the host engine, the precompiled kernels
 * (k_scan_agg_hash, k_scan_join_agg_hash, k_group_hash_init, k_group_compact)
 * and obx_gpu_group_hash_host_model, which runs the very same functions over
 * host memory. No JIT source reads it, so build.sh does not embed it.
 *
 * The reference's hash group-by grows its table until the work area is spent
 * (ob_exec_hash_struct_vec.h:1718); here the work area is the cap, and the
 * table is sized once, before the scan, from what the host then knows.
 *
 * Layout: three arrays behind one base pointer, each `slots` long:
 *   keys    u64 per slot, OBX_KEY_EMPTY = free
 *   counts  u64 per slot, the group's row count
 *   cells   n_aggs cells of 4 u64 limbs per slot (slot-major)
 * i.e. 16 + 32 * n_aggs bytes per slot, whatever OBX_DEV_MAX_AGGS is (a gslot
 * costs 272). Three arrays, not one record array with a runtime stride,
 * because the probe sequence, the init's key fill and the compaction's
 * liveness test read keys only: eight keys share a 64-byte line, so a linear
 * probe of a few steps stays in the line it started in, where a strided
 * record would put every step on a line of its own (80 bytes at two
 * aggregates) and misalign the cells against lines. The price is that a row
 * touches three lines (key, count, cells) where a record would touch one or
 * two. Byte offsets are 64-bit: 2^26 slots of 272 bytes pass 2^32.
 *
 * Counter block of a sized-table scan (OBX_GH_COUNTER_WORDS u64, in front of
 * the table in the same allocation, 64-byte aligned):
 *   0..15   as the other scans': 0 passed (unused here), 1 LDS overflow
 *           (unused), 2 table full, 8..15 striped survivor sums
 *   16..23  striped counts of CAS winners = live keys (one 64-byte line; every
 *           workgroup reads it once per block as the stop word)
 *   24      k_group_compact's record cursor
 */
#ifndef OBX_GROUPHASH_H_
#define OBX_GROUPHASH_H_

#include "obx_dev.h"

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define OBX_GH_FN __host__ __device__ static __forceinline__
#else
#define OBX_GH_FN static inline
#endif

#define OBX_GH_MIN_SLOTS (1ull << 13)
#define OBX_GH_MAX_GROUPS (1ull << 24) /* largest cap a caller may grant */
#define OBX_GH_COUNTER_WORDS 32
#define OBX_GH_WINNERS 16 /* first of the 8 winner words */
#define OBX_GH_CURSOR 24

/* by-value view: what the kernels get */
typedef struct obx_gh_dev {
  unsigned long long *base; /* first key */
  uint64_t off_keys;        /* byte offsets of the three arrays from base */
  uint64_t off_counts;
  uint64_t off_cells;
  uint32_t log2_slots;
  uint32_t n_aggs;
} obx_gh_dev;

OBX_GH_FN uint64_t obx_gh_pow2ceil(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

/* THE sizing rule. cap = min(max_groups, bound): bound is an upper bound on
   the scan's surviving rows (the table's row count), so no scan has more
   groups than that. in_flight = the rows all workgroups together may insert
   between two looks at the stop word (grid x rows of the largest block). A
   scan that stays within max_groups then fills at most half the table; a
   refused one stops at no more than max_groups + in_flight live keys, which
   still leaves cap slots free. */
OBX_GH_FN uint64_t obx_gh_slots(uint64_t max_groups, uint64_t bound,
                                uint64_t in_flight) {
  const uint64_t cap = max_groups < bound ? max_groups : bound;
  const uint64_t s = obx_gh_pow2ceil(2 * cap + in_flight);
  return s < OBX_GH_MIN_SLOTS ? OBX_GH_MIN_SLOTS : s;
}

OBX_GH_FN uint32_t obx_gh_log2(uint64_t pow2) {
  uint32_t l = 0;
  while ((1ull << l) < pow2) l++;
  return l;
}

/* bytes of one slot over the three arrays = bytes of one compacted record */
OBX_GH_FN uint64_t obx_gh_slot_bytes(uint32_t n_aggs) {
  return 16 + 32 * (uint64_t)n_aggs;
}
OBX_GH_FN uint64_t obx_gh_table_bytes(uint64_t slots, uint32_t n_aggs) {
  return slots * obx_gh_slot_bytes(n_aggs);
}

OBX_GH_FN obx_gh_dev obx_gh_view(void *base, uint64_t slots, uint32_t n_aggs) {
  obx_gh_dev v;
  v.base = (unsigned long long *)base;
  v.off_keys = 0;
  v.off_counts = slots * 8;
  v.off_cells = slots * 16;
  v.log2_slots = obx_gh_log2(slots);
  v.n_aggs = n_aggs;
  return v;
}

OBX_GH_FN uint64_t obx_gh_n_slots(const obx_gh_dev &v) {
  return 1ull << v.log2_slots;
}
OBX_GH_FN unsigned long long *obx_gh_keys(const obx_gh_dev &v) {
  return (unsigned long long *)((char *)v.base + v.off_keys);
}
OBX_GH_FN unsigned long long *obx_gh_count(const obx_gh_dev &v, uint64_t s) {
  return (unsigned long long *)((char *)v.base + v.off_counts) + s;
}
OBX_GH_FN unsigned long long *obx_gh_cell(const obx_gh_dev &v, uint64_t s,
                                          uint32_t a) {
  return (unsigned long long *)((char *)v.base + v.off_cells) +
         (s * v.n_aggs + a) * 4;
}

/* gtable_home's hash (obx_steps.h) with a runtime shift */
OBX_GH_FN uint64_t obx_gh_home(uint64_t key, uint32_t log2_slots) {
  return ((key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots)) &
         ((1ull << log2_slots) - 1);
}

/* one slot's key as another workgroup may just have written it; slots are
   shared across XCDs, so agent scope on both the load and the CAS */
OBX_GH_FN unsigned long long obx_gh_load_key(unsigned long long *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
OBX_GH_FN unsigned long long obx_gh_cas_key(unsigned long long *p,
                                            unsigned long long key) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned long long expect = OBX_KEY_EMPTY;
  __hip_atomic_compare_exchange_strong(p, &expect, key, __ATOMIC_RELAXED,
                                       __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  return expect; /* the old word */
#else
  const unsigned long long old = *p;
  if (old == OBX_KEY_EMPTY) *p = key;
  return old;
#endif
}

/* find-or-insert, as gtable_slot: returns the key's slot, or -1 when `slots`
   probe steps found neither the key nor a free slot. *won = this call's CAS
   took a free slot (exactly one call per live key wins); *steps = probe
   steps taken (slots looked at). */
OBX_GH_FN int64_t obx_gh_find_or_insert(const obx_gh_dev &v, uint64_t key,
                                        bool *won, uint64_t *steps) {
  unsigned long long *keys = obx_gh_keys(v);
  const uint64_t mask = obx_gh_n_slots(v) - 1;
  uint64_t idx = obx_gh_home(key, v.log2_slots);
  *won = false;
  for (uint64_t probe = 0; probe <= mask; probe++) {
    *steps = probe + 1;
    const unsigned long long k = obx_gh_load_key(&keys[idx]);
    if (k == key) return (int64_t)idx;
    if (k == OBX_KEY_EMPTY) {
      const unsigned long long c = obx_gh_cas_key(&keys[idx], key);
      if (c == OBX_KEY_EMPTY) { *won = true; return (int64_t)idx; }
      if (c == key) return (int64_t)idx;
    }
    idx = (idx + 1) & mask;
  }
  return -1;
}

/* lookup only (the host model's "found again") */
OBX_GH_FN int64_t obx_gh_find(const obx_gh_dev &v, uint64_t key) {
  unsigned long long *keys = obx_gh_keys(v);
  const uint64_t mask = obx_gh_n_slots(v) - 1;
  uint64_t idx = obx_gh_home(key, v.log2_slots);
  for (uint64_t probe = 0; probe <= mask; probe++) {
    const unsigned long long k = obx_gh_load_key(&keys[idx]);
    if (k == key) return (int64_t)idx;
    if (k == OBX_KEY_EMPTY) return -1;
    idx = (idx + 1) & mask;
  }
  return -1;
}

/* what the host decides after the kernel: the scan stands iff every live key
   is within the grant and no row was turned away by a full table */
OBX_GH_FN bool obx_gh_refused(uint64_t live, uint64_t full_rows,
                              uint64_t max_groups) {
  return live > max_groups || full_rows != 0;
}

#endif /* OBX_GROUPHASH_H_ */
