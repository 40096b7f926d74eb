/*
 * obx_jit_dev.h — plan-independent device helpers of the hipRTC-generated
 * kernels (obx_jit_scan.inc, obx_jit_filter.inc). Everything a generator
 * would otherwise paste verbatim into every source lives here once;
 * build.sh embeds this file for hipRTC next to obx_dev.h and
 * obx_dev_common.h, and generated sources include it after
 * obx_dev_common.h (whose types, WG and table constants it uses).
 */
#ifndef OBX_JIT_DEV_H
#define OBX_JIT_DEV_H

/* packed width in bits of a column's data stream */
#define PW(dc)                                              \
  (((dc).flags & OBX_DF_BITPACK) ? (uint32_t)(dc).width     \
                                 : (uint32_t)(dc).width * 8u)

/* LDS-DMA stage of one block; the partial tail chunk is handled
   by the exec mask (the LDS destination must stay uniform +
   lane-linear for global_load_lds addressing) */
__device__ __forceinline__ void stage2(
    const uint8_t *__restrict__ buf, uint64_t block_byte, uint32_t block_len,
    uint8_t *dst) {
  const uint32_t n16 = (block_len + 15) >> 4;
  const uint8_t *src = buf + block_byte;
  for (uint32_t i = threadIdx.x; i < n16; i += WG) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) uint32_t
             *)(src + (size_t)i * 16),
        (__attribute__((address_space(3))) uint32_t
             *)(dst + (size_t)i * 16),
        16, 0, 0);
  }
}

__device__ __forceinline__ void stage2(
    const uint8_t *__restrict__ buf, const dev_block &blk,
    uint8_t *dst) {
  stage2(buf, blk.block_byte, blk.block_len, dst);
}

/* A blk_leaf (32 B) as its four u64 words, for the scan's packed-descriptor
   path: mi holds mode in bits 0-7 and invert in bits 8-15. Whole-word loads
   of a wave-uniform address stay scalar; the byte fields read through the
   struct compile to vector byte loads. */
struct jit_leafw {
  uint64_t mask, lo, hi, mi;
};
typedef uint64_t __attribute__((may_alias)) jit_u64a;
__device__ __forceinline__ jit_leafw jit_load_leafw(
    const blk_leaf *__restrict__ p) {
  const jit_u64a *w = (const jit_u64a *)p;
  jit_leafw l;
  l.mask = w[0];
  l.lo = w[1];
  l.hi = w[2];
  l.mi = w[3];
  return l;
}
__device__ __forceinline__ blk_leaf jit_leaf_of(const jit_leafw &w) {
  blk_leaf l;
  l.mask = w.mask;
  l.lo = w.lo;
  l.hi = w.hi;
  l.mode = (uint8_t)w.mi;
  l.invert = (uint8_t)(w.mi >> 8);
  return l;
}
/* leaf_class (obx_dev_common.h) over a jit_leafw and the leaf column's
   dev_col flags */
__device__ __forceinline__ uint8_t jit_leaf_class(const jit_leafw &w,
                                                  uint32_t col_flags) {
  const uint8_t mode = (uint8_t)w.mi;
  if (mode == OBX_LEAF_NONE) return 0;
  if (mode == OBX_LEAF_ALL && !(col_flags & OBX_DF_HAS_EXT)) return 1;
  return 2;
}

/* 32-bit-offset packed read from an 8-B-aligned base */
__device__ __forceinline__ uint64_t jit_bread(
    const uint8_t *__restrict__ b, uint32_t bitpos, uint32_t k) {
  const uint64_t *w = (const uint64_t *)b;
  uint32_t widx = bitpos >> 6, sh = bitpos & 63;
  uint64_t v = w[widx] >> sh;
  if (sh + k > 64) v |= w[widx + 1] << (64 - sh);
  if (k < 64) v &= (((uint64_t)1 << k) - 1);
  return v;
}

/* the 32 bits at bitpos from a 4-B-aligned base (callers mask
   their fields out of it) */
__device__ __forceinline__ uint32_t jit_bread32(
    const uint8_t *__restrict__ b, uint32_t bitpos) {
  const uint32_t *w = (const uint32_t *)b;
  const uint32_t widx = bitpos >> 5;
  return __builtin_amdgcn_alignbit(w[widx + 1], w[widx], bitpos & 31);
}

/* claim-or-find the global group-table slot of a key; -1 = table full */
__device__ __forceinline__ int jit_gslot(gslot *gt, uint64_t key) {
  uint32_t idx = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >>
                            (64 - OBX_GTABLE_SHIFT)) &
                 (OBX_GTABLE_SLOTS - 1);
  for (int probe = 0; probe < OBX_GTABLE_SLOTS; probe++) {
    unsigned long long ck = atomicCAS(&gt[idx].key, OBX_KEY_EMPTY,
                                      (unsigned long long)key);
    if (ck == OBX_KEY_EMPTY || ck == key) return (int)idx;
    idx = (idx + 1) & (OBX_GTABLE_SLOTS - 1);
  }
  return -1;
}

/* three-valued block verdicts (0 none, 1 all, 2 mixed) under AND / OR */
__device__ __forceinline__ uint8_t f3and(uint8_t a, uint8_t b) {
  return (a == 0 || b == 0) ? 0 : ((a == 1 && b == 1) ? 1 : 2);
}
__device__ __forceinline__ uint8_t f3or(uint8_t a, uint8_t b) {
  return (a == 1 || b == 1) ? 1 : ((a == 0 && b == 0) ? 0 : 2);
}

#endif /* OBX_JIT_DEV_H */
