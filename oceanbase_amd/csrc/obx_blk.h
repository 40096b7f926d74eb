/*
 * obx_blk.h — the small steps the precompiled kernels share (obx_kernels.hip,
 * obx_project.hip, obx_keys.hip, obx_join.hip): opening a block, storing
 * a datum, and a workgroup sum. The JIT kernels emit their own forms of the
 * first two and need no workgroup sum, so this header is not part of the
 * hipRTC compile input.
 */
#ifndef OBX_BLK_H
#define OBX_BLK_H
#include "obx_dev_common.h"

/* Open block `cur` for the workgroup. STAGE: wait until the previous block's
 * LDS reads are done, copy the block into lds_blk and wait for the copy; the
 * view then reads LDS. Otherwise the view reads the global buffer (no
 * barrier). */
template <bool STAGE>
__device__ __forceinline__ blk_view blk_open(const uint8_t *__restrict__ buf,
                                             const dev_block &cur,
                                             uint8_t *lds_blk) {
  const uint64_t blk_bit = cur.block_byte * 8;
  if (STAGE) {
    __syncthreads(); /* drain previous block's LDS reads */
    stage_issue(buf, cur, lds_blk);
    stage_wait();
  }
  blk_view bv;
  bv.base = STAGE ? lds_blk : buf;
  bv.bit_bias = STAGE ? blk_bit : 0;
  bv.rbase_bit = STAGE ? 0 : blk_bit;
  return bv;
}

/* the low `len` bytes of uv, little-endian, to dst (a VEC_FIXED datum) */
__device__ __forceinline__ void store_datum(uint8_t *dst, uint64_t uv,
                                            uint32_t len) {
  if (len == 8)       /* aligned: hipMalloc base + 8-B stride */
    *(uint64_t *)dst = uv;
  else if (len == 4)
    *(uint32_t *)dst = (uint32_t)uv;
  else
    for (uint32_t i = 0; i < len; i++) dst[i] = (uint8_t)(uv >> (i * 8));
}

/* sum of one value per thread over the workgroup, valid in thread 0 */
__device__ __forceinline__ uint64_t wg_sum(uint64_t v) {
  __shared__ uint64_t part[WAVES];
  for (int off = 32; off > 0; off >>= 1) v += shflxor64(v, off);
  __syncthreads(); /* part of a previous call fully read */
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t s = 0;
  for (uint32_t w = 0; w < WAVES; w++) s += part[w];
  return s;
}

#endif /* OBX_BLK_H */
