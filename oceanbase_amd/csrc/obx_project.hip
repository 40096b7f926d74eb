/*
 * obx_project.hip — filtered projection: decode ONLY the filter's survivors.
 *
 * The device half of obx_gpu_scan_project, the whole-range form of
 * ObIMicroBlockReader::get_rows(row_ids, ...) (ob_imicro_block_reader.h): the
 * filter kernels leave block-local row ids and per-block counts; here an
 * exclusive scan of the counts places every block in the dense result, and
 * k_project_sel gathers the survivors of each projected column into
 * compacted VEC_FIXED vectors with a null flag per row.
 *
 * A translation unit of its own, so the scan kernels of obx_kernels.hip keep
 * their code and register allocation.
 */
#include "obx_blk.h"
#include "obx_project.h"

__device__ __forceinline__ uint64_t shflup64(uint64_t v, uint32_t d) {
  uint32_t lo = __shfl_up((int)(uint32_t)v, d, 64);
  uint32_t hi = __shfl_up((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}

/* workgroup-wide exclusive prefix sum of one value per thread; total = the
   sum over the workgroup. Safe to call repeatedly (leading barrier). */
__device__ __forceinline__ uint64_t wg_scan_excl(uint64_t mine,
                                                 uint64_t &total) {
  __shared__ uint64_t wv_sum[WAVES];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint64_t v = mine;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    uint64_t o = shflup64(v, d);
    if (lane >= d) v += o;
  }
  __syncthreads(); /* wv_sum of a previous call fully read */
  if (lane == 63) wv_sum[wv] = v;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (uint32_t w = 0; w < WAVES; w++) {
    if (w < wv) before += wv_sum[w];
    all += wv_sum[w];
  }
  total = all;
  return before + v - mine;
}

/* ---------------- block offsets: exclusive 64-bit scan of blk_counts ------
 * Two launches: per-tile sums, then every tile adds the sums of the tiles
 * before it (a few hundred values at SF=100's ~450 K blocks) to its own
 * local scan. off has n + 1 entries; off[n] is the result's row count. */
extern "C" __global__ __launch_bounds__(WG) void k_project_tile_sums(
    const uint32_t *__restrict__ counts, uint32_t n,
    uint64_t *__restrict__ tile_sums) {
  const uint64_t base = (uint64_t)blockIdx.x * OBX_PROJ_TILE;
  uint64_t s = 0;
  for (uint32_t k = 0; k < OBX_PROJ_TILE / WG; k++) {
    uint64_t i = base + (uint64_t)k * WG + threadIdx.x;
    if (i < n) s += counts[i];
  }
  uint64_t total;
  (void)wg_scan_excl(s, total);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

extern "C" __global__ __launch_bounds__(WG) void k_project_offsets(
    const uint32_t *__restrict__ counts, uint32_t n,
    const uint64_t *__restrict__ tile_sums, uint64_t *__restrict__ off) {
  constexpr uint32_t PER = OBX_PROJ_TILE / WG;
  uint64_t s = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += WG) s += tile_sums[j];
  uint64_t tile_base;
  (void)wg_scan_excl(s, tile_base);

  const uint64_t first = (uint64_t)blockIdx.x * OBX_PROJ_TILE +
                         (uint64_t)threadIdx.x * PER;
  uint32_t c[PER];
  uint64_t mine = 0;
  for (uint32_t k = 0; k < PER; k++) {
    c[k] = first + k < n ? counts[first + k] : 0;
    mine += c[k];
  }
  uint64_t tile_total;
  uint64_t run = tile_base + wg_scan_excl(mine, tile_total);
  for (uint32_t k = 0; k < PER; k++) {
    if (first + k < n) off[first + k] = run;
    run += c[k];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
    off[n] = tile_base + tile_total;
}

/* ---------------- gather-decode ------------------------------------------
 * Grid-stride over blocks. A block without survivors is skipped on its
 * count alone. Otherwise lane i takes survivor i of the block: row
 * r = row_ids[row_start + i], every projected column's datum to
 * (off[b] + i) * len of its vector (consecutive lanes, consecutive datums),
 * one byte of null flags (bit p = projected position p is NULL; at most
 * OBX_DEV_MAX_COLS = 8 positions) and, if asked, the table-global row
 * number. row_ids == nullptr is the unfiltered scan: identity row ids,
 * count = row_count, offset = the block's first row. out_rows bounds every
 * store. */
template <bool STAGE>
__device__ __forceinline__ void project_sel_body(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const int32_t *__restrict__ row_ids,
    const uint32_t *__restrict__ blk_counts, const uint64_t *__restrict__ off,
    const proj_args &pa, uint8_t *__restrict__ out_nulls,
    uint64_t *__restrict__ out_row_nos, uint64_t out_rows, uint8_t *lds_blk) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    if (row_ids && blk_counts[b] == 0) continue; /* workgroup-uniform */
    const dev_block &cur = blocks[b];
    const uint32_t rows = cur.row_count;
    uint32_t cnt = row_ids ? blk_counts[b] : rows;
    if (cnt > rows) cnt = rows;
    if (cnt == 0) continue;
    const blk_view bv = blk_open<STAGE>(buf, cur, lds_blk);
    const uint64_t row_start = dev_block_row_start(&cur);
    const uint64_t o = row_ids ? off[b] : row_start;
    /* (loading several row ids per lane ahead of the decode calls was
       measured: no gain, profiles/r04_scan_project.md) */
    for (uint32_t i = tid; i < cnt; i += WG) {
      const uint64_t dst_row = o + i;
      if (dst_row >= out_rows) break;
      uint32_t r = row_ids ? (uint32_t)row_ids[row_start + i] : i;
      if (r >= rows) r = rows - 1; /* never read past the block */
      uint32_t nullmask = 0;
      for (uint32_t p = 0; p < pa.n_proj; p++) {
        const uint32_t datum_len = pa.len[p];
        bool isn;
        int64_t v = col_value2(bv, cur, cur.cols[pa.col[p]], r, isn);
        store_datum(pa.out[p] + dst_row * datum_len, isn ? 0 : (uint64_t)v,
                    datum_len);
        nullmask |= (isn ? 1u : 0u) << p;
      }
      out_nulls[dst_row] = (uint8_t)nullmask;
      if (out_row_nos) out_row_nos[dst_row] = row_start + r;
    }
  }
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_project_sel(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const int32_t *__restrict__ row_ids,
    const uint32_t *__restrict__ blk_counts, const uint64_t *__restrict__ off,
    const proj_args pa, uint8_t *__restrict__ out_nulls,
    uint64_t *__restrict__ out_row_nos, uint64_t out_rows) {
  project_sel_body<false>(buf, blocks, n_blocks, row_ids, blk_counts, off, pa,
                          out_nulls, out_row_nos, out_rows, nullptr);
}

extern "C" __global__ __launch_bounds__(WG, 2) void k_project_sel_lds(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const int32_t *__restrict__ row_ids,
    const uint32_t *__restrict__ blk_counts, const uint64_t *__restrict__ off,
    const proj_args pa, uint8_t *__restrict__ out_nulls,
    uint64_t *__restrict__ out_row_nos, uint64_t out_rows) {
  __shared__ uint8_t lds_blk[OBX_LDS_STAGE_BYTES + 32];
  project_sel_body<true>(buf, blocks, n_blocks, row_ids, blk_counts, off, pa,
                         out_nulls, out_row_nos, out_rows, lds_blk);
}

/* ---------------- window null bits ---------------------------------------
 * obx_gpu_fetch_proj hands out null flags bit-packed relative to the
 * window's first row: out bit i (LSB-first) = flag `bit` of result row
 * start + i. One thread per output byte. */
extern "C" __global__ __launch_bounds__(WG) void k_project_pack_nulls(
    const uint8_t *__restrict__ nulls, uint64_t start, uint64_t n,
    uint32_t bit, uint8_t *__restrict__ out) {
  const uint64_t n_bytes = (n + 7) / 8;
  for (uint64_t j = (uint64_t)blockIdx.x * WG + threadIdx.x; j < n_bytes;
       j += (uint64_t)gridDim.x * WG) {
    uint32_t byte = 0;
    for (uint32_t k = 0; k < 8; k++) {
      const uint64_t i = j * 8 + k;
      if (i < n) byte |= ((nulls[start + i] >> bit) & 1u) << k;
    }
    out[j] = (uint8_t)byte;
  }
}
