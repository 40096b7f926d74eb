/*
 * obx_pax_load.cpp — the PAX (microblock) loader: payload checksum, host
 * parse of each block header into a flat dev_block, and the upload. Sibling
 * of obx_cs_load.cpp; both fold their blocks with obx_fold_block
 * (obx_plan.cpp) and end in obx_finish_load (obx_engine.cpp).
 */
#include <cstring>

#include "obx_host.h"

/* Load-time payload checksum (the reference verifies data_checksum_ when a
 * block enters the block cache, before any decode — check_payload_checksum,
 * ob_micro_block_header.cpp:257-271). ob_crc64_sse42 semantics = CRC-32C in
 * a u64 accumulator; the host has the crc32 instruction, same as the
 * reference's hardware path. Independent of the oracle's implementation. */
__attribute__((target("sse4.2")))
static uint64_t host_crc32c(const uint8_t *buf, int64_t len) {
  uint64_t crc = 0;
  int64_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint64_t w;
    memcpy(&w, buf + i, 8);
    crc = __builtin_ia32_crc32di(crc, w);
  }
  for (; i < len; i++) crc = __builtin_ia32_crc32qi((uint32_t)crc, buf[i]);
  return crc;
}

/* ---- host block parsing (mirrors ObMicroBlockDecoder pointer math,
 * ob_micro_block_decoder.cpp:360-380, and the per-decoder init functions
 * cited in oracle/obx_codec.c) ------------------------------------------- */
static int parse_block(const obx_col_schema *cols, uint16_t n_cols,
                       const uint8_t *block, uint64_t dev_off,
                       uint64_t block_len, uint64_t row_start,
                       dev_block *out) {
  const obx_micro_header *h = (const obx_micro_header *)block;
  if (h->magic != OBX_MICRO_BLOCK_MAGIC) return OBX_INVALID_ARGUMENT;
  if (h->column_count != n_cols) return OBX_INVALID_ARGUMENT;
  if (h->data_zlength > (int64_t)block_len ||
      h->data_zlength < OBX_MICRO_HEADER_SIZE)
    return OBX_INVALID_ARGUMENT;
  if ((int64_t)host_crc32c(block + OBX_MICRO_HEADER_SIZE,
                           (int64_t)h->data_zlength - OBX_MICRO_HEADER_SIZE) !=
      h->data_checksum)
    return OBX_PHYSIC_CHECKSUM_ERROR;
  memset(out, 0, sizeof(*out));
  out->row_start_lo = (uint32_t)row_start;
  out->row_start_hi = (uint32_t)(row_start >> 32);
  out->row_count = h->row_count;
  out->block_len = (uint32_t)block_len;
  out->block_byte = dev_off;
  const uint64_t meta_base =
      dev_off + h->header_size + (uint64_t)n_cols * sizeof(obx_col_header);
  const obx_col_header *chp =
      (const obx_col_header *)(block + h->header_size);
  const uint8_t *meta_host = block + h->header_size +
                             (uint64_t)n_cols * sizeof(obx_col_header);
  const uint8_t evb = obx_hdr_extend_value_bit(h);

  for (uint16_t c = 0; c < n_cols; c++) {
    const obx_col_header *ch = &chp[c];
    dev_col *dc = &out->cols[c];
    const int sc = obx_store_class(ch->obj_type);
    const int64_t tss = obx_type_store_size(ch->obj_type);
    dc->enc = (uint8_t)ch->type;
    dc->datum_len = cols[c].len;
    dc->tss = (uint8_t)(tss > 0 ? tss : cols[c].len);
    dc->ext_width = evb;
    if (sc == OBX_SC_INT) dc->flags |= OBX_DF_SIGNED;
    if (sc == OBX_SC_STRING) dc->flags |= OBX_DF_STRING;
    const uint64_t col_base = meta_base + ch->offset;
    const uint8_t *col_host = meta_host + ch->offset;
    const int has_ext = (ch->attr & OBX_COL_ATTR_HAS_EXTEND_VALUE) ? 1 : 0;
    const int bp = (ch->attr & OBX_COL_ATTR_BIT_PACKING) ? 1 : 0;

    switch (ch->type) {
      case OBX_COL_RAW: {
        if (bp) dc->flags |= OBX_DF_BITPACK;
        dc->width = (uint8_t)ch->length;
        uint64_t ext_bits = has_ext ? (uint64_t)evb * h->row_count : 0;
        if (has_ext) {
          dc->flags |= OBX_DF_HAS_EXT;
          dc->ext_bit = col_base * 8;
        }
        if (bp) {
          dc->data_bit = col_base * 8 + ext_bits;
        } else {
          dc->data_bit = (col_base + (ext_bits + 7) / 8) * 8;
        }
        break;
      }
      case OBX_COL_DICT: {
        const obx_dict_meta *dm = (const obx_dict_meta *)col_host;
        if (bp) dc->flags |= OBX_DF_BITPACK;
        dc->width = dm->row_ref_size;
        dc->count = dm->count;
        dc->entry_len = (uint8_t)dm->data_size;
        dc->dict_byte = col_base + sizeof(obx_dict_meta);
        dc->data_bit = (col_base + ch->length) * 8; /* refs follow meta */
        break;
      }
      case OBX_COL_RLE: {
        const obx_rle_meta *rm = (const obx_rle_meta *)col_host;
        dc->runs = rm->count;
        dc->rib = rm->attr & 7;
        dc->rfb = (rm->attr >> 3) & 7;
        dc->aux_byte = col_base + sizeof(obx_rle_meta);
        const obx_dict_meta *dm =
            (const obx_dict_meta *)(col_host + rm->offset);
        dc->count = dm->count;
        dc->entry_len = (uint8_t)dm->data_size;
        dc->dict_byte = col_base + rm->offset + sizeof(obx_dict_meta);
        break;
      }
      case OBX_COL_CONST: {
        const obx_const_meta *cm = (const obx_const_meta *)col_host;
        dc->runs = cm->count; /* exception count */
        dc->rib = cm->attr & 7;
        dc->rfb = cm->const_ref;
        if (cm->count == 0) {
          if (cm->const_ref > 0) {
            dc->count = 0; /* null-const */
          } else {
            dc->count = 1;
            int64_t cell = (sc == OBX_SC_INT) ? tss : cols[c].len;
            uint64_t v = 0;
            memcpy(&v, col_host + cm->offset, (size_t)cell);
            dc->base = (sc == OBX_SC_INT)
                           ? (int64_t)obx_sign_extend(v, tss, 1)
                           : (sc == OBX_SC_DECIMAL
                                  ? (int64_t)obx_sign_extend(v, cell, 1)
                                  : (int64_t)v);
          }
        } else {
          dc->aux_byte = col_base + sizeof(obx_const_meta);
          const obx_dict_meta *dm =
              (const obx_dict_meta *)(col_host + cm->offset);
          dc->count = dm->count;
          dc->entry_len = (uint8_t)dm->data_size;
          dc->dict_byte = col_base + cm->offset + sizeof(obx_dict_meta);
        }
        break;
      }
      case OBX_COL_INTEGER_BASE_DIFF: {
        const obx_intdiff_meta *im = (const obx_intdiff_meta *)col_host;
        if (bp) dc->flags |= OBX_DF_BITPACK;
        dc->width = im->length;
        uint64_t b = 0;
        memcpy(&b, col_host + sizeof(obx_intdiff_meta), (size_t)tss);
        dc->base = (int64_t)obx_sign_extend(b, tss, sc == OBX_SC_INT);
        uint64_t data0 = col_base + ch->length;
        uint64_t ext_bits = has_ext ? (uint64_t)evb * h->row_count : 0;
        if (has_ext) {
          dc->flags |= OBX_DF_HAS_EXT;
          dc->ext_bit = data0 * 8;
        }
        if (bp) dc->data_bit = data0 * 8 + ext_bits;
        else dc->data_bit = (data0 + (ext_bits + 7) / 8) * 8;
        break;
      }
      case OBX_COL_STRING_PREFIX: {
        const obx_sprefix_meta *pm = (const obx_sprefix_meta *)col_host;
        dc->count = pm->count;
        dc->entry_len = pm->hex_char_cnt;
        dc->rib = pm->pib;
        dc->dict_byte = col_base + sizeof(obx_sprefix_meta); /* hex chars */
        dc->aux_byte = dc->dict_byte + pm->hex_char_cnt;     /* end index */
        /* fixed cell stride: 1 + max suffix (raw or nibble-packed) */
        {
          const uint8_t *ends = col_host + sizeof(obx_sprefix_meta) +
                                pm->hex_char_cnt;
          uint64_t prev = 0, min_pl = ~0ull;
          for (uint32_t j = 0; j < pm->count; j++) {
            uint64_t e2 = 0;
            memcpy(&e2, ends + (size_t)j * pm->pib, pm->pib);
            if (e2 - prev < min_pl) min_pl = e2 - prev;
            prev = e2;
          }
          uint32_t max_suffix = pm->string_size - (uint32_t)min_pl;
          dc->width = (uint8_t)(1 + (pm->hex_char_cnt
                                         ? (max_suffix + 1) / 2
                                         : max_suffix));
        }
        uint64_t data0 = col_base + ch->length;
        uint64_t ext_bits = has_ext ? (uint64_t)evb * h->row_count : 0;
        if (has_ext) {
          dc->flags |= OBX_DF_HAS_EXT;
          dc->ext_bit = data0 * 8;
        }
        dc->data_bit = (data0 + (ext_bits + 7) / 8) * 8;
        break;
      }
      case OBX_COL_SUBSTR: {
        const obx_substr_meta *sm3 = (const obx_substr_meta *)col_host;
        if (sm3->ref_col >= n_cols) return OBX_INVALID_ARGUMENT;
        dc->runs = sm3->exc_cnt;
        dc->rib = sm3->rib;
        dc->width = (uint8_t)sm3->ref_col; /* ref column index */
        dc->base = sm3->start_pos;
        dc->dict_byte = col_base + sizeof(obx_substr_meta); /* exc rids */
        dc->aux_byte = dc->dict_byte + (uint64_t)sm3->exc_cnt * sm3->rib;
        break;
      }
      case OBX_COL_EQUAL: {
        const obx_coleq_meta *em = (const obx_coleq_meta *)col_host;
        if (em->ref_col >= n_cols) return OBX_INVALID_ARGUMENT;
        dc->runs = em->exc_cnt;
        dc->rib = em->rib;
        dc->width = (uint8_t)em->ref_col; /* ref column index */
        dc->dict_byte = col_base + sizeof(obx_coleq_meta); /* exc row_ids */
        dc->aux_byte = dc->dict_byte + (uint64_t)em->exc_cnt * em->rib;
        break;
      }
      case OBX_COL_HEX_PACKING: {
        const obx_hex_meta *hm = (const obx_hex_meta *)col_host;
        dc->width = (uint8_t)((hm->string_size + 1) / 2); /* row stride B */
        dc->count = hm->char_cnt;
        dc->dict_byte = col_base + sizeof(obx_hex_meta); /* char array */
        uint64_t data0 = col_base + ch->length;
        uint64_t ext_bits = has_ext ? (uint64_t)evb * h->row_count : 0;
        if (has_ext) {
          dc->flags |= OBX_DF_HAS_EXT;
          dc->ext_bit = data0 * 8;
        }
        dc->data_bit = (data0 + (ext_bits + 7) / 8) * 8;
        break;
      }
      case OBX_COL_STRING_DIFF: {
        const obx_sdiff_meta *sm = (const obx_sdiff_meta *)col_host;
        dc->runs = sm->diff_desc_cnt;
        dc->entry_len = sm->hex_char_cnt;
        dc->dict_byte = col_base + sizeof(obx_sdiff_meta); /* descs */
        const uint8_t *descs = col_host + sizeof(obx_sdiff_meta);
        uint32_t diff_len = 0;
        for (uint32_t i = 0; i < sm->diff_desc_cnt; i++)
          if (descs[i] & 1) diff_len += descs[i] >> 1;
        dc->rib = (uint8_t)diff_len;
        dc->width = (uint8_t)(sm->hex_char_cnt ? (diff_len + 1) / 2
                                               : diff_len);
        dc->aux_byte = dc->dict_byte + sm->diff_desc_cnt +
                       sm->hex_char_cnt; /* common bytes */
        uint64_t data0 = col_base + ch->length;
        uint64_t ext_bits = has_ext ? (uint64_t)evb * h->row_count : 0;
        if (has_ext) {
          dc->flags |= OBX_DF_HAS_EXT;
          dc->ext_bit = data0 * 8;
        }
        dc->data_bit = (data0 + (ext_bits + 7) / 8) * 8;
        break;
      }
      default:
        return OBX_NOT_SUPPORTED;
    }
  }
  return OBX_SUCCESS;
}

int obx_pax_host_load(const obx_blockset *bs, obx_table_facts &h,
                      std::vector<dev_block> &blocks) {
  if (bs->n_cols > OBX_DEV_MAX_COLS) return OBX_NOT_SUPPORTED;
  for (uint16_t c = 0; c < bs->n_cols; c++) {
    /* decimal scale bounds the P10 tables (reference: decimal-int
       precision <= 18 digits on this path) */
    if (bs->cols[c].scale < 0 || bs->cols[c].scale > 18)
      return OBX_NOT_SUPPORTED;
  }
  h.n_cols = bs->n_cols;
  h.total_bytes = bs->block_offsets[bs->n_blocks];
  memcpy(h.cols, bs->cols, sizeof(obx_col_schema) * bs->n_cols);
  blocks.resize(bs->n_blocks);
  for (uint32_t b = 0; b < bs->n_blocks; b++) {
    const uint64_t off = bs->block_offsets[b];
    int rc = parse_block(bs->cols, bs->n_cols, bs->data + off, off,
                         bs->block_offsets[b + 1] - off, h.total_rows,
                         &blocks[b]);
    if (rc != OBX_SUCCESS) return rc;
    obx_fold_block(h, blocks[b]);
  }
  /* dict stability: identical dict payload in every block enables the
     JIT's persistent (whole-kernel) histograms/value tables */
  for (uint16_t c = 0; c < bs->n_cols; c++) {
    h.col_dict_stable[c] = h.col_dict_any[c];
    if (!h.col_dict_stable[c]) continue;
    const dev_col &d0 = blocks[0].cols[c];
    size_t dlen = (size_t)d0.count * d0.entry_len;
    for (uint32_t b = 1; b < bs->n_blocks && h.col_dict_stable[c]; b++) {
      const dev_col &db = blocks[b].cols[c];
      if (db.count != d0.count || db.entry_len != d0.entry_len ||
          memcmp(bs->data + db.dict_byte, bs->data + d0.dict_byte, dlen))
        h.col_dict_stable[c] = false;
    }
  }
  return OBX_SUCCESS;
}

extern "C" int obx_gpu_load_blocks(obx_gpu_ctx *ctx, const obx_blockset *bs) {
  if (!ctx || !bs) return OBX_INVALID_ARGUMENT;
  auto h = std::make_unique<obx_handle>();
  std::vector<dev_block> blocks;
  int rc = obx_pax_host_load(bs, *h, blocks);
  if (rc != OBX_SUCCESS) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMalloc(&h->d_buf, h->total_bytes + 64));
  HIP_TRY(hipMemset(h->d_buf + h->total_bytes, 0, 64));
  HIP_TRY(hipMemcpy(h->d_buf, bs->data, h->total_bytes, hipMemcpyHostToDevice));
  return obx_finish_load(ctx, std::move(h), blocks);
}

extern "C" uint64_t obx_crc32c(const uint8_t *buf, int64_t len) {
  return host_crc32c(buf, len);
}
