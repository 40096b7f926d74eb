/*
 * obx_codec.c — CPU ORACLE (test infrastructure + reported CPU baseline).
 *
 * Faithful C restatement of the reference's PAX microblock encoder, decoder
 * and white-filter semantics. NOT the product path: the GPU engine
 * (oceanbase_amd/csrc) must never route through this library; only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may call it.
 *
 * Restates, function by function (all paths under /root/reference/):
 *   encoder: src/storage/blocksstable/encoding/ob_micro_block_encoder.cpp:492-700
 *            (build_block / store_encoding_meta_and_fix_cols),
 *            ob_raw_encoder.cpp:84-290, ob_dict_encoder.cpp:84-440,
 *            ob_rle_encoder.cpp:60-170, ob_const_encoder.cpp:100-330,
 *            ob_integer_base_diff_encoder.cpp:139-280,
 *            ob_icolumn_encoder.h:175-268 (store_fix_bits/fill_column_store)
 *   decoder: encoding/ob_micro_block_decoder.cpp:360-380 (pointer math),
 *            ob_raw_decoder.cpp (decode), ob_dict_decoder.cpp,
 *            ob_rle_decoder.cpp:18-31,536-561, ob_const_decoder.cpp,
 *            ob_integer_base_diff_decoder.{h:133,cpp},
 *            ob_encoding_util.h:416-580 (load_data_to_datum widening)
 *   filter:  sql/engine/basic/ob_pushdown_filter.{h:383-455,cpp:1559-1632}
 *            white-op semantics, AND combine, NULL -> no-match (except NU)
 *
 * Parity pinning: see oracle/obx_format.h header note (reference unbuildable
 * in-container, no stored golden vectors upstream; pinned by format fidelity
 * + recreated reference test assertions + independent Python model).
 */
#include "obx_format.h"
#include "../include/obx.h"

#include <pthread.h>
#include <stdlib.h>
#include <string.h>

/* ===================================================================== */
/* helpers                                                               */
/* ===================================================================== */

/* Block payload checksum, restating ob_crc64_sse42 semantics
 * (deps/oblib/src/lib/checksum/ob_crc64.cpp:448-520 and the crc32q
 * hardware path): CRC-32C (Castagnoli, reflected poly 0x82f63b78,
 * init 0, no final xor) accumulated in a 64-bit register — i.e. the
 * stored int64 data_checksum is the CRC-32C of the payload,
 * zero-extended. The writer sets it over everything after the micro
 * header (ob_imicro_block_writer.cpp:193); the decoder verifies it
 * before trusting interior payloads (check_payload_checksum,
 * ob_micro_block_header.cpp:257-271). */
static uint32_t crc32c_tab[256];
static pthread_once_t crc32c_once = PTHREAD_ONCE_INIT;
static void crc32c_fill(void) {
  for (uint32_t n = 0; n < 256; n++) {
    uint32_t c = n;
    for (int k = 0; k < 8; k++) c = (c & 1) ? 0x82f63b78u ^ (c >> 1) : c >> 1;
    crc32c_tab[n] = c;
  }
}
/* once, and complete before any caller reads it: the generator's and the
 * scan's worker threads all come here first (a thread that saw entry 1 set
 * while another was still filling the table stored a wrong checksum, and
 * the engine then refused the block at load) */
static void crc32c_init(void) { pthread_once(&crc32c_once, crc32c_fill); }
uint64_t obx_crc32c(const uint8_t *buf, int64_t len) {
  crc32c_init();
  uint64_t crc = 0;
  for (int64_t i = 0; i < len; i++)
    crc = crc32c_tab[(crc ^ buf[i]) & 0xff] ^ (crc >> 8);
  return crc;
}

static inline int64_t datum_int(const uint8_t *p, int len, int sc) {
  /* read a datum payload as int64 (sign rules per store class) */
  uint64_t v = 0;
  memcpy(&v, p, (size_t)len);
  if (sc == OBX_SC_INT || sc == OBX_SC_DECIMAL) {
    return (int64_t)obx_sign_extend(v, len, 1);
  }
  return (int64_t)v;
}

static inline int null_at(const uint8_t *nulls, uint32_t r) {
  return nulls && ((nulls[r >> 3] >> (r & 7)) & 1);
}

/* datum compare for dict sort: ObIntSC/ObDecimalIntSC signed,
 * ObStringSC binary memcmp (dict sort order recorded in IS_SORTED attr,
 * ob_dict_encoder.cpp:127-165) */
static int datum_cmp(const uint8_t *a, const uint8_t *b, int len, int sc) {
  if (sc == OBX_SC_STRING) {
    return memcmp(a, b, (size_t)len);
  }
  int64_t va = datum_int(a, len, sc), vb = datum_int(b, len, sc);
  return va < vb ? -1 : (va > vb ? 1 : 0);
}

/* ===================================================================== */
/* per-column stats + dict build                                         */
/* ===================================================================== */

typedef struct dict_builder {
  /* first-appearance hash (open addressing), then sorted.
     Mirrors ObEncodingHashTable node lists (ob_encoding_hash_util.cpp). */
  uint32_t cap;            /* power of two */
  int32_t *slots;          /* -1 empty, else entry idx */
  uint32_t count;
  uint8_t *entries;        /* count * len datum bytes, appearance order */
  uint32_t *ref_of_row;    /* per row: entry idx (or count for NULL) */
  uint32_t *remap;         /* appearance idx -> sorted ref */
  uint64_t null_cnt;
} dict_builder;

static uint64_t hash64(const uint8_t *p, int len) {
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < len; i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

static int dict_build(dict_builder *db, const uint8_t *data,
                      const uint8_t *nulls, uint32_t rows, int len) {
  uint32_t cap = 16;
  while (cap < rows * 2u && cap < (1u << 20)) cap <<= 1;
  db->cap = cap;
  db->slots = (int32_t *)malloc(sizeof(int32_t) * cap);
  db->entries = (uint8_t *)malloc((size_t)len * (rows ? rows : 1));
  db->ref_of_row = (uint32_t *)malloc(sizeof(uint32_t) * rows);
  db->remap = NULL;
  db->count = 0;
  db->null_cnt = 0;
  if (!db->slots || !db->entries || !db->ref_of_row) return OBX_INTERNAL_ERROR;
  memset(db->slots, -1, sizeof(int32_t) * cap);
  for (uint32_t r = 0; r < rows; r++) {
    const uint8_t *d = data + (size_t)r * len;
    if (null_at(nulls, r)) { db->ref_of_row[r] = UINT32_MAX; db->null_cnt++; continue; }
    uint64_t h = hash64(d, len) & (cap - 1);
    for (;;) {
      int32_t e = db->slots[h];
      if (e < 0) {
        db->slots[h] = (int32_t)db->count;
        memcpy(db->entries + (size_t)db->count * len, d, (size_t)len);
        db->ref_of_row[r] = db->count++;
        break;
      }
      if (memcmp(db->entries + (size_t)e * len, d, (size_t)len) == 0) {
        db->ref_of_row[r] = (uint32_t)e;
        break;
      }
      h = (h + 1) & (cap - 1);
    }
  }
  return OBX_SUCCESS;
}

/* sort dict entries, fill remap (appearance ref -> sorted ref).
 * insertion sort is fine: dicts on this path are tiny. */
static void dict_sort(dict_builder *db, int len, int sc) {
  uint32_t n = db->count;
  uint32_t *order = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
  for (uint32_t i = 0; i < n; i++) order[i] = i;
  for (uint32_t i = 1; i < n; i++) {
    uint32_t k = order[i];
    uint32_t j = i;
    while (j > 0 && datum_cmp(db->entries + (size_t)order[j - 1] * len,
                              db->entries + (size_t)k * len, len, sc) > 0) {
      order[j] = order[j - 1]; j--;
    }
    order[j] = k;
  }
  db->remap = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
  uint8_t *sorted = (uint8_t *)malloc((size_t)len * (n ? n : 1));
  for (uint32_t i = 0; i < n; i++) {
    db->remap[order[i]] = i;
    memcpy(sorted + (size_t)i * len, db->entries + (size_t)order[i] * len,
           (size_t)len);
  }
  free(db->entries);
  db->entries = sorted;
  free(order);
}

static void dict_free(dict_builder *db) {
  free(db->slots); free(db->entries); free(db->ref_of_row); free(db->remap);
  memset(db, 0, sizeof(*db));
}

/* sorted ref of row r (count for NULL, ob_dict_encoder.cpp:100-115) */
static inline uint32_t dict_ref(const dict_builder *db, uint32_t r) {
  uint32_t a = db->ref_of_row[r];
  return a == UINT32_MAX ? db->count : (db->remap ? db->remap[a] : a);
}

/* ===================================================================== */
/* encoder                                                               */
/* ===================================================================== */

typedef struct enc_buf { uint8_t *p; int64_t len, cap; } enc_buf;
static int eb_nop(enc_buf *b, int64_t n) {
  if (b->len + n > b->cap) return OBX_BUF_NOT_ENOUGH;
  memset(b->p + b->len, 0, (size_t)n);
  b->len += n;
  return 0;
}

/* store the [ext bits][packed bits] + [fixed data] region of one column
 * (ObIColumnEncoder::fill_column_store, ob_icolumn_encoder.h:224-268).
 * get_val(r) returns the k-bit/ fixed value for row r. */
typedef struct fix_store_spec {
  int ext_bit;              /* block-level extend_value_bit (0/1) */
  int has_ext;              /* this column stores ext bits */
  int bit_len;              /* bit packing width, 0 if byte mode */
  int fix_len;              /* fixed byte width, 0 if bit mode */
} fix_store_spec;

static int store_fix_region(enc_buf *mb, const fix_store_spec *s,
                            uint32_t rows, const uint8_t *nulls,
                            uint64_t (*get_val)(void *, uint32_t), void *c,
                            const uint8_t *fix_src, int fix_src_stride) {
  int64_t bits = 0;
  if (s->has_ext) bits += (int64_t)s->ext_bit * rows;
  bits += (int64_t)s->bit_len * rows;
  int64_t bits_bytes = (bits + 7) / 8;
  int64_t total = bits_bytes + (int64_t)s->fix_len * rows;
  uint8_t *base = mb->p + mb->len;
  /* encoder reserves 8 zero bytes of slack for 9-byte bit writes then
     reverts (ob_icolumn_encoder.h:239-263); we keep cap margin instead */
  if (eb_nop(mb, total)) return OBX_BUF_NOT_ENOUGH;
  if (mb->len + 8 > mb->cap) return OBX_BUF_NOT_ENOUGH;
  memset(mb->p + mb->len, 0, 8);
  int64_t pos = 0;
  if (s->has_ext) {
    for (uint32_t r = 0; r < rows; r++) {
      obx_bs_set(base, pos, s->ext_bit, null_at(nulls, r) ? 1 : 0 /*STORED_NULL*/);
      pos += s->ext_bit;
    }
  }
  if (s->bit_len > 0) {
    for (uint32_t r = 0; r < rows; r++) {
      if (!null_at(nulls, r)) obx_bs_set(base, pos, s->bit_len, get_val(c, r));
      pos += s->bit_len;
    }
  }
  if (s->fix_len > 0) {
    uint8_t *fp = base + bits_bytes;
    for (uint32_t r = 0; r < rows; r++) {
      if (!null_at(nulls, r)) {
        if (fix_src) {
          memcpy(fp, fix_src + (size_t)r * fix_src_stride, (size_t)s->fix_len);
        } else {
          uint64_t v = get_val(c, r);
          memcpy(fp, &v, (size_t)s->fix_len);
        }
      }
      fp += s->fix_len;
    }
  }
  return 0;
}

/* value getter contexts */
typedef struct {
  const uint8_t *data; int len; int sc; uint64_t mask;
} raw_get_ctx;
static uint64_t raw_get(void *c, uint32_t r) {
  raw_get_ctx *g = (raw_get_ctx *)c;
  uint64_t v = 0;
  memcpy(&v, g->data + (size_t)r * g->len, (size_t)g->len);
  return v & g->mask;
}
typedef struct { const dict_builder *db; } ref_get_ctx;
static uint64_t ref_get(void *c, uint32_t r) {
  return dict_ref(((ref_get_ctx *)c)->db, r);
}
typedef struct {
  const uint8_t *data; int len; uint64_t base; uint64_t mask;
} diff_get_ctx;
static uint64_t diff_get(void *c, uint32_t r) {
  diff_get_ctx *g = (diff_get_ctx *)c;
  uint64_t v = 0;
  memcpy(&v, g->data + (size_t)r * g->len, (size_t)g->len);
  return (v & g->mask) - g->base;
}

/* per-column encode. Returns 0 or status. Updates col header + meta buf. */
static int encode_column(enc_buf *mb, obx_col_header *ch,
                         const obx_col_schema *cs, const uint8_t *data,
                         const uint8_t *nulls, uint32_t rows, uint8_t enc,
                         int block_ext_bit, const obx_col_schema *all_cols,
                         const uint8_t *const *all_data,
                         const uint8_t *const *all_nulls, uint16_t col_idx) {
  const int len = cs->len;
  const int sc = obx_store_class(cs->obj_type);
  const int64_t tss = obx_type_store_size(cs->obj_type); /* -1 for dec/char */
  const uint64_t mask = (sc == OBX_SC_INT) ? obx_integer_mask(tss)
                                           : ~(uint64_t)0;
  uint64_t null_cnt = 0;
  if (nulls) for (uint32_t r = 0; r < rows; r++) null_cnt += null_at(nulls, r);

  ch->version = 0;
  ch->obj_type = cs->obj_type;
  ch->attr = 0;
  ch->extend_value_offset = 0;
  const int64_t pos_bak = mb->len;
  ch->offset = (uint32_t)pos_bak;

  if (enc == OBX_ENC_AUTO) {
    /* simplified cost ranking (writer policy, not parity-relevant;
       reference: ob_encoding_util.h:270-303 cost model) */
    dict_builder db;
    int rc = dict_build(&db, data, nulls, rows, len);
    if (rc) { dict_free(&db); return rc; }
    uint32_t nd = db.count;
    /* count runs */
    uint64_t runs = 0; uint32_t prev = UINT32_MAX - 1;
    for (uint32_t r = 0; r < rows; r++) {
      uint32_t x = db.ref_of_row[r];
      if (x != prev) { runs++; prev = x; }
    }
    /* const suitability (ObConstEncoder::traverse, ob_const_encoder.h:
       48-49): exceptions vs the dominant value (null competes) bounded
       by MAX_EXCEPTION_SIZE=32 and MAX_EXCEPTION_PCT=10 */
    uint32_t cmax = null_cnt;
    {
      uint32_t *freq = (uint32_t *)calloc((size_t)nd + 1, 4);
      if (freq) {
        for (uint32_t r = 0; r < rows; r++) {
          uint32_t x = db.ref_of_row[r]; /* UINT32_MAX sentinel = null */
          if (x <= nd) freq[x]++;
        }
        for (uint32_t i = 0; i <= nd; i++)
          if (freq[i] > cmax) cmax = freq[i];
        free(freq);
      }
    }
    uint32_t cexc = rows - cmax;
    uint32_t cpct = rows / 10 > 1 ? rows / 10 : 1;
    dict_free(&db);
    if (nd == 1 && null_cnt == 0) enc = OBX_ENC_CONST;
    else if (cexc > 0 && cexc <= 32 && cexc <= cpct && nd <= 255)
      /* accept-on-equal boundary: the reference rejects only when
         count_ > MAX(rows*10/100, 1) (ob_const_encoder.cpp:103-104) */
      enc = OBX_ENC_CONST;
    else if (runs * 8 <= rows) enc = OBX_ENC_RLE;
    else if (nd <= 64 && nd * 4 <= rows) enc = OBX_ENC_DICT;
    else if (sc == OBX_SC_INT && null_cnt < rows) enc = OBX_ENC_INTEGER_BASE_DIFF;
    else if (sc == OBX_SC_STRING && null_cnt < rows) {
      /* char columns with wide dictionaries: prefer the string
         transforms (the reference's cost ranking covers these the same
         way, ob_encoding_util.h:270-303) — STRING_DIFF when some byte
         positions are common, else HEX_PACKING when <=16 distinct chars */
      int vary_any = 0, common_any = 0;
      uint8_t seen[256]; memset(seen, 0, sizeof(seen));
      uint32_t nch = 0; int first = -1;
      for (uint32_t r = 0; r < rows; r++) {
        if (null_at(nulls, r)) continue;
        if (first < 0) first = (int)r;
        for (int i = 0; i < len; i++) {
          uint8_t cc = data[(size_t)r * len + i];
          if (!seen[cc]) { seen[cc] = 1; nch++; }
        }
      }
      for (int i = 0; first >= 0 && i < len; i++) {
        int v = 0;
        for (uint32_t r = 0; r < rows; r++) {
          if (null_at(nulls, r)) continue;
          if (data[(size_t)r * len + i] != data[(size_t)first * len + i]) {
            v = 1; break;
          }
        }
        if (v) vary_any = 1; else common_any = 1;
      }
      if (first >= 0 && common_any) enc = OBX_ENC_STRING_DIFF;
      else if (first >= 0 && nch <= 16) enc = OBX_ENC_HEX_PACKING;
      else enc = OBX_ENC_RAW;
      (void)vary_any;
    }
    else enc = OBX_ENC_RAW;
    if (enc == OBX_ENC_INTEGER_BASE_DIFF) {
      /* int-diff only pays when delta width < raw width; fall back to raw
         like ObIntegerBaseDiffEncoder::traverse (:156-199) */
      uint64_t mn = ~(uint64_t)0, mx = 0;
      for (uint32_t r = 0; r < rows; r++) {
        if (null_at(nulls, r)) continue;
        uint64_t v = 0; memcpy(&v, data + (size_t)r * len, (size_t)len);
        v &= mask;
        if (v < mn) mn = v;
        if (v > mx) mx = v;
      }
      if (mn >= mx) enc = OBX_ENC_RAW;
    }
  }

  switch (enc) {
    case OBX_ENC_RAW: {
      /* ObRawEncoder::traverse + store_fix_data (ob_raw_encoder.cpp:84-290) */
      ch->type = OBX_COL_RAW;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      if (null_cnt) ch->attr |= OBX_COL_ATTR_HAS_EXTEND_VALUE;
      fix_store_spec s = { block_ext_bit, null_cnt > 0, 0, 0 };
      raw_get_ctx g = { data, len, sc, mask };
      if (sc == OBX_SC_INT) {
        uint64_t mx = 0;
        for (uint32_t r = 0; r < rows; r++) {
          if (null_at(nulls, r)) continue;
          uint64_t v = raw_get(&g, r);
          if (v > mx) mx = v;
        }
        int bp = 0;
        int64_t size = obx_packing_size(&bp, mx);
        if (bp) { s.bit_len = (int)size; ch->attr |= OBX_COL_ATTR_BIT_PACKING; }
        else s.fix_len = (int)size;
      } else {
        s.fix_len = len; /* decimal/char: fixed datum bytes */
      }
      ch->length = (uint32_t)(s.bit_len ? s.bit_len : s.fix_len);
      int rc = store_fix_region(mb, &s, rows, nulls, raw_get, &g,
                                s.bit_len ? NULL : data, len);
      if (rc) return rc;
      break;
    }
    case OBX_ENC_DICT: {
      /* ObDictEncoder (ob_dict_encoder.cpp:84-440) */
      dict_builder db;
      int rc = dict_build(&db, data, nulls, rows, len);
      if (rc) { dict_free(&db); return rc; }
      dict_sort(&db, len, sc);
      uint32_t count = db.count;
      /* dict entry byte size: ObIntSC -> get_int_size(max), else datum len */
      int64_t entry_len = len;
      if (sc == OBX_SC_INT) {
        uint64_t mx = 0;
        for (uint32_t i = 0; i < count; i++) {
          uint64_t v = 0;
          memcpy(&v, db.entries + (size_t)i * len, (size_t)len);
          v &= mask;
          if (v > mx) mx = v;
        }
        entry_len = obx_int_size(mx);
      }
      uint64_t max_ref = count ? count - 1 : 0;
      if (null_cnt) max_ref = count; /* null ref = count */
      int bp = 0;
      int64_t ref_size = obx_packing_size(&bp, max_ref);
      ch->type = OBX_COL_DICT;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      if (bp) ch->attr |= OBX_COL_ATTR_BIT_PACKING;
      obx_dict_meta dm;
      memset(&dm, 0, sizeof(dm));
      dm.version = 0;
      dm.row_ref_size = (uint8_t)ref_size;
      dm.count = count;
      dm.data_size = (uint16_t)entry_len;
      dm.attr = OBX_DICT_ATTR_FIX_LENGTH | OBX_DICT_ATTR_IS_SORTED;
      int64_t meta_size = (int64_t)sizeof(dm) + (int64_t)count * entry_len;
      if (mb->len + meta_size > mb->cap) { dict_free(&db); return OBX_BUF_NOT_ENOUGH; }
      memcpy(mb->p + mb->len, &dm, sizeof(dm));
      uint8_t *pay = mb->p + mb->len + sizeof(dm);
      for (uint32_t i = 0; i < count; i++) {
        if (sc == OBX_SC_INT) {
          uint64_t v = 0;
          memcpy(&v, db.entries + (size_t)i * len, (size_t)len);
          v &= mask;
          memcpy(pay + (size_t)i * entry_len, &v, (size_t)entry_len);
        } else {
          memcpy(pay + (size_t)i * entry_len, db.entries + (size_t)i * len,
                 (size_t)len);
        }
      }
      mb->len += meta_size;
      ch->length = (uint32_t)meta_size;
      /* refs (store_fix_data, ob_dict_encoder.cpp:373-393): no ext bits —
         null is ref==count */
      fix_store_spec s = { block_ext_bit, 0, bp ? (int)ref_size : 0,
                           bp ? 0 : (int)ref_size };
      ref_get_ctx g = { &db };
      rc = store_fix_region(mb, &s, rows, NULL /*nulls folded into refs*/,
                            ref_get, &g, NULL, 0);
      dict_free(&db);
      if (rc) return rc;
      break;
    }
    case OBX_ENC_RLE: {
      /* ObRLEEncoder (ob_rle_encoder.cpp:60-170) */
      dict_builder db;
      int rc = dict_build(&db, data, nulls, rows, len);
      if (rc) { dict_free(&db); return rc; }
      dict_sort(&db, len, sc);
      uint32_t count = db.count;
      /* runs over sorted refs */
      uint64_t runs = 0; uint64_t max_row_id = 0; uint32_t prev = UINT32_MAX;
      for (uint32_t r = 0; r < rows; r++) {
        uint32_t x = dict_ref(&db, r);
        if (r == 0 || x != prev) { runs++; max_row_id = r; prev = x; }
      }
      uint64_t max_ref = count ? count - 1 : 0;
      if (null_cnt) max_ref = count;
      int64_t row_id_byte = obx_byte_packed_int_size(max_row_id);
      int64_t ref_byte = obx_byte_packed_int_size(max_ref);
      obx_rle_meta rm;
      memset(&rm, 0, sizeof(rm));
      rm.version = 0;
      rm.attr = (uint8_t)((row_id_byte & 7) | ((ref_byte & 7) << 3));
      rm.count = (uint32_t)runs;
      rm.offset = (uint32_t)(sizeof(rm) + runs * (row_id_byte + ref_byte));
      int64_t need = (int64_t)rm.offset;
      if (mb->len + need > mb->cap) { dict_free(&db); return OBX_BUF_NOT_ENOUGH; }
      memcpy(mb->p + mb->len, &rm, sizeof(rm));
      uint8_t *rid = mb->p + mb->len + sizeof(rm);
      uint8_t *ref = rid + runs * row_id_byte;
      uint64_t j = 0; prev = UINT32_MAX;
      for (uint32_t r = 0; r < rows; r++) {
        uint32_t x = dict_ref(&db, r);
        if (r == 0 || x != prev) {
          uint64_t rr = r, xx = x;
          memcpy(rid + j * row_id_byte, &rr, (size_t)row_id_byte);
          memcpy(ref + j * ref_byte, &xx, (size_t)ref_byte);
          j++; prev = x;
        }
      }
      mb->len += need;
      /* dict meta at +offset (ob_rle_encoder.cpp:119-127) */
      int64_t entry_len = len;
      if (sc == OBX_SC_INT) {
        uint64_t mx = 0;
        for (uint32_t i = 0; i < count; i++) {
          uint64_t v = 0;
          memcpy(&v, db.entries + (size_t)i * len, (size_t)len);
          v &= mask;
          if (v > mx) mx = v;
        }
        entry_len = obx_int_size(mx);
      }
      obx_dict_meta dm;
      memset(&dm, 0, sizeof(dm));
      dm.version = 0;
      dm.row_ref_size = 0; /* refs live in RLE runs, not a per-row stream */
      dm.count = count;
      dm.data_size = (uint16_t)entry_len;
      dm.attr = OBX_DICT_ATTR_FIX_LENGTH | OBX_DICT_ATTR_IS_SORTED;
      int64_t dsize = (int64_t)sizeof(dm) + (int64_t)count * entry_len;
      if (mb->len + dsize > mb->cap) { dict_free(&db); return OBX_BUF_NOT_ENOUGH; }
      memcpy(mb->p + mb->len, &dm, sizeof(dm));
      uint8_t *pay = mb->p + mb->len + sizeof(dm);
      for (uint32_t i = 0; i < count; i++) {
        if (sc == OBX_SC_INT) {
          uint64_t v = 0;
          memcpy(&v, db.entries + (size_t)i * len, (size_t)len);
          v &= mask;
          memcpy(pay + (size_t)i * entry_len, &v, (size_t)entry_len);
        } else {
          memcpy(pay + (size_t)i * entry_len, db.entries + (size_t)i * len,
                 (size_t)len);
        }
      }
      mb->len += dsize;
      ch->type = OBX_COL_RLE;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      ch->length = (uint32_t)(need + dsize);
      dict_free(&db);
      break;
    }
    case OBX_ENC_CONST: {
      /* ObConstEncoder (ob_const_encoder.cpp:52-350): the most frequent
         value (null counts as a candidate) becomes the const; every
         other row is an exception [ref + row_id] ahead of an embedded
         dict of the distinct values. Reference AUTO suitability bounds
         are MAX_EXCEPTION_SIZE=32 / MAX_EXCEPTION_PCT=10
         (ob_const_encoder.h:48-49); a FORCED const accepts anything the
         format itself can hold (count <= 255, refs <= 255). */
      int pure_const = (null_cnt == 0);
      for (uint32_t r = 1; pure_const && r < rows; r++) {
        if (memcmp(data, data + (size_t)r * len, (size_t)len) != 0)
          pure_const = 0;
      }
      int all_null = (null_cnt == rows);
      if (pure_const || all_null) {
        /* store_meta_without_dict (ob_const_encoder.cpp:147-200):
           const_ref 1 marks the null-const, 0 a value-const */
        obx_const_meta cm;
        memset(&cm, 0, sizeof(cm));
        cm.version = 0;
        cm.count = 0;
        cm.const_ref = all_null ? 1 : 0;
        cm.offset = (uint16_t)sizeof(cm);
        int64_t cell = all_null ? 0 : ((sc == OBX_SC_INT) ? tss : len);
        if (mb->len + (int64_t)sizeof(cm) + cell > mb->cap)
          return OBX_BUF_NOT_ENOUGH;
        memcpy(mb->p + mb->len, &cm, sizeof(cm));
        /* store_value (ob_const_encoder.cpp:200-240): ObIntSC stores
           type_store_size bytes, others datum bytes */
        if (cell) memcpy(mb->p + mb->len + sizeof(cm), data, (size_t)cell);
        mb->len += (int64_t)sizeof(cm) + cell;
        ch->type = OBX_COL_CONST;
        ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
        ch->length = (uint32_t)(sizeof(cm) + cell);
        break;
      }
      /* exception path: dict + [exc refs][exc row_ids] */
      dict_builder db;
      int rc = dict_build(&db, data, nulls, rows, len);
      if (rc) { dict_free(&db); return rc; }
      dict_sort(&db, len, sc);
      uint32_t count = db.count;
      /* choose the const ref: most frequent value; null (ref == count)
         competes too (ob_const_encoder.cpp:72-94) */
      uint32_t *freq = (uint32_t *)calloc((size_t)count + 1, 4);
      if (!freq) { dict_free(&db); return OBX_BUF_NOT_ENOUGH; }
      for (uint32_t r = 0; r < rows; r++) freq[dict_ref(&db, r)]++;
      uint32_t const_ref = 0, max_cnt = 0;
      for (uint32_t i = 0; i <= count; i++)
        if (freq[i] > max_cnt) { max_cnt = freq[i]; const_ref = i; }
      free(freq);
      uint32_t exc = rows - max_cnt;
      uint64_t max_ref = null_cnt ? count : (count ? count - 1 : 0);
      uint64_t max_row_id = 0;
      for (uint32_t r = rows; r-- > 0;) {
        if (dict_ref(&db, r) != const_ref) { max_row_id = r; break; }
      }
      if (exc > 255 || max_ref > 255) {
        dict_free(&db);
        return OBX_NOT_SUPPORTED; /* format bound (uint8 fields) */
      }
      int64_t row_id_byte = obx_byte_packed_int_size(max_row_id);
      obx_const_meta cm;
      memset(&cm, 0, sizeof(cm));
      cm.version = 0;
      cm.count = (uint8_t)exc;
      cm.const_ref = (uint8_t)const_ref;
      cm.attr = (uint8_t)(row_id_byte & 7);
      cm.offset = (uint16_t)(sizeof(cm) + exc * (row_id_byte + 1));
      if (mb->len + (int64_t)cm.offset > mb->cap) {
        dict_free(&db);
        return OBX_BUF_NOT_ENOUGH;
      }
      memcpy(mb->p + mb->len, &cm, sizeof(cm));
      /* dict_ref_gen before row_id_gen (ob_const_encoder.cpp:321-345) */
      uint8_t *eref = mb->p + mb->len + sizeof(cm);
      uint8_t *erid = eref + exc;
      uint32_t j = 0;
      for (uint32_t r = 0; r < rows && j < exc; r++) {
        uint32_t x = dict_ref(&db, r);
        if (x != const_ref) {
          eref[j] = (uint8_t)x;
          uint64_t rr = r;
          memcpy(erid + (size_t)j * row_id_byte, &rr, (size_t)row_id_byte);
          j++;
        }
      }
      mb->len += (int64_t)cm.offset;
      /* embedded dict meta at +offset, like RLE's */
      int64_t entry_len = len;
      if (sc == OBX_SC_INT) {
        uint64_t mx = 0;
        for (uint32_t i = 0; i < count; i++) {
          uint64_t v = 0;
          memcpy(&v, db.entries + (size_t)i * len, (size_t)len);
          v &= mask;
          if (v > mx) mx = v;
        }
        entry_len = obx_int_size(mx);
      }
      obx_dict_meta dm;
      memset(&dm, 0, sizeof(dm));
      dm.version = 0;
      dm.row_ref_size = 0; /* refs live in the exception list */
      dm.count = count;
      dm.data_size = (uint16_t)entry_len;
      dm.attr = OBX_DICT_ATTR_FIX_LENGTH | OBX_DICT_ATTR_IS_SORTED;
      int64_t dsize = (int64_t)sizeof(dm) + (int64_t)count * entry_len;
      if (mb->len + dsize > mb->cap) {
        dict_free(&db);
        return OBX_BUF_NOT_ENOUGH;
      }
      memcpy(mb->p + mb->len, &dm, sizeof(dm));
      uint8_t *pay = mb->p + mb->len + sizeof(dm);
      for (uint32_t i = 0; i < count; i++) {
        if (sc == OBX_SC_INT) {
          uint64_t v = 0;
          memcpy(&v, db.entries + (size_t)i * len, (size_t)len);
          v &= mask;
          memcpy(pay + (size_t)i * entry_len, &v, (size_t)entry_len);
        } else {
          memcpy(pay + (size_t)i * entry_len, db.entries + (size_t)i * len,
                 (size_t)len);
        }
      }
      mb->len += dsize;
      dict_free(&db);
      ch->type = OBX_COL_CONST;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      ch->length = (uint32_t)(cm.offset + dsize);
      break;
    }
    case OBX_ENC_INTEGER_BASE_DIFF: {
      /* ObIntegerBaseDiffEncoder (ob_integer_base_diff_encoder.cpp:139-280) */
      if (sc != OBX_SC_INT) return OBX_NOT_SUPPORTED;
      uint64_t mn = ~(uint64_t)0, mx = 0;
      int any = 0;
      for (uint32_t r = 0; r < rows; r++) {
        if (null_at(nulls, r)) continue;
        uint64_t v = 0; memcpy(&v, data + (size_t)r * len, (size_t)len);
        v &= mask;
        if (v < mn) mn = v;
        if (v > mx) mx = v;
        any = 1;
      }
      if (!any) return OBX_NOT_SUPPORTED;
      uint64_t delta = mx - mn;
      int bp = 0;
      int64_t dsize = obx_packing_size(&bp, delta);
      ch->type = OBX_COL_INTEGER_BASE_DIFF;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      if (null_cnt) ch->attr |= OBX_COL_ATTR_HAS_EXTEND_VALUE;
      if (bp) ch->attr |= OBX_COL_ATTR_BIT_PACKING;
      obx_intdiff_meta im;
      im.version = 0;
      im.length = (uint8_t)dsize;
      int64_t meta_size = (int64_t)sizeof(im) + tss;
      if (mb->len + meta_size > mb->cap) return OBX_BUF_NOT_ENOUGH;
      memcpy(mb->p + mb->len, &im, sizeof(im));
      memcpy(mb->p + mb->len + sizeof(im), &mn, (size_t)tss);
      mb->len += meta_size;
      ch->length = (uint32_t)meta_size;
      fix_store_spec s = { block_ext_bit, null_cnt > 0, bp ? (int)dsize : 0,
                           bp ? 0 : (int)dsize };
      diff_get_ctx g = { data, len, mn, mask };
      int rc = store_fix_region(mb, &s, rows, nulls, diff_get, &g, NULL, 0);
      if (rc) return rc;
      break;
    }
    case OBX_ENC_HEX_PACKING: {
      /* ObHexStringEncoder (ob_hex_string_encoder.{h,cpp}): <=16 distinct
         chars map to nibbles; build_index assigns indices in ascending
         char order; packing is HIGH nibble first. */
      if (sc != OBX_SC_STRING) return OBX_NOT_SUPPORTED;
      uint8_t seen[256]; memset(seen, 0, sizeof(seen));
      uint32_t nch = 0; int any = 0;
      for (uint32_t r = 0; r < rows; r++) {
        if (null_at(nulls, r)) continue;
        any = 1;
        for (int i = 0; i < len; i++) {
          uint8_t cc = data[(size_t)r * len + i];
          if (!seen[cc]) { seen[cc] = 1; nch++; }
        }
      }
      if (!any || nch > 16) return OBX_NOT_SUPPORTED;
      uint8_t chars[16]; uint8_t idx_of[256]; uint32_t k = 0;
      for (int i = 0; i < 256; i++)
        if (seen[i]) { idx_of[i] = (uint8_t)k; chars[k++] = (uint8_t)i; }
      ch->type = OBX_COL_HEX_PACKING;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      if (null_cnt) ch->attr |= OBX_COL_ATTR_HAS_EXTEND_VALUE;
      obx_hex_meta hm = { 0, (uint8_t)nch, (uint16_t)len };
      int64_t meta_size = (int64_t)sizeof(hm) + nch;
      if (mb->len + meta_size > mb->cap) return OBX_BUF_NOT_ENOUGH;
      memcpy(mb->p + mb->len, &hm, sizeof(hm));
      memcpy(mb->p + mb->len + sizeof(hm), chars, nch);
      mb->len += meta_size;
      ch->length = (uint32_t)meta_size;
      int stride = (len + 1) / 2;
      uint8_t *scr = (uint8_t *)calloc((size_t)rows * stride + 1, 1);
      if (!scr) return OBX_INTERNAL_ERROR;
      for (uint32_t r = 0; r < rows; r++) {
        if (null_at(nulls, r)) continue;
        uint8_t *rp = scr + (size_t)r * stride;
        for (int i = 0; i < len; i++) {
          uint8_t nib = idx_of[data[(size_t)r * len + i]];
          rp[i / 2] |= (uint8_t)(nib << (((i + 1) % 2) * 4));
        }
      }
      fix_store_spec s = { block_ext_bit, null_cnt > 0, 0, stride };
      int rc = store_fix_region(mb, &s, rows, nulls, NULL, NULL, scr, stride);
      free(scr);
      if (rc) return rc;
      break;
    }
    case OBX_ENC_STRING_DIFF: {
      /* ObStringDiffEncoder (ob_string_diff_encoder.{h,cpp}): byte
         positions that never vary across non-null rows are stored once
         (common_data); varying runs are described by DiffDesc bytes
         (bit0 = diff, bits1-7 = run length) and each row stores only its
         diff bytes, nibble-packed like HEX_PACKING when the diff chars
         fit 16 (is_hex_packing). */
      if (sc != OBX_SC_STRING || len < 1) return OBX_NOT_SUPPORTED;
      int first = -1;
      for (uint32_t r = 0; r < rows; r++)
        if (!null_at(nulls, r)) { first = (int)r; break; }
      if (first < 0) return OBX_NOT_SUPPORTED;
      uint8_t vary[256]; memset(vary, 0, (size_t)len);
      for (uint32_t r = 0; r < rows; r++) {
        if (null_at(nulls, r)) continue;
        for (int i = 0; i < len; i++)
          if (data[(size_t)r * len + i] != data[(size_t)first * len + i])
            vary[i] = 1;
      }
      uint8_t descs[256]; int nd = 0; int diff_len = 0;
      for (int i = 0; i < len;) {
        int j = i;
        while (j < len && vary[j] == vary[i] && j - i < 127) j++;
        descs[nd++] = (uint8_t)((vary[i] & 1) | ((j - i) << 1));
        if (vary[i]) diff_len += j - i;
        i = j;
      }
      /* hex-packability of the diff bytes only */
      uint8_t seen[256]; memset(seen, 0, sizeof(seen));
      uint32_t nch = 0;
      for (uint32_t r = 0; r < rows && nch <= 16; r++) {
        if (null_at(nulls, r)) continue;
        for (int i = 0; i < len; i++) {
          if (!vary[i]) continue;
          uint8_t cc = data[(size_t)r * len + i];
          if (!seen[cc]) { seen[cc] = 1; nch++; }
        }
      }
      int use_hex = diff_len > 0 && nch <= 16 && (diff_len + 1) / 2 < diff_len;
      uint8_t chars[16]; uint8_t idx_of[256]; uint32_t k = 0;
      if (use_hex)
        for (int i = 0; i < 256; i++)
          if (seen[i]) { idx_of[i] = (uint8_t)k; chars[k++] = (uint8_t)i; }
      ch->type = OBX_COL_STRING_DIFF;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      if (null_cnt) ch->attr |= OBX_COL_ATTR_HAS_EXTEND_VALUE;
      obx_sdiff_meta sm2 = { 0, (uint8_t)(use_hex ? nch : 0), (uint16_t)len,
                             (uint8_t)nd };
      int64_t meta_size = (int64_t)sizeof(sm2) + nd + (use_hex ? nch : 0) +
                          (len - diff_len);
      if (mb->len + meta_size > mb->cap) return OBX_BUF_NOT_ENOUGH;
      uint8_t *mp = mb->p + mb->len;
      memcpy(mp, &sm2, sizeof(sm2)); mp += sizeof(sm2);
      memcpy(mp, descs, (size_t)nd); mp += nd;
      if (use_hex) { memcpy(mp, chars, nch); mp += nch; }
      for (int i = 0; i < len; i++)
        if (!vary[i]) *mp++ = data[(size_t)first * len + i];
      mb->len += meta_size;
      ch->length = (uint32_t)meta_size;
      int stride = use_hex ? (diff_len + 1) / 2 : diff_len;
      uint8_t *scr = (uint8_t *)calloc((size_t)rows * (stride ? stride : 1) + 1, 1);
      if (!scr) return OBX_INTERNAL_ERROR;
      for (uint32_t r = 0; r < rows && stride; r++) {
        if (null_at(nulls, r)) continue;
        uint8_t *rp = scr + (size_t)r * stride;
        int pos = 0;
        for (int i = 0; i < len; i++) {
          if (!vary[i]) continue;
          uint8_t cc = data[(size_t)r * len + i];
          if (use_hex)
            rp[pos / 2] |= (uint8_t)(idx_of[cc] << (((pos + 1) % 2) * 4));
          else
            rp[pos] = cc;
          pos++;
        }
      }
      fix_store_spec s = { block_ext_bit, null_cnt > 0, 0, stride };
      int rc = store_fix_region(mb, &s, rows, nulls, NULL, NULL, scr,
                                stride ? stride : 1);
      free(scr);
      if (rc) return rc;
      break;
    }
    case OBX_ENC_STRING_PREFIX: {
      /* ObStringPrefixEncoder (ob_string_prefix_encoder.{h,cpp}); our
         writer picks the longest equal-length prefix with <=15 distinct
         values (the reference's ObMultiPrefixTree is writer policy — the
         FORMAT carries per-prefix lengths via the end-offset index). */
      if (sc != OBX_SC_STRING || len < 2) return OBX_NOT_SUPPORTED;
      int first = -1;
      for (uint32_t r = 0; r < rows; r++)
        if (!null_at(nulls, r)) { first = (int)r; break; }
      if (first < 0) return OBX_NOT_SUPPORTED;
      int plen = 0;
      uint8_t pfx[15 * 8];
      uint32_t np = 0;
      for (int p = len - 1; p >= 1; p--) {
        np = 0;
        int ok2 = 1;
        for (uint32_t r = 0; r < rows && ok2; r++) {
          if (null_at(nulls, r)) continue;
          const uint8_t *s2 = data + (size_t)r * len;
          uint32_t j = 0;
          for (; j < np; j++)
            if (memcmp(pfx + (size_t)j * p, s2, (size_t)p) == 0) break;
          if (j == np) {
            if (np >= 15) { ok2 = 0; break; }
            memcpy(pfx + (size_t)np * p, s2, (size_t)p);
            np++;
          }
        }
        if (ok2) { plen = p; break; }
      }
      if (plen < 1) return OBX_NOT_SUPPORTED;
      const int max_suffix = len - plen;
      /* suffix hex packability */
      uint8_t seen[256]; memset(seen, 0, sizeof(seen));
      uint32_t nch = 0;
      for (uint32_t r = 0; r < rows && nch <= 16; r++) {
        if (null_at(nulls, r)) continue;
        for (int i = plen; i < len; i++) {
          uint8_t cc = data[(size_t)r * len + i];
          if (!seen[cc]) { seen[cc] = 1; nch++; }
        }
      }
      int use_hex = nch <= 16 && (max_suffix + 1) / 2 < max_suffix;
      uint8_t chars[16]; uint8_t idx_of[256]; uint32_t k2 = 0;
      if (use_hex)
        for (int i = 0; i < 256; i++)
          if (seen[i]) { idx_of[i] = (uint8_t)k2; chars[k2++] = (uint8_t)i; }
      int pib = (int)obx_byte_packed_int_size((uint64_t)np * plen);
      obx_sprefix_meta pm;
      pm.version = 0;
      pm.count = (uint8_t)np;
      pm.string_size = (uint16_t)len;
      pm.hex_char_cnt = (uint8_t)(use_hex ? nch : 0);
      pm.pib = (uint8_t)pib;
      int64_t meta_size = (int64_t)sizeof(pm) + (use_hex ? nch : 0) +
                          (int64_t)np * pib + (int64_t)np * plen;
      if (mb->len + meta_size > mb->cap) return OBX_BUF_NOT_ENOUGH;
      uint8_t *mp = mb->p + mb->len;
      memcpy(mp, &pm, sizeof(pm)); mp += sizeof(pm);
      if (use_hex) { memcpy(mp, chars, nch); mp += nch; }
      for (uint32_t j = 0; j < np; j++) { /* cumulative END offsets */
        uint64_t end = (uint64_t)(j + 1) * plen;
        memcpy(mp, &end, (size_t)pib); mp += pib;
      }
      for (uint32_t j = 0; j < np; j++) {
        memcpy(mp, pfx + (size_t)j * plen, (size_t)plen); mp += plen;
      }
      mb->len += meta_size;
      ch->type = OBX_COL_STRING_PREFIX;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      if (null_cnt) ch->attr |= OBX_COL_ATTR_HAS_EXTEND_VALUE;
      ch->length = (uint32_t)meta_size;
      int stride = 1 + (use_hex ? (max_suffix + 1) / 2 : max_suffix);
      uint8_t *scr = (uint8_t *)calloc((size_t)rows * stride + 1, 1);
      if (!scr) return OBX_INTERNAL_ERROR;
      for (uint32_t r = 0; r < rows; r++) {
        if (null_at(nulls, r)) continue;
        const uint8_t *s2 = data + (size_t)r * len;
        uint32_t j = 0;
        for (; j < np; j++)
          if (memcmp(pfx + (size_t)j * plen, s2, (size_t)plen) == 0) break;
        uint8_t *rp = scr + (size_t)r * stride;
        rp[0] = (uint8_t)j;
        for (int i = 0; i < max_suffix; i++) {
          uint8_t cc = s2[plen + i];
          if (use_hex)
            rp[1 + i / 2] |= (uint8_t)(idx_of[cc] << (((i + 1) % 2) * 4));
          else
            rp[1 + i] = cc;
        }
      }
      fix_store_spec s = { block_ext_bit, null_cnt > 0, 0, stride };
      int rc = store_fix_region(mb, &s, rows, nulls, NULL, NULL, scr,
                                stride);
      free(scr);
      if (rc) return rc;
      break;
    }
    case OBX_ENC_COLUMN_SUBSTR: {
      /* ObInterColSubStrEncoder (ob_inter_column_substring_encoder.{h,cpp})
         restated with same_start + fix_length always set: find the best
         uniform start slice of the nearest previous wider char column;
         rows that are not that substring (or differ in null-ness) go to
         the exception list. */
      if (sc != OBX_SC_STRING) return OBX_NOT_SUPPORTED;
      int ref = -1;
      for (int j = (int)col_idx - 1; j >= 0; j--) {
        if (obx_store_class(all_cols[j].obj_type) == OBX_SC_STRING &&
            all_cols[j].len >= len) { ref = j; break; }
      }
      if (ref < 0 || !all_data) return OBX_NOT_SUPPORTED;
      const uint8_t *rd = all_data[ref];
      const uint8_t *rn = all_nulls ? all_nulls[ref] : NULL;
      const int rlen = all_cols[ref].len;
      uint32_t best_exc = rows + 1; int best_start = 0;
      for (int st = 0; st + len <= rlen; st++) {
        uint32_t exc2 = 0;
        for (uint32_t r = 0; r < rows; r++) {
          int ln = null_at(nulls, r), rnl = null_at(rn, r);
          if (ln != rnl ||
              (!ln && memcmp(data + (size_t)r * len,
                             rd + (size_t)r * rlen + st, (size_t)len) != 0))
            exc2++;
        }
        if (exc2 < best_exc) { best_exc = exc2; best_start = st; }
      }
      if (best_exc * 4 > rows) return OBX_NOT_SUPPORTED;
      int rib = (int)obx_byte_packed_int_size(rows ? rows - 1 : 0);
      obx_substr_meta sm3;
      sm3.version = 0;
      sm3.attr = 3; /* same_start | fix_length */
      sm3.start_pos = (uint16_t)best_start;
      sm3.ref_col = (uint16_t)ref;
      sm3.exc_cnt = (uint16_t)best_exc;
      sm3.rib = (uint8_t)rib;
      sm3.ref_len = (uint8_t)rlen;
      int64_t meta_size = (int64_t)sizeof(sm3) + (int64_t)best_exc * rib +
                          (best_exc + 7) / 8 + (int64_t)best_exc * len;
      if (mb->len + meta_size > mb->cap) return OBX_BUF_NOT_ENOUGH;
      uint8_t *mp = mb->p + mb->len;
      memcpy(mp, &sm3, sizeof(sm3)); mp += sizeof(sm3);
      uint8_t *rid_p = mp;
      uint8_t *nb_p = rid_p + (size_t)best_exc * rib;
      uint8_t *dat_p = nb_p + (best_exc + 7) / 8;
      memset(nb_p, 0, (best_exc + 7) / 8);
      uint32_t k3 = 0;
      for (uint32_t r = 0; r < rows; r++) {
        int ln = null_at(nulls, r), rnl = null_at(rn, r);
        if (ln == rnl &&
            (ln || memcmp(data + (size_t)r * len,
                          rd + (size_t)r * rlen + best_start,
                          (size_t)len) == 0))
          continue;
        memcpy(rid_p + (size_t)k3 * rib, &r, (size_t)rib);
        if (ln) {
          nb_p[k3 / 8] |= (uint8_t)(1u << (k3 % 8));
          memset(dat_p + (size_t)k3 * len, 0, (size_t)len);
        } else {
          memcpy(dat_p + (size_t)k3 * len, data + (size_t)r * len,
                 (size_t)len);
        }
        k3++;
      }
      mb->len += meta_size;
      ch->type = OBX_COL_SUBSTR;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      ch->length = (uint32_t)meta_size;
      break;
    }
    case OBX_ENC_COLUMN_EQUAL: {
      /* ObColumnEqualEncoder (ob_column_equal_encoder.{h,cpp}): equals the
         nearest previous column with the same shape except at exception
         rows; is_datum_equal treats both-null as equal (h:83-101). */
      int ref = -1;
      for (int j = (int)col_idx - 1; j >= 0; j--) {
        if (all_cols[j].len == cs->len &&
            obx_store_class(all_cols[j].obj_type) == sc) { ref = j; break; }
      }
      if (ref < 0 || !all_data) return OBX_NOT_SUPPORTED;
      const uint8_t *rd = all_data[ref];
      const uint8_t *rn = all_nulls ? all_nulls[ref] : NULL;
      uint32_t exc = 0;
      for (uint32_t r = 0; r < rows; r++) {
        int ln = null_at(nulls, r), rnl = null_at(rn, r);
        if (ln != rnl ||
            (!ln && memcmp(data + (size_t)r * len, rd + (size_t)r * len,
                           (size_t)len) != 0))
          exc++;
      }
      if (exc * 4 > rows) return OBX_NOT_SUPPORTED; /* not worth it */
      int rib = (int)obx_byte_packed_int_size(rows ? rows - 1 : 0);
      obx_coleq_meta em;
      em.version = 0;
      em.ref_col = (uint16_t)ref;
      em.exc_cnt = (uint16_t)exc;
      em.rib = (uint8_t)rib;
      int64_t meta_size = (int64_t)sizeof(em) + (int64_t)exc * rib +
                          (exc + 7) / 8 + (int64_t)exc * len;
      if (mb->len + meta_size > mb->cap) return OBX_BUF_NOT_ENOUGH;
      uint8_t *mp = mb->p + mb->len;
      memcpy(mp, &em, sizeof(em)); mp += sizeof(em);
      uint8_t *rid_p = mp;
      uint8_t *nb_p = rid_p + (size_t)exc * rib;
      uint8_t *dat_p = nb_p + (exc + 7) / 8;
      memset(nb_p, 0, (exc + 7) / 8);
      uint32_t k = 0;
      for (uint32_t r = 0; r < rows; r++) {
        int ln = null_at(nulls, r), rnl = null_at(rn, r);
        if (ln == rnl &&
            (ln || memcmp(data + (size_t)r * len, rd + (size_t)r * len,
                          (size_t)len) == 0))
          continue;
        memcpy(rid_p + (size_t)k * rib, &r, (size_t)rib);
        if (ln) {
          nb_p[k / 8] |= (uint8_t)(1u << (k % 8));
          memset(dat_p + (size_t)k * len, 0, (size_t)len);
        } else {
          memcpy(dat_p + (size_t)k * len, data + (size_t)r * len,
                 (size_t)len);
        }
        k++;
      }
      mb->len += meta_size;
      ch->type = OBX_COL_EQUAL;
      ch->attr |= OBX_COL_ATTR_FIX_LENGTH;
      ch->length = (uint32_t)meta_size;
      break;
    }
    default:
      return OBX_NOT_SUPPORTED;
  }
  return OBX_SUCCESS;
}

int64_t obx_encode_block(const obx_col_schema *cols, uint16_t n_cols,
                         const uint8_t *const *col_data,
                         const uint8_t *const *null_bitmaps,
                         uint32_t row_count, const uint8_t *enc_request,
                         uint8_t *out, int64_t out_cap) {
  if (!cols || !n_cols || !col_data || !row_count || !out)
    return OBX_INVALID_ARGUMENT;
  const int64_t hdr = OBX_MICRO_HEADER_SIZE;
  const int64_t chs = (int64_t)n_cols * sizeof(obx_col_header);
  if (hdr + chs + 8 > out_cap) return OBX_BUF_NOT_ENOUGH;

  /* block-level extend value bit (store_encoding_meta_and_fix_cols,
     ob_micro_block_encoder.cpp:499-512): 1 if any column has nulls */
  int ext_bit = 0;
  for (uint16_t c = 0; c < n_cols; c++) {
    if (null_bitmaps && null_bitmaps[c]) {
      for (uint32_t r = 0; r < row_count; r++) {
        if (null_at(null_bitmaps[c], r)) { ext_bit = 1; break; }
      }
    }
    if (ext_bit) break;
  }

  obx_col_header *chp = (obx_col_header *)(out + hdr);
  memset(out, 0, (size_t)(hdr + chs));
  enc_buf mb = { out + hdr + chs, 0, out_cap - hdr - chs - 8 };
  for (uint16_t c = 0; c < n_cols; c++) {
    uint8_t enc = enc_request ? enc_request[c] : OBX_ENC_AUTO;
    int rc = encode_column(&mb, &chp[c], &cols[c], col_data[c],
                           null_bitmaps ? null_bitmaps[c] : NULL, row_count,
                           enc, ext_bit ? 1 : 0,
                           cols, col_data, null_bitmaps, c);
    if (rc) return rc;
  }

  obx_micro_header *h = (obx_micro_header *)out;
  memset(h, 0, sizeof(*h));
  h->magic = OBX_MICRO_BLOCK_MAGIC;
  h->version = OBX_MICRO_BLOCK_VERSION;
  h->header_size = OBX_MICRO_HEADER_SIZE;
  h->column_count = n_cols;
  h->rowkey_column_count = 1; /* >0 required by is_valid(); no rowkey use */
  h->row_count = row_count;
  h->row_store_type = OBX_ROW_STORE_ENCODING;
  obx_hdr_set_opt(h, 0 /*row_index_byte: all cols fix-stored*/,
                  (uint8_t)ext_bit);
  h->var_column_count = 0;
  h->row_data_offset = (uint32_t)(hdr + chs + mb.len);
  int64_t total = hdr + chs + mb.len;
  h->original_length = (int32_t)total;
  h->data_length = (int32_t)total;
  h->data_zlength = (int32_t)total;
  h->data_checksum =
      (int64_t)obx_crc32c(out + OBX_MICRO_HEADER_SIZE,
                          total - OBX_MICRO_HEADER_SIZE);
  /* set_header_checksum (ob_micro_block_header.cpp:20-50):
     xor of 16-bit words of the listed fields */
  {
    int16_t ck = 0;
    ck ^= h->magic; ck ^= h->version;
    ck ^= (int16_t)h->row_store_type; ck ^= (int16_t)h->opt;
#define FMT(v) do { uint64_t x = (uint64_t)(v); \
    for (int i = 0; i < 4; i++) ck = (int16_t)(ck ^ (int16_t)((x >> (i*16)) & 0xFFFF)); } while (0)
#define FMT32(v) do { uint32_t x = (uint32_t)(v); \
    for (int i = 0; i < 2; i++) ck = (int16_t)(ck ^ (int16_t)((x >> (i*16)) & 0xFFFF)); } while (0)
    FMT32(h->column_count); FMT32(h->rowkey_column_count);
    FMT32(0 /*has_column_checksum*/); FMT32(h->var_column_count);
    FMT(h->header_size); FMT(h->row_count); FMT(h->row_data_offset);
    FMT(h->original_length); FMT(h->max_merged_trans_version);
    FMT(h->data_length); FMT(h->data_zlength); FMT(h->data_checksum);
#undef FMT
#undef FMT32
    h->header_checksum = ck;
  }
  return total;
}

/* ===================================================================== */
/* decoder                                                               */
/* ===================================================================== */

typedef struct col_dec {
  const obx_col_header *ch;
  const uint8_t *meta;       /* block meta region + ch->offset */
  const uint8_t *data;       /* column bit/fix data region */
  int64_t bits_off;          /* bit offset of packed values (after ext bits) */
  int64_t fix_off;           /* byte offset of fixed data (after bit region) */
  /* dict */
  const obx_dict_meta *dm;
  const uint8_t *dict_pay;
  const uint8_t *refs;
  /* rle */
  const obx_rle_meta *rm;
  const uint8_t *rle_rid, *rle_ref;
  /* const */
  const obx_const_meta *cm;
  /* int diff */
  const obx_intdiff_meta *im;
  uint64_t base;
  /* string transforms (HEX_PACKING / STRING_DIFF) */
  const obx_hex_meta *hm;
  const obx_sdiff_meta *sm;
  const uint8_t *str_chars;  /* hex char array */
  const uint8_t *str_descs;  /* diff descs */
  const uint8_t *str_common; /* common bytes */
  /* STRING_PREFIX */
  const obx_sprefix_meta *pm;
  const uint8_t *pfx_ends, *pfx_data;
  /* COLUMN_EQUAL / COLUMN_SUBSTR: block context for the ref decode */
  const obx_coleq_meta *em;
  const obx_substr_meta *ssm;
  const uint8_t *exc_rid, *exc_nb, *exc_dat;
  const obx_col_header *chp0; /* column header array base */
  const uint8_t *meta_region;
} col_dec;

struct col_dec;
static int col_dec_row(const col_dec *d, const obx_micro_header *h,
                       const obx_col_schema *cs, uint32_t r,
                       int64_t *out, int *is_null);

static int col_dec_init(col_dec *d, const obx_micro_header *h,
                        const obx_col_header *ch, const uint8_t *meta_region) {
  memset(d, 0, sizeof(*d));
  d->ch = ch;
  d->meta = meta_region + ch->offset;
  /* block context for span encodings (COLUMN_EQUAL's ref decode); the
     header array immediately precedes the meta region */
  d->chp0 = (const obx_col_header *)(meta_region -
                                     (size_t)h->column_count *
                                         sizeof(obx_col_header));
  d->meta_region = meta_region;
  int ext = (ch->attr & OBX_COL_ATTR_HAS_EXTEND_VALUE) ? 1 : 0;
  int evb = obx_hdr_extend_value_bit(h);
  switch (ch->type) {
    case OBX_COL_RAW: {
      d->data = d->meta;
      int64_t ext_bits = ext ? (int64_t)evb * h->row_count : 0;
      if (ch->attr & OBX_COL_ATTR_BIT_PACKING) {
        d->bits_off = ext_bits;
      } else {
        d->fix_off = (ext_bits + 7) / 8;
      }
      break;
    }
    case OBX_COL_DICT: {
      d->dm = (const obx_dict_meta *)d->meta;
      d->dict_pay = d->meta + sizeof(obx_dict_meta);
      d->refs = d->meta + ch->length; /* ob_dict_decoder.cpp:222 */
      d->data = d->refs;
      break;
    }
    case OBX_COL_RLE: {
      d->rm = (const obx_rle_meta *)d->meta;
      d->rle_rid = d->meta + sizeof(obx_rle_meta);
      int rib = d->rm->attr & 7, rfb = (d->rm->attr >> 3) & 7;
      d->rle_ref = d->rle_rid + (int64_t)d->rm->count * rib;
      (void)rfb;
      d->dm = (const obx_dict_meta *)(d->meta + d->rm->offset);
      d->dict_pay = (const uint8_t *)d->dm + sizeof(obx_dict_meta);
      break;
    }
    case OBX_COL_CONST: {
      d->cm = (const obx_const_meta *)d->meta;
      if (d->cm->count > 0) {
        d->dm = (const obx_dict_meta *)(d->meta + d->cm->offset);
        d->dict_pay = (const uint8_t *)d->dm + sizeof(obx_dict_meta);
      } else {
        d->dict_pay = d->meta + d->cm->offset; /* const datum bytes */
      }
      break;
    }
    case OBX_COL_INTEGER_BASE_DIFF: {
      d->im = (const obx_intdiff_meta *)d->meta;
      int64_t tss = obx_type_store_size(ch->obj_type);
      if (tss < 1 || tss > 8) return OBX_NOT_SUPPORTED;
      d->base = 0;
      memcpy(&d->base, d->meta + sizeof(obx_intdiff_meta), (size_t)tss);
      d->base = obx_sign_extend(d->base, tss,
                                obx_store_class(ch->obj_type) == OBX_SC_INT);
      d->data = d->meta + ch->length; /* diffs follow meta */
      int64_t ext_bits = ext ? (int64_t)evb * h->row_count : 0;
      if (ch->attr & OBX_COL_ATTR_BIT_PACKING) {
        d->bits_off = ext_bits;
      } else {
        d->fix_off = (ext_bits + 7) / 8;
      }
      break;
    }
    case OBX_COL_HEX_PACKING: {
      d->hm = (const obx_hex_meta *)d->meta;
      d->str_chars = d->meta + sizeof(obx_hex_meta);
      d->data = d->meta + ch->length;
      int64_t ext_bits = ext ? (int64_t)evb * h->row_count : 0;
      d->fix_off = (ext_bits + 7) / 8;
      break;
    }
    case OBX_COL_STRING_PREFIX: {
      d->pm = (const obx_sprefix_meta *)d->meta;
      d->str_chars = d->meta + sizeof(obx_sprefix_meta);
      d->pfx_ends = d->str_chars + d->pm->hex_char_cnt;
      d->pfx_data = d->pfx_ends + (size_t)d->pm->count * d->pm->pib;
      d->data = d->meta + ch->length;
      int64_t ext_bits = ext ? (int64_t)evb * h->row_count : 0;
      d->fix_off = (ext_bits + 7) / 8;
      break;
    }
    case OBX_COL_SUBSTR: {
      d->ssm = (const obx_substr_meta *)d->meta;
      if (d->ssm->ref_col >= h->column_count) return OBX_INVALID_ARGUMENT;
      uint8_t rt = d->chp0[d->ssm->ref_col].type;
      if (rt == OBX_COL_EQUAL || rt == OBX_COL_SUBSTR)
        return OBX_NOT_SUPPORTED; /* one level only */
      d->exc_rid = d->meta + sizeof(obx_substr_meta);
      d->exc_nb = d->exc_rid + (size_t)d->ssm->exc_cnt * d->ssm->rib;
      d->exc_dat = d->exc_nb + (d->ssm->exc_cnt + 7) / 8;
      break;
    }
    case OBX_COL_EQUAL: {
      d->em = (const obx_coleq_meta *)d->meta;
      if (d->em->ref_col >= h->column_count) return OBX_INVALID_ARGUMENT;
      if (d->chp0[d->em->ref_col].type == OBX_COL_EQUAL)
        return OBX_NOT_SUPPORTED; /* one level only */
      d->exc_rid = d->meta + sizeof(obx_coleq_meta);
      d->exc_nb = d->exc_rid + (size_t)d->em->exc_cnt * d->em->rib;
      d->exc_dat = d->exc_nb + (d->em->exc_cnt + 7) / 8;
      break;
    }
    case OBX_COL_STRING_DIFF: {
      d->sm = (const obx_sdiff_meta *)d->meta;
      d->str_descs = d->meta + sizeof(obx_sdiff_meta);
      d->str_chars = d->str_descs + d->sm->diff_desc_cnt;
      d->str_common = d->str_chars + d->sm->hex_char_cnt;
      d->data = d->meta + ch->length;
      int64_t ext_bits = ext ? (int64_t)evb * h->row_count : 0;
      d->fix_off = (ext_bits + 7) / 8;
      break;
    }
    default:
      return OBX_NOT_SUPPORTED;
  }
  return OBX_SUCCESS;
}

/* is row null? (ext bits for RAW/INT_DIFF; ref==count for DICT/RLE;
 * const_ref for CONST null blocks) */
static inline int col_dec_is_null(const col_dec *d, const obx_micro_header *h,
                                  uint32_t r) {
  int evb = obx_hdr_extend_value_bit(h);
  switch (d->ch->type) {
    case OBX_COL_RAW:
    case OBX_COL_INTEGER_BASE_DIFF:
    case OBX_COL_HEX_PACKING:
    case OBX_COL_STRING_DIFF:
    case OBX_COL_STRING_PREFIX:
      if (!(d->ch->attr & OBX_COL_ATTR_HAS_EXTEND_VALUE)) return 0;
      return obx_bs_get(d->data, (int64_t)r * evb, evb) != 0;
    default:
      return 0; /* dict-family nulls surface via ref == count below */
  }
}

/* dict ref of row r for DICT encoding */
static inline uint64_t dec_dict_ref(const col_dec *d, uint32_t r) {
  if (d->ch->attr & OBX_COL_ATTR_BIT_PACKING) {
    return obx_bs_get(d->refs, (int64_t)r * d->dm->row_ref_size,
                      d->dm->row_ref_size);
  }
  uint64_t v = 0;
  memcpy(&v, d->refs + (size_t)r * d->dm->row_ref_size, d->dm->row_ref_size);
  return v;
}

/* run index for RLE row r: last run with start <= r
 * (upper_bound, ob_rle_decoder.cpp:18-31) */
static inline uint64_t rle_run_of(const col_dec *d, uint32_t r) {
  int rib = d->rm->attr & 7;
  uint64_t lo = 0, hi = d->rm->count; /* find first start > r, then -1 */
  while (lo < hi) {
    uint64_t mid = (lo + hi) / 2;
    uint64_t s = 0;
    memcpy(&s, d->rle_rid + mid * rib, (size_t)rib);
    if (s <= r) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

static inline uint64_t rle_ref_of(const col_dec *d, uint32_t r) {
  int rib = d->rm->attr & 7, rfb = (d->rm->attr >> 3) & 7;
  (void)rib;
  uint64_t run = rle_run_of(d, r);
  uint64_t v = 0;
  memcpy(&v, d->rle_ref + run * rfb, (size_t)rfb);
  return v;
}

/* decode row r into (value_int64, is_null); for char columns value is the
 * raw bytes packed little-endian into the int64 (len <= 8). */
static int col_dec_row(const col_dec *d, const obx_micro_header *h,
                       const obx_col_schema *cs, uint32_t r,
                       int64_t *out, int *is_null) {
  const int sc = obx_store_class(cs->obj_type);
  const int64_t tss = obx_type_store_size(cs->obj_type);
  *is_null = 0;
  switch (d->ch->type) {
    case OBX_COL_RAW: {
      if (col_dec_is_null(d, h, r)) { *is_null = 1; *out = 0; return 0; }
      uint64_t v;
      if (d->ch->attr & OBX_COL_ATTR_BIT_PACKING) {
        v = obx_bs_get(d->data, d->bits_off + (int64_t)r * d->ch->length,
                       d->ch->length);
        /* bit-packed ints are zero-extended (ObRawDecoder::decode,
           ob_raw_decoder.cpp:503-520: plain memcpy, no mask) */
      } else {
        v = 0;
        memcpy(&v, d->data + d->fix_off + (size_t)r * d->ch->length,
               d->ch->length);
        if (sc == OBX_SC_INT) v = obx_sign_extend(v, tss, 1);
      }
      *out = (int64_t)v;
      return 0;
    }
    case OBX_COL_DICT: {
      uint64_t ref = dec_dict_ref(d, r);
      if (ref >= d->dm->count) { *is_null = 1; *out = 0; return 0; }
      uint64_t v = 0;
      memcpy(&v, d->dict_pay + ref * d->dm->data_size, d->dm->data_size);
      if (sc == OBX_SC_INT) v = obx_sign_extend(v, tss, 1);
      *out = (int64_t)v;
      return 0;
    }
    case OBX_COL_RLE: {
      uint64_t ref = rle_ref_of(d, r);
      if (ref >= d->dm->count) { *is_null = 1; *out = 0; return 0; }
      uint64_t v = 0;
      memcpy(&v, d->dict_pay + ref * d->dm->data_size, d->dm->data_size);
      if (sc == OBX_SC_INT) v = obx_sign_extend(v, tss, 1);
      *out = (int64_t)v;
      return 0;
    }
    case OBX_COL_CONST: {
      if (d->cm->count == 0) {
        if (d->cm->const_ref > 0) { *is_null = 1; *out = 0; return 0; }
        uint64_t v = 0;
        int64_t cell = (sc == OBX_SC_INT) ? tss : cs->len;
        memcpy(&v, d->dict_pay, (size_t)cell);
        if (sc == OBX_SC_INT) v = obx_sign_extend(v, tss, 1);
        *out = (int64_t)v;
        return 0;
      }
      /* exception path: refs first, then row_ids (ob_const_encoder.cpp:
         store_meta, dict_ref_gen before row_id_gen) */
      int rib = d->cm->attr & 7;
      const uint8_t *exc_ref = d->meta + sizeof(obx_const_meta);
      const uint8_t *exc_rid = exc_ref + d->cm->count;
      uint64_t ref = d->cm->const_ref;
      for (uint32_t i = 0; i < d->cm->count; i++) {
        uint64_t rid = 0;
        memcpy(&rid, exc_rid + (size_t)i * rib, (size_t)rib);
        if (rid == r) { ref = exc_ref[i]; break; }
      }
      if (ref >= d->dm->count) { *is_null = 1; *out = 0; return 0; }
      uint64_t v = 0;
      memcpy(&v, d->dict_pay + ref * d->dm->data_size, d->dm->data_size);
      if (sc == OBX_SC_INT) v = obx_sign_extend(v, tss, 1);
      *out = (int64_t)v;
      return 0;
    }
    case OBX_COL_STRING_PREFIX: {
      if (col_dec_is_null(d, h, r)) { *is_null = 1; *out = 0; return 0; }
      int n = d->pm->string_size;
      /* prefix lengths from the cumulative end-offset index */
      int use_hex = d->pm->hex_char_cnt > 0;
      /* max suffix for the fixed stride: n - min prefix length */
      uint64_t e0 = 0;
      memcpy(&e0, d->pfx_ends, d->pm->pib);
      uint64_t min_pl = e0, prev = 0;
      for (uint32_t j = 0; j < d->pm->count; j++) {
        uint64_t e2 = 0;
        memcpy(&e2, d->pfx_ends + (size_t)j * d->pm->pib, d->pm->pib);
        if (e2 - prev < min_pl) min_pl = e2 - prev;
        prev = e2;
      }
      int max_suffix = n - (int)min_pl;
      int stride = 1 + (use_hex ? (max_suffix + 1) / 2 : max_suffix);
      const uint8_t *rp = d->data + d->fix_off + (size_t)r * stride;
      uint32_t ref = rp[0] & 0xF;
      if (ref >= d->pm->count) return OBX_INVALID_ARGUMENT;
      uint64_t pstart = 0, pend = 0;
      if (ref > 0)
        memcpy(&pstart, d->pfx_ends + (size_t)(ref - 1) * d->pm->pib,
               d->pm->pib);
      memcpy(&pend, d->pfx_ends + (size_t)ref * d->pm->pib, d->pm->pib);
      int plen = (int)(pend - pstart);
      uint64_t v = 0;
      for (int i = 0; i < plen; i++)
        v |= (uint64_t)d->pfx_data[pstart + i] << (8 * i);
      for (int i = 0; i < n - plen; i++) {
        uint8_t cc;
        if (use_hex) {
          uint8_t nib = (uint8_t)((rp[1 + i / 2] >>
                                   (((i + 1) % 2) * 4)) & 0xF);
          cc = d->str_chars[nib];
        } else {
          cc = rp[1 + i];
        }
        v |= (uint64_t)cc << (8 * (plen + i));
      }
      *out = (int64_t)v;
      return 0;
    }
    case OBX_COL_SUBSTR: {
      for (uint32_t i = 0; i < d->ssm->exc_cnt; i++) {
        uint64_t rid = 0;
        memcpy(&rid, d->exc_rid + (size_t)i * d->ssm->rib,
               (size_t)d->ssm->rib);
        if (rid == r) {
          if ((d->exc_nb[i / 8] >> (i % 8)) & 1) {
            *is_null = 1; *out = 0; return 0;
          }
          uint64_t v = 0;
          memcpy(&v, d->exc_dat + (size_t)i * cs->len, (size_t)cs->len);
          *out = (int64_t)v;
          return 0;
        }
        if (rid > r) break;
      }
      col_dec rd;
      int rc2 = col_dec_init(&rd, h, &d->chp0[d->ssm->ref_col],
                             d->meta_region);
      if (rc2) return rc2;
      int64_t rv = 0; int rnull = 0;
      obx_col_schema rcs; /* the REF column's schema shape for decode */
      rcs.obj_type = d->chp0[d->ssm->ref_col].obj_type;
      rcs.scale = 0; rcs.precision = 0;
      rcs.len = d->ssm->ref_len;
      rc2 = col_dec_row(&rd, h, &rcs, r, &rv, &rnull);
      if (rc2) return rc2;
      if (rnull) { *is_null = 1; *out = 0; return 0; }
      uint64_t mask2 = cs->len >= 8 ? ~0ull : ((1ull << (8 * cs->len)) - 1);
      *out = (int64_t)(((uint64_t)rv >> (8 * d->ssm->start_pos)) & mask2);
      return 0;
    }
    case OBX_COL_EQUAL: {
      /* exception lookup (ascending row_ids), else the ref column's row */
      for (uint32_t i = 0; i < d->em->exc_cnt; i++) {
        uint64_t rid = 0;
        memcpy(&rid, d->exc_rid + (size_t)i * d->em->rib,
               (size_t)d->em->rib);
        if (rid == r) {
          if ((d->exc_nb[i / 8] >> (i % 8)) & 1) {
            *is_null = 1; *out = 0; return 0;
          }
          uint64_t v = 0;
          memcpy(&v, d->exc_dat + (size_t)i * cs->len, (size_t)cs->len);
          if (sc == OBX_SC_INT) v = obx_sign_extend(v, tss, 1);
          else if (sc == OBX_SC_DECIMAL) v = obx_sign_extend(v, cs->len, 1);
          *out = (int64_t)v;
          return 0;
        }
        if (rid > r) break;
      }
      col_dec rd;
      int rc2 = col_dec_init(&rd, h, &d->chp0[d->em->ref_col],
                             d->meta_region);
      if (rc2) return rc2;
      return col_dec_row(&rd, h, cs, r, out, is_null);
    }
    case OBX_COL_HEX_PACKING: {
      if (col_dec_is_null(d, h, r)) { *is_null = 1; *out = 0; return 0; }
      int n = d->hm->string_size;
      const uint8_t *rp = d->data + d->fix_off + (size_t)r * ((n + 1) / 2);
      uint64_t v = 0;
      for (int i = 0; i < n; i++) {
        uint8_t nib = (uint8_t)((rp[i / 2] >> (((i + 1) % 2) * 4)) & 0xF);
        v |= (uint64_t)d->str_chars[nib] << (8 * i);
      }
      *out = (int64_t)v;
      return 0;
    }
    case OBX_COL_STRING_DIFF: {
      if (col_dec_is_null(d, h, r)) { *is_null = 1; *out = 0; return 0; }
      int n = d->sm->string_size;
      int use_hex = d->sm->hex_char_cnt > 0;
      /* diff_len from the descs */
      int diff_len = 0;
      for (int i = 0; i < d->sm->diff_desc_cnt; i++)
        if (d->str_descs[i] & 1) diff_len += d->str_descs[i] >> 1;
      int stride = use_hex ? (diff_len + 1) / 2 : diff_len;
      const uint8_t *rp = d->data + d->fix_off + (size_t)r * stride;
      uint64_t v = 0;
      int pos = 0, cpos = 0, dpos = 0;
      for (int i = 0; i < d->sm->diff_desc_cnt; i++) {
        int cnt = d->str_descs[i] >> 1;
        if (d->str_descs[i] & 1) {
          for (int j = 0; j < cnt; j++, pos++, dpos++) {
            uint8_t cc;
            if (use_hex) {
              uint8_t nib = (uint8_t)((rp[dpos / 2] >>
                                       (((dpos + 1) % 2) * 4)) & 0xF);
              cc = d->str_chars[nib];
            } else {
              cc = rp[dpos];
            }
            v |= (uint64_t)cc << (8 * pos);
          }
        } else {
          for (int j = 0; j < cnt; j++, pos++, cpos++)
            v |= (uint64_t)d->str_common[cpos] << (8 * pos);
        }
      }
      (void)n;
      *out = (int64_t)v;
      return 0;
    }
    case OBX_COL_INTEGER_BASE_DIFF: {
      if (col_dec_is_null(d, h, r)) { *is_null = 1; *out = 0; return 0; }
      uint64_t diff;
      if (d->ch->attr & OBX_COL_ATTR_BIT_PACKING) {
        diff = obx_bs_get(d->data, d->bits_off + (int64_t)r * d->im->length,
                          d->im->length);
      } else {
        diff = 0;
        memcpy(&diff, d->data + d->fix_off + (size_t)r * d->im->length,
               d->im->length);
      }
      /* base already sign-extended at init (ob_integer_base_diff_decoder.h:
         150-158); value = base + diff */
      *out = (int64_t)(d->base + diff);
      return 0;
    }
    default:
      return OBX_NOT_SUPPORTED;
  }
}

int obx_decode_block(const obx_col_schema *cols, uint16_t n_cols,
                     const uint8_t *block, int64_t block_len,
                     const uint16_t *proj_cols, uint16_t n_proj,
                     uint8_t *const *out_cols, uint8_t *const *out_nulls,
                     uint32_t *row_count) {
  /* length/shape guard: header + column headers must fit. The column
     PAYLOADS are trusted only after the data checksum below verifies —
     the reference's checksum-before-decode model (check_payload_checksum,
     ob_micro_block_header.cpp:257-271). */
  if (block_len < (int64_t)sizeof(obx_micro_header))
    return OBX_INVALID_ARGUMENT;
  const obx_micro_header *h = (const obx_micro_header *)block;
  if (h->magic != OBX_MICRO_BLOCK_MAGIC) return OBX_INVALID_ARGUMENT;
  if (h->column_count != n_cols) return OBX_INVALID_ARGUMENT;
  if ((int64_t)h->header_size +
          (int64_t)n_cols * (int64_t)sizeof(obx_col_header) > block_len)
    return OBX_INVALID_ARGUMENT;
  if (h->data_zlength > block_len || h->data_zlength < OBX_MICRO_HEADER_SIZE)
    return OBX_INVALID_ARGUMENT;
  if ((int64_t)obx_crc32c(block + OBX_MICRO_HEADER_SIZE,
                          (int64_t)h->data_zlength - OBX_MICRO_HEADER_SIZE) !=
      h->data_checksum)
    return OBX_PHYSIC_CHECKSUM_ERROR;
  const uint8_t *meta_region = block + h->header_size +
                               (int64_t)n_cols * sizeof(obx_col_header);
  const obx_col_header *chp =
      (const obx_col_header *)(block + h->header_size);
  if (row_count) *row_count = h->row_count;
  for (uint16_t pi = 0; pi < n_proj; pi++) {
    uint16_t c = proj_cols[pi];
    if (c >= n_cols) return OBX_INVALID_ARGUMENT;
    col_dec d;
    int rc = col_dec_init(&d, h, &chp[c], meta_region);
    if (rc) return rc;
    uint8_t *out = out_cols[pi];
    uint8_t *on = out_nulls ? out_nulls[pi] : NULL;
    if (on) memset(on, 0, (h->row_count + 7) / 8);
    const int len = cols[c].len;
    for (uint32_t r = 0; r < h->row_count; r++) {
      int64_t v; int isn;
      rc = col_dec_row(&d, h, &cols[c], r, &v, &isn);
      if (rc) return rc;
      if (isn) {
        if (on) on[r >> 3] |= (uint8_t)(1u << (r & 7));
        memset(out + (size_t)r * len, 0, (size_t)len);
      } else {
        memcpy(out + (size_t)r * len, &v, (size_t)len);
      }
    }
  }
  return OBX_SUCCESS;
}

/* ===================================================================== */
/* white filter (ObWhiteFilterExecutor semantics)                        */
/* ===================================================================== */

/* compare a decoded value against leaf operands.
 * int/decimal: signed 64-bit; char(N<=8): lexicographic byte compare via
 * big-endian reordering (collation binary). */
static inline int64_t char_key(int64_t raw_le, int len) {
  /* map little-endian packed bytes to an order-preserving integer */
  uint64_t v = (uint64_t)raw_le;
  /* bswap brings lexicographic byte order to unsigned integer order */
  uint64_t be = __builtin_bswap64(v) >> (8 * (8 - len));
  return (int64_t)be;
}

/* Black (generic-expression) filter evaluation: the postfix program of
 * obx.h's OBX_BX_* bytecode over the leaf's referenced column values,
 * with SQL three-valued logic — the restatement of
 * ObPhysicalFilterExecutor::filter_batch's decode-then-eval-expr loop
 * (ob_pushdown_filter.cpp:2066) for the engine's bounded expression
 * shapes. Arithmetic wraps mod 2^64 (documented container semantics);
 * x/0 and NULL operands yield NULL; the row passes iff the result is
 * non-NULL and nonzero. Returns 0 on malformed programs. */
int obx__black_eval(const obx_filter_leaf *lf, const int64_t *vals,
                    const int *nulls) {
  int64_t st[8];
  int nu[8];
  int sp = 0;
  for (int p = 0; p < lf->n_bprog; p++) {
    uint8_t op = lf->bprog[p];
    if (op < 0x40) {
      if (op >= lf->n_bcols || sp >= 8) return 0;
      st[sp] = vals[op];
      nu[sp++] = nulls[op];
    } else if (op < 0x50) {
      int k = op & 0x0F;
      if (k >= OBX_BX_MAX_CONST || sp >= 8) return 0;
      st[sp] = lf->bconst[k];
      nu[sp++] = 0;
    } else if (op == 0x54) { /* NEG */
      if (sp < 1) return 0;
      st[sp - 1] = (int64_t)(0 - (uint64_t)st[sp - 1]);
    } else if (op == 0x72) { /* NOT (three-valued) */
      if (sp < 1) return 0;
      if (!nu[sp - 1]) st[sp - 1] = !st[sp - 1];
    } else {
      if (sp < 2) return 0;
      sp--;
      int64_t a = st[sp - 1], b = st[sp];
      int na = nu[sp - 1], nb = nu[sp];
      int rn = na || nb;
      int64_t r = 0;
      switch (op) {
        case 0x50: r = (int64_t)((uint64_t)a + (uint64_t)b); break;
        case 0x51: r = (int64_t)((uint64_t)a - (uint64_t)b); break;
        case 0x52: r = (int64_t)((uint64_t)a * (uint64_t)b); break;
        case 0x53:
          if (b == 0) rn = 1;
          else if (a == INT64_MIN && b == -1) r = a;
          else r = a / b;
          break;
        case 0x55: /* MOD: x % 0 -> NULL; INT64_MIN % -1 == 0 */
          if (b == 0) rn = 1;
          else if (a == INT64_MIN && b == -1) r = 0;
          else r = a % b;
          break;
        case 0x60: r = a < b; break;
        case 0x61: r = a <= b; break;
        case 0x62: r = a > b; break;
        case 0x63: r = a >= b; break;
        case 0x64: r = a == b; break;
        case 0x65: r = a != b; break;
        case 0x70: /* AND: false dominates NULL */
          if ((!na && !a) || (!nb && !b)) { r = 0; rn = 0; }
          else if (rn) r = 0;
          else r = 1;
          break;
        case 0x71: /* OR: true dominates NULL */
          if ((!na && a) || (!nb && b)) { r = 1; rn = 0; }
          else if (rn) r = 0;
          else r = 0;
          break;
        default: return 0;
      }
      st[sp - 1] = r;
      nu[sp - 1] = rn;
    }
  }
  if (sp != 1) return 0;
  return !nu[0] && st[0] != 0;
}

/* stack-discipline validation of a black program */
int obx__bprog_valid(const obx_filter_leaf *lf) {
  if (lf->n_bprog == 0 || lf->n_bprog > OBX_BX_MAX_PROG ||
      lf->n_bcols > OBX_BX_MAX_COLS)
    return 0;
  int sp = 0;
  for (int p = 0; p < lf->n_bprog; p++) {
    uint8_t op = lf->bprog[p];
    if (op < 0x40) {
      if (op >= lf->n_bcols) return 0;
      sp++;
    } else if (op < 0x50) {
      if ((op & 0x0F) >= OBX_BX_MAX_CONST) return 0;
      sp++;
    } else if (op == 0x54 || op == 0x72) {
      if (sp < 1) return 0;
    } else if ((op >= 0x50 && op <= 0x53) || op == 0x55 ||
               (op >= 0x60 && op <= 0x65) || op == 0x70 || op == 0x71) {
      if (sp < 2) return 0;
      sp--;
    } else {
      return 0;
    }
    if (sp > 8) return 0;
  }
  return sp == 1;
}

static inline int leaf_match(const obx_filter_leaf *lf, int64_t v, int is_null,
                             int sc, int len) {
  if (lf->op == OBX_OP_NU) return is_null;
  if (lf->op == OBX_OP_NN) return !is_null;
  if (is_null) return 0; /* NULL never matches a comparison
                            (ob_pushdown_filter white eval) */
  int64_t x = v, lo = lf->lo, hi = lf->hi;
  if (sc == OBX_SC_STRING) {
    x = char_key(v, len);
    lo = char_key(lf->lo, len);
    hi = char_key(lf->hi, len);
  }
  switch (lf->op) {
    case OBX_OP_EQ: return x == lo;
    case OBX_OP_LE: return x <= lo;
    case OBX_OP_LT: return x < lo;
    case OBX_OP_GE: return x >= lo;
    case OBX_OP_GT: return x > lo;
    case OBX_OP_NE: return x != lo;
    case OBX_OP_BT: return x >= lo && x <= hi;
    case OBX_OP_IN: {
      for (int i = 0; i < lf->n_in; i++) {
        int64_t e = lf->in_list[i];
        if (sc == OBX_SC_STRING) e = char_key(e, len);
        if (x == e) return 1;
      }
      return 0;
    }
    default: return 0;
  }
}

/* evaluate the filter's combine program over per-leaf booleans
 * (ObPushdownFilterExecutor::execute AND/OR, ob_pushdown_filter.cpp:1559;
 * n_prog == 0 is the conjunctive default) */
static int combine_leaves(const obx_filter_desc *f, const int *leaf_res) {
  if (f->n_prog == 0) {
    for (int i = 0; i < f->n_leaves; i++)
      if (!leaf_res[i]) return 0;
    return 1;
  }
  int stack[16];
  int sp = 0;
  for (int p = 0; p < f->n_prog; p++) {
    uint8_t t = f->prog[p];
    if (t < f->n_leaves) {
      stack[sp++] = leaf_res[t];
    } else if (t == OBX_TOK_AND && sp >= 2) {
      sp--; stack[sp - 1] = stack[sp - 1] && stack[sp];
    } else if (t == OBX_TOK_OR && sp >= 2) {
      sp--; stack[sp - 1] = stack[sp - 1] || stack[sp];
    } else {
      return 0; /* malformed program: validated by callers */
    }
  }
  return sp == 1 ? stack[0] : 0;
}

int obx__combine_leaves(const obx_filter_desc *f, const int *leaf_res) {
  return combine_leaves(f, leaf_res);
}

/* program validity: operands in range, final stack depth 1 */
int obx__prog_valid(const obx_filter_desc *f) {
  if (f->n_prog == 0) return 1;
  int sp = 0;
  for (int p = 0; p < f->n_prog; p++) {
    uint8_t t = f->prog[p];
    if (t < f->n_leaves) sp++;
    else if ((t == OBX_TOK_AND || t == OBX_TOK_OR) && sp >= 2) sp--;
    else return 0;
    if (sp > 15) return 0;
  }
  return sp == 1;
}

int obx_cpu_filter_block(const obx_col_schema *cols, uint16_t n_cols,
                         const uint8_t *block, int64_t block_len,
                         const obx_filter_desc *filter,
                         uint8_t *result_bits, uint32_t *row_count,
                         uint32_t *popcnt) {
  const obx_micro_header *h = (const obx_micro_header *)block;
  if (h->magic != OBX_MICRO_BLOCK_MAGIC) return OBX_INVALID_ARGUMENT;
  /* read == verify, as decode (the reference checks the block checksum
     before any use, ObMicroBlockReader init / block cache) */
  if ((int64_t)h->header_size +
          (int64_t)n_cols * (int64_t)sizeof(obx_col_header) > block_len)
    return OBX_INVALID_ARGUMENT;
  if (h->data_zlength > block_len || h->data_zlength < OBX_MICRO_HEADER_SIZE)
    return OBX_INVALID_ARGUMENT;
  if ((int64_t)obx_crc32c(block + OBX_MICRO_HEADER_SIZE,
                          (int64_t)h->data_zlength - OBX_MICRO_HEADER_SIZE) !=
      h->data_checksum)
    return OBX_PHYSIC_CHECKSUM_ERROR;
  const uint8_t *meta_region = block + h->header_size +
                               (int64_t)n_cols * sizeof(obx_col_header);
  const obx_col_header *chp =
      (const obx_col_header *)(block + h->header_size);
  uint32_t rows = h->row_count;
  if (row_count) *row_count = rows;
  memset(result_bits, 0, (rows + 7) / 8);

  col_dec dec[8];
  col_dec bdec[8][OBX_BX_MAX_COLS];
  int sc_of[8], len_of[8];
  uint16_t nl = filter ? filter->n_leaves : 0;
  if (nl > 8) return OBX_INVALID_ARGUMENT;
  for (uint16_t i = 0; i < nl; i++) {
    const obx_filter_leaf *lf = &filter->leaves[i];
    if (lf->op == OBX_OP_BLACK) {
      if (!obx__bprog_valid(lf)) return OBX_INVALID_ARGUMENT;
      for (int j = 0; j < lf->n_bcols; j++) {
        uint16_t c = lf->bcols[j];
        if (c >= n_cols) return OBX_INVALID_ARGUMENT;
        int rc = col_dec_init(&bdec[i][j], h, &chp[c], meta_region);
        if (rc) return rc;
      }
      sc_of[i] = 0;
      len_of[i] = 8;
      continue;
    }
    uint16_t c = lf->col;
    if (c >= n_cols) return OBX_INVALID_ARGUMENT;
    int rc = col_dec_init(&dec[i], h, &chp[c], meta_region);
    if (rc) return rc;
    sc_of[i] = obx_store_class(cols[c].obj_type);
    len_of[i] = cols[c].len;
  }
  if (filter && !obx__prog_valid(filter)) return OBX_INVALID_ARGUMENT;
  uint32_t pc = 0;
  for (uint32_t r = 0; r < rows; r++) {
    int pass = 1;
    if (filter && filter->n_prog == 0) {
      for (uint16_t i = 0; i < nl && pass; i++) {
        const obx_filter_leaf *lf = &filter->leaves[i];
        if (lf->op == OBX_OP_BLACK) {
          int64_t bvv[OBX_BX_MAX_COLS]; int bnn[OBX_BX_MAX_COLS];
          for (int j = 0; j < lf->n_bcols; j++)
            if (col_dec_row(&bdec[i][j], h, &cols[lf->bcols[j]], r,
                            &bvv[j], &bnn[j]))
              return OBX_INTERNAL_ERROR;
          pass = obx__black_eval(lf, bvv, bnn);
          continue;
        }
        int64_t v; int isn;
        if (col_dec_row(&dec[i], h, &cols[lf->col], r, &v, &isn))
          return OBX_INTERNAL_ERROR;
        pass = leaf_match(lf, v, isn, sc_of[i], len_of[i]);
      }
    } else if (filter && nl > 0) {
      int leaf_res[8];
      for (uint16_t i = 0; i < nl; i++) {
        const obx_filter_leaf *lf = &filter->leaves[i];
        if (lf->op == OBX_OP_BLACK) {
          int64_t bvv[OBX_BX_MAX_COLS]; int bnn[OBX_BX_MAX_COLS];
          for (int j = 0; j < lf->n_bcols; j++)
            if (col_dec_row(&bdec[i][j], h, &cols[lf->bcols[j]], r,
                            &bvv[j], &bnn[j]))
              return OBX_INTERNAL_ERROR;
          leaf_res[i] = obx__black_eval(lf, bvv, bnn);
          continue;
        }
        int64_t v; int isn;
        if (col_dec_row(&dec[i], h, &cols[lf->col], r, &v, &isn))
          return OBX_INTERNAL_ERROR;
        leaf_res[i] = leaf_match(lf, v, isn, sc_of[i], len_of[i]);
      }
      pass = combine_leaves(filter, leaf_res);
    }
    if (pass) { result_bits[r >> 3] |= (uint8_t)(1u << (r & 7)); pc++; }
  }
  if (popcnt) *popcnt = pc;
  return OBX_SUCCESS;
}

/* internal: expose col_dec to obx_agg.c */
int obx__col_dec_init(void *d, const void *h, const void *ch,
                      const uint8_t *meta_region) {
  return col_dec_init((col_dec *)d, (const obx_micro_header *)h,
                      (const obx_col_header *)ch, meta_region);
}
int obx__col_dec_row(const void *d, const void *h, const obx_col_schema *cs,
                     uint32_t r, int64_t *out, int *is_null) {
  return col_dec_row((const col_dec *)d, (const obx_micro_header *)h, cs, r,
                     out, is_null);
}
int obx__leaf_match(const obx_filter_leaf *lf, int64_t v, int is_null, int sc,
                    int len) {
  return leaf_match(lf, v, is_null, sc, len);
}
size_t obx__col_dec_size(void) { return sizeof(col_dec); }
