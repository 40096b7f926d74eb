/*
 * obx_plan.cpp — the load-time fold of a table's blocks into its facts, and
 * the per-query plan builder that reads them. No HIP header: both run the
 * same in the engine and in the GPU-free probes (obx_probes.cpp).
 */
#include <cstring>

#include "obx_facts.h"

void summarize_col_classes(obx_table_facts &h) {
  const uint32_t nc = h.n_cols;
  const bool first = h.col_class.size() == nc;
  const uint8_t *cls = h.col_class.data() + h.col_class.size() - nc;
  const uint8_t *cnt = h.col_cnt.data() + h.col_cnt.size() - nc;
  for (uint32_t c = 0; c < nc; c++) {
    const uint8_t k = cls[c];
    if (first) h.col_grp16_every[c] = true;
    if ((k & 0xF) == 5) h.col_span_any[c] = true;
    if ((k & 0xF) != 1 || cnt[c] >= 16) h.col_grp16_every[c] = false;
    if ((k & 0xF) > 3 || (k & 0x10)) h.col_slow_any[c] = true;
    if (cnt[c] > h.col_cnt_max[c]) h.col_cnt_max[c] = cnt[c];
  }
}

void obx_fold_block(obx_table_facts &h, const dev_block &db) {
  const bool first = h.col_class.empty();
  if ((db.block_byte & 15) ||
      (uint64_t)db.block_len + 24 > OBX_LDS_STAGE_BYTES ||
      db.row_count > 4096 /* OBX_MAX_BLOCK_ROWS */)
    h.lds_ok = false;
  for (uint16_t c = 0; c < h.n_cols; c++) {
    const dev_col &dc = db.cols[c];
    uint8_t cls;
    switch (dc.enc) {
      case OBX_D_RAW: cls = 0; break;
      case OBX_D_DICT: cls = 1; break;
      case OBX_D_INTDIFF: cls = 2; break;
      case OBX_D_CONST: cls = dc.runs == 0 ? 3 : 4; break;
      case OBX_D_EQUAL: case OBX_D_SUBSTR:
        cls = 5; break; /* span: no device group keys */
      default: cls = 4; break;
    }
    if (dc.flags & OBX_DF_STRING) cls |= 0x10;
    h.col_class.push_back(cls);
    h.col_cnt.push_back((uint8_t)(dc.count > 254 ? 255 : dc.count));
    if (first) {
      h.col_dict_every[c] = true;
      h.col_dict_any[c] = true;
      h.col_raw8_every[c] = true;
      h.col_rangefam_every[c] = true;
    }
    if ((cls & 0xF) != 1 || (cls & 0x10) || dc.count > 63)
      h.col_dict_every[c] = false;
    if ((cls & 0xF) != 1 || dc.count > 63)
      h.col_dict_any[c] = false; /* dict (possibly char) everywhere */
    if (!(dc.enc == OBX_D_RAW && !(dc.flags & OBX_DF_BITPACK) &&
          !(dc.flags & OBX_DF_STRING) && !(dc.flags & OBX_DF_HAS_EXT) &&
          dc.width == 8 && (dc.data_bit & 63) == 0))
      h.col_raw8_every[c] = false;
    if (!((dc.enc == OBX_D_RAW || dc.enc == OBX_D_INTDIFF) &&
          !(dc.flags & OBX_DF_STRING) && !(dc.flags & OBX_DF_HAS_EXT)))
      h.col_rangefam_every[c] = false;
    if (dc.count > h.col_maxcnt[c]) h.col_maxcnt[c] = dc.count;
    if (dc.flags & OBX_DF_HAS_EXT) h.col_ext_any[c] = true;
    uint32_t w = 255; /* no packed stream: blocks multi-row reads */
    if (dc.enc == OBX_D_RAW || dc.enc == OBX_D_DICT || dc.enc == OBX_D_INTDIFF)
      w = (dc.flags & OBX_DF_BITPACK) ? dc.width : (uint32_t)dc.width * 8;
    if (w > h.col_maxw[c]) h.col_maxw[c] = w;
    uint64_t slot = 0;
    if (!obx_bdesc_pack_col(&dc, db.block_byte, &slot))
      h.col_bdesc_unfit[c] = true;
  }
  summarize_col_classes(h);
  if (db.row_count > h.max_block_rows) h.max_block_rows = db.row_count;
  if (db.block_len > h.max_block_len) h.max_block_len = db.block_len;
  h.n_blocks++;
  h.total_rows += db.row_count;
}

/* build plan header + device leaves (pure: no HIP calls). resolve turns the
   set ids of IN_SET leaves into device views; the GPU-free probes pass
   none, and such a leaf is then an unknown id. */
int build_plan(obx_set_resolver resolve, const void *resolve_arg,
               const obx_table_facts &h, const obx_filter_desc *filter,
               const obx_agg_desc *agg, dev_plan_hdr &ph,
               dev_leaf pl[OBX_DEV_MAX_LEAVES]) {
  memset(&ph, 0, sizeof(ph));
  memset(pl, 0, sizeof(dev_leaf) * OBX_DEV_MAX_LEAVES);
  uint16_t nl = filter ? filter->n_leaves : 0;
  if (nl > OBX_DEV_MAX_LEAVES) return OBX_INVALID_ARGUMENT;
  ph.n_leaves = nl;
  if (filter && filter->n_prog) {
    /* validate the combine program (operand range, stack discipline) */
    int sp = 0;
    for (int p = 0; p < filter->n_prog; p++) {
      uint8_t t = filter->prog[p];
      if (t < nl) sp++;
      else if ((t == OBX_TOK_AND || t == OBX_TOK_OR) && sp >= 2) sp--;
      else return OBX_INVALID_ARGUMENT;
      if (sp > 8) return OBX_INVALID_ARGUMENT;
    }
    if (sp != 1) return OBX_INVALID_ARGUMENT;
    ph.n_prog = filter->n_prog;
    memcpy(ph.prog, filter->prog, filter->n_prog);
  }
  for (uint16_t i = 0; i < nl; i++) {
    const obx_filter_leaf *lf = &filter->leaves[i];
    if (lf->col >= h.n_cols) return OBX_INVALID_ARGUMENT;
    if (lf->op > OBX_OP_IN_SET) return OBX_INVALID_ARGUMENT;
    pl[i].col = lf->col;
    pl[i].op = lf->op;
    if (lf->op == OBX_OP_IN_SET) {
      /* the set's device view rides in the leaf's in_list words; keys
         compare as decoded datums, so no char order map */
      const obx_keyset_dev *ks =
          resolve ? resolve(resolve_arg, lf->lo) : nullptr;
      if (!ks) return OBX_INVALID_ARGUMENT;
      obx_keyset_to_leaf(*ks, pl[i].in_list);
      continue;
    }
    pl[i].vlo = lf->lo;
    pl[i].vhi = lf->hi;
    pl[i].n_in = lf->n_in;
    for (int j = 0; j < lf->n_in && j < 8; j++) pl[i].in_list[j] = lf->in_list[j];
    if (lf->op == OBX_OP_BLACK) {
      /* stack-discipline validation mirroring the oracle's
         obx__bprog_valid */
      if (lf->n_bprog == 0 || lf->n_bprog > OBX_BX_MAX_PROG ||
          lf->n_bcols == 0 || lf->n_bcols > OBX_BX_MAX_COLS)
        return OBX_INVALID_ARGUMENT;
      int sp = 0;
      for (int p = 0; p < lf->n_bprog; p++) {
        uint8_t op2 = lf->bprog[p];
        if (op2 < 0x40) {
          if (op2 >= lf->n_bcols) return OBX_INVALID_ARGUMENT;
          sp++;
        } else if (op2 < 0x50) {
          if ((op2 & 0x0F) >= OBX_BX_MAX_CONST) return OBX_INVALID_ARGUMENT;
          sp++;
        } else if (op2 == 0x54 || op2 == 0x72) {
          if (sp < 1) return OBX_INVALID_ARGUMENT;
        } else if ((op2 >= 0x50 && op2 <= 0x53) || op2 == 0x55 ||
                   (op2 >= 0x60 && op2 <= 0x65) || op2 == 0x70 ||
                   op2 == 0x71) {
          if (sp < 2) return OBX_INVALID_ARGUMENT;
          sp--;
        } else {
          return OBX_INVALID_ARGUMENT;
        }
        if (sp > 8) return OBX_INVALID_ARGUMENT;
      }
      if (sp != 1) return OBX_INVALID_ARGUMENT;
      for (int j = 0; j < lf->n_bcols; j++) {
        if (lf->bcols[j] >= h.n_cols) return OBX_INVALID_ARGUMENT;
        pl[i].bcols[j] = lf->bcols[j];
      }
      pl[i].n_bcols = lf->n_bcols;
      pl[i].n_bprog = lf->n_bprog;
      memcpy(pl[i].bprog, lf->bprog, lf->n_bprog);
      memcpy(pl[i].bconst, lf->bconst, sizeof(pl[i].bconst));
      pl[i].col = lf->bcols[0]; /* pruning/lowering anchor */
      continue;
    }
    /* char columns compare byte-lexicographically: order-map the operands
       exactly like the oracle's char_key (low len LE bytes -> BE int) */
    if (obx_store_class(h.cols[lf->col].obj_type) == OBX_SC_STRING) {
      uint32_t len = h.cols[lf->col].len;
      auto ck = [len](int64_t x) -> int64_t {
        return (int64_t)(__builtin_bswap64((uint64_t)x) >> (8 * (8 - len)));
      };
      pl[i].char_len = (uint8_t)len;
      pl[i].vlo = ck(lf->lo);
      pl[i].vhi = ck(lf->hi);
      for (int j = 0; j < lf->n_in && j < 8; j++)
        pl[i].in_list[j] = ck(lf->in_list[j]);
    }
  }
  /* AND-only plans: merge a lower-bound and an upper-bound leaf on the
     same column into one OP_BT leaf (the reference's range-node build,
     ObWhiteFilterExecutor; one pass instead of two in the kernels) */
  if (filter && !filter->n_prog && nl > 1) {
    for (uint16_t i = 0; i < nl; i++) {
      if (pl[i].op != OBX_OP_GE && pl[i].op != OBX_OP_GT) continue;
      for (uint16_t k = 0; k < nl; k++) {
        if (k == i || pl[k].col != pl[i].col) continue;
        if (pl[k].op != OBX_OP_LE && pl[k].op != OBX_OP_LT) continue;
        int64_t lo = pl[i].vlo, hi = pl[k].vlo;
        if (pl[i].op == OBX_OP_GT) {
          if (lo == INT64_MAX) continue;
          lo++;
        }
        if (pl[k].op == OBX_OP_LT) {
          if (hi == INT64_MIN) continue;
          hi--;
        }
        pl[i].op = OBX_OP_BT;
        pl[i].vlo = lo;
        pl[i].vhi = hi;
        /* drop leaf k */
        for (uint16_t m = k; m + 1 < nl; m++) pl[m] = pl[m + 1];
        nl--;
        ph.n_leaves = nl;
        if (k < i) i--;
        i--; /* re-examine the merged leaf (another pair may exist) */
        break;
      }
    }
  }

  /* resolve needed value slots */
  int slot_of_col[64];
  for (int i = 0; i < 64; i++) slot_of_col[i] = -1;
  auto need = [&](uint16_t c) -> uint8_t {
    if (slot_of_col[c] < 0) {
      if (ph.n_need >= OBX_DEV_MAX_NEED) return 0xFF;
      slot_of_col[c] = ph.n_need;
      ph.need_cols[ph.n_need++] = c;
    }
    return (uint8_t)slot_of_col[c];
  };
  if (agg) {
    if (agg->n_group_cols > 2 || agg->n_aggs > OBX_DEV_MAX_AGGS)
      return OBX_INVALID_ARGUMENT;
    ph.n_group_cols = agg->n_group_cols;
    for (int g = 0; g < agg->n_group_cols; g++) {
      if (agg->group_cols[g] >= h.n_cols) return OBX_INVALID_ARGUMENT;
      ph.group_idx[g] = need(agg->group_cols[g]);
      ph.group_len[g] = h.cols[agg->group_cols[g]].len;
    }
    ph.n_aggs = agg->n_aggs;
    for (int a = 0; a < agg->n_aggs; a++) {
      const obx_agg_expr *e = &agg->aggs[a];
      dev_agg *da = &ph.aggs[a];
      da->kind = e->kind;
      da->ia = da->ib = da->ic = 0xFF;
      if (e->col_a != UINT16_MAX && e->col_a >= h.n_cols)
        return OBX_INVALID_ARGUMENT;
      if (e->col_a != UINT16_MAX) da->ia = need(e->col_a);
      if (e->kind == OBX_AGG_SUM_PROD2 || e->kind == OBX_AGG_SUM_PROD3 ||
          e->kind == OBX_AGG_SUM_MUL) {
        if (e->col_b >= h.n_cols) return OBX_INVALID_ARGUMENT;
        da->ib = need(e->col_b);
        static const int64_t P10[19] = {1ll,10ll,100ll,1000ll,10000ll,
          100000ll,1000000ll,10000000ll,100000000ll,1000000000ll,
          10000000000ll,100000000000ll,1000000000000ll,10000000000000ll,
          100000000000000ll,1000000000000000ll,10000000000000000ll,
          100000000000000000ll,1000000000000000000ll};
        da->one_b = P10[h.cols[e->col_b].scale];
        if (e->kind == OBX_AGG_SUM_PROD3) {
          if (e->col_c >= h.n_cols) return OBX_INVALID_ARGUMENT;
          da->ic = need(e->col_c);
          da->one_c = P10[h.cols[e->col_c].scale];
        }
      }
    }
    /* group keys decode via col_value (no block context): COLUMN_EQUAL
       group columns would misdecode — reject them (value/filter columns
       on COLUMN_EQUAL are fully supported via col_value2) */
    for (uint32_t g = 0; g < ph.n_group_cols; g++)
      if (h.col_span_any[ph.need_cols[ph.group_idx[g]]])
        return OBX_NOT_SUPPORTED;
  }
  /* group aggregates into row passes: aggs whose inputs fit in <=3 shared
     decoded columns run together (COUNT(*) needs no pass — filled from the
     group counts at flush) */
  if (agg) {
    bool used[OBX_DEV_MAX_AGGS] = {};
    ph.n_passes = 0;
    for (int a = 0; a < agg->n_aggs; a++) {
      if (used[a]) continue;
      const dev_agg *da = &ph.aggs[a];
      if (da->kind == OBX_AGG_COUNT && da->ia == 0xFF) { used[a] = true; continue; }
      dev_pass *pp = &ph.passes[ph.n_passes++];
      memset(pp, 0, sizeof(*pp));
      auto col_sel = [&](uint8_t need_idx) -> int {
        if (need_idx == 0xFF) return -1;
        for (int k = 0; k < pp->n_cols; k++)
          if (pp->cols[k] == need_idx) return k;
        if (pp->n_cols >= 3) return -2; /* no room */
        pp->cols[pp->n_cols] = need_idx;
        return pp->n_cols++;
      };
      auto try_add = [&](int idx) -> bool {
        const dev_agg *d = &ph.aggs[idx];
        uint8_t save_n = pp->n_cols;
        int sa = col_sel(d->ia), sb = col_sel(d->ib), sc = col_sel(d->ic);
        if (sa == -2 || sb == -2 || sc == -2) { pp->n_cols = save_n; return false; }
        dev_pass_agg *pa = &pp->aggs[pp->n_aggs++];
        pa->kind = d->kind;
        pa->agg_idx = (uint8_t)idx;
        pa->sa = (uint8_t)(sa < 0 ? 0xFF : sa);
        pa->sb = (uint8_t)(sb < 0 ? 0xFF : sb);
        pa->sc = (uint8_t)(sc < 0 ? 0xFF : sc);
        pa->one_b = d->one_b;
        pa->one_c = d->one_c;
        return true;
      };
      try_add(a);
      used[a] = true;
      for (int b2 = a + 1; b2 < agg->n_aggs; b2++) {
        if (used[b2]) continue;
        const dev_agg *d2 = &ph.aggs[b2];
        if (d2->kind == OBX_AGG_COUNT && d2->ia == 0xFF) { used[b2] = true; continue; }
        if (try_add(b2)) used[b2] = true;
      }
    }
  }

  return OBX_SUCCESS;
}
