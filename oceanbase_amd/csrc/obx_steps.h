/*
 * obx_steps.h — the steps the precompiled scan kernels are assembled from
 * (obx_kernels.hip, obx_join.hip): the filter window, grouping, aggregate
 * operands and terms, the LDS and global sinks, the global group table, the
 * LDS group table of the fused bodies (start state, the aggregate passes of
 * a row window, the flush) and the growth-path body. Each step exists once;
 * the kernel files hold only the assemblies, and obx_join.hip the one step
 * that is the join's own. Like obx_blk.h, not part of the hipRTC compile
 * input.
 */
#ifndef OBX_STEPS_H
#define OBX_STEPS_H
#include "obx_blk.h"
#include "obx_grouphash.h"

struct prog_spec { uint8_t n; uint8_t t[15]; };

/* cold path: evaluate a combine-program filter for one row window.
 * __noinline__ + by-value args keep its registers off the hot AND path
 * (called once per block window only when the plan has a program). */
__device__ __forceinline__ void filter_prog_phase(
    const blk_view bv, const dev_block &cur,
    const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bl, uint32_t n_leaves, prog_spec ps,
    uint32_t rows, uint32_t w0, uint64_t blk_bit, lds3_u64 *pass_bm,
    lds3_u64 *leaf_bm_flat) {
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63;
  const uint32_t wv = tid >> 6;
  const uint32_t iters = (rows + WG - 1) / WG;
  uint8_t cls[8];
  for (uint32_t i = 0; i < n_leaves; i++) {
    cls[i] = leaf_class(cur, plan_leaves[i], bl[i]);
    if (cls[i] != 2) continue;
    leaf_ctx lc = make_leaf_ctx(cur, plan_leaves[i], bl[i], blk_bit);
    const bool slow = lc.slow;
    for (uint32_t it = 0; it < iters; it++) {
      uint32_t rr = it * WG + tid;
      uint32_t r = w0 + rr;
      bool pass = rr < rows;
      if (pass)
        pass = slow ? leaf_match(bv, cur, plan_leaves[i], bl[i], r)
                    : leaf_ctx_match(bv, lc, plan_leaves[i], r);
      uint64_t m = __ballot(pass);
      if (lane == 0)
        leaf_bm_flat[i * (OBX_MAX_BLOCK_ROWS / 64) + it * WAVES + wv] = m;
    }
  }
  __syncthreads();
  for (uint32_t it = 0; it < iters; it++) {
    uint32_t rr = it * WG + tid;
    uint64_t vm = __ballot(rr < rows);
    if (lane == 0) {
      uint64_t stack[8];
      int sp = 0;
      for (uint32_t p = 0; p < ps.n; p++) {
        uint8_t t = ps.t[p];
        if (t < n_leaves) {
          stack[sp++] =
              cls[t] == 2
                  ? leaf_bm_flat[t * (OBX_MAX_BLOCK_ROWS / 64) +
                                 it * WAVES + wv]
                  : cls[t] == 1 ? vm : 0;
        } else if (t == 128) {
          sp--; stack[sp - 1] &= stack[sp];
        } else {
          sp--; stack[sp - 1] |= stack[sp];
        }
      }
      pass_bm[it * WAVES + wv] = stack[0] & vm;
    }
  }
  __syncthreads();
}

/* every in-range row of the window passes */
__device__ __forceinline__ void pass_all(uint64_t *pass_bm, uint32_t rows) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t iters = (rows + WG - 1) / WG;
  for (uint32_t it = 0; it < iters; it++) {
    uint32_t rr = it * WG + tid;
    uint64_t m = __ballot(rr < rows);
    if (lane == 0) pass_bm[it * WAVES + wv] = m;
  }
}

/* ---- phase 1 of both scan bodies: filter one row window [w0, w0 + rows)
   into the LDS pass bitmap, one leaf at a time (the reference's per-leaf
   bitmap combine, ob_pushdown_filter.cpp:1559; a single live leaf context
   keeps uniform state inside the SGPR budget). AND-only plans fold
   progressively; plans with a combine program evaluate per-leaf bitmaps
   (leaf_bm) then a word-wise postfix pass. blk_verdict is the block's
   fold_prog3 class: 1 = every row passes. ---- */
template <bool PROG>
__device__ __forceinline__ void filter_window(
    const blk_view &bv, const dev_block &cur,
    const dev_leaf *__restrict__ plan_leaves, const blk_leaf *bl,
    const dev_plan_hdr &ph, uint8_t blk_verdict, uint64_t blk_bit,
    uint32_t rows, uint32_t w0, uint64_t *pass_bm, uint64_t *leaf_bm) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t iters = (rows + WG - 1) / WG;
  if (blk_verdict == 1) {
    pass_all(pass_bm, rows);
  } else if constexpr (!PROG) {
    bool first = true;
    for (uint32_t i = 0; i < ph.n_leaves; i++) {
      const blk_leaf lfb = bl[i];
      if (lfb.mode == OBX_LEAF_ALL &&
          !(cur.cols[plan_leaves[i].col].flags & OBX_DF_HAS_EXT))
        continue; /* every row passes this leaf */
      leaf_ctx lc = make_leaf_ctx(cur, plan_leaves[i], bl[i], blk_bit);
      const bool slow = lc.slow;
      for (uint32_t it = 0; it < iters; it++) {
        uint64_t prev = first ? ~0ull : pass_bm[it * WAVES + wv];
        if (!prev) { if (first && lane == 0) pass_bm[it * WAVES + wv] = 0;
                     continue; }
        uint32_t rr = it * WG + tid;
        uint32_t r = w0 + rr;
        bool pass = rr < rows && ((prev >> lane) & 1);
        if (pass)
          pass = slow ? leaf_match(bv, cur, plan_leaves[i], bl[i], r)
                      : leaf_ctx_match(bv, lc, plan_leaves[i], r);
        uint64_t m = __ballot(pass);
        if (lane == 0) pass_bm[it * WAVES + wv] = m;
      }
      first = false;
    }
    if (first) pass_all(pass_bm, rows); /* no live leaves */
  } else {
    prog_spec ps;
    ps.n = ph.n_prog;
    for (int p = 0; p < 15; p++) ps.t[p] = ph.prog[p];
    filter_prog_phase(bv, cur, plan_leaves, bl, ph.n_leaves, ps, rows, w0,
                      blk_bit, (lds3_u64 *)pass_bm, (lds3_u64 *)leaf_bm);
  }
}

/* ---- grouping: a surviving row -> its slot in a group table.
   Fast path (the reference's storage group-by pushdown design,
   ob_pushdown_aggregate_vec.h:445 / read_reference): when every group
   column is dict-encoded and the ref product is small, rows map to cells
   by packed REFS alone; cell -> slot resolves lazily, once per block, via
   the dict values (cell_slot, 254 = not resolved yet). NULL group values
   set flag bits in the top key byte (data bytes stay zero). ---- */
struct group_ctx {
  col_ctx g0, g1;
  const dev_col *gd0, *gd1;
  uint32_t dim0;
  bool ref_fast;
};

__device__ __forceinline__ group_ctx group_open(const dev_plan_hdr &ph,
                                                const dev_block &cur,
                                                uint64_t blk_bit) {
  group_ctx g;
  g.gd0 = g.gd1 = nullptr;
  if (ph.n_group_cols > 0) {
    g.gd0 = &cur.cols[ph.need_cols[ph.group_idx[0]]];
    g.g0 = make_col_ctx(*g.gd0, blk_bit);
  }
  if (ph.n_group_cols > 1) {
    g.gd1 = &cur.cols[ph.need_cols[ph.group_idx[1]]];
    g.g1 = make_col_ctx(*g.gd1, blk_bit);
  }
  g.dim0 = (ph.n_group_cols > 0) ? g.g0.count + 1 : 1;
  const uint32_t dim1 = (ph.n_group_cols > 1) ? g.g1.count + 1 : 1;
  g.ref_fast = ph.n_group_cols > 0 && g.g0.kind == 1 &&
               (ph.n_group_cols < 2 || g.g1.kind == 1) &&
               g.dim0 * dim1 <= 64;
  return g;
}

/* Slot of surviving row r, 255 = none. find(key) is the table's
   find-or-insert (a slot, or < 0 when full; slots past 254 do not fit the
   u8 map either): a row without a slot counts into counters[1]. count(slot)
   takes the row into the slot's row count. */
template <class FIND, class COUNT>
__device__ __forceinline__ uint8_t group_row(
    const blk_view &bv, const dev_plan_hdr &ph, const group_ctx &g,
    uint8_t *cell_slot, uint32_t r, unsigned long long *counters, FIND find,
    COUNT count) {
  uint32_t cell = 0;
  uint8_t cs = 254;
  if (g.ref_fast) {
    cell = (uint32_t)bit_read_at(
        bv.base, bv.rbase_bit + g.g0.data_bit + (uint64_t)r * g.g0.W, g.g0.W);
    if (cell > g.g0.count) cell = g.g0.count; /* nope -> null bucket */
    if (ph.n_group_cols > 1) {
      uint32_t ref1 = (uint32_t)bit_read_at(
          bv.base, bv.rbase_bit + g.g1.data_bit + (uint64_t)r * g.g1.W,
          g.g1.W);
      if (ref1 > g.g1.count) ref1 = g.g1.count;
      cell += ref1 * g.dim0;
    }
    cs = cell_slot[cell];
  }
  if (cs == 254) {
    int s = find(build_group_key(bv, ph.n_group_cols, g.gd0, g.gd1,
                                 ph.group_len[0], ph.group_len[1], r));
    cs = (s < 0 || s >= 255) ? 255 : (uint8_t)s;
    if (cs == 255) atomicAdd(&counters[1], 1ull);
    if (g.ref_fast) cell_slot[cell] = cs;
  }
  if (cs != 255) count(cs);
  return cs;
}

/* ---- aggregates: one row's contribution to one aggregate (or to a
   SUM_PROD2 and the SUM_PROD3 fused with it, obx_fuse_p3). ---- */
struct agg_opnd {
  col_ctx cx;
  const dev_col *dc; /* nullptr: the aggregate has no such operand */
};

__device__ __forceinline__ agg_opnd opnd_open(const dev_plan_hdr &ph,
                                              const dev_block &cur,
                                              uint8_t idx, uint64_t blk_bit) {
  agg_opnd o;
  o.dc = nullptr;
  if (idx != 0xFF) {
    o.dc = &cur.cols[ph.need_cols[idx]];
    o.cx = make_col_ctx(*o.dc, blk_bit);
  }
  return o;
}

/* ctx fast path, or the full decoder for a slow encoding */
__device__ __forceinline__ int64_t opnd_value(const blk_view &bv,
                                              const dev_block &cur,
                                              const agg_opnd &o, uint32_t r,
                                              bool &isn) {
  return (o.cx.kind == 4) ? col_value2(bv, cur, *o.dc, r, isn)
                          : ctx_value(bv, o.cx, r, isn);
}

/* where a term goes: a lane stripe of an LDS cell (c1: the fused mate's),
   or a 256-bit cell of the global table (the mate's is the next one) */
struct lds_sink {
  unsigned long long *c0, *c1;
  __device__ __forceinline__ void count() const { atomicAdd(&c0[0], 1ull); }
  __device__ __forceinline__ void add(i128v v) const { lds_acc_i128(c0, v); }
  __device__ __forceinline__ void add_mate(i128v v) const {
    lds_acc_i128(c1, v);
  }
  __device__ __forceinline__ void minmax(int64_t v, bool is_min) const {
    cas_minmax(&c0[0], v, is_min);
    c0[1] = 1;
  }
};

struct gcell_sink {
  unsigned long long *c0;
  __device__ __forceinline__ void count() const { g_acc_i128(c0, 1ull, 0ull); }
  __device__ __forceinline__ void add(i128v v) const {
    g_acc_i128(c0, v.lo, v.hi);
  }
  __device__ __forceinline__ void add_mate(i128v v) const {
    g_acc_i128(c0 + 4, v.lo, v.hi);
  }
  __device__ __forceinline__ void minmax(int64_t v, bool is_min) const {
    cas_minmax(&c0[0], v, is_min);
    c0[1] = 1;
  }
};

/* the term of kind `kind` and its null rule: a NULL operand drops the term
   (a NULL c drops only the PROD3 half of a fused pair) */
template <class SINK>
__device__ __forceinline__ void agg_term(uint32_t kind, bool fuse_p3,
                                         int64_t one_b, int64_t one_c,
                                         int64_t va, bool na, int64_t vb,
                                         bool nb, int64_t vc, bool nc,
                                         const SINK sink) {
  switch (kind) {
    case 0: /* COUNT(col) */
      if (!na) sink.count();
      break;
    case 1: /* SUM */
      if (!na) sink.add(i128_from_i64(va));
      break;
    case 2: case 3: /* MIN / MAX */
      if (!na) sink.minmax(va, kind == 2);
      break;
    case 4: /* SUM_PROD2 (+ fused PROD3 mate) */
      if (!na && !nb) {
        i128v p2 = i128_mul_i64(va, one_b - vb);
        sink.add(p2);
        if (fuse_p3 && !nc) sink.add_mate(i128_mul_pos_i64(p2, one_c + vc));
      }
      break;
    case 5: /* SUM_PROD3 standalone */
      if (!na && !nb && !nc)
        sink.add(i128_mul_pos_i64(i128_mul_i64(va, one_b - vb), one_c + vc));
      break;
    case 6: /* SUM_MUL */
      if (!na && !nb) sink.add(i128_mul_i64(va, vb));
      break;
    default: break;
  }
}

/* fetch the operands the kind reads, then its term. ag2 is the fused mate
   (ag itself when not fused). */
template <class SINK>
__device__ __forceinline__ void agg_row(
    const blk_view &bv, const dev_block &cur, uint32_t kind, bool fuse_p3,
    const dev_agg &ag, const dev_agg &ag2, const agg_opnd &oa,
    const agg_opnd &ob, const agg_opnd &oc, uint32_t r, const SINK sink) {
  bool na = false, nb = false, nc = false;
  int64_t va = 0, vb = 0, vc = 0;
  if (oa.dc) va = opnd_value(bv, cur, oa, r, na);
  if (kind >= 4 && ob.dc) vb = opnd_value(bv, cur, ob, r, nb);
  if ((kind == 5 || fuse_p3) && oc.dc) vc = opnd_value(bv, cur, oc, r, nc);
  agg_term(kind, fuse_p3, ag.one_b, ag2.one_c, va, na, vb, nb, vc, nc, sink);
}

/* merge the NST lane stripes of one aggregate's LDS cell into its global
   cell: min/max per stripe that saw a value, sums as one 256-bit add */
template <uint32_t NST>
__device__ __forceinline__ void flush_cells(
    const unsigned long long (*st)[2], uint8_t kind,
    unsigned long long *gcell) {
  if (kind == 2 || kind == 3) {
    for (uint32_t s = 0; s < NST; s++) {
      if (st[s][1]) {
        cas_minmax(&gcell[0], (int64_t)st[s][0], kind == 2);
        gcell[1] = 1;
      }
    }
  } else {
    uint64_t lo = 0, hi = 0;
    for (uint32_t s = 0; s < NST; s++) {
      uint64_t l = st[s][0];
      uint64_t nlo = lo + l;
      hi += st[s][1] + (nlo < l);
      lo = nlo;
    }
    if (lo | hi) g_acc_i128(gcell, lo, hi);
  }
}

/* ---- global group table (open addressing over 1 << SHIFT gslots) ---- */
template <uint32_t SHIFT>
__device__ __forceinline__ uint32_t gtable_home(uint64_t key) {
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - SHIFT)) &
         ((1u << SHIFT) - 1);
}

/* find-or-insert a key; returns its slot, or -1 when the table is full */
template <uint32_t SHIFT>
__device__ __forceinline__ int gtable_slot(gslot *gt, uint64_t key) {
  uint32_t idx = gtable_home<SHIFT>(key);
  for (uint32_t probe = 0; probe < (1u << SHIFT); probe++) {
    unsigned long long k = __hip_atomic_load(
        &gt[idx].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == key) return (int)idx;
    if (k == OBX_KEY_EMPTY) {
      unsigned long long c = atomicCAS(&gt[idx].key, OBX_KEY_EMPTY,
                                       (unsigned long long)key);
      if (c == OBX_KEY_EMPTY || c == key) return (int)idx;
    }
    idx = (idx + 1) & ((1u << SHIFT) - 1);
  }
  return -1;
}

/* compile-time tag: hands a constant to a generic lambda */
template <int V> struct kc { static constexpr int v = V; };

/* ---- the per-workgroup LDS group table of the fused scan bodies
   (scan_filter_agg_body, join_scan_body): its start state, the aggregate
   passes of one row window, its flush. kind_of(a) is what cell a holds: the
   plan's kind, or dev_join's where the join step owns cells. ---- */

/* the low word a cell of a kind starts from (the high word starts at 0) */
__device__ __forceinline__ unsigned long long cell_init(uint8_t kind) {
  return (kind == 2)   ? (unsigned long long)INT64_MAX  /* MIN */
         : (kind == 3) ? (unsigned long long)INT64_MIN  /* MAX */
                       : 0ull;
}

template <class KIND_OF>
__device__ __forceinline__ void lds_table_init(lds_table *tab,
                                               uint32_t n_aggs,
                                               KIND_OF kind_of) {
  for (uint32_t s = threadIdx.x; s < OBX_LTABLE_SLOTS; s += WG) {
    tab->key[s] = OBX_KEY_EMPTY;
    for (uint32_t st = 0; st < OBX_STRIPES; st++) {
      tab->count[s][st] = 0;
      for (uint32_t a = 0; a < n_aggs; a++) {
        tab->cell[s][a][st][0] = cell_init(kind_of(a));
        tab->cell[s][a][st][1] = 0;
      }
    }
  }
}

/* phase 3 of both bodies: one pass per aggregate of the plan over the row
   window [w0, w0 + rows), reading the pass bitmap and the row -> slot map
   the earlier phases left (operand ctxs live one at a time). The kind is a
   constant of each rows_of instantiation, so its switch stays OUT of the row
   loop (measured); COUNT(*) needs no pass (filled from the row count at
   flush; a cell the join step owns is COUNT(*) in the plan); PROD2+PROD3
   with shared inputs run as one fused pass. */
__device__ __forceinline__ void agg_passes(
    const blk_view &bv, const dev_block &cur, const dev_plan_hdr &ph,
    uint64_t blk_bit, uint32_t rows, uint32_t w0, const uint64_t *pass_bm,
    const uint8_t *row_slot, lds_table *tab) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t stripe = lane & (OBX_STRIPES - 1);
  const uint32_t iters = (rows + WG - 1) / WG;
  for (uint32_t a = 0; a < ph.n_aggs; a++) {
    const dev_agg ag = ph.aggs[a];
    if (ag.kind == 0 && ag.ia == 0xFF) continue; /* COUNT(*) at flush */
    const bool fuse_p3 = obx_fuse_p3(ph.aggs, ph.n_aggs, a);
    const dev_agg ag2 = fuse_p3 ? ph.aggs[a + 1] : ag;
    const agg_opnd oa = opnd_open(ph, cur, ag.ia, blk_bit);
    const agg_opnd ob = opnd_open(ph, cur, ag.ib, blk_bit);
    const agg_opnd oc = opnd_open(ph, cur, ag2.ic, blk_bit);
    auto rows_of = [&](auto kind, auto fuse) {
      for (uint32_t it = 0; it < iters; it++) {
        uint32_t rr = it * WG + tid;
        uint64_t m = pass_bm[it * WAVES + wv];
        if (!m) continue;
        bool pass = (m >> lane) & 1;
        uint8_t slot8 = pass && rr < rows ? row_slot[rr] : 255;
        if (slot8 == 255) continue;
        agg_row(bv, cur, kind.v, fuse.v != 0, ag, ag2, oa, ob, oc, w0 + rr,
                lds_sink{tab->cell[slot8][a][stripe],
                         fuse.v ? tab->cell[slot8][a + 1][stripe] : nullptr});
      }
    };
    switch (ag.kind) {
      case 0: rows_of(kc<0>{}, kc<0>{}); break; /* COUNT(col) */
      case 1: rows_of(kc<1>{}, kc<0>{}); break; /* SUM */
      case 2: rows_of(kc<2>{}, kc<0>{}); break; /* MIN */
      case 3: rows_of(kc<3>{}, kc<0>{}); break; /* MAX */
      case 4: /* SUM_PROD2, optionally with its PROD3 mate */
        if (fuse_p3) rows_of(kc<4>{}, kc<1>{});
        else rows_of(kc<4>{}, kc<0>{});
        break;
      case 5: rows_of(kc<5>{}, kc<0>{}); break; /* SUM_PROD3 alone */
      case 6: rows_of(kc<6>{}, kc<0>{}); break; /* SUM_MUL */
      default: break;
    }
    if (fuse_p3) a++; /* consumed the PROD3 mate */
  }
}

/* the end of both bodies: the workgroup's passed rows into counters[0], then
   every live slot of the LDS table into the global table (lane stripes
   merged). A slot without a place in a full global table (more than
   OBX_GTABLE_SLOTS distinct groups, no workgroup past its LDS table) writes
   nothing: its rows count into counters[1] as an LDS overflow does, and the
   host takes the growth path. A COUNT(*) cell is the slot's row count:
   kind_of(a) == 0 with no operand in the plan decides that for both
   callers, since the host rewrites COUNT(payload) to COUNT(*) and never
   marks it in own_mask, while a cell of own_mask holds no operand in the
   plan but has its own kind in kind_of. */
template <class KIND_OF>
__device__ __forceinline__ void lds_table_flush(
    const lds_table *tab, const unsigned long long *wg_passed,
    const dev_plan_hdr &ph, KIND_OF kind_of, gslot *__restrict__ gtable,
    unsigned long long *__restrict__ counters) {
  if (threadIdx.x == 0 && *wg_passed) atomicAdd(&counters[0], *wg_passed);
  for (uint32_t s = threadIdx.x; s < OBX_LTABLE_SLOTS; s += WG) {
    uint64_t key = tab->key[s];
    if (key == OBX_KEY_EMPTY) continue;
    unsigned long long cnt = 0;
    for (uint32_t st = 0; st < OBX_STRIPES; st++) cnt += tab->count[s][st];
    const int gi = gtable_slot<OBX_GTABLE_SHIFT>(gtable, key);
    if (gi < 0) {
      atomicAdd(&counters[1], cnt);
      continue;
    }
    const uint32_t idx = (uint32_t)gi;
    atomicAdd(&gtable[idx].count, cnt);
    for (uint32_t a = 0; a < ph.n_aggs; a++) {
      const uint8_t kind = kind_of(a);
      if (kind == 0 && ph.aggs[a].ia == 0xFF) /* COUNT(*): the row count */
        g_acc_i128(gtable[idx].cells[a], cnt, 0);
      else
        flush_cells<OBX_STRIPES>(tab->cell[s][a], kind, gtable[idx].cells[a]);
    }
  }
}

/* ---- the growth path: one body for k_scan_agg_direct and
   k_scan_join_agg_direct (the OBX_GTABLE_BIG table) and for k_scan_agg_hash
   and k_scan_join_agg_hash (the sized table). No LDS table: every surviving
   row resolves its key in the global table (a full table is surfaced as
   counters[2]) and accumulates with global atomics, each aggregate on its own (no
   PROD2+PROD3 fusing); the survivor count goes to the striped counters
   8..15. AND-combined leaves only. `join` is what a join adds between the
   filter and the table:
     admit(bv, cur, ph, r, pv)  does row r take part (probe hit)? sets pv
     key(rk, pv)                the group key from the real columns' key rk
     own(a, pv, sink)           true when cell a is the join's: its term
                                goes to sink
   no_join is the plain scan's: every row, the key as built, no cell. ---- */
struct no_join {
  __device__ __forceinline__ bool admit(const blk_view &, const dev_block &,
                                        const dev_plan_hdr &, uint32_t,
                                        uint64_t &) const { return true; }
  __device__ __forceinline__ uint64_t key(uint64_t rk, uint64_t) const {
    return rk;
  }
  template <class SINK>
  __device__ __forceinline__ bool own(uint32_t, uint64_t, const SINK) const {
    return false;
  }
};

/* `table` is where the groups live, the second small policy:
     COUNTED                    the table counts its CAS winners and the scan
                                stops once they pass the grant
     find(key, won)             find-or-insert: the slot, or < 0 when full
     count(slot)                the slot's row count word
     cell(slot, a)              aggregate a's 256-bit cell (gcell_sink)
     stop(counters, lane)       wave-uniform: start no further block
     won(counters, w, ...)      take this iteration's winners into the count
     FOLD                       adjacent lanes with one key fold their rows
                                into the first of them before the table is
                                touched (wave_run, below)
   gslot_table is the OBX_GTABLE_BIG table of gslots: full means every slot
   holds another key, nothing is counted, nothing stops the scan. */
struct gslot_table {
  static constexpr bool COUNTED = false;
  static constexpr bool FOLD = false;
  gslot *gt;
  __device__ __forceinline__ int64_t find(uint64_t key, bool &) const {
    return gtable_slot<OBX_GTABLE_BIG_SHIFT>(gt, key);
  }
  __device__ __forceinline__ unsigned long long *count(int64_t s) const {
    return &gt[s].count;
  }
  __device__ __forceinline__ unsigned long long *cell(int64_t s,
                                                      uint32_t a) const {
    return gt[s].cells[a];
  }
  __device__ __forceinline__ bool stop(const unsigned long long *,
                                       uint32_t) const { return false; }
  __device__ __forceinline__ void won(unsigned long long *, bool, uint32_t,
                                      uint32_t) const {}
};

/* the sized table (obx_grouphash.h) behind a grant of max_groups. Winners
   are counted per wave: a ballot over the lanes still in this iteration, one
   add of its popcount by the first winner lane into one of 8 striped words,
   and only when the iteration had a winner. stop() reads those 8 words (one
   64-byte line) and counters[2] at agent scope. */
struct sized_table {
  static constexpr bool COUNTED = true;
  /* measured, profiles/r11_group_hash.md: 13-42 % off the kernel on keys
     clustered in runs of 4, nothing beyond spread on random keys */
  static constexpr bool FOLD = true;
  obx_gh_dev v;
  uint64_t max_groups;
  __device__ __forceinline__ int64_t find(uint64_t key, bool &w) const {
    uint64_t steps;
    return obx_gh_find_or_insert(v, key, &w, &steps);
  }
  __device__ __forceinline__ unsigned long long *count(int64_t s) const {
    return obx_gh_count(v, (uint64_t)s);
  }
  __device__ __forceinline__ unsigned long long *cell(int64_t s,
                                                      uint32_t a) const {
    return obx_gh_cell(v, (uint64_t)s, a);
  }
  __device__ __forceinline__ bool stop(unsigned long long *counters,
                                       uint32_t lane) const {
    unsigned long long w = 0;
    if (lane < 8)
      w = __hip_atomic_load(&counters[OBX_GH_WINNERS + lane],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (lane == 8)
      w = __hip_atomic_load(&counters[2], __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT)
              ? max_groups + 1 : 0;
    for (int off = 8; off > 0; off >>= 1)
      w += (unsigned long long)__shfl_xor((long long)w, off, 64);
    /* lanes 0..15 now hold the sum of lanes 0..15 */
    w = (unsigned long long)__shfl((long long)w, 0, 64);
    return w > max_groups;
  }
  __device__ __forceinline__ void won(unsigned long long *counters, bool w,
                                      uint32_t lane, uint32_t wave_id) const {
    const uint64_t m = __ballot(w);
    if (w && lane == (uint32_t)__ffsll((unsigned long long)m) - 1)
      atomicAdd(&counters[OBX_GH_WINNERS + (wave_id & 7)],
                (unsigned long long)__popcll(m));
  }
};

/* ---- the wave fold: rows of one key in adjacent lanes (a table clustered
   on the group column, l_orderkey's shape) reach the table as one row. A
   run is a maximal stretch of lanes with equal keys; a lane without a row
   carries OBX_KEY_EMPTY and so never joins a row's run. Its first lane
   leads: it alone finds the slot, adds the run's length to the count and
   applies every aggregate's folded term. All 64 lanes call these. ---- */
struct wave_run {
  bool lead;     /* first lane of a run of rows */
  uint32_t end;  /* one past the run's last lane */
  uint32_t n;    /* lanes in the run, from this one on */
};

__device__ __forceinline__ wave_run wave_run_of(uint64_t key, bool live,
                                                uint32_t lane) {
  const uint64_t prev = (uint64_t)__shfl_up((long long)key, 1, 64);
  const bool head = lane == 0 || prev != key;
  const uint64_t heads = __ballot(head);
  const uint64_t above = lane == 63 ? 0 : heads >> (lane + 1);
  wave_run w;
  w.end = above ? lane + 1 + (uint32_t)__ffsll((unsigned long long)above) - 1
                : 64;
  w.n = w.end - lane;
  w.lead = head && live;
  return w;
}

/* one row's term, held back: what agg_term would have done to a cell */
struct held_term {
  uint64_t lo, hi;
  uint32_t op; /* 0 nothing, 1 add {lo, hi}, 2 MIN of lo, 3 MAX of lo */
};
struct hold_sink {
  held_term *t;
  __device__ __forceinline__ void count() const {
    t->op = 1; t->lo = 1; t->hi = 0;
  }
  __device__ __forceinline__ void add(i128v v) const {
    t->op = 1; t->lo = v.lo; t->hi = v.hi;
  }
  __device__ __forceinline__ void add_mate(i128v) const {}
  __device__ __forceinline__ void minmax(int64_t v, bool is_min) const {
    t->op = is_min ? 2 : 3; t->lo = (uint64_t)v; t->hi = 0;
  }
};

/* fold the run's held terms into its first lane (segmented reduction: a
   lane takes the term `off` lanes up while that lane is inside its run) */
__device__ __forceinline__ void wave_run_fold(held_term &t, const wave_run &w,
                                              uint32_t lane) {
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const uint64_t olo = (uint64_t)__shfl_down((long long)t.lo, off, 64);
    const uint64_t ohi = (uint64_t)__shfl_down((long long)t.hi, off, 64);
    const uint32_t oop = (uint32_t)__shfl_down((int)t.op, off, 64);
    if (lane + off >= w.end || !oop) continue;
    if (!t.op) {
      t.lo = olo; t.hi = ohi; t.op = oop;
    } else if (oop == 1) {
      const uint64_t nlo = t.lo + olo;
      t.hi += ohi + (nlo < olo);
      t.lo = nlo;
    } else if (oop == 2 ? (int64_t)olo < (int64_t)t.lo
                        : (int64_t)olo > (int64_t)t.lo) {
      t.lo = olo;
    }
  }
}

template <class SINK>
__device__ __forceinline__ void held_apply(const held_term &t,
                                           const SINK sink) {
  i128v v; v.lo = t.lo; v.hi = t.hi;
  if (t.op == 1) sink.add(v);
  else if (t.op) sink.minmax((int64_t)t.lo, t.op == 2);
}

template <class JOIN, class TABLE>
__device__ __forceinline__ void scan_direct_body(
    const uint8_t *__restrict__ buf, const dev_block *__restrict__ blocks,
    uint32_t n_blocks, const dev_leaf *__restrict__ plan_leaves,
    const blk_leaf *__restrict__ bleaves, const dev_plan_hdr &ph,
    const TABLE table, unsigned long long *__restrict__ counters,
    const JOIN join) {
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63, wv = tid >> 6;
  unsigned long long lane_cnt = 0;
  for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    if constexpr (TABLE::COUNTED)
      if (table.stop(counters, lane)) break;
    const dev_block &cur = blocks[b];
    const blk_leaf *bl = bleaves + (size_t)b * ph.n_leaves;
    bool skip = false;
    for (uint32_t i = 0; i < ph.n_leaves; i++)
      if (leaf_class(cur, plan_leaves[i], bl[i]) == 0) { skip = true; break; }
    if (skip) continue;
    const blk_view bv = blk_open<false>(buf, cur, nullptr);
    const dev_col *gd0 = nullptr, *gd1 = nullptr;
    if (ph.n_group_cols > 0) gd0 = &cur.cols[ph.need_cols[ph.group_idx[0]]];
    if (ph.n_group_cols > 1) gd1 = &cur.cols[ph.need_cols[ph.group_idx[1]]];
    const uint32_t kl0 = ph.group_len[0], kl1 = ph.group_len[1];
    const uint32_t rows = cur.row_count;
    /* a folding table keeps the wave together to the end of the window:
       rows past the block and rows the filter or the join drops ride along
       as lanes without a row. Otherwise such a lane leaves at once. */
    const uint32_t span = TABLE::FOLD ? (rows + WG - 1) / WG * WG : rows;
    for (uint32_t r = tid; r < span; r += WG) {
      bool live = !TABLE::FOLD || r < rows;
      for (uint32_t i = 0; live && i < ph.n_leaves; i++)
        live = leaf_match(bv, cur, plan_leaves[i], bl[i], r);
      if constexpr (!TABLE::FOLD) { if (!live) continue; }
      uint64_t pv = 0;
      if (live && !join.admit(bv, cur, ph, r, pv)) live = false;
      if constexpr (!TABLE::FOLD) { if (!live) continue; }
      uint64_t key = OBX_KEY_EMPTY;
      if (live) {
        lane_cnt++;
        key = join.key(
            build_group_key(bv, ph.n_group_cols, gd0, gd1, kl0, kl1, r), pv);
      }
      wave_run run = {live, lane + 1, 1};
      if constexpr (TABLE::FOLD) run = wave_run_of(key, live, lane);
      int64_t gi = -1;
      if (run.lead) {
        bool won = false;
        gi = table.find(key, won);
        if constexpr (TABLE::COUNTED)
          table.won(counters, won, lane, blockIdx.x * WAVES + wv);
        if (gi < 0) /* global table full: surfaced as counters[2] */
          atomicAdd(&counters[2], (unsigned long long)run.n);
        else
          atomicAdd(table.count(gi), (unsigned long long)run.n);
      }
      if constexpr (!TABLE::FOLD) { if (gi < 0) continue; }
      for (uint32_t a = 0; a < ph.n_aggs; a++) {
        /* row r's term of aggregate a, into whatever sink takes it */
        auto term_into = [&](auto sink) {
          if (join.own(a, pv, sink)) return;
          const dev_agg ag = ph.aggs[a];
          if (ag.kind == 0 && ag.ia == 0xFF) return; /* COUNT(*): count */
          bool na = false, nb = false, nc = false;
          int64_t va = 0, vb = 0, vc = 0;
          if (ag.ia != 0xFF)
            va = col_value2(bv, cur, cur.cols[ph.need_cols[ag.ia]], r, na);
          if (ag.kind >= 4 && ag.ib != 0xFF)
            vb = col_value2(bv, cur, cur.cols[ph.need_cols[ag.ib]], r, nb);
          if (ag.kind == 5 && ag.ic != 0xFF)
            vc = col_value2(bv, cur, cur.cols[ph.need_cols[ag.ic]], r, nc);
          agg_term(ag.kind, false, ag.one_b, ag.one_c, va, na, vb, nb, vc, nc,
                   sink);
        };
        if constexpr (TABLE::FOLD) {
          held_term t = {0, 0, 0};
          if (live) term_into(hold_sink{&t});
          wave_run_fold(t, run, lane);
          if (run.lead && gi >= 0) held_apply(t, gcell_sink{table.cell(gi, a)});
        } else {
          term_into(gcell_sink{table.cell(gi, a)});
        }
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1)
    lane_cnt += (unsigned long long)__shfl_xor((long long)lane_cnt, off, 64);
  if (lane == 0 && lane_cnt)
    atomicAdd(&counters[8 + ((blockIdx.x * WAVES + wv) & 7)], lane_cnt);
}

#endif /* OBX_STEPS_H */
