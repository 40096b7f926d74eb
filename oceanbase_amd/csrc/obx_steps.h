/*
 * obx_steps.h — the steps the precompiled scan kernels are assembled from
 * (obx_kernels.hip, obx_join.hip): the filter window, grouping, aggregate
 * operands and terms, the LDS and global sinks, the flush and the global
 * group table. Each step exists once; the kernel files hold only the
 * assemblies. Like obx_blk.h, not part of the hipRTC compile input.
 */
#ifndef OBX_STEPS_H
#define OBX_STEPS_H
#include "obx_blk.h"

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

#endif /* OBX_STEPS_H */
