/*
 * obx_jit_rt.cpp — the hipRTC half of the JIT: the embedded device headers,
 * the compile cache, and prepare / launch of a generated kernel. The source
 * text, the cache keys and every eligibility decision come from the
 * generators (obx_jit_gen.cpp, through obx_jit.h); jit_launch is the only
 * place of the JIT that touches a device pointer.
 */
#include <hip/hiprtc.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <string>

#include "obx_host.h"
#include "obx_jit.h"

static const char *OBX_JIT_SRC_DEV_H =
#include "obx_embed_dev_h.inc"
    ;
static const char *OBX_JIT_SRC_COMMON_H =
#include "obx_embed_common_h.inc"
    ;
static const char *OBX_JIT_SRC_JIT_DEV_H =
#include "obx_embed_jit_dev_h.inc"
    ;
static const char *OBX_JIT_SRC_KEYSET_H =
#include "obx_embed_keyset_h.inc"
    ;

/* The compile cache: one for the process, on purpose. A context is cheap and
   a hipRTC compile is not, and a process opens many contexts over the same
   plans. A module is loaded on one device, so the device ordinal is part of
   the key; contexts run on their own threads (include/obx.h), so the mutex
   is held across lookup, compile and insert: the second asker of a plan
   waits for the first one's compile and then hits. An entry is complete
   before the lock is dropped and never changes afterwards. Entries outlive
   the context that compiled them and modules are never unloaded: a pointer
   handed out stays good, and the cost is bounded by the plans a process
   runs. jit_get is the only way in. */
static struct {
  std::mutex mu;
  std::map<std::string, jit_entry> entries;
} g_jit;

/* compile (or fetch) a generated kernel for a device, which the caller has
   made current; nullptr on any failure (the caller falls back to the
   precompiled kernels). gen_src() builds the source and runs only on a cache
   miss; failures are cached too, so a plan that does not compile costs one
   attempt. dump_name is the OBX_JIT_DUMP file and the file name in the
   compile log. meta is what the entry says of its kernel besides mod / fn. */
template <class GenSrc>
static const jit_entry *jit_get(int device, const std::string &key,
                                GenSrc &&gen_src, const char *kernel,
                                const char *dump_name, const jit_entry &meta) {
  std::lock_guard<std::mutex> lock(g_jit.mu);
  const auto ins =
      g_jit.entries.emplace("d" + std::to_string(device) + "|" + key, meta);
  jit_entry &ent = ins.first->second; /* fn stays null unless all succeeds */
  if (!ins.second) return ent.fn ? &ent : nullptr;
  const std::string src = gen_src();
  if (const char *dump_dir = getenv("OBX_JIT_DUMP")) {
    FILE *f = fopen((std::string(dump_dir) + "/" + dump_name).c_str(), "w");
    if (!f) f = fopen((std::string("/tmp/") + dump_name).c_str(), "w");
    if (f) { fwrite(src.data(), 1, src.size(), f); fclose(f); }
  }
  hiprtcProgram prog;
  const char *hdrs[4] = {OBX_JIT_SRC_COMMON_H, OBX_JIT_SRC_DEV_H,
                         OBX_JIT_SRC_JIT_DEV_H, OBX_JIT_SRC_KEYSET_H};
  const char *hdr_names[4] = {"obx_dev_common.h", "obx_dev.h",
                              "obx_jit_dev.h", "obx_keyset.h"};
  if (hiprtcCreateProgram(&prog, src.c_str(), dump_name, 4, hdrs,
                          hdr_names) != HIPRTC_SUCCESS)
    return nullptr;
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-DOBX_HIPRTC=1"};
  if (hiprtcCompileProgram(prog, 4, opts) != HIPRTC_SUCCESS) {
    size_t lsz = 0;
    hiprtcGetProgramLogSize(prog, &lsz);
    if (lsz > 1) {
      std::string log(lsz, '\0');
      hiprtcGetProgramLog(prog, &log[0]);
      fprintf(stderr, "obx: JIT compile failed (%s):\n%s\n", kernel,
              log.c_str());
    }
    hiprtcDestroyProgram(&prog);
    return nullptr;
  }
  size_t csz = 0;
  hiprtcGetCodeSize(prog, &csz);
  std::string code(csz, '\0');
  hiprtcGetCode(prog, &code[0]);
  hiprtcDestroyProgram(&prog);
  if (hipModuleLoadData(&ent.mod, code.data()) != hipSuccess ||
      hipModuleGetFunction(&ent.fn, ent.mod, kernel) != hipSuccess) {
    fprintf(stderr, "obx: JIT module load failed (%s)\n", kernel);
    ent.fn = nullptr;
    return nullptr;
  }
  return &ent;
}

/* prepare (compile/lookup) before the timed region; nullptr = use the
   precompiled kernels */
const jit_entry *jit_prepare(int device, const obx_table_facts &h,
                             const dev_plan_hdr &ph, const dev_leaf *pl) {
  const char *e = getenv("OBX_JIT");
  if (e && e[0] == '0') return nullptr;
  jit_scan_choice c;
  if (!jit_scan_choose(h, ph, pl, false, c)) return nullptr;
  jit_entry meta; /* the signature carries all of it: same for every hit */
  meta.kind = c.kind;
  if (c.kind == 2) {
    meta.wpb = c.st.wpb;
    meta.bdesc = c.st.bdesc != 0;
    meta.bd_cols = c.st.bd_cols;
    meta.joint = jit_joint_form_of(c.st);
  }
  return jit_get(
      device, jit_scan_key(ph, c), [&] { return jit_scan_source(ph, c); },
      "k_jit_scan", "obx_jit_src.hip", meta);
}

const jit_entry *jit_prepare_filter(int device, const obx_table_facts &h,
                                    const dev_plan_hdr &ph, const dev_leaf *pl,
                                    int want_row_ids) {
  const char *e = getenv("OBX_JIT");
  if (e && e[0] == '0') return nullptr;
  jit_fstrategy st;
  if (!jit_build_fstrategy(h, ph, pl, st)) return nullptr;
  if (want_row_ids) {
    /* ordered selection vectors need the per-block mask capture of the
       staged kernel and a bounded chunk count for the LDS mask array */
    uint32_t nch = ((h.max_block_rows ? h.max_block_rows : 4096) + 63) / 64;
    if (!st.fstage || nch > 256) return nullptr;
    st.frid = 1;
    st.fnch = (uint16_t)nch;
  }
  return jit_get(
      device, jit_fstrategy_sig(ph, st),
      [&] { return jit_gen_source_filter(ph, st); }, "k_jit_filter",
      "obx_jit_filter_src.hip", jit_entry());
}

int jit_launch(const jit_entry *je, obx_handle &h, const obx_bdesc *bd,
               hipStream_t stream, uint32_t *grid_out) {
  /* v2 keeps its accumulators for the kernel's lifetime and flushes once
     per workgroup: its grid is a multiple of the resident set (the grid
     the strategy proved its i64 bound for); v1 merges per block and keeps
     the fixed grid */
  const uint32_t grid = je->wpb ? jit_grid_for(h.n_blocks, h.n_cus, je->wpb)
                                : grid_for(h.n_blocks);
  *grid_out = grid;
  /* the v2 kernel takes the descriptor array last (null when its strategy
     reads dev_block); v1 has no such parameter and ignores the entry */
  void *args[8] = {&h.d_buf,     &h.d_blocks, &h.n_blocks,   &h.d_pleaves,
                   &h.d_bleaves, &h.d_gtable, &h.d_counters, &bd};
  return hipModuleLaunchKernel(je->fn, grid, 1, 1, OBX_WG_HOST, 1, 1, 0,
                               stream, args, nullptr) == hipSuccess
             ? 0
             : -1;
}
