#!/bin/bash
# Builds the MI355X product engine (libobx.so) in-tree for gfx950.
# The .so is git-ignored but ships to the GPU box via the gpurun snapshot.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-hipcc}
# embed the device headers for the hipRTC JIT (obx_jit_rt.cpp)
python3 - << 'PYEOF'
for src, out in (("obx_dev.h", "obx_embed_dev_h.inc"),
                 ("obx_dev_common.h", "obx_embed_common_h.inc"),
                 ("obx_keyset.h", "obx_embed_keyset_h.inc"),
                 ("obx_jit_dev.h", "obx_embed_jit_dev_h.inc")):
    txt = open(src).read()
    assert ')OBXRAW"' not in txt
    open(out, "w").write('R"OBXRAW(' + txt + ')OBXRAW"\n')
PYEOF
# The plan builder, the JIT generators and the GPU-free probes are plain C++
# (no HIP header, no device pass); everything after -x hip is HIP.
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared \
    -x c++ obx_plan.cpp obx_jit_gen.cpp obx_probes.cpp \
    -x hip obx_engine.cpp obx_jit_rt.cpp obx_pax_load.cpp obx_cs_load.cpp \
    obx_kernels.hip obx_project.hip obx_cs_kernels.hip obx_keys.hip \
    obx_join.hip \
    -L/opt/rocm/lib -lhiprtc \
    -o ../libobx.so
echo "built oceanbase_amd/libobx.so"
