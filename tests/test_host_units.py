"""The HIP-free host units compile without HIP.

The plan builder (obx_plan.cpp), the JIT generators (obx_jit_gen.cpp) and
the GPU-free probes (obx_probes.cpp) see a table only through
obx_table_facts and include no HIP header. A host compiler, called directly
and with no ROCm include directory, must accept each of them: a generator
that starts to read a device pointer, or a shared header that grows a HIP
dependency, fails here.
"""
import os
import shutil
import subprocess

import pytest

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     "oceanbase_amd", "csrc")
UNITS = ("obx_plan.cpp", "obx_jit_gen.cpp", "obx_probes.cpp")


def _host_compiler():
    """$CXX, else c++, else ROCm's clang++; never hipcc."""
    for cand in (os.environ.get("CXX"), "c++",
                 "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if not cand:
            continue
        exe = shutil.which(cand.split()[0])
        if exe and "hipcc" not in os.path.basename(exe):
            return [exe] + cand.split()[1:]
    return None


@pytest.fixture(scope="module")
def cxx():
    cc = _host_compiler()
    assert cc, "no host C++ compiler found ($CXX, c++, ROCm clang++)"
    return cc


@pytest.mark.parametrize("unit", UNITS)
def test_unit_compiles_without_hip(cxx, unit):
    cmd = cxx + ["-std=c++17", "-fsyntax-only", "-Wall", unit]
    assert not any("rocm" in a.lower() for a in cmd[1:]), cmd
    env = {k: v for k, v in os.environ.items()
           if k not in ("CPATH", "CPLUS_INCLUDE_PATH", "C_INCLUDE_PATH")}
    r = subprocess.run(cmd, cwd=_CSRC, env=env, capture_output=True, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("unit", UNITS)
def test_unit_names_no_hip_header(unit):
    """... and not by luck of the include path: what the unit pulls in, as
    the preprocessor lists it, has no HIP or hipRTC header in it."""
    cc = _host_compiler()
    assert cc, "no host C++ compiler found ($CXX, c++, ROCm clang++)"
    r = subprocess.run(cc + ["-std=c++17", "-M", unit], cwd=_CSRC,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = r.stdout.replace("\\\n", " ").split()
    assert not [d for d in deps if "/hip/" in d or "hiprtc" in d], deps
