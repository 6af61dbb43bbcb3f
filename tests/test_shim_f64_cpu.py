"""CPU (compile only, hipcc --offload-arch=gfx950): the library's own SQP stages behind the shim headers instantiate for linsys_t = double —
mpcgpu_compat::use_mpcg_generate_kkt<double> and use_mpcg_line_search<double> (include/mpcgpu_compat/sqp_stages.cuh) call the _f64 entry points.
The float instantiations are compiled next to them: one header text serves both."""
import os
import subprocess

from conftest import ROOT
from mpcgpu_amd import build

PROGRAM = r"""
#define STATE_SIZE 14
#define KNOT_POINTS 32
#include "mpcsim.cuh"
#include <type_traits>

static_assert(std::is_same<decltype(mpcgpu_compat::mpcg_entries<double>::generate_kkt), decltype(&mpcg_generate_kkt_f64) const>::value, "the _f64 entry");

int main() {
    mpcg_plant* plant = nullptr;
    mpcgpu_compat::use_mpcg_generate_kkt<double>(plant, 1e-4f, 1e-4f);
    mpcgpu_compat::use_mpcg_line_search<double>(10.f, 1e-4f, 1e-4f, 1.0f / 64);
    mpcgpu_compat::use_mpcg_generate_kkt<float>(plant, 1e-4f, 1e-4f);
    mpcgpu_compat::use_mpcg_line_search<float>(10.f, 1e-4f, 1e-4f, 1.0f / 64);
    double rho = 1e-3;
    return mpcgpu_compat::stages<double>().globalize_and_step && mpcgpu_compat::stages<float>().globalize_and_step && rho > 0 ? 0 : 1;
}
"""


def test_double_stages_compile(tmp_path):
    src = tmp_path / "stages_f64.cpp"
    src.write_text(PROGRAM)
    r = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-DUSE_DOUBLES", "-DLINSYS_SOLVE=1", "-I" + os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "stages_f64.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
