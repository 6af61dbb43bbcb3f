"""CPU (compile only, hipcc --offload-arch=gfx950): the simulate_and_shift stage of the shim headers instantiates for linsys_t = double —
mpcgpu_compat::use_mpcg_simulate_and_shift<double> (include/mpcgpu_compat/sqp_stages.cuh) calls mpcg_simulate_f64 / mpcg_advance_horizon_f64, and
simulateMPC<double> of include/mpcsim.cuh compiles under -DUSE_DOUBLES with all three library stages.  The float instantiation is compiled next to it:
one body serves both."""
import os
import subprocess

from conftest import ROOT
from mpcgpu_amd import build

PROGRAM = r"""
#define STATE_SIZE 14
#define KNOT_POINTS 32
#include "mpcsim.cuh"
#include <type_traits>

static_assert(std::is_same<linsys_t, double>::value, "-DUSE_DOUBLES: linsys_t = double");
static_assert(mpcgpu_compat::mpcg_entries<double>::simulate == &mpcg_simulate_f64, "the _f64 entry");
static_assert(mpcgpu_compat::mpcg_entries<double>::advance_horizon == &mpcg_advance_horizon_f64, "the _f64 entry");
static_assert(mpcgpu_compat::mpcg_entries<float>::simulate == &mpcg_simulate, "the float entry");
static_assert(mpcgpu_compat::mpcg_entries<float>::advance_horizon == &mpcg_advance_horizon, "the float entry");

int main() {
    mpcg_plant* plant = nullptr;
    double *d_plan = nullptr, *d_goals = nullptr, *d_xs = nullptr;
    float *f_plan = nullptr, *f_goals = nullptr;
    mpcgpu_compat::use_mpcg_generate_kkt<double>(plant, 1e-4f, 1e-4f);
    mpcgpu_compat::use_mpcg_line_search<double>(10.f, 1e-4f, 1e-4f, 1.0f / 64);
    mpcgpu_compat::use_mpcg_simulate_and_shift<double>(d_plan, d_goals, 400, 1.0f / 64, 2000.0, 4);
    mpcgpu_compat::use_mpcg_simulate_and_shift<float>(f_plan, f_goals, 400, 1.0f / 64, 2000.0, 4);
    if (!mpcgpu_compat::stages<double>().simulate_and_shift || !mpcgpu_compat::stages<float>().simulate_and_shift) return 1;
    auto res = simulateMPC<double, toplevel_return_type>(14, 7, KNOT_POINTS, 400, 1.0f / 64, d_goals, d_plan, d_xs, 0, 0, 0, 1e-7, std::string("compile only"));
    static_assert(std::is_same<decltype(std::get<2>(res)), double&>::value, "tracking errors in linsys_t");
    return 0;
}
"""


def test_double_simulate_and_shift_stage_compiles(tmp_path):
    src = tmp_path / "stages_sim_f64.cpp"
    src.write_text(PROGRAM)
    r = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-DUSE_DOUBLES", "-DLINSYS_SOLVE=1", "-I" + os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "stages_sim_f64.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
