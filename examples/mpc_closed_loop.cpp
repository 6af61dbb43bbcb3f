// mpc_closed_loop.cpp — the MPC loop closed on the device.  Two runs on the reference's precomputed trajectory (mpcgpu_amd/data/iiwa_traj_0_0.f32):
//   1. simulateMPC (the reference's entry point, include/mpcsim.cuh:147) over THIS repo's shim headers with ALL THREE library stages registered:
//      mpcgpu_compat::use_mpcg_generate_kkt, use_mpcg_line_search and use_mpcg_simulate_and_shift (mpcg_simulate + mpcg_advance_horizon with the
//      host bookkeeping of include/mpcsim.cuh:280-352) — no stage is a host callback of the program's own.  The plant is integrated at 0.2 ms under
//      the PREVIOUS plan's controls, as the reference does; a fixed number of SQP iterations per control update of 2,000 us.
//   2. a batched run over the C ABI alone: B windows, U control updates, per update K iterations of the six SQP calls (rho per trajectory on the
//      device), then mpcg_simulate under the previous plan and mpcg_advance_horizon — the host decides WHEN to shift from the clock bookkeeping, which
//      is the same for every trajectory, so nothing synchronises inside an update; tracking errors wait in a device buffer and are read at the end.
// Compiled with -DUSE_DOUBLES (examples/mpc_closed_loop_f64; linsys_t = double, the reference's USE_DOUBLES build) both runs are in double: the stages
// are the <double> ones, the batched part calls the _f64 entry of all eight stages, and the float data file is widened on load.  The batched part's
// substep is (linsys_t)2e-4f either way — ten substeps per 2,000 us; simulateMPC's stage uses linsys_t(2e-4) as the reference does (include/mpcg.h).
// --integrator 1: both runs' KKT blocks and merits use semi-implicit Euler (option "integrator", the stages' integrator_type); --sim-integrator 1: both runs'
// plant substeps too (option "sim_integrator").  The JSON line carries "integrator" and "sim_integrator" when either flag is given, and is what it was without.
// --gravity G: the controller's model is the plant cloned with the reference's scalar gato_plant::GRAVITY = G (mpcg_plant_clone_gravity, base acceleration
// {0, 0, G}; 9.81: the arm stands on the ground) in both runs, and the file's controls — made for zero gravity — gain the gravity torques
// mpcg_inverse_dynamics(q_row, 0, 0) once, up front, on the device.  --sim-gravity G (default: --gravity) is the SIMULATED plant's scalar in the batched run,
// as --sim-integrator is its integrator: the plant need not be the controller's model.  (simulateMPC's stages share one plant, stages<T>().dynmem: the
// controller's.)  The JSON line carries "gravity" and "sim_gravity" when either is non-zero, and is what it was otherwise.
// --q-cost Q / --u-relative 1 (the batched run): its KKT blocks and merits come from mpcg_generate_kkt_xuref / mpcg_compute_merit_xuref with the running cost
// 1/2 |ee - goal|^2 + 1/2 Q |q - q_plan|^2 + 1/2 qd_cost |qd|^2 + 1/2 r_cost |u - [u-relative] u_plan|^2, the reference row read from the trajectory's own plan at
// the offset mpcg_advance_horizon advances: "stay near the planned posture", and (with --gravity) penalise what the control adds to the plan's gravity-compensating
// torque instead of the torque itself.  The JSON line carries "q_cost" and "u_relative" when either is given, and is what it was without.
// --u-max X --u-weight W [--sim-saturate] (the batched run): the controller's model is cloned with the soft torque limits |u_i| <= X at weight W
// (mpcg_plant_clone_limits), which the _xuref entries penalise — with the neutral cost ee_cost = 1, q_cost = 0 unless --q-cost / --u-relative say otherwise —, and
// with --sim-saturate the simulated plant clamps every control it applies to [-X, X].  The JSON line then carries "u_max", "u_weight", "sim_saturate" and
// "u_excess_peak", the largest max(|u| - X, 0) over the controls of every iterate the SQP calls left; with --u-max inf, or without it, it is what it was
// (--u-weight or --sim-saturate without --u-max is refused).
// --periods-us p0,p1,... (the batched run): trajectory b updates every p[b mod count] microseconds — every trajectory on its own schedule.  The clocks
// (prev_simulation_time, time_since_timestep, shifted) then live in device arrays and the run calls mpcg_simulate_clk / mpcg_advance_horizon_clk, which decide
// each trajectory's shift on the device; the host ShiftClock is run once per distinct period for the expected shift counts.  The JSON line then carries
// "periods_us", "expected_shifts" and "shifts" per trajectory, and "tracking_errors" as one list per trajectory; without the flag it is what it was.
// Prints one JSON line; exits 0 only if every tracking error is finite and every trajectory shifted the expected number of times.
//   hipcc --offload-arch=gfx950 -O2 -DLINSYS_SOLVE=1 [-DUSE_DOUBLES] -Iinclude examples/mpc_closed_loop.cpp -Lmpcgpu_amd -lmpcg_hip
//   mpc_closed_loop [--batch 4] [--knots 16] [--updates 17] [--iters 1] [--mpc-steps 16] [--integrator {0,1}] [--sim-integrator {0,1}] [--gravity G] [--sim-gravity G]
//                   [--q-cost Q] [--u-relative {0,1}] [--u-max X] [--u-weight W] [--sim-saturate] [--periods-us p0,p1,...]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define STATE_SIZE 14
#define KNOT_POINTS 32
#define PCG_MAX_ITER 3000
#include "mpcsim.cuh"

typedef linsys_t T;               // float, or double under -DUSE_DOUBLES; LS(entry) is the library entry point of that type
#ifdef USE_DOUBLES
#define LS(entry) entry##_f64
#else
#define LS(entry) entry
#endif
static const int n = 14, m = 7, ROWW = 27, ROWS = 400;      // a row of the data file: x (14), u (7), end-effector pose (6)

#define MPCG_OK_OR_DIE(h, expr)                                                                              \
    do {                                                                                                     \
        if ((expr) != MPCG_OK) { fprintf(stderr, "%s: %s\n", #expr, mpcg_last_error(h)); exit(1); }          \
    } while (0)

static std::vector<T> load_rows(const std::string& exe) {
    const std::string dir = exe.substr(0, exe.find_last_of('/') + 1);
    for (const std::string& p : {dir + "../mpcgpu_amd/data/iiwa_traj_0_0.f32", std::string("mpcgpu_amd/data/iiwa_traj_0_0.f32")}) {
        if (FILE* f = fopen(p.c_str(), "rb")) {
            std::vector<float> v((size_t)ROWS * ROWW);
            const size_t got = fread(v.data(), sizeof(float), v.size(), f);
            fclose(f);
            if (got == v.size()) return std::vector<T>(v.begin(), v.end());      // (widened under USE_DOUBLES)
        }
    }
    fprintf(stderr, "cannot read mpcgpu_amd/data/iiwa_traj_0_0.f32\n");
    exit(1);
}

template <typename V>
static V* to_device(const std::vector<V>& v) {
    V* p = nullptr;
    gpuErrchk(hipMalloc(reinterpret_cast<void**>(&p), v.size() * sizeof(V)));
    gpuErrchk(hipMemcpy(p, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice));
    return p;
}
template <typename V>
static V* dalloc(size_t count) { return to_device(std::vector<V>(count, V(0))); }

// The clock bookkeeping of include/mpcsim.cuh:294-347 for a constant simulation period: does update `u` (from 0) shift the horizon?
struct ShiftClock {
    double since = 0, timestep;
    bool shifted = false;
    explicit ShiftClock(double dt) : timestep(dt) {}
    bool update(double sim_us) {
        since += sim_us * 1e-6;
        const bool shift = !shifted && since > (double)(T)(1 * timestep);      // SHIFT_THRESHOLD
        if (shift) shifted = true;
        if (since > timestep) { shifted = false; since = std::fmod(since, timestep); }
        return shift;
    }
};

// u_row += tau_row for `count` rows of (x, u) of the plan
__global__ void gather_q(const T* rows, T* q, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count * m) q[i] = rows[(size_t)(i / m) * (n + m) + i % m];
}
__global__ void add_to_u(T* rows, const T* tau, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count * m) rows[(size_t)(i / m) * (n + m) + n + i % m] += tau[i];
}

// *peak = max(*peak, max over the controls of `batch` iterates of max(|u| - u_max, 0)): one workgroup, no atomics
__global__ void u_excess_peak(const T* xu, int batch, int N, double u_max, double* peak) {
    __shared__ double part[256];
    const size_t L = (size_t)(n + m) * N - m;
    double worst = 0.0;
    for (long i = threadIdx.x; i < (long)batch * (N - 1) * m; i += 256) {
        const long b = i / ((long)(N - 1) * m), r = i - b * (long)(N - 1) * m;
        const double e = fabs((double)xu[b * L + (size_t)(r / m) * (n + m) + n + r % m]) - u_max;
        worst = e > worst ? e : worst;
    }
    part[threadIdx.x] = worst;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w && part[threadIdx.x + w] > part[threadIdx.x]) part[threadIdx.x] = part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0] > *peak) *peak = part[0];
}

static mpcg_plant* clone_with_limits(const mpcg_plant* src, double u_max, double u_weight, bool saturate) {
    mpcg_limits lim;
    for (int i = 0; i < m; ++i) {
        lim.q_lo[i] = lim.qd_lo[i] = -INFINITY; lim.q_hi[i] = lim.qd_hi[i] = INFINITY;
        lim.u_lo[i] = -u_max; lim.u_hi[i] = u_max;
    }
    lim.q_weight = lim.qd_weight = 0.0; lim.u_weight = u_weight;
    lim.flags = saturate ? MPCG_LIMITS_SIM_SATURATE : 0u;
    mpcg_plant* p = nullptr;
    if (mpcg_plant_clone_limits(&p, src, &lim) != MPCG_OK) { fprintf(stderr, "mpcg_plant_clone_limits: %s\n", mpcg_last_error(nullptr)); exit(1); }
    return p;
}

static mpcg_plant* clone_with_gravity(const mpcg_plant* src, double g) {
    const double base_accel[3] = {0.0, 0.0, g};
    mpcg_plant* p = nullptr;
    if (mpcg_plant_clone_gravity(&p, src, base_accel) != MPCG_OK) { fprintf(stderr, "mpcg_plant_clone_gravity: %s\n", mpcg_last_error(nullptr)); exit(1); }
    return p;
}

int main(int argc, char** argv) {
    int B = 4, N = 16, U = 17, K = 1, mpc_steps = 16;
    double gravity = 0.0, sim_gravity = 0.0, q_cost = 0.0, u_max = INFINITY, u_weight = 0.0;
    bool sim_saturate = false, u_max_given = false, u_weight_given = false;
    bool sim_gravity_given = false;
    int u_relative = 0;
    std::vector<double> periods;                                              // --periods-us: empty = one clock on the host, 2,000 us for all
    int integrator = -1, sim_integrator = -1;                                 // -1: not given (0)
    for (int i = 1; i < argc; i += 2) {
        if (!strcmp(argv[i], "--sim-saturate")) { sim_saturate = true; --i; continue; }      // (a flag without a value)
        if (i + 1 >= argc) break;
        if (!strcmp(argv[i], "--batch")) B = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--knots")) N = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--updates")) U = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--iters")) K = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--mpc-steps")) mpc_steps = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--integrator")) integrator = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--sim-integrator")) sim_integrator = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--gravity")) gravity = atof(argv[i + 1]);
        else if (!strcmp(argv[i], "--sim-gravity")) { sim_gravity = atof(argv[i + 1]); sim_gravity_given = true; }
        else if (!strcmp(argv[i], "--q-cost")) q_cost = atof(argv[i + 1]);
        else if (!strcmp(argv[i], "--u-relative")) u_relative = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--u-max")) { u_max = atof(argv[i + 1]); u_max_given = true; }
        else if (!strcmp(argv[i], "--periods-us")) {
            for (const char* c = argv[i + 1]; *c;) {
                char* end = nullptr;
                periods.push_back(strtod(c, &end));
                if (end == c || (*end && *end != ',')) { fprintf(stderr, "--periods-us takes a comma-separated list of numbers\n"); return 2; }
                c = *end ? end + 1 : end;
            }
        }
        else if (!strcmp(argv[i], "--u-weight")) { u_weight = atof(argv[i + 1]); u_weight_given = true; }
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (B < 1 || N < 2 || N > 128 || U < 1 || K < 1 || mpc_steps < 1) { fprintf(stderr, "need batch >= 1, 2 <= knots <= 128, updates, iters, mpc-steps >= 1\n"); return 2; }
    if (integrator < -1 || integrator > 1 || sim_integrator < -1 || sim_integrator > 1) { fprintf(stderr, "--integrator and --sim-integrator take 0 or 1\n"); return 2; }
    if (!sim_gravity_given) sim_gravity = gravity;
    if (!std::isfinite(gravity) || !std::isfinite(sim_gravity)) { fprintf(stderr, "--gravity and --sim-gravity take finite numbers\n"); return 2; }
    if (!std::isfinite(q_cost) || q_cost < 0.0 || u_relative < 0 || u_relative > 1) { fprintf(stderr, "--q-cost takes a finite number >= 0, --u-relative 0 or 1\n"); return 2; }
    if ((u_weight_given || sim_saturate) && !u_max_given) { fprintf(stderr, "--u-weight and --sim-saturate need --u-max\n"); return 2; }
    if (!(u_max > 0.0) || !std::isfinite(u_weight) || u_weight < 0.0) { fprintf(stderr, "--u-max takes a number > 0 (inf: no limit), --u-weight a finite number >= 0\n"); return 2; }
    for (double p : periods)
        if (!std::isfinite(p) || p < 0.0) { fprintf(stderr, "--periods-us takes finite numbers >= 0\n"); return 2; }
    const bool clocks = !periods.empty();                                     // the batched run keeps per-trajectory clocks on the device
    const bool limits = std::isfinite(u_max);                                 // the batched run's plants carry torque limits: its cost comes from the _xuref entries
    const bool xuref = q_cost != 0.0 || u_relative != 0 || limits;           // the batched run's cost tracks the joint-space plan (the _xuref entries)
    const bool flagged = integrator >= 0 || sim_integrator >= 0;
    const unsigned integ = integrator > 0 ? 1u : 0u, sim_integ = sim_integrator > 0 ? 1u : 0u;
    const float dt = 1.0f / 64, qd_cost = 1e-4f, mu = 10.f;                  // include/common/settings.cuh:84-94, include/pcg/sqp.cuh:51
    const double period_us = 2000;                                            // SIMULATION_PERIOD
    const std::vector<T> rows = load_rows(argv[0]);
    std::vector<T> plan((size_t)ROWS * (n + m)), plan_goals((size_t)ROWS * 6);
    for (int t = 0; t < ROWS; ++t) {
        memcpy(&plan[(size_t)t * (n + m)], &rows[(size_t)t * ROWW], (n + m) * sizeof(T));
        memcpy(&plan_goals[(size_t)t * 6], &rows[(size_t)t * ROWW + n + m], 6 * sizeof(T));
    }
    unsigned seed = 99u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return ((seed >> 8) & 0xffff) / 65536.0f - 0.5f; };
    mpcg_plant* plant = nullptr;
    if (mpcg_plant_create_iiwa14(&plant, -1) != MPCG_OK) { fprintf(stderr, "mpcg_plant_create_iiwa14: %s\n", mpcg_last_error(nullptr)); return 1; }
    // the controller's model and the simulated plant of the batched run: the plain plant, or clones with gato_plant::GRAVITY = G
    mpcg_plant* plant_ctrl = gravity != 0.0 ? clone_with_gravity(plant, gravity) : plant;
    mpcg_plant* plant_sim = sim_gravity == gravity ? plant_ctrl : (sim_gravity != 0.0 ? clone_with_gravity(plant, sim_gravity) : plant);
    T* d_plan = to_device(plan);
    T* d_plan_goals = to_device(plan_goals);
    if (gravity != 0.0) {                                                     // the file's controls hold the arm without gravity: u_row += ID(q_row, 0, 0), once
        mpcg_handle* hid = nullptr;                                           // (a handle for this call alone: count <= max_batch x knot_points)
        if (mpcg_create(&hid, -1, n, 32, (uint32_t)((ROWS + 31) / 32)) != MPCG_OK) { fprintf(stderr, "mpcg_create: %s\n", mpcg_last_error(nullptr)); return 1; }
        T *d_q = dalloc<T>((size_t)ROWS * m), *d_tau = dalloc<T>((size_t)ROWS * m);
        const int blocks = (ROWS * m + 255) / 256;
        hipLaunchKernelGGL(gather_q, dim3(blocks), dim3(256), 0, nullptr, d_plan, d_q, ROWS);
        MPCG_OK_OR_DIE(hid, LS(mpcg_inverse_dynamics)(hid, plant_ctrl, d_q, nullptr, nullptr, d_tau, (uint32_t)ROWS, nullptr));
        hipLaunchKernelGGL(add_to_u, dim3(blocks), dim3(256), 0, nullptr, d_plan, d_tau, ROWS);
        gpuErrchk(hipMemcpy(plan.data(), d_plan, plan.size() * sizeof(T), hipMemcpyDeviceToHost));      // (the batched run's plans and iterates are cut from it below)
        gpuErrchk(hipFree(d_q));
        gpuErrchk(hipFree(d_tau));
        mpcg_destroy(hid);
    }

    // ---- 1. simulateMPC with the three library stages (single trajectory, KNOT_POINTS knots) ----
    std::vector<linsys_t> mpc_errors;
    {
        const float r_cost = KNOT_POINTS == 64 ? 1e-3f : 1e-4f;
        mpcgpu_compat::use_mpcg_generate_kkt<T>(plant_ctrl, qd_cost, r_cost, integ);
        mpcgpu_compat::use_mpcg_line_search<T>(mu, qd_cost, r_cost, dt, integ);
        mpcgpu_compat::use_mpcg_simulate_and_shift<T>(d_plan, d_plan_goals, ROWS, dt, period_us, (uint32_t)mpc_steps, 0, T(2e-4), sim_integ);
        auto& st = mpcgpu_compat::stages<T>();
        st.sqp_max_iter = 2;
        st.const_update_freq = false;         // a fixed number of SQP iterations per update (the wall-clock time box would make the run depend on the machine)
        std::vector<T> xs0(plan.begin(), plan.begin() + n);
        for (int i = 0; i < n; ++i) xs0[i] += 0.04f * rnd();                 // the measured state is off the plan
        T* d_xs = to_device(xs0);
        auto res = simulateMPC<T, toplevel_return_type>(n, m, KNOT_POINTS, ROWS, dt, d_plan_goals, d_plan, d_xs, 0, 0, 0, (T)1e-7, std::string("mpc_closed_loop"));
        mpc_errors = std::get<1>(res);
        gpuErrchk(hipFree(d_xs));
    }

    // ---- 2. B windows through U control updates over the C ABI, nothing synchronises inside an update ----
    const int TS = N + 24;                                                    // rows of a trajectory's own plan
    if (TS > ROWS) { fprintf(stderr, "knots too large for the data file\n"); return 2; }
    const float r_cost = N == 64 ? 1e-3f : 1e-4f;
    const size_t L = (size_t)(n + m) * N - m, nn = n * n, mm = m * m, nm = n * m;
    std::vector<T> bplan((size_t)B * TS * (n + m)), bgoals((size_t)B * TS * 6), xu((size_t)B * L), goals((size_t)B * 6 * N), xs((size_t)B * n);
    for (int b = 0; b < B; ++b) {
        const int t0 = (int)(((long)b * 37) % (ROWS - TS));
        memcpy(&bplan[(size_t)b * TS * (n + m)], &plan[(size_t)t0 * (n + m)], (size_t)TS * (n + m) * sizeof(T));
        memcpy(&bgoals[(size_t)b * TS * 6], &plan_goals[(size_t)t0 * 6], (size_t)TS * 6 * sizeof(T));
        memcpy(&xu[(size_t)b * L], &plan[(size_t)t0 * (n + m)], L * sizeof(T));
        memcpy(&goals[(size_t)b * 6 * N], &plan_goals[(size_t)t0 * 6], (size_t)6 * N * sizeof(T));
        for (int i = 0; i < n; ++i) xs[(size_t)b * n + i] = xu[(size_t)b * L + i] + 0.04f * rnd();
    }
    // the batched run's plants: with --u-max, limits clones of the two above (simulateMPC's stages call the plain entries, which refuse a plant with limits)
    mpcg_plant* plant_ctrl_b = limits ? clone_with_limits(plant_ctrl, u_max, u_weight, false) : plant_ctrl;
    mpcg_plant* plant_sim_b = limits ? clone_with_limits(plant_sim, u_max, u_weight, sim_saturate) : plant_sim;
    double* d_peak = nullptr;
    if (limits) { d_peak = dalloc<double>(1); gpuErrchk(hipMemset(d_peak, 0, sizeof(double))); }
    mpcg_handle* h = nullptr;
    if (mpcg_create(&h, -1, n, (uint32_t)N, (uint32_t)B) != MPCG_OK) { fprintf(stderr, "mpcg_create: %s\n", mpcg_last_error(nullptr)); return 1; }
    MPCG_OK_OR_DIE(h, mpcg_set_option(h, "integrator", (int)integ));
    MPCG_OK_OR_DIE(h, mpcg_set_option(h, "sim_integrator", (int)sim_integ));
    T *d_bplan = to_device(bplan), *d_bgoals = to_device(bgoals), *d_xu = to_device(xu), *d_xu_old = to_device(xu), *d_goals = to_device(goals), *d_xs = to_device(xs);
    T* d_G = dalloc<T>((size_t)B * ((nn + mm) * N - mm));
    T* d_C = dalloc<T>((size_t)B * (nn + nm) * (N - 1));
    T *d_g = dalloc<T>((size_t)B * L), *d_c = dalloc<T>((size_t)B * n * N), *d_S = dalloc<T>((size_t)B * 3 * nn * N), *d_Pinv = dalloc<T>((size_t)B * 3 * nn * N);
    T *d_gamma = dalloc<T>((size_t)B * n * N), *d_lambda = dalloc<T>((size_t)B * n * N), *d_dz = dalloc<T>((size_t)B * L), *d_merit = dalloc<T>((size_t)B * 8);
    T *d_merit_ref = dalloc<T>(B), *d_eePos = dalloc<T>((size_t)B * 3), *d_err = dalloc<T>(B), *d_err_hist = dalloc<T>((size_t)U * B);
    T *d_rho = to_device(std::vector<T>((size_t)B, (T)1e-3)), *d_drho = dalloc<T>(B), *d_ones = to_device(std::vector<T>((size_t)B, 1.0f));
    int32_t *d_step = dalloc<int32_t>(B), *d_offset = dalloc<int32_t>(B), *d_done = dalloc<int32_t>(B);
    uint32_t* d_iters = dalloc<uint32_t>(B);
    uint8_t *d_exit = dalloc<uint8_t>(B), *d_gave_up = dalloc<uint8_t>(B);
    hipStream_t s;
    gpuErrchk(hipStreamCreate(&s));
    T steps[8];
    for (int p = 0; p < 8; ++p) steps[p] = -1.0f / (float)(1 << p);
    const T zero = 0;
    // the generalised cost's reference: each trajectory's own plan, at the offset mpcg_advance_horizon advances (read when the kernels run)
    const mpcg_xuref ref = {d_bplan, (uint32_t)TS, (uint32_t)TS, d_offset, 1.0, q_cost, u_relative ? MPCG_XUREF_U_RELATIVE : 0u};
    auto merit_of = [&](const T* dz, const T* st, uint32_t count, T* out) {
        return xuref ? LS(mpcg_compute_merit_xuref)(h, plant_ctrl_b, m, dt, d_goals, d_xs, d_xu, dz, st, count, mu, qd_cost, r_cost, &ref, out, (uint32_t)B, s)
                     : LS(mpcg_compute_merit)(h, plant_ctrl, m, dt, d_goals, d_xs, d_xu, dz, st, count, mu, qd_cost, r_cost, out, (uint32_t)B, s);
    };
    ShiftClock clock(dt);
    double prev_us = 0;
    int shifts = 0;
    // --periods-us: the clocks of all trajectories on the device, zero at the start; the decisions of every update wait in d_did_hist
    std::vector<double> sim_us((size_t)B, period_us);
    for (int b = 0; clocks && b < B; ++b) sim_us[b] = periods[(size_t)b % periods.size()];
    double *d_sim_us = to_device(sim_us), *d_prev_us = dalloc<double>(B), *d_since = dalloc<double>(B);
    int32_t *d_shifted = dalloc<int32_t>(B), *d_did = dalloc<int32_t>(B), *d_did_hist = dalloc<int32_t>((size_t)U * B);
    for (int u = 0; u < U; ++u) {                                             // no host synchronisation in here
        // one SQP call (include/pcg/sqp.cuh): x_s = x_0 of the iterate, drho = 1, merit of the start iterate, K iterations
        gpuErrchk(hipMemcpyAsync(d_drho, d_ones, B * sizeof(T), hipMemcpyDeviceToDevice, s));
        gpuErrchk(hipMemsetAsync(d_gave_up, 0, B, s));
        MPCG_OK_OR_DIE(h, merit_of(nullptr, &zero, 1, d_merit_ref));
        for (int it = 0; it < K; ++it) {
            if (xuref) MPCG_OK_OR_DIE(h, LS(mpcg_generate_kkt_xuref)(h, plant_ctrl_b, m, dt, d_goals, d_xs, d_xu, qd_cost, r_cost, &ref, d_G, d_C, d_g, d_c, (uint32_t)B, s));
            else MPCG_OK_OR_DIE(h, LS(mpcg_generate_kkt)(h, plant_ctrl, m, dt, d_goals, d_xs, d_xu, qd_cost, r_cost, d_G, d_C, d_g, d_c, (uint32_t)B, s));
            MPCG_OK_OR_DIE(h, LS(mpcg_form_schur_rhov)(h, m, d_G, d_C, d_g, d_c, d_S, d_Pinv, d_gamma, d_rho, (uint32_t)B, MPCG_PRECOND_SS, s));
            MPCG_OK_OR_DIE(h, LS(mpcg_pcg_solve)(h, d_S, d_Pinv, d_gamma, d_lambda, (uint32_t)B, PCG_MAX_ITER, (T)1e-7, MPCG_PRECOND_SS, d_iters, d_exit, s));
            MPCG_OK_OR_DIE(h, LS(mpcg_compute_dz)(h, m, d_G, d_C, d_g, d_lambda, d_dz, (uint32_t)B, s));
            MPCG_OK_OR_DIE(h, merit_of(d_dz, steps, 8, d_merit));
            MPCG_OK_OR_DIE(h, LS(mpcg_line_search_step_rho)(h, m, d_merit, steps, 8, d_merit_ref, d_dz, d_xu, d_step, d_rho, d_drho, d_gave_up, (T)1.2, (T)1e-3, (T)10, (T)1e-3,
                                                        (uint32_t)B, s));
        }
        // the plant runs under the PREVIOUS plan for one period, offset by the previous period (include/mpcsim.cuh:288-291, :352)
        if (limits) hipLaunchKernelGGL(u_excess_peak, dim3(1), dim3(256), 0, s, d_xu, B, N, u_max, d_peak);
        if (clocks) {                                                         // every trajectory's own offset, period and shift decision, on the device
            MPCG_OK_OR_DIE(h, LS(mpcg_simulate_clk)(h, plant_sim_b, m, d_xs, d_xu_old, dt, d_prev_us, d_sim_us, (T)2e-4f, d_eePos, d_done, (uint32_t)B, s));
            gpuErrchk(hipMemcpyAsync(d_xu_old, d_xu, (size_t)B * L * sizeof(T), hipMemcpyDeviceToDevice, s));
            MPCG_OK_OR_DIE(h, LS(mpcg_advance_horizon_clk)(h, m, d_xu, d_lambda, d_goals, d_xs, d_eePos, d_bplan, d_bgoals, (uint32_t)TS, (uint32_t)TS, 0, d_offset, d_done,
                                                           d_err, dt, (double)(T)(1 * dt), d_sim_us, d_prev_us, d_since, d_shifted, d_did, (uint32_t)B, s));
            gpuErrchk(hipMemcpyAsync(d_err_hist + (size_t)u * B, d_err, B * sizeof(T), hipMemcpyDeviceToDevice, s));
            gpuErrchk(hipMemcpyAsync(d_did_hist + (size_t)u * B, d_did, B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
            continue;
        }
        MPCG_OK_OR_DIE(h, LS(mpcg_simulate)(h, plant_sim_b, m, d_xs, d_xu_old, dt, prev_us, period_us, (T)2e-4f, d_eePos, (uint32_t)B, s));
        gpuErrchk(hipMemcpyAsync(d_xu_old, d_xu, (size_t)B * L * sizeof(T), hipMemcpyDeviceToDevice, s));
        const bool shift = clock.update(period_us);
        MPCG_OK_OR_DIE(h, LS(mpcg_advance_horizon)(h, m, shift ? 1 : 0, d_xu, d_lambda, d_goals, d_xs, d_eePos, d_bplan, d_bgoals, (uint32_t)TS, (uint32_t)TS, 0,
                                               d_offset, d_done, d_err, (uint32_t)B, s));
        if (shift) {
            gpuErrchk(hipMemcpyAsync(d_err_hist + (size_t)shifts * B, d_err, B * sizeof(T), hipMemcpyDeviceToDevice, s));
            ++shifts;
        }
        prev_us = period_us;
    }
    gpuErrchk(hipStreamSynchronize(s));
    std::vector<T> err((size_t)U * B), xs_end((size_t)B * n);
    std::vector<int32_t> offset(B);
    gpuErrchk(hipMemcpy(err.data(), d_err_hist, err.size() * sizeof(T), hipMemcpyDeviceToHost));
    gpuErrchk(hipMemcpy(offset.data(), d_offset, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    gpuErrchk(hipMemcpy(xs_end.data(), d_xs, xs_end.size() * sizeof(T), hipMemcpyDeviceToHost));

    double peak = 0.0;
    if (limits) gpuErrchk(hipMemcpy(&peak, d_peak, sizeof(double), hipMemcpyDeviceToHost));

    bool ok = (int)mpc_errors.size() == mpc_steps;
    for (linsys_t e : mpc_errors) ok = ok && std::isfinite((double)e);
    for (T x : xs_end) ok = ok && std::isfinite((double)x);
    // --periods-us: the expected count of each trajectory from the host clock, run once per distinct period; its errors are those of the updates it shifted in
    std::vector<int32_t> did((size_t)U * B, 0);
    std::vector<int> expected((size_t)B, 0);
    if (clocks) {
        gpuErrchk(hipMemcpy(did.data(), d_did_hist, did.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < periods.size() && i < (size_t)B; ++i) {
            size_t first = 0;
            while (periods[first] != periods[i]) ++first;
            if (first == i) {
                ShiftClock c(dt);
                for (int u = 0; u < U; ++u) expected[i] += c.update(periods[i]) ? 1 : 0;
            } else expected[i] = expected[first];
        }
        for (int b = (int)periods.size(); b < B; ++b) expected[b] = expected[(size_t)b % periods.size()];
        for (int b = 0; b < B; ++b) {
            int count = 0;
            for (int u = 0; u < U; ++u)
                if (did[(size_t)u * B + b]) { ++count; ok = ok && std::isfinite((double)err[(size_t)u * B + b]); }
            ok = ok && count == expected[b] && offset[b] == expected[b];
        }
    } else {
        for (int i = 0; i < shifts * B; ++i) ok = ok && std::isfinite((double)err[i]);
        for (int b = 0; b < B; ++b) ok = ok && offset[b] == shifts;
    }
    printf("{\"batch\": %d, \"knots\": %d, \"updates\": %d, \"iters\": %d, ", B, N, U, K);
    if (flagged) printf("\"integrator\": %u, \"sim_integrator\": %u, ", integ, sim_integ);
    if (gravity != 0.0 || sim_gravity != 0.0) printf("\"gravity\": %g, \"sim_gravity\": %g, ", gravity, sim_gravity);
    if (q_cost != 0.0 || u_relative != 0) printf("\"q_cost\": %g, \"u_relative\": %d, ", q_cost, u_relative);
    if (limits) printf("\"u_max\": %g, \"u_weight\": %g, \"sim_saturate\": %d, \"u_excess_peak\": %.9g, ", u_max, u_weight, sim_saturate ? 1 : 0, peak);
    if (clocks) {
        printf("\"periods_us\": [");
        for (int b = 0; b < B; ++b) printf("%s%.17g", b ? ", " : "", sim_us[b]);
        printf("], \"expected_shifts\": [");
        for (int b = 0; b < B; ++b) printf("%s%d", b ? ", " : "", expected[b]);
        printf("], \"shifts\": [");
    } else {
        printf("\"expected_shifts\": %d, \"shifts\": [", shifts);
    }
    for (int b = 0; b < B; ++b) printf("%s%d", b ? ", " : "", offset[b]);
    printf("], \"tracking_errors\": [");
    for (int b = 0; clocks && b < B; ++b) {                                     // one list per trajectory: the updates it shifted in
        printf("%s[", b ? ", " : "");
        bool any = false;
        for (int u = 0; u < U; ++u)
            if (did[(size_t)u * B + b]) { printf("%s%.9g", any ? ", " : "", (double)err[(size_t)u * B + b]); any = true; }
        printf("]");
    }
    for (int i = 0; !clocks && i < shifts; ++i) {
        printf("%s[", i ? ", " : "");
        for (int b = 0; b < B; ++b) printf("%s%.9g", b ? ", " : "", (double)err[(size_t)i * B + b]);
        printf("]");
    }
    printf("], \"simulate_mpc\": {\"knots\": %d, \"control_updates\": %zu, \"tracking_errors\": [", KNOT_POINTS, mpc_errors.size());
    for (size_t i = 0; i < mpc_errors.size(); ++i) printf("%s%.9g", i ? ", " : "", (double)mpc_errors[i]);
    printf("]}, \"ok\": %s}\n", ok ? "true" : "false");

    for (void* p : {(void*)d_plan, (void*)d_plan_goals, (void*)d_bplan, (void*)d_bgoals, (void*)d_xu, (void*)d_xu_old, (void*)d_goals, (void*)d_xs, (void*)d_G, (void*)d_C,
                    (void*)d_g, (void*)d_c, (void*)d_S, (void*)d_Pinv, (void*)d_gamma, (void*)d_lambda, (void*)d_dz, (void*)d_merit, (void*)d_merit_ref, (void*)d_eePos,
                    (void*)d_err, (void*)d_err_hist, (void*)d_rho, (void*)d_drho, (void*)d_ones, (void*)d_step, (void*)d_offset, (void*)d_done, (void*)d_iters,
                    (void*)d_exit, (void*)d_gave_up, (void*)d_sim_us, (void*)d_prev_us, (void*)d_since, (void*)d_shifted, (void*)d_did,
                    (void*)d_did_hist})
        gpuErrchk(hipFree(p));
    gpuErrchk(hipStreamDestroy(s));
    if (limits) { gpuErrchk(hipFree(d_peak)); mpcg_plant_destroy(plant_ctrl_b); mpcg_plant_destroy(plant_sim_b); }
    if (plant_sim != plant_ctrl && plant_sim != plant) mpcg_plant_destroy(plant_sim);
    if (plant_ctrl != plant) mpcg_plant_destroy(plant_ctrl);
    mpcg_plant_destroy(plant);
    mpcg_destroy(h);
    return ok ? 0 : 1;
}
