// sqp_line_search_stage.cpp — sqpSolvePcg (the reference's entry point, include/pcg/sqp.cuh:22) over THIS repo's shim headers with BOTH library stages
// registered: mpcgpu_compat::use_mpcg_generate_kkt (KKT assembly) and mpcgpu_compat::use_mpcg_line_search (the reference's line search,
// include/pcg/sqp.cuh:264-353, over mpcg_compute_merit + mpcg_line_search_step) — no stage of the SQP iteration is a host callback of the program's own.
// One window of the reference's precomputed trajectory (mpcgpu_amd/data/iiwa_traj_0_0.f32), the plan perturbed off the dynamics; four SQP
// iterations; the merit of the iterate before and after is evaluated with mpcg_compute_merit itself.  Prints one JSON line, exits 0 if the merit
// went down and rho stayed inside [RHO_MIN, RHO_MAX].  (examples/mpcsim_iiwa_demo.cpp keeps its own host line search over the constraint violation.)
//   hipcc --offload-arch=gfx950 -O2 -DLINSYS_SOLVE=1 -Iinclude examples/sqp_line_search_stage.cpp -Lmpcgpu_amd -lmpcg_hip
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#define STATE_SIZE 14
#define KNOT_POINTS 32
#define PCG_MAX_ITER 3000
#include "mpcsim.cuh"

typedef float T;
static const int n = 14, m = 7, N = KNOT_POINTS, ROWW = 27;      // a row of the data file: x (14), u (7), end-effector pose (6)

int main(int, char** argv) {
    const std::string exe = argv[0], dir = exe.substr(0, exe.find_last_of('/') + 1);
    std::vector<T> rows(400 * ROWW);
    bool read = false;
    for (const std::string& p : {dir + "../mpcgpu_amd/data/iiwa_traj_0_0.f32", std::string("mpcgpu_amd/data/iiwa_traj_0_0.f32")})
        if (FILE* f = fopen(p.c_str(), "rb")) {
            read = fread(rows.data(), sizeof(T), rows.size(), f) == rows.size();
            fclose(f);
            if (read) break;
        }
    if (!read) { fprintf(stderr, "cannot read mpcgpu_amd/data/iiwa_traj_0_0.f32\n"); return 1; }
    const size_t L = (size_t)(n + m) * N - m;
    std::vector<T> xu(L, 0.f), goals(6 * N, 0.f);
    for (int k = 0; k < N; ++k) {
        const T* r = &rows[(size_t)k * ROWW];
        for (int i = 0; i < n; ++i) xu[(size_t)k * (n + m) + i] = r[i];
        if (k < N - 1) for (int i = 0; i < m; ++i) xu[(size_t)k * (n + m) + n + i] = r[n + i];
        for (int i = 0; i < 6; ++i) goals[6 * k + i] = r[n + m + i];
    }
    unsigned s = 99u;
    auto rnd = [&s]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0f - 0.5f; };
    for (size_t e = n; e < L; ++e) xu[e] += 0.02f * rnd();             // the plan is off the dynamics; x_0 stays (sqpSolvePcg takes x_s = x_0)

    const float mu = 10.f, qd_cost = 1e-4f, r_cost = 1e-4f, dt = 1.0f / 64;       // include/pcg/sqp.cuh:51, include/common/settings.cuh:84-94
    mpcg_plant* plant = nullptr;
    if (mpcg_plant_create_iiwa14(&plant, -1) != MPCG_OK) { fprintf(stderr, "mpcg_plant_create_iiwa14: %s\n", mpcg_last_error(nullptr)); return 1; }
    mpcgpu_compat::use_mpcg_generate_kkt<T>(plant, qd_cost, r_cost);
    mpcgpu_compat::use_mpcg_line_search<T>(mu, qd_cost, r_cost, dt);
    auto& st = mpcgpu_compat::stages<T>();
    st.sqp_max_iter = 4;
    st.const_update_freq = false;

    T *d_xu, *d_goal, *d_xs, *d_lambda, *d_merit;
    gpuErrchk(hipMalloc(&d_xu, L * sizeof(T)));
    gpuErrchk(hipMalloc(&d_goal, goals.size() * sizeof(T)));
    gpuErrchk(hipMalloc(&d_xs, n * sizeof(T)));
    gpuErrchk(hipMalloc(&d_lambda, (size_t)n * N * sizeof(T)));
    gpuErrchk(hipMalloc(&d_merit, sizeof(T)));
    gpuErrchk(hipMemcpy(d_xu, xu.data(), L * sizeof(T), hipMemcpyHostToDevice));
    gpuErrchk(hipMemcpy(d_goal, goals.data(), goals.size() * sizeof(T), hipMemcpyHostToDevice));
    gpuErrchk(hipMemcpy(d_xs, xu.data(), n * sizeof(T), hipMemcpyHostToDevice));
    gpuErrchk(hipMemset(d_lambda, 0, (size_t)n * N * sizeof(T)));
    mpcg_handle* h = mpcg_compat::handle_for(n, N);
    auto merit = [&]() {
        const float zero = 0.f;
        T v = 0;
        if (mpcg_compute_merit(h, plant, m, dt, d_goal, d_xs, d_xu, nullptr, &zero, 1, mu, qd_cost, r_cost, d_merit, 1, nullptr) != MPCG_OK)
            mpcg_compat::die("mpcg_compute_merit", h);
        gpuErrchk(hipMemcpy(&v, d_merit, sizeof(T), hipMemcpyDeviceToHost));
        return (double)v;
    };
    const double before = merit();
    pcg_config<T> config;
    config.pcg_exit_tol = (T)1e-7;
    config.pcg_max_iter = PCG_MAX_ITER;
    T rho = 1e-3f;
    auto res = sqpSolvePcg<T>(n, m, N, dt, d_goal, d_lambda, d_xu, st.dynmem, config, rho, (T)1e-3);
    const double after = merit();
    const uint32_t sqp_iter = std::get<3>(res);
    const bool ok = std::isfinite(after) && after < before && sqp_iter == st.sqp_max_iter && rho >= 1e-3f && rho <= 10.f;
    printf("{\"knots\": %d, \"sqp_iterations\": %u, \"merit_before\": %.6e, \"merit_after\": %.6e, \"rho\": %.4g, \"ok\": %s}\n", N, sqp_iter, before, after,
           (double)rho, ok ? "true" : "false");
    for (void* p : {(void*)d_xu, (void*)d_goal, (void*)d_xs, (void*)d_lambda, (void*)d_merit}) (void)hipFree(p);
    mpcg_plant_destroy(plant);
    return ok ? 0 : 1;
}
