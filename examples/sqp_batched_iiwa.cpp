// sqp_batched_iiwa.cpp — a BATCHED SQP iteration that never leaves the device, over the C ABI alone (include/mpcg.h): for B windows of the reference's
// precomputed trajectory (mpcgpu_amd/data/iiwa_traj_0_0.f32, perturbed as in mpcsim_iiwa_demo.cpp) K iterations of
//     mpcg_generate_kkt -> mpcg_form_schur (SS) -> mpcg_pcg_solve -> mpcg_compute_dz -> mpcg_compute_merit (8 step sizes -1 / 2^p) -> mpcg_line_search_step
// — the stages of include/pcg/sqp.cuh:190-353 of the reference, whose line search runs eight cooperative launches, a device synchronisation and a
// read-back per iteration for ONE trajectory.  Here nothing synchronises inside an iteration: the merit of every trajectory and iteration and the
// accepted exponents wait in device buffers and are read once at the end.  Without --adapt-rho, rho stays at its initial value (one scalar per
// mpcg_form_schur call).  With it every trajectory carries its own rho, drho and "finished" flag in device memory: mpcg_form_schur_rhov reads the
// rho vector and mpcg_line_search_step_rho applies the reference's adaptation (sqp.cuh:304-320: a failed line search multiplies drho and rho by
// 1.2, a success divides them, rho > 10 gives the trajectory up and resets rho) — still without a synchronisation inside an iteration; the JSON line
// then also carries "rho_final", "drho_final" and "done" per trajectory.  --merit-f32 sets option "merit_f32" = 1 on the handle: every mpcg_compute_merit
// of the run evaluates its point merits in packed float (the reference's own arithmetic; merits within 1e-5 max(1, |merit|) of the default's).
// Compiled with -DUSE_DOUBLES (examples/sqp_batched_iiwa_f64; linsys_t = double, the reference's USE_DOUBLES build) the six calls are the library's double entry
// points — mpcg_generate_kkt_f64 -> mpcg_form_schur(_rhov)_f64 -> mpcg_pcg_solve_f64 -> mpcg_compute_dz_f64 -> mpcg_compute_merit_f64 ->
// mpcg_line_search_step(_rho)_f64 — on the same inputs widened to double; the merits are then printed with 17 digits.  --merit-f32 has no effect there.
// --integrator 1 sets option "integrator" = 1: the KKT blocks and every merit of the run use semi-implicit Euler (q' = q + dt qd'; both builds, float and double);
// the JSON line then carries "integrator".  Without the flag the line is what it was.
// --gravity G clones the plant with the reference's scalar gato_plant::GRAVITY = G (mpcg_plant_clone_gravity, base acceleration {0, 0, G}; 9.81: the arm stands
// on the ground) and, because the file's controls were made for zero gravity, adds the gravity torques mpcg_inverse_dynamics(q_k, 0, 0) to the iterate's controls
// once, up front, on the device; the JSON line then carries "gravity".  With G = 0 or without the flag nothing of this runs and the line is what it was.
// Prints one JSON line; exits 0 only if every trajectory's merit went down.
//   hipcc --offload-arch=gfx950 -O2 [-DUSE_DOUBLES] -Iinclude examples/sqp_batched_iiwa.cpp -Lmpcgpu_amd -lmpcg_hip
//   sqp_batched_iiwa [--batch 8] [--knots 32] [--iters 4] [--mu 10] [--rho 1e-3] [--adapt-rho] [--merit-f32] [--integrator {0,1}] [--gravity G]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "mpcg.h"

// linsys_t as in the reference's include/common/settings.cuh:41-49; LS(entry) is the library entry point of that type
#ifdef USE_DOUBLES
typedef double linsys_t;
#define LS(entry) entry##_f64
#define MERIT_FMT "%.17g"
#else
typedef float linsys_t;
#define LS(entry) entry
#define MERIT_FMT "%.9g"
#endif

static const int n = 14, m = 7, ROWW = 27, ROWS = 400;      // a row of the data file: x (14), u (7), end-effector pose (6)

#define HIP_OK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); exit(1); }       \
    } while (0)
#define MPCG_OK_OR_DIE(h, expr)                                                                              \
    do {                                                                                                     \
        if ((expr) != MPCG_OK) { fprintf(stderr, "%s: %s\n", #expr, mpcg_last_error(h)); exit(1); }          \
    } while (0)

static std::vector<float> load_rows(const std::string& exe) {
    const std::string dir = exe.substr(0, exe.find_last_of('/') + 1);
    for (const std::string& p : {dir + "../mpcgpu_amd/data/iiwa_traj_0_0.f32", std::string("mpcgpu_amd/data/iiwa_traj_0_0.f32")}) {
        if (FILE* f = fopen(p.c_str(), "rb")) {
            std::vector<float> v((size_t)ROWS * ROWW);
            const size_t got = fread(v.data(), sizeof(float), v.size(), f);
            fclose(f);
            if (got == v.size()) return v;
        }
    }
    fprintf(stderr, "cannot read mpcgpu_amd/data/iiwa_traj_0_0.f32\n");
    exit(1);
}

template <typename T>
static T* dalloc(size_t count) {
    T* p = nullptr;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
    HIP_OK(hipMemset(p, 0, count * sizeof(T)));
    return p;
}

// u_k += tau_k for the `count` knots that have a control: knot s is trajectory s / per, knot s % per, of an iterate of L values per trajectory
__global__ void gather_q(const linsys_t* xu, linsys_t* q, int count, int per, size_t L) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count * m) q[i] = xu[(size_t)(i / m / per) * L + (size_t)(i / m % per) * (n + m) + i % m];
}
__global__ void add_to_u(linsys_t* xu, const linsys_t* tau, int count, int per, size_t L) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count * m) xu[(size_t)(i / m / per) * L + (size_t)(i / m % per) * (n + m) + n + i % m] += tau[i];
}

int main(int argc, char** argv) {
    int B = 8, N = 32, K = 4;
    double gravity = 0.0;
    linsys_t mu = 10.f, rho = (linsys_t)1e-3;
    bool adapt = false, merit_f32 = false;
    int integrator = -1;                                                      // -1: not given (the handle's default, 0)
    for (int i = 1; i < argc; i += 2) {
        if (!strcmp(argv[i], "--adapt-rho")) { adapt = true; --i; continue; }
        if (!strcmp(argv[i], "--merit-f32")) { merit_f32 = true; --i; continue; }
        if (i + 1 >= argc) break;
        if (!strcmp(argv[i], "--batch")) B = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--knots")) N = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--iters")) K = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--mu")) mu = (linsys_t)atof(argv[i + 1]);
        else if (!strcmp(argv[i], "--rho")) rho = (linsys_t)atof(argv[i + 1]);
        else if (!strcmp(argv[i], "--integrator")) integrator = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--gravity")) gravity = atof(argv[i + 1]);
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (B < 1 || N < 2 || N + 1 > ROWS || K < 1) { fprintf(stderr, "need batch >= 1, 2 <= knots < %d, iters >= 1\n", ROWS); return 2; }
    if (integrator < -1 || integrator > 1) { fprintf(stderr, "--integrator takes 0 or 1\n"); return 2; }
    if (!std::isfinite(gravity)) { fprintf(stderr, "--gravity takes a finite number\n"); return 2; }
    const linsys_t dt = 1.0f / 64, qd_cost = (linsys_t)1e-4, r_cost = (linsys_t)(N == 64 ? 1e-3 : 1e-4);      // include/common/settings.cuh:84-94
    const size_t L = (size_t)(n + m) * N - m;
    const std::vector<float> rows = load_rows(argv[0]);

    // B windows spread over the file; the measured state is off the plan and the plan is off the dynamics (mpcsim_iiwa_demo.cpp)
    std::vector<float> xu((size_t)B * L), goals((size_t)B * 6 * N), xs((size_t)B * n);
    unsigned s = 99u;
    auto rnd = [&s]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0f - 0.5f; };
    for (int b = 0; b < B; ++b) {
        const int t0 = (int)(((long)b * 37) % (ROWS - N));
        float* w = &xu[(size_t)b * L];
        for (int k = 0; k < N; ++k) {
            const float* r = &rows[(size_t)(t0 + k) * ROWW];
            for (int i = 0; i < n; ++i) w[(size_t)k * (n + m) + i] = r[i];
            if (k < N - 1) for (int i = 0; i < m; ++i) w[(size_t)k * (n + m) + n + i] = r[n + i];
            for (int i = 0; i < 6; ++i) goals[((size_t)b * N + k) * 6 + i] = r[n + m + i];
        }
        for (int i = 0; i < n; ++i) xs[(size_t)b * n + i] = w[i] + 0.04f * rnd();
        for (size_t e = n; e < L; ++e) w[e] += 0.02f * rnd();
    }

    mpcg_handle* h = nullptr;
    mpcg_plant* plant = nullptr;
    if (mpcg_create(&h, -1, n, (uint32_t)N, (uint32_t)B) != MPCG_OK) { fprintf(stderr, "mpcg_create: %s\n", mpcg_last_error(nullptr)); return 1; }
    if (merit_f32) MPCG_OK_OR_DIE(h, mpcg_set_option(h, "merit_f32", 1));
    if (integrator >= 0) MPCG_OK_OR_DIE(h, mpcg_set_option(h, "integrator", integrator));
    if (mpcg_plant_create_iiwa14(&plant, -1) != MPCG_OK) { fprintf(stderr, "mpcg_plant_create_iiwa14: %s\n", mpcg_last_error(nullptr)); return 1; }
    if (gravity != 0.0) {                                                     // the plant with gato_plant::GRAVITY = G: a clone, the plain one is not needed any more
        const double base_accel[3] = {0.0, 0.0, gravity};
        mpcg_plant* heavy = nullptr;
        if (mpcg_plant_clone_gravity(&heavy, plant, base_accel) != MPCG_OK) { fprintf(stderr, "mpcg_plant_clone_gravity: %s\n", mpcg_last_error(nullptr)); return 1; }
        mpcg_plant_destroy(plant);
        plant = heavy;
    }

    const size_t nn = n * n, mm = m * m, nm = n * m;
    linsys_t* d_xu = dalloc<linsys_t>((size_t)B * L);
    linsys_t* d_goals = dalloc<linsys_t>(goals.size());
    linsys_t* d_xs = dalloc<linsys_t>(xs.size());
    linsys_t* d_G = dalloc<linsys_t>((size_t)B * ((nn + mm) * N - mm));
    linsys_t* d_C = dalloc<linsys_t>((size_t)B * (nn + nm) * (N - 1));
    linsys_t* d_g = dalloc<linsys_t>((size_t)B * L);
    linsys_t* d_c = dalloc<linsys_t>((size_t)B * n * N);
    linsys_t* d_S = dalloc<linsys_t>((size_t)B * 3 * nn * N);
    linsys_t* d_Pinv = dalloc<linsys_t>((size_t)B * 3 * nn * N);
    linsys_t* d_gamma = dalloc<linsys_t>((size_t)B * n * N);
    linsys_t* d_lambda = dalloc<linsys_t>((size_t)B * n * N);
    linsys_t* d_dz = dalloc<linsys_t>((size_t)B * L);
    linsys_t* d_merit = dalloc<linsys_t>((size_t)B * 8);
    linsys_t* d_merit_ref = dalloc<linsys_t>(B);
    linsys_t* d_merit_hist = dalloc<linsys_t>((size_t)(K + 1) * B);
    int32_t* d_step_hist = dalloc<int32_t>((size_t)K * B);
    uint32_t* d_iters = dalloc<uint32_t>(B);
    uint8_t* d_exit = dalloc<uint8_t>(B);
    // --adapt-rho: the per-trajectory state of the rho adaptation (rho = the initial value, drho = 1, nobody finished)
    linsys_t* d_rho = dalloc<linsys_t>(B);
    linsys_t* d_drho = dalloc<linsys_t>(B);
    uint8_t* d_done = dalloc<uint8_t>(B);
    {
        const std::vector<linsys_t> rho0((size_t)B, rho), one((size_t)B, 1);
        HIP_OK(hipMemcpy(d_rho, rho0.data(), B * sizeof(linsys_t), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_drho, one.data(), B * sizeof(linsys_t), hipMemcpyHostToDevice));
    }
    for (auto pr : {std::make_pair(d_xu, &xu), std::make_pair(d_goals, &goals), std::make_pair(d_xs, &xs)}) {      // the float inputs, widened under USE_DOUBLES
        const std::vector<linsys_t> w(pr.second->begin(), pr.second->end());
        HIP_OK(hipMemcpy(pr.first, w.data(), w.size() * sizeof(linsys_t), hipMemcpyHostToDevice));
    }

    hipStream_t st;
    HIP_OK(hipStreamCreate(&st));
    linsys_t steps[8];
    for (int p = 0; p < 8; ++p) steps[p] = -1.0f / (float)(1 << p);          // alpha = -1 / 2^p (include/common/merit.cuh:47)
    const linsys_t zero = 0;
    if (gravity != 0.0) {                                                     // the file's controls hold the arm without gravity: u_k += ID(q_k, 0, 0), once
        const int count = B * (N - 1), blocks = (count * m + 255) / 256;
        linsys_t* d_q = dalloc<linsys_t>((size_t)count * m);
        linsys_t* d_tau = dalloc<linsys_t>((size_t)count * m);
        hipLaunchKernelGGL(gather_q, dim3(blocks), dim3(256), 0, st, d_xu, d_q, count, N - 1, L);
        MPCG_OK_OR_DIE(h, LS(mpcg_inverse_dynamics)(h, plant, d_q, nullptr, nullptr, d_tau, (uint32_t)count, st));
        hipLaunchKernelGGL(add_to_u, dim3(blocks), dim3(256), 0, st, d_xu, d_tau, count, N - 1, L);
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipFree(d_q));
        HIP_OK(hipFree(d_tau));
    }
    // the merit of the start iterate: the reference's compute_merit (include/pcg/sqp.cuh:171-187) — with the initial-state term, like the eight trials
    MPCG_OK_OR_DIE(h, LS(mpcg_compute_merit)(h, plant, m, dt, d_goals, d_xs, d_xu, nullptr, &zero, 1, mu, qd_cost, r_cost, d_merit_ref, (uint32_t)B, st));
    HIP_OK(hipMemcpyAsync(d_merit_hist, d_merit_ref, B * sizeof(linsys_t), hipMemcpyDeviceToDevice, st));
    for (int it = 0; it < K; ++it) {                                          // no host synchronisation in here
        MPCG_OK_OR_DIE(h, LS(mpcg_generate_kkt)(h, plant, m, dt, d_goals, d_xs, d_xu, qd_cost, r_cost, d_G, d_C, d_g, d_c, (uint32_t)B, st));
        if (adapt) MPCG_OK_OR_DIE(h, LS(mpcg_form_schur_rhov)(h, m, d_G, d_C, d_g, d_c, d_S, d_Pinv, d_gamma, d_rho, (uint32_t)B, MPCG_PRECOND_SS, st));
        else MPCG_OK_OR_DIE(h, LS(mpcg_form_schur)(h, m, d_G, d_C, d_g, d_c, d_S, d_Pinv, d_gamma, rho, (uint32_t)B, MPCG_PRECOND_SS, st));
        MPCG_OK_OR_DIE(h, LS(mpcg_pcg_solve)(h, d_S, d_Pinv, d_gamma, d_lambda, (uint32_t)B, 3000, (linsys_t)1e-7, MPCG_PRECOND_SS, d_iters, d_exit, st));
        MPCG_OK_OR_DIE(h, LS(mpcg_compute_dz)(h, m, d_G, d_C, d_g, d_lambda, d_dz, (uint32_t)B, st));
        MPCG_OK_OR_DIE(h, LS(mpcg_compute_merit)(h, plant, m, dt, d_goals, d_xs, d_xu, d_dz, steps, 8, mu, qd_cost, r_cost, d_merit, (uint32_t)B, st));
        if (adapt) MPCG_OK_OR_DIE(h, LS(mpcg_line_search_step_rho)(h, m, d_merit, steps, 8, d_merit_ref, d_dz, d_xu, d_step_hist + (size_t)it * B, d_rho, d_drho, d_done,
                                                               (linsys_t)1.2, (linsys_t)1e-3, (linsys_t)10, rho, (uint32_t)B, st));
        else MPCG_OK_OR_DIE(h, LS(mpcg_line_search_step)(h, m, d_merit, steps, 8, d_merit_ref, d_dz, d_xu, d_step_hist + (size_t)it * B, (uint32_t)B, st));
        HIP_OK(hipMemcpyAsync(d_merit_hist + (size_t)(it + 1) * B, d_merit_ref, B * sizeof(linsys_t), hipMemcpyDeviceToDevice, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    std::vector<linsys_t> hist((size_t)(K + 1) * B);
    std::vector<int32_t> expo((size_t)K * B);
    HIP_OK(hipMemcpy(hist.data(), d_merit_hist, hist.size() * sizeof(linsys_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(expo.data(), d_step_hist, expo.size() * sizeof(int32_t), hipMemcpyDeviceToHost));

    bool ok = true;
    for (int b = 0; b < B; ++b) ok = ok && std::isfinite(hist[(size_t)K * B + b]) && hist[(size_t)K * B + b] < hist[b];
    printf("{\"batch\": %d, \"knots\": %d, \"iters\": %d, \"mu\": %g, \"rho\": %g, ", B, N, K, (double)mu, (double)rho);
    if (integrator >= 0) printf("\"integrator\": %d, ", integrator);
    if (gravity != 0.0) printf("\"gravity\": %g, ", gravity);
    printf("\"merit\": [");
    for (int b = 0; b < B; ++b) {
        printf("%s[", b ? ", " : "");
        for (int it = 0; it <= K; ++it) printf("%s" MERIT_FMT, it ? ", " : "", (double)hist[(size_t)it * B + b]);
        printf("]");
    }
    printf("], \"exponents\": [");
    for (int b = 0; b < B; ++b) {
        printf("%s[", b ? ", " : "");
        for (int it = 0; it < K; ++it) printf("%s%d", it ? ", " : "", expo[(size_t)it * B + b]);
        printf("]");
    }
    if (adapt) {
        std::vector<linsys_t> rho_f(B), drho_f(B);
        std::vector<uint8_t> done_f(B);
        HIP_OK(hipMemcpy(rho_f.data(), d_rho, B * sizeof(linsys_t), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(drho_f.data(), d_drho, B * sizeof(linsys_t), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(done_f.data(), d_done, B * sizeof(uint8_t), hipMemcpyDeviceToHost));
        printf("], \"rho_final\": [");
        for (int b = 0; b < B; ++b) printf("%s" MERIT_FMT, b ? ", " : "", (double)rho_f[b]);
        printf("], \"drho_final\": [");
        for (int b = 0; b < B; ++b) printf("%s" MERIT_FMT, b ? ", " : "", (double)drho_f[b]);
        printf("], \"done\": [");
        for (int b = 0; b < B; ++b) printf("%s%d", b ? ", " : "", (int)done_f[b]);
    }
    printf("], \"ok\": %s}\n", ok ? "true" : "false");

    for (void* p : {(void*)d_xu, (void*)d_goals, (void*)d_xs, (void*)d_G, (void*)d_C, (void*)d_g, (void*)d_c, (void*)d_S, (void*)d_Pinv, (void*)d_gamma,
                    (void*)d_lambda, (void*)d_dz, (void*)d_merit, (void*)d_merit_ref, (void*)d_merit_hist, (void*)d_step_hist, (void*)d_iters, (void*)d_exit,
                    (void*)d_rho, (void*)d_drho, (void*)d_done})
        HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(st));
    mpcg_plant_destroy(plant);
    mpcg_destroy(h);
    return ok ? 0 : 1;
}
