// sqp_stages.cuh — plug points for the stages of MPCGPU's SQP / MPC loop around the linear-system section (KKT
// assembly with the robot dynamics, merit / line search, plant simulation + horizon shift).  The shim versions of sqpSolvePcg / sqpSolveQdldl /
// simulateMPC (include/pcg/sqp.cuh, include/qdldl/sqp.cuh, include/mpcsim.cuh of THIS repo) keep the reference's names, argument lists and
// return tuples and run the linear-system section on libmpcg_hip; wherever the reference calls one of those stages' kernels they call the
// function registered here.  All three are in the library now and register themselves for the IIWA-14: use_mpcg_generate_kkt (mpcg_generate_kkt; T = double:
// mpcg_generate_kkt_f64), use_mpcg_line_search (mpcg_compute_merit + mpcg_line_search_step, T = double: their _f64 twins, with the alpha / rho logic of include/pcg/sqp.cuh:264-353) and
// use_mpcg_simulate_and_shift (mpcg_simulate + mpcg_advance_horizon, T = double: their _f64 twins, with the host bookkeeping of include/mpcsim.cuh:280-352).  A maintainer porting
// MPCGPU with another robot registers thin wrappers around the reference's kernels instead; examples/mpcsim_shim_demo.cpp registers a synthetic
// convex problem.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <functional>
#include <memory>
#include <type_traits>

#ifndef CONST_UPDATE_FREQ
#define CONST_UPDATE_FREQ 1      // include/common/settings.cuh:56-58
#endif
#ifndef SQP_MAX_TIME_US
#define SQP_MAX_TIME_US 2000     // include/common/settings.cuh:161-163
#endif
#ifndef SIMULATION_PERIOD
#define SIMULATION_PERIOD 2000   // include/common/settings.cuh:70-72 [us]
#endif

namespace mpcgpu_compat {

inline void require_stage(bool present, const char* which);

template <typename T>
struct sqp_stages {
    // generate_kkt_submatrices<<<knot_points, KKT_THREADS>>> (include/pcg/sqp.cuh:190-204, include/common/kkt.cuh:22-163):
    // fill d_G_dense, d_C_dense, d_g, d_c for the current iterate d_xu.
    std::function<void(uint32_t state_size, uint32_t control_size, uint32_t knot_points, T* d_G_dense, T* d_C_dense, T* d_g, T* d_c,
                       void* d_dynMem_const, float timestep, T* d_eePos_traj, T* d_xs, T* d_xu)> generate_kkt;
    // everything after compute_dz in one SQP iteration (include/pcg/sqp.cuh:265-353): line search over alpha = -1/2^p,
    // rho adaptation, xu += alpha dz.  Returns false to stop the SQP loop.
    std::function<bool(uint32_t state_size, uint32_t control_size, uint32_t knot_points, T* d_xu, T* d_dz, T& rho, T rho_reset,
                       uint32_t sqp_iter)> globalize_and_step;
    // simple_simulate + horizon shift of one control step (include/mpcsim.cuh:288-341).  Returns the tracking error; sets
    // done when the reference trajectory is exhausted.
    std::function<T(uint32_t state_size, uint32_t control_size, uint32_t knot_points, T* d_xs, T* d_xu, T* d_lambda,
                    T* d_eePos_goal, double sqp_solve_time_us, bool& done)> simulate_and_shift;
    // d_dynMem_const of the reference (gato_plant::initializeDynamicsConstMem<T>(), include/mpcsim.cuh:194): handed to every SQP call by
    // simulateMPC and on to the generate_kkt stage.  With the library's own stage (use_mpcg_generate_kkt below) it is an mpcg_plant*.
    void* dynmem = nullptr;
    uint32_t sqp_max_iter = 20;          // SQP_MAX_ITER with TIME_LINSYS (include/common/settings.cuh:152-158)
    // The SQP time box (include/common/settings.cuh:56-58 CONST_UPDATE_FREQ = 1, :161-163 SQP_MAX_TIME_US = 2000): with
    // const_update_freq the loop is left as soon as sqpTimecheck() — wall time since the start of the call, allocation included,
    // as the reference measures it (include/pcg/sqp.cuh:35, :161-169) — exceeds sqp_max_time_us; checked after every stage.
    bool const_update_freq = CONST_UPDATE_FREQ != 0;
    double sqp_max_time_us = SQP_MAX_TIME_US;
};

template <typename T>
inline sqp_stages<T>& stages() {
    static sqp_stages<T> s;
    return s;
}

// The library's own generate_kkt_submatrices (mpcg_generate_kkt: IIWA-14 dynamics, tracking cost, Euler integrator on the device) as the
// generate_kkt stage — the default when an mpcg_plant is supplied; use_mpcg_line_search below adds the merit function / line search,
// use_mpcg_simulate_and_shift the plant simulation and the horizon shift.
// qd_cost / r_cost: QD_COST / R_COST of include/common/settings.cuh:84-94.  Needs gbd_pcg_compat/gpu_pcg.cuh (handle cache) before this header.
// T = float runs the float entry points, T = double (the reference's USE_DOUBLES build, linsys_t = double) their _f64 twins: mpcg_entries<T> names them.
// integrator_type (the reference's INTEGRATOR_TYPE, include/common/integrator.cuh): 0 explicit Euler (default), 1 semi-implicit Euler.  Each stage sets it on
// the handle before its own calls: use_mpcg_generate_kkt and use_mpcg_line_search option "integrator" (give both the same value: the line search must
// measure the map the KKT stage linearised), use_mpcg_simulate_and_shift option "sim_integrator" (the reference's plant is explicit Euler whatever the controller uses).
#ifdef MPCG_H
template <typename T> struct mpcg_entries;
template <> struct mpcg_entries<float> {
    static constexpr auto generate_kkt = &mpcg_generate_kkt;
    static constexpr auto compute_merit = &mpcg_compute_merit;
    static constexpr auto line_search_step = &mpcg_line_search_step;
    static constexpr auto simulate = &mpcg_simulate;
    static constexpr auto advance_horizon = &mpcg_advance_horizon;
};
template <> struct mpcg_entries<double> {
    static constexpr auto generate_kkt = &mpcg_generate_kkt_f64;
    static constexpr auto compute_merit = &mpcg_compute_merit_f64;
    static constexpr auto line_search_step = &mpcg_line_search_step_f64;
    static constexpr auto simulate = &mpcg_simulate_f64;
    static constexpr auto advance_horizon = &mpcg_advance_horizon_f64;
};
template <typename T>
inline void use_mpcg_generate_kkt(mpcg_plant* plant, float qd_cost, float r_cost, unsigned integrator_type = 0) {
    auto& st = stages<T>();
    st.dynmem = plant;
    st.generate_kkt = [qd_cost, r_cost, integrator_type](uint32_t state_size, uint32_t control_size, uint32_t knot_points, T* d_G_dense, T* d_C_dense, T* d_g, T* d_c,
                                         void* d_dynMem_const, float timestep, T* d_eePos_traj, T* d_xs, T* d_xu) {
        mpcg_handle* h = mpcg_compat::handle_for(state_size, knot_points);
        if (mpcg_set_option(h, "integrator", (int)integrator_type) != MPCG_OK) mpcg_compat::die("use_mpcg_generate_kkt: integrator_type", h);
        if (mpcg_entries<T>::generate_kkt(h, static_cast<const mpcg_plant*>(d_dynMem_const), control_size, timestep, d_eePos_traj, d_xs, d_xu, qd_cost, r_cost,
                                          d_G_dense, d_C_dense, d_g, d_c, 1, /*stream*/ nullptr) != MPCG_OK)
            mpcg_compat::die("generate_kkt_submatrices", h);
    };
}

// The library's own line search as the globalize_and_step stage: include/pcg/sqp.cuh:264-353 of the reference over mpcg_compute_merit (the eight
// step sizes alpha = -1 / 2^p in ONE call instead of eight cooperative launches on eight streams) and mpcg_line_search_step (selection :292-301 and
// the saxpy :317, 332-338 on the device), a 4-byte read-back of the chosen exponent, and the drho / rho / rho_max / rho_reset logic of :304-320 with
// the reference's constants (include/common/settings.cuh:185-196).  mu: 10 in the reference (sqp.cuh:51); timestep as handed to sqpSolve*.
// Register a generate_kkt stage FIRST (use_mpcg_generate_kkt): this wraps it to remember the goals and d_xs of the current call, which the
// stage's signature does not carry.  merit_ref is evaluated at the first SQP iteration of a call (sqp.cuh:171-187) and carried afterwards (:352).
// The reference compares the eight trial merits of ls_gato_compute_merit, which include the initial-state term |x_0 - x_s|_1
// (include/common/merit.cuh:68-77), against an initial merit from compute_merit, which leaves it out (:133-135) — two different functions, and a
// step that does not move x_0 can never win by that term.  Here d_xs is passed to all nine evaluations: one function.
template <typename T>
inline void use_mpcg_line_search(float mu, float qd_cost, float r_cost, float timestep, unsigned integrator_type = 0) {
    static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "use_mpcg_line_search: float or double (the _f64 entry points)");
    struct ls_state {
        T *d_goal = nullptr, *d_xs = nullptr;
        T* d_buf = nullptr;              // merit[8], merit_ref, step: ten elements that live as long as the process (the stage table is a static)
        T drho = 1;
    };
    auto s = std::make_shared<ls_state>();
    auto& st = stages<T>();
    require_stage((bool)st.generate_kkt, "generate_kkt (register it before use_mpcg_line_search)");
    auto kkt = st.generate_kkt;
    st.generate_kkt = [s, kkt](uint32_t state_size, uint32_t control_size, uint32_t knot_points, T* d_G_dense, T* d_C_dense, T* d_g, T* d_c,
                               void* d_dynMem_const, float dt, T* d_eePos_traj, T* d_xs, T* d_xu) {
        s->d_goal = d_eePos_traj; s->d_xs = d_xs;
        kkt(state_size, control_size, knot_points, d_G_dense, d_C_dense, d_g, d_c, d_dynMem_const, dt, d_eePos_traj, d_xs, d_xu);
    };
    st.globalize_and_step = [s, mu, qd_cost, r_cost, timestep, integrator_type](uint32_t state_size, uint32_t control_size, uint32_t knot_points, T* d_xu, T* d_dz, T& rho,
                                                                T rho_reset, uint32_t sqp_iter) -> bool {
        const T rho_factor = T(1.2), rho_max = T(10), rho_min = T(1e-3);       // include/common/settings.cuh:185-196
        mpcg_handle* h = mpcg_compat::handle_for(state_size, knot_points);
        const mpcg_plant* plant = static_cast<const mpcg_plant*>(stages<T>().dynmem);
        if (mpcg_set_option(h, "integrator", (int)integrator_type) != MPCG_OK) mpcg_compat::die("use_mpcg_line_search: integrator_type", h);
        if (!s->d_buf && hipMalloc(reinterpret_cast<void**>(&s->d_buf), 10 * sizeof(T)) != hipSuccess) mpcg_compat::die("use_mpcg_line_search: hipMalloc", h);
        T *d_merit = s->d_buf, *d_merit_ref = s->d_buf + 8;
        int32_t* d_step = reinterpret_cast<int32_t*>(s->d_buf + 9);
        T steps[8];
        for (int p = 0; p < 8; ++p) steps[p] = -1.0f / (float)(1 << p);       // alpha sign (include/common/merit.cuh:47)
        if (sqp_iter == 0) {                                                   // (:86, :171-187)
            s->drho = 1;
            const T zero = 0;
            if (mpcg_entries<T>::compute_merit(h, plant, control_size, timestep, s->d_goal, s->d_xs, d_xu, nullptr, &zero, 1, mu, qd_cost, r_cost, d_merit_ref, 1,
                                               /*stream*/ nullptr) != MPCG_OK)
                mpcg_compat::die("compute_merit", h);
        }
        if (mpcg_entries<T>::compute_merit(h, plant, control_size, timestep, s->d_goal, s->d_xs, d_xu, d_dz, steps, 8, mu, qd_cost, r_cost, d_merit, 1, nullptr) != MPCG_OK)
            mpcg_compat::die("ls_gato_compute_merit", h);                      // (:264-282)
        if (mpcg_entries<T>::line_search_step(h, control_size, d_merit, steps, 8, d_merit_ref, d_dz, d_xu, d_step, 1, nullptr) != MPCG_OK)
            mpcg_compat::die("line_search_step", h);                           // (:292-301, :317, :332-338, :352)
        int32_t p = -1;
        if (hipMemcpy(&p, d_step, sizeof(p), hipMemcpyDeviceToHost) != hipSuccess) mpcg_compat::die("use_mpcg_line_search: hipMemcpy", h);
        if (p < 0) {                                                           // line search failure (:304-315)
            s->drho = std::max(s->drho * rho_factor, rho_factor);
            rho = std::max(rho * s->drho, rho_min);
            if (rho > rho_max) { rho = rho_reset; return false; }
            return true;
        }
        s->drho = std::min(s->drho / rho_factor, 1 / rho_factor);              // (:319-320)
        rho = std::max(rho * s->drho, rho_min);
        return true;
    };
}
// The library's own plant simulation and horizon shift as the simulate_and_shift stage: include/mpcsim.cuh:280-352 of the reference over
// mpcg_simulate (simple_simulate: all substeps of a control update in ONE launch) and mpcg_advance_horizon (tracking error, just_shift, tail fills,
// start-state copy on the device), with the reference's host bookkeeping: the plant runs under the PREVIOUS plan (d_xu_old, :288-291) for
// simulation_time = SIMULATION_PERIOD under const_update_freq, else the SQP solve time (:280-284), offset by the previous simulation time
// (prev_simulation_time, :352); time_since_timestep accumulates and the horizon shifts once it passes shift_threshold (SHIFT_THRESHOLD = one
// timestep, include/common/settings.cuh:66-68), `shifted` holding the next shift back until a whole timestep has passed (:297, :343-347).
// One 4-byte read-back per shifting control update: the tracking error the stage returns (updates that do not shift return the last one).
//   d_xu_traj, d_eePos_traj, traj_steps   the precomputed plan simulateMPC was given: traj_steps rows of state_size + control_size / of 6
//   simulation_period_us                  > 0: that constant period (CONST_UPDATE_FREQ); 0: the SQP solve time; < 0: by stages<T>().const_update_freq
//   max_control_updates                   > 0: `done` after that many updates (a demo's bound); 0: only when the plan is used up (:252)
//   xu_fill_lead                          0: the reference's source row of the xu tail (:316); knot_points - 1: the row its goal fill uses
// Needs an mpcg_plant in stages<T>().dynmem (use_mpcg_generate_kkt).
// T = float: mpcg_simulate / mpcg_advance_horizon; T = double: their _f64 twins (mpcg_entries<T>), one body for both.  sim_step is T(2e-4) as
// integrator.cuh:304 has it: with T = double that substep runs ten full substeps and a remainder of almost a whole one per 2,000 us (include/mpcg.h).
template <typename T>
inline void use_mpcg_simulate_and_shift(const T* d_xu_traj, const T* d_eePos_traj, uint32_t traj_steps, float timestep, double simulation_period_us = -1,
                                        uint32_t max_control_updates = 0, uint32_t xu_fill_lead = 0, T sim_step = T(2e-4), unsigned integrator_type = 0) {
    static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "use_mpcg_simulate_and_shift: float or double (the _f64 entry points)");
    struct sim_state {
        T* d_xu_old = nullptr;           // the plan the plant runs under: the previous update's d_xu (:185-192, :291)
        T* d_buf = nullptr;              // eePos[3], tracking error, then traj_offset and done (an int32 in an element's place each): six elements that live as long as the process
        double prev_simulation_time = 0, time_since_timestep = 0;
        bool shifted = false;
        uint32_t traj_offset = 0, updates = 0;
        T tracking_error = 0;
    };
    auto s = std::make_shared<sim_state>();
    auto& st = stages<T>();
    st.simulate_and_shift = [=](uint32_t state_size, uint32_t control_size, uint32_t knot_points, T* d_xs, T* d_xu, T* d_lambda, T* d_eePos_goal,
                                double sqp_solve_time_us, bool& done) -> T {
        mpcg_handle* h = mpcg_compat::handle_for(state_size, knot_points);
        const mpcg_plant* plant = static_cast<const mpcg_plant*>(stages<T>().dynmem);
        const size_t traj_len = (size_t)(state_size + control_size) * knot_points - control_size;
        if (mpcg_set_option(h, "sim_integrator", (int)integrator_type) != MPCG_OK) mpcg_compat::die("use_mpcg_simulate_and_shift: integrator_type", h);
        if (!s->d_buf) {
            if (hipMalloc(reinterpret_cast<void**>(&s->d_buf), 6 * sizeof(T)) != hipSuccess || hipMemset(s->d_buf, 0, 6 * sizeof(T)) != hipSuccess ||
                hipMalloc(reinterpret_cast<void**>(&s->d_xu_old), traj_len * sizeof(T)) != hipSuccess ||
                hipMemcpy(s->d_xu_old, d_xu_traj, traj_len * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess)      // (:192)
                mpcg_compat::die("use_mpcg_simulate_and_shift: hipMalloc", h);
        }
        T *d_eePos = s->d_buf, *d_err = s->d_buf + 3;
        int32_t *d_offset = reinterpret_cast<int32_t*>(s->d_buf + 4), *d_done = reinterpret_cast<int32_t*>(s->d_buf + 5);
        const double period = simulation_period_us < 0 ? (stages<T>().const_update_freq ? (double)SIMULATION_PERIOD : 0.0) : simulation_period_us;
        const double simulation_time = period > 0 ? period : sqp_solve_time_us;                                       // (:280-284)
        if (mpcg_entries<T>::simulate(h, plant, control_size, d_xs, s->d_xu_old, timestep, s->prev_simulation_time, simulation_time, sim_step, d_eePos, 1,
                          /*stream*/ nullptr) != MPCG_OK)
            mpcg_compat::die("simple_simulate", h);                                                                   // (:288)
        if (hipMemcpyAsync(s->d_xu_old, d_xu, traj_len * sizeof(T), hipMemcpyDeviceToDevice, nullptr) != hipSuccess)  // (:291)
            mpcg_compat::die("use_mpcg_simulate_and_shift: hipMemcpy", h);
        s->time_since_timestep += simulation_time * 1e-6;
        const T shift_threshold = 1 * timestep;                                                                      // SHIFT_THRESHOLD
        const bool shift = !s->shifted && s->time_since_timestep > shift_threshold;                                   // (:297)
        if (mpcg_entries<T>::advance_horizon(h, control_size, shift ? 1 : 0, d_xu, d_lambda, d_eePos_goal, d_xs, d_eePos, d_xu_traj, d_eePos_traj, traj_steps, 0,
                                 xu_fill_lead, d_offset, d_done, d_err, 1, nullptr) != MPCG_OK)
            mpcg_compat::die("just_shift", h);                                                                        // (:300-348)
        if (shift) {
            if (hipMemcpy(&s->tracking_error, d_err, sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) mpcg_compat::die("use_mpcg_simulate_and_shift: hipMemcpy", h);
            ++s->traj_offset;
            s->shifted = true;
        }
        if (s->time_since_timestep > timestep) {                                                                      // (:343-347)
            s->shifted = false;
            s->time_since_timestep = std::fmod(s->time_since_timestep, (double)timestep);
        }
        s->prev_simulation_time = simulation_time;                                                                    // (:352)
        ++s->updates;
        done = s->traj_offset >= traj_steps || (max_control_updates && s->updates >= max_control_updates);            // (:252)
        return s->tracking_error;
    };
}
#endif

inline void require_stage(bool present, const char* which) {
    if (!present) {
        fprintf(stderr, "mpcgpu_compat: stage '%s' is not registered (mpcgpu_compat::stages<T>()); it is outside libmpcg_hip's scope\n", which);
        exit(EXIT_FAILURE);             // the reference's error convention: abort
    }
}

}  // namespace mpcgpu_compat
