// sim_advance.inc — the body of advance_horizon_kernel (IO = float) and of advance_horizon_f64_kernel (IO = double), included INSIDE each kernel
// (sim_plant.hip.h) with IO and the argument struct `a` in scope.  Copies only, and the tracking error in IO (tracking_error_of: one rounding per operation).
    const size_t b = blockIdx.x;
    const uint32_t n = a.n, m = a.m, N = a.N, nm = n + m, t = threadIdx.x;
    const size_t len = (size_t)nm * N - m;
    IO* xu = a.xu + b * len;
    const IO* xs = a.xs + b * n;
    if (a.done && a.done[b] != 0) return;                    // frozen (uniform; done is written behind the barriers below)
    if (!a.shift) {                                          // mpcsim.cuh:348 alone
        for (uint32_t e = t; e < n; e += ADV_THREADS) xu[e] = xs[e];
        return;
    }
    IO* lam = a.lambda + b * (size_t)n * N;
    IO* goal = a.goal + b * (size_t)6 * N;
    const IO* xut = a.xu_traj + b * (size_t)a.traj_stride * nm;
    const IO* gt = a.goal_traj + b * (size_t)a.traj_stride * 6;
    const uint32_t off = (uint32_t)a.traj_offset[b] + 1;     // (:310; a value that is no row of the plan takes the else branch and reads the plan's last row)
    const bool inside = off >= 1 && (uint64_t)off + N < a.traj_steps;    // (:314, :327)
    IO err = 0;
    if (t == 0) err = tracking_error_of(a.eePos + b * 3, goal);          // (:303-306) against knot 0 of the unshifted goals
    // xu: x_0 from xs (:348, the last write of the reference); everything else below the last n + m elements from one knot up (just_shift: knots
    // 0..N-3 whole, x_{N-2} <- x_{N-1} without a control, integrator.cuh:258-263); the last n + m elements u_{N-2}, x_{N-1} from the plan (:316) or
    // the final plan position with zero velocity and zero control (:320-322).
    advance_sweep(xu, len, [&](size_t e) -> IO {
        if (e < n) return xs[e];
        if (e + nm < len) return xu[e + nm];
        const uint32_t r = (uint32_t)(e + nm - len);         // 0..m-1: u_{N-2}; m..m+n-1: x_{N-1}
        if (inside) return xut[(size_t)nm * (off + a.lead) - m + r];
        return r >= m && r - m < n / 2 ? xut[(size_t)(a.traj_steps - 1) * nm + (r - m)] : IO(0);
    });
    advance_sweep(goal, (size_t)6 * N, [&](size_t e) -> IO {         // (:326-334)
        if (e + 6 < (size_t)6 * N) return goal[e + 6];
        return gt[(size_t)(inside ? off + N - 1 : a.traj_steps - 1) * 6 + (e + 6 - (size_t)6 * N)];
    });
    advance_sweep(lam, (size_t)n * (N - 1), [&](size_t e) -> IO { return lam[e + n]; });         // the last knot of lambda keeps its value (:337-338)
    if (t == 0) {
        a.tracking_error[b] = err;
        a.traj_offset[b] = (int32_t)off;
        if (off >= a.traj_steps) a.done[b] = 1;              // (:252)
    }
