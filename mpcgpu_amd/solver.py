"""Host-side mirror of the reference's PCG interface, over the C ABI (include/mpcg.h).

Names follow the reference (GBD-PCG as used by include/pcg/sqp.cuh and include/mpcsim.cuh):
`pcg_config` (fields pcg_block, pcg_exit_tol, pcg_max_iter — include/mpcsim.cuh:213-216),
`pcgSharedMemSize` (include/pcg/sqp.cuh:151), `checkPcgOccupancy`
(examples/track_iiwa_pcg.cu:24).  Tensors are torch CUDA tensors used purely as device memory;
all arithmetic happens in libmpcg_hip.so.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import torch

from . import _lib
from .synth import CONTROL_SIZE, STATE_SIZE, pcg_max_iter

PCG_NUM_THREADS = 128   # include/common/settings.cuh:111-113 (reference launch shape; informational)

# per dtype of a call's tensors: the suffix of its C entry and the ctypes scalar of the HOST arrays it takes
_PRECISION = {torch.float32: ("", C.c_float), torch.float64: ("_f64", C.c_double)}
_PRECOND = {"ss": _lib.MPCG_PRECOND_SS, "jacobi": _lib.MPCG_PRECOND_JACOBI, "none": _lib.MPCG_PRECOND_NONE}


def layout(n: int, m: int, N: int) -> dict:
    """Elements per trajectory of the reference's device arrays, by kind (the layouts of synth.py; "csr": include/qdldl/sqp.cuh:148)."""
    return {"bd": 3 * n * n * N,                               # S, Pinv
            "state": n * N,                                    # gamma, lambda, c
            "xu": (n + m) * N - m,                             # xu, g, dz
            "G_dense": (n * n + m * m) * N - m * m,
            "C_dense": (n * n + n * m) * (N - 1),
            "gains": (N - 1) * m * n,                          # K of riccati_gains
            "goals": 6 * N,                                    # eePos_traj of a call, eePos_goal
            "xs": n,
            "eePos": 3,
            "csr": (N - 1) * n * n + N * (n * (n + 1)) // 2,   # nnz of the lower triangle
            "one": 1}


@dataclass
class pcg_config:
    """include/mpcsim.cuh:213-216."""
    pcg_block: int = PCG_NUM_THREADS
    pcg_exit_tol: float = 1e-4
    pcg_max_iter: int = 167


def pcgSharedMemSize(state_size: int, knot_points: int) -> int:
    """Dynamic LDS bytes of one trajectory's workgroup (0 = unsupported shape)."""
    return int(_lib.load().mpcg_pcg_lds_bytes(state_size, knot_points))


def gain_blocks(K: torch.Tensor, n: int, m: int) -> torch.Tensor:
    """The gains of PcgSolver.riccati_gains, flat [B, (N-1) m n] (or [(N-1) m n]) in column-major m x n blocks, as a VIEW [B, N-1, m, n]:
    gain_blocks(K, n, m)[b, k] @ dx is K_k dx of trajectory b.  No copy: the view is strided."""
    B = _batch(K)
    if K.numel() % (B * m * n):
        raise ValueError(f"gain_blocks: {K.numel()} elements are not {B} trajectories of {m} x {n} blocks")
    return K.view(B, -1, n, m).transpose(-1, -2)


def _ptr(t: torch.Tensor | None):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _batch(t: torch.Tensor) -> int:
    """The trajectories of a call, from its leading tensor: [B, ...], or a flat one for a single trajectory."""
    return t.shape[0] if t.dim() > 1 else 1


def _ok(lib, rc, where):
    """MpcgError unless rc is MPCG_OK.  `where`: the handle whose last error is the text, None for the create-time error, or the text itself."""
    if rc != _lib.MPCG_OK:
        raise _lib.MpcgError(rc, where if isinstance(where, str) else lib.mpcg_last_error(where).decode())


class Plant:
    """Device-side robot model for mpcg_generate_kkt: the reference's d_dynMem_const (GRiD robotModel,
    gato_plant::initializeDynamicsConstMem, include/dynamics/iiwa/iiwa_eepos_plant.cuh:63-66) as data.
    `gravity` = (gx, gy, gz): the linear acceleration the chain's root starts from, in the base frame (include/mpcg.h, GRAVITY: GRiD's scalar g is
    (0, 0, g); the physical gravitational acceleration is its negative).  None: (0, 0, 0), the reference's gravity-compensated iiwa.  A plant never
    changes: `with_gravity` returns a new one (mpcg_plant_clone_gravity), and `with_limits` one with soft joint, velocity and torque limits
    (mpcg_plant_clone_limits), which the _xuref entries penalise and simulate may saturate at."""

    def __init__(self, model=None, device: int | None = None, gravity=None):
        import numpy as np
        from . import iiwa
        self.lib = _lib.load()
        self._p = None
        self.model = model or iiwa.Model()
        m = self.model
        dev = torch.cuda.current_device() if device is None else int(device)
        xi = np.array([t[0] for t in m.X_trig], np.int32); xc = np.array([t[1] for t in m.X_trig], np.float64); xj = np.array([t[2] for t in m.X_trig], np.int32)
        hi = np.array([t[0] for t in m.Xhom_trig], np.int32); hc = np.array([t[1] for t in m.Xhom_trig], np.float64); hj = np.array([t[2] for t in m.Xhom_trig], np.int32)
        Icol = np.ascontiguousarray(m.I.transpose(0, 2, 1).reshape(-1))          # back to the column-major table
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        Xc, Hc = np.ascontiguousarray(m.X_const), np.ascontiguousarray(m.Xhom_const)
        h = C.c_void_p()
        _ok(self.lib, self.lib.mpcg_plant_create(C.byref(h), dev, iiwa.NJ, p(Xc), p(Icol), p(Hc), p(xi), p(xc), p(xj), len(xi), p(hi), p(hc), p(hj), len(hi)), None)
        self._p = h
        if gravity is not None:
            heavy = self.with_gravity(gravity)
            self.lib.mpcg_plant_destroy(h)
            self._p, heavy._p = heavy._p, None

    def _clone(self, entry, arg) -> "Plant":
        """A new Plant around what the clone entry `entry` (mpcg_plant_clone_gravity / _limits) makes of this one and `arg`; MpcgError if it refuses."""
        h = C.c_void_p()
        _ok(self.lib, entry(C.byref(h), self._p, arg), None)
        new = object.__new__(Plant)
        new.lib, new.model, new._p = self.lib, self.model, h
        return new

    def with_gravity(self, gravity) -> "Plant":
        """A new Plant: this one's tables with `gravity` (mpcg_plant_clone_gravity); this one is not touched, either may be closed first."""
        g = [float(v) for v in gravity]
        if len(g) != 3:
            raise ValueError("gravity: three components (gx, gy, gz)")
        return self._clone(self.lib.mpcg_plant_clone_gravity, (C.c_double * 3)(*g))

    @property
    def gravity(self):
        out = (C.c_double * 3)()
        _ok(self.lib, self.lib.mpcg_plant_get_gravity(self._p, out), "mpcg_plant_get_gravity")
        return tuple(out)

    @staticmethod
    def _bounds(name, pair):
        """(lo, hi) -> two lists of 7 floats; None: no bound; a scalar broadcasts.  TypeError on anything that is not a pair of None / scalar / 7 numbers."""
        import numpy as np
        if pair is None:
            pair = (None, None)
        if isinstance(pair, (str, bytes)) or not hasattr(pair, "__len__") or len(pair) != 2:
            raise TypeError(f"with_limits: {name} must be a pair (lo, hi) or None")
        out = []
        for side, v in zip((-math.inf, math.inf), pair):
            if v is None:
                out.append([side] * 7)
                continue
            try:
                a = np.asarray(v)
            except (TypeError, ValueError):
                a = np.asarray(None)
            if a.dtype.kind not in "fiu" or a.shape not in ((), (7,)):
                raise TypeError(f"with_limits: a bound of {name} must be None, a number or 7 numbers")
            out.append([float(x) for x in np.broadcast_to(a.astype(np.float64), (7,))])
        return out

    def with_limits(self, q=None, qd=None, u=None, q_weight: float = 0.0, qd_weight: float = 0.0, u_weight: float = 0.0,
                    sim_saturate: bool = False) -> "Plant":
        """A new Plant: this one's tables and gravity with soft limits (mpcg_plant_clone_limits; include/mpcg.h, LIMITS).  q, qd, u = (lo, hi): each side
        None (no bound), a number (every joint) or 7 numbers.  The _xuref entries given the new plant add 1/2 weight viol^2 per bound kind to the cost;
        sim_saturate: simulate clamps the controls it applies to u's bounds.  The plain generate_kkt / compute_merit refuse such a plant."""
        lim = _lib.mpcg_limits()
        for name, pair in (("q", q), ("qd", qd), ("u", u)):
            lo, hi = self._bounds(name, pair)
            setattr(lim, name + "_lo", (C.c_double * 7)(*lo))
            setattr(lim, name + "_hi", (C.c_double * 7)(*hi))
        lim.q_weight, lim.qd_weight, lim.u_weight = float(q_weight), float(qd_weight), float(u_weight)
        lim.flags = _lib.MPCG_LIMITS_SIM_SATURATE if sim_saturate else 0
        return self._clone(self.lib.mpcg_plant_clone_limits, C.byref(lim))

    @property
    def limits(self):
        """None for a plant without limits; otherwise a dict: q, qd, u = (lo, hi) tuples of 7 floats, q_weight, qd_weight, u_weight, sim_saturate."""
        lim, has = _lib.mpcg_limits(), C.c_int(0)
        _ok(self.lib, self.lib.mpcg_plant_get_limits(self._p, C.byref(lim), C.byref(has)), "mpcg_plant_get_limits")
        if not has.value:
            return None
        return {"q": (tuple(lim.q_lo), tuple(lim.q_hi)), "qd": (tuple(lim.qd_lo), tuple(lim.qd_hi)), "u": (tuple(lim.u_lo), tuple(lim.u_hi)),
                "q_weight": lim.q_weight, "qd_weight": lim.qd_weight, "u_weight": lim.u_weight,
                "sim_saturate": bool(lim.flags & _lib.MPCG_LIMITS_SIM_SATURATE)}

    def close(self):
        if getattr(self, "_p", None):
            self.lib.mpcg_plant_destroy(self._p)
            self._p = None

    __del__ = close


@dataclass
class XuRef:
    """The joint-space plan and the weights of the generalised running cost (mpcg_xuref, include/mpcg.h):
        J_k = 1/2 ee_cost |ee(q_k) - goal_k|^2 + 1/2 q_cost |q_k - q_ref|^2 + 1/2 qd_cost |qd_k - [qd_relative] qd_ref|^2 + 1/2 r_cost |u_k - [u_relative] u_ref|^2
    xu_traj: the plan advance_horizon takes — [T, 21] shared by the batch; [B, T, 21] per trajectory; or, with traj_batch_stride = S > 0, [rows, 21] with
    trajectory b's plan starting at row b S (traj_steps, default S, rows of it are the plan; (B - 1) S + traj_steps <= rows);
    traj_offset: int32 [B] on the device or None (= 0), read when the kernel runs: row clamp(traj_offset[b] + k, 0, traj_steps - 1) is knot k's reference."""
    xu_traj: torch.Tensor
    traj_offset: torch.Tensor | None = None
    traj_batch_stride: int = 0
    ee_cost: float = 1.0
    q_cost: float = 0.0
    qd_relative: bool = False
    u_relative: bool = False
    traj_steps: int | None = None


class Clocks:
    """The clock state of B trajectories of an MPC loop on the device (include/mpcsim.cuh:280-352, per trajectory): prev_sim_us (float64 [B],
    prev_simulation_time — what simulate_clk takes as its time offsets), since_s (float64 [B], time_since_timestep) and shifted (int32 [B]).
    A new loop starts from zeros; advance_horizon_clk updates all three in place."""

    def __init__(self, B: int, device="cuda"):
        self.prev_sim_us = torch.zeros(B, dtype=torch.float64, device=device)
        self.since_s = torch.zeros(B, dtype=torch.float64, device=device)
        self.shifted = torch.zeros(B, dtype=torch.int32, device=device)


class QdldlSolver:
    """The reference's LINSYS_SOLVE == 0 path (include/qdldl/sqp.cuh) as a selectable solver: CSR lower-triangle pattern
    (include/utils/csr.cuh:40-73) + elimination tree once, then numeric LDL^T factor + solve per call on the HOST
    (libmpcg_hip's own implementation of the QDLDL algorithm; pure host code, works without a GPU)."""

    def __init__(self, knot_points: int, state_size: int = STATE_SIZE):
        import numpy as np
        self.lib = _lib.load()
        self.n, self.N = int(state_size), int(knot_points)
        h = C.c_void_p()
        _ok(self.lib, self.lib.mpcg_ldl_create(C.byref(h), self.n, self.N), "mpcg_ldl_create")
        self._l = h
        cp, ri = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        nnz, slnz = C.c_uint32(), C.c_uint32()
        self.lib.mpcg_ldl_pattern(self._l, C.byref(cp), C.byref(ri), C.byref(nnz), C.byref(slnz))
        self.nnz, self.sum_lnz = nnz.value, slnz.value
        self.col_ptr = np.ctypeslib.as_array(cp, shape=(self.n * self.N + 1,)).copy()
        self.row_ind = np.ctypeslib.as_array(ri, shape=(self.nnz,)).copy()

    def close(self):
        if getattr(self, "_l", None):
            self.lib.mpcg_ldl_destroy(self._l)
            self._l = None

    __del__ = close

    def solve_host(self, val, gamma):
        """qdldl_solve_schur (include/qdldl/sqp.cuh:22-49) on host arrays: val [nnz] float32, gamma [nN] float32."""
        import numpy as np
        val = np.ascontiguousarray(val, np.float32)
        gamma = np.ascontiguousarray(gamma, np.float32)
        assert val.size == self.nnz and gamma.size == self.n * self.N
        lam = np.empty_like(gamma)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _ok(self.lib, self.lib.mpcg_ldl_solve(self._l, p(val), p(gamma), p(lam)), "mpcg_ldl_solve: zero pivot")
        return lam

    def solve_schur(self, sol: "PcgSolver", d_val, d_gamma, d_lambda):
        """The reference's timed region (include/qdldl/sqp.cuh:268-273): D2H(values, gamma), factor + solve, H2D(lambda)."""
        _ok(self.lib, self.lib.mpcg_qdldl_solve_schur(sol._h, self._l, _ptr(d_val), _ptr(d_gamma), _ptr(d_lambda), _stream()), sol._h)
        return d_lambda


class PcgSolver:
    """One handle per (device, state_size, knot_points).  `solve` is the batched hot path,
    `solve_ref` the reference's single-trajectory 12-argument launch.  `control_size` is the default of
    `form_schur` / `compute_dz` / `generate_kkt` / `compute_merit` / `line_search_step` / `simulate` / `advance_horizon` (None: 7, the IIWA-14's)."""

    def __init__(self, knot_points: int, max_batch: int = 1, state_size: int = STATE_SIZE, device: int | None = None,
                 control_size: int | None = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("mpcgpu_amd.PcgSolver needs a HIP device (no CPU fallback)")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.n, self.N, self.max_batch = int(state_size), int(knot_points), int(max_batch)
        self.control_size = CONTROL_SIZE if control_size is None else int(control_size)
        self._dims_of = (self.control_size, layout(self.n, self.control_size, self.N))
        h = C.c_void_p()
        _ok(self.lib, self.lib.mpcg_create(C.byref(h), self.device, self.n, self.N, self.max_batch), None)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mpcg_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        _ok(self.lib, rc, self._h)

    def set_option(self, key: str, value: int):
        self._check(self.lib.mpcg_set_option(self._h, key.encode(), int(value)))

    def last_error(self) -> str:
        """mpcg_last_error: the text of the handle's last error — or warning (the symmetry latch leaves one)."""
        return self.lib.mpcg_last_error(self._h).decode()

    def get_option(self, key: str) -> int:
        v = C.c_int()
        self._check(self.lib.mpcg_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def checkPcgOccupancy(self) -> int:
        """Number of trajectories resident on the GPU at once (never aborts: no grid sync here)."""
        v = C.c_uint32()
        self._check(self.lib.mpcg_check_pcg_occupancy(self._h, C.byref(v)))
        return v.value

    def _dims(self, control_size=None):
        """(m, the array lengths by kind) of a call: the handle's control_size unless the call names one."""
        m = self.control_size if control_size is None else int(control_size)
        if m != self._dims_of[0]:
            self._dims_of = (m, layout(self.n, m, self.N))
        return self._dims_of

    def _fn(self, base, dt):
        """The C entry mpcg_`base` for float32 tensors, its _f64 twin for float64 ones."""
        return getattr(self.lib, "mpcg_" + base + _PRECISION[dt][0])

    def _chk(self, t, numel, dtype, name):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == dtype and t.numel() == numel):
            raise ValueError(f"{name}: need contiguous cuda {dtype} tensor with {numel} elements, "
                             f"got {tuple(t.shape)} {t.dtype} {t.device}")

    def _chk_each(self, B, L, dtype, arrays, optional=False):
        """_chk of B trajectories of each (tensor, kind of L, name); optional: a None among them is an argument left out."""
        for t, kind, name in arrays:
            if t is not None or not optional:
                self._chk(t, B * L[kind], dtype, name)

    def _out(self, t, shape, dtype, like, name):
        """The caller's output `t`, or a new one of `shape` on the device of `like`; checked either way."""
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=like.device)
        self._chk(t, math.prod(shape), dtype, name)
        return t

    @staticmethod
    def _one_dtype(name, *tensors):
        """float32 or float64, shared by every tensor given (None entries are optional arguments left out): TypeError otherwise."""
        dts = {t.dtype for t in tensors if t is not None}
        if len(dts) != 1 or not dts <= {torch.float32, torch.float64}:
            raise TypeError(f"{name}: the tensors must all be float32 or all be float64, got {sorted(str(d) for d in dts)}")
        return dts.pop()

    def solve(self, S, Pinv, gamma, lam, config: pcg_config | None = None, precond: str = "ss",
              iters: torch.Tensor | None = None, exits: torch.Tensor | None = None):
        """In-place batched solve.  S, Pinv: [B, 3*n*n*N]; gamma, lam: [B, n*N] (lam in/out).
        Returns (iters uint32-as-int32 [B], max_iter_exit uint8 [B]) device tensors; no sync."""
        return self._solve("mpcg_pcg_solve", torch.float32, torch.float32, ("S", "Pinv"), S, Pinv, gamma, lam, config, precond, iters, exits)

    def _solve(self, entry, mat_dt, vec_dt, names, S, Pinv, gamma, lam, config, precond, iters, exits):
        """solve, solve_f16 and solve_f64: the C entry `entry` on matrices of mat_dt, called `names` in a refusal, and vectors of vec_dt."""
        cfg = config or pcg_config(pcg_max_iter=pcg_max_iter(self.N))
        B = _batch(lam)
        L = self._dims_of[1]                                   # the hot path: no call for it, and these two kinds are the same for any m
        self._chk(S, B * L["bd"], mat_dt, names[0])
        self._chk(Pinv, B * L["bd"], mat_dt, names[1])
        self._chk(gamma, B * L["state"], vec_dt, "gamma")
        self._chk(lam, B * L["state"], vec_dt, "lambda")
        if iters is None:
            iters = torch.empty(B, dtype=torch.int32, device=lam.device)
        if exits is None:
            exits = torch.empty(B, dtype=torch.uint8, device=lam.device)
        if precond not in ("ss", "jacobi"):
            raise ValueError("precond must be 'ss' or 'jacobi'")
        _ok(self.lib, getattr(self.lib, entry)(self._h, _ptr(S), _ptr(Pinv), _ptr(gamma), _ptr(lam), B,
                                               int(cfg.pcg_max_iter), float(cfg.pcg_exit_tol), _PRECOND[precond],
                                               _ptr(iters), _ptr(exits), _stream()), self._h)
        return iters, exits

    def to_f16(self, M: torch.Tensor) -> torch.Tensor:
        """Round a bd-layout fp32 matrix buffer to half precision on the device (mpcg_convert_f32_to_f16)."""
        self._chk(M, M.numel(), torch.float32, "M")
        out = torch.empty(M.shape, dtype=torch.float16, device=M.device)
        self._check(self.lib.mpcg_convert_f32_to_f16(self._h, _ptr(M), _ptr(out), M.numel(), _stream()))
        return out

    def solve_f16(self, S16, Pinv16, gamma, lam, config: pcg_config | None = None, precond: str = "ss",
                  iters: torch.Tensor | None = None, exits: torch.Tensor | None = None):
        """`solve` with S / Pinv stored in half precision (arithmetic stays fp32)."""
        return self._solve("mpcg_pcg_solve_f16", torch.float16, torch.float32, ("S16", "Pinv16"), S16, Pinv16, gamma, lam, config, precond, iters, exits)

    def solve_f64(self, S, Pinv, gamma, lam, config: pcg_config | None = None, precond: str = "ss",
                  iters: torch.Tensor | None = None, exits: torch.Tensor | None = None):
        """`solve` in double precision (linsys_t = double, USE_DOUBLES=1 of include/common/settings.cuh:41-49)."""
        return self._solve("mpcg_pcg_solve_f64", torch.float64, torch.float64, ("S", "Pinv"), S, Pinv, gamma, lam, config, precond, iters, exits)

    def solve_ref(self, d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, d_v_temp, d_eta_new_temp,
                  d_pcg_iters, d_pcg_exit, pcg_max_iter: int, pcg_exit_tol: float):
        """The reference kernel's argument list, in order (include/pcg/sqp.cuh:137-150)."""
        self._solve_ref("mpcg_pcg_solve_ref", (d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, d_v_temp, d_eta_new_temp, d_pcg_iters, d_pcg_exit),
                        pcg_max_iter, pcg_exit_tol)

    def _solve_ref(self, entry, arrays, pcg_max_iter, pcg_exit_tol):
        """solve_ref and solve_ref_f64: the C entry `entry` on the ten arrays of the reference's launch, unchecked as there."""
        self._check(getattr(self.lib, entry)(self._h, *map(_ptr, arrays), int(pcg_max_iter), float(pcg_exit_tol), _stream()))

    def solve_ref_f64(self, d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, d_v_temp, d_eta_new_temp,
                      d_pcg_iters, d_pcg_exit, pcg_max_iter: int, pcg_exit_tol: float):
        """The reference kernel's argument list with linsys_t = double (pcg<double, n, N>; include/pcg/sqp.cuh:137-150)."""
        self._solve_ref("mpcg_pcg_solve_ref_f64", (d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, d_v_temp, d_eta_new_temp, d_pcg_iters, d_pcg_exit),
                        pcg_max_iter, pcg_exit_tol)

    def block_solve(self, S, gamma, lam=None):
        """Batched block-tridiagonal direct solve (the GPU counterpart of qdldl_solve_schur,
        include/qdldl/sqp.cuh:22-49).  S: [B, 3*n*n*N], gamma: [B, n*N]; returns lambda [B, n*N].
        float32 tensors: mpcg_block_solve (option "block_solve_f64" = 1: the sweep in double, float in and out);
        float64 tensors: mpcg_block_solve_f64 (linsys_t = double).  Mixed or other dtypes raise TypeError."""
        B = _batch(gamma)
        L = self._dims()[1]
        dt = self._one_dtype("block_solve", S, gamma, lam)
        self._chk_each(B, L, dt, ((S, "bd", "S"), (gamma, "state", "gamma")))
        lam = self._out(lam, (B, L["state"]), dt, gamma, "lambda")
        self._check(self._fn("block_solve", dt)(self._h, _ptr(S), _ptr(gamma), _ptr(lam), B, _stream()))
        return lam

    def riccati_gains(self, G, C, rho, control_size: int | None = None, K=None):
        """The time-varying LQR gains K_k = du_k/dx_k of the regularised LQ subproblem, by a backward Riccati sweep over the KKT blocks
        (mpcg_riccati_gains, include/mpcg_riccati.h).  CALL IT BEFORE form_schur, which overwrites G with its block inverses.
        G: [B, (n^2+m^2)N - m^2] and C: [B, (n^2+nm)(N-1)] as generate_kkt returns them; rho: a Python float, or a device tensor [B] of the
        arrays' dtype (what line_search_step_rho adapts), read when the kernel runs.  Returns K flat [B, (N-1) m n]: `gain_blocks` views it
        as [B, N-1, m, n].  float32 tensors: mpcg_riccati_gains (float64 inside, K rounded once); float64 tensors: mpcg_riccati_gains_f64.
        Mixed dtypes raise TypeError."""
        B = _batch(G)
        m, L = self._dims(control_size)
        rho_t = rho if isinstance(rho, torch.Tensor) else None
        dt = self._one_dtype("riccati_gains", G, C, rho_t, K)
        self._chk_each(B, L, dt, ((G, "G_dense", "G"), (C, "C_dense", "C")))
        if rho_t is not None:
            self._chk(rho_t, B, dt, "rho")
        K = self._out(K, (B, L["gains"]), dt, G, "K")
        self._check(self._fn("riccati_gains", dt)(self._h, m, _ptr(G), _ptr(C), 0.0 if rho_t is not None else float(rho), _ptr(rho_t), _ptr(K), B,
                                                  _stream()))
        return K

    def form_schur(self, G_dense, C_dense, g, c, rho, precond: str = "ss", S=None, Pinv=None, gamma=None,
                   control_size: int | None = None):
        """form_schur_system (include/pcg/linsys_setup.cuh:620-656), batched.  G_dense is overwritten by
        its block inverses (the reference's side effect).  Returns (S, Pinv, gamma) device tensors.
        rho: a Python float (one value for the call), or a device tensor [B] of the operands' dtype — one value per trajectory, read
        when the kernels run (mpcg_form_schur_rhov; what line_search_step_rho adapts)."""
        B = _batch(c)
        m, L = self._dims(control_size)
        dt = self._one_dtype("form_schur", c)                  # of c alone: another tensor of another dtype is a ValueError below
        self._chk_each(B, L, dt, ((G_dense, "G_dense", "G_dense"), (C_dense, "C_dense", "C_dense"), (g, "xu", "g"), (c, "state", "c")))
        S, Pinv, gamma = (self._out(t, (B, L[kind]), dt, c, name) for t, kind, name in ((S, "bd", "S"), (Pinv, "bd", "Pinv"), (gamma, "state", "gamma")))
        pc = _PRECOND[precond]
        if isinstance(rho, torch.Tensor):
            self._chk(rho, B, dt, "rho")
            entry, rho_arg = "form_schur_rhov", _ptr(rho)
        else:
            entry, rho_arg = "form_schur", float(rho)
        self._check(self._fn(entry, dt)(self._h, m, _ptr(G_dense), _ptr(C_dense), _ptr(g), _ptr(c), _ptr(S), _ptr(Pinv), _ptr(gamma), rho_arg, B, pc,
                                        _stream()))
        return S, Pinv, gamma

    def generate_kkt(self, plant: "Plant", eePos_traj, xs, xu, timestep: float, qd_cost: float, r_cost: float,
                     control_size: int | None = None):
        """generate_kkt_submatrices (include/common/kkt.cuh:22-163), batched: eePos_traj [B, 6N], xs [B, n], xu [B, (n+m)N - m]
        -> (G_dense, C_dense, g, c) device tensors in the layouts form_schur consumes.
        float32 tensors: mpcg_generate_kkt; float64 tensors: mpcg_generate_kkt_f64 (linsys_t = double: inputs used as they are, outputs not rounded to
        float).  Mixed dtypes raise TypeError."""
        return self._generate_kkt(False, plant, eePos_traj, xs, xu, timestep, qd_cost, r_cost, None, control_size)

    def _generate_kkt(self, xuref: bool, plant, eePos_traj, xs, xu, timestep, qd_cost, r_cost, ref, control_size):
        """generate_kkt (ref = None) and generate_kkt_xuref (xuref): the C entry of that name or its _f64 twin; only the latter may leave eePos_traj out."""
        name = "generate_kkt_xuref" if xuref else "generate_kkt"
        B = _batch(xu)
        m, L = self._dims(control_size)
        dt = self._one_dtype(name, eePos_traj, xs, xu, *((ref.xu_traj,) if xuref else ()))
        self._chk_each(B, L, dt, ((eePos_traj, "goals", "eePos_traj"),), optional=xuref)
        self._chk_each(B, L, dt, ((xs, "xs", "xs"), (xu, "xu", "xu")))
        x = (C.byref(self._xuref(name, ref, dt, B, self.n, m)),) if xuref else ()
        G, Cd, g, c = (torch.empty(B, L[kind], device=xu.device, dtype=dt) for kind in ("G_dense", "C_dense", "xu", "state"))
        self._check(self._fn(name, dt)(self._h, plant._p, m, float(timestep), _ptr(eePos_traj), _ptr(xs), _ptr(xu), float(qd_cost), float(r_cost), *x,
                                       _ptr(G), _ptr(Cd), _ptr(g), _ptr(c), B, _stream()))
        return G, Cd, g, c

    def _xuref(self, name, ref: "XuRef", dt, B, n, m):
        """The mpcg_xuref of a call over B trajectories of dtype dt."""
        t = ref.xu_traj
        if t.dtype != dt:
            raise TypeError(f"{name}: xu_traj must have the dtype of the other tensors ({dt}), got {t.dtype}")
        stride = int(ref.traj_batch_stride)
        self._chk(t, t.numel(), dt, "xu_traj")
        if t.numel() % (n + m):
            raise ValueError(f"{name}: xu_traj must hold rows of {n + m} values")
        rows = t.numel() // (n + m)
        if t.dim() == 3:                                       # [B, T, 21]: a plan per trajectory
            if stride not in (0, int(t.shape[-2])) or int(t.shape[0]) != B:
                raise ValueError(f"{name}: a [B, T, 21] plan has B trajectories and traj_batch_stride T")
            stride = int(t.shape[-2])
        T = int(ref.traj_steps) if ref.traj_steps is not None else (stride if stride else rows)
        if T < 1 or (stride and stride < T) or (B - 1) * stride + T > rows:
            raise ValueError(f"{name}: xu_traj holds {rows} rows, fewer than (B - 1) traj_batch_stride + traj_steps, or traj_batch_stride < traj_steps")
        if ref.traj_offset is not None:
            self._chk(ref.traj_offset, B, torch.int32, "traj_offset")
        flags = (_lib.MPCG_XUREF_QD_RELATIVE if ref.qd_relative else 0) | (_lib.MPCG_XUREF_U_RELATIVE if ref.u_relative else 0)
        return _lib.mpcg_xuref(t.data_ptr(), T, stride, ref.traj_offset.data_ptr() if ref.traj_offset is not None else None,
                               float(ref.ee_cost), float(ref.q_cost), flags)

    def generate_kkt_xuref(self, plant: "Plant", eePos_traj, xs, xu, timestep: float, qd_cost: float, r_cost: float, ref: "XuRef",
                           control_size: int | None = None):
        """generate_kkt with the generalised running cost of `ref` (mpcg_generate_kkt_xuref; float64 tensors: mpcg_generate_kkt_xuref_f64): the same
        layouts, C and c.  eePos_traj may be None exactly when ref.ee_cost == 0.  Mixed dtypes raise TypeError."""
        return self._generate_kkt(True, plant, eePos_traj, xs, xu, timestep, qd_cost, r_cost, ref, control_size)

    def compute_merit_xuref(self, plant: "Plant", eePos_traj, xs, xu, dz, step_sizes, timestep: float, mu: float, qd_cost: float, r_cost: float,
                            ref: "XuRef", merit=None, control_size: int | None = None):
        """compute_merit with the generalised running cost of `ref` (mpcg_compute_merit_xuref; float64 tensors: mpcg_compute_merit_xuref_f64); what
        line_search_step(_rho) consumes.  eePos_traj may be None exactly when ref.ee_cost == 0.  Mixed dtypes raise TypeError."""
        return self._compute_merit(True, plant, eePos_traj, xs, xu, dz, step_sizes, timestep, mu, qd_cost, r_cost, ref, merit, control_size)

    def compute_dz(self, Ginv_dense, C_dense, g, lam, dz=None, control_size: int | None = None):
        """compute_dz (include/common/dz.cuh:124-136), batched."""
        B = _batch(lam)
        m, L = self._dims(control_size)
        dt = self._one_dtype("compute_dz", lam)                # of lam alone: another tensor of another dtype is a ValueError below
        self._chk_each(B, L, dt, ((Ginv_dense, "G_dense", "Ginv_dense"), (C_dense, "C_dense", "C_dense"), (g, "xu", "g"), (lam, "state", "lam")))
        dz = self._out(dz, (B, L["xu"]), dt, lam, "dz")
        self._check(self._fn("compute_dz", dt)(self._h, m, _ptr(Ginv_dense), _ptr(C_dense), _ptr(g), _ptr(lam), _ptr(dz), B, _stream()))
        return dz

    @staticmethod
    def _steps(step_sizes, dtype=torch.float32):
        """The HOST array of step sizes both line-search calls take (copied into the launch): floats, or doubles for the _f64 entries."""
        vals = [float(v) for v in step_sizes]
        return (_PRECISION[dtype][1] * len(vals))(*vals), len(vals)

    def compute_merit(self, plant: "Plant", eePos_traj, xs, xu, dz, step_sizes, timestep: float, mu: float, qd_cost: float,
                      r_cost: float, merit=None, control_size: int | None = None):
        """ls_gato_compute_merit / compute_merit (include/common/merit.cuh:16-143), batched over trajectories and step sizes:
        merit [B, A] float of the trial iterates xu + step_sizes[a] * dz.  xs = None: no initial-state term (the reference's compute_merit);
        dz = None is allowed when every step size is 0.
        float32 tensors: mpcg_compute_merit; float64 tensors: mpcg_compute_merit_f64 (the trial iterate and the merits in double, the step sizes
        marshalled as doubles).  Mixed dtypes raise TypeError."""
        return self._compute_merit(False, plant, eePos_traj, xs, xu, dz, step_sizes, timestep, mu, qd_cost, r_cost, None, merit, control_size)

    def _compute_merit(self, xuref: bool, plant, eePos_traj, xs, xu, dz, step_sizes, timestep, mu, qd_cost, r_cost, ref, merit, control_size):
        """compute_merit (ref = None) and compute_merit_xuref (xuref): the C entry of that name or its _f64 twin; only the latter may leave eePos_traj out."""
        name = "compute_merit_xuref" if xuref else "compute_merit"
        B = _batch(xu)
        m, L = self._dims(control_size)
        dt = self._one_dtype(name, eePos_traj, xs, xu, dz, merit, *((ref.xu_traj,) if xuref else ()))
        arr, A = self._steps(step_sizes, dt)
        self._chk_each(B, L, dt, ((eePos_traj, "goals", "eePos_traj"),), optional=xuref)
        self._chk(xu, B * L["xu"], dt, "xu")
        self._chk_each(B, L, dt, ((xs, "xs", "xs"), (dz, "xu", "dz")), optional=True)
        x = (C.byref(self._xuref(name, ref, dt, B, self.n, m)),) if xuref else ()
        merit = self._out(merit, (B, A), dt, xu, "merit")
        self._check(self._fn(name, dt)(self._h, plant._p, m, float(timestep), _ptr(eePos_traj), _ptr(xs), _ptr(xu), _ptr(dz), arr, A,
                                       float(mu), float(qd_cost), float(r_cost), *x, _ptr(merit), B, _stream()))
        return merit

    def line_search_step(self, merit, step_sizes, merit_ref, dz, xu, step=None, control_size: int | None = None):
        """The step selection and update of include/pcg/sqp.cuh:292-301, 317, 332-338, 352 per trajectory: the first strictly smallest merit below
        merit_ref wins; xu and merit_ref are updated in place.  Returns the chosen index per trajectory (int32 [B], -1: no step).
        float32 tensors: mpcg_line_search_step; float64 tensors: mpcg_line_search_step_f64.  Mixed dtypes raise TypeError."""
        return self._line_search("line_search_step", merit, step_sizes, merit_ref, dz, xu, step, control_size)

    def _line_search(self, name, merit, step_sizes, merit_ref, dz, xu, step, control_size, rho=(), params=()):
        """line_search_step, and line_search_step_rho with its device state rho = (rho, drho, done) and its four scalars `params`."""
        B = merit_ref.numel()
        m, L = self._dims(control_size)
        dt = self._one_dtype(name, merit, merit_ref, dz, xu, *rho[:2])
        arr, A = self._steps(step_sizes, dt)
        self._chk(merit, B * A, dt, "merit")
        self._chk_each(B, L, dt, ((merit_ref, "one", "merit_ref"), (dz, "xu", "dz"), (xu, "xu", "xu")))
        if rho:
            self._chk_each(B, L, dt, ((rho[0], "one", "rho"), (rho[1], "one", "drho")))
            self._chk(rho[2], B, torch.uint8, "done")
        step = self._out(step, (B,), torch.int32, xu, "step")
        self._check(self._fn(name, dt)(self._h, m, _ptr(merit), arr, A, _ptr(merit_ref), _ptr(dz), _ptr(xu), _ptr(step), *map(_ptr, rho),
                                       *map(float, params), B, _stream()))
        return step

    def line_search_step_rho(self, merit, step_sizes, merit_ref, dz, xu, rho, drho, done, rho_factor: float = 1.2, rho_min: float = 1e-3,
                             rho_max: float = 10.0, rho_reset: float = 1e-3, step=None, control_size: int | None = None):
        """line_search_step followed by the rho adaptation of include/pcg/sqp.cuh:304-320 with device state per trajectory: rho, drho (float32
        [B]) and done (uint8 [B]) are updated in place; a trajectory with done != 0 is frozen (step = MPCG_STEP_FROZEN, nothing else written).
        `rho` is the tensor form_schur takes: nothing is read back inside an SQP loop.
        float32 tensors: mpcg_line_search_step_rho; float64 tensors (rho and drho float64 too): mpcg_line_search_step_rho_f64.  Mixed dtypes raise TypeError."""
        return self._line_search("line_search_step_rho", merit, step_sizes, merit_ref, dz, xu, step, control_size, (rho, drho, done),
                                 (rho_factor, rho_min, rho_max, rho_reset))

    def simulate(self, plant: "Plant", xs, xu, timestep: float, time_offset_us: float, sim_time_us: float, sim_step: float = 2e-4,
                 eePos=None, control_size: int | None = None):
        """simple_simulate (include/common/integrator.cuh:295-325), batched, one launch for all substeps: the plant states xs [B, n] are
        integrated in place over sim_time_us under the controls of the plan xu [B, (n+m)N - m], starting time_offset_us into it.
        eePos (optional, [B, 3]) receives the end-effector position of the new state — what advance_horizon(shift=1) takes.
        float32 tensors: mpcg_simulate (sim_step is rounded to float).  float64 tensors: mpcg_simulate_f64 — the inputs used as they are, the state
        stored without a rounding, sim_step a double: at the default 2e-4 the reference's double schedule runs ten substeps AND a remainder of
        almost a whole one per 2,000 us (include/mpcg.h); pass float(numpy.float32(2e-4)) for the float entry's ten.  Mixed dtypes raise TypeError."""
        return self._simulate("simulate", plant, xs, xu, timestep, (time_offset_us, sim_time_us), sim_step, eePos, (), control_size)

    def _simulate(self, name, plant, xs, xu, timestep, times, sim_step, eePos, done, control_size):
        """simulate (times: two numbers, done = ()) and simulate_clk (times: two float64 [B] tensors, done = (done,))."""
        on_device = name == "simulate_clk"
        B = _batch(xs)
        m, L = self._dims(control_size)
        dt = self._one_dtype(name, xs, xu, eePos)
        self._chk_each(B, L, dt, ((xs, "xs", "xs"), (xu, "xu", "xu")))
        if on_device:
            self._chk_each(B, L, torch.float64, ((times[0], "one", "time_offset_us"), (times[1], "one", "sim_time_us")))
        self._chk_each(B, L, dt, ((eePos, "eePos", "eePos"),), optional=True)
        self._chk_each(B, L, torch.int32, [(t, "one", "done") for t in done], optional=True)
        self._check(self._fn(name, dt)(self._h, plant._p, m, _ptr(xs), _ptr(xu), float(timestep), *map(_ptr if on_device else float, times),
                                       float(sim_step), _ptr(eePos), *map(_ptr, done), B, _stream()))
        return xs

    def inverse_dynamics(self, plant: "Plant", q, qd=None, qdd=None, tau=None):
        """tau = ID(q, qd, qdd) of the plant, its gravity included, for q [count, 7] (qd, qdd: None = 0; both None: the gravity torques), in the dtype
        of q.  float32 tensors: mpcg_inverse_dynamics (float64 inside, rounded once); float64 tensors: mpcg_inverse_dynamics_f64.  count is at most
        max_batch x knot_points.  Mixed dtypes raise TypeError."""
        dt = self._one_dtype("inverse_dynamics", q, qd, qdd, tau)
        if q.numel() % 7:
            raise ValueError("inverse_dynamics: q must hold [count, 7] values")
        count = q.numel() // 7
        self._chk(q, count * 7, dt, "q")
        for t, name in ((qd, "qd"), (qdd, "qdd")):
            if t is not None:
                self._chk(t, count * 7, dt, name)
        tau = self._out(tau, (count, 7), dt, q, "tau")
        self._check(self._fn("inverse_dynamics", dt)(self._h, plant._p, _ptr(q), _ptr(qd), _ptr(qdd), _ptr(tau), count, _stream()))
        return tau

    def _chk_shift(self, name, B, L, dt, m, lam, eePos_goal, eePos, xu_traj, eePos_traj, traj_offset, done, tracking_error, need_eePos):
        """What a shift reads and writes besides xu and xs: ValueError naming the first array that is missing (eePos only if need_eePos) or is
        not what B trajectories need; returns the plan's (traj_steps, traj_batch_stride)."""
        given = {"lam": lam, "eePos_goal": eePos_goal, "xu_traj": xu_traj, "eePos_traj": eePos_traj, "traj_offset": traj_offset, "done": done,
                 "tracking_error": tracking_error}
        if need_eePos or eePos is not None:
            given["eePos"] = eePos
        for arg, t in given.items():
            if t is None:
                raise ValueError(f"{name} needs {arg}")
        per_traj, T = xu_traj.dim() == 3, int(xu_traj.shape[-2])
        plans = B if per_traj else 1
        count = {"lam": B * L["state"], "eePos_goal": B * L["goals"], "eePos": B * L["eePos"], "xu_traj": plans * T * (self.n + m),
                 "eePos_traj": plans * T * 6}
        for arg, t in given.items():
            self._chk(t, count.get(arg, B), torch.int32 if arg in ("traj_offset", "done") else dt, arg)
        return T, (T if per_traj else 0)

    def advance_horizon(self, shift: bool, xu, xs, lam=None, eePos_goal=None, eePos=None, xu_traj=None, eePos_traj=None, traj_offset=None,
                        done=None, tracking_error=None, xu_fill_lead: int = 0, control_size: int | None = None):
        """The rest of a control update (include/mpcsim.cuh:300-348) per trajectory.  shift=False: xu[:, :n] = xs only.  shift=True: tracking error,
        traj_offset += 1, the one-knot shift of xu / eePos_goal / lam with their tails refilled from the plan, then the start-state copy; done
        (int32 [B]) is set when a trajectory has used up its plan, and a trajectory with done != 0 on entry is frozen.
        The plan: xu_traj [T, n+m] and eePos_traj [T, 6] shared by the batch, or [B, T, n+m] and [B, T, 6] per trajectory.
        xu_fill_lead: 0 = the reference's source row of the xu tail, N - 1 = the row its goal fill uses.
        float32 tensors: mpcg_advance_horizon; float64 tensors: mpcg_advance_horizon_f64 (the copies and the tracking error in double).  traj_offset and
        done are int32 for both.  Mixed dtypes raise TypeError."""
        B = _batch(xs)
        m, L = self._dims(control_size)
        dt = self._one_dtype("advance_horizon", xu, xs, lam, eePos_goal, eePos, xu_traj, eePos_traj, tracking_error)
        self._chk_each(B, L, dt, ((xu, "xu", "xu"), (xs, "xs", "xs")))
        T = stride = 0
        if shift:
            T, stride = self._chk_shift("advance_horizon(shift=True)", B, L, dt, m, lam, eePos_goal, eePos, xu_traj, eePos_traj, traj_offset, done,
                                        tracking_error, False)
        elif done is not None:
            self._chk(done, B, torch.int32, "done")
        self._check(self._fn("advance_horizon", dt)(self._h, m, 1 if shift else 0, _ptr(xu), _ptr(lam), _ptr(eePos_goal), _ptr(xs), _ptr(eePos),
                                                    _ptr(xu_traj), _ptr(eePos_traj), T, stride, int(xu_fill_lead), _ptr(traj_offset), _ptr(done),
                                                    _ptr(tracking_error), B, _stream()))
        return xu

    def simulate_clk(self, plant: "Plant", xs, xu, timestep: float, time_offset_us, sim_time_us, sim_step: float = 2e-4, eePos=None, done=None,
                     control_size: int | None = None):
        """simulate with the times on the device: time_offset_us and sim_time_us are float64 [B] tensors, and trajectory b gets what simulate gives it
        with its own pair, bit for bit.  done (optional, int32 [B]): a trajectory with done != 0 is frozen (nothing of it is written); one whose times
        are no schedule (non-finite, negative, more than MPCG_SIM_MAX_SUBSTEPS substeps) is not simulated and gets done = MPCG_DONE_BAD_CLOCK.
        A loop passes Clocks.prev_sim_us as time_offset_us.  float32 tensors: mpcg_simulate_clk; float64: mpcg_simulate_clk_f64.  Mixed dtypes raise TypeError."""
        return self._simulate("simulate_clk", plant, xs, xu, timestep, (time_offset_us, sim_time_us), sim_step, eePos, (done,), control_size)

    def advance_horizon_clk(self, xu, xs, lam, eePos_goal, eePos, xu_traj, eePos_traj, traj_offset, done, tracking_error, timestep: float, sim_time_us,
                            clocks: Clocks, did_shift=None, shift_threshold_s: float | None = None, xu_fill_lead: int = 0, control_size: int | None = None):
        """advance_horizon with the shift decided per trajectory on the device from `clocks` (include/mpcsim.cuh:294-352): since += sim_time_us * 1e-6;
        a trajectory shifts when it has not yet shifted in this timestep and since > shift_threshold_s (default: the reference's, one timestep rounded
        to the tensors' dtype); since wraps at the timestep; prev_sim_us = sim_time_us.  sim_time_us: float64 [B]; did_shift (optional, int32 [B])
        receives the decisions.  A frozen trajectory keeps its clock; a non-finite or negative time sets done = MPCG_DONE_BAD_CLOCK.  Every array of
        advance_horizon(shift=True) is required.  float32 tensors: mpcg_advance_horizon_clk; float64: mpcg_advance_horizon_clk_f64.  Mixed dtypes raise TypeError."""
        B = _batch(xs)
        m, L = self._dims(control_size)
        dt = self._one_dtype("advance_horizon_clk", xu, xs, lam, eePos_goal, eePos, xu_traj, eePos_traj, tracking_error)
        self._chk_each(B, L, dt, ((xu, "xu", "xu"), (xs, "xs", "xs")))
        T, stride = self._chk_shift("advance_horizon_clk", B, L, dt, m, lam, eePos_goal, eePos, xu_traj, eePos_traj, traj_offset, done, tracking_error, True)
        self._chk(clocks.shifted, B, torch.int32, "clocks.shifted")
        self._chk_each(B, L, torch.int32, ((did_shift, "one", "did_shift"),), optional=True)
        self._chk_each(B, L, torch.float64, ((sim_time_us, "one", "sim_time_us"), (clocks.prev_sim_us, "one", "clocks.prev_sim_us"),
                                             (clocks.since_s, "one", "clocks.since_s")))
        if shift_threshold_s is None:
            shift_threshold_s = float(torch.tensor(1 * timestep, dtype=dt))
        self._check(self._fn("advance_horizon_clk", dt)(self._h, m, _ptr(xu), _ptr(lam), _ptr(eePos_goal), _ptr(xs), _ptr(eePos), _ptr(xu_traj),
                                                        _ptr(eePos_traj), T, stride, int(xu_fill_lead), _ptr(traj_offset), _ptr(done), _ptr(tracking_error),
                                                        float(timestep), float(shift_threshold_s), _ptr(sim_time_us), _ptr(clocks.prev_sim_us),
                                                        _ptr(clocks.since_s), _ptr(clocks.shifted), _ptr(did_shift), B, _stream()))
        return xu

    def csr_nnz(self) -> int:
        """nnz of the lower triangle (include/qdldl/sqp.cuh:148)."""
        return self._dims()[1]["csr"]

    def prep_csr(self):
        """prep_csr (include/utils/csr.cuh:40-73): (col_ptr int32 [nN+1], row_ind int32 [nnz]) on the device."""
        dev = torch.device("cuda", self.device)
        col_ptr = torch.empty(self.n * self.N + 1, dtype=torch.int32, device=dev)
        row_ind = torch.empty(self.csr_nnz(), dtype=torch.int32, device=dev)
        self._check(self.lib.mpcg_prep_csr(self._h, _ptr(col_ptr), _ptr(row_ind), _stream()))
        return col_ptr, row_ind

    def bd_to_csr_lowertri(self, S, mult: float = 1.0):
        """Values of the QDLDL path's d_val from a bd-layout S, batched: [B, nnz]."""
        B = _batch(S)
        self._chk(S, B * self._dims()[1]["bd"], torch.float32, "S")
        val = torch.empty(B, self.csr_nnz(), device=S.device)
        self._check(self.lib.mpcg_bd_to_csr_lowertri(self._h, _ptr(S), _ptr(val), float(mult), B, _stream()))
        return val

    def probe_hbm_read(self, src, sink=None):
        """Pure read of `src` (measurement aid: the device's HBM read ceiling, mpcg_probe_hbm_read)."""
        if sink is None:
            sink = torch.zeros(1, dtype=torch.float32, device=src.device)
        nbytes = src.numel() * src.element_size()
        self._check(self.lib.mpcg_probe_hbm_read(self._h, _ptr(src), nbytes - nbytes % 16, _ptr(sink), _stream()))
        return sink

    def bt_spmv(self, M, x, y=None, cols: int = 3):
        B = _batch(x)
        self._chk_each(B, self._dims()[1], torch.float32, ((M, "bd", "M"), (x, "state", "x")))
        if y is None:
            y = torch.empty_like(x)
        self._check(self.lib.mpcg_bt_spmv(self._h, _ptr(M), _ptr(x), _ptr(y), B, int(cols), _stream()))
        return y
