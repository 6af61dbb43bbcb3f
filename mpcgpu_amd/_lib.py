"""ctypes binding of the C ABI declared in include/mpcg.h and include/mpcg_riccati.h.

The library is the product: if it is missing or does not load, importing fails loudly —
there is no Python/CPU fallback for any compute entry point.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmpcg_hip.so")

MPCG_OK = 0
MPCG_ERR_INVALID = -1
MPCG_ERR_UNSUPPORTED = -2
MPCG_ERR_HIP = -3
MPCG_ERR_NOMEM = -4
MPCG_PRECOND_NONE = 0
MPCG_PRECOND_JACOBI = 1
MPCG_PRECOND_SS = 3
MPCG_MAX_STEP_SIZES = 16
MPCG_STEP_FROZEN = -2
MPCG_SIM_MAX_SUBSTEPS = 65536
MPCG_DONE_BAD_CLOCK = 2
MPCG_XUREF_QD_RELATIVE = 1
MPCG_XUREF_U_RELATIVE = 2
MPCG_LIMITS_SIM_SATURATE = 1


class mpcg_xuref(C.Structure):
    """The HOST struct of the _xuref entries (include/mpcg.h), copied into the launch."""
    _fields_ = [("d_xu_traj", C.c_void_p), ("traj_steps", C.c_uint32), ("traj_batch_stride", C.c_uint32), ("d_traj_offset", C.c_void_p),
                ("ee_cost", C.c_double), ("q_cost", C.c_double), ("flags", C.c_uint32)]


class mpcg_limits(C.Structure):
    """The soft limits of a plant (include/mpcg.h, LIMITS): -inf / +inf = no bound on that side."""
    _fields_ = [("q_lo", C.c_double * 7), ("q_hi", C.c_double * 7), ("qd_lo", C.c_double * 7), ("qd_hi", C.c_double * 7),
                ("u_lo", C.c_double * 7), ("u_hi", C.c_double * 7),
                ("q_weight", C.c_double), ("qd_weight", C.c_double), ("u_weight", C.c_double), ("flags", C.c_uint32)]


# every symbol include/mpcg.h declares: name -> (restype, argtypes); tests/test_abi.py holds each row against the header's prototype.
# Device pointers travel as integers (_p).  An entry with an _f64 twin is ONE row of _pair: _T stands for the entry's scalar type (float, and
# double in the twin) and _TP for a HOST pointer to it; what is double in both twins (timestep, the _us times, mpcg_xuref, mpcg_limits) stays _d.
_p, _u32, _int, _d, _T, _TP = C.c_void_p, C.c_uint32, C.c_int, C.c_double, "T", "T*"


def _pair(name, args):
    """The rows of the entry `name` and of `name`_f64 (both return int)."""
    rows = {}
    for suffix, T in (("", C.c_float), ("_f64", C.c_double)):
        rows[name + suffix] = (_int, [T if a is _T else C.POINTER(T) if a is _TP else a for a in args])
    return rows


SYMBOLS = {
    "mpcg_abi_version": (_int, []),
    "mpcg_build_info": (C.c_char_p, []),
    "mpcg_create": (_int, [C.POINTER(_p), _int, _u32, _u32, _u32]),
    "mpcg_destroy": (_int, [_p]),
    "mpcg_last_error": (C.c_char_p, [_p]),
    "mpcg_pcg_lds_bytes": (C.c_size_t, [_u32, _u32]),
    "mpcg_pcg_lds_bytes_f64": (C.c_size_t, [_u32, _u32]),
    "mpcg_check_pcg_occupancy": (_int, [_p, C.POINTER(_u32)]),
    **_pair("mpcg_pcg_solve", [_p, _p, _p, _p, _p, _u32, _u32, _T, _int, _p, _p, _p]),
    **_pair("mpcg_pcg_solve_ref", [_p] * 11 + [_u32, _T, _p]),
    "mpcg_pcg_solve_f16": (_int, [_p, _p, _p, _p, _p, _u32, _u32, C.c_float, _int, _p, _p, _p]),
    "mpcg_bt_spmv": (_int, [_p, _p, _p, _p, _u32, _int, _p]),
    "mpcg_probe_hbm_read": (_int, [_p, _p, C.c_size_t, _p, _p]),
    "mpcg_convert_f32_to_f16": (_int, [_p, _p, _p, C.c_size_t, _p]),
    **_pair("mpcg_form_schur", [_p, _u32, _p, _p, _p, _p, _p, _p, _p, _T, _u32, _int, _p]),
    **_pair("mpcg_form_schur_rhov", [_p, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _u32, _int, _p]),
    **_pair("mpcg_compute_dz", [_p, _u32, _p, _p, _p, _p, _p, _u32, _p]),
    **_pair("mpcg_block_solve", [_p, _p, _p, _p, _u32, _p]),
    "mpcg_prep_csr": (_int, [_p, _p, _p, _p]),
    "mpcg_bd_to_csr_lowertri": (_int, [_p, _p, _p, C.c_float, _u32, _p]),
    "mpcg_plant_create": (_int, [C.POINTER(_p), _int, _u32, _p, _p, _p, _p, _p, _p, _u32, _p, _p, _p, _u32]),
    "mpcg_plant_create_iiwa14": (_int, [C.POINTER(_p), _int]),
    "mpcg_plant_clone_gravity": (_int, [C.POINTER(_p), _p, C.POINTER(_d)]),
    "mpcg_plant_get_gravity": (_int, [_p, C.POINTER(_d)]),
    "mpcg_plant_clone_limits": (_int, [C.POINTER(_p), _p, C.POINTER(mpcg_limits)]),
    "mpcg_plant_get_limits": (_int, [_p, C.POINTER(mpcg_limits), C.POINTER(_int)]),
    "mpcg_plant_destroy": (_int, [_p]),
    **_pair("mpcg_inverse_dynamics", [_p, _p, _p, _p, _p, _p, _u32, _p]),
    **_pair("mpcg_generate_kkt", [_p, _p, _u32, _T, _p, _p, _p, _T, _T, _p, _p, _p, _p, _u32, _p]),
    **_pair("mpcg_generate_kkt_xuref", [_p, _p, _u32, _T, _p, _p, _p, _T, _T, C.POINTER(mpcg_xuref), _p, _p, _p, _p, _u32, _p]),
    **_pair("mpcg_compute_merit", [_p, _p, _u32, _T, _p, _p, _p, _p, _TP, _u32, _T, _T, _T, _p, _u32, _p]),
    **_pair("mpcg_compute_merit_xuref", [_p, _p, _u32, _T, _p, _p, _p, _p, _TP, _u32, _T, _T, _T, C.POINTER(mpcg_xuref), _p, _u32, _p]),
    **_pair("mpcg_line_search_step", [_p, _u32, _p, _TP, _u32, _p, _p, _p, _p, _u32, _p]),
    **_pair("mpcg_line_search_step_rho", [_p, _u32, _p, _TP, _u32, _p, _p, _p, _p, _p, _p, _p, _T, _T, _T, _T, _u32, _p]),
    **_pair("mpcg_simulate", [_p, _p, _u32, _p, _p, _d, _d, _d, _T, _p, _u32, _p]),
    **_pair("mpcg_simulate_clk", [_p, _p, _u32, _p, _p, _d, _p, _p, _T, _p, _p, _u32, _p]),
    **_pair("mpcg_advance_horizon", [_p, _u32, _u32, _p, _p, _p, _p, _p, _p, _p, _u32, _u32, _u32, _p, _p, _p, _u32, _p]),
    **_pair("mpcg_advance_horizon_clk", [_p, _u32, _p, _p, _p, _p, _p, _p, _p, _u32, _u32, _u32, _p, _p, _p, _d, _d, _p, _p, _p, _p, _p, _u32, _p]),
    "mpcg_ldl_create": (_int, [C.POINTER(_p), _u32, _u32]),
    "mpcg_ldl_destroy": (_int, [_p]),
    "mpcg_ldl_pattern": (_int, [_p, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32)), C.POINTER(_u32), C.POINTER(_u32)]),
    "mpcg_ldl_solve": (_int, [_p, _p, _p, _p]),
    "mpcg_qdldl_solve_schur": (_int, [_p, _p, _p, _p, _p, _p]),
    "mpcg_set_option": (_int, [_p, C.c_char_p, _int]),
    "mpcg_get_option": (_int, [_p, C.c_char_p, C.POINTER(_int)]),
}

# the second table, include/mpcg_riccati.h (tests/test_riccati_ref_cpu.py holds each row against that header's prototype)
SYMBOLS_RICCATI = {
    **_pair("mpcg_riccati_gains", [_p, _u32, _p, _p, _T, _p, _p, _u32, _p]),
}

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m mpcgpu_amd.build` "
                "(hipcc --offload-arch=gfx950).  mpcgpu_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in {**SYMBOLS, **SYMBOLS_RICCATI}.items():
            fn = getattr(lib, name)      # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class MpcgError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__(f"mpcg error {code}: {text}")
        self.code = code
