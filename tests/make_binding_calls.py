"""Generates tests/golden/binding_calls.json: what the Python binding (mpcgpu_amd/solver.py over mpcgpu_amd/_lib.py) hands to the C ABI, call by call.
Run on the GPU box: `python tests/make_binding_calls.py [--out PATH] [--force]` (an existing table is kept unless --force is given).
tests/test_gpu_binding_calls.py records the same table again and compares exactly.

While it records, _lib.load() returns a proxy of the library that logs every C call — the entry's name and each argument in a normal form — and
forwards it.  The normal form of an argument:
  a pointer        the label of the case's tensor whose data_ptr() it is, "null", "handle" / "plant" / "ldl" (an object the library made), "stream"
                   (the cases run on a side stream, so the stream is no null pointer) or "fresh" (memory the wrapper allocated; host arrays too);
  an int           itself; a float: float.hex(); bytes: "b:" + the text;
  a ctypes array   {"array": element type, "values": [...]};
  byref(struct)    {"struct": type, "fields": {...}}, each field normalised the same way; byref of anything else: "out:" + its type.
Per case the table holds the C calls and what the method returned — dtype, shape and label of a tensor ("fresh" when the wrapper allocated it), other
values as they are — or the type name of the exception (an MpcgError with its code).

A sweep() takes a valid call and makes ONE tensor wrong per case (a shorter one, another dtype, a non-contiguous one, one on the CPU).  Those run
with the proxy closed: a C call would be recorded as the exception "ReachedC" and is NOT forwarded, so no kernel ever sees such a tensor.  Only tensors
that the wrapper checks are listed.  The other refusals are Python's own or the library's argument checks (an unknown option, a plant with limits
given to a plain entry); nothing here is meant to make a kernel misbehave.

Shapes: state 14, control 7, 4 knots, batch 2, three step sizes, max_iter 2; 2 knots once for advance_horizon; (n, m, N) = (6, 3, 2) with an
explicit control_size for form_schur / compute_dz / solve / block_solve."""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "binding_calls.json")

n, m, N, B, T = 14, 7, 4, 2, 9
STEPS = (1.0, 0.5, 0.25)
DT = 1.0 / 64


class ReachedC(Exception):
    """A call that a sweep() made wrong got as far as the library (it is not forwarded)."""


class Recorder:
    """The proxy of the library (`self.lib`) and the table of cases."""

    def __init__(self, lib):
        self.real, self.lib = lib, _Proxy(self)
        self.labels, self.objects, self.calls, self.open, self.cases = {}, {}, [], True, []

    def norm(self, a):
        if a is None:
            return "null"
        if isinstance(a, bool) or isinstance(a, int):
            return int(a)
        if isinstance(a, float):
            return a.hex()
        if isinstance(a, bytes):
            return "b:" + a.decode()
        if isinstance(a, C.c_void_p):
            return self.pointer(a.value)
        if isinstance(a, C.Array):
            return {"array": a._type_.__name__, "values": [self.norm(v) for v in a]}
        if isinstance(a, C.Structure):
            return {"struct": type(a).__name__, "fields": {f: self.field(t, getattr(a, f)) for f, t in a._fields_}}
        if hasattr(a, "_obj"):                                  # byref(...)
            return self.norm(a._obj) if isinstance(a._obj, C.Structure) else "out:" + type(a._obj).__name__
        return "?" + type(a).__name__

    def field(self, ctype, v):
        return self.pointer(v) if ctype is C.c_void_p else self.norm(v)

    def pointer(self, v):
        import torch
        if not v:
            return "null"
        if v == torch.cuda.current_stream().cuda_stream:
            return "stream"
        return self.labels.get(v) or self.objects.get(v) or "fresh"

    def result(self, r):
        import torch
        if isinstance(r, torch.Tensor):
            return {"tensor": self.labels.get(r.data_ptr(), "fresh"), "dtype": str(r.dtype), "shape": list(r.shape), "device": r.device.type}
        if isinstance(r, (tuple, list)):
            return [self.result(v) for v in r]
        if isinstance(r, dict):
            return {k: self.result(v) for k, v in r.items()}
        if hasattr(r, "dtype") and hasattr(r, "shape"):         # a numpy array
            return {"array": str(r.dtype), "shape": list(r.shape)}
        if r is None or isinstance(r, (bool, int, str)):
            return r
        if isinstance(r, float):
            return r.hex()
        return type(r).__name__                                 # a Plant, a solver

    def case(self, name, fn, tensors=None, forward=True):
        """Runs fn() as the case `name`; `tensors`: label -> tensor, what its pointers are called in the record."""
        self.labels = {t.data_ptr(): k for k, t in (tensors or {}).items() if t.is_cuda}
        assert len(self.labels) == sum(t.is_cuda for t in (tensors or {}).values()), f"{name}: two tensors share an address"
        self.calls, self.open = [], forward
        rec = {"case": name}
        try:
            rec["returns"] = self.result(fn())
        except Exception as e:
            rec["raises"] = type(e).__name__ + (f"({e.code})" if hasattr(e, "code") else "")
        rec["calls"], self.calls, self.open = self.calls, [], True      # (what is called between two cases belongs to neither)
        assert all(c["case"] != name for c in self.cases), name
        self.cases.append(rec)
        return rec

    def made(self, what, handle):
        """Remembers the address of something the library made, so that later calls show it by kind."""
        self.objects[handle.value] = what
        return handle


class _Proxy:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        rec, fn = self._rec, getattr(self._rec.real, name)

        def call(*args):
            rec.calls.append([name] + [rec.norm(a) for a in args])
            if not rec.open:
                raise ReachedC(name)
            return fn(*args)
        return call


def tensors_of(kw):
    """label -> tensor for every tensor of a method's keyword arguments, those of an XuRef (`ref.`) and of a Clocks (`clocks.`) included."""
    import torch
    from mpcgpu_amd.solver import Clocks, XuRef
    out = {}
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            out[k] = v
        elif isinstance(v, XuRef):
            out.update({f"{k}.{f.name}": getattr(v, f.name) for f in dataclasses.fields(v) if isinstance(getattr(v, f.name), torch.Tensor)})
        elif isinstance(v, Clocks):
            out.update({f"{k}.{a}": getattr(v, a) for a in ("prev_sim_us", "since_s", "shifted")})
    return out


def wrong(t, kind):
    """The tensor t with one thing wrong."""
    import torch
    if kind == "short":
        return t[..., :-1].contiguous()
    if kind == "dtype":
        other = {torch.float32: torch.float64, torch.float64: torch.float32, torch.float16: torch.float32, torch.int32: torch.int64,
                 torch.uint8: torch.int32}
        return t.to(other[t.dtype])
    if kind == "strided":
        s = t.new_zeros(t.numel(), 2)[:, 0].view(t.shape) if t.dim() == 1 else t.new_zeros(*t.shape, 2)[..., 0]
        assert not s.is_contiguous() and s.shape == t.shape
        return s
    assert kind == "cpu"
    return t.cpu()


KINDS = ("short", "dtype", "strided", "cpu")


def record():
    """The table as a dict (what main() writes)."""
    import numpy as np
    import torch
    from mpcgpu_amd import _lib, iiwa, synth
    import mpcgpu_amd.solver as sv
    from mpcgpu_amd.solver import Clocks, PcgSolver, Plant, QdldlSolver, XuRef, pcg_config, pcgSharedMemSize

    rec = Recorder(_lib.load())
    real_load = _lib.load
    _lib.load = lambda: rec.lib
    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            _cases(rec, np, torch, iiwa, synth, sv, Clocks, PcgSolver, Plant, QdldlSolver, XuRef, pcg_config, pcgSharedMemSize)
        side.synchronize()
    finally:
        _lib.load = real_load
    return {"shape": {"n": n, "m": m, "N": N, "B": B, "T": T, "steps": list(STEPS)}, "cases": rec.cases}


def _cases(rec, np, torch, iiwa, synth, sv, Clocks, PcgSolver, Plant, QdldlSolver, XuRef, pcg_config, pcgSharedMemSize):
    F = {"f32": torch.float32, "f64": torch.float64}
    dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64, device="cuda")
    zeros = lambda dt, *shape: torch.zeros(*shape, dtype=dt, device="cuda")

    def call(name, obj, method, kw, forward=True):
        """The case `name`: obj.method(**kw), its tensors labelled by their keyword."""
        return rec.case(name, lambda: getattr(obj, method)(**kw), tensors_of(kw), forward)

    def sweep(name, obj, method, make, checked, kinds=KINDS):
        """Per tensor of `checked` and per kind: the valid call `make()` with that one tensor wrong, never forwarded to the library."""
        for path in checked:
            for kind in kinds:
                kw = make()
                holder, _, attr = path.rpartition(".")
                if holder:
                    setattr(kw[holder], attr, wrong(getattr(kw[holder], attr), kind))
                else:
                    kw[path] = wrong(kw[path], kind)
                call(f"{name} {path} {kind}", obj, method, kw, forward=False)

    # ---- the objects ----
    rec.case("pcgSharedMemSize", lambda: pcgSharedMemSize(n, N))
    sol = PcgSolver(N, max_batch=B)
    rec.case("PcgSolver", lambda: PcgSolver(N, max_batch=B).close())
    rec.case("PcgSolver generic", lambda: PcgSolver(2, B, 6, None, 3).close())
    rec.case("PcgSolver unsupported", lambda: PcgSolver(N, state_size=65))
    sol2 = PcgSolver(2, max_batch=B)                                  # the shortest horizon, for advance_horizon
    solg = PcgSolver(2, max_batch=B, state_size=6)                    # the generic shape: control_size is given per call
    plant = Plant()
    for s in (sol, sol2, solg):
        rec.made("handle", s._h)
    rec.made("plant", plant._p)
    rec.case("Plant", lambda: Plant().close())
    rec.case("Plant gravity", lambda: Plant(gravity=(0.0, 0.0, -9.81)).gravity)

    # ---- options and facts ----
    rec.case("set_option", lambda: sol.set_option("check_symmetry", 1))
    rec.case("get_option", lambda: sol.get_option("check_symmetry"))
    rec.case("set_option unknown", lambda: sol.set_option("no_such_option", 1))
    rec.case("last_error", lambda: sol.last_error())
    rec.case("get_option unknown", lambda: sol.get_option("no_such_option"))
    rec.case("set_option back", lambda: sol.set_option("check_symmetry", 0))
    rec.case("checkPcgOccupancy", lambda: sol.checkPcgOccupancy() > 0)
    rec.case("csr_nnz", lambda: (sol.csr_nnz(), solg.csr_nnz()))
    rec.case("prep_csr", lambda: sol.prep_csr())

    # ---- the linear system: solve*, block_solve, form_schur, compute_dz ----
    k = synth.make_kkt(N, B, 5)
    kg = synth.make_kkt(2, B, 6, n=6, m=3)
    cfg = pcg_config(pcg_exit_tol=1e-6, pcg_max_iter=2)

    host = {id(kk): (synth.form_schur(kk, dtype=np.float64), synth.pack_kkt_dense(kk, np.float64)) for kk in (k, kg)}

    def system(kk, dt):
        S, Pinv, gamma = host[id(kk)][0]
        return {"S": dev(S, dt), "Pinv": dev(Pinv, dt), "gamma": dev(gamma, dt), "lam": zeros(dt, B, gamma.shape[1])}

    def outs(kw):
        return dict(kw, iters=zeros(torch.int32, B), exits=zeros(torch.uint8, B))

    for p, meth in (("f32", "solve"), ("f64", "solve_f64")):
        dt = F[p]
        call(f"{meth}", sol, meth, dict(system(k, dt), config=cfg))
        call(f"{meth} outputs given", sol, meth, outs(dict(system(k, dt), config=cfg, precond="jacobi")))
        call(f"{meth} default config", sol, meth, system(k, dt))
        call(f"{meth} one trajectory", sol, meth, {a: t[0].clone() for a, t in system(k, dt).items()} | {"config": cfg})
        call(f"{meth} generic", solg, meth, dict(system(kg, dt), config=cfg))
        call(f"{meth} precond", sol, meth, dict(system(k, dt), config=cfg, precond="none"))
        sweep(meth, sol, meth, lambda: dict(system(k, dt), config=cfg), ("S", "Pinv", "gamma", "lam"))

    def system16():
        a = system(k, torch.float32)
        return {"S16": a["S"].half(), "Pinv16": a["Pinv"].half(), "gamma": a["gamma"], "lam": a["lam"]}
    call("to_f16", sol, "to_f16", {"M": system(k, torch.float32)["S"]})
    sweep("to_f16", sol, "to_f16", lambda: {"M": system(k, torch.float32)["S"]}, ("M",), KINDS[1:])       # (any length is one)
    call("solve_f16", sol, "solve_f16", dict(system16(), config=cfg))
    call("solve_f16 outputs given", sol, "solve_f16", outs(dict(system16(), config=cfg, precond="jacobi")))
    call("solve_f16 default config", sol, "solve_f16", system16())
    call("solve_f16 precond", sol, "solve_f16", dict(system16(), precond="none"))
    sweep("solve_f16", sol, "solve_f16", lambda: dict(system16(), config=cfg), ("S16", "Pinv16", "gamma", "lam"))

    for p, meth in (("f32", "solve_ref"), ("f64", "solve_ref_f64")):
        dt = F[p]
        a = {a: t[0].clone() for a, t in system(k, dt).items()}
        call(meth, sol, meth, {"d_S": a["S"], "d_Pinv": a["Pinv"], "d_gamma": a["gamma"], "d_lambda": a["lam"], "d_r": zeros(dt, n * N),
                               "d_p": zeros(dt, n * N), "d_v_temp": zeros(dt, N + 1), "d_eta_new_temp": zeros(dt, N + 1),
                               "d_pcg_iters": zeros(torch.int32, 1), "d_pcg_exit": zeros(torch.bool, 1), "pcg_max_iter": 2, "pcg_exit_tol": 1e-6})

    for p, dt in F.items():
        bs = lambda kk=k: {a: t for a, t in system(kk, dt).items() if a != "Pinv"}
        call(f"block_solve {p}", sol, "block_solve", {a: t for a, t in bs().items() if a != "lam"})
        call(f"block_solve {p} lam given", sol, "block_solve", bs())
        call(f"block_solve {p} generic", solg, "block_solve", bs(kg))
        sweep(f"block_solve {p}", sol, "block_solve", bs, ("S", "gamma", "lam"))

        def kkt(kk=k):
            return dict(zip(("G_dense", "C_dense", "g", "c"), (dev(a, dt) for a in host[id(kk)][1])))

        def schur_outs(kw, nn=n, NN=N):
            return dict(kw, S=zeros(dt, B, 3 * nn * nn * NN), Pinv=zeros(dt, B, 3 * nn * nn * NN), gamma=zeros(dt, B, nn * NN))
        call(f"form_schur {p}", sol, "form_schur", dict(kkt(), rho=1e-3))
        call(f"form_schur {p} outputs given", sol, "form_schur", schur_outs(dict(kkt(), rho=1e-3, precond="jacobi")))
        call(f"form_schur {p} rho tensor", sol, "form_schur", dict(kkt(), rho=torch.full((B,), 1e-3, dtype=dt, device="cuda"), precond="none"))
        call(f"form_schur {p} rho tensor outputs given", sol, "form_schur", schur_outs(dict(kkt(), rho=torch.full((B,), 1e-3, dtype=dt, device="cuda"))))
        call(f"form_schur {p} generic", solg, "form_schur", schur_outs(dict(kkt(kg), rho=1e-3, control_size=3), 6, 2))
        call(f"form_schur {p} one trajectory", sol, "form_schur", {a: t[0].clone() for a, t in kkt().items()} | {"rho": 1e-3})
        call(f"form_schur {p} precond", sol, "form_schur", dict(kkt(), rho=1e-3, precond="ssor"))
        sweep(f"form_schur {p}", sol, "form_schur", lambda: schur_outs(dict(kkt(), rho=torch.full((B,), 1e-3, dtype=dt, device="cuda"))),
              ("G_dense", "C_dense", "g", "c", "rho", "S", "Pinv", "gamma"))

        def dz_args(kk=k, **more):
            a = kkt(kk)
            return dict({"Ginv_dense": a["G_dense"], "C_dense": a["C_dense"], "g": a["g"], "lam": torch.ones_like(a["c"])}, **more)
        call(f"compute_dz {p}", sol, "compute_dz", dz_args())
        call(f"compute_dz {p} dz given", sol, "compute_dz", dz_args(dz=zeros(dt, B, (n + m) * N - m)))
        call(f"compute_dz {p} generic", solg, "compute_dz", dz_args(kg, control_size=3))
        sweep(f"compute_dz {p}", sol, "compute_dz", lambda: dz_args(dz=zeros(dt, B, (n + m) * N - m)), ("Ginv_dense", "C_dense", "g", "lam", "dz"))

    S32 = lambda: system(k, torch.float32)["S"]
    call("bd_to_csr_lowertri", sol, "bd_to_csr_lowertri", {"S": S32()})
    call("bd_to_csr_lowertri one trajectory", sol, "bd_to_csr_lowertri", {"S": S32()[0].clone(), "mult": -1.0})
    sweep("bd_to_csr_lowertri", sol, "bd_to_csr_lowertri", lambda: {"S": S32()}, ("S",))
    call("probe_hbm_read", sol, "probe_hbm_read", {"src": zeros(torch.float32, 37)})
    call("probe_hbm_read sink given", sol, "probe_hbm_read", {"src": zeros(torch.float64, 8), "sink": zeros(torch.float32, 1)})
    spmv = lambda: {"M": S32(), "x": torch.ones(B, n * N, device="cuda")}
    call("bt_spmv", sol, "bt_spmv", spmv())
    call("bt_spmv y given", sol, "bt_spmv", dict(spmv(), y=zeros(torch.float32, B, n * N), cols=1))
    sweep("bt_spmv", sol, "bt_spmv", spmv, ("M", "x"))

    # ---- the plant entries ----
    windows = {NN: iiwa.random_windows(NN, B, 7) for NN in (N, 2)}
    xu_h, goals_h, xs_h = windows[N]
    fx = np.load(iiwa.TRAJ_FIXTURE)
    plan_h, plan_goals_h = fx["xu"][:2 * T].astype(np.float64), fx["eepos"][:2 * T].astype(np.float64)
    limited = plant.with_limits(q=(-2.0, 2.0), u=(None, 100.0), q_weight=1.0, u_weight=0.5, sim_saturate=True)
    rec.made("plant", limited._p)

    def refs(dt):
        """name -> a fresh XuRef: the shapes of plan the _xuref entries take."""
        shared, per = dev(plan_h[:T], dt), dev(plan_h.reshape(2, T, n + m), dt)
        return {"shared plan": XuRef(shared), "shared plan offsets": XuRef(shared, i32(0, 3), ee_cost=0.5, q_cost=2.0, qd_relative=True),
                "plan per trajectory": XuRef(per, u_relative=True), "plan per trajectory offsets": XuRef(per, i32(1, 2), traj_batch_stride=T),
                "strided plan": XuRef(dev(plan_h, dt), None, 6, traj_steps=5), "strided plan offsets": XuRef(dev(plan_h, dt), i32(2, 0), 7)}

    for p, dt in F.items():
        state = lambda: {"eePos_traj": dev(goals_h.reshape(B, -1), dt), "xs": dev(xs_h, dt), "xu": dev(xu_h, dt)}
        cost = {"timestep": DT, "qd_cost": 1e-4, "r_cost": 1e-4}
        call(f"generate_kkt {p}", sol, "generate_kkt", dict(state(), plant=plant, **cost))
        call(f"generate_kkt {p} control_size", sol, "generate_kkt", dict(state(), plant=plant, control_size=7, **cost))
        call(f"generate_kkt {p} limits", sol, "generate_kkt", dict(state(), plant=limited, **cost))
        sweep(f"generate_kkt {p}", sol, "generate_kkt", lambda: dict(state(), plant=plant, **cost), ("eePos_traj", "xs", "xu"))
        for name in refs(dt):
            call(f"generate_kkt_xuref {p} {name}", sol, "generate_kkt_xuref", dict(state(), plant=limited, ref=refs(dt)[name], **cost))
        ee0 = XuRef(dev(plan_h[:T], dt), ee_cost=0.0, q_cost=1.0)
        call(f"generate_kkt_xuref {p} no goals", sol, "generate_kkt_xuref", dict(state(), plant=plant, ref=ee0, **cost) | {"eePos_traj": None})
        sweep(f"generate_kkt_xuref {p}", sol, "generate_kkt_xuref", lambda: dict(state(), plant=plant, ref=refs(dt)["shared plan offsets"], **cost),
              ("eePos_traj", "xs", "xu", "ref.xu_traj", "ref.traj_offset"))
        call(f"generate_kkt_xuref {p} short plan", sol, "generate_kkt_xuref",
             dict(state(), plant=plant, ref=XuRef(dev(plan_h[:T], dt), traj_batch_stride=T), **cost), forward=False)
        call(f"generate_kkt_xuref {p} ragged plan", sol, "generate_kkt_xuref",
             dict(state(), plant=plant, ref=XuRef(dev(plan_h[:T].reshape(-1)[:-1], dt)), **cost), forward=False)
        call(f"generate_kkt_xuref {p} batch of plans", sol, "generate_kkt_xuref",
             dict(state(), plant=plant, ref=XuRef(dev(plan_h[:T].reshape(1, T, n + m), dt)), **cost), forward=False)

        mcost = {"step_sizes": STEPS, "timestep": DT, "mu": 10.0, "qd_cost": 1e-4, "r_cost": 1e-4}
        trial = lambda: dict(state(), dz=dev(0.01 * xu_h[::-1], dt))
        call(f"compute_merit {p}", sol, "compute_merit", dict(trial(), plant=plant, **mcost))
        call(f"compute_merit {p} merit given", sol, "compute_merit", dict(trial(), plant=plant, merit=zeros(dt, B, 3), control_size=7, **mcost))
        call(f"compute_merit {p} no xs no dz", sol, "compute_merit", dict(trial(), plant=plant, **mcost) | {"xs": None, "dz": None, "step_sizes": (0.0,)})
        call(f"compute_merit {p} limits", sol, "compute_merit", dict(trial(), plant=limited, **mcost))
        sweep(f"compute_merit {p}", sol, "compute_merit", lambda: dict(trial(), plant=plant, merit=zeros(dt, B, 3), **mcost),
              ("eePos_traj", "xs", "xu", "dz", "merit"))
        for name in ("shared plan offsets", "plan per trajectory", "strided plan"):
            call(f"compute_merit_xuref {p} {name}", sol, "compute_merit_xuref", dict(trial(), plant=limited, ref=refs(dt)[name], **mcost))
        call(f"compute_merit_xuref {p} merit given no goals", sol, "compute_merit_xuref",
             dict(trial(), plant=plant, ref=ee0, merit=zeros(dt, B, 3), **mcost) | {"eePos_traj": None, "xs": None})
        sweep(f"compute_merit_xuref {p}", sol, "compute_merit_xuref",
              lambda: dict(trial(), plant=plant, ref=refs(dt)["shared plan offsets"], merit=zeros(dt, B, 3), **mcost),
              ("eePos_traj", "xs", "xu", "dz", "merit", "ref.xu_traj", "ref.traj_offset"))

        ls = lambda: {"merit": dev([[3.0, 1.0, 2.0], [5.0, 6.0, 7.0]], dt), "step_sizes": STEPS, "merit_ref": dev([4.0, 4.0], dt),
                      "dz": dev(0.01 * xu_h[::-1], dt), "xu": dev(xu_h, dt)}
        call(f"line_search_step {p}", sol, "line_search_step", ls())
        call(f"line_search_step {p} step given", sol, "line_search_step", dict(ls(), step=zeros(torch.int32, B), control_size=7))
        sweep(f"line_search_step {p}", sol, "line_search_step", lambda: dict(ls(), step=zeros(torch.int32, B)), ("merit", "merit_ref", "dz", "xu", "step"))
        lsr = lambda: dict(ls(), rho=dev([1e-3, 1e-2], dt), drho=dev([1.0, 1.0], dt), done=zeros(torch.uint8, B))
        call(f"line_search_step_rho {p}", sol, "line_search_step_rho", lsr())
        call(f"line_search_step_rho {p} step given", sol, "line_search_step_rho",
             dict(lsr(), rho_factor=1.5, rho_min=1e-4, rho_max=20.0, rho_reset=2e-3, step=zeros(torch.int32, B), control_size=7))
        sweep(f"line_search_step_rho {p}", sol, "line_search_step_rho", lambda: dict(lsr(), step=zeros(torch.int32, B)),
              ("merit", "merit_ref", "dz", "xu", "rho", "drho", "done", "step"))

        sim = lambda: {"plant": plant, "xs": dev(xs_h, dt), "xu": dev(xu_h, dt), "timestep": DT}
        call(f"simulate {p}", sol, "simulate", dict(sim(), time_offset_us=0.0, sim_time_us=650.0))
        call(f"simulate {p} eePos given", sol, "simulate",
             dict(sim(), time_offset_us=100.0, sim_time_us=650.0, sim_step=1e-4, eePos=zeros(dt, B, 3), control_size=7) | {"plant": limited})
        sweep(f"simulate {p}", sol, "simulate", lambda: dict(sim(), time_offset_us=0.0, sim_time_us=650.0, eePos=zeros(dt, B, 3)), ("xs", "xu", "eePos"))
        clk = lambda: dict(sim(), time_offset_us=f64(0.0, 100.0), sim_time_us=f64(650.0, 300.0))
        call(f"simulate_clk {p}", sol, "simulate_clk", clk())
        call(f"simulate_clk {p} eePos and done given", sol, "simulate_clk",
             dict(clk(), sim_step=1e-4, eePos=zeros(dt, B, 3), done=zeros(torch.int32, B), control_size=7))
        sweep(f"simulate_clk {p}", sol, "simulate_clk", lambda: dict(clk(), eePos=zeros(dt, B, 3), done=zeros(torch.int32, B)),
              ("xs", "xu", "time_offset_us", "sim_time_us", "eePos", "done"))

        q = lambda: dev(xs_h[:, :7], dt)
        call(f"inverse_dynamics {p}", sol, "inverse_dynamics", {"plant": plant, "q": q()})
        call(f"inverse_dynamics {p} all given", sol, "inverse_dynamics",
             {"plant": limited, "q": q(), "qd": dev(xs_h[:, 7:], dt), "qdd": dev(xs_h[:, 7:] * 2, dt), "tau": zeros(dt, B, 7)})
        call(f"inverse_dynamics {p} ragged q", sol, "inverse_dynamics", {"plant": plant, "q": zeros(dt, 13)}, forward=False)
        sweep(f"inverse_dynamics {p}", sol, "inverse_dynamics",
              lambda: {"plant": plant, "q": q(), "qd": dev(xs_h[:, 7:], dt), "qdd": dev(xs_h[:, 7:] * 2, dt), "tau": zeros(dt, B, 7)}, ("q", "qd", "qdd", "tau"))

        def horizon(NN=N, per_traj=False):
            xu, goals, xs = windows[NN]
            rows = (lambda a: a.reshape(2, T, -1)) if per_traj else (lambda a: a[:T])
            return {"xu": dev(xu, dt), "xs": dev(xs, dt), "lam": zeros(dt, B, n * NN), "eePos_goal": dev(goals.reshape(B, -1), dt), "eePos": dev(goals[:, 0, :3], dt),
                    "xu_traj": dev(rows(plan_h), dt), "eePos_traj": dev(rows(plan_goals_h), dt), "traj_offset": i32(0, T - 1), "done": zeros(torch.int32, B),
                    "tracking_error": zeros(dt, B)}
        start = lambda: {a: t for a, t in horizon().items() if a in ("xu", "xs")}
        call(f"advance_horizon {p} no shift", sol, "advance_horizon", dict(start(), shift=False))
        call(f"advance_horizon {p} no shift done given", sol, "advance_horizon", dict(start(), shift=False, done=zeros(torch.int32, B), control_size=7))
        call(f"advance_horizon {p} no shift all given", sol, "advance_horizon", dict(horizon(), shift=False))
        sweep(f"advance_horizon {p} no shift", sol, "advance_horizon", lambda: dict(start(), shift=False, done=zeros(torch.int32, B)), ("xu", "xs", "done"))
        call(f"advance_horizon {p} shift", sol, "advance_horizon", dict(horizon(), shift=True))
        call(f"advance_horizon {p} shift no eePos", sol, "advance_horizon", dict(horizon(), shift=True, xu_fill_lead=N - 1) | {"eePos": None})
        call(f"advance_horizon {p} shift plan per trajectory", sol, "advance_horizon", dict(horizon(per_traj=True), shift=True, control_size=7))
        call(f"advance_horizon {p} shift two knots", sol2, "advance_horizon", dict(horizon(2), shift=True))
        for missing in ("lam", "eePos_goal", "xu_traj", "eePos_traj", "traj_offset", "done", "tracking_error"):
            call(f"advance_horizon {p} shift without {missing}", sol, "advance_horizon", dict(horizon(), shift=True) | {missing: None}, forward=False)
        everything = ("xu", "xs", "lam", "eePos_goal", "eePos", "xu_traj", "eePos_traj", "traj_offset", "done", "tracking_error")
        sweep(f"advance_horizon {p} shift", sol, "advance_horizon", lambda: dict(horizon(), shift=True), everything)
        sweep(f"advance_horizon {p} shift plan per trajectory", sol, "advance_horizon", lambda: dict(horizon(per_traj=True), shift=True),
              ("xu_traj", "eePos_traj"))

        hclk = lambda **kw: dict(horizon(**kw), timestep=DT, sim_time_us=f64(2000.0, 16000.0), clocks=Clocks(B))
        call(f"advance_horizon_clk {p}", sol, "advance_horizon_clk", hclk())
        call(f"advance_horizon_clk {p} plan per trajectory all given", sol, "advance_horizon_clk",
             dict(hclk(per_traj=True), did_shift=zeros(torch.int32, B), shift_threshold_s=0.01, xu_fill_lead=N - 1, control_size=7))
        call(f"advance_horizon_clk {p} two knots", sol2, "advance_horizon_clk", hclk(NN=2))
        sweep(f"advance_horizon_clk {p}", sol, "advance_horizon_clk", lambda: dict(hclk(), did_shift=zeros(torch.int32, B)),
              everything + ("sim_time_us", "did_shift", "clocks.prev_sim_us", "clocks.since_s", "clocks.shifted"))

    # ---- Plant ----
    seven = [0.1 * j for j in range(1, 8)]
    rec.case("with_gravity", lambda: plant.with_gravity((0.0, 0.0, -9.81)))
    rec.case("with_gravity two components", lambda: plant.with_gravity((0.0, -9.81)))
    rec.case("gravity", lambda: plant.gravity)
    rec.case("limits of a plant without", lambda: plant.limits)
    rec.case("limits", lambda: limited.limits)
    rec.case("with_limits nothing", lambda: plant.with_limits().limits)
    rec.case("with_limits seven per side", lambda: plant.with_limits(q=([-v for v in seven], seven), qd=(None, seven), u=(np.float32(-3), 4), qd_weight=2.0).limits)
    for what, bad in (("a string", "ab"), ("a number", 1.0), ("three", (0.0, 1.0, 2.0)), ("a side of three numbers", ((0.0, 1.0, 2.0), None)),
                      ("a side that is text", ("lo", None)), ("a side of 7 by 1", (None, [[v] for v in seven]))):
        rec.case(f"with_limits {what}", lambda: plant.with_limits(qd=bad))
    rec.case("with_limits refused by the library", lambda: plant.with_limits(q=(1.0, -1.0)))

    # ---- QdldlSolver ----
    ldl = QdldlSolver(N)
    rec.made("ldl", ldl._l)
    rec.case("QdldlSolver", lambda: QdldlSolver(2, state_size=6).close())
    val = sol.bd_to_csr_lowertri(S32()[0].clone())
    gamma0 = system(k, torch.float32)["gamma"][0].clone()
    rec.case("solve_host", lambda: ldl.solve_host(val[0].cpu().numpy(), gamma0.cpu().numpy()))
    call("solve_schur", ldl, "solve_schur", {"sol": sol, "d_val": val, "d_gamma": gamma0, "d_lambda": zeros(torch.float32, n * N)})
    torch.cuda.current_stream().synchronize()
    for obj in (ldl, limited, plant, solg, sol2, sol):
        rec.case(f"close {type(obj).__name__} {len(rec.cases)}", obj.close)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--force", action="store_true", help="overwrite an existing table")
    args = ap.parse_args()
    if os.path.exists(args.out) and not args.force:
        sys.exit(f"{args.out} exists: the table is a record of the binding before a change — pass --force to replace it")
    table = record()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, separators=(",", ":"), sort_keys=False)
        f.write("\n")
    refused = sum("raises" in c for c in table["cases"])
    print(f"{len(table['cases'])} cases ({refused} refused), {sum(len(c['calls']) for c in table['cases'])} C calls -> {args.out} "
          f"({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
