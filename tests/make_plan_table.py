"""Generates tests/golden/pcg_plan_table.json: what the PCG launch policy (mpcg_pcg.hip) does with each of a fixed list of calls.
Run on the GPU box: `python tests/make_plan_table.py [--out PATH]`.  tests/test_gpu_plan.py replays the same cases and compares.

Per case a fresh handle (max_batch = the call's batch), the options of the case, one call (two for the cases that show a block-asymmetric
Pinv to the handle) with max_iter = 3 on a single stream, then per call: the return code, every "last_kernel_*" option, "symmetry_state" after
the call has finished, and mpcg_check_pcg_occupancy of the handle.  One system per (state_size, N, precision) is built once and repeated
across the batch on the device.  The recorded values hold for the device's CU count (num_cus, stored in the file).

Grid (include/mpcg.h, Options: the kernel-selection table):
  float SS and block-Jacobi, N in KNOTS, default options: batch in {1, C, C + 1, ceil(2.5 C) - 1, ceil(2.5 C), 4 C - 1, 4 C} (C = num_cus) — a
    batch on each side of every threshold the policy tests: batch > C, 2 batch >= 5 C, batch >= 4 C — in every precision;
  every other option set: SS, batch 1 and 4 C; at the two largest N batch 1 and C only;
  fp16 storage: the default options and "pcg_lpk" = 0; double: F64_OPTS; state_size 7 (the generic kernel) in float and double; the
  reference-shaped `_ref` / `_ref_f64` entries.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "pcg_plan_table.json")

KNOTS = (2, 16, 17, 32, 33, 36, 37, 64, 65, 128, 129, 256, 384, 512, 729, 730)     # 729: the largest N mpcg_create takes; 730 refused
LAST = ("family", "waves", "reg_rows", "lds_rows", "lds_extra", "stream_bufs", "cluster", "lds_bytes")
ASYM = "asym"       # pseudo-option: the call(s) of the case see a Pinv whose right blocks are not the transposes of the left ones
F32_OPTS = {
    "default": (),
    "rpl0": (("pcg_rpl", 0),), "rpl1": (("pcg_rpl", 1),),
    "rplw4": (("rpl_waves", 4),), "rplw8": (("rpl_waves", 8),), "rplw16": (("rpl_waves", 16),),
    "lpk0": (("pcg_lpk", 0),), "lpk1": (("pcg_lpk", 1),),
    "lqb0": (("pcg_lqb", 0),), "lqb1": (("pcg_lqb", 1),), "lpk1_lqb1": (("pcg_lpk", 1), ("pcg_lqb", 1)),
    "cluster0": (("cluster", 0),), "cluster2": (("cluster", 2),), "cluster3": (("cluster", 3),),
    "cluster2_sym": (("cluster", 2), ("assume_symmetric", 1)),    # an ungated cluster: up to 128 knots its fix-up is the lane-pair launch
    "fixup0": (("cluster_fixup", 0),),
    "knobs_8_3": (("pcg_waves", 8), ("pcg_reg_rows", 3)),          # a compiled pcg_traj_kernel variant
    "knobs_16_5": (("pcg_waves", 16), ("pcg_reg_rows", 5)),        # none compiled: MPCG_ERR_UNSUPPORTED
    "check_sym": (("check_symmetry", 1),),                          # + a second call with the asymmetric Pinv
    "assume_sym": (("assume_symmetric", 1),),
    "asym": ((ASYM, 1),),                                          # two calls, both with the asymmetric Pinv
}
F16_OPTS = {"default": (), "lpk0": (("pcg_lpk", 0),)}
F64_OPTS = {
    "default": (),
    "lqk-1": (("pcg_lqk", -1),), "lqk0": (("pcg_lqk", 0),), "lqk1": (("pcg_lqk", 1),),
    "rpl0": (("pcg_rpl", 0),),
    "cluster0": (("cluster", 0),), "cluster2": (("cluster", 2),),
    "fixup0": (("cluster_fixup", 0),),
    "asym": ((ASYM, 1),),
}
SECOND_CALL_ASYM = ("check_sym", "asym")


def cases(num_cus):
    """(id, dict) of every case, in the order they run."""
    c = num_cus
    full = (1, c, c + 1, math.ceil(2.5 * c) - 1, math.ceil(2.5 * c), 4 * c - 1, 4 * c)
    out = []
    for N in KNOTS:
        big = N >= 729
        for prec, table in (("f32", F32_OPTS), ("f16", F16_OPTS), ("f64", F64_OPTS)):
            for name, opts in table.items():
                # EXCLUDED: double with a forced "cluster" >= 2 at N <= 32.  Such a call reaches the clustered row-per-lane kernel with a null
                # scratch pointer whenever the row-per-lane kernel is off ("pcg_rpl" = 0 or explicit knobs): reserve_f64 returns early at
                # N <= 32 without allocating (mpcg_pcg.hip: reserve_f64) — a GPU fault.  Never run it.
                if prec == "f64" and N <= 32 and any(k == "cluster" and v >= 2 for k, v in opts):
                    continue
                pcs = ("ss", "jacobi") if name == "default" else ("ss",)
                batches = (1, c) if big else full if name == "default" else (1, 4 * c)
                for pc in pcs:
                    for B in batches:
                        out.append((f"{prec}/n14/N{N}/{name}/{pc}/B{B}", dict(prec=prec, n=14, N=N, opts=opts, pc=pc, B=B, entry="solve",
                                                                               asym2=name in SECOND_CALL_ASYM)))
    for prec in ("f32", "f64"):                 # state_size 7: the generic kernel
        for N in (16, 64):
            for pc in ("ss", "jacobi"):
                for B in (1, 4 * c):
                    out.append((f"{prec}/n7/N{N}/default/{pc}/B{B}", dict(prec=prec, n=7, N=N, opts=(), pc=pc, B=B, entry="solve", asym2=False)))
    for prec in ("f32", "f64"):                 # the reference's 12-argument launch (one trajectory, SS)
        for N in (16, 32, 64, 128, 256):
            out.append((f"{prec}/n14/N{N}/default/ref/B1", dict(prec=prec, n=14, N=N, opts=(), pc="ss", B=1, entry="ref", asym2=False)))
    return out


def _system(n, N, prec, Bmax, torch, synth, to_f16):
    """(S, Pinv, Pinv with asymmetric right blocks, gamma), each [Bmax, ...] on the device: one trajectory's system repeated."""
    if n == 14:
        k = synth.make_kkt(N, 1, 9100 + N)
        S, P, g = synth.form_schur(k, precond="ss", dtype=np.float64 if prec == "f64" else np.float32)
    else:                                       # (no dynamics of odd state size in synth: a diagonally dominant block-tridiagonal system)
        S = np.zeros((N, 3, n, n))
        P = np.zeros((N, 3, n, n))
        S[:, 1], P[:, 1] = -3.0 * np.eye(n), -np.eye(n) / 3.0
        S[1:, 0] = S[:-1, 2] = -0.2 * np.eye(n)
        P[1:, 0] = P[:-1, 2] = -0.02 * np.eye(n)
        dt = np.float64 if prec == "f64" else np.float32
        S, P, g = S.reshape(1, -1).astype(dt), P.reshape(1, -1).astype(dt), np.ones((1, n * N), dt)
    Pa = P.reshape(N, 3, n * n).copy()
    Pa[:-1, 2] *= 1.25
    dev = [torch.from_numpy(np.ascontiguousarray(a).reshape(1, -1)).cuda() for a in (S, P, Pa.reshape(1, -1), g)]
    if prec == "f16":
        dev[:3] = [to_f16(m) for m in dev[:3]]
    return [m.repeat(Bmax, 1) for m in dev]


def run_case(lib, case, sysd, torch):
    """The record of one case: {"create": rc} for a refused handle, else {"set": rc} / {"calls": [...]}."""
    from mpcgpu_amd import _lib
    p = case
    h = C.c_void_p()
    rc = lib.mpcg_create(C.byref(h), torch.cuda.current_device(), p["n"], p["N"], p["B"])
    if rc != 0:
        return {"create": rc}
    rec = {}
    try:
        for k, v in p["opts"]:
            if k == ASYM:
                continue
            rc = lib.mpcg_set_option(h, k.encode(), int(v))
            if rc != 0:
                return {"set": rc}
        asym_first = any(k == ASYM for k, _ in p["opts"])
        S, P, Pa, g = sysd
        B, n, N = p["B"], p["n"], p["N"]
        f64 = p["prec"] == "f64"
        pc = _lib.MPCG_PRECOND_SS if p["pc"] == "ss" else _lib.MPCG_PRECOND_JACOBI
        calls = []
        for ci in range(2 if p["asym2"] else 1):
            Pm = Pa if (asym_first or ci == 1) else P
            lam = torch.zeros(B, n * N, dtype=torch.float64 if f64 else torch.float32, device="cuda")
            it = torch.zeros(B, dtype=torch.int32, device="cuda")
            ex = torch.zeros(B, dtype=torch.uint8, device="cuda")
            ptr = lambda t: C.c_void_p(t.data_ptr())
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if p["entry"] == "ref":
                r, q = torch.empty_like(lam[0]), torch.empty_like(lam[0])
                fn = lib.mpcg_pcg_solve_ref_f64 if f64 else lib.mpcg_pcg_solve_ref
                rc = fn(h, ptr(S), ptr(Pm), ptr(g), ptr(lam), ptr(r), ptr(q), None, None, ptr(it), ptr(ex), 3, 0.0, st)
            else:
                fn = {"f32": lib.mpcg_pcg_solve, "f16": lib.mpcg_pcg_solve_f16, "f64": lib.mpcg_pcg_solve_f64}[p["prec"]]
                rc = fn(h, ptr(S[:B]), ptr(Pm[:B]), ptr(g[:B]), ptr(lam), B, 3, 0.0, pc, ptr(it), ptr(ex), st)
            torch.cuda.synchronize()
            vals = []
            for key in ("last_kernel_" + f for f in LAST):
                v = C.c_int()
                assert lib.mpcg_get_option(h, key.encode(), C.byref(v)) == 0
                vals.append(v.value)
            v = C.c_int()
            assert lib.mpcg_get_option(h, b"symmetry_state", C.byref(v)) == 0
            occ = C.c_uint32()
            orc_ = lib.mpcg_check_pcg_occupancy(h, C.byref(occ))
            calls.append({"rc": rc, "last": vals, "sym": v.value, "occ": [orc_, occ.value if orc_ == 0 else 0]})
        rec["calls"] = calls
        return rec
    finally:
        lib.mpcg_destroy(h)


def run(num_cus_expected=None):
    """Yields (case id, record) for every case.  Systems are built lazily per (n, N, precision) and dropped when the next one is needed."""
    import torch
    from mpcgpu_amd import _lib, synth, PcgSolver
    lib = _lib.load()
    torch.cuda.set_device(0)
    probe = PcgSolver(16, max_batch=1)
    num_cus = probe.get_option("num_cus")
    yield "num_cus", num_cus
    if num_cus_expected is not None and num_cus != num_cus_expected:
        return
    all_cases = cases(num_cus)
    need = {}
    for cid, p in all_cases:
        key = (p["n"], p["N"], p["prec"])
        need[key] = max(need.get(key, 0), p["B"])
    cur_key, sysd = None, None
    for cid, p in all_cases:
        key = (p["n"], p["N"], p["prec"])
        if key != cur_key:
            sysd = None
            torch.cuda.empty_cache()
            sysd = _system(p["n"], p["N"], p["prec"], need[key], torch, synth, probe.to_f16)
            cur_key = key
        yield cid, run_case(lib, p, sysd, torch)
    probe.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    it = run()
    _, num_cus = next(it)
    table = {"num_cus": num_cus, "max_iter": 3, "last_fields": list(LAST), "cases": {}}
    for i, (cid, rec) in enumerate(it):
        table["cases"][cid] = rec
        if i % 250 == 0:
            print(f"{i} {cid}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, separators=(",", ":"), sort_keys=False)
        f.write("\n")
    print(f"{len(table['cases'])} cases, num_cus = {num_cus} -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
