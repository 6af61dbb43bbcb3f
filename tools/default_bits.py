#!/usr/bin/env python3
"""Do two builds of the library compute the same BYTES with every option at its default?  Dumps, from fixed inputs, the outputs of the plant kernels'
entries — mpcg_generate_kkt (default, "kkt_analytic" = 0, "kkt_f32" = 1 and 2) and mpcg_generate_kkt_f64 (both gradient routes); mpcg_compute_merit (default,
"merit_f32" = 1) and mpcg_compute_merit_f64 at nine step sizes; mpcg_simulate and mpcg_simulate_f64 (state and end-effector position) — at 1024 x 128 and
1 x 32, as one SHA-256 per output array over the array's bytes (the arrays of the large shape are gigabytes), and compares two such dumps.

    python tools/default_bits.py dump [--root DIR] OUT.json      one build, in a process of its own (DIR: another checkout, built there; default: this one)
    python tools/default_bits.py compare A.json B.json           exit status 1 on any difference

A build that changes a default instantiation of a kernel shows up here as a differing array.  Needs an MI355X for `dump`."""
import hashlib
import json
import os
import sys

STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]
MU = 10.0


def dump(root, out):
    import numpy as np
    import torch
    from mpcgpu_amd import PcgSolver, Plant, iiwa
    dev = torch.device("cuda", 0)
    plant = Plant()
    sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
    arrays = {}
    for N, B in ((128, 1024), (32, 1)):
        xu, ee, xs = (np.ascontiguousarray(a, np.float32) for a in iiwa.random_windows(N, B, seed=3))
        dz = (0.05 * np.random.default_rng(4).standard_normal(xu.shape)).astype(np.float32)
        rng = np.random.default_rng(5)
        wide = lambda a: a.astype(np.float64) * (1.0 + 1e-12 * rng.uniform(-1, 1, a.shape))
        h32 = tuple(torch.from_numpy(a).to(dev) for a in (ee.reshape(B, -1), xs, xu, dz))
        h64 = tuple(torch.from_numpy(a).to(dev) for a in (ee.reshape(B, -1).astype(np.float64), wide(xs), wide(xu), wide(dz)))
        r, qd = iiwa.r_cost(N), iiwa.QD_COST
        for name, args, opts in (("kkt", h32, {}), ("kkt difference", h32, {"kkt_analytic": 0}), ("kkt kkt_f32=1", h32, {"kkt_f32": 1}), ("kkt kkt_f32=2", h32, {"kkt_f32": 2}),
                                 ("kkt_f64", h64, {}), ("kkt_f64 difference", h64, {"kkt_analytic": 0})):
            sol = PcgSolver(N, max_batch=B)
            for k, v in opts.items():
                sol.set_option(k, v)
            goal, s, x, _ = args
            outs = sol.generate_kkt(plant, goal, s, x, iiwa.TIMESTEP, qd, r)
            torch.cuda.synchronize()
            for t, arr in zip(outs, "GCgc"):
                assert bool(torch.isfinite(t).all()), (name, arr)
                arrays[f"{B}x{N} {name} {arr}"] = sha(t)
            del outs, sol
        for name, args, opts in (("merit", h32, {}), ("merit merit_f32=1", h32, {"merit_f32": 1}), ("merit_f64", h64, {})):
            sol = PcgSolver(N, max_batch=B)
            for k, v in opts.items():
                sol.set_option(k, v)
            goal, s, x, z = args
            t = sol.compute_merit(plant, goal, s, x, z, STEPS9, iiwa.TIMESTEP, MU, qd, r)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(t).all()), name
            arrays[f"{B}x{N} {name} [9 step sizes]"] = sha(t)
        for name, args, ss in (("simulate", h32, 2e-4), ("simulate_f64", h64, 2e-4)):
            sol = PcgSolver(N, max_batch=B)
            _, s, x, _ = args
            s, pos = s.clone(), torch.zeros(B, 3, device=dev, dtype=s.dtype)
            sol.simulate(plant, s, x, iiwa.TIMESTEP, 15000.0, 2100.0, ss, eePos=pos)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(pos).all()), name
            arrays[f"{B}x{N} {name} state"] = sha(s)
            arrays[f"{B}x{N} {name} eePos"] = sha(pos)
    with open(out, "w") as f:
        json.dump({"root": os.path.basename(os.path.abspath(root)), "arrays": arrays}, f, indent=1)
    print(f"{len(arrays)} arrays -> {out}")
    return 0


def compare(a, b):
    A, B = (json.load(open(p))["arrays"] for p in (a, b))
    differ = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
    for k in differ:
        print("DIFFERS:", k)
    print(json.dumps({"arrays": len(set(A) | set(B)), "identical": len(set(A) | set(B)) - len(differ), "differ": len(differ)}))
    return 1 if differ else 0


if __name__ == "__main__":
    from ab_timing import select_build
    root = select_build()
    argv = sys.argv[1:]
    if len(argv) == 2 and argv[0] == "dump":
        sys.exit(dump(root, argv[1]))
    if len(argv) == 3 and argv[0] == "compare":
        sys.exit(compare(argv[1], argv[2]))
    sys.exit(__doc__)
