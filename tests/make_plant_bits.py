#!/usr/bin/env python3
"""Record what every kernel selection of mpcgpu_amd/csrc/mpcg_plant.hip computes, for tests/test_gpu_plant_bits.py.

Run ONCE, on the GPU, on the commit whose results a change of the host path has to reproduce bit for bit:
    python tests/make_plant_bits.py [--commit HASH] [--out PATH]      ->  tests/golden/plant_bits_parent.json
(HASH defaults to `git rev-parse HEAD`; it is stored in the file.)  Only the public Python API is used.

Selections, 36 + 18 + 8 = 62 (one kernel instantiation each):
    kkt    T in {float, double} x build x integrator in {0, 1} x COST in {0, 1, 2}; the float builds are the default, "kkt_analytic" = 0, "kkt_f32" = 1 and
           "kkt_f32" = 2, the double builds "kkt_analytic" = 1 and 0.  COST 0: generate_kkt; 1: generate_kkt_xuref with the plain plant; 2: with a limits plant.
    merit  {float, float with "merit_f32", double} x integrator x COST, the entries as above.
    sim    T x "sim_integrator" x {plain plant, limits plant with sim_saturate}.
Inputs: the seeded cases and the limits builders of tests/test_gpu_xuref.py and tests/test_gpu_limits.py (imported, read-only), the cost setting COSTS["all"]
(q_cost != 0, both relative flags), limits cut from each case's own values, so that they are violated.  The double selections get the genuinely double twin of
each case.  Shapes, the smallest at which each kernel's packing can go wrong:
    kkt    N = 4, B = 3: nine (trajectory, knot) items — in the packed build a lane pair straddles two trajectories and the last pair has a dead half; the four
           groups of a wavefront hold knots of different trajectories, and the k == 0 and k == N - 2 paths occur in one wavefront.
    merit  N = 3, B = 3, step sizes (0, -1/2, -1): 27 items, an odd count for the packed build; a zero and a moving step.
    sim    N = 5, B = 5: two wavefronts, the second partly empty; the call of test_simulate_saturates_at_the_torque_limits (it starts 14,000 us into knot 0,
           substeps of 1/128 s) over 3.5 substeps: three full ones and a remainder, across two knot boundaries.
Stored: the commit, one SHA-256 of the input bytes, and per selection and output array its shape and the SHA-256 of its bytes — digests, not arrays: a mismatch
names the selection and the array, which is what finds a wrong choice of kernel.

Before anything is written: every selection is run twice from fresh solvers and gives the same digests; every output is finite; and selections that are meant
to differ do differ (explicit and semi-implicit, the three COST values pairwise, analytic and difference quotients, float64-inside and float arithmetic,
saturating and plain simulate) — the case a wrong instantiation must not hide in.  "kkt_f32" = 1 against 2 is not required to differ.
"""
import hashlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
OUT = os.path.join(ROOT, "tests", "golden", "plant_bits_parent.json")

KKT_SHAPE, MERIT_SHAPE, SIM_SHAPE = (4, 3), (3, 3), (5, 5)
MERIT_STEPS = (0.0, -0.5, -1.0)
SIM_CALL = dict(time_offset_us=14000.0, sim_time_us=3.5e6 / 128, sim_step=1 / 128)
KKT_BUILDS = {"float": {"default": (), "difference": (("kkt_analytic", 0),), "kkt_f32=1": (("kkt_f32", 1),), "kkt_f32=2": (("kkt_f32", 2),)},
              "double": {"analytic": (("kkt_analytic", 1),), "difference": (("kkt_analytic", 0),)}}
MERIT_BUILDS = {"float": ("float", ()), "float+merit_f32": ("float", (("merit_f32", 1),)), "double": ("double", ())}
DTYPES = {"float": np.float32, "double": np.float64}


def selections():
    """Every key of the record, in order: 36 kkt, 18 merit, 8 sim."""
    keys = [f"kkt/{T}/{build}/integrator={i}/cost={c}" for T in KKT_BUILDS for build in KKT_BUILDS[T] for i in (0, 1) for c in (0, 1, 2)]
    keys += [f"merit/{build}/integrator={i}/cost={c}" for build in MERIT_BUILDS for i in (0, 1) for c in (0, 1, 2)]
    keys += [f"sim/{T}/sim_integrator={i}/{p}" for T in DTYPES for i in (0, 1) for p in ("plain", "saturate")]
    return keys


def _limit_arrays(lim):
    return [np.asarray(getattr(lim, k), np.float64) for k in ("q_lo", "q_hi", "qd_lo", "qd_hi", "u_lo", "u_hi", "q_weight", "qd_weight", "u_weight")]


def inputs():
    """The cases and limits of every family (the imported builders cache them) and the SHA-256 of all their bytes."""
    import test_gpu_limits as TL
    import test_gpu_xuref as TX
    h = hashlib.sha256()
    for (N, B), limits in ((KKT_SHAPE, TL.kkt_limits), (MERIT_SHAPE, TL.merit_limits), (SIM_SHAPE, TL.kkt_limits)):
        for double in (False, True):
            if (N, B) == SIM_SHAPE and double:
                continue                                       # simulate: one case for both precisions, as the suite's own test
            cs = TX.case(N, B, double)
            for a in (cs.xu, cs.goals, cs.xs, cs.dz, cs.plan, cs.offsets, *_limit_arrays(limits(N, B, double))):
                h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run(key):
    """One selection from a fresh solver: {array name: numpy array}."""
    import torch
    import test_gpu_limits as TL
    import test_gpu_xuref as TX
    family, *parts = key.split("/")
    co = TX.COSTS["all"]
    if family == "sim":
        T, integ, which = parts
        dtype = DTYPES[T]
        N, B = SIM_SHAPE
        cs = TX.case(N, B)
        lim = TL.kkt_limits(N, B)
        u = cs.xu[:, :21 * (N - 1)].reshape(B, N - 1, 21)[:, :, 14:]
        assert ((u < lim.u_lo) | (u > lim.u_hi)).any(), "no control beyond its bound: the saturating kernel would have nothing to clamp"
        pl = TL.with_limits(lim, sim_saturate=True) if which == "saturate" else TX.plant()
        sol = TX.solver(N, B)
        sol.set_option("sim_integrator", int(integ[-1]))
        xs = TX.dev(cs.xs, dtype)
        ee = torch.zeros(B, 3, device="cuda", dtype=xs.dtype)
        sol.simulate(pl, xs, TX.dev(cs.xu, dtype), TX.DT, SIM_CALL["time_offset_us"], SIM_CALL["sim_time_us"], SIM_CALL["sim_step"], eePos=ee)
        torch.cuda.synchronize()
        return {"xs": xs.cpu().numpy(), "eePos": ee.cpu().numpy()}
    if family == "kkt":
        T, build, integ, cost = parts
        opts, (N, B) = KKT_BUILDS[T][build], KKT_SHAPE
    else:
        build, integ, cost = parts
        (T, opts), (N, B) = MERIT_BUILDS[build], MERIT_SHAPE
    dtype, cost = DTYPES[T], int(cost[-1])
    cs = TX.case(N, B, T == "double")
    sol = TX.solver(N, B, opts, int(integ[-1]))
    if family == "kkt":
        if cost == 0:
            out = sol.generate_kkt(TX.plant(), TX.dev(cs.goals, dtype), TX.dev(cs.xs, dtype), TX.dev(cs.xu, dtype), TX.DT, co.qd_cost, co.r_cost)
        elif cost == 1:
            out = cs.kkt(sol, co, dtype)
        else:
            out = TL.kkt(cs, sol, co, TL.with_limits(TL.kkt_limits(N, B, T == "double")), dtype)
        torch.cuda.synchronize()
        return {name: t.cpu().numpy() for name, t in zip(("G", "C", "g", "c"), out)}
    if cost == 0:
        out = sol.compute_merit(TX.plant(), TX.dev(cs.goals, dtype), TX.dev(cs.xs, dtype), TX.dev(cs.xu, dtype), TX.dev(cs.dz, dtype), MERIT_STEPS, TX.DT, TX.MU,
                                co.qd_cost, co.r_cost)
    elif cost == 1:
        out = cs.merit(sol, co, MERIT_STEPS, dtype)
    else:
        out = TL.merit(cs, sol, co, TL.with_limits(TL.merit_limits(N, B, T == "double")), MERIT_STEPS, dtype)
    torch.cuda.synchronize()
    return {"merit": out.cpu().numpy()}


def digests(arrays):
    return {name: {"shape": list(a.shape), "sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()} for name, a in arrays.items()}


def must_differ(rec):
    """The pairs of selections that differ in one axis whose two values are meant to compute different numbers."""
    def axes(key):
        p = key.split("/")
        return (p[0], tuple(p[1:-3]), p[-3], p[-2], p[-1]) if p[0] == "kkt" else (p[0], (), p[1], p[2], p[3])      # family, T, build or T, integrator, cost or plant
    same_arithmetic = ({"kkt_f32=1", "kkt_f32=2"},)
    pairs = []
    for a, b in itertools.combinations(rec, 2):
        xa, xb = axes(a), axes(b)
        if xa[:2] != xb[:2] or sum(p != q for p, q in zip(xa[2:], xb[2:])) != 1:
            continue
        if xa[0] == "merit" and xa[2] != xb[2] and "double" in (xa[2], xb[2]):
            continue                                           # float against double arrays: other inputs, other sizes
        if xa[0] == "sim" and xa[2] != xb[2]:
            continue
        if {xa[2], xb[2]} in same_arithmetic:
            continue
        pairs.append((a, b))
    return pairs


def write(record, path):
    """Strict JSON, one line per output array, so that a re-recording shows in a diff as the arrays that moved."""
    lines = []
    for key, arrays in record["selections"].items():
        rows = ",\n".join(f"   {json.dumps(name)}: {json.dumps(d, sort_keys=True)}" for name, d in arrays.items())
        lines.append(f"  {json.dumps(key)}: {{\n{rows}}}")
    with open(path, "w") as f:
        f.write(f'{{"commit": {json.dumps(record["commit"])},\n "inputs_sha256": {json.dumps(record["inputs_sha256"])},\n "selections": {{\n' + ",\n".join(lines) + "}}\n")


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else OUT
    if "--commit" in args:
        commit = args[args.index("--commit") + 1]
    else:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    record = {"commit": commit, "inputs_sha256": inputs(), "selections": {}}
    for key in selections():
        first, second = run(key), run(key)
        for name, a in first.items():
            if not np.isfinite(a).all():
                raise SystemExit(f"{key}: {name} is not finite")
        if digests(first) != digests(second):
            raise SystemExit(f"{key}: two runs from fresh solvers give different bits")
        record["selections"][key] = digests(first)
    sel = record["selections"]
    pairs = must_differ(sel)
    same = [(a, b) for a, b in pairs if sel[a] == sel[b]]
    if same:
        raise SystemExit("selections that are meant to differ compute the same bits:\n" + "\n".join(f"  {a}  ==  {b}" for a, b in same))
    write(record, out_path)
    print(f"wrote {out_path}: {len(sel)} selections, {len(pairs)} pairs checked to differ, {os.path.getsize(out_path)} bytes, commit {commit}")


if __name__ == "__main__":
    main()
