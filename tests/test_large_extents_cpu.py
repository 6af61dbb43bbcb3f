"""CPU: the large-extent checker (tests/large_extents.py) without a GPU — the conditions and the memory cap over every spec the GPU files
(tests/test_gpu_large_*.py) use, the per-knot byte constants the library's two route switches are made of, and defects planted in a numpy
model of a batched kernel with the wrap modulus scaled down from 2^32 to 2^16 (2^31 to 2^15): each must fail, by the array's name."""
import numpy as np
import pytest

import arena_specs as A
import large_extents as le

SPECS = le.all_specs()


@pytest.mark.parametrize("spec", SPECS, ids=[s.label for s in SPECS])
def test_every_spec_meets_the_conditions_and_the_memory_cap(spec):
    le.check_conditions(spec)
    assert spec.B % 4 != 0 and spec.D % 2 == 1 and spec.D >= 3 and spec.B % spec.D != 0
    assert le.need_bytes(spec) <= le.CAP_BYTES, (spec.label, le.need_bytes(spec))
    largest = max(le.nbytes(a, spec.B) for a in spec.arrays)
    assert largest >= 0.95 * 2 ** 31, (spec.label, largest)                 # every spec is about a line at 2^31 or 2^32 bytes (dz: knots x C's bytes per knot, C itself has N - 1)
    assert len({s.label for s in SPECS}) == len(SPECS)


def test_convert_spec():
    assert le.CONVERT_COUNT > 2 ** 31 - 1 and 4 * le.CONVERT_COUNT > 2 ** 33 and 2 * le.CONVERT_COUNT > 2 ** 32
    assert le.CONVERT_COUNT % 8 == 5 and le.CONVERT_COUNT % 2048 != 0          # a ragged tail, in the last block
    assert le.convert_need() <= le.CAP_BYTES


def test_per_knot_bytes_and_the_thresholds_in_knots():
    """The table of the issue, from the two functions mpcg_producers.hip switches by."""
    assert (le.schur_bytes_per_knot(14, 4), le.schur_bytes_per_knot(14, 8)) == (2352, 4704)            # S / Pinv
    assert (le.dz_bytes_per_knot(14, 7, 4), le.dz_bytes_per_knot(14, 7, 8)) == (1176, 2352)            # C
    assert ((196 + 49) * 4, (196 + 49) * 8) == (980, 1960)                                             # G
    first = lambda per: -(-2 ** 31 // per)                                                             # the first knot count on the LDS route
    assert (first(2352), first(4704)) == (913046, 456523)
    assert (first(1176) - 1, first(2352) - 1) == (1826091, 913045)                                      # dz: the last on the four-knot route


def test_formation_and_dz_batches_straddle_their_threshold_within_one_trajectory():
    for prec, (N, B, D) in le.FORM.items():
        per = le.schur_bytes_per_knot(14, le.E[prec]) * N
        assert B * per < 2 ** 31 <= (B + 1) * per and (N - 1 + 15) // 16 >= 2, prec
    assert (2 ** 31 - 41502 * 22 * 2352, 41503 * 22 * 2352 - 2 ** 31) == (4160, 47584)
    assert (2 ** 31 - 22826 * 20 * 4704, 22827 * 20 * 4704 - 2 ** 31) == (13568, 80512)
    for prec, (N, B, D) in le.FORM_4G.items():
        per = le.schur_bytes_per_knot(14, le.E[prec]) * N
        assert (B - 1) * per < 2 ** 32 < B * per, prec                        # the FIRST batch whose S passes 2^32 bytes
    assert (83005 * 22 * 2352 - 2 ** 32, 45653 * 20 * 4704 - 2 ** 32) == (43424, 66944)
    for prec, (N, B, D) in le.DZ.items():
        per = le.dz_bytes_per_knot(14, 7, le.E[prec]) * N
        assert B * per < 2 ** 31 <= (B + 1) * per, prec
    assert (2 ** 31 - 67633 * 27 * 1176, 67634 * 27 * 1176 - 2 ** 31) == (632, 31120)
    assert (2 ** 31 - 41502 * 22 * 2352, 41503 * 22 * 2352 - 2 ** 31) == (4160, 47584)


def test_pcg_specs_cover_the_families_of_the_plan_table():
    """Every float family the plan can select, fp16 storage, and the double families 8, 9, 10 (the double families 3 and 5 are pointer-indexed
    like their float twins, which run)."""
    import collections
    import json
    import os
    table = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "pcg_plan_table.json")))
    at = table["last_fields"].index("family")
    can = collections.defaultdict(set)
    for key, case in table["cases"].items():
        for call in case.get("calls", ()):
            if call.get("rc") == 0 and "last" in call:
                can[key.split("/")[0]].add(call["last"][at])
    mine = collections.defaultdict(set)
    for r in le.PCG_ROWS:
        mine[r.prec].add(r.family)
    assert mine["f32"] == can["f32"] == {0, 3, 5, 6, 7, 11}
    assert mine["f64"] == {8, 9, 10} <= can["f64"]
    assert le.f16_row().family in can["f16"]
    assert {r.n for r in le.PCG_ROWS if r.family == 3} == {13}
    for s in le.pcg_specs():
        S = next(a for a in s.arrays if a.name == "S")
        assert le.nbytes(S, s.B) > 2 ** 32 and le.nbytes(S, s.B - 8) <= 2 ** 32 + 8 * le.nbytes(S, 1), s.label
        assert all(a.const == (a.name in ("iters", "exits")) for a in s.arrays)


def test_pick_batch_is_the_first_admissible_batch_past_the_line():
    for per in (7056, 14112, 18252, 19992, 303408):
        B, D = le.pick_batch(2 ** 32, per)
        assert B * per > 2 ** 32 and B % 4 and B % D and D in (3, 5)
        assert all((b * per <= 2 ** 32) or b % 4 == 0 or (b % 5 == 0 and b % 3 == 0) for b in range(B - 6, B))


# ---- a numpy model of a batched kernel: y[b] = x[b] * rho[b] + e, flag[b] = 2 rho[b]; offsets computed as a kernel computes them ----
W16 = (2 ** 15, 2 ** 16)
T = 7


def model_spec(D, B):
    arrays = [le.arr("x", np.float32, T, "in"), le.arr("rho", np.float32, 1, "in"), le.arr("y", np.float32, T, "out"), le.arr("flag", np.uint8, 1, "out")]
    return le.Spec(f"model D{D} B{B}", arrays, D, B, 0)


def model_inputs(D):
    x = np.random.default_rng(5).standard_normal((D, T)).astype(np.float32)
    rho = (1.5 + np.arange(D)).astype(np.float32).reshape(D, 1)
    return {"x": x, "rho": rho}


def kernel(defect=None):
    W = 2 ** 16

    def call(a, Bt):
        x, rho, y, flag = (a[k].reshape(-1) for k in ("x", "rho", "y", "flag"))
        b = np.arange(Bt, dtype=np.int64)[:, None]
        e = np.arange(T, dtype=np.int64)[None, :]
        idx = b * T + e                                  # element index; byte offset 4 idx
        ld, st, rb = idx, idx, b
        loaded = np.ones(idx.shape, bool)
        stored = np.ones(idx.shape, bool)
        if defect == "load byte offset in 16 bits":
            ld = (4 * idx % W) // 4
        elif defect == "store byte offset in 16 bits":
            st = (4 * idx % W) // 4
        elif defect == "element index in 16 bits":
            ld = st = idx % W
        elif defect == "resource length truncated to 16 bits":
            records = 4 * Bt * T % W if 4 * Bt * T >= W else 4 * Bt * T       # accesses at or beyond it are dropped: loads give 0
            loaded = stored = 4 * idx < records
        elif defect == "store predicate offset < 2^15":
            stored = 4 * idx < 2 ** 15
        elif defect == "per-trajectory scalar offset in 16 bits":
            rb = (4 * b % W) // 4
        else:
            assert defect is None
        v = np.where(loaded, x[ld], np.float32(0)) * rho[rb] + e.astype(np.float32)
        y[st[stored]] = v[stored]
        flag[:] = (2 * rho).astype(np.uint8)
    return call


def test_the_correct_model_passes():
    out = le.run_numpy(model_spec(3, 9403), model_inputs(3), kernel(), W16)
    assert np.array_equal(out["y"], model_inputs(3)["x"] * model_inputs(3)["rho"] + np.arange(T, dtype=np.float32))


@pytest.mark.parametrize("defect,array", [("load byte offset in 16 bits", "y"), ("store byte offset in 16 bits", "y"), ("element index in 16 bits", "y"),
                                          ("resource length truncated to 16 bits", "y"), ("store predicate offset < 2^15", "y"),
                                          ("per-trajectory scalar offset in 16 bits", "y")])
def test_planted_defects_fail_by_name(defect, array):
    B = 16411 if defect.startswith("per-trajectory") or defect.startswith("element") else 9403        # 4 B > 2^16 / B T > 2^16 / 4 B T > 2^16
    with pytest.raises(AssertionError) as err:
        le.run_numpy(model_spec(3, B), model_inputs(3), kernel(defect), W16)
    text = str(err.value)
    assert f"array '{array}'" in text and "byte offset" in text and "mod 65536" in text, text
    if defect in ("store predicate offset < 2^15", "resource length truncated to 16 bits"):
        assert "never written" in text, text


def test_a_wrapped_scalar_is_invisible_with_four_tiles_and_the_d_condition_refuses_them():
    """2^16 mod (4 x 4) = 0: the wrapped rho of trajectory b is the rho of a trajectory with the same tile index, every comparison holds — the
    checker must refuse D = 4 before it compares anything."""
    spec, inputs, call = model_spec(4, 16411), model_inputs(4), kernel("per-trajectory scalar offset in 16 bits")
    big = {a.name: np.empty((spec.B, a.traj), a.dtype) for a in spec.arrays}
    small = {k: v.copy() for k, v in inputs.items()}
    small.update(y=np.zeros((4, T), np.float32), flag=np.zeros((4, 1), np.uint8))
    kernel()(small, 4)
    for a in spec.arrays[:2]:
        le.fill_tiled(a, big[a.name], inputs[a.name], 4, spec.B)
    call(big, spec.B)
    for a in spec.arrays:
        le.compare_tiled(a, big[a.name], small[a.name], 4, spec.B, "blind", W16)      # passes: the defect is invisible
    with pytest.raises(AssertionError, match="D condition"):
        le.run_numpy(spec, inputs, call, W16)
    with pytest.raises(AssertionError, match="D condition"):
        le.check_conditions(model_spec(3, 9402))                                    # B a multiple of D
    with pytest.raises(AssertionError, match="multiple of 4"):
        le.check_conditions(model_spec(3, 9404))


def test_even_tile_counts_equal_tiles_and_modified_inputs_are_refused():
    arrays = [le.arr("x", np.float32, 2 ** 10, "in"), le.arr("y", np.float32, 2 ** 10, "out")]
    with pytest.raises(AssertionError, match="D condition"):
        le.check_conditions(le.Spec("blind", arrays, 2, 17, 0))
    spec = model_spec(3, 9403)
    inputs = model_inputs(3)
    inputs["x"][2] = inputs["x"][0]
    inputs["rho"][2] = inputs["rho"][0]
    with pytest.raises(AssertionError, match="carry the same bits"):
        le.run_numpy(spec, inputs, kernel(), W16)
    with pytest.raises(AssertionError, match="input array 'x' was modified"):
        le.run_numpy(model_spec(3, 9403), model_inputs(3), lambda a, Bt: (kernel()(a, Bt), a["x"].__setitem__((0, 0), 1.0)), W16)


def test_masks_and_roles_come_from_the_arena_specs():
    arrays = {a.name: a for a in le.from_arena(A.form_schur("f32", 14, 7, 22, 1, "jacobi", True))}
    assert arrays["G"].role == "inout" and arrays["rho"].traj == 1 and arrays["S"].mask.sum() == 2 * 196
    assert arrays["Pinv"].mask.sum() == 2 * 22 * 196                 # block-Jacobi: every off-diagonal block keeps the caller's bytes
