"""The containment helper (tests/containment.py) is honest — no GPU.  A numpy model of a "four items per wavefront" kernel — six trajectories of
three items (the KKT items of N = 4), one item per 16-lane row, four rows per wavefront, so wavefronts and packed pairs straddle trajectories
and the last wavefront has two dead rows that redo the last item — is correct as written and passes the whole sweep; each planted defect
fails, and the message names the array, the healthy trajectory that was harmed and the poisoned trajectory next to it."""
import numpy as np
import pytest

import containment as ct

B, K, W = ct.B, 3, 16
ITEMS = B * K
DONE = np.array([0, 0, 1, 0, 0, 0], np.int32)             # trajectory 2 is frozen: its rows are dead, its outputs are never written (NaN fill)


def model(x, done, defect=None, dtype=np.float32):
    """y[item] = x[item] / max |x[item]| + (x[item + 1][0] if the next item belongs to the same trajectory), s[b] = the sum of y over b's items.
    Rows without an item of their own — behind the last item, or of a frozen trajectory — redo the last item and store nothing."""
    x = np.asarray(x, dtype).reshape(ITEMS, W)
    y = np.full((ITEMS, W), np.nan, dtype)
    s = np.full(B, np.nan, dtype)
    with np.errstate(all="ignore"):
        for w0 in range(0, ITEMS + (-ITEMS) % 4, 4):
            rows = list(range(w0, w0 + 4))
            live = [i < ITEMS and not done[i // K] for i in rows]
            src = [i if ok else ITEMS - 1 for i, ok in zip(rows, live)]           # a dead row redoes the last item
            wave = np.stack([x[i] for i in src])
            for r, (i, ok, j) in enumerate(zip(rows, live, src)):
                scale = np.abs(wave).max() if defect == "row_reduction_over_the_wavefront" else np.abs(wave[r]).max()
                if defect == "pair_partner_leaks":                                # items 2 p and 2 p + 1 share a packed value: the scale of both halves
                    mate = j ^ 1
                    scale = np.maximum(scale, np.abs(x[mate]).max()) if mate < ITEMS else scale
                nxt = min(j + 1, ITEMS - 1)
                same = (j + 1) // K == j // K and j + 1 < ITEMS
                halo = dtype(same) * x[nxt][0] if defect == "select_by_multiplication" else (x[nxt][0] if same else dtype(0))
                v = wave[r] / scale + halo
                if ok:
                    y[i] = v
                elif defect == "dead_row_stores" and i < ITEMS:
                    y[i] = v
    y = y.reshape(B, K, W)
    with np.errstate(all="ignore"):
        for b in range(B):
            if not done[b]:
                s[b] = y[b].sum(dtype=dtype)
    return {"y": y, "s": s}


def inputs():
    return {"x": np.random.default_rng(3).standard_normal((B, K, W)).astype(np.float32)}


def run(defect):
    return lambda a: model(a["x"], DONE, defect)


def test_the_correct_model_passes_the_whole_sweep():
    """Also the two cases that must NOT fail: the frozen trajectory's outputs are the NaN fill in both runs (equal as bit patterns, unequal as
    floats), and a poisoned trajectory's own outputs differ from the clean run's in every case."""
    seen = []

    def own(out, pset, tag):
        clean = model(inputs()["x"], DONE)
        for b in pset:
            seen.append(not np.array_equal(out["y"][b].view(np.uint32), clean["y"][b].view(np.uint32)))
    runs = ct.sweep("model", inputs(), ["x"], run(None), matrices=("x",), blocks={"x": W}, own=own)
    assert runs == 9 * len(ct.SETS) and all(seen) and len(seen) == 9 * 4
    clean = model(inputs()["x"], DONE)
    assert np.isnan(clean["y"][2]).all() and np.isnan(clean["s"][2]) and np.isfinite(clean["y"][[0, 1, 3, 4, 5]]).all()


# (defect, pattern label, poisoned set, the healthy trajectory that is harmed, what the message says of the neighbour)
DEFECTS = [("select_by_multiplication", "nan_one@first", (1,), 0, "poisoned trajectory 1 (directly adjacent)"),
           ("select_by_multiplication", "inf_one@first", (0, 3), 2, "poisoned trajectory 3 (directly adjacent)"),
           ("row_reduction_over_the_wavefront", "nan_all", (1,), 0, "poisoned trajectory 1 (directly adjacent)"),
           ("row_reduction_over_the_wavefront", "huge", (1,), 2, "poisoned trajectory 1 (directly adjacent)"),
           ("row_reduction_over_the_wavefront", "nan_one@first", (5,), 4, "poisoned trajectory 5 (directly adjacent)"),
           ("dead_row_stores", "nan_one@last", (5,), 2, "poisoned trajectory 5 (3 ahead of it)"),
           ("pair_partner_leaks", "nan_one@first", (1,), 0, "poisoned trajectory 1 (directly adjacent)"),
           ("pair_partner_leaks", "zero_all", (0, 3), 1, "poisoned trajectory 0 (directly adjacent)")]


@pytest.mark.parametrize("defect,label,pset,harmed,says", DEFECTS, ids=[f"{d[0]}-{d[1]}-{'_'.join(map(str, d[2]))}" for d in DEFECTS])
def test_every_planted_defect_fails_by_name(defect, label, pset, harmed, says):
    done = DONE if defect == "dead_row_stores" else np.where(np.arange(B) == 2, 0, DONE)      # (trajectory 2 live: it is the one harmed in two rows)
    fn = dict(ct.patterns(K * W, W, matrix=True))[label]
    x = inputs()["x"]
    clean = model(x, done, defect)
    bad = model(ct.poison(x, pset, fn), done, defect)
    with pytest.raises(AssertionError) as e:
        ct.check(clean, bad, pset, entry=f"model [{label}]")
    msg = str(e.value)
    assert f"model [{label}]" in msg and f"healthy trajectory {harmed} " in msg and says in msg and "at element " in msg, msg
    assert ("array 's'" in msg) or ("array 'y'" in msg), msg
    ct.check(model(x, done), model(ct.poison(x, pset, fn), done), pset)          # the same case on the correct model passes


def test_each_defect_is_found_by_the_sweep_and_by_no_finite_comparison():
    """Finite data cannot reveal them: the planted models agree with themselves on healthy data (what the composition tests compare), and for
    each of them the sweep raises."""
    for defect in sorted({d[0] for d in DEFECTS}):
        with pytest.raises(AssertionError, match="healthy trajectory"):
            ct.sweep("model", inputs(), ["x"], run(defect), matrices=("x",), blocks={"x": W})


def test_a_difference_in_a_healthy_trajectory_names_its_first_element_and_counts():
    clean = {"y": np.zeros((B, 5), np.float64), "flag": np.zeros(B, np.int32)}
    bad = {"y": clean["y"].copy(), "flag": clean["flag"].copy()}
    bad["y"][1] = np.nan                                                            # the poisoned trajectory itself: not looked at
    ct.check(clean, bad, (1,))
    bad["flag"][4] = 1                                                              # integer outputs of healthy trajectories are checked too
    with pytest.raises(AssertionError, match=r"array 'flag' of healthy trajectory 4 .* element 0 .*poisoned trajectory 1 \(3 behind it\)"):
        ct.check(clean, bad, (1,))
    bad["flag"][4] = 0
    bad["y"][2, 3] = -0.0                                                           # a sign bit is a difference: bit patterns, not values
    with pytest.raises(AssertionError, match=r"array 'y' of healthy trajectory 2 .* element 3 .*1 of 5 elements.*directly adjacent"):
        ct.check(clean, bad, (1,))


def test_a_sweep_that_never_reaches_the_entry_fails():
    """An input the entry ignores: the poisoned trajectories' outputs never change, and the sweep says so instead of passing empty."""
    ignores = lambda a: {"y": np.ones((B, 4), np.float32)}
    with pytest.raises(AssertionError, match="poisoning 'x' never changed an output of a poisoned trajectory"):
        ct.sweep("model", inputs(), ["x"], ignores)


def test_per_trajectory_slices_for_arrays_that_are_not_batch_major():
    clean = {"t": np.arange(12.0).reshape(2, 6)}                                    # [row, trajectory]
    bad = {"t": clean["t"].copy()}
    sl = {"t": [(slice(None), b) for b in range(6)]}
    bad["t"][:, 5] = np.inf
    ct.check(clean, bad, (5,), sl)
    bad["t"][1, 0] = 7.0
    with pytest.raises(AssertionError, match="healthy trajectory 0 .* element 1 "):
        ct.check(clean, bad, (5,), sl)


def test_patterns_and_what_may_be_poisoned():
    labels = [l for l, _ in ct.patterns(10, 4, matrix=True)]
    assert labels == ["nan_one@first", "nan_one@last", "nan_one@middle", "inf_one@first", "inf_one@last", "inf_one@middle", "nan_all", "huge", "zero_all"]
    assert [l for l, _ in ct.patterns(1)] == ["nan_one@first", "inf_one@first", "nan_all", "huge"]
    for dt, v in ((np.float32, 3e38), (np.float64, 1e308)):
        a = ct.poison(np.ones((B, 10), dt), (0, 3), dict(ct.patterns(10, 4))["huge"])
        assert np.isfinite(a).all() and (np.abs(a[0, 4:8]) == dt(v)).all() and a[0, 4] == -a[0, 5] and (a[[1, 2, 4, 5]] == 1).all() and (a[3] == a[0]).all()
        assert (np.delete(a[0], range(4, 8)) == 1).all()
    a = ct.poison(np.ones((B, 2, 5), np.float32), (5,), dict(ct.patterns(10))["nan_one@last"])
    assert np.isnan(a[5, 1, 4]) and np.isnan(a).sum() == 1
    assert np.isposinf(ct.poison(np.ones((B, 10)), (1,), dict(ct.patterns(10))["inf_one@middle"])[1, 5])
    for bad in (np.zeros(B, np.int32), np.zeros(B, np.uint8)):
        with pytest.raises(TypeError, match="only float32 / float64 data arrays"):
            ct.poison(bad, (1,), ct.nan_all)
