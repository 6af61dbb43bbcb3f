"""Non-finite containment: a trajectory whose floating-point data are Inf, NaN or about to overflow harms no neighbour in the batch.  No GPU here.

An entry is run twice on the same handle configuration — once with healthy data, once with one input array of some trajectories poisoned —
and `check` asserts ONE thing: every output array of every trajectory outside the poisoned set carries the bits of the clean run.  There is no
tolerance: the reference of a case is the same call with healthy data in the poisoned slots, which the suites of each entry pin to their float64
restatements.  Bit patterns are compared (uint32 / uint64 views), so the NaN fill of a never-written slot equals itself.

Only floating-point DATA arrays are poisoned: integer arrays (traj_offset, mpc_done, done), host scalars and whatever the host validates stay
as they are (`poison` refuses anything else).

tests/test_containment_cpu.py holds this file to account with numpy models of four-items-per-wavefront kernels and planted defects."""
import numpy as np

SETS = ((1,), (5,), (0, 3))          # of B = 6: inside a wavefront of four; the last trajectory, the one dead rows redo; the first and a pair with healthy ones between and after
B = 6
HUGE = {np.dtype(np.float32): 3e38, np.dtype(np.float64): 1e308}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


# ---- poison patterns: each a function of ONE trajectory's copy of a floating-point input array (1-D, modified in place and returned) ----
def nan_one(a, pos):
    a[pos] = np.nan
    return a


def inf_one(a, pos):
    a[pos] = np.inf
    return a


def nan_all(a):
    a[:] = np.nan
    return a


def huge(a, start, length):
    """Finite +-3e38 (float) / +-1e308 (double), alternating, in one block: the non-finite value is produced inside the kernel, not loaded."""
    v = HUGE[a.dtype]
    blk = a[start:start + length]
    blk[:] = np.where(np.arange(blk.size) % 2 == 0, v, -v).astype(a.dtype)
    return a


def zero_all(a):
    """The trajectory's matrices all zero: a 0 / 0 inside."""
    a[:] = 0
    return a


def positions(L):
    """The single-element positions: the first element of the trajectory, one in the middle, and the last — adjacent in memory and in the item
    flattening to the next trajectory's first."""
    out, seen = {}, set()
    for where, pos in (("first", 0), ("last", L - 1), ("middle", L // 2)):          # (a one- or two-element array: each position once)
        if pos not in seen:
            out[where] = pos
            seen.add(pos)
    return out


def patterns(L, block=14, matrix=False):
    """[(label, fn)] for an array of L elements per trajectory: the two single-element patterns at every position, nan_all, huge in the block
    of `block` elements around the middle, and for matrices zero_all."""
    out = []
    for name, fn in (("nan_one", nan_one), ("inf_one", inf_one)):
        for where, pos in positions(L).items():
            out.append((f"{name}@{where}", lambda a, fn=fn, pos=pos: fn(a, pos)))
    out.append(("nan_all", nan_all))
    blk = min(block, L)
    start = min((L // 2) // blk * blk, L - blk)
    out.append(("huge", lambda a: huge(a, start, blk)))
    if matrix:
        out.append(("zero_all", zero_all))
    return out


def poison(array, poisoned_set, fn):
    """A copy of `array` ([B, ...], floating point) with fn applied to the flattened copy of every trajectory of the set."""
    array = np.asarray(array)
    if array.dtype not in HUGE:
        raise TypeError(f"only float32 / float64 data arrays are poisoned, not {array.dtype}")
    out = np.array(array, copy=True)
    flat = out.reshape(out.shape[0], -1)
    for b in poisoned_set:
        flat[b] = fn(flat[b].copy())
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(UINT[a.dtype.itemsize]) if a.dtype.kind in "fc" else a.reshape(-1)


def neighbour(b, poisoned_set):
    """'trajectory p (d behind / ahead)' of the nearest poisoned trajectory."""
    if not poisoned_set:
        return "no poisoned trajectory"
    p = min(poisoned_set, key=lambda q: (abs(q - b), q))
    d = b - p
    return f"poisoned trajectory {p}" + (" (directly adjacent)" if abs(d) == 1 else f" ({abs(d)} {'behind' if d > 0 else 'ahead of'} it)")


def check(clean_outputs, poisoned_outputs, poisoned_set, per_trajectory_slices=None, entry="entry"):
    """Every output array, every trajectory NOT in poisoned_set: bit-for-bit equality of the two runs.  per_trajectory_slices: {array name:
    [index of trajectory 0, index of trajectory 1, ...]} for arrays that are not [B, ...] (default: a[b]).  The poisoned trajectories' own
    outputs are not looked at.  The message names the entry, the array, the trajectory, the first differing element and the poisoned
    trajectory it is nearest to."""
    poisoned_set = tuple(poisoned_set)
    assert sorted(clean_outputs) == sorted(poisoned_outputs), (entry, sorted(clean_outputs), sorted(poisoned_outputs))
    for name in sorted(clean_outputs):
        c, p = np.asarray(clean_outputs[name]), np.asarray(poisoned_outputs[name])
        assert c.shape == p.shape and c.dtype == p.dtype, (entry, name, c.shape, p.shape, c.dtype, p.dtype)
        sl = (per_trajectory_slices or {}).get(name)
        count = len(sl) if sl is not None else c.shape[0]
        for b in range(count):
            if b in poisoned_set:
                continue
            idx = sl[b] if sl is not None else b
            cb, pb = _bits(c[idx]), _bits(p[idx])
            if np.array_equal(cb, pb):
                continue
            e = int(np.flatnonzero(cb != pb)[0])
            vc, vp = np.asarray(c[idx]).reshape(-1)[e], np.asarray(p[idx]).reshape(-1)[e]
            raise AssertionError(f"{entry}: array '{name}' of healthy trajectory {b} differs from the clean run at element {e} "
                                 f"({vp!r} against {vc!r}; {int((cb != pb).sum())} of {cb.size} elements differ); nearest: {neighbour(b, poisoned_set)} "
                                 f"of the poisoned set {sorted(poisoned_set)}")


def differs(clean_outputs, poisoned_outputs, poisoned_set, per_trajectory_slices=None):
    """Does any output of a POISONED trajectory differ between the two runs?  (What `check` does not look at: the poison arrived.)"""
    for name in clean_outputs:
        c, p = np.asarray(clean_outputs[name]), np.asarray(poisoned_outputs[name])
        sl = (per_trajectory_slices or {}).get(name)
        for b in poisoned_set:
            idx = sl[b] if sl is not None else b
            if not np.array_equal(_bits(c[idx]), _bits(p[idx])):
                return True
    return False


def sweep(entry, inputs, poisonable, run, sets=SETS, slices=None, matrices=(), blocks=None, own=None, only=None):
    """run(inputs) -> {name: numpy array} is called once on the healthy inputs and once per (array of `poisonable`, pattern, poisoned set) with
    that array poisoned; `check` after each.  matrices: arrays that also get zero_all; blocks: {array: block length of `huge`}; own(outputs,
    poisoned_set, label): further assertions on the poisoned trajectories themselves; only: restrict the patterns to these labels.
    Every array of `poisonable` must change an output of a poisoned trajectory in at least one case.  Returns the number of poisoned runs."""
    clean = run(inputs)
    runs = 0
    for name in poisonable:
        L = int(np.asarray(inputs[name])[0].size)
        reached = False
        for label, fn in patterns(L, (blocks or {}).get(name, 14), name in matrices):
            if only is not None and label not in only:
                continue
            for pset in sets:
                bad = dict(inputs)
                bad[name] = poison(inputs[name], pset, fn)
                out = run(bad)
                tag = f"{entry} [{name} <- {label}]"
                check(clean, out, pset, slices, tag)
                if own is not None:
                    own(out, pset, tag)
                reached = reached or differs(clean, out, pset, slices)
                runs += 1
        # (a sweep that never changes the poisoned trajectories' own outputs has not reached the kernel: a wrong array name, an input the entry ignores)
        assert reached, f"{entry}: poisoning '{name}' never changed an output of a poisoned trajectory"
    return runs
