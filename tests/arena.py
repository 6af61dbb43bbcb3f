"""Guard-banded arena: every array of one library call carved out of ONE allocation filled with 0xFF bytes, so that a kernel which reads or
writes past an array, or writes an array it was told to leave alone, is caught exactly, on small inputs, with no tolerance.

0xFF bytes are a NaN in half, float and double, -1 in int32 and 255 in uint8: one pattern poisons every input band (a value read from a band
and used in arithmetic surfaces as NaN) and marks every output (an element nobody wrote still holds it).

A call's arrays are described by specs (spec()): name, numpy dtype, element count, role, smallest alignment the entry accepts, and the
extents the bands are sized from.  Roles:
  in         must come back bit-identical
  out        every element must be written (mask: elements the header says are NOT written — they must keep what they held)
  inout      read and written; float elements must come back finite (mask as for out)
  untouched  passed to the call, must keep the fill
layout() is a pure function of the specs (no numpy arrays, no torch): offsets and bands in bytes.
  bands      one between any two arrays, one before the first and one after the last.  Interior: >= 4 KiB and >= two knots' extent of each
             neighbour.  First and last: >= 64 KiB and >= the largest single-trajectory extent in the arena, so an over-access of a whole
             trajectory still lands inside the allocation and is a test failure, not a fault.
  "aligned"  every array starts on a multiple of 256 bytes
  "minimal"  every array starts at exactly its smallest accepted alignment a: offset = a (mod 2a)
Arena(specs, mode, backing) holds the memory — "numpy" (CPU tests; fake entries poke Arena.raw) or "torch" (one uint8 CUDA tensor; view()
gives typed tensors whose data pointers the library sees).  run(fn) snapshots the allocation, calls fn(views), and verifies:
  1. every band byte is still 0xFF (the failure names the array, the side and the byte offset of the first damage);
  2. every in / untouched array is bit-identical to what went in;
  3. no must-write element still holds what it held before the call (the fill, or a sentinel put() there when the fill is a legitimate
     value of the output), and unmasked float outputs are finite;
  4. masked elements still hold what they held.
It returns the out / inout arrays (numpy copies) for the caller to compare.
What it cannot see: an over-read whose value is discarded by a predicate rather than by arithmetic, and anything in handle-owned scratch."""
import collections

import numpy as np

FILL = 0xFF
ROLES = ("in", "out", "inout", "untouched")
MODES = ("aligned", "minimal")
INTERIOR_MIN = 4096
EDGE_MIN = 65536

Spec = collections.namedtuple("Spec", "name dtype count role align knot traj mask")
Layout = collections.namedtuple("Layout", "offset nbytes bands total")      # bands: (start, end, name before or None, name after or None)


def spec(name, dtype, count, role, align=None, knot=1, traj=None, mask=None):
    """knot / traj: elements of one knot (S, Pinv: one block row) and of one trajectory (default: the whole array).  mask: bool [count],
    True = not written by the call."""
    dt = np.dtype(dtype)
    assert role in ROLES, role
    align = dt.itemsize if align is None else int(align)
    assert align >= dt.itemsize and align % dt.itemsize == 0 and align & (align - 1) == 0, (name, align)
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=bool).reshape(-1)
        assert mask.size == count and role in ("out", "inout"), name
    return Spec(name, dt, int(count), role, align, int(knot), int(count if traj is None else traj), mask)


def _up(x, a):
    return -(-x // a) * a


def _place(pos, align, mode):
    if mode == "aligned":
        return _up(pos, 256)
    p = _up(pos, align)
    return p + align if p % (2 * align) == 0 else p


def layout(specs, mode):
    assert mode in MODES, mode
    assert len({s.name for s in specs}) == len(specs) > 0
    size = lambda s, elems: elems * s.dtype.itemsize
    edge = max([EDGE_MIN] + [size(s, s.traj) for s in specs])
    offset, nbytes, bands = {}, {}, []
    pos, prev = 0, None
    for s in specs:
        gap = edge if prev is None else max(INTERIOR_MIN, 2 * size(prev, prev.knot), 2 * size(s, s.knot))
        off = _place(pos + gap, s.align, mode)
        bands.append((pos, off, prev.name if prev else None, s.name))
        offset[s.name], nbytes[s.name] = off, size(s, s.count)
        pos, prev = off + nbytes[s.name], s
    total = _up(pos + edge, 256)
    bands.append((pos, total, prev.name, None))
    return Layout(offset, nbytes, tuple(bands), total)


def _first(bad):
    return int(np.flatnonzero(bad)[0])


def verify(specs, lay, before, after):
    """The four checks on two snapshots (uint8 numpy arrays of the whole allocation).  AssertionError names the array."""
    for start, end, left, right in lay.bands:
        bad = after[start:end] != FILL
        if bad.any():
            i = _first(bad)
            where = []
            if left is not None:
                where.append(f"after array '{left}': first damaged byte {i} bytes past its end")
            if right is not None:
                where.append(f"before array '{right}': first damaged byte {end - start - i} bytes ahead of its start")
            raise AssertionError("band written, " + "; ".join(where) + f" ({int(bad.sum())} bytes damaged)")
    outs = {}
    for s in specs:
        off, nb, w = lay.offset[s.name], lay.nbytes[s.name], s.dtype.itemsize
        b = before[off:off + nb].reshape(s.count, w)
        a = after[off:off + nb].reshape(s.count, w)
        changed = (a != b).any(axis=1)
        if s.role in ("in", "untouched"):
            if changed.any():
                what = "input array" if s.role == "in" else "array the call must leave untouched"
                raise AssertionError(f"{what} '{s.name}' was modified: first at element {_first(changed)} of {s.count}")
            continue
        masked = s.mask if s.mask is not None else np.zeros(s.count, bool)
        if (changed & masked).any():
            raise AssertionError(f"array '{s.name}': element {_first(changed & masked)} is one the call must not write, and it was written")
        values = np.frombuffer(after[off:off + nb].tobytes(), dtype=s.dtype)
        if s.role == "out" and (~changed & ~masked).any():
            raise AssertionError(f"output array '{s.name}': element {_first(~changed & ~masked)} of {s.count} still holds the fill: never written"
                                 + (", or computed from a fill NaN that was read (its payload propagates)" if s.dtype.kind == "f" else ""))
        if s.dtype.kind == "f":
            bad = ~np.isfinite(values) & ~masked
            if bad.any():
                raise AssertionError(f"array '{s.name}': element {_first(bad)} of {s.count} is not finite ({values[_first(bad)]}): "
                                     "the fill was read and used, or the element was never written")
        outs[s.name] = values
    return outs


def _torch_dtype(dt):
    import torch
    return {"float16": torch.float16, "float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8}[dt.name]


class Arena:
    def __init__(self, specs, mode, backing="numpy"):
        self.specs, self.mode, self.backing = list(specs), mode, backing
        self.by_name = {s.name: s for s in self.specs}
        self.lay = layout(self.specs, mode)
        if backing == "numpy":
            store = np.empty(self.lay.total + 256, np.uint8)
            skip = -store.ctypes.data % 256
            self.raw = store[skip:skip + self.lay.total]
            self.raw[:] = FILL
            base = self.raw.ctypes.data
        else:
            import torch
            self.raw = torch.full((self.lay.total,), FILL, dtype=torch.uint8, device="cuda")
            base = self.raw.data_ptr()
        assert base % 256 == 0, base
        self.base = base

    def _bytes(self, name):
        off = self.lay.offset[name]
        return self.raw[off:off + self.lay.nbytes[name]]

    def view(self, name, *shape):
        """The array as the call sees it: a typed view into the allocation (numpy array or CUDA tensor), optionally reshaped."""
        s = self.by_name[name]
        v = self._bytes(name).view(s.dtype if self.backing == "numpy" else _torch_dtype(s.dtype))
        return v.reshape(*shape) if shape else v

    def views(self):
        return {s.name: self.view(s.name) for s in self.specs}

    def address(self, name):
        return self.base + self.lay.offset[name]

    def put(self, name, values):
        """Copy values in, bit for bit (NaN payloads included)."""
        s = self.by_name[name]
        data = np.ascontiguousarray(values, dtype=s.dtype).reshape(-1)
        assert data.size == s.count, (name, data.size, s.count)
        raw = np.frombuffer(data.tobytes(), np.uint8)
        if self.backing == "numpy":
            self._bytes(name)[:] = raw
        else:
            import torch
            self._bytes(name).copy_(torch.from_numpy(raw.copy()))

    def refill(self, *names):
        """Back to the fill (the outputs, before a second call in the same arena)."""
        for name in names:
            if self.backing == "numpy":
                self._bytes(name)[:] = FILL
            else:
                self._bytes(name).fill_(FILL)

    def snapshot(self):
        if self.backing == "numpy":
            return self.raw.copy()
        import torch
        torch.cuda.synchronize()
        return self.raw.cpu().numpy()

    def plain(self):
        """Separately allocated copies of every array as it stands now (torch backing): what an ordinary caller of the same call passes."""
        assert self.backing == "torch"
        return {s.name: self.view(s.name).clone() for s in self.specs}

    def run(self, fn):
        before = self.snapshot()
        fn(self.views())
        return verify(self.specs, self.lay, before, self.snapshot())


def both_ways(specs, mode, inputs, call, tag=""):
    """The GPU tests' one move.  inputs: name -> values of every in / inout array (and sentinels of outputs whose fill is a legitimate value).
    call(arrays) makes the library call on a dict of tensors.  It runs once on separately allocated tensors and once inside an arena:
    the arena's four checks, and every out / inout array bit for bit what the plain call gave.  Returns the arena's outputs."""
    import torch
    ar = Arena(specs, mode, "torch")
    for name, values in inputs.items():
        ar.put(name, values)
    plain = ar.plain()
    call(plain)
    torch.cuda.synchronize()
    try:
        got = ar.run(call)
    except AssertionError as e:
        raise AssertionError(f"{tag} [{mode}]: {e}") from None
    for name, values in got.items():
        want = plain[name].cpu().numpy().reshape(-1)
        assert values.tobytes() == want.tobytes(), f"{tag} [{mode}]: '{name}' differs between the arena and separately allocated tensors"
    return got
