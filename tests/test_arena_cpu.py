"""The arena helper (tests/arena.py) is honest — no GPU.  The layout properties, for both layouts, over every spec list the GPU arena files
build (tests/arena_specs.py); then fake "entries" written in numpy on a numpy-backed arena: a correct one passes, and each planted defect
fails with a message that names the array."""
import numpy as np
import pytest

import arena
import arena_specs as A

LISTS = A.all_spec_lists()


@pytest.mark.parametrize("mode", arena.MODES)
def test_layout_properties_over_every_spec_list(mode):
    assert len(LISTS) > 500
    for label, specs in LISTS:
        lay = arena.layout(specs, mode)
        size = lambda s, elems: elems * s.dtype.itemsize
        edge = max([65536] + [size(s, s.traj) for s in specs])
        pos = 0
        for i, s in enumerate(specs):
            off, end = lay.offset[s.name], lay.offset[s.name] + lay.nbytes[s.name]
            assert lay.nbytes[s.name] == size(s, s.count), label
            gap = off - pos                                    # no overlap: every array starts behind the previous one's end plus its band
            if i == 0:
                assert gap >= edge, (label, s.name, gap)
            else:
                prev = specs[i - 1]
                assert gap >= max(4096, 2 * size(prev, prev.knot), 2 * size(s, s.knot)), (label, s.name, gap)
            if mode == "aligned":
                assert off % 256 == 0, (label, s.name, off)
            else:                                              # exactly the stated alignment: a multiple of it and of nothing larger
                assert off % s.align == 0 and off % (2 * s.align) == s.align, (label, s.name, off, s.align)
            assert lay.bands[i] == (pos, off, specs[i - 1].name if i else None, s.name), label
            pos = end
        assert lay.total - pos >= edge and lay.bands[-1] == (pos, lay.total, specs[-1].name, None), label
        covered = sum(e - s_ for s_, e, _, _ in lay.bands) + sum(lay.nbytes.values())
        assert covered == lay.total, label                     # bands and arrays tile the allocation


def test_minimal_layout_of_the_examples_in_the_issue():
    specs = A.pcg("f32", 14, 3, 5, True)
    lay = arena.layout(specs, "minimal")
    assert lay.offset["S"] % 32 == 16 and lay.offset["gamma"] % 8 == 4 and lay.offset["exits"] % 2 == 1
    assert arena.layout(A.pcg("f32", 14, 3, 5, True, "f16"), "minimal").offset["S"] % 8 == 4
    assert arena.layout(A.pcg("f64", 14, 3, 5, True), "minimal").offset["S"] % 16 == 8


def test_the_fill_is_a_nan_in_every_float_format_and_marks_the_integers():
    raw = np.full(8, arena.FILL, np.uint8)
    for dt in (np.float16, np.float32, np.float64):
        assert np.isnan(raw.view(dt)).all()
    assert (raw.view(np.int32) == -1).all() and (raw == 255).all()


# ---- fake entries: y[i] = 2 x[i] + w[i] for count elements, flags[b] = 1, keep[] read only, spare[] not to be touched; y[1] is masked ----
COUNT, NFLAG = 37, 5
MASK = np.zeros(COUNT, bool)
MASK[1] = True
SPECS = [arena.spec("x", np.float32, COUNT, "in"), arena.spec("w", np.float32, COUNT, "in"), arena.spec("spare", np.float32, 9, "untouched"),
         arena.spec("y", np.float32, COUNT, "out", mask=MASK), arena.spec("acc", np.float64, COUNT, "inout"),
         arena.spec("flags", np.uint8, NFLAG, "out")]


def correct(ar, v):
    keep = ~MASK
    v["y"][keep] = 2 * v["x"][keep] + v["w"][keep]
    v["acc"][:] = v["acc"] + v["x"]
    v["flags"][:] = 1


def make(mode):
    ar = arena.Arena(SPECS, mode, "numpy")
    rng = np.random.default_rng(5)
    ar.put("x", rng.standard_normal(COUNT))
    ar.put("w", rng.standard_normal(COUNT))
    ar.put("acc", rng.standard_normal(COUNT))
    return ar


def raw_f32(ar, name, index):
    """Four raw bytes at element `index` of a float array (past either end: into the band)."""
    at = ar.lay.offset[name] + 4 * index
    return ar.raw[at:at + 4]


def past_the_end(ar, v):
    correct(ar, v)
    raw_f32(ar, "y", COUNT)[:] = np.frombuffer(np.float32(1.0).tobytes(), np.uint8)


def before_the_start(ar, v):
    correct(ar, v)
    raw_f32(ar, "y", -1)[:] = np.frombuffer(np.float32(1.0).tobytes(), np.uint8)


def wide_store_into_the_last_flag(ar, v):
    correct(ar, v)
    at = ar.lay.offset["flags"] + NFLAG - 1
    ar.raw[at:at + 4] = np.frombuffer(np.uint32(1).tobytes(), np.uint8)      # a 32-bit store of the value 1 where a byte belongs


def one_bit_in_an_input(ar, v):
    correct(ar, v)
    raw_f32(ar, "w", 20)[0] ^= 1


def writes_the_untouched(ar, v):
    correct(ar, v)
    v["spare"][3] = 0.0


def leaves_one_unwritten(ar, v):
    keep = ~MASK
    keep[11] = False
    v["y"][keep] = 2 * v["x"][keep] + v["w"][keep]
    v["acc"][:] = v["acc"] + v["x"]
    v["flags"][:] = 1


def overwrites_the_masked(ar, v):
    correct(ar, v)
    v["y"][1] = 0.0


def reads_past_an_input(ar, v):
    """The last element adds 0 x x[count]: the band's NaN must surface in y (with the fill's own payload here: numpy propagates it)."""
    correct(ar, v)
    beyond = raw_f32(ar, "x", COUNT).view(np.float32)[0]
    v["y"][COUNT - 1] = v["y"][COUNT - 1] + np.float32(0.0) * beyond


DEFECTS = [(past_the_end, "after array 'y'", "0 bytes past its end"), (before_the_start, "before array 'y'", "4 bytes ahead of its start"),
           (wide_store_into_the_last_flag, "after array 'flags'", "0 bytes past its end"), (one_bit_in_an_input, "input array 'w'", "element 20"),
           (writes_the_untouched, "'spare'", "untouched"), (leaves_one_unwritten, "output array 'y'", "element 11"),
           (overwrites_the_masked, "array 'y'", "must not write"), (reads_past_an_input, "array 'y'", "fill NaN that was read")]


@pytest.mark.parametrize("mode", arena.MODES)
def test_a_correct_entry_passes_and_hands_its_outputs_back(mode):
    ar = make(mode)
    x, w, acc = (ar.view(k).copy() for k in ("x", "w", "acc"))
    out = ar.run(lambda v: correct(ar, v))
    assert sorted(out) == ["acc", "flags", "y"]
    keep = ~MASK
    assert np.array_equal(out["y"][keep], (2 * x + w)[keep]) and np.isnan(out["y"][1])
    assert np.array_equal(out["acc"], acc + x) and (out["flags"] == 1).all()


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("defect,names,says", DEFECTS, ids=[d[0].__name__ for d in DEFECTS])
def test_every_planted_defect_fails_and_names_the_array(defect, names, says, mode):
    ar = make(mode)
    with pytest.raises(AssertionError) as e:
        ar.run(lambda v: defect(ar, v))
    assert names in str(e.value) and says in str(e.value), str(e.value)


def test_a_sentinel_marks_an_output_whose_legitimate_value_is_the_fill():
    """d_step = -1 (no step) is the fill of an int32: the caller puts a sentinel there first, and 'never written' means 'still the sentinel'."""
    specs = [arena.spec("step", np.int32, 3, "out")]
    for write_all in (True, False):
        ar = arena.Arena(specs, "minimal", "numpy")
        ar.put("step", [-7, -7, -7])

        def entry(v):
            v["step"][:2] = -1
            if write_all:
                v["step"][2] = -1
        if write_all:
            assert (ar.run(entry)["step"] == -1).all()
        else:
            with pytest.raises(AssertionError, match="'step'.*element 2"):
                ar.run(entry)
