"""GPU (MI355X): every kernel selection of the plant entry points (mpcgpu_amd/csrc/mpcg_plant.hip) computes the SAME BITS as the commit recorded in
tests/golden/plant_bits_parent.json (tests/make_plant_bits.py wrote it, on the GPU, on the parent of the change that gave the KKT, merit and simulate
kernels one selection each; the hash is in the file).  The host path chooses among 36 KKT, 18 point-merit and 8 simulate instantiations, and a wrong choice
still gives plausible numbers — so all 62 selections are replayed on the recorded inputs and every output array's SHA-256 is compared: a mismatch names the
selection and the array.  Shapes, inputs and the maker's own conditions (two runs agree, everything finite, selections that are meant to differ do differ):
the docstring of tests/make_plant_bits.py.  The imported builders' assertions accept every shape the issue names, so none was replaced."""
import json
import os

import pytest

import make_plant_bits as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec():
    with open(M.OUT) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def inputs(rec):
    """The seeded inputs, rebuilt once; the selections' runs read them through the builders' caches."""
    assert M.inputs() == rec["inputs_sha256"], "other inputs: nothing about the kernels can be concluded"


def test_record_is_small_names_its_commit_and_holds_every_selection(rec):
    assert os.path.getsize(M.OUT) < 32 * 1024                     # digests, not arrays: 178 of them at about 110 bytes
    assert len(rec["commit"]) == 40 and int(rec["commit"], 16) >= 0
    keys = M.selections()
    assert len(keys) == len(set(keys)) == 62
    assert set(rec["selections"]) == set(keys)
    assert sum(k.startswith("kkt/") for k in keys) == 36 and sum(k.startswith("merit/") for k in keys) == 18 and sum(k.startswith("sim/") for k in keys) == 8


@pytest.mark.parametrize("key", M.selections())
def test_selection_computes_the_recorded_bits(rec, inputs, key):
    want = rec["selections"][key]
    got = M.digests(M.run(key))
    assert set(got) == set(want), key
    for name in want:
        assert got[name]["shape"] == want[name]["shape"], f"{key}: the shape of {name}"
        assert got[name]["sha256"] == want[name]["sha256"], f"{key}: {name} has other bits than commit {rec['commit'][:12]} computed"
