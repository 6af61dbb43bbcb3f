"""GPU: the PCG launch policy against its recorded table (tests/golden/pcg_plan_table.json, written by tests/make_plan_table.py).
Every case of the generator is replayed in the same order on a fresh handle: return code, every "last_kernel_*" option, "symmetry_state"
after the call and mpcg_check_pcg_occupancy must be what the table says.  The table holds for the CU count it was recorded on."""
import json
import os

import pytest

import make_plan_table as mpt

pytestmark = pytest.mark.gpu


def test_launch_plan_matches_the_recorded_table():
    with open(mpt.OUT) as f:
        table = json.load(f)
    assert table["last_fields"] == list(mpt.LAST) and table["max_iter"] == 3
    run = mpt.run(num_cus_expected=table["num_cus"])
    _, num_cus = next(run)
    if num_cus != table["num_cus"]:
        pytest.skip(f"the table was recorded on {table['num_cus']} CUs, this device has {num_cus}")
    expected = table["cases"]
    seen, bad = [], []
    for cid, rec in run:
        seen.append(cid)
        if rec != expected.get(cid):
            bad.append(f"{cid}: got {rec}, table {expected.get(cid)}")
    assert seen == list(expected), "the generator's case list differs from the table's"
    assert not bad, f"{len(bad)} of {len(seen)} cases differ:\n" + "\n".join(bad[:20])
