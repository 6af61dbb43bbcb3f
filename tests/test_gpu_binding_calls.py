"""GPU: the Python binding against its recorded table (tests/golden/binding_calls.json, written by tests/make_binding_calls.py): per case — every
public method of PcgSolver, Plant and QdldlSolver in both precisions, each optional argument given and left out, and each refusal — the C entries
called with every argument in its normal form, and the dtype and shape of what comes back or the type of the exception.  The comparison is exact."""
import json

import pytest

import make_binding_calls as mbc

pytestmark = pytest.mark.gpu


def test_binding_calls_match_the_recorded_table():
    with open(mbc.OUT) as f:
        table = json.load(f)
    got = json.loads(json.dumps(mbc.record()))
    assert got["shape"] == table["shape"]
    assert [c["case"] for c in got["cases"]] == [c["case"] for c in table["cases"]]
    bad = [f"{have['case']}:\n  got   {have}\n  table {want}" for have, want in zip(got["cases"], table["cases"]) if have != want]
    assert not bad, f"{len(bad)} of {len(table['cases'])} cases differ:\n" + "\n".join(bad[:20])
    assert not any(c.get("raises") == "ReachedC" for c in table["cases"])
