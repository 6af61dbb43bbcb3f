"""GPU: mpcg_set_option / mpcg_get_option against their recorded table (tests/golden/option_table.json, written by tests/make_option_table.py):
every key's default, and per key and value the return code of the set, its error text, what a get reads back and whether "auto_cfg" fell.
The comparison is exact.  No solve kernel is launched."""
import json

import pytest

import make_option_table as mot

pytestmark = pytest.mark.gpu


def test_options_match_the_recorded_table():
    with open(mot.OUT) as f:
        table = json.load(f)
    assert table["keys"] == list(mot.KEYS) and table["values"] == list(mot.VALUES) and table["knots"] == list(mot.KNOTS)
    got = json.loads(json.dumps(mot.record()))
    bad = []
    for hn, want in table["handles"].items():
        have = got["handles"][hn]
        for key in mot.KEYS:
            if have["defaults"][key] != want["defaults"][key]:
                bad.append(f"{hn} default of {key}: got {have['defaults'][key]}, table {want['defaults'][key]}")
            for v, rec in want["set"][key].items():
                if have["set"][key][v] != rec:
                    bad.append(f"{hn} {key} = {v}: got {have['set'][key][v]}, table {rec}")
    assert not bad, f"{len(bad)} entries differ:\n" + "\n".join(bad[:30])
    assert got == table
