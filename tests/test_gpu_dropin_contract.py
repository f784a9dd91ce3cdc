"""The drop-in compressors keep their contract (tests/_dropin_contract.py says what is recorded
and why the inputs make it reproducible): for every case the `sync_buffer` keys with their
descriptors and aliasing after each call, the order and arguments of the codec and aggregator
calls, the number of generator draws and the bytes of every message and updated tensor equal
tests/golden/dropin_contract.json, recorded before the drop-ins were merged onto
chocosgd_amd/wire.py."""
import json

import pytest

import _dropin_contract as C
from conftest import golden_json

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return golden_json("dropin_contract.json")


def test_every_case_is_recorded(recorded):
    assert sorted(recorded["cases"]) == C.NAMES


@pytest.mark.parametrize("name", C.NAMES)
def test_dropin_contract(name, recorded, monkeypatch):
    want = recorded["cases"][name]
    got = json.loads(json.dumps(C.run_case(name, monkeypatch, recorded["traced"])))
    for part in ("calls", "codec", "agg", "rng"):
        if got[part] != want[part]:
            print(part, "got", json.dumps(got[part]))
            print(part, "want", json.dumps(want[part]))
        assert got[part] == want[part], f"{name}: {part} differs"
    # a hash that differed between two runs of the recording package is not in the file
    assert set(want["hashes"]) <= set(got["hashes"])
    assert {k: got["hashes"][k] for k in want["hashes"]} == want["hashes"], f"{name}: bytes differ"
