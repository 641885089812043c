"""Replays tests/golden/abi_refusals.json against the built library: every C ABI entry that has a twin on a conditioned view
must refuse each recorded argument tuple with the recorded return code and lcgp_last_error() text.  The table was written
by tests/golden/gen_abi_refusals.py from the library BEFORE the entries were folded onto shared checked routines, so a check
that drifts between a model entry and its view twin shows here.  Host only: every call is refused before anything is
enqueued and no pointer is dereferenced.
"""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "abi_refusals.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_abi_refusals", os.path.join(GOLDEN, "gen_abi_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_covers_the_twinned_entries(table):
    from lcgp_amd import _hip
    entries = {r[0] for r in table["rows"]}
    assert entries <= set(_hip.SIGNATURES)
    twins = {e for e in _hip.SIGNATURES if e.startswith("lcgp_condition_") and e.replace("lcgp_condition_vr", "lcgp_variance_reduction")
             .replace("lcgp_condition_", "lcgp_") in _hip.SIGNATURES}
    assert twins <= entries and len(table["rows"]) > 800
    assert all(r[2] == -1 and r[3] for r in table["rows"])


def test_refusals_are_those_recorded(table, gen):
    from lcgp_amd import _hip
    _hip.build_library()
    lib = _hip.load()
    assert lib.lcgp_version() == table["library_version"]
    wrong = []
    for entry, args, rc, text in table["rows"]:
        got = gen.call(lib, _hip.SIGNATURES, entry, args)
        if got != (rc, text):
            wrong.append((entry, args, got, (rc, text)))
    assert not wrong, "%d of %d refusals differ, the first: %r" % (len(wrong), len(table["rows"]), wrong[:3])
