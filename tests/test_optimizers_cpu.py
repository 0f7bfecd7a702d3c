"""The five optimisers of gprc_amd.fit against tests/golden/optimizer_iterates.json (tests/golden/make_optimizer_record.py): the
same closed-form objectives replayed on the current code -- no GPU, no native library -- must give every returned field and the whole
sequence of points the objective was asked at, every float bit for bit.  The record pins the evaluation order, the one-entry cache,
the sentinel and the raising paths; it is not regenerated to make this test pass."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_optimizer_record", os.path.join(GOLDEN, "make_optimizer_record.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

with open(os.path.join(GOLDEN, "optimizer_iterates.json")) as f:
    RECORD = json.load(f)["cases"]
CASES = M.cases()
_replayed = {}


def replay(name):
    if name not in _replayed:
        call, objective = CASES[name]()
        _replayed[name] = M.run(call, objective)
    return _replayed[name]


def test_the_record_and_the_recorder_list_the_same_cases():
    assert sorted(RECORD) == sorted(CASES)
    walked = {name.split("/")[0] for name in RECORD}
    assert walked == {"optimize", "optimize_gpc", "optimize_sparse", "optimize_iterative", "optimize_multistart", "promise"}
    assert sum("raised" in r for r in RECORD.values()) >= 8 and sum("result" in r for r in RECORD.values()) >= 30


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_optimiser_reproduces_the_record(name):
    got, want = replay(name), RECORD[name]
    assert got["calls"] == want["calls"]            # where the objective was evaluated, in order: hex strings, so bit for bit
    assert got == want                              # par, noise, Z, value, counts, convergence, se, best_index, every entry of `all`; or the exception


@pytest.mark.parametrize("variant", [v[0] for v in M.promise_variants()])
def test_one_start_of_multistart_is_what_optimize_runs(variant):
    """optimize_multistart's docstring: "Each instance runs exactly what `optimize` runs from its start." """
    one, multi = replay("promise/optimize/" + variant), replay("promise/optimize_multistart/" + variant)
    asked = [[[theta], [noise]] for theta, noise in one["calls"]]
    if "raised" in one and len(asked) > 1 and asked[-1] == asked[-2]:
        asked.pop()       # a first point that fails: `optimize` asks it again for the gradient and raises from there, a round raises at once
    assert asked == multi["calls"]
    assert one.get("raised") == multi.get("raised")
    if "result" in one:
        assert multi["all"] == [one["result"]] and multi["result"] == dict(one["result"], best_index=0)
