"""CPU: the plan executor (rspnet_amd/engine.py) issues exactly the backend calls it issued before it was restructured.

tests/golden/engine_op_trace.json holds, per case of tests/op_trace_util.py, the number of calls, their histogram by method, the
sha256 of the trace text (method, argument shapes / strides / dtypes / offsets, geometries, scalars; the BranchStreams.run and
side_task calls and the gradient-hook calls in between) and the peak of live bytes among the tensors the backend returned —
written by tools/gen_engine_trace.py from the commit before the restructuring.  The text holds no tensor value, so it is the
same on every machine.  When a hash differs, `tools/gen_engine_trace.py --dump DIR <case>` on both trees and a diff of the two
texts show the first call that changed."""
import json
import os

import pytest

from op_trace_util import BRANCHES, CASES, run_case

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_op_trace.json")) as _f:
    FIXTURE = json.load(_f)

_reached = {}


def test_fixture_lists_the_cases():
    assert sorted(FIXTURE) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_executor_issues_the_recorded_calls(name):
    be, _, reached = run_case(name)
    _reached[name] = reached
    got, exp = be.summary(), FIXTURE[name]
    assert got["lines"] == exp["lines"]
    assert got["methods"] == exp["methods"]
    assert got["sha256"] == exp["sha256"]
    assert got["peak_live_bytes"] <= exp["peak_live_bytes"]
    assert reached == CASES[name][3]            # the case still takes the branches it is there for


def test_cases_reach_every_branch():
    for name in CASES:                           # (run alone, this test traces the cases itself)
        if name not in _reached:
            _reached[name] = run_case(name)[2]
    assert {b for r in _reached.values() for b in r} == set(BRANCHES)
