"""CPU: the launch plan of every convolution descriptor in tests/golden/conv_plan.json (kernel names, workspace sizes, executed
fractions, stat tiles; written by tools/conv_plan_table.py from the library as it was before the plan moved into one function) is
what the built library reports now — strings, integers and fractions exactly.  Host arithmetic only, no GPU call."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from rspnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "conv_plan_table.py")


def _tool():
    spec = importlib.util.spec_from_file_location("conv_plan_table", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan.json")) as f:
        return json.load(f)


def _first_difference(cases, got, want):
    for c, g, w in zip(cases, got, want):
        if g != w:
            return {"desc": c, "got": g, "want": w}
    return None


def test_descriptor_list_is_the_committed_one(golden):
    tool = _tool()
    assert [list(c) for c in tool.all_cases()] == golden["cases"]
    assert tool.OPTIONS == golden["options"]
    assert [n for n, _ in tool.ENV_SWITCHES] == list(golden["env"])


def test_plan_of_every_descriptor_under_every_option(golden):
    tool = _tool()
    want = tool.expand(golden)
    got = tool.table(_lib.load(), _lib)
    assert got["cases"] == want["cases"]
    for opts, g, w in zip(tool.OPTIONS, got["rows"], want["rows"]):
        assert len(g) == len(w)
        assert g == w, (opts, _first_difference(got["cases"], g, w))


@pytest.mark.parametrize("switch", ["RSP_NO_PERSIST", "RSP_NO_HALF_BLOCK", "RSP_NO_MULTI_SPLIT", "RSP_DIRECT_MAX_TILES"])
def test_plan_under_an_environment_switch(golden, switch):
    """The A/B switches are read once per process: a child interpreter per switch, over NAME_CASES + SETS."""
    tool = _tool()
    value = dict(tool.ENV_SWITCHES)[switch]
    res = subprocess.run([sys.executable, TOOL, "--subset"], env=dict(os.environ, **{switch: value}), check=True,
                         capture_output=True, text=True)
    got, want = json.loads(res.stdout), golden["env"][switch]
    assert len(got) == len(want)
    assert got == want, (switch, _first_difference(tool.subset_cases(), got, want))
