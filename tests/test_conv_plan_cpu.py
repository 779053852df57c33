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
    """The A/B switches, set in this process through their options (rsp_conv3d_set_option), over NAME_CASES + SETS: the rows the
    committed table recorded under the environment variable."""
    tool = _tool()
    got, want = tool.switch_rows(_lib.load(), _lib, switch), golden["env"][switch]
    assert len(got) == len(want)
    assert got == want, (switch, _first_difference(tool.subset_cases(), got, want))


# (option, variable, value in the child's environment, effective value expected): distinct non-default integers; flags set by an
# EMPTY value, since a flag variable counts as set when it is present at all
ENV_ROUTE = [("narrow_max_tiles", "RSP_NARROW_MAX_TILES", "301", 301), ("narrow32_max_units", "RSP_NARROW32_MAX_UNITS", "302", 302),
             ("tall_min_tiles", "RSP_TALL_MIN_TILES", "303", 303), ("two_level_min_chunks", "RSP_TWO_LEVEL_MIN_CHUNKS", "304", 304),
             ("direct_max_tiles", "RSP_DIRECT_MAX_TILES", "305", 305), ("no_persist", "RSP_NO_PERSIST", "", 1),
             ("no_half_block", "RSP_NO_HALF_BLOCK", "", 1), ("no_pad_skip", "RSP_NO_PAD_SKIP", "", 1), ("no_dmajor", "RSP_NO_DMAJOR", "", 1),
             ("no_tm_skip", "RSP_NO_TM_SKIP", "", 1), ("no_multi_split", "RSP_NO_MULTI_SPLIT", "", 1)]


def test_environment_variables_reach_the_option_table():
    """One child interpreter (ctypes only: no torch, no GPU) with all eleven variables set: rsp_conv3d_set_option(name, -1) returns
    the previous EFFECTIVE value, which is the environment's for every option."""
    code = ("import ctypes, json, sys; lib = ctypes.CDLL(sys.argv[1]); "
            "print(json.dumps({n: lib.rsp_conv3d_set_option(n.encode(), -1) for n in sys.argv[2:]}))")
    env = dict(os.environ, **{var: value for _, var, value, _ in ENV_ROUTE})
    res = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH] + [n for n, _, _, _ in ENV_ROUTE], env=env, check=True,
                         capture_output=True, text=True)
    assert json.loads(res.stdout) == {n: want for n, _, _, want in ENV_ROUTE}
