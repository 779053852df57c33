"""CPU: every (pass, kernel instance) the full-size workloads select is also selected by a per-kernel case of tests/test_kernels_gpu.py.

The workloads are WORKLOADS of tools/conv_plan_table.py (the convolutions of the four benchmark models at full size); the per-kernel
cases are CONV_CASES, NARROW32_CASES, the two fuzz lists and NAME_CASES, each of which a GPU test compares with a reference (or, for
NAME_CASES, with the instance that ran) under the default planning options.  Both sides are planned with rsp_conv3d_kernel_name on
the built library: host arithmetic only, no GPU call, and the case lists are read from the test module's source without importing
it.  When a planning threshold moves and a workload lands on an instance no case runs, this fails and names the instance and one
descriptor that selects it; the cure is a case in CONV_CASES, not an entry here."""
import ast
import ctypes as C
import importlib.util
import os

from rspnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_TESTS = os.path.join(ROOT, "tests", "test_kernels_gpu.py")
LITERAL_LISTS = ("CONV_CASES", "NARROW32_CASES", "NAME_CASES")
GENERATED_LISTS = ("_fuzz_cases", "_fuzz_depth_cases")
PASSES = ("fwd", "dgrad", "wgrad")


def _tool():
    spec = importlib.util.spec_from_file_location("conv_plan_table", os.path.join(ROOT, "tools", "conv_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def per_kernel_cases(source=None, without=()):
    """{list name: [(N, D, H, W, Cin, Cout, k, s, p), ...]} of the per-kernel case lists, from the module's syntax tree: the literal
    lists by literal_eval, the two seeded generators by running their own (torch-free) function bodies.  `without`: cases left out."""
    if source is None:
        with open(KERNEL_TESTS) as f:
            source = f.read()
    tree = ast.parse(source)
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) in LITERAL_LISTS:
            out[node.targets[0].id] = ast.literal_eval(node.value)
        elif isinstance(node, ast.FunctionDef) and node.name in GENERATED_LISTS:
            scope = {}
            exec(compile(ast.Module(body=[node], type_ignores=[]), KERNEL_TESTS, "exec"), scope)
            out[node.name] = scope[node.name]()
    assert sorted(out) == sorted(LITERAL_LISTS + GENERATED_LISTS), sorted(out)
    return {name: [c for c in cases if c not in without] for name, cases in out.items()}


def planned_pairs(lib, descs):
    """{(pass, kernel name): the first descriptor that selects it} under the options in effect."""
    pairs = {}
    for d in descs:
        ref = C.byref(_lib.ConvDesc(*d))
        for which, what in enumerate(PASSES):
            pairs.setdefault((what, lib.rsp_conv3d_kernel_name(ref, which).decode()), d)
    return pairs


def missing_pairs(lib, tool, cases):
    needed = planned_pairs(lib, [tool.desc_tuple(*w) for w in tool.WORKLOADS])
    tested = planned_pairs(lib, [tool.desc_tuple(*c) for group in cases.values() for c in group])
    return needed, tested, {pair: d for pair, d in needed.items() if pair not in tested}


def _report(missing):
    return "\n".join(f"no per-kernel case runs {what} on {name}; selected by the descriptor {d}" for (what, name), d in sorted(missing.items()))


NEW_CASE = (16, 4, 14, 14, 144, 288, (1, 3, 3), (1, 1, 1), (0, 1, 1))      # S3D-G Mixed_4e's (1,3,3): the 144-wide half-block dgrad tile


def test_every_instance_the_workloads_select_has_a_per_kernel_case():
    lib, tool = _lib.load(), _tool()
    cases = per_kernel_cases()
    needed, tested, missing = missing_pairs(lib, tool, cases)
    print(f"{len(needed)} (pass, instance) pairs over {len(tool.WORKLOADS)} workload descriptors; "
          f"{len(tested)} over {sum(len(g) for g in cases.values())} per-kernel cases")
    if missing:
        print(_report(missing))
    assert not missing, _report(missing)
    assert len(needed) >= 30 and all(name for _, name in needed)      # (the query answered: an unknown descriptor would give "")


def test_the_closure_notices_a_case_that_leaves():
    """Without the S3D-G (16,4,14,14) 144 -> 288 (1,3,3) layer in CONV_CASES the input gradient on the 144-wide half-block tile with
    the slice-major K walk has no per-kernel case: the check above reports exactly that pair, with a descriptor that selects it."""
    lib, tool = _lib.load(), _tool()
    assert NEW_CASE in per_kernel_cases()["CONV_CASES"]
    _, _, missing = missing_pairs(lib, tool, per_kernel_cases(without=(NEW_CASE,)))
    assert list(missing) == [("dgrad", "igemm_persist_kernel<128, 144, 4, 1, true, 2>")], _report(missing)
    d = missing[("dgrad", "igemm_persist_kernel<128, 144, 4, 1, true, 2>")]
    assert lib.rsp_conv3d_kernel_name(C.byref(_lib.ConvDesc(*d)), 1).decode() == "igemm_persist_kernel<128, 144, 4, 1, true, 2>"
    assert "dgrad on igemm_persist_kernel<128, 144, 4, 1, true, 2>" in _report(missing) and str(d) in _report(missing)
