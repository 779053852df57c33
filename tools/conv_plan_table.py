#!/usr/bin/env python
"""The launch plan of every convolution descriptor of a fixed list, as the library's host queries report it: kernel names, workspace
sizes, executed fractions and stat tiles, under the default planning options and the non-default ones.  ctypes only, no GPU, no torch.

    python tools/conv_plan_table.py OUT.json        # the whole table (tests/golden/conv_plan.json was written this way)
    python tools/conv_plan_table.py --subset        # NAME_CASES + SETS as planned now (under an RSP_* variable, say), JSON on stdout

tests/test_conv_plan_cpu.py regenerates it from the built library and demands equality with the committed table: a change to the
planning code that moves any dispatch decision, workspace size or fraction shows up there without a GPU."""
import ast
import ctypes as C
import importlib.util
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# option sets every descriptor is planned under (rsp_conv3d_set_option; -1 restores the default)
OPTIONS = [{}, {"narrow_max_tiles": 0}, {"narrow32_max_units": 0}, {"tall_min_tiles": 2}, {"tall_min_tiles": 768}, {"two_level_min_chunks": 8}]
# A/B switches planned over the subset: (environment variable = key of the table's "env" section, value), and each one's option name
ENV_SWITCHES = [("RSP_NO_PERSIST", "1"), ("RSP_NO_HALF_BLOCK", "1"), ("RSP_NO_MULTI_SPLIT", "1"), ("RSP_DIRECT_MAX_TILES", "4")]
SWITCH_OPTIONS = {"RSP_NO_PERSIST": "no_persist", "RSP_NO_HALF_BLOCK": "no_half_block", "RSP_NO_MULTI_SPLIT": "no_multi_split", "RSP_DIRECT_MAX_TILES": "direct_max_tiles"}

# Convolution geometries of the four benchmark workloads at full size (C3D, R3D-18, R(2+1)D-VCOP at batch 32, 16 x 112 x 112; S3D-G at
# batch 16, 16 x 224 x 224): (N, D, H, W, Cin, Cout, k, s, p, in_ld, out_ld).  The pitches wider than the channel count are S3D-G's
# concat slices and R(2+1)D's padded mid-channel counts.
WORKLOADS = [
    (32,16,112,112,4,64,(3,3,3),(1,1,1),(1,1,1),4,64), (32,16,56,56,64,128,(3,3,3),(1,1,1),(1,1,1),64,128),
    (32,8,28,28,128,256,(3,3,3),(1,1,1),(1,1,1),128,256), (32,8,28,28,256,256,(3,3,3),(1,1,1),(1,1,1),256,256),
    (32,4,14,14,256,512,(3,3,3),(1,1,1),(1,1,1),256,512), (32,4,14,14,512,512,(3,3,3),(1,1,1),(1,1,1),512,512),
    (32,2,7,7,512,512,(3,3,3),(1,1,1),(1,1,1),512,512), (32,16,112,112,4,64,(7,7,7),(1,2,2),(3,3,3),4,64),
    (32,8,28,28,64,64,(3,3,3),(1,1,1),(1,1,1),64,64), (32,8,28,28,64,128,(1,1,1),(2,2,2),(0,0,0),64,128),
    (32,8,28,28,64,128,(3,3,3),(2,2,2),(1,1,1),64,128), (32,4,14,14,128,128,(3,3,3),(1,1,1),(1,1,1),128,128),
    (32,4,14,14,128,256,(1,1,1),(2,2,2),(0,0,0),128,256), (32,4,14,14,128,256,(3,3,3),(2,2,2),(1,1,1),128,256),
    (32,2,7,7,256,256,(3,3,3),(1,1,1),(1,1,1),256,256), (32,2,7,7,256,512,(1,1,1),(2,2,2),(0,0,0),256,512),
    (32,2,7,7,256,512,(3,3,3),(2,2,2),(1,1,1),256,512), (32,1,4,4,512,512,(3,3,3),(1,1,1),(1,1,1),512,512),
    (32,16,112,112,4,84,(1,7,7),(1,2,2),(0,3,3),4,84), (32,16,56,56,83,64,(3,1,1),(1,1,1),(1,0,0),84,64),
    (32,16,56,56,64,144,(1,3,3),(1,1,1),(0,1,1),64,144), (32,16,56,56,144,64,(3,1,1),(1,1,1),(1,0,0),144,64),
    (32,16,56,56,64,232,(1,3,3),(1,2,2),(0,1,1),64,232), (32,16,28,28,230,128,(3,1,1),(2,1,1),(1,0,0),232,128),
    (32,16,56,56,64,44,(1,1,1),(1,2,2),(0,0,0),64,44), (32,16,28,28,42,128,(1,1,1),(2,1,1),(0,0,0),44,128),
    (32,8,28,28,128,288,(1,3,3),(1,1,1),(0,1,1),128,288), (32,8,28,28,288,128,(3,1,1),(1,1,1),(1,0,0),288,128),
    (32,8,28,28,128,460,(1,3,3),(1,2,2),(0,1,1),128,460), (32,8,14,14,460,256,(3,1,1),(2,1,1),(1,0,0),460,256),
    (32,8,28,28,128,88,(1,1,1),(1,2,2),(0,0,0),128,88), (32,8,14,14,85,256,(1,1,1),(2,1,1),(0,0,0),88,256),
    (32,4,14,14,256,576,(1,3,3),(1,1,1),(0,1,1),256,576), (32,4,14,14,576,256,(3,1,1),(1,1,1),(1,0,0),576,256),
    (32,4,14,14,256,924,(1,3,3),(1,2,2),(0,1,1),256,924), (32,4,7,7,921,512,(3,1,1),(2,1,1),(1,0,0),924,512),
    (32,4,14,14,256,172,(1,1,1),(1,2,2),(0,0,0),256,172), (32,4,7,7,170,512,(1,1,1),(2,1,1),(0,0,0),172,512),
    (32,2,7,7,512,1152,(1,3,3),(1,1,1),(0,1,1),512,1152), (32,2,7,7,1152,512,(3,1,1),(1,1,1),(1,0,0),1152,512),
    (16,16,224,224,4,64,(1,7,7),(2,2,2),(0,3,3),4,64), (16,8,112,112,64,64,(7,1,1),(1,1,1),(3,0,0),64,64),
    (16,8,56,56,64,64,(1,1,1),(1,1,1),(0,0,0),64,64), (16,8,56,56,64,192,(1,3,3),(1,1,1),(0,1,1),64,192),
    (16,8,56,56,192,192,(3,1,1),(1,1,1),(1,0,0),192,192), (16,8,28,28,192,64,(1,1,1),(1,1,1),(0,0,0),192,256),
    (16,8,28,28,192,96,(1,1,1),(1,1,1),(0,0,0),192,96), (16,8,28,28,192,16,(1,1,1),(1,1,1),(0,0,0),192,16),
    (16,8,28,28,192,176,(1,1,1),(1,1,1),(0,0,0),192,176), (16,8,28,28,96,128,(1,3,3),(1,1,1),(0,1,1),96,128),
    (16,8,28,28,128,128,(3,1,1),(1,1,1),(1,0,0),128,128), (16,8,28,28,16,32,(1,3,3),(1,1,1),(0,1,1),16,32),
    (16,8,28,28,32,32,(3,1,1),(1,1,1),(1,0,0),32,32), (16,8,28,28,192,32,(1,1,1),(1,1,1),(0,0,0),192,256),
    (16,8,28,28,256,128,(1,1,1),(1,1,1),(0,0,0),256,480), (16,8,28,28,256,128,(1,1,1),(1,1,1),(0,0,0),256,128),
    (16,8,28,28,256,32,(1,1,1),(1,1,1),(0,0,0),256,32), (16,8,28,28,256,288,(1,1,1),(1,1,1),(0,0,0),256,288),
    (16,8,28,28,128,192,(1,3,3),(1,1,1),(0,1,1),128,192), (16,8,28,28,192,192,(3,1,1),(1,1,1),(1,0,0),192,192),
    (16,8,28,28,32,96,(1,3,3),(1,1,1),(0,1,1),32,96), (16,8,28,28,96,96,(3,1,1),(1,1,1),(1,0,0),96,96),
    (16,8,28,28,256,64,(1,1,1),(1,1,1),(0,0,0),256,480), (16,4,14,14,480,192,(1,1,1),(1,1,1),(0,0,0),480,512),
    (16,4,14,14,480,96,(1,1,1),(1,1,1),(0,0,0),480,96), (16,4,14,14,480,16,(1,1,1),(1,1,1),(0,0,0),480,16),
    (16,4,14,14,480,304,(1,1,1),(1,1,1),(0,0,0),480,304), (16,4,14,14,96,208,(1,3,3),(1,1,1),(0,1,1),96,208),
    (16,4,14,14,208,208,(3,1,1),(1,1,1),(1,0,0),208,208), (16,4,14,14,16,48,(1,3,3),(1,1,1),(0,1,1),16,48),
    (16,4,14,14,48,48,(3,1,1),(1,1,1),(1,0,0),48,48), (16,4,14,14,480,64,(1,1,1),(1,1,1),(0,0,0),480,512),
    (16,4,14,14,512,160,(1,1,1),(1,1,1),(0,0,0),512,512), (16,4,14,14,512,112,(1,1,1),(1,1,1),(0,0,0),512,112),
    (16,4,14,14,512,24,(1,1,1),(1,1,1),(0,0,0),512,24), (16,4,14,14,512,296,(1,1,1),(1,1,1),(0,0,0),512,296),
    (16,4,14,14,112,224,(1,3,3),(1,1,1),(0,1,1),112,224), (16,4,14,14,224,224,(3,1,1),(1,1,1),(1,0,0),224,224),
    (16,4,14,14,24,64,(1,3,3),(1,1,1),(0,1,1),24,64), (16,4,14,14,64,64,(3,1,1),(1,1,1),(1,0,0),64,64),
    (16,4,14,14,512,64,(1,1,1),(1,1,1),(0,0,0),512,512), (16,4,14,14,512,128,(1,1,1),(1,1,1),(0,0,0),512,512),
    (16,4,14,14,512,128,(1,1,1),(1,1,1),(0,0,0),512,128), (16,4,14,14,512,280,(1,1,1),(1,1,1),(0,0,0),512,280),
    (16,4,14,14,128,256,(1,3,3),(1,1,1),(0,1,1),128,256), (16,4,14,14,256,256,(3,1,1),(1,1,1),(1,0,0),256,256),
    (16,4,14,14,512,112,(1,1,1),(1,1,1),(0,0,0),512,528), (16,4,14,14,512,144,(1,1,1),(1,1,1),(0,0,0),512,144),
    (16,4,14,14,512,32,(1,1,1),(1,1,1),(0,0,0),512,32), (16,4,14,14,512,288,(1,1,1),(1,1,1),(0,0,0),512,288),
    (16,4,14,14,144,288,(1,3,3),(1,1,1),(0,1,1),144,288), (16,4,14,14,288,288,(3,1,1),(1,1,1),(1,0,0),288,288),
    (16,4,14,14,32,64,(1,3,3),(1,1,1),(0,1,1),32,64), (16,4,14,14,512,64,(1,1,1),(1,1,1),(0,0,0),512,528),
    (16,4,14,14,528,256,(1,1,1),(1,1,1),(0,0,0),528,832), (16,4,14,14,528,160,(1,1,1),(1,1,1),(0,0,0),528,160),
    (16,4,14,14,528,32,(1,1,1),(1,1,1),(0,0,0),528,32), (16,4,14,14,528,448,(1,1,1),(1,1,1),(0,0,0),528,448),
    (16,4,14,14,160,320,(1,3,3),(1,1,1),(0,1,1),160,320), (16,4,14,14,320,320,(3,1,1),(1,1,1),(1,0,0),320,320),
    (16,4,14,14,32,128,(1,3,3),(1,1,1),(0,1,1),32,128), (16,4,14,14,128,128,(3,1,1),(1,1,1),(1,0,0),128,128),
    (16,4,14,14,528,128,(1,1,1),(1,1,1),(0,0,0),528,832), (16,2,7,7,832,256,(1,1,1),(1,1,1),(0,0,0),832,832),
    (16,2,7,7,832,160,(1,1,1),(1,1,1),(0,0,0),832,160), (16,2,7,7,832,32,(1,1,1),(1,1,1),(0,0,0),832,32),
    (16,2,7,7,832,448,(1,1,1),(1,1,1),(0,0,0),832,448), (16,2,7,7,160,320,(1,3,3),(1,1,1),(0,1,1),160,320),
    (16,2,7,7,320,320,(3,1,1),(1,1,1),(1,0,0),320,320), (16,2,7,7,32,128,(1,3,3),(1,1,1),(0,1,1),32,128),
    (16,2,7,7,128,128,(3,1,1),(1,1,1),(1,0,0),128,128), (16,2,7,7,832,128,(1,1,1),(1,1,1),(0,0,0),832,832),
    (16,2,7,7,832,384,(1,1,1),(1,1,1),(0,0,0),832,1024), (16,2,7,7,832,192,(1,1,1),(1,1,1),(0,0,0),832,192),
    (16,2,7,7,832,48,(1,1,1),(1,1,1),(0,0,0),832,48), (16,2,7,7,832,624,(1,1,1),(1,1,1),(0,0,0),832,624),
    (16,2,7,7,192,384,(1,3,3),(1,1,1),(0,1,1),192,384), (16,2,7,7,384,384,(3,1,1),(1,1,1),(1,0,0),384,384),
    (16,2,7,7,48,128,(1,3,3),(1,1,1),(0,1,1),48,128), (16,2,7,7,832,128,(1,1,1),(1,1,1),(0,0,0),832,1024),
]


def _lib_module():
    spec = importlib.util.spec_from_file_location("_rsp_lib", os.path.join(ROOT, "rspnet_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _literal(path, name):
    """The value of a module-level literal assignment, without importing the module (both sources import torch)."""
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == name:
            return ast.literal_eval(node.value)
    raise KeyError(name)


def desc_tuple(N, D, H, W, cin, cout, k, s=(1, 1, 1), p=None, in_ld=None, out_ld=None):
    p = tuple(x // 2 for x in k) if p is None else p
    do, ho, wo = ((i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip((D, H, W), k, s, p))
    return (N, D, H, W, cin, do, ho, wo, cout, *k, *s, *p, in_ld or cin, out_ld or cout)


def subset_cases():
    cases = [desc_tuple(*c) for c in _literal("tests/test_kernels_gpu.py", "NAME_CASES")]
    for name, geoms in _literal("tools/geom_bench.py", "SETS").items():
        cases += [desc_tuple(*g) for g in geoms]
    return cases


def random_cases(n=240, seed=20240611):
    """Seeded random descriptors: kernel 1..7 and stride 1..2 per dimension, channel counts on every tile width, a third of them not
    multiples of 4 (the scalar-gather plans), some with a pitch wider than the channel count."""
    rng = random.Random(seed)
    chans = [8, 16, 24, 32, 48, 64, 96, 128, 144, 160, 192, 256, 288, 320, 512, 576]
    odd = [3, 6, 17, 42, 83, 85, 130, 170, 230, 461]
    cases = []
    while len(cases) < n:
        k = tuple(rng.randint(1, 7) for _ in range(3))
        if k[0] * k[1] * k[2] > 343:
            continue
        s = tuple(rng.randint(1, 2) for _ in range(3))
        p = tuple(rng.randint(0, kk // 2) for kk in k)
        dims = (rng.choice([1, 2, 4, 8, 16]), rng.choice([4, 7, 14, 28, 56]), rng.choice([4, 7, 14, 28, 56, 112]))
        if any(i + 2 * pp < kk for i, kk, pp in zip(dims, k, p)):
            continue
        cin = rng.choice(odd if rng.random() < 0.33 else chans)
        cout = rng.choice(odd if rng.random() < 0.33 else chans)
        in_ld = cin + rng.choice([0, 0, 0, 4, 32, 3])
        out_ld = cout + rng.choice([0, 0, 0, 4, 64, 1])
        cases.append(desc_tuple(rng.choice([1, 2, 8, 16, 32]), *dims, cin, cout, k, s, p, in_ld, out_ld))
    return cases


def all_cases():
    return subset_cases() + [desc_tuple(*w) for w in WORKLOADS] + random_cases()


def plan_rows(lib, mod, cases):
    """Per descriptor: [names x 3, fwd / dgrad / wgrad workspace bytes, executed fractions x 3, stat tiles]."""
    rows = []
    for c in cases:
        ref = C.byref(mod.ConvDesc(*c))
        rows.append([lib.rsp_conv3d_kernel_name(ref, w).decode() for w in (0, 1, 2)] +
                    [lib.rsp_conv3d_fwd_workspace(ref), lib.rsp_conv3d_dgrad_workspace(ref), lib.rsp_conv3d_wgrad_workspace(ref)] +
                    [lib.rsp_conv3d_executed_fraction(ref, w) for w in (0, 1, 2)] + [lib.rsp_conv3d_stat_tiles(ref)])
    return rows


def planned(lib, mod, cases, opts):      # plan_rows under an option set; the options are back at their defaults afterwards
    for name, value in opts.items():
        assert lib.rsp_conv3d_set_option(name.encode(), value) >= 0, name
    try:
        return plan_rows(lib, mod, cases)
    finally:
        for name in opts:
            lib.rsp_conv3d_set_option(name.encode(), -1)


def table(lib, mod):
    cases = all_cases()
    return {"cases": [list(c) for c in cases], "options": OPTIONS, "rows": [planned(lib, mod, cases, opts) for opts in OPTIONS]}


def switch_rows(lib, mod, variable):      # the subset's plan under one of ENV_SWITCHES, set through its option
    return planned(lib, mod, subset_cases(), {SWITCH_OPTIONS[variable]: int(dict(ENV_SWITCHES)[variable])})


def compact(tab):
    """Kernel names as indices into one sorted list (the table repeats a few dozen strings some ten thousand times)."""
    names = sorted({x for rows in tab["rows"] for r in rows for x in r[:3]})
    idx = {n: i for i, n in enumerate(names)}
    return dict(tab, names=names, rows=[[[idx[x] for x in r[:3]] + r[3:] for r in rows] for rows in tab["rows"]])


def expand(tab):
    names = tab["names"]
    return {"cases": tab["cases"], "options": tab["options"],
            "rows": [[[names[x] for x in r[:3]] + r[3:] for r in rows] for rows in tab["rows"]]}


if __name__ == "__main__":
    mod = _lib_module()
    lib = mod.load()
    if sys.argv[1:] == ["--subset"]:
        sys.exit(json.dump(plan_rows(lib, mod, subset_cases()), sys.stdout))
    tab = compact(table(lib, mod))
    tab["env"] = {variable: switch_rows(lib, mod, variable) for variable, _ in ENV_SWITCHES}
    with open(sys.argv[1], "w") as f:
        json.dump(tab, f, separators=(",", ":"))
        f.write("\n")
