"""CPU: the parts the drivers share (rspnet_amd.framework: DeviceMeters, the argument helpers, load_states) seen through the
drivers that use them: meter layout and partial update, the two command lines against tests/golden/driver_cli.json (dumped from
the drivers as they were before they shared a parser block), import separation, the arch check of the three checkpoint loaders."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path
from unittest import mock

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "driver_cli.json")


# ---- meters ----------------------------------------------------------------------------------------------------------------
def meter_classes():
    from rspnet_amd import _lib
    from rspnet_amd.finetune import Meters
    from rspnet_amd.pretrain import PretextMeters
    return {3: (Meters, _lib.ClsMeters), 8: (PretextMeters, _lib.PretextMeters)}


@pytest.mark.parametrize("N", (3, 8))
def test_meter_layout(N):
    cls, struct = meter_classes()[N]
    m = cls("cpu")
    assert len(cls.KEYS) == len(cls.NAMES) == len(cls.FMTS) == N
    assert m.buf.dtype == torch.uint8 and m.buf.numel() == ctypes.sizeof(struct) == 12 * N
    for view, dtype, offset in ((m.val, torch.float32, 0), (m.sum, torch.float32, 4 * N), (m.count, torch.int32, 8 * N)):
        assert view.dtype == dtype and view.numel() == N
        assert view.data_ptr() == m.buf.data_ptr() + offset
        assert offset == getattr(struct, {0: "val", 4 * N: "sum", 8 * N: "count"}[offset]).offset


@pytest.mark.parametrize("N,k", ((3, 2), (8, 8)))
def test_meter_partial_update_and_fp32_sums(N, k):
    cls, _ = meter_classes()[N]
    m = cls("cpu")
    # a recognisable bit pattern in every entry, NaN payloads and negative counts included: untouched means bit-identical
    m.buf.copy_(torch.arange(1, 12 * N + 1, dtype=torch.uint8) * 37)
    before = m.buf.clone()
    v0 = [np.float32(x) for x in (0.1, 33.333332, 2.7182817, 100.0, 1e-3, 6.25, 0.3, 99.99)[:k]]
    v1 = [np.float32(x) for x in (0.7, 66.666664, 3.1415927, 0.0, 1e3, 12.5, 0.9, 0.01)[:k]]
    n0, n1 = 3, 7
    m.val[:k], m.sum[:k], m.count[:k] = 0, 0, 0
    m.update([torch.tensor(x) for x in v0], n0)
    m.update([torch.tensor(x) for x in v1], n1)
    want = [np.float32(np.float32(a * np.float32(n0)) + np.float32(b * np.float32(n1))) for a, b in zip(v0, v1)]
    assert m.val[:k].tolist() == [float(b) for b in v1]
    assert m.sum[:k].tolist() == [float(w) for w in want]
    assert m.count[:k].tolist() == [n0 + n1] * k
    for lo in (0, 4 * N, 8 * N):      # entries k..N-1 of val, sum and count
        assert torch.equal(m.buf[lo + 4 * k:lo + 4 * N], before[lo + 4 * k:lo + 4 * N])
    stats = m.read()
    assert list(stats) == list(cls.KEYS)
    assert stats[cls.KEYS[0]] == {"val": float(v1[0]), "avg": float(want[0] / np.float32(n0 + n1)), "sum": float(want[0]),
                                  "count": n0 + n1}


# ---- command lines ---------------------------------------------------------------------------------------------------------
def cli_dump(tmp: Path) -> dict:
    """Per driver: every argparse action by dest (option strings, default, type and action class names) and the namespaces that
    four argument vectors parse to, the temporary directory written as <TMP> and run_dir cut down to its run id."""
    from rspnet_amd import finetune, pretrain
    parsers = []
    orig = argparse.ArgumentParser.parse_args

    def spy(self, *a, **k):
        parsers.append(self)
        return orig(self, *a, **k)

    out = {}
    for name, mod in (("pretrain", pretrain), ("finetune", finetune)):
        exp, prev = tmp / name / "exp", tmp / name / "prev"
        (prev / "run_4_x").mkdir(parents=True)
        (prev / "run_4_x" / "config.json").write_text("{}")
        (prev / "checkpoint.pth.tar").write_bytes(b"")
        vectors = {"minimal": ["-c", "cfg.json", "-e", str(exp)],
                   "continue": ["-e", str(prev), "--continue"],
                   "ws_seed_debug": ["-c", "cfg.json", "-e", str(exp), "--ws", "2", "--seed", "7", "-d"],
                   "overlays": ["-c", "cfg.json", "-e", str(exp), "-x", '{"a": 1}', "-x", '{"b": {"c": 2}}']}
        del parsers[:]
        spaces = {}
        with mock.patch.object(argparse.ArgumentParser, "parse_args", spy), \
                mock.patch.object(pretrain, "visible_gpu_count", lambda: 3):      # pretext's --ws default: no child interpreter here
            for key, argv in vectors.items():
                ns = dict(vars(mod.parse_args(argv)))
                ns["run_dir"] = pretrain.RUN_DIR_NAME_REGEX.match(Path(ns["run_dir"]).name).group(0)
                spaces[key] = {k: v.replace(str(tmp), "<TMP>") if isinstance(v, str) else v for k, v in ns.items()}
        actions = {a.dest: {"option_strings": list(a.option_strings), "default": a.default, "required": a.required,
                            "type": None if a.type is None else a.type.__name__, "action": type(a).__name__}
                   for a in parsers[0]._actions}
        out[name] = {"actions": actions, "namespaces": spaces}
    return json.loads(json.dumps(out))


def test_command_lines_unchanged(tmp_path):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = cli_dump(tmp_path)
    for name in ("pretrain", "finetune"):
        assert got[name]["actions"] == golden[name]["actions"], name
        assert got[name]["namespaces"] == golden[name]["namespaces"], name
    assert got == golden


def test_finetune_does_not_import_the_pretext_driver():
    code = ("import sys; import rspnet_amd.finetune; assert 'rspnet_amd.finetune' in sys.modules; "
            "assert 'rspnet_amd.pretrain' not in sys.modules, 'rspnet_amd.finetune imported rspnet_amd.pretrain'")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- checkpoint arch check -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module,method", (("pretrain", "load_model"), ("pretrain", "load_checkpoint"), ("finetune", "load_checkpoint"),
                                           ("visualization", "load_model")))
def test_wrong_arch_is_refused_by_every_loader(module, method, tmp_path):
    """The check needs the engine's device and arch only and comes before any state is loaded: a stand-in model is enough."""
    import importlib
    engine_cls = importlib.import_module(f"rspnet_amd.{module}").Engine
    eng = object.__new__(engine_cls)
    eng.device, eng.arch, eng.model = torch.device("cpu"), "c3d", mock.MagicMock()
    path = tmp_path / "wrong.pth.tar"
    torch.save({"arch": "resnet18", "model": {}, "epoch": 1}, path)
    with pytest.raises(ValueError) as e:
        getattr(eng, method)(path)
    assert str(e.value) == "Loading checkpoint arch resnet18 does not match current arch c3d"
