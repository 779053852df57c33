"""CPU: step fingerprints (rspnet_amd/fingerprint.py) -- the numpy restatement against known answers worked out from the definition,
totals, the jsonl file and tools/fingerprint_diff.py, the opt-in hook of the fine-tune Engine on the torch checker backend (same
run -> same file, other seed -> other file, key absent -> nothing runs, NaN halt before the optimizer), check_ranks over gloo, and the
argument checks of the C entry point."""
import ctypes
import json
import os
import sys
import tempfile
from unittest import mock

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import finetune_loop_util as U
from cpu_ops import CpuOps
from rspnet_amd import _lib, ops
from rspnet_amd import fingerprint as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fingerprint_diff  # noqa: E402


@pytest.fixture()
def cpu_backend():
    prev = ops.set_backend(CpuOps())
    yield
    ops.set_backend(prev)


# ---- known answers -----------------------------------------------------------------------------------------------------------
def case_D():
    i = np.arange(8193)
    return (((37 * i) % 101 - 50) / 8).astype(np.float32)


def case_E():
    w = case_D().view(np.uint32).copy()
    w[0] = 0x7FC00000
    v = w.view(np.float32)
    v[5] = -0.0
    v[8191] = np.inf
    v[8192] = -np.inf
    return v


def _swapped(a, i, j):
    b = a.copy()
    b[[i, j]] = b[[j, i]]
    return b


B = np.arange(10, dtype=np.float32)
C = ((np.arange(20000, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.uint32)
KNOWN = [("A", np.array([1.0], np.float32), "00000000b1aab1b6", 1.0, 1.0, 1.0, 0),
         ("B", B, "00000003f62a9fb4", 285.0, 45.0, 9.0, 0),
         ("B'", _swapped(B, 2, 7), "000000030a28ac15", 285.0, 45.0, 9.0, 0),
         ("C", C, "000026f441ebf9b1", 0.0, 0.0, 0.0, 0),
         ("D", case_D(), "00000ff74603c94b", 108838.171875, 25859.875, 6.25, 0),
         ("E", case_E(), "00000ff72b6d48a1", 108742.015625, 25841.375, 6.25, 3),
         ("Z", np.zeros(0, np.float32), "0000000000000000", 0.0, 0.0, 0.0, 0)]


@pytest.mark.parametrize("case", KNOWN, ids=[k[0] for k in KNOWN])
def test_reference_records_known_answers(case):
    """The inputs are multiples of 1/8: every order of summation gives the same double, so the floats are exact."""
    _, data, h, sumsq, sum_abs, max_abs, nonfinite = case
    r = F.reference_records([data])[0]
    assert f"{int(r['hash']):016x}" == h
    assert (float(r["sumsq"]), float(r["sum_abs"]), float(r["max_abs"]), int(r["nonfinite"])) == (sumsq, sum_abs, max_abs, nonfinite)


def test_reference_records_of_a_list_and_of_torch_tensors():
    datas = [k[1] for k in KNOWN]
    rec = F.reference_records(datas)
    assert rec.dtype == F.REC_DTYPE and rec.dtype.itemsize == 32 and [f"{int(h):016x}" for h in rec["hash"]] == [k[2] for k in KNOWN]
    # the 20 000 words of C as the 10 000 int64 they are; fp32 through torch
    as_i64 = torch.from_numpy(C.view(np.int64).copy())
    rec2 = F.reference_records([torch.from_numpy(case_E().copy()), as_i64])
    assert rec2[0].tobytes() == rec[5].tobytes() and rec2[1].tobytes() == rec[3].tobytes()
    with pytest.raises(TypeError):
        F.reference_records([torch.zeros(4, dtype=torch.float16)])
    # plain float64 sums of a non-trivial tensor: the fixed order of the kernel is within n * 2^-53 of them
    x = np.random.default_rng(5).standard_normal(3 * 8192 + 17).astype(np.float32)
    r = F.reference_records([x])[0]
    assert abs(r["sumsq"] / np.sum(x.astype(np.float64) ** 2) - 1) < 1e-11 and r["max_abs"] == np.abs(x).max()
    # any single bit changes the hash, whatever its position
    for pos in (0, 4, 8191, 8192, x.size - 1):
        y = x.copy()
        y.view(np.uint32)[pos] ^= 1
        assert F.reference_records([y])[0]["hash"] != r["hash"]


def test_totals():
    rec = F.reference_records([B, case_E(), np.zeros(0, np.float32)])
    t = F.totals(rec)
    h = [int(x) for x in rec["hash"]]
    assert t["hash"] == (h[0] * 1 + h[1] * 3 + h[2] * 5) % (1 << 64)
    assert t["norm"] == (285.0 + 108742.015625) ** 0.5 and t["sum_abs"] == 45.0 + 25841.375 and t["max_abs"] == 9.0 and t["nonfinite"] == 3
    # two tensors trading places is seen by the total
    assert F.totals(rec[[1, 0, 2]])["hash"] != t["hash"]
    assert F.totals(rec[:0]) == {"hash": 0, "norm": 0.0, "sum_abs": 0.0, "max_abs": 0.0, "nonfinite": 0}


# ---- the file and the diff tool ----------------------------------------------------------------------------------------------
class Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 2)
        self.bn = torch.nn.BatchNorm1d(2)

    def forward(self, x):
        return self.bn(self.lin(x))


def test_writer_header_and_lines(cpu_backend, tmp_path):
    torch.manual_seed(0)
    m = Tiny()
    fp = F.StepFingerprints(tmp_path, every=2, halt_on_nonfinite=True)
    assert [fp.due(s) for s in range(4)] == [True, False, True, False]
    for s in (0, 2):
        assert fp.due(s)
        m.zero_grad()
        m(torch.randn(4, 3)).square().sum().backward()
        grec = fp.after_backward(m)
        srec = fp.after_step(0, s, m)
    lines = [json.loads(l) for l in open(tmp_path / "fingerprints.jsonl")]
    state_names = ["lin.weight", "lin.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]
    assert lines[0] == {"version": 1, "chunk": 8192,
                        "names": {"grad": ["lin.weight", "lin.bias", "bn.weight", "bn.bias"], "state": state_names}}
    assert len(lines) == 3 and [l["global_step"] for l in lines[1:]] == [0, 2] and set(lines[1]) == {"epoch", "step", "global_step", "grad", "state"}
    last = lines[2]
    for side, rec in (("grad", grec), ("state", srec)):
        assert set(last[side]) == {"hash", "norm", "sum_abs", "max_abs", "nonfinite", "tensors"}
        assert last[side]["tensors"] == [f"{int(h):016x}" for h in rec["hash"]] and last[side]["hash"] == f"{F.totals(rec)['hash']:016x}"
        assert last[side]["norm"] == F.totals(rec)["norm"]
    assert np.array_equal(grec, F.reference_records([p.grad for p in m.parameters()]))
    # the int64 counter went in as raw words: hash only
    assert srec[6]["hash"] == F.reference_records([torch.tensor(2)])[0]["hash"] and srec[6]["sumsq"] == 0.0
    # rank 1 writes nothing; every = 0 in a config constructs nothing
    assert F.StepFingerprints(tmp_path, 1, rank=1).path is None
    assert F.StepFingerprints.from_config({}, tmp_path) is None and F.StepFingerprints.from_config({"fingerprint": {"every": 0}}, tmp_path) is None
    with pytest.raises(TypeError):
        F.named_state(torch.nn.Linear(2, 2).half())


def _write(path, names, hashes_per_record):
    head = {"version": 1, "chunk": 8192, "names": {"grad": names, "state": names}}
    with open(path, "w") as f:
        f.write(json.dumps(head) + "\n")
        for i, hs in enumerate(hashes_per_record):
            side = {"hash": f"{sum(hs):016x}", "norm": 1.0, "sum_abs": 1.0, "max_abs": 1.0, "nonfinite": 0, "tensors": [f"{h:016x}" for h in hs]}
            f.write(json.dumps({"epoch": 0, "step": i, "global_step": 10 * i, "grad": side, "state": dict(side, hash=f"{7:016x}", tensors=[f"{7:016x}"] * len(hs))}) + "\n")
    return str(path)


def test_fingerprint_diff_tool(tmp_path, capsys):
    names = ["conv.weight", "conv.bias", "fc.weight"]
    same = [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]
    a, b = _write(tmp_path / "a.jsonl", names, same), _write(tmp_path / "b.jsonl", names, same)
    assert fingerprint_diff.main([a, b]) == 0
    assert "identical over 4 records" in capsys.readouterr().out
    other = [list(r) for r in same]
    other[2][1] = 99
    other[3][0] = 98
    c = _write(tmp_path / "c.jsonl", names, other)
    assert fingerprint_diff.main([a, c]) == 1
    out = capsys.readouterr().out
    assert "global_step 20" in out and "grad" in out and "conv.bias" in out and "conv.weight" not in out and "state" not in out
    assert F.first_difference(a, c) == (2, 20, {"grad": ["conv.bias"]})
    d = _write(tmp_path / "d.jsonl", names[:2] + ["fc.bias"], same)
    assert fingerprint_diff.main([a, d]) == 2
    assert "headers" in capsys.readouterr().err
    with pytest.raises(ValueError, match="headers"):
        F.first_difference(a, d)


# ---- the fine-tune Engine on the checker backend -----------------------------------------------------------------------------
def _engine(tmp, seed, fp_cfg, train_steps=1):
    """The Engine as tests/test_finetune_loop_cpu.py builds it (fixture clips and sizes), its weights drawn from `seed`; the first
    `train_steps` batches of the fixture's epoch."""
    from rspnet_amd.finetune import Engine
    _, meta, _ = U.load()
    meta = dict(meta, train_steps=train_steps)
    cfg = U.config(meta)
    if fp_cfg is not None:
        cfg["fingerprint"] = fp_cfg
    os.makedirs(tmp, exist_ok=True)
    torch.manual_seed(seed)
    dev = torch.device("cpu")
    return Engine(U.make_args(tmp), cfg, 0, train_loader=U.FixtureLoader(meta, "train", dev), validate_loader=U.FixtureLoader(meta, "val", dev))


def test_engine_runs_are_identical_or_told_apart(cpu_backend, tmp_path):
    paths = []
    for tag, seed, n in (("a", 3, 2), ("b", 3, 2), ("c", 4, 1)):
        eng = _engine(tmp_path / tag, seed, {"every": 1}, train_steps=n)
        eng.train_epoch()
        paths.append(str(tmp_path / tag / "fingerprints.jsonl"))
    head, recs = F.load_file(paths[0])
    assert len(recs) == 2 and [r["global_step"] for r in recs] == [0, 1]
    assert "fc.weight" in head["names"]["grad"] and any(n.endswith("num_batches_tracked") for n in head["names"]["state"])
    assert all(r["grad"]["nonfinite"] == 0 and r["grad"]["norm"] > 0 for r in recs)
    assert fingerprint_diff.main(paths[:2]) == 0
    assert fingerprint_diff.main([paths[0], paths[2]]) == 1
    assert F.first_difference(paths[0], paths[2])[0] == 0


def test_engine_without_the_key_issues_nothing(cpu_backend, tmp_path):
    with mock.patch.object(F.FingerprintSet, "run") as run:
        eng = _engine(tmp_path, 3, None)
        assert eng.fingerprints is None
        eng.train_epoch()
        assert not run.called
    assert not (tmp_path / "fingerprints.jsonl").exists()
    eng = _engine(tmp_path / "zero", 3, {"every": 0, "halt_on_nonfinite": True})
    assert eng.fingerprints is None


def test_engine_halts_on_a_nonfinite_gradient_before_the_optimizer(cpu_backend, tmp_path):
    eng = _engine(tmp_path, 3, {"every": 1, "halt_on_nonfinite": True})
    with torch.no_grad():
        eng.model.module.fc.weight[0, 0] = float("nan")
    before = {n: p.detach().clone() for n, p in eng.model.module.named_parameters()}
    with pytest.raises(FloatingPointError, match="fc.weight"):
        eng.train_epoch()
    for n, p in eng.model.module.named_parameters():
        assert torch.equal(p.detach().view(torch.int32), before[n].view(torch.int32)), n      # bit for bit, the NaN included
    assert not (tmp_path / "fingerprints.jsonl").exists()      # halted before the first record


# ---- check_ranks over gloo -----------------------------------------------------------------------------------------------------
def _ranks_worker(rank, ws, port, tmp):
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from rspnet_amd import fingerprint as FF
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    names = ["conv1.weight", "conv1.bias", "fc.weight"]
    g = np.random.default_rng(11)
    tensors = [g.standard_normal(n).astype(np.float32) for n in (9000, 7, 300)]
    FF.check_ranks(FF.reference_records(tensors), names)                      # equal everywhere: returns
    if rank == 1:
        tensors[1].view(np.uint32)[3] ^= 1                                    # one bit of one tensor on one rank
    try:
        FF.check_ranks(FF.reference_records(tensors), names)
        msg = "returned"
    except RuntimeError as e:
        msg = str(e)
    with open(os.path.join(tmp, f"msg{rank}.txt"), "w") as f:
        f.write(msg)
    dist.barrier()
    dist.destroy_process_group()


def test_check_ranks_over_gloo():
    from oracle.ref_harness import _free_port
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_ranks_worker, args=(2, _free_port(), tmp), nprocs=2, join=True)
        msgs = [open(os.path.join(tmp, f"msg{r}.txt")).read() for r in range(2)]
    for m in msgs:
        assert "conv1.bias" in m and "conv1.weight" not in m and "fc.weight" not in m and "1 of 3 tensors differ" in m, m
        assert "ranks [0]" in m and "ranks [1]" in m
    assert msgs[0] == msgs[1]
    # no process group: nothing to compare, nothing raised
    F.check_ranks(F.reference_records([B]), ["b"])


# ---- the C entry point ---------------------------------------------------------------------------------------------------------
def test_abi_names_and_argument_checks():
    lib = _lib.load()
    assert hasattr(lib, "rsp_fingerprint") and hasattr(lib, "rsp_fingerprint_workspace")
    assert ctypes.sizeof(_lib.FingerprintJob) == 32 and ctypes.sizeof(_lib.FingerprintRec) == 32
    assert lib.rsp_fingerprint_workspace(5) == 5 * 32 and lib.rsp_fingerprint_workspace(0) == 0 and lib.rsp_fingerprint_workspace(-1) == 0
    P = ctypes.c_void_p(1 << 20)      # non-null, aligned, never touched: nothing is launched
    assert lib.rsp_fingerprint(P, 3, 5, P, P, 5 * 32 - 1, None) == -2
    assert lib.rsp_last_error().startswith(b"rsp_fingerprint: ") and b"workspace" in lib.rsp_last_error()
    assert lib.rsp_fingerprint(P, -1, 5, P, P, 1 << 20, None) == -1
    assert lib.rsp_last_error().startswith(b"rsp_fingerprint: ")
    assert lib.rsp_fingerprint(P, 3, -1, P, P, 1 << 20, None) == -1 and lib.rsp_last_error().startswith(b"rsp_fingerprint: ")
    assert lib.rsp_fingerprint(None, 3, 5, P, P, 1 << 20, None) == -1 and lib.rsp_last_error().startswith(b"rsp_fingerprint: ")
    assert lib.rsp_fingerprint(None, 0, 0, None, None, 0, None) == 0      # no job: no launch, no error
    assert lib.rsp_version() == 130
