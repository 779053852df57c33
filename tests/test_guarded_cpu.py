"""CPU: the guarded-memory detector itself (tests/guarded.py) on small fake "ops" written in torch, each with one planted defect of the
kind a wrong kernel would have.  The fakes allocate the way rspnet_amd/ops.py does — through the module's own `torch` name — and reach
outside their operands the way a kernel with a wrong extent would: inside the block the guard owns.  This is the evidence that
tests/test_guarded_memory_gpu.py fails on a wrong kernel; nothing wrong is ever run on a GPU."""
import re

import pytest
import torch

from guarded import BAND_MAX, BAND_MIN, GuardError, Guarded
from rspnet_amd import ops as O

CPU = torch.device("cpu")
N = 24                      # elements of every operand here: 96 bytes, bands of 64 KiB + 16


def outside(t, k):
    """The float k places from t's first element: k < 0 or k >= t.numel() is outside t, in the guard's band."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + k)


def fake_op(x, defect=None):
    """y = 2 * x, with ops.py's allocation idiom."""
    y = O.torch.empty(x.shape, dtype=torch.float32, device=x.device)
    y.copy_(2 * x)
    if defect == "behind":
        outside(y, N).fill_(1.0)
    elif defect == "front":
        outside(y, -1).fill_(1.0)
    elif defect == "far":
        outside(y, N + (BAND_MIN + 16) // 4 - 1).fill_(1.0)
    elif defect == "unwritten":
        y[5] = torch.tensor(-1, dtype=torch.int32).view(torch.float32)      # what the allocation held before the op
    elif defect == "input":
        x[3] = 0.0
    elif defect == "read":
        y[N - 1] = 2 * outside(x, N)[0]
    elif defect == "nan":
        y[7] = float("nan")
    return y


def run(defect, check=True):
    x_cpu = torch.arange(N, dtype=torch.float32) + 1
    with Guarded(CPU) as G:
        x = G.put(x_cpu, name="x")
        y = fake_op(x, defect)
        if check:
            G.check()
    return x_cpu, y


def report_of(defect):
    with pytest.raises(GuardError) as e:
        run(defect)
    lines = str(e.value).splitlines()
    assert lines[0] == "guarded memory: 1 finding(s)", lines
    return lines[1].strip()


def test_clean_op_passes():
    x, y = run(None)
    assert torch.equal(y, 2 * x)


def test_store_behind_the_output_is_reported():
    line = report_of("behind")
    assert re.search(r"output test_guarded_cpu\.py:\d+ \(fake_op\): back band written, first bad byte at offset 96 of the payload, 4 bytes", line), line


def test_store_in_front_of_the_output_is_reported():
    line = report_of("front")
    assert re.search(r"output test_guarded_cpu\.py:\d+ \(fake_op\): front band written, first bad byte at offset -4 of the payload, 4 bytes", line), line


def test_store_into_the_far_end_of_a_band_is_reported():
    line = report_of("far")
    last = 96 + BAND_MIN + 16 - 4
    assert f"(fake_op): back band written, first bad byte at offset {last} of the payload, 4 bytes" in line, line


def test_unwritten_element_is_reported():
    line = report_of("unwritten")
    assert re.search(r"output test_guarded_cpu\.py:\d+ \(fake_op\): never written, first bad byte at offset 20 of the payload, 1 elements", line), line


def test_changed_input_is_reported():
    line = report_of("input")
    # 4.0 -> 0.0: bytes 00 00 80 40 -> 00 00 00 00, the two high bytes change
    assert line.startswith("input x: input changed, first bad byte at offset 14 of the payload, 2 bytes"), line


def test_read_from_an_inputs_band_gives_nan():
    x, y = run("read", check=False)          # no separate check for reads: the value check of the test body fails on the NaN
    assert torch.isnan(y[N - 1])
    assert torch.equal(y[:N - 1], 2 * x[:N - 1])
    err = (y.double() - 2 * x.double()).abs().max().item()
    assert not err <= 1e-5                   # how close() in the kernel tests fails on it


def test_computed_nan_is_not_reported_as_unwritten():
    x, y = run("nan")
    assert y[7].view(torch.int32).item() == 0x7FC00000


def test_test_owned_outputs_and_integer_outputs_are_exempt_from_the_unwritten_check():
    with Guarded(CPU) as G:
        G.alloc((4, 6))                                                       # the test's own: partially written by design (slices)
        idx = O.torch.empty((3, 5), dtype=torch.int32, device=CPU)            # -1 is a legal neighbour index
        assert bool((idx == -1).all())
        G.check()


def test_layout_alignment_and_band_sizes():
    with Guarded(CPU) as G:
        a = G.alloc((N,))
        big = G.alloc((BAND_MAX // 4 + 100,))
        odd = G.alloc((17, 83))                                               # 5644 bytes
        assert a.data_ptr() % 32 == 16 and big.data_ptr() % 32 == 16 and odd.data_ptr() % 32 == 16
        assert [b.band for b in G.blocks] == [BAND_MIN + 16, BAND_MAX + 16, BAND_MIN + 16]
        assert bool((a.view(torch.int32) == -1).all()) and bool(torch.isnan(a).all())
        for b in G.blocks:
            assert b.block.numel() == 2 * b.band + b.nbytes and bool((b.block == 0xFF).all())
    with Guarded(CPU, skew=8) as G:
        a = G.alloc((N,), torch.int64)
        assert a.data_ptr() % 16 == 8 and a.shape == (N,) and a.dtype == torch.int64


def test_proxy_forwards_everything_else_and_leaves_host_allocations_alone():
    with Guarded(CPU) as G:
        assert O.torch.float32 is torch.float32 and O.torch.cuda is torch.cuda and O.torch.Tensor is torch.Tensor
        z = O.torch.zeros(5, dtype=torch.float32, device=CPU)
        assert bool((z == 0).all()) and len(G.blocks) == 1
        like = O.torch.empty_like(z)
        assert like.shape == z.shape and len(G.blocks) == 2
        t = O.torch.empty(7)                                                  # no device: not the guard's business
        p = O.torch.empty(7, device="meta")
        assert len(G.blocks) == 2 and t.shape == p.shape == (7,)
    assert O.torch is torch


class FakeHip:
    """The workspace part of rspnet_amd.ops.HipOps, on the CPU."""

    def __init__(self):
        self._ws = {"kept": torch.zeros(8, dtype=torch.uint8)}

    def _workspace(self, dev, nbytes):
        buf = self._ws.get(dev)
        if buf is None or buf.numel() < nbytes:
            buf = self._ws[dev] = O.torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        return buf


def test_workspace_is_refilled_before_every_call_and_guarded():
    hip = FakeHip()
    with Guarded(CPU, hip=hip) as G:
        assert hip._ws == {}
        ws = hip._workspace(CPU, 100)
        assert bool((ws == 0xFF).all())
        ws.zero_()                                                            # an op's partials
        ws2 = hip._workspace(CPU, 100)
        assert ws2.data_ptr() == ws.data_ptr() and bool((ws2 == 0xFF).all())
        assert G.blocks[0].kind == "workspace"
        G.check()
        torch.as_strided(ws2, (1,), (1,), ws2.storage_offset() + ws2.numel()).zero_()      # one byte past the workspace
        with pytest.raises(GuardError) as e:
            G.check()
        assert "workspace test_guarded_cpu.py" in str(e.value) and "(_workspace): back band written, first bad byte at offset 256" in str(e.value)


def test_everything_is_restored_after_an_exception():
    hip = FakeHip()
    kept = hip._ws
    method = hip._workspace
    with pytest.raises(ZeroDivisionError):
        with Guarded(CPU, hip=hip):
            assert O.torch is not torch and hip._ws is not kept and "_workspace" in vars(hip)
            1 / 0
    assert O.torch is torch and hip._ws is kept and "_workspace" not in vars(hip) and hip._workspace == method
    with pytest.raises(GuardError):
        run("behind")
    assert O.torch is torch
