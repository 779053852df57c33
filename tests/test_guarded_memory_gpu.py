"""GPU: the per-kernel test bodies again, with every operand inside guarded memory (tests/guarded.py).

Each body of test_kernels_gpu / test_bn_eval_bwd_gpu / test_retrieval_gpu / test_knn_gpu / test_pack_gpu listed below runs unchanged, at its own cases
and tolerances, while the module's dev() / dev_empty() hand out guarded allocations and rspnet_amd.ops allocates its outputs and
workspaces from the guard too.  The body's comparison against CpuOps / fp64 stays the value check (a read outside an operand meets the
NaN moat and fails it); Guarded.check() then asserts that no band byte changed, no input changed and no float32 output of the op kept
an unwritten word.  tests/test_guarded_cpu.py shows the detector reporting each of these on planted defects.

Alignment: payloads are 16-byte and not 32-byte aligned for the conv / BatchNorm family, 8-byte and not 16-byte aligned for the
search kernels — what include/rspnet_hip.h promises and no more.

test_pitched_conv is new: conv_fwd into a channel slice (out= / out_ld=) and conv_wgrad from a channel-slice dy, where a row overrun
cannot hide behind the next row's owner; and conv_fwd from rows of a wider pitch (in_ld=)."""
import contextlib
import inspect

import numpy as np
import pytest
import torch

import test_bn_eval_bwd_gpu as B
import test_kernels_gpu as K
import test_knn_gpu as Q
import test_pack_gpu as P
import test_retrieval_gpu as R
from guarded import Guarded
from rspnet_amd.ops import ConvGeom

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def hip():
    from rspnet_amd import ops
    assert ops.backend().name == "hip"
    return ops.backend()


def _cases_of(fn):
    """The (id, kwargs) list of a body: its own parametrize marks, so the guarded run follows the case lists of the module."""
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    if not marks:
        return [("", {})]
    assert len(marks) == 1, fn.__name__
    names, values = marks[0].args
    names = [n.strip() for n in names.split(",")]
    ids = marks[0].kwargs.get("ids")
    out = []
    for v in values:
        vals = (v,) if len(names) == 1 else tuple(v)
        label = ids(v) if callable(ids) and len(names) == 1 else "-".join(str(x) for x in vals)
        out.append((label, dict(zip(names, vals))))
    return out


# (module, body, payload skew): every case of every body listed here
BODIES = [(K, name, 16) for name in (
    "test_conv_fwd_dgrad_wgrad", "test_conv_tall_and_narrow32_instances", "test_conv_fuzz", "test_conv_fuzz_padded_depth",
    "test_bn_finalize", "test_bn_act_pool_fwd_bwd", "test_maxpool_fwd_bwd", "test_head_fwd_bwd", "test_logits_and_loss",
    "test_gate_fwd_bwd_and_channel_slices", "test_bn_act_pool_channel_slices", "test_mlp_head_pieces",
    "test_channel_padded_unit_uses_the_parameters_own_lengths", "test_deferred_running_statistics_update",
    "test_virtual_pixel_stem_equals_padded_stem", "test_bn_act_gate_fused_is_bit_identical_to_the_three_ops",
    "test_bn_act_pool_fwd_overlapping_window_equals_apply_then_maxpool", "test_bn_act_gate_bwd_fused_matches_the_two_ops",
    "test_momentum_and_sgd", "test_clip_gather", "test_queue_enqueue_and_rows_gather",
    "test_wgrad_without_a_kept_table_computes_its_own")]
BODIES += [(B, "test_bn_eval_act_pool_bwd_matches_autograd", 16)]
BODIES += [(R, "test_cosine_topk_edges", 8), (R, "test_zero_rows_and_strided_inputs", 8)]
BODIES += [(Q, "test_knn_matches_fp64_reference", 8), (Q, "test_zero_rows_bad_labels_and_valid", 8),
           (Q, "test_tie_straddling_rank_k_goes_to_the_lower_index", 8)]
# the batched re-pack and the input gradient over its buffers: the dgrad buffers' unowned tails stay the NaN pattern (the bodies
# declare them and look at the word set themselves), the workspace is the NaN pattern too, and dx must come out finite and whole
BODIES += [(P, name, 16) for name in ("test_forward_layout_equals_the_single_packer", "test_packed_dgrad", "test_one_table_many_jobs")]

GUARDED = [pytest.param(mod, name, skew, kw, id=f"{name}[{label}]" if label else name)
           for mod, name, skew in BODIES for label, kw in _cases_of(getattr(mod, name))]


@contextlib.contextmanager
def placed_in(mod, G):
    """The module's device placement pointed at the guard, for the length of one body."""
    saved = {n: getattr(mod, n) for n in ("dev", "dev_empty", "GUARD") if hasattr(mod, n)}
    try:
        if "GUARD" in saved:      # (a module whose ops leave part of an output unwritten by contract tells the guard which)
            mod.GUARD = G
        if mod is Q:      # (its dev() takes numpy arrays and returns a list)
            mod.dev = lambda *arrays: [G.put(torch.from_numpy(np.array(a))) for a in arrays]
        else:
            mod.dev, mod.dev_empty = G.put, G.empty
        yield
    finally:
        for n, f in saved.items():
            setattr(mod, n, f)


@pytest.mark.parametrize("mod,name,skew,kw", GUARDED)
def test_guarded(hip, mod, name, skew, kw):
    fn = getattr(mod, name)
    if "hip" in inspect.signature(fn).parameters:
        kw = dict(kw, hip=hip)
    with Guarded(DEV, skew=skew) as G:
        with placed_in(mod, G):
            fn(**kw)
        G.check()
        # the guard was in the way: the op's outputs came from it (the optimizer kernels work in place and allocate nothing), and so
        # did the body's operands (the stem test places its own)
        assert name == "test_momentum_and_sgd" or any(b.proxy for b in G.blocks), "the op allocated nothing through the guard"
        assert name == "test_virtual_pixel_stem_equals_padded_stem" or any(not b.proxy for b in G.blocks), "no operand was guarded"


def test_guard_is_in_effect_on_the_device(hip):
    """What the cases above rely on, looked at once: inside the guard an op's output, statistics and workspace lie in guarded blocks at
    the promised alignment, the workspace is the NaN pattern when the kernel starts, and all of it is undone on the way out."""
    from rspnet_amd import ops
    g = ConvGeom(1, 2, 7, 7, 256, 512, (3, 3, 3), (1, 1, 1), (1, 1, 1))      # split-K: partials in the workspace
    kept_ws = hip._ws
    with Guarded(DEV) as G:
        assert ops.torch is not torch and hip._ws == {}
        xd, wd = G.put(K.rnd(1, 2, 7, 7, 256, seed=5)), G.put(K.rnd(512, 256, 3, 3, 3, seed=6))
        y, st = hip.conv_fwd(g, xd, hip.conv_pack_fwd(g, wd), None, True)
        inside = lambda t: any(b.payload.data_ptr() <= t.data_ptr() < b.payload.data_ptr() + max(b.nbytes, 1) for b in G.blocks)
        assert inside(xd) and inside(y) and inside(st)
        assert xd.data_ptr() % 32 == 16 and y.data_ptr() % 32 == 16 and st.data_ptr() % 32 == 16
        ws = [b for b in G.blocks if b.kind == "workspace"]
        assert len(ws) == 1 and list(hip._ws.values())[0].data_ptr() == ws[0].payload.data_ptr()
        assert bool((hip._workspace(DEV, 1024) == 0xFF).all())
        G.check()
    assert ops.torch is torch and hip._ws is kept_ws and "_workspace" not in vars(hip)
    with Guarded(DEV, skew=8) as G:
        assert G.put(torch.zeros(5)).data_ptr() % 16 == 8
    # capture tests stay unguarded: the guard refuses to activate on a capturing stream
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    t = torch.zeros(8, device=DEV)
    guard = Guarded(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            t.add_(1.0)
            with pytest.raises(RuntimeError, match="capturing"):
                guard.__enter__()
    torch.cuda.current_stream().wait_stream(side)
    assert ops.torch is torch and hip._ws is kept_ws


def _conv_case(N, D, H, W, Cin, Cout, s=None):
    found = [c for c in K.CONV_CASES if c[:6] == (N, D, H, W, Cin, Cout) and (s is None or c[7] == s)]
    assert len(found) == 1, (N, D, H, W, Cin, Cout, found)
    return found[0]


# one entry of CONV_CASES per tile family
PITCHED_CASES = [_conv_case(2, 4, 10, 10, 64, 128), _conv_case(2, 4, 7, 7, 192, 16), _conv_case(2, 4, 12, 12, 64, 132),
                 _conv_case(1, 2, 7, 7, 256, 576), _conv_case(2, 4, 9, 9, 64, 96), _conv_case(3, 4, 7, 7, 48, 72, (2, 2, 2))]


@pytest.mark.parametrize("case", PITCHED_CASES, ids=lambda c: "x".join(map(str, c[:6])) + f"k{c[6]}s{c[7]}")
def test_pitched_conv(hip, case):
    """conv_fwd (bias + statistics) into channels [24, 24 + Cout) of a tensor of pitch Cout + 40, and conv_wgrad (+ dbias) from a dy
    that is the same kind of slice, against CpuOps at the per-kernel tolerance; the other 40 channels of every row keep their 0xFF
    bytes (the forward's) and are never read (the weight gradient's: they are NaN).  Last, the forward from an x whose rows have pitch
    Cin + 40 (in_ld=), the 40 being NaN."""
    N, D, H, W, Cin, Cout, k, s, p = case
    g = ConvGeom(N, D, H, W, Cin, Cout, k, s, p)
    c0, pitch = 24, Cout + 40
    x = K.rnd(N, D, H, W, Cin, seed=1)
    w = K.rnd(Cout, Cin, *k, seed=2, scale=(Cin * k[0] * k[1] * k[2]) ** -0.5)
    b = K.rnd(Cout, seed=3)
    y_ref, st_ref = K.CPU.conv_fwd(g, x, w, b, True)
    dy = K.rnd(*y_ref.shape, seed=4)
    dw_ref, db_ref = torch.empty_like(w), torch.empty_like(b)
    K.CPU.conv_wgrad(g, x, dy, dw_ref, db_ref)
    with Guarded(DEV) as G:
        xd, wd, bd = G.put(x), G.put(w), G.put(b)
        wide = G.alloc(tuple(y_ref.shape[:4]) + (pitch,), name="wide y")
        view = wide[..., c0:c0 + Cout]
        y, st = hip.conv_fwd(g, xd, hip.conv_pack_fwd(g, wd), bd, True, out=view, out_ld=pitch)
        assert y.data_ptr() == view.data_ptr()
        K.close(view, y_ref, 2e-5, "pitched conv fwd")
        K.close(st.double().sum(0), st_ref.double().sum(0), 2e-5, "stat partials")
        bits = wide.view(torch.int32)
        assert bool((bits[..., :c0] == -1).all()) and bool((bits[..., c0 + Cout:] == -1).all()), "a store outside the channel slice"
        dwide = G.alloc(tuple(y_ref.shape[:4]) + (pitch,), name="wide dy")
        dwide[..., c0:c0 + Cout] = dy.to(DEV)
        dw, db = G.alloc(w.shape, name="dw"), G.alloc(b.shape, name="db")
        hip.conv_wgrad(g, xd, dwide[..., c0:c0 + Cout], dw, db)
        K.close(dw, dw_ref, 2e-5, "wgrad from a pitched dy")
        K.close(db, db_ref, 2e-5, "dbias from a pitched dy")
        dbits = dwide.view(torch.int32)
        assert bool((dbits[..., :c0] == -1).all()) and bool((dbits[..., c0 + Cout:] == -1).all())
        # in_ld=: the input as the first Cin channels of rows of pitch Cin + 40 (the other 40 are NaN: never read)
        xwide = G.alloc((N, D, H, W, Cin + 40), name="wide x")
        xwide[..., :Cin] = xd
        y2, st2 = hip.conv_fwd(g, xwide, hip.conv_pack_fwd(g, wd), None, False, in_ld=Cin + 40)
        assert st2 is None
        K.close(y2, y_ref - b, 2e-5, "conv fwd from a pitched x")
        G.check()
