"""Trace of the plan executor's backend calls (test infrastructure).

`TraceOps` wraps the torch checker backend (tests/cpu_ops_eval.py), forwards every call and appends one text line per call:
the method name and, for every argument, a tensor's (shape, strides, dtype, storage offset), a ConvGeom / PoolGeom's fields,
scalars as themselves.  `tracing()` installs it and also logs every `BranchStreams.run` (node type, branch), every
`BranchStreams.side_task` (cost, whether it was collected for later) and every `after_param_grads` hook call (node index).
No tensor VALUE enters a line, so the text depends on the executor's control flow and on shapes only and is the same on every
machine: tests/test_engine_trace_cpu.py compares it with tests/golden/engine_op_trace.json, written by
tools/gen_engine_trace.py from the commit BEFORE a restructuring of rspnet_amd/engine.py.  `values=True` adds exact
checksums of every tensor argument and result to each line (same machine, same thread count only).

The optional backend capabilities the executor probes for are switchable, so both sides of each probe are traced:
`maxpool_fused` (hasattr bn_act_maxpool_fwd), `eval_bwd` (hasattr bn_eval_act_pool_bwd), `gate_pool_keep` (the attribute, with
`pool_idx` support in bn_act_gate_fwd); the ones the checker lacks are compositions of its primitives, as in
tests/teacher_forced.py.

The peak number of live bytes among the tensors the backend RETURNED is tracked with weak references: a restructuring must not
keep saved state or gradients alive for longer."""
import contextlib
import hashlib
import weakref
from collections import Counter

import numpy as np
import torch
from torch import nn

from cpu_ops_eval import CpuOpsEval
from rspnet_amd import engine, ops
from rspnet_amd.moco import split_wrapper
from rspnet_amd.ops import ConvGeom, PoolGeom

CPU = torch.device("cpu")
# write-only tensor arguments (positions; the keywords `out`, `dy_out`, `batch_stats_out` always are): buffers that may be
# uninitialised before the call, so `values` checksums them after the call only
OUTPUTS = {"conv_wgrad": (3, 4), "bn_act_pool_bwd": (9, 10), "bn_eval_act_pool_bwd": (8, 9), "bn_act_gate_bwd": (10, 11, 12, 13),
           "gate_bwd": (5, 6), "head_bwd": (7, 8, 9, 10), "linear_bwd": (5, 6)}
OUTPUT_KEYWORDS = ("out", "dy_out", "batch_stats_out")


def _dtype(t):
    return str(t.dtype).replace("torch.", "")


class TraceOps:
    name = "op-trace"

    def __init__(self, maxpool_fused=True, eval_bwd=True, gate_pool_keep=False, values=False):
        self.inner = CpuOpsEval()
        self.caps = {"bn_act_maxpool_fwd": maxpool_fused, "bn_eval_act_pool_bwd": eval_bwd}
        self.gate_pool_keep = gate_pool_keep
        self.values = values
        self.lines = []
        self.live = 0
        self.peak = 0
        self._seen = set()

    # ---- the record ------------------------------------------------------------------------------------------------
    def log(self, line):
        self.lines.append(line)

    def _fmt(self, v, values=True):
        if isinstance(v, torch.Tensor):
            s = f"T{tuple(v.shape)}/{tuple(v.stride())}/{_dtype(v)}/{v.storage_offset()}"
            if self.values and values:
                d = v.detach().double()
                s += f"={float(d.sum()).hex()},{float(d.abs().sum()).hex()}"
            return s
        if isinstance(v, ConvGeom):
            return f"CG{(v.N, v.Di, v.Hi, v.Wi, v.Cin, v.Cout, tuple(v.k), tuple(v.s), tuple(v.p), v.Cin_alg)}"
        if isinstance(v, PoolGeom):
            return f"PG{(v.N, v.Di, v.Hi, v.Wi, v.C, tuple(v.k), tuple(v.s), tuple(v.p))}"
        if isinstance(v, (list, tuple)):
            return "[" + ",".join(self._fmt(e) for e in v) + "]"
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        return type(v).__name__

    def _track(self, out, args):
        for t in (out if isinstance(out, (list, tuple)) else (out,)):
            if isinstance(t, (list, tuple)):
                self._track(t, args)
            elif isinstance(t, torch.Tensor) and id(t) not in self._seen and not any(t is a for a in args):
                n = t.numel() * t.element_size()
                self._seen.add(id(t))
                self.live += n
                weakref.finalize(t, self._dropped, id(t), n)
        self.peak = max(self.peak, self.live)

    def _dropped(self, key, n):
        self._seen.discard(key)
        self.live -= n

    def _traced(self, name, fn):
        def call(*args, **kwargs):
            outs = OUTPUTS.get(name, ())
            line = "|".join([name] + [self._fmt(a, i not in outs) for i, a in enumerate(args)]
                            + [f"{k}={self._fmt(kwargs[k], k not in OUTPUT_KEYWORDS)}" for k in sorted(kwargs)])
            out = fn(*args, **kwargs)
            if self.values:
                line += "|->" + self._fmt(out) + "|after:" + ",".join(
                    self._fmt(a) for a in list(args) + [kwargs[k] for k in sorted(kwargs)] if isinstance(a, torch.Tensor))
            self.lines.append(line)
            self._track(out, list(args) + list(kwargs.values()))
            return out
        return call

    def __getattr__(self, name):
        if name.startswith("__") or name in ("inner", "caps"):
            raise AttributeError(name)
        if name in self.caps:
            if not self.caps[name]:
                raise AttributeError(name)
            fn = getattr(self, "_" + name, None) or getattr(self.inner, name)
            return self._traced(name, fn)
        own = getattr(type(self), "_" + name, None)
        fn = own.__get__(self) if own is not None else getattr(self.inner, name)
        return self._traced(name, fn) if callable(fn) else fn

    # ---- capabilities the checker lacks, composed from its primitives ---------------------------------------------------
    def _bn_act_maxpool_fwd(self, pg, y, scale_shift, relu, keep):
        a = self.inner.bn_act_pool_fwd(PoolGeom(pg.N, pg.Di, pg.Hi, pg.Wi, pg.C), y, scale_shift, None, relu)
        return self.inner.maxpool_fwd(pg, a, keep)

    def _bn_act_gate_fwd(self, pg, y, scale_shift, relu, w, b, keep_act, pool=None, out=None, pool_idx=False):
        if not pool_idx:
            return self.inner.bn_act_gate_fwd(pg, y, scale_shift, relu, w, b, keep_act, pool=pool, out=out)
        assert self.gate_pool_keep and pool is not None and not keep_act and out is None
        a = self.inner.bn_act_pool_fwd(pg, y, scale_shift, None, relu)
        o, mean, gate = self.inner.gate_fwd(a, w, b)
        o, idx = self.inner.maxpool_fwd(pool, o, True)
        return o, None, mean, gate, idx

    def _bn_act_gate_pool_idx_ok(self, pool, y, scale_shift):
        return True

    # ---- what a fixture stores ---------------------------------------------------------------------------------------
    def summary(self):
        return {"lines": len(self.lines), "methods": dict(sorted(Counter(l.split("|", 1)[0] for l in self.lines).items())),
                "sha256": hashlib.sha256("\n".join(self.lines).encode()).hexdigest(), "peak_live_bytes": self.peak}


@contextlib.contextmanager
def tracing(be, **constants):
    """Install `be` as the op backend, log BranchStreams.run / side_task and the gradient hooks into it, and set the given
    module constants of rspnet_amd.engine (GATE_BWD_FUSED, GATE_POOL_APART) for the duration."""
    BS = engine.BranchStreams
    run0, task0, iter0 = BS.run, BS.side_task, engine.run_backward_iter

    def run(self, node, fn):
        be.log(f"run|{type(node).__name__}|{getattr(node, 'branch', 0)}")
        return run0(self, node, fn)

    def side_task(self, fn, keepalive, cost=0.0):
        be.log(f"side_task|{cost!r}|collected={BS.deferred is not None}")
        return task0(self, fn, keepalive, cost)

    def backward_iter(plan, ctx, dfeat, grad_of, after_param_grads=None, want_input_grad=False, packed=None):
        hook = after_param_grads
        if hook is not None:
            def hook(ni, grads_ready):
                be.log(f"hook|{ni}")
                return after_param_grads(ni, grads_ready)
        return iter0(plan, ctx, dfeat, grad_of, hook, want_input_grad, packed)

    saved = {k: getattr(engine, k) for k in constants}
    prev = ops.set_backend(be)
    BS.run, BS.side_task = run, side_task
    engine.run_backward_iter = split_wrapper.run_backward_iter = backward_iter
    for k, v in constants.items():
        setattr(engine, k, v)
    try:
        yield be
    finally:
        for k, v in saved.items():
            setattr(engine, k, v)
        engine.run_backward_iter = split_wrapper.run_backward_iter = iter0
        BS.run, BS.side_task = run0, task0
        ops.set_backend(prev)


# ---- the cases -------------------------------------------------------------------------------------------------------
def _np(d):
    return {k: (None if v is None else np.asarray(v.detach() if isinstance(v, torch.Tensor) else v)) for k, v in d.items()}


def _pretext(arch):
    """One golden pretext step: the query pass (kept) and the two key passes (not kept) through FlatEncoderPair."""
    from golden_util import build_inputs, cases_for, load_case
    from model_util import run_model_step
    a, _, seed = cases_for(arch, 1)[0]
    z, meta = load_case(a, 1, seed)
    _, inputs = build_inputs(a, meta)
    res, post, mom_post, grads = run_model_step(a, meta, inputs, 0, CPU, "fused")
    return {**{"out." + k: v for k, v in res.items()}, **{"grad." + k: v for k, v in grads.items()}}


def _pretext_lanes(arch, piece=4):
    """The same step as the operation list rspnet_amd/graph_step.py captures in "lanes" mode, issued eagerly, with the backward cut
    into pieces of `piece` plan nodes (as on a GPU whose weight-gradient lane has a hardware queue of its own): the second key pass
    reports its batch moments (run_forward's `deferred`), and the weight gradients are collected in BranchStreams.deferred."""
    from golden_util import build_inputs, cases_for, load_case
    from model_util import ReplayRNG, make_cfg
    from rspnet_amd.graph_step import GraphedPretextStep
    from rspnet_amd.moco import Loss, ModelFactory
    from rspnet_amd.optim import SGD
    a, _, seed = cases_for(arch, 1)[0]
    z, meta = load_case(a, 1, seed)
    _, (state, mom, clips, perms_B, sh) = build_inputs(a, meta)
    wrapped = ModelFactory(make_cfg(a, meta["K"], m=meta["m"], T=meta["T"])).build_moco_diffloss(device=CPU)
    model = wrapped.module
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    model.train()
    params = [p for p in wrapped.parameters() if p.requires_grad]
    names = {id(p): n for n, p in model.named_parameters()}
    opt = SGD(params, lr=meta["lr"], momentum=meta["sgd_momentum"], dampening=0.0, weight_decay=meta["weight_decay"], nesterov=False)
    stepper = GraphedPretextStep(wrapped, Loss(margin=meta["margin"], A=meta["A"], M=meta["M"]), opt)
    stepper._piece_agreed = piece
    im_q, im_k = torch.from_numpy(clips[0][0]), torch.from_numpy(clips[0][1])
    steps, box = stepper._schedule(im_q, im_k, "lanes")
    model._defer_reduce = model._defer_backward = True
    try:
        with ReplayRNG([perms_B[0], sh[0], sh[1]], meta["speed"]):
            host = model._host_part(im_q.shape[0], CPU)
            for op in steps:
                if op[0] in ("g", "e"):
                    if op[2] == "update":
                        grads = {"grad." + names[id(p)]: p.grad for p in params}
                    else:
                        op[3](host)
    finally:
        model._defer_reduce = model._defer_backward = False
    loss, loss_A, loss_M, out, rl = box["outs"]
    return _np({"out.loss": loss, "out.logits1": out[0], "out.logits2": out[1], **grads})


def _finetune(arch, mode, be):
    """MultiTaskWrapper(finetune=True).  train: eval-mode forward only, then a train-mode forward and backward.  frozen: eval-mode
    forward and backward (frozen BatchNorm); frozen_affine: the same with BatchNorm's weight / bias frozen."""
    import finetune_util as FT
    import frozen_bn_util as FB
    if mode == "train":
        z, meta, _, state, x = FT.load(arch)
    else:
        z, meta, state, x = FB.load(arch)
    model = FT.build_model(arch, meta["classes"], state, CPU)
    xt, tt = torch.from_numpy(x), torch.from_numpy(z["target"])
    out = {}
    if mode == "train":
        model.eval()
        with torch.no_grad():
            out["out.logits_eval"] = model(xt)
        model.train()
    elif mode == "frozen_affine":
        from rspnet_amd.models import ModelFactory
        cfg = {"model": {"arch": arch}, "dataset": {"num_classes": meta["classes"]}, "freeze_bn": True, "freeze_bn_affine": True}
        model = ModelFactory(cfg)._post_process_model(model)
        model.train()
    else:
        model.eval()
    logits = model(xt)
    loss = nn.CrossEntropyLoss()(logits, tt)
    try:
        loss.backward()
    except RuntimeError as e:
        be.log(f"raised|RuntimeError|{e}")
    out["out.logits"] = logits
    out.update({"grad." + n: p.grad for n, p in model.named_parameters()})
    return _np(out)


def _run_plan(plan, packed, x, params, be, keep_free=True, want_input_grad=False, training=True):
    """Forward (kept) and backward of a plan with a gradient hook and stand-alone gradient tensors; then a forward that keeps
    nothing."""
    out, ctx = engine.run_forward(plan, x, packed, keep=True, training=training)
    gen = torch.Generator().manual_seed(7)
    dout = torch.randn(out.shape, generator=gen)
    grads = {id(p): torch.full_like(p, float("nan")) for p in params.values()}
    dx = engine.run_backward(plan, ctx, dout, lambda p: grads[id(p)], lambda ni, ready: None, want_input_grad=want_input_grad)
    res = {"out.kept": out, "out.dx": dx, **{"grad." + n: grads[id(p)] for n, p in params.items()}}
    if keep_free:
        res["out.free"], none = engine.run_forward(plan, x, packed, keep=False, training=training)
        assert none is None
    return _np(res)


def _gate_unit(be):
    """ConvBN -> Gate -> Pool (a front-end unit of S3D-G) and ConvBN -> Gate into a concat slice beside a Pool branch."""
    gen = torch.manual_seed(11)
    c1, c2 = nn.Conv3d(4, 8, (1, 3, 3), 1, (0, 1, 1), bias=False), nn.Conv3d(8, 8, (3, 1, 1), 1, (1, 0, 0), bias=False)
    b1, b2 = nn.BatchNorm3d(8), nn.BatchNorm3d(8)
    g1, g2 = nn.Conv3d(8, 8, 1), nn.Conv3d(8, 8, 1)
    nodes = [engine.ConvBN(c1, b1, 0, 1, (1, 3, 3), (1, 1, 1), (0, 1, 1)), engine.Gate(g1, 1, 2),
             engine.Pool(2, 3, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
             engine.ConvBN(c2, b2, 3, 4, (3, 1, 1), (1, 1, 1), (1, 0, 0)), engine.Gate(g2, 4, 5, into=(6, 0, 16)),
             engine.Pool(3, 7, (3, 3, 3), (1, 1, 1), (1, 1, 1), branch=1),
             engine.ConvBN(nn.Conv3d(8, 8, 1, bias=False), nn.BatchNorm3d(8), 7, 8, (1, 1, 1), into=(6, 8, 16), branch=1)]
    plan = engine.Plan(nodes, 0, 6)
    params = {}
    for i, n in enumerate(nodes):
        for part in ("conv", "bn"):
            for pn, p in (getattr(n, part).named_parameters() if hasattr(n, part) else ()):
                params[f"{i}.{part}.{pn}"] = p
    x = torch.randn(2, 2, 8, 8, 4)
    return _run_plan(plan, engine.PackedWeights(), x, params, be, want_input_grad=True)


def _s3dg_flat_plan(be):
    """S3D-G's plan on the flat parameters of a pretext model (every group runs as one GEMM) with gradient tensors that are NOT
    adjacent (the group's weight gradient goes through a temporary), a gradient hook, and the smallest clip the plan accepts."""
    from model_util import make_cfg
    from rspnet_amd.moco import ModelFactory
    torch.manual_seed(5)
    model = ModelFactory(make_cfg("s3dg", 64)).build_moco_diffloss(device=CPU).module
    model._prepare()                                      # the flat parameter buffers: sibling filters back to back
    enc = model.encoder_q
    params = {n: p for n, p in enc.encoder.named_parameters()}
    x = torch.zeros(2, 8, 32, 32, 4)
    x[..., :3] = torch.randn(2, 8, 32, 32, 3)
    return _run_plan(enc.plan(), enc._packed, x, params, be, keep_free=False)


def _vstem_pad_unit(be):
    """The spatial half of R(2+1)D's stem on virtual pixels, with its odd mid-channel count padded (tests/virtual_stem_util.py)."""
    torch.manual_seed(17)
    conv, bn = nn.Conv3d(3, 45, (1, 7, 7), (1, 2, 2), (0, 3, 3), bias=False), nn.BatchNorm3d(45)
    node = engine.ConvBN(conv, bn, 0, 1, (1, 7, 7), (1, 2, 2), (0, 3, 3), cout_pad=48, virtual_w=True)
    x = torch.zeros(2, 3, 12, 24, 4)
    x[..., :3] = torch.randn(2, 3, 12, 24, 3)
    params = {"conv.weight": conv.weight, "bn.weight": bn.weight, "bn.bias": bn.bias}
    return _run_plan(engine.Plan([node], 0, 1), engine.PackedWeights(), x, params, be)


def _frozen_unit(be):
    """One eval-mode ConvBN with a conv bias and channel padding, a residual unit behind it: both exits of the eval-mode
    backward's padding and bias code."""
    torch.manual_seed(13)
    c1, c2 = nn.Conv3d(4, 6, 3, 1, 1, bias=True), nn.Conv3d(8, 6, 1, bias=False)
    b1, b2 = nn.BatchNorm3d(6), nn.BatchNorm3d(6)
    for b in (b1, b2):
        b.running_mean.normal_()
        b.running_var.uniform_(0.5, 1.5)
    c3, b3 = nn.Conv3d(6, 6, 1, bias=False), nn.BatchNorm3d(6)
    nodes = [engine.ConvBN(c1, b1, 0, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), cout_pad=8),
             engine.ConvBN(c2, b2, 1, 2, (1, 1, 1)),
             engine.ConvBN(c3, b3, 2, 3, (1, 1, 1), residual=2)]
    params = {f"{i}.{part}.{pn}": p for i, n in enumerate(nodes) for part in ("conv", "bn")
              for pn, p in getattr(n, part).named_parameters()}
    return _run_plan(engine.Plan(nodes, 0, 3), engine.PackedWeights(), torch.randn(2, 2, 4, 4, 4), params, be, training=False)


# name -> (backend flags, engine constants, function of the backend, the branches the case is there for)
CASES = {
    "pretext:resnet18": ({}, {}, lambda be: _pretext("resnet18"),
                         ["virtual_stem", "residual", "stem_pool_free", "stem_pool_kept_fused"]),
    "pretext:resnet18:no_maxpool_op": ({"maxpool_fused": False}, {}, lambda be: _pretext("resnet18"), ["stem_pool_kept_apart"]),
    "pretext:r2plus1d": ({}, {}, lambda be: _pretext("r2plus1d-vcop"), ["cout_pad"]),
    "plan:vstem_pad": ({}, {}, _vstem_pad_unit, ["cout_pad", "virtual_stem", "hook"]),
    "pretext:s3dg": ({"gate_pool_keep": True}, {}, lambda be: _pretext("s3dg"),
                     ["group_gemm", "gate_fused", "gate_pool_free", "gate_pool_kept", "into_slice", "pool_node"]),
    "pretext:c3d:conv": ({}, {}, lambda be: _pretext("c3d:conv"), ["train", "conv_bias_train", "convbias", "input_grad"]),
    "pretext:c3d:convbn": ({}, {}, lambda be: _pretext("c3d:convbn"), ["input_grad"]),
    "pretext:c3d:lanes": ({}, {}, lambda be: _pretext_lanes("c3d"), ["deferred_stats", "tasks_collected"]),
    "plan:s3dg:flat": ({}, {}, _s3dg_flat_plan, ["group_gemm", "group_grads_apart", "hook"]),
    "plan:gate": ({"gate_pool_keep": True}, {}, _gate_unit, ["gate_fused", "gate_pool_kept", "hook", "input_grad"]),
    "plan:gate:no_pool_keep": ({}, {}, _gate_unit, ["gate_pool_not_kept"]),
    "plan:gate:pool_apart": ({"gate_pool_keep": True}, {"GATE_POOL_APART": True}, _gate_unit, ["gate_pool_not_kept"]),
    "plan:gate:bwd_unfused": ({"gate_pool_keep": True}, {"GATE_BWD_FUSED": False}, _gate_unit, ["gate_bwd_unfused"]),
    "plan:frozen_unit": ({}, {}, _frozen_unit, ["eval_backward", "eval_pad", "eval_conv_bias", "residual"]),
    "finetune:c3d": ({}, {}, lambda be: _finetune("c3d", "train", be), ["train", "eval_forward"]),
    "finetune:s3dg": ({}, {}, lambda be: _finetune("s3dg", "train", be), ["group_members", "gate_node", "eval_forward"]),
    "frozen:c3d": ({}, {}, lambda be: _finetune("c3d", "frozen", be), ["eval_backward", "eval_conv_bias"]),
    "frozen:c3d:affine": ({}, {}, lambda be: _finetune("c3d", "frozen_affine", be), ["eval_frozen_affine", "eval_conv_bias"]),
    "frozen:r2plus1d": ({}, {}, lambda be: _finetune("r2plus1d-vcop", "frozen", be), ["eval_backward", "eval_pad"]),
    "frozen:s3dg": ({}, {}, lambda be: _finetune("s3dg", "frozen", be), ["eval_backward", "gate_node", "group_members"]),
    "frozen:c3d:no_op": ({"eval_bwd": False}, {}, lambda be: _finetune("c3d", "frozen", be), ["eval_backward_missing"]),
}


def _has(lines, *needles):
    return any(all(n in l for n in needles) for l in lines)


def _calls(lines, name):
    return [l.split("|") for l in lines if l.startswith(name + "|")]


def _dims(t):
    """Shape of a tensor as TraceOps._fmt wrote it."""
    return [int(v) for v in t.split("/")[0][2:-1].split(",") if v.strip()]


# branch -> evidence in the trace that the executor took it
BRANCHES = {
    "train": lambda L: _has(L, "bn_finalize|") and _has(L, "conv_wgrad|"),
    "conv_bias_train": lambda L: any(l.startswith("conv_fwd|") and l.split("|")[4].startswith("T") and l.split("|")[5] == "True" for l in L),
    "virtual_stem": lambda L: _has(L, "conv_fwd|", "out_ld="),
    "residual": lambda L: any(l.startswith("bn_act_pool_bwd|") and l.split("|")[9] == "True" for l in L)
    or any(l.startswith("bn_eval_act_pool_bwd|") and l.split("|")[8] == "True" for l in L),
    "stem_pool_free": lambda L: any(l.startswith("bn_act_pool_fwd|") and "(1, 1, 1))" in l.split("|")[1] and "(3, 3, 3)" in l.split("|")[1] for l in L),
    "stem_pool_kept_fused": lambda L: _has(L, "bn_act_maxpool_fwd|"),
    "stem_pool_kept_apart": lambda L: not _has(L, "bn_act_maxpool_fwd|") and _has(L, "maxpool_fwd|", "|True"),
    "cout_pad": lambda L: any(_dims(c[1])[1] != _dims(c[4])[0] for c in _calls(L, "bn_finalize")),
    "group_gemm": lambda L: any(l.startswith("bn_act_pool_bwd|") and "dy_out=T" in l for l in L),
    "group_members": lambda L: _has(L, "run|ConvBNGroup") and not any(l.startswith("bn_act_pool_bwd|") and "dy_out=T" in l for l in L),
    "group_grads_apart": lambda L: any(l.startswith("bn_act_pool_bwd|") and "dy_out=T" in l for l in L),
    "gate_fused": lambda L: _has(L, "bn_act_gate_fwd|") and _has(L, "bn_act_gate_bwd|"),
    "gate_pool_free": lambda L: _has(L, "bn_act_gate_fwd|", "|False|", "pool=PG"),
    "gate_pool_kept": lambda L: _has(L, "bn_act_gate_fwd|", "pool_idx=True"),
    "gate_pool_not_kept": lambda L: not _has(L, "pool_idx=True") and _has(L, "bn_act_gate_fwd|", "pool=None") and _has(L, "maxpool_fwd|"),
    "gate_bwd_unfused": lambda L: _has(L, "bn_act_gate_fwd|", "|True|out=") and _has(L, "gate_bwd|") and not _has(L, "bn_act_gate_bwd|"),
    "gate_node": lambda L: _has(L, "gate_fwd|") and _has(L, "gate_bwd|"),
    "pool_node": lambda L: _has(L, "maxpool_fwd|") and _has(L, "maxpool_bwd|"),
    "into_slice": lambda L: _has(L, "bn_act_pool_fwd|", "out=T") and _has(L, "bn_act_gate_fwd|", "out=T"),
    "convbias": lambda L: _has(L, "eltwise|'relu_bwd'"),
    "input_grad": lambda L: sum(l.startswith("conv_dgrad_packed|") for l in L) >= sum(l.startswith("conv_wgrad|") for l in L) - 1,
    "deferred_stats": lambda L: _has(L, "bn_finalize|", "batch_stats_out=T"),
    "tasks_collected": lambda L: _has(L, "side_task|", "collected=True"),
    "hook": lambda L: _has(L, "hook|"),
    "eval_forward": lambda L: _has(L, "conv_fwd|", "|None|False"),
    "eval_backward": lambda L: _has(L, "bn_eval_act_pool_bwd|"),
    "eval_pad": lambda L: any(c[9].startswith("T") and _dims(c[2])[-1] != _dims(c[9])[0] for c in _calls(L, "bn_eval_act_pool_bwd")),
    "eval_conv_bias": lambda L: _has(L, "bn_eval_act_pool_bwd|"),
    "eval_frozen_affine": lambda L: any(l.startswith("bn_eval_act_pool_bwd|") and l.split("|")[9] == "None" for l in L),
    "eval_backward_missing": lambda L: _has(L, "raised|RuntimeError|" + engine.EVAL_BACKWARD_MISSING),
}


def run_case(name, values=False):
    """-> (TraceOps after the run, {result name: array | None}, the branches the case reached)."""
    flags, constants, fn, claims = CASES[name]
    be = TraceOps(values=values, **flags)
    torch.manual_seed(0)
    with tracing(be, **constants):
        results = fn(be)
    reached = [b for b in claims if BRANCHES[b](be.lines)]
    return be, results, reached
