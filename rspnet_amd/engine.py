"""Plan executor: runs a backbone's layer plan forward/backward through the HIP ops.

A backbone (rspnet_amd/models/*) is an ``nn.Module`` tree that only *holds* parameters under the reference's
state-dict names; its ``plan()`` lists fused units over numbered tensor slots:

  ConvBN      conv3d → BatchNorm3d [→ + residual] [→ ReLU] [→ disjoint MaxPool3d]             (all four backbones)
  ConvBNGroup ConvBN units that read one tensor with one geometry: one GEMM over their filters   (S3D-G inception siblings)
  ConvBias    conv3d + bias [→ ReLU], no BatchNorm                                              ('conv' projection head)
  Pool        stand-alone MaxPool3d with overlapping windows                                    (ResNet stem, S3D-G)
  Gate        S3D-G self-gating  x * sigmoid(W·mean(x) + b)
A channel concat (S3D-G inception) is no node: the branches' last units write channel slices of one tensor (`into`).

Forward keeps, per ConvBN, only the conv input, the raw conv output y and the per-channel (mean, invstd, scale,
shift); the activation / ReLU mask / pool arg-max are recomputed from y in backward.
Activations are (N, D, H, W, C) tensors.
"""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import torch
from torch import nn

from . import ops as _ops
from .ops import ConvGeom, PoolGeom

Triple = Tuple[int, int, int]


@dataclass
class ConvBN:
    conv: nn.Module                 # holds .weight (Cout,Cin,kT,kH,kW) [, .bias]
    bn: nn.Module                   # holds weight/bias/running_mean/running_var/num_batches_tracked, .eps, .momentum
    src: int
    dst: int
    k: Triple
    s: Triple = (1, 1, 1)
    p: Triple = (0, 0, 0)
    relu: bool = True
    pool: Optional[Tuple[Triple, Triple]] = None   # (kernel, stride), disjoint windows only
    residual: Optional[int] = None                 # slot added before the ReLU
    into: Optional[Tuple[int, int, int]] = None    # (concat slot, channel offset, total channels): write a slice
    branch: int = 0                                # > 0: node of a side branch that may run beside its siblings (BranchStreams)
    virtual_w: bool = False                        # 3-channel stem with W stride 2: run on "virtual pixels" (VirtualStem)
    cout_pad: int = 0                              # run with Cout zero-padded to this many channels (0: as is).  R(2+1)D's
    #   mid-channel counts (83, 230, 921 ...) are not multiples of 4; padded, this conv's output and the next conv's input are
    #   16-byte rows and both take the LDS-DMA kernels instead of the scalar gather.  Pad channels carry zero weights and
    #   gamma = beta = 0, so they are exactly 0 after BN+ReLU and contribute nothing downstream; their gradients are dropped.


@dataclass
class ConvBNGroup:
    """ConvBN units that read the SAME tensor with the same geometry (S3D-G's inception siblings branch0 / branch1.0 /
    branch2.0, models/s3dg.py:80-88): when their filters sit back to back in memory (rspnet_amd/flat.py `adjacent`) they run
    as ONE convolution over the concatenated filters — one GEMM instead of three in forward, one dgrad whose K runs over all
    members (the fan-out sum of their input gradients comes out of the GEMM, no adds) and one wgrad in backward.  BatchNorm
    stays per member (channel slices of the shared conv output / statistics).  With any other parameter layout (fine-tune
    path, stand-alone use) the members simply run one by one."""
    members: List[ConvBN]
    cat: Optional["_CatConv"] = field(default=None, repr=False, compare=False)      # what PackedWeights keys on: holds the concatenated filters


@dataclass
class ConvBias:
    """nn.Conv3d(bias=True) [+ ReLU] without BatchNorm: the two convs of ConvFc (moco/split_wrapper.py:18-39)."""
    conv: nn.Module
    src: int
    dst: int
    k: Triple
    s: Triple = (1, 1, 1)
    p: Triple = (0, 0, 0)
    relu: bool = False


@dataclass
class Pool:
    """Stand-alone MaxPool3d (overlapping / padded windows allowed)."""
    src: int
    dst: int
    k: Triple
    s: Triple
    p: Triple = (0, 0, 0)
    branch: int = 0


@dataclass
class Gate:
    """S3D-G self-gating: x * sigmoid(conv1x1x1(mean(x)))   (models/s3dg.py:63-72)."""
    conv: nn.Module                                # excitation: weight (C,C,1,1,1), bias (C)
    src: int
    dst: int
    into: Optional[Tuple[int, int, int]] = None
    branch: int = 0


@dataclass
class Plan:
    nodes: List[object]
    input_slot: int = 0
    output_slot: int = 0
    gate_fusion: Optional[dict] = field(default=None, repr=False, compare=False)      # cached tables of _gate_fusion /
    pool_fusion: Optional[dict] = field(default=None, repr=False, compare=False)      # _pool_fusion, built at the first use


@dataclass
class _Saved:
    x: torch.Tensor
    y: torch.Tensor
    mi: torch.Tensor
    ss: torch.Tensor
    cg: ConvGeom
    pg: PoolGeom
    res: Optional[torch.Tensor] = None
    eval_mode: bool = False                        # BatchNorm ran on its running statistics: mi is _eval_mean_invstd's
    gate: Optional["_SavedGate"] = None            # the self-gating unit fused behind this BatchNorm (_gate_fusion): one backward op
    y_sel: Optional[torch.Tensor] = None           # pooled unit: y at each window's selected position (ops.bn_act_pool_sel_fwd)


# What the other node kinds' backwards need, one record type per kind (ForwardCtx.saved).  _SavedVStem: a ConvBN that ran as two
# convolutions over virtual pixels (VirtualStem); _SavedGroup: a ConvBNGroup that ran as ONE GEMM — `per` holds, per member, its
# channel slice [off, off + C) of the shared convolution output and its BatchNorm vectors (a group whose members ran one by one keeps
# a _Saved per member, keyed (index, j)); _SavedGate: `at` = plan index of the Gate node, `x` = what the gate multiplied — None when it
# ran fused behind a ConvBN (_gate_fusion): that ConvBN's _Saved.gate is this record too, and its backward recomputes the activation
_SavedVStem = NamedTuple("_SavedVStem", [("x_e", torch.Tensor), ("x_o", torch.Tensor), ("y", torch.Tensor), ("mi", torch.Tensor),
                                         ("ss", torch.Tensor), ("cg", ConvGeom), ("pg", PoolGeom), ("vs", "VirtualStem")])
_SavedMember = NamedTuple("_SavedMember", [("off", int), ("C", int), ("mi", torch.Tensor), ("ss", torch.Tensor), ("pg", PoolGeom)])
_SavedGroup = NamedTuple("_SavedGroup", [("x", torch.Tensor), ("y", torch.Tensor), ("cg", ConvGeom), ("per", List[_SavedMember])])
_SavedPool = NamedTuple("_SavedPool", [("pg", PoolGeom), ("idx", torch.Tensor)])      # idx: arg-max
_SavedGate = NamedTuple("_SavedGate", [("at", int), ("x", Optional[torch.Tensor]), ("mean", torch.Tensor), ("gate", torch.Tensor)])
_SavedConvBias = NamedTuple("_SavedConvBias", [("x", torch.Tensor), ("y", torch.Tensor), ("cg", ConvGeom)])
SavedState = Union[_Saved, _SavedVStem, _SavedGroup, _SavedPool, _SavedGate, _SavedConvBias]


@dataclass
class ForwardCtx:
    # plan index (or (group index, member) where a group ran its members one by one) -> what that node's backward needs
    saved: Dict[Union[int, Tuple[int, int]], SavedState] = field(default_factory=dict)
    feat_shape: Optional[Tuple[int, ...]] = None
    packed: Optional["PackedWeights"] = None       # the encoder's weight cache (dgrad layouts are fetched from it in backward)
    head: object = None                            # the projection heads' saved state (moco/split_wrapper.py)


class PackedWeights:
    """Packed copies of one encoder's convolution weights: the forward layout of every conv and, for convs whose input needs
    a gradient, the dgrad layouts.  The weights change once per step, so all copies are rebuilt together by ONE batched launch
    (ops.PackSet) the first time one of them is needed after `invalidate()`; channel padding (3 -> 4 channel stems, R(2+1)D's
    odd mid-channel counts) is applied by the re-pack itself.  A conv seen for the first time is packed on its own and joins
    the batch at the next rebuild."""

    def __init__(self):
        self._entries = []        # (geometry, which, conv module): ONE per distinct packed layout of a conv
        self._index = {}          # (id(conv), which, layout signature) -> (set number, position)
        self._sets = []
        self._ptrs = []
        self._dirty = True
        self._virtual = {}        # id(conv) -> VirtualStem: derived filters that are re-gathered before every re-pack

    def invalidate(self):
        self._dirty = True

    def refresh_now(self):
        """Re-pack on the CURRENT stream if the weights changed: for callers that are about to use the copies from several
        streams (two passes through one encoder side by side) and need the re-pack ordered before the fork."""
        if self._dirty and self._entries:
            self._refresh()

    def _refresh(self):
        be = _ops.backend()
        for vs in self._virtual.values():
            vs.refresh()
        ptrs = [c.weight.data_ptr() for _, _, c in self._entries]
        if len(self._sets) > 1 or ptrs != self._ptrs:      # new members since the last rebuild, or the parameters moved
            self._sets = [be.pack_set([(g, which, c.weight.data) for g, which, c in self._entries])] if self._entries else []
            self._index = {(id(c), which, be.pack_signature(g, which, c.weight.data)): (0, i)
                           for i, (g, which, c) in enumerate(self._entries)}
            self._ptrs = ptrs
        for ps in self._sets:
            ps.run()
        self._dirty = False

    def _lookup(self, conv, cg: ConvGeom, which: int):
        if self._dirty:
            self._refresh()
        # the packed layout depends on channels / kernel / stride / padding / stem applicability only: every input geometry a
        # conv is applied to (diff_speed's T_real values, a partial last batch, eval sizes) shares one packed copy
        key = (id(conv), which, _ops.backend().pack_signature(cg, which, conv.weight.data))
        at = self._index.get(key)
        if at is None:
            ps = _ops.backend().pack_set([(cg, which, conv.weight.data)])
            ps.run()
            self._sets.append(ps)
            self._entries.append((cg, which, conv))
            self._ptrs.append(conv.weight.data_ptr())
            at = self._index[key] = (len(self._sets) - 1, 0)
        return self._sets[at[0]].packed[at[1]]

    def get(self, conv, cg: ConvGeom):
        """conv: whatever holds `.weight` — a conv module, a group's _CatConv, a VirtualStem holder."""
        return self._lookup(conv, cg, 0)

    def get_dgrad(self, conv, cg: ConvGeom):
        return self._lookup(conv, cg, 1)

    def virtual_stem(self, node) -> "VirtualStem":
        vs = self._virtual.get(id(node.conv))
        if vs is None or vs.device != node.conv.weight.device:
            vs = self._virtual[id(node.conv)] = VirtualStem(node)
        return vs


class _CatConv:
    """Stands in for a conv module where the engine / PackedWeights expect `.weight`: the concatenated filters of a group."""
    weight: torch.Tensor = None


def _adjacent_cat(ts):
    """If the tensors sit back to back in one storage (flat parameter / gradient buffers, rspnet_amd/flat.py), the single
    tensor that covers them — dim 0 concatenated — else None."""
    t0 = ts[0]
    if not all(t.is_contiguous() and t.shape[1:] == t0.shape[1:] and t.dtype == t0.dtype for t in ts):
        return None
    end = t0.data_ptr() + t0.numel() * t0.element_size()
    for t in ts[1:]:
        if t.data_ptr() != end or t.untyped_storage().data_ptr() != t0.untyped_storage().data_ptr():
            return None
        end += t.numel() * t.element_size()
    shape = (sum(t.shape[0] for t in ts),) + tuple(t0.shape[1:])
    stride = tuple(t0.stride())
    return torch.as_strided(t0, shape, stride, t0.storage_offset())


INPUT_CHANNEL_PAD = 4
GATE_BWD_FUSED = not os.environ.get("RSP_NO_GATE_BWD_FUSION")      # (A/B switch for measurements)
# (A/B switches) key passes: conv1 leaves its stem kernel pooled (_Forward.stem_pooled); query pass: pooled units keep y at the
# selected positions and the BatchNorm backward's reduce reads that instead of y (_Forward.bn_apply)
STEM_POOLED = not os.environ.get("RSP_NO_STEM_POOLED")
BN_BWD_SEL = not os.environ.get("RSP_NO_BN_BWD_SEL")


class VirtualStem:
    """A 3-channel stem convolution with kernel width 7 and stride 2 along W (R3D-18's 7x7x7 conv1, models/resnet.py:124; the
    (1,7,7) spatial half of R(2+1)D's conv1, models/r2plus1d_vcop.py:57) without the zero fourth channel.

    The implicit-GEMM kernel wants 16-byte pixels, so the clip is gathered with its 3 channels padded to 4 and a quarter of the
    matrix work multiplies zeros.  But an output column wo reads 7 pixels = 21 CONTIGUOUS floats of a packed 3-channel row, starting
    at float 6 wo - 9; seen as 16-byte "virtual pixels" (4 floats, 84 per 112-pixel row) that window starts 3 floats into virtual
    pixel 3g - 3 for wo = 2g and 1 float into virtual pixel 3g - 1 for wo = 2g + 1.  Each parity of wo is therefore an ORDINARY
    convolution over the virtual row — kernel width 6, stride 3, 4 "channels", its own weight tensor with the 21 real values shifted
    by 3 (even) or 1 (odd) floats inside the 24 — and writes every second output column (channel pitch 2 Cout).  K per output drops
    from 7 * 4 = 28 to 24 floats per kernel row: 14 % less matrix work on the layer that is a third of R3D-18's step.
    The packed row carries 3 zero virtual pixels on the left and 2 on the right, so both parities run without padding along W
    (the odd one from a base address 2 virtual pixels in) and the output-size formula gives exactly Wo / 2 columns."""

    def __init__(self, node):
        self.conv = node.conv
        w = node.conv.weight
        Cout, cin, kT, kH, kW = w.shape
        assert cin == 3 and kW == 7 and node.s[2] == 2 and node.p[2] == 3
        self.holders, self.idx, self.src, self.dst = [], [], [], []
        co = torch.arange(Cout).view(Cout, 1, 1, 1, 1)
        c4 = torch.arange(4).view(1, 4, 1, 1, 1)
        kt = torch.arange(kT).view(1, 1, kT, 1, 1)
        kh = torch.arange(kH).view(1, 1, 1, kH, 1)
        j = torch.arange(6).view(1, 1, 1, 1, 6)
        for off in (3, 1):                               # even wo, odd wo
            r = 4 * j + c4 - off                         # float inside the 21-float window
            valid = ((r >= 0) & (r < 21)).expand(Cout, 4, kT, kH, 6)
            real = ((((co * 3 + r % 3) * kT + kt) * kH + kh) * 7 + torch.div(r, 3, rounding_mode="floor")).expand(Cout, 4, kT, kH, 6)
            idx = torch.where(valid, real, torch.full_like(real, w.numel())).reshape(-1)      # sentinel -> the appended zero
            flat_valid = valid.reshape(-1).nonzero().view(-1)
            self.idx.append(idx.to(w.device))
            self.src.append(flat_valid.to(w.device))
            self.dst.append(real.reshape(-1)[flat_valid].to(w.device))
            h = _CatConv()
            h.weight = torch.zeros((Cout, 4, kT, kH, 6), dtype=w.dtype, device=w.device)
            self.holders.append(h)
        self.device = w.device
        self.refresh()

    enabled = not os.environ.get("RSP_NO_VIRTUAL_STEM")      # (A/B switch for measurements)

    @staticmethod
    def applies(node, xin) -> bool:
        w = node.conv.weight
        W = xin.shape[3]
        return (VirtualStem.enabled and node.virtual_w and w.shape[1] == 3 and xin.shape[4] == 4 and w.shape[4] == 7 and node.s[2] == 2 and node.p[2] == 3
                and (3 * W) % 4 == 0 and W % 2 == 0 and getattr(node.conv, "bias", None) is None and node.residual is None
                and node.into is None)

    def refresh(self):
        """class weights <- current parameter values (two gathers of 8/7 the filter size), called by PackedWeights ahead of every
        re-pack: the pack set then lays them out with the rest"""
        w = self.conv.weight
        ext = torch.cat([w.data.reshape(-1), w.data.new_zeros(1)])
        for h, idx in zip(self.holders, self.idx):
            torch.index_select(ext, 0, idx, out=h.weight.view(-1))

    def pack_rows(self, xin):
        """(N,D,H,W,4) clip with a zero 4th channel -> packed 3-channel rows as virtual pixels: (N,D,H,Wv+5,4) for the even outputs and
        the same memory from 2 virtual pixels in for the odd ones."""
        N, D, H, W, _ = xin.shape
        Wp = 3 * W // 4 + 5
        flat = torch.zeros(N * D * H * Wp * 4 + 8, dtype=xin.dtype, device=xin.device)
        xv = flat[:N * D * H * Wp * 4].view(N, D, H, Wp, 4)
        xv.view(N, D, H, Wp * 4)[..., 12:12 + 3 * W].view(N, D, H, W, 3).copy_(xin[..., :3])
        return xv, torch.as_strided(flat, (N, D, H, Wp, 4), xv.stride(), 8)


class BranchStreams:
    """Side branches of a block (S3D-G's inception branches 1-3, models/s3dg.py:80-99) on their own HIP streams — while the step is
    being CAPTURED into a HIP graph (rspnet_amd/graph_step.py).  The late blocks launch a few dozen workgroups per kernel; as
    graph nodes without a common stream order four of them run side by side (tools/stream_overlap_probe.py: x1.14-1.31 on one
    block).  Issued eagerly the same forks gain nothing (x1.0: the host feeds one kernel at a time), so outside a capture
    every node stays on the caller's stream.

    Forks are FLAT: only the stream the capture began on (`origin`) forks, and everything joins back into it.  ROCm 7.2's
    hipStreamEndCapture dies with a segmentation fault on a stream forked from a forked stream (tools/graph_nest_probe.py), so a
    pass that itself runs on a side stream (the query forward beside the key passes) keeps its branches in line.

    Ordering: a side stream first waits for the trunk (its inputs — and every earlier reader of memory its allocator pool may
    recycle — are complete), the trunk waits for all side streams when the next trunk node comes up; a tensor produced on a
    side stream is consumed there or, after that join, on the trunk."""
    _streams: Dict[Tuple, "torch.cuda.Stream"] = {}
    origin = None          # raw handle of the capturing stream, set by GraphedPretextStep around the capture
    SMALL_WGRAD_FLOPS = float(os.environ.get("RSP_WGRAD_ASIDE_GFLOP", "50")) * 1e9      # weight gradients below this size run beside the input gradient (side_task); swept 50 / 120 /
    #   300 / 1000 GFLOP: larger ones compete with the input gradient for the matrix pipe (R(2+1)D 77.9 -> 80.2 ms at 300)

    # ... and mid-sized ones whose operands are small enough not to fight the input gradient for HBM: since tiles differ in length
    #  a second matrix kernel fills the ragged ends of the launches — C3D 93.7 -> 92.9 ms with conv3a / conv4 included;
    # R(2+1)D's 266-GFLOP weight gradients stream 1.3 GB each and stay in line (77.9 -> 80.2 ms beside the input gradient)
    MID_WGRAD_FLOPS = float(os.environ.get("RSP_WGRAD_MID_GFLOP", "400")) * 1e9
    MID_WGRAD_BYTES = float(os.environ.get("RSP_WGRAD_MID_MB", "450")) * 1e6
    EAGER_TASKS = not os.environ.get("RSP_NO_EAGER_OVERLAP")
    # Issued eagerly, a weight gradient below AHEAD_MAX_FLOPS is handed to the task lane WITHOUT joining the previous one first (the
    # lane keeps its own order; what the tasks read stays alive until the join): the trunk no longer stalls where a weight gradient
    # outlasts the trunk's work up to the next one.  profiles/r06/experiments_r6.txt r6u-v: R3D-18 1 321-1 326 -> 1 344-1 346 clips/s,
    # R(2+1)D 446.3 -> 448.3-450.3, C3D 352.7-353.3 -> 353.6-354.7; without the cap C3D loses 0.5 % (its 177-355 GFLOP weight gradients
    # queue up beside the input gradients and fight them for the whole backward instead of filling their ragged ends).
    RUN_AHEAD = bool(int(os.environ.get("RSP_TASK_RUN_AHEAD", "1")))
    AHEAD_MAX_FLOPS = float(os.environ.get("RSP_TASK_AHEAD_MAX_GFLOP", "100")) * 1e9
    # a list while rspnet_amd/graph_step.py captures a piece of the backward as a LINEAR graph: side tasks are not run but collected
    # there as (fn, keepalive, FLOPs) — the stepper captures them as a graph of their own and replays it on the weight-gradient lane
    deferred = None

    def __init__(self, x: torch.Tensor):
        self.dev = x.device
        self.on = bool(x.is_cuda and _ops.backend().name == "hip" and BranchStreams.origin is not None
                       and torch.cuda.is_current_stream_capturing()
                       and torch.cuda.current_stream(self.dev).cuda_stream == BranchStreams.origin)
        self.origin_h = BranchStreams.origin
        # Inception branches as parallel graph branches: x1.14-1.31 on a block of its own and 51 -> 47 ms per S3D-G step when they were
        # the only concurrency in the graph; with the three forward passes and the weight gradients on streams of their own the
        # machine is already fed and the extra forks cost more in joins than they fill (41.6 -> 40.1 ms without them): off,
        # RSP_BRANCH_FORKS=1 brings them back
        self.fork_branches = self.on and bool(os.environ.get("RSP_BRANCH_FORKS"))
        # issued eagerly, the weight-gradient side task still pays (the host is far ahead of those kernels); the inception branches
        # do not (x1.00: dozens of tiny launches, the host feeds one at a time) and stay in line
        if (not self.on and BranchStreams.EAGER_TASKS and x.is_cuda and _ops.backend().name == "hip"
                and not torch.cuda.is_current_stream_capturing()):
            self.on = True
            self.origin_h = torch.cuda.current_stream(self.dev).cuda_stream
            # (measured: S3D-G issued eagerly 394 clips/s with the branches in line, 355-358 forked)
        self.active: Dict[int, "torch.cuda.Stream"] = {}
        self.task = None       # (task stream, tensors its kernels still read) of the outstanding side task

    def _get(self, key):
        key = (self.dev.index if self.dev.index is not None else torch.cuda.current_device(), key)
        st = BranchStreams._streams.get(key)
        if st is None:
            # the weight-gradient side task shares the process's "w" lane: one of three streams MEASURED to overlap with the
            # main stream and with one another (rspnet_amd/streams.py: HIP multiplexes streams onto a few hardware queues)
            if key[1] == "task":
                from . import streams as _streams
                st = _streams.lane(self.dev, "w")
            else:
                st = torch.cuda.Stream(device=self.dev)
            BranchStreams._streams[key] = st
        return st

    def side_task(self, fn, keepalive, cost: float = 0.0):
        """Run `fn` — a kernel sequence whose results nobody reads before the end of the pass: a SMALL weight gradient, which on
        its own leaves most of the machine idle — on a task stream beside the trunk (R3D-18 +1.2 %, R(2+1)D +1.1 %).  Only from
        the trunk (flat forks); one task outstanding, the previous one is joined first.  `keepalive`: the tensors it reads,
        held until the join so that the graph's memory pool does not hand their blocks out again underneath it."""
        if BranchStreams.deferred is not None:
            BranchStreams.deferred.append((fn, keepalive, cost))      # (cost: FLOPs — rspnet_amd/graph_step.py places its cuts by it)
            return
        cur = torch.cuda.current_stream(self.dev) if self.on else None
        if cur is None or cur.cuda_stream != self.origin_h:
            return fn()
        held = []
        if BranchStreams.RUN_AHEAD and cost < BranchStreams.AHEAD_MAX_FLOPS and not torch.cuda.is_current_stream_capturing():
            # issued eagerly the task stream is a lane of its own (rspnet_amd/streams.py) and keeps its own order: the trunk does not
            # wait for the previous task before it hands over the next one — a weight gradient longer than the trunk's work up to
            # the next one no longer stalls the trunk — and everything the tasks read stays alive until the join
            if self.task is not None:
                held = self.task[1]
        else:
            self.join_task()
        ts = self._get("task")
        ts.wait_stream(cur)
        with torch.cuda.stream(ts):
            fn()
        held.append(keepalive)
        self.task = (ts, held)

    @contextlib.contextmanager
    def grads_ready(self):
        """Stream context ordered behind everything issued so far on the trunk AND on the side-task stream — for work that reads
        this pass's gradients but that the trunk need not wait for (an asynchronous all-reduce of a finished gradient bucket:
        RCCL orders it behind the stream it is issued from).  The trunk itself is not held up, unlike with join_task()."""
        cur = torch.cuda.current_stream(self.dev) if self.on else None
        if cur is None or cur.cuda_stream != self.origin_h or torch.cuda.is_current_stream_capturing():
            self.join_task()
            yield
            return
        ts = self._get("task")
        ts.wait_stream(cur)
        with torch.cuda.stream(ts):
            yield

    def join_task(self):
        if self.task is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self.task[0])
            self.task = None

    def run(self, node, fn):
        br = getattr(node, "branch", 0) if (self.on and self.fork_branches) else 0
        if br == 0:
            self.join()
            return fn()
        st = self.active.get(br)
        if st is None:
            st = self._get(br)
            st.wait_stream(torch.cuda.current_stream(self.dev))
            self.active[br] = st
        with torch.cuda.stream(st):
            return fn()

    def join(self):
        if self.active:
            main = torch.cuda.current_stream(self.dev)
            for st in self.active.values():
                main.wait_stream(st)
            self.active = {}

    def finish(self):
        self.join()
        if self.on:
            self.join_task()


def _readers(plan: "Plan") -> Dict[int, List[int]]:
    """{slot: indices of the plan nodes that read it, as input or as residual}"""
    readers: Dict[int, List[int]] = {}
    for i, n in enumerate(plan.nodes):
        for m in (n.members if isinstance(n, ConvBNGroup) else [n]):
            for slot in (getattr(m, "src", None), getattr(m, "residual", None)):
                if slot is not None:
                    readers.setdefault(slot, []).append(i)
    return readers


def _gate_fusion(plan: "Plan"):
    """{index of a ConvBN: (index of the Gate that is the only reader of its output, index of the Pool that is the only reader of
    the gate's output | None)} — S3D-G's sep_conv units (models/s3dg.py:36-72) and, for the two front-end ones, the max-pool
    behind them (:105-109).  The three run as one op (ops.bn_act_gate_fwd)."""
    if plan.gate_fusion is not None:
        return plan.gate_fusion
    readers = _readers(plan)
    table = {}
    if not os.environ.get("RSP_NO_GATE_FUSION"):
        for i, n in enumerate(plan.nodes[:-1]):
            g = plan.nodes[i + 1]
            if not (isinstance(n, ConvBN) and isinstance(g, Gate) and g.src == n.dst and g.branch == n.branch):
                continue
            if n.residual is not None or n.pool or n.into is not None or n.cout_pad or n.virtual_w or n.dst == plan.output_slot:
                continue
            if readers.get(n.dst) != [i + 1]:
                continue
            pi = None
            if i + 2 < len(plan.nodes):
                q = plan.nodes[i + 2]
                if (isinstance(q, Pool) and g.into is None and q.src == g.dst and q.branch == n.branch and readers.get(g.dst) == [i + 2]
                        and g.dst != plan.output_slot):
                    pi = i + 2
            table[i] = (i + 1, pi)
    plan.gate_fusion = table
    return table


GATE_POOL_APART = bool(os.environ.get("RSP_NO_GATE_POOL_KEEP"))      # (A/B switch: the kept forward of a gated unit runs its max-pool apart)


def _pool_fusion(plan: "Plan"):
    """{index of a ConvBN: index of the Pool that is the only reader of its output} — the ResNet stems (conv1 -> bn1 -> relu ->
    MaxPool3d(3, 2, 1), models/resnet.py:124-139,203-207).  A forward that keeps nothing for a backward (the two key passes) applies
    the BatchNorm and takes the window maximum in ONE pass over the convolution output (rsp_bn_act_pool_fwd takes any window): the
    activated tensor — 411 MB per pass on R3D-18 — is neither written nor read back.  Same arithmetic per element, same bits."""
    if plan.pool_fusion is not None:
        return plan.pool_fusion
    readers = _readers(plan)
    table = {}
    if not os.environ.get("RSP_NO_POOL_FUSION"):
        gated = _gate_fusion(plan)
        for i, n in enumerate(plan.nodes[:-1]):
            q = plan.nodes[i + 1]
            if not (isinstance(n, ConvBN) and isinstance(q, Pool) and q.src == n.dst and q.branch == n.branch) or i in gated:
                continue
            if n.pool or n.into is not None or n.cout_pad or n.dst == plan.output_slot or readers.get(n.dst) != [i + 1]:
                continue
            table[i] = i + 1
    plan.pool_fusion = table
    return table


# ---- helpers of both directions ----------------------------------------------------------------------------------------
def _view(t, into, C):
    return t if into is None else t[..., into[1]:into[1] + C]


def _out_view(slots, into, lead_shape, C, device):
    """Where a node with `into` = (concat slot, channel offset, total channels) writes: its channel slice of the concat tensor,
    which is allocated on first use.  None without `into`: the op allocates its output, and the caller puts it into the node's slot."""
    if into is None:
        return None
    slot, off, total = into
    if slot not in slots:
        slots[slot] = torch.empty(tuple(lead_shape) + (total,), dtype=torch.float32, device=device)
    return _view(slots[slot], into, C)


def _eval_scale_shift(bn, bias) -> torch.Tensor:
    """Eval-mode BatchNorm folded into the (scale, shift) pair the fused BN kernel consumes: y = conv + b,
    out = (y - running_mean) / sqrt(running_var + eps) * gamma + beta  =  conv * scale + shift."""
    scale = bn.weight.data * torch.rsqrt(bn.running_var + float(bn.eps))
    shift = bn.bias.data - bn.running_mean * scale
    if bias is not None:
        shift = shift + bias.data * scale
    return torch.stack([scale, shift]).contiguous()


def _eval_mean_invstd(bn, bias) -> torch.Tensor:
    """What the eval-mode backward needs next to (scale, shift): xhat = (conv - mean') * invstd with mean' = running_mean - b
    (the saved convolution output carries no bias) and invstd = 1 / sqrt(running_var + eps)."""
    mean = bn.running_mean if bias is None else bn.running_mean - bias.data
    return torch.stack([mean, torch.rsqrt(bn.running_var + float(bn.eps))]).contiguous()


EVAL_BACKWARD_MISSING = ("backward through an eval-mode backbone (BatchNorm on running statistics) is not implemented: "
                         "freeze the backbone (only_train_fc) or call model.train()")


def _handler(table, node):
    fn = table.get(type(node))
    if fn is None:
        raise NotImplementedError(f"plan node {type(node).__name__}")
    return fn


class _Forward:
    """One forward through a plan: the state run_forward's node handlers share, and one handler per node type."""

    def __init__(self, plan, x, packed, keep, training, deferred):
        self.be = _ops.backend()
        self.plan, self.packed, self.keep, self.training, self.deferred = plan, packed, keep, training, deferred
        self.slots: Dict[int, torch.Tensor] = {plan.input_slot: x}
        self.ctx = ForwardCtx(packed=packed) if keep else None
        self.pool_fusion = _pool_fusion(plan)
        self.gate_fusion = _gate_fusion(plan) if training else {}
        self.skipped = set()        # nodes that ran inside the kernel of the ConvBN in front of them
        self.y_sel = None           # what the last bn_apply kept for the backward's reduce (_Saved.y_sel), taken by its caller

    def finalize(self, bn, stats, rows, bias_d):
        # deferred: {id(BatchNorm module): [2][C] buffer} — this pass reports its batch moments there and leaves the running
        # statistics to a later rsp_bn_running_update (ops.BnEmaSet); otherwise bn_finalize moves them itself
        bso = self.deferred.get(id(bn)) if self.deferred is not None else None
        if bso is not None:
            return self.be.bn_finalize(stats, rows, bias_d, bn.weight.data, bn.bias.data, float(bn.eps), float(bn.momentum), None, None,
                                       batch_stats_out=bso)
        return self.be.bn_finalize(stats, rows, bias_d, bn.weight.data, bn.bias.data, float(bn.eps), float(bn.momentum),
                                   bn.running_mean, bn.running_var)

    def bn_apply(self, node, y, ss, C, dims, xin, key=None, sel=False):
        """BatchNorm apply [+ residual] [+ ReLU] [+ pool] of a convolution output y with `C` channels and dims (N, do, ho, wo)
        -> (PoolGeom a backward needs, residual).  sel: the caller stores self.y_sel in the unit's _Saved (pooled units of a kept
        pass: y at each window's selected position, for the backward's reduce)."""
        be, slots = self.be, self.slots
        pk, ps = node.pool if node.pool else ((1, 1, 1), (1, 1, 1))
        pg = PoolGeom(*dims, C, pk, ps, (0, 0, 0))
        res = slots[node.residual] if node.residual is not None else None
        pi = self.pool_fusion.get(key) if key is not None else None
        if pi is not None:      # the max-pool behind this unit taken by the kernel that applies the BatchNorm (_pool_fusion)
            pnode = self.plan.nodes[pi]
            pgf = PoolGeom(*dims, C, pnode.k, pnode.s, pnode.p)
            if not self.keep:
                slots[pnode.dst] = be.bn_act_pool_fwd(pgf, y, ss, res, node.relu)
                self.skipped.add(pi)
                return pgf, res
            # kept for a backward: the same pass also writes the arg-max (the Pool node's saved state); the BatchNorm backward
            # recomputes the activation from y as everywhere, so the activated tensor is never materialised
            fused = be.bn_act_maxpool_fwd(pgf, y, ss, node.relu, True) if (res is None and hasattr(be, "bn_act_maxpool_fwd")) else None
            if fused is not None:
                slots[pnode.dst], idx = fused
                self.ctx.saved[pi] = _SavedPool(pgf, idx)
                self.skipped.add(pi)
                return pg, res
        out = _out_view(slots, node.into, (dims[0],) + pg.out_dims, C, xin.device)
        if out is not None:
            be.bn_act_pool_fwd(pg, y, ss, res, node.relu, out=out)
        else:
            if (sel and self.keep and self.training and BN_BWD_SEL and node.pool and res is None and pi is None
                    and hasattr(be, "bn_act_pool_sel_fwd")):
                got = be.bn_act_pool_sel_fwd(pg, y, ss, node.relu)
                if got is not None:
                    slots[node.dst], self.y_sel = got
                    return pg, res
            slots[node.dst] = be.bn_act_pool_fwd(pg, y, ss, res, node.relu)
        return pg, res

    def convbn_virtual(self, node, key, xin):
        """ConvBN of a 3-channel stride-2 stem as two ordinary convolutions over virtual pixels (see VirtualStem)."""
        N, D, H, W, _ = xin.shape
        Cp = max(node.cout_pad, node.conv.weight.shape[0])
        vs = self.packed.virtual_stem(node)
        x_e, x_o = vs.pack_rows(xin)
        (kT, kH, _), (sT, sH, _), (pT, pH, _) = node.k, node.s, node.p
        cg = ConvGeom(N, D, H, x_e.shape[3], 4, Cp, (kT, kH, 6), (sT, sH, 3), (pT, pH, 0), Cin_alg=3 * 7 / 6)
        do, ho, g = cg.out_dims
        y = torch.empty((N, do, ho, 2 * g, Cp), dtype=torch.float32, device=xin.device)
        yv = y.view(N, do, ho, g, 2 * Cp)
        parts = []
        for c, xc in enumerate((x_e, x_o)):
            _, st = self.be.conv_fwd(cg, xc, self.packed.get(vs.holders[c], cg), None, True, out=yv[..., c * Cp:(c + 1) * Cp], out_ld=2 * Cp)
            parts.append(st)
        rows = N * do * ho * 2 * g
        mi, ss = self.finalize(node.bn, torch.cat(parts), rows, None)
        pg, _ = self.bn_apply(node, y, ss, Cp, (N, do, ho, 2 * g), xin, key)
        if self.keep:
            self.ctx.saved[key] = _SavedVStem(x_e, x_o, y, mi, ss, cg, pg, vs)

    def convbn(self, node, key):
        be, keep = self.be, self.keep
        xin = self.slots[node.src]
        if self.training and node.virtual_w and VirtualStem.applies(node, xin):
            return self.convbn_virtual(node, key, xin)
        N, D, H, W, Cin = xin.shape
        w = node.conv.weight
        Cout = w.shape[0]
        Cp = max(node.cout_pad, Cout)
        cg = ConvGeom(N, D, H, W, Cin, Cp, node.k, node.s, node.p, Cin_alg=w.shape[1])
        bias = getattr(node.conv, "bias", None)
        bn = node.bn
        bias_d = None if bias is None else bias.data
        if self.stem_pooled(node, key, xin, cg, bias_d):
            return
        if self.training:
            # (no shipped backbone has a conv bias on channel-padded units; if one does, the conv needs it at the padded length)
            bias_conv = bias_d if (bias_d is None or Cp == Cout) else torch.cat([bias_d, bias_d.new_zeros(Cp - Cout)])
            y, stats = be.conv_fwd(cg, xin, self.packed.get(node.conv, cg), bias_conv, True)
            # (zero-padded output channels, Cp > Cout: the BatchNorm vectors keep their Cout entries, the kernels treat the rest
            #  as gamma = beta = 0 and leave the running statistics of the real channels alone)
            mi, ss = self.finalize(bn, stats, cg.rows, bias_d)
        else:
            y, _ = be.conv_fwd(cg, xin, self.packed.get(node.conv, cg), None, False)     # bias folded into the shift
            ss = _eval_scale_shift(bn, bias)
            mi = _eval_mean_invstd(bn, bias) if keep else None
            if Cp != Cout:
                pad = torch.zeros((2, Cp - Cout), dtype=ss.dtype, device=ss.device)
                ss, mi = (None if v is None else torch.cat([v, pad], dim=1).contiguous() for v in (ss, mi))
        dims = (N,) + cg.out_dims
        gated = self.gate_fusion.get(key)
        if gated is not None:
            return self.bn_gate(node, key, gated, xin, y, mi, ss, cg, dims)
        pg, res = self.bn_apply(node, y, ss, cg.Cout, dims, xin, key, sel=True)
        if keep:
            self.ctx.saved[key] = _Saved(xin, y, mi, ss, cg, pg, res, eval_mode=not self.training, y_sel=self.y_sel)
            self.y_sel = None

    def stem_pooled(self, node, key, xin, cg, bias_d) -> bool:
        """A 4-channel stem with BatchNorm -> ReLU -> MaxPool(1,2,2) behind it in a training-mode pass that keeps nothing (the key
        passes' conv1): its full-size output would be written only to be read back once and pooled to a quarter.  BatchNorm apply and
        ReLU are monotone per channel and commute with the window maximum (minimum, for a negative scale), so the stem kernel leaves
        the window maximum and minimum of its raw output and a small pass applies BatchNorm + ReLU to them: same values, half the
        bytes written and a quarter read.  False where it does not apply — the caller goes on as ever."""
        be = self.be
        if (self.keep or not self.training or not STEM_POOLED or not node.pool or tuple(node.pool[0]) != (1, 2, 2)
                or tuple(node.pool[1]) != (1, 2, 2) or node.residual is not None or node.cout_pad or node.virtual_w
                or xin.shape[4] != 4 or cg.Cout > 64 or self.gate_fusion.get(key) is not None or self.pool_fusion.get(key) is not None
                or not hasattr(be, "stem_pooled_fwd")):
            return False
        _, ho, wo = cg.out_dims
        if ho % 2 or wo % 2:
            return False
        got = be.stem_pooled_fwd(cg, xin, self.packed.get(node.conv, cg), bias_d)
        if got is None:
            return False
        ymax, ymin, stats = got
        _, ss = self.finalize(node.bn, stats, cg.rows, bias_d)
        out = _out_view(self.slots, node.into, ymax.shape[:4], cg.Cout, xin.device)
        if out is not None:
            be.bn_act_minmax_fwd(ymax, ymin, ss, node.relu, out=out)
        else:
            self.slots[node.dst] = be.bn_act_minmax_fwd(ymax, ymin, ss, node.relu)
        return True

    def bn_gate(self, node, key, gated, xin, y, mi, ss, cg, dims):
        """The rest of a ConvBN with the Gate behind it: BatchNorm-apply + self-gating (+ the max-pool behind a front-end unit, when
        nothing is kept for a backward) in two passes over y: see _gate_fusion"""
        be, keep, slots = self.be, self.keep, self.slots
        gi, pi = gated
        gnode = self.plan.nodes[gi]
        pnode = self.plan.nodes[pi] if pi is not None else None
        pg = PoolGeom(*dims, cg.Cout)
        pool = PoolGeom(*dims, cg.Cout, pnode.k, pnode.s, pnode.p) if pnode is not None else None
        # (a backward recomputes the activation from y: nothing but the (sample, channel) means and gates is kept)
        keep_act = keep and not GATE_BWD_FUSED
        # a forward a backward follows pools in the same pass only if that pass can also write the pool's arg-max
        with_idx = (keep and pool is not None and not keep_act and getattr(be, "gate_pool_keep", False) and not GATE_POOL_APART
                    and be.bn_act_gate_pool_idx_ok(pool, y, ss))
        if keep and not with_idx:
            pnode = pool = None
        out = _out_view(slots, gnode.into, dims, cg.Cout, xin.device)
        gw, gb = gnode.conv.weight.data, gnode.conv.bias.data
        if with_idx:
            o, a, mean, gate, idx = be.bn_act_gate_fwd(pg, y, ss, node.relu, gw, gb, False, pool=pool, out=out, pool_idx=True)
            self.ctx.saved[pi] = _SavedPool(pool, idx)
        else:
            o, a, mean, gate = be.bn_act_gate_fwd(pg, y, ss, node.relu, gw, gb, keep_act, pool=pool, out=out)
        if pnode is not None:
            slots[pnode.dst] = o
            self.skipped.add(pi)
        elif gnode.into is None:
            slots[gnode.dst] = o
        self.skipped.add(gi)
        if keep:
            sg = self.ctx.saved[gi] = _SavedGate(gi, a if keep_act else None, mean, gate)
            self.ctx.saved[key] = _Saved(xin, y, mi, ss, cg, pg, None, gate=None if keep_act else sg)

    def group(self, node, ni):
        """One GEMM over the members' concatenated filters (see ConvBNGroup); falls back to member-by-member execution."""
        ms = node.members
        wcat = _adjacent_cat([m.conv.weight.data for m in ms]) if self.training else None
        if wcat is None:
            for j, m in enumerate(ms):
                self.convbn(m, (ni, j))
            return
        xin = self.slots[ms[0].src]
        N, D, H, W, Cin = xin.shape
        if node.cat is None:
            node.cat = _CatConv()
        node.cat.weight = wcat
        cg = ConvGeom(N, D, H, W, Cin, wcat.shape[0], ms[0].k, ms[0].s, ms[0].p)
        y, stats = self.be.conv_fwd(cg, xin, self.packed.get(node.cat, cg), None, True)
        off, per = 0, []
        for m in ms:
            C = m.conv.weight.shape[0]
            mi, ss = self.finalize(m.bn, stats[:, off:off + C], cg.rows, None)
            pg, _ = self.bn_apply(m, y[..., off:off + C], ss, C, (N,) + cg.out_dims, xin)
            per.append(_SavedMember(off, C, mi, ss, pg))
            off += C
        if self.keep:
            self.ctx.saved[ni] = _SavedGroup(xin, y, cg, per)

    def convbias(self, node, ni):
        xin = self.slots[node.src]
        N, D, H, W, Cin = xin.shape
        cg = ConvGeom(N, D, H, W, Cin, node.conv.weight.shape[0], node.k, node.s, node.p)
        y, _ = self.be.conv_fwd(cg, xin, self.packed.get(node.conv, cg), node.conv.bias.data, False)
        if node.relu:
            y = self.be.eltwise("relu_fwd", y, out=y)
        self.slots[node.dst] = y
        if self.keep:
            self.ctx.saved[ni] = _SavedConvBias(xin, y, cg)

    def pool(self, node, ni):
        xin = self.slots[node.src]
        N, D, H, W, Cc = xin.shape
        pg = PoolGeom(N, D, H, W, Cc, node.k, node.s, node.p)
        self.slots[node.dst], idx = self.be.maxpool_fwd(pg, xin, self.keep)
        if self.keep:
            self.ctx.saved[ni] = _SavedPool(pg, idx)

    def gate(self, node, ni):
        xin = self.slots[node.src]
        out = _out_view(self.slots, node.into, tuple(xin.shape[:4]), xin.shape[4], xin.device)
        o, mean, gate = self.be.gate_fwd(xin, node.conv.weight.data, node.conv.bias.data, out=out)
        if node.into is None:
            self.slots[node.dst] = o
        if self.keep:
            self.ctx.saved[ni] = _SavedGate(ni, xin, mean, gate)

    HANDLERS = {ConvBN: convbn, ConvBNGroup: group, ConvBias: convbias, Pool: pool, Gate: gate}

    def run_node(self, ni, node):
        if ni not in self.skipped:
            _handler(self.HANDLERS, node)(self, node, ni)


def run_forward(plan: Plan, x: torch.Tensor, packed: PackedWeights, keep: bool, training: bool = True,
                deferred: Optional[Dict[int, torch.Tensor]] = None) -> Tuple[torch.Tensor, Optional[ForwardCtx]]:
    """Execute `plan` on x (N,D,H,W,C).  keep=True records what backward needs.  training=True: batch-statistics BN (the
    pretext step never runs anything else: pretrain.py:225); training=False: running-statistics BN for the fine-tune /
    validation forward (finetune.py:333-345) and for fine-tuning with frozen BatchNorm (keep=True: the backward then runs
    bn_eval_act_pool_bwd per ConvBN; no virtual stem, no grouped convolutions, no gate fusion in this mode, so Gate and Pool nodes
    keep their ordinary saved state)."""
    fw = _Forward(plan, x, packed, keep, training, deferred)
    branches = BranchStreams(x)
    for ni, node in enumerate(plan.nodes):
        branches.run(node, lambda: fw.run_node(ni, node))
    branches.finish()
    out = fw.slots[plan.output_slot]
    if keep:
        fw.ctx.feat_shape = tuple(out.shape)
    return out, fw.ctx


def run_backward(plan: Plan, ctx: ForwardCtx, dfeat: torch.Tensor, grad_of, after_param_grads=None,
                 want_input_grad: bool = False, packed: Optional[PackedWeights] = None):
    """Backward through the plan in one go: see run_backward_iter."""
    it = run_backward_iter(plan, ctx, dfeat, grad_of, after_param_grads, want_input_grad, packed)
    try:
        while True:
            next(it)
    except StopIteration as done:
        return done.value


class _Backward:
    """One backward through a plan: the state run_backward_iter's node handlers share, and one handler per node type; a ConvBN's
    handler goes on by the type of record its forward saved."""

    def __init__(self, plan, ctx, dfeat, grad_of, after_param_grads, want_input_grad, packed):
        self.be = _ops.backend()
        self.plan, self.ctx, self.grad_of, self.hook, self.want_input_grad = plan, ctx, grad_of, after_param_grads, want_input_grad
        self.packed = packed if packed is not None else ctx.packed
        self.dslots: Dict[int, torch.Tensor] = {plan.output_slot: dfeat}
        self.branches = BranchStreams(dfeat)

    def add_grad(self, slot, g):
        # gradient accumulation at fan-out points; g is always the fresh output of the op that produced it, so the sum is
        # written over it (no allocation, nothing else aliases it)
        if g is None:
            return
        if slot in self.dslots:
            self.dslots[slot] = self.be.eltwise("add", self.dslots[slot].contiguous(), g, out=g)
        else:
            self.dslots[slot] = g

    def take_grad(self, node, C):
        """The incoming gradient of a node's output: its channel slice of a concat tensor's gradient, or its own slot's (popped)."""
        return _view(self.dslots[node.into[0]], node.into, C) if node.into is not None else self.dslots.pop(node.dst)

    def issued(self, ni):
        """The parameter gradients of node `ni` have been issued (see run_backward_iter: after_param_grads)."""
        if self.hook is not None:
            self.hook(ni, self.branches.grads_ready)

    def input_grad(self, src, cg, dy, conv):
        """dgrad into slot `src` — unless that is the plan's input and nobody asked for its gradient."""
        if src != self.plan.input_slot or self.want_input_grad:
            self.add_grad(src, self.be.conv_dgrad_packed(cg, dy, self.packed.get_dgrad(conv, cg)))

    def convbn(self, node, ni, key=None):
        key = ni if key is None else key
        sv = self.ctx.saved.pop(key)
        if isinstance(sv, _SavedVStem):
            return self.convbn_virtual(node, sv, ni)
        if sv.gate is not None:
            return self.convbn_gated(node, sv, ni)
        if sv.eval_mode:
            return self.convbn_eval(node, sv, ni)
        bn, grad_of = node.bn, self.grad_of
        dout = self.take_grad(node, sv.cg.Cout)
        sel = {} if sv.y_sel is None else {"y_sel": sv.y_sel}
        dy, dres = self.be.bn_act_pool_bwd(sv.pg, sv.y, sv.res, dout, bn.weight.data, sv.mi, sv.ss, node.relu,
                                           node.residual is not None, grad_of(bn.weight), grad_of(bn.bias), **sel)
        self.convbn_tail(node, sv, ni, dy, dres, True)

    def convbn_virtual(self, node, sv, ni):
        be, grad_of, vs, cg = self.be, self.grad_of, sv.vs, sv.cg
        assert node.src == self.plan.input_slot and not self.want_input_grad, "a virtual-pixel stem reads the clip: no input gradient"
        dout = self.dslots.pop(node.dst)
        bn = node.bn
        dy, _ = be.bn_act_pool_bwd(sv.pg, sv.y, None, dout, bn.weight.data, sv.mi, sv.ss, node.relu, False, grad_of(bn.weight), grad_of(bn.bias))
        gw = grad_of(node.conv.weight)
        if gw is not None:
            N, do, ho, Wo, Cp = dy.shape
            dyv = dy.view(N, do, ho, Wo // 2, 2 * Cp)
            gflat = gw.view(-1)
            gflat.zero_()
            for c, xc in enumerate((sv.x_e, sv.x_o)):
                gv = torch.empty_like(vs.holders[c].weight)
                be.conv_wgrad(cg, xc, dyv[..., c * Cp:(c + 1) * Cp], gv)
                # every real filter element appears once in a class's virtual filter: unique indices, order-independent
                gflat.index_add_(0, vs.dst[c], gv.view(-1).index_select(0, vs.src[c]))
        self.issued(ni)

    def convbn_gated(self, node, sv, ni):
        """... with the self-gating unit behind this BatchNorm, whose forward kept no activation: both backwards as one op"""
        bn, grad_of, sg = node.bn, self.grad_of, sv.gate
        gnode = self.plan.nodes[sg.at]
        dout = self.take_grad(gnode, sv.cg.Cout)
        dy = self.be.bn_act_gate_bwd(sv.pg, sv.y, dout, bn.weight.data, sv.mi, sv.ss, node.relu, gnode.conv.weight.data, sg.mean, sg.gate,
                                     grad_of(bn.weight), grad_of(bn.bias), grad_of(gnode.conv.weight), grad_of(gnode.conv.bias))
        self.issued(sg.at)
        self.convbn_tail(node, sv, ni, dy, None, True)

    def convbn_eval(self, node, sv, ni):
        """ConvBN whose forward ran BatchNorm on its running statistics: dy = scale * dz in one pass (bn_eval_act_pool_bwd)."""
        be, grad_of = self.be, self.grad_of
        if not hasattr(be, "bn_eval_act_pool_bwd"):
            raise RuntimeError(EVAL_BACKWARD_MISSING)
        bn = node.bn
        dout = self.take_grad(node, sv.cg.Cout)
        bias = getattr(node.conv, "bias", None)
        gbias = grad_of(bias) if bias is not None else None
        dgamma, dbeta = grad_of(bn.weight), grad_of(bn.bias)
        # the bias gradient comes from the dbeta sums — also with frozen affine parameters: the sums then land in a scratch vector
        sums = dbeta if (dbeta is not None or gbias is None) else torch.empty_like(bn.bias.data)
        dy, dres = be.bn_eval_act_pool_bwd(sv.pg, sv.y, sv.res, dout, sv.mi, sv.ss, node.relu, node.residual is not None, dgamma, sums)
        if gbias is not None:
            # out = (conv + b) * scale + shift0: d/db = scale * sum dz.  (Train-mode BatchNorm subtracts the batch mean and cancels
            # it; running statistics do not.)
            torch.mul(sv.ss[0][:gbias.shape[0]], sums, out=gbias)
        self.convbn_tail(node, sv, ni, dy, dres, False)

    def convbn_tail(self, node, sv, ni, dy, dres, zero_bias):
        """Behind the BatchNorm backward: residual fan-out, the weight gradient (beside the trunk where it is small), the hook, dgrad."""
        be, grad_of = self.be, self.grad_of
        if node.residual is not None:
            self.add_grad(node.residual, dres)
        bias = getattr(node.conv, "bias", None)
        if bias is not None and zero_bias:
            gb = grad_of(bias)
            if gb is not None:
                # A conv bias in front of train-mode BatchNorm has an identically-zero gradient (BN subtracts the
                # batch mean); the reference's autograd produces ~1e-8 rounding noise there.
                gb.zero_()
        # (a channel-padded geometry writes only the parameter's own channels: the reduce drops the padding's gradients)
        gw = grad_of(node.conv.weight)
        # (side stream: a gradient hook — the bucketed all-reduce of the data-parallel path — joins the task before it lets a
        #  bucket go, see run_backward_iter's docstring)
        if (sv.cg.flops < BranchStreams.SMALL_WGRAD_FLOPS or
                (sv.cg.flops < BranchStreams.MID_WGRAD_FLOPS and sv.cg.bytes < BranchStreams.MID_WGRAD_BYTES)):
            self.branches.side_task(lambda: be.conv_wgrad(sv.cg, sv.x, dy, gw), (sv.x, dy), cost=float(sv.cg.flops))
        else:
            be.conv_wgrad(sv.cg, sv.x, dy, gw)
        self.issued(ni)
        self.input_grad(node.src, sv.cg, dy, node.conv)

    def group(self, node, ni):
        sv = self.ctx.saved.pop(ni, None)
        ms = node.members
        if sv is None:                                   # forward ran the members one by one
            for j in range(len(ms) - 1, -1, -1):
                self.convbn(ms[j], ni, (ni, j))
            return
        be, grad_of = self.be, self.grad_of
        dy_cat = torch.empty_like(sv.y)
        for m, p in zip(ms, sv.per):
            be.bn_act_pool_bwd(p.pg, sv.y[..., p.off:p.off + p.C], None, self.take_grad(m, p.C), m.bn.weight.data, p.mi, p.ss, m.relu, False,
                               grad_of(m.bn.weight), grad_of(m.bn.bias), dy_out=dy_cat[..., p.off:p.off + p.C])
        gws = [grad_of(m.conv.weight) for m in ms]
        gcat = _adjacent_cat(gws) if all(g is not None for g in gws) else None
        if gcat is not None:
            be.conv_wgrad(sv.cg, sv.x, dy_cat, gcat)
        else:
            tmp = torch.empty_like(node.cat.weight)
            be.conv_wgrad(sv.cg, sv.x, dy_cat, tmp)
            off = 0
            for m, g in zip(ms, gws):
                if g is not None:
                    g.copy_(tmp[off:off + g.shape[0]])
                off += m.conv.weight.shape[0]
        self.issued(ni)
        self.input_grad(ms[0].src, sv.cg, dy_cat, node.cat)

    def convbias(self, node, ni):
        sv = self.ctx.saved.pop(ni)
        dout = self.dslots.pop(node.dst)
        dz = self.be.eltwise("relu_bwd", sv.y, dout.contiguous()) if node.relu else dout.contiguous()
        self.be.conv_wgrad(sv.cg, sv.x, dz, self.grad_of(node.conv.weight), self.grad_of(node.conv.bias))
        self.issued(ni)
        self.input_grad(node.src, sv.cg, dz, node.conv)

    def pool(self, node, ni):
        sv = self.ctx.saved.pop(ni)
        self.add_grad(node.src, self.be.maxpool_bwd(sv.pg, self.dslots.pop(node.dst), sv.idx))

    def gate(self, node, ni):
        sv = self.ctx.saved.pop(ni)
        if sv.x is None:      # its backward runs with the BatchNorm's in front of it (convbn_gated)
            return
        dout = self.take_grad(node, sv.x.shape[4])
        self.add_grad(node.src, self.be.gate_bwd(sv.x, dout, node.conv.weight.data, sv.mean, sv.gate, self.grad_of(node.conv.weight),
                                                 self.grad_of(node.conv.bias)))
        self.issued(ni)

    HANDLERS = {ConvBN: convbn, ConvBNGroup: group, ConvBias: convbias, Pool: pool, Gate: gate}


def run_backward_iter(plan: Plan, ctx: ForwardCtx, dfeat: torch.Tensor, grad_of, after_param_grads=None,
                      want_input_grad: bool = False, packed: Optional[PackedWeights] = None):
    """Generator form of the backward: yields the index of each plan node once its kernels have been issued, so that a caller can
    cut the backward into pieces (rspnet_amd/graph_step.py captures each piece as a linear HIP graph and runs the weight gradients
    that `BranchStreams.deferred` collected beside the next piece); the generator's return value is run_backward's.

    Backward through the plan.  `grad_of(param)` returns the (pre-allocated, flat-buffer) gradient view to
    fill for a parameter, or None to skip it.  `after_param_grads(node_index, grads_ready)` is called once a node's parameter
    gradients have been ISSUED (used to launch bucketed all-reduces overlapped with the rest of backward); a weight gradient may
    still be running on the side-task stream then — the hook issues whatever reads gradients inside `with grads_ready():`, a
    stream context ordered behind all of them (BranchStreams.grads_ready).
    want_input_grad: also propagate to the plan's input slot and return that gradient (projection-head sub-plans, whose
    input is the backbone feature; the backbone's own input is the clip and needs none)."""
    bw = _Backward(plan, ctx, dfeat, grad_of, after_param_grads, want_input_grad, packed)
    # (side branches of a block — engine.BranchStreams — each own their slots; the fan-out sum at the block's input happens on the
    #  trunk after the join: the block's last backward node, the grouped pointwise convolution, is a trunk node)
    for ni in range(len(plan.nodes) - 1, -1, -1):
        node = plan.nodes[ni]
        bw.branches.run(node, lambda: _handler(bw.HANDLERS, node)(bw, node, ni))
        yield ni
    bw.branches.finish()
    return bw.dslots.get(plan.input_slot) if want_input_grad else None
