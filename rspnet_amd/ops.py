"""Tensor-level gateway to the HIP kernels (one method per C-ABI entry point family).

Activations are torch tensors of shape (N, D, H, W, C) (NDHWC, contiguous, fp32); torch is used only as the
owner of device memory and of the current stream.  ``HipOps`` is the only product backend: it requires CUDA/HIP
tensors and the built ``librspnet_hip.so`` and raises otherwise.  ``set_backend`` exists so that the host logic
(graph executor, DDP exchange, optimizer) can be exercised by CPU tests with a checker backend living under
``tests/``; nothing in this package ever selects another backend by itself.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib


@dataclass(frozen=True)
class ConvGeom:
    """Geometry of one nn.Conv3d application (groups=1, dilation=1)."""
    N: int
    Di: int
    Hi: int
    Wi: int
    Cin: int
    Cout: int
    k: Tuple[int, int, int]
    s: Tuple[int, int, int]
    p: Tuple[int, int, int]
    Cin_alg: float = 0  # algorithmic input channels when Cin includes zero padding (FLOP / byte accounting only; may be fractional)

    @property
    def out_dims(self):
        return tuple((i + 2 * p - k) // s + 1 for i, k, s, p in zip((self.Di, self.Hi, self.Wi), self.k, self.s, self.p))

    @property
    def rows(self):
        d, h, w = self.out_dims
        return self.N * d * h * w

    @property
    def flops(self):
        """Algorithmic FLOPs of one pass (2*MACs, padded taps included — SURVEY.md §8d)."""
        return int(2 * self.rows * self.Cout * (self.Cin_alg or self.Cin) * self.k[0] * self.k[1] * self.k[2])

    @property
    def bytes(self):
        """Algorithmic bytes of one pass (forward, dgrad or wgrad alike): input + output activations + weights, each moved
        once — what a launch must touch at least; the measured L2-miss traffic is priced against it."""
        taps = self.k[0] * self.k[1] * self.k[2]
        cin = self.Cin_alg or self.Cin
        return int(4 * (self.N * self.Di * self.Hi * self.Wi * cin + self.rows * self.Cout + self.Cout * cin * taps))

    def desc(self, in_ld=None, out_ld=None) -> _lib.ConvDesc:
        do, ho, wo = self.out_dims
        return _lib.ConvDesc(self.N, self.Di, self.Hi, self.Wi, self.Cin, do, ho, wo, self.Cout, *self.k, *self.s, *self.p,
                             in_ld or self.Cin, out_ld or self.Cout)


@dataclass(frozen=True)
class PoolGeom:
    """Geometry of the (optional) MaxPool3d fused behind BN+ReLU. k=s=(1,1,1), p=0 means no pooling."""
    N: int
    Di: int
    Hi: int
    Wi: int
    C: int
    k: Tuple[int, int, int] = (1, 1, 1)
    s: Tuple[int, int, int] = (1, 1, 1)
    p: Tuple[int, int, int] = (0, 0, 0)

    @property
    def out_dims(self):
        return tuple((i + 2 * p - k) // s + 1 for i, k, s, p in zip((self.Di, self.Hi, self.Wi), self.k, self.s, self.p))

    def desc(self, in_ld=None, out_ld=None, res_ld=None) -> _lib.PoolDesc:
        do, ho, wo = self.out_dims
        return _lib.PoolDesc(self.N, self.Di, self.Hi, self.Wi, self.C, do, ho, wo, *self.k, *self.s, *self.p,
                             in_ld or self.C, out_ld or self.C, res_ld or self.C)


@functools.lru_cache(maxsize=4096)
def _conv_plan(g: "ConvGeom", in_ld, out_ld):
    """ctypes descriptor + geometry-derived sizes of one conv application, built once per distinct geometry (the
    per-launch host cost matters for the small-layer backbones: ~700-2500 launches per step).  Names and workspace sizes are read
    off the plan the library's launch path executes (conv_igemm.hip plan_conv): one decision, not a second derivation."""
    lib = _lib.load()
    d = g.desc(in_ld=in_ld, out_ld=out_ld)
    ref = C.byref(d)
    names = tuple(lib.rsp_conv3d_kernel_name(ref, which).decode() for which in (0, 1, 2))
    return (d, ref, lib.rsp_conv3d_stat_tiles(ref), lib.rsp_conv3d_fwd_workspace(ref), lib.rsp_conv3d_dgrad_workspace(ref),
            lib.rsp_conv3d_wgrad_workspace(ref), g.out_dims, names)


@functools.lru_cache(maxsize=4096)
def executed_fraction(g: "ConvGeom", which: int) -> float:
    """Share of the algorithmic MACs of one pass (0 forward, 1 dgrad, 2 wgrad) the kernels execute after skipping padding chunks
    (rsp_conv3d_executed_fraction; host arithmetic, measurement bookkeeping only)."""
    d = g.desc()
    return float(_lib.load().rsp_conv3d_executed_fraction(C.byref(d), which))


@functools.lru_cache(maxsize=8192)
def _pack_signature(g: "ConvGeom", which: int, cout_src: int, cin_src: int):
    lib = _lib.load()
    d = g.desc()
    buf = (_lib.PackJob * 64)()
    cnt = lib.rsp_conv3d_pack_jobs(C.byref(d), which, cout_src, cin_src, C.c_void_p(1 << 20), C.c_void_p(1 << 30), buf, 64)
    lib.rsp_conv3d_pack_forget(C.c_void_p(1 << 30))      # (a probe with dummy pointers: nothing to remember about that address)
    if cnt < 0:
        _lib.check(cnt, "rsp_conv3d_pack_jobs")
    n = (lib.rsp_conv3d_packed_dgrad_elems if which else lib.rsp_conv3d_packed_fwd_elems)(C.byref(d))
    return (int(n), bytes(buf)[:cnt * C.sizeof(_lib.PackJob)])


@functools.lru_cache(maxsize=4096)
def _stem_pooled_ok(g: "ConvGeom") -> bool:
    d = g.desc()
    return bool(_lib.load().rsp_conv3d_stem_pooled_applicable(C.byref(d)))


@functools.lru_cache(maxsize=4096)
def _pool_plan(pg: "PoolGeom", in_ld, out_ld, res_ld):
    lib = _lib.load()
    d = pg.desc(in_ld=in_ld, out_ld=out_ld, res_ld=res_ld)
    ref = C.byref(d)
    return d, ref, lib.rsp_bn_bwd_workspace(ref), pg.out_dims


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """torch's current HIP stream of the current device as a raw handle.  (torch.cuda.current_stream() builds a Stream object
    through three Python layers: 7 us a call, 8 ms of host time per S3D-G step at ~1 150 kernel calls; the raw query is the same
    lookup without the wrapper.)"""
    if _raw_stream is not None and _get_device is not None:
        return C.c_void_p(_raw_stream(_get_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: torch.Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise _lib.RspError(f"{name}: expected a HIP device tensor (rspnet_amd has no CPU path)")
    if t.dtype != dtype:
        raise _lib.RspError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.RspError(f"{name}: expected a contiguous tensor")
    return t


def _search_operands(who: str, q: torch.Tensor, g: torch.Tensor):
    """The checks the cosine search's callers make on the query and gallery matrices; (Nq, Ng, D, row pitch of q, row pitch of g)."""
    for n, t in (("q", q), ("g", g)):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise _lib.RspError(f"{who}: {n} must be a float32 HIP device matrix with unit column stride")
    Nq, D = q.shape
    Ng = g.shape[0]
    if g.shape[1] != D:
        raise _lib.RspError(f"{who}: feature dims differ ({D} vs {g.shape[1]})")
    return Nq, Ng, D, q.stride(0) if Nq > 1 else D, g.stride(0) if Ng > 1 else D


def _rows_ld(t: torch.Tensor, name: str) -> int:
    """Channel pitch of an NDHWC tensor that is either contiguous or a channel slice of a contiguous one."""
    if not t.is_cuda or t.dtype != torch.float32:
        raise _lib.RspError(f"{name}: expected a float32 HIP device tensor (rspnet_amd has no CPU path)")
    if t.is_contiguous():
        return t.shape[-1]
    ld = t.stride(-2)
    exp, ok = ld, t.stride(-1) == 1
    for dim in range(t.dim() - 2, -1, -1):
        ok = ok and (t.stride(dim) == exp or t.shape[dim] == 1)
        exp *= t.shape[dim]
    if not ok:
        raise _lib.RspError(f"{name}: expected a dense NDHWC tensor or a channel slice of one")
    return ld


def _dy_target(y, in_ld: int, dy_out):
    """Where a BatchNorm backward writes dy: dy_out when given (it must have y's shape and channel pitch), else a fresh tensor — which
    a y that is a channel slice cannot have."""
    if dy_out is not None:
        if _rows_ld(dy_out, "dy_out") != in_ld or dy_out.shape != y.shape:
            raise _lib.RspError("dy_out: expected the shape and channel pitch of y")
        return dy_out
    if not y.is_contiguous():
        raise _lib.RspError("y is a channel slice: pass dy_out with the same pitch")
    return torch.empty_like(y)


KnnResult = collections.namedtuple("KnnResult", "pred rank hits votes idx dist")      # of HipOps.knn_classify
ReprResult = collections.namedtuple("ReprResult", "sums gram colsum")                  # of HipOps.repr_stats
KmeansResult = collections.namedtuple("KmeansResult", "assign counts changed objective info")      # of HipOps.kmeans_fit
TsneAffinities = collections.namedtuple("TsneAffinities", "pmat rows beta dmat info")                  # of HipOps.tsne_affinities


class HipOps:
    """Calls into librspnet_hip.so on the current HIP stream of the current device."""

    name = "hip"

    def __init__(self):
        self.lib = _lib.load(init_gpu=True)
        self._ws = {}
        # geometry -> [row-geometry table of the weight-gradient kernels, event behind its fill | None, raw handle of the fill
        # stream, pinned by a captured graph?] (see _rowgeom_table), least recently used first
        self._rowgeom = collections.OrderedDict()
        self._rowgeom_bytes = 0
        self._rowgeom_streams = {}      # raw handle -> stream object of every stream a table was handed to (for eviction)
        # bench.py sets this to a list to collect (kind, algorithmic_flops, start_event, end_event, kernel name, algorithmic
        # bytes, geometry) per MFMA launch
        # group, recorded on the stream the kernels run on (torch's current stream).
        self.event_log = None
        self.hbm_log = None      # (kind, algorithmic bytes, start, end) per streaming launch group, with event_log

    def _ev(self):
        if self.event_log is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def _log(self, kind, g, e0, kernel=""):
        # kernel = the template instance the library dispatches for this launch (rsp_conv3d_kernel_name)
        if e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            which = {"conv_fwd": 0, "conv_dgrad": 1, "conv_wgrad": 2}[kind]
            self.event_log.append((kind, g.flops, e0, e1, kernel, g.bytes, g, g.flops * executed_fraction(g, which)))

    def _log_hbm(self, kind, nbytes, e0):
        """bench.py's roofline pass: a streaming (HBM-bound) launch group with its algorithmic bytes — every operand tensor moved
        once."""
        if e0 is not None and self.hbm_log is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.hbm_log.append((kind, int(nbytes), e0, e1))

    # one grow-only scratch buffer per (device, stream): kernels on one stream are serialised, so they can share it; work issued
    # on different streams (independent branches of a layer graph) must not
    def _workspace(self, dev, nbytes: int) -> torch.Tensor:
        if torch.cuda.is_current_stream_capturing():
            # inside a HIP-graph capture the scratch comes from the graph's own memory pool, per call: it lives exactly as long as
            # the graph (a cached buffer would outlive a destroyed graph's pool, or be freed under a live graph when it grows),
            # and the pool's stream-aware reuse keeps kernels on forked streams apart
            return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
        key = (dev, _stream().value)
        buf = self._ws.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None:
                buf.record_stream(torch.cuda.current_stream(dev))
            buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=dev)
            self._ws[key] = buf
        return buf

    def set_option(self, name: str, value: int) -> int:
        """rsp_conv3d_set_option: a planning option of the convolution launchers (process-wide; e.g. "narrow_max_tiles").  Returns
        the previous value.  The per-geometry plan cache (kernel names, workspace sizes) is dropped with it."""
        prev = self.lib.rsp_conv3d_set_option(name.encode(), int(value))
        if prev < 0:
            _lib.check(prev, "rsp_conv3d_set_option")
        _conv_plan.cache_clear()
        executed_fraction.cache_clear()
        return prev

    @contextlib.contextmanager
    def options(self, **kw):
        """Planning options (set_option) for the length of a `with` block: sets each, then restores every one on the way out, an
        exception included, to what it was before (-1, i.e. the environment or the default, when the call showed no override).
        Caches: set_option drops the two that hold what the library PLANS per geometry — _conv_plan (kernel names, workspace sizes)
        and executed_fraction.  The row-geometry tables of _rowgeom_table stay: a table holds input offsets and validity bits per
        output position, a function of the geometry alone — "no_pad_skip" changes which chunks the kernels walk, not the table —
        and so do the pack signatures and the grow-only workspaces (sized per call from the fresh plan)."""
        before = {}
        try:
            for name, value in kw.items():
                prev = self.set_option(name, value)       # the effective value before
                self.set_option(name, -1)
                unset = self.set_option(name, value)      # ... and what the environment / the default gives
                before[name] = -1 if prev == unset else prev      # (prev differs from it only as an override)
            yield self
        finally:
            for name, value in before.items():
                self.set_option(name, value)

    # ---- conv -------------------------------------------------------------------------------------------------
    def conv_pack_fwd(self, g: ConvGeom, w_ref: torch.Tensor) -> torch.Tensor:
        _chk(w_ref, "w_ref")
        d = g.desc()
        n = self.lib.rsp_conv3d_packed_fwd_elems(C.byref(d))
        out = torch.empty(n, dtype=torch.float32, device=w_ref.device)
        _lib.check(self.lib.rsp_conv3d_pack_fwd(C.byref(d), _ptr(w_ref), _ptr(out), _stream()), "rsp_conv3d_pack_fwd")
        return out

    def conv_fwd(self, g: ConvGeom, x, w_packed, bias, want_stats: bool, out: Optional[torch.Tensor] = None,
                 out_ld: Optional[int] = None, in_ld: Optional[int] = None):
        _chk(x, "x")
        d, dref, tiles, wsb, _, _, (do, ho, wo), names = _conv_plan(g, in_ld, out_ld)
        if out is None:
            out = torch.empty((g.N, do, ho, wo, g.Cout), dtype=torch.float32, device=x.device)
        stats = None
        if want_stats:
            stats = torch.empty((tiles, g.Cout, 2), dtype=torch.float32, device=x.device)
        ws = self._workspace(x.device, wsb) if wsb else None
        e0 = self._ev()
        _lib.check(self.lib.rsp_conv3d_fwd(dref, _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(out), _ptr(stats),
                                           _ptr(ws), wsb, _stream()), "rsp_conv3d_fwd")
        self._log("conv_fwd", g, e0, names[0])
        return out, stats

    def stem_pooled_fwd(self, g: ConvGeom, x, w_packed, bias):
        """Stem convolution of a pass that keeps nothing, when only BatchNorm -> ReLU -> MaxPool(1,2,2) reads its output: the kernel
        leaves the window maximum and minimum of the raw output (a quarter of its size each) instead of the output itself —
        (y_max, y_min, stats) with the stats of conv_fwd, or None where the shape is not covered
        (rsp_conv3d_stem_pooled_applicable; the caller runs conv_fwd then).  bn_act_minmax_fwd finishes the unit."""
        _chk(x, "x")
        d, dref, tiles, _, _, _, (do, ho, wo), names = _conv_plan(g, None, None)
        if not _stem_pooled_ok(g) or x.data_ptr() % 16:
            return None
        ymax = torch.empty((g.N, do, ho // 2, wo // 2, g.Cout), dtype=torch.float32, device=x.device)
        ymin = torch.empty_like(ymax)
        stats = torch.empty((tiles, g.Cout, 2), dtype=torch.float32, device=x.device)
        e0 = self._ev()
        _lib.check(self.lib.rsp_conv3d_stem_pooled_fwd(dref, _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(ymax), _ptr(ymin), _ptr(stats),
                                                       _stream()), "rsp_conv3d_stem_pooled_fwd")
        self._log("conv_fwd", g, e0, names[0])
        return ymax, ymin, stats

    def bn_act_minmax_fwd(self, ymax, ymin, scale_shift, relu: bool, out=None):
        """BatchNorm apply (+ ReLU) of a unit whose window maximum / minimum stem_pooled_fwd left: what bn_act_pool_fwd gives on the
        full-size output (==, NaNs in the same places).  out: as bn_act_pool_fwd's."""
        _chk(ymax, "ymax")
        _chk(ymin, "ymin")
        if out is None:
            out = torch.empty_like(ymax)
        Cc = ymax.shape[-1]
        e0 = self._ev()
        _lib.check(self.lib.rsp_bn_act_minmax_fwd(_ptr(ymax), _ptr(ymin), ymax.numel() // Cc, Cc, _rows_ld(out, "out"), _ptr(scale_shift),
                                                  int(relu), _ptr(out), _stream()), "rsp_bn_act_minmax_fwd")
        self._log_hbm("bn_act_pool_fwd", 4 * (2 * ymax.numel() + out.numel()), e0)
        return out

    def conv_dgrad(self, g: ConvGeom, dy, w_ref):
        _chk(dy, "dy")
        _chk(w_ref, "w_ref")
        d, dref, _, _, wsb, _, _, names = _conv_plan(g, None, None)
        dx = torch.empty((g.N, g.Di, g.Hi, g.Wi, g.Cin), dtype=torch.float32, device=dy.device)
        ws = self._workspace(dy.device, wsb)
        e0 = self._ev()
        _lib.check(self.lib.rsp_conv3d_dgrad(dref, _ptr(dy), _ptr(w_ref), _ptr(dx), _ptr(ws), wsb, _stream()),
                   "rsp_conv3d_dgrad")
        self._log("conv_dgrad", g, e0, names[1])
        return dx

    def conv_dgrad_packed(self, g: ConvGeom, dy, w_packed):
        """dgrad over weights re-packed by a PackSet (which=1 entry)."""
        _chk(dy, "dy")
        d, dref, _, _, wsb, _, _, names = _conv_plan(g, None, None)
        dx = torch.empty((g.N, g.Di, g.Hi, g.Wi, g.Cin), dtype=torch.float32, device=dy.device)
        ws = self._workspace(dy.device, wsb)
        e0 = self._ev()
        _lib.check(self.lib.rsp_conv3d_dgrad_packed(dref, _ptr(dy), _ptr(_chk(w_packed, "w_packed")), _ptr(dx), _ptr(ws), wsb,
                                                    _stream()), "rsp_conv3d_dgrad_packed")
        self._log("conv_dgrad", g, e0, names[1])
        return dx

    def pack_signature(self, g: ConvGeom, which: int, w_ref):
        """Hashable identity of the packed layout `pack_set` would build for (g, which): the library's own job records with the
        pointers replaced by fixed dummies — equal for every input geometry that shares the layout."""
        return _pack_signature(g, which, int(w_ref.shape[0]), int(w_ref.shape[1]))

    def pack_set(self, entries):
        """entries: list of (ConvGeom, which, w_ref) with which = 0 (forward layout) / 1 (dgrad layouts) and w_ref the LIVE
        reference-layout weight tensor (it may have fewer channels than the geometry: zero padding).  Allocates the packed
        buffers and the device job table once; PackSet.run() re-packs all of them with one launch."""
        return PackSet(self, entries)

    def conv_wgrad(self, g: ConvGeom, x, dy, dw_out: torch.Tensor, dbias_out: Optional[torch.Tensor] = None):
        """dw_out (Cout,Cin,kT,kH,kW) and dbias_out are written in place (they are views of the flat grad buffer)."""
        _chk(x, "x")
        _chk(dw_out, "dw_out")
        dy_ld = _rows_ld(dy, "dy")                # dy may be a channel slice of a wider gradient tensor
        d, dref, _, _, _, wsb, _, names = _conv_plan(g, None, None if dy_ld == g.Cout else dy_ld)
        ws = self._workspace(x.device, wsb)
        if dw_out.shape[0] > g.Cout or dw_out.shape[1] > g.Cin or (dbias_out is not None and tuple(dw_out.shape[:2]) != (g.Cout, g.Cin)):
            raise _lib.RspError("conv_wgrad: dw_out has more channels than the geometry, or a bias gradient with padded channels")
        table = self._rowgeom_table(g, d, dref, x.device)
        e0 = self._ev()
        # (a geometry with zero-padded channels the parameter does not have: their gradients are dropped by the reduce)
        _lib.check(self.lib.rsp_conv3d_wgrad(dref, _ptr(x), _ptr(dy), _ptr(dw_out), _ptr(dbias_out), dw_out.shape[0], dw_out.shape[1],
                                             _ptr(table), _ptr(ws), wsb, _stream()), "rsp_conv3d_wgrad")
        self._log("conv_wgrad", g, e0, names[2])

    ROWGEOM_MAX_TABLES = 128
    ROWGEOM_MAX_BYTES = 2 << 30

    def _rowgeom_table(self, g: ConvGeom, d, dref, dev):
        """The weight-gradient kernels' per-row geometry table of this geometry (rsp_conv3d_rowgeom): computed once and kept — it
        depends on the positions only, not on channels or data.  None where the table-free path runs (kernel dims above 8).

        The table is filled on the stream that first needs it (often the engine's side-task stream) and then handed to weight
        gradients on ANY stream: the fill's event travels with the entry, and a caller on another stream waits for it until it has
        completed once.  The cache is bounded (count and bytes, least recently used first; ~8 bytes per output position, 50 MB for
        C3D's conv1): an evicted table is released behind every stream a table was ever handed to; tables baked into a captured
        graph's kernel arguments are never evicted."""
        if max(g.k) > 8:
            return None
        key = (dev, g.N, g.Di, g.Hi, g.Wi, g.k, g.s, g.p, d.in_ld)
        ent = self._rowgeom.get(key)
        capturing = torch.cuda.is_current_stream_capturing()
        here = _stream().value
        if ent is None:
            if capturing:
                return None                    # (first seen inside a capture: this call computes its own, the cache fills on the next eager step)
            nbytes = int(self.lib.rsp_conv3d_rowgeom_bytes(dref))
            t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(self.lib.rsp_conv3d_rowgeom(dref, _ptr(t), _stream()), "rsp_conv3d_rowgeom")
            ev = torch.cuda.Event()
            ev.record()
            ent = self._rowgeom[key] = [t, ev, here, False]
            self._rowgeom_bytes += nbytes
            self._rowgeom_evict(dev)
        else:
            self._rowgeom.move_to_end(key)
            if ent[1] is not None and not capturing:      # (a capture starts behind a device-wide synchronize; event queries are illegal inside)
                if ent[1].query():
                    ent[1] = None              # the fill is complete: visible to every stream from now on
                elif here != ent[2]:
                    torch.cuda.current_stream(dev).wait_event(ent[1])
            if capturing:
                ent[3] = True
        if here not in self._rowgeom_streams and not capturing:
            self._rowgeom_streams[here] = torch.cuda.current_stream(dev)
        return ent[0]

    def _rowgeom_evict(self, dev):
        if len(self._rowgeom) <= self.ROWGEOM_MAX_TABLES and self._rowgeom_bytes <= self.ROWGEOM_MAX_BYTES:
            return
        for key in list(self._rowgeom)[:-1]:           # never the entry just added
            if len(self._rowgeom) <= self.ROWGEOM_MAX_TABLES and self._rowgeom_bytes <= self.ROWGEOM_MAX_BYTES:
                break
            t, _, _, pinned = self._rowgeom[key]
            if pinned:
                continue
            for st in self._rowgeom_streams.values():  # a weight gradient on any of them may still be reading it
                t.record_stream(st)
            self._rowgeom_bytes -= t.numel()
            del self._rowgeom[key]

    # ---- batch norm -------------------------------------------------------------------------------------------
    def bn_finalize(self, stats, count: int, conv_bias, gamma, beta, eps: float, momentum: float, running_mean,
                    running_var, batch_stats_out=None):
        """batch_stats_out ([2][c_valid] view of a BnEmaSet): report this pass's batch moments there instead of moving the
        running statistics (deferred update, rsp_bn_running_update)."""
        tiles, Cc, _ = stats.shape
        if stats.is_contiguous():
            _chk(stats, "stats")
            stat_ld = Cc
        else:      # channel slice of a wider convolution's partials
            if not stats.is_cuda or stats.dtype != torch.float32 or stats.stride(2) != 1 or stats.stride(1) != 2 or stats.stride(0) % 2:
                raise _lib.RspError("stats: expected [tiles][C][2] float32 partials or a channel slice of them")
            stat_ld = stats.stride(0) // 2
        mi = torch.empty((2, Cc), dtype=torch.float32, device=stats.device)
        ss = torch.empty((2, Cc), dtype=torch.float32, device=stats.device)
        wsb = int(self.lib.rsp_bn_finalize_workspace(tiles, Cc))
        ws = self._workspace(stats.device, wsb)
        # the parameter vectors may be shorter than the convolution's (zero-padded) channel count: gamma's length says how many
        c_valid = Cc if gamma is None else int(gamma.shape[0])
        _lib.check(self.lib.rsp_bn_finalize(_ptr(stats), tiles, Cc, c_valid, stat_ld, count, _ptr(conv_bias), _ptr(gamma), _ptr(beta),
                                            eps, momentum, _ptr(running_mean), _ptr(running_var), _ptr(batch_stats_out), _ptr(mi),
                                            _ptr(ss), _ptr(ws), wsb, _stream()), "rsp_bn_finalize")
        return mi, ss

    def bn_ema_set(self, entries):
        """entries: list of (running_mean, running_var, momentum) of BatchNorm layers whose running-statistics update is deferred;
        returns a BnEmaSet: `.stats[i]` is the [2][C] buffer layer i's bn_finalize reports into, `.run()` applies all updates."""
        return BnEmaSet(self, entries)

    def bn_act_pool_fwd(self, pg: PoolGeom, y, scale_shift, residual, relu: bool, out=None):
        in_ld = _rows_ld(y, "y")             # y may be a channel slice of a wider conv output
        if out is None:
            do, ho, wo = pg.out_dims
            out = torch.empty((pg.N, do, ho, wo, pg.C), dtype=torch.float32, device=y.device)
        d, dref, _, _ = _pool_plan(pg, in_ld, _rows_ld(out, "out"), None if residual is None else _rows_ld(residual, "residual"))
        e0 = self._ev()
        _lib.check(self.lib.rsp_bn_act_pool_fwd(dref, _ptr(y), _ptr(scale_shift), _ptr(residual), int(relu), None, _ptr(out),
                                                _stream()), "rsp_bn_act_pool_fwd")
        n_in = pg.N * pg.Di * pg.Hi * pg.Wi * pg.C
        self._log_hbm("bn_act_pool_fwd", 4 * (n_in * (1 if residual is None else 2) + out.numel()), e0)
        return out

    def bn_act_pool_sel_fwd(self, pg: PoolGeom, y, scale_shift, relu: bool):
        """bn_act_pool_fwd of a pooled unit (disjoint windows of 4 or 8 positions, no residual) whose backward follows: (out, y_sel)
        with out as bn_act_pool_fwd's and y_sel the raw y at each window's selected position, which bn_act_pool_bwd takes as
        `y_sel` to read a pooled-size tensor in its reduce pass instead of all of y — or None where the shape is not covered."""
        in_ld = _rows_ld(y, "y")
        d, dref, _, (do, ho, wo) = _pool_plan(pg, in_ld, None, None)
        if not self.lib.rsp_bn_act_pool_sel_applicable(dref) or y.data_ptr() % 16 or scale_shift.data_ptr() % 16:
            return None
        out = torch.empty((pg.N, do, ho, wo, pg.C), dtype=torch.float32, device=y.device)
        ysel = torch.empty_like(out)
        e0 = self._ev()
        _lib.check(self.lib.rsp_bn_act_pool_sel_fwd(dref, _ptr(y), _ptr(scale_shift), int(relu), _ptr(out), _ptr(ysel), _stream()),
                   "rsp_bn_act_pool_sel_fwd")
        self._log_hbm("bn_act_pool_fwd", 4 * (pg.N * pg.Di * pg.Hi * pg.Wi * pg.C + 2 * out.numel()), e0)
        return out, ysel

    def bn_act_maxpool_fwd(self, pg: PoolGeom, y, scale_shift, relu: bool, keep: bool):
        """BatchNorm apply (+ ReLU) and an OVERLAPPING max-pool (the ResNet stems' 3x3x3 / 2 / 1) in one pass over the convolution
        output, with the arg-max a backward needs (keep) — (out, idx | None), or None when the shape is not covered
        (rsp_bn_act_maxpool_applicable; the caller runs bn_act_pool_fwd + maxpool_fwd then).  Same bits as those two."""
        in_ld = _rows_ld(y, "y")
        do, ho, wo = pg.out_dims
        d = pg.desc(in_ld=in_ld)
        if not self.lib.rsp_bn_act_maxpool_applicable(C.byref(d)) or y.data_ptr() % 16 or scale_shift.data_ptr() % 16:
            return None
        out = torch.empty((pg.N, do, ho, wo, pg.C), dtype=torch.float32, device=y.device)
        idx = torch.empty((pg.N, do, ho, wo, pg.C), dtype=torch.int32, device=y.device) if keep else None
        e0 = self._ev()
        _lib.check(self.lib.rsp_bn_act_maxpool_fwd(C.byref(d), _ptr(y), _ptr(scale_shift), int(relu), None, _ptr(out), _ptr(idx),
                                                   _stream()), "rsp_bn_act_maxpool_fwd")
        self._log_hbm("bn_act_pool_fwd", 4 * (pg.N * pg.Di * pg.Hi * pg.Wi * pg.C + out.numel() * (2 if keep else 1)), e0)
        return out, idx

    def bn_act_pool_bwd(self, pg: PoolGeom, y, residual, dout, gamma, mean_invstd, scale_shift, relu: bool,
                        want_dres: bool, dgamma_out, dbeta_out, dy_out=None, y_sel=None):
        """dy_out: where to write dy (same channel pitch as y — a slice of a wider gradient tensor when y is a slice).
        y_sel: what bn_act_pool_sel_fwd kept for this unit; the reduce pass then reads it instead of y (same bits)."""
        in_ld = _rows_ld(y, "y")
        d, dref, wsb, _ = _pool_plan(pg, in_ld, _rows_ld(dout, "dout"), None if residual is None else _rows_ld(residual, "residual"))
        dy = _dy_target(y, in_ld, dy_out)
        dres = torch.empty_like(y) if want_dres else None
        ws = self._workspace(y.device, wsb)
        c_valid = pg.C if gamma is None else int(gamma.shape[0])      # < C: zero-padded channels (gamma / dgamma / dbeta are short)
        e0 = self._ev()
        n_in = y.numel()
        if y_sel is not None:
            if residual is not None or want_dres:
                raise _lib.RspError("bn_act_pool_bwd: y_sel with a residual")
            _lib.check(self.lib.rsp_bn_act_pool_sel_bwd(dref, _ptr(y), _ptr(_chk(y_sel, "y_sel")), _ptr(dout), _ptr(gamma), _ptr(mean_invstd),
                                                        _ptr(scale_shift), int(relu), _ptr(dy), _ptr(dgamma_out), _ptr(dbeta_out), c_valid,
                                                        _ptr(ws), wsb, _stream()), "rsp_bn_act_pool_sel_bwd")
            # reduce pass: y_sel + dout read; apply pass: y + dout read, dy written
            self._log_hbm("bn_bwd(reduce+apply)", 4 * (y_sel.numel() + 2 * dout.numel() + 2 * n_in), e0)
            return dy, dres
        _lib.check(self.lib.rsp_bn_act_pool_bwd(dref, _ptr(y), _ptr(residual), _ptr(dout), _ptr(gamma),
                                                _ptr(mean_invstd), _ptr(scale_shift), int(relu), _ptr(dy), _ptr(dres),
                                                _ptr(dgamma_out), _ptr(dbeta_out), c_valid, None, None, _ptr(ws), wsb, _stream()),
                   "rsp_bn_act_pool_bwd")
        # reduce pass: y (+ residual) + dout read; apply pass: the same again, dy (+ dres) written
        self._log_hbm("bn_bwd(reduce+apply)", 4 * (2 * (n_in * (1 if residual is None else 2) + dout.numel()) + n_in * (2 if want_dres else 1)), e0)
        return dy, dres

    def bn_eval_act_pool_bwd(self, pg: PoolGeom, y, residual, dout, mean_invstd, scale_shift, relu: bool, want_dres: bool,
                             dgamma_out, dbeta_out, dy_out=None):
        """Backward of bn_act_pool_fwd on RUNNING statistics (eval-mode BatchNorm), one pass: dy = scale * dz, dres = dz, and — when
        asked for — dgamma = sum dz*xhat, dbeta = sum dz with xhat = (y - mean_invstd[0]) * mean_invstd[1].  scale_shift is what the
        forward applied; mean_invstd holds running_mean - conv_bias and rsqrt(running_var + eps).  dgamma_out / dbeta_out may be
        shorter than C (zero-padded channels: dy = 0 there).  dy_out as in bn_act_pool_bwd."""
        in_ld = _rows_ld(y, "y")
        d, dref, _, _ = _pool_plan(pg, in_ld, _rows_ld(dout, "dout"), None if residual is None else _rows_ld(residual, "residual"))
        dy = _dy_target(y, in_ld, dy_out)
        if want_dres and residual is None:
            raise _lib.RspError("want_dres without a residual")
        dres = torch.empty(y.shape, dtype=torch.float32, device=y.device) if want_dres else None
        if want_dres and d.res_ld != pg.C:
            raise _lib.RspError("residual: a residual whose gradient is wanted must be contiguous")
        sums = dgamma_out is not None or dbeta_out is not None
        c_valid = pg.C
        for v in (dgamma_out, dbeta_out):
            if v is not None:
                c_valid = int(v.shape[0])
        wsb = int(self.lib.rsp_bn_eval_bwd_workspace(dref)) if sums else 0
        ws = self._workspace(y.device, wsb) if sums else None
        e0 = self._ev()
        _lib.check(self.lib.rsp_bn_eval_act_pool_bwd(dref, _ptr(y), _ptr(residual), _ptr(dout), _ptr(mean_invstd), _ptr(scale_shift),
                                                     int(relu), _ptr(dy), _ptr(dres), _ptr(dgamma_out), _ptr(dbeta_out), c_valid,
                                                     _ptr(ws), wsb, _stream()), "rsp_bn_eval_act_pool_bwd")
        # one pass: y (+ residual) + dout read, dy (+ dres) written
        n_in = y.numel()
        self._log_hbm("bn_eval_bwd(one pass)", 4 * (n_in * (1 if residual is None else 2) + dout.numel() + n_in * (2 if want_dres else 1)), e0)
        return dy, dres

    # ---- stand-alone pooling / gating --------------------------------------------------------------------------
    def maxpool_fwd(self, pg: PoolGeom, x, keep: bool):
        do, ho, wo = pg.out_dims
        out = torch.empty((pg.N, do, ho, wo, pg.C), dtype=torch.float32, device=x.device)
        idx = torch.empty((pg.N, do, ho, wo, pg.C), dtype=torch.int32, device=x.device) if keep else None
        d = pg.desc(in_ld=_rows_ld(x, "x"))
        _lib.check(self.lib.rsp_maxpool3d_fwd(C.byref(d), _ptr(x), _ptr(out), _ptr(idx), _stream()), "rsp_maxpool3d_fwd")
        return out, idx

    def maxpool_bwd(self, pg: PoolGeom, dout, idx):
        dx = torch.empty((pg.N, pg.Di, pg.Hi, pg.Wi, pg.C), dtype=torch.float32, device=dout.device)
        d = pg.desc(out_ld=_rows_ld(dout, "dout"))
        _lib.check(self.lib.rsp_maxpool3d_bwd(C.byref(d), _ptr(dout), _ptr(idx), _ptr(dx), _stream()), "rsp_maxpool3d_bwd")
        return dx

    def gate_fwd(self, x, w, b, out=None):
        _chk(x, "x")
        N, D, H, W, Cc = x.shape
        P = D * H * W
        if out is None:
            out = torch.empty_like(x)
        mean = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
        gate = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
        wsb = self.lib.rsp_gate_fwd_workspace(N, P, Cc)
        ws = self._workspace(x.device, wsb)
        _lib.check(self.lib.rsp_gate_fwd(_ptr(x), N, P, Cc, Cc, _ptr(_chk(w, "w")), _ptr(_chk(b, "b")), _ptr(out),
                                         _rows_ld(out, "out"), _ptr(mean), _ptr(gate), _ptr(ws), wsb, _stream()),
                   "rsp_gate_fwd")
        return out, mean, gate

    gate_pool_keep = True      # bn_act_gate_fwd(pool=..., pool_idx=True): the pooled form can also write the pool's arg-max

    def bn_act_gate_fwd(self, pg: PoolGeom, y, scale_shift, relu: bool, w, b, keep_act: bool, pool: Optional[PoolGeom] = None,
                        out=None, pool_idx: bool = False):
        """BatchNorm-apply (+ReLU) and the self-gating unit behind it as one op (models/s3dg.py:52-72; pg: the unit-window
        geometry of y).  a = act(y*scale + shift); gate = sigmoid(W mean(a) + b); out = a * gate — through `pool` (a max-pool
        geometry over a's dims, models/s3dg.py:105-109) when given.  keep_act: also materialise a for the backward (then no pool).
        Returns (out, a | None, mean, gate).  Two passes over y instead of the five tensor passes of bn_act_pool_fwd + gate_fwd."""
        N, P, Cc = pg.N, pg.Di * pg.Hi * pg.Wi, pg.C
        y_ld = _rows_ld(y, "y")
        if keep_act and pool is not None:
            raise _lib.RspError("bn_act_gate_fwd: the pooled form keeps no activation")
        a = torch.empty((N, pg.Di, pg.Hi, pg.Wi, Cc), dtype=torch.float32, device=y.device) if keep_act else None
        mean = torch.empty((N, Cc), dtype=torch.float32, device=y.device)
        gate = torch.empty((N, Cc), dtype=torch.float32, device=y.device)
        wsb = self.lib.rsp_gate_fwd_workspace(N, P, Cc)
        ws = self._workspace(y.device, wsb)
        _lib.check(self.lib.rsp_bn_gate_sums(_ptr(y), N, P, Cc, y_ld, _ptr(scale_shift), int(relu), _ptr(a), Cc, _ptr(_chk(w, "w")),
                                             _ptr(_chk(b, "b")), _ptr(mean), _ptr(gate), _ptr(ws), wsb, _stream()), "rsp_bn_gate_sums")
        og = pool if pool is not None else pg
        if out is None:
            do, ho, wo = og.out_dims
            out = torch.empty((N, do, ho, wo, Cc), dtype=torch.float32, device=y.device)
        if keep_act:
            _lib.check(self.lib.rsp_gate_apply(_ptr(a), N, P, Cc, Cc, _ptr(gate), _ptr(out), _rows_ld(out, "out"), _stream()),
                       "rsp_gate_apply")
        elif pool_idx:
            # the pooled form for a forward a backward follows: the max-pool's arg-max written by the same pass (returned fifth);
            # the caller has checked bn_act_gate_pool_idx_ok
            d, dref, _, _ = _pool_plan(og, y_ld, _rows_ld(out, "out"), None)
            idx = torch.empty(tuple(out.shape), dtype=torch.int32, device=y.device)
            _lib.check(self.lib.rsp_bn_act_maxpool_fwd(dref, _ptr(y), _ptr(scale_shift), int(relu), _ptr(gate), _ptr(out), _ptr(idx),
                                                       _stream()), "rsp_bn_act_maxpool_fwd")
            return out, a, mean, gate, idx
        else:
            d, dref, _, _ = _pool_plan(og, y_ld, _rows_ld(out, "out"), None)
            _lib.check(self.lib.rsp_bn_act_pool_fwd(dref, _ptr(y), _ptr(scale_shift), None, int(relu), _ptr(gate), _ptr(out),
                                                    _stream()), "rsp_bn_act_pool_fwd")
        return out, a, mean, gate

    def bn_act_gate_pool_idx_ok(self, pool: PoolGeom, y, scale_shift) -> bool:
        """Whether bn_act_gate_fwd(pool=pool, pool_idx=True) is available for this shape (rsp_bn_act_maxpool_applicable)."""
        d = pool.desc(in_ld=_rows_ld(y, "y"))
        return bool(self.lib.rsp_bn_act_maxpool_applicable(C.byref(d))) and y.data_ptr() % 16 == 0 and scale_shift.data_ptr() % 16 == 0

    def bn_act_gate_bwd(self, pg: PoolGeom, y, dout, gamma, mean_invstd, scale_shift, relu: bool, w, mean, gate,
                        dgamma_out, dbeta_out, dw_out, db_out):
        """Backward of bn_act_gate_fwd(keep_act=False): dout is the gradient of the gated output (possibly a channel slice of
        a concat gradient).  Gate parameter gradients into dw_out / db_out, BatchNorm's into dgamma_out / dbeta_out; returns dy.
        The activation is recomputed from y, and the gate's data gradient dout*gate + dmean/P is formed inside the BatchNorm
        backward kernels: seven tensor passes instead of the nine of gate_bwd + bn_act_pool_bwd."""
        N, P, Cc = pg.N, pg.Di * pg.Hi * pg.Wi, pg.C
        _chk(y, "y")
        dout_ld = _rows_ld(dout, "dout")
        dmean = torch.empty((N, Cc), dtype=torch.float32, device=y.device)
        wsb = self.lib.rsp_gate_bwd_workspace(N, P, Cc)
        ws = self._workspace(y.device, wsb)
        _lib.check(self.lib.rsp_gate_bwd_params(_ptr(y), _ptr(scale_shift), int(relu), _ptr(dout), N, P, Cc, Cc, dout_ld, _ptr(_chk(w, "w")),
                                                _ptr(mean), _ptr(gate), _ptr(dw_out), _ptr(db_out), _ptr(dmean), _ptr(ws), wsb,
                                                _stream()), "rsp_gate_bwd_params")
        d, dref, wsb2, _ = _pool_plan(pg, Cc, dout_ld, None)
        ws2 = self._workspace(y.device, wsb2)
        dy = torch.empty_like(y)
        c_valid = pg.C if gamma is None else int(gamma.shape[0])
        _lib.check(self.lib.rsp_bn_act_pool_bwd(dref, _ptr(y), None, _ptr(dout), _ptr(gamma), _ptr(mean_invstd), _ptr(scale_shift),
                                                int(relu), _ptr(dy), None, _ptr(dgamma_out), _ptr(dbeta_out), c_valid, _ptr(gate),
                                                _ptr(dmean), _ptr(ws2), wsb2, _stream()), "rsp_bn_act_pool_bwd")
        return dy

    def gate_bwd(self, x, dout, w, mean, gate, dw_out, db_out):
        _chk(x, "x")
        N, D, H, W, Cc = x.shape
        P = D * H * W
        dx = torch.empty_like(x)
        wsb = self.lib.rsp_gate_bwd_workspace(N, P, Cc)
        ws = self._workspace(x.device, wsb)
        _lib.check(self.lib.rsp_gate_bwd(_ptr(x), _ptr(dout), N, P, Cc, Cc, _rows_ld(dout, "dout"), _ptr(w), _ptr(mean),
                                         _ptr(gate), _ptr(dx), Cc, _ptr(dw_out), _ptr(db_out), _ptr(ws), wsb, _stream()),
                   "rsp_gate_bwd")
        return dx

    # ---- heads / contrastive ----------------------------------------------------------------------------------
    def head_fwd(self, feat, w1, b1, w2, b2):
        _chk(feat, "feat")
        N, D, H, W, Cc = feat.shape
        P = D * H * W
        dim = w1.shape[0]
        dev = feat.device
        o1 = torch.empty((N, dim), dtype=torch.float32, device=dev)
        o2 = torch.empty((N, dim), dtype=torch.float32, device=dev)
        pooled = torch.empty((N, Cc), dtype=torch.float32, device=dev)
        raw = torch.empty((2, N, dim), dtype=torch.float32, device=dev)
        _lib.check(self.lib.rsp_head_fwd(_ptr(feat), N, P, Cc, Cc, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), dim, _ptr(o1),
                                         _ptr(o2), _ptr(pooled), _ptr(raw), _stream()), "rsp_head_fwd")
        return o1, o2, pooled, raw

    def head_bwd(self, d1, d2, pooled, raw, w1, w2, feat_shape, dw1, db1, dw2, db2):
        N, D, H, W, Cc = feat_shape
        P = D * H * W
        dim = w1.shape[0]
        dfeat = torch.empty(feat_shape, dtype=torch.float32, device=d1.device)
        wsb = self.lib.rsp_head_bwd_workspace(N, dim)
        ws = self._workspace(d1.device, wsb)
        _lib.check(self.lib.rsp_head_bwd(_ptr(_chk(d1, "d1")), _ptr(_chk(d2, "d2")), _ptr(pooled), _ptr(raw), _ptr(w1),
                                         _ptr(w2), N, P, Cc, Cc, dim, _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2),
                                         _ptr(dfeat), _ptr(ws), wsb, _stream()), "rsp_head_bwd")
        return dfeat

    # generic pieces of the 'mlp' head
    def spatial_mean_fwd(self, x):
        _chk(x, "x")
        N, D, H, W, Cc = x.shape
        mean = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.rsp_spatial_mean_fwd(_ptr(x), N, D * H * W, Cc, Cc, _ptr(mean), _stream()), "rsp_spatial_mean_fwd")
        return mean

    def spatial_mean_bwd(self, dmean, shape):
        N, D, H, W, Cc = shape
        dx = torch.empty(shape, dtype=torch.float32, device=dmean.device)
        _lib.check(self.lib.rsp_spatial_mean_bwd(_ptr(_chk(dmean, "dmean")), N, D * H * W, Cc, Cc, _ptr(dx), _stream()),
                   "rsp_spatial_mean_bwd")
        return dx

    def linear_fwd(self, x, w, b, relu: bool):
        B, Cin = x.shape
        y = torch.empty((B, w.shape[0]), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.rsp_linear_fwd(_ptr(_chk(x, "x")), B, Cin, _ptr(_chk(w, "w")), _ptr(b), w.shape[0], int(relu), _ptr(y),
                                           _stream()), "rsp_linear_fwd")
        return y

    def linear_bwd(self, x, y, dy, w, relu: bool, dw_out, db_out, want_dx=True):
        B, Cin = x.shape
        Cout = w.shape[0]
        dx = torch.empty_like(x) if want_dx else None
        wsb = self.lib.rsp_linear_bwd_workspace(B, Cout)
        ws = self._workspace(x.device, wsb)
        _lib.check(self.lib.rsp_linear_bwd(_ptr(x), _ptr(y), _ptr(_chk(dy, "dy")), _ptr(w), B, Cin, Cout, int(relu), _ptr(dx),
                                           _ptr(dw_out), _ptr(db_out), _ptr(ws), wsb, _stream()), "rsp_linear_bwd")
        return dx

    def l2norm_fwd(self, x):
        y = torch.empty_like(x)
        _lib.check(self.lib.rsp_l2norm_fwd(_ptr(_chk(x, "x")), x.shape[0], x.shape[1], _ptr(y), _stream()), "rsp_l2norm_fwd")
        return y

    def l2norm_bwd(self, x, dy):
        dx = torch.empty_like(x)
        _lib.check(self.lib.rsp_l2norm_bwd(_ptr(x), _ptr(_chk(dy, "dy")), x.shape[0], x.shape[1], _ptr(dx), _stream()),
                   "rsp_l2norm_bwd")
        return dx

    def logits_fwd(self, qA, qM, kA, kM, knegA, knegM, queue, inv_T: float):
        B, dim = qA.shape
        K = queue.shape[1]
        dev = qA.device
        for n, t in (("qA", qA), ("qM", qM), ("kA", kA), ("kM", kM), ("knegA", knegA), ("knegM", knegM), ("queue", queue)):
            _chk(t, n)
        l1 = torch.empty((B, K + 1), dtype=torch.float32, device=dev)
        l2 = torch.empty((B, K + 1), dtype=torch.float32, device=dev)
        lp = torch.empty((B, 1), dtype=torch.float32, device=dev)
        ln = torch.empty((B, 1), dtype=torch.float32, device=dev)
        _lib.check(self.lib.rsp_logits_fwd(_ptr(qA), _ptr(qM), _ptr(kA), _ptr(kM), _ptr(knegA), _ptr(knegM), _ptr(queue), B,
                                           dim, qM.shape[1], K, inv_T, _ptr(l1), _ptr(l2), _ptr(lp), _ptr(ln), _stream()),
                   "rsp_logits_fwd")
        return l1, l2, lp, ln

    def logits_bwd(self, dl1, dl2, dlp, dln, kA, kM, knegA, knegM, queue, inv_T: float):
        B, dim = kA.shape
        K = queue.shape[1]
        dev = kA.device
        dqA = torch.empty((B, dim), dtype=torch.float32, device=dev)
        dqM = torch.empty((B, kM.shape[1]), dtype=torch.float32, device=dev)
        wsb = self.lib.rsp_logits_bwd_workspace(B, dim, K)
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_logits_bwd(_ptr(_chk(dl1, "dl1")), _ptr(_chk(dl2, "dl2")), _ptr(_chk(dlp, "dlp")),
                                           _ptr(_chk(dln, "dln")), _ptr(kA), _ptr(kM), _ptr(knegA), _ptr(knegM), _ptr(queue),
                                           B, dim, kM.shape[1], K, inv_T, _ptr(dqA), _ptr(dqM), _ptr(ws), wsb, _stream()),
                   "rsp_logits_bwd")
        return dqA, dqM

    # ---- retrieval search (cos_search.hip, retrieval.hip) --------------------------------------------------------
    def cosine_topk(self, q, g, k: int, splits: int = 0):
        """The k nearest rows of g (Ng, D) for every row of q (Nq, D) by cosine distance: (idx int32 (Nq, k), dist fp32 (Nq, k)),
        best first; ties go to the lower gallery index; idx -1 / dist +inf past Ng.  Rows may be strided (unit column stride,
        even row pitch).  splits: gallery split count (0: automatic); the result does not depend on it."""
        Nq, Ng, D, ldq, ldg = _search_operands("cosine_topk", q, g)
        idx = torch.empty((Nq, k), dtype=torch.int32, device=q.device)
        dist = torch.empty((Nq, k), dtype=torch.float32, device=q.device)
        wsb = self.lib.rsp_cosine_topk_workspace(Nq, Ng, D, k, int(splits))
        ws = self._workspace(q.device, wsb)
        _lib.check(self.lib.rsp_cosine_topk(_ptr(q), ldq, Nq, _ptr(g), ldg, Ng, D, int(k), int(splits), _ptr(idx), _ptr(dist), _ptr(ws),
                                            wsb, _stream()), "rsp_cosine_topk")
        return idx, dist

    def topk_hits(self, idx, y_q, y_g, ks):
        """counts[i] = queries whose label is among the labels of their first ks[i] neighbours (int32 device vector)."""
        _chk(idx, "idx", torch.int32)
        _chk(y_q, "y_q", torch.int64)
        _chk(y_g, "y_g", torch.int64)
        ks_host = (C.c_int32 * len(ks))(*[int(x) for x in ks])
        counts = torch.empty(len(ks), dtype=torch.int32, device=idx.device)
        _lib.check(self.lib.rsp_topk_hits(_ptr(idx), idx.shape[0], idx.shape[1], _ptr(y_q), _ptr(y_g), y_g.shape[0], ks_host,
                                          len(ks), _ptr(counts), _stream()), "rsp_topk_hits")
        return counts

    # ---- weighted kNN classifier (cos_search.hip, knn.hip) ---------------------------------------------------------
    def knn_classify(self, q, g, y_g, k: int, T: float, num_classes: int, y_q=None, valid: Optional[int] = None, splits: int = 0,
                     want_idx: bool = False, want_votes: bool = False):
        """The k (1..256) cosine neighbours in g (Ng, D) of every row of q (Nq, D) vote for their class y_g with weight
        exp((s - 1) / T) (rsp_knn_classify; the search's ranking and tie rules, the Nq x Ng matrix never stored).  Returns the named
        tuple (pred int32 (Nq,), rank int32 (Nq,) | None, hits int32 (2,) | None, votes fp32 (Nq, num_classes) | None, idx int32
        (Nq, k) | None, dist fp32 (Nq, k) | None).  rank -- #classes that beat the query's own, ties to the lower class -- and hits
        -- rows i < valid with rank < 1 and rank < 5 -- come with y_q; votes / idx and dist when asked for.  Rows of q and g may be
        strided (unit column stride, even row pitch)."""
        Nq, Ng, D, ldq, ldg = _search_operands("knn_classify", q, g)
        _chk(y_g, "y_g", torch.int64)
        if y_g.numel() != Ng:
            raise _lib.RspError(f"knn_classify: {Ng} gallery rows, {y_g.numel()} labels")
        if y_q is not None:
            _chk(y_q, "y_q", torch.int64)
            if y_q.numel() != Nq:
                raise _lib.RspError(f"knn_classify: {Nq} query rows, {y_q.numel()} labels")
        elif valid is not None:
            raise _lib.RspError("knn_classify: valid counts hits, which need y_q")
        k, num_classes, dev = int(k), int(num_classes), q.device
        shaped = 1 <= k <= 256 and 1 <= num_classes <= 1024          # (the call itself rejects the rest, before any launch)
        pred = torch.empty(Nq, dtype=torch.int32, device=dev)
        rank = torch.empty(Nq, dtype=torch.int32, device=dev) if y_q is not None else None
        hits = torch.empty(2, dtype=torch.int32, device=dev) if y_q is not None else None
        votes = torch.empty((Nq, num_classes), dtype=torch.float32, device=dev) if want_votes and shaped else None
        idx = torch.empty((Nq, k), dtype=torch.int32, device=dev) if want_idx and shaped else None
        dist = torch.empty((Nq, k), dtype=torch.float32, device=dev) if want_idx and shaped else None
        wsb = int(self.lib.rsp_knn_classify_workspace(Nq, Ng, D, k, num_classes, int(splits))) if shaped else 0
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_knn_classify(_ptr(q), ldq, Nq, _ptr(y_q), _ptr(g), ldg, Ng, _ptr(y_g), D, k, float(T), num_classes,
                                             int(splits), Nq if valid is None else int(valid), _ptr(idx), _ptr(dist), _ptr(votes),
                                             _ptr(pred), _ptr(rank), _ptr(hits), _ptr(ws), wsb, _stream()), "rsp_knn_classify")
        return KnnResult(pred, rank, hits, votes, idx, dist)

    # ---- label-free representation statistics (repr_stats.hip) ------------------------------------------------------
    def repr_stats(self, x, t: float = 2.0, want_gram: bool = True):
        """The pair sums, the Gram matrix and the column sums of the rows of x (N, D) from one rsp_repr_stats call (the N x N matrix
        never stored; include/rspnet_hip.h states the rule).  Returns the named tuple (sums: the 40-byte rsp_repr_sums as a uint8
        device tensor -- pair sums of exp(2 t (s - 1)), s, s^2 over the valid pairs i < j, then the valid and invalid row counts --,
        gram fp64 (D, D) | None, colsum fp64 (D,) | None).  Rows may be strided (unit column stride, even row pitch)."""
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
            raise _lib.RspError("repr_stats: x must be a float32 HIP device matrix with unit column stride")
        N, D = x.shape
        ld, dev = x.stride(0) if N > 1 else D, x.device
        sums = torch.empty(C.sizeof(_lib.ReprSums), dtype=torch.uint8, device=dev)
        shaped = want_gram and 2 <= D <= 4096          # (the call itself rejects the rest, before any launch)
        gram = torch.empty((D, D), dtype=torch.float64, device=dev) if shaped else None
        colsum = torch.empty(D, dtype=torch.float64, device=dev) if shaped else None
        wsb = int(self.lib.rsp_repr_stats_workspace(N, D))
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_repr_stats(_ptr(x), ld, N, D, 2.0 * float(t), _ptr(sums), _ptr(gram), _ptr(colsum), _ptr(ws), wsb,
                                           _stream()), "rsp_repr_stats")
        return ReprResult(sums, gram, colsum)

    # ---- linear probe on frozen features (linear_probe.hip) ---------------------------------------------------------
    @staticmethod
    def _probe_x(who: str, x):
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
            raise _lib.RspError(f"{who}: x must be a float32 HIP device matrix with unit column stride")
        N, D = x.shape
        return N, D, x.stride(0) if N > 1 else D

    def linear_probe_fit(self, x, y, w, b, mom, lr, steps: int, batch: Optional[int] = None, first_step: int = 0,
                         momentum: float = 0.9, weight_decay: float = 1e-4, normalize: bool = True, scale: float = 8.0):
        """``steps`` SGD steps of the softmax classifier z = (x f) w^T + b on the rows of x (N, D) with labels y (N,) int64, all from
        one rsp_linear_probe_fit call (include/rspnet_hip.h states the rule).  w (C, D), b (C,) and mom (C * D + C,) are updated in
        place; lr: the device vector of learning rates, indexed by first_step + t.  Returns (loss_trace fp32 (steps,), counts int32
        (2,): valid and invalid rows).  Rows of x may be strided (unit column stride, even row pitch)."""
        N, D, ld = self._probe_x("linear_probe_fit", x)
        _chk(y, "y", torch.int64)
        for n, t in (("w", w), ("b", b), ("mom", mom), ("lr", lr)):
            _chk(t, n)
        Cc = w.shape[0]
        if w.dim() != 2 or w.shape[1] != D or b.numel() != Cc or mom.numel() != Cc * D + Cc or y.numel() != N:
            raise _lib.RspError(f"linear_probe_fit: x {tuple(x.shape)}, y {tuple(y.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}, "
                                f"mom {tuple(mom.shape)} do not fit")
        steps, first_step = int(steps), int(first_step)
        batch = N if batch is None else int(batch)
        if steps >= 1 and first_step >= 0 and lr.numel() < first_step + steps:
            raise _lib.RspError(f"linear_probe_fit: {lr.numel()} learning rates for steps up to {first_step + steps}")
        dev = x.device
        loss = torch.empty(max(steps, 1), dtype=torch.float32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        wsb = int(self.lib.rsp_linear_probe_workspace(N, D, Cc, batch))      # (0 for sizes the call itself rejects, before any launch)
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_linear_probe_fit(_ptr(x), ld, N, D, _ptr(y), Cc, batch, first_step, steps, _ptr(lr), float(momentum),
                                                 float(weight_decay), int(bool(normalize)), float(scale), _ptr(w), _ptr(b), _ptr(mom),
                                                 _ptr(loss), _ptr(counts), _ptr(ws), wsb, _stream()), "rsp_linear_probe_fit")
        return loss[:steps], counts

    def linear_probe_logits(self, x, w, b, normalize: bool = True, scale: float = 8.0):
        """logits (N, C) of the probe (w, b) on the rows of x (rsp_linear_probe_logits): NaN in every class of an invalid row."""
        N, D, ld = self._probe_x("linear_probe_logits", x)
        _chk(w, "w")
        _chk(b, "b")
        Cc = w.shape[0]
        if w.dim() != 2 or w.shape[1] != D or b.numel() != Cc:
            raise _lib.RspError(f"linear_probe_logits: x {tuple(x.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)} do not fit")
        logits = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
        wsb = int(self.lib.rsp_linear_probe_workspace(N, D, Cc, 1))
        ws = self._workspace(x.device, wsb)
        _lib.check(self.lib.rsp_linear_probe_logits(_ptr(x), ld, N, D, _ptr(w), _ptr(b), Cc, int(bool(normalize)), float(scale),
                                                    _ptr(logits), Cc, _ptr(ws), wsb, _stream()), "rsp_linear_probe_logits")
        return logits

    # ---- clustering evaluation (cluster.hip) -------------------------------------------------------------------------
    def kmeans_fit(self, x, cent, max_iters: int):
        """Spherical k-means on the rows of x (N, D) from the centroids cent (C, D), updated in place, all ``max_iters`` iterations from
        one rsp_kmeans_fit call (include/rspnet_hip.h states the rule).  Returns the named tuple (assign int32 (N,), counts int32
        (C,), changed int32 (max_iters,), objective fp64 (max_iters,), info: the 32-byte rsp_kmeans_info as a uint8 device tensor).
        Rows of x may be strided (unit column stride, even row pitch)."""
        N, D, ld = self._probe_x("kmeans_fit", x)
        _chk(cent, "cent")
        if cent.dim() != 2 or cent.shape[1] != D:
            raise _lib.RspError(f"kmeans_fit: x {tuple(x.shape)} and cent {tuple(cent.shape)} do not fit")
        Cc, iters, dev = cent.shape[0], int(max_iters), x.device
        assign = torch.empty(N, dtype=torch.int32, device=dev)
        counts = torch.empty(Cc, dtype=torch.int32, device=dev)
        changed = torch.empty(max(iters, 1), dtype=torch.int32, device=dev)
        objective = torch.empty(max(iters, 1), dtype=torch.float64, device=dev)
        info = torch.empty(C.sizeof(_lib.KmeansInfo), dtype=torch.uint8, device=dev)
        wsb = int(self.lib.rsp_kmeans_workspace(N, D, Cc))      # (0 for sizes the call itself rejects, before any launch)
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_kmeans_fit(_ptr(x), ld, N, D, _ptr(cent), Cc, iters, _ptr(assign), _ptr(counts), _ptr(changed),
                                           _ptr(objective), _ptr(info), _ptr(ws), wsb, _stream()), "rsp_kmeans_fit")
        return KmeansResult(assign, counts, changed[:iters], objective[:iters], info)

    def kmeans_assign(self, x, cent, want_sim: bool = True):
        """(assign int32 (N,), sim fp32 (N,) | None) of the rows of x against the centroids cent (rsp_kmeans_assign): the cosine
        search's single neighbour, -1 / NaN for an invalid row."""
        N, D, ld = self._probe_x("kmeans_assign", x)
        _chk(cent, "cent")
        if cent.dim() != 2 or cent.shape[1] != D:
            raise _lib.RspError(f"kmeans_assign: x {tuple(x.shape)} and cent {tuple(cent.shape)} do not fit")
        Cc, dev = cent.shape[0], x.device
        assign = torch.empty(N, dtype=torch.int32, device=dev)
        sim = torch.empty(N, dtype=torch.float32, device=dev) if want_sim else None
        wsb = int(self.lib.rsp_cosine_topk_workspace(N, Cc, D, 1, 0))
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_kmeans_assign(_ptr(x), ld, N, D, _ptr(cent), Cc, _ptr(assign), _ptr(sim), _ptr(ws), wsb, _stream()),
                   "rsp_kmeans_assign")
        return assign, sim

    def contingency(self, assign, y, num_clusters: int, num_classes: int):
        """(table int64 (num_clusters, num_classes), dropped int64 (1,)): table[c][l] = #{i: assign[i] == c, y[i] == l}; the rows
        with assign < 0 or a label outside [0, num_classes) are counted in dropped (rsp_contingency)."""
        _chk(assign, "assign", torch.int32)
        _chk(y, "y", torch.int64)
        if assign.dim() != 1 or y.numel() != assign.numel():
            raise _lib.RspError(f"contingency: {assign.numel()} assignments, {y.numel()} labels")
        Cc, L, dev = int(num_clusters), int(num_classes), assign.device
        shaped = 1 <= Cc <= 1024 and 1 <= L <= 1024          # (the call itself rejects the rest, before any launch)
        table = torch.empty((Cc, L) if shaped else (1, 1), dtype=torch.int64, device=dev)
        dropped = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(self.lib.rsp_contingency(_ptr(assign), _ptr(y), assign.numel(), Cc, L, _ptr(table), _ptr(dropped), _stream()),
                   "rsp_contingency")
        return table, dropped

    # ---- embedding maps (tsne.hip) ----------------------------------------------------------------------------------------
    def tsne_affinities(self, x, perplexity: float = 30.0, want_dmat: bool = False):
        """The joint t-SNE affinities of the rows of x (N, D) from one rsp_tsne_affinities call (include/rspnet_hip.h states the
        rule).  Returns the named tuple (pmat fp32 (N, N): p over the M listed rows in its top-left M x M, 0 elsewhere; rows int32
        (N,): the valid rows in ascending order, -1 behind; beta fp32 (N,) by rank, NaN behind; dmat fp32 (N, N) | None; info: the
        32-byte rsp_tsne_info as a uint8 device tensor).  Rows of x may be strided (unit column stride, even row pitch)."""
        N, D, ld = self._probe_x("tsne_affinities", x)
        dev = x.device
        shaped = 2 <= N <= 16384          # (the call itself rejects the rest, before any launch)
        n = N if shaped else 1
        pmat = torch.empty((n, n), dtype=torch.float32, device=dev)
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        beta = torch.empty(n, dtype=torch.float32, device=dev)
        dmat = torch.empty((n, n), dtype=torch.float32, device=dev) if want_dmat else None
        info = torch.empty(C.sizeof(_lib.TsneInfo), dtype=torch.uint8, device=dev)
        wsb = int(self.lib.rsp_tsne_affinities_workspace(N, D))      # (0 for sizes the call itself rejects)
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_tsne_affinities(_ptr(x), ld, N, D, float(perplexity), _ptr(pmat), n, _ptr(rows), _ptr(beta), _ptr(dmat),
                                                _ptr(info), _ptr(ws), wsb, _stream()), "rsp_tsne_affinities")
        return TsneAffinities(pmat, rows, beta, dmat, info)

    def tsne_fit(self, aff, sched, first_iter: int, iters: int, y, inc, gains):
        """``iters`` iterations of the t-SNE descent on the affinities ``aff`` (of tsne_affinities), all from one rsp_tsne_fit call.
        y, inc and gains (N, 2) fp32 are updated in place (the rows that are not listed are neither read nor written); sched
        (>= first_iter + iters, 4) fp32 on the device: lr, momentum, exaggeration and a pad word per iteration.  Returns kl_trace
        fp64 (iters,)."""
        N = aff.pmat.shape[0]
        for n, t in (("pmat", aff.pmat), ("sched", sched), ("y", y), ("inc", inc), ("gains", gains)):
            _chk(t, n)
        _chk(aff.rows, "rows", torch.int32)
        iters, first_iter = int(iters), int(first_iter)
        if any(tuple(t.shape) != (N, 2) for t in (y, inc, gains)) or sched.dim() != 2 or sched.shape[1] != 4:
            raise _lib.RspError(f"tsne_fit: y {tuple(y.shape)}, inc {tuple(inc.shape)}, gains {tuple(gains.shape)} must be ({N}, 2), "
                                f"sched {tuple(sched.shape)} (iterations, 4)")
        if iters >= 1 and first_iter >= 0 and sched.shape[0] < first_iter + iters:
            raise _lib.RspError(f"tsne_fit: {sched.shape[0]} schedule entries for iterations up to {first_iter + iters}")
        dev = y.device
        kl = torch.empty(max(iters, 1), dtype=torch.float64, device=dev)
        wsb = int(self.lib.rsp_tsne_fit_workspace(N))
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_tsne_fit(_ptr(aff.pmat), aff.pmat.stride(0), _ptr(aff.rows), _ptr(aff.info), N, _ptr(sched), first_iter,
                                         iters, _ptr(y), _ptr(inc), _ptr(gains), _ptr(kl), _ptr(ws), wsb, _stream()), "rsp_tsne_fit")
        return kl[:iters]

    # ---- fine-tune criterion, accuracy and meters (classify.hip) -------------------------------------------------
    def xent_metrics(self, logits, target, n_crop: int = 1, valid: Optional[int] = None, want_grad: bool = True, meters=None):
        """Crop mean, cross-entropy (loss and, with want_grad, its gradient with respect to the crop logits), top-1 / top-5
        accuracy over the first `valid` samples and the meter update, in one call (rsp_xent_metrics).  logits: (S * n_crop,
        classes) fp32 with unit column stride; target: (S,) int64; meters: the 36-byte device struct (uint8 tensor) or None.
        Returns (avg_logits (S, classes), loss (1,), acc (2,): acc1 / acc5 in percent, dlogits | None).  Ties go to the lower
        class index.  With fewer than 5 classes acc[1] is not written (undefined here), with valid = 0 neither element is."""
        if not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
            raise _lib.RspError("xent_metrics: logits must be a float32 HIP device matrix with unit column stride")
        _chk(target, "target", torch.int64)
        rows, classes = logits.shape
        if n_crop < 1 or rows % n_crop or target.numel() != rows // n_crop:
            raise _lib.RspError(f"xent_metrics: {rows} rows, n_crop {n_crop}, {target.numel()} targets do not fit")
        S = rows // n_crop
        if meters is not None:
            _chk(meters, "meters", torch.uint8)
            if meters.numel() < C.sizeof(_lib.ClsMeters):
                raise _lib.RspError("xent_metrics: meters must hold one rsp_cls_meters")
        dev = logits.device
        avg = torch.empty((S, classes), dtype=torch.float32, device=dev)
        dlogits = torch.empty((rows, classes), dtype=torch.float32, device=dev) if want_grad else None
        out = torch.empty(3, dtype=torch.float32, device=dev)
        wsb = int(self.lib.rsp_xent_metrics_workspace(rows, n_crop))
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_xent_metrics(_ptr(logits), rows, classes, logits.stride(0) if rows > 1 else classes, int(n_crop),
                                             _ptr(target), S if valid is None else int(valid), _ptr(avg), _ptr(dlogits),
                                             C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 4), _ptr(meters), _ptr(ws),
                                             wsb, _stream()), "rsp_xent_metrics")
        return avg, out[:1], out[1:], dlogits

    # ---- pretext accuracies and meters (pretext_metrics.hip) -----------------------------------------------------
    def pretext_metrics(self, logits1, logits2, lposM, lnegM, losses, meters_buf=None):
        """The pretext loop's per-step accuracies and its eight meter updates in one call (rsp_pretext_metrics).  logits1 / logits2:
        dense (B, K1) fp32 with the positive in column 0; lposM / lnegM: B fp32 each; losses: the (3,) fp32 (loss, loss_A, loss_M) of
        loss_fwd_bwd; meters_buf: the 96-byte device struct (uint8 tensor) or None.  Returns acc (5,): acc1_A, acc5_A, acc1_A_n,
        acc5_A_n, acc1_M in percent.  An exact tie with the positive goes to the positive; a NaN positive is a miss."""
        for n, t in (("logits1", logits1), ("logits2", logits2), ("l_pos_M", lposM), ("l_neg_M", lnegM), ("losses", losses)):
            _chk(t, n)
        if logits1.dim() != 2 or logits2.shape != logits1.shape:
            raise _lib.RspError(f"pretext_metrics: logits must be two (B, K1) matrices of one shape, got {tuple(logits1.shape)} and "
                                f"{tuple(logits2.shape)}")
        B, K1 = logits1.shape
        if lposM.numel() != B or lnegM.numel() != B or losses.numel() != 3:
            raise _lib.RspError(f"pretext_metrics: expected {B} ranking logits per side and 3 losses, got {lposM.numel()}, "
                                f"{lnegM.numel()} and {losses.numel()}")
        if meters_buf is not None:
            _chk(meters_buf, "meters", torch.uint8)
            if meters_buf.numel() < C.sizeof(_lib.PretextMeters):
                raise _lib.RspError("pretext_metrics: meters must hold one rsp_pretext_meters")
        dev = logits1.device
        acc = torch.empty(5, dtype=torch.float32, device=dev)
        wsb = int(self.lib.rsp_pretext_metrics_workspace(B))
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_pretext_metrics(_ptr(logits1), _ptr(logits2), _ptr(lposM), _ptr(lnegM), B, K1, _ptr(losses), _ptr(acc),
                                                _ptr(meters_buf), _ptr(ws), wsb, _stream()), "rsp_pretext_metrics")
        return acc

    # ---- step fingerprints (fingerprint.hip) ---------------------------------------------------------------------------
    def fingerprint(self, table, n_jobs: int, total_chunks: int, out):
        """One 32-byte record per job of a device-resident rsp_fingerprint_job table (rsp_fingerprint; rspnet_amd/fingerprint.py
        builds the table and reads the records).  table: uint8, n_jobs * 32 bytes; out: uint8, n_jobs * 32 bytes, every record written."""
        _chk(table, "table", torch.uint8)
        _chk(out, "out", torch.uint8)
        n_jobs, total_chunks = int(n_jobs), int(total_chunks)
        rec = C.sizeof(_lib.FingerprintRec)
        if n_jobs < 0 or table.numel() < n_jobs * C.sizeof(_lib.FingerprintJob) or out.numel() < n_jobs * rec:
            raise _lib.RspError(f"fingerprint: {n_jobs} jobs do not fit a table of {table.numel()} and records of {out.numel()} bytes")
        if total_chunks < 0 or table.device != out.device:
            raise _lib.RspError("fingerprint: total_chunks must not be negative, table and records on one device")
        wsb = int(self.lib.rsp_fingerprint_workspace(total_chunks))
        ws = self._workspace(out.device, wsb)
        _lib.check(self.lib.rsp_fingerprint(_ptr(table), n_jobs, total_chunks, _ptr(out), _ptr(ws), wsb, _stream()), "rsp_fingerprint")
        return out

    # ---- similarity maps and their picture panels (cam.hip) --------------------------------------------------------
    def cam_maps(self, feat_q, feat_k, k_row, w_qA, w_qM, w_kA, w_kM):
        """The four similarity maps of MoCoDiffLossTwoFc.cam_visualize from the two NDHWC feature maps (B, T', H', W', C) — dense, or
        channel slices of a wider tensor — in one call (rsp_cam_maps).  k_row: (B,) int32, the row of feat_k that pairs with sample b.
        Returns (4, B, T', H', W') fp32, order qA, qM, kA, kM."""
        ld_q, ld_k = _rows_ld(feat_q, "feat_q"), _rows_ld(feat_k, "feat_k")
        if feat_q.dim() != 5 or feat_q.shape != feat_k.shape:
            raise _lib.RspError(f"cam_maps: feature maps must be two (B, T', H', W', C) tensors of one shape, got "
                                f"{tuple(feat_q.shape)} and {tuple(feat_k.shape)}")
        B, D, H, W, Cc = feat_q.shape
        P = D * H * W
        _chk(k_row, "k_row", torch.int32)
        if k_row.numel() != B:
            raise _lib.RspError(f"cam_maps: k_row must hold {B} rows, not {k_row.numel()}")
        for n, w, like in (("w_qA", w_qA, w_kA), ("w_qM", w_qM, w_kM), ("w_kA", w_kA, w_qA), ("w_kM", w_kM, w_qM)):
            _chk(w, n)
            if w.dim() != 2 or w.shape[1] != Cc or w.shape != like.shape:
                raise _lib.RspError(f"cam_maps: {n} must be (dim, {Cc}) and match the other encoder's, got {tuple(w.shape)}")
        dev = feat_q.device
        out = torch.empty((4, B, D, H, W), dtype=torch.float32, device=dev)
        wsb = int(self.lib.rsp_cam_maps_workspace(B, Cc))
        ws = self._workspace(dev, wsb)
        _lib.check(self.lib.rsp_cam_maps(_ptr(feat_q), ld_q, _ptr(feat_k), ld_k, _ptr(k_row), B, P, Cc, _ptr(w_qA), _ptr(w_qM),
                                         _ptr(w_kA), _ptr(w_kM), w_qA.shape[0], w_qM.shape[0], _ptr(out), _ptr(ws), wsb, _stream()),
                   "rsp_cam_maps")
        return out

    def cam_overlay(self, maps, clip_a, clip_b, t: int):
        """N picture panels (N, size, size, 3) uint8 RGB in one launch (rsp_cam_overlay): maps (N, T', H', W') fp32; frame `t` of
        sample n % B of the un-normalised [0, 1] clip (B, 3, T, size, size) under panel n — clip_a for the first half of the panels,
        clip_b for the second (clip_b None: clip_a for all)."""
        _chk(maps, "maps")
        _chk(clip_a, "clip_a")
        if maps.dim() != 4 or clip_a.dim() != 5 or clip_a.shape[1] != 3 or clip_a.shape[3] != clip_a.shape[4]:
            raise _lib.RspError(f"cam_overlay: expected maps (N, T', H', W') and clips (B, 3, T, size, size), got {tuple(maps.shape)} "
                                f"and {tuple(clip_a.shape)}")
        if clip_b is not None and (_chk(clip_b, "clip_b").shape != clip_a.shape):
            raise _lib.RspError("cam_overlay: the two clips must have one shape")
        N, Tp, Hp, Wp = maps.shape
        B, _, T, size, _ = clip_a.shape
        out = torch.empty((N, size, size, 3), dtype=torch.uint8, device=maps.device)
        _lib.check(self.lib.rsp_cam_overlay(_ptr(maps), N, Tp, Hp, Wp, _ptr(clip_a), _ptr(clip_b), B, T, int(t), size, _ptr(out),
                                            _stream()), "rsp_cam_overlay")
        return out

    def loss_fwd_bwd(self, l1, l2, lp, ln, margin: float, A: float, M: float):
        B, K1 = l1.shape
        dev = l1.device
        for n, t in (("logits1", l1), ("logits2", l2), ("l_pos_M", lp), ("l_neg_M", ln)):
            _chk(t, n)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        d1 = torch.empty_like(l1)
        d2 = torch.empty_like(l2)
        dp = torch.empty_like(lp)
        dn = torch.empty_like(ln)
        scratch = torch.empty(2 * B, dtype=torch.float32, device=dev)
        _lib.check(self.lib.rsp_loss_fwd_bwd(_ptr(l1), _ptr(l2), _ptr(lp), _ptr(ln), B, K1, margin, A, M, _ptr(losses),
                                             _ptr(d1), _ptr(d2), _ptr(dp), _ptr(dn), _ptr(scratch), _stream()),
                   "rsp_loss_fwd_bwd")
        return losses, d1, d2, dp, dn

    def queue_enqueue(self, queue, ptr: int, keys):
        dim, K = queue.shape
        _lib.check(self.lib.rsp_queue_enqueue(_ptr(_chk(queue, "queue")), dim, K, ptr, _ptr(_chk(keys, "keys")),
                                              keys.shape[0], _stream()), "rsp_queue_enqueue")

    def queue_enqueue_dev(self, queue, queue_ptr, keys):
        """queue[:, ptr:ptr+n] = keys.T with ptr read from / advanced in the device buffer `queue_ptr` (int64, 1 element)."""
        dim, K = queue.shape
        _chk(queue_ptr, "queue_ptr", torch.int64)
        _lib.check(self.lib.rsp_queue_enqueue_dev(_ptr(_chk(queue, "queue")), dim, K, _ptr(queue_ptr), _ptr(_chk(keys, "keys")),
                                                  keys.shape[0], _stream()), "rsp_queue_enqueue_dev")

    # ---- glue -------------------------------------------------------------------------------------------------
    def clip_gather(self, im, src, step, T_out: int, c_out: Optional[int] = None):
        _chk(im, "im")
        _chk(src, "src", torch.int32)
        _chk(step, "step", torch.int32)
        B_in, Cc, T_in, H, W = im.shape
        B_out = src.shape[0]
        c_out = c_out or Cc
        out = torch.empty((B_out, T_out, H, W, c_out), dtype=torch.float32, device=im.device)
        e0 = self._ev()
        _lib.check(self.lib.rsp_clip_gather(_ptr(im), B_in, Cc, T_in, H, W, _ptr(src), _ptr(step), B_out, T_out, c_out, _ptr(out),
                                            _stream()), "rsp_clip_gather")
        self._log_hbm("clip_gather", 4 * (B_out * T_out * H * W * Cc + out.numel()), e0)
        return out

    def clip_gather_multi(self, jobs, T_out: int, c_out: Optional[int] = None):
        """jobs: [(im, src, step)] of ONE geometry (same clip shape, same number of output clips) -> their gathered clips, from one
        launch (rsp_clip_gather_multi)."""
        im0, src0, _ = jobs[0]
        B_in, Cc, T_in, H, W = im0.shape
        B_out = src0.shape[0]
        c_out = c_out or Cc
        outs = []
        for im, src, step in jobs:
            _chk(im, "im")
            _chk(src, "src", torch.int32)
            _chk(step, "step", torch.int32)
            if tuple(im.shape) != tuple(im0.shape) or src.shape[0] != B_out or step.shape[0] != B_out:
                raise _lib.RspError("clip_gather_multi: the jobs must share one geometry")
            outs.append(torch.empty((B_out, T_out, H, W, c_out), dtype=torch.float32, device=im.device))
        n = len(jobs)
        arr = C.c_void_p * n
        e0 = self._ev()
        _lib.check(self.lib.rsp_clip_gather_multi(n, arr(*[j[0].data_ptr() for j in jobs]), arr(*[j[1].data_ptr() for j in jobs]),
                                                  arr(*[j[2].data_ptr() for j in jobs]), arr(*[o.data_ptr() for o in outs]), B_in, Cc,
                                                  T_in, H, W, B_out, T_out, c_out, _stream()), "rsp_clip_gather_multi")
        self._log_hbm("clip_gather", 4 * n * (B_out * T_out * H * W * Cc + outs[0].numel()), e0)
        return outs

    def momentum_update(self, k_flat, q_flat, m: float):
        e0 = self._ev()
        _lib.check(self.lib.rsp_momentum_update(_ptr(_chk(k_flat, "k")), _ptr(_chk(q_flat, "q")), k_flat.numel(), m,
                                                _stream()), "rsp_momentum_update")
        self._log_hbm("momentum_update", 4 * 3 * k_flat.numel(), e0)

    def sgd_step(self, p, g, buf, lr: float, mu: float, wd: float, gscale: float, first: bool):
        e0 = self._ev()
        _lib.check(self.lib.rsp_sgd_step(_ptr(_chk(p, "p")), _ptr(_chk(g, "g")), _ptr(_chk(buf, "buf")), p.numel(), lr, mu,
                                         wd, gscale, int(first), _stream()), "rsp_sgd_step")
        self._log_hbm("sgd_step", 4 * 5 * p.numel(), e0)

    def rows_gather(self, x, idx):
        _chk(x, "x")
        _chk(idx, "idx", torch.int32)
        n, width = idx.shape[0], x.shape[1]
        out = torch.empty((n, width), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.rsp_rows_gather(_ptr(x), _ptr(idx), n, width, _ptr(out), _stream()), "rsp_rows_gather")
        return out

    def eltwise(self, op: str, a, b=None, out=None):
        """op in relu_fwd / relu_bwd / sigmoid_fwd / sigmoid_bwd / add; dense tensors, `out` may alias an input."""
        code = {"relu_fwd": 0, "relu_bwd": 1, "sigmoid_fwd": 2, "sigmoid_bwd": 3, "add": 4}[op]
        _chk(a, "a")
        if b is not None:
            _chk(b, "b")
            if b.shape != a.shape:
                raise _lib.RspError(f"eltwise {op}: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
        if out is None:
            out = torch.empty_like(a)
        _lib.check(self.lib.rsp_eltwise(code, _ptr(a), _ptr(b), _ptr(_chk(out, "out")), a.numel(), _stream()), "rsp_eltwise")
        return out

    # ---- clip augmentation ---------------------------------------------------------------------------
    def augment_batch(self, descs, n_clips, T, size, mean, std, out, blur9=None):
        """descs: uint8 device tensor holding n_clips rsp_augment_clip_desc records; out: (n_clips, 3, T, size, size) f32."""
        _chk(descs, "descs", torch.uint8)
        _chk(out, "out")
        assert descs.numel() >= n_clips * C.sizeof(_lib.AugmentClipDesc) and out.is_contiguous()
        assert out.numel() == n_clips * 3 * T * size * size
        nbytes = int(self.lib.rsp_augment_workspace(n_clips, T, size))
        ws = self._workspace(out.device, nbytes)
        m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        b9 = None if blur9 is None else (C.c_float * 9)(*blur9)
        _lib.check(self.lib.rsp_augment_batch(_ptr(descs), n_clips, T, size, m3, s3, b9, _ptr(out), 3 * T * size * size, _ptr(ws),
                                              ws.numel(), _stream()), "rsp_augment_batch")
        return out


class BnEmaSet:
    """Batch moments of a list of BatchNorm layers (one flat buffer) + the device-resident job table of their deferred
    running-statistics update (rsp_bn_running_update: one launch for all layers)."""

    def __init__(self, be: "HipOps", entries):
        self.be = be
        dev = entries[0][0].device
        sizes = [int(rm.shape[0]) for rm, _, _ in entries]
        self.flat = torch.zeros(2 * sum(sizes), dtype=torch.float32, device=dev)
        self.stats, self.ptrs, jobs, off = [], [], [], 0
        for (rm, rv, mom), c in zip(entries, sizes):
            _chk(rm, "running_mean")
            _chk(rv, "running_var")
            v = self.flat[off:off + 2 * c].view(2, c)
            self.stats.append(v)
            self.ptrs.append((rm.data_ptr(), rv.data_ptr()))
            jobs.append(bytes(_lib.BnEmaJob(rm.data_ptr(), rv.data_ptr(), v.data_ptr(), c, float(mom))))
            off += 2 * c
        self.keep = [e[:2] for e in entries]
        self.max_c, self.n = max(sizes), len(sizes)
        self.table = torch.frombuffer(bytearray(b"".join(jobs)), dtype=torch.uint8).to(dev)

    def run(self):
        _lib.check(self.be.lib.rsp_bn_running_update(_ptr(self.table), self.n, self.max_c, _stream()), "rsp_bn_running_update")


class PackSet:
    """Persistent packed copies of a set of convolution weights + the device-resident job tables that rebuild them.
    Forward-layout and dgrad-layout jobs run as two launches: packing both layouts of the SAME weight concurrently reads it in
    two conflicting patterns and is several times slower than the two passes back to back (tools/pack_probe.py: 31 + 62 us
    apart, 221 us together on a 512x512x27 filter)."""

    def __init__(self, be: "HipOps", entries):
        self.be = be
        self.packed = []
        jobs = {0: [], 1: []}
        self.max_blocks = {0: 0, 1: 0}
        dev = None
        for g, which, w_ref in entries:
            _chk(w_ref, "w_ref")
            dev = w_ref.device
            d = g.desc()
            n = (be.lib.rsp_conv3d_packed_dgrad_elems if which else be.lib.rsp_conv3d_packed_fwd_elems)(C.byref(d))
            out = torch.empty(n, dtype=torch.float32, device=dev)
            buf = (_lib.PackJob * 64)()
            cnt = be.lib.rsp_conv3d_pack_jobs(C.byref(d), which, w_ref.shape[0], w_ref.shape[1], _ptr(w_ref), _ptr(out), buf, 64)
            if cnt < 0:
                _lib.check(cnt, "rsp_conv3d_pack_jobs")
            kind = 1 if which else 0
            jobs[kind].extend(bytes(buf)[i * C.sizeof(_lib.PackJob):(i + 1) * C.sizeof(_lib.PackJob)] for i in range(cnt))
            self.max_blocks[kind] = max([self.max_blocks[kind]] + [int(buf[i].blocks) for i in range(cnt)])
            self.packed.append(out)
        self.sources = [e[2] for e in entries]            # keep the weights (and their storage) alive
        self.tables = {}
        for kind, js in jobs.items():
            if js:
                self.tables[kind] = (torch.frombuffer(bytearray(b"".join(js)), dtype=torch.uint8).to(dev), len(js))

    def run(self):
        for kind, (table, n) in self.tables.items():
            _lib.check(self.be.lib.rsp_pack_run(_ptr(table), n, self.max_blocks[kind], _stream()), "rsp_pack_run")

    def __del__(self):
        # the library keeps a per-address note about packed stem buffers (three real input channels): withdrawn with the buffers
        try:
            for t in self.packed:
                self.be.lib.rsp_conv3d_pack_forget(_ptr(t))
        except Exception:      # noqa: BLE001 - interpreter shutdown: the library may be gone
            pass


_backend = None


def backend():
    """The active op backend; instantiates HipOps (and therefore requires the built library) on first use."""
    global _backend
    if _backend is None:
        _backend = HipOps()
    return _backend


def set_backend(b):
    """TEST HOOK ONLY: swap the op backend (tests/cpu_ops.py).  Returns the previous one."""
    global _backend
    prev, _backend = _backend, b
    return prev
