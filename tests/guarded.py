"""Guarded memory for the kernel tests: every operand inside a larger allocation that the test owns.

    with Guarded(DEV) as G:
        x = G.put(cpu_tensor)              # an input: [front band | payload | back band], bands and payload start as 0xFF bytes
        out = G.alloc(shape, dtype)        # an output the test hands to a kernel
        ... run the op (its own outputs and workspaces come from G too: rspnet_amd.ops.torch is a proxy meanwhile) ...
        G.check()

A store outside an operand lands in a band (a changed byte), a store into an input changes its recorded bits, an output element
nobody wrote still holds the word 0xFFFFFFFF (a NaN no arithmetic produces; int32 -1), and a read outside an operand brings that NaN
into the result, where the test's own comparison fails on it.  Nothing here can fault: every such access stays inside the block.

The payload pointer is 16-byte aligned and not 32-byte aligned (skew=16, the conv / BatchNorm family's contract); skew=8 gives the
search kernels' 8-byte alignment, skew=4 the 4-byte alignment of the kernels that promise a float pointer and no more (an element
of 8 bytes and a byte buffer the op allocates itself still start on 8: what the allocator and the header give them).  ops_module may be a list: every module
named has its `torch` replaced (rspnet_amd.fingerprint allocates its table and records itself; rspnet_amd.ops the workspace).
Not a conftest, no pytest settings: a helper the guarded tests import."""
import os
import sys

import torch

FILL = 0xFF
BAND_MIN, BAND_MAX = 64 << 10, 4 << 20
_HERE = os.path.abspath(__file__)


class GuardError(AssertionError):
    pass


class _Block:
    __slots__ = ("name", "block", "band", "nbytes", "payload", "kind", "bits", "proxy", "dtype", "partial")


class _TorchProxy:
    """Stands in for the `torch` module inside rspnet_amd.ops: forwards every attribute, routes device allocations to the guard."""

    def __init__(self, guard):
        object.__setattr__(self, "_guard", guard)

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)

    def _mine(self, device, kw):
        return device is not None and self._guard._same_device(device) and not kw.get("pin_memory") \
            and kw.get("layout", torch.strided) == torch.strided and not kw.get("requires_grad")

    def empty(self, *size, **kw):
        if not self._mine(kw.get("device"), kw) or "out" in kw:
            return torch.empty(*size, **kw)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        return self._guard.alloc(size, kw.get("dtype") or torch.get_default_dtype(), _proxy=True)

    def zeros(self, *size, **kw):
        if not self._mine(kw.get("device"), kw) or "out" in kw:
            return torch.zeros(*size, **kw)
        return self.empty(*size, **kw).zero_()

    def empty_like(self, t, **kw):
        if not self._mine(kw.get("device", t.device), kw):
            return torch.empty_like(t, **kw)
        meta = torch.empty_like(t, device="meta", **{k: v for k, v in kw.items() if k != "device"})
        flat = self._guard.alloc((meta.numel(),), meta.dtype, _proxy=True)
        return flat.view(meta.shape) if meta.is_contiguous() else flat.as_strided(meta.shape, meta.stride())


class Guarded:
    def __init__(self, device, skew=16, hip=None, ops_module=None):
        """hip: the backend whose workspace is guarded (default: rspnet_amd.ops.backend() on a HIP device, none on the CPU);
        ops_module: the module, or the list of modules, whose `torch` is replaced (default: rspnet_amd.ops)."""
        self.device = torch.device(device)
        assert skew in (4, 8, 16), skew
        self.skew = skew
        self.blocks = []
        if ops_module is None:
            from rspnet_amd import ops as ops_module
        self._modules = list(ops_module) if isinstance(ops_module, (list, tuple)) else [ops_module]
        if hip is None and self.device.type == "cuda":
            from rspnet_amd import ops
            hip = ops.backend()
        self._hip = hip

    # ---- activation ---------------------------------------------------------------------------------------------------
    def __enter__(self):
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Guarded: refusing to activate while a stream is capturing")
        self._saved_torch = [m.torch for m in self._modules]
        proxy = _TorchProxy(self)
        for m in self._modules:
            m.torch = proxy
        hip = self._hip
        if hip is not None:
            self._saved_ws = hip._ws
            self._had_own_workspace = "_workspace" in vars(hip)
            self._saved_workspace = hip._workspace
            hip._ws = {}
            inner = self._saved_workspace

            def workspace(dev, nbytes):
                buf = inner(dev, nbytes)
                buf.fill_(FILL)                  # (on the current stream, in front of the kernel that uses it)
                return buf
            hip._workspace = workspace
        return self

    def __exit__(self, *exc):
        for m, saved in zip(self._modules, self._saved_torch):
            m.torch = saved
        hip = self._hip
        if hip is not None:
            hip._ws = self._saved_ws
            if self._had_own_workspace:
                hip._workspace = self._saved_workspace
            else:
                del hip._workspace               # (the instance attribute: the class's method shows again)
        return False

    def _same_device(self, device):
        d = torch.device(device)
        if d.type != self.device.type:
            return False
        if d.type != "cuda":
            return True
        return (d.index if d.index is not None else torch.cuda.current_device()) == \
               (self.device.index if self.device.index is not None else torch.cuda.current_device())

    # ---- allocations --------------------------------------------------------------------------------------------------
    def _call_site(self):
        f = sys._getframe(1)
        while f is not None and (os.path.abspath(f.f_code.co_filename) == _HERE or f.f_code.co_name == "<lambda>"):
            f = f.f_back
        if f is None:
            return "?"
        return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})"

    def alloc(self, shape, dtype=torch.float32, name=None, _proxy=False):
        shape = tuple(int(s) for s in ((shape,) if isinstance(shape, int) else shape))
        itemsize = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * itemsize
        b = _Block()
        b.name = name or self._call_site()
        # (a byte buffer an op allocates is a workspace, a job table or a record array: structs with 8-byte members)
        skew = max(self.skew, 8) if itemsize > self.skew or (_proxy and dtype == torch.uint8) else self.skew
        band = (min(max(nbytes, BAND_MIN), BAND_MAX) + 63) // 64 * 64 + skew
        block = torch.full((2 * band + nbytes,), FILL, dtype=torch.uint8, device=self.device)
        b.block, b.band, b.nbytes = block, band, nbytes
        b.payload = block[band:band + nbytes]
        b.proxy, b.dtype = _proxy, dtype
        b.kind = "workspace" if "(_workspace)" in b.name else ("output" if _proxy else "operand")
        b.bits = None
        b.partial = False
        self.blocks.append(b)
        return b.payload.view(dtype).view(shape)

    def block_of(self, t):
        """The block whose payload holds the first element of t."""
        p = t.data_ptr()
        for b in self.blocks:
            if b.payload.data_ptr() <= p < b.payload.data_ptr() + max(b.nbytes, 1):
                return b
        raise KeyError("not a guarded tensor")

    def allow_unwritten(self, t):
        """An op's output that its contract leaves partly untouched (the test says which words, and looks at them itself)."""
        self.block_of(t).partial = True

    def empty(self, *shape, dtype=torch.float32):
        """alloc with torch.empty's way of giving the size: empty(2, 3) or empty((2, 3))."""
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        return self.alloc(shape, dtype)

    def put(self, cpu_tensor, name=None):
        name = name or self._call_site()
        src = cpu_tensor.detach().contiguous()
        t = self.alloc(src.shape, src.dtype, name=name)
        t.copy_(src)
        b = self.blocks[-1]
        b.kind = "input"
        b.bits = b.payload.clone()
        return t

    # ---- the check ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _first_and_count(bad):
        idx = bad.nonzero()
        return int(idx[0]), int(idx.numel())

    def check(self):
        """One synchronisation, then every block: bands intact, inputs unchanged, float32 outputs of the op fully written."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        probes = []
        for b in self.blocks:
            front, back = b.block[:b.band], b.block[b.band + b.nbytes:]
            probes.append((front != FILL).any())
            probes.append((back != FILL).any())
            probes.append((b.payload != b.bits).any() if b.bits is not None else torch.zeros((), dtype=torch.bool, device=self.device))
            written = b.proxy and b.kind == "output" and b.nbytes and b.dtype == torch.float32 and not b.partial
            probes.append((b.payload.view(torch.int32) == -1).any() if written
                          else torch.zeros((), dtype=torch.bool, device=self.device))
        if not probes:
            return
        flags = torch.stack(probes).cpu().view(-1, 4).tolist()
        report = []
        for b, (f, k, c, u) in zip(self.blocks, flags):
            if f:
                first, n = self._first_and_count(b.block[:b.band] != FILL)
                report.append(f"{b.kind} {b.name}: front band written, first bad byte at offset {first - b.band} of the payload, "
                              f"{n} bytes (payload {b.nbytes} bytes)")
            if k:
                first, n = self._first_and_count(b.block[b.band + b.nbytes:] != FILL)
                report.append(f"{b.kind} {b.name}: back band written, first bad byte at offset {b.nbytes + first} of the payload, "
                              f"{n} bytes (payload {b.nbytes} bytes)")
            if c:
                first, n = self._first_and_count(b.payload != b.bits)
                report.append(f"{b.kind} {b.name}: input changed, first bad byte at offset {first} of the payload, {n} bytes "
                              f"(payload {b.nbytes} bytes)")
            if u:
                first, n = self._first_and_count(b.payload.view(torch.int32) == -1)
                report.append(f"{b.kind} {b.name}: never written, first bad byte at offset {4 * first} of the payload, "
                              f"{n} elements (payload {b.nbytes} bytes)")
        if report:
            raise GuardError("guarded memory: " + str(len(report)) + " finding(s)\n  " + "\n  ".join(report))
