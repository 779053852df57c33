"""Step fingerprints: one 32-byte record per tensor -- an exact bit hash, sum of squares, sum of magnitudes, largest magnitude and
the count of non-finite elements -- for any list of device tensors from ONE HIP call (rsp_fingerprint, csrc/fingerprint.hip), and
what a training driver builds on it: a NaN guard that names the tensor, a cross-rank parameter check, and a per-step file that says
whether two runs computed the same bits (tools/fingerprint_diff.py).  The project's own: the reference has nothing like it.

The record (``REC_DTYPE`` mirrors rsp_fingerprint_rec), with w_i the i-th 32-bit word of the tensor and v_i the same word as fp32:

    hash       sum_i fmix32((w_i + i * 0x9E3779B1) mod 2^32) mod 2^64, fmix32 = murmur3's 32-bit finaliser.  The finaliser is a
               bijection, so a change of any single word always changes the hash; several simultaneous changes escape with
               probability about 2^-32 per tensor.  The position enters, so a swap of two unequal elements is seen.
    nonfinite  words whose exponent field is all ones (they stay in the hash and are left out of the float fields)
    sumsq, sum_abs   fp64;  max_abs   exact fp32 maximum of |v| over the finite elements

``reference_records`` restates the kernel in numpy, summation order included: both give the same 32 bytes for the same values, so
a file written on the checker backend of the CPU tests compares with one written on the GPU.  It is also what this layer runs when
the active op backend has no ``fingerprint`` (that checker backend) -- the arrangement xent_metrics and pretext_metrics have.

This module imports neither driver."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, ops

CHUNK = 8192                      # RSP_FP_CHUNK: 32-bit words per partial
VERSION = 1
FILE_NAME = "fingerprints.jsonl"
REC_DTYPE = np.dtype([("hash", "<u8"), ("sumsq", "<f8"), ("sum_abs", "<f8"), ("max_abs", "<f4"), ("nonfinite", "<u4")])
assert REC_DTYPE.itemsize == C.sizeof(_lib.FingerprintRec) == 32 and C.sizeof(_lib.FingerprintJob) == 32
_THREADS, _GROUPS = 256, CHUNK // (4 * 256)
_BLOCK_CHUNKS = 512               # reference_records works through a tensor this many chunks at a time (bounds its memory)


# ---- the definition in numpy ---------------------------------------------------------------------------------------------
def _words_and_kind(t) -> Tuple[np.ndarray, int]:
    """A tensor (torch, any device; or numpy) as its little-endian 32-bit words + the job kind: fp32 -> 0, int64 / uint32 -> 1."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(t)
    if a.dtype == np.float32:
        return a.reshape(-1).view(np.uint32), 0
    if a.dtype == np.int64:
        return a.reshape(-1).astype("<i8", copy=False).view(np.uint32), 1
    if a.dtype == np.uint32:
        return a.reshape(-1), 1
    raise TypeError(f"fingerprint: fp32 (kind 0) and int64 (kind 1) tensors only, got {a.dtype}")


def _fmix32(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def _butterfly(v: np.ndarray, op) -> np.ndarray:
    """The wave's xor butterfly over the last axis (64 lanes), offsets 32 .. 1; lane 0 of the result."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., lanes ^ o])
    return v[..., 0]


def _chunk_partials(w: np.ndarray, first_index: int, floats: bool):
    """Kernel 1 over a whole number of chunks (the last may be short): per chunk (hash, sumsq, sum_abs, max_abs, nonfinite)."""
    n = w.size
    nch = -(-n // CHUNK)
    pad = nch * CHUNK - n
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(first_index)).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = _fmix32(w + idx * np.uint32(0x9E3779B1)).astype(np.uint64)
    h = np.concatenate([h, np.zeros(pad, np.uint64)]).reshape(nch, CHUNK).sum(axis=1, dtype=np.uint64)      # exact in any order
    if not floats:
        z = np.zeros(nch)
        return h, z, z, np.zeros(nch, np.float32), np.zeros(nch, np.uint32)
    bad = (w & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    mag = (w & np.uint32(0x7FFFFFFF)).view(np.float32).copy()
    mag[bad] = 0.0                                                    # (adding +0.0 to a non-negative sum changes no bit)
    mag = np.concatenate([mag, np.zeros(pad, np.float32)])
    nonfinite = np.concatenate([bad, np.zeros(pad, bool)]).reshape(nch, CHUNK).sum(axis=1).astype(np.uint32)
    mx = mag.reshape(nch, CHUNK).max(axis=1)
    # element j of a chunk belongs to thread (j / 4) % 256, each thread adds in index order: [chunk][group][thread][k] -> 32 steps
    d = mag.astype(np.float64).reshape(nch, _GROUPS, _THREADS, 4).transpose(0, 2, 1, 3).reshape(nch, _THREADS, _GROUPS * 4)
    sq, ab = np.zeros((nch, _THREADS)), np.zeros((nch, _THREADS))
    for s in range(_GROUPS * 4):
        x = d[:, :, s]
        sq = sq + x * x                                               # x * x is exact in fp64: one rounding, as the kernel's fma
        ab = ab + x
    out = []
    for v in (sq, ab):
        wv = _butterfly(v.reshape(nch, 4, 64), np.add)                # per wave, then the four waves in wave order
        out.append(((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3])
    return h, out[0], out[1], mx, nonfinite


def _finish(parts) -> tuple:
    """Kernel 2 over one job's partials: lane l adds chunks l, l + 64, ... in order, then the butterfly."""
    h, sq, ab, mx, nf = parts
    nch = h.size
    rows = -(-nch // 64)
    res = []
    for v in (sq, ab):
        p = np.concatenate([v, np.zeros(rows * 64 - nch)]).reshape(rows, 64)
        acc = np.zeros(64)
        for r in range(rows):
            acc = acc + p[r]
        res.append(float(_butterfly(acc, np.add)))
    return (int(h.sum(dtype=np.uint64)), res[0], res[1], np.float32(mx.max() if nch else 0.0), int(nf.sum(dtype=np.uint64)))


def reference_records(tensors: Iterable) -> np.ndarray:
    """The records of `tensors` (torch tensors on any device, or numpy arrays: fp32 -> kind 0, int64 / uint32 words -> kind 1) from
    the definition, in numpy on host copies -- the same bits the kernel gives, the two doubles included."""
    tensors = list(tensors)
    out = np.zeros(len(tensors), dtype=REC_DTYPE)
    for s, t in enumerate(tensors):
        w, kind = _words_and_kind(t)
        if w.size >= 1 << 31:
            raise ValueError("fingerprint: a tensor must have fewer than 2^31 words")
        if w.size == 0:
            continue
        parts = [_chunk_partials(w[b:b + _BLOCK_CHUNKS * CHUNK], b, kind == 0) for b in range(0, w.size, _BLOCK_CHUNKS * CHUNK)]
        out[s] = _finish(tuple(np.concatenate(c) for c in zip(*parts)))
    return out


# ---- the device call ---------------------------------------------------------------------------------------------------------
def _kind(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.int64:
        return 1
    raise TypeError(f"fingerprint: fp32 (kind 0) and int64 (kind 1) tensors only, got {t.dtype}")


class FingerprintSet:
    """A named list of tensors + the device-resident job table of their fingerprint call (built as ops.BnEmaSet builds its table).
    ``run()`` enqueues ONE rsp_fingerprint call on the current stream and returns the device (n, 32) uint8 records; ``read()`` is
    the only host sync.  Tensors whose storage moves between calls (the fine-tune gradients are fresh allocations every backward)
    are handed to ``run(tensors)``: the table is re-uploaded from pinned memory, non-blocking, only when an address changed.

    On an op backend without ``fingerprint`` (the torch checker backend of the CPU tests) ``run`` evaluates ``reference_records``."""

    def __init__(self, names: Sequence[str], tensors: Sequence[torch.Tensor]):
        self.names = list(names)
        self.be = ops.backend()
        self.native = hasattr(self.be, "fingerprint")
        self.records = None
        self._table = self._host = self._uploaded = None
        self._ptrs: List[int] = []
        self._set(list(tensors), first=True)

    def _set(self, tensors: List[torch.Tensor], first: bool = False):
        if len(tensors) != len(self.names):
            raise ValueError(f"fingerprint: {len(self.names)} names, {len(tensors)} tensors")
        kinds, words = [], []
        for name, t in zip(self.names, tensors):
            k = _kind(t)
            if not t.is_contiguous():
                raise ValueError(f"fingerprint: {name} is not contiguous")
            n = t.numel() * (2 if k else 1)
            if n >= 1 << 31:
                raise ValueError(f"fingerprint: {name} has 2^31 words or more")
            if self.native and not t.is_cuda:
                raise _lib.RspError(f"fingerprint: {name}: expected a HIP device tensor (rspnet_amd has no CPU path)")
            kinds.append(k)
            words.append(n)
        if first:
            self.kinds, self.words = kinds, words
            self.chunk0, c = [], 0
            for n in words:
                self.chunk0.append(c)
                c += -(-n // CHUNK)
            self.total_chunks = c
        elif kinds != self.kinds or words != self.words:
            raise ValueError("fingerprint: the tensors handed to run() must keep the sizes and types the set was built with")
        self.tensors = [t.detach() for t in tensors]            # keeps the storage alive
        if not self.native or not tensors:
            return
        ptrs = [t.data_ptr() for t in tensors]
        if ptrs == self._ptrs:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fingerprint: a tensor moved; the job table cannot be rebuilt inside a graph capture")
        dev = tensors[0].device
        if self._host is None:
            self._host = torch.empty(32 * len(tensors), dtype=torch.uint8).pin_memory()
            self._table = torch.empty(32 * len(tensors), dtype=torch.uint8, device=dev)
        elif self._uploaded is not None:
            self._uploaded.synchronize()                        # the previous upload has read the pinned table
        jobs = b"".join(bytes(_lib.FingerprintJob(p, n, c0, k, 0)) for p, n, c0, k in zip(ptrs, self.words, self.chunk0, self.kinds))
        self._host.copy_(torch.frombuffer(bytearray(jobs), dtype=torch.uint8))
        self._table.copy_(self._host, non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record()
        self._ptrs = ptrs

    def run(self, tensors: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
        if tensors is not None:
            self._set(list(tensors))
        n = len(self.names)
        if not self.native:
            rec = reference_records(self.tensors)
            self.records = torch.from_numpy(rec.view(np.uint8).reshape(n, 32).copy())
            return self.records
        if n == 0:
            self.records = torch.empty((0, 32), dtype=torch.uint8)
            return self.records
        out = torch.empty((n, 32), dtype=torch.uint8, device=self._table.device)
        self.be.fingerprint(self._table, n, self.total_chunks, out)
        self.records = out
        return out

    def read(self) -> np.ndarray:
        """The records of the last ``run`` as a structured array (``REC_DTYPE``): the host waits for the call here."""
        if self.records is None:
            raise RuntimeError("fingerprint: read() before run()")
        return self.records.cpu().numpy().reshape(-1).view(REC_DTYPE).copy()


# ---- what to fingerprint -----------------------------------------------------------------------------------------------------
def _unwrap(model):
    return getattr(model, "module", model)


def named_gradients(model) -> List[Tuple[str, torch.Tensor]]:
    """(name, p.grad) of every parameter that has a gradient (in the pretext model: the views of g_flat)."""
    return [(n, p.grad) for n, p in _unwrap(model).named_parameters() if p.grad is not None]


def named_parameters(model) -> List[Tuple[str, torch.Tensor]]:
    return [(n, p.detach()) for n, p in _unwrap(model).named_parameters()]


def named_state(model) -> List[Tuple[str, torch.Tensor]]:
    """The entries of state_dict(): parameters and buffers.  fp32 is hashed with its norms, int64 counters (num_batches_tracked,
    queue_ptr) as raw words; anything else raises."""
    out = []
    for n, t in _unwrap(model).state_dict().items():
        _kind(t)
        out.append((n, t.detach()))
    return out


def totals(records: np.ndarray) -> dict:
    """One line for a whole list: hash = sum_s hash_s * (2 s + 1) mod 2^64 (so two tensors swapping their contents is seen), norm =
    sqrt(sum of sumsq), sum_abs, max_abs and nonfinite over the list, in list order."""
    h, sq, ab = 0, 0.0, 0.0
    for s, r in enumerate(records):
        h = (h + int(r["hash"]) * (2 * s + 1)) & 0xFFFFFFFFFFFFFFFF
        sq += float(r["sumsq"])
        ab += float(r["sum_abs"])
    return {"hash": h, "norm": math.sqrt(sq), "sum_abs": ab, "max_abs": float(records["max_abs"].max()) if len(records) else 0.0,
            "nonfinite": int(records["nonfinite"].sum(dtype=np.uint64))}


def _few(names: Sequence[str], limit: int = 8) -> str:
    """At most `limit` names in list order: all of them, or the first and the last limit / 2 around an ellipsis."""
    names = list(names)
    if len(names) <= limit:
        return ", ".join(names)
    return ", ".join(names[:limit // 2]) + ", ..., " + ", ".join(names[-(limit // 2):])


def check_ranks(records: np.ndarray, names: Sequence[str], group=None):
    """Every rank holds the same bits in these tensors, or RuntimeError on EVERY rank.  One int64 per rank is all-gathered (the
    total hash); only on a mismatch the per-tensor hashes follow, and the message names the first differing tensors and the ranks
    that hold each value.  Meant for parameters: BatchNorm running statistics legitimately differ between sync_buffers() calls."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    world = dist.get_world_size(group)
    if world <= 1:
        return
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    mine = torch.from_numpy(np.array([totals(records)["hash"]], dtype=np.uint64).view(np.int64)).to(dev)
    got = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(got, mine, group=group)
    if all(torch.equal(g, got[0]) for g in got):
        return
    per = torch.from_numpy(np.ascontiguousarray(records["hash"]).view(np.int64).copy()).to(dev)
    every = [torch.zeros_like(per) for _ in range(world)]
    dist.all_gather(every, per, group=group)
    table = torch.stack(every).cpu().numpy().view(np.uint64)            # [rank][tensor]
    bad = [s for s in range(table.shape[1]) if len(set(table[:, s].tolist())) > 1]
    lines = []
    for s in bad[:8]:
        by_value = {}
        for r in range(world):
            by_value.setdefault(int(table[r, s]), []).append(r)
        lines.append(f"{names[s]}: " + ", ".join(f"ranks {rs} hold {v:016x}" for v, rs in by_value.items()))
    raise RuntimeError(f"fingerprint: {len(bad)} of {len(names)} tensors differ between the {world} ranks; the first: " + "; ".join(lines))


# ---- the drivers' hook -------------------------------------------------------------------------------------------------------
def _side(records: np.ndarray) -> dict:
    t = totals(records)
    t["hash"] = f"{t['hash']:016x}"
    t["tensors"] = [f"{int(h):016x}" for h in records["hash"]]
    return t


class StepFingerprints:
    """Every `every`-th global step: the gradient records after the backward (with ``halt_on_nonfinite``: FloatingPointError naming
    the tensors that hold a NaN / Inf, before the optimizer has touched a parameter), the state records after the step (parameters
    checked across ranks), one line in RUN_DIR/fingerprints.jsonl on rank 0.  Nothing is launched on a step that is not due."""

    def __init__(self, run_dir, every: int, halt_on_nonfinite: bool = False, rank: int = 0, group=None):
        self.every, self.halt, self.rank, self.group = int(every), bool(halt_on_nonfinite), int(rank), group
        self.path = None if run_dir is None or self.rank != 0 else os.path.join(str(run_dir), FILE_NAME)
        self.global_step = 0
        self._sets = {}
        self._grad = None
        self._header_done = False

    @classmethod
    def from_config(cls, cfg, run_dir, rank: int = 0, group=None) -> Optional["StepFingerprints"]:
        """The ``fingerprint`` key of a driver config ({"every": N, "halt_on_nonfinite": bool}); None -- nothing constructed, no call
        ever issued -- when the key is absent or ``every`` is 0."""
        node = cfg.get("fingerprint") if hasattr(cfg, "get") else None
        if not node or int(node.get("every", 0)) <= 0:
            return None
        return cls(run_dir, int(node["every"]), bool(node.get("halt_on_nonfinite", False)), rank, group)

    def due(self, global_step: int) -> bool:
        self.global_step = int(global_step)
        return self.every > 0 and self.global_step % self.every == 0

    def _records(self, which: str, named) -> Tuple[List[str], np.ndarray]:
        names, tensors = [n for n, _ in named], [t for _, t in named]
        fs = self._sets.get(which)
        if fs is None or fs.names != names:
            fs = self._sets[which] = FingerprintSet(names, tensors)
            fs.run()
        else:
            fs.run(tensors)
        return names, fs.read()

    def after_backward(self, model):
        names, rec = self._records("grad", named_gradients(model))
        self._grad = (names, rec)
        if self.halt and int(rec["nonfinite"].sum(dtype=np.uint64)) > 0:
            bad = [n for n, r in zip(names, rec) if r["nonfinite"] > 0]
            raise FloatingPointError(f"fingerprint: non-finite gradient at global step {self.global_step}: "
                                     f"{int(rec['nonfinite'].sum(dtype=np.uint64))} elements in {len(bad)} of {len(names)} tensors: {_few(bad)}")
        return rec

    def after_step(self, epoch: int, step: int, model, global_step: Optional[int] = None):
        if global_step is not None:
            self.global_step = int(global_step)
        names, rec = self._records("state", named_state(model))
        params = {n for n, _ in _unwrap(model).named_parameters()}
        keep = [i for i, n in enumerate(names) if n in params]
        check_ranks(rec[keep], [names[i] for i in keep], self.group)
        grad, self._grad = self._grad, None
        self._write(epoch, step, grad, (names, rec))
        return rec

    def _write(self, epoch, step, grad, state):
        if self.path is None:
            return
        header = {"version": VERSION, "chunk": CHUNK, "names": {"grad": list(grad[0]) if grad else [], "state": list(state[0])}}
        if not self._header_done:
            if os.path.exists(self.path) and os.path.getsize(self.path) > 0:
                with open(self.path) as f:
                    if json.loads(f.readline()) != header:
                        raise RuntimeError(f"{self.path} was started for another list of tensors")
            else:
                with open(self.path, "w") as f:
                    f.write(json.dumps(header) + "\n")
            self._header_done = True
        line = {"epoch": int(epoch), "step": int(step), "global_step": self.global_step,
                "grad": _side(grad[1]) if grad else None, "state": _side(state[1])}
        with open(self.path, "a") as f:
            f.write(json.dumps(line) + "\n")


# ---- reading the file (tools/fingerprint_diff.py) ----------------------------------------------------------------------------
def load_file(path) -> Tuple[dict, List[dict]]:
    with open(path) as f:
        lines = [json.loads(l) for l in f if l.strip()]
    if not lines or lines[0].get("version") != VERSION or "names" not in lines[0]:
        raise ValueError(f"{path}: not a fingerprint file of version {VERSION}")
    return lines[0], lines[1:]


def first_difference(a_path, b_path):
    """None when the two files hold the same records (over the shorter one's length), else (index, global_step, {"grad": [names],
    "state": [names]}) of the first record that differs.  Headers that disagree raise ValueError."""
    (ha, ra), (hb, rb) = load_file(a_path), load_file(b_path)
    if ha != hb:
        raise ValueError(f"the headers of {a_path} and {b_path} disagree: the two runs fingerprinted different lists of tensors")
    for i, (x, y) in enumerate(zip(ra, rb)):
        if x.get("global_step") != y.get("global_step"):
            raise ValueError(f"record {i}: global_step {x.get('global_step')} against {y.get('global_step')}: the runs were sampled differently")
        diff = {}
        for side in ("grad", "state"):
            sx, sy = x.get(side), y.get(side)
            if sx == sy:
                continue
            if sx is None or sy is None:
                diff[side] = ["<missing on one side>"]
                continue
            names = ha["names"][side]
            diff[side] = [names[j] for j, (p, q) in enumerate(zip(sx["tensors"], sy["tensors"])) if p != q] or ["<totals only>"]
        if diff:
            return i, x["global_step"], diff
    return None
