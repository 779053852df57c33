"""Shared by the linear-probe tests: seeded clustered inputs, the fp64 reference computed once per case, the error measures and
their gate."""
import functools

import numpy as np

from rspnet_amd import linear_probe

GATE = 2e-5      # the GPU suite's per-kernel gate

# (N, D, C, batch, steps): the trajectory cases
TRAJECTORIES = [(300, 34, 7, 300, 100), (300, 34, 7, 64, 100), (129, 30, 5, 64, 100), (600, 70, 101, 600, 100), (700, 70, 300, 256, 120)]
FULL_BATCH = [(300, 34, 7), (129, 30, 5), (600, 70, 101)]


@functools.lru_cache(maxsize=None)
def case_inputs(N, D, C, held_out=0):
    """(x, y, x2, y2): C standard-normal class means, uniform labels, x = mean[y] + N(0, 1) + 0.7 * (one shared standard-normal
    direction), fp32; x2 / y2: ``held_out`` more rows drawn the same way from the same means."""
    rng = np.random.default_rng(1000 * N + D)
    means = rng.standard_normal((C, D))
    y = rng.integers(0, C, size=N)
    noise = rng.standard_normal((N, D))
    shared = rng.standard_normal((1, D))
    x = (means[y] + noise + 0.7 * shared).astype(np.float32)
    y2 = rng.integers(0, C, size=held_out)
    x2 = (means[y2] + rng.standard_normal((held_out, D)) + 0.7 * shared).astype(np.float32)
    for a in (x, y, x2, y2):
        a.setflags(write=False)
    return x, y, x2, y2


@functools.lru_cache(maxsize=None)
def trajectory_reference(N, D, C, batch, steps, held_out=0):
    """The defaults of linear_probe.fit from zeros, on the rows in their order: (ProbeRef, fp64 logits of the training rows)."""
    x, y, x2, _ = case_inputs(N, D, C, held_out)
    ref = linear_probe.probe_reference(x, y, C, linear_probe.lr_schedule(0.125, steps), steps, batch, x2=x2 if held_out else None)
    return ref, linear_probe.reference_logits(ref.w, ref.b, x)


@functools.lru_cache(maxsize=None)
def step_state(N, D, C):
    """A random nonzero state (w, b, mom) for the one-step cases."""
    rng = np.random.default_rng(7 + 1000 * N + 10 * D + C)
    w = (0.1 * rng.standard_normal((C, D))).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    mom = (0.01 * rng.standard_normal(C * D + C)).astype(np.float32)
    for a in (w, b, mom):
        a.setflags(write=False)
    return w, b, mom


@functools.lru_cache(maxsize=None)
def step_reference(N, D, C):
    """One full-batch step with first_step = 1 (the momentum term is live), lr[1] = 0.125."""
    x, y, _, _ = case_inputs(N, D, C)
    w, b, mom = step_state(N, D, C)
    return linear_probe.probe_reference(x, y, C, np.array([9.0, 0.125], dtype=np.float32), 1, N, w0=w, b0=b, mom0=mom, first_step=1)


def errors(w, b, trace, ref, mom=None):
    """max|dW| / max|W| and max|db| / max|W| (b moves with W: one scale for the classifier), max|d loss_trace| (absolute),
    max|d mom| / max|mom|."""
    wmax = max(float(np.abs(ref.w).max()), 1e-300)
    e = {"w": float(np.abs(np.asarray(w, dtype=np.float64) - ref.w).max()) / wmax,
         "b": float(np.abs(np.asarray(b, dtype=np.float64) - ref.b).max()) / wmax,
         "loss": float(np.abs(np.asarray(trace, dtype=np.float64) - ref.loss_trace).max())}
    if mom is not None:
        e["mom"] = float(np.abs(np.asarray(mom, dtype=np.float64) - ref.mom).max()) / max(float(np.abs(ref.mom).max()), 1e-300)
    return e


def check(w, b, trace, ref, what="", mom=None):
    """Prints every figure, then asserts the gate; returns the errors."""
    e = errors(w, b, trace, ref, mom)
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v <= GATE, (what, k, v)      # (a NaN fails the comparison)
    return e


def hits(logits, y):
    """(hits1, hits5) of fp64 logits: rank = #{c: z[c] > z[t]} + #{c < t: z[c] == z[t]}; a NaN row is a miss."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(y)
    zt = z[np.arange(len(y)), y][:, None]
    rank = ((z > zt) | ((z == zt) & (np.arange(z.shape[1])[None, :] < y[:, None]))).sum(axis=1)
    rank = np.where(np.isnan(z).any(axis=1), z.shape[1], rank)
    return int((rank < 1).sum()), int((rank < 5).sum())
