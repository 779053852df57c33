"""TEST-ONLY helpers of the similarity-map tests: fp64 torch restatements of rsp_cam_maps (the reference's NCDHW einsums, with the
`k_row` pairing) and of rsp_cam_overlay, the checker backend with both ops, and the fixture loader."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from cpu_ops import CpuOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ARCHS = ["c3d", "resnet18", "r2plus1d-vcop", "s3dg"]
MAP_NAMES = ("Ms_qA", "Ms_qM", "Ms_kA", "Ms_kM")


def cam_maps_ref(q_F, k_F, k_row, q_wA, q_wM, k_wA, k_wM, dtype=torch.float64):
    """moco/builder_diffspeed_diffloss.py:468-488 on NCDHW features (B, C, T', H', W'), row k_row[b] of k_F paired with sample b.
    Returns (4, B, T', H', W'), order qA, qM, kA, kM."""
    q_F, k_F = q_F.to(dtype), k_F.to(dtype)[k_row.long()]
    q_wA, q_wM, k_wA, k_wM = (w.to(dtype) for w in (q_wA, q_wM, k_wA, k_wM))
    q_X, k_X = q_F.mean(dim=(2, 3, 4)), k_F.mean(dim=(2, 3, 4))

    def one(w_other, x_other, w_self, feat):
        return torch.einsum("bc,bcthw->bthw", torch.einsum("bn,nc->bc", torch.einsum("nc,bc->bn", w_other, x_other), w_self), feat)

    return torch.stack([one(k_wA, k_X, q_wA, q_F), one(k_wM, k_X, q_wM, q_F), one(q_wA, q_X, k_wA, k_F), one(q_wM, q_X, k_wM, k_F)])


def jet(v):
    """The project's colour map: analytic jet on the continuous value, channels last (r, g, b)."""
    return torch.stack([(1.5 - (4 * v - 3).abs()).clamp(0, 1), (1.5 - (4 * v - 2).abs()).clamp(0, 1),
                        (1.5 - (4 * v - 1).abs()).clamp(0, 1)], dim=-1)


def cam_overlay_ref(maps, clip_a, clip_b, t, dtype=torch.float64):
    """maps (N, T', H', W'); clips (B, 3, T, size, size) in [0, 1].  Returns (N, size, size, 3) uint8."""
    maps = maps.to(dtype)
    N = maps.shape[0]
    B, size = clip_a.shape[0], clip_a.shape[-1]
    m = maps.mean(dim=1)
    lo, hi = m.amin(dim=(1, 2), keepdim=True), m.amax(dim=(1, 2), keepdim=True)
    rng = hi - lo
    v = torch.where(rng > 0, (m - lo) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(m))
    v = F.interpolate(v[:, None], size=(size, size), mode="bilinear", align_corners=False)[:, 0]
    colour = jet(v)
    frames = []
    for n in range(N):
        clip = clip_b if (clip_b is not None and n >= N // 2) else clip_a
        frames.append(clip[n % B, :, t].to(dtype).permute(1, 2, 0))
    px = 0.6 * (torch.stack(frames) * 255.0) + 0.4 * (colour * 255.0)
    return torch.round(px).clamp(0, 255).to(torch.uint8)


class CamCpuOps(CpuOps):
    """The checker backend plus the two cam ops, through the restatements above (fp32, as the kernels compute)."""

    def cam_maps(self, feat_q, feat_k, k_row, w_qA, w_qM, w_kA, w_kM):
        ncdhw = lambda x: x.permute(0, 4, 1, 2, 3)
        return cam_maps_ref(ncdhw(feat_q), ncdhw(feat_k), k_row, w_qA, w_qM, w_kA, w_kM, dtype=torch.float32).contiguous()

    def cam_overlay(self, maps, clip_a, clip_b, t):
        return cam_overlay_ref(maps, clip_a, clip_b, t, dtype=torch.float32)


def load_fixture(arch):
    z = np.load(os.path.join(GOLDEN, f"cam_{arch.replace('-', '_')}.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def fixture_inputs(arch, meta):
    """(state dict of numpy arrays, im_q, im_k) from the portable generators, as tools/gen_golden_cam.py built them."""
    from oracle import portable as P
    with open(os.path.join(GOLDEN, f"state_spec_{arch.replace('-', '_')}.json")) as f:
        spec = {k: (tuple(s), d) for k, (s, d) in json.load(f).items()}
    state = P.fill_state(spec, meta["seed"])
    im_q, im_k = P.clips(meta["seed"], 0, (meta["B"], 3, meta["T"], meta["HW"], meta["HW"]))
    return state, im_q, im_k


def restated_maps(arch, state, im_q, im_k, perms, speed, aligned=False, dtype=torch.float64):
    """The reference's cam_visualize restated: oracle.restatement's eval-mode encoders (bn_eval) in `dtype` plus the four formulas.
    aligned=False: key features of the batch shuffled by perms[2], as the reference pairs them; True: keys in the caller's order."""
    from oracle import restatement as R
    sd = {k: (torch.from_numpy(v).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v.copy())) for k, v in state.items()}
    default = torch.get_default_dtype()
    torch.set_default_dtype(dtype)            # (restatement.diff_speed allocates with torch.empty)
    try:
        q, k, _ = R.diff_speed(torch.from_numpy(im_q).to(dtype), torch.from_numpy(im_k).to(dtype),
                               torch.from_numpy(np.asarray(perms[0])), speed)
        if not aligned:
            k = k[torch.from_numpy(np.asarray(perms[2])).long()]
        with torch.no_grad(), R.bn_eval():
            _, _, k_F = R.encoder_forward(arch, sd, "encoder_k", k)
            _, _, q_F = R.encoder_forward(arch, sd, "encoder_q", q)
    finally:
        torch.set_default_dtype(default)
    ident = torch.arange(q_F.shape[0])
    return cam_maps_ref(q_F, k_F, ident, sd["encoder_q.fc1.2.weight"], sd["encoder_q.fc2.2.weight"], sd["encoder_k.fc1.2.weight"],
                        sd["encoder_k.fc2.2.weight"], dtype=dtype)


def rel_err(mine, ref):
    mine, ref = np.asarray(mine, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(mine - ref).max()) / max(float(np.abs(ref).max()), 1e-300)
