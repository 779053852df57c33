#!/usr/bin/env python
"""Similarity maps (rsp_cam_maps) against the torch composition a user would otherwise write on the same device tensors — NDHWC ->
NCDHW permute copies plus the reference's twelve einsums (moco/builder_diffspeed_diffloss.py:468-488) — at the feature-map shapes
of the BASELINE configurations, and one line for a whole MoCoDiffLossTwoFc.cam_visualize call next to the two eval-mode encoder
forwards it contains.  Both bodies run in ONE process in interleaved blocks (medians over the blocks, with their spread); every
block ends in a device synchronise.  One MI355X.

    python tools/cam_bench.py [--arch c3d ...] [--out profiles/cam_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from rspnet_amd import ops
from rspnet_amd.engine import INPUT_CHANNEL_PAD
from rspnet_amd.moco import ModelFactory

# arch -> (config file, batch, clip size): the BASELINE shapes (T = 32 frames in, speed 2: 16 frames through the encoders)
CASES = {"c3d": ("c3d.json", 32, 112), "resnet18": ("resnet18.json", 32, 112), "r2plus1d-vcop": ("r2plus1d.json", 32, 112),
         "s3dg": ("s3dg.json", 16, 224)}
ap = argparse.ArgumentParser()
ap.add_argument("--arch", nargs="*", default=sorted(CASES), choices=sorted(CASES))
ap.add_argument("--iters", type=int, default=200, help="calls per block")
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "cam_bench needs the GPU: a CPU run says nothing about it"
dev = torch.device("cuda", 0)
be = ops.backend()
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def torch_maps(q_F, k_F, q_wA, q_wM, k_wA, k_wM):
    q_F, k_F = q_F.permute(0, 4, 1, 2, 3).contiguous(), k_F.permute(0, 4, 1, 2, 3).contiguous()
    q_X, k_X = q_F.mean(dim=(2, 3, 4)), k_F.mean(dim=(2, 3, 4))

    def one(w_other, x_other, w_self, feat):
        return torch.einsum("bc,bcthw->bthw", torch.einsum("bn,nc->bc", torch.einsum("nc,bc->bn", w_other, x_other), w_self), feat)

    return one(k_wA, k_X, q_wA, q_F), one(k_wM, k_X, q_wM, q_F), one(q_wA, q_X, k_wA, k_F), one(q_wM, q_X, k_wM, k_F)


def block(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def interleaved(bodies, n):
    for fn in bodies.values():
        for _ in range(10):
            fn()
    res = {k: [] for k in bodies}
    for _ in range(args.blocks):
        for k, fn in bodies.items():
            res[k].append(block(fn, n))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


for arch in args.arch:
    cfg_file, B, size = CASES[arch]
    with open(os.path.join(ROOT, "rspnet_amd", "config", "pretrain", cfg_file)) as f:
        cfg = json.load(f)
    cfg["batch_size"] = B
    cfg["moco"]["k"] = cfg["moco"]["k"] // B * B
    torch.manual_seed(0)
    model = ModelFactory(cfg).build_moco_diffloss(device=dev).module.eval()
    g = torch.Generator(device=dev).manual_seed(1)
    T = int(cfg["temporal_transforms"]["size"])
    im_q = torch.rand(B, 3, T, size, size, device=dev, generator=g)
    im_k = torch.rand(B, 3, T, size, size, device=dev, generator=g)
    with torch.no_grad():
        model.cam_visualize(im_q, im_k, align_keys=True)
        q_F, k_F = model.encoder_q._get_last_feature(), model.encoder_k._get_last_feature()
        ws = [w.contiguous() for w in model.encoder_q._get_fc_weight() + model.encoder_k._get_fc_weight()]
        k_row = torch.arange(B, dtype=torch.int32, device=dev)
        mine = be.cam_maps(q_F, k_F, k_row, *ws)
        theirs = torch.stack(torch_maps(q_F, k_F, *ws))
        err = float((mine - theirs).abs().max() / theirs.abs().max())
        r = interleaved({"hip": lambda: be.cam_maps(q_F, k_F, k_row, *ws), "torch": lambda: torch_maps(q_F, k_F, *ws)}, args.iters)
        mb = 2 * q_F.numel() * 4 / 2**20
        say(f"{arch} B={B} feature {tuple(q_F.shape[1:])} ({mb:.1f} MiB both): rsp_cam_maps median {r['hip'][0] * 1e3:.1f} us "
            f"(min {r['hip'][1] * 1e3:.1f}, max {r['hip'][2] * 1e3:.1f}); torch permute + 12 einsums median {r['torch'][0] * 1e3:.1f} us "
            f"(min {r['torch'][1] * 1e3:.1f}, max {r['torch'][2] * 1e3:.1f}); torch / hip = {r['torch'][0] / r['hip'][0]:.2f}; "
            f"max |diff| / max |map| = {err:.1e}; {args.blocks} blocks x {args.iters} calls")
        x = torch.zeros((B, T // 2, size, size, INPUT_CHANNEL_PAD), device=dev)
        x[..., :3] = im_q[:, :, ::2].permute(0, 2, 3, 4, 1)

        def forwards():
            model.encoder_k.forward_ndhwc(x, keep=False, training=False)
            model.encoder_q.forward_ndhwc(x, keep=False, training=False)

        n = max(args.iters // 20, 5)
        r2 = interleaved({"call": lambda: model.cam_visualize(im_q, im_k, align_keys=True), "forwards": forwards}, n)
        say(f"{arch} B={B} {size}x{size}: cam_visualize median {r2['call'][0]:.2f} ms (min {r2['call'][1]:.2f}, max {r2['call'][2]:.2f}); "
            f"its two eval-mode encoder forwards {r2['forwards'][0]:.2f} ms (min {r2['forwards'][1]:.2f}, max {r2['forwards'][2]:.2f}); "
            f"rsp_cam_maps = {r['hip'][0] / r2['call'][0] * 100:.2f} % of the call; {args.blocks} blocks x {n} calls")
    del model

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
