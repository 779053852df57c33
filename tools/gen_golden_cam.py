"""Generate the similarity-map fixtures tests/golden/cam_<arch>.npz from the REFERENCE's own MoCoDiffLossTwoFc.cam_visualize (build
container only).  TEST INFRASTRUCTURE ONLY.

    python tools/gen_golden_cam.py [arch ...]

Per architecture (B = 4, T = 32, 64 x 64, K = 64, diff_speed = [2]): the portable state over the committed state spec
(oracle.portable.fill_state: non-trivial BatchNorm running statistics — with freshly initialised ones the S3D-G maps are ~1e-13),
portable clips, three fixed non-identity permutations; the reference model in eval mode, cam_visualize under the replayed draws.
Stored: seed, sizes, permutations, speed, the four fp32 maps and `floor`: per map max|ref_fp32 - restated_fp64| / max|restated_fp64|,
the fp64 side being oracle.restatement's eval-mode encoders in double plus the four formulas (tests/cam_util.py; the reference itself
cannot run in fp64: its _diff_speed allocates fp32 buffers).  A floor above 1e-4 means the state is badly conditioned for that
architecture: the next seed is taken — by that oracle-only criterion, never by how the HIP path lands.  Only recorded results and
settings are stored."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import portable as P
from oracle import ref_harness as R

import cam_util

B, T, HW, K, SPEED = 4, 32, 64, 64, 2
FLOOR_MAX = 1e-4


def permutations(seed):
    """[the _diff_speed permutation, shuffle #1 (k_negative pass), shuffle #2 (k pass)]: portable, none the identity."""
    out = []
    for i in range(3):
        for bump in range(100):
            p = P.permutation(f"cam_perm{i}", seed + 1000 * bump, B)
            if not np.array_equal(p, np.arange(B)):
                break
        out.append(p)
    return out


def reference_maps(arch, state, im_q, im_k, perms):
    model = R.build_reference_model(arch, K=K, diff_speed=(SPEED,))
    R.ensure_process_group()          # (the reference's shuffle-BN all-gathers: a gloo group of one rank)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    model.eval()
    with R._ReplayRNG(perms, SPEED) as rng:
        maps = model.cam_visualize(torch.from_numpy(im_q), torch.from_numpy(im_k))
    assert rng.calls == [B, B, B], rng.calls
    post = model.state_dict()
    assert all(np.array_equal(post[k].numpy(), v) for k, v in state.items()), "the reference moved its state in eval mode"
    return [m.numpy().astype(np.float32) for m in maps]


def generate(arch):
    for seed in range(1, 50):
        meta = {"arch": arch, "seed": seed, "B": B, "T": T, "HW": HW, "K": K, "speed": SPEED}
        state, im_q, im_k = cam_util.fixture_inputs(arch, meta)
        perms = permutations(seed)
        ref = reference_maps(arch, state, im_q, im_k, perms)
        restated = cam_util.restated_maps(arch, state, im_q, im_k, perms, SPEED).numpy()
        floor = np.asarray([cam_util.rel_err(r, w) for r, w in zip(ref, restated)])
        print(f"{arch}: seed {seed}, maps {ref[0].shape}, max|map| {[float(np.abs(r).max()) for r in ref]}, floor {floor}")
        if float(floor.max()) <= FLOOR_MAX:
            break
    else:
        raise SystemExit(f"{arch}: no well-conditioned seed")
    out = {"meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), "perms": np.stack(perms).astype(np.int64),
           "floor": floor.astype(np.float64)}
    out.update({name: m for name, m in zip(cam_util.MAP_NAMES, ref)})
    path = os.path.join(cam_util.GOLDEN, f"cam_{arch.replace('-', '_')}.npz")
    np.savez_compressed(path, **out)
    print(f"{arch}: wrote {path}, {os.path.getsize(path)} bytes")


def main():
    for arch in (sys.argv[1:] or cam_util.ARCHS):
        generate(arch)


if __name__ == "__main__":
    main()
