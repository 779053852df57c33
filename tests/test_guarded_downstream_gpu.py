"""GPU: the kernels behind the training path -- fused augmentation, fine-tune criterion, pretext meters, similarity maps and overlay,
fingerprints, top-k hit counter, element-wise ops, the device-pointer enqueue, the min/max BatchNorm follower -- with every operand
inside guarded memory (tests/guarded.py), as tests/test_guarded_memory_gpu.py does for the training path.

Where a value test already exists its body runs unchanged (check_case of test_finetune_loop_gpu, test_shapes of
test_pretext_metrics_gpu, check_maps and the overlay body of test_cam_gpu, two bodies of test_augment_gpu, test_topk_hits_counts of
test_retrieval_gpu), at its own tolerance, with the module's placement hook pointed at the guard; the op's outputs and workspaces
come from the guard too (Guarded(ops_module=[...]) for rspnet_amd.augment and rspnet_amd.fingerprint, which allocate themselves).
The body's comparison is the value check -- a read outside an operand meets NaN (byte 255 in a uint8 image) and fails it --, and
every case ends in Guarded.check(): no band byte changed, no input changed, no float32 output of the op kept an unwritten word.
tests/test_guarded_downstream_cpu.py shows the detector reporting planted defects.

Alignment: what include/rspnet_hip.h promises and no more -- 4 bytes (skew=4) for the float / int32 operands of the criterion, the
meters, the maps, the fingerprints, the hit counter, the element-wise ops and the enqueue; the kernels that take a 16-byte path when
the pointers allow it (maps, fingerprint, element-wise, follower) run at skew 16 as well; the crops of the augmentation start at an
odd address."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import guarded_downstream_util as U
import test_augment_gpu as AUG
import test_cam_gpu as CAM
import test_finetune_loop_gpu as X
import test_kernels_gpu as K
import test_pretext_metrics_gpu as P
import test_retrieval_gpu as R
from guarded import Guarded
from rspnet_amd import _lib, augment, fingerprint as F, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
UNWRITTEN = -1              # the guard's fill as an int32


@pytest.fixture(scope="module")
def hip():
    assert ops.backend().name == "hip"
    return ops.backend()


@contextlib.contextmanager
def placed(mod, **hooks):
    """The module's placement hooks pointed at the guard, for the length of one body."""
    saved = {n: getattr(mod, n) for n in hooks}
    try:
        for n, f in hooks.items():
            setattr(mod, n, f)
        yield
    finally:
        for n, f in saved.items():
            setattr(mod, n, f)


def op_outputs(G, nbytes=None):
    return [b for b in G.blocks if b.proxy and b.kind == "output" and (nbytes is None or b.nbytes == nbytes)]


# ---- rsp_augment_batch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(U.VARIANTS))
def test_augment_batch_pitched_source_and_strided_output(hip, variant):
    """Two crops of different (h, w), one down- and one upsampled to 24, each a region of a wider white frame (row_pitch > 3w,
    frame_pitch > h * row_pitch, odd start address) with a black outer ring, written with out_clip_stride one clip + 17 floats:
    within 5e-6 of the restatement, the gaps and the float in front still the guard's fill."""
    params = U.VARIANTS[variant]
    clips = [U.ringed_clip(20 + i, h, w) for i, (h, w) in enumerate(U.SHAPES)]
    want = U.expected(clips, params, AUG.MEAN, AUG.STD)
    with Guarded(DEV, skew=8) as G:
        descs = []
        for clip, p in zip(clips, params):
            buf, offset, row_pitch, frame_pitch = U.framed(clip)
            src = G.put(buf)
            descs.append(U.clip_desc(_lib.AugmentClipDesc, src.data_ptr() + offset, row_pitch, frame_pitch, clip.shape[1], clip.shape[2], p))
            assert (src.data_ptr() + offset) % 2 == 1
        ddev = G.put(U.desc_bytes(descs))
        out = U.output_buffer(G)
        wsb = int(hip.lib.rsp_augment_workspace(len(clips), U.T, U.SIZE))
        ws = hip._workspace(DEV, wsb)
        m3, s3 = (C.c_float * 3)(*AUG.MEAN), (C.c_float * 3)(*AUG.STD)
        b9 = (C.c_float * 9)(*augment._gaussian_kernel2d().reshape(-1).tolist())
        _lib.check(hip.lib.rsp_augment_batch(ddev.data_ptr(), len(clips), U.T, U.SIZE, m3, s3, b9, out.data_ptr() + 4, U.STRIDE,
                                             ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream), "rsp_augment_batch")
        U.check_output(out, want, AUG.TOL)
        G.check()


@pytest.mark.parametrize("body,kw", [("test_flip_is_an_exact_mirror_and_identity_pipeline_is_resize_plus_normalise", {}),
                                     ("test_matches_reference_fixture", {"case": AUG.CASES[0]}),
                                     ("test_aug_plus_matches_reference_fixture", {"seed": int(AUG.GOLD["plus_seeds"][0])})],
                         ids=["flip", "fixture", "aug_plus"])
def test_augment_collate(hip, body, kw):
    """FusedGPUCollateFn as the drivers call it: its output (allocated in rspnet_amd/augment.py) and the workspace inside the guard."""
    with Guarded(DEV, ops_module=[ops, augment]) as G:
        getattr(AUG, body)(**kw)
        assert len(op_outputs(G)) >= 1 and any(b.kind == "workspace" for b in G.blocks)
        G.check()


# ---- rsp_xent_metrics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_crop", [1, 3])
@pytest.mark.parametrize("classes", [4, 5, 101, 400])
@pytest.mark.parametrize("S", [1, 7, 80])
def test_xent_metrics(hip, S, classes, n_crop):
    """check_case of test_finetune_loop_gpu with ld = classes + 3 (the three floats behind every row are NaN), S samples of n_crop
    rows each -- 1, 7 and 80 rows at n_crop = 1 --, valid 0, 1 and S.  What the header leaves untouched stays untouched: acc[1]
    with fewer than 5 classes, both accuracies with valid = 0."""
    rng = np.random.default_rng(1000 * S + 10 * classes + n_crop)
    rows = S * n_crop
    scale = 80.0 if (rows + classes) % 3 == 0 else 1.0
    logits = (rng.uniform(-1, 1, (rows, classes)) * scale).astype(np.float32)
    target = rng.integers(0, classes, S).astype(np.int64)
    for valid in sorted({0, 1, S}):
        with Guarded(DEV, skew=4) as G, placed(X, place=G.put, place_empty=G.empty):
            X.check_case(hip, logits, n_crop, target, valid, padded=True)
            (scalars,) = op_outputs(G, 12)                      # loss, acc1, acc5
            words = scalars.payload.view(torch.int32).cpu().tolist()
            untouched = [1, 2] if valid == 0 else [2] if classes < 5 else []
            assert [i for i in range(3) if words[i] == UNWRITTEN] == untouched, (words, untouched)
            if untouched:
                G.allow_unwritten(scalars.payload)
            assert len(op_outputs(G)) == 3 and any(b.kind == "workspace" for b in G.blocks)
            G.check()


# ---- rsp_pretext_metrics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K1", [5, 65, 16385])
@pytest.mark.parametrize("B", [1, 5, 33])
def test_pretext_metrics(hip, B, K1):
    """test_shapes of test_pretext_metrics_gpu: odd K1, so the rows of the dense matrices start 4 bytes off every wider boundary."""
    with Guarded(DEV, skew=4) as G, placed(P, place=G.put, place_empty=G.empty):
        P.test_shapes(B, K1)
        assert len(G.blocks) == 6
        G.check()


# ---- rsp_cam_maps, rsp_cam_overlay -------------------------------------------------------------------------------------------
# (seed, B, T', H', W', C, dim_A, dim_M, pitch): R3D-18's shipped shape and two cases of the geometry fuzz, all with ld > C
CAM_CASES = [(1,) + CAM.SHIPPED[1] + (128, 128, 520), (3 + 130,) + CAM.FUZZ[3], (3 + 83,) + CAM.FUZZ[4]]


@pytest.mark.parametrize("skew", [4, 16])
@pytest.mark.parametrize("case", CAM_CASES, ids=lambda c: "x".join(map(str, c[1:6])) + f"ld{c[8]}")
def test_cam_maps(hip, case, skew):
    seed, B, Tp, Hp, Wp, Cc, dA, dM, pitch = case
    assert pitch > Cc
    for identity in (False, True):
        with Guarded(DEV, skew=skew) as G, placed(CAM, dev=G.put):
            CAM.check_maps(seed + (0 if not identity else 1), B, Tp, Hp, Wp, Cc, dA, dM, pitch, identity=identity)
            assert len(op_outputs(G)) == 2 and any(b.kind == "workspace" for b in G.blocks)
            G.check()


def test_cam_overlay(hip):
    with Guarded(DEV, skew=4) as G, placed(CAM, dev=G.put):
        CAM.test_cam_overlay_matches_restatement(112, 1)
        assert len(op_outputs(G)) == 3
        G.check()


# ---- rsp_fingerprint ---------------------------------------------------------------------------------------------------------
FP_LENGTHS = (1, 63, 64, 65, 1000003)


@pytest.mark.parametrize("skew", [4, 16])
def test_fingerprint(hip, skew):
    """One job per length, each tensor in a block of its own (what lies behind its last word is NaN: it would be counted and
    hashed), at 4-byte and at 16-byte aligned addresses; the table and the records are the module's own allocations.  The records
    are the restatement's 32 bytes each, so a record nobody wrote cannot pass."""
    rng = np.random.default_rng(77)
    host = [rng.standard_normal(n).astype(np.float32) for n in FP_LENGTHS] + [np.arange(-3, 30, dtype=np.int64) * 2654435761]
    want = F.reference_records(host)
    with Guarded(DEV, skew=skew, ops_module=[ops, F]) as G:
        tensors = [G.put(torch.from_numpy(h)) for h in host]
        assert all(t.data_ptr() % (2 * skew) == skew for t in tensors[:-1])
        fs = F.FingerprintSet([f"n{h.size}" for h in host], tensors)
        assert fs.native
        fs.run()
        got = fs.read()
        assert got.tobytes() == want.tobytes(), [n for n, g, w in zip(fs.names, got, want) if g.tobytes() != w.tobytes()]
        assert [int(g["nonfinite"]) for g in got] == [0] * len(host)
        assert len(op_outputs(G)) == 2 and any(b.kind == "workspace" for b in G.blocks)      # table, records; partials
        G.check()


# ---- rsp_topk_hits -----------------------------------------------------------------------------------------------------------
def test_topk_hits(hip):
    with Guarded(DEV, skew=4) as G, placed(R, dev=G.put):
        R.test_topk_hits_counts()
        assert len(op_outputs(G)) == 1
        G.check()


# ---- rsp_eltwise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skew", [4, 16])
@pytest.mark.parametrize("n", [1, 255, 1000003])
def test_eltwise(hip, n, skew):
    """All five ops against the checker at the 1e-6 of tests/test_nonfinite_gpu.py, into a fresh output and in place over either
    operand (same bits); skew 4: the scalar loop, skew 16: float4 with a scalar tail."""
    a, b = K.rnd(n, seed=1), K.rnd(n, seed=2)
    for op in ("relu_fwd", "relu_bwd", "sigmoid_fwd", "sigmoid_bwd", "add"):
        binary = op in ("relu_bwd", "sigmoid_bwd", "add")
        x = torch.sigmoid(a) if op == "sigmoid_bwd" else a
        ref = K.CPU.eltwise(op, x, b if binary else None)
        with Guarded(DEV, skew=skew) as G:
            xd, bd = G.put(x), G.put(b) if binary else None
            out = hip.eltwise(op, xd, bd)
            K.close(out, ref, 1e-6, op)
            over_a = G.alloc((n,), name="in place over a").copy_(x)
            assert hip.eltwise(op, over_a, bd, out=over_a) is over_a
            assert torch.equal(over_a.view(torch.int32), out.view(torch.int32)), op
            if binary:
                over_b = G.alloc((n,), name="in place over b").copy_(b)
                hip.eltwise(op, xd, over_b, out=over_b)
                assert torch.equal(over_b.view(torch.int32), out.view(torch.int32)), op
            assert len(op_outputs(G)) == 1
            G.check()


# ---- rsp_queue_enqueue_dev -----------------------------------------------------------------------------------------------------
def test_queue_enqueue_dev(hip):
    """The pointer at K - n (the slab ends on the queue's last column, the pointer wraps to 0), then at 0 and at n."""
    dim, Kq, n = 20, 24, 8
    q = K.rnd(dim, Kq, seed=1)
    ptr = torch.tensor([Kq - n], dtype=torch.int64)
    with Guarded(DEV, skew=4) as G:
        qd = G.alloc((dim, Kq), name="queue").copy_(q)
        pd = G.alloc((1,), torch.int64, name="queue_ptr").copy_(ptr)
        for step, want_ptr in enumerate((0, n, 2 * n)):
            keys = K.rnd(n, dim, seed=10 + step)
            hip.queue_enqueue_dev(qd, pd, G.put(keys))
            K.CPU.queue_enqueue_dev(q, ptr, keys)
            assert int(ptr) == want_ptr and torch.equal(pd.cpu(), ptr)
            assert torch.equal(qd.cpu(), q)
        G.check()


# ---- rsp_bn_act_minmax_fwd -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,skew", [(64, 16), (64, 4), (6, 16), (300, 4)])
def test_bn_act_minmax_fwd_into_a_channel_slice(hip, Cc, skew):
    """out = act(fma(scale, scale >= 0 ? max : min, shift)) into channels [8, 8 + C) of rows of C + 24 floats: the float4 instance
    (C = 64 at 16-byte alignment) and the scalar one (4-byte alignment; C = 6; C = 300: two channel blocks), 150 positions (no
    multiple of the positions a workgroup takes per trip).  Against fp64 at 1e-6: one fma against one rounding of the exact value."""
    pos = (2, 3, 5, 5)
    ymin = K.rnd(*pos, Cc, seed=1)
    ymax = ymin + K.rnd(*pos, Cc, seed=2).abs()
    sc = K.rnd(Cc, seed=3) + 0.25
    sc[3::7] = 0.0
    sc[5::7] = -sc[5::7].abs() - 0.1
    ss = torch.stack([sc, K.rnd(Cc, seed=4) * 0.5]).contiguous()
    pick = torch.where(sc >= 0, ymax.double(), ymin.double())
    z = pick * sc.double() + ss[1].double()
    for relu in (True, False):
        ref = torch.relu(z) if relu else z
        with Guarded(DEV, skew=skew) as G:
            wide = G.alloc(pos + (Cc + 24,), name="wide out")
            hip.bn_act_minmax_fwd(G.put(ymax), G.put(ymin), G.put(ss), relu, out=wide[..., 8:8 + Cc])
            K.close(wide[..., 8:8 + Cc], ref, 1e-6, f"follower into a slice, relu={relu}")
            bits = wide.view(torch.int32)
            assert bool((bits[..., :8] == UNWRITTEN).all()) and bool((bits[..., 8 + Cc:] == UNWRITTEN).all()), "a store outside the slice"
            dense = hip.bn_act_minmax_fwd(G.put(ymax), G.put(ymin), G.put(ss), relu)
            K.close(dense, ref, 1e-6, f"follower, relu={relu}")
            G.check()
