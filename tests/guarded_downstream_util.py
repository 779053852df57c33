"""The augmentation case of tests/test_guarded_downstream_gpu.py, apart from the call itself: where the crops and the output lie
inside guarded memory (tests/guarded.py), what the restatement expects, and the check afterwards.  tests/test_guarded_downstream_cpu.py
runs the same layout and the same check around a torch stand-in of the kernel with one planted defect each, on the CPU.

Layout.  Every crop (T, h, w, 3) uint8 is a region of a larger "decoded frame" buffer: rows of `row_pitch` = 3 * (w + 7) + 2 bytes,
frames of (h + 5) rows + 11 bytes, the region starting 2 rows and 3 pixels + 2 bytes in (an odd address: the header promises no
alignment for src).  Everything around the region is the guard's byte 255 -- white, not a NaN -- so the crop gets a black outer ring:
a tap taken one pixel outside the region then reads 255 where the restatement clamps to 0, far outside the 5e-6 of the comparison.
The output is one float into a guarded allocation, with `out_clip_stride` = one clip + 17 floats: element 0, the 17 floats behind
every clip and the guard's bands must keep their fill."""
import torch

from oracle import augment as A

FILL32 = -1                 # the guard's 0xFF bytes as an int32
T, SIZE = 2, 24
SHAPES = [(37, 53), (12, 9)]      # one downsample and one upsample to 24: the y1 / x1 clamps of the upsample are live
GAP = 17
CLIP = 3 * T * SIZE * SIZE
STRIDE = CLIP + GAP

# (gray, flip, ops, gray_after, blur) per variant, one entry per clip: with and without contrast, blur and flip
VARIANTS = {
    "plain": [A.ClipParams(), A.ClipParams()],
    "contrast": [A.ClipParams(ops=[(A.CONTRAST, 1.3)]), A.ClipParams(gray=True, ops=[(A.BRIGHTNESS, 0.8), (A.CONTRAST, 0.7), (A.HUE, -0.2)])],
    "blur": [A.ClipParams(blur=True), A.ClipParams(blur=True, gray=True, gray_after=True, ops=[(A.SATURATION, 1.2)])],
    "flip": [A.ClipParams(flip=True), A.ClipParams(flip=True)],
    "all": [A.ClipParams(flip=True, blur=True, ops=[(A.SATURATION, 0.9), (A.CONTRAST, 1.25), (A.HUE, 0.3), (A.BRIGHTNESS, 1.1)]),
            A.ClipParams(flip=True, blur=True, ops=[(A.CONTRAST, 0.6)])],
}


def ringed_clip(seed, h, w):
    clip = A.synthetic_clip(seed, T, h, w).clone()
    clip[:, 0], clip[:, -1], clip[:, :, 0], clip[:, :, -1] = 0, 0, 0, 0
    return clip


def framed(clip):
    """(buffer uint8 1-D, byte offset of the region, row_pitch, frame_pitch): the crop inside its white frame."""
    t, h, w, _ = clip.shape
    row_pitch = 3 * (w + 7) + 2
    frame_pitch = (h + 5) * row_pitch + 11
    offset = 2 * row_pitch + 3 * 3 + 2
    buf = torch.full((t * frame_pitch,), 255, dtype=torch.uint8)
    torch.as_strided(buf, (t, h, w, 3), (frame_pitch, row_pitch, 3, 1), offset).copy_(clip)
    assert row_pitch > 3 * w and frame_pitch > h * row_pitch and offset % 2 == 1
    return buf, offset, row_pitch, frame_pitch


def region(buf, offset, row_pitch, frame_pitch, h, w, shift=0):
    """The crop as the descriptor addresses it (shift: bytes off, for the planted read past a row)."""
    return torch.as_strided(buf, (T, h, w, 3), (frame_pitch, row_pitch, 3, 1), buf.storage_offset() + offset + shift)


def clip_desc(desc_type, src_ptr, row_pitch, frame_pitch, h, w, params):
    d = desc_type()
    d.src, d.frame_pitch, d.row_pitch, d.h, d.w = src_ptr, frame_pitch, row_pitch, h, w
    d.gray = (2 if params.gray_after else 1 if params.gray else 0) + (4 if params.blur else 0)
    d.flip, d.n_ops = int(params.flip), len(params.ops)
    for i, (op, f) in enumerate(params.ops):
        d.op[i], d.factor[i], d.one_minus[i] = op, f, 1.0 - f
    return d


def expected(clips, params, mean, std):
    return [A.augment_clip(c, SIZE, p, mean, std) for c, p in zip(clips, params)]


def output_buffer(G):
    """1 + n_clips * STRIDE floats of guarded memory; the kernel's `out` is element 1."""
    return G.alloc((1 + len(SHAPES) * STRIDE,), name="augment out")


def check_output(buf, want, tol):
    """Every clip within tol of the restatement (a NaN -- an element nobody wrote -- fails), and every float that is not part of a
    clip still the guard's fill."""
    bits = buf.view(torch.int32).cpu()
    vals = buf.detach().cpu()
    assert int(bits[0]) == FILL32, "a store in front of the first clip"
    for i, w in enumerate(want):
        lo = 1 + i * STRIDE
        got = vals[lo:lo + CLIP].view(3, T, SIZE, SIZE)
        err = (got - w).abs().max().item()
        assert err <= tol, f"clip {i}: max error {err:.3e} against the restatement (tolerance {tol})"
        gap = bits[lo + CLIP:lo + STRIDE]
        assert bool((gap == FILL32).all()), f"clip {i}: {int((gap != FILL32).sum())} floats of the gap behind it were written"


def desc_bytes(descs):
    return torch.frombuffer(bytearray(b"".join(bytes(d) for d in descs)), dtype=torch.uint8)
