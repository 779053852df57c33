"""CPU: the detector of tests/test_guarded_downstream_gpu.py's augmentation case -- the layout of tests/guarded_downstream_util.py
inside guarded memory, the comparison with the restatement, the gap check and Guarded.check() -- around a torch stand-in of the
kernel with one planted defect of the kind a wrong kernel would have: a short write, an overrun into the gap between two clips (and
one past the last clip, into the band), and a read past a pitched uint8 row.  Every access stays inside the block the guard owns;
nothing wrong is ever run on a GPU.  Also the guard's own additions: 4-byte alignment, several modules at once, an output that the
contract leaves partly untouched."""
import pytest
import torch

import guarded_downstream_util as U
from guarded import GuardError, Guarded
from rspnet_amd import fingerprint as F, ops as O

CPU = torch.device("cpu")
MEAN, STD = [0.43, 0.40, 0.37], [0.23, 0.22, 0.22]
TOL = 5e-6


def stand_in(srcs, params, out, defect=None):
    """What rsp_augment_batch does, from torch ops on the guarded buffers: every crop read through its pitches, every clip written
    at its stride behind out[1]."""
    for i, ((buf, offset, row_pitch, frame_pitch, h, w), p) in enumerate(zip(srcs, params)):
        shift = 3 if defect == "read" and i == 1 else 0             # one pixel to the right: the last column lies past the row's crop
        crop = U.region(buf, offset, row_pitch, frame_pitch, h, w, shift)
        res = U.A.augment_clip(crop, U.SIZE, p, MEAN, STD).reshape(-1)
        n = U.CLIP - (1 if defect == "short" and i == 1 else 0)
        lo = 1 + i * U.STRIDE
        out[lo:lo + n] = res[:n]
        if defect == "gap" and i == 0:
            out[lo + U.CLIP] = 0.0
        if defect == "band" and i == 1:
            torch.as_strided(out, (1,), (1,), out.storage_offset() + out.numel()).fill_(0.0)


def run(defect, variant="all"):
    params = U.VARIANTS[variant]
    clips = [U.ringed_clip(20 + i, h, w) for i, (h, w) in enumerate(U.SHAPES)]
    want = U.expected(clips, params, MEAN, STD)
    with Guarded(CPU, skew=8) as G:
        srcs = []
        for clip in clips:
            buf, offset, row_pitch, frame_pitch = U.framed(clip)
            srcs.append((G.put(buf), offset, row_pitch, frame_pitch, clip.shape[1], clip.shape[2]))
        out = U.output_buffer(G)
        stand_in(srcs, params, out, defect)
        U.check_output(out, want, TOL)
        G.check()


@pytest.mark.parametrize("variant", list(U.VARIANTS))
def test_clean_stand_in_passes(variant):
    run(None, variant)


def test_short_write_is_reported():
    with pytest.raises(AssertionError, match=r"clip 1: max error nan against the restatement"):
        run("short")


def test_overrun_into_the_gap_is_reported():
    with pytest.raises(AssertionError, match=r"clip 0: 1 floats of the gap behind it were written"):
        run("gap")


def test_overrun_past_the_last_gap_is_reported():
    with pytest.raises(GuardError, match=r"augment out: back band written, first bad byte at offset \d+ of the payload, 4 bytes"):
        run("band")


def test_read_past_a_pitched_uint8_row_is_reported():
    """The taps of the last output column land on the white frame instead of the black ring: an error of the order of the whole
    normalised range, against a tolerance of 5e-6."""
    with pytest.raises(AssertionError, match=r"clip 1: max error [0-9.]+e[+-]\d+ against the restatement") as e:
        run("read")
    assert float(str(e.value).split("max error ")[1].split()[0]) > 0.5


def test_layout_is_pitched_odd_and_ringed():
    for i, (h, w) in enumerate(U.SHAPES):
        clip = U.ringed_clip(20 + i, h, w)
        buf, offset, row_pitch, frame_pitch = U.framed(clip)
        assert row_pitch > 3 * w and frame_pitch > h * row_pitch and offset % 2 == 1
        assert torch.equal(U.region(buf, offset, row_pitch, frame_pitch, h, w), clip)
        assert int(clip[:, 0].max()) == 0 and int(clip[:, :, -1].max()) == 0 and int(clip[:, 1:-1, 1:-1].max()) > 0
        inside = torch.zeros_like(buf, dtype=torch.bool)
        U.region(inside, offset, row_pitch, frame_pitch, h, w).fill_(True)
        assert bool((buf[~inside] == 255).all())


# ---- the guard's additions -------------------------------------------------------------------------------------------------
def test_skew_4_gives_floats_4_bytes_and_wider_elements_and_op_byte_buffers_8():
    with Guarded(CPU, skew=4) as G:
        assert G.alloc((5,)).data_ptr() % 8 == 4 and G.alloc((5,), torch.int32).data_ptr() % 8 == 4
        assert G.alloc((5,), torch.int64).data_ptr() % 16 == 8 and G.alloc((5,), torch.float64).data_ptr() % 16 == 8
        assert G.alloc((36,), torch.uint8).data_ptr() % 8 == 4                               # the test's own byte buffer: as asked
        assert O.torch.empty(64, dtype=torch.uint8, device=CPU).data_ptr() % 16 == 8         # the op's: a table, records, a workspace
        G.check()


def test_several_modules_are_guarded_at_once_and_restored():
    with Guarded(CPU, ops_module=[O, F]) as G:
        assert O.torch is F.torch and O.torch is not torch
        a = O.torch.empty(3, dtype=torch.float32, device=CPU)
        b = F.torch.empty((2, 32), dtype=torch.uint8, device=CPU)
        assert len(G.blocks) == 2 and all(blk.proxy for blk in G.blocks)
        a.fill_(1.0)
        G.check()
        assert G.block_of(b[1]) is G.blocks[1]
    assert O.torch is torch and F.torch is torch
    with pytest.raises(ZeroDivisionError):
        with Guarded(CPU, ops_module=[O, F]):
            1 / 0
    assert O.torch is torch and F.torch is torch


def test_an_output_the_contract_leaves_partly_untouched():
    with Guarded(CPU) as G:
        out = O.torch.empty(3, dtype=torch.float32, device=CPU)
        out[:2] = 1.0
        with pytest.raises(GuardError, match="never written, first bad byte at offset 8"):
            G.check()
        G.allow_unwritten(out)
        G.check()
        assert out.view(torch.int32)[2].item() == -1
