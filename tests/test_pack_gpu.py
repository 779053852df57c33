"""GPU: the batched weight re-pack (PackSet.run -> rsp_pack_run -> pack_batch_kernel) and the input gradient over its buffers
(rsp_conv3d_dgrad_packed), kernel by kernel, at the cases of tests/pack_util.py.

The other per-kernel suites pack with conv_pack_fwd and call conv_dgrad, which re-packs into its own workspace: both run
pack_weight_kernel, one division chain per element.  pack_batch_kernel is the kernel every training step runs instead: filters
staged through LDS in chunks, incremental index walks, a transposed read for the dgrad layouts, the slice-major K order, zero
padding for a source narrower than the geometry, and a second path for the stem layout.  Here it is held to the other packer bit for
bit, to the source as a permutation, and — through conv_dgrad_packed — to conv_dgrad's bits and an fp64 transposed convolution.

Weights are 1 ... numel as exact float32 (every word distinct and non-zero) unless a test says otherwise.  Packed buffers start as
0xFF bytes (the word no finite weight has), so padding must be WRITTEN as +0.0 and the part of a dgrad buffer no job owns — the
allocation is an upper bound, rsp_conv3d_packed_dgrad_elems — must stay untouched and unread: its NaNs would show in dx.

dev() / dev_empty() / GUARD are the placement hooks tests/test_guarded_memory_gpu.py points at guarded memory when it runs the
bodies of test_forward_layout_equals_the_single_packer, test_packed_dgrad and test_one_table_many_jobs again."""
import ctypes as C
import functools

import pytest
import torch

import pack_util as U
import test_kernels_gpu as K
from guarded import Guarded
from rspnet_amd import _lib
from rspnet_amd.ops import ConvGeom

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = None      # the Guarded instance while a body runs inside one (test_guarded_memory_gpu.placed_in)


def dev(t):
    return t.to(DEV)


def dev_empty(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def hip():
    from rspnet_amd import ops
    assert ops.backend().name == "hip"
    return ops.backend()


def _stream():
    from rspnet_amd import ops
    return ops._stream()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def ramp(c, sign=1.0):
    """The case's source weight, 1 ... numel."""
    shape = U.src_shape(c)
    n = 1
    for s in shape:
        n *= s
    assert n < (1 << 24)
    return (torch.arange(1, n + 1, dtype=torch.float32) * sign).view(shape)


def padded(c, w_src):
    """The source zero-padded to the geometry's (Cout, Cin)."""
    full = torch.zeros((c[5], c[4]) + tuple(c[8]), dtype=w_src.dtype)
    full[:w_src.shape[0], :w_src.shape[1]] = w_src
    return full


def new_set(hip, entries):
    """A PackSet whose buffers start as 0xFF bytes; its dgrad buffers are declared partly written to the guard, if there is one
    (the test looks at their tails itself: written_exactly)."""
    ps = hip.pack_set(entries)
    for (g, which, _), t in zip(entries, ps.packed):
        bits(t).fill_(-1)
        if which and GUARD is not None:
            GUARD.allow_unwritten(t)
    return ps


def written_exactly(c, which, packed):
    """Every word the jobs own is written, and no other: [0, sum O x Kld) for the dgrad layouts, the whole buffer for the forward
    one.  (No weight of these tests has the bits 0xFFFFFFFF.)"""
    g = U.geom(c)
    _, jobs = U.jobs_of(g, which, c[7], c[6])
    n = U.written_elems(jobs)
    assert packed.numel() == U.packed_elems(g, which) and (which or n == packed.numel())
    unwritten = bits(packed) == -1
    assert not bool(unwritten[:n].any()), "a word of the packed layout was never written"
    assert bool(unwritten[n:].all()), "a store past the last job's rows"
    return n


# ---- 1. forward layout: both packers give the same bits ---------------------------------------------------------------------
@pytest.mark.parametrize("case", U.PACK_CASES, ids=U.case_id)
def test_forward_layout_equals_the_single_packer(hip, case):
    g = U.geom(case)
    w_src = ramp(case)
    wd, wfd = dev(w_src), dev(padded(case, w_src))
    ps = new_set(hip, [(g, 0, wd)])
    ps.run()
    n = written_exactly(case, 0, ps.packed[0])
    ref = dev_empty(n)
    bits(ref).fill_(-1)
    d = g.desc()
    _lib.check(hip.lib.rsp_conv3d_pack_fwd(C.byref(d), _ptr(wfd), _ptr(ref), _stream()), "rsp_conv3d_pack_fwd")
    hip.lib.rsp_conv3d_pack_forget(_ptr(ref))
    assert not bool((bits(ref) == -1).any())
    assert torch.equal(bits(ps.packed[0]), bits(ref)), "pack_batch_kernel and the single-convolution packer differ in some bit"


# ---- 2. packing is a permutation ---------------------------------------------------------------------------------------------
def _live_words(c, wb):
    """The source's words (int32) at the taps some non-empty class of the input gradient holds: all of them, except where the
    grid is too small for a residue (case 16)."""
    T = c[8][0] * c[8][1] * c[8][2]
    live = sorted((t * c[8][1] + h) * c[8][2] + w for t, h, w in U.live_taps(c))
    return wb.reshape(wb.shape[0], wb.shape[1], T)[:, :, live]


SPECIALS = [0x7FC00001, 0x7FA5A5A5, 0x7F800000, 0xFF800000, 0x80000000, 0x00000123]      # two NaNs, +Inf, -Inf, -0.0, a denormal


def _plant_specials(c, w_src):
    """... written as words at live taps of six different filters (no float arithmetic touches them on the way)."""
    live = sorted(U.live_taps(c))
    w = w_src.clone()
    wb = w.view(torch.int32)
    for i, word in enumerate(SPECIALS):
        t, h, x = live[(i * 5) % len(live)]
        wb[(i * 7) % w.shape[0], (i * 5 + 1) % w.shape[1], t, h, x] = word - (1 << 32) if word >= (1 << 31) else word
    return w


@pytest.mark.parametrize("special", [False, True], ids=["ramp", "nonfinite"])
@pytest.mark.parametrize("case", U.PACK_CASES, ids=U.case_id)
def test_packing_is_a_permutation(hip, case, special):
    """The non-zero words of a packed layout are the source's words, each once; the rest of what the jobs own is +0.0.  Bits, not
    values: NaN payloads, infinities, -0.0 and a denormal pass through unchanged."""
    g = U.geom(case)
    w_src = _plant_specials(case, ramp(case)) if special else ramp(case)
    assert int((bits(w_src) == 0).sum()) == 0
    wd = dev(w_src)
    ps = new_set(hip, [(g, 0, wd), (g, 1, wd)])
    ps.run()
    for which, packed in ((0, ps.packed[0]), (1, ps.packed[1])):
        n = written_exactly(case, which, packed)
        src = (bits(w_src) if which == 0 else _live_words(case, bits(w_src))).flatten()
        got = bits(packed)[:n].cpu()
        nz = got[got != 0]
        assert nz.numel() == src.numel() and int((got == 0).sum()) == n - src.numel(), (which, nz.numel(), src.numel(), n)
        assert torch.equal(torch.sort(nz).values, torch.sort(src).values), f"which={which}: not the source's words"
    assert torch.equal(bits(wd).cpu(), bits(w_src)), "the source changed"


# ---- 3. packed input gradient -------------------------------------------------------------------------------------------------
DGRAD_CASES = [c for c in U.PACK_CASES if c[4] > 4]


@functools.lru_cache(maxsize=None)
def _dgrad_operands(case):
    """(w_src, w_full, dy, fp64 reference of dx) of a case, computed once (the guarded run uses them again; nobody writes them).
    Weights drawn as the kernel tests draw them: the 2e-5 of the per-kernel suite is a bound for such operands."""
    N, D, H, W, Cin, Cout, cin_src, cout_src, k, s, p = case
    g = U.geom(case)
    w_src = K.rnd(cout_src, cin_src, *k, seed=42, scale=(Cin * k[0] * k[1] * k[2]) ** -0.5)
    w_full = padded(case, w_src)
    dy = K.rnd(N, *g.out_dims, Cout, seed=43)
    opad = tuple(i - ((o - 1) * ss - 2 * pp + kk) for i, o, ss, pp, kk in zip((D, H, W), g.out_dims, s, p, k))
    ref = torch.nn.functional.conv_transpose3d(dy.double().permute(0, 4, 1, 2, 3), w_full.double(), None, s, p, opad)
    return w_src, w_full, dy, ref.permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("case", DGRAD_CASES, ids=U.case_id)
def test_packed_dgrad(hip, case):
    """conv_dgrad_packed over the batched packer's buffer: the bits of conv_dgrad (which packs for itself), and the fp64
    transposed convolution at the per-kernel tolerance.  The tail of the packed buffer is the NaN pattern meanwhile."""
    g = U.geom(case)
    w_src, w_full, dy, ref = _dgrad_operands(case)
    wd, wfd, dyd = dev(w_src), dev(w_full), dev(dy)
    ps = new_set(hip, [(g, 1, wd)])
    ps.run()
    written_exactly(case, 1, ps.packed[0])
    dx = hip.conv_dgrad_packed(g, dyd, ps.packed[0])
    dx_own = hip.conv_dgrad(g, dyd, wfd)
    assert tuple(dx.shape) == tuple(ref.shape)
    K.close(dx, ref, 2e-5, "dgrad over the batched re-pack")
    assert torch.equal(bits(dx), bits(dx_own)), "conv_dgrad_packed and conv_dgrad differ in some bit"


def _ids(c):
    return "x".join(map(str, c[:6])) + f"k{c[6]}s{c[7]}p{c[8]}"


def _dgrad_bits(hip, case):
    N, D, H, W, Cin, Cout, k, s, p = case
    g = ConvGeom(N, D, H, W, Cin, Cout, k, s, p)
    gen = torch.Generator(device=DEV).manual_seed(7)
    w = torch.randn(Cout, Cin, *k, device=DEV, generator=gen) * 0.05
    dy = torch.randn(N, *g.out_dims, Cout, device=DEV, generator=gen)
    ps = hip.pack_set([(g, 1, w)])
    bits(ps.packed[0]).fill_(-1)
    ps.run()
    dx = hip.conv_dgrad_packed(g, dy, ps.packed[0])
    kp = hip.lib.rsp_last_conv_kernel().decode()
    dx_own = hip.conv_dgrad(g, dy, w)
    assert kp == hip.lib.rsp_last_conv_kernel().decode()
    assert torch.equal(bits(dx), bits(dx_own)), "conv_dgrad_packed and conv_dgrad differ in some bit"


@pytest.mark.parametrize("case", [c for c in K.CONV_CASES + K._fuzz_cases() + K._fuzz_depth_cases() if c[4] > 4], ids=_ids)
def test_packed_dgrad_bits_at_the_kernel_suites_cases(hip, case):
    """conv_dgrad is held to the reference at these cases by test_kernels_gpu; here only: the same bits from the packed route."""
    _dgrad_bits(hip, case)


@pytest.mark.parametrize("case", K.TALL_CASES + K.NARROW32_CASES, ids=_ids)
def test_packed_dgrad_bits_at_the_tall_and_narrow32_cases(hip, case):
    with hip.options(**({"tall_min_tiles": 2, "narrow32_max_units": 0} if case in K.TALL_CASES else {})):
        _dgrad_bits(hip, case)


# ---- 4. one table, many jobs --------------------------------------------------------------------------------------------------
def _table_order():
    """All cases, the two stem layouts between GEMM layouts and case 18 (576 rows) in the middle of the table."""
    order = [1, 19, 2, 20] + list(range(3, 19)) + [21]
    assert sorted(order) == list(range(1, 22)) and order.index(18) not in (0, 20)
    return [U.PACK_CASES[n - 1] for n in order]


def test_one_table_many_jobs(hip):
    """Every case x both layouts in ONE PackSet (21 forward jobs in one launch, 47 dgrad jobs in the other): each buffer holds the
    bits of its own one-entry set.  grid.x is sized for the 576-row job; the stem jobs' 2 and 4 blocks and the 4-row dgrad jobs run
    beside it, the surplus workgroups exit."""
    cases = _table_order()
    srcs = [dev(ramp(c)) for c in cases]
    entries = [(U.geom(c), which, w) for c, w in zip(cases, srcs) for which in (0, 1)]
    ps = new_set(hip, entries)
    assert ps.max_blocks[0] >= 576 and ps.tables[0][1] == 21 and ps.tables[1][1] == 47
    small = [U.jobs_of(U.geom(c), 0, c[7], c[6])[1][0].blocks for c in cases]
    assert min(small) <= 4 and max(small) == ps.max_blocks[0]
    ps.run()
    i = 0
    for c, w in zip(cases, srcs):
        for which in (0, 1):
            written_exactly(c, which, ps.packed[i])
            one = new_set(hip, [(U.geom(c), which, w)])
            one.run()
            assert torch.equal(bits(ps.packed[i]), bits(one.packed[0])), (U.case_id(c), which)
            i += 1


# ---- 5. re-run after an in-place update ---------------------------------------------------------------------------------------
RERUN = [3, 8, 10, 13, 19, 21]


def test_rerun_after_an_in_place_update(hip):
    """The job table holds the weights' addresses, not their values: after w.mul_(-0.5) the same set re-packs the new values — run()
    again, and a graph of run() captured BEFORE the update (one stream, two kernel nodes in a line)."""
    cases = [U.PACK_CASES[n - 1] for n in RERUN]
    srcs = [dev(ramp(c)) for c in cases]
    entries = [(U.geom(c), which, w) for c, w in zip(cases, srcs) for which in (0, 1)]
    ps = new_set(hip, entries)
    ps.run()
    before = [t.clone() for t in ps.packed]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ps.run()
    torch.cuda.current_stream().wait_stream(side)
    for w in srcs:
        w.mul_(-0.5)
    fresh = new_set(hip, [(U.geom(c), which, dev(ramp(c, -0.5))) for c in cases for which in (0, 1)])
    fresh.run()
    for how in ("run", "replay"):
        for t in ps.packed:
            bits(t).fill_(-1)
        ps.run() if how == "run" else graph.replay()
        torch.cuda.synchronize()
        for (g, which, _), got, want, old in zip(entries, ps.packed, fresh.packed, before):
            assert torch.equal(bits(got), bits(want)), (how, g, which)
            assert not torch.equal(bits(got), bits(old))


# ---- 6. shared layouts --------------------------------------------------------------------------------------------------------
def test_a_packed_buffer_serves_every_geometry_of_its_signature(hip):
    mk = lambda N, D, H, W: ConvGeom(N, D, H, W, 64, 128, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    a, b = mk(2, 4, 8, 8), mk(3, 5, 9, 9)
    w = dev(K.rnd(128, 64, 3, 3, 3, seed=61, scale=(64 * 27) ** -0.5))
    assert hip.pack_signature(a, 1, w) == hip.pack_signature(b, 1, w)
    pa, pb = new_set(hip, [(a, 1, w)]), new_set(hip, [(b, 1, w)])
    pa.run()
    pb.run()
    assert torch.equal(bits(pa.packed[0]), bits(pb.packed[0]))
    dy = dev(K.rnd(3, *b.out_dims, 128, seed=62))
    assert torch.equal(bits(hip.conv_dgrad_packed(b, dy, pa.packed[0])), bits(hip.conv_dgrad_packed(b, dy, pb.packed[0])))
    assert torch.equal(bits(hip.conv_dgrad_packed(b, dy, pa.packed[0])), bits(hip.conv_dgrad(b, dy, w)))


# ---- 7. stem mark life cycle --------------------------------------------------------------------------------------------------
def test_stem_mark_follows_what_was_packed_into_the_address(hip):
    """One packed stem buffer through: jobs from a 3-channel source (marked: the three-k-step instance, input channel 3 ignored) ->
    rsp_conv3d_pack_fwd of 4-channel filters into the SAME address (mark withdrawn: four steps, channel 3 counts) -> marked again,
    rsp_conv3d_pack_forget, jobs from the 4-channel source."""
    case = U.PACK_CASES[18]
    g = U.geom(case)
    lib, d = hip.lib, g.desc()
    x = dev(K.rnd(g.N, g.Di, g.Hi, g.Wi, 4, seed=71))
    x0 = x.clone()
    x0[..., 3] = 0
    w4 = dev(K.rnd(64, 4, 3, 3, 3, seed=72, scale=0.1))
    w3 = w4[:, :3].contiguous()
    w3p = w4.clone()
    w3p[:, 3] = 0
    assert bool((x[..., 3] != 0).all()) and bool((w4[:, 3] != 0).all())
    buf = dev_empty(U.packed_elems(g, 0))

    def pack_by_jobs(w):
        jobs = (_lib.PackJob * 64)()
        cnt = lib.rsp_conv3d_pack_jobs(C.byref(d), 0, w.shape[0], w.shape[1], _ptr(w), _ptr(buf), jobs, 64)
        assert cnt == 1 and jobs[0].kind == 1, lib.rsp_last_error()
        table = dev(torch.frombuffer(bytearray(bytes(jobs)[:C.sizeof(_lib.PackJob)]), dtype=torch.uint8))
        bits(buf).fill_(-1)
        _lib.check(lib.rsp_pack_run(_ptr(table), 1, jobs[0].blocks, _stream()), "rsp_pack_run")
        torch.cuda.synchronize()
        assert not bool((bits(buf) == -1).any())

    def fwd(xx, wp):
        y, _ = hip.conv_fwd(g, xx, wp, None, False)
        return y, lib.rsp_last_conv_kernel().decode()

    try:
        y4_ref, n4 = fwd(x, hip.conv_pack_fwd(g, w4))               # four-channel filters in a fresh buffer
        y3_ref, n3 = fwd(x0, hip.conv_pack_fwd(g, w3p))             # channel 3 gone from both operands, four steps
        assert n4.endswith(", 4>") and n3.endswith(", 4>") and not torch.equal(y4_ref, y3_ref)
        pack_by_jobs(w3)
        y, name = fwd(x, buf)
        assert name.startswith("stem_") and name.endswith(", 3>"), name
        assert torch.equal(bits(y), bits(y3_ref)), "the three-step instance must ignore input channel 3"
        bits(buf).fill_(-1)
        _lib.check(lib.rsp_conv3d_pack_fwd(C.byref(d), _ptr(w4), _ptr(buf), _stream()), "rsp_conv3d_pack_fwd")
        y, name = fwd(x, buf)
        assert name.endswith(", 4>"), name
        assert torch.equal(bits(y), bits(y4_ref)), "four-channel filters in a buffer that was marked three-channel"
        pack_by_jobs(w3)
        assert fwd(x, buf)[1].endswith(", 3>")
        lib.rsp_conv3d_pack_forget(_ptr(buf))
        assert fwd(x, buf)[1].endswith(", 4>"), "the mark outlived rsp_conv3d_pack_forget"
        pack_by_jobs(w4)
        y, name = fwd(x, buf)
        assert name.endswith(", 4>"), name
        assert torch.equal(bits(y), bits(y4_ref))
    finally:
        lib.rsp_conv3d_pack_forget(_ptr(buf))


# ---- 8. guarded memory: a source the header promises no more than float alignment for ------------------------------------------
UNALIGNED = [3, 6, 9, 12, 19, 21]


def test_source_weight_at_a_four_byte_aligned_address(hip):
    """Both layouts of six cases from sources that start 4 bytes into a 16-byte aligned block (w_ref is a float pointer and no
    more), inside guarded memory: the forward buffers fully written, the dgrad buffers written exactly up to sum O x Kld, no band
    byte changed, the sources unchanged, and the bits of the same sets over aligned sources."""
    cases = [U.PACK_CASES[n - 1] for n in UNALIGNED]
    with Guarded(DEV) as G:
        srcs, keep = [], []
        for c in cases:
            w = ramp(c)
            t = G.alloc((w.numel() + 1,), name=f"w of case {U.PACK_CASES.index(c) + 1}")[1:]
            assert t.data_ptr() % 8 == 4
            t.copy_(w.flatten())
            srcs.append(t.view(w.shape))
            keep.append(bits(t).clone())
        entries = [(U.geom(c), which, w) for c, w in zip(cases, srcs) for which in (0, 1)]
        ps = hip.pack_set(entries)
        for (g, which, _), t in zip(entries, ps.packed):
            if which:
                G.allow_unwritten(t)
        ps.run()
        G.check()
        for c, w, b in zip(cases, srcs, keep):
            assert torch.equal(bits(w).flatten(), b), "a source changed"
        i = 0
        for c in cases:
            wa = G.put(ramp(c))
            for which in (0, 1):
                written_exactly(c, which, ps.packed[i])
                one = hip.pack_set([(U.geom(c), which, wa)])
                if which:
                    G.allow_unwritten(one.packed[0])
                one.run()
                assert torch.equal(bits(ps.packed[i]), bits(one.packed[0])), (U.case_id(c), which)
                i += 1
        G.check()
