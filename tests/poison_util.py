"""TEST-ONLY: where a non-finite operand element must show in a kernel's output, by index arithmetic alone (numpy, no convolution).

A NaN in an operand marks exactly the outputs computed from it: the mask is independent of any tolerance, so a kernel that reads a
neighbouring element "times a zero weight" (right on finite data, inside every guard band) gets a wider mask than the one predicted
here, and one that drops a tap gets a narrower one.  tests/test_nonfinite_cpu.py checks these predictions against
torch.nn.functional.conv3d / max_pool3d in float64 before tests/test_nonfinite_gpu.py holds the HIP kernels to them.

Layouts as in rspnet_amd.ops: activations (N, D, H, W, C), weights (Cout, Cin, kT, kH, kW).  The case lists and the poison positions of
the GPU module live here too, so that the CPU module can check their caps (conditions on the inputs, not measurements)."""
import numpy as np

from rspnet_amd.ops import ConvGeom, PoolGeom


def _axis_hits(i, n_out, k, s, p):
    """(o, kt) pairs of one axis with o * s - p + kt == i, 0 <= o < n_out, 0 <= kt < k: who reads input coordinate i."""
    out = []
    for kt in range(k):
        num = i + p - kt
        if num >= 0 and num % s == 0 and num // s < n_out:
            out.append((num // s, kt))
    return out


def _axis_reads(o, n_in, k, s, p):
    """(i, kt) pairs of one axis with i == o * s - p + kt in range: what output coordinate o reads."""
    return [(o * s - p + kt, kt) for kt in range(k) if 0 <= o * s - p + kt < n_in]


def _hits3(g, d, h, w):
    """Output positions and taps that read input position (d, h, w): list of ((od, oh, ow), (kt, kh, kw))."""
    do, ho, wo = g.out_dims
    return [((od, oh, ow), (kt, kh, kw))
            for od, kt in _axis_hits(d, do, g.k[0], g.s[0], g.p[0])
            for oh, kh in _axis_hits(h, ho, g.k[1], g.s[1], g.p[1])
            for ow, kw in _axis_hits(w, wo, g.k[2], g.s[2], g.p[2])]


def _reads3(g, od, oh, ow):
    """Input positions and taps that output position (od, oh, ow) reads (padding taps left out)."""
    dims = (g.Di, g.Hi, g.Wi)
    return [((i, j, l), (kt, kh, kw))
            for i, kt in _axis_reads(od, dims[0], g.k[0], g.s[0], g.p[0])
            for j, kh in _axis_reads(oh, dims[1], g.k[1], g.s[1], g.p[1])
            for l, kw in _axis_reads(ow, dims[2], g.k[2], g.s[2], g.p[2])]


def conv_fwd_x_mask(g: ConvGeom, poisons):
    """Forward, poisoned x[n, d, h, w, ci]: every y[n, od, oh, ow, :] with a tap on it, all Cout channels."""
    m = np.zeros((g.N,) + g.out_dims + (g.Cout,), dtype=bool)
    for n, d, h, w, _ in poisons:
        for (od, oh, ow), _tap in _hits3(g, d, h, w):
            m[n, od, oh, ow, :] = True
    return m


def conv_dgrad_mask(g: ConvGeom, poisons):
    """Input gradient, poisoned dy[n, od, oh, ow, co]: every in-range dx[n, id, ih, iw, :] with id == od * sT - pT + kt for a tap."""
    m = np.zeros((g.N, g.Di, g.Hi, g.Wi, g.Cin), dtype=bool)
    for n, od, oh, ow, _ in poisons:
        for (i, j, l), _tap in _reads3(g, od, oh, ow):
            m[n, i, j, l, :] = True
    return m


def conv_wgrad_x_mask(g: ConvGeom, poisons):
    """Weight gradient, poisoned x[..., ci]: dw[:, ci, taps whose output position exists]; dbias stays finite.  (dw mask, dbias mask)"""
    m = np.zeros((g.Cout, g.Cin) + tuple(g.k), dtype=bool)
    for _, d, h, w, ci in poisons:
        for _pos, (kt, kh, kw) in _hits3(g, d, h, w):
            m[:, ci, kt, kh, kw] = True
    return m, np.zeros(g.Cout, dtype=bool)


def conv_wgrad_dy_masks(g: ConvGeom, poisons):
    """Weight gradient, poisoned dy[..., co]: (must, may, dbias mask).  must: dw[co, :, taps whose input position is in range]; may:
    all of dw[co]; dbias[co].  The mirror image of conv_fwd_w_masks: a weight gradient formed as a matrix product over output rows
    (torch's own, in float64 always and in float32 at some shapes; the HIP kernels' MFMA tiles) multiplies the NaN by the explicit
    zero that stands for a padded tap, and one operand element serves every tap of the row — neither is wrong, so the test asserts
    must <= NaN set <= may."""
    must = np.zeros((g.Cout, g.Cin) + tuple(g.k), dtype=bool)
    may = np.zeros_like(must)
    b = np.zeros(g.Cout, dtype=bool)
    for _, od, oh, ow, co in poisons:
        b[co] = True
        may[co] = True
        for _pos, (kt, kh, kw) in _reads3(g, od, oh, ow):
            must[co, :, kt, kh, kw] = True
    return must, may, b


def conv_fwd_w_masks(g: ConvGeom, poisons):
    """Forward, poisoned w[co, ci, kt, kh, kw]: (must, may).  must: channel co where that tap reads a real input element; may: all of
    channel co (a convolution over explicit padding zeros multiplies them by the NaN; one that skips or masks padding taps does not)."""
    do, ho, wo = g.out_dims
    must = np.zeros((g.N, do, ho, wo, g.Cout), dtype=bool)
    may = np.zeros_like(must)
    for co, _ci, kt, kh, kw in poisons:
        may[..., co] = True
        for od in range(do):
            if not 0 <= od * g.s[0] - g.p[0] + kt < g.Di:
                continue
            for oh in range(ho):
                if not 0 <= oh * g.s[1] - g.p[1] + kh < g.Hi:
                    continue
                for ow in range(wo):
                    if 0 <= ow * g.s[2] - g.p[2] + kw < g.Wi:
                        must[:, od, oh, ow, co] = True
    return must, may


def pool_window_mask(pg: PoolGeom, poisons):
    """Pooling, poisoned x[n, d, h, w, c]: every out[n, od, oh, ow, c] whose window holds the position (same channel only)."""
    m = np.zeros((pg.N,) + pg.out_dims + (pg.C,), dtype=bool)
    for n, d, h, w, c in poisons:
        for (od, oh, ow), _tap in _hits3(pg, d, h, w):
            m[n, od, oh, ow, c] = True
    return m


def channels_hit(mask):
    """Channels (last axis) with at least one marked element: whose summed statistics turn non-finite."""
    return mask.reshape(-1, mask.shape[-1]).any(axis=0)


# ---- the convolution cases of the GPU module --------------------------------------------------------------------------------------
# (N, D, H, W, Cin, Cout, k, s, p): the smallest of each kernel family in test_kernels_gpu.CONV_CASES
CONV_POISON_CASES = [
    (2, 4, 10, 10, 64, 128, (3, 3, 3), (1, 1, 1), (1, 1, 1)),      # tap-major 128-wide
    (2, 5, 6, 6, 83, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0)),         # scalar gather, K tail
    (3, 4, 7, 7, 128, 96, (3, 3, 3), (1, 1, 1), (1, 1, 1)),        # slice-major, padded-tap skipping, depth-major rows
    (2, 4, 8, 8, 64, 128, (3, 3, 3), (2, 2, 2), (1, 1, 1)),        # dgrad parity classes
    (1, 2, 7, 7, 256, 512, (3, 3, 3), (1, 1, 1), (1, 1, 1)),       # K split
    (2, 4, 12, 12, 64, 132, (1, 3, 3), (1, 1, 1), (0, 1, 1)),      # 16-wide half block, ragged
    (3, 4, 7, 7, 48, 72, (3, 3, 3), (2, 2, 2), (1, 1, 1)),         # 64 + 8 columns, strided
    (2, 4, 12, 12, 4, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1)),        # stem
    (2, 5, 18, 20, 4, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3)),        # stem
    (1, 1, 5, 5, 8, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1)),           # M = 25: corner poison only
]
DIRECT_CASES = [CONV_POISON_CASES[0], CONV_POISON_CASES[3], CONV_POISON_CASES[4]]
DIRECT_MAX_TILES = 448          # what test_kernels_gpu.test_conv_cases_also_pass_on_the_direct_kernel sets
TALL_CASE = (3, 4, 16, 16, 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1))      # from test_kernels_gpu.TALL_CASES: slice-major, depth-major rows
INF_CASE = CONV_POISON_CASES[0]


def case_id(c):
    return "x".join(map(str, c[:6])) + f"k{c[6]}s{c[7]}"


def _boundary_position(dims):
    """Position of row 128 of a (N, D, H, W) position grid — the first row of the second 128-row tile — moved on to the next row
    that is interior in H and W when that one lies on the frame's edge (its footprint of neighbouring rows still straddles the tile
    boundary).  None when the grid has no more than 128 rows."""
    N, D, H, W = dims
    rows = N * D * H * W
    if rows <= 128:
        return None
    pick = None
    for r in range(128, min(rows, 128 + 2 * W + 4)):
        n, rem = divmod(r, D * H * W)
        d, rem = divmod(rem, H * W)
        h, w = divmod(rem, W)
        if pick is None:
            pick = (n, d, h, w)
        if 0 < h < H - 1 and 0 < w < W - 1:
            return (n, d, h, w)
    return pick


def activation_poisons(dims, C, real_channels=None, corner_only=False):
    """The poisons of one launch on an (N, D, H, W, C) tensor, each in a different channel: element 0 (the corner, where padding is
    at its fullest), the last element (last row, last channel: K tail and ragged last tile) and, on a grid of more than 128 rows, one
    element on a 128-row tile boundary.  real_channels (stems: 3 of the 4 are real, the fourth is zero padding by contract) bounds the
    channels used."""
    N, D, H, W = dims
    cmax = (real_channels or C) - 1
    out = [(0, 0, 0, 0, 0)]
    if corner_only:
        return out
    out.append((N - 1, D - 1, H - 1, W - 1, cmax))
    mid = _boundary_position(dims)
    if mid is not None:
        out.append(mid + (max(1, cmax // 2),))
    assert len({c for *_, c in out}) == len(out), out
    return out


def conv_poisons(case):
    """(g, x poisons, dy poisons, w poison) of one convolution case.  The M = 25 case gets the corner poison alone: with two more
    the footprints would cover more than half of its outputs."""
    N, D, H, W, Cin, Cout, k, s, p = case
    g = ConvGeom(N, D, H, W, Cin, Cout, k, s, p)
    tiny = g.rows <= 25
    px = activation_poisons((N, D, H, W), Cin, 3 if Cin == 4 else None, tiny)
    pdy = activation_poisons((N,) + g.out_dims, Cout, None, tiny)
    # the weight poison: last output channel (the ragged column), last real input channel, the corner tap (padding where there is any;
    # the centre plane in depth where a single frame leaves the first plane nothing real to read)
    pw = [(Cout - 1, (3 if Cin == 4 else Cin) - 1, 0 if D > 1 else k[0] // 2, 0, 0)]
    return g, px, pdy, pw


def poison(t, coords, value=float("nan")):
    """A copy of tensor / array t with `value` at each coordinate."""
    t = t.clone() if hasattr(t, "clone") else t.copy()
    for c in coords:
        t[tuple(c)] = value
    return t


INF_POISON = (1, 2, 5, 5, 7)        # one +Inf of INF_CASE's input: interior, away from the three NaN footprints' channels


# ---- BatchNorm / pooling cases of the GPU module ----------------------------------------------------------------------------------
# train-mode chain: ((N, D, H, W, C), window, residual); the poisoned channel
TRAIN_CHAIN_CASES = [((2, 3, 5, 5, 83), (1, 1, 1), False), ((2, 4, 8, 8, 64), (1, 2, 2), False), ((2, 3, 5, 5, 64), (1, 1, 1), True)]
TRAIN_CHAIN_CHANNEL = 5
# finite scale / shift (the eval-mode situation), disjoint windows: the unit window on the scalar path, 4 and 8 positions that tile
# the input, and 8 positions over odd sizes (floor mode drops the tail)
EVAL_POOL_CASES = [PoolGeom(2, 3, 5, 5, 83), PoolGeom(2, 4, 8, 8, 64, (1, 2, 2), (1, 2, 2)), PoolGeom(2, 4, 8, 8, 64, (2, 2, 2), (2, 2, 2)),
                   PoolGeom(2, 5, 7, 7, 64, (2, 2, 2), (2, 2, 2))]
OVERLAP_POOL = PoolGeom(1, 5, 9, 11, 20, (3, 3, 3), (2, 2, 2), (1, 1, 1))
# maxpool_fwd / maxpool_bwd: the float4 sliding 3x3x3 kernel, the scalar kernel (83 channels, padded and strided), the disjoint float4 one
MAXPOOL_CASES = [PoolGeom(1, 3, 4, 9, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1)), PoolGeom(2, 4, 7, 7, 83, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
                 PoolGeom(2, 2, 6, 6, 64, (2, 2, 2), (2, 2, 2), (0, 0, 0))]
GATE_FUSED_SHAPE = (3, 2, 7, 7, 48)
GATE_SHAPE = (3, 18, 192)           # (N, P, C)


def pool_id(pg):
    return f"{pg.N}x{pg.Di}x{pg.Hi}x{pg.Wi}x{pg.C}k{pg.k}s{pg.s}p{pg.p}"


def window_poisons(pg: PoolGeom):
    """Three poisons in three different windows: the first element of the first window (channel 0), the middle element of a window
    in the middle (channel 1) and the last element of the last window (last channel).  Elements in (kt, kh, kw) scan order; a
    padded window's element is moved into range."""
    dims, outs = (pg.Di, pg.Hi, pg.Wi), pg.out_dims
    nwin = pg.k[0] * pg.k[1] * pg.k[2]

    def at(n, win, elem, c):
        kt, rem = divmod(elem, pg.k[1] * pg.k[2])
        kh, kw = divmod(rem, pg.k[2])
        pos = tuple(min(max(o * s - p + kk, 0), n_in - 1) for o, s, p, kk, n_in in zip(win, pg.s, pg.p, (kt, kh, kw), dims))
        return (n,) + pos + (c,)

    return [at(0, (0, 0, 0), 0, 0), at(0, tuple(o // 2 for o in outs), nwin // 2, 1),
            at(pg.N - 1, tuple(o - 1 for o in outs), nwin - 1, pg.C - 1)]
