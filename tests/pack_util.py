"""Case list and host-side helpers of the batched weight re-pack tests (test_pack_jobs_cpu.py, test_pack_gpu.py and the guarded
run of its bodies).  No GPU import: ctypes, the library's host queries and plain Python.

A case is (N, D, H, W, Cin, Cout, Cin_src, Cout_src, k, s, p): the geometry the packed layout is built for and the channel counts of
the SOURCE weight (Cout_src, Cin_src, kT, kH, kW), which may be smaller (the packers zero-pad).  Spatial sizes are as small as the
stride-parity class structure allows: the packers look at channels, kernel and stride only.  What each case reaches in
pack_batch_kernel (T = kT*kH*kW filters taps, CH = min(128, 4096 // T) filters staged per LDS chunk):"""
import ctypes as C

from rspnet_amd import _lib
from rspnet_amd.ops import ConvGeom

_1, _2, _0 = (1, 1, 1), (2, 2, 2), (0, 0, 0)
PACK_CASES = [
    (1, 2, 5, 5, 208, 160, 208, 160, _1, _1, _0),                      # 1  T = 1 (dcl = 256, dt = 0); C beyond one 128-filter chunk
    (1, 2, 6, 6, 64, 128, 64, 128, _1, _2, _0),                        # 2  8 parity classes, 7 with no tap: one dgrad job
    (1, 5, 4, 4, 232, 128, 230, 128, (3, 1, 1), (2, 1, 1), (1, 0, 0)),  # 3  padded input channels; classes of [1, 2] taps
    (1, 2, 6, 6, 64, 84, 64, 83, (1, 3, 3), _1, (0, 1, 1)),            # 4  padded output channel
    (1, 4, 4, 4, 84, 64, 83, 64, (3, 1, 1), _1, (1, 0, 0)),            # 5  its partner: padded row o in the dgrad layout
    (1, 2, 5, 5, 129, 130, 129, 130, (3, 3, 3), _1, _1),               # 6  last chunk of 1 filter (fwd) / 2 filters (dgrad); Kld != K
    (1, 2, 5, 5, 128, 96, 128, 96, (3, 3, 3), _1, _1),                 # 7  slice-major K, both layouts
    (1, 4, 8, 8, 32, 512, 32, 512, (3, 3, 3), _2, _1),                 # 8  8 jobs, taps [1,2,2,4,2,4,4,8]: slice-major per class
    (1, 2, 9, 9, 8, 24, 8, 24, (1, 7, 7), (1, 2, 2), (0, 3, 3)),       # 9  T = 49 (CH = 83), taps [9,12,12,16]
    (1, 3, 7, 7, 16, 40, 16, 40, (3, 5, 5), (1, 1, 2), (1, 2, 2)),     # 10 T = 75 (CH = 54), taps [45,30]
    (1, 5, 5, 5, 64, 32, 64, 32, (5, 5, 5), _1, _2),                   # 11 T = 125 (CH = 32), slice-major
    (1, 7, 7, 7, 8, 24, 8, 24, (7, 7, 7), _1, (3, 3, 3)),              # 12 T = 343 > 256: dcl = 0 in the transposed read, CH = 11
    (1, 7, 8, 8, 8, 24, 8, 24, (7, 7, 7), _2, (3, 3, 3)),              # 13 the same, 8 classes of 27 ... 64 taps
    (1, 4, 8, 8, 8, 16, 8, 16, (4, 8, 8), _1, _0),                     # 14 T = 256 exactly (dcl = 1, dt = 0)
    (1, 5, 8, 8, 12, 20, 12, 20, (5, 8, 8), (1, 2, 1), _0),            # 15 T = 320, two classes of 160
    (1, 1, 1, 1, 64, 128, 64, 128, (3, 3, 3), _2, _1),                 # 16 classes empty because the GRID is empty: one job
    (1, 2, 6, 6, 144, 288, 144, 288, (1, 3, 3), _1, (0, 1, 1)),        # 17 144 = 128 + 16 columns in dgrad
    (1, 2, 4, 4, 256, 576, 256, 576, (1, 3, 3), _1, (0, 1, 1)),        # 18 largest O (576 rows) against the smallest in one table
    (2, 4, 12, 12, 4, 64, 3, 64, (3, 3, 3), _1, _1),                   # 19 stem layout (kind == 1, 2 blocks), resident kernel
    (1, 3, 23, 17, 4, 45, 3, 45, (1, 7, 7), (1, 2, 2), (0, 3, 3)),     # 20 stem layout, Cout = 45 < 64
    (1, 5, 18, 20, 4, 64, 3, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3)),     # 21 NOT a stem at this size: Cin_src 3 of 4 on the GEMM layout, T = 343
]
# what the CPU test pins per case number (1-based): number of dgrad jobs, their tap counts, kind / blocks of the forward job
PINS = {2: {"dgrad_jobs": 1}, 8: {"dgrad_jobs": 8, "dgrad_taps": [1, 2, 2, 4, 2, 4, 4, 8]}, 16: {"dgrad_jobs": 1},
        19: {"fwd_kind": 1, "fwd_blocks": 2}, 21: {"fwd_kind": 0}}


def case_id(c):
    return f"{PACK_CASES.index(c) + 1}-" + "x".join(map(str, c[:8])) + "k" + "".join(map(str, c[8])) + "s" + "".join(map(str, c[9]))


def geom(c) -> ConvGeom:
    N, D, H, W, Cin, Cout, _, _, k, s, p = c
    return ConvGeom(N, D, H, W, Cin, Cout, k, s, p)


def src_shape(c):
    return (c[7], c[6]) + tuple(c[8])


def jobs_of(g: ConvGeom, which: int, cout_src: int, cin_src: int, max_jobs: int = 64, src=1 << 20, dst=1 << 30):
    """(return value, job records) of rsp_conv3d_pack_jobs on dummy pointers (host arithmetic only; the stem mark the call may
    leave on `dst` is withdrawn)."""
    lib = _lib.load()
    d = g.desc()
    buf = (_lib.PackJob * 64)()
    cnt = lib.rsp_conv3d_pack_jobs(C.byref(d), which, cout_src, cin_src, C.c_void_p(src), C.c_void_p(dst), buf, max_jobs)
    lib.rsp_conv3d_pack_forget(C.c_void_p(dst))
    return cnt, [buf[i] for i in range(max(cnt, 0))]


def packed_elems(g: ConvGeom, which: int) -> int:
    lib = _lib.load()
    d = g.desc()
    return int((lib.rsp_conv3d_packed_dgrad_elems if which else lib.rsp_conv3d_packed_fwd_elems)(C.byref(d)))


def written_elems(jobs) -> int:
    """Floats the jobs write: O x Kld per GEMM-layout job, `total` per stem-layout job."""
    return sum(int(j.total) for j in jobs)


def live_taps(c):
    """Kernel taps (kt, kh, kw) that some non-empty stride-parity class of the input gradient holds, from k, s, p and the input
    size alone: position i of the input (residue r = i mod s) receives tap k iff (r + p - k) mod s == 0, and residue r exists on
    the grid iff r < size."""
    _, D, H, W, _, _, _, _, k, s, p = c
    per_dim = []
    for size, kk, ss, pp in zip((D, H, W), k, s, p):
        per_dim.append([{t for t in range(kk) if (r + pp - t) % ss == 0} for r in range(min(ss, size))])
    out = set()
    for a in per_dim[0]:
        for b in per_dim[1]:
            for cw in per_dim[2]:
                out |= {(t, h, w) for t in a for h in b for w in cw}
    return out
