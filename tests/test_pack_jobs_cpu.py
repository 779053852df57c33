"""CPU: the job records rsp_conv3d_pack_jobs writes for every case of tests/pack_util.py (host arithmetic on dummy pointers: nothing
is dereferenced, nothing is launched) — what tests/test_pack_gpu.py relies on when it runs them — and the messages its rejections
leave in rsp_last_error()."""
import ctypes as C

import pytest

import pack_util as U
from rspnet_amd import _lib
from rspnet_amd.ops import ConvGeom, _pack_signature

SRC, DST = 1 << 20, 1 << 30


@pytest.mark.parametrize("case", U.PACK_CASES, ids=U.case_id)
def test_jobs_of_every_case(case):
    num = U.PACK_CASES.index(case) + 1
    pins = U.PINS.get(num, {})
    g = U.geom(case)
    cin_src, cout_src = case[6], case[7]
    n0, fwd = U.jobs_of(g, 0, cout_src, cin_src, src=SRC, dst=DST)
    assert n0 == 1 and len(fwd) == 1, "the forward layout is exactly one job"
    n1, dg = U.jobs_of(g, 1, cout_src, cin_src, src=SRC, dst=DST)
    assert 1 <= n1 <= case[9][0] * case[9][1] * case[9][2]
    for j in fwd + dg:
        assert j.ntaps >= 1 and j.src == SRC
        assert (j.Cout_src, j.Cin_src, j.kT, j.kH, j.kW) == (cout_src, cin_src) + tuple(case[8])
        if j.kind == 0:
            assert j.blocks == j.O and j.total == j.O * j.Kld
            assert j.ntaps == j.nTd * j.nTh * j.nTw and j.Kld % 4 == 0 and 0 <= j.Kld - j.ntaps * j.C < 4
    j = fwd[0]
    assert j.dst == DST
    if j.kind == 0:
        assert (j.transpose, j.O, j.C) == (0, g.Cout, g.Cin)
        assert j.total == U.packed_elems(g, 0)
    else:
        assert j.kind == 1 and j.total == U.packed_elems(g, 0) and j.blocks == (j.total + 4095) // 4096
    # the dgrad layouts: class after class from w_packed on, no gap; together no more than the allocation
    off = 0
    for j in dg:
        assert j.kind == 0 and (j.transpose, j.O, j.C) == (1, g.Cin, g.Cout)
        assert j.dst == DST + 4 * off
        off += j.O * j.Kld
    assert off == U.written_elems(dg) <= U.packed_elems(g, 1)
    assert U.packed_elems(g, 1) % 64 == 0      # (rounded up to 256 bytes)
    # every live tap of the kernel is in exactly one class
    assert sum(j.ntaps for j in dg) == len(U.live_taps(case))
    if "dgrad_jobs" in pins:
        assert n1 == pins["dgrad_jobs"]
    if "dgrad_taps" in pins:
        assert [j.ntaps for j in dg] == pins["dgrad_taps"]
    if "fwd_kind" in pins:
        assert fwd[0].kind == pins["fwd_kind"]
    if "fwd_blocks" in pins:
        assert fwd[0].blocks == pins["fwd_blocks"]


def test_the_table_reaches_what_it_says():
    """The properties the case list is chosen for, from the records themselves: a table with 576 rows beside one of at most 4
    blocks, a slice-major and a tap-major class in one dgrad set, both stem-layout cases, a filter longer than a workgroup."""
    from_case = lambda n, which: U.jobs_of(U.geom(U.PACK_CASES[n - 1]), which, U.PACK_CASES[n - 1][7], U.PACK_CASES[n - 1][6])[1]
    assert from_case(18, 0)[0].blocks == 576 and from_case(20, 0)[0].blocks <= 4
    slice_major = lambda j: j.ntaps > 1 and j.C % 32 == 0 and j.C * j.ntaps >= 48 * 32      # (k_slice_major of conv_igemm.hip)
    assert sorted({slice_major(j) for j in from_case(8, 1)}) == [False, True]
    assert slice_major(from_case(7, 0)[0]) and slice_major(from_case(7, 1)[0]) and slice_major(from_case(11, 0)[0])
    assert [from_case(n, 0)[0].kind for n in (19, 20, 21)] == [1, 1, 0]
    assert [c[8][0] * c[8][1] * c[8][2] for c in (U.PACK_CASES[n - 1] for n in (1, 9, 10, 11, 12, 14, 15))] == [1, 49, 75, 125, 343, 256, 320]


def test_pack_signature_is_shared_by_geometries_with_the_same_classes():
    mk = lambda N, D, H, W: ConvGeom(N, D, H, W, 64, 128, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    a, b, flat = mk(2, 4, 8, 8), mk(3, 5, 9, 9), mk(2, 1, 8, 8)
    for which in (0, 1):
        assert _pack_signature(a, which, 128, 64) == _pack_signature(b, which, 128, 64)
    assert U.jobs_of(a, 1, 128, 64)[0] == 8 and U.jobs_of(flat, 1, 128, 64)[0] == 4      # D = 1: the odd depth residue has no position
    assert _pack_signature(flat, 1, 128, 64) != _pack_signature(a, 1, 128, 64)
    assert _pack_signature(a, 1, 128, 63) != _pack_signature(a, 1, 128, 64)                # the source's own lengths are part of it


def test_every_rejection_leaves_a_message_naming_the_function():
    lib = _lib.load()
    g = U.geom(U.PACK_CASES[7])      # 32 -> 512, stride 2: 8 classes
    stale = ConvGeom(1, 2, 5, 5, 8, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1)).desc()

    def rejected(which, cout_src, cin_src, max_jobs):
        stale.Do += 1      # an unrelated rejection first, so that a call that sets no message shows that one's text
        assert lib.rsp_conv3d_pack_fwd(C.byref(stale), C.c_void_p(SRC), C.c_void_p(DST), None) == -1
        stale.Do -= 1
        assert lib.rsp_last_error().startswith(b"rsp_conv3d_pack_fwd: ")
        cnt, _ = U.jobs_of(g, which, cout_src, cin_src, max_jobs=max_jobs)
        assert cnt == -1
        return lib.rsp_last_error()

    for which in (0, 1):
        assert rejected(which, 513, 32, 64).startswith(b"rsp_conv3d_pack_jobs: ")      # Cout_src > Cout
        assert rejected(which, 512, 33, 64).startswith(b"rsp_conv3d_pack_jobs: ")      # Cin_src > Cin
        msg = rejected(which, 512, 32, 0)
        assert msg.startswith(b"rsp_conv3d_pack_jobs: ") and b"max_jobs" in msg
    msg = rejected(1, 512, 32, 7)                                                       # one short of the class count
    assert msg.startswith(b"rsp_conv3d_pack_jobs: ") and b"max_jobs" in msg
    assert U.jobs_of(g, 1, 512, 32, max_jobs=8)[0] == 8 and U.jobs_of(g, 0, 512, 32, max_jobs=1)[0] == 1
