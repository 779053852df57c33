"""CPU: the C-ABI library loads and exports exactly the symbols include/rspnet_hip.h declares (no compute calls)."""
import ctypes
import os
import re

from rspnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    text = open(os.path.join(ROOT, "include", "rspnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rsp_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert header_functions() == sorted(_lib.SIGNATURES)


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    for name in header_functions():
        assert getattr(lib, name) is not None, name
    assert lib.rsp_version() >= 100
    assert lib.rsp_strerror(-2) == b"workspace too small"


def test_geometry_queries_without_gpu():
    lib = _lib.load()
    d = _lib.ConvDesc(32, 16, 56, 56, 64, 16, 56, 56, 128, 3, 3, 3, 1, 1, 1, 1, 1, 1, 64, 128)
    assert lib.rsp_conv3d_packed_fwd_elems(ctypes.byref(d)) == 128 * 27 * 64
    assert lib.rsp_conv3d_stat_tiles(ctypes.byref(d)) == 32 * 16 * 56 * 56 // 128
    bad = _lib.ConvDesc(32, 16, 56, 56, 64, 15, 56, 56, 128, 3, 3, 3, 1, 1, 1, 1, 1, 1, 64, 128)   # wrong Do
    assert lib.rsp_conv3d_packed_fwd_elems(ctypes.byref(bad)) == 0
    # invalid descriptor / null pointers are rejected before any launch
    assert lib.rsp_conv3d_fwd(ctypes.byref(bad), None, None, None, None, None, None, 0, None) == -1
    assert b"descriptor" in lib.rsp_last_error()


# the ten names version 120 exported and 130 does not, spelled stem + retired suffix: a search of the tree for a retired name finds nothing
RETIRED = [stem + suffix for stem, suffixes in (
    ("rsp_bn_finalize", ("_v", "_x")), ("rsp_bn_act_pool_bwd", ("_v", "_g")), ("rsp_conv3d_wgrad", ("_v", "_t")),
    ("rsp_bn_act_pool", ("_gate_fwd",)), ("rsp_bn_act_maxpool", ("_gate_fwd",)), ("rsp_bn_stat", ("s", "_tiles"))) for suffix in suffixes]


def test_version_130_has_one_entry_point_per_operation():
    """rsp_version() 130 folded the suffixed variants into the plain names: none of the old symbols is exported any more."""
    lib = _lib.load()
    assert lib.rsp_version() == 130
    assert len(RETIRED) == 10
    for name in RETIRED:
        assert not hasattr(lib, name), name
        assert name not in _lib.SIGNATURES


def test_folded_entry_points_reject_bad_arguments_before_any_launch():
    """The union of the argument checks of the former variants, through the one entry point each operation has now: RSP_EINVAL
    with the plain name in rsp_last_error(), on dummy pointers (nothing is dereferenced, nothing is launched)."""
    lib = _lib.load()
    P = ctypes.c_void_p(1 << 20)      # non-null, 16-byte aligned, never touched
    Cin, Cout = 8, 12
    d = _lib.ConvDesc(2, 4, 6, 6, Cin, 4, 6, 6, Cout, 3, 3, 3, 1, 1, 1, 1, 1, 1, Cin, Cout)
    wgrad = lambda dbias, cov, civ: lib.rsp_conv3d_wgrad(ctypes.byref(d), P, P, P, dbias, cov, civ, None, P, 1 << 30, None)
    for args, what in (((None, 0, Cin), b"valid channel counts"), ((None, Cout + 1, Cin), b"valid channel counts"),
                       ((P, Cout, Cin - 1), b"bias gradient")):
        assert wgrad(*args) == -1, args
        err = lib.rsp_last_error()
        assert err.startswith(b"rsp_conv3d_wgrad: ") and what in err, err
    C_ = 16
    pd = _lib.PoolDesc(2, 4, 6, 6, C_, 4, 6, 6, 1, 1, 1, 1, 1, 1, 0, 0, 0, C_, C_, C_)
    bwd = lambda c_valid, gate, dmean: lib.rsp_bn_act_pool_bwd(ctypes.byref(pd), P, None, P, P, P, P, 1, P, None, P, P, c_valid, gate,
                                                                dmean, P, 1 << 30, None)
    for args, what in (((C_, P, None), b"needs dmean"), ((0, None, None), b"valid channel count")):
        assert bwd(*args) == -1, args
        err = lib.rsp_last_error()
        assert err.startswith(b"rsp_bn_act_pool_bwd: ") and what in err, err
    assert lib.rsp_bn_finalize(P, 4, C_, C_ + 1, C_, 288, None, P, P, 1e-5, 0.1, P, P, None, P, P, P, 1 << 30, None) == -1
    err = lib.rsp_last_error()
    assert err.startswith(b"rsp_bn_finalize: ") and b"bad size" in err, err


def test_ops_fail_loudly_without_gpu_tensors():
    import pytest
    import torch
    from rspnet_amd import ops
    be = ops.HipOps()
    with pytest.raises(_lib.RspError):
        be.momentum_update(torch.zeros(8), torch.zeros(8), 0.9)


def test_missing_library_is_a_hard_error(monkeypatch):
    """No CPU / eager fallback: without the built .so every op backend construction raises."""
    import pytest
    from rspnet_amd import ops
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/librspnet_hip.so")
    with pytest.raises(_lib.RspError):
        _lib.load()
    with pytest.raises(_lib.RspError):
        ops.HipOps()


def test_constant_division_matches_integer_division():
    """The conv kernels decode rows / k positions with multiply-high by a host-computed magic number (conv_igemm.hip FastDiv);
    the same arithmetic evaluated on the host must equal n // d for every divisor a descriptor can produce, up to 2^31 - 1."""
    import numpy as np
    lib = _lib.load()
    rng = np.random.default_rng(7)
    divisors = sorted(set(list(range(1, 130)) + [143, 144, 160, 192, 208, 224, 230, 232, 288, 343, 384, 460, 480, 512, 528, 832, 921,
                                                  1024, 2048, 4095, 4096, 4097, 65535, 65536, 1 << 20, (1 << 20) + 1, (1 << 30) - 1,
                                                  1 << 30, (1 << 31) - 1] + [int(x) for x in rng.integers(1, 1 << 31, 40)]))
    top = (1 << 31) - 1
    for d in divisors:
        ns = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, top, top - 1, top - d, (top // d) * d, (top // d) * d - 1}
        ns |= {int(x) for x in rng.integers(0, 1 << 31, 64)}
        ns |= {k * d - 1 for k in rng.integers(1, max(2, top // d), 16)} | {k * d for k in rng.integers(1, max(2, top // d), 16)}
        for n in ns:
            n = int(n)
            if 0 <= n <= top:
                assert lib.rsp_fastdiv_check(d, n) == n // d, (d, n)


def test_tile_plan_option_changes_the_dispatch_not_the_interface():
    """rsp_conv3d_set_option("narrow_max_tiles", v): launches of less than one round of 128-wide tiles run on the 64-wide tile by
    default; 0 switches that off (the parity tests' second evaluation order), a negative value restores the default.  Host
    arithmetic only: checked through the dispatch predictor."""
    lib = _lib.load()
    d = _lib.ConvDesc(16, 4, 14, 14, 528, 4, 14, 14, 448, 1, 1, 1, 1, 1, 1, 0, 0, 0, 528, 448)      # S3D-G 14 x 14 pointwise: 98 x 4 tiles
    big = _lib.ConvDesc(32, 8, 28, 28, 256, 8, 28, 28, 256, 3, 3, 3, 1, 1, 1, 1, 1, 1, 256, 256)    # C3D conv3b: 1568 x 2 tiles
    name = lambda dd: lib.rsp_conv3d_kernel_name(ctypes.byref(dd), 0).decode()
    assert name(d).startswith("igemm_persist_kernel<128, 64,") and name(big).startswith("igemm_persist_kernel<128, 128,")
    prev = lib.rsp_conv3d_set_option(b"narrow_max_tiles", 0)
    try:
        assert prev == 512
        assert name(d).startswith("igemm_persist_kernel<128, 128,") and name(big).startswith("igemm_persist_kernel<128, 128,")
    finally:
        assert lib.rsp_conv3d_set_option(b"narrow_max_tiles", -1) == 0
    assert name(d).startswith("igemm_persist_kernel<128, 64,")
    # round 6: launches of less than one 128 x 64 unit per CU take the 32-wide tile (whole K per unit, no reduce launch); 33..64-column
    # launches of at least a round of 256-row tiles take the 256 x 64 instance
    tiny = _lib.ConvDesc(16, 4, 14, 14, 512, 4, 14, 14, 64, 1, 1, 1, 1, 1, 1, 0, 0, 0, 512, 64)       # S3D-G branch3 pointwise: 98 tiles
    tall = _lib.ConvDesc(32, 8, 28, 28, 64, 8, 28, 28, 64, 3, 3, 3, 1, 1, 1, 1, 1, 1, 64, 64)         # R3D-18 layer1: 784 tiles of 256 rows
    assert name(tiny).startswith("igemm_persist_kernel<128, 32,") and name(tall) == "igemm_persist_kernel<128, 64, 2, 2, true, 4>"
    assert lib.rsp_conv3d_set_option(b"narrow32_max_units", 0) == 256 and lib.rsp_conv3d_set_option(b"tall_min_tiles", 768) == 0
    try:
        assert name(tiny).startswith("igemm_persist_kernel<128, 64,") and name(tall) == "igemm_persist_kernel<256, 64, 4, 1, true, 3>"
    finally:
        assert lib.rsp_conv3d_set_option(b"narrow32_max_units", -1) == 0 and lib.rsp_conv3d_set_option(b"tall_min_tiles", -1) == 768
    assert name(tiny).startswith("igemm_persist_kernel<128, 32,") and name(tall).startswith("igemm_persist_kernel<128, 64,")
    assert lib.rsp_conv3d_set_option(b"no_such_option", 1) == -1 and b"unknown option" in lib.rsp_last_error()


# the option table of rsp_conv3d_set_option (csrc/common.h RSP_CONV_OPTIONS): name, environment variable, flag?, built-in default
CONV_OPTIONS = [("narrow_max_tiles", "RSP_NARROW_MAX_TILES", False, 512), ("narrow32_max_units", "RSP_NARROW32_MAX_UNITS", False, 256),
                ("tall_min_tiles", "RSP_TALL_MIN_TILES", False, 0), ("two_level_min_chunks", "RSP_TWO_LEVEL_MIN_CHUNKS", False, 0),
                ("direct_max_tiles", "RSP_DIRECT_MAX_TILES", False, 0), ("no_persist", "RSP_NO_PERSIST", True, 0),
                ("no_half_block", "RSP_NO_HALF_BLOCK", True, 0), ("no_pad_skip", "RSP_NO_PAD_SKIP", True, 0),
                ("no_dmajor", "RSP_NO_DMAJOR", True, 0), ("no_tm_skip", "RSP_NO_TM_SKIP", True, 0),
                ("no_multi_split", "RSP_NO_MULTI_SPLIT", True, 0)]


def test_every_conv_option_is_accepted_overridden_and_restored():
    """Each of the eleven names: its default (in a clean environment; else what the variable says) comes back as the previous
    effective value, an override is returned by the call that lifts it, and the option is back at its default afterwards."""
    lib = _lib.load()
    for name, var, flag, dflt in CONV_OPTIONS:
        want = dflt if var not in os.environ else (1 if flag else int(os.environ[var] or 0))
        assert lib.rsp_conv3d_set_option(name.encode(), 7) == want, name
        assert lib.rsp_conv3d_set_option(name.encode(), -1) == 7, name
        assert lib.rsp_conv3d_set_option(name.encode(), -1) == want, name


def test_no_memset_or_memcpy_nodes_in_the_step_kernels():
    """Round 6: a hipMemsetAsync captured into a LINEAR HIP graph (rspnet_amd/graph_step.py, "lanes") was not reliably ordered against
    the kernels around it on this stack — R3D-18's shortcut input gradients came out wrong in a few replays per hundred
    (profiles/r06/experiments_r6.txt, r6race).  Everything a captured pretext step launches from this library is therefore a KERNEL: no
    hipMemset* / hipMemcpy* in the sources of the step's ops (augment.hip is the data path: never captured)."""
    import re
    csrc = os.path.join(ROOT, "rspnet_amd", "csrc")
    bad = []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".h")) or name == "augment.hip":
            continue
        with open(os.path.join(csrc, name)) as f:
            for i, line in enumerate(f, 1):
                code = line.split("//")[0]
                if re.search(r"\bhipMem(set|cpy)\w*\s*\(", code):
                    bad.append((name, i, line.strip()))
    assert not bad, bad
