"""CPU: the deterministic-mode switch (include/mxvl.h mxvl_set_deterministic) -- the C switch, the Python mode and how _abi.launch
carries it to the library, the workspace queries, and what every entry with an order-dependent sum answers before it launches."""
import ctypes
import types

import pytest
import torch

import medical_image_analysis_amd as pkg
from medical_image_analysis_amd import _abi

NULL, SHAPE, UNSUPPORTED = -1, -3, -7


@pytest.fixture
def lib():
    """the loaded library with the switch off, and off again (Python mode back to the default) whatever the test did"""
    lib = _abi.load()
    try:
        lib.mxvl_set_deterministic(0)
        yield lib
    finally:
        lib.mxvl_set_deterministic(0)
        _abi.set_deterministic(None)
        _abi._det_lib = 0


def test_switch_returns_the_previous_value_and_round_trips(lib):
    assert lib.mxvl_set_deterministic(1) == 0
    assert lib.mxvl_set_deterministic(1) == 1
    assert lib.mxvl_set_deterministic(7) == 1                     # any non-zero value is "on" ...
    assert lib.mxvl_set_deterministic(0) == 1                     # ... and reads back as 1
    assert lib.mxvl_set_deterministic(0) == 0


def test_python_mode_follows_torch_unless_overridden(lib, monkeypatch):
    flag = [False]
    monkeypatch.setattr(torch, "are_deterministic_algorithms_enabled", lambda: flag[0])
    pkg.set_deterministic(None)
    assert pkg.is_deterministic() is False
    flag[0] = True
    assert pkg.is_deterministic() is True                         # read at each call, not at set time
    pkg.set_deterministic(False)
    assert pkg.is_deterministic() is False
    flag[0] = False
    pkg.set_deterministic(True)
    assert pkg.is_deterministic() is True
    pkg.set_deterministic(None)
    assert pkg.is_deterministic() is False
    with pytest.raises(TypeError):
        pkg.set_deterministic(1)


def test_launch_pushes_the_mode_to_the_library_before_the_call(lib, monkeypatch):
    """a stub library and a no-op device guard (the technique of test_abi.py): the switch is set before the entry runs, and only
    when the mode changed"""
    events = []

    class Guard:
        def __init__(self, device):
            pass

        def __enter__(self):
            pass

        def __exit__(self, *exc):
            pass

    def set_det(on):
        events.append(("set", on))
        return 0

    stub = types.SimpleNamespace(mxvl_ok=lambda *a: events.append(("call", a)) or 0, mxvl_set_deterministic=set_det)
    monkeypatch.setattr(_abi, "_lib", stub)
    monkeypatch.setattr(_abi, "_det_lib", 0)
    monkeypatch.setattr(torch.cuda, "device", Guard)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0x1000))
    flag = [False]
    monkeypatch.setattr(torch, "are_deterministic_algorithms_enabled", lambda: flag[0])

    _abi.launch("mxvl_ok", 1, device="cuda:0")
    assert events == [("call", (1, 0x1000))]                      # off and never changed: the library is not told anything
    del events[:]
    _abi.set_deterministic(True)
    _abi.launch("mxvl_ok", 2, device="cuda:0")
    _abi.launch("mxvl_ok", 3, device="cuda:0")
    assert events == [("set", 1), ("call", (2, 0x1000)), ("call", (3, 0x1000))]
    del events[:]
    _abi.set_deterministic(None)                                  # follows torch: off, then on
    _abi.launch("mxvl_ok", 4, device="cuda:0")
    flag[0] = True
    _abi.launch("mxvl_ok", 5, device="cuda:0")
    assert events == [("set", 0), ("call", (4, 0x1000)), ("set", 1), ("call", (5, 0x1000))]
    del events[:]
    with pytest.raises(AttributeError):                           # an unknown entry still raises before anything is called
        _abi.launch("mxvl_no_such_entry", 1, device="cuda:0")
    assert events == []


def _scan_desc(batch, dim, L, N, G, z=True, fold=False):
    d = _abi.ScanDesc()
    d.batch, d.dim, d.seqlen, d.dstate, d.n_groups, d.io_dtype = batch, dim, L, N, G, _abi.MXVL_BF16
    d.flags = _abi.SCAN_FOLD_BATCH if fold else 0
    d.u = d.delta = d.A = d.B = d.C = 4096                        # fake non-null pointers, never dereferenced
    d.z = 4096 if z else None
    d.u_bs = d.delta_bs = d.z_bs = dim * L
    d.u_ds = d.delta_ds = d.z_ds = L
    d.B_bs = d.C_bs = G * N * L
    d.B_gs = d.C_gs = N * L
    d.B_ns = d.C_ns = L
    d.A_ds, d.A_ns = N, 1
    return d


def _scan_ws_formula(batch, dim, L, N, G, z, fold):
    """the formula of include/mxvl.h (mxvl_set_deterministic), restated"""
    dpg = dim // G
    tile_rows, passes = 16, 1
    if not fold and dpg % 32 == 0 and batch * G * (dpg // 32) >= 256 and N <= 40:    # 16-bit rows (_scan_desc): dstate <= 40
        tile_rows = 32
    if N == 1 and not z and not fold:
        rw = min(max(batch * dim // 8192, 8), 64)
        while rw > 1 and dpg % (4 * rw) != 0:
            rw -= 1
        if dpg % (4 * rw) == 0:
            tile_rows, passes = min(tile_rows, 4 * rw), -(-L // 256)
    tiles = -(-dpg // tile_rows)
    return 4 * (2 * tiles * batch * G * N * L + batch * passes * dim * (N + 2))


SCAN_SHAPES = [(3, 192, 300, 16, 2, True, False),                 # multi-tile, multi-batch, grouped: 6 tiles of 16 rows per group
               (16, 2048, 4080, 16, 1, True, False),              # the ARM-large step: the 8-wave walk, 64 tiles of 32 rows
               (2, 2048, 4096, 16, 1, True, False),               # 128 32-row tiles: too few for the 8-wave walk, 128 tiles of 16 rows
               (16, 2048, 200, 40, 1, True, False),               # the last dstate whose 32 parked rows fit the LDS: the 8-wave walk
               (16, 2048, 200, 48, 1, True, False),               # the 8-wave walk's LDS does not fit: 128 tiles of 16 rows
               (18, 96, 200, 16, 1, True, True),                  # folded
               (3, 96, 1100, 1, 1, False, False),                 # dstate 1 without z: rw 8, 16-row bound, 5 passes of 256 steps
               (2, 24, 520, 1, 2, False, False),                  # dstate 1, 12 channels per group: rw 3 -> 12-row tiles
               (2, 6, 64, 1, 1, False, False)]                    # dstate 1, 4 does not divide dim / n_groups: the general kernels


@pytest.mark.parametrize("shape", SCAN_SHAPES)
def test_scan_workspace_query_is_zero_when_off_and_the_headers_formula_when_on(lib, shape):
    d = _scan_desc(*shape)
    assert lib.mxvl_scan_bwd_workspace_bytes(ctypes.byref(d)) == 0
    lib.mxvl_set_deterministic(1)
    assert lib.mxvl_scan_bwd_workspace_bytes(ctypes.byref(d)) == _scan_ws_formula(*shape)
    bad = _scan_desc(*shape)
    bad.dim = 0
    assert lib.mxvl_scan_bwd_workspace_bytes(ctypes.byref(bad)) == -1
    lib.mxvl_set_deterministic(0)
    assert lib.mxvl_scan_bwd_workspace_bytes(ctypes.byref(d)) == 0


def test_scan_workspace_of_the_arm_large_step_is_what_design_md_says(lib):
    """DESIGN.md's memory figure: 64 tiles x batch 16 x 16 states x 4080 steps x 4 B = 267 MB per dB / dC at d_inner 2048"""
    got = _scan_ws_formula(16, 2048, 4080, 16, 1, True, False)
    assert got == 4 * (2 * 64 * 16 * 16 * 4080 + 16 * 2048 * 18) and 5.3e8 < got < 5.4e8


def test_scan_bwd_refuses_a_missing_or_short_workspace_before_any_launch(lib):
    b = _abi.ScanBwdDesc()
    b.fwd = _scan_desc(3, 192, 128, 16, 2)                         # one chunk: no checkpoint needed
    b.dout = b.du = b.ddelta = b.dz = b.dA = b.dB = b.dC = 4096
    need = _scan_ws_formula(3, 192, 128, 16, 2, True, False)
    lib.mxvl_set_deterministic(1)
    assert lib.mxvl_scan_bwd(ctypes.byref(b), None) == NULL
    b.workspace, b.workspace_bytes = 4096, need - 1
    assert lib.mxvl_scan_bwd(ctypes.byref(b), None) == SHAPE
    b.workspace, b.workspace_bytes = 4098, need
    assert lib.mxvl_scan_bwd(ctypes.byref(b), None) == -5          # MXVL_ERR_STRIDE: not 4-byte aligned
    b.workspace, b.workspace_bytes = None, need
    assert lib.mxvl_scan_bwd(ctypes.byref(b), None) == NULL


def _conv_bwd_desc(batch, dim, L, W=4, ptr=4096):
    d = _abi.Conv1dBwdDesc()
    f = d.fwd
    f.batch, f.dim, f.seqlen, f.width, f.io_dtype, f.silu = batch, dim, L, W, _abi.MXVL_BF16, 1
    f.x_bs, f.x_ds, d.dy_bs, d.dy_ds, d.dx_bs, d.dx_ds = dim * L, L, dim * L, L, dim * L, L
    f.x = f.weight = d.dy = d.dx = d.dweight = ptr
    return d


@pytest.mark.parametrize("batch,dim,L,W,ptr,slots", [(23, 4, 200, 4, 4096, 3),      # vector short rows: 10 rows per workgroup
                                                     (11, 4, 197, 4, 4096, 3),      # staged short rows: 5 rows per workgroup
                                                     (2, 3, 1028, 4, 4096, 4),      # vector tiles: batch x 2 tiles
                                                     (2, 3, 1028, 4, 4098, 4),      # the same rows unaligned: staged tiles
                                                     (3, 5, 2049, 5, 4096, 9)])     # any width: batch x 3 tiles
def test_conv1d_workspace_query_and_refusals(lib, batch, dim, L, W, ptr, slots):
    d = _conv_bwd_desc(batch, dim, L, W, ptr)
    assert lib.mxvl_conv1d_bwd_workspace_bytes(ctypes.byref(d)) == 0
    lib.mxvl_set_deterministic(1)
    need = 4 * slots * dim * (W + 1)
    assert lib.mxvl_conv1d_bwd_workspace_bytes(ctypes.byref(d)) == need
    assert lib.mxvl_conv1d_bwd(ctypes.byref(d), None) == NULL
    d.workspace, d.workspace_bytes = 8192, need - 1
    assert lib.mxvl_conv1d_bwd(ctypes.byref(d), None) == SHAPE
    d.fwd.width = 9
    assert lib.mxvl_conv1d_bwd_workspace_bytes(ctypes.byref(d)) == -1


def test_entries_that_refuse_the_mode(lib):
    g = _abi.GemmTnDesc()
    g.M = g.N = 1024
    g.K, g.io_dtype = 32768, _abi.MXVL_BF16
    g.a_rs = g.b_rs = g.c_rs = 1024
    g.a = g.b = g.c = 4096
    m = _abi.MambaInnerBwdDesc()
    lib.mxvl_set_deterministic(1)
    assert lib.mxvl_gemm_tn(ctypes.byref(g), None) == UNSUPPORTED
    assert lib.mxvl_mamba_inner_bwd(ctypes.byref(m), None) == UNSUPPORTED
    lib.mxvl_set_deterministic(0)
    assert lib.mxvl_mamba_inner_bwd(ctypes.byref(m), None) != UNSUPPORTED        # off: the ordinary argument checks answer


def test_wgrad_takes_the_library_form_under_the_mode(lib, monkeypatch):
    """gemm_tn_takes is False under the mode for operands it accepts otherwise (meta tensors posing as device tensors: no GPU)"""
    from medical_image_analysis_amd import selective_scan_interface as ssi
    a = types.SimpleNamespace(is_cuda=True, dtype=torch.bfloat16, shape=(32768, 1024), stride=lambda i: (1024, 1)[i], data_ptr=lambda: 4096)
    assert ssi.gemm_tn_wins(32768, 1024, 1024)
    pkg.set_deterministic(False)
    assert ssi.gemm_tn_takes(a, a) is True
    pkg.set_deterministic(True)
    assert ssi.gemm_tn_takes(a, a) is False
