"""The decode-projection dispatch as a table: mxvl_decode_gemm_plan (return code and its five output ints) and, for every descriptor
the argument checks refuse, the return code of mxvl_decode_gemv with a NULL stream, over a grid of weight formats, dtypes, row counts,
K, N and descriptor variants.  tests/golden/decode_plan_grid.npz was recorded by `record()` below from the library of the commit
BEFORE the host dispatch was folded into one weight-format visitor (csrc/decode_gemm.hip with_format); the library of this tree has to
reproduce every entry exactly.  Fake non-null pointers as in tests/test_abi.py: a refused descriptor returns from the checks, an
accepted one is only planned -- nothing is launched, no GPU needed."""
import ctypes
import itertools
import os

import numpy as np

from medical_image_analysis_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_plan_grid.npz")

_W = (_abi.MXVL_W_INT8, _abi.MXVL_W_MXFP4, _abi.MXVL_W_FP8, _abi.MXVL_W_INT4)
FLAGS = (0,) + _W + tuple(a | b for a, b in itertools.combinations(_W, 2))      # no format, each one, every pair of two
DTYPES = (_abi.MXVL_BF16, _abi.MXVL_F16, 0, 3)
ROWS = (1, 3, 8, 9, 16, 17, 18, 32, 33, 48, 80, 81)
KS = (32, 64, 72, 96, 128, 192, 256, 2048, 4096, 5504, 11008)
NS = (16, 64, 4096, 11008, 12288)
# (name, swiglu, w2_scale, split_acc, k_splits, norm_weight, out_f32, w_scale); k_splits = 1 asks for the matrix-core kernels at every
# row count, as the stepper does; "rowwise" (k_splits = 0) leaves <= 8 rows of 16-bit weights to the per-row GEMV
VARIANTS = (("rowwise", 0, 0, 0, 0, 0, 0, 1), ("plain", 0, 0, 0, 1, 0, 0, 1), ("swiglu", 1, 1, 0, 1, 0, 0, 1), ("swiglu_no_w2_scale", 1, 0, 0, 1, 0, 0, 1),
            ("split1", 0, 0, 1, 1, 0, 0, 1), ("split2", 0, 0, 1, 2, 0, 0, 1), ("split4", 0, 0, 1, 4, 0, 0, 1), ("split8", 0, 0, 1, 8, 0, 0, 1),
            ("norm", 0, 0, 0, 1, 1, 0, 1), ("out_f32", 0, 0, 0, 1, 0, 1, 1), ("w_scale_null", 0, 0, 0, 1, 0, 0, 0))
WIDE_MODES = (0, 3, 4, 5, 6)          # mxvl_set_decode_gemm_wide: the A/B modes move the 16-bit plan (bf16, "plain" only)
NOT_CALLED = 127                      # gemv column of a descriptor the plan accepts: mxvl_decode_gemv would launch it


def _sweep_one(lib, d, out, flag, dtype, rows, K, N, variant):
    _, swiglu, w2s, acc, ks, norm, f32, ws = variant
    d.rows, d.K, d.N, d.dtype, d.swiglu, d.out_f32, d.k_splits = rows, K, N, dtype | flag, swiglu, f32, ks
    d.W2 = 64 if swiglu else None
    d.w_scale, d.w2_scale = (64 if ws else None), (64 if w2s else None)
    d.split_acc, d.norm_weight = (64 if acc else None), (64 if norm else None)
    rc = lib.mxvl_decode_gemm_plan(ctypes.byref(d), out)
    # only what the plan refuses goes to the launch entry: it returns from the same checks before any launch
    return (rc,) + tuple(out) + ((lib.mxvl_decode_gemv(ctypes.byref(d), None) if rc != 0 else NOT_CALLED),)


def sweep():
    """(n, 7) int32: plan return code, kind, waves, tiles per wave, ring stages, workgroups, gemv return code -- the grid in a fixed order"""
    lib = _abi.load()
    d = _abi.GemvDesc()
    d.x = d.W = d.y = 64                                   # fake non-null pointers, never dereferenced
    out = (ctypes.c_int32 * 5)()
    table = [_sweep_one(lib, d, out, *case) for case in itertools.product(FLAGS, DTYPES, ROWS, KS, NS, VARIANTS)]
    try:
        for mode in WIDE_MODES:
            lib.mxvl_set_decode_gemm_wide(mode)
            table += [_sweep_one(lib, d, out, 0, _abi.MXVL_BF16, *case, VARIANTS[1]) for case in itertools.product(ROWS, KS, NS)]
    finally:
        lib.mxvl_set_decode_gemm_wide(1)
    return np.asarray(table, dtype=np.int32)


def record():
    np.savez_compressed(GOLDEN, table=sweep())


def test_decode_plan_and_refusals_match_the_recorded_dispatch():
    want = np.load(GOLDEN)["table"]
    got = sweep()
    assert got.shape == want.shape and want.shape[0] == len(FLAGS) * len(DTYPES) * len(ROWS) * len(KS) * len(NS) * len(VARIANTS) \
        + len(WIDE_MODES) * len(ROWS) * len(KS) * len(NS)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {len(want)} descriptors dispatch differently; first at index {bad[0]}: {got[bad[0]]} != recorded {want[bad[0]]}"
    # the grid reaches every kind and every error code of the checks, so the comparison above is not vacuous
    assert set(np.unique(want[:, 1])) >= {0, 1, 2, 3, 4, 5, 6} and set(np.unique(want[:, 0])) >= {0, -1, -2, -3, -7}
