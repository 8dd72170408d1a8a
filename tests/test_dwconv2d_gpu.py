"""csrc/dwconv2d.hip against float64: every launch geometry dw_geometry() can choose (batch parts, planes per pass, ragged last pass and
last part, V = 4 / V = 1 by shape and by an unaligned base, the d == 1 arms of dw_div), in fp32 / bf16 / fp16, forward and backward,
with a derived per-element error bound.

The model is the one of test_conv1d_gpu.py (fp64_bounds.py: U, _ulp, _rho, FLOOR) with the window replaced by the nine zero-padded taps:
with mag = |b| + sum |w||x|, pre = b + sum w x carries 10 U mag (a bias and nine fmas), SiLU adds |y| rho(pre), dx is nine fmas over the
kernel's own dpre, and dweight / dbias are bounded for ANY summation order over the n non-zero dy of a channel, which covers the register
sums, the wave reduction and the atomics.  Every tolerance also holds one ulp of the output type and the floor.

Every tensor a kernel touches is a view into a larger buffer pre-filled with a NaN bit pattern: a store outside the view changes the
pattern, a load outside it reaches an output as NaN, and an element the kernel never wrote stays NaN.  Launches go through _abi.launch
with the test's own pointers.  The CPU tests (no `gpu` mark) hold the reference and the bound in place: against torch's float64
convolution, against an honest fp32 implementation (must stay under the bound), against planted errors (must not), and the restated
geometry must find every configuration in the case list."""
import types
import zlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fp64_bounds import FLOOR, U, _Buf, _ratio, _report, _rho, _ulp
from medical_image_analysis_amd import _abi

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
_DT = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
gpu = pytest.mark.gpu
MAX_PLANE, MAX_PADDED = 4096, 8172                                # dw_check: H W and (H + 2)(W + 2); 8 * 8172 + 160 = 65536 bytes of LDS


# ---- 1. reference and bound ------------------------------------------------------------------------------------------------------------
def _taps(H, W):
    """tap k = 3 ky + kx of output (h, w) reads the plane padded by one at (h + ky, w + kx): the rows and columns of that shifted slice"""
    return [(slice(ky, ky + H), slice(kx, kx + W)) for ky in range(3) for kx in range(3)]


def _dw_ref(x, w, b, silu, dy, io):
    """x, dy (B, C, H, W) as the kernel gets them (16-bit values widen exactly), w (C, 9) and b (C,) fp32.  Returns y, dx, dw, db in
    float64 with per-element tolerances ty, tdx, tdw, tdb; dx .. db are None without dy, db without b.  Nine shifted slices
    accumulated in place: nothing nine times the size of x is ever held."""
    B, C, H, W = x.shape
    taps = _taps(H, W)
    col = lambda v: v.reshape(1, C, 1, 1)
    w64 = w.double()
    wa = w64.abs()
    xp = F.pad(x.double(), (1, 1, 1, 1))
    xpa = xp.abs()
    pre, mag = torch.zeros(B, C, H, W, dtype=torch.float64), torch.zeros(B, C, H, W, dtype=torch.float64)
    if b is not None:
        pre += col(b.double())
        mag += col(b.double().abs())
    for k, (r, c) in enumerate(taps):
        pre.addcmul_(xp[:, :, r, c], col(w64[:, k]))
        mag.addcmul_(xpa[:, :, r, c], col(wa[:, k]))
    tpre = 10 * U * mag                                           # the bias and an fp32 fma chain of nine, first order
    if silu:
        s = torch.sigmoid(pre)
        y = pre * s
        g = s * (1 + pre * (1 - s))
        ty = g.abs() * tpre + y.abs() * _rho(pre)
    else:
        y, ty = pre, tpre
    res = types.SimpleNamespace(y=y, ty=(ty + _ulp(y, io)).clamp_min(FLOOR), dx=None, tdx=None, dw=None, tdw=None, db=None, tdb=None,
                                pre_range=(float(pre.min()), float(pre.max())))
    if dy is None:
        return res
    dy64 = dy.double()
    if silu:
        gp = s * (1 - s) * (2 + pre * (1 - 2 * s))
        dpre = dy64 * g
        tdpre = dy64.abs() * (gp.abs() * tpre + 3 * _rho(pre) * s * (1 + (pre * (1 - s)).abs()))
    else:
        dpre, tdpre = dy64, torch.zeros_like(dy64)
    dpa = dpre.abs()
    dp, tdp, dpp = (F.pad(t, (1, 1, 1, 1)) for t in (dpre, tdpre, dpa))
    dx, t1, t2 = (torch.zeros(B, C, H, W, dtype=torch.float64) for _ in range(3))
    dw, s1, s2 = (torch.zeros(C, 9, dtype=torch.float64) for _ in range(3))
    for k, (r, c) in enumerate(taps):
        fr, fc = taps[8 - k]                                      # dx[h][w] = sum_k w[ky][kx] dpre[h + 1 - ky][w + 1 - kx], zero outside
        dx.addcmul_(dp[:, :, fr, fc], col(w64[:, k]))
        t1.addcmul_(tdp[:, :, fr, fc], col(wa[:, k]))
        t2.addcmul_(dpp[:, :, fr, fc], col(wa[:, k]))
        dw[:, k] = (dpre * xp[:, :, r, c]).sum((0, 2, 3))
        s1[:, k] = (dpa * xpa[:, :, r, c]).sum((0, 2, 3))
        s2[:, k] = (tdpre * xpa[:, :, r, c]).sum((0, 2, 3))
    n = (dy64 != 0).sum((0, 2, 3)).double()                       # worst case of any summation order over that many terms
    res.dx, res.tdx = dx, (t1 + 9 * U * t2 + _ulp(dx, io)).clamp_min(FLOOR)
    res.dw, res.tdw = dw, (n[:, None] * U * s1 + s2 + _ulp(dw, torch.float32)).clamp_min(FLOOR)
    if b is not None:
        res.db = dpre.sum((0, 2, 3))
        res.tdb = (n * U * dpa.sum((0, 2, 3)) + tdpre.sum((0, 2, 3)) + _ulp(res.db, torch.float32)).clamp_min(FLOOR)
    return res


def _ratios(ref, y, dx=None, dw=None, db=None):
    return dict(y=None if y is None else _ratio(y, ref.y, ref.ty), dx=None if dx is None else _ratio(dx, ref.dx, ref.tdx),
                dw=None if dw is None else _ratio(dw, ref.dw, ref.tdw), db=None if db is None or ref.db is None else _ratio(db, ref.db, ref.tdb))


# ---- 2. dw_geometry() and dw_vec4() restated, and the cases --------------------------------------------------------------------------
def _geometry(B, C, H, W, tiles, aligned):
    """-> (parts, nb, grid_y, P, the planes of every pass of every batch part, V); tiles = 1 forward, 2 backward"""
    parts = min(-(-1024 // C), B)
    nb = -(-B // parts)
    grid_y = -(-B // nb)
    P = min(max(1, min(16, 32768 // (tiles * 4 * (H + 2) * (W + 2)))), nb)
    passes = tuple(tuple(min(P, end - b0) for b0 in range(y * nb, end, P)) for y, end in ((y, min(B, (y + 1) * nb)) for y in range(grid_y)))
    return parts, nb, grid_y, P, passes, 4 if H * W % 4 == 0 and aligned else 1


def _aligned(dtype, shift):
    """whether a view `shift` elements past a 256-byte boundary is 16-byte aligned"""
    return shift * (4 if dtype == torch.float32 else 2) % 16 == 0


BOTH, NEITHER, BIAS_ONLY, SILU_ONLY = (True, True), (False, False), (True, False), (False, True)      # (bias, silu)


class Case:
    def __init__(self, B, C, H, W, combos=(BOTH, NEITHER), dtypes=DTYPES, shifts=(), scale=1.0):
        self.shape, self.combos, self.dtypes, self.shifts, self.scale = (B, C, H, W), combos, dtypes, shifts, scale
        self.id = f"B{B}C{C}H{H}W{W}" + ("-sat" if scale != 1.0 else "")

    def twin(self):
        """the same planes on three channels at most: what the CPU tests of the bound run on"""
        B, C, H, W = self.shape
        return Case(B, min(C, 3), H, W, self.combos, self.dtypes, self.shifts, self.scale)


ALL4 = (BOTH, NEITHER, BIAS_ONLY, SILU_ONLY)
CASES = [
    Case(19, 1024, 14, 14, ALL4, shifts=(1, 2)),                  # stage 3: nb 19, P 16 both ways, passes of 16 + 3, V = 4 across rows
    Case(10, 520, 28, 28, ALL4),                                  # parts 2, nb 5; forward P 5, backward P 4 with passes of 4 + 1
    Case(7, 512, 7, 7, ALL4, shifts=(1, 2)),                      # parts of 4 and 3, P 4, V = 1 by shape
    Case(2, 1024, 64, 64, dtypes=DTYPES[:2]),                     # largest square plane: P 1, two passes, 34 848 bytes backward
    Case(5, 300, 6, 6),                                           # parts 4, nb 2, grid_y 3, last part of 1; V = 4 with W % 4 != 0
    Case(6, 1030, 2, 2), Case(4, 1100, 1, 1),                     # one vector spanning both rows; H W = 1: dw_div's d == 1 arms, P > 1
    Case(3, 1024, 1, 70), Case(3, 1024, 31, 1),                   # H = 1 / W = 1 with P > 1
    Case(2, 3, 1, 2720), Case(2, 3, 1, 2722),                     # thin planes, V = 4 and V = 1; the second is the largest admitted
    Case(2, 24, 56, 56), Case(1, 3, 9, 13),                       # nb 1, P 1: the regime test_vmamba_gpu.py stays in
]
SATURATED = Case(5, 300, 6, 6, combos=(BOTH,), scale=30.0)        # pre-activations beyond +-100: the sigmoid saturates both ways
# the unaligned runs: x, dy, y and dx each start `shift` elements past a 16-byte boundary (fp32: one and two, 16-bit: one)
SHIFTED = [(c, dt, s) for c in CASES for dt in c.dtypes for s in c.shifts if s == 1 or dt == torch.float32]


def _params(cases):
    return [pytest.param(c, dt, bi, si, id=f"{c.id}-{_DT[dt]}-{'bias' if bi else 'nobias'}-{'silu' if si else 'linear'}")
            for c in cases for dt in c.dtypes for bi, si in c.combos]


def _data(case, dtype, bias, silu, backward=True):
    """inputs of a case (CPU, io dtype) and the float64 reference"""
    B, C, H, W = case.shape
    g = torch.Generator().manual_seed(zlib.crc32(f"dwconv2d {case.id} {_DT[dtype]} {bias} {silu}".encode()))
    x = (torch.randn(B, C, H, W, generator=g) * case.scale).to(dtype)
    w = torch.randn(C, 9, generator=g)
    b = torch.randn(C, generator=g) if bias else None
    dy = torch.randn(B, C, H, W, generator=g).to(dtype) if backward else None
    return types.SimpleNamespace(x=x, w=w, b=b, dy=dy, ref=_dw_ref(x, w, b, silu, dy, dtype))


# ---- CPU: the case list reaches what it says it reaches --------------------------------------------------------------------------------
def test_cases_cover_every_launch_geometry():
    need = ("P16", "P_mid", "P1_passes", "ragged_pass", "ragged_part", "grid_y", "v4_straddle", "v4_rows", "v1_shape", "v1_unaligned",
            "W1", "H1", "HW1", "largest", "P_differs")
    seen = {k: set() for k in need}
    for c, dt, shift in [(c, dt, 0) for c in CASES for dt in c.dtypes] + SHIFTED:
        B, C, H, W = c.shape
        assert H * W <= MAX_PLANE and (H + 2) * (W + 2) <= MAX_PADDED
        f, b = (_geometry(B, C, H, W, tiles, _aligned(dt, shift)) for tiles in (1, 2))
        ragged = lambda geo: any(p[-1] < geo[3] and len(p) > 1 for p in geo[4])
        hit = dict(P16=f[3] == 16 and b[3] == 16, P_mid=1 < f[3] < 16 and 1 < b[3] < 16,
                   P1_passes=all(geo[3] == 1 and len(geo[4][0]) > 1 for geo in (f, b)), ragged_pass=ragged(f) and ragged(b),
                   ragged_part=sum(f[4][-1]) < f[1], grid_y=f[2] > 1, v4_straddle=f[5] == 4 and W % 4 != 0, v4_rows=f[5] == 4 and W % 4 == 0,
                   v1_shape=H * W % 4 != 0, v1_unaligned=H * W % 4 == 0 and f[5] == 1, W1=W == 1 and H > 1, H1=H == 1 and W > 1,
                   HW1=H * W == 1, largest=(H + 2) * (W + 2) == MAX_PADDED, P_differs=f[3] != b[3])
        assert f[5] == b[5] and (shift == 0 or f[5] == 1), "a shifted base takes the scalar kernels"
        for k, v in hit.items():
            if v:
                seen[k].add(dt)
    for k in need:                                                # the 64 x 64 plane, the only P = 1 with several passes, skips fp16
        assert seen[k] >= set(DTYPES[:2] if k == "P1_passes" else DTYPES), f"{k}: only {sorted(_DT[d] for d in seen[k])}"
    # and the rows of the table are what they were chosen for
    assert _geometry(19, 1024, 14, 14, 1, True) == (1, 19, 1, 16, ((16, 3),), 4) and _geometry(19, 1024, 14, 14, 2, True)[3:5] == (16, ((16, 3),))
    assert _geometry(10, 520, 28, 28, 1, True) == (2, 5, 2, 5, ((5,), (5,)), 4) and _geometry(10, 520, 28, 28, 2, True)[3:5] == (4, ((4, 1), (4, 1)))
    assert _geometry(7, 512, 7, 7, 2, True) == (2, 4, 2, 4, ((4,), (3,)), 1)
    assert _geometry(2, 1024, 64, 64, 2, True) == (1, 2, 1, 1, ((1, 1),), 4) and 2 * 4 * 66 * 66 == 34848
    assert _geometry(5, 300, 6, 6, 2, True) == (4, 2, 3, 2, ((2,), (2,), (1,)), 4)
    assert _geometry(6, 1030, 2, 2, 2, True)[3:] == (6, ((6,),), 4) and _geometry(4, 1100, 1, 1, 2, True)[3:] == (4, ((4,),), 1)
    assert _geometry(2, 3, 1, 2720, 2, True)[5] == 4 and _geometry(2, 3, 1, 2722, 2, True)[5] == 1 and 2 * 4 * 3 * 2724 + 160 == 65536
    assert all(_geometry(*c.shape, 2, True)[1] > 1 for c in CASES[:10] if c.shape[1] >= 300), "more than one plane per workgroup"
    assert SATURATED.shape == CASES[4].shape


# ---- CPU: the reference against torch's own float64 convolution ------------------------------------------------------------------------
def _parts64(x, w, b, silu, dy):
    """the operation with torch's functional ops in float64: kernel (C, 1, 3, 3), pre, sigmoid(pre), y, dpre"""
    C = w.shape[0]
    k = w.double().view(C, 1, 3, 3)
    pre = F.conv2d(x.double(), k, None if b is None else b.double(), padding=1, groups=C)
    s = torch.sigmoid(pre)
    return k, pre, s, (pre * s if silu else pre), (dy.double() * s * (1 + pre * (1 - s)) if silu else dy.double())


def _grads64(x, k, dpre):
    C = k.shape[0]
    dw = torch.nn.grad.conv2d_weight(x.double(), k.shape, dpre, padding=1, groups=C)
    return F.conv_transpose2d(dpre, k, padding=1, groups=C), dw.reshape(C, 9), dpre.sum((0, 2, 3))


@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (2, 3, 1, 6), (2, 3, 6, 1), (4, 2, 1, 1), (2, 2, 2, 2)])
@pytest.mark.parametrize("bias,silu", ALL4)
def test_ref_equals_torch_float64(shape, bias, silu):
    g = torch.Generator().manual_seed(sum(shape))
    x, dy, w = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g), torch.randn(shape[1], 9, generator=g)
    b = torch.randn(shape[1], generator=g) if bias else None
    r = _dw_ref(x, w, b, silu, dy, torch.float32)
    k, _, _, y, dpre = _parts64(x, w, b, silu, dy)
    dx, dw, db = _grads64(x, k, dpre)
    for got, want in ((r.y, y), (r.dx, dx), (r.dw, dw)) + (((r.db, db),) if bias else ()):
        assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))
    assert (r.db is None) == (not bias)


# ---- CPU: an honest fp32 implementation stays under the bound ------------------------------------------------------------------------
def _honest_fp32(x, w, b, silu, dy, io):
    """the operation as anybody would write it in fp32: what the bound has to let through"""
    C = w.shape[0]
    xf, wf = x.float().requires_grad_(True), w.clone().requires_grad_(True)
    bf = b.clone().requires_grad_(True) if b is not None else None
    pre = F.conv2d(xf, wf.view(C, 1, 3, 3), bf, padding=1, groups=C)
    y = F.silu(pre) if silu else pre
    y.backward(dy.float())
    return y.detach().to(io), xf.grad.to(io), wf.grad, None if b is None else bf.grad


@pytest.mark.parametrize("case,dtype,bias,silu", _params([c.twin() for c in CASES + [SATURATED]]))
def test_honest_fp32_within_bound(case, dtype, bias, silu):
    d = _data(case, dtype, bias, silu)
    _report(f"honest {case.id} {_DT[dtype]} bias={bias} silu={silu}", **_ratios(d.ref, *_honest_fp32(d.x, d.w, d.b, silu, d.dy, dtype)))


# ---- CPU: the bound notices planted errors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,last_part", [((7, 3, 14, 14), 3), ((3, 2, 64, 64), 1)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
def test_bound_flags_planted_errors(dtype, shape, last_part):
    g = torch.Generator().manual_seed(11 + shape[0])
    B, C, H, W = shape
    x, dy = torch.randn(*shape, generator=g).to(dtype), torch.randn(*shape, generator=g).to(dtype)
    w, b = torch.randn(C, 9, generator=g), torch.randn(C, generator=g)
    r = _dw_ref(x, w, b, True, dy, dtype)
    k, pre, s, y, dpre = _parts64(x, w, b, True, dy)
    dx, dw, db = _grads64(x, k, dpre)
    io = lambda t: t.to(dtype)
    # what the float64 values themselves give once rounded: inside
    _report(f"unplanted {_DT[dtype]} {shape}", **_ratios(r, io(y), io(dx), dw.float(), db.float()))
    planted = {}
    # (1) taps mirrored left to right; (2) convolution instead of correlation
    for name, dims in (("mirrored", (-1,)), ("convolution", (-1, -2))):
        planted[name] = _ratios(r, io(_parts64(x, w.view(C, 3, 3).flip(dims).reshape(C, 9), b, True, dy)[3]))
    # (3) the left border replicated instead of zero-padded
    xr = F.pad(F.pad(x.double(), (1, 0, 0, 0), mode="replicate"), (0, 1, 1, 1))
    pr = F.conv2d(xr, k, b.double(), groups=C)
    planted["replicated border"] = _ratios(r, io(pr * torch.sigmoid(pr)))
    # (4) plane q = 1 of a pass computed from plane q - 1's input
    yq = y.clone()
    yq[1] = y[0]
    planted["plane q from q - 1"] = _ratios(r, io(yq))
    # (5) dweight / dbias without the last batch element; (6) without the whole last batch part
    for name, keep in (("last element missing", B - 1), ("last part missing", B - last_part)):
        _, dwm, dbm = _grads64(x[:keep], k, dpre[:keep])
        planted[name] = _ratios(r, None, None, dwm.float(), dbm.float())
        assert planted[name]["dw"] > 1 and planted[name]["db"] > 1
    # (7) SiLU's gradient without its pre s (1 - s) term
    dxs, dws, dbs = _grads64(x, k, dy.double() * s)
    planted["silu' short"] = _ratios(r, None, io(dxs), dws.float(), dbs.float())
    # (8) dx with the taps not flipped
    planted["dx unflipped"] = _ratios(r, None, io(F.conv2d(dpre, k, padding=1, groups=C)))
    for name, ratios in planted.items():
        worst = max(v for v in ratios.values() if v is not None)
        print(f"planted {_DT[dtype]} {shape} {name}: max err / tol {worst:.1f}")
        assert worst > 1, name


# ---- what the two entries refuse before any launch ----------------------------------------------------------------------------------
def _entry_calls(ptrs, stream):
    """-> fwd(**changes), bwd(**changes): the status of a call whose arguments are a valid 2 x 4 x 8 x 8 bf16 descriptor over `ptrs`
    (x, weight, bias, y, dy, dx, dweight, dbias) with `changes` applied"""
    lib = _abi.load()
    good = dict(zip(("x", "weight", "bias", "y", "dy", "dx", "dweight", "dbias"), ptrs), B=2, C=4, H=8, W=8, ksize=3, io_dtype=_abi.MXVL_BF16)

    def fwd(**kw):
        a = {**good, **kw}
        return lib.mxvl_dwconv2d_fwd(a["x"], a["weight"], a["bias"], a["y"], a["B"], a["C"], a["H"], a["W"], a["ksize"], a["io_dtype"], 1, stream)

    def bwd(**kw):
        a = {**good, **kw}
        return lib.mxvl_dwconv2d_bwd(a["x"], a["weight"], a["bias"], a["dy"], a["dx"], a["dweight"], a["dbias"], a["B"], a["C"], a["H"], a["W"],
                                     a["ksize"], a["io_dtype"], 1, stream)
    return fwd, bwd


def _assert_refusals(fwd, bwd):
    code = {v: k for k, v in _abi.STATUS.items()}
    for call in (fwd, bwd):
        assert call(x=None) == code["MXVL_ERR_NULL"] and call(weight=None) == code["MXVL_ERR_NULL"]
        for k in ("B", "C", "H", "W"):
            assert call(**{k: 0}) == code["MXVL_ERR_SHAPE"] and call(**{k: -3}) == code["MXVL_ERR_SHAPE"], k
        assert call(ksize=5) == code["MXVL_ERR_UNSUPPORTED"] and call(ksize=1) == code["MXVL_ERR_UNSUPPORTED"]
        assert call(H=17, W=241) == code["MXVL_ERR_UNSUPPORTED"], "H W = 4097"
        assert call(H=65, W=64) == code["MXVL_ERR_UNSUPPORTED"]
        # the padded plane: 8 (H + 2)(W + 2) + 160 bytes of LDS in the backward; 1 x 2722 and 2 x 2041 are the last to fit 64 KB
        for H, W in ((1, 2723), (2723, 1), (2, 2042), (2042, 2), (1, 2800), (1, 4096), (4096, 1), (2, 2048)):
            assert H * W <= MAX_PLANE and (H + 2) * (W + 2) > MAX_PADDED
            assert call(H=H, W=W) == code["MXVL_ERR_UNSUPPORTED"], (H, W)
        for bad in (3, -1, 1 << 20):
            assert call(io_dtype=bad) == code["MXVL_ERR_DTYPE"]
    assert fwd(y=None) == code["MXVL_ERR_NULL"]
    for k in ("dy", "dx", "dweight", "dbias"):                    # dbias: a bias is set, so its gradient needs somewhere to go
        assert bwd(**{k: None}) == code["MXVL_ERR_NULL"], k


def test_dwconv_refusals_without_gpu():
    """every call below returns before anything is launched, so the pointers are never dereferenced"""
    _assert_refusals(*_entry_calls((0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000), None))


@gpu
def test_dwconv_refusals_and_valid_descriptor():
    n = 2 * 4 * 2 * 2041                                          # room for the largest planes admitted, 1 x 2722 and 2 x 2041
    t = [torch.zeros(n, dtype=torch.bfloat16, device=DEV) for _ in range(4)]
    f = [torch.zeros(4 * 9, device=DEV) for _ in range(4)]
    x, y, dy, dx = (v.data_ptr() for v in t)
    w, b, dw, db = (v.data_ptr() for v in f)
    with torch.cuda.device(DEV):
        fwd, bwd = _entry_calls((x, w, b, y, dy, dx, dw, db), _abi.stream_ptr(torch.device(DEV)))
        _assert_refusals(fwd, bwd)
        for call in (fwd, bwd):
            assert call() == 0 and call(bias=None, dbias=None) == 0 and call(H=1, W=2722) == 0 and call(H=2, W=2041) == 0
            assert call(H=64, W=64, B=1, C=1) == 0
        assert bwd(bias=None) == 0, "a dbias nobody asked for is ignored"
        torch.cuda.synchronize()


# ---- GPU: the two entries on guarded buffers -------------------------------------------------------------------------------------------
def _launch_both(case, dtype, d, silu, shift=0):
    """mxvl_dwconv2d_fwd and _bwd on views into NaN-patterned buffers -> y, dx, dweight, dbias after the guard / input / coverage checks"""
    shape = case.shape
    B, C, H, W = shape
    f32 = torch.float32
    x, dy = _Buf.flat(shape, dtype, DEV, d.x, shift), _Buf.flat(shape, dtype, DEV, d.dy, shift)
    y, dx = _Buf.flat(shape, dtype, DEV, None, shift), _Buf.flat(shape, dtype, DEV, None, shift)
    w, b = _Buf.flat((C, 9), f32, DEV, d.w), (_Buf.flat((C,), f32, DEV, d.b) if d.b is not None else None)
    dw = _Buf.flat((C, 9), f32, DEV, torch.zeros(C, 9))           # zeros, as the wrapper allocates them
    db = _Buf.flat((C,), f32, DEV, torch.zeros(C)) if d.b is not None else None
    ptr = lambda buf: None if buf is None else buf.view.data_ptr()
    for buf in (x, dy, y, dx):
        assert (ptr(buf) % 16 == 0) == _aligned(dtype, shift) and buf.view.is_contiguous()
    dev, meta = x.view.device, (B, C, H, W, 3, _abi.dtype_code(dtype), int(silu))
    _abi.launch("mxvl_dwconv2d_fwd", ptr(x), ptr(w), ptr(b), ptr(y), *meta, device=dev)
    _abi.launch("mxvl_dwconv2d_bwd", ptr(x), ptr(w), ptr(b), ptr(dy), ptr(dx), ptr(dw), ptr(db), *meta, device=dev)
    torch.cuda.synchronize()
    assert all(buf.unchanged() for buf in (x, dy, w) + ((b,) if b is not None else ())), "an input was modified"
    assert y.guard_intact() and dx.guard_intact(), "store outside y / dx"
    assert dw.guard_intact() and (db is None or db.guard_intact()), "store outside dweight / dbias"
    assert y.written() and dx.written(), "y / dx not fully written (or a read outside x / dy reached them)"
    out = (y.view, dx.view, dw.view, db.view if db is not None else None)
    assert all(bool(torch.isfinite(t).all()) for t in out if t is not None)
    return out


@gpu
@pytest.mark.parametrize("case,dtype,bias,silu", _params(CASES + [SATURATED]))
def test_dwconv2d_forward_backward(case, dtype, bias, silu):
    d = _data(case, dtype, bias, silu)
    if case.scale != 1.0:
        assert d.ref.pre_range[0] < -100 and d.ref.pre_range[1] > 100
    f, b = (_geometry(*case.shape, tiles, True) for tiles in (1, 2))
    _report(f"dwconv2d {case.id} {_DT[dtype]} bias={bias} silu={silu} fwd nb {f[1]} P {f[3]} bwd P {b[3]} V {f[5]}",
            **_ratios(d.ref, *_launch_both(case, dtype, d, silu)))


@gpu
@pytest.mark.parametrize("case,dtype", [pytest.param(c, dt, id=f"{c.id}-{_DT[dt]}") for c, dt in dict.fromkeys((c, dt) for c, dt, _ in SHIFTED)])
def test_dwconv2d_unaligned_base(case, dtype):
    """x, dy, y and dx one element (fp32: also two) past a 16-byte boundary: dw_vec4 has to choose V = 1, nothing else changes"""
    d = _data(case, dtype, True, True)
    for shift in (s for c, dt, s in SHIFTED if (c, dt) == (case, dtype)):
        assert _geometry(*case.shape, 2, _aligned(dtype, shift))[5] == 1
        _report(f"dwconv2d {case.id} {_DT[dtype]} base + {shift}", **_ratios(d.ref, *_launch_both(case, dtype, d, True, shift)))


# ---- GPU: vmamba.dwconv3x3_act, the wrapper --------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """every _abi.launch as (entry, arguments)"""
    seen, real = [], _abi.launch

    def recording(name, *a, **kw):
        seen.append((name, a))
        return real(name, *a, **kw)

    monkeypatch.setattr(_abi, "launch", recording)
    return seen


def _conv(C, g, bias=True, k=3, padding=1, groups=None):
    conv = nn.Conv2d(C, C, k, padding=padding, groups=groups or C, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        if bias:
            conv.bias.copy_(torch.randn(C, generator=g))
    return conv


def _wrapper_run(what, x_cpu, make_input, conv, dy_cpu, make_dy, io, launches, autocast=None):
    """dwconv3x3_act + SiLU on make_input(leaf) -> checks y, the leaf's gradient brought back to (B, C, H, W), dweight and dbias"""
    from medical_image_analysis_amd import vmamba as vm
    C = conv.in_channels
    w, b = conv.weight.detach().reshape(C, 9).clone(), (conv.bias.detach().clone() if conv.bias is not None else None)
    ref = _dw_ref(x_cpu.to(io), w, b, True, dy_cpu.to(io), io)
    convd = conv.to(DEV)
    leaf, x, grad_of = make_input(x_cpu.to(DEV))
    with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
        y = vm.dwconv3x3_act(x, convd, nn.SiLU())
    assert y.dtype == io and [n for n, _ in launches] == ["mxvl_dwconv2d_fwd"] and launches[0][1][9] == _abi.dtype_code(io)
    y.backward(make_dy(dy_cpu.to(DEV)))
    assert [n for n, _ in launches] == ["mxvl_dwconv2d_fwd", "mxvl_dwconv2d_bwd"] and launches[1][1][12] == _abi.dtype_code(io)
    dx = grad_of(leaf.grad)
    assert dx.dtype == x_cpu.dtype and convd.weight.grad.dtype == torch.float32 and convd.weight.grad.shape == (C, 1, 3, 3)
    _report(what, **_ratios(ref, y, dx, convd.weight.grad.reshape(C, 9), convd.bias.grad if b is not None else None))
    return leaf


_plain = lambda t: (t.requires_grad_(True),) * 2 + ((lambda g: g),)
_same = lambda t: t


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
def test_wrapper_strided_inputs(dtype, launches):
    """the two non-contiguous views SS2D passes: the first half of a chunk(2, dim=1) (channel_first) and a permuted channel-last tensor"""
    B, C, H, W = 3, 5, 6, 7
    g = torch.Generator().manual_seed(2024)
    x, other, dy = (torch.randn(B, C, H, W, generator=g).to(dtype) for _ in range(3))

    def chunked(xd):
        xz = torch.cat([xd, other.to(DEV)], 1).requires_grad_(True)
        half = xz.chunk(2, dim=1)[0]
        assert not half.is_contiguous()
        return xz, half, lambda gr: gr[:, :C]

    xz = _wrapper_run(f"wrapper chunk {_DT[dtype]}", x, chunked, _conv(C, g), dy, _same, dtype, launches)
    assert not bool(xz.grad[:, C:].any()), "the other half of the chunk has no gradient"
    launches.clear()

    def permuted(xd):
        xl = xd.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        v = xl.permute(0, 3, 1, 2)
        assert not v.is_contiguous()
        return xl, v, lambda gr: gr.permute(0, 3, 1, 2)

    _wrapper_run(f"wrapper permute {_DT[dtype]}", x, permuted, _conv(C, g, bias=False), dy, _same, dtype, launches)


@gpu
@pytest.mark.parametrize("dtype", DTYPES[1:], ids=_DT.get)
def test_wrapper_autocast(dtype, launches):
    """fp32 input and parameters under 16-bit autocast: the kernel gets the autocast dtype, the gradients come back in fp32"""
    g = torch.Generator().manual_seed(77)
    x, dy = torch.randn(2, 6, 7, 7, generator=g), torch.randn(2, 6, 7, 7, generator=g)

    def check_fp32(xd):
        xd.requires_grad_(True)
        return xd, xd, lambda gr: gr

    leaf = _wrapper_run(f"wrapper autocast {_DT[dtype]}", x, check_fp32, _conv(6, g), dy, lambda t: t.to(dtype), dtype, launches, autocast=dtype)
    assert leaf.grad.dtype == torch.float32


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
def test_wrapper_strided_and_foreign_dy(dtype, launches):
    """a dy that is a permuted view, and a dy handed to backward() in a wider dtype (the kernel has to see it in x's dtype, whoever casts it)"""
    g = torch.Generator().manual_seed(31)
    x, dy = torch.randn(2, 5, 9, 4, generator=g).to(dtype), torch.randn(2, 5, 9, 4, generator=g).to(dtype)

    def strided(t):
        v = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not v.is_contiguous()
        return v

    _wrapper_run(f"wrapper strided dy {_DT[dtype]}", x, _plain, _conv(5, g), dy, strided, dtype, launches)
    launches.clear()
    other = torch.float64 if dtype == torch.float32 else torch.float32      # widens exactly: the kernel sees the same dy
    _wrapper_run(f"wrapper {other} dy {_DT[dtype]}", x, _plain, _conv(5, g), dy, lambda t: t.to(other), dtype, launches)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
def test_wrapper_other_activations(dtype, launches):
    """nn.Identity: the silu = 0 arm alone.  nn.GELU: torch's activation on the kernel's output, forward and backward -- y is exactly
    gelu of the Identity route's y, and the gradients obey the bound for the dy that torch's gelu backward hands the kernel."""
    from medical_image_analysis_amd import vmamba as vm
    B, C, H, W = 3, 5, 6, 7
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(B, C, H, W, generator=g).to(dtype), torch.randn(B, C, H, W, generator=g).to(dtype)
    conv = _conv(C, g)
    w, b = conv.weight.detach().reshape(C, 9).clone(), conv.bias.detach().clone()
    conv = conv.to(DEV)
    grads = lambda xd: (xd.grad, conv.weight.grad.reshape(C, 9), conv.bias.grad)
    xd = x.to(DEV).requires_grad_(True)
    y_lin = vm.dwconv3x3_act(xd, conv, nn.Identity())
    y_lin.backward(dy.to(DEV))
    assert launches[0][1][10] == 0 and launches[1][1][13] == 0, "silu off"
    _report(f"wrapper Identity {_DT[dtype]}", **_ratios(_dw_ref(x, w, b, False, dy, dtype), y_lin, *grads(xd)))
    conv.zero_grad()
    xg = x.to(DEV).requires_grad_(True)
    y = vm.dwconv3x3_act(xg, conv, nn.GELU())
    y.backward(dy.to(DEV))
    yl = y_lin.detach().requires_grad_(True)
    want = F.gelu(yl)
    assert torch.equal(y, want)
    dy_pre, = torch.autograd.grad(want, yl, dy.to(DEV))
    _report(f"wrapper GELU {_DT[dtype]}", **_ratios(_dw_ref(x, w, b, False, dy_pre.cpu(), dtype), None, *grads(xg)))
    assert len(launches) == 4 and all(a[-1] == 0 for _, a in launches), "two launches each, all with silu off"


@gpu
@pytest.mark.parametrize("shape,kw", [pytest.param(shape, kw, id=what) for what, shape, kw in (
    ("5x5", (2, 4, 9, 9), dict(k=5, padding=2)), ("padding0", (2, 4, 9, 9), dict(padding=0)), ("groups2", (2, 4, 9, 9), dict(groups=2)),
    ("65x64", (1, 2, 65, 64), {}), ("1x2800", (1, 2, 1, 2800), {}), ("2800x1", (1, 2, 2800, 1), {}))])
def test_wrapper_falls_back_to_torch(shape, kw, launches):
    """what the kernel does not serve is torch's act(conv(x)), and nothing of libmxvl is launched"""
    from medical_image_analysis_amd import vmamba as vm
    g = torch.Generator().manual_seed(9)
    conv, act = _conv(shape[1], g, **kw).to(DEV), nn.SiLU()
    x = torch.randn(*shape, generator=g).to(DEV).requires_grad_(True)
    y = vm.dwconv3x3_act(x, conv, act)
    assert torch.equal(y, act(conv(x)))
    y.backward(torch.ones_like(y))
    assert launches == [] and x.grad is not None and bool(torch.isfinite(x.grad).all())
