"""csrc/conv1d.hip against float64: every kernel its dispatch can choose (three forward, five backward, two single-token
steps), in fp32 / bf16 / fp16, on the strided layouts the mixer really passes, with a derived per-element error bound.

Every tensor a kernel touches is a view into a larger buffer pre-filled with a NaN bit pattern: a store outside the view changes
the pattern, a load outside it reaches an output as NaN, and an element the kernel never wrote stays NaN.  Launches go through the
descriptors of _abi, so the strides are the test's own.  The CPU tests (no `gpu` mark) hold the reference and the bound in place:
against the goldens, against an honest fp32 implementation (must stay under the bound) and against planted errors (must not)."""
import ctypes
import functools
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, load_golden
from fp64_bounds import FLOOR, GUARD, U, _Buf as _FlatBuf, _ratio, _report, _rho, _ulp
from medical_image_analysis_amd import _abi

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
_DT = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
gpu = pytest.mark.gpu

# ---- 1. reference and bound (U, FLOOR, _ulp, _rho, _ratio: fp64_bounds.py) ------------------------------------------------------------
def _windows(x64, W):
    """xw[..., t, k] = x[..., t - (W-1) + k], zero before the row starts"""
    return F.pad(x64, (W - 1, 0)).unfold(-1, W, 1)


def _fwd_part(xw, w, b, silu, io):
    """xw (B, D, T, W) float64 windows, w (D, W), b (D,) or None -> y, its tolerance, and what the backward needs"""
    W = w.shape[1]
    w64 = w.double()[:, None, :]
    b64 = b.double()[:, None] if b is not None else torch.zeros(w.shape[0], 1, dtype=torch.float64)
    pre = b64 + (xw * w64).sum(-1)
    mag = b64.abs() + (xw.abs() * w64.abs()).sum(-1)
    tpre = (W + 1) * U * mag                                     # fp32 fma chain, first order
    if silu:
        s = torch.sigmoid(pre)
        y = pre * s
        g = s * (1 + pre * (1 - s))
        ty = g.abs() * tpre + y.abs() * _rho(pre)
    else:
        s = g = None
        y, ty = pre, tpre
    return types.SimpleNamespace(pre=pre, tpre=tpre, s=s, g=g, y=y, ty=(ty + _ulp(y, io)).clamp_min(FLOOR))


def _conv_ref(x, w, b, silu, dy, io_dtype, dw0=None, db0=None):
    """x, dy (B, D, L) as the kernel gets them (16-bit values widen exactly), w (D, W) and b (D,) fp32.  Returns y, dx, dw, db in
    float64 with per-element tolerances ty, tdx, tdw, tdb; dx .. db are None without dy, db without b."""
    W = w.shape[1]
    xw = _windows(x.double(), W)
    f = _fwd_part(xw, w, b, silu, io_dtype)
    r = types.SimpleNamespace(y=f.y, ty=f.ty, dx=None, tdx=None, dw=None, tdw=None, db=None, tdb=None, xw=xw)
    if dy is None:
        return r
    dy64 = dy.double()
    if silu:
        gp = f.s * (1 - f.s) * (2 + f.pre * (1 - 2 * f.s))
        dpre = dy64 * f.g
        tdpre = dy64.abs() * (gp.abs() * f.tpre + 3 * _rho(f.pre) * f.s * (1 + (f.pre * (1 - f.s)).abs()))
    else:
        dpre, tdpre = dy64, torch.zeros_like(dy64)
    wrev = w.double().flip(-1)[:, None, :]                       # dx[s] = sum_m w[W-1-m] dpre[s+m], dpre beyond L is 0
    dpw, tdpw = F.pad(dpre, (0, W - 1)).unfold(-1, W, 1), F.pad(tdpre, (0, W - 1)).unfold(-1, W, 1)
    r.dx = (dpw * wrev).sum(-1)
    r.tdx = ((tdpw * wrev.abs()).sum(-1) + W * U * (dpw.abs() * wrev.abs()).sum(-1) + _ulp(r.dx, io_dtype)).clamp_min(FLOOR)
    n_d = (dy64 != 0).sum((0, 2)).double()                       # worst case of any summation order over that many terms
    dw0 = torch.zeros_like(w, dtype=torch.float64) if dw0 is None else dw0.double()
    r.dw = dw0 + (dpre[..., None] * xw).sum((0, 2))
    r.tdw = ((tdpre[..., None] * xw.abs()).sum((0, 2)) + n_d[:, None] * U * (dw0.abs() + (dpre.abs()[..., None] * xw.abs()).sum((0, 2)))
             + _ulp(r.dw, torch.float32)).clamp_min(FLOOR)
    if b is not None:
        db0 = torch.zeros_like(b, dtype=torch.float64) if db0 is None else db0.double()
        r.db = db0 + dpre.sum((0, 2))
        r.tdb = (tdpre.sum((0, 2)) + n_d * U * (db0.abs() + dpre.abs().sum((0, 2))) + _ulp(r.db, torch.float32)).clamp_min(FLOOR)
    r.dpre = dpre
    return r


def _update_ref(x, state, w, b, silu, io_dtype):
    """one decode step: x (B, D), state (B, D, W).  -> y, ty (float64) and the new state, a bit-exact shift"""
    new = torch.cat([state[..., 1:], x[..., None].to(state.dtype)], -1)
    f = _fwd_part(new.double()[:, :, None, :], w, b, silu, io_dtype)
    return f.y[..., 0], f.ty[..., 0], new


def _state_ref(h, x, dt, A, Bm, Cm, D, z, dt_bias, softplus, io_dtype, skip_col=None):
    """mxvl_state_update in float64: h (B, D, N) fp32 state, x / dt / z (B, D), A (D, N), Bm / Cm (B, N), D / dt_bias (D,).
    -> h', its tolerance, y, its tolerance.  skip_col plants an error: that state column is left as it was."""
    h, x, dt, A, Bm, Cm = (t.double() for t in (h, x, dt, A, Bm, Cm))
    N = h.shape[-1]
    dtv = dt + (dt_bias.double() if dt_bias is not None else 0.0)
    t0 = U * dtv.abs()
    if softplus:
        dts = torch.where(dtv > 20.0, dtv, torch.log1p(torch.exp(dtv.clamp_max(20.0))))
        tdt = torch.sigmoid(dtv) * t0 + dts * _rho(dtv)
    else:
        dts, tdt = dtv, t0
    a = dts[..., None] * A
    e = torch.exp(a)
    te = e * (A.abs() * tdt[..., None] + U * a.abs() + _rho(a))
    xB = x[..., None] * Bm[:, None, :]
    hn = h * e + xB * dts[..., None]
    thn = (h.abs() * te + xB.abs() * tdt[..., None] + 3 * U * ((h * e).abs() + (xB * dts[..., None]).abs())
           + _ulp(hn, torch.float32)).clamp_min(FLOOR)
    if skip_col is not None:
        hn = hn.clone()
        hn[..., skip_col] = h[..., skip_col]
    hc = hn * Cm[:, None, :]
    dx = D.double() * x if D is not None else torch.zeros_like(x)
    y = hc.sum(-1) + dx
    ty = (Cm.abs()[:, None, :] * thn).sum(-1) + (N + 1) * U * (hc.abs().sum(-1) + dx.abs())
    if z is not None:
        z = z.double()
        sz = z * torch.sigmoid(z)
        ty = sz.abs() * ty + (y * sz).abs() * _rho(z)
        y = y * sz
    return hn, thn, y, (ty + _ulp(y, io_dtype)).clamp_min(FLOOR)


# ---- 2. strided buffers with guard bands (GUARD, the NaN patterns and the buffer itself: fp64_bounds.py) --------------------------------
def _padded_len(L):
    return L + 4 - L % 4                                          # > L and a multiple of 4


def _layout(kind, B, D, L):
    """-> (elements of storage, offset of the view, (batch, channel, step) strides) of a (B, D, L) view"""
    Lp = _padded_len(L)
    n, off, st = {
        "contig": (B * D * L, 0, (D * L, L, 1)),
        "half": (B * 2 * D * L, 0, (2 * D * L, L, 1)),            # xz[:, :d]
        "cmajor": (D * B * L, 0, (L, B * L, 1)),                  # the batch stride is the smaller one
        "cmajor_half": (2 * D * B * L, 0, (L, B * L, 1)),         # dxz[:, :d] of a channel-major d(xz)
        "padded": (B * D * Lp, 0, (D * Lp, Lp, 1)),
        "cmajor_padded": (D * B * Lp, 0, (Lp, B * Lp, 1)),        # the multi-direction core's rows
        "shift1": (B * D * L + 1, 1, (D * L, L, 1)),
        "shift2": (B * D * L + 2, 2, (D * L, L, 1)),
    }[kind]
    return n + 2 * GUARD, GUARD + off, st


def _rows_aligned(lay, dtype):
    """rows_aligned() of conv1d.hip for a view of an allocation that is itself aligned (asserted at every launch)"""
    _, off, st = lay
    es, al = (4, 16) if dtype == torch.float32 else (2, 8)
    return (off * es) % al == 0 and st[0] % 4 == 0 and st[1] % 4 == 0


class _Buf(_FlatBuf):
    @classmethod
    def rows(cls, kind, B, D, L, dtype, device, data=None):
        n, off, st = _layout(kind, B, D, L)
        return cls(n, off, st, (B, D, L), dtype, device, data)


def _fwd_desc(x, w, b, y, silu):
    d = _abi.Conv1dDesc()
    d.batch, d.dim, d.seqlen, d.width = x.shape[0], x.shape[1], x.shape[2], w.shape[1]
    d.io_dtype, d.silu = _abi.dtype_code(x.dtype), int(silu)
    d.x_bs, d.x_ds = x.stride(0), x.stride(1)
    d.x, d.weight, d.bias = x.data_ptr(), w.data_ptr(), _abi.ptr(b)
    if y is not None:
        d.y_bs, d.y_ds, d.y = y.stride(0), y.stride(1), y.data_ptr()
    return d


def _launch_fwd(x, w, b, y, silu):
    _abi.launch("mxvl_conv1d_fwd", _fwd_desc(x, w, b, y, silu), device=x.device)


def _launch_bwd(x, w, b, silu, dy, dx, dw, db):
    d = _abi.Conv1dBwdDesc()
    d.fwd = _fwd_desc(x, w, b, None, silu)
    d.dy_bs, d.dy_ds, d.dx_bs, d.dx_ds = dy.stride(0), dy.stride(1), dx.stride(0), dx.stride(1)
    d.dy, d.dx, d.dweight, d.dbias = dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), _abi.ptr(db)
    _abi.launch("mxvl_conv1d_bwd", d, device=x.device)


# ---- 3. the dispatch of mxvl_conv1d_fwd / _bwd, restated, and the cases ---------------------------------------------------------------
FWD_KERNELS = ("fwd_vec", "fwd4", "fwd0")
BWD_KERNELS = ("bwd_vec_rows", "bwd_short", "bwd_vec", "bwd4", "bwd0")


def _fwd_kernel_for(W, L, lx, ly, dtype):
    if W == 4 and L % 4 == 0 and _rows_aligned(lx, dtype) and _rows_aligned(ly, dtype):
        return "fwd_vec"
    return "fwd4" if W == 4 else "fwd0"


def _bwd_kernel_for(W, L, D, lx, ldy, ldx, dtype):
    """-> (kernel, whether the LDS tile kernel stages its full tiles as vectors: `p.vec && t0 + TILE <= L`)"""
    vec = _rows_aligned(lx, dtype) and _rows_aligned(ldy, dtype)
    dx_al = _rows_aligned(ldx, dtype)
    S = 1024 // (L + 3) if W == 4 and L + 3 <= 512 and D <= 65535 else 0
    bvec = vec and W == 4 and L % 4 == 0 and L > 512 and dx_al
    svec = vec and W == 4 and L % 4 == 0 and L <= 512 and D <= 65535 and dx_al
    RW = 256 // ((L + 7) // 8) if svec else 0
    if svec and RW >= 2:
        return "bwd_vec_rows", False
    if S >= 2:
        return "bwd_short", False
    if bvec:
        return "bwd_vec", False
    return ("bwd4" if W == 4 else "bwd0"), (vec and L >= 1024)


class Case:
    def __init__(self, kernel, B, D, L, W=4, x="contig", y=None, dy=None, dx=None, bias=True, silu=True, prefill=False,
                 scale=1.0, vec_tiles=False, only=None):
        self.kernel, self.B, self.D, self.L, self.W = kernel, B, D, L, W
        self.x, self.dy, self.dx = x, dy or x, dx or x
        self.y = y or (self.dx if dx else ("contig" if x == "half" else x))
        self.bias, self.silu, self.prefill, self.scale, self.vec_tiles, self.only = bias, silu, prefill, scale, vec_tiles, only
        self.backward = kernel in BWD_KERNELS
        lay = f"{self.x}.{self.dy}.{self.dx}" if self.backward else f"{self.x}.{self.y}"
        flags = "".join(f"-{n}" for n, on in (("nobias", not bias), ("nosilu", not silu), ("prefill", prefill), ("sat", scale != 1.0)) if on)
        self.id = f"{kernel}-B{B}D{D}L{L}W{W}-{lay}{flags}"

    def lay(self, which):
        return _layout(getattr(self, which), self.B, self.D, self.L)

    def dtypes(self):
        return self.only or DTYPES


MIXER = dict(x="half", dy="cmajor", dx="cmajor_half")             # what _MambaInnerFn passes: three layouts in one call
CMAJOR = dict(x="cmajor")
OPTIONS = (dict(silu=False), dict(bias=False), dict(prefill=True))

FWD_CASES = (
    [Case("fwd_vec", 2, 3, L, x=lx, y=ly) for L in (4, 8, 12, 20, 2052)
     for lx, ly in (("contig", "contig"), ("half", "contig"), ("cmajor", "cmajor"), ("padded", "padded"))]
    + [Case("fwd4", 2, 3, L) for L in (1, 2, 3, 5, 197, 1025)]
    + [Case("fwd4", 2, 3, 12, x="shift1"), Case("fwd4", 2, 3, 12, x="contig", y="shift2"), Case("fwd4", 2, 3, 197, x="half", y="cmajor_padded")]
    + [Case("fwd0", 2, 3, L, W=W) for W in (1, 2, 3, 5, 8) for L in (1, 7, 50)]
    + [Case(k, 2, 3, L, W=W, bias=bi, silu=si) for k, L, W in (("fwd_vec", 20, 4), ("fwd4", 197, 4), ("fwd0", 50, 3))
       for bi, si in ((False, True), (True, False), (False, False))]
)
# more work items than the 4096 x 256 threads of the capped grid: the grid-stride loop takes a second turn (fp16 only)
GRID_CASES = [Case("fwd_vec", 8, 256, 4104), Case("fwd4", 4, 256, 4101), Case("fwd0", 4, 256, 4101, W=3)]

BWD_CASES = (
    [Case("bwd_vec_rows", B, 4, L, **lay) for B, L in ((5, 8), (3, 12), (23, 200), (9, 512)) for lay in ({}, MIXER, CMAJOR)]
    + [Case("bwd_short", 7, 4, 197), Case("bwd_short", 3, 4, 509), Case("bwd_short", 5, 4, 1), Case("bwd_short", 4, 4, 3),
       Case("bwd_short", 6, 4, 197, x="padded"),                  # aligned pointers, L % 4 != 0
       Case("bwd_short", 6, 4, 197, x="cmajor_padded"), Case("bwd_short", 7, 4, 197, **MIXER)]
    + [Case("bwd_vec", 2, 3, L, **lay) for L in (516, 1028, 2052) for lay in ({}, MIXER, CMAJOR)]
    + [Case("bwd4", 2, 3, 510), Case("bwd4", 2, 3, 1025), Case("bwd4", 2, 3, 2051),
       Case("bwd4", 2, 3, 2051, x="padded", dx="contig", vec_tiles=True),   # vector body + scalar halos on tiles 0 and 1, scalar last tile
       Case("bwd4", 2, 3, 2051, x="cmajor_padded", vec_tiles=True),
       Case("bwd4", 2, 3, 2052, x="contig", dx="shift2", vec_tiles=True)]
    + [Case("bwd0", 2, 3, L, W=W) for W in (1, 2, 3, 5, 8) for L in (50, 1030)]
    + [Case("bwd0", 2, 3, 2048, W=3, vec_tiles=True)]              # vector body with two-step halos
    + [Case(k, B, 3, L, W=W, **lay, **opt) for k, B, L, W, lay in (
        ("bwd_vec_rows", 5, 200, 4, MIXER), ("bwd_short", 7, 197, 4, MIXER), ("bwd_vec", 2, 1028, 4, MIXER),
        ("bwd4", 2, 1025, 4, {}), ("bwd0", 2, 1030, 5, {})) for opt in OPTIONS]
    # pre-activations over +-100 and beyond: the sigmoid saturates both ways, everything stays finite and inside the bound
    + [Case("bwd_short", 4, 4, 197, scale=30.0, only=[torch.bfloat16, torch.float16])]
)


def _params(cases, *more):
    out = [(c, dt) for c in cases for dt in c.dtypes()]
    for extra in more:
        out = [p + (e,) for p in out for e in extra]
    return [pytest.param(*p, id="-".join([p[0].id, _DT[p[1]], *map(str, p[2:])])) for p in out]


def _sparse_mask(L, W):
    """few terms per channel, all of them where a kernel can drop or double one: row start, row end, both sides of every tile edge"""
    m = torch.zeros(L, dtype=torch.bool)
    m[:W] = True                                                  # with the next line: the first and the last step of every row,
    m[-8:] = True                                                 # where the rows of a group meet in the short-row kernels
    if L > 1024:
        for e in range(1024, L, 1024):
            m[e - 5:e + 5] = True
    return m


@functools.lru_cache(maxsize=None)
def _data(case, dtype, dy_kind):
    """inputs of a case (CPU, io dtype) and the float64 reference, computed once and shared by the CPU and the GPU test"""
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.id}{_DT[dtype]}{dy_kind}".encode()))
    x = (torch.randn(c.B, c.D, c.L, generator=g) * c.scale).to(dtype)
    w = torch.randn(c.D, c.W, generator=g)
    b = torch.randn(c.D, generator=g) if c.bias else None
    dy = dw0 = db0 = None
    if c.backward:
        dy = torch.randn(c.B, c.D, c.L, generator=g)
        if dy_kind == "sparse":
            dy = dy * _sparse_mask(c.L, c.W)
        dy = dy.to(dtype)
        if c.prefill:
            dw0, db0 = torch.randn(c.D, c.W, generator=g), (torch.randn(c.D, generator=g) if c.bias else None)
    r = _conv_ref(x, w, b, c.silu, dy, dtype, dw0, db0)
    del r.xw
    r.dpre = None
    return types.SimpleNamespace(x=x, w=w, b=b, dy=dy, dw0=dw0, db0=db0, ref=r)


def _honest_fp32(x, w, b, silu, dy, io, dw0=None, db0=None):
    """the operation as anybody would write it in fp32: what the bound has to let through"""
    D, W = w.shape
    xf, wf = x.float().requires_grad_(True), w.clone().requires_grad_(True)
    bf = b.clone().requires_grad_(True) if b is not None else None
    pre = F.conv1d(xf, wf[:, None, :], bf, groups=D, padding=W - 1)[..., :x.shape[-1]]
    y = F.silu(pre) if silu else pre
    if dy is None:
        return y.detach().to(io), None, None, None
    y.backward(dy.float())
    dw = wf.grad if dw0 is None else dw0 + wf.grad
    db = None if b is None else (bf.grad if db0 is None else db0 + bf.grad)
    return y.detach().to(io), xf.grad.to(io), dw, db


def _ratios(ref, y, dx=None, dw=None, db=None):
    return dict(y=_ratio(y, ref.y, ref.ty), dx=None if dx is None else _ratio(dx, ref.dx, ref.tdx),
                dw=None if dw is None else _ratio(dw, ref.dw, ref.tdw), db=None if db is None or ref.db is None else _ratio(db, ref.db, ref.tdb))


# ---- CPU: the table reaches what it says it reaches ----------------------------------------------------------------------------------
def test_cases_land_on_their_kernels_and_cover_all_eight():
    seen = set()
    for c in FWD_CASES + GRID_CASES + BWD_CASES:
        assert c.D <= 8 or c in GRID_CASES
        for dt in c.dtypes():
            fk = _fwd_kernel_for(c.W, c.L, c.lay("x"), c.lay("y"), dt)
            if c.backward:
                bk, vec_tiles = _bwd_kernel_for(c.W, c.L, c.D, c.lay("x"), c.lay("dy"), c.lay("dx"), dt)
                assert (bk, vec_tiles) == (c.kernel, c.vec_tiles), f"{c.id} {_DT[dt]}: takes {bk}, vector tiles {vec_tiles}"
                seen.add((bk, dt))
            else:
                assert fk == c.kernel, f"{c.id} {_DT[dt]}: takes {fk}"
            seen.add((fk, dt))
    assert seen >= {(k, dt) for k in FWD_KERNELS + BWD_KERNELS for dt in DTYPES}
    for k in FWD_KERNELS:                                          # the second turn of the grid-stride loop
        c = next(c for c in GRID_CASES if c.kernel == k)
        assert c.B * c.D * ((c.L + 7) // 8 if k == "fwd_vec" else (c.L + 3) // 4) > 4096 * 256
    for k in BWD_KERNELS:                                          # every option on every backward kernel
        for opt in ("nosilu", "nobias", "prefill"):
            assert any(c.kernel == k and c.id.endswith(opt) for c in BWD_CASES), (k, opt)
    short = [c for c in BWD_CASES if c.kernel == "bwd_short"]
    assert any(c.B > 1024 // (c.L + 3) and c.B % (1024 // (c.L + 3)) for c in short), "ragged last group of the short-row kernel"
    assert any(1024 // (c.L + 3) == 2 for c in short) and any(c.kernel == "bwd4" and c.L == 510 for c in BWD_CASES)


# ---- CPU: the reference against the goldens --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["conv1d_L3", "conv1d_L9", "conv1d_L197"])
def test_conv_ref_reproduces_goldens(name):
    g = load_golden(name)
    w = g["weight"].squeeze(1)
    r = _conv_ref(g["x"], w, g["bias"], True, g["dy"], torch.float32)
    assert_close(r.y, g["y"], 1e-5, 1e-5, "y")
    assert_close(r.dx, g["dx"], 1e-5, 1e-4, "dx")
    assert_close(r.dw, g["dweight"].squeeze(1), 1e-4, 1e-4, "dweight")
    assert_close(r.db, g["dbias"], 1e-4, 1e-4, "dbias")
    assert_close(_conv_ref(g["x"], w, g["bias"], False, None, torch.float32).y, g["y_noact"], 1e-5, 1e-5, "y_noact")
    # the goldens are honest fp32 results themselves: inside the bound
    _report(name, y=_ratio(g["y"], r.y, r.ty), dx=_ratio(g["dx"], r.dx, r.tdx), dw=_ratio(g["dweight"].squeeze(1), r.dw, r.tdw),
            db=_ratio(g["dbias"], r.db, r.tdb))


def test_step_refs_reproduce_mamba_step_golden():
    """_update_ref and _state_ref chained as Mamba.step chains the two kernels (the loop of test_decode_step_kernels_golden)"""
    g = {k: v.double() for k, v in load_golden("mamba_step").items()}
    A = -torch.exp(g["p_A_log"])
    Bz, T, d = g["xs"].shape[0], g["xs"].shape[1], g["p_conv1d.weight"].shape[0]
    N, R = A.shape[1], g["p_dt_proj.weight"].shape[1]
    w, b = g["p_conv1d.weight"].squeeze(1).float(), g["p_conv1d.bias"].float()
    conv_state, ssm_state = torch.zeros(Bz, d, w.shape[1], dtype=torch.float64), torch.zeros(Bz, d, N, dtype=torch.float64)
    for t in range(T):
        x, z = (g["xs"][:, t] @ g["p_in_proj.weight"].t()).chunk(2, dim=-1)
        x, _, conv_state = _update_ref(x, conv_state, w, b, True, torch.float32)
        dt, Bm, Cm = torch.split(x @ g["p_x_proj.weight"].t(), [R, N, N], dim=-1)
        dt = dt @ g["p_dt_proj.weight"].t()
        ssm_state, _, y, _ = _state_ref(ssm_state, x, dt, A, Bm, Cm, g["p_D"], z, g["p_dt_proj.bias"], True, torch.float32)
        assert_close(y @ g["p_out_proj.weight"].t(), g["outs"][:, t], 2e-5, 1e-4, f"out[{t}]")
        assert_close(conv_state, g["conv_states"][t], 1e-6, 1e-6, f"conv_state[{t}]")
        assert_close(ssm_state, g["ssm_states"][t], 1e-5, 1e-4, f"ssm_state[{t}]")


# ---- CPU: an honest fp32 implementation stays under the bound ------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", _params(FWD_CASES))
def test_honest_fp32_forward_within_bound(case, dtype):
    d = _data(case, dtype, "dense")
    y, _, _, _ = _honest_fp32(d.x, d.w, d.b, case.silu, None, dtype)
    _report(f"honest {case.id} {_DT[dtype]}", **_ratios(d.ref, y))


@pytest.mark.parametrize("case,dtype,dy_kind", _params(BWD_CASES, ("dense", "sparse")))
def test_honest_fp32_backward_within_bound(case, dtype, dy_kind):
    d = _data(case, dtype, dy_kind)
    out = _honest_fp32(d.x, d.w, d.b, case.silu, d.dy, dtype, d.dw0, d.db0)
    _report(f"honest {case.id} {_DT[dtype]} {dy_kind}", **_ratios(d.ref, *out))


def _grid_rows(c):
    """64 (b, d) rows: the first, the last four (the second turn of the loop lands there), random ones between"""
    n = c.B * c.D
    g = torch.Generator().manual_seed(c.L)
    rows = torch.cat([torch.tensor([0, n - 4, n - 3, n - 2, n - 1]), torch.randint(1, n - 4, (59,), generator=g)])
    return rows // c.D, rows % c.D


@functools.lru_cache(maxsize=None)
def _grid_data(case):
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    x = torch.randn(c.B, c.D, c.L, generator=g).to(torch.float16)
    w, b = torch.randn(c.D, c.W, generator=g), torch.randn(c.D, generator=g)
    bi, di = _grid_rows(c)
    r = _conv_ref(x[bi, di][None], w[di], b[di], True, None, torch.float16)   # the sampled rows as the channels of one batch
    del r.xw
    return types.SimpleNamespace(x=x, w=w, b=b, bi=bi, di=di, ref=r)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in GRID_CASES])
def test_honest_fp32_grid_rows_within_bound(case):
    d = _grid_data(case)
    y, _, _, _ = _honest_fp32(d.x[d.bi, d.di][None], d.w[d.di], d.b[d.di], True, None, torch.float16)
    _report(f"honest {case.id} fp16", y=_ratio(y, d.ref.y, d.ref.ty))


def _state_inputs(B, D, N, dtype, softplus, seed, T=2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    # softplus on: dt + bias spread over about [-30, 30], across the threshold at 20; off: a positive step as the mixer has it
    dt = (torch.rand(T, B, D, generator=g) * 60 - 30) if softplus else (torch.rand(T, B, D, generator=g) * 0.5 + 1e-3)
    return types.SimpleNamespace(h0=r(B, D, N), x=r(T, B, D).to(dtype), dt=dt.to(dtype), A=-torch.rand(D, N, generator=g) - 0.05,
                                 Bm=r(T, B, N).to(dtype), Cm=r(T, B, N).to(dtype), D=r(D), z=r(T, B, D).to(dtype), dt_bias=torch.rand(D, generator=g) * 0.5)


STATE_SHAPES = [(3, 100, 16), (2, 7, 1), (1, 300, 5)]
STATE_VARIANTS = [(), ("D",), ("z",), ("dt_bias",), ("D", "z", "dt_bias")]     # the optional arguments left out


def _honest_state_fp32(h, x, dt, A, Bm, Cm, D, z, dt_bias, softplus, io):
    x, dt, Bm, Cm = x.float(), dt.float(), Bm.float(), Cm.float()
    dtv = dt + dt_bias if dt_bias is not None else dt
    dtv = F.softplus(dtv) if softplus else dtv
    hn = h * torch.exp(dtv[..., None] * A) + (x * dtv)[..., None] * Bm[:, None, :]
    y = (hn * Cm[:, None, :]).sum(-1)
    if D is not None:
        y = y + D * x
    if z is not None:
        y = y * F.silu(z.float())
    return hn, y.to(io)


@pytest.mark.parametrize("softplus", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
@pytest.mark.parametrize("shape", STATE_SHAPES)
def test_honest_fp32_state_update_within_bound(shape, dtype, softplus):
    s = _state_inputs(*shape, dtype, softplus, seed=shape[1])
    for drop in STATE_VARIANTS:
        opt = {k: (None if k in drop else getattr(s, k)) for k in ("D", "z", "dt_bias")}
        z = opt["z"][0] if opt["z"] is not None else None
        hn, y = _honest_state_fp32(s.h0, s.x[0], s.dt[0], s.A, s.Bm[0], s.Cm[0], opt["D"], z, opt["dt_bias"], softplus, dtype)
        rh, th, ry, ty = _state_ref(s.h0, s.x[0], s.dt[0], s.A, s.Bm[0], s.Cm[0], opt["D"], z, opt["dt_bias"], softplus, dtype)
        _report(f"honest state {shape} {_DT[dtype]} softplus={softplus} without {drop}", state=_ratio(hn, rh, th), y=_ratio(y, ry, ty))


# ---- CPU: the bound notices planted errors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
def test_bound_flags_planted_errors(dtype):
    g = torch.Generator().manual_seed(7)
    B, D, L, W = 2, 3, 2052, 4
    x, w, b = torch.randn(B, D, L, generator=g).to(dtype), torch.randn(D, W, generator=g), torch.randn(D, generator=g)
    dy = (torch.randn(B, D, L, generator=g) * _sparse_mask(L, W)).to(dtype)
    r = _conv_ref(x, w, b, True, dy, dtype)
    # (1) the three x-halo taps of the second tile missing from dweight: dpre[t] x[t-3+k] with t - 3 + k < 1024 <= t
    dw = r.dw.clone()
    for t in (1024, 1025, 1026):
        for k in range(W):
            if t - (W - 1) + k < 1024:
                dw[:, k] -= (r.dpre[:, :, t] * r.xw[:, :, t, k]).sum(0)
    halo = _ratio(dw, r.dw, r.tdw)
    # (2) dx[L-1] takes dpre at t = L for the next row's first step instead of zero
    dx = r.dx.clone()
    nxt = r.dpre.reshape(B * D, L).roll(-1, 0).reshape(B, D, L)[..., 0]
    dx[..., L - 1] += w.double()[:, W - 2] * nxt
    over = _ratio(dx.to(dtype), r.dx, r.tdx)
    # (3) taps reversed
    rev = _ratio(_conv_ref(x, w.flip(-1), b, True, None, dtype).y.to(dtype), r.y, r.ty)
    print(f"planted {_DT[dtype]}: dweight halo {halo:.1f} dx overrun {over:.1f} taps reversed {rev:.1f}")
    assert halo > 1 and over > 1 and rev > 1
    assert _ratio(r.dw.float(), r.dw, r.tdw) <= 1 and _ratio(r.dx.to(dtype), r.dx, r.tdx) <= 1 and _ratio(r.y.to(dtype), r.y, r.ty) <= 1
    # (4) one state column skipped
    s = _state_inputs(3, 100, 16, dtype, True, seed=3)
    args = (s.h0, s.x[0], s.dt[0], s.A, s.Bm[0], s.Cm[0], s.D, s.z[0], s.dt_bias, True, dtype)
    rh, th, ry, ty = _state_ref(*args)
    bh, _, by, _ = _state_ref(*args, skip_col=5)
    print(f"planted {_DT[dtype]}: state column skipped: state {_ratio(bh.float(), rh, th):.1f} y {_ratio(by.to(dtype), ry, ty):.1f}")
    assert _ratio(bh.float(), rh, th) > 1 and _ratio(by.to(dtype), ry, ty) > 1
    assert _ratio(rh.float(), rh, th) <= 1 and _ratio(ry.to(dtype), ry, ty) <= 1


# ---- CPU: what the entries refuse before any launch ----------------------------------------------------------------------------------
def _fake_desc(**kw):
    d = _abi.Conv1dBwdDesc()
    f = d.fwd
    f.batch, f.dim, f.seqlen, f.width, f.io_dtype, f.silu = 2, 4, 16, 4, _abi.MXVL_BF16, 1
    f.x_bs, f.x_ds, f.y_bs, f.y_ds = 64, 16, 64, 16
    f.x, f.weight, f.bias, f.y = 0x1000, 0x2000, 0x3000, 0x4000      # never dereferenced: every descriptor below is refused
    d.dy_bs, d.dy_ds, d.dx_bs, d.dx_ds = 64, 16, 64, 16
    d.dy, d.dx, d.dweight, d.dbias = 0x5000, 0x6000, 0x7000, 0x8000
    for k, v in kw.items():
        setattr(f if hasattr(f, k) else d, k, v)
    return d


def test_conv_descriptor_refusals_without_gpu():
    lib = _abi.load()
    code = {v: k for k, v in _abi.STATUS.items()}
    fwd = lambda **kw: lib.mxvl_conv1d_fwd(ctypes.byref(_fake_desc(**kw).fwd), None)
    bwd = lambda **kw: lib.mxvl_conv1d_bwd(ctypes.byref(_fake_desc(**kw)), None)
    for call in (fwd, bwd):
        assert call(width=9) == code["MXVL_ERR_UNSUPPORTED"]
        for bad in (3, -1, 1 << 20):
            assert call(io_dtype=bad) == code["MXVL_ERR_DTYPE"]
        assert call(x=None) == code["MXVL_ERR_NULL"] and call(weight=None) == code["MXVL_ERR_NULL"]
        assert call(x_bs=-64) == code["MXVL_ERR_STRIDE"] and call(x_ds=-16) == code["MXVL_ERR_STRIDE"]
        for k in ("batch", "dim", "seqlen", "width"):
            assert call(**{k: 0}) == code["MXVL_ERR_SHAPE"], k
    assert fwd(y=None) == code["MXVL_ERR_NULL"]
    for k in ("dy", "dx", "dweight", "dbias"):                     # dbias: a bias is set, so its gradient needs somewhere to go
        assert bwd(**{k: None}) == code["MXVL_ERR_NULL"], k
    assert lib.mxvl_conv1d_fwd(None, None) == code["MXVL_ERR_NULL"] and lib.mxvl_conv1d_bwd(None, None) == code["MXVL_ERR_NULL"]


# ---- GPU: forward ------------------------------------------------------------------------------------------------------------------------
def _gpu_forward(c, dtype, d):
    x = _Buf.rows(c.x, c.B, c.D, c.L, dtype, DEV, d.x)
    y = _Buf.rows(c.y, c.B, c.D, c.L, dtype, DEV)
    w, b = d.w.to(DEV), (d.b.to(DEV) if d.b is not None else None)
    assert tuple(x.view.stride()) == c.lay("x")[2] and tuple(y.view.stride()) == c.lay("y")[2]
    _launch_fwd(x.view, w, b, y.view, c.silu)
    torch.cuda.synchronize()
    assert x.unchanged(), "x modified"
    assert y.guard_intact(), "store outside y"
    assert y.written(), "y not fully written (or a read outside x reached it)"
    return y.view


@gpu
@pytest.mark.parametrize("case,dtype", _params(FWD_CASES))
def test_conv1d_forward(case, dtype):
    d = _data(case, dtype, "dense")
    y = _gpu_forward(case, dtype, d)
    _report(f"{case.kernel} {_DT[dtype]} {case.id}", **_ratios(d.ref, y))


@gpu
@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in GRID_CASES])
def test_conv1d_forward_grid_stride(case):
    d = _grid_data(case)
    y = _gpu_forward(case, torch.float16, d)
    _report(f"{case.kernel} fp16 {case.id}", y=_ratio(y[d.bi.to(DEV), d.di.to(DEV)][None], d.ref.y, d.ref.ty))


# ---- GPU: backward -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,dtype,dy_kind", _params(BWD_CASES, ("dense", "sparse")))
def test_conv1d_backward(case, dtype, dy_kind):
    c, d = case, _data(case, dtype, dy_kind)
    y = _gpu_forward(c, dtype, d)
    x = _Buf.rows(c.x, c.B, c.D, c.L, dtype, DEV, d.x)
    dy = _Buf.rows(c.dy, c.B, c.D, c.L, dtype, DEV, d.dy)
    dx = _Buf.rows(c.dx, c.B, c.D, c.L, dtype, DEV)
    w, b = d.w.to(DEV), (d.b.to(DEV) if d.b is not None else None)
    dw = _Buf.flat((c.D, c.W), torch.float32, DEV, d.dw0 if d.dw0 is not None else torch.zeros(c.D, c.W))
    db = _Buf.flat((c.D,), torch.float32, DEV, d.db0 if d.db0 is not None else torch.zeros(c.D)) if c.bias else None
    for buf, which in ((x, "x"), (dy, "dy"), (dx, "dx")):
        assert tuple(buf.view.stride()) == c.lay(which)[2]
    _launch_bwd(x.view, w, b, c.silu, dy.view, dx.view, dw.view, db.view if db is not None else None)
    torch.cuda.synchronize()
    assert x.unchanged() and dy.unchanged(), "an input was modified"
    assert dx.guard_intact(), "store outside dx"
    assert dw.guard_intact() and (db is None or db.guard_intact()), "store outside dweight / dbias"
    assert dx.written(), "dx not fully written (or a read outside x / dy reached it)"
    _report(f"{c.kernel} {_DT[dtype]} {c.id} {dy_kind}", **_ratios(d.ref, y, dx.view, dw.view, db.view if db is not None else None))
    for t in (y, dx.view, dw.view):
        assert bool(torch.isfinite(t).all())


# ---- GPU: the single-token steps -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
@pytest.mark.parametrize("W", [2, 3, 4, 8])
@pytest.mark.parametrize("shape", [(3, 100), (1, 7)])
def test_conv1d_update_steps(shape, W, dtype):
    from medical_image_analysis_amd.causal_conv1d import causal_conv1d_update
    B, D = shape
    g = torch.Generator().manual_seed(100 * D + W)
    w, bias = torch.randn(D, W, generator=g), torch.randn(D, generator=g)
    for b in (bias, None):
        for silu in (True, False):
            x, st = torch.randn(B, D, generator=g).to(dtype), torch.randn(B, D, W, generator=g).to(dtype)
            ry, ty, rst = _update_ref(x, st, w, b, silu, dtype)
            st_d = st.to(DEV)
            y = causal_conv1d_update(x.to(DEV), st_d, w.to(DEV), b.to(DEV) if b is not None else None, "silu" if silu else None)
            assert torch.equal(st_d.cpu(), rst), "the new state is the old taps 1 .. W-1, then x, bit for bit"
            _report(f"conv1d_update {_DT[dtype]} {shape} W{W} bias={b is not None} silu={silu}", y=_ratio(y, ry, ty))
    # six steps from a zero state are the first six outputs of the convolution of the same sequence
    xs = torch.randn(B, D, 6, generator=g).to(dtype)
    r = _conv_ref(xs, w, bias, True, None, dtype)
    st_d = torch.zeros(B, D, W, dtype=dtype, device=DEV)
    ys = torch.stack([causal_conv1d_update(xs[..., t].to(DEV), st_d, w.to(DEV), bias.to(DEV), "silu") for t in range(6)], -1)
    _report(f"conv1d_update {_DT[dtype]} {shape} W{W} six steps", y=_ratio(ys, r.y, r.ty))


@gpu
@pytest.mark.parametrize("softplus", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
@pytest.mark.parametrize("shape", STATE_SHAPES)
def test_selective_state_update_steps(shape, dtype, softplus):
    from medical_image_analysis_amd.selective_state_update import selective_state_update
    s = _state_inputs(*shape, dtype, softplus, seed=shape[1])
    dev = lambda t: None if t is None else t.to(DEV)
    for drop in STATE_VARIANTS:
        opt = {k: (None if k in drop else getattr(s, k)) for k in ("D", "z", "dt_bias")}
        h = s.h0.to(DEV)
        for t in range(2):                                          # the second step reads the state the first one wrote
            z = opt["z"][t] if opt["z"] is not None else None
            rh, th, ry, ty = _state_ref(h.cpu(), s.x[t], s.dt[t], s.A, s.Bm[t], s.Cm[t], opt["D"], z, opt["dt_bias"], softplus, dtype)
            y = selective_state_update(h, dev(s.x[t]), dev(s.dt[t]), dev(s.A), dev(s.Bm[t]), dev(s.Cm[t]), dev(opt["D"]), z=dev(z),
                                       dt_bias=dev(opt["dt_bias"]), dt_softplus=softplus)
            assert y.dtype == dtype and y.shape == s.x[t].shape
            _report(f"state_update {_DT[dtype]} {shape} softplus={softplus} without {drop} step {t}", state=_ratio(h, rh, th), y=_ratio(y, ry, ty))


# ---- GPU: the wrappers refuse mis-shaped arguments before anything is enqueued -------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    count, real = [], _abi.launch

    def counting(name, *a, **kw):
        count.append(name)
        return real(name, *a, **kw)

    monkeypatch.setattr(_abi, "launch", counting)
    return count


@gpu
def test_selective_state_update_refuses_bad_shapes(launches):
    from medical_image_analysis_amd.selective_state_update import selective_state_update
    B, D, N = 2, 6, 4
    good = dict(state=torch.zeros(B, D, N), x=torch.randn(B, D), dt=torch.rand(B, D), A=-torch.rand(D, N), B=torch.randn(B, N),
                C=torch.randn(B, N), D=torch.randn(D), z=torch.randn(B, D), dt_bias=torch.rand(D))
    bad = dict(x=[(B, D + 1), (B + 1, D), (B * D,)], dt=[(B, D + 1), (B, 1), (B + 1, D), (D,)], A=[(D, N + 1), (D + 1, N)],
               B=[(B, N + 1), (B + 1, N), (B, 1, N)], C=[(B, N + 1), (B, N - 1), (B + 1, N), (N,)], z=[(B, D - 1), (B + 1, D), (D,)],
               D=[(D + 1,), (D - 1,), (1,), (B, D)], dt_bias=[(D + 1,), (D - 1,), (1,), (B, D)])
    for name, shapes in bad.items():
        for shp in shapes:
            kw = {k: v.to(DEV) for k, v in good.items()}
            kw[name] = torch.rand(*shp, device=DEV)
            with pytest.raises(RuntimeError, match="shape mismatch"):
                selective_state_update(**kw)
    assert launches == [], "a mis-shaped call reached the kernel"
    selective_state_update(**{k: v.to(DEV) for k, v in good.items()})
    assert launches == ["mxvl_state_update"]


@gpu
def test_causal_conv1d_update_refuses_bad_shapes(launches):
    from medical_image_analysis_amd.causal_conv1d import causal_conv1d_update
    B, D, W = 2, 6, 4
    good = dict(x=torch.randn(B, D), conv_state=torch.zeros(B, D, W), weight=torch.randn(D, W), bias=torch.randn(D))
    bad = dict(conv_state=[(B, D, W - 1), (B, D, W + 1), (B, D - 1, W), (B + 1, D, W), (B, D * W), (B, W, D)],
               weight=[(D + 1, W), (D - 1, W), (D, W + 1)], bias=[(D + 1,), (D - 1,), (1,), (D, 1)], x=[(B, D + 1), (B + 1, D), (B, D, 1)])
    for name, shapes in bad.items():
        for shp in shapes:
            kw = {k: v.to(DEV) for k, v in good.items()}
            kw[name] = torch.rand(*shp, device=DEV)
            with pytest.raises(RuntimeError, match="must be"):
                causal_conv1d_update(**kw)
    assert launches == [], "a mis-shaped call reached the kernel"
    causal_conv1d_update(**{k: v.to(DEV) for k, v in good.items()})
    assert launches == ["mxvl_conv1d_update"]


@gpu
def test_causal_conv1d_fn_refuses_bad_bias(launches):
    from medical_image_analysis_amd.causal_conv1d import causal_conv1d_fn
    B, D, L, W = 2, 6, 10, 4
    x, w = torch.randn(B, D, L, device=DEV), torch.randn(D, W, device=DEV)
    for shp in ((D + 1,), (D - 1,), (1,), (D, 1), (B, D)):
        with pytest.raises(RuntimeError, match="bias must be"):
            causal_conv1d_fn(x, w, torch.randn(*shp, device=DEV), "silu")
    assert launches == [], "a mis-shaped call reached the kernel"
    causal_conv1d_fn(x, w, torch.randn(D, device=DEV), "silu")
    assert launches == ["mxvl_conv1d_fwd"]
