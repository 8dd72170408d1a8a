"""csrc/dir_perm.hip: every kernel perm_launch() can choose (`vec`: 16-bit io with 16-byte stacked rows, `short`: padded_len <= 256 and at
most six directions, generic), gather and merge, plain and gated, in fp32 / bf16 / fp16.

What is exact is compared as bits: the gather (indexing plus zero padding), the ungated merge and the `pre` of the gated merge (an fp32
sum over the directions in ascending k, rounded once to the io dtype: acc = 0; acc += y_k[inv_k]).  The gated outputs go against a float64
restatement with a per-element bound in the model of fp64_bounds.py (U = 2^-24 per fp32 operation, first order; _rho(z) the relative error
of the kernels' sigmoid; _ulp one unit in the last place of the output type; FLOOR), with s = sigmoid(z), g = dout scale:

    out = S silu(z) scale, S the exact sum of the K terms.  The fp32 sum carries (K - 1) U sum |y_k| in ANY order of the terms; silu(z) =
        fl(z s) carries rho + U, the two multiplications U each:
        t_out = |silu(z)| scale (K - 1) U sum |y_k|  +  |out| (rho + 3 U)  +  ulp(out)
    dz  = g pre s (1 + z (1 - s)) with the `pre` the kernel is handed (an input, exact).  fl(1 - s) carries s rho + U (1 - s) absolutely
        (for z >> 0 that is far more than (1 - s) itself can absorb relatively), the fma then |z| times that plus U |inner|, inner = 1 +
        z (1 - s); s inner adds rho + U relatively; g, g pre and the last product U each:
        t_dz = |g pre| (s |z| (s rho + U (1 - s))  +  |s inner| (rho + 2 U))  +  |dz| 3 U  +  ulp(dz)
    dy  = gather(g z s): fl(z s) carries rho + U, g and the product U each:  t_dy = |dy| (rho + 3 U) + ulp(dy); padding is exactly zero.

The 16-bit kernels round the fp32 result once more on the store; one ulp of the output type covers that second rounding.  Two CPU tests
hold the bound in place: an honest fp32 torch implementation with the same rounding points stays under it (so does a K-descending sum),
and a dropped direction, `scale` applied twice, a gate taken from the neighbouring channel and a `pre` taken after the gate do not.

Every tensor a kernel touches is a view into a NaN-patterned buffer with guard bands (fp64_bounds._Buf).  The (batch, dim, seqlen) tensors
are halves of a (B, 2 D, L) buffer, as the mixer passes the x and z parts of xz (the other half must keep its pattern: a store to channel
D + r of a ragged last row group lands there), or channel-major (D, B, L) storage as the mixer's `out` and `pre`; the index tensors are
guarded too.  Launches go through _abi.launch with the test's own descriptor."""
import ctypes
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

from fp64_bounds import FLOOR, GUARD, U, _assert_buffers, _Buf, _ptr, _ratio, _report, _rho, _ulp
from medical_image_analysis_amd import _abi

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALF = DTYPES[1:]
_DT = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
_ESZ = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}
gpu = pytest.mark.gpu
SCALE = float(torch.tensor(0.3, dtype=torch.float32))             # the descriptor carries a float: the reference uses what the kernel gets
MAX_LEN, MAX_DIRS, GATHER_ROWS, MERGE_ROWS, VEC_ROWS = 256 * 20, 6, 8, 4, 8


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- 1. perm_launch() restated, and the cases --------------------------------------------------------------------------------------------
def _path(dtype, L, Lp, K, stacked_strides, stacked_offset_bytes=0):
    short = Lp <= 256 and K <= MAX_DIRS
    vec = (short and dtype != torch.float32 and Lp % 8 == 0 and L <= 248 and stacked_offset_bytes % 16 == 0
           and all(s % 8 == 0 for s in stacked_strides[:3]))
    return "vec" if vec else "short" if short else "generic"


class Case:
    """layout of the stacked tensor: 'flat' contiguous, 'mixer' (K, D, B, Lp) storage as _MultiDirMixerFn allocates it, 'shift4' rows
    of Lp + 8 elements with the view starting 4 elements into them"""

    def __init__(self, L, Lp, K, D=11, B=2, layout="flat"):
        self.L, self.Lp, self.K, self.D, self.B, self.layout = L, Lp, K, D, B, layout
        self.id = f"L{L}Lp{Lp}K{K}D{D}" + ("" if layout == "flat" else "-" + layout)

    def stacked_geom(self):
        """-> (elements of storage, offset past the guard, strides) of the (B, K, D, Lp) view"""
        B, K, D, Lp = self.B, self.K, self.D, self.Lp
        if self.layout == "mixer":
            return B * K * D * Lp, 0, (Lp, D * B * Lp, B * Lp, 1)
        Lq = Lp + 8 if self.layout == "shift4" else Lp
        return B * K * D * Lq, 4 if self.layout == "shift4" else 0, (K * D * Lq, D * Lq, Lq, 1)

    def path(self, dtype):
        _, off, strides = self.stacked_geom()
        return _path(dtype, self.L, self.Lp, self.K, strides, (GUARD + off) * _ESZ[dtype])


CASES = [
    Case(197, 200, 4, D=43, layout="mixer"),                      # the production geometry, ragged D: vec in 16-bit, short in fp32
    Case(248, 248, 6),                                            # vec, no padding lanes, full sentinel range
    Case(248, 256, 4),                                            # vec, eight padding elements that read the sentinel
    Case(1, 8, 1, D=1),                                           # vec: one token, one direction, one channel
    Case(249, 256, 4),                                            # short in 16-bit: the first length the uint8 index tile refuses
    Case(256, 256, 4),                                            # short, every thread live
    Case(197, 197, 4),                                            # short by Lp % 8
    Case(197, 200, 4, layout="shift4"),                           # short by alignment
    Case(1, 1, 1, D=1),
    Case(10, 16, 4, D=1), Case(10, 16, 4, D=3), Case(10, 16, 4, D=9),   # below, across and past a row group (8 gather, 4 merge, 8 vec)
    Case(10, 16, 7),                                              # generic by K > 6 at a short length
    Case(257, 264, 4),                                            # generic, the first length past short
    Case(4097, 4104, 4, D=5),                                     # generic, 17 steps per thread
    Case(5120, 5120, 2, D=2),                                     # generic at the MAXT limit, no padding
]
_VS = dict(zip(DTYPES, ("short", "vec", "vec")))                  # vec where the dtype allows it
_ALL = lambda path: dict.fromkeys(DTYPES, path)
# name -> (the path each dtype has to take, predicate over the case)
NEED = {
    "production 197 / 200 / 4, ragged D": (_VS, lambda c: (c.L, c.Lp, c.K) == (197, 200, 4) and c.layout == "mixer" and c.D % 8 and c.D % 4 and c.D > 8),
    "L = Lp = 248, six directions": (_VS, lambda c: (c.L, c.Lp, c.K) == (248, 248, 6)),
    "L 248 with eight padding elements": (_VS, lambda c: (c.L, c.Lp) == (248, 256)),
    "one token, one direction, one channel, Lp 8": (_VS, lambda c: (c.L, c.Lp, c.K, c.D) == (1, 8, 1, 1)),
    "L 249: past the index tile": (_ALL("short"), lambda c: (c.L, c.Lp) == (249, 256)),
    "L = Lp = 256": (_ALL("short"), lambda c: (c.L, c.Lp) == (256, 256)),
    "Lp % 8 != 0": (_ALL("short"), lambda c: c.Lp % 8 != 0 and c.L > 1 and c.L <= 248),
    "stacked view 4 elements into its rows": (_ALL("short"), lambda c: c.layout == "shift4" and c.Lp % 8 == 0 and c.L <= 248),
    "L = Lp = K = 1": (_ALL("short"), lambda c: (c.L, c.Lp, c.K) == (1, 1, 1)),
    "D 1 below a row group": (_VS, lambda c: c.D == 1 and c.K > 1 and c.L > 1),
    "D 3 below a merge row group": (_VS, lambda c: c.D == 3),
    "D 9 past a row group": (_VS, lambda c: c.D == 9),
    "K 7 at a short length": (_ALL("generic"), lambda c: c.K > MAX_DIRS and c.Lp <= 256),
    "Lp 264: first past short": (_ALL("generic"), lambda c: c.K <= MAX_DIRS and 256 < c.Lp <= 264 and c.L > 256),
    "17 steps per thread": (_ALL("generic"), lambda c: -(-c.L // 256) == 17 and c.Lp > c.L),
    "L = Lp = 5120, the limit": (_ALL("generic"), lambda c: c.L == c.Lp == MAX_LEN),
}


def _missing(cases):
    return [f"{k} ({_DT[dt]}: {want})" for k, (paths, pred) in NEED.items() for dt, want in paths.items()
            if not any(pred(c) and c.path(dt) == want for c in cases)]


def test_cases_cover_every_dispatch_path():
    assert _missing(CASES) == [], "not reached"
    for c in CASES:
        assert _missing([o for o in CASES if o is not c]), f"{c.id} reaches nothing of its own"
    assert [c.path(torch.bfloat16) for c in CASES] == [c.path(torch.float16) for c in CASES] == (
        ["vec"] * 4 + ["short"] * 5 + ["vec"] * 3 + ["generic"] * 4)
    assert [c.path(torch.float32) for c in CASES] == ["short"] * 12 + ["generic"] * 4
    # in 16-bit the view 4 elements into its rows is refused by the alignment alone
    assert _path(torch.bfloat16, 197, 200, 4, CASES[7].stacked_geom()[2], 0) == "vec"


# ---- 2. reference and bound ------------------------------------------------------------------------------------------------------------
def _perms(K, L, g):
    perm = torch.stack([torch.randperm(L, generator=g) for _ in range(K)])
    return perm, torch.argsort(perm, dim=1)


def _gather_ref(x, perm, Lp):
    """(B, D, L) -> (B, K, D, Lp): indexing plus zero padding"""
    B, D, L = x.shape
    out = torch.zeros(B, perm.shape[0], D, Lp, dtype=x.dtype)
    for k in range(perm.shape[0]):
        out[:, k, :, :L] = x[:, :, perm[k]]
    return out


def _merge_sum(y, inv, descending=False):
    """(B, K, D, Lp) -> the fp32 sum the kernels form: acc = 0, acc += y_k[inv_k] for k ascending"""
    B, K, D, _ = y.shape
    L = inv.shape[1]
    acc = torch.zeros(B, D, L, dtype=torch.float32)
    for k in (reversed(range(K)) if descending else range(K)):
        acc += y[:, k, :, :L].float()[:, :, inv[k]]
    return acc


def _gated_ref(y, z, dout, perm, inv, Lp, scale, io):
    """float64 restatement of the gated merge and of the gated gather with the tolerances of the docstring; `pre` is exact"""
    B, K, D, _ = y.shape
    L = inv.shape[1]
    S, Sabs = torch.zeros(B, D, L, dtype=torch.float64), torch.zeros(B, D, L, dtype=torch.float64)
    for k in range(K):
        t = y[:, k, :, :L].double()[:, :, inv[k]]
        S += t
        Sabs += t.abs()
    pre = _merge_sum(y, inv).to(io)
    z64 = z.double()
    s, rho = torch.sigmoid(z64), _rho(z64)
    silu = z64 * s
    out = S * silu * scale
    tout = (silu.abs() * scale * (K - 1) * U * Sabs + out.abs() * (rho + 3 * U) + _ulp(out, io)).clamp_min(FLOOR)
    g, p = dout.double() * scale, pre.double()
    inner = 1 + z64 * (1 - s)
    dz = g * p * s * inner
    tdz = ((g * p).abs() * (s * z64.abs() * (s * rho + U * (1 - s)) + (s * inner).abs() * (rho + 2 * U)) + dz.abs() * 3 * U
           + _ulp(dz, io)).clamp_min(FLOOR)
    gg = g * silu
    tgg = (gg.abs() * (rho + 3 * U) + _ulp(gg, io)).clamp_min(FLOOR)
    dy, tdy = _gather_ref(gg, perm, Lp), _gather_ref(tgg, perm, Lp).clamp_min(FLOOR)
    return types.SimpleNamespace(pre=pre, out=out, tout=tout, dz=dz, tdz=tdz, dy=dy, tdy=tdy)


def _ratios(ref, out=None, dz=None, dy=None):
    return dict(out=None if out is None else _ratio(out, ref.out, ref.tout), dz=None if dz is None else _ratio(dz, ref.dz, ref.tdz),
                dy=None if dy is None else _ratio(dy, ref.dy, ref.tdy))


def _data(case, dtype):
    B, K, D, L, Lp = case.B, case.K, case.D, case.L, case.Lp
    g = torch.Generator().manual_seed(zlib.crc32(f"dir_perm {case.id} {_DT[dtype]}".encode()))
    perm, inv = _perms(K, L, g)
    r = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(dtype)
    return types.SimpleNamespace(perm=perm, inv=inv, x=r(B, D, L), y=r(B, K, D, Lp), z=r(B, D, L, scale=2.0), dout=r(B, D, L))


# ---- CPU: an honest fp32 implementation stays under the bound, planted errors do not ---------------------------------------------------
def _honest_fp32(y, z, dout, pre, perm, inv, Lp, scale, io, descending=False):
    """the same rounding points (fp32 throughout, one rounding to the io dtype per output) with torch's own ops"""
    acc, zf = _merge_sum(y, inv, descending), z.float()
    out = (acc * F.silu(zf) * scale).to(io)
    g, s = dout.float() * scale, torch.sigmoid(zf)
    dz = (g * pre.float() * (s * (1 + zf * (1 - s)))).to(io)
    return out, dz, _gather_ref((g * (zf * s)).to(io), perm, Lp)


_SMALL = [Case(50, 56, 4, D=5), Case(37, 40, 6, D=3), Case(300, 304, 7, D=2), Case(9, 9, 1, D=4)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
@pytest.mark.parametrize("case", _SMALL, ids=lambda c: c.id)
def test_honest_fp32_within_bound(case, dtype):
    d = _data(case, dtype)
    ref = _gated_ref(d.y, d.z, d.dout, d.perm, d.inv, case.Lp, SCALE, dtype)
    for desc in (False, True):
        _report(f"honest {case.id} {_DT[dtype]} {'descending' if desc else 'ascending'}",
                **_ratios(ref, *_honest_fp32(d.y, d.z, d.dout, ref.pre, d.perm, d.inv, case.Lp, SCALE, dtype, desc)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
@pytest.mark.parametrize("case", _SMALL[:3], ids=lambda c: c.id)
def test_bound_flags_planted_errors(case, dtype):
    d = _data(case, dtype)
    Lp = case.Lp
    ref = _gated_ref(d.y, d.z, d.dout, d.perm, d.inv, Lp, SCALE, dtype)
    honest = lambda **kw: _honest_fp32(kw.get("y", d.y), kw.get("z", d.z), d.dout, kw.get("pre", ref.pre), d.perm, d.inv, Lp, kw.get("scale", SCALE), dtype)
    dropped = d.y.clone()
    dropped[:, -1] = 0
    planted = {
        "dropped direction": _ratios(ref, honest(y=dropped)[0]),
        "scale applied twice": _ratios(ref, *honest(scale=SCALE * SCALE)),
        "gate from the neighbouring channel": _ratios(ref, *honest(z=d.z.roll(1, dims=1))),
        "pre taken after the gate": _ratios(ref, None, honest(pre=honest()[0])[1]),
    }
    for name, ratios in planted.items():
        worst = max(v for v in ratios.values() if v is not None)
        print(f"planted {case.id} {_DT[dtype]} {name}: max err / tol {worst:.1f}")
        assert worst > 1, name


def test_merge_sum_is_ascending_fp32():
    """the exact reference of the ungated merge is the ascending fp32 sum: a descending sum differs in the last bit somewhere, so the
    bit comparison of the GPU tests tells the two apart"""
    d = _data(_SMALL[1], torch.float32)
    assert not torch.equal(_merge_sum(d.y, d.inv), _merge_sum(d.y, d.inv, descending=True))


# ---- what the two entries refuse before any launch ---------------------------------------------------------------------------------------
def _descriptor(**kw):
    d = _abi.DirPermDesc()
    d.batch, d.dim, d.seqlen, d.padded_len, d.n_dirs, d.io_dtype = 2, 4, 10, 16, 4, _abi.MXVL_BF16
    d.rows_bs, d.rows_ds, d.stacked_bs, d.stacked_ks, d.stacked_ds = 40, 10, 256, 64, 16
    d.index, d.rows, d.stacked = 0x1000, 0x2000, 0x3000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_dir_perm_refusals_without_gpu():
    """every call below returns before anything is launched, so the pointers are never dereferenced"""
    lib = _abi.load()
    code = {v: k for k, v in _abi.STATUS.items()}
    gate = dict(gate=0x4000, gate_bs=40, gate_ds=10, gate_scale=0.25)
    for entry in (lib.mxvl_dir_gather, lib.mxvl_dir_merge):
        call = lambda **kw: entry(ctypes.byref(_descriptor(**kw)), None)
        assert call(seqlen=MAX_LEN + 1, padded_len=MAX_LEN + 8) == code["MXVL_ERR_UNSUPPORTED"]
        assert call(padded_len=9) == code["MXVL_ERR_SHAPE"]
        assert call(batch=65536) == code["MXVL_ERR_UNSUPPORTED"]
        for k in ("index", "rows", "stacked"):
            assert call(**{k: None}) == code["MXVL_ERR_NULL"], k
        for k in ("batch", "dim", "seqlen", "n_dirs"):
            assert call(**{k: 0}) == code["MXVL_ERR_SHAPE"], k
    call = lambda **kw: lib.mxvl_dir_gather(ctypes.byref(_descriptor(**gate, **kw)), None)
    assert call(pre=None, dgate=0x6000) == code["MXVL_ERR_NULL"], "the gated gather needs pre"
    assert call(pre=0x5000, dgate=None) == code["MXVL_ERR_NULL"], "the gated gather needs dgate"


# ---- GPU: the two entries on guarded buffers -------------------------------------------------------------------------------------------
def _half(case, dtype, data=None, second=False):
    """(B, D, L) as the first / second half of the channels of a (B, 2 D, L) buffer"""
    B, D, L = case.B, case.D, case.L
    return _Buf(2 * B * D * L + 2 * GUARD, GUARD + (D * L if second else 0), (2 * D * L, L, 1), (B, D, L), dtype, DEV, data)


def _channel_major(case, dtype, data=None):
    """(B, D, L) over (D, B, L) storage"""
    B, D, L = case.B, case.D, case.L
    return _Buf(B * D * L + 2 * GUARD, GUARD, (L, B * L, 1), (B, D, L), dtype, DEV, data)


def _stacked(case, dtype, data=None):
    n, off, strides = case.stacked_geom()
    return _Buf(n + 2 * GUARD, GUARD + off, strides, (case.B, case.K, case.D, case.Lp), dtype, DEV, data)


def _index(idx):
    """(K, L) int32 behind guard bands: the bits ride in a float32 _Buf"""
    return _Buf.flat(tuple(idx.shape), torch.float32, DEV, idx.to(torch.int32).view(torch.float32))


def _launch(merge, case, dtype, rows, stacked, index, gate=None, pre=None, dgate=None):
    d = _abi.DirPermDesc()
    d.batch, d.dim, d.seqlen, d.padded_len, d.n_dirs, d.io_dtype = case.B, case.D, case.L, case.Lp, case.K, _abi.dtype_code(dtype)
    d.rows_bs, d.rows_ds = rows.view.stride()[:2]
    d.stacked_bs, d.stacked_ks, d.stacked_ds = stacked.view.stride()[:3]
    d.index, d.rows, d.stacked = _ptr(index), _ptr(rows), _ptr(stacked)
    assert (d.stacked % 16 == 0) == ((GUARD + case.stacked_geom()[1]) * _ESZ[dtype] % 16 == 0)
    d.gate, d.pre, d.dgate, d.gate_scale = _ptr(gate), _ptr(pre), _ptr(dgate), SCALE
    for name, buf in (("gate", gate), ("pre", pre), ("dgate", dgate)):
        if buf is not None:
            bs, ds = buf.view.stride()[:2]
            setattr(d, name + "_bs", bs)
            setattr(d, name + "_ds", ds)
    _abi.launch("mxvl_dir_merge" if merge else "mxvl_dir_gather", d, device=rows.view.device)
    torch.cuda.synchronize()


def _params():
    return [pytest.param(c, dt, id=f"{c.id}-{_DT[dt]}") for c in CASES for dt in DTYPES]


@gpu
@pytest.mark.parametrize("case,dtype", _params())
def test_plain_gather_and_merge_bit_exact(case, dtype):
    d = _data(case, dtype)
    what = f"dir_perm {case.id} {_DT[dtype]} {case.path(dtype)}"
    # gather: x half of xz -> stacked; pre / dgate are handed over without a gate and must stay as they are
    x, X, perm = _half(case, dtype, d.x), _stacked(case, dtype), _index(d.perm)
    pre, dgate = _channel_major(case, dtype), _half(case, dtype, second=True)
    _launch(False, case, dtype, x, X, perm, pre=pre, dgate=dgate)
    _assert_buffers(what + " gather", inputs=[("rows", x), ("index", perm)], outputs=[("stacked", X)], untouched=[("pre", pre), ("dgate", dgate)])
    assert torch.equal(_bits(X.view.cpu()), _bits(_gather_ref(d.x, d.perm, case.Lp))), what + " gather"
    # merge: stacked -> the x half of d(xz)
    y, out, inv = _stacked(case, dtype, d.y), _half(case, dtype), _index(d.inv)
    _launch(True, case, dtype, out, y, inv, pre=pre, dgate=dgate)
    _assert_buffers(what + " merge", inputs=[("stacked", y), ("index", inv)], outputs=[("rows", out)], untouched=[("pre", pre), ("dgate", dgate)])
    assert torch.equal(_bits(out.view.cpu()), _bits(_merge_sum(d.y, d.inv).to(dtype))), what + " merge"


@gpu
@pytest.mark.parametrize("case,dtype", _params())
def test_gated_merge_and_gather(case, dtype):
    d = _data(case, dtype)
    what = f"dir_perm gated {case.id} {_DT[dtype]} {case.path(dtype)}"
    ref = _gated_ref(d.y, d.z, d.dout, d.perm, d.inv, case.Lp, SCALE, dtype)
    y, z, inv, perm = _stacked(case, dtype, d.y), _half(case, dtype, d.z, second=True), _index(d.inv), _index(d.perm)
    # training form: out and pre, both channel-major as the mixer allocates them; a dgate handed over is not the merge's to write
    out, pre, dgate = _channel_major(case, dtype), _channel_major(case, dtype), _half(case, dtype, second=True)
    _launch(True, case, dtype, out, y, inv, gate=z, pre=pre, dgate=dgate)
    _assert_buffers(what + " merge", inputs=[("stacked", y), ("gate", z), ("index", inv)], outputs=[("rows", out), ("pre", pre)],
                    untouched=[("dgate", dgate)])
    assert torch.equal(_bits(pre.view.cpu()), _bits(ref.pre)), what + " pre"
    # inference form: pre == NULL; the same out, and nothing else is written
    out2 = _channel_major(case, dtype)
    _launch(True, case, dtype, out2, y, inv, gate=z, dgate=dgate)
    _assert_buffers(what + " merge without pre", inputs=[("stacked", y), ("gate", z), ("index", inv)], outputs=[("rows", out2)],
                    untouched=[("dgate", dgate)])
    assert torch.equal(_bits(out2.view), _bits(out.view)), what + " out with and without pre"
    # the backward: d(out) -> d(stacked) and dz, the z half of d(xz)
    dout, prein, dy, dz = _half(case, dtype, d.dout), _channel_major(case, dtype, ref.pre), _stacked(case, dtype), _half(case, dtype, second=True)
    _launch(False, case, dtype, dout, dy, perm, gate=z, pre=prein, dgate=dz)
    _assert_buffers(what + " gather", inputs=[("rows", dout), ("gate", z), ("pre", prein), ("index", perm)], outputs=[("stacked", dy), ("dgate", dz)])
    assert not bool(_bits(dy.view[..., case.L:].cpu()).any()), what + " padding is +0"
    _report(what, **_ratios(ref, out.view, dz.view, dy.view))
