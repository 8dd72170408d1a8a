"""csrc/gemm_swiglu.hip (MODE 0 mxvl_gemm_swiglu_fwd, MODE 1 mxvl_gemm_swiglu_bwd, MODE 2 mxvl_gemm_nt) and csrc/gemm_tn.hip (mxvl_gemm_tn,
mxvl_colsum) against float64: every branch of the persistent tile walks at the smallest shape that reaches it, every operand and output
once as a column block of a wider buffer, every tensor a view into a NaN-patterned buffer with guard bands (fp64_bounds._Buf), and
per-element bounds counted from the kernels' operations -- no outlier budget anywhere.

Two input families.  EXACT: operands and bias are small integers times a power of two, |bias| + sum |x||w| < 2^24 in units of the common
scale (asserted on the CPU), so every partial sum in any order is exact in fp32 and the accumulator has ONE possible value: ab, c, the
column sums and mxvl_gemm_tn (atomics included, with and without `accumulate`) must equal the reference bit for bit, the d_h inside MODE 1
too (probe columns a = 0, b = 2 make da = io(d_h b / 2) = d_h itself).  The scale keeps most |a| < 8, so the gate is not only tested in
saturation.  GAUSSIAN (the distributions of test_fused_ops_gpu.py): the accumulator may differ from the float64 sum by
    tol_acc = n 2^-23 (|bias| + sum |x||w|),      n = the additions on the longest path,
one full ulp per addition because the matrix unit's internal rounding is not documented as nearest-even.  n = K for gemm_swiglu (the
accumulator starts at the bias: K products join it); n = K + (K parts of the tile) + 1 for gemm_tn (the chains of the parts, one atomic
add per part, and the c that was there).  K <= 256 keeps tol_acc ~ 2^-15 sum|x||w| well under a dropped term (~ sum|x||w| / K); gemm_tn
cannot run below K = 512 and is held at K = 512 / 576 (n ~ 600: 7e-5 sum|a||b| against 2e-3 for a dropped k-row).

Bounds, per element.
  ab, c      tol = tol_acc + ulp_io(|ref| + tol_acc) / 2: the store's rounding to nearest, i.e. got == io(ref) wherever ref is not within
             tol_acc of a tie (_near_tie).
  h          io(silu(a32) b32) from the UNROUNDED accumulators: s = silu(a) carries |s| _rho(a) + |silu'(a)| ta + ta^2 / 4 (|silu''| <=
             1/2), the product e = |b| es + (|s| + es) tb + U |h| (one fp32 rounding), the store ulp_io(|h| + e) / 2.  A gate taken from
             the rounded ab is off by ~ ulp_io(a) |silu'(a) b| and must fail (it does: CPU test).
  MODE 1     d_h = io(acc); where acc is within tol_acc of a tie (`flip`) the kernel may hold the neighbouring io number.  da = d_h b sg
             (1 + a (1 - sg)), db = d_h a sg with the fp32 terms test_norm_act_gpu.py derives for the SwiGLU backward (|d_h b| 3 rho sg
             (1 + |a (1 - sg)|) and |db| rho), + flip ulp_io(d_h) |d da / d d_h| on those elements only (where tol_acc >= ulp_io(d_h) / 2,
             fp16 d_h near zero, "the neighbour" becomes any io number within tol_acc: tol_acc + ulp), + the store's HALF ulp at |ref| +
             the rest (the sibling allows a whole one; with a whole ulp a d_h used unrounded stays inside, and that planted error has to
             show).  Every element is checked.
  partial    slab row 2 (m / 256) + wm by itself against the float64 column sum of what the kernel WROTE to dab over that slab's 128
             rows: a lane adds 4 values, the row_shr / row_bcast tree 5 more: 128 U sum|dab| covers any order over the 128 rows.  Slab rows
             wholly beyond M are written and zero; with partial == NULL nothing is written.
  gemm_tn    tol_acc alone (fp32 output: the roundings of its additions are the n counted ones).
  colsum     partial row rg against the float64 sum of rows rg, rg + R, ...: ceil(rows / R) U sum|x| (one chain per lane).

CPU tests (no `gpu` mark) hold all of this in place: the restated dispatch must find every path in the case lists and agree with the
library's exported counts; the references equal torch's float64 autograd; fp32 emulations of the summation orders (16-term MFMA blocks
chained over K, and every term added one by one; for gemm_tn the per-unit partials of the restated K ranges added in several arrival
orders) stay under the bounds on both families; twelve planted errors exceed them.

Measured on an MI355X, largest err / tol as bf16 / fp16 (the one-by-one fp32 emulation in brackets).  Gaussian family: gemm_swiglu_fwd ab
0.997 / 0.977 (0.986 / 0.927), h 0.994 / 0.963 (0.980 / 0.861); gemm_nt c 0.995 / 0.965 (0.978 / 0.928); gemm_swiglu_bwd dab 1.000 /
0.998 (0.999 / 0.996), partial 0.007 / 0.008 (0.003 / 0.004); gemm_tn c 0.001 / 0.001 (below 0.001); colsum 0.078 / 0.058 (0.05).  The
16-bit outputs sit just under 1 because the store's half ulp is nearly the whole bound and some element always lands next to a tie;
gemm_tn and the column sums are far below their any-order worst case, yet a dropped k-row or row is 10^3 times over it.  Exact family:
every bit-for-bit assertion held on every path; ab, c, h and dab read 1.000 there (an accumulator exactly on a tie moves by exactly the
half ulp that is the whole bound when tol_acc = 0), gemm_tn and colsum 0.  No kernel needed a change."""
import ctypes
import functools
import types
import zlib

import pytest
import torch

from fp64_bounds import FLOOR, GUARD, U, _assert_buffers, _Buf, _near_tie, _ptr, _ratio, _report, _rho, _rnd, _ulp
from medical_image_analysis_amd import _abi

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IO = (BF16, F16)
_DT = {F32: "fp32", BF16: "bf16", F16: "fp16"}
gpu = pytest.mark.gpu
NS = types.SimpleNamespace
ERR = {name: code for code, name in _abi.STATUS.items()}
_cdiv = lambda a, b: -(-a // b)


# ---- 1. the dispatch restated ------------------------------------------------------------------------------------------------------------
GS_BM, GS_BN, GS_BK, GS_GROUP_M = 256, 128, 64, 4                 # gemm_swiglu.hip:51
TN_BM, TN_BN, TN_BK, TN_EPI_STEPS = 256, 256, 32, 20              # gemm_tn.hip:54, :309


def _gs_geometry(mode, M, K, H):
    """gemm_swiglu.hip: the entries' ntm / ntn / ntm_x (:497, :516, :536), launch_gemm_swiglu's grid (:478-479) and the kernel's tile walk
    (:117-132 and :305): for every workgroup the tiles it accumulates, the holes it skips before its first tile and between tiles"""
    bn = GS_BN if mode == 0 else 2 * GS_BN
    ntm, ntn = _cdiv(M, GS_BM), _cdiv(H, bn)
    ntm_x = _cdiv(ntm, 8)
    grid = min(8 * ntm_x * ntn, 256)
    lstride, per_group, nlocal, nk = grid >> 3, GS_GROUP_M * ntn, ntm_x * ntn, K // GS_BK

    def locate(loc, xcd):
        grp, li = divmod(loc, per_group)
        gsz = min(ntm_x - grp * GS_GROUP_M, GS_GROUP_M)
        mt = (grp * GS_GROUP_M + li % gsz) * 8 + xcd
        return mt, li // gsz, mt < ntm

    walks, holes_start, holes_loop = [], 0, 0
    for wg in range(grid):
        xcd, local, tiles = wg & 7, wg >> 3, []
        while local < nlocal:
            mt, nt, ok = locate(local, xcd)
            if ok:
                tiles.append((mt, nt))
            elif tiles:
                holes_loop += 1
            else:
                holes_start += 1
            local += lstride
        walks.append(tiles)
    assert sorted(t for w in walks for t in w) == [(m, n) for m in range(ntm) for n in range(ntn)], "every tile exactly once"
    return NS(ntm=ntm, ntn=ntn, ntm_x=ntm_x, grid=grid, nk=nk, walks=walks, per_wg=max(len(w) for w in walks),
              idle=sum(not w for w in walks), holes_start=holes_start, holes_loop=holes_loop,
              last_group=ntm_x - GS_GROUP_M * ((ntm_x - 1) // GS_GROUP_M),
              buf1_start=any((i * nk) & 1 for w in walks for i in range(len(w))),       # stage buffer = (K steps done so far) & 1 (:286)
              slabs=2 * ntm, slabs_beyond=2 * ntm - _cdiv(M, 128))


def _gs_partials(M):
    """mxvl_gemm_swiglu_bwd_partials (:523)"""
    return 2 * _cdiv(M, GS_BM) if M > 0 else 0


def _tn_geometry(M, N, K, q):
    """gemm_tn.hip with slices_per_xcd = q forced (tn_slices_per_xcd :311-312): the tail split of mxvl_gemm_tn (:343-358) and the kernel's
    locate (:90-110) -> every (xcd, unit) with its tile and K-step range"""
    f = abs(q)
    ntm, ntn, nk = _cdiv(M, TN_BM), _cdiv(N, TN_BN), K // TN_BK
    assert 1 <= f <= 8 and nk // (8 * f) >= 1, "the forced count is taken as it is"
    ntiles, slices, n_fast = ntm * ntn, 8 * f, ntn <= ntm
    nunits, ksl = f * ntiles, nk // (8 * f)
    ntail = nunits % 32
    nfull, tailf, best = nunits - ntail, 1, None
    for t in range(1, 5):
        if not (ntail > 0 and ksl // t >= 4):
            break
        cost = ((ntail * t + 31) // 32) * (_cdiv(ksl, t) + TN_EPI_STEPS)
        if best is None or cost < best:
            best, tailf = cost, t
    if q < 0:
        tailf = 1
    units = []
    for xcd in range(8):
        for u0 in range(nfull + ntail * tailf):
            u, part = u0, 0
            if u >= nfull:
                part, v = divmod(u - nfull, ntail)
                u = nfull + v
            sl, tile = xcd + 8 * (u // ntiles), u % ntiles
            mt, nt = divmod(tile, ntn) if n_fast else (tile % ntm, tile // ntm)
            k0, k1 = sl * nk // slices, (sl + 1) * nk // slices
            if u >= nfull:
                ln = k1 - k0
                k0, k1 = k0 + part * ln // tailf, k0 + (part + 1) * ln // tailf
            units.append(NS(xcd=xcd, wg=u0 % 32, mt=mt, nt=nt, k0=k0, k1=k1, tail=u >= nfull))
    parts = torch.zeros(ntm, ntn, dtype=torch.int64)
    for mt in range(ntm):
        for nt in range(ntn):
            rng = sorted((u.k0, u.k1) for u in units if (u.mt, u.nt) == (mt, nt))
            assert rng[0][0] == 0 and rng[-1][1] == nk and all(a[1] == b[0] for a, b in zip(rng, rng[1:])) and all(a < b for a, b in rng)
            parts[mt, nt] = len(rng)
    lens = {u.k1 - u.k0 for u in units}
    return NS(ntm=ntm, ntn=ntn, nk=nk, slices=slices, n_fast=n_fast, nfull=nfull, ntail=ntail, tailf=tailf, units=units, parts=parts,
              lens=lens, first_tiles=[(u.mt, u.nt) for u in units if u.xcd == 0][:3])


def _cs_geometry(rows, C):
    """mxvl_colsum_partials (:371-377) and mxvl_colsum's grid (:385-387); per row group: trips of the 4-rows-in-flight loop, remainder"""
    tiles = _cdiv(C, 512)
    R = max(1, min(2048 // tiles, _cdiv(rows, 16)))
    per = [_cdiv(rows - rg, R) for rg in range(R)]
    return NS(R=R, tiles=tiles, grid=_cdiv(tiles * R, 4), main=max(n // 4 for n in per), rem={n % 4 for n in per})


# ---- 2. inputs -----------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("exact", "gauss")
X_SCALE, W_SCALE, B_SCALE = 2.0 ** -5, 2.0 ** -5, 2.0 ** -3         # the exact family: integers in [-15, 15] (bias [-8, 8]) times these


def _gen(*what):
    return torch.Generator().manual_seed(zlib.crc32(" ".join(str(w) for w in what).encode()))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=8)
def _gs_inputs(mode, M, K, H, io, family, bias):
    """CPU tensors as the kernel reads them, float64 accumulators, sum of magnitudes and tol_acc.  mode 0: w (2H, K), bias (2H);
    mode 1: x = dy, w = w3t (H, K), ab (M, 2H) with probe columns; mode 2: w = b (N = H, K), bias (N)"""
    g = _gen("gs", mode, M, K, H, _DT[io], family, bias)
    wr = 2 * H if mode == 0 else H
    if family == "exact":
        x, w, b = X_SCALE * _ints(g, -15, 15, M, K), W_SCALE * _ints(g, -15, 15, wr, K), B_SCALE * _ints(g, -8, 8, wr)
    elif mode == 0:
        x, w, b = torch.randn(M, K, generator=g), K ** -0.5 * torch.randn(wr, K, generator=g), 0.5 * torch.randn(wr, generator=g)
    else:
        x, w, b = 0.5 * torch.randn(M, K, generator=g), K ** -0.5 * torch.randn(wr, K, generator=g), 0.3 * torch.randn(wr, generator=g)
    x, w = x.to(io), w.to(io)
    b = None if bias is None or mode == 1 else b.to(F32 if bias == "f32" else io)
    acc = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    if b is not None:
        acc, mag = acc + b.double(), mag + b.double().abs()
    d = NS(mode=mode, M=M, K=K, H=H, io=io, family=family, x=x, w=w, bias=b, acc=acc, mag=mag,
           tol_acc=torch.zeros_like(mag) if family == "exact" else K * 2.0 ** -23 * mag, ab=None)
    if mode == 1:
        ab = 2.0 * torch.randn(M, 2 * H, generator=g)
        if family == "exact":                                     # probe columns: sigmoid(0) = 1 / 2, so da = io(d_h 2 / 2) = d_h
            ab[:, 0:H:3], ab[:, H::3] = 0.0, 2.0
        d.ab = ab.to(io)
    return d


def _exact_headroom(d):
    """the exact family's promise: every operand an integer in its unit, |bias| + sum |x||w| below 2^24 units of the common scale"""
    unit = X_SCALE * W_SCALE
    whole = lambda t, s: bool(((t.double() / s) == (t.double() / s).round()).all())
    assert whole(d.x, X_SCALE) and whole(d.w, W_SCALE) and (d.bias is None or whole(d.bias, B_SCALE)) and B_SCALE % unit == 0
    return float(d.mag.max()) / unit


@functools.lru_cache(maxsize=4)
def _tn_inputs(K, M, N, io, family):
    g = _gen("tn", K, M, N, _DT[io], family)
    if family == "exact":
        a, b, c0 = _ints(g, -3, 3, K, M), 0.5 * _ints(g, -3, 3, K, N), 0.5 * _ints(g, -64, 64, M, N)
    else:
        a, b, c0 = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g), 8.0 * torch.randn(M, N, generator=g)
    a, b = a.to(io), b.to(io)
    return NS(K=K, M=M, N=N, io=io, family=family, a=a, b=b, c0=c0, prod=a.double().t() @ b.double(),
              mag=a.double().abs().t() @ b.double().abs())


def _cs_inputs(rows, C, io, family):
    g = _gen("cs", rows, C, _DT[io], family)
    x = 0.25 * _ints(g, -4, 4, rows, C) if family == "exact" else torch.randn(rows, C, generator=g)
    return x.to(io)


# ---- 3. references and bounds ----------------------------------------------------------------------------------------------------------
def _io_tol(ref, tol_acc, io):
    """an fp32 value within tol_acc of ref, rounded to nearest in io"""
    return (tol_acc + 0.5 * _ulp(ref.abs() + tol_acc, io)).clamp_min(FLOOR)


def _gs0_ref(d):
    """-> float64 ab (M, 2H), h (M, H) and their tolerances"""
    H, io = d.H, d.io
    a, b, ta, tb = d.acc[:, :H], d.acc[:, H:], d.tol_acc[:, :H], d.tol_acc[:, H:]
    sg = torch.sigmoid(a)
    s, ds = a * sg, sg * (1 + a * (1 - sg))
    es = s.abs() * _rho(a) + ds.abs() * ta + 0.25 * ta * ta
    h = s * b
    e = b.abs() * es + (s.abs() + es) * tb + U * h.abs() + b.abs() * FLOOR
    return NS(ab=d.acc, tab=_io_tol(d.acc, d.tol_acc, io), h=h, th=(e + 0.5 * _ulp(h.abs() + e, io)).clamp_min(FLOOR))


def _gs0_ratios(d, ab, h):
    r = _gs0_ref(d)
    out = dict(h=_ratio(h, r.h, r.th), ab=None if ab is None else _ratio(ab, r.ab, r.tab))
    if d.family == "exact" and ab is not None:
        assert torch.equal(ab.cpu(), d.acc.to(d.io)), "exact family: ab is not io(accumulator) bit for bit"
    return out


def _nt_ratios(d, c):
    if d.family == "exact":
        assert torch.equal(c.cpu(), d.acc.to(d.io)), "exact family: c is not io(accumulator) bit for bit"
    return dict(c=_ratio(c, d.acc, _io_tol(d.acc, d.tol_acc, d.io)))


def _gs1_ref(d):
    """MODE 1 -> d_h, dab (M, 2H) in float64 and the tolerance"""
    H, io = d.H, d.io
    a, b = d.ab[:, :H].double(), d.ab[:, H:].double()
    dh = _rnd(d.acc, io)
    # how far the kernel's d_h can be from io(acc): nowhere off a tie; the neighbour next to one; and where tol_acc is no longer small
    # against the spacing (fp16 d_h near zero: tol_acc scales with sum|dy||w|, the ulp with |d_h|) any io number within tol_acc
    near, ulp = _near_tie(d.acc, d.tol_acc, io) & (d.tol_acc > 0), _ulp(dh, io)
    flip = near.double() * torch.where(d.tol_acc < 0.5 * ulp, ulp, d.tol_acc + _ulp(d.acc.abs() + d.tol_acc, io))
    sg, rho = torch.sigmoid(a), _rho(a)
    ka, kb = b * sg * (1 + a * (1 - sg)), a * sg                  # d da / d d_h, d db / d d_h
    da, db = dh * ka, dh * kb
    ea = (dh * b).abs() * 3 * rho * sg * (1 + (a * (1 - sg)).abs()) + flip * ka.abs()
    eb = db.abs() * rho + flip * kb.abs()
    dab, e = torch.cat([da, db], 1), torch.cat([ea, eb], 1)
    return NS(dh=dh, dab=dab, tdab=(e + 0.5 * _ulp(dab.abs() + e, io)).clamp_min(FLOOR))


def _slab_sums(dab, M):
    """float64 column sums of dab (as written) and of |dab| over the 128-row slabs, one row per slab of 2 ceil(M / 256)"""
    w = dab.double().cpu()
    pad = torch.zeros(_gs_partials(M) * 128 - M, w.shape[1], dtype=torch.float64)
    w = torch.cat([w, pad]).view(-1, 128, w.shape[1])
    return w.sum(1), w.abs().sum(1)


def _gs1_ratios(d, dab, partial):
    r = _gs1_ref(d)
    out = dict(dab=_ratio(dab, r.dab, r.tdab), partial=None)
    if d.family == "exact":                                       # the probe columns show d_h itself
        assert torch.equal(dab.cpu()[:, 0:d.H:3], r.dh.to(d.io)[:, 0::3]), "exact family: d_h is not io(accumulator) bit for bit"
    if partial is not None:
        s, sabs = _slab_sums(dab, d.M)
        p = partial.double().cpu()
        assert p.shape == s.shape
        beyond = p[_cdiv(d.M, 128):]
        assert bool((beyond == 0).all()), "a slab row wholly beyond M is not zero"
        out["partial"] = _ratio(p, s, (128 * U * sabs).clamp_min(FLOOR))
    return out


def _tn_tol(d, geo, accumulate):
    n = d.K + geo.parts.repeat_interleave(TN_BM, 0).repeat_interleave(TN_BN, 1)[:d.M, :d.N].double() + 1
    mag = d.mag + (d.c0.double().abs() if accumulate else 0.0)
    return torch.zeros_like(mag).clamp_min(FLOOR) if d.family == "exact" else (n * 2.0 ** -23 * mag).clamp_min(FLOOR)


def _tn_ratios(d, geo, accumulate, c):
    ref = d.prod + (d.c0.double() if accumulate else 0.0)
    if d.family == "exact":
        assert torch.equal(c.cpu(), ref.float()), "exact family: c is not the exact sum bit for bit"
    return dict(c=_ratio(c, ref, _tn_tol(d, geo, accumulate)))


def _cs_ratios(x, partial, R, family):
    rows, p, out = x.shape[0], partial.double().cpu(), []
    assert p.shape[0] == R
    for rg in range(R):
        grp = x[rg::R].double()
        if family == "exact":
            assert torch.equal(p[rg], grp.sum(0)), "exact family: a column sum is not exact"
        out.append(_ratio(p[rg], grp.sum(0), (_cdiv(rows, R) * U * grp.abs().sum(0)).clamp_min(FLOOR)))
    return dict(partial=max(out))


# ---- 4. the case lists -------------------------------------------------------------------------------------------------------------------
KS = (64, 128, 192)
BIAS = ("f32", "io", None)
GS0_M, GS0_H = (1, 33, 129, 257, 300), (1, 7, 8, 9, 127, 129, 136)
GS0_BIG = [(2100, 192, 2179), (8200, 64, 800)]
GS1_M, GS1_H = (1, 33, 100, 129, 257, 300), (8, 120, 128, 136, 256, 264)
GS1_BIG = [(2100, 192, 4104)]
TN_CASES = [(512, 256, 256, 2), (512, 8, 264, 2), (576, 264, 8, 1), (576, 40, 520, 2), (4096, 256, 136, 1), (2048, 1032, 1544, 1),
            (2048, 1544, 1032, 1), (2048, 1032, 1544, -1)]       # (K, M, N, forced slices per XCD)
TN_GAUSS = [(512, 256, 256, 2), (512, 8, 264, 2), (576, 264, 8, 1), (576, 40, 520, 2)]
CS_ROWS, CS_C = (1, 3, 15, 16, 17, 67, 1000), (8, 512, 520)


def _k_of(i, j):
    return KS[(i + j) % 3]


def _gs0_cases(H):
    """(M, K, bias kind) of the small grid for one H: K and the bias kind rotate so that every H sees all three of each"""
    j = GS0_H.index(H)
    return [(M, _k_of(i, j), BIAS[(i + 2 * j) % 3]) for i, M in enumerate(GS0_M)]


def _gs1_cases(H):
    j = GS1_H.index(H)
    return [(M, _k_of(i, j), BIAS[(i + 2 * j) % 3]) for i, M in enumerate(GS1_M)]


# ---- CPU: the case lists reach what they say they reach ------------------------------------------------------------------------------
def test_cases_cover_every_path():
    # gemm_swiglu MODE 0
    small = [_gs_geometry(0, M, K, H) for H in GS0_H for M, K, _ in _gs0_cases(H)]
    assert all(g.per_wg == 1 and g.grid == 8 * g.ntn and g.idle == 8 * g.ntn - g.ntm * g.ntn for g in small)
    assert {g.nk for g in small} == {1, 2, 3} and {g.ntn for g in small} == {1, 2} and {g.ntm for g in small} == {1, 2}
    assert {(K, b) for H in GS0_H for _, K, b in _gs0_cases(H)} == {(K, b) for K in KS for b in BIAS}
    for H in GS0_H:
        assert {K for _, K, _ in _gs0_cases(H)} == set(KS) and {b for _, _, b in _gs0_cases(H)} == set(BIAS)
    assert {H % 8 for H in GS0_H} >= {0, 1, 7} and any(H % 2 and H > 128 for H in GS0_H), "16-byte stores, the element tail, odd cbase"
    a = _gs_geometry(0, *GS0_BIG[0])
    assert (a.ntm, a.ntn, a.ntm_x, a.grid) == (9, 18, 2, 256) and 8 * a.ntm_x * a.ntn == 288 and a.per_wg == 2
    assert a.holes_start == 2 * 7 * 9 and a.nk % 2 == 1 and a.buf1_start and a.last_group == 2 and 2179 % 128 == 3 and 2179 % 2 == 1
    b = _gs_geometry(0, *GS0_BIG[1])
    assert (b.ntm, b.ntn, b.ntm_x, b.grid) == (33, 7, 5, 256) and b.last_group == 1 and b.nk == 1 and b.per_wg == 2
    assert b.holes_loop == 7 * 3 and b.holes_start == 7 * 4 == b.idle, "XCDs 1..7: locals 28..31 start beyond the last token tile, and so does the second tile of locals 0..2"
    assert b.buf1_start, "nk == 1: every second tile of a workgroup starts in buffer 1"
    # MODE 1 and 2
    for mode in (1, 2):
        small = [_gs_geometry(mode, M, K, H) for H in GS1_H for M, K, _ in _gs1_cases(H)]
        assert all(g.per_wg == 1 for g in small) and {g.nk for g in small} == {1, 2, 3} and {g.ntn for g in small} == {1, 2}
        c = _gs_geometry(mode, *GS1_BIG[0])
        assert (c.ntm, c.ntn, c.grid, c.per_wg) == (9, 17, 256, 2) and c.holes_start > 0 and c.buf1_start and 4104 % 256 == 8
    assert {_gs_geometry(1, M, 64, 8).slabs_beyond for M in GS1_M} == {0, 1} and _gs_geometry(1, 300, 64, 8).slabs == 4
    assert [_gs_geometry(1, M, 64, 8).slabs_beyond for M in (100, 300, 129, 257)] == [1, 1, 0, 1]
    assert any(H <= 128 for H in GS1_H) and any(H >= 256 for H in GS1_H), "MODE 2's second-half bias clamp (col + 128 < H) taken and not taken"
    for H in GS1_H:
        assert {K for _, K, _ in _gs1_cases(H)} == set(KS) and {b for _, _, b in _gs1_cases(H)} == set(BIAS)
    # gemm_tn
    geo = {c: _tn_geometry(c[1], c[2], c[0], c[3]) for c in TN_CASES}
    g = geo[(512, 256, 256, 2)]
    assert g.lens == {1} and g.slices == 16, "units of one K step"
    assert geo[(576, 264, 8, 1)].lens == {2, 3} and geo[(576, 40, 520, 2)].lens == {1, 2}, "uneven slices"
    g = geo[(4096, 256, 136, 1)]
    assert (g.nfull, g.ntail, g.tailf) == (0, 1, 4) and int(g.parts.max()) == 32
    g, t, n = geo[(2048, 1032, 1544, 1)], geo[(2048, 1544, 1032, 1)], geo[(2048, 1032, 1544, -1)]
    assert (g.nfull, g.ntail, g.tailf, g.n_fast) == (32, 3, 2, False) and (t.nfull, t.ntail, t.tailf, t.n_fast) == (32, 3, 2, True)
    assert g.first_tiles == [(0, 0), (1, 0), (2, 0)] and t.first_tiles == [(0, 0), (0, 1), (0, 2)], "both tile orders"
    assert (n.tailf, n.ntail) == (1, 3) and sorted(set(g.parts.flatten().tolist())) == [8, 16]
    assert any(8 in (c[1], c[2]) for c in TN_CASES) and all(c in TN_CASES and c[0] <= 576 for c in TN_GAUSS)
    # colsum
    cs = {(r, C): _cs_geometry(r, C) for r in CS_ROWS for C in CS_C}
    assert [cs[(r, 8)].R for r in CS_ROWS] == [1, 1, 1, 1, 2, 5, 63] and cs[(1000, 520)].tiles == 2 and cs[(1000, 520)].R == 63
    assert cs[(1, 8)].main == 0 and cs[(3, 8)].rem == {3} and cs[(15, 8)].main == 3 and cs[(16, 8)].rem == {0}
    assert cs[(67, 8)].main == 3 and cs[(67, 8)].rem == {1, 2} and cs[(1000, 520)].main >= 3 and cs[(1000, 520)].rem == {0, 3}
    assert cs[(1000, 520)].grid == 32 and cs[(1, 520)].grid == 1, "a workgroup with idle waves"


def test_restated_counts_match_the_library():
    lib = _abi.load()
    for M in (0, 1, 100, 128, 129, 256, 257, 300, 2100, 8200):
        assert lib.mxvl_gemm_swiglu_bwd_partials(M) == _gs_partials(M)
        assert M == 0 or _gs_geometry(1, M, 64, 8).slabs == _gs_partials(M)
    for rows in CS_ROWS + (4096, 65280):
        for C in CS_C + (2752,):
            assert lib.mxvl_colsum_partials(rows, C) == _cs_geometry(rows, C).R
    assert lib.mxvl_colsum_partials(16, 7) == 0 and lib.mxvl_colsum_partials(0, 8) == 0


def test_exact_family_is_exact_in_fp32():
    worst = 0.0
    for mode, shapes in ((0, GS0_BIG + [(300, 192, 136)]), (1, GS1_BIG), (2, GS1_BIG + [(300, 192, 264)])):
        for M, K, H in shapes:
            worst = max(worst, _exact_headroom(_gs_inputs(mode, min(M, 300), K, H, BF16, "exact", "f32")))
    assert worst < 2 ** 24 and 8 * 128 + 192 * 15 * 15 < 2 ** 24, "|bias| + K max|x||w| in units of 2^-10"
    for K, M, N in ((4096, 64, 64), (2048, 64, 64)):
        d = _tn_inputs(K, M, N, F16, "exact")
        assert float((d.mag + d.c0.double().abs()).max()) / 0.5 < 2 ** 24 and bool(((d.prod * 2) == (d.prod * 2).round()).all())
    d = _gs_inputs(0, 300, 192, 136, BF16, "exact", "f32")
    assert float((d.acc[:, :136].abs() < 8).double().mean()) > 0.9, "most gates outside saturation"
    assert bool((d.acc.to(BF16).double() != d.acc).any()), "the io rounding is exercised"


# ---- CPU: the references against torch's float64 autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("io", IO, ids=_DT.get)
def test_references_equal_torch_float64(io):
    d = _gs_inputs(0, 33, 64, 9, io, "gauss", "f32")
    x, w, b = d.x.double().requires_grad_(True), d.w.double(), d.bias.double()
    ab = torch.nn.functional.linear(x, w, b)
    h = torch.nn.functional.silu(ab[:, :9]) * ab[:, 9:]
    r = _gs0_ref(d)
    close = lambda got, want: float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert close(r.ab, ab.detach()) and close(r.h, h.detach())
    # MODE 1: with dy standing for the gradient at w3's output, autograd through silu(a) b @ w3t with d_h held at its io rounding
    d = _gs_inputs(1, 33, 64, 8, io, "gauss", None)
    r = _gs1_ref(d)
    t = d.ab.double().requires_grad_(True)
    (torch.nn.functional.silu(t[:, :8]) * t[:, 8:]).backward(r.dh)
    assert close(r.dab, t.grad)
    assert close(d.acc, d.x.double() @ d.w.double().t()) and close(r.dh, d.acc.to(io).double())


# ---- CPU: fp32 emulations of the summation orders ----------------------------------------------------------------------------------------
def _emu_acc(x, w, bias, order):
    """the accumulator in fp32: starts at the bias, then 16-term MFMA blocks (each block's dot product rounded once) chained over K
    (`block`), or every product added by itself (`seq`: the most roundings any internal order of the matrix unit can make)"""
    acc = (bias.float() if bias is not None else torch.zeros(w.shape[0])).expand(x.shape[0], w.shape[0]).clone()
    step = 16 if order == "block" else 1
    for k in range(0, x.shape[1], step):
        acc = acc + (x[:, k:k + step].double() @ w[:, k:k + step].double().t()).float()
    return acc


def _emu_gs(d, order):
    acc, H, io = _emu_acc(d.x, d.w, d.bias, order), d.H, d.io
    if d.mode == 0:
        a, b = acc[:, :H], acc[:, H:]
        return acc.to(io), (a * torch.sigmoid(a) * b).to(io)
    if d.mode == 2:
        return acc.to(io)
    gv, a, b = acc.to(io).float(), d.ab[:, :H].float(), d.ab[:, H:].float()
    sg = torch.sigmoid(a)
    dab = torch.cat([gv * b * (sg * (1.0 + a * (1.0 - sg))), gv * (a * sg)], 1).to(io)
    return dab, _emu_partial(dab, d.M)


def _emu_partial(dab, M):
    """fp32 slab sums: 4 token tiles added per lane, then the 32 lanes"""
    v = torch.cat([dab.float(), torch.zeros(_gs_partials(M) * 128 - M, dab.shape[1])]).view(-1, 4, 32, dab.shape[1])
    lane = ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]
    s = torch.zeros_like(lane[:, 0])
    for j in range(32):
        s = s + lane[:, j]
    return s


def _emu_tn(d, geo, accumulate, order):
    """per unit: 16-term blocks chained over its K steps from zero; then the units of a tile added into c in `order`"""
    c = d.c0.clone() if accumulate else torch.zeros(d.M, d.N)
    units = sorted(geo.units, key=lambda u: (u.k0, u.xcd))
    if order == "reversed":
        units = units[::-1]
    elif order != "natural":
        units = [units[i] for i in torch.randperm(len(units), generator=_gen("order", order)).tolist()]
    for u in units:
        rm, rn = slice(u.mt * TN_BM, min((u.mt + 1) * TN_BM, d.M)), slice(u.nt * TN_BN, min((u.nt + 1) * TN_BN, d.N))
        acc = torch.zeros(rm.stop - rm.start, rn.stop - rn.start)
        for k in range(u.k0 * TN_BK, u.k1 * TN_BK, 16):
            acc = acc + (d.a[k:k + 16, rm].double().t() @ d.b[k:k + 16, rn].double()).float()
        c[rm, rn] = c[rm, rn] + acc
    return c


@pytest.mark.parametrize("io", IO, ids=_DT.get)
@pytest.mark.parametrize("family", FAMILIES)
def test_emulated_summation_orders_within_bound(io, family):
    for order in ("block", "seq"):
        for M, K, H, bias in ((40, 192, 24, "f32"), (33, 64, 9, "io"), (5, 128, 136, None)):
            d = _gs_inputs(0, M, K, H, io, family, bias)
            _report(f"emulated fwd {order} {M}x{K}x{H} {_DT[io]} {family}", **_gs0_ratios(d, *_emu_gs(d, order)))
        for M, K, H in ((300, 192, 24), (33, 64, 8)):
            d = _gs_inputs(1, M, K, H, io, family, None)
            _report(f"emulated bwd {order} {M}x{K}x{H} {_DT[io]} {family}", **_gs1_ratios(d, *_emu_gs(d, order)))
            d = _gs_inputs(2, M, K, H, io, family, "f32")
            _report(f"emulated nt {order} {M}x{K}x{H} {_DT[io]} {family}", **_nt_ratios(d, _emu_gs(d, order)))
    for K, M, N, q in ((512, 24, 16, 2), (576, 264, 8, 1), (576, 16, 24, 2)):
        d, geo = _tn_inputs(K, M, N, io, family), _tn_geometry(M, N, K, q)
        for accumulate in (0, 1):
            for order in ("natural", "reversed", "shuffle1", "shuffle2"):
                _report(f"emulated tn {K}x{M}x{N} q{q} acc{accumulate} {order} {_DT[io]} {family}",
                        **_tn_ratios(d, geo, accumulate, _emu_tn(d, geo, accumulate, order)))
    for rows, C in ((67, 8), (1000, 16)):
        x, R = _cs_inputs(rows, C, io, family), _cs_geometry(rows, C).R
        p = torch.stack([functools.reduce(lambda s, r: s + x[r].float(), range(rg, rows, R), torch.zeros(C)) for rg in range(R)])
        _report(f"emulated colsum {rows}x{C} {_DT[io]} {family}", **_cs_ratios(x, p, R, family))


# ---- CPU: the bounds notice planted errors ---------------------------------------------------------------------------------------------
def _trunc(v, io):
    """float64 -> io by truncation"""
    ulp = _ulp(v, io)
    return (torch.sign(v) * torch.floor(v.abs() / ulp) * ulp).to(io)


def _planted_fwd(kind, d):
    """-> (ab, h) as a kernel with one error would write them"""
    H, io, K = d.H, d.io, d.K
    x, w = d.x.double(), d.w.double()
    bias = d.bias.double()
    step = lambda k: x[:, 64 * k:64 * k + 64] @ w[:, 64 * k:64 * k + 64].t()
    acc = d.acc.clone()
    if kind == "one K step skipped":
        acc = acc - step(1)
    elif kind == "stage buffers swapped for one step":           # step 1 multiplies the buffer that still holds step 0
        acc = acc - step(1) + step(0)
    elif kind == "w1 and w2 halves exchanged":
        acc = torch.cat([acc[:, H:], acc[:, :H]], 1)
    elif kind == "weight row transposed with its neighbour":
        acc[:, [3, 4]] = acc[:, [4, 3]]
    a, b = acc[:, :H], acc[:, H:]
    ab, h = acc.to(io), (a * torch.sigmoid(a) * b).to(io)
    if kind == "bias added after the rounding":
        ab = ((acc - bias).to(io).double() + bias).to(io)
    elif kind == "truncation":
        ab, h = _trunc(acc, io), _trunc(a * torch.sigmoid(a) * b, io)
    elif kind == "h gated from the rounded ab":
        ar, br = ab[:, :H].double(), ab[:, H:].double()
        h = (ar * torch.sigmoid(ar) * br).to(io)
    elif kind == "last 8 columns of a ragged tile dropped":
        h[:, H - 8:] = float("nan")
        ab[:, 2 * H - 8:] = float("nan")
    return ab, h


FWD_PLANTS = {"one K step skipped": ("ab", "h"), "stage buffers swapped for one step": ("ab", "h"), "w1 and w2 halves exchanged": ("ab", "h"),
              "weight row transposed with its neighbour": ("ab", "h"), "bias added after the rounding": ("ab",), "truncation": ("ab", "h"),
              "h gated from the rounded ab": ("h",), "last 8 columns of a ragged tile dropped": ("ab", "h")}
INDEX_PLANTS = ("one K step skipped", "stage buffers swapped for one step", "w1 and w2 halves exchanged", "weight row transposed with its neighbour")


@pytest.mark.parametrize("io", IO, ids=_DT.get)
def test_bounds_flag_planted_errors(io):
    d = _gs_inputs(0, 300, 192, 136, io, "gauss", "f32")
    _report(f"unplanted fwd {_DT[io]}", **_gs0_ratios(d, *_planted_fwd("none", d)))
    for kind, outs in FWD_PLANTS.items():
        r = _gs0_ratios(d, *_planted_fwd(kind, d))
        print(f"planted fwd {_DT[io]} {kind}: " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        assert all(r[o] > 1 for o in outs), kind
        assert all(r[o] <= 1 for o in r if o not in outs), kind
    e = _gs_inputs(0, 300, 192, 136, io, "exact", "f32")
    _gs0_ratios(e, *_planted_fwd("none", e))
    for kind in INDEX_PLANTS:                                      # at zero tolerance: not one element may move
        with pytest.raises(AssertionError, match="bit for bit"):
            _gs0_ratios(e, *_planted_fwd(kind, e))
    # MODE 1
    d = _gs_inputs(1, 300, 192, 136, io, "gauss", None)
    r = _gs1_ref(d)
    H = d.H
    a, b = d.ab[:, :H].double(), d.ab[:, H:].double()
    sg = torch.sigmoid(a)
    good = r.dab.to(io)
    _report(f"unplanted bwd {_DT[io]}", **_gs1_ratios(d, good, _emu_partial(good, d.M)))
    unr = torch.cat([d.acc * b * sg * (1 + a * (1 - sg)), d.acc * a * sg], 1).to(io)
    p = _emu_partial(good, d.M)
    planted = {"d_h used unrounded": _gs1_ratios(d, unr, None)["dab"],
               "column sum in the neighbouring slab row": _gs1_ratios(d, good, p[[1, 0, 2, 3]])["partial"]}
    if io == BF16:                                                # in fp16 the roundings of 128 rows add up to about the bound itself
        planted["sums of the unrounded gradients"] = _gs1_ratios(d, good, _slab_sums(r.dab, d.M)[0].float())["partial"]
    with pytest.raises(AssertionError, match="beyond M"):
        _gs1_ratios(d, good, p[[0, 1, 3, 2]])
    e = _gs_inputs(1, 300, 192, 136, io, "exact", None)
    re_ = _gs1_ref(e)
    _gs1_ratios(e, re_.dab.to(io), None)
    if io == BF16:                                                # fp16 holds every accumulator of the exact family: nothing to round
        ae, be = e.ab[:, :H].double(), e.ab[:, H:].double()
        se = torch.sigmoid(ae)
        with pytest.raises(AssertionError, match="d_h"):
            _gs1_ratios(e, torch.cat([_trunc(e.acc, io).double() * be * se * (1 + ae * (1 - se)), e.acc * ae * se], 1).to(io), None)
    # MODE 2 shares MODE 0's plants through the same accumulator; gemm_tn
    for family in FAMILIES:
        t, geo = _tn_inputs(512, 24, 16, io, family), _tn_geometry(24, 16, 512, 2)
        u = geo.units[5]
        twice = (t.a[32 * u.k0:32 * u.k1].double().t() @ t.b[32 * u.k0:32 * u.k1].double())
        for name, c, acc in (("one K slice counted twice", t.prod + twice, 0), ("accumulate ignored", t.prod, 1),
                             ("one K slice counted twice", t.prod + t.c0.double() + twice, 1)):
            if family == "exact":
                with pytest.raises(AssertionError, match="bit for bit"):
                    _tn_ratios(t, geo, acc, c.float())
            else:
                planted[f"gemm_tn {name} (accumulate {acc})"] = _tn_ratios(t, geo, acc, c.float())["c"]
    x = _cs_inputs(67, 8, io, "gauss")
    planted["colsum: row groups of R + 1"] = _cs_ratios(x, torch.stack([x[rg::6].float().sum(0) for rg in range(5)]), 5, "gauss")["partial"]
    for name, v in planted.items():
        print(f"planted {_DT[io]} {name}: {v:.3g}")
        assert v > 1, name


# ---- GPU: launches on guarded buffers ----------------------------------------------------------------------------------------------------
def _view(shape, dtype, data=None, rs=None, lead=0):
    """a (rows, cols) view with row stride rs, `lead` elements into its first row: a column block of a wider buffer"""
    rows, cols = shape
    rs = cols if rs is None else rs
    return _Buf(2 * GUARD + lead + (rows - 1) * rs + cols, GUARD + lead, (rs, 1), shape, dtype, DEV, data)


def _vec(n, dtype, data, shift):
    return None if data is None else _Buf.flat((n,), dtype, DEV, data, shift)


def _bias_code(b):
    return _abi.dtype_code(b.dtype) if b is not None else 0


def _gpu_gs0(d, strided, want_ab=True):
    M, K, H, io = d.M, d.K, d.H, d.io
    x = _view((M, K), io, d.x, *((K + 16, 8) if strided else ()))
    w = _view((2 * H, K), io, d.w, *((K + 8, 8) if strided else ()))
    bias = _vec(2 * H, d.bias.dtype if d.bias is not None else F32, d.bias, 1 if strided else 0)
    ab = _view((M, 2 * H), io, None, *(((2 * H + 5) | 1, 3) if strided else ()))      # odd strides and odd offsets: the entry takes them
    h = _view((M, H), io, None, *(((H + 3) | 1, 1) if strided else ()))
    desc = _abi.GemmSwigluDesc()
    desc.M, desc.K, desc.H, desc.io_dtype, desc.bias_dtype = M, K, H, _abi.dtype_code(io), _bias_code(d.bias)
    desc.x_rs, desc.w_rs, desc.ab_rs, desc.h_rs = (b.view.stride(0) for b in (x, w, ab, h))
    desc.x, desc.weight, desc.bias, desc.ab, desc.h = _ptr(x), _ptr(w), _ptr(bias), _ptr(ab) if want_ab else None, _ptr(h)
    _abi.launch("mxvl_gemm_swiglu_fwd", desc, device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_buffers(f"gemm_swiglu_fwd {M}x{K}x{H} {_DT[io]} strided={strided} ab={want_ab}", inputs=(("x", x), ("weight", w), ("bias", bias)),
                    outputs=(("h", h),) + ((("ab", ab),) if want_ab else ()), untouched=() if want_ab else (("ab", ab),))
    return (ab.view.cpu() if want_ab else None), h.view.cpu()


def _gpu_gs1(d, strided, want_partial=True):
    M, K, H, io = d.M, d.K, d.H, d.io
    dy = _view((M, K), io, d.x, *((K + 16, 8) if strided else ()))
    w = _view((H, K), io, d.w, *((K + 8, 8) if strided else ()))
    ab = _view((M, 2 * H), io, d.ab, *((2 * H + 6, 2) if strided else ()))
    dab = _view((M, 2 * H), io, None, *((2 * H + 10, 6) if strided else ()))
    partial = _view((_gs_partials(M), 2 * H), F32)
    desc = _abi.GemmSwigluBwdDesc()
    desc.M, desc.K, desc.H, desc.io_dtype = M, K, H, _abi.dtype_code(io)
    desc.dy_rs, desc.w_rs, desc.ab_rs, desc.dab_rs = (b.view.stride(0) for b in (dy, w, ab, dab))
    desc.dy, desc.w3t, desc.ab, desc.dab, desc.partial = _ptr(dy), _ptr(w), _ptr(ab), _ptr(dab), _ptr(partial) if want_partial else None
    _abi.launch("mxvl_gemm_swiglu_bwd", desc, device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_buffers(f"gemm_swiglu_bwd {M}x{K}x{H} {_DT[io]} strided={strided} partial={want_partial}",
                    inputs=(("dy", dy), ("w3t", w), ("ab", ab)), outputs=(("dab", dab),) + ((("partial", partial),) if want_partial else ()),
                    untouched=() if want_partial else (("partial", partial),))
    return dab.view.cpu(), (partial.view.cpu() if want_partial else None)


def _gpu_nt(d, strided):
    M, K, N, io = d.M, d.K, d.H, d.io
    a = _view((M, K), io, d.x, *((K + 16, 8) if strided else ()))
    b = _view((N, K), io, d.w, *((K + 8, 8) if strided else ()))
    bias = _vec(N, d.bias.dtype if d.bias is not None else F32, d.bias, 1 if strided else 0)
    c = _view((M, N), io, None, *((N + 6, 2) if strided else ()))
    desc = _abi.GemmNtDesc()
    desc.M, desc.K, desc.N, desc.io_dtype, desc.bias_dtype = M, K, N, _abi.dtype_code(io), _bias_code(d.bias)
    desc.a_rs, desc.b_rs, desc.c_rs = (t.view.stride(0) for t in (a, b, c))
    desc.a, desc.b, desc.bias, desc.c = _ptr(a), _ptr(b), _ptr(bias), _ptr(c)
    _abi.launch("mxvl_gemm_nt", desc, device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_buffers(f"gemm_nt {M}x{K}x{N} {_DT[io]} strided={strided}", inputs=(("a", a), ("b", b), ("bias", bias)), outputs=(("c", c),))
    return c.view.cpu()


def _gpu_tn(d, q, accumulate, strided):
    K, M, N, io = d.K, d.M, d.N, d.io
    a = _view((K, M), io, d.a, *((M + 24, 16) if strided else ()))
    b = _view((K, N), io, d.b, *((N + 8, 0) if strided else ()))
    c = _view((M, N), F32, d.c0 if accumulate else None, *((N + 3, 1) if strided else ()))
    desc = _abi.GemmTnDesc()
    desc.M, desc.N, desc.K, desc.io_dtype, desc.accumulate, desc.slices_per_xcd = M, N, K, _abi.dtype_code(io), accumulate, q
    desc.a_rs, desc.b_rs, desc.c_rs = (t.view.stride(0) for t in (a, b, c))
    desc.a, desc.b, desc.c = _ptr(a), _ptr(b), _ptr(c)
    _abi.launch("mxvl_gemm_tn", desc, device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_buffers(f"gemm_tn {K}x{M}x{N} q{q} {_DT[io]} acc{accumulate} strided={strided}", inputs=(("a", a), ("b", b)), outputs=(("c", c),))
    return c.view.cpu()


def _gpu_cs(x, io, strided):
    rows, C = x.shape
    R = _cs_geometry(rows, C).R
    xb = _view((rows, C), io, x, *((C + 8, 8) if strided else ()))
    partial = _view((R, C), F32)
    _abi.launch("mxvl_colsum", _ptr(xb), _ptr(partial), rows, C, xb.view.stride(0), R, _abi.dtype_code(io), device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_buffers(f"colsum {rows}x{C} {_DT[io]} strided={strided}", inputs=(("x", xb),), outputs=(("partial", partial),))
    return partial.view.cpu(), R


def _worst(worst, ratios):
    for k, v in ratios.items():
        if v is not None:
            worst[k] = max(worst.get(k, 0.0), v)


@gpu
@pytest.mark.parametrize("H", GS0_H)
@pytest.mark.parametrize("io", IO, ids=_DT.get)
def test_gemm_swiglu_fwd(H, io):
    worst = {}
    for M, K, bias in _gs0_cases(H):
        for family in FAMILIES:
            d = _gs_inputs(0, M, K, H, io, family, bias)
            for strided in (False, True):
                r = _gs0_ratios(d, *_gpu_gs0(d, strided))
                _report(f"gemm_swiglu_fwd {M}x{K}x{H} {_DT[io]} {family} bias={bias} strided={strided}", **r)
                _worst(worst, {f"{family}.{k}": v for k, v in r.items()})
            none, h = _gpu_gs0(d, M % 2 == 0, want_ab=False)          # ab == NULL: nothing written there, the same h
            assert none is None
            _report(f"gemm_swiglu_fwd {M}x{K}x{H} {_DT[io]} {family} ab=NULL", **_gs0_ratios(d, None, h))
    print(f"worst gemm_swiglu_fwd H{H} {_DT[io]}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@gpu
@pytest.mark.parametrize("M,K,H", GS0_BIG, ids=lambda v: str(v))
@pytest.mark.parametrize("io", IO, ids=_DT.get)
def test_gemm_swiglu_fwd_tile_walk(M, K, H, io):
    geo = _gs_geometry(0, M, K, H)
    assert geo.per_wg >= 2 and geo.holes_start + geo.holes_loop > 0
    for family, strided, bias in (("exact", True, "io"), ("gauss", False, "f32")):
        d = _gs_inputs(0, M, K, H, io, family, bias)
        _report(f"gemm_swiglu_fwd walk {M}x{K}x{H} {_DT[io]} {family} strided={strided}", **_gs0_ratios(d, *_gpu_gs0(d, strided)))


@gpu
@pytest.mark.parametrize("H", GS1_H)
@pytest.mark.parametrize("io", IO, ids=_DT.get)
def test_gemm_swiglu_bwd(H, io):
    worst = {}
    for M, K, _ in _gs1_cases(H):
        for family in FAMILIES:
            d = _gs_inputs(1, M, K, H, io, family, None)
            for strided in (False, True):
                r = _gs1_ratios(d, *_gpu_gs1(d, strided))
                _report(f"gemm_swiglu_bwd {M}x{K}x{H} {_DT[io]} {family} strided={strided}", **r)
                _worst(worst, {f"{family}.{k}": v for k, v in r.items()})
            dab, none = _gpu_gs1(d, M % 2 == 0, want_partial=False)
            assert none is None
            _report(f"gemm_swiglu_bwd {M}x{K}x{H} {_DT[io]} {family} partial=NULL", **_gs1_ratios(d, dab, None))
    print(f"worst gemm_swiglu_bwd H{H} {_DT[io]}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@gpu
@pytest.mark.parametrize("N", GS1_H)
@pytest.mark.parametrize("io", IO, ids=_DT.get)
def test_gemm_nt(N, io):
    worst = {}
    for M, K, bias in _gs1_cases(N):
        for family in FAMILIES:
            d = _gs_inputs(2, M, K, N, io, family, bias)
            for strided in (False, True):
                r = _nt_ratios(d, _gpu_nt(d, strided))
                _report(f"gemm_nt {M}x{K}x{N} {_DT[io]} {family} bias={bias} strided={strided}", **r)
                _worst(worst, {f"{family}.{k}": v for k, v in r.items()})
    print(f"worst gemm_nt N{N} {_DT[io]}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("io", IO, ids=_DT.get)
def test_gemm_256_tile_walk(mode, io):
    M, K, H = GS1_BIG[0]
    assert _gs_geometry(mode, M, K, H).per_wg >= 2
    for family, strided, bias in (("exact", True, "io"), ("gauss", False, "f32")):
        d = _gs_inputs(mode, M, K, H, io, family, bias)
        r = _gs1_ratios(d, *_gpu_gs1(d, strided)) if mode == 1 else _nt_ratios(d, _gpu_nt(d, strided))
        _report(f"mode {mode} walk {M}x{K}x{H} {_DT[io]} {family} strided={strided}", **r)


@gpu
@pytest.mark.parametrize("K,M,N,q", TN_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("io", IO, ids=_DT.get)
def test_gemm_tn(K, M, N, q, io):
    geo = _tn_geometry(M, N, K, q)
    for family in FAMILIES if (K, M, N, q) in TN_GAUSS else ("exact",):
        d = _tn_inputs(K, M, N, io, family)
        for accumulate, strided in ((0, False), (1, True), (0, True)) if M * N <= 2 ** 18 else ((0, True), (1, False)):
            r = _tn_ratios(d, geo, accumulate, _gpu_tn(d, q, accumulate, strided))
            _report(f"gemm_tn {K}x{M}x{N} q{q} tailf{geo.tailf} {_DT[io]} {family} acc{accumulate} strided={strided}", **r)


@gpu
@pytest.mark.parametrize("C", CS_C)
@pytest.mark.parametrize("io", IO, ids=_DT.get)
def test_colsum(C, io):
    worst = {}
    for rows in CS_ROWS:
        for family in FAMILIES:
            x = _cs_inputs(rows, C, io, family)
            for strided in (False, True):
                p, R = _gpu_cs(x, io, strided)
                r = _cs_ratios(x, p, R, family)
                _report(f"colsum {rows}x{C} R{R} {_DT[io]} {family} strided={strided}", **r)
                _worst(worst, {f"{family}.{k}": v for k, v in r.items()})
    print(f"worst colsum C{C} {_DT[io]}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ---- GPU: refusals, every one before any launch ------------------------------------------------------------------------------------------
def _refuse(entry, make, base, cases):
    lib, stream = _abi.load(), _abi.stream_ptr(torch.device(DEV))

    def call(**kw):
        desc = make()
        for k, v in {**base, **kw}.items():
            setattr(desc, k, v)
        return getattr(lib, entry)(ctypes.byref(desc), stream)

    assert call() == 0, entry
    for kw, code in cases:
        assert call(**kw) == ERR[code], (entry, kw, code)
    assert getattr(lib, entry)(None, stream) == ERR["MXVL_ERR_NULL"]
    torch.cuda.synchronize()


@gpu
def test_refusals():
    """every MXVL_ERR_* branch of the five entries; the tensors are large enough for any of these descriptors, were one to launch"""
    bf, f16c, f32c = (_abi.dtype_code(t) for t in (BF16, F16, F32))
    t16 = lambda: torch.zeros(1 << 16, dtype=BF16, device=DEV)
    x, w, ab, h, bias = t16(), t16(), t16(), t16(), torch.zeros(1 << 12, device=DEV)
    part = torch.zeros(1 << 14, device=DEV)
    p = lambda t, off=0: t.data_ptr() + off
    N_, D_, S_, ST_, U_ = "MXVL_ERR_NULL", "MXVL_ERR_DTYPE", "MXVL_ERR_SHAPE", "MXVL_ERR_STRIDE", "MXVL_ERR_UNSUPPORTED"
    _refuse("mxvl_gemm_swiglu_fwd", _abi.GemmSwigluDesc,
            dict(M=40, K=128, H=24, io_dtype=bf, bias_dtype=f32c, x_rs=128, w_rs=128, ab_rs=48, h_rs=24, x=p(x), weight=p(w), bias=p(bias), ab=p(ab), h=p(h)),
            [(dict(x=None), N_), (dict(weight=None), N_), (dict(h=None), N_), (dict(io_dtype=f32c), D_), (dict(M=0), S_), (dict(K=0), S_), (dict(H=0), S_),
             (dict(K=96), U_), (dict(bias_dtype=f16c), D_), (dict(x_rs=132), ST_), (dict(w_rs=132), ST_), (dict(x=p(x, 2)), ST_), (dict(weight=p(w, 8)), ST_),
             (dict(x_rs=120), ST_), (dict(w_rs=64), ST_), (dict(h_rs=23), ST_), (dict(ab_rs=47), ST_)])
    _refuse("mxvl_gemm_swiglu_bwd", _abi.GemmSwigluBwdDesc,
            dict(M=40, K=128, H=24, io_dtype=bf, dy_rs=128, w_rs=128, ab_rs=48, dab_rs=48, dy=p(x), w3t=p(w), ab=p(ab), dab=p(h), partial=p(part)),
            [(dict(dy=None), N_), (dict(w3t=None), N_), (dict(ab=None), N_), (dict(dab=None), N_), (dict(io_dtype=f32c), D_), (dict(M=0), S_), (dict(K=-64), S_),
             (dict(H=0), S_), (dict(K=96), U_), (dict(H=20), U_), (dict(dy_rs=132), ST_), (dict(w_rs=132), ST_), (dict(dy=p(x, 8)), ST_), (dict(w3t=p(w, 2)), ST_),
             (dict(ab_rs=49), ST_), (dict(dab_rs=49), ST_), (dict(ab=p(ab, 2)), ST_), (dict(dab=p(h, 2)), ST_), (dict(dy_rs=64), ST_), (dict(w_rs=120), ST_),
             (dict(ab_rs=46), ST_), (dict(dab_rs=46), ST_), (dict(partial=p(part, 4)), ST_), (dict(partial=p(part, 8)), ST_)])
    _refuse("mxvl_gemm_nt", _abi.GemmNtDesc,
            dict(M=40, K=128, N=24, io_dtype=bf, bias_dtype=bf, a_rs=128, b_rs=128, c_rs=24, a=p(x), b=p(w), bias=p(ab), c=p(h)),
            [(dict(a=None), N_), (dict(b=None), N_), (dict(c=None), N_), (dict(io_dtype=f32c), D_), (dict(M=0), S_), (dict(K=0), S_), (dict(N=-8), S_),
             (dict(K=96), U_), (dict(N=20), U_), (dict(bias_dtype=f16c), D_), (dict(a_rs=132), ST_), (dict(b_rs=132), ST_), (dict(a=p(x, 2)), ST_),
             (dict(b=p(w, 8)), ST_), (dict(c_rs=25), ST_), (dict(c=p(h, 2)), ST_), (dict(a_rs=120), ST_), (dict(b_rs=64), ST_), (dict(c_rs=22), ST_)])
    _refuse("mxvl_gemm_tn", _abi.GemmTnDesc,
            dict(M=24, N=16, K=512, io_dtype=bf, accumulate=0, slices_per_xcd=0, a_rs=24, b_rs=16, c_rs=16, a=p(x), b=p(w), c=p(part)),
            [(dict(a=None), N_), (dict(b=None), N_), (dict(c=None), N_), (dict(io_dtype=f32c), D_), (dict(M=0), S_), (dict(N=0), S_), (dict(K=0), S_),
             (dict(K=544), U_), (dict(K=448), U_), (dict(M=20), U_), (dict(N=12), U_), (dict(a_rs=28), ST_), (dict(b_rs=20), ST_), (dict(a=p(x, 2)), ST_),
             (dict(b=p(w, 8)), ST_), (dict(c=p(part, 2)), ST_), (dict(a_rs=16), ST_), (dict(b_rs=8), ST_), (dict(c_rs=15), ST_)])
    lib, stream = _abi.load(), _abi.stream_ptr(torch.device(DEV))
    tn = _abi.GemmTnDesc()                                        # deterministic mode: the atomics of gemm_tn are refused
    tn.M, tn.N, tn.K, tn.io_dtype, tn.a_rs, tn.b_rs, tn.c_rs, tn.a, tn.b, tn.c = 24, 16, 512, bf, 24, 16, 16, p(x), p(w), p(part)
    _abi.set_deterministic(True)
    try:
        _abi.sync_deterministic()
        assert lib.mxvl_gemm_tn(ctypes.byref(tn), stream) == ERR[U_]
    finally:
        _abi.set_deterministic(None)
        _abi.sync_deterministic()
    assert lib.mxvl_gemm_tn(ctypes.byref(tn), stream) == 0
    cs = lambda **kw: lib.mxvl_colsum(*[{**dict(x=p(x), partial=p(part), rows=40, cols=24, rs=24, n=3, io=bf), **kw}[k]
                                        for k in ("x", "partial", "rows", "cols", "rs", "n", "io")], stream)
    assert _cs_geometry(40, 24).R == 3 and cs() == 0
    for kw, code in [(dict(x=None), N_), (dict(partial=None), N_), (dict(io=f32c), D_), (dict(rows=0), S_), (dict(cols=0), S_), (dict(cols=20), U_),
                     (dict(n=2), U_), (dict(n=4), U_), (dict(rs=16), ST_), (dict(rs=28), ST_), (dict(x=p(x, 2)), ST_), (dict(partial=p(part, 4)), ST_)]:
        assert cs(**kw) == ERR[code], ("mxvl_colsum", kw, code)
    torch.cuda.synchronize()
