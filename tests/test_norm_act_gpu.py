"""csrc/fused_norm_act.hip against float64: the ten vector instantiations of add + LayerNorm and the wave-per-row pair, the six dtype
triples with and without a branch, every optional pointer, the grid-stride loops, and the five SwiGLU gate kernels in fp32 / bf16 / fp16,
with per-element error bounds built from counted operations (fp64_bounds.py: U, _ulp, _rho, FLOOR).

What the operations were given, and from where: build.py compiles with `-O3 -ffp-contract=fast` and neither -ffast-math nor
-fno-hip-fp32-correctly-rounded-divide-sqrt, so `/ (float)C` is the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence: ONE
rounding, U.  `rsqrtf` lowers to v_rsq_f32 (with a denormal pre-scale), documented at one ulp: 2 U.  Contraction only removes roundings.

add + LN forward.  D = the longest addition chain of the path, its division included: 4 K + log2(LPR) + 1 for C = 4 K LPR on the vector
kernels, ceil(C / 64) + 7 for a wave per row.  With S = sum |h| over the row, statistics in float64 of the kernel's OWN h, eps the fp32
value the descriptor carries:
    dmean = D U S / C
    dvar  = (D + 4) U var + dmean^2 + U (var + eps)      the chain of squares, the shift of the centre, the rounding of `+ eps`
    rho   = dvar / (2 (var + eps)) + 2 U                  (the add's rounding is inside dvar) + v_rsq_f32's ulp
    dxh   = (dmean + U |d|) rstd + |d| rstd (rho + U)     d = h - mean: its subtraction, the product with rstd
    tol_n = |gamma| dxh + U (|xh gamma| + |n|) + ulp_out(n)
mean is held to dmean, rstd to rstd rho.  h = x + branch is held to the exact sum of the widened inputs: half an fp32 ulp in an fp32 stream,
one bf16 ulp in a bf16 stream (the fp32 sum is rounded again).

add + LN backward.  mean and rstd are INPUTS: the reference is dx = rstd (g - m1 - xh m2) + dh in float64 with g = dn gamma, xh = (h - mean)
rstd, m1 = mean(g), m2 = mean(g xh) on the same fp32 values.  xh carries 2 U (subtraction, product), g one, the chains D:
    dm1 = (D + 1) U sum|g| / C,   dm2 = (D + 1) U sum|g xh| / C + mean(|g| dxh)
    dt  = U |g| + dm1 + |xh| dm2 + |m2| dxh + U |xh m2| + 2 U (|g| + |m1| + |xh m2|)      the product and the two subtractions
    tol = rstd (dt + (U + rr) |t|) + U |dx| + ulp(dx)     the product with rstd, the add of dh, the store
(dxh = 2 U |xh| and rr = 0 here; the wrapper tests, where mean and rstd come from the forward kernel, pass the forward's dxh and rho).
dbranch is the branch dtype's rounding of the same fp32 value, so it also EQUALS dx cast to that dtype.  The sums of the partial rows,
added in float64, are bounded for any summation order over the rows: rows U sum|dn xh| + sum|dn| dxh for dgamma, rows U sum|dn| for dbeta,
and rows U sum|.| against the float64 column sum of what the kernel WROTE for the branch sums (include/mxvl.h: "as written").

SwiGLU.  s = silu(a), rho = _rho(a).  fp32: y = s b, tol = |b| |s| rho + ulp(y).  16-bit: y = io(io(s) b) and the product of two 16-bit
numbers is exact in fp32, so the kernel must give the reference's very number unless its fp32 s can round to another 16-bit number than
the float64 s does -- `flip`, where s lies within |s| rho of a tie:  tol = |b| (|s| rho + flip ulp_io(s)) + flip ulp_io(y).  This is
the bound |b| (|s| rho + ulp_io(s)) + ulp_io(y) with its two ulp terms kept only where they can arise; without that a kernel that omits
the inner rounding stays inside it everywhere (its error is at most |b| ulp_io(s) / 2 + ulp_io(y)), and that planted error has to show.
Backward: da = dy b sg (1 + a (1 - sg)), tol = |dy b| 3 rho sg (1 + |a (1 - sg)|) + ulp_io(da) (the sigmoid-derivative bound of
test_dwconv2d_gpu.py); db = dy a sg, tol = |db| rho + ulp_io(db).  The column-sum kernels add sum(partial) against the float64 column sum of
the kernel's own dab, within ceil(rows / R) U sum|dab|.  A silu below FLOOR may be flushed: |b| FLOOR.

Every tensor a kernel reads or writes is a view into a NaN-patterned buffer with guard bands (fp64_bounds._Buf); launches go through
_abi.launch with the test's own pointers.  The CPU tests (no `gpu` mark) hold reference and bound in place: against torch's float64
autograd, against fp32 emulations of each path's summation order (must stay under the bound on every input family), against planted errors
(must not), and the restated dispatch must find every path in the case lists.

Measured on an MI355X, largest err / tol (the fp32 emulation of the summation order in brackets).  Forward: n 0.50 wherever n is 16-bit
(0.50) and 0.32 in fp32 (0.33) on every path; rstd 0.61 on the 64-lane vector kernels, 0.62 on the narrow rows, 0.62 on a wave per row
(0.63 / 0.64 / 0.66); mean 0.08 / 0.20 / 0.29 (0.14 / 0.18 / 0.28); h 1.00 in an fp32 stream (exact ties of the half-ulp bound) and 0.50 in
bf16.  Backward: dx 0.33 in fp32 and 0.50 in bf16 (0.34 / 0.50), dbranch 0.50 in 16-bit; dgamma up to 0.59 (one-row launches: a single
fp32 rounding against the ulp term), dbeta and the branch sums below 0.1 -- their any-order bound over the rows is a worst case no real
order comes near.  SwiGLU: fp32 y 0.30, dab 0.32 (0.18 / 0.18); 16-bit dab 0.50 (0.50); bf16 y 0.92 at an element where the inner
rounding can flip, 0 elsewhere, fp16 y 0 throughout: outside the flip set every 16-bit y was the reference's own number."""
import math
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

from fp64_bounds import FLOOR, U, _assert_buffers, _Buf, _fma32, _near_tie, _ptr, _ratio, _report, _rho, _rnd, _ulp
from medical_image_analysis_amd import _abi

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
_DT = {F32: "fp32", BF16: "bf16", F16: "fp16"}
gpu = pytest.mark.gpu
TRIPLES = [(F32, F32, F32), (F32, BF16, BF16), (F32, F32, BF16), (BF16, BF16, BF16), (F32, F16, F16), (F32, F32, F16)]   # (stream, branch, n)
_tid = lambda t: "-".join(_DT[d] for d in t)


# ---- 1. the dispatch of fused_norm_act.hip restated ------------------------------------------------------------------------------------
VEC_WIDTHS = (64, 128, 192, 384, 256, 512, 768, 1024, 1536, 2048)
ANY_WIDTHS = (1, 7, 63, 65, 100, 320, 1280, 2304)
LN_BWD_PARTIALS = 768


def _dispatch_k(C):
    """-> (path, K, LPR): the instantiation dispatch_k() launches for a row width"""
    if C % 256 != 0:
        return {128: ("vec", 1, 32), 384: ("vec", 3, 32), 64: ("vec", 1, 16), 192: ("vec", 3, 16)}.get(C, ("any", 0, 64))
    return ("vec", C // 256, 64) if C // 256 in (1, 2, 3, 4, 6, 8) else ("any", 0, 64)


def _ln_partials(rows):
    return min((rows + 3) // 4, LN_BWD_PARTIALS)


def _ln_geometry(C, rows, bwd):
    """launch_ln / launch_ln_any -> path, K, LPR, grid, loop (a wave / workgroup walks more than one row group), idle (a wave with fewer
    live rows than it has sub-rows), empty (workgroups that own no row)"""
    path, K, LPR = _dispatch_k(C)
    if path == "vec":
        grid, per = min((rows + 3) // 4, LN_BWD_PARTIALS if bwd else 2048), 4 * (64 // LPR)
        return types.SimpleNamespace(path=path, K=K, LPR=LPR, grid=grid, loop=rows > grid * per, idle=rows % (64 // LPR) != 0,
                                     empty=(grid - 1) * per >= rows)
    grid = _ln_partials(rows) if bwd else min(rows, 8192)
    return types.SimpleNamespace(path=path, K=K, LPR=LPR, grid=grid, loop=rows > grid, idle=False, empty=False)


def _depth(C):
    path, K, LPR = _dispatch_k(C)
    return 4 * K + int(math.log2(LPR)) + 1 if path == "vec" else -(-C // 64) + 7


def _sw_partials(rows, H):
    """mxvl_swiglu_partials"""
    return 0 if rows <= 0 or H <= 0 or H % 2 else max(1, min(rows, 8192 // ((H + 511) // 512)))


def _sw_kernel(entry, H, io, aligned=True):
    """the kernel an entry point launches: launch_swiglu and the `vec` predicate of mxvl_swiglu_bwd_colsum"""
    if entry in ("fwd", "bwd"):
        return ("pair_" if H % 2 == 0 else "scalar_") + entry
    assert H % 2 == 0
    return "colsum16" if H % 8 == 0 and io != F32 and aligned else "colsum_pair"


def _sw_grid(entry, rows, H):
    """-> (workgroups, whether a wave / thread walks more than one item)"""
    if entry == "colsum":
        return -(-((H + 511) // 512) * _sw_partials(rows, H) // 4), rows > _sw_partials(rows, H)
    if H % 2 == 0:
        work = rows * ((H + 511) // 512)
        grid = min((work + 3) // 4, 256 * 32)
        return grid, work > grid * 4
    grid = min((rows * H + 255) // 256, 256 * 64)
    return grid, rows * H > grid * 256


def _tw(H, vec):
    """equal-width column tiles of the column-sum kernels: even for the pair kernel, multiples of 8 for the 16-byte one"""
    per = -(-H // ((H + 511) // 512))
    return (per + 7) & ~7 if vec else (per + 1) & ~1


def _aligned16(io, shift):
    return shift * (4 if io == F32 else 2) % 16 == 0


# ---- 2. references and bounds ----------------------------------------------------------------------------------------------------------
def _eps32(eps):
    return float(torch.tensor(eps, dtype=F32))


def _h_ratio(h, x, br, res):
    exact = x.double() + br.double()
    return _ratio(h, exact, (_ulp(exact, res) * (0.5 if res == F32 else 1.0)).clamp_min(FLOOR))


def _ln_fwd_ref(h, gamma, beta, eps, C, out):
    """h (rows, C): the kernel's own h -> float64 mean, rstd, n with their tolerances, and dxh / rho for a backward that gets the kernel's
    statistics"""
    eps, D = _eps32(eps), _depth(C)
    h64, g = h.double(), gamma.double()
    mean = h64.mean(1, keepdim=True)
    d = h64 - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + eps) ** -0.5
    dmean = D * U * h64.abs().sum(1, keepdim=True) / C
    dvar = (D + 4) * U * var + dmean ** 2 + U * (var + eps)
    rho = dvar / (2 * (var + eps)) + 2 * U
    xh = d * rstd
    n = xh * g + (beta.double() if beta is not None else 0.0)
    dxh = (dmean + U * d.abs()) * rstd + d.abs() * rstd * (rho + U)
    tn = g.abs() * dxh + U * ((xh * g).abs() + n.abs()) + _ulp(n, out)
    return types.SimpleNamespace(mean=mean[:, 0], tmean=dmean[:, 0].clamp_min(FLOOR), rstd=rstd[:, 0], trstd=(rstd * rho)[:, 0],
                                 n=n, tn=tn.clamp_min(FLOOR), dxh=dxh, rho=rho, mean_k=mean, rstd_k=rstd)


def _ln_bwd_ref(h, mean, rstd, gamma, dn, dh, C, res, brd, dxh=None, rr=0.0):
    """the kernel's formula in float64 on the values it reads; mean / rstd (rows,) or (rows, 1)"""
    D, rows = _depth(C), h.shape[0]
    h64, g64, dn64 = h.double(), gamma.double(), dn.double()
    mean, rstd = mean.double().reshape(rows, 1), rstd.double().reshape(rows, 1)
    xh = (h64 - mean) * rstd
    dxh = 2 * U * xh.abs() if dxh is None else dxh
    g = dn64 * g64
    gx = g * xh
    m1, m2 = g.mean(1, keepdim=True), gx.mean(1, keepdim=True)
    dm1 = (D + 1) * U * g.abs().mean(1, keepdim=True)
    dm2 = (D + 1) * U * gx.abs().mean(1, keepdim=True) + (g.abs() * dxh).mean(1, keepdim=True)
    t = g - m1 - xh * m2
    mag = g.abs() + m1.abs() + (xh * m2).abs()
    dt = U * g.abs() + dm1 + xh.abs() * dm2 + m2.abs() * dxh + U * (xh * m2).abs() + 2 * U * mag
    dx = rstd * t + (dh.double() if dh is not None else 0.0)
    tfp = rstd * (dt + (U + rr) * t.abs()) + U * dx.abs()
    px = dn64 * xh
    dgamma, dbeta = px.sum(0), dn64.sum(0)
    tdg = rows * U * px.abs().sum(0) + (dn64.abs() * dxh).sum(0) + _ulp(dgamma, F32)
    tdb = rows * U * dn64.abs().sum(0) + _ulp(dbeta, F32)
    return types.SimpleNamespace(dx=dx, tdx=(tfp + _ulp(dx, res)).clamp_min(FLOOR), tdbr=(tfp + _ulp(dx, brd)).clamp_min(FLOOR),
                                 dgamma=dgamma, tdg=tdg.clamp_min(FLOOR), dbeta=dbeta, tdb=tdb.clamp_min(FLOOR))


def _colsum_ratio(partial, written, n_terms):
    """sum of the partial rows (float64, host) against the float64 column sum of what the kernel wrote: any order over n_terms rows"""
    w = written.double().cpu()
    return _ratio(partial.double().cpu().sum(0), w.sum(0), (n_terms * U * w.abs().sum(0)).clamp_min(FLOOR))


def _sw_ref(ab, dy, io):
    """ab (rows, 2H), dy (rows, H) as the kernel gets them -> y, da, db in float64 with tolerances"""
    H = ab.shape[1] // 2
    a, b = ab[:, :H].double(), ab[:, H:].double()
    sg = torch.sigmoid(a)
    s, rho = a * sg, _rho(a)
    if io == F32:
        y = s * b
        ty = b.abs() * s.abs() * rho + _ulp(y, io)
    else:
        y = _rnd(_rnd(s, io) * b, io)
        flip = (_near_tie(s, s.abs() * rho, io) | (s.abs() < 2 * FLOOR)).double()
        ty = b.abs() * (s.abs() * rho + flip * _ulp(s, io)) + flip * _ulp(y, io)
    r = types.SimpleNamespace(y=y, ty=(ty + b.abs() * FLOOR).clamp_min(FLOOR), da=None, a_range=(float(a.min()), float(a.max())))
    if dy is not None:
        g = dy.double()
        r.da, r.db = g * b * sg * (1 + a * (1 - sg)), g * a * sg
        r.tda = ((g * b).abs() * 3 * rho * sg * (1 + (a * (1 - sg)).abs()) + _ulp(r.da, io)).clamp_min(FLOOR)
        r.tdb = (r.db.abs() * rho + _ulp(r.db, io)).clamp_min(FLOOR)
        r.dab, r.tdab = torch.cat([r.da, r.db], 1), torch.cat([r.tda, r.tdb], 1)
    return r


# ---- 3. inputs -------------------------------------------------------------------------------------------------------------------------
FAMILIES = {"randn": 1e-5, "offset100": 1e-5, "tiny": 1e-5, "tiny_eps1e-2": 1e-2, "const": 1e-5, "spike": 1e-5, "big": 1e-5}   # -> eps
_SCALE = {"randn": 1.0, "offset100": 0.1, "tiny": 1e-4, "tiny_eps1e-2": 1e-4, "const": 0.0, "spike": 1.0, "big": 1e4}


def _family(name, rows, C, g):
    r = torch.randn(rows, C, generator=g)
    if name == "randn":
        return 2.0 * r + 0.5
    if name == "offset100":                                       # separates one-pass from two-pass variance
        return 100.0 + 0.1 * r
    if name.startswith("tiny"):
        return 1e-4 * r
    if name == "const":                                           # var = 0, rstd = eps^-1/2; halves of these are bf16 numbers
        return (1.5 + 0.25 * (torch.arange(rows) % 4).float())[:, None].expand(rows, C).clone()
    if name == "spike":
        r[:, C // 3] = 1e3
        return r
    return 1e4 * r


class Ln:
    """one add + LN launch: forward (branch, beta) or backward (dbr, pdbr, dh)"""

    def __init__(self, C, rows, triple, branch=True, beta=True, family="randn", dbr=None, pdbr=True, dh=True):
        self.C, self.rows, self.triple, self.branch, self.beta, self.family = C, rows, triple, branch, beta, family
        self.dbr, self.pdbr, self.dh = (triple[0] != triple[1] if dbr is None else dbr), pdbr, dh
        self.eps = FAMILIES[family]

    def gen(self, what):
        return torch.Generator().manual_seed(zlib.crc32(f"{what} {self.C} {self.rows} {_tid(self.triple)} {self.family}".encode()))

    def id(self, bwd):
        arms = (f"dbr{int(self.dbr)} pdbr{int(self.pdbr)} dh{int(self.dh)}" if bwd else f"br{int(self.branch)} beta{int(self.beta)}")
        return f"C{self.C} rows{self.rows} {_tid(self.triple)} {self.family} {arms}"


def _ln_fwd_inputs(c):
    """x (+ branch) whose sum is the family, built in the kernel's dtypes so the reference sees what the kernel sees"""
    res, brd, _ = c.triple
    g = c.gen("fwd")
    hf = _family(c.family, c.rows, c.C, g)
    br = None
    if c.branch:
        br = (hf / 2 if c.family == "const" else 0.25 * _SCALE[c.family] * torch.randn(c.rows, c.C, generator=g)).to(brd)
        hf = hf - br.float()
    gamma, beta = 1.0 + 0.2 * torch.randn(c.C, generator=g), 0.1 * torch.randn(c.C, generator=g)
    return types.SimpleNamespace(x=hf.to(res), br=br, gamma=gamma, beta=beta if c.beta else None, eps=c.eps)


def _ln_bwd_inputs(c):
    """h in the stream dtype, mean / rstd the fp32 roundings of its float64 statistics, dn in the dtype of n, dh in the stream dtype"""
    res, _, out = c.triple
    g = c.gen("bwd")
    h = _family(c.family, c.rows, c.C, g).to(res)
    gamma = 1.0 + 0.2 * torch.randn(c.C, generator=g)
    st = _ln_fwd_ref(h, gamma, None, c.eps, c.C, out)
    dn = torch.randn(c.rows, c.C, generator=g).to(out)
    dh = torch.randn(c.rows, c.C, generator=g).to(res) if c.dh else None
    return types.SimpleNamespace(h=h, mean=st.mean.float(), rstd=st.rstd.float(), gamma=gamma, dn=dn, dh=dh)


# ---- 4. the case lists -----------------------------------------------------------------------------------------------------------------
ARM_WIDTHS = (1024, 64, 100)                                      # one vector, one narrow, one wave-per-row width for every crossed arm
SMALL_ROWS = (1, 2, 3, 5)
ARM_TRIPLES = (TRIPLES[0], TRIPLES[3], TRIPLES[4])                # fp32 all through, the bf16 stream, fp16 branch / n


def _fwd_cases(C):
    cs = [Ln(C, 111, t, branch=b) for t in TRIPLES for b in (True, False)]
    cs += [Ln(C, r, t) for r in SMALL_ROWS for t in (TRIPLES[1], TRIPLES[3])]
    if C in ARM_WIDTHS:
        cs += [Ln(C, 37, t, family=f) for f in FAMILIES for t in ARM_TRIPLES]
        cs += [Ln(C, 37, t, beta=False, branch=b) for t in (TRIPLES[0], TRIPLES[3]) for b in (True, False)]
    return cs


def _bwd_cases(C):
    cs = [Ln(C, 111, t, dbr=b) for t in TRIPLES for b in (True, False)]
    cs += [Ln(C, r, t) for r in SMALL_ROWS for t in (TRIPLES[1], TRIPLES[3])]
    if C in ARM_WIDTHS:
        cs += [Ln(C, 37, t, family=f) for f in ("offset100", "tiny", "spike", "big") for t in ARM_TRIPLES]
        cs += [Ln(C, 37, t, dbr=dbr, pdbr=pd, dh=dh) for t in (TRIPLES[1], TRIPLES[3])
               for dbr, pd, dh in ((True, True, False), (False, True, False), (True, False, True), (False, False, False), (False, True, True))]
    return cs


def _rpw(C):
    return 64 // _dispatch_k(C)[2]


# the grid-stride loops: one width per LPR plus the largest K, and the wave-per-row kernels
FWD_LOOPS = [Ln(C, 2048 * 4 * _rpw(C) + 3, TRIPLES[1]) for C in (64, 128, 2048)] + [Ln(64, 2048 * 16 + 3, TRIPLES[3]), Ln(7, 8192 + 5, TRIPLES[1])]
BWD_LOOPS = [Ln(C, 768 * 4 * _rpw(C) + 3, TRIPLES[1]) for C in (64, 128, 2048)] + [Ln(64, 768 * 16 + 3, TRIPLES[3], pdbr=True),
                                                                                   Ln(65, 4 * 768 + 5, TRIPLES[1]), Ln(7, 4 * 768 + 5, TRIPLES[3])]
ALL_WIDTHS = VEC_WIDTHS + ANY_WIDTHS

SW_DTYPES = (F32, BF16, F16)
SW_H = (2, 6, 8, 64, 170, 512, 514, 520, 1030, 2730, 2752, 1, 7, 513)
SW_ROWS = (1, 2, 3, 65)
# (rows, H, entries): R + 1, 2 R + 1 and 3 R + 5 rows for the rows-in-flight loops of the column-sum kernels; the grid caps of the others
SW_BIG = [(k * _sw_partials(10 ** 6, H) + e, H, ("colsum",)) for H in (8, 520) for k, e in ((1, 1), (2, 1), (3, 5))] + \
         [(4 * 8192 + 3, 2, ("fwd", "bwd")), (8177, 513, ("fwd", "bwd"))]
SW_SAT = [(65, 170), (65, 513), (7, 520)]                         # pair / scalar / the column-sum kernels on saturated gates


def _sw_inputs(rows, H, io, saturated=False):
    g = torch.Generator().manual_seed(zlib.crc32(f"swiglu {rows} {H} {_DT[io]} {saturated}".encode()))
    ab = 2.0 * torch.randn(rows, 2 * H, generator=g)
    if saturated:                                                 # |a| >= 88: exp2 overflows and v_rcp returns 0; 1e4 only where it fits
        vals = [20.0, 88.0, 100.0] + ([1e4] if io != F16 else [])
        sat = torch.tensor([s * v for v in vals for s in (1.0, -1.0)])
        pick = torch.randint(0, 2 * len(sat), (rows, H), generator=g)
        ab[:, :H] = torch.where(pick < len(sat), sat[pick.clamp_max(len(sat) - 1)], ab[:, :H])
    ab, dy = ab.to(io), torch.randn(rows, H, generator=g).to(io)
    return types.SimpleNamespace(ab=ab, dy=dy, ref=_sw_ref(ab, dy, io))


# ---- CPU: the case lists reach what they say they reach ------------------------------------------------------------------------------
def test_cases_cover_every_path():
    inst = {_dispatch_k(C) for C in ALL_WIDTHS}
    assert inst == {("vec", K, 64) for K in (1, 2, 3, 4, 6, 8)} | {("vec", K, L) for K in (1, 3) for L in (16, 32)} | {("any", 0, 64)}
    assert [_dispatch_k(C)[0] for C in VEC_WIDTHS] == ["vec"] * 10 and all(_dispatch_k(C)[0] == "any" for C in ANY_WIDTHS)
    assert 320 % 256 != 0 and 1280 % 256 == 0 and 2304 % 256 == 0, "both default: arms of dispatch_k"
    for bwd, per_width, loops in ((False, _fwd_cases, FWD_LOOPS), (True, _bwd_cases, BWD_LOOPS)):
        seen, arms = set(), set()
        for C in ALL_WIDTHS:
            for c in per_width(C):
                geo = _ln_geometry(C, c.rows, bwd)
                seen.add((geo.path, geo.K, geo.LPR, c.triple, c.dbr if bwd else c.branch))
                kind = "vec64" if geo.LPR == 64 and geo.path == "vec" else geo.path if geo.path == "any" else "narrow"
                arms.add((kind, "beta0" if not c.beta else "", (c.dbr, c.pdbr, c.dh) if bwd else None, c.family))
                if geo.path == "vec" and geo.LPR < 64 and c.rows in SMALL_ROWS:
                    arms.add(("idle", geo.LPR, c.rows, geo.idle))
                assert not geo.loop or geo.path == "any"
        assert seen == {i + (t, b) for i in inst for t in TRIPLES for b in (True, False)}
        for kind in ("vec64", "narrow", "any"):
            fams = {a[3] for a in arms if a[0] == kind}
            assert fams >= (set(FAMILIES) if not bwd else {"randn", "offset100", "tiny", "spike", "big"}), (kind, fams)
            if bwd:
                got = {a[2] for a in arms if a[0] == kind}
                assert got >= {(d, p, h) for d in (True, False) for p in (True, False) for h in (True, False) if (d, p, h) not in
                               ((True, False, False), (False, False, True))}, kind
                assert any(not a[2][2] for a in arms if a[0] == kind) and any(not a[2][0] and a[2][1] for a in arms if a[0] == kind)
            else:
                assert any(a[1] == "beta0" for a in arms if a[0] == kind), kind
        for L in (16, 32):                                        # waves with 1, 2 and 3 live sub-rows of four, with one of two
            assert {a[2] % (64 // L) for a in arms if a[:2] == ("idle", L) and a[3]} == set(range(1, 64 // L))
        loop = {(g.path, g.LPR, g.K) for g in (_ln_geometry(c.C, c.rows, bwd) for c in loops) if g.loop}
        assert loop >= {("vec", 16, 1), ("vec", 32, 1), ("vec", 64, 8), ("any", 64, 0)}, loop
        assert all(_ln_geometry(c.C, c.rows, bwd).loop for c in loops)
        assert any(_ln_geometry(c.C, c.rows, bwd).grid == (LN_BWD_PARTIALS if bwd else 2048) for c in loops)
    # workgroups without a row: every narrow-row backward of more than 4 rows has them (the grid is the caller's n_partials)
    assert _ln_geometry(64, 111, True).empty and _ln_geometry(128, 111, True).empty and not _ln_geometry(256, 111, True).empty
    assert _ln_geometry(7, 4 * 768 + 5, True).grid == 768 and _ln_geometry(7, 8197, False).grid == 8192

    kernels = set()
    shapes = [(r, H, ("fwd", "bwd", "colsum")) for H in SW_H for r in SW_ROWS] + SW_BIG + [(r, H, ("fwd", "bwd", "colsum")) for r, H in SW_SAT]
    for rows, H, entries in shapes:
        for io in SW_DTYPES:
            for e in entries:
                if e == "colsum" and H % 2:
                    continue
                for shift in (0, 2) if e == "colsum" and io != F32 else (0,):
                    kernels.add((_sw_kernel(e, H, io, _aligned16(io, shift)), io, _sw_grid(e, rows, H)[1]))
    want = {(k, io) for k in ("pair_fwd", "pair_bwd", "scalar_fwd", "scalar_bwd", "colsum_pair") for io in SW_DTYPES} | \
           {("colsum16", io) for io in (BF16, F16)}
    assert {k[:2] for k in kernels} == want
    assert {k[:2] for k in kernels if k[2]} == want, "every kernel also with its loop taken"
    assert _sw_kernel("colsum", 520, BF16, _aligned16(BF16, 2)) == "colsum_pair" and _sw_kernel("colsum", 520, BF16) == "colsum16"
    # the tile arithmetic: several tiles, tw rounded up, tiles of the two column-sum kernels ending at different columns
    assert [(_tw(H, False), _tw(H, True)) for H in (520, 2752)] == [(260, 264), (460, 464)] and _tw(2730, False) == 456 and _tw(1030, False) == 344
    assert _tw(514, False) == 258 and _tw(512, True) == 512 and all(_tw(H, v) <= 512 and _tw(H, v) * ((H + 511) // 512) >= H for H in SW_H for v in (0, 1))
    assert [_sw_partials(10 ** 6, H) for H in (8, 520)] == [8192, 4096] and [s[0] for s in SW_BIG[:6]] == [8193, 16385, 24581, 4097, 8193, 12293]
    assert _sw_grid("fwd", 4 * 8192 + 3, 2) == (8192, True) and _sw_grid("fwd", 8177, 513) == (256 * 64, True) and 8176 * 513 <= 256 * 64 * 256
    assert _sw_partials(3, 7) == 0 and _sw_partials(1, 2) == 1


def test_restated_partials_match_the_library():
    lib = _abi.load()
    for rows in (1, 2, 3, 4, 5, 111, 3071, 3072, 3073, 12291, 10 ** 6):
        assert lib.mxvl_add_layernorm_partials(rows) == _ln_partials(rows)
        for H in SW_H:
            assert lib.mxvl_swiglu_partials(rows, H) == _sw_partials(rows, H)


# ---- CPU: the references against torch's float64 autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 7, 64, 100, 256])
@pytest.mark.parametrize("beta,dh", [(True, True), (False, False)])
def test_ln_ref_equals_torch_float64(C, beta, dh):
    g = torch.Generator().manual_seed(C)
    rows, eps = 9, _eps32(1e-5)
    h = (2.0 * torch.randn(rows, C, generator=g) + 0.5).double().requires_grad_(True)
    gamma, b = (1.0 + 0.2 * torch.randn(C, generator=g)).double().requires_grad_(True), (0.1 * torch.randn(C, generator=g)).double().requires_grad_(True)
    dn, gh = torch.randn(rows, C, generator=g).double(), torch.randn(rows, C, generator=g).double()
    n = F.layer_norm(h, (C,), gamma, b if beta else None, eps)
    ((n * dn).sum() + ((h * gh).sum() if dh else 0.0)).backward()
    close = lambda got, want: float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    f = _ln_fwd_ref(h.detach(), gamma.detach(), b.detach() if beta else None, eps, C, F32)
    assert close(f.n, n.detach())
    r = _ln_bwd_ref(h.detach(), f.mean, f.rstd, gamma.detach(), dn, gh if dh else None, C, F32, F32)      # exact statistics
    assert close(r.dx, h.grad) and close(r.dgamma, gamma.grad) and (not beta or close(r.dbeta, b.grad))


@pytest.mark.parametrize("H", [1, 6, 170])
def test_swiglu_ref_equals_torch_float64(H):
    g = torch.Generator().manual_seed(H)
    ab, dy = 2.0 * torch.randn(5, 2 * H, generator=g), torch.randn(5, H, generator=g)
    r = _sw_ref(ab, dy, F32)
    t = ab.double().requires_grad_(True)
    y = F.silu(t[:, :H]) * t[:, H:]
    y.backward(dy.double())
    for got, want in ((r.y, y.detach()), (r.dab, t.grad)):
        assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))


# ---- CPU: each path's summation order in fp32 stays under the bound --------------------------------------------------------------------
def _tree(v):
    """the xor butterfly of wsum over the lanes of dim 1: every lane ends with the same sum"""
    idx, off = torch.arange(v.shape[1]), v.shape[1] // 2
    while off:
        v = v + v[:, idx ^ off]
        off //= 2
    return v[:, :1]


def _chains(v, C):
    """fp32 (rows, C) -> (steps, rows, lanes) in the order a lane walks its elements, and the mask of steps that exist"""
    path, K, LPR = _dispatch_k(C)
    if path == "vec":                                             # column (k LPR + lane) 4 + j, walked k-major
        return v.view(-1, K, LPR, 4).permute(1, 3, 0, 2).reshape(4 * K, -1, LPR), torch.ones(4 * K, 1, LPR, dtype=torch.bool)
    steps = -(-C // 64)
    pad = F.pad(v, (0, steps * 64 - C))
    return pad.view(-1, steps, 64).permute(1, 0, 2), (torch.arange(steps * 64) < C).view(steps, 1, 64)


def _emu_ln_fwd(x, br, gamma, beta, eps, C, triple):
    res, _, out = triple
    path, K, LPR = _dispatch_k(C)
    v = x.float()
    if br is not None:
        v = (v + br.float()).to(res).float()
    ch, on = _chains(v, C)
    cf = torch.tensor(float(C))
    if path == "vec":
        p = v.view(-1, K, LPR, 4)
        pk = (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])
        s = torch.zeros_like(pk[:, 0])
        for k in range(K):
            s = s + pk[:, k]
    else:
        s = torch.zeros_like(ch[0])
        for i in range(ch.shape[0]):
            s = s + torch.where(on[i], ch[i], torch.zeros(()))
    mean = _tree(s) / cf
    q = torch.zeros_like(ch[0])
    for i in range(ch.shape[0]):
        d = ch[i] - mean
        q = torch.where(on[i], _fma32(d, d, q), q)
    rstd = torch.rsqrt(_tree(q) / cf + torch.tensor(eps, dtype=F32))
    n = _fma32((v - mean) * rstd, gamma.expand_as(v), (beta if beta is not None else torch.zeros(C)).expand_as(v))
    return v.to(res), n.to(out), mean[:, 0], rstd[:, 0]


def _emu_ln_bwd(h, mean, rstd, gamma, dn, dh, C, triple):
    res, brd, _ = triple
    mean, rstd, cf = mean[:, None], rstd[:, None], torch.tensor(float(C))
    xh = (h.float() - mean) * rstd
    g = dn.float() * gamma
    (cg, on), (cx, _) = _chains(g, C), _chains(xh, C)
    s1, s2 = torch.zeros_like(cg[0]), torch.zeros_like(cg[0])
    for i in range(cg.shape[0]):
        s1 = s1 + torch.where(on[i], cg[i], torch.zeros(()))
        s2 = torch.where(on[i], _fma32(cg[i], cx[i], s2), s2)
    m1, m2 = _tree(s1) / cf, _tree(s2) / cf
    o = rstd * (g - m1 - xh * m2) + (dh.float() if dh is not None else 0.0)
    return o.to(res), o.to(brd), (dn.float() * xh).sum(0), dn.float().sum(0)


def _fwd_ratios(c, d, h, n, mean, rstd):
    ref = _ln_fwd_ref(h, d.gamma, d.beta, d.eps, c.C, c.triple[2])
    return dict(h=_h_ratio(h, d.x, d.br, c.triple[0]) if d.br is not None else None, mean=_ratio(mean, ref.mean, ref.tmean),
                rstd=_ratio(rstd, ref.rstd, ref.trstd), n=_ratio(n, ref.n, ref.tn))


def _bwd_ratios(c, d, dx, dbr, pg, pb, pd):
    ref = _ln_bwd_ref(d.h, d.mean, d.rstd, d.gamma, d.dn, d.dh, c.C, c.triple[0], c.triple[1])
    if dbr is not None:
        assert torch.equal(dbr.cpu(), dx.cpu().to(c.triple[1])), "dbranch is not dx rounded to the branch dtype"
    return dict(dx=_ratio(dx, ref.dx, ref.tdx), dbr=None if dbr is None else _ratio(dbr, ref.dx, ref.tdbr),
                dgamma=_ratio(pg.double().cpu().sum(0), ref.dgamma, ref.tdg), dbeta=_ratio(pb.double().cpu().sum(0), ref.dbeta, ref.tdb),
                sums=None if pd is None else _colsum_ratio(pd, dbr if dbr is not None else dx, c.rows))


@pytest.mark.parametrize("C", ALL_WIDTHS)
def test_emulated_summation_orders_within_bound(C):
    worst = {}
    for fam in FAMILIES:
        for t in ARM_TRIPLES:
            c = Ln(C, 16, t, family=fam)
            d = _ln_fwd_inputs(c)
            r = _fwd_ratios(c, d, *_emu_ln_fwd(d.x, d.br, d.gamma, d.beta, _eps32(d.eps), C, t))
            _report(f"emulated fwd C{C} {fam} {_tid(t)}", **r)
            b = _ln_bwd_inputs(c)
            dx, dbr, dg, db = _emu_ln_bwd(b.h, b.mean, b.rstd, b.gamma, b.dn, b.dh, C, t)
            rb = _bwd_ratios(c, b, dx, dbr, dg[None], db[None], dbr.float().sum(0)[None])
            _report(f"emulated bwd C{C} {fam} {_tid(t)}", **rb)
            for k, v in {**r, **rb}.items():
                if v is not None:
                    worst[(k, _tid(t))] = max(worst.get((k, _tid(t)), 0.0), v)
    print(f"emulation C{C} {_dispatch_k(C)}: worst " + " ".join(f"{k}/{t} {v:.3f}" for (k, t), v in sorted(worst.items())))


def _emu_swiglu(ab, dy, io):
    """the gate in fp32 torch with the kernels' rounding points"""
    H = ab.shape[1] // 2
    a, b, g = ab[:, :H].float(), ab[:, H:].float(), dy.float()
    sg = torch.sigmoid(a)
    y = ((a * sg).to(io).float() * b).to(io)
    return y, torch.cat([g * b * (sg * (1.0 + a * (1.0 - sg))), g * (a * sg)], 1).to(io)


@pytest.mark.parametrize("io", SW_DTYPES, ids=_DT.get)
@pytest.mark.parametrize("saturated", [False, True])
def test_emulated_swiglu_within_bound(io, saturated):
    d = _sw_inputs(300, 170, io, saturated)
    y, dab = _emu_swiglu(d.ab, d.dy, io)
    _report(f"emulated swiglu {_DT[io]} saturated={saturated}", y=_ratio(y, d.ref.y, d.ref.ty), dab=_ratio(dab, d.ref.dab, d.ref.tdab))
    if saturated:
        assert d.ref.a_range[0] <= -100 and d.ref.a_range[1] >= 100


# ---- CPU: the bounds notice planted errors ---------------------------------------------------------------------------------------------
def _planted_fwd(kind, h, gamma, beta, eps, out):
    h64, C = h.double(), h.shape[1]
    mean = h64.mean(1, keepdim=True)
    if kind == "lanes":                                           # LPR 16 summed as 32: the neighbouring row's lanes in the mean
        rs = h64.sum(1)
        mean = ((rs + rs[torch.arange(h.shape[0]) ^ 1]) / C)[:, None]
    d = h64 - mean
    var = (d * d).mean(1, keepdim=True)
    if kind == "onepass":                                         # E[x^2] - mean^2 in fp32
        v = h.float()
        m = v.mean(1, keepdim=True)
        var = ((v * v).mean(1, keepdim=True) - m * m).double()
    if kind == "cminus1":
        var = var * C / (C - 1)
    rstd = (var + {"eps2": 2 * eps, "eps0": 0.0}.get(kind, eps)) ** -0.5
    n = d * rstd * gamma.double() + (0.0 if kind == "nobeta" else beta.double())
    return n.to(out), mean[:, 0].float(), rstd[:, 0].float()


@pytest.mark.parametrize("C", [64, 1024, 100])
@pytest.mark.parametrize("triple", ARM_TRIPLES, ids=_tid)
def test_ln_bounds_flag_planted_errors(C, triple):
    res, brd, out = triple
    # forward: kind -> the family it has to show on
    for kind, fam in (("none", "randn"), ("onepass", "offset100"), ("eps2", "tiny_eps1e-2"), ("eps2", "tiny"), ("eps0", "tiny"), ("cminus1", "randn"),
                      ("nobeta", "randn"), ("lanes", "randn")):
        if (kind == "lanes" and C != 64) or (kind == "onepass" and res != F32):
            continue                                              # bf16 rows of 100 +- 0.1 hold three values: nothing left to cancel
        c = Ln(C, 16, triple, family=fam)
        d = _ln_fwd_inputs(c)
        h = (d.x.float() + d.br.float()).to(res)
        eps = _eps32(d.eps)
        ref = _ln_fwd_ref(h, d.gamma, d.beta, eps, C, out)
        n, mean, rstd = _planted_fwd(kind, h, d.gamma, d.beta, eps, out)
        r = dict(n=_ratio(n, ref.n, ref.tn), mean=_ratio(mean, ref.mean, ref.tmean), rstd=_ratio(rstd, ref.rstd, ref.trstd))
        print(f"planted fwd C{C} {_tid(triple)} {kind} on {fam}: " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        if kind == "none":
            assert max(r.values()) <= 1
        elif kind == "nobeta":
            assert r["n"] > 1
        elif kind == "lanes":
            assert r["mean"] > 1 and r["n"] > 1
        else:
            assert r["rstd"] > 1 and r["n"] > 1, kind
    # backward, 111 rows of the first family
    c = Ln(C, 111, triple, dbr=True)
    d = _ln_bwd_inputs(c)
    ref = _ln_bwd_ref(d.h, d.mean, d.rstd, d.gamma, d.dn, d.dh, C, res, brd)
    xh = (d.h.double() - d.mean.double()[:, None]) * d.rstd.double()[:, None]
    honest = dict(dx=_ratio(ref.dx.to(res), ref.dx, ref.tdx), dbr=_ratio(ref.dx.to(brd), ref.dx, ref.tdbr),
                  dgamma=_ratio(ref.dgamma.float(), ref.dgamma, ref.tdg), dbeta=_ratio(ref.dbeta.float(), ref.dbeta, ref.tdb))
    _report(f"unplanted bwd C{C} {_tid(triple)}", **honest)
    planted = {"last row missing from dgamma": _ratio((d.dn.double() * xh)[:-1].sum(0).float(), ref.dgamma, ref.tdg),
               "last row missing from dbeta": _ratio(d.dn.double()[:-1].sum(0).float(), ref.dbeta, ref.tdb),
               "dh not added": _ratio((ref.dx - d.dh.double()).to(res), ref.dx, ref.tdx)}
    if brd == BF16:                                               # the sums of the unrounded fp32 values instead of the written ones
        planted["sums of unrounded values"] = _colsum_ratio(ref.dx.sum(0)[None], ref.dx.to(brd), 111)
    for name, v in planted.items():
        print(f"planted bwd C{C} {_tid(triple)} {name}: {v:.3g}")
        assert v > 1, name


@pytest.mark.parametrize("io", SW_DTYPES, ids=_DT.get)
def test_swiglu_bounds_flag_planted_errors(io):
    d = _sw_inputs(300, 170, io)
    H, r = 170, d.ref
    a, b, g = d.ab[:, :H].double(), d.ab[:, H:].double(), d.dy.double()
    sg = torch.sigmoid(a)
    _report(f"unplanted swiglu {_DT[io]}", y=_ratio(r.y.to(io), r.y, r.ty), dab=_ratio(r.dab.to(io), r.dab, r.tdab))
    swapped = _sw_ref(torch.cat([d.ab[:, H:], d.ab[:, :H]], 1), d.dy, io)
    planted = {"halves swapped": _ratio(swapped.y.to(io), r.y, r.ty), "halves swapped, backward": _ratio(swapped.dab.to(io), r.dab, r.tdab),
               "da with 1 - a (1 - s)": _ratio((g * b * sg * (1 - a * (1 - sg))).to(io), r.da, r.tda)}
    if io != F32:
        planted["inner rounding omitted"] = _ratio((a * sg * b).to(io), r.y, r.ty)
    for name, v in planted.items():
        print(f"planted swiglu {_DT[io]} {name}: {v:.3g}")
        assert v > 1, name


# ---- GPU: add + LN through the C-ABI on guarded buffers --------------------------------------------------------------------------------
def _gpu_ln_fwd(c):
    d = _ln_fwd_inputs(c)
    (res, brd, out), shape, dev = c.triple, (c.rows, c.C), torch.device(DEV)
    x, br = _Buf.flat(shape, res, DEV, d.x), (_Buf.flat(shape, brd, DEV, d.br) if d.br is not None else None)
    gamma, beta = _Buf.flat((c.C,), F32, DEV, d.gamma), (_Buf.flat((c.C,), F32, DEV, d.beta) if d.beta is not None else None)
    h, n = _Buf.flat(shape, res, DEV), _Buf.flat(shape, out, DEV)
    mean, rstd = _Buf.flat((c.rows,), F32, DEV), _Buf.flat((c.rows,), F32, DEV)
    desc = _abi.AddLnDesc()
    desc.rows, desc.cols, desc.eps = c.rows, c.C, d.eps
    desc.res_dtype, desc.branch_dtype, desc.out_dtype = (_abi.dtype_code(t) for t in c.triple)
    desc.x, desc.branch, desc.gamma, desc.beta = _ptr(x), _ptr(br), _ptr(gamma), _ptr(beta)
    desc.h, desc.n, desc.mean, desc.rstd = _ptr(h), _ptr(n), _ptr(mean), _ptr(rstd)
    _abi.launch("mxvl_add_layernorm_fwd", desc, device=dev)
    torch.cuda.synchronize()
    _assert_buffers(c.id(False), inputs=(("x", x), ("branch", br), ("gamma", gamma), ("beta", beta)),
                    outputs=(("n", n), ("mean", mean), ("rstd", rstd)) + ((("h", h),) if br is not None else ()),
                    untouched=() if br is not None else (("h", h),))
    hk = h.view.cpu() if br is not None else d.x
    return _fwd_ratios(c, d, hk, n.view.cpu(), mean.view.cpu(), rstd.view.cpu())


def _gpu_ln_bwd(c):
    d = _ln_bwd_inputs(c)
    (res, brd, out), shape, dev = c.triple, (c.rows, c.C), torch.device(DEV)
    n_part = _ln_partials(c.rows)
    dn, h, dh = _Buf.flat(shape, out, DEV, d.dn), _Buf.flat(shape, res, DEV, d.h), (_Buf.flat(shape, res, DEV, d.dh) if d.dh is not None else None)
    gamma, mean, rstd = _Buf.flat((c.C,), F32, DEV, d.gamma), _Buf.flat((c.rows,), F32, DEV, d.mean), _Buf.flat((c.rows,), F32, DEV, d.rstd)
    dx, dbr = _Buf.flat(shape, res, DEV), (_Buf.flat(shape, brd, DEV) if c.dbr else None)
    pg, pb = _Buf.flat((n_part, c.C), F32, DEV), _Buf.flat((n_part, c.C), F32, DEV)
    pd = _Buf.flat((n_part, c.C), F32, DEV) if c.pdbr else None
    desc = _abi.AddLnBwdDesc()
    desc.rows, desc.cols, desc.n_partials = c.rows, c.C, n_part
    desc.res_dtype, desc.branch_dtype, desc.out_dtype = (_abi.dtype_code(t) for t in c.triple)
    desc.dn, desc.dh, desc.h, desc.gamma, desc.mean, desc.rstd = _ptr(dn), _ptr(dh), _ptr(h), _ptr(gamma), _ptr(mean), _ptr(rstd)
    desc.dx, desc.dbranch, desc.partial_dgamma, desc.partial_dbeta, desc.partial_dbranch = _ptr(dx), _ptr(dbr), _ptr(pg), _ptr(pb), _ptr(pd)
    _abi.launch("mxvl_add_layernorm_bwd", desc, device=dev)
    torch.cuda.synchronize()
    _assert_buffers(c.id(True), inputs=(("dn", dn), ("h", h), ("dh", dh), ("gamma", gamma), ("mean", mean), ("rstd", rstd)),
                    outputs=(("dx", dx), ("dbranch", dbr), ("partial_dgamma", pg), ("partial_dbeta", pb), ("partial_dbranch", pd)))
    cpu = lambda b: None if b is None else b.view.cpu()
    return _bwd_ratios(c, d, cpu(dx), cpu(dbr), cpu(pg), cpu(pb), cpu(pd))


@gpu
@pytest.mark.parametrize("C", ALL_WIDTHS)
def test_add_ln_forward(C):
    for c in _fwd_cases(C):
        _report(f"add_ln fwd {_dispatch_k(C)} {c.id(False)}", **_gpu_ln_fwd(c))


@gpu
@pytest.mark.parametrize("C", ALL_WIDTHS)
def test_add_ln_backward(C):
    for c in _bwd_cases(C):
        _report(f"add_ln bwd {_dispatch_k(C)} {c.id(True)}", **_gpu_ln_bwd(c))


@gpu
@pytest.mark.parametrize("c", FWD_LOOPS, ids=lambda c: f"C{c.C}-rows{c.rows}-{_tid(c.triple)}")
def test_add_ln_forward_grid_stride(c):
    geo = _ln_geometry(c.C, c.rows, False)
    assert geo.loop
    _report(f"add_ln fwd loop {_dispatch_k(c.C)} grid {geo.grid} {c.id(False)}", **_gpu_ln_fwd(c))


@gpu
@pytest.mark.parametrize("c", BWD_LOOPS, ids=lambda c: f"C{c.C}-rows{c.rows}-{_tid(c.triple)}")
def test_add_ln_backward_grid_stride(c):
    geo = _ln_geometry(c.C, c.rows, True)
    assert geo.loop
    _report(f"add_ln bwd loop {_dispatch_k(c.C)} grid {geo.grid} {c.id(True)}", **_gpu_ln_bwd(c))


# ---- GPU: the SwiGLU gate kernels ------------------------------------------------------------------------------------------------------
def _gpu_swiglu(rows, H, io, d, entries):
    """the entries on guarded buffers -> {name: ratio}; the column sums also 2 elements past a 16-byte boundary in 16-bit"""
    dev, code, out = torch.device(DEV), _abi.dtype_code(io), {}
    for e in entries:
        if e == "colsum" and H % 2:
            continue
        for shift in (0, 2) if e == "colsum" and io != F32 else (0,):
            ab, dy = _Buf.flat((rows, 2 * H), io, DEV, d.ab, shift), _Buf.flat((rows, H), io, DEV, d.dy, shift)
            what = f"swiglu {e} rows{rows} H{H} {_DT[io]} +{shift} {_sw_kernel(e, H, io, _aligned16(io, shift))}"
            if e == "fwd":
                y = _Buf.flat((rows, H), io, DEV)
                _abi.launch("mxvl_swiglu_fwd", _ptr(ab), _ptr(y), rows, H, code, device=dev)
                torch.cuda.synchronize()
                _assert_buffers(what, inputs=(("ab", ab),), outputs=(("y", y),))
                out["y"] = _ratio(y.view, d.ref.y, d.ref.ty)
                continue
            dab = _Buf.flat((rows, 2 * H), io, DEV, None, shift)
            assert (_ptr(dab) % 16 == 0) == _aligned16(io, shift)
            if e == "bwd":
                _abi.launch("mxvl_swiglu_bwd", _ptr(ab), _ptr(dy), _ptr(dab), rows, H, code, device=dev)
                part = None
            else:
                R = _sw_partials(rows, H)
                part = _Buf.flat((R, 2 * H), F32, DEV)
                _abi.launch("mxvl_swiglu_bwd_colsum", _ptr(ab), _ptr(dy), _ptr(dab), _ptr(part), R, rows, H, code, device=dev)
            torch.cuda.synchronize()
            _assert_buffers(what, inputs=(("ab", ab), ("dy", dy)), outputs=(("dab", dab), ("partial", part)))
            key = e + (f"+{shift}" if shift else "")
            out[f"{key}.dab"] = _ratio(dab.view, d.ref.dab, d.ref.tdab)
            if part is not None:
                out[f"{key}.sums"] = _colsum_ratio(part.view, dab.view, -(-rows // R))
    return out


@gpu
@pytest.mark.parametrize("H", SW_H)
@pytest.mark.parametrize("io", SW_DTYPES, ids=_DT.get)
def test_swiglu_kernels(H, io):
    for rows in SW_ROWS:
        d = _sw_inputs(rows, H, io)
        _report(f"swiglu rows{rows} H{H} {_DT[io]}", **_gpu_swiglu(rows, H, io, d, ("fwd", "bwd", "colsum")))


@gpu
@pytest.mark.parametrize("rows,H,entries", SW_BIG, ids=lambda v: str(v) if isinstance(v, int) else None)
@pytest.mark.parametrize("io", SW_DTYPES, ids=_DT.get)
def test_swiglu_loops_and_grid_caps(rows, H, entries, io):
    assert all(_sw_grid(e, rows, H)[1] for e in entries)
    d = _sw_inputs(rows, H, io)
    _report(f"swiglu rows{rows} H{H} {_DT[io]} R {_sw_partials(rows, H)}", **_gpu_swiglu(rows, H, io, d, entries))


@gpu
@pytest.mark.parametrize("rows,H", SW_SAT)
@pytest.mark.parametrize("io", SW_DTYPES, ids=_DT.get)
def test_swiglu_saturated_gates(rows, H, io):
    d = _sw_inputs(rows, H, io, saturated=True)
    assert d.ref.a_range[0] <= -100 and d.ref.a_range[1] >= 100
    _report(f"swiglu saturated rows{rows} H{H} {_DT[io]}", **_gpu_swiglu(rows, H, io, d, ("fwd", "bwd", "colsum")))


# ---- GPU: the wrappers -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    """every _abi.launch as (entry, first argument)"""
    seen, real = [], _abi.launch

    def recording(name, first, *a, **kw):
        seen.append((name, first))
        return real(name, first, *a, **kw)

    monkeypatch.setattr(_abi, "launch", recording)
    return seen


def _wrapper_ln(what, launches, x, br, br_kernel, w, b, eps, out_dt, use_h=True, use_n=True):
    """fused_ops.add_layer_norm on x (+ br), a loss on h and / or n -> every output and gradient against float64.  br_kernel: the branch
    as the kernel reads it after the wrapper's cast (CPU)."""
    from medical_image_analysis_amd.fused_ops import add_layer_norm
    launches.clear()
    h, n = add_layer_norm(x, br, w, b, eps, out_dtype=out_dt)
    C = x.shape[-1]
    rows, res, out = x.numel() // C, x.dtype, n.dtype
    g = torch.Generator().manual_seed(rows + C)
    gh, gn = torch.randn(rows, C, generator=g).to(res), torch.randn(rows, C, generator=g).to(out)
    loss = 0.0
    if use_h:
        loss = loss + (h.float() * gh.to(DEV).view(x.shape).float()).sum()
    if use_n:
        loss = loss + (n.float() * gn.to(DEV).view(x.shape).float()).sum()
    ins = [t for t in (x, br, w, b) if t is not None]
    grads = dict(zip([k for k, t in zip("xrwb", (x, br, w, b)) if t is not None], torch.autograd.grad(loss, ins)))
    fwd, bwd = launches
    assert (fwd[0], bwd[0]) == ("mxvl_add_layernorm_fwd", "mxvl_add_layernorm_bwd")
    assert (bwd[1].dh is None) == (not use_h), "an unused h has to reach the kernel as a NULL dh"
    assert (fwd[1].beta is None) == (b is None) and (fwd[1].branch is None) == (br is None)
    hk, xc = h.detach().cpu().reshape(rows, C), x.detach().cpu().reshape(rows, C)
    gamma, beta = w.detach().cpu().float(), (b.detach().cpu().float() if b is not None else None)
    f = _ln_fwd_ref(hk, gamma, beta, eps, C, out)
    ratios = dict(h=_h_ratio(hk, xc, br_kernel.reshape(rows, C), res) if br is not None else None, n=_ratio(n.reshape(rows, C), f.n, f.tn))
    if br is None:
        assert torch.equal(hk, xc)
    brd = min(br.dtype, br_kernel.dtype, key=lambda t: torch.finfo(t).bits) if br is not None else res
    r = _ln_bwd_ref(hk, f.mean_k, f.rstd_k, gamma, gn if use_n else torch.zeros(rows, C), gh if use_h else None, C, res, brd, dxh=f.dxh, rr=f.rho)
    ratios.update(dx=_ratio(grads["x"].reshape(rows, C), r.dx, r.tdx), dgamma=_ratio(grads["w"], r.dgamma, r.tdg))
    if br is not None:
        assert grads["r"].dtype == br.dtype
        ratios["dbr"] = _ratio(grads["r"].reshape(rows, C), r.dx, r.tdbr)
    if b is not None:
        ratios["dbeta"] = _ratio(grads["b"], r.dbeta, r.tdb)
    _report(what, **ratios)
    return fwd[1], bwd[1]


def _params(C, g):
    w = (1.0 + 0.2 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    return w, (0.1 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)


@gpu
@pytest.mark.parametrize("C", [256, 64, 100])
def test_wrapper_rare_dtype_combinations(C, launches):
    """the casts that bring a combination without a kernel to a built one"""
    g = torch.Generator().manual_seed(C)
    w, b = _params(C, g)
    x, br = (2.0 * torch.randn(3, 7, C, generator=g) + 0.5), torch.randn(3, 7, C, generator=g)
    xd, bd = x.to(DEV).requires_grad_(True), br.to(BF16).to(DEV).requires_grad_(True)
    f, _ = _wrapper_ln(f"wrapper C{C} fp32 x, bf16 branch, fp32 n", launches, xd, bd, br.to(BF16).float(), w, b, 1e-5, F32)
    assert (f.res_dtype, f.branch_dtype, f.out_dtype) == (_abi.MXVL_F32,) * 3
    xd, bd = x.to(BF16).to(DEV).requires_grad_(True), br.to(DEV).requires_grad_(True)
    f, _ = _wrapper_ln(f"wrapper C{C} bf16 x, fp32 branch", launches, xd, bd, br.to(BF16), w, b, 1e-5, None)
    assert (f.res_dtype, f.branch_dtype, f.out_dtype) == (_abi.MXVL_BF16,) * 3


@gpu
@pytest.mark.parametrize("C", [256, 64, 100])
@pytest.mark.parametrize("res", [F32, BF16], ids=_DT.get)
def test_wrapper_strided_inputs_optional_bias_and_unused_outputs(C, res, launches):
    g = torch.Generator().manual_seed(C + 1)
    w, b = _params(C, g)
    big_x = (2.0 * torch.randn(3, 14, C, generator=g) + 0.5).to(res).to(DEV).requires_grad_(True)
    big_b = torch.randn(3, 7, 2 * C, generator=g).to(res).to(DEV).requires_grad_(True)
    x, br = big_x[:, ::2], big_b[..., :C]
    assert not x.is_contiguous() and not br.is_contiguous()
    tag = f"wrapper C{C} {_DT[res]}"
    _wrapper_ln(f"{tag} strided x and branch", launches, x, br, br.detach().cpu(), w, b, 1e-5, None)
    _wrapper_ln(f"{tag} bias=None", launches, x, br, br.detach().cpu(), w, None, 1e-5, None)
    _wrapper_ln(f"{tag} loss on h alone", launches, x, br, br.detach().cpu(), w, b, 1e-5, None, use_n=False)
    _wrapper_ln(f"{tag} loss on n alone", launches, x, br, br.detach().cpu(), w, b, 1e-5, None, use_h=False)
    _wrapper_ln(f"{tag} no branch, loss on n alone", launches, x, None, None, w, b, 1e-5, None, use_h=False)
    _wrapper_ln(f"{tag} no branch, loss on h alone", launches, x, None, None, w, b, 1e-5, None, use_n=False)


@gpu
@pytest.mark.parametrize("H", [170, 513, 520])
@pytest.mark.parametrize("io", SW_DTYPES, ids=_DT.get)
def test_wrapper_swiglu(H, io):
    """fused_ops.swiglu on a non-contiguous ab, forward and backward"""
    from medical_image_analysis_amd.fused_ops import swiglu
    d = _sw_inputs(3 * 7, H, io)
    base = torch.zeros(3, 14, 2 * H, dtype=io, device=DEV)
    base[:, ::2] = d.ab.view(3, 7, 2 * H).to(DEV)
    base.requires_grad_(True)
    ab = base[:, ::2]
    assert not ab.is_contiguous()
    y = swiglu(ab)
    dab, = torch.autograd.grad(y, ab, d.dy.view(3, 7, H).to(DEV))
    _report(f"wrapper swiglu H{H} {_DT[io]}", y=_ratio(y.reshape(-1, H), d.ref.y, d.ref.ty), dab=_ratio(dab.reshape(-1, 2 * H), d.ref.dab, d.ref.tdab))
