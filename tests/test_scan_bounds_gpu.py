"""The selective scan (csrc/scan_fwd.hip, scan_fwd_stream.h, scan_bwd.hip, scan_n1.h, scan_n1_short.h, scan_n1_bwd.h) against float64:
every instantiation the two dispatch functions can launch, forced and named, in fp32 / bf16 / fp16, with a derived per-element
bound on every output and every gradient.  tests/test_scan_gpu.py keeps the coarse parity bound against the reference's goldens.

Every tensor a kernel touches is a view into a larger buffer pre-filled with a NaN bit pattern (fp64_bounds._Buf): a store outside
the view changes the pattern, a load outside it reaches an output as NaN, an element the kernel never wrote stays NaN.  Launches go
through the descriptors of _abi, filled by the production code (_fill_fwd / _fill_bwd), so strides and base pointers are the test's
own.  The CPU tests (no `gpu` mark) hold the reference and the bound in place: against the goldens, against two honest fp32
implementations (must stay under the bound) and against planted errors (must not).

Input families (section 2):
  standard   the distribution of conftest.scan_inputs: A = -0.5 rand, delta = 0.5 rand, bias = 0.5 rand, the rest randn
  long       A = -(0.002 + 0.006 rand): |A| dl <= 0.011 a step, so the state entering a 128-step chunk is still > 0.24 of what it was
             128 steps earlier for EVERY (channel, state): chunk hand-over carries most of the value
  mamba      A = -[1 .. N], dt log-uniform in [1e-3, 0.1] through the bias (inverse softplus), delta = 0.1 randn
  edges      standard, with planted delta + bias in {-20, -10, 0, just below 20, just above 20, 60, 100}, z in {-30, 0, 30}, a zero
             row of u and a channel with A = 0 (softplus on)
"""
import ctypes
import functools
import types

import pytest
import torch

from conftest import golden_names, load_golden
from fp64_bounds import FLOOR, GUARD, U, _assert_buffers, _Buf, _ratio, _report, _rho, _ulp
from medical_image_analysis_amd import _abi
from medical_image_analysis_amd import selective_scan_interface as ssi

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
_DT = {F32: "fp32", BF16: "bf16", F16: "fp16"}
gpu = pytest.mark.gpu
CH = 128                                 # mxvl_scan_chunk_len: checkpoint spacing, and the chunk of every kernel's walk

# ---- 1. reference and bound (U, FLOOR, _ulp, _rho, _ratio: fp64_bounds.py) ------------------------------------------------------------
# Roundings of the state recurrence h_t = a_t h_{t-1} + b_t beyond the sequential form's one fma per step.  The kernels compose (a, b)
# segments: a lane folds its T steps (scan_fwd.hip: T = 8 or 16 fmas on h, the segment's product of a's as ONE exp2 of A2 * sum(dl)),
# the lanes of a row run a log-step prefix over the segments (scan16_x2 / scan_generic: log2(LPR) <= 6 levels, one fma on h and one
# multiply on P each), and a second serial pass applies the incoming state (T more fmas).  Any h_t therefore went through at most
# 2 * 16 + 2 * 6 = 44 roundings inside its chunk, each relative to a partial sum bounded by the magnitude recurrence H_t.  The same
# count covers the backward's reverse walk (scan_bwd.hip, T = 8, 16 lanes a row) and the wave-wide scans of the dstate-1 kernels
# (scan_n1.h / scan_n1_bwd.h: T = 4 or 8, 64 lanes: 2 * 8 + 2 * 6).  The error a chunk leaves in its last state enters the next chunk
# through E, so the count is added to E at every chunk boundary and to the tolerance of every step.
K_PREFIX = 44
# Relative error of a = exp(dl A) beyond dl's own: A2 = A log2e is rounded once (U |x|), the product with dl or with the sum of up to
# 16 deltas of a lane once more (U |x|), that sum has up to 15 adds ((T - 1) U |x|: the dl of a lane share one sign in every family),
# v_exp_f32 is good to one ulp (2 U), and a product of per-step a's that stands for a segment adds U per factor (below, per step)
_A_EXP = 18.0
_A_ABS = 16.0


def _softplus64(v):
    return torch.where(v > 20.0, v, torch.log1p(torch.exp(v.clamp_max(20.0))))


def _expand(x):
    """the descriptor's tensors in float64 with delta / bias per channel and B / C per channel: (u, dlr, t0, A, Bx, Cx, z, D)"""
    u = x["u"].double()
    Bn, Dn, L = u.shape
    A = x["A"].double()
    Bm, Cm = x["B"].double(), x["C"].double()
    if Bm.dim() == 3:
        Bm, Cm = Bm.unsqueeze(1), Cm.unsqueeze(1)
    dpg = Dn // Bm.shape[1]
    ratio = Dn // x["delta"].shape[1]
    dlr = x["delta"].double().repeat_interleave(ratio, 1)
    t0 = torch.zeros_like(dlr)
    if x.get("delta_bias") is not None:
        dlr = dlr + x["delta_bias"].double().repeat_interleave(ratio)[None, :, None]
        t0 = U * dlr.abs()                                               # one fp32 add
    Bx, Cx = Bm.repeat_interleave(dpg, 1), Cm.repeat_interleave(dpg, 1)  # (batch, dim, N, L)
    z = x["z"].double() if x.get("z") is not None else None
    Dv = x["D"].double() if x.get("D") is not None else None
    return u, dlr, t0, A, Bx, Cx, z, Dv, dpg


def _scan_ref(x, dout=None, io=F32, out_f32=False):
    """x: dict of u (B, D, L), delta (B, D / ratio, L), A (D, N), B / C (B, G, N, L), optional D, z, delta_bias (D / ratio), softplus.
    16-bit inputs widen exactly.  -> namespace of float64 out, last, ckpt (B, D, chunks, N), and with dout du, ddelta (per CHANNEL, as
    the kernels write it), dz, dA, dB, dC, dD, dbias (per channel), each with its tolerance t<name>."""
    u, dlr, t0, A, Bx, Cx, z, Dv, dpg = _expand(x)
    Bn, Dn, L = u.shape
    N = A.shape[1]
    G = Dn // dpg
    oio = F32 if out_f32 else io
    if x["softplus"]:
        dl = _softplus64(dlr)
        sg = torch.where(dlr > 20.0, torch.ones_like(dlr), torch.sigmoid(dlr))      # d softplus
        tdl = sg * t0 + dl * _rho(dlr)
    else:
        dl, sg, tdl = dlr, None, t0
    xa = dl[:, :, None, :] * A[None, :, :, None]
    a = torch.exp(xa)
    ra = A.abs()[None, :, :, None] * tdl[:, :, None, :] + (_A_EXP * xa.abs() + _A_ABS) * U
    Bu = Bx * u[:, :, None, :]
    b = dl[:, :, None, :] * Bu
    tb = Bu.abs() * tdl[:, :, None, :] + 2 * U * b.abs()
    hs, ths = torch.empty_like(a), torch.empty_like(a)
    h = torch.zeros(Bn, Dn, N, dtype=torch.float64)
    H, E = h.clone(), h.clone()
    for t in range(L):
        if t and t % CH == 0:
            E = E + K_PREFIX * U * H
        at = a[..., t]
        E = at * E + at * H * (ra[..., t] + U) + tb[..., t]
        H = at * H + b[..., t].abs()
        h = at * h + b[..., t]
        E = E + 2 * U * H                                                # the step's product and add
        hs[..., t], ths[..., t] = h, E + K_PREFIX * U * H
    r = types.SimpleNamespace(hs=hs, ths=ths)
    Ch = Cx * hs
    Du = Dv[None, :, None] * u if Dv is not None else torch.zeros_like(u)
    y = Ch.sum(2) + Du
    ty = (Cx.abs() * ths).sum(2) + (N + 1) * U * (Ch.abs().sum(2) + Du.abs())
    if z is not None:
        s = torch.sigmoid(z)
        sz = z * s
        r.out, r.tout = y * sz, sz.abs() * ty + (y * sz).abs() * _rho(z)
    else:
        r.out, r.tout = y, ty
    r.tout = (r.tout + 0.5 * _ulp(r.out, oio)).clamp_min(FLOOR)
    r.last, r.tlast = hs[..., L - 1], ths[..., L - 1].clamp_min(FLOOR)
    nc = (L + CH - 1) // CH
    r.ckpt = torch.zeros(Bn, Dn, nc, N, dtype=torch.float64)
    r.tckpt = torch.full_like(r.ckpt, FLOOR)
    for c in range(1, nc):
        r.ckpt[:, :, c], r.tckpt[:, :, c] = hs[..., c * CH - 1], ths[..., c * CH - 1].clamp_min(FLOOR)
    if dout is None:
        return r
    go = dout.double()
    if z is not None:
        dy, tdy = go * sz, (go * sz).abs() * (_rho(z) + U)
        gp = s * (1 + z * (1 - s))                                       # d silu
        r.dz = go * y * gp
        # y is recomputed from a recomputed state (ty); silu' = s (1 + z (1 - s)): two sigmoids' worth of _rho, three products
        r.tdz = (go.abs() * (gp.abs() * ty + y.abs() * (2 * _rho(z) * s * (1 + (z * (1 - s)).abs()) + 3 * U * gp.abs()))
                 + 0.5 * _ulp(r.dz, io)).clamp_min(FLOOR)
    else:
        dy, tdy = go, torch.zeros_like(go)
        r.dz = r.tdz = None
    # adjoint g_t = a_{t+1} g_{t+1} + C_t dy_t: the same recurrence walked backwards, the same magnitude / error model
    src = Cx * dy[:, :, None, :]
    tsrc = Cx.abs() * tdy[:, :, None, :] + 2 * U * src.abs()
    gs, tgs = torch.empty_like(a), torch.empty_like(a)
    g = torch.zeros(Bn, Dn, N, dtype=torch.float64)
    Gm, Eg = g.clone(), g.clone()
    for t in range(L - 1, -1, -1):
        if t + 1 < L:
            if (t + 1) % CH == 0:
                Eg = Eg + K_PREFIX * U * Gm
            an = a[..., t + 1]
            Eg = an * Eg + an * Gm * (ra[..., t + 1] + U)
            Gm, g = an * Gm, an * g
        Eg = Eg + tsrc[..., t]
        Gm, g = Gm + src[..., t].abs(), g + src[..., t]
        Eg = Eg + 2 * U * Gm
        gs[..., t], tgs[..., t] = g, Eg + K_PREFIX * U * Gm
    zero = torch.zeros(Bn, Dn, N, 1, dtype=torch.float64)
    hp, thp = torch.cat([zero, hs[..., :-1]], -1), torch.cat([zero, ths[..., :-1]], -1)      # h_{t-1}
    dl4, tdl4, u4, A4 = dl[:, :, None, :], tdl[:, :, None, :], u[:, :, None, :], A[None, :, :, None]
    # du = sum_n g dl B + D dy
    v = gs * dl4 * Bx
    Ddy = Dv[None, :, None] * dy if Dv is not None else torch.zeros_like(dy)
    r.du = v.sum(2) + Ddy
    r.tdu = ((tgs * (dl4 * Bx).abs() + (gs * Bx).abs() * tdl4).sum(2) + (N + 2) * U * (v.abs().sum(2) + Ddy.abs())
             + (Dv.abs()[None, :, None] * tdy if Dv is not None else 0.0) + 0.5 * _ulp(r.du, io)).clamp_min(FLOOR)
    # d dl = sum_n g (A a h_{t-1} + B u), times softplus'
    w1, w2 = gs * A4 * a * hp, gs * Bu
    ddl = (w1 + w2).sum(2)
    tddl = ((tgs * ((A4 * a * hp).abs() + Bu.abs()) + (gs * A4 * a).abs() * thp + w1.abs() * ra).sum(2)
            + (N + 3) * U * (w1.abs() + w2.abs()).sum(2))
    if sg is not None:
        dd32 = ddl * sg
        tdd32 = sg * tddl + dd32.abs() * (_rho(dlr) + U) + ddl.abs() * sg * (1 - sg) * t0
    else:
        dd32, tdd32 = ddl, tddl
    r.ddelta, r.tddelta = dd32, (tdd32 + 0.5 * _ulp(dd32, io)).clamp_min(FLOOR)
    # the fp32 sums may run in any order: n_terms U sum|terms| plus the terms' own errors
    def _sum(terms, terr, dims, extra):
        n = 1
        for d in dims:
            n *= terms.shape[d]
        val = terms.sum(dims)
        return val, (terr.sum(dims) + (n + extra) * U * terms.abs().sum(dims) + 0.5 * _ulp(val, F32)).clamp_min(FLOOR)
    w = gs * a * hp * dl4                                                # dA over batch and time
    r.dA, r.tdA = _sum(w, tgs * (a * hp * dl4).abs() + (gs * a * dl4).abs() * thp + (gs * a * hp).abs() * tdl4 + w.abs() * ra, (0, 3), 3)
    w = (gs * dl4 * u4).view(Bn, G, dpg, N, L)                           # dB over the channels of a group
    r.dB, r.tdB = _sum(w, (tgs * (dl4 * u4).abs() + (gs * u4).abs() * tdl4).view(Bn, G, dpg, N, L), (2,), 2)
    w = (hs * dy[:, :, None, :]).view(Bn, G, dpg, N, L)
    r.dC, r.tdC = _sum(w, (ths * dy.abs()[:, :, None, :] + hs.abs() * tdy[:, :, None, :]).view(Bn, G, dpg, N, L), (2,), 1)
    r.dD = r.tdD = r.dbias = r.tdbias = None
    if Dv is not None:
        r.dD, r.tdD = _sum(dy * u, tdy * u.abs(), (0, 2), 1)
    if x.get("delta_bias") is not None:
        r.dbias, r.tdbias = _sum(dd32, tdd32, (0, 2), 0)
    r.gs, r.dy = gs, dy
    return r


OUTS = ("out", "last", "ckpt", "du", "ddelta", "dz", "dA", "dB", "dC", "dD", "dbias")


def _ratios(got, ref):
    """max err / tol of every output `got` (a dict) holds"""
    return {k: _ratio(got[k].reshape(getattr(ref, k).shape), getattr(ref, k), getattr(ref, "t" + k))
            for k in OUTS if got.get(k) is not None and getattr(ref, k, None) is not None}


# ---- 2. input families ------------------------------------------------------------------------------------------------------------------
FAMILIES = ("standard", "long", "mamba", "edges")


def _inputs(family, B, D, L, N, G=1, ratio=1, z=True, Dv=True, bias=True, softplus=True, dtype=F32, seed=0):
    """CPU tensors in the kernels' dtypes (io tensors `dtype`, weights fp32) and a dout"""
    g = torch.Generator().manual_seed(seed + 1000 * FAMILIES.index(family))
    rand = lambda *s: torch.rand(*s, generator=g)
    randn = lambda *s: torch.randn(*s, generator=g)
    D1 = D // ratio
    A = -0.5 * rand(D, N)
    Bm, Cm, u = randn(B, G, N, L), randn(B, G, N, L), randn(B, D, L)
    delta, bv = 0.5 * rand(B, D1, L), 0.5 * rand(D1)
    if family == "long":
        A = -(0.002 + 0.006 * rand(D, N))
    elif family == "mamba":
        A = -torch.arange(1, N + 1, dtype=torch.float32).repeat(D, 1)
        dt = torch.exp(rand(D1) * (torch.log(torch.tensor(0.1)) - torch.log(torch.tensor(1e-3))) + torch.log(torch.tensor(1e-3)))
        if softplus and bias:
            bv, delta = dt + torch.log(-torch.expm1(-dt)), 0.1 * randn(B, D1, L)
        else:                                                            # no softplus / no bias to carry dt: delta is dt itself
            bv, delta = torch.zeros(D1), (dt[None, :, None] * (0.5 + rand(B, D1, L))).clamp(1e-3, 0.1)
    x = dict(u=u.to(dtype), delta=delta.to(dtype), A=A.contiguous(), B=Bm.to(dtype), C=Cm.to(dtype), D=randn(D) if Dv else None,
             z=randn(B, D, L).to(dtype) if z else None, delta_bias=bv if bias else None, softplus=bool(softplus))
    if family == "edges":
        assert softplus, "the edges family plants delta + bias = -20: without softplus the state would grow like e^10 a step"
        x["A"][0] = 0.0                                                  # a channel that never forgets
        x["u"][B - 1, D - 1] = 0.0                                       # a zero row
        vals = [-20.0, -10.0, 0.0, 19.99, 20.01, 60.0, 100.0]
        for i, v in enumerate(vals):                                     # spread over rows and steps, first and last step included
            bi, di, ti = i % B, (3 * i) % D1, (i * (L - 1)) // (len(vals) - 1)
            x["delta"][bi, di, ti] = v - (float(bv[di]) if bias else 0.0)
        if z:
            for i, v in enumerate([-30.0, 0.0, 30.0]):
                x["z"][i % B, (5 * i + 1) % D, (i * (L - 1)) // 2] = v
    return x, randn(B, D, L)


# ---- 3. two honest fp32 implementations, and the planted errors ---------------------------------------------------------------------------
def _shift(v, s, fill):
    return torch.cat([torch.full_like(v[..., :s], fill), v[..., :-s]], -1)


def _scan_impl(a, b, chunked, drop_carry=None):
    """h_t = a_t h_{t-1} + b_t along the last axis, in a's dtype.  chunked: 128-step chunks, inside each a log-step prefix composition
    of the (a, b) maps (Hillis-Steele), then the carry applied.  drop_carry: the chunk whose incoming state is lost (a planted error)"""
    L = a.shape[-1]
    out = torch.empty_like(b)
    h = torch.zeros_like(b[..., 0])
    if not chunked:
        for t in range(L):
            if drop_carry is not None and t == drop_carry * CH:
                h = torch.zeros_like(h)
            h = a[..., t] * h + b[..., t]
            out[..., t] = h
        return out
    for c in range((L + CH - 1) // CH):
        P, S = a[..., c * CH:(c + 1) * CH].clone(), b[..., c * CH:(c + 1) * CH].clone()
        s = 1
        while s < P.shape[-1]:
            S = S + P * _shift(S, s, 0.0)
            P = P * _shift(P, s, 1.0)
            s *= 2
        if drop_carry == c:
            h = torch.zeros_like(h)
        out[..., c * CH:(c + 1) * CH] = S + P * h[..., None]
        h = out[..., min(L, (c + 1) * CH) - 1]
    return out


PLANTS = {   # name -> (family that exposes it, the outputs of which at least one must leave the bound)
    "carry_dropped": ("long", ("out",)),
    "last_state_early": ("standard", ("last",)),
    "state_left_out": ("standard", ("out",)),
    "Du_dropped": ("standard", ("out",)),
    "gate_neighbour": ("standard", ("out",)),
    "delta_group_neighbour": ("standard", ("out",)),
    "BC_group_neighbour": ("standard", ("out",)),
    "a_scaled": ("long", ("out",)),
    "two_ulps": ("standard", ("out",)),
    "dBdC_channel_missing": ("standard", ("dB", "dC")),
    "dbias_batch_missing": ("standard", ("dbias",)),
    "dA_last_chunk_missing": ("long", ("dA",)),
    "dz_gate_for_derivative": ("standard", ("dz",)),
}


def _impl(x, dout, dt=F32, chunked=False, io=F32, out_f32=False, plant=None):
    """the scan and its gradients computed in `dt` by the textbook formulas (fp32: an honest implementation; float64 with `plant`:
    the reference plus exactly one planted error)"""
    c = lambda t: None if t is None else t.to(dt)
    u, A, z, Dv = c(x["u"]), c(x["A"]), c(x.get("z")), c(x.get("D"))
    Bm, Cm = c(x["B"]), c(x["C"])
    Bn, Dn, L = u.shape
    N, G = A.shape[1], Bm.shape[1]
    dpg, ratio = Dn // G, Dn // x["delta"].shape[1]
    rows = torch.arange(Dn) // ratio
    if plant == "delta_group_neighbour":                                 # the last channel of delta group 0 reads group 1's row
        rows[ratio - 1] = 1
    dlr = c(x["delta"])[:, rows]
    if x.get("delta_bias") is not None:
        dlr = dlr + c(x["delta_bias"])[rows][None, :, None]
    if x["softplus"]:
        dl = torch.where(dlr > 20.0, dlr, torch.log1p(torch.exp(dlr.clamp_max(20.0))))
        sg = torch.where(dlr > 20.0, torch.ones_like(dlr), torch.sigmoid(dlr))
    else:
        dl, sg = dlr, None
    grp = torch.arange(Dn) // dpg
    if plant == "BC_group_neighbour":                                    # the last channel of group 0 reads group 1's B / C
        grp[dpg - 1] = 1
    Bx, Cx = Bm[:, grp], Cm[:, grp]
    a = torch.exp(dl[:, :, None, :] * A[None, :, :, None])
    if plant == "a_scaled":
        a[:, 1, N - 1] *= 1 + 2.0 ** -12
    b = dl[:, :, None, :] * Bx * u[:, :, None, :]
    hs = _scan_impl(a, b, chunked, drop_carry=1 if plant == "carry_dropped" else None)
    Ch = Cx * hs
    if plant == "state_left_out":
        Ch[0, 2, N - 1, L // 2] = 0.0
    Du = Dv[None, :, None] * u if Dv is not None else torch.zeros_like(u)
    if plant == "Du_dropped":
        Du[:, 3] = 0.0
    y = Ch.sum(2) + Du
    r = {}
    if z is not None:
        s = torch.sigmoid(z)
        sz = z * s
        szo = sz.clone()
        if plant == "gate_neighbour":
            szo[0, 1, L // 3] = sz[0, 1, L // 3 - 1]
        out = y * szo
    else:
        out = y
    oio = F32 if out_f32 else io
    r["out"] = out.to(oio).to(dt) if dt == F32 else out
    if plant == "two_ulps":
        r["out"] = out.to(io).double()
        r["out"][0, 0, L // 2] += 2 * float(_ulp(out[0, 0, L // 2].double(), io))
    r["last"] = hs[..., L - 2 if plant == "last_state_early" else L - 1]
    nc = (L + CH - 1) // CH
    r["ckpt"] = torch.zeros(Bn, Dn, nc, N, dtype=dt)
    for k in range(1, nc):
        r["ckpt"][:, :, k] = hs[..., k * CH - 1]
    if dout is None:
        return r
    go = c(dout.to(oio))
    if z is not None:
        dy = go * sz
        r["dz"] = go * y * (sz if plant == "dz_gate_for_derivative" else s * (1 + z * (1 - s)))
    else:
        dy = go
    src = Cx * dy[:, :, None, :]
    an = torch.cat([a[..., 1:], torch.ones_like(a[..., :1])], -1)       # g_t = a_{t+1} g_{t+1} + src_t, walked in reversed time
    gs = _scan_impl(an.flip(-1), src.flip(-1), chunked).flip(-1)
    hp = torch.cat([torch.zeros_like(hs[..., :1]), hs[..., :-1]], -1)
    dl4, u4, A4 = dl[:, :, None, :], u[:, :, None, :], A[None, :, :, None]
    r["du"] = (gs * dl4 * Bx).sum(2) + (Dv[None, :, None] * dy if Dv is not None else 0.0)
    dd = (gs * (A4 * a * hp + Bx * u4)).sum(2)
    dd = dd * sg if sg is not None else dd
    r["ddelta"] = dd
    w = gs * a * hp * dl4
    if plant == "dA_last_chunk_missing":
        w = w[..., :(nc - 1) * CH]
    r["dA"] = w.sum((0, 3))
    keep = torch.ones(Dn, dtype=dt)
    if plant == "dBdC_channel_missing":
        keep[dpg - 1] = 0.0
    k4 = keep[None, :, None, None]
    r["dB"] = (gs * dl4 * u4 * k4).view(Bn, G, dpg, N, L).sum(2)
    r["dC"] = (hs * dy[:, :, None, :] * k4).view(Bn, G, dpg, N, L).sum(2)
    if Dv is not None:
        r["dD"] = (dy * u).sum((0, 2))
    if x.get("delta_bias") is not None:
        r["dbias"] = (dd[1:] if plant == "dbias_batch_missing" else dd).sum((0, 2))
    if dt == F32:
        for k in ("du", "ddelta", "dz"):
            if k in r:
                r[k] = r[k].to(io).to(dt)
    return r


# the CPU tests' shape: two B / C groups, two delta groups a B / C group, a ragged third chunk, 16-bit and fp32
_CPU_SHAPE = dict(B=2, D=8, L=300, N=4, G=2, ratio=2)


@functools.lru_cache(maxsize=None)
def _cpu_case(family, dtype):
    x, dout = _inputs(family, dtype=dtype, **_CPU_SHAPE)
    dout = dout.to(dtype)
    return x, dout, _scan_ref(x, dout, dtype)


def test_float64_reference_reproduces_the_goldens():
    """out, last_state and every gradient of the committed scan_* goldens: the reference's selective_scan_ref and its autograd are an
    fp32 implementation of the same operation, so they are held to the very bound the kernels get"""
    for name in golden_names("scan_"):
        g = load_golden(name)
        x = dict(u=g["u"], delta=g["delta"], A=g["A"], B=g["B"], C=g["C"], D=g.get("D"), z=g.get("z"),
                 delta_bias=g.get("delta_bias"), softplus=bool(int(g["delta_softplus"])))
        r = _scan_ref(x, g["dout"], F32)
        pairs = dict(out="out", last="last_state", du="du", ddelta="ddelta", dz="dz", dA="dA", dB="dB", dC="dC", dD="dD",
                     dbias="ddelta_bias")
        _report(name, **_ratios({k: g[gk] for k, gk in pairs.items() if gk in g}, r))


@pytest.mark.parametrize("chunked", [False, True], ids=["sequential", "chunked"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_honest_fp32_implementations_stay_under_the_bound(family, dtype, chunked):
    x, dout, ref = _cpu_case(family, dtype)
    _report(f"fp32 {'chunked' if chunked else 'sequential'} {family} {_DT[dtype]}", **_ratios(_impl(x, dout, F32, chunked, dtype), ref))


@pytest.mark.parametrize("plant", sorted(PLANTS))
def test_planted_errors_leave_the_bound(plant):
    family, outs = PLANTS[plant]
    dtype = BF16 if plant == "two_ulps" else F32
    x, dout, ref = _cpu_case(family, dtype)
    clean = _ratios(_impl(x, dout, torch.float64, True, dtype), ref)
    assert max(clean.values()) < 1e-3, f"the float64 implementation itself is off the reference: {clean}"
    rat = _ratios(_impl(x, dout, torch.float64, True, dtype, plant=plant), ref)
    print(f"{plant} on {family}: " + " ".join(f"{k} {v:.3g}" for k, v in rat.items()))
    assert max(rat[k] for k in outs) > 1.0, f"{plant} stays under the bound on {family}: {rat}"


# ---- 4. launches on guarded buffers -----------------------------------------------------------------------------------------------------
IO_NAMES = ("u", "delta", "z", "B", "C", "out", "dout", "du", "ddelta", "dz")
ROW_LOCAL = ("out", "last", "ckpt", "du", "ddelta", "dz")        # no atomics: the same instantiation gives the same bits
XDBL_R = 8                                                       # dt_rank rows in front of B and C in the x_dbl-shaped buffer
PITCH_PAD = 8                                                    # extra elements a row of the strided `out`


def C(name, fwd, bwd, B=2, dpg=24, G=1, L=129, N=16, dtype=F32, z=True, Dv=True, bias=True, softplus=True, ratio=1, out_f32=False,
      fold=False, fam="standard", fv=0, bv=0, layout="contig", last=True, seed=0):
    """one GPU case: the shape, the options, the forward / backward variant forced through mxvl_set_scan_variant (0: automatic) and
    the kernels the two dispatch functions must pick for it"""
    return types.SimpleNamespace(**{k: v for k, v in locals().items()}, D=dpg * G)


def _path_ids(c):
    """ALL_PATHS entries a case stands for: the hooks' names; the forward hook does not say which state-count instantiation of the
    stream kernels ran (compile-time 16 or run-time), the dstate does"""
    f = c.fwd
    if f.startswith("scan_fwd_stream") and "fold" not in f and "pk" not in f:
        f += "/N16" if c.N == 16 else "/Nrt"
    return f, c.bwd


@functools.lru_cache(maxsize=None)
def _problem(fam, B, D, L, N, G, ratio, z, Dv, bias, softplus, dtype, out_f32, seed):
    """inputs, dout and the float64 reference of a case, shared by every launch geometry of the same problem"""
    x, dout = _inputs(fam, B, D, L, N, G, ratio, z, Dv, bias, softplus, dtype, seed)
    dout = dout.to(F32 if out_f32 else dtype)
    return x, dout, _scan_ref(x, dout, dtype, out_f32)


def _problem_of(c):
    return _problem(c.fam, c.B, c.D, c.L, c.N, c.G, c.ratio, c.z, c.Dv, c.bias, c.softplus, c.dtype, c.out_f32, c.seed)


def _call(entry, desc):
    """the raw status of one libmxvl entry on torch's current stream (a refusal is a result here, not an exception)"""
    with torch.cuda.device(DEV):
        return getattr(_abi.load(), entry)(ctypes.byref(desc), _abi.stream_ptr(torch.device(DEV)))


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                    # a faulted device serves nothing that follows: end the session here
        pytest.exit(f"the GPU reported {e}: no further launch", returncode=3)


def _mk(shape, dtype, data=None, shift=0, layout="contig"):
    """a (B, D, L) view by layout: contiguous `shift` elements off the aligned start, channel-major storage (D, B, L), or rows with a
    pitch of L + PITCH_PAD"""
    if layout == "cmajor":
        Bn, Dn, L = shape
        return _Buf(Bn * Dn * L + 2 * GUARD, GUARD, (L, Bn * L, 1), shape, dtype, DEV, data)
    if layout == "pitch":
        Bn, Dn, L = shape
        Lp = L + PITCH_PAD
        return _Buf(Bn * Dn * Lp + 2 * GUARD, GUARD, (Dn * Lp, Lp, 1), shape, dtype, DEV, data)
    return _Buf.flat(shape, dtype, DEV, data, shift)


def _run(c, shifts=None, layout=None, fv=None, bv=None, fold=None, expect_rc=0):
    """forward and backward of case `c` on guarded buffers -> namespace(res: dict of CPU tensors, fwd / bwd: the hooks' names, rc).
    shifts: {tensor name: elements off the vector boundary}; layout: contig / xz / cmajor / xdbl / ostride.  Asserts the buffers."""
    shifts, layout = shifts or {}, layout or c.layout
    fv, bv, fold = (c.fv if fv is None else fv), (c.bv if bv is None else bv), (c.fold if fold is None else fold)
    x, dout, ref = _problem_of(c)
    lib = _abi.load()
    io, oio = c.dtype, (F32 if c.out_f32 else c.dtype)
    Bn, Dn, L, N, G = c.B, c.D, c.L, c.N, c.G
    lay3 = "cmajor" if layout == "cmajor" else "contig"
    mk = lambda name, shape, dt, data=None, lay=lay3: _mk(shape, dt, data, shifts.get(name, 0), lay)
    bufs, t = {}, {}                                             # name -> _Buf (what is checked), name -> tensor (what is passed)

    def put(name, buf, view=None):
        bufs[name], t[name] = buf, (buf.view if view is None else view)

    if layout == "xz":                                           # u | z halves of one (B, 2 D, L) buffer, du | dz of its gradient
        if c.z:
            put("xz", _Buf.flat((Bn, 2 * Dn, L), io, DEV, torch.cat([x["u"], x["z"]], 1)))
            put("dxz", _Buf.flat((Bn, 2 * Dn, L), io, DEV))
            t["u"], t["z"], t["du"], t["dz"] = t["xz"][:, :Dn], t["xz"][:, Dn:], t["dxz"][:, :Dn], t["dxz"][:, Dn:]
        else:                                                    # no gate: the other half is nobody's, and must keep the pattern
            half = lambda data=None: _Buf(Bn * 2 * Dn * L + 2 * GUARD, GUARD, (2 * Dn * L, L, 1), (Bn, Dn, L), io, DEV, data)
            put("u", half(x["u"]))
            put("du", half())
    else:
        put("u", mk("u", (Bn, Dn, L), io, x["u"]))
        put("du", mk("du", (Bn, Dn, L), io))
        if c.z:
            put("z", mk("z", (Bn, Dn, L), io, x["z"]))
    if "dz" not in t:
        put("dz", mk("dz", (Bn, Dn, L), io))                     # without z: handed over all the same, and must stay untouched
    put("delta", mk("delta", tuple(x["delta"].shape), io, x["delta"]))
    put("ddelta", mk("ddelta", (Bn, Dn, L), io))
    put("out", mk("out", (Bn, Dn, L), oio, None, "pitch" if layout == "ostride" else lay3))
    put("dout", mk("dout", (Bn, Dn, L), oio, dout))
    if layout == "xdbl":                                         # B and C as row slices of x_dbl (B, R + 2 N, L); dB / dC likewise
        assert G == 1
        rows = XDBL_R + 2 * N
        filler = torch.randn(Bn, rows, L, generator=torch.Generator().manual_seed(1)).to(io)
        filler[:, XDBL_R:XDBL_R + N], filler[:, XDBL_R + N:] = x["B"][:, 0], x["C"][:, 0]
        put("x_dbl", _Buf.flat((Bn, rows, L), io, DEV, filler))
        t["B"], t["C"] = t["x_dbl"][:, XDBL_R:XDBL_R + N].unsqueeze(1), t["x_dbl"][:, XDBL_R + N:].unsqueeze(1)
        put("dx_dbl", _Buf(Bn * rows * L + 2 * GUARD, GUARD + XDBL_R * L, (rows * L, L, 1), (Bn, 2 * N, L), F32, DEV,
                           torch.zeros(Bn, 2 * N, L)))
        t["dB"], t["dC"] = t["dx_dbl"][:, :N].unsqueeze(1), t["dx_dbl"][:, N:].unsqueeze(1)
    else:
        put("B", _Buf.flat((Bn, G, N, L), io, DEV, x["B"], shifts.get("B", 0)))
        put("C", _Buf.flat((Bn, G, N, L), io, DEV, x["C"], shifts.get("C", 0)))
        put("dB", _Buf.flat((Bn, G, N, L), F32, DEV, torch.zeros(Bn, G, N, L)))
        put("dC", _Buf.flat((Bn, G, N, L), F32, DEV, torch.zeros(Bn, G, N, L)))
    put("A", _Buf.flat((Dn, N), F32, DEV, x["A"]))
    put("dA", _Buf.flat((Dn, N), F32, DEV, torch.zeros(Dn, N)))
    for name, grad in (("D", "dD"), ("delta_bias", "dbias")):
        if x[name] is not None:
            put(name, _Buf.flat(tuple(x[name].shape), F32, DEV, x[name]))
            put(grad, _Buf.flat((Dn,), F32, DEV, torch.zeros(Dn)))
    if c.last and not fold:
        put("last", _Buf.flat((Bn, Dn, N), F32, DEV))
    slots = lib.mxvl_scan_fold_slots(Bn, L, Dn, G) if fold else 0
    put("ckpt", _Buf.flat((Dn, slots, N) if fold else (Bn, Dn, (L + CH - 1) // CH, N), F32, DEV))

    fd = _abi.ScanDesc()
    ssi._fill_fwd(fd, t["u"], t["delta"], t["A"], t["B"], t["C"], t.get("D"), t.get("z"), t.get("delta_bias"), c.softplus, t["out"],
                  t.get("last"), t["ckpt"], c.out_f32, fold)
    bd = _abi.ScanBwdDesc()
    ssi._fill_bwd(bd, t["u"], t["delta"], t["A"], t["B"], t["C"], t.get("D"), t.get("z"), t.get("delta_bias"), c.softplus, t["ckpt"],
                  t["dout"], t["du"], t["ddelta"], t["dz"], t["dA"], t["dB"], t["dC"], t.get("dD"), t.get("dbias"), c.out_f32, fold)
    r = types.SimpleNamespace(res=None, fwd=None, bwd=None, rc=0, t=t, bufs=bufs)
    lib.mxvl_set_scan_variant(fv | (bv << 8))
    try:
        r.rc = _call("mxvl_scan_fwd", fd)
        r.fwd = lib.mxvl_last_scan_kernel().decode()
        if r.rc == 0:
            _sync()
            bufs["ckpt"].before = bufs["ckpt"].raw.clone()       # from here on the checkpoints are an input
            r.rc = _call("mxvl_scan_bwd", bd)
            r.bwd = lib.mxvl_last_scan_bwd_kernel().decode()
            _sync()
    finally:
        lib.mxvl_set_scan_variant(0)
    assert r.rc == expect_rc, f"{c.name}: status {_abi.STATUS.get(r.rc, r.rc)}, expected {_abi.STATUS.get(expect_rc, expect_rc)}"
    what = f"{c.name} {layout} {shifts or ''}"
    ins = [(k, bufs[k]) for k in ("u", "xz", "z", "delta", "dout", "x_dbl", "B", "C", "A", "D", "delta_bias") if k in bufs]
    if r.rc != 0:                                                # a refusal comes before anything is enqueued
        mine = ("du", "dxz", "ddelta", "dz") if r.bwd is not None else [k for k in bufs if bufs[k].before is None]
        _assert_buffers(what, ins, (), [(k, bufs[k]) for k in mine if k in bufs])
        return r
    outs = ["du", "dxz", "ddelta", "out", "last", "ckpt", "dA", "dB", "dx_dbl", "dC", "dD", "dbias"] + (["dz"] if c.z else [])
    _assert_buffers(what, ins + [("ckpt (backward)", bufs["ckpt"])], [(k, bufs[k]) for k in outs if k in bufs],
                    [] if c.z else [("dz", bufs["dz"])])
    r.res = {k: t[k].detach().cpu() for k in ("out", "last", "ckpt", "du", "ddelta", "dA", "dB", "dC", "dD", "dbias") if k in t}
    if c.z:
        r.res["dz"] = t["dz"].detach().cpu()
    r.fold = fold
    return r


def _fold_ckpt(c, got, ref):
    """a folded call's checkpoints (dim, slots, N): slot k of the one part these shapes fold into holds the state entering step
    128 k of the batch elements laid end to end.  At a row start the state is cut (the walk multiplies what it carried by a = 0), so
    those slots hold nothing a caller may rely on; every other slot is compared"""
    ks = [(k, divmod(k * CH, c.L)) for k in range(got.shape[1])]
    ks = [(k, b, s) for k, (b, s) in ks if s > 0]
    if not ks:
        return None
    sel = lambda v: torch.stack([v[b, :, :, s - 1] for _, b, s in ks], 1)
    return _ratio(got[:, [k for k, _, _ in ks]], sel(ref.hs), sel(ref.ths).clamp_min(FLOOR))


def _check(c, r, names=True):
    """kernel names, then every output against the float64 reference over all elements"""
    ref = _problem_of(c)[2]
    if names:
        assert (r.fwd, r.bwd) == (c.fwd, c.bwd), f"{c.name}: launched {r.fwd} / {r.bwd}, expected {c.fwd} / {c.bwd}"
    res = dict(r.res)
    fold_ckpt = None
    if r.fold:
        assert res["ckpt"].shape[1] == (c.B * c.L + CH - 1) // CH, "these shapes fold into one part"
        fold_ckpt = _fold_ckpt(c, res.pop("ckpt"), ref)
    rat = _ratios(res, ref)
    if fold_ckpt is not None:
        rat["ckpt"] = fold_ckpt
    _report(f"{c.name} {_DT[c.dtype]} [{r.fwd} | {r.bwd}]", **rat)
    return rat


def _same_bits(what, r0, r1, keys=ROW_LOCAL):
    for k in keys:
        if k in r0.res and k in r1.res:
            assert torch.equal(r0.res[k], r1.res[k]), f"{what}: {k} differs from the reference launch of the same kernel"


# ---- 5. the cases: every instantiation, forced and named --------------------------------------------------------------------------------
def _gen(T=8, lpr=16, w=4, nu=2, occ=None):
    return f"scan_fwd<T{T},LPR{lpr},W{w},NU{nu}" + (f",occ{occ}>" if occ else ">")


def _stream(w, occ, vec=True, fold=False, pk=False):
    return f"scan_fwd_stream<W{w},{'vec' if vec else 'scalar'},occ{occ}" + (",fold" if fold else "") + (",pk>" if pk else ">")


def _bwd(w=4, vec=True, n16=True, fold=False, dma=False):
    return f"scan_bwd<W{w},{'vec' if vec else 'scalar'},{'N16' if n16 else 'Nrt'}" + (",fold" if fold else "") + (",dma>" if dma else ">")


N1F, N1S = "scan_n1_fwd<T{}>", "scan_n1_short_fwd"
NOZ = dict(z=False)

CASES = [
    # the tiled forward (scan_fwd.hip), every variant id with an even and an odd state count; the backward's waves forced in turn.
    # Rows of L % 4 != 0 steps cannot start on vector boundaries: both directions go element-wise
    C("fwd1_even", _gen(), _bwd(4, True, False), L=136, N=8, G=2, fv=1, bv=2),
    C("fwd1_odd", _gen(nu=1), _bwd(4, False, False), L=129, N=3, dpg=40, dtype=BF16, fam="long", fv=1),
    C("fwd2", _gen(nu=1), _bwd(4, False, False), B=3, L=257, N=2, dpg=4, G=4, dtype=F16, fam="mamba", fv=2),
    C("fwd3_even", _gen(lpr=32), _bwd(8, True, True), L=392, fam="long", fv=3, bv=1),
    C("fwd3_odd", _gen(lpr=32, nu=1), _bwd(8, False, False), L=257, N=15, fam="long", fv=3, bv=1),
    C("fwd4_even", _gen(lpr=64), _bwd(4, True, False), B=1, L=520, N=32, fam="long", fv=4),
    C("fwd4_odd", _gen(lpr=64, nu=1), _bwd(8, True, False), B=1, L=520, N=17, dtype=BF16, fam="long", fv=4, bv=1),
    C("fwd5_even", _gen(w=2), _bwd(4, True, False), L=128, N=8, fam="edges", fv=5),
    C("fwd5_odd", _gen(w=2, nu=1), _bwd(8, False, False), L=127, N=3, dpg=40, fam="mamba", fv=5, bv=1),
    C("fwd6_even", _gen(w=8), _bwd(4, False, False), B=1, L=257, N=64, dpg=40, fam="long", fv=6, bv=2),
    C("fwd6_odd", _gen(w=8, nu=1), _bwd(4, True, False), L=136, N=15, dpg=96, ratio=3, dtype=F16, fv=6),
    C("fwd7_even", _gen(T=16), _bwd(4, True, True), L=392, dpg=40, fam="mamba", fv=7, bv=2),
    C("fwd7_n1_gated", _gen(T=16, nu=1), _bwd(4, True, False), L=520, N=1, dpg=64, fam="long", fv=7),
    C("fwd8", _gen(nu=1, occ=4), _bwd(4, True, False), L=136, N=8, Dv=False, fv=8),
    C("fwd9_even", _gen(occ=3), _bwd(4, True, False), L=136, N=2, bias=False, fv=9),
    C("fwd9_odd", _gen(nu=1, occ=4), _bwd(4, True, False), L=136, N=3, softplus=False, fv=9),
    # an id the switch does not know: the one-wave instantiation nothing else launches
    C("fwd_w1_even", _gen(w=1), _bwd(4, True, False), L=136, N=2, dpg=4, G=2, fv=99),
    C("fwd_w1_odd", _gen(w=1, nu=1), _bwd(4, False, False), B=1, L=7, N=3, fv=99),
    # automatic picks at small sizes: rows of at most 128 steps stream, longer ones spread over 32 / 64 lanes
    C("auto_L8", _stream(4, 2), _bwd(4, True, True), B=3, L=8),
    C("auto_L1", _stream(4, 2, False), _bwd(4, False, True), L=1),
    C("auto_L129_edges", _gen(lpr=32), _bwd(4, False, True), L=129, fam="edges"),
    C("auto_L520_N32", _gen(lpr=64), _bwd(4, True, False), B=1, L=520, N=32, dtype=F16, **NOZ),
    C("auto_N17_L128", _gen(), _bwd(4, True, False), L=128, N=18, dpg=40),
    C("auto_N17", _gen(nu=1), _bwd(4, True, False), L=128, N=17, dpg=40, G=2, dtype=BF16),
    # options off one at a time, delta channel groups, the fp32-out mode
    C("ratio4", _gen(lpr=32), _bwd(4, True, True), L=136, dpg=96, ratio=4, fam="mamba", fv=3),
    C("ratio3_bf16", _stream(4, 2), _bwd(4, True, True), L=128, dpg=96, ratio=3, dtype=BF16),
    C("out_f32_bf16", _stream(4, 2), _bwd(8, True, True), L=136, dpg=64, dtype=BF16, out_f32=True, fv=14, bv=1),
    C("out_f32_fp16_scalar", _gen(lpr=64), _bwd(4, False, False), L=257, N=8, dtype=F16, out_f32=True, fam="long"),
    C("plain", _stream(4, 2), _bwd(4, True, True), L=128, z=False, Dv=False, bias=False, softplus=False),
    # rows by LDS-DMA in the backward: 16-bit, eight waves, dstate 16, whole 8-step lanes
    C("bwd_dma_bf16", _stream(8, 3), _bwd(8, True, True, dma=True), L=392, dpg=40, dtype=BF16, fam="long", fv=12, bv=1),
    C("bwd_dma_fp16", _gen(lpr=32), _bwd(8, True, True, dma=True), L=136, dpg=64, G=2, dtype=F16, fam="edges", bv=1),
    C("bwd_w8_L4_bf16", _gen(lpr=32), _bwd(8, False, True), L=132, dtype=BF16, bv=1),       # rows only 8-byte aligned
    C("bwd_w4_bf16", _stream(4, 2), _bwd(4, True, True), L=128, dtype=BF16, fam="mamba", bv=2),
    # enough 32-row tiles for the eight-wave backward (256), at the last dstate whose 32 parked rows fit the LDS and the first that
    # does not: the dispatch goes back to four waves there (it used to refuse the call); so does a forced eight-wave walk
    C("bwd_wide_N19", _gen(nu=1), _bwd(8, True, False), L=4, N=19, dpg=32, G=128),
    C("bwd_wide_N20", _gen(), _bwd(4, True, False), L=4, N=20, dpg=32, G=128),
    C("bwd_wide_N40_bf16", _gen(), _bwd(8, True, False), L=8, N=40, dpg=32, G=128, dtype=BF16),
    C("bwd_wide_N42_bf16", _gen(), _bwd(4, True, False), L=8, N=42, dpg=32, G=128, dtype=BF16, **NOZ),
    C("bwd_w8_forced_N64", _gen(), _bwd(4, True, False), B=1, L=8, N=64, bv=1),
    C("pk15", _stream(4, 2, pk=True), _bwd(4, True, True), L=136, dtype=BF16, fv=15),
    C("pk16", _stream(8, 3, pk=True), _bwd(4, True, True), L=392, dpg=40, fam="long", fv=16),
    C("pk17", _stream(4, 3, pk=True), _bwd(4, True, True), L=128, dtype=F16, fam="edges", fv=17),
    C("pk18", _stream(8, 2, pk=True), _bwd(4, True, True), L=520, B=1, dpg=64, G=2, fam="mamba", fv=18),
    # the batch folded into the sequence
    C("fold_5x200", _stream(4, 2, fold=True), _bwd(4, True, True, fold=True), B=5, L=200, fold=True, fam="long"),
    C("fold_7x8_bf16", _stream(4, 2, fold=True, pk=True), _bwd(8, True, True, fold=True, dma=True), B=7, L=8, dpg=32, dtype=BF16,
      fold=True, bv=1),
    C("fold_3x104_w8", _stream(4, 2, fold=True), _bwd(8, True, True, fold=True), B=3, L=104, dpg=64, fold=True, bv=1, fam="edges"),
    C("fold_3x104_pk", _stream(4, 2, fold=True, pk=True), _bwd(4, True, True, fold=True), B=3, L=104, G=2, fold=True, fv=15),
    C("fold_5x200_fp16", _stream(4, 2, fold=True, pk=True), _bwd(4, True, True, fold=True), B=5, L=200, dpg=40, dtype=F16, fold=True),
    # the folded forward's eight-wave walks: 512 tiles, reached with 512 groups of four channels
    C("fold_w8", _stream(8, 3, fold=True), _bwd(4, True, True, fold=True), B=2, L=8, dpg=4, G=512, fold=True),
    C("fold_w8_pk", _stream(8, 2, fold=True, pk=True), _bwd(4, True, True, fold=True), B=2, L=8, dpg=4, G=512, dtype=BF16, fold=True),
    # dstate 1 without z: the flat-row kernels, two passes at T = 4 (L > 256) and T = 8 (L > 512), the fp32 dout forms
    C("n1_T4", N1F.format(4), "scan_n1_bwd<T4>", L=136, N=1, G=2, **NOZ),
    C("n1_T4_two_passes", N1F.format(4), "scan_n1_bwd<T4>", L=260, N=1, dpg=40, dtype=F16, fam="long", **NOZ),
    C("n1_T8_two_passes", N1F.format(8), "scan_n1_bwd<T8>", L=520, N=1, dpg=40, dtype=BF16, fam="long", **NOZ),
    C("n1_L8", N1F.format(8), "scan_n1_bwd<T8>", B=3, L=8, N=1, dpg=4, G=4, dtype=F16, **NOZ),
    C("n1_L128_edges", N1F.format(4), "scan_n1_bwd<T4>", L=128, N=1, dpg=96, fam="edges", **NOZ),
    C("n1_ratio4_mamba", N1F.format(4), "scan_n1_bwd<T4>", L=392, N=1, ratio=4, fam="mamba", **NOZ),
    C("n1_T8_dout_f32", N1F.format(8), "scan_n1_bwd<T8,dout_f32>", L=136, N=1, dtype=BF16, out_f32=True, **NOZ),
    C("n1_T4_dout_f32", N1F.format(4), "scan_n1_bwd<T4,dout_f32>", L=260, N=1, dtype=F16, out_f32=True, ratio=3, **NOZ),
    C("n1_general_fwd", _gen(w=1, nu=1), "scan_n1_bwd<T4>", L=128, N=1, fv=30, **NOZ),
    C("n1_general_bwd", N1F.format(4), _bwd(4, True, False), L=128, N=1, bv=3, **NOZ),
    # dstate 1, short rows the flat-row kernels cannot take: a lane per row, one or two waves by the LDS a wave needs
    C("n1_short_L7", N1S, "scan_n1_short_bwd<W2>", L=7, N=1, dpg=64, **NOZ),
    C("n1_short_L1", N1S, "scan_n1_short_bwd<W2>", B=1, L=1, N=1, dpg=64, **NOZ),
    C("n1_short_L63", N1S, "scan_n1_short_bwd<W1>", L=63, N=1, dpg=64, G=2, fam="edges", **NOZ),
    C("n1_short_bf16", N1S, "scan_n1_short_bwd<W1>", L=99, N=1, dpg=64, dtype=BF16, fam="long", **NOZ),
    C("n1_short_fwd_only", N1S, _bwd(4, False, False), L=127, N=1, dpg=64, dtype=BF16, fam="long", **NOZ),   # 64 rows x 127 steps: the backward's LDS is short
    C("n1_short_f32out_w2", N1S, "scan_n1_short_bwd<W2,dout_f32>", L=7, N=1, dpg=64, dtype=BF16, out_f32=True, **NOZ),
    C("n1_short_f32out_w1", N1S, "scan_n1_short_bwd<W1,dout_f32>", L=65, N=1, dpg=64, dtype=F16, out_f32=True, **NOZ),
]
# the streaming forward (scan_fwd_stream.h): every (waves, occupancy) id, vector and element-wise rows, compile-time and run-time state
# count; dtype, family, backward waves and the shape rotate
for _i, (_fv, _w, _occ) in enumerate(((10, 4, 3), (12, 8, 3), (14, 4, 2), (20, 8, 2))):
    for _j, (_N, _L) in enumerate(((16, (128, 520)[_i % 2]), (16, (129, 7)[_i % 2]), ((8, 2, 3, 15)[_i], (136, 392)[_i % 2]),
                                   ((3, 8, 15, 2)[_i], (127, 257)[_i % 2]))):
        _vec, _dt, _bv = _L % 4 == 0, (F32, BF16, F16)[(_i + _j) % 3], (0, 1, 2)[(_i + _j) % 3]
        CASES.append(C(f"stream{_fv}_{'vec' if _vec else 'scalar'}_N{_N}", _stream(_w, _occ, _vec),
                       _bwd(8 if _bv == 1 else 4, _vec, _N == 16, dma=_bv == 1 and _vec and _N == 16 and _dt != F32 and _L % 8 == 0),
                       B=1 + (_i + _j) % 3, L=_L, N=_N, dpg=(24, 40, 4, 64)[_j], G=(1, 2)[_i % 2], dtype=_dt,
                       fam=FAMILIES[(_i + _j) % 3], fv=_fv, bv=_bv, **(NOZ if _j == 3 else {})))
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES), sorted(c.name for c in CASES if sum(d.name == c.name for d in CASES) > 1)

# every instantiation mxvl_scan_fwd's and mxvl_scan_bwd's dispatch can launch, read off dispatch_fwd / try_n1_fwd / try_n1_short_fwd
# (scan_fwd.hip) and dispatch_bwd / launch_bwd / try_n1_bwd / try_n1_short_bwd (scan_bwd.hip).  Forward stream kernels exist with the
# state count at compile time (/N16) and at run time (/Nrt) under one name
ALL_PATHS = (
    [_gen(T, lpr, w, nu) for T, lpr, w in ((8, 16, 4), (8, 32, 4), (8, 64, 4), (8, 16, 2), (8, 16, 8), (16, 16, 4), (8, 16, 1)) for nu in (2, 1)]
    + [_gen(nu=1, occ=4), _gen(occ=3)]
    + [_stream(w, occ, vec) + ns for w, occ in ((4, 3), (8, 3), (4, 2), (8, 2)) for vec in (True, False) for ns in ("/N16", "/Nrt")]
    + [_stream(w, occ, pk=True) for w, occ in ((4, 2), (8, 3), (4, 3), (8, 2))]
    + [_stream(8, 2, fold=True, pk=True), _stream(4, 2, fold=True, pk=True), _stream(8, 3, fold=True), _stream(4, 2, fold=True)]
    + [N1F.format(4), N1F.format(8), N1S]
    + [_bwd(w, vec, n16) for w in (4, 8) for vec in (True, False) for n16 in (True, False)]
    + [_bwd(8, True, True, dma=True), _bwd(8, True, True, fold=True, dma=True), _bwd(8, True, True, fold=True), _bwd(4, True, True, fold=True)]
    + [f"scan_n1_bwd<T{T}{f}>" for T in (4, 8) for f in ("", ",dout_f32")]
    + [f"scan_n1_short_bwd<W{w}{f}>" for w in (1, 2) for f in ("", ",dout_f32")]
)
# instantiations no case reaches: name -> (why, the smallest shape that would)
UNREACHED = {}


def test_every_dispatch_path_is_some_cases_expected_kernel():
    assert len(set(ALL_PATHS)) == len(ALL_PATHS)
    covered = {p for c in CASES for p in _path_ids(c)}
    assert covered <= set(ALL_PATHS), f"cases name kernels the dispatch cannot launch: {sorted(covered - set(ALL_PATHS))}"
    missing = [p for p in ALL_PATHS if p not in covered and p not in UNREACHED]
    assert not missing, f"no case runs {missing}"
    assert not [p for p in UNREACHED if p in covered], "a reached path is still listed as unreached"


def test_cases_cover_the_shapes_the_kernels_turn_on():
    """the sizes at which a mechanism exists: one lane's span, one chunk and one past it, an 8-step tail chunk, ragged multi-chunk rows,
    two passes of the dstate-1 kernels; ragged 16- / 32-row tiles, the dstate-1 backward's dpg % 4, the short kernels' 64 | dpg"""
    have = lambda k: {getattr(c, k) for c in CASES}
    assert have("L") >= {1, 7, 8, 127, 128, 129, 136, 257, 392, 520}
    assert have("dpg") >= {4, 24, 40, 64, 96} and have("G") >= {1, 2, 4} and have("B") >= {1, 2, 3}
    assert have("N") >= {1, 2, 3, 8, 15, 16, 17, 32, 64} and have("ratio") >= {1, 3, 4}
    assert {(c.N, c.z) for c in CASES} >= {(1, True), (1, False)}
    assert have("dtype") == {F32, BF16, F16} and have("fam") == set(FAMILIES)
    for k in ("z", "Dv", "bias", "softplus", "out_f32"):
        assert have(k) == {True, False}, k
    assert {(c.B, c.L) for c in CASES if c.fold} >= {(5, 200), (7, 8), (3, 104)}


@gpu
@pytest.mark.parametrize("name", sorted(CASE))
def test_scan_kernels_against_float64(name):
    c = CASE[name]
    _check(c, _run(c))


# ---- 6. layouts: the views the mixers really pass ----------------------------------------------------------------------------------------
# xz      u and z as the halves of one (B, 2 D, L) buffer, du and dz written into the halves of its gradient
# cmajor  channel-major storage (D, B, L) of every (B, D, L) tensor
# xdbl    B and C as row slices of an x_dbl-shaped (B, R + 2 N, L) buffer, dB and dC into the matching slices of a zero-filled fp32 buffer
#         whose other rows must keep the pattern
# ostride out into rows with a pitch
# None of them moves a row off a 16-byte boundary, so the instantiation of the contiguous launch serves them, and the row-local results
# must be the same bits
LAYOUTS = ("xz", "cmajor", "xdbl", "ostride")
LAY_BASE = {
    "general": C("lay_general", _gen(lpr=32), _bwd(4, True, True), L=136, fam="long", fv=3),
    "stream": C("lay_stream", _stream(4, 2), _bwd(8, True, True, dma=True), L=136, dpg=40, dtype=BF16, fv=14, bv=1),
    "n1": C("lay_n1", N1F.format(4), "scan_n1_bwd<T4>", L=136, N=1, **NOZ),
    "fold": C("lay_fold", _stream(4, 2, fold=True), _bwd(4, True, True, fold=True), B=3, L=104, fold=True, fam="long"),
}


@functools.lru_cache(maxsize=None)
def _base_run(kind, table="lay"):
    c = (LAY_BASE if table == "lay" else AL_BASE)[kind]
    r = _run(c)
    _check(c, r)
    return r


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", sorted(LAY_BASE))
def test_scan_layouts(kind, layout):
    c = LAY_BASE[kind]
    r = _run(c, layout=layout)
    _check(c, r)
    _same_bits(f"{c.name} {layout}", _base_run(kind), r)


# ---- 7. alignment: the contract of include/mxvl.h --------------------------------------------------------------------------------------
# Which tensors' rows the general kernels move in vectors, as the header states it: every io tensor on 4-element boundaries, and for the
# 16-bit dtypes the rows read eight at a time on 16-byte boundaries (forward: u, delta, z; backward: those, dout, and B / C, which travel
# by LDS-DMA).  A direction whose tensor is off takes the element-wise instantiation; the other direction does not care.
FWD_V4, FWD_V16B = {"u", "delta", "z", "B", "C", "out"}, {"u", "delta", "z"}
BWD_V4, BWD_V16B = {"u", "delta", "z", "B", "C", "dout", "du", "ddelta", "dz"}, {"u", "delta", "z", "B", "C", "dout"}
N1_ROWS = {"u", "delta", "B", "C"}                              # what the dstate-1 kernels need aligned to be taken at all
AL_BASE = {
    "fp32": C("al_fp32", _stream(4, 2), _bwd(4, True, True), L=136, fv=14),
    "bf16": C("al_bf16", _stream(4, 2), _bwd(8, True, True, dma=True), L=136, dpg=40, dtype=BF16, fam="long", fv=14, bv=1),
    "fp16": C("al_fp16", _stream(4, 2), _bwd(4, True, True), L=136, dtype=F16, fam="mamba", fv=14, bv=2),     # 16-bit rows, no LDS-DMA
    "n1_fp32": C("al_n1_fp32", N1F.format(4), "scan_n1_bwd<T4>", L=136, N=1, **NOZ),
    "n1_bf16": C("al_n1_bf16", N1F.format(8), "scan_n1_bwd<T8>", L=136, N=1, dtype=BF16, **NOZ),
}


def _names_when_shifted(c, shifts):
    """the kernels the header's rule sends a launch with these shifted views to"""
    sixteen = c.dtype != F32
    off4 = {k for k, s in shifts.items() if s % 4}
    off8 = {k for k, s in shifts.items() if s % 8}
    fvec = not (off4 & FWD_V4) and not (sixteen and off8 & FWD_V16B)
    bvec = not (off4 & BWD_V4) and not (sixteen and off8 & BWD_V16B)
    if c.N == 1 and not c.z:
        T = 0 if off4 & N1_ROWS else (4 if off8 & N1_ROWS or not sixteen else 8)
        # off the 4-element boundary the general kernels serve: L = 136 rows of a small problem spread over 32 lanes (scan_fwd.hip)
        return (N1F.format(T) if T else _gen(lpr=32, nu=1)), (f"scan_n1_bwd<T{T}>" if T else _bwd(4, False, False))
    w = 8 if c.bv == 1 else 4
    return _stream(4, 2, fvec), _bwd(w, bvec, True, dma=bvec and sixteen and w == 8)


def _scalar_twin(a, b):
    """the same general instantiation but for the row access (and the LDS-DMA that rides on it): the header promises the same results"""
    norm = lambda n: n.replace(",scalar", ",vec").replace(",dma", "")
    return norm(a) == norm(b)


def _shifted(kind, shifts):
    c = AL_BASE[kind]
    base = _base_run(kind, "al")
    r = _run(c, shifts=shifts)
    want = _names_when_shifted(c, shifts)
    assert (r.fwd, r.bwd) == want, f"{c.name} {shifts}: launched {r.fwd} / {r.bwd}, the header's rule says {want}"
    _check(c, r, names=False)
    if _scalar_twin(r.fwd, base.fwd):
        _same_bits(f"{c.name} {shifts} forward", base, r, ("out", "last", "ckpt"))
    if _scalar_twin(r.bwd, base.bwd):
        _same_bits(f"{c.name} {shifts} backward", base, r, ("du", "ddelta", "dz"))


def _al_params():
    for kind, c in AL_BASE.items():
        for name in IO_NAMES:
            if c.z or name not in ("z", "dz"):
                yield pytest.param(kind, name, id=f"{kind}-{name}")


@gpu
@pytest.mark.parametrize("kind,tensor", list(_al_params()))
def test_scan_one_tensor_off_the_vector_boundary(kind, tensor):
    """fp32: 1 and 2 elements; 16-bit: 1 and 4 elements, the header's 8-byte case.  For the dstate-1 kernels the shifts of out, dout,
    du and ddelta are the ones that flip out_vec, do_vec, du_vec and dd_vec one at a time"""
    for s in ((1, 2) if AL_BASE[kind].dtype == F32 else (1, 4)):
        _shifted(kind, {tensor: s})


@gpu
@pytest.mark.parametrize("kind", sorted(AL_BASE))
def test_scan_every_tensor_off_the_vector_boundary(kind):
    c = AL_BASE[kind]
    for s in ((1, 2) if c.dtype == F32 else (1, 4)):
        _shifted(kind, {k: s for k in IO_NAMES if c.z or k not in ("z", "dz")})


@gpu
@pytest.mark.parametrize("dtype,shift", [(F32, 1), (F32, 2), (BF16, 1), (BF16, 4)], ids=["fp32-1", "fp32-2", "bf16-1", "bf16-4"])
def test_scan_fold_is_refused_on_views_off_the_vector_boundary(dtype, shift):
    """a fold request on views the folded walks cannot move in vectors.  16-bit rows 4 elements (8 bytes) off: u / delta / z are read 16
    bytes at a time and refuse in the forward, B / C travel by LDS-DMA in the backward only and refuse there, out / du / ddelta / dz move
    in 8-byte vectors in both and still fold -- those launches are checked like any other"""
    c = C("fold_shifted", _stream(4, 2, fold=True, pk=dtype != F32), _bwd(4, True, True, fold=True), B=3, L=104, dtype=dtype, fold=True)
    half = dtype != F32 and shift == 4
    fwd_refuses = ("u", "delta", "z") if half else ("u", "delta", "z", "B", "C", "out")
    bwd_refuses = ("B", "C", "dout") if half else ("dout", "du", "ddelta", "dz")
    for name in fwd_refuses:
        r = _run(c, shifts={name: shift}, expect_rc=-7)
        assert r.bwd is None, "the forward itself must refuse"
    for name in bwd_refuses:
        r = _run(c, shifts={name: shift}, expect_rc=-7)
        assert r.fwd == c.fwd and r.bwd is not None, "the forward folds, the backward must refuse"
    for name in (("out", "du", "ddelta", "dz") if half else ()):
        _check(c, _run(c, shifts={name: shift}))
