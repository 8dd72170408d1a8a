"""OCP microscaling FP4 (MX v1.0, MXFP4) weights for the frozen report LLM: `low_resource="mxfp4"`.

Along K a weight row is cut into blocks of 32.  A block stores one E8M0 scale byte (a power of two, bias 127) and 32 E2M1 codes
(sign | 2 exponent bits | 1 mantissa bit: 0, 0.5, 1, 1.5, 2, 3, 4, 6 and their negatives), two codes per byte with the element of
even k in the low nibble: 4.25 bits per weight.

    X = floor(log2(max_block |w|)) - 2   (clamped to E8M0's -127 .. 127; an all-zero block: X = -127, zero codes)
    code = nearest E2M1 value to w / 2^X, ties to the even mantissa, saturated at +-6

The represented weight value(code) * 2^X is exact in bf16, and in fp16 for X in [-15, 13] (the quantiser refuses an fp16 weight
outside that range).  The decode step reads codes and scales directly (mxvl_decode_gemv with MXVL_W_MXFP4, csrc/decode_gemm.h
decode_gemm_w4_kernel); prompt prefill and stage-3 training through the frozen LLM dequantise one weight at a time into the scratch
buffer the int8 path uses (int8_linear.DequantScratch) and run F.linear on it, in eager torch.  What 4-bit weights cost in report
quality is not measured here."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .int8_linear import DequantScratch

BLOCK = 32
FP16_X_RANGE = (-15, 13)                                        # 0.5 * 2^-15 = fp16's 2^-16 (subnormal, exact) .. 6 * 2^13 = 49152


def quantize_mxfp4(W):
    """W (N, K) floating, K % 32 == 0 -> (packed (N, K / 2) uint8, scale (N, K / 32) uint8).  Evaluated in fp32 with exact steps
    only (frexp, ldexp, round-half-even), so the result does not depend on the device.  fp16: ValueError if a non-zero block needs
    X outside [-15, 13], where its elements would not be exact in fp16."""
    N, K = W.shape
    if K % BLOCK:
        raise ValueError(f"MXFP4 needs in_features % {BLOCK} == 0, got {K}")
    Wf = W.detach().float().reshape(N, K // BLOCK, BLOCK)
    amax = Wf.abs().amax(dim=2)
    _, e = torch.frexp(amax)                                                     # amax = m * 2^e, m in [0.5, 1): floor(log2) = e - 1
    X = torch.where(amax > 0, (e - 3).clamp(-127, 127), torch.full_like(e, -127))
    if W.dtype == torch.float16:
        bad = (amax > 0) & ((X < FP16_X_RANGE[0]) | (X > FP16_X_RANGE[1]))
        if bool(bad.any()):
            raise ValueError(f"MXFP4 of an fp16 weight: {int(bad.sum())} block(s) need a scale exponent outside [{FP16_X_RANGE[0]}, {FP16_X_RANGE[1]}] "
                             f"(found {int(X[bad].min())} .. {int(X[bad].max())}); their elements are not exact in fp16 -- use bf16")
    a = torch.ldexp(Wf, -X[:, :, None]).abs()                                    # |w| / 2^X < 8, exact
    # the grid's step is 0.5 below 2, 1 below 4, 2 above; torch.round is half-to-even and an even count of steps is an even code
    mag = torch.where(a < 2, torch.round(a * 2), torch.where(a < 4, 2 + torch.round(a), 4 + torch.round(a * 0.5))).clamp_(max=7).to(torch.uint8)
    code = torch.where((Wf < 0) & (mag > 0), mag | 8, mag).reshape(N, K)
    packed = code[:, 0::2] | (code[:, 1::2] << 4)
    return packed.contiguous(), (X + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4(packed, scale, dtype, out=None):
    """dtype(value(code) * 2^(scale - 127)) as an (N, K) matrix, written into `out` (a flat buffer of at least N * K elements of
    `dtype`) when given."""
    N, K = packed.shape[0], packed.shape[1] * 2
    code = torch.stack((packed & 15, packed >> 4), dim=2).reshape(N, K // BLOCK, BLOCK).int()
    # E2M1 decoded arithmetically (no table to upload: this runs inside captured graphs): m = code & 7 is 0, 0.5 for m < 2, else
    # (1 + (m & 1) / 2) * 2^((m >> 1) - 1); code & 8 is the sign
    m = code & 7
    mag = torch.where(m < 2, 0.5 * m, torch.ldexp(1.0 + 0.5 * (m & 1), (m >> 1) - 1))
    w = torch.ldexp(torch.where(code >= 8, -mag, mag), (scale.int() - 127)[:, :, None]).reshape(N, K)
    if out is None:
        return w.to(dtype)
    view = out[:N * K].view(N, K)
    view.copy_(w)
    return view


class _MxFp4LinearFn(torch.autograd.Function):
    """F.linear on the dequantised weight; saves codes and scales only (never the 16-bit weight), backward re-creates it:
    dx = dy @ Wdq.  The weight gets no gradient."""

    @staticmethod
    def forward(ctx, x, packed, scale, bias, scratch, dtype):
        w = dequantize_mxfp4(packed, scale, dtype, scratch.get(packed.numel() * 2, dtype, packed.device))
        ctx.save_for_backward(packed, scale)
        ctx.scratch, ctx.wdtype, ctx.xdtype = scratch, dtype, x.dtype
        return F.linear(x, w, bias)

    @staticmethod
    def backward(ctx, dy):
        packed, scale = ctx.saved_tensors
        w = dequantize_mxfp4(packed, scale, ctx.wdtype, ctx.scratch.get(packed.numel() * 2, ctx.wdtype, packed.device))
        dx = (dy.to(ctx.wdtype) @ w).to(ctx.xdtype)
        return dx, None, None, None, None, None


class MxFp4Linear(nn.Module):
    """nn.Linear with a frozen MXFP4 weight.  Buffers `weight_packed` (uint8, (N, K / 2)), `weight_scale` (uint8 E8M0, (N, K / 32)),
    optional `bias` (activation dtype): the state-dict keys.  A 16-bit `weight` in a state dict is quantised on load."""

    def __init__(self, in_features, out_features, bias=False, dtype=torch.float16, device=None, scratch=None):
        super().__init__()
        if in_features % BLOCK:
            raise ValueError(f"MXFP4 needs in_features % {BLOCK} == 0, got {in_features}")
        self.in_features, self.out_features, self.wdtype = in_features, out_features, dtype
        self.register_buffer("weight_packed", torch.zeros(out_features, in_features // 2, dtype=torch.uint8, device=device))
        self.register_buffer("weight_scale", torch.zeros(out_features, in_features // BLOCK, dtype=torch.uint8, device=device))
        self.register_buffer("bias", torch.zeros(out_features, dtype=dtype, device=device) if bias else None)
        self.scratch = scratch if scratch is not None else DequantScratch()

    @classmethod
    def from_linear(cls, lin: nn.Linear, scratch=None):
        packed, scale = quantize_mxfp4(lin.weight)                       # (before anything is built: an fp16 weight out of range raises here)
        m = cls(lin.in_features, lin.out_features, bias=lin.bias is not None, dtype=lin.weight.dtype, device=lin.weight.device, scratch=scratch)
        m.weight_packed, m.weight_scale = packed, scale
        if lin.bias is not None:
            m.bias = lin.bias.detach().clone()
        return m

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        w = state_dict.get(prefix + "weight")
        if w is not None and w.is_floating_point():
            state_dict = {k: v for k, v in state_dict.items() if k != prefix + "weight"}
            state_dict[prefix + "weight_packed"], state_dict[prefix + "weight_scale"] = quantize_mxfp4(w)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def dequantize(self, dtype=None):
        """A fresh (N, K) tensor of the represented weights Wdq, exact in `dtype` (default: the 16-bit type the module was built for)."""
        return dequantize_mxfp4(self.weight_packed, self.weight_scale, self.wdtype if dtype is None else dtype)

    def forward(self, x):
        dev = x.device.type
        dt = torch.get_autocast_dtype(dev) if torch.is_autocast_enabled(dev) else x.dtype
        return _MxFp4LinearFn.apply(x, self.weight_packed, self.weight_scale, self.bias, self.scratch, dt)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, mxfp4"
