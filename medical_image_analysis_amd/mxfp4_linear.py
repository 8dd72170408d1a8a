"""OCP microscaling FP4 (MX v1.0, MXFP4) weights for the frozen report LLM: `low_resource="mxfp4"`.

Along K a weight row is cut into blocks of 32.  A block stores one E8M0 scale byte (a power of two, bias 127) and 32 E2M1 codes
(sign | 2 exponent bits | 1 mantissa bit: 0, 0.5, 1, 1.5, 2, 3, 4, 6 and their negatives), two codes per byte with the element of
even k in the low nibble: 4.25 bits per weight.

    X = floor(log2(max_block |w|)) - 2   (clamped to E8M0's -127 .. 127; an all-zero block: X = -127, zero codes)
    code = nearest E2M1 value to w / 2^X, ties to the even mantissa, saturated at +-6

The represented weight value(code) * 2^X is exact in bf16, and in fp16 for X in [-15, 13] (the quantiser refuses an fp16 weight
outside that range).  The decode step reads codes and scales directly (mxvl_decode_gemv with MXVL_W_MXFP4, csrc/decode_gemm.h
decode_gemm_w4_kernel); prompt prefill and stage-3 training through the frozen LLM dequantise one weight at a time into the scratch
buffer the int8 path uses (quant_linear.DequantScratch) and run F.linear on it, in eager torch.  What 4-bit weights cost in report
quality is not measured here."""
from __future__ import annotations

import torch

from ._abi import MXVL_W_MXFP4
from .quant_linear import QuantLinear, dequant_result

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
    return dequant_result(w, dtype, out)


class MxFp4Linear(QuantLinear):
    """nn.Linear with a frozen MXFP4 weight.  Buffers `weight_packed` (uint8, (N, K / 2)), `weight_scale` (uint8 E8M0, (N, K / 32)),
    optional `bias` (activation dtype): the state-dict keys.  A 16-bit `weight` in a state dict is quantised on load."""
    NAME, CODES, SCALES, KIND, W_FLAG = "mxfp4", "weight_packed", "weight_scale", "mxfp4", MXVL_W_MXFP4
    quantize, dequantize_into = staticmethod(quantize_mxfp4), staticmethod(dequantize_mxfp4)

    @staticmethod
    def buffers(N, K):
        if K % BLOCK:
            raise ValueError(f"MXFP4 needs in_features % {BLOCK} == 0, got {K}")
        return ((N, K // 2), torch.uint8), ((N, K // BLOCK), torch.uint8)
