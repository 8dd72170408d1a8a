"""Row-wise FP8 weights for the frozen report LLM: `low_resource="fp8"`.

A weight row stores OCP E4M3 codes (torch.float8_e4m3fn: sign | 4 exponent bits, bias 7 | 3 mantissa bits; no infinities, largest
finite value 448, 0x7f / 0xff NaN) and one fp32 scale:

    scale[n] = max_k |W[n][k]| / 448   (fp32)        code[n][k] = rne_e4m3(clamp(W[n][k] / scale[n], -448, 448))

The represented weight is float(code) * scale[n]: the bytes of int8, on the number format gfx950 converts natively.  It is also the
per-channel layout of FP8 checkpoints -- transformers' FbgemmFp8Linear holds `weight` (float8_e4m3fn, (N, K)) and `weight_scale`
(fp32, (N, 1)); those two keys load verbatim, its activation clamp `input_scale_ub` is dropped: activations stay 16-bit here (W8A16).
The decode step reads codes and scales directly (mxvl_decode_gemv with MXVL_W_FP8, csrc/decode_gemm.h decode_gemm_w8f_kernel); prompt
prefill and stage-3 training through the frozen LLM dequantise one weight at a time into the scratch buffer the int8 path uses
(quant_linear.DequantScratch) and run F.linear on it, in eager torch.  What 8-bit float weights cost in report quality is not
measured here."""
from __future__ import annotations

import torch

from ._abi import MXVL_W_FP8
from .quant_linear import QuantLinear, dequant_result

E4M3_MAX = 448.0


def quantize_rowwise_fp8(W):
    """W (N, K) floating -> (codes (N, K) float8_e4m3fn, scale (N, 1) fp32), evaluated in fp32.  An all-zero row gives scale 0 and
    codes +0; no NaN code (0x7f / 0xff) is ever produced: the ratio is clamped before torch's cast (which rounds to nearest, ties to
    even, but answers NaN above 448 instead of saturating), and a non-finite weight raises."""
    Wf = W.detach().float()
    amax = Wf.abs().amax(dim=1, keepdim=True)
    if not bool(torch.isfinite(amax).all()):
        raise ValueError("quantize_rowwise_fp8: the weight holds inf or NaN")
    scale = amax / E4M3_MAX
    ratio = torch.where(scale > 0, Wf / scale, torch.zeros_like(Wf))
    return ratio.clamp_(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn), scale


def dequantize_rowwise_fp8(codes, scale, dtype, out=None):
    """dtype(codes.float() * scale), written into `out` (a flat buffer of at least N * K elements of `dtype`) when given."""
    return dequant_result(codes.float() * scale.reshape(-1, 1), dtype, out)


class Fp8Linear(QuantLinear):
    """nn.Linear with a frozen row-wise E4M3 weight.  Buffers `weight` (float8_e4m3fn, (N, K)), `weight_scale` (fp32, (N, 1)), optional
    `bias` (activation dtype) -- the state-dict keys of transformers' FbgemmFp8Linear, whose checkpoints load (`input_scale_ub` is
    ignored); a 16-bit or fp32 `weight` in a state dict is quantised on load, codes with a NaN byte are refused."""
    NAME, CODES, SCALES, KIND, W_FLAG, IGNORED_KEYS = "fp8", "weight", "weight_scale", "fp8 e4m3 row-wise", MXVL_W_FP8, ("input_scale_ub",)
    quantize, dequantize_into = staticmethod(quantize_rowwise_fp8), staticmethod(dequantize_rowwise_fp8)

    @staticmethod
    def buffers(N, K):
        return ((N, K), torch.float8_e4m3fn), ((N, 1), torch.float32)

    def _load_from_state_dict(self, state_dict, prefix, *args):
        w = state_dict.get(prefix + "weight")
        if w is not None and w.dtype == torch.float8_e4m3fn and bool(((w.view(torch.uint8) & 0x7f) == 0x7f).any()):
            raise ValueError(f"{prefix[:-1] or type(self).__name__}: the E4M3 codes of `weight` hold NaN bytes (0x7f / 0xff)")
        super()._load_from_state_dict(state_dict, prefix, *args)
