"""Row-wise absmax int8 weights for the frozen report LLM -- the storage of the reference's `--low_resource`
(CXPMRG_Bench_MambaXray_VL/configs/config.py:31; models/MambaXrayVL_DownStream.py:82-92 loads the LLM with load_in_8bit=True, i.e.
bitsandbytes' Linear8bitLt / Int8Params):

    SCB[n] = max_k |W[n][k]|   (fp32)        CB[n][k] = round_half_even(W[n][k] * 127 / SCB[n])   (int8)

The represented weight is CB[n][k] * SCB[n] / 127.  The decode step reads CB / SCB directly (mxvl_decode_gemv with MXVL_W_INT8,
csrc/decode_gemm.h); the multi-token paths -- prompt prefill, stage-3 training through the frozen LLM -- dequantise one weight at a
time into a scratch buffer shared by every layer of a decoder and run F.linear on it: eager torch on purpose, it runs once per
generate / training step and layer, not once per token.  Activations stay 16-bit (W8A16): bitsandbytes' LLM.int8() also quantises
the activations row-wise and routes outlier columns through fp16; same weight format here, more accurate arithmetic, no token
parity with a bitsandbytes run claimed."""
from __future__ import annotations

import torch

from ._abi import MXVL_W_INT8
from .quant_linear import DequantScratch, QuantLinear, dequant_result      # (DequantScratch: re-exported, it used to live here)


def quantize_rowwise_int8(W):
    """W (N, K) floating -> (CB (N, K) int8, SCB (N) fp32).  An all-zero row gives SCB = 0, CB = 0 (no NaN); -128 is never produced."""
    Wf = W.detach().float()
    scb = Wf.abs().amax(dim=1)
    ratio = torch.where(scb[:, None] > 0, Wf * 127.0 / scb[:, None], torch.zeros_like(Wf))
    cb = torch.round(ratio).clamp_(-127, 127).to(torch.int8)                 # torch.round: half to even
    return cb, scb


def dequantize_rowwise_int8(cb, scb, dtype, out=None):
    """dtype(CB.float() * (SCB / 127)), written into `out` (a flat buffer of at least N * K elements of `dtype`) when given."""
    return dequant_result(cb.float() * (scb / 127.0)[:, None], dtype, out)


class Int8Linear(QuantLinear):
    """nn.Linear with a frozen row-wise int8 weight.  Buffers `weight` (int8, (N, K)), `SCB` (fp32, (N)), optional `bias` (activation
    dtype) -- the state-dict keys of bitsandbytes' Linear8bitLt, whose checkpoints load (its `weight_format` entry is ignored);
    a 16-bit `weight` in a state dict is quantised on load."""
    NAME, CODES, SCALES, KIND, W_FLAG, IGNORED_KEYS = "int8", "weight", "SCB", "int8 row-wise", MXVL_W_INT8, ("weight_format",)
    quantize, dequantize_into = staticmethod(quantize_rowwise_int8), staticmethod(dequantize_rowwise_int8)

    @staticmethod
    def buffers(N, K):
        return ((N, K), torch.int8), ((N,), torch.float32)
