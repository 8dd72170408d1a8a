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
import torch.nn as nn
import torch.nn.functional as F


def quantize_rowwise_int8(W):
    """W (N, K) floating -> (CB (N, K) int8, SCB (N) fp32).  An all-zero row gives SCB = 0, CB = 0 (no NaN); -128 is never produced."""
    Wf = W.detach().float()
    scb = Wf.abs().amax(dim=1)
    ratio = torch.where(scb[:, None] > 0, Wf * 127.0 / scb[:, None], torch.zeros_like(Wf))
    cb = torch.round(ratio).clamp_(-127, 127).to(torch.int8)                 # torch.round: half to even
    return cb, scb


def dequantize_rowwise_int8(cb, scb, dtype, out=None):
    """dtype(CB.float() * (SCB / 127)), written into `out` (a flat buffer of at least N * K elements of `dtype`) when given."""
    w = cb.float() * (scb / 127.0)[:, None]
    if out is None:
        return w.to(dtype)
    view = out[:cb.numel()].view(cb.shape)
    view.copy_(w)
    return view


class DequantScratch:
    """One flat buffer per (dtype, device): every Int8Linear of a decoder writes its dequantised weight here in turn, so the 16-bit
    copy of at most ONE projection exists at a time.  `reserve` (quantize_int8_ calls it with the decoder's largest weight) fixes the
    size before the first use, so the buffer of a (dtype, device) is allocated once and keeps its address -- a step captured in a
    hipGraph (use_graph="torch") never names a buffer that a later, larger weight replaced."""

    def __init__(self):
        self.bufs, self.numel = {}, 0

    def reserve(self, numel):
        self.numel = max(self.numel, numel)

    def get(self, numel, dtype, device):
        self.reserve(numel)
        key = (dtype, str(device))
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < self.numel:
            buf = self.bufs[key] = torch.empty(self.numel, dtype=dtype, device=device)
        return buf


class _Int8LinearFn(torch.autograd.Function):
    """F.linear on the dequantised weight; saves CB / SCB only (never the 16-bit weight), backward re-creates it: dx = dy @ Wdq.  The
    weight gets no gradient."""

    @staticmethod
    def forward(ctx, x, cb, scb, bias, scratch, dtype):
        w = dequantize_rowwise_int8(cb, scb, dtype, scratch.get(cb.numel(), dtype, cb.device))
        ctx.save_for_backward(cb, scb)
        ctx.scratch, ctx.wdtype, ctx.xdtype = scratch, dtype, x.dtype
        return F.linear(x, w, bias)

    @staticmethod
    def backward(ctx, dy):
        cb, scb = ctx.saved_tensors
        w = dequantize_rowwise_int8(cb, scb, ctx.wdtype, ctx.scratch.get(cb.numel(), ctx.wdtype, cb.device))
        dx = (dy.to(ctx.wdtype) @ w).to(ctx.xdtype)
        return dx, None, None, None, None, None


class Int8Linear(nn.Module):
    """nn.Linear with a frozen row-wise int8 weight.  Buffers `weight` (int8, (N, K)), `SCB` (fp32, (N)), optional `bias` (activation
    dtype) -- the state-dict keys of bitsandbytes' Linear8bitLt, whose checkpoints load (its `weight_format` entry is ignored);
    a 16-bit `weight` in a state dict is quantised on load."""

    def __init__(self, in_features, out_features, bias=False, dtype=torch.float16, device=None, scratch=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("weight", torch.zeros(out_features, in_features, dtype=torch.int8, device=device))
        self.register_buffer("SCB", torch.zeros(out_features, dtype=torch.float32, device=device))
        self.register_buffer("bias", torch.zeros(out_features, dtype=dtype, device=device) if bias else None)
        self.scratch = scratch if scratch is not None else DequantScratch()

    @classmethod
    def from_linear(cls, lin: nn.Linear, scratch=None):
        m = cls(lin.in_features, lin.out_features, bias=lin.bias is not None, dtype=lin.weight.dtype, device=lin.weight.device, scratch=scratch)
        cb, scb = quantize_rowwise_int8(lin.weight)
        m.weight, m.SCB = cb, scb
        if lin.bias is not None:
            m.bias = lin.bias.detach().clone()
        return m

    def _apply(self, fn, *args, **kwargs):
        # .to(dtype) / .half() leave the int8 codes alone but would cast the scales: SCB stays fp32 (only the bias follows the activations)
        scb = self.SCB
        super()._apply(fn, *args, **kwargs)
        self.SCB = scb.to(self.SCB.device)
        return self

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        local = {k: state_dict[k] for k in (prefix + "weight", prefix + "SCB", prefix + "bias") if k in state_dict}    # (`weight_format` dropped)
        w = local.get(prefix + "weight")
        if w is not None and w.is_floating_point():
            local[prefix + "weight"], local[prefix + "SCB"] = quantize_rowwise_int8(w)
        super()._load_from_state_dict(local, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def dequantized(self, dtype):
        """A fresh dtype(CB.float() * (SCB / 127)) tensor (tests, export)."""
        return dequantize_rowwise_int8(self.weight, self.SCB, dtype)

    def forward(self, x):
        dev = x.device.type
        dt = torch.get_autocast_dtype(dev) if torch.is_autocast_enabled(dev) else x.dtype
        return _Int8LinearFn.apply(x, self.weight, self.SCB, self.bias, self.scratch, dt)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, int8 row-wise"
