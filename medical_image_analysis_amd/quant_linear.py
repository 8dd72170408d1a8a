"""What the quantised Linear modules of the frozen report LLM share (the classes of weight_formats.WEIGHT_FORMATS): the decode step
reads their codes and scales directly (mxvl_decode_gemv with the class's ABI flag); the multi-token paths -- prompt prefill, stage-3
training through the frozen LLM -- dequantise one weight at a time into a scratch buffer shared by every layer of a decoder and run
F.linear on it: eager torch on purpose, it runs once per generate / training step and layer, not once per token."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F


class DequantScratch:
    """One flat buffer per (dtype, device): every quantised Linear of a decoder writes its dequantised weight here in turn, so the
    16-bit copy of at most ONE projection exists at a time.  `reserve` (quantize_int8_ calls it with the decoder's largest weight) fixes
    the size before the first use, so the buffer of a (dtype, device) is allocated once and keeps its address -- a step captured in a
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


def dequant_result(w, dtype, out=None):
    """The tail of every dequantiser: the fp32 (N, K) weight `w` as `dtype`, written into the head of `out` (a flat buffer of at least
    N * K elements of `dtype`) when given."""
    if out is None:
        return w.to(dtype)
    view = out[:w.numel()].view(w.shape)
    view.copy_(w)
    return view


class _QuantLinearFn(torch.autograd.Function):
    """F.linear on the dequantised weight; saves codes and scales only (never the 16-bit weight), backward re-creates it:
    dx = dy @ Wdq.  The weight gets no gradient."""

    @staticmethod
    def forward(ctx, x, codes, scales, bias, dequant, dtype):
        w = dequant(codes, scales, dtype)                 # (the module's: into its scratch buffer)
        ctx.save_for_backward(codes, scales)
        ctx.dequant, ctx.wdtype, ctx.xdtype = dequant, dtype, x.dtype
        return F.linear(x, w, bias)

    @staticmethod
    def backward(ctx, dy):
        w = ctx.dequant(*ctx.saved_tensors, ctx.wdtype)
        dx = (dy.to(ctx.wdtype) @ w).to(ctx.xdtype)
        return dx, None, None, None, None, None


class QuantLinear(nn.Module):
    """nn.Linear with a frozen quantised weight.  A subclass declares
        CODES, SCALES       the names of its two buffers (its state-dict keys beside `bias`)
        NAME                its name in weight_formats.WEIGHT_FORMATS (and as a `low_resource` value)
        W_FLAG              the weight-format bit of mxvl_gemv_desc.dtype its buffers are read with
        K_MULTIPLE          what the decode kernel of the format needs every in_features to be a multiple of
        KIND                the word of extra_repr
        buffers(N, K)       -> (codes, scales) shapes and dtypes as (shape, dtype) pairs
        quantize(W)         -> (codes, scales);  dequantize_into(codes, scales, dtype, out=None) -> (N, K) weight
    A 16-bit `weight` in a state dict is quantised on load."""
    CODES = SCALES = KIND = NAME = None
    W_FLAG, K_MULTIPLE = 0, 64
    IGNORED_KEYS = ()               # state-dict entries of a foreign checkpoint format that are dropped on load

    def __init__(self, in_features, out_features, bias=False, dtype=torch.float16, device=None, scratch=None):
        super().__init__()
        self.in_features, self.out_features, self.wdtype = in_features, out_features, dtype
        for name, (shape, dt) in zip((self.CODES, self.SCALES), self.buffers(out_features, in_features)):
            self.register_buffer(name, torch.zeros(shape, dtype=dt, device=device))
        self.register_buffer("bias", torch.zeros(out_features, dtype=dtype, device=device) if bias else None)
        self.scratch = scratch if scratch is not None else DequantScratch()

    @property
    def codes(self):
        return getattr(self, self.CODES)

    @property
    def scales(self):
        return getattr(self, self.SCALES)

    def set_quantized(self, codes, scales):
        setattr(self, self.CODES, codes)
        setattr(self, self.SCALES, scales)

    @classmethod
    def from_linear(cls, lin: nn.Linear, scratch=None):
        codes, scales = cls.quantize(lin.weight)                         # (before anything is built: a weight the format refuses raises here)
        m = cls(lin.in_features, lin.out_features, bias=lin.bias is not None, dtype=lin.weight.dtype, device=lin.weight.device, scratch=scratch)
        m.set_quantized(codes, scales)
        if lin.bias is not None:
            m.bias = lin.bias.detach().clone()
        return m

    def _apply(self, fn, *args, **kwargs):
        # .to(dtype) / .half() / .float() cast every floating buffer, and scales (fp8: the codes too) are floating: both buffers come
        # through with their bits (moved to the new device), only the bias follows the activations
        codes, scales = self.codes, self.scales
        super()._apply(fn, *args, **kwargs)
        self.set_quantized(codes.to(self.codes.device), scales.to(self.scales.device))
        return self

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        local = {k: v for k, v in state_dict.items() if k.startswith(prefix) and k[len(prefix):] not in self.IGNORED_KEYS}
        w = local.get(prefix + "weight")
        if w is not None and w.is_floating_point() and w.dtype != self.codes.dtype:       # (floating codes -- fp8 -- load as they are)
            del local[prefix + "weight"]
            local[prefix + self.CODES], local[prefix + self.SCALES] = self.quantize(w)
        super()._load_from_state_dict(local, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def _scratch_weight(self, codes, scales, dtype):
        numel = self.in_features * self.out_features
        return self.dequantize_into(codes, scales, dtype, self.scratch.get(numel, dtype, codes.device))

    def dequantize(self, dtype=None):
        """A fresh (N, K) tensor of the represented weights (tests, export), in `dtype` (default: the 16-bit type the module was built for)."""
        return self.dequantize_into(self.codes, self.scales, self.wdtype if dtype is None else dtype)

    def forward(self, x):
        dev = x.device.type
        dt = torch.get_autocast_dtype(dev) if torch.is_autocast_enabled(dev) else x.dtype
        return _QuantLinearFn.apply(x, self.codes, self.scales, self.bias, self._scratch_weight, dt)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, {self.KIND}"
