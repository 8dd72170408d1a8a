"""Group-wise int4 weights for the frozen report LLM, in the arithmetic of GPTQ checkpoints: `low_resource="int4"`, and the format
`build_report_decoder(<a GPTQ checkpoint directory>)` decodes in.

Along K a weight row is cut into groups of 128.  A group stores one fp16 scale s, one zero point z in 0..15 and 128 unsigned 4-bit
codes q in 0..15; the represented weight is

    w[n][k] = dtype_rne( float(s[n][k / 128]) * (q[n][k] - z[n][k / 128]) )

-- the product is exact in fp32 and rounded once to the decoder's 16-bit dtype (fp16: GPTQ's own `scales * (q - zeros)`): 4.25 bits
per weight.  Buffers (include/mxvl.h MXVL_W_INT4):

    qcodes       (N, K / 2) uint8: the eight codes of columns 8 i .. 8 i + 7 are one little-endian 32-bit word, the code of column
                 8 i + e in nibble (e >> 1) + 4 * (e & 1) (bytes e0 | e2 << 4, e4 | e6 << 4, e1 | e3 << 4, e5 | e7 << 4): the order in
                 which the decode kernel lifts pairs of codes straight into packed 16-bit operands
    qscale_zero  (N, K / 128) int32: fp16 bits of s | z << 16

A GPTQ state dict (`qweight` / `qzeros` / `scales` / optional `g_idx`, `bias`; 4 bits, group size 128, no act-order) is repacked
once on load; a 16-bit `weight` is quantised on load (round to nearest, asymmetric: quantize_int4).  The decode step reads codes and
scales directly (mxvl_decode_gemv with MXVL_W_INT4, csrc/decode_gemm.h decode_gemm_w4i_kernel); prompt prefill and stage-3 training
through the frozen LLM dequantise one weight at a time into the scratch buffer the int8 path uses (quant_linear.DequantScratch) and
run F.linear on it, in eager torch.  The report quality of real GPTQ checkpoints is not measured here."""
from __future__ import annotations

import torch

from ._abi import MXVL_W_INT4
from .quant_linear import QuantLinear, dequant_result

GROUP = 128
FP16_MAX = 65504.0
FP16_TINY = 2.0 ** -24                                          # the smallest fp16 subnormal
_NIBBLE_OF = tuple((e >> 1) + 4 * (e & 1) for e in range(8))    # column 8 i + e -> nibble of the word
GPTQ_KEYS = ("qweight", "qzeros", "scales", "g_idx")


def pack_int4(q, z, s):
    """q (N, K) codes 0..15, z (N, K / 128) zero points 0..15, s (N, K / 128) fp16 scales -> (qcodes, qscale_zero)."""
    N, K = q.shape
    q8 = q.reshape(N, K // 8, 8).to(torch.int32)
    word = torch.zeros(N, K // 8, dtype=torch.int32, device=q.device)
    for e in range(8):
        word |= q8[:, :, e] << (4 * _NIBBLE_OF[e])
    codes = word.contiguous().view(torch.uint8).reshape(N, K // 2)            # little-endian bytes of the words
    sz = s.to(torch.float16).contiguous().view(torch.int16).to(torch.int32) & 0xffff
    return codes.contiguous(), (sz | (z.to(torch.int32) << 16)).contiguous()


def unpack_int4(codes, scales):
    """(qcodes, qscale_zero) -> (q (N, K) int32, z (N, K / 128) int32, s (N, K / 128) fp16): the inverse of pack_int4.  Arithmetic
    ops and views only (no table, no host read)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    b = codes.reshape(N, K // 8, 4).to(torch.int32)
    nib = torch.stack((b & 15, b >> 4), dim=3).reshape(N, K // 8, 2, 4)       # nibbles 0..7 of a word as [odd column?][pair]
    q = nib.transpose(2, 3).reshape(N, K)                                     # column 2 p + h of the word = nibble p + 4 h
    half = scales.contiguous().view(torch.int16).reshape(N, K // GROUP, 2)    # (low, high) halves of the little-endian words
    return q, half[:, :, 1].to(torch.int32), half[:, :, 0].contiguous().view(torch.float16)


def quantize_int4(W):
    """W (N, K) floating, K % 128 == 0 -> (qcodes, qscale_zero): round-to-nearest asymmetric quantisation per group of 128 along K,
    over a range that always holds zero.  Evaluated in fp32, every step one IEEE operation (or exact), rounding half to even:
        lo = min(min_g, 0), hi = max(max_g, 0);  s = fp16((hi - lo) / 15);  z = clamp(round(-lo / s), 0, 15)
        q = clamp(round(w / s) + z, 0, 15)
    An all-zero group gives s = 1, z = 0, q = 0; any other group whose scale rounds to zero takes fp16's smallest subnormal.
    ValueError: K % 128 != 0, a scale that is not finite in fp16, and for an fp16 weight 15 s > 65504 (an element could overflow)."""
    N, K = W.shape
    if K % GROUP:
        raise ValueError(f"int4 (group {GROUP}) needs in_features % {GROUP} == 0, got {K}")
    Wf = W.detach().float().reshape(N, K // GROUP, GROUP)
    lo, hi = Wf.amin(dim=2).clamp(max=0.0), Wf.amax(dim=2).clamp(min=0.0)
    span = hi - lo
    s16 = (span / 15.0).to(torch.float16)
    if not bool(torch.isfinite(s16).all()):
        raise ValueError(f"quantize_int4: a group scale is not finite in fp16 (largest range / 15 = {float((span / 15.0).max())!r})")
    s = s16.float()
    s = torch.where(span > 0, s.clamp(min=FP16_TINY), torch.ones_like(s))
    if W.dtype == torch.float16 and float(s.max()) * 15.0 > FP16_MAX:
        raise ValueError(f"int4 of an fp16 weight: 15 x the largest group scale {float(s.max())!r} exceeds {FP16_MAX}; an element could overflow fp16 -- use bf16")
    z = torch.round(-lo / s).clamp_(0, 15)
    q = (torch.round(Wf / s[:, :, None]) + z[:, :, None]).clamp_(0, 15)
    return pack_int4(q.reshape(N, K).to(torch.int32), z.to(torch.int32), s.to(torch.float16))


def dequantize_int4(codes, scales, dtype, out=None):
    """dtype_rne(float(s) * (q - z)) as an (N, K) matrix -- the element rule of MXVL_W_INT4, bit for bit: the fp32 product is exact
    and the cast rounds once -- written into `out` (a flat buffer of at least N * K elements of `dtype`) when given."""
    N, K = codes.shape[0], codes.shape[1] * 2
    q, z, s = unpack_int4(codes, scales)
    w = ((q - z.repeat_interleave(GROUP, dim=1)).float().reshape(N, K // GROUP, GROUP) * s.float()[:, :, None]).reshape(N, K)
    return dequant_result(w, dtype, out)


def check_gptq_config(qc):
    """The `quantization_config` of a GPTQ checkpoint (or the same keys as keyword defaults) -> the checkpoint format, "gptq" or
    "gptq_v2".  What this build does not decode raises a ValueError that names the value."""
    qc = dict(qc or {})
    if qc.get("quant_method", "gptq") != "gptq":
        raise ValueError(f"quantization_config: quant_method={qc['quant_method']!r}; only 'gptq' checkpoints load as int4")
    if int(qc.get("bits", 4)) != 4:
        raise ValueError(f"GPTQ checkpoint: bits={qc['bits']!r}; only 4-bit checkpoints load (MXVL_W_INT4)")
    if int(qc.get("group_size", GROUP)) != GROUP:
        raise ValueError(f"GPTQ checkpoint: group_size={qc['group_size']!r}; only group_size={GROUP} loads")
    if qc.get("desc_act", False):
        raise ValueError(f"GPTQ checkpoint: desc_act={qc['desc_act']!r} (act-order); the decode kernel needs groups of consecutive input channels")
    fmt = qc.get("checkpoint_format") or "gptq"
    if fmt not in ("gptq", "gptq_v2"):
        raise ValueError(f"GPTQ checkpoint: checkpoint_format={fmt!r}; 'gptq' and 'gptq_v2' load")
    return fmt


def import_gptq(qweight, qzeros, scales, g_idx=None, quantization_config=None):
    """The tensors of one GPTQ QuantLinear -> (qcodes, qscale_zero), exactly (no arithmetic on the values):
        qweight int32 (K / 8, N):    q[k][n] = (qweight[k // 8][n] >> 4 (k % 8)) & 15
        qzeros  int32 (K / g, N / 8): stored = (qzeros[G][n // 8] >> 4 (n % 8)) & 15;  z = (stored + 1) & 15 for checkpoint format
                                      "gptq" (the default), z = stored for "gptq_v2"
        scales  fp16  (K / g, N);    g_idx int32 (K), optional, must be k // g (anything else is act-order)."""
    fmt = check_gptq_config(quantization_config)
    if qweight is None or qzeros is None or scales is None:
        raise ValueError("GPTQ checkpoint: `qweight`, `qzeros` and `scales` must all be present")
    if scales.dtype != torch.float16:
        raise ValueError(f"GPTQ checkpoint: scales are {scales.dtype}; the format holds fp16 scales (they are stored as they are, not converted)")
    K, N = qweight.shape[0] * 8, qweight.shape[1]
    if N % 8:
        raise ValueError(f"GPTQ checkpoint: out_features={N} is not a multiple of 8 (qzeros packs eight columns per word)")
    if K % GROUP:
        raise ValueError(f"GPTQ checkpoint: in_features={K} is not a multiple of group_size={GROUP}")
    G = K // GROUP
    if tuple(qzeros.shape) != (G, N // 8) or tuple(scales.shape) != (G, N):
        raise ValueError(f"GPTQ checkpoint: qweight {tuple(qweight.shape)} needs qzeros {(G, N // 8)} and scales {(G, N)}, "
                         f"got {tuple(qzeros.shape)} and {tuple(scales.shape)}")
    if g_idx is not None:
        gi = g_idx.reshape(-1).long()
        if gi.numel() != K:
            raise ValueError(f"GPTQ checkpoint: g_idx has {gi.numel()} entries, expected in_features={K}")
        bad = (gi != torch.arange(K, device=gi.device) // GROUP).nonzero()
        if bad.numel():
            k = int(bad[0])
            raise ValueError(f"GPTQ checkpoint: g_idx[{k}]={int(gi[k])}, expected {k // GROUP}: a non-trivial g_idx is act-order "
                             "(desc_act), which the decode kernel does not read")
    shifts = torch.arange(0, 32, 4, device=qweight.device, dtype=torch.int32)
    q = ((qweight.to(torch.int32)[:, None, :] >> shifts[None, :, None]) & 15).reshape(K, N).t()            # (N, K)
    stored = ((qzeros.to(torch.int32)[:, :, None] >> shifts[None, None, :]) & 15).reshape(G, N).t()        # (N, G)
    z = (stored + 1) & 15 if fmt == "gptq" else stored
    return pack_int4(q, z, scales.t())


class Int4GroupLinear(QuantLinear):
    """nn.Linear with a frozen group-wise int4 weight.  Buffers `qcodes` (uint8, (N, K / 2)), `qscale_zero` (int32, (N, K / 128)),
    optional `bias` (activation dtype): the state-dict keys.  A GPTQ state dict (`qweight`, `qzeros`, `scales`, optional `g_idx`)
    is repacked on load, read by `gptq_config` (the checkpoint's `quantization_config`; None: format "gptq", 4 bits, group 128);
    a 16-bit `weight` is quantised on load."""
    NAME, CODES, SCALES, KIND, W_FLAG, K_MULTIPLE = "int4", "qcodes", "qscale_zero", "int4-g128", MXVL_W_INT4, 128
    quantize, dequantize_into = staticmethod(quantize_int4), staticmethod(dequantize_int4)
    gptq_config = None

    @staticmethod
    def buffers(N, K):
        if K % GROUP:
            raise ValueError(f"int4 (group {GROUP}) needs in_features % {GROUP} == 0, got {K}")
        return ((N, K // 2), torch.uint8), ((N, K // GROUP), torch.int32)

    def _load_from_state_dict(self, state_dict, prefix, *args):
        if prefix + "qweight" in state_dict:
            local = {k: v for k, v in state_dict.items() if k.startswith(prefix) and k[len(prefix):] not in GPTQ_KEYS}
            try:
                codes, scales = import_gptq(*(state_dict.get(prefix + k) for k in GPTQ_KEYS), quantization_config=self.gptq_config)
            except ValueError as e:
                raise ValueError(f"{prefix[:-1] or type(self).__name__}: {e}") from None
            if codes.shape != self.qcodes.shape:
                raise ValueError(f"{prefix[:-1] or type(self).__name__}: the GPTQ tensors describe a ({codes.shape[0]}, {codes.shape[1] * 2}) "
                                 f"weight, the module holds ({self.out_features}, {self.in_features})")
            local[prefix + self.CODES], local[prefix + self.SCALES] = codes, scales
            state_dict = local
        super()._load_from_state_dict(state_dict, prefix, *args)
