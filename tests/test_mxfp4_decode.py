"""low_resource="mxfp4": OCP MXFP4 LLM weights (mxfp4_linear.py) and the W4A16 decode projections (mxvl_decode_gemv with
MXVL_W_MXFP4, csrc/decode_gemm.h decode_gemm_w4_kernel)."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from medical_image_analysis_amd import _abi
from medical_image_analysis_amd.int8_linear import Int8Linear
from medical_image_analysis_amd.mxfp4_linear import MxFp4Linear, dequantize_mxfp4, quantize_mxfp4
from medical_image_analysis_amd.report_decoder import ReportDecoder, _KernelStepper

DEV = "cuda" if torch.cuda.is_available() else "cpu"
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
LUT = torch.tensor(E2M1 + [-v for v in E2M1], dtype=torch.float64)


def _unpack(packed):
    """(N, K / 2) bytes -> (N, K) codes, the element of even k from the LOW nibble"""
    return torch.stack((packed & 15, packed >> 4), dim=2).reshape(packed.shape[0], -1).long()


# ---- 1. quantiser ---------------------------------------------------------------------------------------------------------------------
def _brute_force(W):
    """An independent restatement: per block of 32, X = floor(log2(max)) - 2; each element the nearest of the 15 E2M1 values to
    w / 2^X, a tie to the value whose mantissa bit is 0.  Plain Python floats (every quantity here is exact in them)."""
    values = [(c, (-1.0 if c & 8 else 1.0) * E2M1[c & 7]) for c in range(16) if c != 8]          # 15 values: one zero
    codes, scales = [], []
    for row in W.double().tolist():
        crow, srow = [], []
        for b in range(0, len(row), 32):
            blk = row[b:b + 32]
            amax = max(abs(v) for v in blk)
            X = max(-127, min(127, math.floor(math.log2(amax)) - 2)) if amax > 0 else -127
            srow.append(X + 127)
            for w in blk:
                r = w / 2.0 ** X
                best = min(values, key=lambda cv: (abs(r - cv[1]), cv[0] & 1))                   # nearest; on a tie the even mantissa
                crow.append(best[0])
        codes.append(crow)
        scales.append(srow)
    return torch.tensor(codes), torch.tensor(scales)


def _quantiser_cases():
    g = torch.Generator().manual_seed(0)
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]                     # every midpoint of the grid
    W = torch.zeros(4, 128)
    # row 0: block 0 holds every tie of both signs with X = 0 (max 7.5: saturates), block 1 is all zero, block 2 has its maximum at an
    # exact power of two (0.125: X = -5, the maximum lands on 4), block 3 the ties again under another scale (X = 5)
    blk = torch.tensor(ties + [-t for t in ties] + [7.0, 7.5, -7.0, 6.0, 4.0, 3.0, 2.0, 1.5, 1.0, 0.5, 0.0, -6.0, -0.1, 0.1, 0.3, -0.26, 6.5, -5.5])
    assert blk.numel() == 32
    W[0, 0:32] = blk
    W[0, 64:96] = torch.rand(32, generator=g) * 0.125
    W[0, 64] = 0.125
    W[0, 96:128] = blk * 32.0
    W[1] = torch.randn(128, generator=g)
    W[2] = torch.randn(128, generator=g) * 1e-3
    W[2, 32:64] *= 2.0 ** 20                                            # neighbouring blocks 20 binades apart
    W[3, 0:32] = torch.tensor([1.0] + [0.0] * 31)                       # maximum exactly 1: X = -2
    W[3, 32:64] = 2.0 ** -10
    W[3, 64:96] = -(2.0 ** 7)
    W[3, 96:128] = torch.randn(32, generator=g).abs().clamp_min(0.01) * 3
    return W.to(torch.bfloat16)                                          # 16-bit weights, as the decoder holds them


def test_quantiser_against_brute_force_and_literal_bytes():
    W = _quantiser_cases()
    packed, scale = quantize_mxfp4(W)
    assert packed.dtype == torch.uint8 and packed.shape == (4, 64) and scale.dtype == torch.uint8 and scale.shape == (4, 4)
    want_codes, want_scale = _brute_force(W)
    assert torch.equal(_unpack(packed), want_codes)
    assert torch.equal(scale.long(), want_scale)
    # literally: ties to even, saturation, the zero block, the power-of-two maxima
    c = _unpack(packed)
    assert c[0, :7].tolist() == [0, 2, 2, 4, 4, 6, 6], "0.25->0 0.75->1 1.25->1 1.75->2 2.5->2 3.5->4 5->4"
    assert c[0, 7:14].tolist() == [0, 10, 10, 12, 12, 14, 14], "a negative that rounds to zero is +0"
    assert c[0, 14:17].tolist() == [7, 7, 15], "7 and 7.5 saturate at 6"
    assert scale[0].tolist() == [127, 0, 122, 132] and not packed[0, 16:32].any(), "the all-zero block: X = -127, zero codes"
    assert c[0, 64] == 6 and scale[3].tolist()[:3] == [125, 115, 132] and c[3, 0] == 6 and c[3, 64] == 14
    assert torch.equal(c[0, 96:128], c[0, 0:32])
    # nibble order: 0.5, -1, 1.5, 6 -> codes 1, 10, 3, 7 -> bytes 0xA1, 0x73; scale byte 127 (X = 0)
    lit = torch.zeros(1, 32)
    lit[0, :4] = torch.tensor([0.5, -1.0, 1.5, 6.0])
    p, s = quantize_mxfp4(lit.to(torch.bfloat16))
    assert p[0, :3].tolist() == [0xA1, 0x73, 0] and s.tolist() == [[127]]
    # dequantize() is codes x scale, exactly
    wdq = dequantize_mxfp4(packed, scale, torch.bfloat16)
    exact = LUT[c] * torch.pow(2.0, scale.double() - 127).repeat_interleave(32, dim=1)
    assert wdq.dtype == torch.bfloat16 and torch.equal(wdq.double(), exact)
    nz = W.double().abs() > 0
    assert ((W.double() - exact).abs()[nz] <= W.double().abs().reshape(4, 4, 32).amax(2).repeat_interleave(32, dim=1)[nz] * 0.25).all()


def test_quantiser_refuses_fp16_weights_outside_the_exact_range():
    W = torch.full((2, 32), 2.0 ** -13, dtype=torch.float16)            # X = -15: 0.5 * 2^-15 is fp16's subnormal 2^-16, still exact
    p, s = quantize_mxfp4(W)
    assert s.tolist() == [[112], [112]] and torch.equal(dequantize_mxfp4(p, s, torch.float16), W)
    W[1, 3] = 60000.0                                                    # X = 13, the top of fp16
    p, s = quantize_mxfp4(W)
    assert s[1, 0] == 140 and torch.isfinite(dequantize_mxfp4(p, s, torch.float16)).all()
    W = torch.zeros(2, 64, dtype=torch.float16)
    W[0, 40] = 2.0 ** -14                                                # X = -16
    with pytest.raises(ValueError, match="fp16"):
        quantize_mxfp4(W)
    p, s = quantize_mxfp4(W.to(torch.bfloat16))                          # bf16 has no such limit
    assert s[0, 1] == 111 and s[0, 0] == 0
    with pytest.raises(ValueError, match="32"):
        quantize_mxfp4(torch.zeros(2, 48))


# ---- 2. MxFp4Linear -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mxfp4_linear_forward_backward_and_saved_tensors(dtype):
    torch.manual_seed(1)
    N, K = 48, 64
    lin = nn.Linear(K, N, bias=True).to(dtype)
    q = MxFp4Linear.from_linear(lin)
    wdq = q.dequantize()
    assert wdq.dtype == dtype and wdq.shape == (N, K) and torch.equal(wdq, dequantize_mxfp4(q.weight_packed, q.weight_scale, dtype))
    x = torch.randn(3, 5, K).to(dtype).requires_grad_(True)
    x2 = x.detach().clone().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        y = q(x)
    assert all(t.dtype == torch.uint8 for t in saved if t.numel() >= N * K // 32), "only codes and scales are kept for backward"
    assert any(t.dtype == torch.uint8 and t.numel() == N * K // 2 for t in saved)
    y2 = F.linear(x2, wdq, lin.bias)
    assert torch.equal(y, y2)
    dy = torch.randn_like(y)
    y.backward(dy)
    y2.backward(dy)
    assert torch.equal(x.grad, x2.grad)
    assert not any(p.requires_grad for p in q.parameters())


def test_mxfp4_linear_state_dicts():
    torch.manual_seed(2)
    lin = nn.Linear(64, 16, bias=True).to(torch.bfloat16)
    q = MxFp4Linear.from_linear(lin)
    sd = q.state_dict()
    assert sorted(sd) == ["bias", "weight_packed", "weight_scale"]
    assert sd["weight_packed"].dtype == torch.uint8 and sd["weight_packed"].shape == (16, 32) and sd["weight_scale"].shape == (16, 2)
    q2 = MxFp4Linear(64, 16, bias=True, dtype=torch.bfloat16)
    q2.load_state_dict(sd)
    assert torch.equal(q2.weight_packed, q.weight_packed) and torch.equal(q2.weight_scale, q.weight_scale) and torch.equal(q2.bias, q.bias)
    q3 = MxFp4Linear(64, 16, bias=True, dtype=torch.bfloat16)
    q3.load_state_dict(lin.state_dict())                                 # a 16-bit weight quantises on load
    assert torch.equal(q3.weight_packed, q.weight_packed) and torch.equal(q3.weight_scale, q.weight_scale)
    q3.to(torch.float16)
    assert q3.weight_packed.dtype == torch.uint8 and q3.weight_scale.dtype == torch.uint8 and q3.bias.dtype == torch.float16


# ---- 3. quantize_mxfp4_ on the tiny golden model ----------------------------------------------------------------------------------------
def _tiny(dtype=torch.float32):
    """The decode_tiny_llama.npz model, as tests/test_report_decoder.py builds it."""
    from conftest import load_golden
    g = load_golden("decode_tiny_llama")
    m = ReportDecoder(vocab_size=48, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, rms_norm_eps=1e-6, max_position_embeddings=128)
    m.load_hf_state_dict({k[2:]: v for k, v in g.items() if k.startswith("p_")})
    return m.to(dtype).eval(), g


_PROJ = [("self_attn", n) for n in ("q_proj", "k_proj", "v_proj", "o_proj")] + [("mlp", n) for n in ("gate_proj", "up_proj", "down_proj")]


def _wdq_twin(qmodel, make):
    """A plain ReportDecoder (from `make`) holding the dequantised weights of `qmodel`."""
    twin = make()
    with torch.no_grad():
        for lq, lt in zip(qmodel.model.layers, twin.model.layers):
            for owner, name in _PROJ:
                dst = getattr(getattr(lt, owner), name).weight
                dst.copy_(getattr(getattr(lq, owner), name).dequantize(dst.dtype))
    return twin


def _storage_census(model):
    seen, quant_bytes, wide = set(), 0, []
    for name, t in list(model.named_parameters()) + list(model.named_buffers()):
        if t is None:
            continue
        st = t.untyped_storage()
        if st.data_ptr() in seen:
            continue
        seen.add(st.data_ptr())
        if any(f"{o}.{n}." in name for o, n in _PROJ):
            if t.dtype == torch.uint8:
                quant_bytes += st.nbytes()
            elif not name.endswith("bias"):
                wide.append(name)
    return quant_bytes, wide


def test_quantize_mxfp4_replaces_the_layer_projections_and_releases_16_bit_storage():
    model, _ = _tiny(torch.bfloat16)
    model.fuse_qkv_()                                   # quantising a fused model must drop the fused 16-bit buffer too
    assert not model.is_mxfp4()
    model.quantize_mxfp4_()
    want, count = 0, 0
    for layer in model.model.layers:
        for owner, name in _PROJ:
            lin = getattr(getattr(layer, owner), name)
            assert isinstance(lin, MxFp4Linear), (owner, name)
            want += lin.out_features * lin.in_features // 2 + lin.out_features * lin.in_features // 32
            count += 1
        assert getattr(layer.self_attn, "qkv_weight", None) is None
    assert count == 7 * len(model.model.layers)
    assert isinstance(model.lm_head, nn.Linear) and model.lm_head.weight.dtype == torch.bfloat16
    assert model.model.embed_tokens.weight.dtype == torch.bfloat16 and model.is_mxfp4() and not model.is_int8()
    at = model.model.layers[0].self_attn
    before = torch.cat([at.q_proj.dequantize(), at.k_proj.dequantize(), at.v_proj.dequantize()])
    for fused in (False, True):
        if fused:
            model.fuse_qkv_()
            assert at.qkv_weight.dtype == torch.uint8 and at.q_proj.weight_packed.data_ptr() == at.qkv_weight.data_ptr()
            assert at.q_proj.weight_scale.data_ptr() == at.qkv_scale.data_ptr() and at.qkv_scale.shape == (at.qkv_weight.shape[0], 2)
            assert torch.equal(dequantize_mxfp4(at.qkv_weight, at.qkv_scale, torch.bfloat16), before), "fusing is exact"
            assert torch.equal(torch.cat([at.q_proj.dequantize(), at.k_proj.dequantize(), at.v_proj.dequantize()]), before)
        got, wide = _storage_census(model)
        assert got == want and not wide, (fused, got, want, wide)


def test_quantisations_do_not_mix():
    m4, _ = _tiny(torch.bfloat16)
    m4.quantize_mxfp4_()
    with pytest.raises(RuntimeError, match="mxfp4"):
        m4.quantize_int8_()
    assert m4.is_mxfp4() and isinstance(m4.model.layers[0].mlp.up_proj, MxFp4Linear)
    m8, _ = _tiny(torch.bfloat16)
    m8.quantize_int8_()
    with pytest.raises(RuntimeError, match="int8"):
        m8.quantize_mxfp4_()
    assert m8.is_int8() and isinstance(m8.model.layers[0].mlp.up_proj, Int8Linear)
    assert m4.quantize_mxfp4_() is m4                   # again on itself: nothing to do


@pytest.mark.parametrize("mode", ["greedy", "beam3"])
def test_mxfp4_torch_decode_matches_a_16_bit_decoder_holding_wdq(mode):
    dtype = torch.float32            # the CPU torch path; both models run the same arithmetic on the same weights
    qmodel, z = _tiny(dtype)
    qmodel.quantize_mxfp4_()
    twin = _wdq_twin(qmodel, lambda: _tiny(dtype)[0])
    emb = z["inputs_embeds"].to(dtype)
    kw = dict(attention_mask=z["attention_mask"], max_new_tokens=8, min_new_tokens=2, eos_token_id=2, pad_token_id=0, use_graph=False)
    if mode == "beam3":
        kw.update(num_beams=3, repetition_penalty=2.0, length_penalty=2.0)
    assert torch.equal(qmodel.generate(emb, **kw), twin.generate(emb, **kw))


# ---- 4. MambaXrayVLDownStream(low_resource="mxfp4") -----------------------------------------------------------------------------------------
def _tiny_llm_cfg():
    return dict(vocab_size=256, hidden_size=128, intermediate_size=384, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=2, max_position_embeddings=512)


def test_downstream_low_resource_mxfp4_builds_mxfp4_layers_and_true_still_builds_int8():
    from medical_image_analysis_amd import mambaxray_vl as mx
    from test_mambaxray_vl import WordTokenizer
    torch.manual_seed(0)
    args = mx.default_args(vision_model="Base-None", max_length=16, low_resource="mxfp4")
    m = mx.MambaXrayVLDownStream(args, tokenizer=WordTokenizer(), llm=mx.build_report_decoder(_tiny_llm_cfg()))
    assert m.llama_model.is_mxfp4() and not m.llama_model.is_int8()
    assert isinstance(m.llama_model.model.layers[1].mlp.up_proj, MxFp4Linear) and isinstance(m.llama_model.lm_head, nn.Linear)
    assert mx.build_report_decoder(_tiny_llm_cfg(), low_resource="mxfp4").is_mxfp4()
    args = mx.default_args(vision_model="Base-None", max_length=16, low_resource=True)
    m = mx.MambaXrayVLDownStream(args, tokenizer=WordTokenizer(), llm=mx.build_report_decoder(_tiny_llm_cfg()))
    assert m.llama_model.is_int8() and not m.llama_model.is_mxfp4()
    assert mx.build_report_decoder(_tiny_llm_cfg(), low_resource=True).is_int8()
    assert mx.build_report_decoder(_tiny_llm_cfg(), low_resource="int8").is_int8(), "every other truthy value keeps int8"


# ---- 5. descriptor validation without a GPU ---------------------------------------------------------------------------------------------
def _desc(rows=18, K=256, N=64, dtype=None, **kw):
    d = _abi.GemvDesc()
    d.rows, d.K, d.N, d.k_splits = rows, K, N, 1
    d.dtype = _abi.MXVL_BF16 | _abi.MXVL_W_MXFP4 if dtype is None else dtype
    d.x, d.W, d.y, d.w_scale = 0x1000, 0x2000, 0x3000, 0x4000             # fake pointers: nothing is launched
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_mxfp4_descriptor_validation_without_gpu():
    lib = _abi.load()
    out = (ctypes.c_int32 * 5)()
    plan = lambda d: lib.mxvl_decode_gemm_plan(ctypes.byref(d), out)
    assert _abi.ABI_VERSION == 13 and lib.mxvl_abi_version() == 13 and _abi.MXVL_W_MXFP4 == 0x200
    assert plan(_desc()) == 0 and out[0] == 4 and out[1] == 4 and out[2] in (1, 2) and out[3] >= 2 and out[4] >= 1
    assert plan(_desc(rows=1, k_splits=0)) == 0 and out[0] == 4, "no mxfp4 form of the <= 8-row GEMV"
    assert plan(_desc(K=72)) < 0 and plan(_desc(K=32)) < 0 and plan(_desc(rows=81)) < 0
    assert plan(_desc(K=64, N=16, rows=80)) == 0 and out[0] == 4
    assert plan(_desc(dtype=_abi.MXVL_BF16 | _abi.MXVL_W_MXFP4 | _abi.MXVL_W_INT8)) == -2, "both weight flags: MXVL_ERR_DTYPE"
    assert plan(_desc(dtype=3 | _abi.MXVL_W_MXFP4)) == -2
    assert plan(_desc(w_scale=None)) == -1, "NULL scale: MXVL_ERR_NULL"
    assert plan(_desc(swiglu=1, W2=0x5000)) == -1, "w2_scale with swiglu"
    assert plan(_desc(swiglu=1, W2=0x5000, w2_scale=0x6000)) == 0 and out[0] == 4 and out[2] == 2
    assert plan(_desc(norm_weight=0x5000)) == -3, "the fused norm is refused: MXVL_ERR_SHAPE"
    assert plan(_desc(out_f32=1)) == -3
    assert plan(_desc(dtype=_abi.MXVL_F16 | _abi.MXVL_W_MXFP4, split_acc=0x7000, k_splits=4, y=None)) == 0 and out[0] == 4 and out[4] == 4
    assert plan(_desc(K=11008, N=4096, swiglu=1, W2=0x5000, w2_scale=0x6000)) == 0
    # the int8 and 16-bit descriptors plan as before
    assert plan(_desc(dtype=_abi.MXVL_BF16 | _abi.MXVL_W_INT8)) == 0 and out[0] == 3
    assert plan(_desc(dtype=_abi.MXVL_BF16)) == 0 and out[0] in (0, 1)


# ---- 6. the projection against float64 ---------------------------------------------------------------------------------------------------
def _ulp(y, dtype):
    """one unit in the last place of `dtype` at |y| (float64 tensors)"""
    mant = 8 if dtype == torch.bfloat16 else 11
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -126 if dtype == torch.bfloat16 else 2.0 ** -14)))
    return torch.pow(2.0, e - (mant - 1))


def _weights(N, K, g):
    """Hand-made codes and scale bytes (not only what the quantiser produces): every code, -0 included; the scale bytes drawn PER BLOCK
    over eight exponents, the largest block maximum 6 * 2^X about 2 * 4 / sqrt(K) -- the amplitude test_int8_decode uses, which keeps
    |gate| of the SwiGLU cases far below the fp32 exp's range.  A kernel that ignores block boundaries is off by up to 2^7."""
    codes = torch.randint(0, 16, (N, K), generator=g)
    codes[:, :16] = torch.arange(16)
    codes[0, :] = 15
    top = math.floor(math.log2(4.0 / K ** 0.5 / 3.0))
    e = 127 + top - torch.randint(0, 8, (N, K // 32), generator=g)
    e[:, 0], e[:, -1] = 127 + top, 127 + top - 7
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8).contiguous()
    wdq = LUT[codes] * torch.pow(2.0, e.double() - 127).repeat_interleave(32, dim=1)
    return packed, e.to(torch.uint8).contiguous(), wdq


def _launch(x, packed, scale, y=None, packed2=None, scale2=None, bias=None, res=None, acc=None, splits=1):
    d = _abi.GemvDesc()
    d.rows, d.K, d.N = x.shape[0], x.shape[1], packed.shape[0]
    d.dtype = _abi.dtype_code(x.dtype) | _abi.MXVL_W_MXFP4
    d.x, d.W, d.w_scale, d.y = x.data_ptr(), packed.data_ptr(), scale.data_ptr(), _abi.ptr(y)
    d.W2, d.w2_scale, d.swiglu = _abi.ptr(packed2), _abi.ptr(scale2), int(packed2 is not None)
    d.bias, d.residual = _abi.ptr(bias), _abi.ptr(res)
    d.k_splits = splits if acc is not None else 0                     # 0: by row count -- must still take the mxfp4 kernel
    d.split_acc = _abi.ptr(acc)
    _abi.launch("mxvl_decode_gemv", d, device=x.device)


def _check_projection(rows, K, N, dtype, epi, splits=1):
    """The tolerance test_int8_decode._check_projection derives, per element: code -> element conversion and the products are exact,
    so the fp32 sum of K terms is within K * 2^-24 * sum_k |w x| of the exact one (first-order bound of any summation order), plus
    one ulp of the output dtype at |y| for the final rounding.  split: the fp32 bound only.
    bias + residual: the kernel rounds (acc + bias) to dtype before the residual add, as the modules do: one more ulp at that value.
    swiglu: y = silu(a) * b with a, b each rounded to dtype (da = fp32 bound + ulp(a), likewise db), silu(a) rounded (ulp(silu(a))),
    the product rounded (ulp(y)); to first order |dy| <= |silu'(a)| |b| da + |silu(a)| db + ulp(silu(a)) |b| + ulp(y)."""
    g = torch.Generator().manual_seed(rows * 131 + K + N)
    dev = torch.device(DEV)
    packed, scale, wdq = _weights(N, K, g)
    x = torch.randn(rows, K, generator=g).to(dtype)
    xd = x.double()
    a = xd @ wdq.t()
    bound_a = K * 2.0 ** -24 * (xd.abs() @ wdq.abs().t())
    xg, pg, sg = x.to(dev), packed.to(dev), scale.to(dev)
    if epi == "split":
        acc = torch.full((splits, rows, N), float("nan"), device=dev)
        _launch(xg, pg, sg, acc=acc, splits=splits)
        got = acc.double().sum(0).cpu()
        assert torch.isfinite(got).all()
        err, tol = (got - a).abs(), bound_a
    elif epi == "swiglu":
        packed2, scale2, wdq2 = _weights(N, K, g)
        b = xd @ wdq2.t()
        bound_b = K * 2.0 ** -24 * (xd.abs() @ wdq2.abs().t())
        y = torch.empty(rows, N, dtype=dtype, device=dev)
        _launch(xg, pg, sg, y=y, packed2=packed2.to(dev), scale2=scale2.to(dev))
        sig = torch.sigmoid(a)
        silu, dsilu = a * sig, sig * (1 + a * (1 - sig))
        want = silu * b
        tol = dsilu.abs() * b.abs() * (bound_a + _ulp(a, dtype)) + silu.abs() * (bound_b + _ulp(b, dtype)) \
            + _ulp(silu, dtype) * b.abs() + _ulp(want, dtype)
        err = (y.double().cpu() - want).abs()
    else:
        bias = torch.randn(N, generator=g).to(dtype)
        res = torch.randn(rows, N, generator=g).to(dtype) if epi == "bias_res" else None
        y = torch.empty(rows, N, dtype=dtype, device=dev)
        _launch(xg, pg, sg, y=y, bias=bias.to(dev), res=None if res is None else res.to(dev))
        lin = a + bias.double()
        want = lin if res is None else lin + res.double()
        tol = bound_a + _ulp(want, dtype) + (_ulp(lin, dtype) if res is not None else 0.0)
        err = (y.double().cpu() - want).abs()
    worst = float((err / tol).max())
    print(f"mxfp4 projection rows={rows} K={K} N={N} {dtype} {epi} splits={splits}: max err / tol = {worst:.3f}")
    assert worst <= 1.0, (rows, K, N, dtype, epi, splits, worst)


# rows: one to five activation tiles, the 8 / 9 edge of the unquantised dispatch, a partly filled last tile.  K: 64 and 128 are a
# quarter and a half of ONE 256-column chunk, 1408 is five chunks and a half (K / 32 = 44: the scale rows are 4-byte aligned;
# at 64 they are 2-byte aligned).  N: one tile, a partly filled workgroup (72 = 4.5 tiles, N % 4 == 0), several workgroups (520).
_ROWS, _KS, _NS = (1, 3, 8, 9, 18, 49, 80), (64, 128, 1408), (16, 72, 520)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("epi", ["bias", "bias_res", "swiglu", "split1", "split4"])
def test_mxfp4_projection_against_float64(dtype, epi):
    """The whole grid of rows x K x N for one dtype and epilogue (63 launches of a few microseconds each).  With 4 splits K = 64 and
    128 leave three planes without a chunk: they must come out as zeros."""
    splits = int(epi[5:]) if epi.startswith("split") else 1
    for rows in _ROWS:
        for K in _KS:
            for N in _NS:
                _check_projection(rows, K, N, dtype, "split" if epi.startswith("split") else epi, splits=splits)


@pytest.mark.gpu
@pytest.mark.parametrize("epi,splits", [("bias", 1), ("bias_res", 1), ("swiglu", 1), ("split", 4)])
@pytest.mark.parametrize("K,N", [(4096, 4096), (11008, 4096)])
def test_mxfp4_projection_real_widths(K, N, epi, splits):
    _check_projection(18, K, N, torch.bfloat16, epi, splits=splits)


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------
_E2E_DTYPE, _E2E_SEED = torch.float16, 37
_E2E_ULP = 2.0 ** -10            # fp16


def _e2e_kwargs(mode):
    kw = dict(max_new_tokens=8, min_new_tokens=2, eos_token_id=2, pad_token_id=0)
    if mode == "beam3":
        kw.update(num_beams=3, repetition_penalty=2.0, length_penalty=2.0)
    elif mode == "sampled":
        # Temperature sampling without a top-k or top-p cut, and a low temperature.  The logits of this random model are nearly flat
        # (96 values with a standard deviation of 0.6; the logit tolerance is 0.01): neighbours in the sorted order lie 0..5
        # tolerances apart, so a cut at a fixed rank falls inside the tolerance at some of the 16 draws for every seed, and at
        # temperature 0.9 a token's CDF interval (~1/96) is no wider than what the tolerance moves its ends by.  At 0.1 the
        # intervals of the likely tokens are many tolerances wide; the seed (of 250 scanned on the CPU) keeps all 16 draws clear
        # of their ends and still draws tokens the greedy decode does not.  The cuts themselves are tests/test_sample_decode.py's.
        kw.update(do_sample=True, temperature=0.1, seed=168)
    return kw


def _servable(dtype):
    """The small random model of test_int8_decode's end-to-end test: the smallest the kernels serve (head_dim 64, every K % 64 == 0;
    K = 128 and 192: half a 256-column chunk and three quarters of one)."""
    torch.manual_seed(7)
    return ReportDecoder(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2,
                         num_key_value_heads=2, rms_norm_eps=1e-6, max_position_embeddings=128).to(dtype).eval()


def _e2e_prompt(dtype):
    return torch.randn(2, 6, 128, generator=torch.Generator().manual_seed(_E2E_SEED)).to(dtype)


def _logit(r):
    return math.inf if r >= 1.0 else -math.inf if r <= 0.0 else math.log(r) - math.log1p(-r)


def _draw_margin(lg, tok, step, row, kw, tol):
    """How far the sampled draw of one row of one step is from changing, as a multiple of `tol`, the largest error of one logit.
    With s = tol / temperature every processed score moves by at most s, every exp(score) by a factor within exp(+-s) and the
    ratio A / B of any two sums of them by a factor within exp(+-2s): logit(A / (A + B)) moves by at most 2s.  The drawn token
    stays what it is if, each by more than 2s,
      - the scores of the k-th and the (k+1)-th token differ (top-k keeps the same set), and so do those of the last token top-p
        keeps and the first it drops (the m kept tokens stay the m largest, in whatever order);
      - logit(the largest mass m - 1 kept tokens have) stays below logit(top_p) and logit(the mass of all m) above it (top-p cuts
        at the same place: a token is kept iff the mass of the greater ones is < top_p);
      - logit(u) stays between the logits of the cumulative masses, in vocabulary order, in front of and behind the drawn token.
    Returns the smallest of these distances / 2s.  The case runs without a repetition penalty or an n-gram ban; `tok` is what
    generate() drew, checked against this restatement of the rule."""
    from medical_image_analysis_amd.report_decoder import sample_uniform
    assert kw.get("repetition_penalty", 1.0) == 1.0 and not kw.get("no_repeat_ngram_size")
    sc = lg.double().clone()
    if step < kw["min_new_tokens"]:
        sc[kw["eos_token_id"]] = -math.inf
    sc = sc / kw["temperature"]
    k, top_p = kw.get("top_k") or sc.numel(), kw.get("top_p", 1.0)
    vals, order = torch.sort(sc, descending=True)
    dist = [float(vals[k - 1] - vals[k])] if k < sc.numel() else []
    p = torch.softmax(vals[:k], dim=-1)
    front = torch.cumsum(p, dim=-1) - p                                  # the mass of the greater tokens
    m = int((front < top_p).sum())
    if m < k:
        dist.append(float(vals[m - 1] - vals[m]))
        dist.append(_logit(float(front[m])) - _logit(top_p))
    if top_p < 1.0:
        dist.append(_logit(top_p) - _logit(float(front[m - 1])))
    kept = torch.zeros_like(sc, dtype=torch.bool)
    kept[order[:m]] = True
    c = torch.where(kept, torch.exp(sc - vals[0]), torch.zeros_like(sc)).cumsum(-1)
    c = c / c[-1]
    u = float(sample_uniform(kw["seed"], row + 1, step)[row])
    assert kept[tok] and (float(c[tok - 1]) if tok else 0.0) <= u < float(c[tok]), (step, row, tok)
    dist.append(_logit(float(c[tok])) - _logit(u) if bool(kept[tok + 1:].any()) else math.inf)
    dist.append(_logit(u) - _logit(float(c[tok - 1])) if tok and bool(kept[:tok].any()) else math.inf)
    return min(dist) / (2.0 * tol / kw["temperature"])


def _torch_path_margin(mode):
    """The eager torch decode of the case on the CPU, fp16, against the logit tolerance of test_mxfp4_kernel_step_logits (8 fp16
    ulps at the row's max), over every row of every step: the smallest top-two logit margin as a multiple of that tolerance and,
    for the sampled case, whose draw is not decided by the top two, the smallest `_draw_margin`.  Returns (margin, draw margin or
    None, steps)."""
    model = _servable(_E2E_DTYPE).quantize_mxfp4_()
    kw = _e2e_kwargs(mode)
    rows = []
    hook = model.lm_head.register_forward_hook(lambda mod, inp, out: rows.append(out[:, -1].float()))
    toks = model.generate(_e2e_prompt(_E2E_DTYPE), use_graph=False, **kw)
    hook.remove()
    worst, draw = float("inf"), float("inf") if mode == "sampled" else None
    for step, lg in enumerate(rows):
        tol = 8 * _E2E_ULP * lg.abs().amax(-1)
        top = lg.topk(2, dim=-1).values
        worst = min(worst, float(((top[:, 0] - top[:, 1]) / tol).min()))
        if mode == "sampled":
            for r in range(lg.shape[0]):
                if step < toks.shape[1] and not bool((toks[r, :step] == kw["eos_token_id"]).any()):     # the row still draws
                    draw = min(draw, _draw_margin(lg[r], int(toks[r, step]), step, r, kw, float(tol[r])))
    return worst, draw, len(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["greedy", "beam3", "sampled"])
def test_mxfp4_kernel_stepper_end_to_end(mode):
    """generate() on the kernel stepper (captured hipGraph) against use_graph="torch" on the same device, fp16, token for token.
    The two paths sum in different orders, so equality is a fair demand only where the torch path is not on a near-tie: the prompt
    seed was picked on the CPU so that the smallest top-two logit margin over all steps exceeds the 8-ulp logit tolerance the
    kernel step is held to, and that is asserted here.  A sampled token is an inverse-CDF draw behind a top-k and a top-p cut,
    which the top two logits do not decide: for that case the seed also keeps every draw further than the same tolerance from
    every cut and from both ends of its CDF interval (`_draw_margin`).  The margins are the CPU path's and the comparison is
    between two device paths, each within the tolerance of it, so the draw margin is held to twice the tolerance."""
    dtype = _E2E_DTYPE
    kw = _e2e_kwargs(mode)
    margin, draw, steps = _torch_path_margin(mode)
    print(f"{mode}: smallest top-two margin over {steps} steps = {margin:.2f} x the logit tolerance"
          + (f", smallest draw margin = {draw:.2f} x" if draw is not None else ""))
    assert steps >= 2 and margin > 1.0, f"{mode}: the torch-path decode of this case sits on a near-tie; pick another prompt seed"
    assert draw is None or draw > 2.0, f"{mode}: a draw of this case sits next to a cut or a CDF boundary; pick another prompt seed"
    qmodel = _servable(dtype).quantize_mxfp4_().to(DEV)
    assert _KernelStepper.supported(qmodel, 6, dtype, DEV)
    emb = _e2e_prompt(dtype).to(DEV)
    ref = qmodel.generate(emb, use_graph="torch", **kw)
    qmodel.__dict__.pop("_steppers", None)              # (the torch-module stepper of the call above)
    got = qmodel.generate(emb, use_graph=True, **kw)
    assert all(type(s) is _KernelStepper and s.mxfp4 and not s.int8 and not s.fused_norm for s in qmodel._steppers.values())
    assert torch.equal(got.cpu(), ref.cpu()), (mode, got.tolist(), ref.tolist())


@torch.no_grad()
def _prefill(model, emb):
    from medical_image_analysis_amd.report_decoder import KVCache
    cache = KVCache()
    attn = torch.ones(emb.shape[:2], dtype=torch.long, device=emb.device)
    return model.forward(emb, attention_mask=attn, past_key_values=cache)[:, -1].float(), cache


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_mxfp4_kernel_step_logits(dtype):
    """The first decode step of an mxfp4 model on the kernel stepper, run eagerly, against the torch modules on the same device:
    the logits agree within 8 output-dtype ulps of the logit row's max (the project's rule: tests/test_report_decoder.py
    test_fused_norm_projection_over_real_checkpoint_ranges, tests/test_int8_decode.py)."""
    qmodel = _servable(dtype).quantize_mxfp4_().to(DEV)
    emb = _e2e_prompt(dtype).to(DEV)
    logits0, cache = _prefill(qmodel, emb)
    tok = logits0.argmax(-1)
    st = _KernelStepper(qmodel, 2, torch.ones(2, 6, dtype=torch.long, device=DEV), cache, 8, dtype)
    assert st.mxfp4 and not st.fused_norm and st.graph is None
    lk = st._body(tok, torch.arange(2, device=DEV), torch.ones(1, dtype=torch.long, device=DEV)).clone()
    attn = torch.ones(2, 7, dtype=torch.long, device=DEV)
    with torch.no_grad():
        lt = qmodel.forward(qmodel.model.embed_tokens(tok)[:, None, :], attention_mask=attn, past_key_values=cache)[:, -1].float()
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    tol = 8 * ulp * lt.abs().amax(-1, keepdim=True)
    worst = float(((lk - lt).abs() / tol).max())
    print(f"first-step logits {dtype}, kernel vs torch: max err / tol = {worst:.3f}")
    assert worst <= 1.0


# ---- 8. what the kernel cannot serve ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mxfp4_decoder_with_unserved_width_takes_torch_or_raises():
    torch.manual_seed(0)
    m = ReportDecoder(vocab_size=64, hidden_size=128, intermediate_size=160, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=2).to(torch.bfloat16).to(DEV).eval()     # head_dim 64, intermediate % 64 != 0 (% 32 == 0)
    assert _KernelStepper.supported(m, 2, torch.bfloat16, DEV)
    m.quantize_mxfp4_()
    assert not _KernelStepper.supported(m, 2, torch.bfloat16, DEV)
    emb = torch.randn(1, 4, 128, device=DEV, dtype=torch.bfloat16)
    assert m.generate(emb, max_new_tokens=4, use_graph="torch").shape == (1, 4)
    with pytest.raises(RuntimeError, match="pass use_graph"):
        m.generate(emb, max_new_tokens=4, use_graph=True)
