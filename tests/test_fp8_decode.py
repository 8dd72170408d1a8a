"""low_resource="fp8": row-wise OCP E4M3 LLM weights (fp8_linear.py) and the W8A16 decode projections (mxvl_decode_gemv with
MXVL_W_FP8, csrc/decode_gemm.h decode_gemm_w8f_kernel)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from medical_image_analysis_amd import _abi
from medical_image_analysis_amd.fp8_linear import Fp8Linear, dequantize_rowwise_fp8, quantize_rowwise_fp8
from medical_image_analysis_amd.int8_linear import Int8Linear
from medical_image_analysis_amd.mxfp4_linear import MxFp4Linear
from medical_image_analysis_amd.report_decoder import ReportDecoder, _KernelStepper

from test_int8_decode import (_PROJ, _ROWS, _KS, _NS, _TAIL, _e2e_kwargs, _e2e_prompt, _prefill, _servable, _tiny, _tiny_llm_cfg, _ulp)
from test_mxfp4_decode import _wdq_twin

DEV = "cuda" if torch.cuda.is_available() else "cpu"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = torch.float8_e4m3fn


def _bytes(t):
    return t.view(torch.uint8)


# ---- 1. quantiser -----------------------------------------------------------------------------------------------------------------------
def _e4m3_table():
    """The 256 byte values in float64 from the bit fields (sign | 4 exponent bits, bias 7 | 3 mantissa bits; exponent 0 is subnormal,
    0x7f / 0xff are the NaNs): not torch's cast."""
    v = np.zeros(256)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        mag = np.nan if (e == 15 and m == 7) else (m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        v[b] = -mag if b & 0x80 else mag
    return v


E4M3 = _e4m3_table()


def _brute_force(W):
    """The contract restated with numpy: scale = fp32(amax / 448), ratio = fp32(W / scale) (+0 in an all-zero row), code = the finite
    E4M3 value nearest to the ratio, ties to the even code; the sign bit is the ratio's."""
    Wf = W.numpy().astype(np.float32)
    scale = (np.abs(Wf).max(axis=1, keepdims=True) / np.float32(448.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, Wf / scale, np.float32(0.0)).astype(np.float32)
    mags = E4M3[:127]                                               # codes 0x00 .. 0x7e: ascending magnitudes
    codes = np.zeros(Wf.shape, dtype=np.uint8)
    for idx in np.ndindex(*Wf.shape):
        r = float(ratio[idx])
        d = np.abs(mags - abs(r))
        best = [c for c in range(127) if d[c] == d.min()]
        assert len(best) <= 2
        c = best[0] if len(best) == 1 else [c for c in best if c % 2 == 0][0]
        codes[idx] = c | (0x80 if np.signbit(r) else 0)
    return codes, scale


def _quantiser_matrix():
    g = torch.Generator().manual_seed(0)
    W = torch.randn(8, 64, generator=g)
    W[0] = 0.0                                                       # all-zero row
    # row 1: amax = 448, so scale = 1 and W is the ratio: exact half-way points between neighbouring codes (normal and subnormal)
    W[1] = torch.rand(64, generator=g) * 300
    W[1, 0] = 448.0
    W[1, 1:9] = torch.tensor([1.0625, 1.1875, -1.0625, 17.0, 19.0, -432.0, 2.0 ** -10, 3 * 2.0 ** -10])
    W[1, 9:13] = torch.tensor([-(2.0 ** -10), 5 * 2.0 ** -10, 15 * 2.0 ** -10, 2.0 ** -11])    # 15 * 2^-10: between the last subnormal and 2^-6
    W[2] = torch.rand(64, generator=g) * 0.5
    W[2, 7] = -3.0                                                   # the row's maximum is negative
    W[3] = torch.randn(64, generator=g) * 0.01
    W[3, 5] = 1.0e4                                                  # one huge outlier: the rest lands in the subnormals or on zero
    W[4] = torch.randn(64, generator=g) * 2.0e-5                      # the subnormal range of a row: ratio < 2^-6 means |W| < 3.5e-5 here
    W[4, 0] = 1.0
    W[5] *= 1.0e-3
    W[6] *= 37.0
    return W


def test_quantiser_against_brute_force_and_error_bound():
    """Error bound per element, in float64: the ratio is r = (W / s)(1 + d), |d| <= 2^-24 (one fp32 division), and the code c is the
    nearest E4M3 value, |c - r| <= max(2^-4 |r|, 2^-10) (half an ulp of a 3-bit mantissa: the spacing in [2^e, 2^(e+1)) is 2^(e-3);
    half the subnormal spacing 2^-9).  So |W - c s| <= s |W / s - r| + s |r - c| <= 2^-24 |W| + max(2^-4 |W| (1 + 2^-24), 2^-10 s):
    the slack added to the issue's bound is 2^-23 |W| -- the division's rounding plus its share inside the 2^-4 term, which also
    covers a ratio that lands a rounding above 448 and is clamped."""
    W = _quantiser_matrix()
    codes, scale = quantize_rowwise_fp8(W)
    assert codes.dtype == F8 and codes.shape == W.shape and scale.dtype == torch.float32 and scale.shape == (8, 1)
    want_codes, want_scale = _brute_force(W)
    assert np.array_equal(scale.numpy(), want_scale), "scale = amax / 448 in fp32"
    got = _bytes(codes).numpy()
    assert np.array_equal(got, want_codes), np.argwhere(got != want_codes)[:8]
    assert not ((got & 0x7f) == 0x7f).any(), "no NaN code"
    assert not got[0].any() and scale[0, 0] == 0 and torch.isfinite(scale).all(), "all-zero row: scale 0, codes +0"
    amax_at = W.abs().argmax(dim=1)
    for n in range(1, 8):
        assert got[n, amax_at[n]] == (0xfe if W[n, amax_at[n]] < 0 else 0x7e), "the row maximum maps to +-448"
    assert got[2, 7] == 0xfe
    # the half-way points of row 1 (scale 1): ties go to the even code
    assert E4M3[got[1, 1:13]].tolist() == [1.0, 1.25, -1.0, 16.0, 20.0, -448.0, 0.0, 2.0 ** -8, -0.0, 2.0 ** -8, 2.0 ** -6, 0.0]
    assert got[1, 9] == 0x80, "the sign of a value that rounds to zero is kept"
    assert ((got[3] & 0x7f) < 8).sum() >= 60 and ((got[4] & 0x7f) < 8).sum() >= 40, "rows 3 and 4 exercise the subnormal codes"
    Wd, s = W.double().numpy(), scale.double().numpy()
    err = np.abs(Wd - E4M3[got] * s)
    bound = np.maximum(2.0 ** -4 * np.abs(Wd), 2.0 ** -10 * s) + 2.0 ** -23 * np.abs(Wd)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert torch.equal(dequantize_rowwise_fp8(codes, scale, torch.float32), (torch.from_numpy(E4M3[got]).float() * scale))
    with pytest.raises(ValueError):
        quantize_rowwise_fp8(torch.tensor([[1.0, float("inf")]]))


# ---- 2. Fp8Linear -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fp8_linear_forward_backward_and_saved_tensors(dtype):
    torch.manual_seed(1)
    N, K = 48, 64
    lin = nn.Linear(K, N, bias=True).to(dtype)
    q = Fp8Linear.from_linear(lin)
    wdq = dequantize_rowwise_fp8(q.weight, q.weight_scale, dtype)
    assert torch.equal(wdq, (q.weight.float() * q.weight_scale).to(dtype))
    x = torch.randn(3, 5, K).to(dtype).requires_grad_(True)
    x2 = x.detach().clone().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        y = q(x)
    assert all(t.dtype == F8 or t.numel() < N * K for t in saved), "only codes / scales are kept for backward"
    assert any(t.dtype == F8 and t.numel() == N * K for t in saved) and any(t.dtype == torch.float32 and t.shape == (N, 1) for t in saved)
    y2 = F.linear(x2, wdq, lin.bias)
    assert torch.equal(y, y2)
    dy = torch.randn_like(y)
    y.backward(dy)
    y2.backward(dy)
    assert torch.equal(x.grad, x2.grad)                                      # dx = dy @ Wdq
    assert not any(p.requires_grad for p in q.parameters()) and q.weight.dtype == F8 and not q.weight.requires_grad
    assert "fp8 e4m3 row-wise" in repr(q) and q.W_FLAG == _abi.MXVL_W_FP8


# ---- 3. state dicts ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a.contiguous()), _bytes(b.contiguous()))


def test_fp8_linear_state_dicts_and_casts():
    torch.manual_seed(2)
    lin = nn.Linear(64, 16, bias=True).to(torch.bfloat16)
    q = Fp8Linear.from_linear(lin)
    sd = q.state_dict()
    assert sorted(sd) == ["bias", "weight", "weight_scale"]
    assert sd["weight"].dtype == F8 and sd["weight"].shape == (16, 64) and sd["weight_scale"].dtype == torch.float32 and sd["weight_scale"].shape == (16, 1)
    # codes + scales load verbatim and are NOT re-quantised: scales nobody would derive from these codes must survive
    odd = dict(sd, weight_scale=sd["weight_scale"] * 1.37, input_scale_ub=torch.tensor([1200.0]))    # (what FbgemmFp8Linear carries)
    q2 = Fp8Linear(64, 16, bias=True, dtype=torch.bfloat16)
    q2.load_state_dict(odd)
    assert _same(q2.weight, q.weight) and _same(q2.weight_scale, odd["weight_scale"]) and torch.equal(q2.bias, q.bias)
    assert sorted(q2.state_dict()) == ["bias", "weight", "weight_scale"]
    for wide in (lin.state_dict(), {k: v.float() for k, v in lin.state_dict().items()}):          # 16-bit and fp32 weights quantise on load
        q3 = Fp8Linear(64, 16, bias=True, dtype=torch.bfloat16)
        q3.load_state_dict(wide)
        assert _same(q3.weight, q.weight) and _same(q3.weight_scale, q.weight_scale)
    nan = _bytes(sd["weight"]).clone()
    nan[3, 5] = 0xff
    holder = nn.ModuleDict({"down_proj": Fp8Linear(64, 16, bias=True, dtype=torch.bfloat16)})
    with pytest.raises(ValueError, match="down_proj"):
        holder.load_state_dict({"down_proj." + k: v for k, v in dict(sd, weight=nan.view(F8)).items()})
    for cast in (lambda m: m.half(), lambda m: m.to(torch.bfloat16), lambda m: m.float(), lambda m: m.to("cpu")):
        m = cast(q3)
        assert m is q3 and _same(q3.weight, q.weight) and _same(q3.weight_scale, q.weight_scale)
        assert q3.weight.dtype == F8 and q3.weight_scale.dtype == torch.float32
    assert q3.half().bias.dtype == torch.float16 and q3.float().bias.dtype == torch.float32, "only the bias follows the activations"


def test_the_other_quantised_linears_round_trip_as_before():
    torch.manual_seed(3)
    lin = nn.Linear(64, 16, bias=True).to(torch.bfloat16)
    for cls, keys in ((Int8Linear, ["SCB", "bias", "weight"]), (MxFp4Linear, ["bias", "weight_packed", "weight_scale"])):
        q = cls.from_linear(lin)
        sd = q.state_dict()
        assert sorted(sd) == keys
        for src in (sd, lin.state_dict()):
            q2 = cls(64, 16, bias=True, dtype=torch.bfloat16)
            q2.load_state_dict(src)
            assert _same(q2.codes, q.codes) and _same(q2.scales, q.scales) and torch.equal(q2.bias, q.bias)
        q2.to(torch.float16)
        assert _same(q2.codes, q.codes) and _same(q2.scales, q.scales) and q2.bias.dtype == torch.float16


# ---- 4. quantize_fp8_ on the tiny golden model ----------------------------------------------------------------------------------------------
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
            if t.dtype == F8 or name.endswith("weight_scale"):
                quant_bytes += st.nbytes()
            elif not name.endswith("bias"):
                wide.append(name)
    return quant_bytes, wide


def _layer_bytes(model):
    return [[(_bytes(getattr(getattr(layer, o), n).weight).clone(), getattr(getattr(layer, o), n).weight_scale.clone()) for o, n in _PROJ]
            for layer in model.model.layers]


def test_quantize_fp8_replaces_the_layer_projections_and_releases_16_bit_storage():
    model, _ = _tiny(torch.bfloat16)
    model.fuse_qkv_()                                   # quantising a fused model must drop the fused 16-bit buffer too
    assert not model.is_fp8() and model.weight_format() is None
    assert model.quantize_fp8_() is model
    want, count = 0, 0
    for layer in model.model.layers:
        for owner, name in _PROJ:
            lin = getattr(getattr(layer, owner), name)
            assert type(lin) is Fp8Linear, (owner, name)
            want += lin.out_features * lin.in_features + 4 * lin.out_features
            count += 1
        assert getattr(layer.self_attn, "qkv_weight", None) is None
    assert count == 7 * len(model.model.layers)
    assert isinstance(model.lm_head, nn.Linear) and model.lm_head.weight.dtype == torch.bfloat16
    assert model.model.embed_tokens.weight.dtype == torch.bfloat16 and model.model.norm.weight.dtype == torch.bfloat16
    assert model.is_fp8() and not model.is_int8() and not model.is_mxfp4() and model.weight_format() is Fp8Linear
    scratch = {id(getattr(getattr(layer, o), n).scratch) for layer in model.model.layers for o, n in _PROJ}
    assert len(scratch) == 1 and model.model.layers[0].mlp.up_proj.scratch.numel == 96 * 64, "one scratch buffer, reserved for the largest weight"
    before = _layer_bytes(model)
    at = model.model.layers[0].self_attn
    for fused in (False, True):
        if fused:
            model.fuse_qkv_()
            assert at.qkv_weight.dtype == F8 and at.q_proj.weight.data_ptr() == at.qkv_weight.data_ptr()
            assert at.q_proj.weight_scale.data_ptr() == at.qkv_scale.data_ptr() and at.qkv_scale.shape == (at.qkv_weight.shape[0], 1)
            assert at.v_proj.weight.untyped_storage().data_ptr() == at.qkv_weight.untyped_storage().data_ptr(), "the modules keep views"
            after = _layer_bytes(model)
            assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for la, lb in zip(before, after) for a, b in zip(la, lb)), "fusing is exact"
        got, wide = _storage_census(model)
        assert got == want and not wide, (fused, got, want, wide)
    # fusing first and quantising afterwards gives the same codes and scales
    other, _ = _tiny(torch.bfloat16)
    other.quantize_fp8_().fuse_qkv_()
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for la, lb in zip(before, _layer_bytes(other)) for a, b in zip(la, lb))


def test_fp8_does_not_mix_with_the_other_quantisations():
    quant = {"fp8": "quantize_fp8_", "int8": "quantize_int8_", "mxfp4": "quantize_mxfp4_"}
    cls = {"fp8": Fp8Linear, "int8": Int8Linear, "mxfp4": MxFp4Linear}
    for have, other in (("fp8", "int8"), ("fp8", "mxfp4"), ("int8", "fp8"), ("mxfp4", "fp8")):
        m, _ = _tiny(torch.bfloat16)
        getattr(m, quant[have])()
        with pytest.raises(RuntimeError, match=have):
            getattr(m, quant[other])()
        assert m.weight_format() is cls[have] and type(m.model.layers[0].mlp.up_proj) is cls[have], "a refused call changes nothing"
        assert getattr(m, quant[have])() is m               # again on itself: nothing to do


# ---- 5. token-exact decoding on the CPU ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "beam3", "sampled"])
def test_fp8_torch_decode_matches_a_16_bit_decoder_holding_wdq(mode):
    dtype = torch.float32            # the CPU torch path; both models run the same arithmetic on the same weights
    qmodel, z = _tiny(dtype)
    qmodel.quantize_fp8_()
    twin = _wdq_twin(qmodel, lambda: _tiny(dtype)[0])
    assert twin.weight_format() is None
    emb = z["inputs_embeds"].to(dtype)
    kw = dict(attention_mask=z["attention_mask"], max_new_tokens=8, min_new_tokens=2, eos_token_id=2, pad_token_id=0, use_graph=False)
    if mode == "beam3":
        kw.update(num_beams=3, repetition_penalty=2.0, length_penalty=2.0)
    elif mode == "sampled":
        kw.update(do_sample=True, temperature=0.9, top_k=20, top_p=0.9, seed=11)
    assert torch.equal(qmodel.generate(emb, **kw), twin.generate(emb, **kw))


# ---- 6. MambaXrayVLDownStream(low_resource="fp8") -------------------------------------------------------------------------------------------
def test_downstream_low_resource_fp8_builds_fp8_layers_and_the_other_values_keep_their_meaning():
    from medical_image_analysis_amd import mambaxray_vl as mx
    from test_mambaxray_vl import WordTokenizer
    torch.manual_seed(0)
    args = mx.default_args(vision_model="Base-None", max_length=16, low_resource="fp8")
    m = mx.MambaXrayVLDownStream(args, tokenizer=WordTokenizer(), llm=mx.build_report_decoder(_tiny_llm_cfg()))
    assert m.llama_model.is_fp8() and not m.llama_model.is_int8() and not m.llama_model.is_mxfp4()
    assert type(m.llama_model.model.layers[1].mlp.up_proj) is Fp8Linear and isinstance(m.llama_model.lm_head, nn.Linear)
    assert mx.build_report_decoder(_tiny_llm_cfg(), low_resource="fp8").is_fp8()
    for low in (True, "int8"):
        args = mx.default_args(vision_model="Base-None", max_length=16, low_resource=low)
        m = mx.MambaXrayVLDownStream(args, tokenizer=WordTokenizer(), llm=mx.build_report_decoder(_tiny_llm_cfg()))
        assert m.llama_model.is_int8() and not m.llama_model.is_fp8()
        assert mx.build_report_decoder(_tiny_llm_cfg(), low_resource=low).is_int8()
    assert mx.build_report_decoder(_tiny_llm_cfg(), low_resource="mxfp4").is_mxfp4()
    assert mx.build_report_decoder(_tiny_llm_cfg(), low_resource=False).weight_format() is None


# ---- 7. descriptor validation without a GPU ---------------------------------------------------------------------------------------------
def _desc(rows=18, K=256, N=64, dtype=None, **kw):
    d = _abi.GemvDesc()
    d.rows, d.K, d.N, d.k_splits = rows, K, N, 1
    d.dtype = _abi.MXVL_BF16 | _abi.MXVL_W_FP8 if dtype is None else dtype
    d.x, d.W, d.y, d.w_scale = 0x1000, 0x2000, 0x3000, 0x4000             # fake pointers: nothing is launched
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_fp8_descriptor_validation_without_gpu():
    lib = _abi.load()
    out = (ctypes.c_int32 * 5)()
    plan = lambda d: lib.mxvl_decode_gemm_plan(ctypes.byref(d), out)
    with open(os.path.join(ROOT, "include", "mxvl.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+MXVL_W_FP8\s+0x800\b", h) and _abi.MXVL_W_FP8 == 0x800
    assert _abi.MXVL_W_FP8 & (_abi.MXVL_W_INT8 | _abi.MXVL_W_MXFP4 | _abi.MXVL_KV_FP8 | _abi.MXVL_BF16 | _abi.MXVL_F16) == 0
    assert _abi.ABI_VERSION == 13 and lib.mxvl_abi_version() == 13 and re.search(r"#define\s+MXVL_ABI_VERSION\s+13\b", h)
    for rows in (1, 3, 8, 9, 16, 17, 18, 48, 80):
        assert plan(_desc(rows=rows)) == 0 and out[0] == 5 and out[1] == 4 and out[2] in (1, 2) and out[3] >= 2 and out[4] >= 1, rows
    assert plan(_desc(rows=1, k_splits=0)) == 0 and out[0] == 5 and out[1] == 4 and out[2] in (1, 2), "no fp8 form of the <= 8-row GEMV"
    for other in (_abi.MXVL_W_INT8, _abi.MXVL_W_MXFP4, _abi.MXVL_W_INT8 | _abi.MXVL_W_MXFP4):
        for base in (_abi.MXVL_BF16, _abi.MXVL_F16, 0):
            assert plan(_desc(dtype=base | _abi.MXVL_W_FP8 | other)) == -2, "two weight flags: MXVL_ERR_DTYPE"
    for bad in (3, 7, 1 << 20, _abi.MXVL_KV_FP8 | _abi.MXVL_BF16):
        assert plan(_desc(dtype=bad | _abi.MXVL_W_FP8)) == -2, "a bad base dtype under the flag"
    assert plan(_desc(dtype=_abi.MXVL_W_FP8)) == 0 and out[0] == 5, "base dtype 0 is bf16, as everywhere"
    assert plan(_desc(w_scale=None)) == -1, "NULL scale: MXVL_ERR_NULL"
    assert plan(_desc(swiglu=1, W2=0x5000)) == -1, "w2_scale with swiglu"
    assert plan(_desc(swiglu=1, W2=0x5000, w2_scale=0x6000)) == 0 and out[0] == 5 and out[2] == 2
    assert plan(_desc(norm_weight=0x5000)) == -3, "the fused norm is refused: MXVL_ERR_SHAPE"
    assert plan(_desc(out_f32=1)) == -3
    assert plan(_desc(K=72)) == -3 and plan(_desc(K=32)) == -3 and plan(_desc(K=96)) == -3 and plan(_desc(rows=81)) < 0
    assert plan(_desc(K=64, N=16, rows=80)) == 0 and out[0] == 5
    assert plan(_desc(dtype=_abi.MXVL_F16 | _abi.MXVL_W_FP8, split_acc=0x7000, k_splits=4, y=None)) == 0 and out[0] == 5 and out[4] == 4
    # the launch entry makes the same decisions before it launches anything
    call = lambda d: lib.mxvl_decode_gemv(ctypes.byref(d), None)
    assert call(_desc(dtype=_abi.MXVL_BF16 | _abi.MXVL_W_FP8 | _abi.MXVL_W_INT8)) == -2 and call(_desc(dtype=3 | _abi.MXVL_W_FP8)) == -2
    assert call(_desc(w_scale=None)) == -1 and call(_desc(norm_weight=0x5000)) == -3 and call(_desc(K=72)) == -3
    # int8 and fp8 share one plan; the other storages plan as before
    for shape in (dict(), dict(rows=80, K=4096, N=4096, split_acc=0x7000, k_splits=4), dict(rows=3, K=4096, N=11008, swiglu=1, W2=0x5000, w2_scale=0x6000)):
        assert plan(_desc(**shape)) == 0
        fp8 = list(out)
        assert plan(_desc(dtype=_abi.MXVL_BF16 | _abi.MXVL_W_INT8, **shape)) == 0 and out[0] == 3 and list(out)[1:] == fp8[1:]
    assert plan(_desc(dtype=_abi.MXVL_BF16 | _abi.MXVL_W_MXFP4)) == 0 and out[0] == 4
    assert plan(_desc(dtype=_abi.MXVL_BF16)) == 0 and out[0] in (0, 1)
    assert plan(_desc(dtype=_abi.MXVL_BF16, rows=2, k_splits=0)) == 0 and out[0] == 2


# ---- 8 / 9. the projection against float64 -----------------------------------------------------------------------------------------------
_GUARD, _SENTINEL = 256, -12288.0        # elements on each side of an output (a multiple of every store width: the base stays aligned);
                                         # -1.5 * 2^13 is exact in bf16, fp16 and fp32
_FINITE = torch.tensor([b for b in range(256) if (b & 0x7f) != 0x7f], dtype=torch.uint8)        # the 254 non-NaN bytes


def _codes(N, K, g):
    """Hand-made codes, not only what the quantiser produces: uniform non-NaN bytes, every one of the 254 of them at least once
    (+-0, the subnormals, +-448 included), row 0 all -448."""
    cb = _FINITE[torch.randint(0, 254, (N * K,), generator=g)]
    cb[K:K + 254] = _FINITE
    cb = cb.view(N, K)
    cb[0, :] = 0xfe
    assert len(torch.unique(cb)) == 254
    return cb


def _guarded(shape, dtype, dev, fill=None):
    """A tensor of `shape` inside a larger allocation whose margins hold a sentinel; returns (tensor, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * _GUARD,), _SENTINEL, dtype=dtype, device=dev)
    inner = buf[_GUARD:_GUARD + n]
    if fill is not None:
        inner.fill_(fill)
    return inner.view(shape), buf


def _guards_intact(buf):
    return bool((buf[:_GUARD] == _SENTINEL).all()) and bool((buf[-_GUARD:] == _SENTINEL).all())


def _launch(x, cb, sc, y=None, cb2=None, sc2=None, bias=None, res=None, acc=None, splits=1):
    d = _abi.GemvDesc()
    d.rows, d.K, d.N = x.shape[0], x.shape[1], cb.shape[0]
    d.dtype = _abi.dtype_code(x.dtype) | _abi.MXVL_W_FP8
    d.x, d.W, d.w_scale, d.y = x.data_ptr(), cb.data_ptr(), sc.data_ptr(), _abi.ptr(y)
    d.W2, d.w2_scale, d.swiglu = _abi.ptr(cb2), _abi.ptr(sc2), int(cb2 is not None)
    d.bias, d.residual = _abi.ptr(bias), _abi.ptr(res)
    d.k_splits = splits if acc is not None else 0                     # 0: by row count -- must still take the fp8 kernel
    d.split_acc = _abi.ptr(acc)
    _abi.launch("mxvl_decode_gemv", d, device=x.device)


def _check_projection(rows, K, N, dtype, epi, splits=1):
    """tests/test_int8_decode.py::_check_projection with |value of the code| in place of |CB| and s = w_scale.  Per element: E4M3 ->
    16-bit conversion and every product are exact, so the fp32 sum of K terms is within K * 2^-24 * s[n] * sum_k |v x| of the exact one
    (first-order bound of any summation order; the one rounding of s * sum is inside it for K >= 64), plus the output-dtype ulps
    that function lists per epilogue -- one at |y|; bias + residual one more at the value rounded before the residual add; swiglu the
    first-order propagation through silu(a) * b.  split_acc: the fp32 bound only.
    Scales: int8's test draws the row ABSMAX as (rand * 2 + 0.05) * 4 / sqrt(K) and its kernel multiplies by absmax / 127; the row
    scale of this format is absmax / 448 (quantize_rowwise_fp8), so that is what w_scale holds here -- the same layer, outputs of
    O(1), |a| under ~25 in the all -448 row, for the reason that test's comment gives: past |a| ~ 88 the SwiGLU epilogue's fp32
    exp(-a) overflows and the first-order formula no longer describes silu(a) b."""
    g = torch.Generator().manual_seed(rows * 131 + K + N)
    dev = torch.device(DEV)
    amp = 4.0 / K ** 0.5
    cb, sc = _codes(N, K, g), (torch.rand(N, generator=g) * 2 + 0.05) * amp / 448.0
    x = torch.randn(rows, K, generator=g).to(dtype)
    v = torch.from_numpy(E4M3)[cb.long()]                             # float64 values of the codes, from the bit fields
    xd, s = x.double(), sc.double()
    a = (xd @ v.t()) * s
    bound_a = K * 2.0 ** -24 * (xd.abs() @ v.abs().t()) * s
    xg, cbg, scg = x.to(dev), cb.to(dev), sc.to(dev)
    if epi == "split":
        acc, buf = _guarded((splits, rows, N), torch.float32, dev, fill=float("nan"))
        _launch(xg, cbg, scg, acc=acc, splits=splits)
        got = acc.double().sum(0).cpu()
        assert torch.isfinite(got).all(), "every element of every plane is written"
        err, tol = (got - a).abs(), bound_a
    elif epi == "swiglu":
        cb2, sc2 = _codes(N, K, g), (torch.rand(N, generator=g) + 0.05) * amp / 448.0
        v2 = torch.from_numpy(E4M3)[cb2.long()]
        b = (xd @ v2.t()) * sc2.double()
        bound_b = K * 2.0 ** -24 * (xd.abs() @ v2.abs().t()) * sc2.double()
        y, buf = _guarded((rows, N), dtype, dev)
        _launch(xg, cbg, scg, y=y, cb2=cb2.to(dev), sc2=sc2.to(dev))
        sig = torch.sigmoid(a)
        silu, dsilu = a * sig, sig * (1 + a * (1 - sig))
        want = silu * b
        tol = dsilu.abs() * b.abs() * (bound_a + _ulp(a, dtype)) + silu.abs() * (bound_b + _ulp(b, dtype)) \
            + _ulp(silu, dtype) * b.abs() + _ulp(want, dtype)
        err = (y.double().cpu() - want).abs()
    else:
        bias = torch.randn(N, generator=g).to(dtype)
        res = torch.randn(rows, N, generator=g).to(dtype) if epi == "bias_res" else None
        y, buf = _guarded((rows, N), dtype, dev)
        _launch(xg, cbg, scg, y=y, bias=bias.to(dev), res=None if res is None else res.to(dev))
        lin = a + bias.double()
        want = lin if res is None else lin + res.double()
        tol = bound_a + _ulp(want, dtype) + (_ulp(lin, dtype) if res is not None else 0.0)
        err = (y.double().cpu() - want).abs()
    assert _guards_intact(buf), (rows, K, N, dtype, epi, splits, "a store outside the output")
    worst = float((err / tol).max())
    print(f"fp8 projection rows={rows} K={K} N={N} {dtype} {epi} splits={splits}: max err / tol = {worst:.3f}")
    assert worst <= 1.0, (rows, K, N, dtype, epi, splits, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("epi", ["bias", "bias_res", "swiglu", "split2", "split4", "split8"])
def test_fp8_projection_against_float64(dtype, epi):
    """int8's grid of rows x K x N and its tails for one dtype and epilogue (77 launches of a few microseconds each)."""
    splits = int(epi[5:]) if epi.startswith("split") else 1
    for rows in _ROWS:
        for K in _KS:
            if K // 64 < splits:
                continue
            for N in _NS:
                _check_projection(rows, K, N, dtype, "split" if splits > 1 else epi, splits=splits)
    for rows, K, N in _TAIL:
        if K // 64 >= splits:
            _check_projection(rows, K, N, dtype, "split" if splits > 1 else epi, splits=splits)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,K,N,epi,splits", [(18, 4096, 4096, "split", 4), (80, 4096, 4096, "split", 4), (3, 4096, 4096, "split", 4),
                                                 (18, 4096, 11008, "swiglu", 1), (80, 4096, 11008, "swiglu", 1), (3, 4096, 11008, "swiglu", 1),
                                                 (18, 4096, 12288, "bias", 1), (80, 11008, 4096, "split", 8)])
def test_fp8_projection_real_widths(rows, K, N, epi, splits):
    """One real-width case per plan the dispatch chooses: the cases of test_int8_projection_real_widths."""
    _check_projection(rows, K, N, torch.bfloat16, epi, splits=splits)


# ---- 10. end to end ---------------------------------------------------------------------------------------------------------------------------
def _record_gemv_dtypes(monkeypatch):
    seen, real = [], _abi.launch

    def launch(name, first, *rest, **kw):
        if name == "mxvl_decode_gemv":
            seen.append(int(first.dtype))
        return real(name, first, *rest, **kw)
    monkeypatch.setattr(_abi, "launch", launch)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["greedy", "beam3", "sampled", "greedy_kv8"])
def test_fp8_kernel_stepper_end_to_end(mode, monkeypatch):
    """generate() on the kernel stepper (captured graph) against use_graph="torch" on the same device, bf16, token for token: the
    comparison and the near-tie rule of test_int8_decode.py::test_quantised_kernel_stepper_end_to_end (a case counts only if the
    eager torch path on the CPU gives the same tokens in bf16 and in fp32; asserted, never skipped).  greedy_kv8: the same with
    kv_cache_dtype="fp8".  The step's mxvl_decode_gemv launches must carry the FP8 bit for the seven layer projections (four
    launches per layer) and not for lm_head."""
    dtype = torch.bfloat16
    kw = _e2e_kwargs(mode.split("_")[0])
    if mode.endswith("kv8"):
        kw["kv_cache_dtype"] = "fp8"
    cpu16 = _servable(dtype).quantize_fp8_().generate(_e2e_prompt(dtype), use_graph=False, **kw)
    cpu32 = _servable(dtype).quantize_fp8_().float().generate(_e2e_prompt(dtype).float(), use_graph=False, **kw)   # same codes and scales
    assert torch.equal(cpu16, cpu32), f"{mode}: the torch-path decode of this case sits on a near-tie; pick another prompt"
    qmodel = _servable(dtype).quantize_fp8_().to(DEV)
    assert qmodel.is_fp8() and _KernelStepper.supported(qmodel, 6, dtype, DEV, kw.get("kv_cache_dtype"))
    emb = _e2e_prompt(dtype).to(DEV)
    ref = qmodel.generate(emb, use_graph="torch", **kw)
    qmodel.__dict__.pop("_steppers", None)              # (the torch-module stepper of the call above)
    seen = _record_gemv_dtypes(monkeypatch)
    got = qmodel.generate(emb, use_graph=True, **kw)
    assert all(type(s) is _KernelStepper and s.fp8 and not s.int8 and not s.mxfp4 and not s.fused_norm and s.kv8 == mode.endswith("kv8")
               for s in qmodel._steppers.values()) and len(qmodel._steppers) == 1
    flagged = [d for d in seen if d & _abi.MXVL_W_FP8]
    assert flagged and all(d == (_abi.MXVL_BF16 | _abi.MXVL_W_FP8) for d in flagged), "mxvl_decode_gemv was reached with the FP8 bit"
    assert len(flagged) == 4 * 2 * (len(seen) - len(flagged)), "four fp8 launches per layer, two layers, one 16-bit lm_head per step"
    assert torch.equal(got.cpu(), ref.cpu()), (mode, got.tolist(), ref.tolist())


@pytest.mark.gpu
def test_fp8_kernel_step_logits_without_graph():
    """The first decode step of an fp8 model on the kernel stepper, run eagerly (no captured graph), against the torch modules on the
    same device: within 8 output-dtype ulps at the logit row's maximum, the figure of
    test_int8_decode.py::test_quantised_kernel_step_logits_without_graph."""
    dtype = torch.bfloat16
    qmodel = _servable(dtype).quantize_fp8_().to(DEV)
    emb = _e2e_prompt(dtype).to(DEV)
    logits0, cache = _prefill(qmodel, emb)
    tok = logits0.argmax(-1)
    st = _KernelStepper(qmodel, 2, torch.ones(2, 6, dtype=torch.long, device=DEV), cache, 8, dtype)
    assert st.fp8 and not st.fused_norm and st.graph is None
    lk = st._body(tok, torch.arange(2, device=DEV), torch.ones(1, dtype=torch.long, device=DEV)).clone()
    attn = torch.ones(2, 7, dtype=torch.long, device=DEV)
    with torch.no_grad():
        lt = qmodel.forward(qmodel.model.embed_tokens(tok)[:, None, :], attention_mask=attn, past_key_values=cache)[:, -1].float()
    tol = 8 * 2.0 ** -7 * lt.abs().amax(-1, keepdim=True)          # 8 bf16 ulps (relative 2^-7 at the row's max)
    worst = float(((lk - lt).abs() / tol).max())
    print(f"fp8 first-step logits, kernel vs torch: max err / tol = {worst:.3f}")
    assert worst <= 1.0


def test_stepper_identity_tells_an_fp8_decoder_from_an_int8_one():
    """generate() keys its stepper cache on (data_ptr, dtype) of the last down_proj's codes: the dtype differs between the storages
    even where an allocator hands the same address to both."""
    a, b = _servable(torch.bfloat16).quantize_fp8_(), _servable(torch.bfloat16).quantize_int8_()
    from medical_image_analysis_amd.report_decoder import _codes as codes_of
    ca, cb = codes_of(a.model.layers[-1].mlp.down_proj), codes_of(b.model.layers[-1].mlp.down_proj)
    assert ca.shape == cb.shape and ca.dtype == F8 and cb.dtype == torch.int8


# ---- 11. what the kernels cannot serve -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fp8_decoder_with_unserved_width_takes_torch_or_raises():
    torch.manual_seed(0)
    model = ReportDecoder(vocab_size=64, hidden_size=160, intermediate_size=192, num_hidden_layers=1, num_attention_heads=2,
                          num_key_value_heads=2).to(torch.bfloat16).to(DEV).eval()        # hidden % 64 != 0 (head_dim 80 is unserved anyway)
    plain_ok = ReportDecoder(vocab_size=64, hidden_size=128, intermediate_size=160, num_hidden_layers=1, num_attention_heads=2,
                             num_key_value_heads=2).to(torch.bfloat16).to(DEV).eval()     # head_dim 64, intermediate % 64 != 0
    assert _KernelStepper.supported(plain_ok, 2, torch.bfloat16, DEV)
    plain_ok.quantize_fp8_()
    assert not _KernelStepper.supported(plain_ok, 2, torch.bfloat16, DEV)
    for m in (model.quantize_fp8_(), plain_ok):
        emb = torch.randn(1, 4, m.config.hidden_size, device=DEV, dtype=torch.bfloat16)
        out = m.generate(emb, max_new_tokens=4, use_graph="torch")
        assert out.shape == (1, 4)
        with pytest.raises(RuntimeError, match="pass use_graph"):
            m.generate(emb, max_new_tokens=4, use_graph=True)
