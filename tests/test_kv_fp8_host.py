"""kv_cache_dtype="fp8" without a GPU: the quantiser (one power-of-two scale per layer and tensor, OCP float8_e4m3fn codes), the
`generate` argument on the CPU eager path, and the C-ABI surface (MXVL_KV_FP8, mxvl_decode_attn_desc.kv_scale, the refusals that come
before any launch)."""
import ctypes
import math
import os
import re

import pytest
import torch

from medical_image_analysis_amd import _abi
from medical_image_analysis_amd.report_decoder import (KVCache, ReportDecoder, kv_fp8_encode, kv_fp8_fake_quant, kv_fp8_scale)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _finite_codes():
    """All 254 finite E4M3 codes (0x7f / 0xff are NaN) as a float8 tensor."""
    b = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
    assert b.numel() == 254
    return b.view(torch.float8_e4m3fn)


# ---- quantiser ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,lo,hi", [(torch.float16, -15, 7), (torch.bfloat16, -100, 100)], ids=["fp16", "bf16"])
def test_every_finite_code_round_trips_under_every_allowed_scale(dtype, lo, hi):
    """code -> code * 2^j in the cache's 16-bit dtype -> code: decode is exact (the fp32 product already is a 16-bit value) and the
    encoder finds the code again, over the whole exponent range the scale rule may choose."""
    codes = _finite_codes()
    for j in range(lo, hi + 1):
        s = torch.tensor(2.0 ** j, dtype=torch.float32)
        exact = codes.float() * s
        x = exact.to(dtype)
        assert torch.equal(x.float(), exact), f"code x 2^{j} is not exact in {dtype}"
        back = kv_fp8_encode(x, s)
        # +0 and -0 keep their sign bit too
        assert torch.equal(back.view(torch.uint8), codes.view(torch.uint8)), f"2^{j}"


def test_encode_saturates_and_fake_quant_is_idempotent():
    s = torch.tensor(0.25)
    x = torch.tensor([1e4, -1e4, 448.0 * 0.25, 449.0 * 0.25, 464.0 * 0.25, -480.0 * 0.25, 65504.0, float("inf"), -float("inf")])
    code = kv_fp8_encode(x, s)
    assert torch.equal(code.float(), torch.tensor([448.0, -448.0, 448.0, 448.0, 448.0, -448.0, 448.0, 448.0, -448.0]))
    # the cast alone would not saturate: this is why the clamp is part of the contract
    assert torch.isnan(torch.tensor([1e4]).to(torch.float8_e4m3fn).float()).all()
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        y = (torch.randn(4096, generator=g) * 3).to(dtype)
        sc = kv_fp8_scale(y)
        once = kv_fp8_fake_quant(y, sc)
        assert once.dtype == dtype and torch.equal(kv_fp8_fake_quant(once, sc), once)
        # on the grid: every value is a code times the scale, within half a step of the input
        assert float((once.float() - y.float()).abs().max()) <= 2.0 ** -4 * float(y.float().abs().max())


def test_scale_rule():
    """j = ceil(log2(amax / 224)), clamped to the dtype's exact range, 0 for amax = 0 / inf / NaN -- checked against float64."""
    def j_of(vals, dtype):
        s = float(kv_fp8_scale(torch.tensor(vals).to(dtype)))
        j = math.log2(s)
        assert j == int(j), "a power of two"
        return int(j)
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        assert j_of([0.0, -0.0], dtype) == 0
        assert j_of([1.0, float("inf")], dtype) == 0 and j_of([-float("inf")], dtype) == 0 and j_of([float("nan"), 2.0], dtype) == 0
        for k in (-6, -1, 0, 1, 5):
            at = 224.0 * 2.0 ** k                       # exactly a power of two times 224: amax / 224 = 2^k
            ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
            assert j_of([at, -at / 2], dtype) == k
            assert j_of([at * (1 + ulp)], dtype) == k + 1           # just above (1.75 * (1 + ulp) is a value of every dtype here)
            assert j_of([-at * (1 - ulp / 2)], dtype) == k          # just below
        # the largest code is 448 = 2 * 224: the prompt's amax lands in (112, 224] code units
        x = torch.tensor([3.0, -7.5, 0.01]).to(dtype)
        assert 112.0 < float(x.float().abs().max() / kv_fp8_scale(x)) <= 224.0
    # clamped to where code x 2^j is exact in the cache dtype
    assert j_of([60000.0], torch.float16) == 7 and j_of([2.0 ** -24], torch.float16) == -15
    assert j_of([2.0 ** 120], torch.bfloat16) == 100 and j_of([2.0 ** -120], torch.bfloat16) == -100
    # against float64 on random magnitudes
    g = torch.Generator().manual_seed(1)
    for v in (torch.rand(200, generator=g) * 16 - 8).exp2().tolist():
        x = torch.tensor([v]).to(torch.bfloat16)
        assert j_of([float(x)], torch.bfloat16) == math.ceil(math.log2(float(x) / 224.0))


# ---- generate(kv_cache_dtype=...) on the CPU eager path ----------------------------------------------------------------------------
def _tiny(dtype=torch.bfloat16):
    torch.manual_seed(7)
    return ReportDecoder(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2,
                         num_key_value_heads=2, rms_norm_eps=1e-6, max_position_embeddings=128).to(dtype).eval()


def _prompt(dtype=torch.bfloat16):
    return torch.randn(2, 6, 128, generator=torch.Generator().manual_seed(5)).to(dtype)


KW = dict(max_new_tokens=8, min_new_tokens=2, eos_token_id=2, pad_token_id=0)


def _restated_update(self, k, v, layer_idx, cache_kwargs=None):
    """An independent restatement of the contract for a plain KVCache: python floats for the scale, torch only for the cast."""
    scales = self.__dict__.setdefault("_restated", {})
    lo, hi = (-15, 7) if k.dtype == torch.float16 else (-100, 100)
    if layer_idx not in scales:
        pair = []
        for t in (k, v):
            amax = float(t.double().abs().max())
            j = math.ceil(math.log2(amax / 224.0)) if (amax > 0 and math.isfinite(amax)) else 0
            pair.append(2.0 ** min(max(j, lo), hi))
        scales[layer_idx] = pair
    out = []
    for t, s in zip((k, v), scales[layer_idx]):
        code = torch.clamp(t.double() / s, -448.0, 448.0).float().to(torch.float8_e4m3fn)
        out.append((code.double() * s).to(t.dtype))
    k, v = out
    if layer_idx in self.k:
        k = torch.cat([self.k[layer_idx], k], dim=-2)
        v = torch.cat([self.v[layer_idx], v], dim=-2)
    self.k[layer_idx], self.v[layer_idx] = k, v
    return k, v


@pytest.mark.parametrize("mode", ["greedy", "beam3", "sampled"])
def test_generate_fp8_equals_a_twin_with_restated_fake_quant(monkeypatch, mode):
    kw = dict(KW)
    if mode == "beam3":
        kw.update(num_beams=3, repetition_penalty=2.0, length_penalty=2.0)
    elif mode == "sampled":
        kw.update(do_sample=True, temperature=0.9, top_k=20, top_p=0.9, seed=11)
    m = _tiny()
    plain = m.generate(_prompt(), use_graph=False, **kw)
    got = m.generate(_prompt(), use_graph=False, kv_cache_dtype="fp8", **kw)
    assert torch.equal(m.generate(_prompt(), use_graph=False, kv_cache_dtype=None, **kw), plain)
    assert torch.equal(m.generate(_prompt(), use_graph=False, kv_cache_dtype="auto", **kw), plain)
    monkeypatch.setattr(KVCache, "update", _restated_update)
    twin = _tiny().generate(_prompt(), use_graph=False, **kw)           # a 16-bit call whose cache fake-quantises by the restatement
    assert torch.equal(got, twin), (got.tolist(), twin.tolist())


def test_fp8_changes_what_the_cache_holds():
    """The mode is not a no-op: the cached values sit on the E4M3 grid of the layer's scale (and the 16-bit ones do not)."""
    m = _tiny()
    caches = {}
    for mode in (None, "fp8"):
        c = caches[mode] = KVCache(mode)
        with torch.no_grad():
            m.forward(_prompt(), attention_mask=torch.ones(2, 6, dtype=torch.long), past_key_values=c)
    c = caches["fp8"]
    assert sorted(c.scale) == [0, 1] and all(t.shape == (2,) and t.dtype == torch.float32 for t in c.scale.values())
    for i in c.k:
        for t, s in ((c.k[i], c.scale[i][0]), (c.v[i], c.scale[i][1])):
            assert torch.equal(kv_fp8_fake_quant(t, s), t)
            assert float(t.float().abs().max() / s) <= 224.0
    assert not torch.equal(caches[None].k[0], c.k[0])


@pytest.mark.parametrize("bad", ["int8", "fp8_e5m2", 8, True, "", torch.float8_e4m3fn])
def test_bad_kv_cache_dtype_raises_before_anything_is_built(bad):
    m = _tiny()
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        m.generate(_prompt(), use_graph=False, num_beams=3, kv_cache_dtype=bad, **KW)
    assert "_beam_states" not in m.__dict__ and "_steppers" not in m.__dict__


def test_downstream_args_carry_kv_cache_dtype():
    from medical_image_analysis_amd.mambaxray_vl import default_args
    assert default_args().kv_cache_dtype is None and default_args(kv_cache_dtype="fp8").kv_cache_dtype == "fp8"


def test_kernel_stepper_refuses_head_dim_256_with_fp8():
    """`supported` is asked for a HIP device (it loads the library, which needs no GPU): head_dim 256 is served in 16 bits only."""
    from medical_image_analysis_amd.report_decoder import _KernelStepper
    torch.manual_seed(0)
    m = ReportDecoder(vocab_size=32, hidden_size=512, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1, rms_norm_eps=1e-6, max_position_embeddings=64).to(torch.bfloat16)
    assert _KernelStepper.supported(m, 2, torch.bfloat16, "cuda:0") is True
    assert _KernelStepper.supported(m, 2, torch.bfloat16, "cuda:0", "auto") is True
    assert _KernelStepper.supported(m, 2, torch.bfloat16, "cuda:0", "fp8") is False
    assert _KernelStepper.supported(_tiny(), 6, torch.bfloat16, "cuda:0", "fp8") is True


# ---- descriptor and refusals (no GPU: every check below returns before a launch) ------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "mxvl.h")) as f:
        return f.read()


def test_descriptor_mirrors_the_header():
    h = _header()
    assert re.search(r"#define\s+MXVL_KV_FP8\s+0x400\b", h) and _abi.MXVL_KV_FP8 == 0x400
    assert _abi.MXVL_KV_FP8 & (_abi.MXVL_W_INT8 | _abi.MXVL_W_MXFP4 | _abi.MXVL_BF16 | _abi.MXVL_F16) == 0
    body = re.search(r"typedef struct mxvl_decode_attn_desc \{(.*?)\} mxvl_decode_attn_desc;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].lstrip("*") for n in names]
    assert names == [n for n, _ in _abi.DecodeAttnDesc._fields_]
    assert names[-1] == "kv_scale" and names[-2] == "dtype", "the new field trails the struct"
    assert _abi.DecodeAttnDesc.kv_scale.offset == 112 and ctypes.sizeof(_abi.DecodeAttnDesc) == 120
    # ABI surface: nothing else moved
    assert _abi.ABI_VERSION == 13 and re.search(r"#define\s+MXVL_ABI_VERSION\s+13\b", h)
    assert len(set(re.findall(r"\b(mxvl_\w+)\s*\([^)]*\bvoid\s*\*\s*hip_stream\s*\)\s*;", h))) == 43


def _desc(dtype, head_dim=128, kv_scale=0x9000):
    a = _abi.DecodeAttnDesc()
    a.rows, a.n_heads, a.n_kv_heads, a.head_dim, a.max_len, a.scale, a.beams = 2, 2, 2, head_dim, 32, head_dim ** -0.5, 0
    a.dtype = dtype
    # fake device pointers: the calls below return before anything is launched or read
    a.qkv, a.cos, a.sin, a.k_cache, a.v_cache = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.slot_table, a.pos, a.mask, a.out = 0x6000, 0x7000, 0x8000, 0xa000
    a.kv_scale = kv_scale
    return a


def test_decode_attn_refusals_with_the_flag():
    lib = _abi.load()
    assert lib.mxvl_abi_version() == 13
    F = _abi.MXVL_KV_FP8
    call = lambda a: lib.mxvl_decode_attn(ctypes.byref(a), None)
    assert call(_desc(_abi.MXVL_BF16 | F, kv_scale=None)) == -1, "the flag without kv_scale: MXVL_ERR_NULL"
    assert call(_desc(F, kv_scale=None)) == -1, "dtype 0 (bf16) | flag"
    for w in (_abi.MXVL_W_INT8, _abi.MXVL_W_MXFP4):
        assert call(_desc(_abi.MXVL_BF16 | F | w)) == -2, "the flag beside a weight flag: MXVL_ERR_DTYPE"
        assert call(_desc(_abi.MXVL_F16 | w)) == -2
    for bad in (3, 7, 1 << 20):
        assert call(_desc(bad | F)) == -2 and call(_desc(bad)) == -2
    assert call(_desc(-1)) == -2
    assert call(_desc(_abi.MXVL_BF16 | F, head_dim=256)) == -7, "no fp8-cache kernel at head_dim 256: MXVL_ERR_UNSUPPORTED"
    assert call(_desc(_abi.MXVL_F16 | F, head_dim=256)) == -7
    assert call(_desc(_abi.MXVL_BF16 | F, head_dim=96)) == -7


def test_other_decode_entries_refuse_the_flag():
    lib = _abi.load()
    d = _abi.GemvDesc()
    d.rows, d.K, d.N = 2, 64, 64
    d.x, d.W, d.y = 0x1000, 0x2000, 0x3000
    for base in (_abi.MXVL_BF16, _abi.MXVL_F16, _abi.MXVL_BF16 | _abi.MXVL_W_INT8):
        d.dtype = base | _abi.MXVL_KV_FP8
        assert lib.mxvl_decode_gemv(ctypes.byref(d), None) == -2
    n = _abi.RmsNormDesc()
    n.rows, n.K, n.eps = 2, 64, 1e-6
    n.x, n.weight, n.y = 0x1000, 0x2000, 0x3000
    for base in (_abi.MXVL_BF16, _abi.MXVL_F16):
        n.dtype = base | _abi.MXVL_KV_FP8
        assert lib.mxvl_decode_rmsnorm(ctypes.byref(n), None) == -2
