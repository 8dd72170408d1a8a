"""Llama-3.x and Qwen3 checkpoints without a GPU: HF parity of the two tiny goldens (tests/golden/make_golden_families.py), the llama3
`inv_freq` bit for bit, `build_report_decoder` reading `head_dim` / `model_type` / the RoPE scaling in both spellings and refusing what
is not built, and the C-ABI surface of MXVL_QK_NORM (mxvl_decode_attn_qknorm_desc, the refusals that come before any launch)."""
import ctypes
import json
import os
import re
import sys

import pytest
import torch

from conftest import assert_close, load_golden
from medical_image_analysis_amd import _abi
from medical_image_analysis_amd.mambaxray_vl import build_report_decoder
from medical_image_analysis_amd.report_decoder import ReportDecoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_families as fam  # noqa: E402


def _tiny(name, dtype=torch.float32, dev="cpu"):
    g = load_golden(name)
    if name == "decode_tiny_qwen3":
        m = ReportDecoder(rms_norm_eps=1e-6, max_position_embeddings=128, qk_norm=True, **fam.TINY_QWEN3)
    else:
        m = ReportDecoder(rms_norm_eps=1e-6, max_position_embeddings=128, rope_theta=fam.LLAMA3_THETA, rope_scaling=fam.LLAMA3_ROPE,
                          **fam.TINY_LLAMA3)
    m.load_hf_state_dict({k[2:]: v.view(torch.bfloat16).float() for k, v in g.items() if k.startswith("p_")})
    return g, m.to(dev).to(dtype).eval()


# ---- HF parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["decode_tiny_qwen3", "decode_tiny_llama3"])
def test_tiny_family_fp32_path_matches_hf(name):
    """fp32 torch path: prompt logits under the tolerance of test_keyed_fp32_path_matches_hf, greedy and beam-3 streams exactly."""
    g, m = _tiny(name)
    emb, att = g["inputs_embeds"], g["attention_mask"]
    with torch.no_grad():
        logits = m(emb, attention_mask=att)
    scale = float(g["logits_prompt"].abs().max())
    assert_close(logits, g["logits_prompt"], 3e-5 * scale, 1e-4, "prompt logits")
    for key, kw in (("greedy", fam.GREEDY), ("beam3", fam.BEAM)):
        out = m.generate(emb, attention_mask=att, use_graph=False, **kw, **fam.GEN)
        assert torch.equal(out, g[key]), f"{key}: {out.tolist()} vs HF {g[key].tolist()}"


def test_tiny_qwen3_is_not_a_qwen2_shape():
    g, m = _tiny("decode_tiny_qwen3")
    cfg = m.config
    assert cfg.head_dim == 64 and cfg.head_dim * cfg.num_attention_heads == 128 != cfg.hidden_size and cfg.qk_norm
    at = m.model.layers[0].self_attn
    assert at.q_proj.weight.shape == (128, 64) and at.k_proj.weight.shape == (64, 64) and at.o_proj.weight.shape == (64, 128)
    assert at.q_norm.weight.shape == at.k_norm.weight.shape == (64,) and not torch.equal(at.q_norm.weight, torch.ones(64))
    assert float(g["margin"]) > 0.012 * float(g["logit_scale"])


def test_llama3_inv_freq_is_hfs_bits_and_all_three_bands_occur():
    g, m = _tiny("decode_tiny_llama3")
    inv = m.model.rotary_emb.inv_freq
    assert inv.dtype == torch.float32 and torch.equal(inv, g["inv_freq"])
    for layer in m.model.layers:
        assert torch.equal(layer.self_attn.rotary_emb.inv_freq, g["inv_freq"])
    plain = ReportDecoder(rope_theta=fam.LLAMA3_THETA, **fam.TINY_LLAMA3).model.rotary_emb.inv_freq
    ratio = plain / inv
    f = fam.LLAMA3_ROPE["factor"]
    assert (ratio == 1).any() and (ratio == f).any() and ((ratio > 1) & (ratio < f)).any()
    assert m.model.rotary_emb.attention_scaling == 1.0
    assert float(g["unscaled_logit_diff"]) > 1e-2 * float(g["logit_scale"]), "the scaling must matter at these positions"
    assert float(g["margin"]) > 0.012 * float(g["logit_scale"])


def test_default_rope_spellings_and_unknown_types():
    base = dict(vocab_size=32, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=4)
    ref = ReportDecoder(**base).model.rotary_emb.inv_freq
    for rs in (None, {"rope_type": "default"}, {"type": "default"}):
        assert torch.equal(ReportDecoder(rope_scaling=rs, **base).model.rotary_emb.inv_freq, ref)
    for kind in ("linear", "dynamic", "yarn", "longrope"):
        with pytest.raises(NotImplementedError, match=kind):
            ReportDecoder(rope_scaling={"rope_type": kind, "factor": 2.0}, **base)


def test_head_dim_default_and_divisibility():
    m = ReportDecoder(vocab_size=32, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=4)
    assert m.config.head_dim == 16 and m.config.qk_norm is False and m.config.rope_scaling is None
    assert not any("q_norm" in k or "k_norm" in k for k in m.state_dict())
    with pytest.raises(ValueError, match="divisible"):
        ReportDecoder(vocab_size=32, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=3)
    m = ReportDecoder(vocab_size=32, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=3, head_dim=32)
    assert m.model.layers[0].self_attn.o_proj.weight.shape == (64, 96)


def test_norm_weights_are_unexpected_without_qk_norm():
    shape = dict(fam.TINY_QWEN3)
    src = ReportDecoder(qk_norm=True, **shape)
    sd = src.state_dict()
    assert sum(k.endswith(("q_norm.weight", "k_norm.weight")) for k in sd) == 4
    ReportDecoder(qk_norm=True, **shape).load_hf_state_dict(sd)
    with pytest.raises(RuntimeError, match="unexpected.*q_norm"):
        ReportDecoder(**shape).load_hf_state_dict(sd)
    with pytest.raises(RuntimeError, match="missing.*q_norm"):
        ReportDecoder(qk_norm=True, **shape).load_hf_state_dict({k: v for k, v in sd.items() if "_norm.weight" not in k or "layernorm" in k})


def test_kernel_stepper_support_follows_head_dim():
    """`supported` is asked for a HIP device (it loads the library, which needs no GPU)."""
    from medical_image_analysis_amd.report_decoder import _KernelStepper
    shape = dict(fam.QWEN3_HD128, num_hidden_layers=1)
    m = ReportDecoder(qk_norm=True, **shape).to(torch.bfloat16)
    assert m.config.hidden_size // m.config.num_attention_heads == 64 and m.config.head_dim == 128
    assert _KernelStepper.supported(m, 6, torch.bfloat16, "cuda:0") is True
    assert _KernelStepper.supported(m, 6, torch.bfloat16, "cuda:0", "fp8") is True
    # hidden / heads would be a served 64, head_dim 32 is not: the range is decided by config.head_dim
    m = ReportDecoder(**dict(shape, head_dim=32)).to(torch.bfloat16)
    assert _KernelStepper.supported(m, 6, torch.bfloat16, "cuda:0") is False
    m = ReportDecoder(**dict(shape, head_dim=256, num_attention_heads=2, num_key_value_heads=1)).to(torch.bfloat16)
    assert _KernelStepper.supported(m, 6, torch.bfloat16, "cuda:0") is True
    assert _KernelStepper.supported(m, 6, torch.bfloat16, "cuda:0", "fp8") is False


# ---- build_report_decoder on checkpoint directories ------------------------------------------------------------------------------------
LLAMA_CFG = dict(fam.TINY_LLAMA3, rms_norm_eps=1e-6, max_position_embeddings=128)
QWEN3_CFG = dict(fam.TINY_QWEN3, rms_norm_eps=1e-6, max_position_embeddings=128)


def _write(tmp_path, name, config, model):
    from safetensors.torch import save_file
    d = tmp_path / name
    d.mkdir()
    (d / "config.json").write_text(json.dumps(config))
    save_file({k: v.contiguous() for k, v in model.state_dict().items() if not k.endswith("_proj.bias")}, str(d / "model.safetensors"))
    return str(d)


@pytest.mark.parametrize("spelling", ["rope_scaling", "rope_parameters"])
def test_build_reads_the_llama3_rope_in_both_spellings(tmp_path, spelling):
    g, src = _tiny("decode_tiny_llama3")
    hf = {k: v for k, v in fam.LLAMA3_ROPE.items()}
    cfg = dict(LLAMA_CFG, model_type="llama", architectures=["LlamaForCausalLM"], attention_bias=False)
    if spelling == "rope_scaling":          # transformers 4: the scaling beside a top-level rope_theta
        cfg.update(rope_theta=fam.LLAMA3_THETA, rope_scaling=hf)
    else:                                   # transformers 5: one dict that also carries rope_theta
        cfg.update(rope_parameters=dict(hf, rope_theta=fam.LLAMA3_THETA))
    m = build_report_decoder(_write(tmp_path, "llama3", cfg, src), dtype=torch.float32).eval()
    assert m.config.rope_theta == fam.LLAMA3_THETA and m.config.rope_scaling["rope_type"] == "llama3"
    assert torch.equal(m.model.rotary_emb.inv_freq, g["inv_freq"])
    out = m.generate(g["inputs_embeds"], attention_mask=g["attention_mask"], use_graph=False, **fam.BEAM, **fam.GEN)
    assert torch.equal(out, g["beam3"])


def test_build_reads_head_dim_and_qk_norm(tmp_path):
    g, src = _tiny("decode_tiny_qwen3")
    cfg = dict(QWEN3_CFG, model_type="qwen3", architectures=["Qwen3ForCausalLM"], attention_bias=False, use_sliding_window=False,
               sliding_window=None, rope_parameters=dict(rope_type="default", rope_theta=10000.0))
    m = build_report_decoder(_write(tmp_path, "qwen3", cfg, src), dtype=torch.float32).eval()
    assert m.config.head_dim == 64 and m.config.qk_norm is True and m.config.rope_scaling is None
    assert torch.equal(m.model.layers[1].self_attn.k_norm.weight, src.model.layers[1].self_attn.k_norm.weight)
    out = m.generate(g["inputs_embeds"], attention_mask=g["attention_mask"], use_graph=False, **fam.GREEDY, **fam.GEN)
    assert torch.equal(out, g["greedy"])
    # the same weights without the model_type: the norm weights have no home, and nothing loads anyway
    with pytest.raises(RuntimeError, match="unexpected.*q_norm"):
        build_report_decoder(_write(tmp_path, "as_qwen2", dict(cfg, model_type="qwen2"), src), dtype=torch.float32)


@pytest.mark.parametrize("change,key", [
    (dict(rope_scaling=dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=32)), "rope_scaling"),
    (dict(rope_parameters=dict(rope_type="linear", factor=2.0, rope_theta=10000.0)), "rope_parameters"),
    (dict(rope_scaling=dict(type="dynamic", factor=2.0)), "rope_scaling"),
    (dict(use_sliding_window=True, sliding_window=32), "use_sliding_window"),
    (dict(model_type="qwen3_moe"), "model_type"),
    (dict(model_type="qwen2_moe"), "model_type"),
    (dict(attention_bias=True), "attention_bias"),
], ids=["yarn", "linear", "dynamic", "sliding", "qwen3_moe", "qwen2_moe", "bias+qk_norm"])
def test_build_refuses_what_is_not_built_and_names_the_key(tmp_path, change, key):
    _, src = _tiny("decode_tiny_qwen3")
    cfg = dict(QWEN3_CFG, model_type="qwen3", attention_bias=False, use_sliding_window=False)
    cfg.update(change)
    with pytest.raises(NotImplementedError, match=key):
        build_report_decoder(_write(tmp_path, "bad", cfg, src), dtype=torch.float32)


def test_qwen2_style_config_builds_what_it_built_before(tmp_path):
    shape = dict(vocab_size=48, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                 rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=128)
    torch.manual_seed(0)
    src = ReportDecoder(**shape)
    cfg = dict(shape, model_type="qwen2", architectures=["Qwen2ForCausalLM"], use_sliding_window=False, sliding_window=4096,
               max_window_layers=2, rope_scaling=None, attention_dropout=0.0, hidden_act="silu", tie_word_embeddings=False)
    m = build_report_decoder(_write(tmp_path, "qwen2", cfg, src), dtype=torch.float32)
    assert list(m.state_dict()) == list(src.state_dict()) and not any("q_norm" in k for k in m.state_dict())
    for k in shape:
        assert getattr(m.config, k) == shape[k], k
    assert m.config.head_dim == 16 and m.config.qk_norm is False and m.config.rope_scaling is None
    assert torch.equal(m.model.rotary_emb.inv_freq, src.model.rotary_emb.inv_freq)
    assert torch.equal(m.lm_head.weight, src.lm_head.weight)
    # a config dict keeps going through _CFG_KEYS alone, and the built-in names are what they were
    from medical_image_analysis_amd import mambaxray_vl as mx
    assert set(mx.LLAMA2_7B) == set(mx.QWEN15_1P8B) == set(shape) and mx.LLAMA2_7B["hidden_size"] == 4096


# ---- descriptor and refusals (no GPU: every check below returns before a launch) ------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "mxvl.h")) as f:
        return f.read()


def _field_names(struct):
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    return [n.split()[-1].lstrip("*") for n in names]


def test_descriptor_mirrors_the_header():
    h = _header()
    assert re.search(r"#define\s+MXVL_QK_NORM\s+0x2000\b", h) and _abi.MXVL_QK_NORM == 0x2000
    others = _abi.MXVL_W_INT8 | _abi.MXVL_W_MXFP4 | _abi.MXVL_W_FP8 | _abi.MXVL_W_INT4 | _abi.MXVL_KV_FP8 | _abi.MXVL_BF16 | _abi.MXVL_F16
    assert _abi.MXVL_QK_NORM & others == 0
    Q = _abi.DecodeAttnQkNormDesc
    assert _field_names("mxvl_decode_attn_qknorm_desc") == [n for n, _ in Q._fields_] == ["attn", "q_norm_weight", "k_norm_weight", "qk_norm_eps"]
    assert Q._fields_[0][1] is _abi.DecodeAttnDesc and Q.attn.offset == 0, "the entry reads the descriptor through the same pointer"
    # the new fields trail the descriptor, which itself did not move
    assert ctypes.sizeof(_abi.DecodeAttnDesc) == 120 and _field_names("mxvl_decode_attn_desc")[-1] == "kv_scale"
    assert (Q.q_norm_weight.offset, Q.k_norm_weight.offset, Q.qk_norm_eps.offset, ctypes.sizeof(Q)) == (120, 128, 136, 144)
    assert _abi.ABI_VERSION == 13 and re.search(r"#define\s+MXVL_ABI_VERSION\s+13\b", h)
    assert len(set(re.findall(r"\b(mxvl_\w+)\s*\([^)]*\bvoid\s*\*\s*hip_stream\s*\)\s*;", h))) == 43


def _desc(dtype, head_dim=128, qw=0xb000, kw=0xc000, qkv=0x1000, kv_scale=0x9000):
    q = _abi.DecodeAttnQkNormDesc()
    a = q.attn
    a.rows, a.n_heads, a.n_kv_heads, a.head_dim, a.max_len, a.scale, a.beams = 2, 2, 2, head_dim, 32, head_dim ** -0.5, 0
    a.dtype = dtype
    # fake device pointers: the calls below return before anything is launched or read
    a.qkv, a.cos, a.sin, a.k_cache, a.v_cache = qkv, 0x2000, 0x3000, 0x4000, 0x5000
    a.slot_table, a.pos, a.mask, a.out = 0x6000, 0x7000, 0x8000, 0xa000
    a.kv_scale = kv_scale
    q.q_norm_weight, q.k_norm_weight, q.qk_norm_eps = qw, kw, 1e-6
    return q


def test_decode_attn_refusals_with_the_flag():
    lib = _abi.load()
    assert lib.mxvl_abi_version() == 13
    F, K = _abi.MXVL_QK_NORM, _abi.MXVL_KV_FP8
    call = lambda q: lib.mxvl_decode_attn(ctypes.byref(q), None)
    for base in (_abi.MXVL_BF16, _abi.MXVL_F16, 0, _abi.MXVL_BF16 | K):
        assert call(_desc(base | F, qw=None)) == -1, "the flag with a NULL q_norm_weight: MXVL_ERR_NULL"
        assert call(_desc(base | F, kw=None)) == -1, "the flag with a NULL k_norm_weight: MXVL_ERR_NULL"
    assert call(_desc(_abi.MXVL_BF16 | F | K, kv_scale=None)) == -1
    for w in (_abi.MXVL_W_INT8, _abi.MXVL_W_MXFP4, _abi.MXVL_W_FP8, _abi.MXVL_W_INT4):
        assert call(_desc(_abi.MXVL_BF16 | F | w)) == -2, "the flag beside a weight-format bit: MXVL_ERR_DTYPE"
        assert call(_desc(_abi.MXVL_F16 | F | K | w)) == -2
    for bad in (3, 7, 0x4000, 1 << 20):
        assert call(_desc(bad | F)) == -2 and call(_desc(bad)) == -2
    assert call(_desc(_abi.MXVL_BF16 | F, head_dim=96)) == -7
    assert call(_desc(_abi.MXVL_BF16 | F | K, head_dim=256)) == -7, "fp8 cache at head_dim 256 stays refused"
    assert call(_desc(_abi.MXVL_BF16 | F, qw=0xb008)) == -7 and call(_desc(_abi.MXVL_F16 | F, qkv=0x1002)) == -7, "16-byte accesses"
    a = _desc(_abi.MXVL_BF16 | F)
    a.attn.n_kv_heads = 0
    assert call(a) == -3


def test_other_decode_entries_refuse_the_flag():
    lib = _abi.load()
    F = _abi.MXVL_QK_NORM
    d = _abi.GemvDesc()
    d.rows, d.K, d.N = 2, 128, 64
    d.x, d.W, d.y, d.w_scale = 0x1000, 0x2000, 0x3000, 0x4000
    for base in (_abi.MXVL_BF16, _abi.MXVL_F16, _abi.MXVL_BF16 | _abi.MXVL_W_INT8, _abi.MXVL_F16 | _abi.MXVL_W_INT4):
        d.dtype = base | F
        assert lib.mxvl_decode_gemv(ctypes.byref(d), None) == -2
    n = _abi.RmsNormDesc()
    n.rows, n.K, n.eps = 2, 64, 1e-6
    n.x, n.weight, n.y = 0x1000, 0x2000, 0x3000
    c = _abi.DecodeCrossAttnDesc()
    c.rows, c.n_heads, c.n_kv_heads, c.head_dim, c.n_keys, c.kv_rows_div, c.scale = 2, 2, 2, 64, 4, 1, 0.125
    c.q_rope, c.k, c.v, c.text_state, c.gate_weight, c.gate_bias, c.out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    for base in (_abi.MXVL_BF16, _abi.MXVL_F16):
        n.dtype = c.dtype = base | F
        assert lib.mxvl_decode_rmsnorm(ctypes.byref(n), None) == -2
        assert lib.mxvl_decode_cross_attn(ctypes.byref(c), None) == -2
