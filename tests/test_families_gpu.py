"""Qwen3 / Llama-3 on the GPU: mxvl_decode_attn with MXVL_QK_NORM (csrc/decode.hip decode_qk_norm_kernel, the in-place pre-pass in
front of the attention kernels) called directly, generate() of the Qwen3-shaped golden on the kernel stepper (16-bit, E4M3 cache,
int8 weights), the llama3-RoPE golden through the torch-module stepper, and the training path of the q/k norm."""
import ctypes
import os
import sys

import pytest
import torch

from conftest import load_golden
from medical_image_analysis_amd import _abi
from medical_image_analysis_amd.hybrid_decoder_layer import Qwen2RMSNorm
from medical_image_analysis_amd.report_decoder import ReportDecoder, _KernelStepper

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_families as fam  # noqa: E402
from keyed_fill import keyed_fill_llama_  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}        # the bound of the decode RMSNorm kernel test (test_report_decoder.py)
GUARD = 512
EPS = 1e-6


# ---- kernel level: the in-place pre-pass form ------------------------------------------------------------------------------------------
def _call(dtype, qkv, st, kc, vc, H, Hkv, D, beams, fp8, gains=None):
    """One mxvl_decode_attn call; gains = (q_norm weight, k_norm weight) sets MXVL_QK_NORM.  Returns (out, q_rope)."""
    rows = qkv.shape[0]
    out = torch.zeros(rows, H * D, dtype=dtype, device=DEV)
    qr = torch.zeros(rows, H * D, dtype=dtype, device=DEV)
    q = _abi.DecodeAttnQkNormDesc()
    a = q.attn
    a.rows, a.n_heads, a.n_kv_heads, a.head_dim, a.max_len, a.scale, a.beams = rows, H, Hkv, D, st["T"], D ** -0.5, beams
    a.dtype = _abi.dtype_code(dtype) | (_abi.MXVL_KV_FP8 if fp8 else 0) | (_abi.MXVL_QK_NORM if gains else 0)
    a.qkv, a.cos, a.sin, a.k_cache, a.v_cache = qkv.data_ptr(), st["cos"].data_ptr(), st["sin"].data_ptr(), kc.data_ptr(), vc.data_ptr()
    a.slot_table, a.pos, a.mask = st["slot"].data_ptr(), st["pos"].data_ptr(), st["mask"].data_ptr()
    a.out, a.q_rope = out.data_ptr(), qr.data_ptr()
    a.kv_scale = st["kvs"].data_ptr() if fp8 else None
    if gains:
        q.q_norm_weight, q.k_norm_weight, q.qk_norm_eps = gains[0].data_ptr(), gains[1].data_ptr(), EPS
    # without the flag the library reads the first 120 bytes only: the plain descriptor
    _abi.check(_abi.load().mxvl_decode_attn(ctypes.byref(q if gains else a), _abi.stream_ptr(qkv.device)), "mxvl_decode_attn")
    torch.cuda.synchronize()
    return out, qr


def _guarded_rows(x):
    """x inside a larger buffer of a recognisable fill: (whole buffer, the view holding x)."""
    buf = torch.full((x.numel() + 2 * GUARD,), 7.0, dtype=x.dtype, device=DEV)
    view = buf[GUARD:GUARD + x.numel()].view(x.shape)
    view.copy_(x)
    return buf, view


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv_e4m3"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rows,beams", [(1, 0), (6, 0), (18, 3)])
def test_qk_norm_prepass_then_the_unflagged_kernels(rows, beams, D, dtype, fp8):
    """The form checked is the IN-PLACE PRE-PASS: (1) after the flagged call the v segment of qkv is bit-identical and the q / k
    segments are Qwen2RMSNorm over head_dim under the rule of test_decode_rmsnorm_kernel_matches_module_rounding (the same
    arithmetic: mismatches < 2e-3 of all elements, none beyond one 16-bit ulp of its row's maximum); (2) an unflagged call on a copy
    of those values into fresh caches gives bit-identical out, q_rope and caches.  Flag off, two calls agree bit for bit and qkv is
    not written."""
    H, Hkv, T, pos_v = 4, 2, 40, 21
    g = torch.Generator().manual_seed(rows * 1000 + D + int(fp8))
    W = (H + 2 * Hkv) * D
    qkv0 = (2.0 * torch.randn(rows, W, generator=g)).to(dtype).to(DEV)
    ang = torch.rand(rows, D // 2, generator=g) * 6.0
    st = dict(T=T, cos=torch.cat([ang.cos(), ang.cos()], -1).to(DEV), sin=torch.cat([ang.sin(), ang.sin()], -1).to(DEV),
              pos=torch.tensor([pos_v], device=DEV), kvs=torch.tensor([0.5, 0.25], dtype=torch.float32, device=DEV))
    nb = max(beams, 1)
    own = torch.arange(rows, dtype=torch.int32)[:, None].expand(-1, T).clone()
    own[:, :9] = (own[:, :9] // nb) * nb                          # the beams of a sample share their prompt lines, as in the stepper
    st["slot"] = own.to(DEV)
    mask = torch.ones(rows, T, dtype=torch.long)
    mask[rows // 2, :3] = 0                                       # left padding
    st["mask"] = mask.to(DEV)
    if fp8:
        mk = lambda: (torch.randn(rows, Hkv, T, D, generator=g) * 2).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    else:
        mk = lambda: torch.randn(rows, Hkv, T, D, generator=g).to(dtype).to(DEV)
    kc0, vc0 = mk(), mk()
    norms = [Qwen2RMSNorm(D, eps=EPS).to(DEV).to(dtype) for _ in range(2)]
    with torch.no_grad():
        for n in norms:
            n.weight.copy_((1.0 + 0.1 * torch.randn(D, generator=g)).to(dtype))
    gains = (norms[0].weight.detach(), norms[1].weight.detach())

    # flag off: the parent's behaviour, twice
    plain = []
    for _ in range(2):
        buf, qkv = _guarded_rows(qkv0)
        kc, vc = kc0.clone(), vc0.clone()
        plain.append(_call(dtype, qkv, st, kc, vc, H, Hkv, D, beams, fp8) + (kc, vc))
        assert torch.equal(qkv, qkv0), "an unflagged call does not write qkv"
    for u, v in zip(*plain):
        assert torch.equal(u, v)

    # (1) the flagged call rewrites q and k in place, and nothing else
    buf, qkv = _guarded_rows(qkv0)
    kc1, vc1 = kc0.clone(), vc0.clone()
    out1, qr1 = _call(dtype, qkv, st, kc1, vc1, H, Hkv, D, beams, fp8, gains=gains)
    assert bool((buf[:GUARD] == 7.0).all()) and bool((buf[-GUARD:] == 7.0).all()), "elements around qkv"
    assert torch.equal(qkv[:, (H + Hkv) * D:], qkv0[:, (H + Hkv) * D:]), "v is untouched"
    with torch.no_grad():
        ref = torch.cat([norms[0](qkv0[:, :H * D].view(rows, H, D)), norms[1](qkv0[:, H * D:(H + Hkv) * D].view(rows, Hkv, D))], dim=1)
    got = qkv[:, :(H + Hkv) * D].view(rows, H + Hkv, D)
    diff = (got.float() - ref.float()).abs()
    row_max = ref.float().abs().amax(-1, keepdim=True)
    print(f"qk-norm rows={rows} D={D} {dtype} fp8={fp8}: mismatching {float((diff > 0).float().mean()):.2e}, max diff / (ulp x row max) "
          f"{float((diff / (ULP[dtype] * row_max)).max()):.3f}")
    assert float((diff > 0).float().mean()) < 2e-3 and bool((diff <= ULP[dtype] * row_max).all())
    assert not torch.equal(out1, plain[0][0]), "the norm must matter for this input"

    # (2) the attention kernels behind the pre-pass are the unflagged ones
    kc2, vc2 = kc0.clone(), vc0.clone()
    out2, qr2 = _call(dtype, qkv.clone(), st, kc2, vc2, H, Hkv, D, beams, fp8)
    assert torch.equal(out1, out2) and torch.equal(qr1, qr2)
    assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2), "the appended cache line (and every other byte of the caches)"
    assert not torch.equal(kc1[:, :, pos_v], kc0[:, :, pos_v])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _qwen3_hd128(dtype, dev=DEV):
    g = load_golden("decode_qwen3_hd128")
    shape = {k[4:]: int(v) for k, v in g.items() if k.startswith("cfg_")}
    assert shape == fam.QWEN3_HD128
    m = ReportDecoder(rms_norm_eps=1e-6, max_position_embeddings=128, rope_theta=float(g["rope_theta"]), qk_norm=True, **shape)
    fam.keyed_qk_gains_(keyed_fill_llama_(m, int(g["weight_seed"])), int(g["weight_seed"]))
    chk = sum(v.double().abs().sum() for k, v in m.state_dict().items() if not k.endswith("_proj.bias")).float()
    assert abs(float(chk) - float(g["weight_checksum"])) <= 1e-6 * float(chk), "keyed weights differ from the generator's"
    return g, m.to(dev).to(dtype).eval()


def _kernel_stepper(m, rows):
    key = [k for k in m._steppers if k[0] == rows][-1]
    return m._steppers[key]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_qwen3_hd128_generate_tokens_match_hf(dtype):
    """head_dim 128 with hidden / heads = 64, QK-norm: greedy and beam-3 streams of the HIP kernel stepper equal HF Qwen3ForCausalLM's."""
    g, m = _qwen3_hd128(dtype)
    emb, att = g["inputs_embeds"].to(DEV).to(dtype), g["attention_mask"].to(DEV)
    for name, kw in (("greedy", fam.GREEDY), ("beam3", fam.BEAM)):
        out = m.generate(emb, attention_mask=att, use_graph=True, **kw, **fam.GEN)
        st = _kernel_stepper(m, emb.shape[0] * kw["num_beams"])
        assert type(st) is _KernelStepper and st.qk_norm and st.D == 128, "generate() must have taken the HIP kernels"
        assert torch.equal(out.cpu(), g[name]), f"{name}: {out.cpu().tolist()} vs HF {g[name].tolist()}"


def _against_the_torch_stepper(prepare, extra, is_mode, prompt_seed=None):
    """What the existing twins assert (test_fp8_kernel_stepper_end_to_end, test_quantised_kernel_stepper_end_to_end): generate() on the
    kernel stepper against use_graph="torch" on the same device, bf16, token for token -- the two round differently, so a case
    counts only if its torch-path decode is not on a near-tie: the eager CPU path gives the same tokens in bf16 and fp32 (asserted,
    never skipped).
    prompt_seed: a prompt of the golden generator's distribution (make_golden_families._prompt), the first that meets the generator's
    robustness rule on the CPU path of THIS configuration (fp8 cache / int8 weights), nothing of it taken from a GPU run: the top-2
    margin of every greedy decision -- of the scores after the repetition penalty and the min-length mask, which is what argmax sees
    -- exceeds 0.012 x the logit scale (bf16 moves a logit by ~0.4 % of it), greedy and beam-3 streams are the same in bf16 and
    fp32, and under 4 draws of N(0, 0.0024 x scale) noise on every step's logits.  (With the margin taken on the RAW logits, as
    the generator does for HF, prompt 128 passes for the fp8 cache although decision 9 of its row 0 has a margin of 0.5 % of the
    scale after the penalty: the two steppers split exactly there, the torch-module one agreeing with the CPU.)"""
    dtype = torch.bfloat16
    g, _ = _qwen3_hd128(dtype, "cpu")
    emb, att = g["inputs_embeds"], g["attention_mask"]
    if prompt_seed is not None:
        emb, att = fam._prompt(prompt_seed, fam.QWEN3_HD128["hidden_size"])
    emb = emb.to(dtype)
    make = lambda: prepare(_qwen3_hd128(dtype, "cpu")[1])
    model = make().to(DEV)
    for kw in (fam.GREEDY, fam.BEAM):
        kw = dict(kw, attention_mask=att, **fam.GEN, **extra)
        cpu16 = make().generate(emb, use_graph=False, **kw)
        cpu32 = make().float().generate(emb.float(), use_graph=False, **kw)
        assert torch.equal(cpu16, cpu32), "the torch-path decode of this case sits on a near-tie; pick another prompt"
        kw["attention_mask"] = att.to(DEV)
        rows = emb.shape[0] * kw["num_beams"]
        assert _KernelStepper.supported(model, rows, dtype, DEV, extra.get("kv_cache_dtype"))
        ref = model.generate(emb.to(DEV), use_graph="torch", **kw)
        model.__dict__.pop("_steppers", None)               # (the torch-module stepper of the call above)
        got = model.generate(emb.to(DEV), use_graph=True, **kw)
        st = list(model._steppers.values())
        assert len(st) == 1 and type(st[0]) is _KernelStepper and st[0].qk_norm and st[0].D == 128 and is_mode(st[0])
        assert torch.equal(got.cpu(), ref.cpu()), (got.tolist(), ref.tolist())
        model.__dict__.pop("_steppers", None)


def test_qwen3_hd128_fp8_cache_end_to_end():
    """kv_cache_dtype="fp8" with QK-norm (the normalised, rotated key is what gets encoded), greedy and beam 3.  An E4M3 code that
    flips moves a cached element by 6 %, so the stored prompt -- robust for the 16-bit cache -- is not for this one: see
    _against_the_torch_stepper for how prompt 430 was chosen."""
    _against_the_torch_stepper(lambda m: m, dict(kv_cache_dtype="fp8"), lambda st: st.kv8 and st.kc[0].dtype == torch.uint8, prompt_seed=430)


def test_qwen3_hd128_int8_weights_end_to_end():
    """low_resource="int8" with QK-norm: o_proj's K is H * head_dim = 1024, not hidden; greedy and beam 3 (prompt 232: the int8
    model is another model than the one the stored prompt was chosen for)."""
    _against_the_torch_stepper(lambda m: m.quantize_("int8"), {}, lambda st: st.int8 and not st.fused_norm, prompt_seed=232)


def test_tiny_llama3_through_the_torch_stepper():
    """The llama3-scaled rotary table on the GPU: the captured torch-module stepper reproduces HF's streams (fp32, head_dim 16)."""
    g = load_golden("decode_tiny_llama3")
    m = ReportDecoder(rms_norm_eps=1e-6, max_position_embeddings=128, rope_theta=fam.LLAMA3_THETA, rope_scaling=fam.LLAMA3_ROPE, **fam.TINY_LLAMA3)
    m.load_hf_state_dict({k[2:]: v.view(torch.bfloat16).float() for k, v in g.items() if k.startswith("p_")})
    m = m.to(DEV).eval()
    assert torch.equal(m.model.rotary_emb.inv_freq.cpu(), g["inv_freq"])
    emb, att = g["inputs_embeds"].to(DEV), g["attention_mask"].to(DEV)
    for name, kw in (("greedy", fam.GREEDY), ("beam3", fam.BEAM)):
        out = m.generate(emb, attention_mask=att, use_graph="torch", **kw, **fam.GEN)
        assert torch.equal(out.cpu(), g[name]), f"{name}: {out.cpu().tolist()} vs HF {g[name].tolist()}"


def test_qwen3_hd128_training_path_gradient():
    """forward_frozen_autocast (fp16 weights frozen, bf16 autocast: q_norm / k_norm through rms_norm_frozen, forward and backward) at
    B 2, T 16: the gradient that reaches inputs_embeds against the module path in fp32 (the same weights in fp32, no autocast, the
    kernels of llm_ops.hip switched off), under the gradient bound of test_rms_norm_frozen_matches_the_module_expression:
    max |ga - gb| <= (4 ulp + 1e-6) x max |gb|, ulp that of the dtype the activations carry (bf16)."""
    from medical_image_analysis_amd import fused_ops
    _, m = _qwen3_hd128(torch.float16)
    _, m32 = _qwen3_hd128(torch.float32)
    for p in list(m.parameters()) + list(m32.parameters()):
        p.requires_grad_(False)
    gen = torch.Generator().manual_seed(16)
    emb = (0.5 * torch.randn(2, 16, fam.QWEN3_HD128["hidden_size"], generator=gen)).to(DEV)
    att = torch.ones(2, 16, dtype=torch.long, device=DEV)
    att[1, :3] = 0
    tgt = torch.randint(0, fam.QWEN3_HD128["vocab_size"], (2, 16), generator=gen).to(DEV)

    def grad(fn):
        e = emb.clone().requires_grad_(True)
        logits = fn(e)
        torch.nn.functional.cross_entropy(logits.float().view(-1, logits.shape[-1]), tgt.view(-1)).backward()
        return e.grad.float()

    def fused(e):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return m.forward_frozen_autocast(e, attention_mask=att)
    ga = grad(fused)
    fused_ops.LLM_OPS = False
    try:
        gb = grad(lambda e: m32(e, attention_mask=att))
    finally:
        fused_ops.LLM_OPS = True
    scale = float(gb.abs().max())
    err = float((ga - gb).abs().max())
    print(f"training path: max |ga - gb| / max |gb| = {err / scale:.4e} (bound {4 * 2.0 ** -8 + 1e-6:.4e})")
    assert bool(torch.isfinite(ga).all()) and scale > 0
    assert err <= (4 * 2.0 ** -8 + 1e-6) * scale, err / scale
