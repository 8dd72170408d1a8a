"""-m gpu: the MFMA flash-attention kernels (csrc/attn.hip, through the C-ABI) against a plain fp32 masked-softmax
reference of the same operation -- forward and all three gradients, every mask mode, ragged lengths, GQA, strided
(B, L, H, D) views, head_dim 32 / 64 / 128, fp32 (exact fp32 MFMA; tolerance 1e-4 as north_star states for attention) and
bf16 / fp16 (the reference is fed the same rounded inputs; tolerance = 16-bit rounding of P and dS)."""
import math

import pytest
import torch

from conftest import assert_close

gpu = pytest.mark.gpu      # every test below but the CPU pin of the reference (test_reference_equals_sdpa_fp64_on_every_masked_geometry)
DEV = "cuda:0"


def permitted(B, Lq, Lk, mask="none", cluster=16, key_mask=None, bias=None, device="cpu"):
    """(B, 1, Lq, Lk) bool: the keys a query may attend -- the mask mode AND key_mask AND bias > -inf (the same for every head)."""
    i = torch.arange(Lq, device=device)[:, None]
    j = torch.arange(Lk, device=device)[None, :]
    allow = torch.ones(Lq, Lk, dtype=torch.bool, device=device)
    if mask == "causal":
        allow = j <= i + (Lk - Lq)
    elif mask == "block_causal":
        allow = (j // cluster) <= (i // cluster)
    if bias is not None:
        allow = allow & (bias > float("-inf"))
    allow = allow[None, None].expand(B, 1, Lq, Lk)
    if key_mask is not None:
        allow = allow & key_mask.bool()[:, None, None, :]
    return allow


def ref_attention(q, k, v, scale, mask="none", cluster=16, key_mask=None, bias=None, keep=None, keep_scale=1.0):
    """fp64 masked softmax (B, H, Lq, D); keep (B, H, Lq, Lk) bool: nn.Dropout's mask on the probabilities, kept ones times keep_scale.
    A query row with no permitted key has zero probabilities (so a zero output and zero gradients): the kernels' contract for such
    rows (lse = +inf, out = 0) and what F.scaled_dot_product_attention computes on the host."""
    q, k, v = q.double(), k.double(), v.double()
    B, H, Lq, D = q.shape
    Hkv, Lk = k.shape[1], k.shape[2]
    if Hkv != H:
        k = k.repeat_interleave(H // Hkv, dim=1)
        v = v.repeat_interleave(H // Hkv, dim=1)
    s = q @ k.transpose(-1, -2) * scale
    i = torch.arange(Lq, device=q.device)[:, None]
    j = torch.arange(Lk, device=q.device)[None, :]
    allow = torch.ones(Lq, Lk, dtype=torch.bool, device=q.device)
    if mask == "causal":
        allow = j <= i + (Lk - Lq)
    elif mask == "block_causal":
        allow = (j // cluster) <= (i // cluster)
    s = s.masked_fill(~allow, float("-inf"))
    if bias is not None:
        s = s + bias.double()
    if key_mask is not None:
        s = s.masked_fill(~key_mask.bool()[:, None, None, :], float("-inf"))
    some = permitted(B, Lq, Lk, mask, cluster, key_mask, bias, q.device).any(-1, keepdim=True)
    # (the all -inf scores of a row without keys are replaced before the softmax as well: its NaN would come back through autograd as 0 * NaN)
    pr = torch.where(some, torch.softmax(torch.where(some, s, torch.zeros_like(s)), dim=-1), torch.zeros_like(s))
    if keep is not None:
        pr = torch.where(keep, pr * keep_scale, torch.zeros_like(pr))
    return pr @ v


def _mk(B, H, Hkv, Lq, Lk, D, dtype, seed, layout="bhld"):
    g = torch.Generator().manual_seed(seed)
    def one(h, L):
        if layout == "blhd":   # the layout a Linear(...).reshape(B, L, H, D).transpose(1, 2) produces
            return torch.randn(B, L, h, D, generator=g).to(DEV, dtype).transpose(1, 2)
        return torch.randn(B, h, L, D, generator=g).to(DEV, dtype)
    return one(H, Lq), one(Hkv, Lk), one(Hkv, Lk)


CASES = [
    # B, H, Hkv, Lq,  Lk,  D,  mask,           layout
    (2, 2, 2, 128, 128, 64, "none", "bhld"),
    (1, 3, 3, 197, 197, 64, "none", "blhd"),            # ViT tokens, ragged tiles
    (2, 4, 4, 401, 401, 32, "none", "blhd"),            # MAE decoder: head_dim 32
    (1, 2, 2, 300, 300, 64, "causal", "bhld"),
    (2, 4, 2, 77, 205, 64, "causal", "blhd"),           # GQA, Lk > Lq (decode-style offset)
    (1, 2, 2, 48, 48, 64, "block_causal", "bhld"),      # the golden's geometry (3 clusters)
    (2, 8, 8, 528, 528, 64, "block_causal", "blhd"),    # several diagonal tiles
    (1, 2, 1, 33, 5, 64, "none", "bhld"),               # fewer keys than one tile
    # several 256-query workgroup tiles, > 3 key tiles (the LDS-DMA ring of the 64-queries-per-wave kernels wraps), ragged ends
    (1, 2, 2, 700, 700, 64, "none", "blhd"),
    (2, 4, 2, 515, 900, 64, "causal", "blhd"),          # GQA, Lk > Lq, diagonal crosses workgroup tiles
    (1, 3, 3, 1040, 1040, 64, "block_causal", "bhld"),
    # head_dim 128 (Llama-2-7B / Qwen heads: the hybrid decoder's training-time attention), forward AND backward
    (2, 4, 2, 230, 230, 128, "causal", "blhd"),         # decoder self-attention: GQA, prompt-length rows
    (1, 4, 4, 41, 197, 128, "none", "blhd"),            # text queries x 197 image keys
    (1, 2, 2, 160, 160, 128, "block_causal", "bhld"),
    # head dims between the instantiated ones run zero-padded on the next larger kernel (tiny test models: 16, 48)
    (2, 4, 4, 9, 9, 16, "causal", "blhd"),
    (1, 3, 3, 70, 70, 48, "none", "bhld"),
]


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", CASES)
def test_attention_fwd_bwd(case, dtype):
    from medical_image_analysis_amd.flash_attention import attention
    B, H, Hkv, Lq, Lk, D, mask, layout = case
    q, k, v = _mk(B, H, Hkv, Lq, Lk, D, dtype, seed=Lq + D)
    if layout == "blhd":
        q, k, v = _mk(B, H, Hkv, Lq, Lk, D, dtype, seed=Lq + D, layout="blhd")
    scale = D ** -0.5
    qs, ks, vs = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    if layout == "blhd":   # keep the strided view as the leaf's view
        leaves = [t.transpose(1, 2).contiguous().requires_grad_(True) for t in (q, k, v)]
        qs, ks, vs = [t.transpose(1, 2) for t in leaves]
    out = attention(qs, ks, vs, scale=scale, mask=mask, cluster=16)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(DEV, dtype)
    out.backward(dout)
    qr, kr, vr = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    ref = ref_attention(qr, kr, vr, scale, mask, 16)
    ref.backward(dout.double())
    if dtype == torch.float32:
        tol_o, tol_g = (1e-4, 1e-4), (2e-4, 1e-3)
    else:
        tol_o, tol_g = (2e-2, 2e-2), (6e-2, 5e-2)
    assert_close(out, ref, *tol_o, f"out {case} {dtype}")
    got = [t.grad for t in (leaves if layout == "blhd" else (qs, ks, vs))]
    want = [qr.grad, kr.grad, vr.grad]
    if layout == "blhd":
        want = [w.transpose(1, 2) for w in want]
    for name, g_, w_ in zip(("dq", "dk", "dv"), got, want):
        sc = max(1.0, float(w_.abs().max()))
        assert_close(g_, w_, tol_g[0] * sc, tol_g[1], f"{name} {case} {dtype}")


@gpu
def test_attention_key_mask_bias_and_head_dim_128():
    from medical_image_analysis_amd.flash_attention import attention
    g = torch.Generator().manual_seed(3)
    B, H, Hkv, Lq, Lk, D = 2, 4, 2, 9, 197, 128          # text queries x image keys, Llama head_dim
    q = torch.randn(B, H, Lq, D, generator=g).to(DEV)
    k = torch.randn(B, Hkv, Lk, D, generator=g).to(DEV)
    v = torch.randn(B, Hkv, Lk, D, generator=g).to(DEV)
    km = torch.ones(B, Lk, dtype=torch.bool)
    km[1, 150:] = False
    km[0, ::7] = False
    km = km.to(DEV)
    out = attention(q, k, v, key_mask=km)
    assert_close(out, ref_attention(q, k, v, D ** -0.5, key_mask=km), 1e-4, 1e-4, "key-masked cross attention, D = 128")
    out16 = attention(q.bfloat16(), k.bfloat16(), v.bfloat16(), key_mask=km)
    assert_close(out16, ref_attention(q.bfloat16(), k.bfloat16(), v.bfloat16(), D ** -0.5, key_mask=km), 2e-2, 2e-2, "bf16 D = 128")
    # additive bias (arbitrary mask tensor), fwd + bwd, D = 64
    q, k, v = _mk(1, 2, 2, 70, 90, 64, torch.float32, seed=8)
    bias = torch.randn(70, 90, generator=g).to(DEV)
    bias[:, 80:] = float("-inf")
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = attention(*leaves, bias=bias)
    refl = [t.double().requires_grad_(True) for t in (q, k, v)]
    ref = ref_attention(*refl, 64 ** -0.5, bias=bias)
    assert_close(out, ref, 1e-4, 1e-4, "bias fwd")
    dout = torch.randn_like(out)
    out.backward(dout)
    ref.backward(dout.double())
    for a, b, n in zip(leaves, refl, "qkv"):
        assert_close(a.grad, b.grad, 2e-4 * max(1.0, float(b.grad.abs().max())), 1e-3, "bias d" + n)


@gpu
def test_attention_block_causal_equals_mask_generate_semantics_at_full_size():
    """The pre-training decoder's geometry (4080 tokens, 8 heads x 64, 16-token clusters), bf16: forward against the fp64
    reference on one batch element, and the property that a query never depends on keys beyond its own cluster."""
    from medical_image_analysis_amd.flash_attention import attention, attention_kvpacked
    B, H, L, D = 2, 8, 4080, 64
    g = torch.Generator().manual_seed(1)
    qh = torch.randn(B, L, H, D, generator=g).to(DEV, torch.bfloat16)
    kv = torch.randn(B, L, 2, H, D, generator=g).to(DEV, torch.bfloat16)
    q = qh.transpose(1, 2)
    out = attention_kvpacked(q, kv, mask="block_causal", cluster=16)
    k, v = kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2)
    ref = ref_attention(q[:1], k[:1], v[:1], D ** -0.5, "block_causal", 16)
    assert_close(out[:1], ref, 2e-2, 2e-2, "block-causal 4080 tokens")
    kv2 = kv.clone()
    kv2[:, 2048:] = torch.randn(B, L - 2048, 2, H, D, generator=g).to(DEV, torch.bfloat16)   # change keys of clusters >= 128
    out2 = attention_kvpacked(q, kv2, mask="block_causal", cluster=16)
    assert torch.equal(out2[:, :, :2048], out[:, :, :2048]), "queries of clusters < 128 never read later keys"
    assert not torch.equal(out2[:, :, 2048:], out[:, :, 2048:])
    # packed-kv gradient layout
    ql = qh.clone().requires_grad_(True)
    kvl = kv.clone().requires_grad_(True)
    o = attention_kvpacked(ql.transpose(1, 2), kvl, mask="block_causal", cluster=16)
    do = torch.randn(o.shape, generator=g).to(DEV, torch.bfloat16)
    o.backward(do)
    qr, kr, vr = [t[:1].detach().double().requires_grad_(True) for t in (q, k, v)]
    r = ref_attention(qr, kr, vr, D ** -0.5, "block_causal", 16)
    r.backward(do[:1].double())
    for name, got, want in (("dq", ql.grad[:1].transpose(1, 2), qr.grad), ("dk", kvl.grad[:1, :, 0].transpose(1, 2), kr.grad),
                            ("dv", kvl.grad[:1, :, 1].transpose(1, 2), vr.grad)):
        sc = max(1.0, float(want.abs().max()))
        assert_close(got, want, 6e-2 * sc, 5e-2, name + " 4080 tokens")


DROP_CASES = [
    # B, H, Hkv, Lq,  Lk,  D,  mask,          key mask, p
    (2, 4, 4, 150, 150, 64, "none", False, 0.1),            # head_dim 64 leaves the 64-queries-per-wave kernels for the general ones
    (1, 4, 2, 77, 205, 64, "causal", True, 0.25),           # GQA + causal offset + a key mask
    (2, 3, 3, 401, 401, 32, "none", False, 0.1),            # MAE decoder geometry
    (1, 4, 2, 130, 197, 128, "none", True, 0.5),            # head_dim 128, text x image keys
    (1, 2, 2, 96, 96, 64, "block_causal", False, 0.1),
]


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", DROP_CASES)
def test_attention_dropout_forward_backward_against_the_host_mask(case, dtype):
    """Attention dropout inside the kernels (mxvl_attn_desc.dropout_p / dropout_seed): with the keep mask rebuilt on the host from the
    same (seed, head, query, key) hash, the forward and all three gradients equal nn.Dropout-on-the-probabilities in fp64; the kept
    fraction is 1 - p; the three kernels (forward, dQ, dK / dV) meet every element with the same bit."""
    from medical_image_analysis_amd import flash_attention as flash
    B, H, Hkv, Lq, Lk, D, mask, use_km, p = case
    q, k, v = _mk(B, H, Hkv, Lq, Lk, D, dtype, 17)
    q.requires_grad_(True); k.requires_grad_(True); v.requires_grad_(True)
    km = None
    if use_km:
        km = torch.rand(B, Lk, generator=torch.Generator().manual_seed(3)) > 0.2
        km[:, 0] = True
        km = km.to(DEV)
    seed = 123456789 + Lq
    scale = D ** -0.5
    out = flash.attention(q, k, v, scale=scale, mask=mask, key_mask=km, _drop=(p, seed))
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(DEV, dtype)
    out.backward(g)
    keep = flash.dropout_keep_mask(seed, B, H, Lq, Lk, p, device=DEV)
    assert abs(float(keep.float().mean()) - (1.0 - p)) < 0.02
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ref = ref_attention(qr, kr, vr, scale, mask, 16, km, None, keep=keep, keep_scale=1.0 / (1.0 - p))
    ref.backward(g.double())
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    sc = lambda t: max(1.0, float(t.detach().abs().max()))
    assert_close(out.float(), ref.float(), tol * sc(ref), tol, "out")
    for name, a, b in (("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad), ("dv", v.grad, vr.grad)):
        assert_close(a.float(), b.float(), tol * sc(b), tol, name)
    # the same seed repeats the draw bit for bit; p = 0 is the undropped kernel
    out2 = flash.attention(q.detach(), k.detach(), v.detach(), scale=scale, mask=mask, key_mask=km, _drop=(p, seed))
    assert torch.equal(out2, out.detach())
    plain = flash.attention(q.detach(), k.detach(), v.detach(), scale=scale, mask=mask, key_mask=km)
    assert not torch.equal(plain, out2)


@gpu
def test_gpu_attention_has_no_library_fallback():
    """Every attention call site dispatches through flash.require: HIP tensors take the MFMA kernels or RAISE (head_dim without a
    kernel, query-dependent masks); only CPU tensors evaluate the torch reference expression.  Attention dropout is drawn inside the
    kernels: a training-mode module with attn_drop > 0 runs on them too."""
    import torch.nn.functional as F
    from medical_image_analysis_amd import flash_attention as flash
    from medical_image_analysis_amd.hybrid_decoder_layer import ScaleDotProductCrossAttention
    from medical_image_analysis_amd.mae import Attention
    q = torch.randn(1, 2, 8, 160, device=DEV)
    with pytest.raises(RuntimeError, match="head_dim 160"):
        flash.require(q, "test")
    with pytest.raises(RuntimeError, match="head_dim 256"):       # 256 is forward-only, 16-bit
        flash.require(torch.randn(1, 2, 8, 256, device=DEV, dtype=torch.bfloat16, requires_grad=True), "test")
    assert flash.require(torch.randn(1, 2, 8, 256, device=DEV, dtype=torch.bfloat16), "test") is True
    assert flash.require(torch.randn(1, 2, 8, 64, device=DEV), "test", 0.1) is True
    assert flash.require(torch.randn(1, 2, 8, 128, device=DEV, requires_grad=True), "test") is True
    assert flash.require(torch.randn(1, 2, 8, 64), "test") is False           # CPU: host-side reference path
    m = Attention(128, num_heads=2, qkv_bias=True, attn_drop=0.1).to(DEV).train()
    ca = ScaleDotProductCrossAttention(0)
    qq, kk = torch.randn(1, 2, 4, 64, device=DEV), torch.randn(1, 2, 6, 64, device=DEV)
    with pytest.raises(RuntimeError, match="query-dependent"):
        ca(qq, kk, kk, attn_mask=torch.ones(1, 4, 6, dtype=torch.bool, device=DEV))
    calls = []
    orig = F.scaled_dot_product_attention
    try:
        F.scaled_dot_product_attention = lambda *a, **k: calls.append(1) or orig(*a, **k)
        xin = torch.randn(2, 9, 128, device=DEV)
        torch.manual_seed(5)
        y1 = m(xin)
        torch.manual_seed(5)
        y2 = m(xin)
        assert torch.equal(y1, y2) and not torch.equal(y1, m(xin))            # dropout: repeatable under the seed, a fresh draw otherwise
        assert not torch.equal(y1, m.eval()(xin))
        ca(qq, kk, kk, key_mask=torch.ones(1, 6, dtype=torch.bool, device=DEV))
    finally:
        F.scaled_dot_product_attention = orig
    assert not calls, "a HIP tensor reached F.scaled_dot_product_attention"


@gpu
def test_block_causal_mask_verdict_is_cached_on_the_tensor_not_on_its_address():
    from medical_image_analysis_amd.flash_attention import is_block_causal_mask
    L = 64
    i = torch.arange(L, device=DEV) // 16
    good = torch.where(i[None, :] <= i[:, None], 0.0, float("-inf"))
    assert is_block_causal_mask(good, 16) and is_block_causal_mask(good, 16)
    ptr = good.data_ptr()
    del good
    bad = torch.zeros(L, L, device=DEV)                    # very likely the recycled allocation
    assert not is_block_causal_mask(bad, 16), f"stale verdict (same address: {bad.data_ptr() == ptr})"
    bad.copy_(torch.where(i[None, :] <= i[:, None], 0.0, float("-inf")))      # in-place update bumps the version counter
    assert is_block_causal_mask(bad, 16)


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_attention_kv_packed_strided_views_head_dim_64(dtype):
    """k / v as the strided halves of ONE (B, L, 2, H, D) projection output (models_pretrain's CrossAttention `kv` Linear): the
    LDS-DMA kernels address rows through the token stride 2*H*D, not H*D."""
    from medical_image_analysis_amd.flash_attention import attention
    B, H, L, D = 2, 4, 333, 64
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, L, H, D, generator=g).to(DEV, dtype).transpose(1, 2).requires_grad_(True)
    kv = torch.randn(B, L, 2, H, D, generator=g).to(DEV, dtype).requires_grad_(True)
    k, v = kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2)
    out = attention(q, k, v, scale=D ** -0.5, mask="block_causal", cluster=16)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(DEV, dtype)
    out.backward(dout)
    qr = q.detach().double().requires_grad_(True)
    kvr = kv.detach().double().requires_grad_(True)
    ref = ref_attention(qr, kvr[:, :, 0].transpose(1, 2), kvr[:, :, 1].transpose(1, 2), D ** -0.5, "block_causal", 16)
    ref.backward(dout.double())
    assert_close(out, ref, 2e-2, 2e-2, "out kv-packed")
    assert_close(q.grad, qr.grad, 6e-2 * max(1.0, float(qr.grad.abs().max())), 5e-2, "dq kv-packed")
    assert_close(kv.grad, kvr.grad, 6e-2 * max(1.0, float(kvr.grad.abs().max())), 5e-2, "dkv kv-packed")


# ---- the masked paths: rows that may attend no key, key mask and bias in every dtype ------------------------------------------
# What stage-2 / stage-3 training calls (hybrid_decoder_layer.py: causal + the padding mask as key_mask, image cross-attention
# with a per-key mask; qformer.py: key mask + dropout; models_pretrain.py: an additive bias).  The kernels' contract for a query
# row without a permitted key: lse = +inf, out = 0, and every backward pass multiplies by exp2(s - inf) = 0.
# Workgroups own 128 query rows (256 in the 64-queries-per-wave kernels), stage 64 keys per tile, and a dK / dV workgroup owns
# 128 keys: every shape is the smallest that puts a whole tile on the wrong side of its mask.
# Tolerances: the ones of test_attention_fwd_bwd (the header of this file), nothing wider.


def _case(B, H, Hkv, Lq, Lk, D, mask, km=None, bias=False):
    return (B, H, Hkv, Lq, Lk, D, mask, km, bias)


# left-padded prompts under the causal mask: pad = 140 leaves the first query workgroup without a key, two wholly masked key
# tiles before a partly masked one, and a dK / dV workgroup all of whose keys are masked; 77 x 205 is the decode-style offset
# (query i sees keys <= i + 128), where pad = 130 leaves rows 0 and 1 without a key
LEFTPAD = [_case(3, 4, 2, 200, 200, D, "causal", ("leftpad", (0, 5, 140))) for D in (32, 64, 128)]
LEFTPAD_OFFSET = [_case(3, 4, 2, 77, 205, D, "causal", ("leftpad", (0, 5, 130))) for D in (32, 64, 128)]
# image cross-attention: sample 0 sees every key, sample 1 has no image, sample 2 only keys 190..196 (the running maximum stays
# -inf across three key tiles)
CROSS = [_case(3, 4, 2, 41, 197, D, "none", ("noimage", None)) for D in (64, 128)]
# causal, Lq > Lk, no mask tensor: rows 0..259 have no key; 16-bit head_dim 64 runs the 64-queries-per-wave kernels and the
# LDS-DMA dK / dV kernel with a whole 256-row workgroup empty
LONGQ = [_case(1, 2, 2, 300, 40, D, "causal") for D in (64, 128)]
ROWS_WITHOUT_KEYS = LEFTPAD + LEFTPAD_OFFSET + CROSS + LONGQ
# additive bias: two query workgroups, four key tiles (the last ragged); alone, with a key mask, under the causal mask
BIAS = [_case(2, 4, 2, 150, 200, D, mask, km, True) for D in (32, 64, 128)
        for mask, km in (("none", None), ("none", ("mixed", None)), ("causal", None))]
HEAD_DIM_256 = [_case(2, 2, 1, 150, 150, 256, "causal", ("leftpad", (0, 70)))]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _geometry(case, device):
    """(key_mask (B, Lk) bool or None, bias (Lq, Lk) fp32 or None) of a case, drawn on the host."""
    B, H, Hkv, Lq, Lk, D, mask, km, has_bias = case
    key_mask = bias = None
    if km is not None:
        kind, arg = km
        key_mask = torch.ones(B, Lk, dtype=torch.bool)
        if kind == "leftpad":
            for b, pad in enumerate(arg):
                key_mask[b, :pad] = False
        elif kind == "noimage":
            key_mask[1] = False
            key_mask[2] = False
            key_mask[2, 190:197] = True
        else:   # "mixed": scattered holes in sample 0, a left pad longer than one key tile in sample 1
            key_mask[0] = torch.rand(Lk, generator=torch.Generator().manual_seed(21)) > 0.2
            key_mask[1, :70] = False
        key_mask = key_mask.to(device)
    if has_bias:
        g = torch.Generator().manual_seed(31)
        bias = torch.randn(Lq, Lk, generator=g)
        holes = torch.rand(Lq, Lk, generator=g) < 0.2
        bias[holes] = float("-inf")
        bias[:, 180:] = float("-inf")
        bias[10:20] = float("-inf")          # rows without keys
        bias = bias.to(device)
    return key_mask, bias


def _inputs(case, dtype, device):
    """q, k, v, dout as (B, H, L, D) views of (B, L, H, D) tensors, the layout the projections produce."""
    B, H, Hkv, Lq, Lk, D = case[:6]
    g = torch.Generator().manual_seed(1000 + Lq + D)
    one = lambda h, L: torch.randn(B, L, h, D, generator=g).to(device, dtype).transpose(1, 2)
    return one(H, Lq), one(Hkv, Lk), one(Hkv, Lk), one(H, Lq)


def _kernel(case, q, k, v, dout, key_mask, bias, drop=None, backward=True):
    from medical_image_analysis_amd.flash_attention import attention
    D, mask = case[5], case[6]
    if not backward:
        return (attention(q, k, v, scale=D ** -0.5, mask=mask, key_mask=key_mask, bias=bias),)
    ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = attention(ql, kl, vl, scale=D ** -0.5, mask=mask, key_mask=key_mask, bias=bias, _drop=drop)
    out.backward(dout)
    return out.detach(), ql.grad, kl.grad, vl.grad


def _reference(case, q, k, v, dout, key_mask, bias, keep=None, keep_scale=1.0):
    D, mask = case[5], case[6]
    qr, kr, vr = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    ref = ref_attention(qr, kr, vr, D ** -0.5, mask, 16, key_mask, bias, keep, keep_scale)
    ref.backward(dout.double())
    return ref.detach(), qr.grad, kr.grad, vr.grad


_BASE = {}


def _baseline(case, dtype):
    """Kernel results, fp64 reference and the permitted set of one (case, dtype): computed once, shared, never written to."""
    if (case, dtype) not in _BASE:
        B, H, Hkv, Lq, Lk = case[:5]
        key_mask, bias = _geometry(case, DEV)
        x = _inputs(case, dtype, DEV)
        allow = permitted(B, Lq, Lk, case[6], 16, key_mask, bias, DEV)
        _BASE[case, dtype] = (x, key_mask, bias, allow, _kernel(case, *x, key_mask, bias), _reference(case, *x, key_mask, bias))
    return _BASE[case, dtype]


def _ratio(got, ref, atol, rtol):
    return float(((got.double() - ref).abs() / (atol + rtol * ref.abs())).max())


def _check(case, dtype, allow, got, ref, what):
    """Finite; exactly zero where no key / no query is permitted; the fp64 reference at this file's tolerances."""
    B, H, Hkv, Lq, Lk = case[:5]
    if dtype == torch.float32:
        tol_o, tol_g = (1e-4, 1e-4), (2e-4, 1e-3)
    else:
        tol_o, tol_g = (2e-2, 2e-2), (6e-2, 5e-2)
    no_key = ~allow.any(-1)                  # (B, 1, Lq): query rows without a permitted key
    no_query = ~allow.any(-2)                # (B, 1, Lk): keys no row may attend
    names = ("out", "dq", "dk", "dv")[:len(got)]
    for name, g_ in zip(names, got):
        assert bool(torch.isfinite(g_).all()), f"{name} {what}: not finite"
    for name, g_ in zip(names, got):
        dead = (no_key.expand(B, H, Lq) if name in ("out", "dq") else no_query.expand(B, Hkv, Lk))
        z = g_[dead]
        assert torch.equal(z, torch.zeros_like(z)), f"{name} {what}: {int((z != 0).sum())} non-zero elements where nothing is permitted"
    for name, g_, r_ in zip(names, got, ref):
        atol, rtol = tol_o if name == "out" else (tol_g[0] * max(1.0, float(r_.abs().max())), tol_g[1])
        print(f"RATIO {what} {str(dtype)[6:]} {name} {_ratio(g_, r_, atol, rtol):.3f}")
        assert_close(g_, r_, atol, rtol, f"{name} {what} {dtype}")
    return no_key, no_query


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ROWS_WITHOUT_KEYS)
def test_attention_rows_without_keys_forward_backward(case, dtype):
    """Left-padded causal self-attention, cross-attention of a sample without an image, causal with Lq > Lk: out and dq of a row
    without keys and dk / dv of a key without queries are exactly zero, everything is finite and equals the fp64 reference."""
    x, key_mask, bias, allow, got, ref = _baseline(case, dtype)
    no_key, no_query = _check(case, dtype, allow, got, ref, f"rows-without-keys {case}")
    assert bool(no_key.any()), "the geometry has rows without keys"
    if case[7] is not None:
        assert bool(no_query.any()), "the geometry has keys without queries"


# The frame attn_q64_kernel's forward and dQ pass share (head_dim 64, 16-bit, no mask tensor): 256 queries per workgroup, 64 per
# wave; 64-key tiles through a three-stage LDS-DMA ring -- tiles 0 and 1 are requested before the loop, tile kt + 2 inside it, a
# ragged last tile re-reads row Lk - 1.  Hkv < H everywhere: the LDS-DMA dK / dV kernel changes head between its two buffers.
Q64_EDGES = [
    _case(1, 2, 1, 64, 64, 64, "none"),             # one tile, no ragged row: only the first request
    _case(1, 2, 1, 65, 65, 64, "causal"),           # two tiles, the second with one valid row; the dK / dV query tile re-reads row Lq - 1
    _case(1, 2, 1, 70, 128, 64, "none"),            # two full tiles; wave 1 holds 6 queries, waves 2 and 3 none (they keep the barriers)
    _case(1, 2, 1, 129, 129, 64, "block_causal"),   # three tiles: the first request inside the loop
    _case(2, 2, 1, 70, 192, 64, "causal"),          # three full tiles, decode-style offset
    _case(1, 2, 1, 257, 193, 64, "causal"),         # four tiles: the ring reuses stage 0; rows 0..63 have no key; a second workgroup with one query
    _case(1, 2, 1, 257, 256, 64, "none"),           # four full tiles
    _case(1, 4, 2, 1, 193, 64, "causal"),           # a single query row; the dK / dV double buffer walks the GQA group
]


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", Q64_EDGES)
def test_attention_64_queries_per_wave_frame_edges(case, dtype):
    """Forward and the three gradients at the edges of the shared tile walk: finite, exactly zero where nothing is permitted, the
    fp64 reference at this file's 16-bit tolerances."""
    x, key_mask, bias, allow, got, ref = _baseline(case, dtype)
    no_key, _ = _check(case, dtype, allow, got, ref, f"q64-edges {case}")
    assert bool(no_key.any()) == (case[:5] == (1, 2, 1, 257, 193)), "only the Lq = Lk + 64 causal case has rows without keys"


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_rows_without_keys_under_dropout(dtype):
    """The left-padded case with dropout drawn in the kernels, against the host's keep mask of the same (seed, head, query, key) hash."""
    from medical_image_analysis_amd import flash_attention as flash
    case = LEFTPAD[1]
    B, H, Hkv, Lq, Lk = case[:5]
    x, key_mask, bias, allow = _baseline(case, dtype)[:4]
    p, seed = 0.25, 987654321
    got = _kernel(case, *x, key_mask, bias, drop=(p, seed))
    keep = flash.dropout_keep_mask(seed, B, H, Lq, Lk, p, device=DEV)
    ref = _reference(case, *x, key_mask, bias, keep=keep, keep_scale=1.0 / (1.0 - p))
    _check(case, dtype, allow, got, ref, f"rows-without-keys dropout {case}")
    assert not torch.equal(got[0], _baseline(case, dtype)[4][0])


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", LEFTPAD + LEFTPAD_OFFSET + CROSS)
def test_attention_masked_content_does_not_leak(case, dtype):
    """K / V at masked keys and Q / dO at rows without keys are overwritten with other finite values, a quarter of them around 1e3:
    a masked score is -inf before the row maximum is taken, so every visible element comes out bit for bit the same and the
    masked ones stay exactly zero."""
    B, H, Hkv, Lq, Lk, D = case[:6]
    (q, k, v, dout), key_mask, bias, allow, base = _baseline(case, dtype)[:5]
    no_key = (~allow.any(-1)).expand(B, H, Lq)
    no_query = (~allow.any(-2)).expand(B, Hkv, Lk)
    masked_key = (~key_mask)[:, None, :].expand(B, Hkv, Lk)
    g = torch.Generator().manual_seed(77)

    def junk(t, where):
        big = torch.where(torch.rand(t.shape, generator=g) < 0.25, 1e3, 1.0)
        return torch.where(where[..., None], (torch.randn(t.shape, generator=g) * big).to(DEV, dtype), t)
    q2, k2, v2, dout2 = junk(q, no_key), junk(k, masked_key), junk(v, masked_key), junk(dout, no_key)
    assert not torch.equal(k2, k) and not torch.equal(q2, q)
    got = _kernel(case, q2, k2, v2, dout2, key_mask, bias)
    for name, a, b, dead in zip(("out", "dq", "dk", "dv"), got, base, (no_key, no_key, no_query, no_query)):
        assert torch.equal(a[~dead], b[~dead]), f"{name}: {int((a[~dead] != b[~dead]).sum())} visible elements changed"
        assert torch.equal(a[dead], torch.zeros_like(a[dead])), f"{name}: masked elements are not zero"


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_non_contiguous_key_mask(dtype):
    """The decoder passes attention_mask[:, :kv_len], a column slice: the same bits as its contiguous copy."""
    case = LEFTPAD_OFFSET[1]
    x, key_mask, bias, allow, base = _baseline(case, dtype)[:5]
    wide = torch.zeros(key_mask.shape[0], key_mask.shape[1] + 11, dtype=torch.bool, device=DEV)
    wide[:, :key_mask.shape[1]] = key_mask
    view = wide[:, :key_mask.shape[1]]
    assert not view.is_contiguous()
    for name, a, b in zip(("out", "dq", "dk", "dv"), _kernel(case, *x, view, bias), base):
        assert torch.equal(a, b), name


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", BIAS)
def test_attention_bias_forward_backward(case, dtype):
    """Additive (Lq, Lk) bias with -inf columns, -inf rows (rows 10..19 have no key) and scattered -inf: alone, with a key mask
    and under the causal mask; head_dim 32 / 64 / 128 in every dtype."""
    x, key_mask, bias, allow, got, ref = _baseline(case, dtype)
    no_key, no_query = _check(case, dtype, allow, got, ref, f"bias {case}")
    assert bool(no_key[:, :, 10:20].all()) and bool(no_query[:, :, 180:].all())


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_attention_head_dim_256_causal_left_padded_forward(dtype):
    """head_dim 256 is forward-only and 16-bit (the prompt pass): causal + a left-pad key mask, padded rows exactly zero."""
    case = HEAD_DIM_256[0]
    B, H, Hkv, Lq, Lk, D = case[:6]
    key_mask, bias = _geometry(case, DEV)
    q, k, v, dout = _inputs(case, dtype, DEV)
    allow = permitted(B, Lq, Lk, case[6], 16, key_mask, bias, DEV)
    got = _kernel(case, q, k, v, dout, key_mask, bias, backward=False)
    ref = (ref_attention(q, k, v, D ** -0.5, case[6], 16, key_mask, bias),)
    no_key, _ = _check(case, dtype, allow, got, ref, f"head_dim 256 {case}")
    assert torch.equal(no_key[1, 0], torch.arange(Lq, device=DEV) < 70) and not bool(no_key[0].any())


def test_reference_equals_sdpa_fp64_on_every_masked_geometry():
    """CPU: ref_attention in fp64 against an independent statement of the same operation -- F.scaled_dot_product_attention in fp64
    with the equivalent boolean (additive when there is a bias) attn_mask and K / V expanded with repeat_interleave -- forward and
    the three gradients to 1e-12, on every geometry of the masked tests above.  SDPA on the host returns exact zeros and zero
    gradients for a fully masked row, which is also what the CPU branch of both attention modules computes."""
    import torch.nn.functional as F
    for case in ROWS_WITHOUT_KEYS + BIAS + HEAD_DIM_256:
        B, H, Hkv, Lq, Lk, D, mask, km, has_bias = case
        key_mask, bias = _geometry(case, "cpu")
        q, k, v, dout = _inputs(case, torch.float64, "cpu")
        ref = _reference(case, q, k, v, dout, key_mask, bias)
        am = torch.ones(Lq, Lk, dtype=torch.bool)
        if mask == "causal":
            am = am.tril(Lk - Lq)
        am = am[None, None].expand(B, 1, Lq, Lk)
        if key_mask is not None:
            am = am & key_mask[:, None, None, :]
        if bias is not None:
            am = torch.where(am, 0.0, float("-inf")).double() + bias.double()
        ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        out = F.scaled_dot_product_attention(ql, kl.repeat_interleave(H // Hkv, dim=1), vl.repeat_interleave(H // Hkv, dim=1),
                                             attn_mask=am, scale=D ** -0.5)
        out.backward(dout)
        rows = am.any(-1) if am.dtype == torch.bool else (am > float("-inf")).any(-1)
        assert bool((~rows).any()), f"{case}: the geometry has rows without keys"
        assert torch.equal(ref[0][(~rows).expand(B, H, Lq)], torch.zeros(int((~rows).sum()) * H, D, dtype=torch.float64))
        for name, a, b in zip(("out", "dq", "dk", "dv"), ref, (out.detach(), ql.grad, kl.grad, vl.grad)):
            assert bool(torch.isfinite(a).all()), f"{name} {case}"
            err = float((a - b).abs().max())
            assert err <= 1e-12, f"{name} {case}: ref_attention and SDPA differ by {err:.3e}"
