"""kv_cache_dtype="fp8" on the GPU: the bytes the fp8-cache attention kernels append (mxvl_decode_attn with MXVL_KV_FP8,
csrc/decode.hip decode_attn_kernel / decode_attn_beams_mfma_kernel over KvE4m3), their attention against a float64 softmax over the
dequantised cache, guard bands, and generate() on the kernel stepper against the torch-module stepper."""
import ctypes

import pytest
import torch

from medical_image_analysis_amd import _abi
from medical_image_analysis_amd.report_decoder import KVCache, ReportDecoder, _KernelStepper, kv_fp8_encode

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}        # the bound of the 16-bit decode-attention tests (test_report_decoder.py)
GUARD, FILL = 4096, 0x5A


def _guarded(shape, codes=None):
    """A byte cache inside a larger buffer of FILL bytes: (whole buffer, the cache view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    if codes is not None:
        view.copy_(codes)
    return buf, view


def _random_codes(g, shape, spread=64.0):
    """Finite E4M3 codes of random values (no NaN code: the kernels may read a masked line, as the 16-bit ones do)."""
    x = torch.randn(*shape, generator=g) * spread
    return x.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def _launch(dtype, qkv, cos, sin, kc, vc, slot, pos, mask, kvs, H, Hkv, D, T, beams=0, fp8=True):
    rows = qkv.shape[0]
    out = torch.zeros(rows, H * D, dtype=dtype, device=DEV)
    qr = torch.zeros(rows, H * D, dtype=dtype, device=DEV)
    a = _abi.DecodeAttnDesc()
    a.rows, a.n_heads, a.n_kv_heads, a.head_dim, a.max_len, a.scale, a.beams = rows, H, Hkv, D, T, D ** -0.5, beams
    a.dtype = _abi.dtype_code(dtype) | (_abi.MXVL_KV_FP8 if fp8 else 0)
    a.qkv, a.cos, a.sin, a.k_cache, a.v_cache = qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr()
    a.slot_table, a.pos, a.mask, a.out, a.q_rope = slot.data_ptr(), pos.data_ptr(), mask.data_ptr(), out.data_ptr(), qr.data_ptr()
    a.kv_scale = kvs.data_ptr() if fp8 else None
    _abi.check(_abi.load().mxvl_decode_attn(ctypes.byref(a), _abi.stream_ptr(qkv.device)), "mxvl_decode_attn")
    torch.cuda.synchronize()
    return out, qr


def _patterns(dtype):
    """Every finite bit pattern of `dtype` with |x| <= 1024, both signs (zeros and subnormals included)."""
    top = {torch.bfloat16: 0x4480, torch.float16: 0x6400}[dtype]
    pos = torch.arange(0, top + 1, dtype=torch.int32)
    vals = torch.cat([pos, pos - 0x8000]).to(torch.int16).view(dtype)
    assert float(vals.float().abs().max()) == 1024.0 and bool(torch.isfinite(vals.float()).all())
    return vals


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_appended_cache_bytes_equal_torch_encode(dtype):
    """The V bytes a step appends are torch's encode of the new values, for every finite 16-bit pattern up to 1024 (round to nearest
    even, E4M3 subnormals, signed zero, the clamp at 448, OCP and not FNUZ codes), under scale 1 (per-row kernel) and 2^-3 (beams
    kernel); the K bytes are the encode of the rotated key the 16-bit kernel appends for the same input."""
    rows, H, Hkv, D, T = 64, 2, 2, 128, 2
    per = rows * Hkv * D
    vals = _patterns(dtype)
    n_calls = (vals.numel() + per - 1) // per
    vals = torch.cat([vals, vals[:n_calls * per - vals.numel()]])
    g = torch.Generator().manual_seed(3)
    cos, sin = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    cos[0, :8] = 1.0                                                    # (the K probes below keep their magnitude)
    cos, sin = cos.to(DEV), sin.to(DEV)
    slot = torch.arange(rows, dtype=torch.int32)[:, None].expand(-1, T).contiguous().to(DEV)
    mask = torch.ones(rows, T, dtype=torch.long, device=DEV)
    pos = torch.tensor([1], device=DEV)
    for s_k, s_v, beams in ((0.5, 1.0, 0), (2.0 ** -2, 2.0 ** -3, 2)):
        kvs = torch.tensor([s_k, s_v], dtype=torch.float32, device=DEV)
        for c in range(n_calls):
            qkv = (torch.randn(rows, (H + 2 * Hkv) * D, generator=g) * 4).to(dtype)
            qkv[:, (H + Hkv) * D:] = vals[c * per:(c + 1) * per].view(rows, Hkv * D)
            if c == 0:
                qkv[0, H * D:H * D + 8] = torch.tensor([3000.0, -3000.0, 0.0, -0.0, 1e-3, 448.0, 460.0, -1e-6]).to(dtype)   # K: clamp and tiny values
            qkv = qkv.to(DEV)
            kbuf, kc = _guarded((rows, Hkv, T, D), _random_codes(g, (rows, Hkv, T, D)).to(DEV))
            vbuf, vc = _guarded((rows, Hkv, T, D), _random_codes(g, (rows, Hkv, T, D)).to(DEV))
            k0, v0 = kc.clone(), vc.clone()
            _launch(dtype, qkv, cos, sin, kc, vc, slot, pos, mask, kvs, H, Hkv, D, T, beams=beams)
            want_v = kv_fp8_encode(qkv[:, (H + Hkv) * D:].view(rows, Hkv, D), kvs[1]).view(torch.uint8)
            assert torch.equal(vc[:, :, 1], want_v), (s_v, c, int((vc[:, :, 1] != want_v).sum()))
            # K: the 16-bit kernel's append is the rotated key (same arithmetic, bit-equal by the existing tests)
            k16 = torch.zeros(rows, Hkv, T, D, dtype=dtype, device=DEV)
            v16 = torch.zeros(rows, Hkv, T, D, dtype=dtype, device=DEV)
            if c == 0:
                _launch(dtype, qkv, cos, sin, k16, v16, slot, pos, mask, kvs, H, Hkv, D, T, beams=0, fp8=False)
                assert torch.equal(v16[:, :, 1].reshape(rows, -1), qkv[:, (H + Hkv) * D:])
                want_k = kv_fp8_encode(k16[:, :, 1], kvs[0]).view(torch.uint8)
                assert torch.equal(kc[:, :, 1], want_k), (s_k, int((kc[:, :, 1] != want_k).sum()))
                assert int((want_k & 0x7f == 0x7e).sum()) > 0, "the K case reaches the clamp"
            # nothing but position 1 moved, inside the caches or around them
            for buf, cache, before in ((kbuf, kc, k0), (vbuf, vc, v0)):
                assert torch.equal(cache[:, :, 0], before[:, :, 0])
                assert bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())


def _oracle(qr, kc, vc, kvs, slot, mask, pos_v, H, Hkv, D):
    """float64 softmax attention of the rotated queries the kernel wrote over the DEQUANTISED cache it appended to."""
    rows = qr.shape[0]
    K = kc.view(torch.float8_e4m3fn).double() * float(kvs[0])
    V = vc.view(torch.float8_e4m3fn).double() * float(kvs[1])
    t = torch.arange(pos_v + 1, device=DEV)
    group = H // Hkv
    ref = torch.zeros(rows, H, D, dtype=torch.float64, device=DEV)
    for m in range(rows):
        sl = slot[m, :pos_v + 1].long()
        live = mask[m, :pos_v + 1] != 0
        for h in range(H):
            sc = (K[sl, h // group, t] @ qr[m, h * D:(h + 1) * D].double()) * D ** -0.5
            ref[m, h] = torch.softmax(sc.masked_fill(~live, float("-inf")), 0) @ V[sl, h // group, t]
    return ref.reshape(rows, H * D)


def _check_untouched(buf, cache, before, pos_v):
    """Guard bands, and every byte of the cache but position pos_v."""
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all()), "bytes around the cache"
    keep = torch.ones(cache.shape[2], dtype=torch.bool, device=DEV)
    keep[pos_v] = False
    assert torch.equal(cache[:, :, keep], before[:, :, keep]), "bytes inside the cache, before and past pos"


@pytest.mark.parametrize("H,Hkv,rows", [(2, 2, 1), (4, 2, 3)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_per_row_kernel_matches_float64_attention_over_the_dequantised_cache(dtype, D, H, Hkv, rows):
    """decode_attn_kernel over KvE4m3 at pos 0, 1, one below / at / one above the positions of one workgroup trip (8 waves x 64 / (D / 16)
    lane groups), and past two trips; rows = 3: row 0 left-padded, a permuted slot table, row 2 sees only the fresh key; rows = 1:
    the only-fresh-key case at one position.  Bound: the 16-bit kernels' (an output-dtype ulp of the reference's max)."""
    NG = 8 * 64 // (D // 16)
    T = 2 * NG + 8
    g = torch.Generator().manual_seed(D + H + rows)
    kvs = torch.tensor([2.0 ** -5, 2.0 ** -4], dtype=torch.float32, device=DEV)
    codes_k, codes_v = _random_codes(g, (rows, Hkv, T, D)).to(DEV), _random_codes(g, (rows, Hkv, T, D)).to(DEV)
    cos, sin = torch.randn(rows, D, generator=g).to(DEV), torch.randn(rows, D, generator=g).to(DEV)
    for pos_v in (0, 1, NG - 1, NG, NG + 1, 2 * NG + 3):
        qkv = torch.randn(rows, (H + 2 * Hkv) * D, generator=g).to(dtype).to(DEV)
        slot = torch.randint(0, rows, (rows, T), generator=g).int()               # every row follows ancestors of its own
        slot[:, pos_v] = torch.arange(rows, dtype=torch.int32)                    # ... and owns the position it writes
        mask = torch.ones(rows, T, dtype=torch.long)
        mask[:, pos_v + 1:] = 0
        if rows == 3:
            mask[0, :min(5, pos_v)] = 0
            mask[2, :pos_v] = 0
        elif pos_v == NG + 1:
            mask[0, :pos_v] = 0
        slot, mask = slot.to(DEV), mask.to(DEV)
        pos = torch.tensor([pos_v], device=DEV)
        kbuf, kc = _guarded((rows, Hkv, T, D), codes_k)
        vbuf, vc = _guarded((rows, Hkv, T, D), codes_v)
        out, qr = _launch(dtype, qkv, cos, sin, kc, vc, slot, pos, mask, kvs, H, Hkv, D, T)
        _check_untouched(kbuf, kc, codes_k, pos_v)
        _check_untouched(vbuf, vc, codes_v, pos_v)
        ref = _oracle(qr, kc, vc, kvs, slot, mask, pos_v, H, Hkv, D)
        tol = ULP[dtype] * float(ref.abs().max())
        err = float((out.double() - ref).abs().max())
        print(f"pos {pos_v}: err / tol = {err / tol:.3f}")
        assert err <= tol, (pos_v, err, tol)
        if rows == 3:      # the row that sees only the fresh key returns exactly its dequantised value
            fresh = (vc[2, :, pos_v].view(torch.float8_e4m3fn).float() * kvs[1]).to(dtype)
            assert torch.equal(out[2].view(H, D), fresh.repeat_interleave(H // Hkv, dim=0))


_BEAMS_SHAPE = (2, 4, 2, 96, 71)             # B, H, Hkv, T, pos
_BEAMS_CASES = [pytest.param(dtype, D, nb, nsh, _BEAMS_SHAPE, id=f"{dt_id}-{D}-{nb}-{nsh_id}")
                for nsh, nsh_id in ((0, "shared0"), (21, "shared21"), (71, "shared_all")) for nb in (2, 3, 5) for D in (64, 128)
                for dtype, dt_id in ((torch.bfloat16, "bf16"), (torch.float16, "fp16"))]
_BEAMS_CASES += [pytest.param(torch.float16, 128, 4, 21, _BEAMS_SHAPE, id="fp16-128-4-shared21"),
                 pytest.param(torch.bfloat16, 128, 5, 1003, (1, 2, 2, 4400, 4350), id="bf16-128-5-waves4")]


@pytest.mark.parametrize("dtype,D,nb,nsh,shape", _BEAMS_CASES)
def test_beams_kernel_matches_float64_attention_over_the_dequantised_cache(dtype, D, nb, nsh, shape):
    """decode_attn_beams_mfma_kernel over KvE4m3: two samples of nb beams, pos = 71 (not a multiple of the 16-position tile), the
    beams' slot tables equal on the first nsh positions (0, mid-tile, all), one masked prompt position in sample 0.  The same oracle
    and bound, and the same appended bytes as the per-row kernel.  nb = 2, 3, 5 at every (D, dtype), nb = 4 at one.
    waves4 is the 4-wave instantiation: the launcher's LDS need is nw * 2 * stage + 16 * D * 2 + 4 * (3 nb D + 2 nb (nw + 1) + nb T)
    bytes with stage = 2 * 16 * D bytes of E4M3 codes; at D 128, nb 5, T 4400 that is 65536 + 4096 + 4 * (1920 + 90 + 22000) =
    165672 with 8 waves, over the 160 KiB (163840) a workgroup may have, and 32768 + 4096 + 4 * (1920 + 50 + 22000) = 132744 with
    4.  One sample, pos = 4350 (mid-tile), the beams agree on the first 1003 positions (mid-tile)."""
    B, H, Hkv, T, pos_v = shape
    rows = B * nb
    g = torch.Generator().manual_seed(D + 7 * nb + nsh)
    kvs = torch.tensor([2.0 ** -4, 2.0 ** -6], dtype=torch.float32, device=DEV)
    codes_k, codes_v = _random_codes(g, (rows, Hkv, T, D)).to(DEV), _random_codes(g, (rows, Hkv, T, D)).to(DEV)
    cos, sin = torch.randn(rows, D, generator=g).to(DEV), torch.randn(rows, D, generator=g).to(DEV)
    qkv = torch.randn(rows, (H + 2 * Hkv) * D, generator=g).to(dtype).to(DEV)
    own = torch.arange(rows, dtype=torch.int32)[:, None]
    slot = own.expand(-1, T).contiguous()
    slot[:, :nsh] = (own // nb) * nb
    for t in range(nsh + 1, pos_v):                                   # (position nsh itself: every beam its own line)
        slot[:, t] = (own[:, 0] // nb) * nb + torch.randint(0, nb, (rows,), generator=g).int()
    slot[:, pos_v] = own[:, 0]
    mask = torch.ones(rows, T, dtype=torch.long)
    mask[:nb, 3] = 0
    mask[:, pos_v + 1:] = 0
    slot, mask = slot.to(DEV), mask.to(DEV)
    pos = torch.tensor([pos_v], device=DEV)
    res = []
    for beams in (0, nb):
        kbuf, kc = _guarded((rows, Hkv, T, D), codes_k)
        vbuf, vc = _guarded((rows, Hkv, T, D), codes_v)
        out, qr = _launch(dtype, qkv, cos, sin, kc, vc, slot, pos, mask, kvs, H, Hkv, D, T, beams=beams)
        _check_untouched(kbuf, kc, codes_k, pos_v)
        _check_untouched(vbuf, vc, codes_v, pos_v)
        res.append((out, qr, kc, vc))
    (o0, q0, k0, v0), (o1, q1, k1, v1) = res
    assert torch.equal(q0, q1) and torch.equal(k0, k1) and torch.equal(v0, v1), "rotated query / cache append are the same arithmetic"
    ref = _oracle(q0, k0, v0, kvs, slot, mask, pos_v, H, Hkv, D)
    tol = ULP[dtype] * float(ref.abs().max())
    for name, o in (("per-row", o0), ("beams", o1)):
        err = float((o.double() - ref).abs().max())
        print(f"{name}: err / tol = {err / tol:.3f}")
        assert err <= tol, (name, err, tol)


# ---- end to end on the smallest model the kernels serve (the `_servable` shape of tests/test_int8_decode.py) ---------------------------
def _servable(dtype):
    torch.manual_seed(7)
    return ReportDecoder(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2,
                         num_key_value_heads=2, rms_norm_eps=1e-6, max_position_embeddings=128).to(dtype).eval()


def _e2e_prompt(dtype, seed):
    return torch.randn(2, 6, 128, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _e2e_kwargs(mode):
    kw = dict(max_new_tokens=8, min_new_tokens=2, eos_token_id=2, pad_token_id=0, kv_cache_dtype="fp8")
    if mode == "beam3":
        kw.update(num_beams=3, repetition_penalty=2.0, length_penalty=2.0)
    elif mode == "sampled":
        kw.update(do_sample=True, temperature=0.9, top_k=20, top_p=0.9, seed=11)
    return kw


def _not_a_near_tie(make, dtype, seed, kw):
    """test_int8_decode.py's rule: the case counts only if the CPU torch path gives the same tokens in bf16 and fp32 (asserted)."""
    cpu16 = make().generate(_e2e_prompt(dtype, seed), use_graph=False, **kw)
    cpu32 = make().float().generate(_e2e_prompt(dtype, seed).float(), use_graph=False, **kw)
    assert torch.equal(cpu16, cpu32), f"seed {seed}: the torch-path decode of this case sits on a near-tie; pick another prompt"


@pytest.mark.parametrize("mode", ["greedy", "beam3", "sampled"])
@pytest.mark.parametrize("weights,seeds", [("16bit", (5, 29)), ("mxfp4", (6,))])
def test_fp8_kernel_stepper_end_to_end(weights, seeds, mode):
    """generate(kv_cache_dtype="fp8") on the kernel stepper (captured graph) against use_graph="torch" on the same device, bf16,
    token for token: greedy, beam 3 at batch 2, sampled with a fixed seed; 16-bit weights over two prompts -- the second one reuses
    the first one's captured stepper, whose scales reset() refilled -- and MXFP4 weights once."""
    dtype = torch.bfloat16
    kw = _e2e_kwargs(mode)
    make = (lambda: _servable(dtype).quantize_mxfp4_()) if weights == "mxfp4" else (lambda: _servable(dtype))
    for seed in seeds:
        _not_a_near_tie(make, dtype, seed, kw)
    model = make().to(DEV)
    rows = 6 if mode == "beam3" else 2
    assert _KernelStepper.supported(model, rows, dtype, DEV, "fp8")
    refs = [model.generate(_e2e_prompt(dtype, seed).to(DEV), use_graph="torch", **kw) for seed in seeds]
    model.__dict__.pop("_steppers", None)               # (the torch-module stepper of the calls above)
    first = None
    for seed, ref in zip(seeds, refs):
        if first is not None:
            first.kv_scale.fill_(3.0)                   # stale scales: reset() has to refill them from the new prompt
        got = model.generate(_e2e_prompt(dtype, seed).to(DEV), use_graph=True, **kw)
        assert torch.equal(got.cpu(), ref.cpu()), (mode, seed, got.tolist(), ref.tolist())
        st = list(model._steppers.values())
        assert len(st) == 1 and type(st[0]) is _KernelStepper and st[0].kv8 and st[0].kc[0].dtype == torch.uint8
        assert st[0].kc[0].shape == (rows, 2, 6 + 8, 64) and st[0].kv_scale.shape == (2, 2)
        assert st[0].graph is not None or st[0].sgraph is not None
        assert first is None or st[0] is first, "one stepper, captured once, reused by the second prompt"
        first = st[0]
        # the scales in the stepper are the prompt's (what a prefill into an fp8 cache fixes)
        cache = KVCache("fp8")
        with torch.no_grad():
            model.forward(_e2e_prompt(dtype, seed).to(DEV), attention_mask=torch.ones(2, 6, dtype=torch.long, device=DEV), past_key_values=cache)
        assert torch.equal(first.kv_scale, torch.stack([cache.scale[0], cache.scale[1]]))
    # a 16-bit call afterwards is another stepper (the mode is part of the key) with 16-bit caches
    kw16 = dict(kw, kv_cache_dtype=None)
    model.generate(_e2e_prompt(dtype, seeds[0]).to(DEV), use_graph=True, **kw16)
    assert sorted(s.kv8 for s in model._steppers.values()) == [False, True]


def test_head_dim_256_with_fp8_raises():
    torch.manual_seed(0)
    m = ReportDecoder(vocab_size=32, hidden_size=512, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1, rms_norm_eps=1e-6, max_position_embeddings=64).to(torch.bfloat16).eval().to(DEV)
    emb = torch.randn(1, 4, 512, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(DEV)
    kw = dict(max_new_tokens=3, eos_token_id=2, pad_token_id=0)
    with pytest.raises(RuntimeError, match="kv_cache_dtype='fp8'"):
        m.generate(emb, use_graph=True, kv_cache_dtype="fp8", **kw)
    assert _KernelStepper.supported(m, 1, torch.bfloat16, DEV) and not _KernelStepper.supported(m, 1, torch.bfloat16, DEV, "fp8")
    lib = _abi.load()
    a = _abi.DecodeAttnDesc()
    a.rows, a.n_heads, a.n_kv_heads, a.head_dim, a.max_len, a.scale = 1, 2, 1, 256, 8, 1.0
    a.dtype = _abi.MXVL_BF16 | _abi.MXVL_KV_FP8
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    for f in ("qkv", "cos", "sin", "k_cache", "v_cache", "slot_table", "pos", "mask", "out", "kv_scale"):
        setattr(a, f, buf.data_ptr())
    assert lib.mxvl_decode_attn(ctypes.byref(a), _abi.stream_ptr(buf.device)) == -7
