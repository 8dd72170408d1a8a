"""Sampled report decoding (generate(do_sample=True, temperature, top_k, top_p, seed)): the torch contract `_SampleState.advance_torch`
against HF itself (tests/golden/decode_tiny_llama_sample.npz, made by tests/golden/make_golden_sample.py), the filters against HF's
warper classes, the counter-based uniform, seeds, validation and the host side of the ABI on the CPU; csrc/sample_step.hip against the
restatement, determinism, the end-to-end graph path and the served-kernel assertion on the GPU (-m gpu)."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden
from medical_image_analysis_amd import _abi
from medical_image_analysis_amd.report_decoder import _SampleState, sample_uniform
from test_report_decoder import KEYED, _model, _model_hd64, _model_keyed

ARGSETS = {
    "plain": dict(),
    "t07_k8": dict(temperature=0.7, top_k=8, min_new_tokens=2, repetition_penalty=2.0),
    "p09": dict(top_p=0.9, temperature=1.3, min_new_tokens=3),
    "k5p8": dict(top_k=5, top_p=0.8, repetition_penalty=1.5),
}


def _sample_golden():
    data = np.load(os.path.join(GOLDEN, "decode_tiny_llama_sample.npz"))
    return int(data["seed"]), json.loads(str(data["cases"])), {k[7:]: torch.from_numpy(data[k]) for k in data.files if k.startswith("tokens_")}


def _state(B, V, dev, max_new=12, fill=0, eos=(2,), **kw):
    return _SampleState(B, V, max_new, fill, list(eos), kw.get("min_new_tokens", 0), kw.get("repetition_penalty", 1.0),
                        kw.get("temperature", 1.0), kw.get("top_k"), kw.get("top_p", 1.0), dev)


# ---- 1. token-exact against HF ----------------------------------------------------------------------------------------------------
def test_generate_sampled_tokens_equal_hf_golden():
    """All four argument sets, all rows: HF's own processors / warpers / stopping with the repeatable draw, integer comparison."""
    seed, cases, streams = _sample_golden()
    assert set(cases) == set(ARGSETS) == set(streams)
    g = load_golden("decode_tiny_llama")
    m = _model(g, "cpu")
    for name, kw in cases.items():
        out = m.generate(g["inputs_embeds"], attention_mask=g["attention_mask"], do_sample=True, seed=seed, pad_token_id=0,
                         eos_token_id=2, **kw)
        assert torch.equal(out, streams[name]), f"{name}: tokens differ\n got {out.tolist()}\nwant {streams[name].tolist()}"


# ---- 2. filters against HF's warper classes -----------------------------------------------------------------------------------------
def _logits(V, rows, seed, bf16):
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)) * 4
    return x.bfloat16().float() if bf16 else x


@pytest.mark.parametrize("V", [48, 32000, 151936])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_top_k_and_temperature_equal_hf_warpers(V, bf16):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper
    x = _logits(V, 6, 11 + V, bf16)
    for k, T in ((1, 1.0), (8, 0.7), (50, 1.3), (V + 5, 0.9)):
        st = _state(6, V, "cpu", top_k=k, temperature=T)
        sc, keep, thresh, kept = st.scores_torch(x)
        want = TopKLogitsWarper(top_k=k)(None, TemperatureLogitsWarper(T)(None, x.clone()))
        assert torch.equal(keep, want > -float("inf")) and torch.equal(sc[keep], want[keep]), (V, k, T)
        assert torch.equal(kept, keep.sum(-1)) and torch.equal(thresh, torch.where(keep, sc, torch.full_like(sc, float("inf"))).min(-1)[0])


@pytest.mark.parametrize("V", [48, 32000, 151936])
@pytest.mark.parametrize("top_p", [0.5, 0.8, 0.9])
def test_top_p_equals_hf_warper_and_keeps_ties_together(V, top_p):
    """Tie-free fp32 inputs: the kept set is HF's exactly.  bf16-rounded inputs (many ties): ours is a superset of HF's and every extra
    token is tied in score with HF's lowest kept token.  An input whose HF cumulative sum lies within 1e-6 of 1 - top_p at the cut
    fails the test loudly instead of excusing a mismatch."""
    from transformers.generation.logits_process import TopPLogitsWarper
    for bf16 in (False, True):
        x = _logits(V, 6, 5 + V, bf16)
        want = TopPLogitsWarper(top_p=top_p)(None, x.clone()) > -float("inf")
        srt = torch.sort(x, descending=False)[0]
        cum = srt.softmax(-1).cumsum(-1)
        assert float((cum - (1 - top_p)).abs().min()) > 1e-6, "generator seed puts HF's cumulative sum on the cut: pick another"
        st = _state(6, V, "cpu", top_p=top_p)
        sc, keep, thresh, kept = st.scores_torch(x)
        if not bf16:
            assert torch.equal(keep, want), (V, top_p, int((keep & ~want).sum()), int((want & ~keep).sum()))
            continue
        assert not bool((want & ~keep).any()), "a token HF keeps is missing"
        low = torch.where(want, x, torch.full_like(x, float("inf"))).min(-1, keepdim=True)[0]
        extra = keep & ~want
        assert bool((x[extra] == low.expand_as(x)[extra]).all()), "an extra token is not tied with HF's lowest kept score"
        assert torch.equal(keep, x >= low)


# ---- 3. the uniform ---------------------------------------------------------------------------------------------------------------------
def test_sample_uniform_is_uniform_and_uncorrelated():
    """rows 0..79 x steps 0..819 at seed 1234 (65 600 fixed values): all in [0, 1), multiples of 2^-24; Kolmogorov-Smirnov distance to
    U(0, 1) 0.002555 (bound 1.95 / sqrt(n) = 0.007613, the alpha = 0.001 critical value); lag-1 correlation 0.00033 along steps and
    0.00390 along rows (bound 4 / sqrt(n) = 0.01562)."""
    u = torch.stack([sample_uniform(1234, 80, s) for s in range(820)], dim=1).numpy()          # (rows, steps)
    n = u.size
    assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all() and (u * 2 ** 24 == np.rint(u * 2 ** 24)).all()
    f = np.sort(u.ravel())
    ks = max(np.max(np.arange(1, n + 1) / n - f), np.max(f - np.arange(n) / n))
    c_step = abs(np.corrcoef(u[:, :-1].ravel(), u[:, 1:].ravel())[0, 1])
    c_row = abs(np.corrcoef(u[:-1].ravel(), u[1:].ravel())[0, 1])
    print(f"KS {ks:.6f} lag-1 steps {c_step:.5f} rows {c_row:.5f}")
    assert ks < 1.95 / math.sqrt(n) and c_step < 4 / math.sqrt(n) and c_row < 4 / math.sqrt(n), (ks, c_step, c_row)
    # the high seed word takes part, and a tensor seed / step (what the captured step passes) equals the int form
    assert not torch.equal(sample_uniform(1234, 8, 3), sample_uniform(1234 + (1 << 40), 8, 3))
    assert torch.equal(sample_uniform(torch.tensor([1234 + (5 << 33)]), 8, torch.tensor(7)), sample_uniform(1234 + (5 << 33), 8, 7))


# ---- 4. seeds and RNG hygiene ----------------------------------------------------------------------------------------------------------
def test_seeds_reproduce_and_leave_the_global_rng_alone():
    g = load_golden("decode_tiny_llama")
    m = _model(g, "cpu")
    kw = dict(attention_mask=g["attention_mask"], do_sample=True, pad_token_id=0, eos_token_id=2, max_new_tokens=12)
    a = m.generate(g["inputs_embeds"], seed=77, **kw)
    assert torch.equal(a, m.generate(g["inputs_embeds"], seed=77, **kw))
    assert not torch.equal(a, m.generate(g["inputs_embeds"], seed=78, **kw))
    before = torch.get_rng_state()
    x = m.generate(g["inputs_embeds"], **kw)
    y = m.generate(g["inputs_embeds"], **kw)
    assert torch.equal(torch.get_rng_state(), before), "generate(seed=None) drew from the global CPU generator"
    assert x.shape != y.shape or not torch.equal(x, y)
    assert len(m._sample_states) == 1                      # one cached state for one argument set


# ---- 5. validation ---------------------------------------------------------------------------------------------------------------------
def test_argument_validation_and_greedy_untouched():
    g = load_golden("decode_tiny_llama")
    m = _model(g, "cpu")
    kw = dict(attention_mask=g["attention_mask"], pad_token_id=0, eos_token_id=2, max_new_tokens=12)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            m.generate(g["inputs_embeds"], do_sample=True, temperature=bad, **kw)
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="top_p"):
            m.generate(g["inputs_embeds"], do_sample=True, top_p=bad, **kw)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="top_k"):
            m.generate(g["inputs_embeds"], do_sample=True, top_k=bad, **kw)
    with pytest.raises(NotImplementedError, match="beam-sample"):
        m.generate(g["inputs_embeds"], do_sample=True, num_beams=3, **kw)
    # the reference's default flags (--do_sample False --temperature 0) keep decoding greedily
    out = m.generate(g["inputs_embeds"], do_sample=False, temperature=0, num_beams=1, min_new_tokens=2, repetition_penalty=2.0,
                     length_penalty=2.0, **kw)
    assert torch.equal(out, g["greedy"])


def test_mirror_module_forwards_the_sampling_flags():
    import inspect
    from medical_image_analysis_amd import mambaxray_vl
    src = inspect.getsource(mambaxray_vl.MambaXrayVLDownStream.generate)
    for name in ("do_sample", "temperature", "top_k", "top_p", "seed"):
        assert re.search(name + r'=_get\(a, "' + name + '"', src), name


# ---- 6. ABI on the host ----------------------------------------------------------------------------------------------------------------
def test_sample_desc_mirrors_header():
    text = open(os.path.join(ROOT, "include", "mxvl.h")).read()
    m = re.search(r"typedef struct mxvl_sample_desc \{(.*?)\} mxvl_sample_desc;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        decl = re.sub(r"^(const\s+)?(void|int32_t|uint32_t|int64_t|float)\s*", "", decl)
        names += [n.strip().lstrip("*").strip() for n in decl.split(",")]
    assert names == [f[0] for f in _abi.SampleDesc._fields_]
    assert _abi.ABI_VERSION == 13 and "#define MXVL_ABI_VERSION 13" in text


def test_sample_step_refuses_bad_descriptors_without_gpu():
    lib = _abi.load()
    assert lib.mxvl_sample_workspace_bytes(80, 151936) == 4 * 80 * 151936 and lib.mxvl_sample_workspace_bytes(0, 5) == 0
    assert lib.mxvl_sample_workspace_bytes(2, 49) == 4 * 2 * 52

    def desc(**kw):
        d = _abi.SampleDesc()
        d.rows, d.vocab, d.max_new, d.min_new, d.n_eos, d.top_k = 6, 32000, 12, 0, 1, 0
        d.repetition_penalty, d.temperature, d.top_p = 1.0, 1.0, 1.0
        for f in ("logits", "seq", "alive", "tok", "cur", "eos", "seed", "unfinished", "scratch", "workspace"):
            setattr(d, f, 64)                               # fake non-null pointers, never dereferenced: nothing is launched
        d.workspace_bytes = 4 * 6 * 32000
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    SHAPE, NULL = -3, -1
    for kw in (dict(vocab=0), dict(vocab=-4), dict(rows=81), dict(rows=0), dict(n_eos=5), dict(top_p=0.0), dict(top_p=1.5),
               dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_k=-1), dict(max_new=0),
               dict(workspace=None), dict(workspace_bytes=4 * 6 * 32000 - 4), dict(rows=80, vocab=1 << 26, workspace_bytes=1 << 40)):
        assert lib.mxvl_sample_step(ctypes.byref(desc(**kw)), None) == SHAPE, kw
    for kw in (dict(logits=None), dict(seed=None), dict(cur=None), dict(eos=None), dict(scratch=None)):
        assert lib.mxvl_sample_step(ctypes.byref(desc(**kw)), None) == NULL, kw
    assert lib.mxvl_sample_step(None, None) == NULL


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
# Tolerance of the mass comparisons.  The kernel accumulates exp(score - max) as integers in units of 2^-40 (truncated), so its sums are
# exact in those units: the quantisation moves any partial sum by at most V * 2^-40 <= 151 936 * 2^-40 = 1.4e-7 relative to Z >= 1.  What
# is left is the per-term error of the fp32 exponential: the argument (s - max) * log2(e) is rounded to fp32 (relative 2^-24 of an
# argument x, i.e. a relative mass error |x| * ln 2 * 2^-24, weighted by the mass 2^x itself: at most 0.53 * 2^-24 summed over a row)
# plus v_exp_f32's 1 ulp (2^-23).  Together below 2^-21; EPS = 2^-19 keeps a factor of four over that, and stays below a third of the
# smallest token mass of the grid (a flat 151 936-token row: 6.6e-6).
EPS = 2.0 ** -19
GPU_SETS = dict(ARGSETS, k1=dict(top_k=1, repetition_penalty=2.0), p_tiny=dict(top_p=1e-6))


def _gpu_logits(kind, rows, V, step, dev):
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(1000 * step + rows + V)) * 4
    if kind == "bf16":
        x = x.bfloat16().float()
    elif kind == "peaked":
        x[0, (7 * step + 3) % V] += 30.0
    elif kind == "flat":
        x[rows - 1] = 1.25
    return x.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fp32", "bf16", "peaked", "flat"])
@pytest.mark.parametrize("name", list(GPU_SETS))
@pytest.mark.parametrize("rows", [1, 6, 16, 80])
@pytest.mark.parametrize("V", [48, 32000, 151936])
def test_sample_step_kernel_vs_restatement(V, rows, name, kind, record_property):
    dev, kw, steps = "cuda:0", GPU_SETS[name], 12
    eos = (2, 5)
    hip, ref = _state(rows, V, dev, max_new=steps, eos=eos, **kw), _state(rows, V, dev, max_new=steps, eos=eos, **kw)
    ref.use_hip = False
    for st in (hip, ref):
        st.seed.fill_(20240607 + (3 << 35))
    top_p, identical, total = kw.get("top_p", 1.0), 0, 0
    ninf = -float("inf")
    for step in range(steps):
        lg = _gpu_logits(kind, rows, V, step, dev)
        if step == 3 and rows > 1:
            ref.alive[rows // 2] = False                                 # a stopped row emits `fill`
        if step == 5:
            lg[0, 2] += 40.0                                             # row 0 very likely draws EOS here (not while masked by min_new)
        hip.seq.copy_(ref.seq), hip.alive.copy_(ref.alive), hip.cur.copy_(ref.cur), hip.unfinished.copy_(ref.unfinished)
        if not bool(ref.unfinished):
            break
        alive0, cur0 = ref.alive.clone(), int(ref.cur)
        sc, keep_ref, thr_ref, kept_ref = ref.scores_torch(lg)
        keep_k = sc >= torch.topk(sc, hip.top_k)[0][:, -1:] if hip.top_k > 0 else torch.ones_like(keep_ref)
        hip.advance(lg)
        ref.advance_torch(lg)
        torch.cuda.synchronize()
        ctx = (V, rows, name, kind, step)
        thr, kept = hip.out_thresh, hip.out_kept
        mass = torch.where(keep_k, (sc.double() - sc.max(-1, keepdim=True)[0].double()).exp(), torch.zeros_like(sc, dtype=torch.double))
        if top_p >= 1.0:
            assert torch.equal(thr, thr_ref) and torch.equal(kept.long(), kept_ref), (ctx, thr.tolist()[:4], thr_ref.tolist()[:4])
        else:
            p64 = mass / mass.sum(-1, keepdim=True)
            s_gt = (p64 * (sc > thr[:, None])).sum(-1)
            assert bool((s_gt < top_p + EPS).all()), (ctx, s_gt.tolist())
            below = keep_k & (sc < thr[:, None])
            nxt = torch.where(below, sc, torch.full_like(sc, ninf)).max(-1)[0]                  # next lower distinct score, if any
            s_nxt = (p64 * (sc > nxt[:, None])).sum(-1)
            assert bool(((s_nxt >= top_p - EPS) | ~below.any(-1)).all()), (ctx, s_nxt.tolist())
            assert torch.equal(kept.long(), (keep_k & (sc >= thr[:, None])).sum(-1)), ctx
        K = keep_k & (sc >= thr[:, None])
        tok = hip.tok
        assert bool((tok[~alive0] == hip.fill).all()), ctx
        t = torch.where(alive0, tok, torch.zeros_like(tok))
        assert bool(((t >= 0) & (t < V)).all()), ctx
        assert bool((K.gather(1, t[:, None])[:, 0] | ~alive0).all()), (ctx, "token outside the kept set")
        c = torch.cumsum(mass * K, dim=-1)
        Z = c[:, -1]
        hi = c.gather(1, t[:, None])[:, 0] / Z
        lo = torch.where(t > 0, c.gather(1, (t - 1).clamp(min=0)[:, None])[:, 0], torch.zeros_like(Z)) / Z
        u = sample_uniform(hip.seed, rows, cur0, device=dev)
        assert bool((((lo - EPS <= u) & (u <= hi + EPS)) | ~alive0).all()), (ctx, lo.tolist()[:4], u.tolist()[:4], hi.tolist()[:4])
        if hip.top_k == 1:
            assert bool(((sc.gather(1, t[:, None])[:, 0] == sc.max(-1)[0]) | ~alive0).all()), ctx
        # bookkeeping given the token
        alive1 = alive0 & ~torch.isin(tok, hip.eos_t)
        unf = bool(alive1.any()) and cur0 + 1 < steps
        assert torch.equal(hip.alive, alive1) and torch.equal(hip.seq[:, cur0], tok) and int(hip.cur) == cur0 + 1, ctx
        assert bool(hip.unfinished) == unf and bool(hip.unf_log[cur0]) == unf and int(hip.ticket) == 0, ctx
        same = (tok == ref.tok)
        identical, total = identical + int(same.sum()), total + rows
    record_property("draws_identical_to_restatement", f"{identical}/{total}")
    assert total > 0


@pytest.mark.gpu
def test_sample_step_kernel_is_deterministic():
    dev, V, rows = "cuda:0", 151936, 80
    lg = _gpu_logits("bf16", rows, V, 1, dev)
    outs = []
    for _ in range(2):
        st = _state(rows, V, dev, max_new=4, top_k=50, top_p=0.9, temperature=0.8, repetition_penalty=2.0)
        st.seed.fill_(99)
        st.advance(lg)
        st.advance(lg)
        torch.cuda.synchronize()
        outs.append((st.tok.clone(), st.out_thresh.clone(), st.out_kept.clone(), st.seq.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


E2E = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8, repetition_penalty=2.0, max_new_tokens=24, min_new_tokens=4,
           pad_token_id=0, eos_token_id=2)


def _e2e_model(which, dev="cuda:0"):
    if which == "hd64":
        return _model_hd64(load_golden("decode_llama_hd64"), dev, torch.bfloat16)
    return _model_keyed(load_golden(KEYED[0]), dev, torch.bfloat16)


def _prompt(m, rows, dev="cuda:0"):
    g = torch.Generator().manual_seed(rows)
    emb = torch.randn(rows, 9, m.config.hidden_size, generator=g).to(dev).bfloat16()
    att = torch.ones(rows, 9, dtype=torch.long, device=dev)
    if rows > 1:
        att[1, :3] = 0                                                     # one left-padded prompt
    return emb, att


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 6, 16])
@pytest.mark.parametrize("which", ["hd64", "hd128"])
def test_generate_sampled_on_the_kernel_stepper(which, rows):
    """(a) graph path twice with one seed: identical; (b) the torch update on the kernel stepper's logits: identical tokens (seed 4242:
    not changed after the first run); (d) seed=None twice differs; (e) one stepper, one state, no re-capture; the update ran in
    mxvl_sample_step."""
    from medical_image_analysis_amd.report_decoder import _KernelStepper
    m = _e2e_model(which)
    emb, att = _prompt(m, rows)
    lib = _abi.load()
    real, calls = lib.mxvl_sample_step, [0]

    def counted(*a):
        calls[0] += 1
        return real(*a)

    lib.mxvl_sample_step = counted
    try:
        a = m.generate(emb, attention_mask=att, seed=4242, **E2E)
        n_first = calls[0]
        b = m.generate(emb, attention_mask=att, seed=4242, **E2E)
        assert n_first >= 2 and calls[0] == n_first + 1, "the second call must replay the captured step (only the prefill update is a host call)"
    finally:
        lib.mxvl_sample_step = real
    assert a.shape[0] == rows and 1 <= a.shape[1] <= 24 and torch.equal(a, b)
    assert len(m._steppers) == 1 and type(next(iter(m._steppers.values()))) is _KernelStepper and len(m._sample_states) == 1
    stepper, state = next(iter(m._steppers.values())), next(iter(m._sample_states.values()))
    graph = stepper.sgraph
    x = m.generate(emb, attention_mask=att, **E2E)
    y = m.generate(emb, attention_mask=att, **E2E)
    assert x.shape != y.shape or not torch.equal(x, y)
    assert len(m._steppers) == 1 and len(m._sample_states) == 1 and stepper.sgraph is graph, "re-captured"
    state.use_hip, stepper.sgraph = False, None                            # the captured step holds the kernel update: capture anew
    try:
        t = m.generate(emb, attention_mask=att, seed=4242, use_graph=True, **E2E)
    finally:
        state.use_hip, stepper.sgraph = True, None
    assert torch.equal(a, t), f"kernel update {a.tolist()} vs torch update {t.tolist()}"


@pytest.mark.gpu
def test_captured_step_draws_a_fresh_number_per_token_and_row():
    """Flat logits (lm_head zeroed) at temperature 1: every token is uniform over the vocabulary, so a capture that replayed one number
    would repeat one token."""
    m = _e2e_model("hd64")
    with torch.no_grad():
        m.lm_head.weight.zero_()
    emb, att = _prompt(m, 6)
    out = m.generate(emb, attention_mask=att, do_sample=True, seed=5, max_new_tokens=24, pad_token_id=0)
    assert out.shape == (6, 24)
    assert all(len(set(r)) > 1 for r in out.tolist()) and len({tuple(r) for r in out.tolist()}) == 6
    V = m.config.vocab_size
    want = torch.stack([(sample_uniform(5, 6, s) * V).floor().long() for s in range(24)], dim=1)
    assert torch.equal(out.cpu(), want), "flat logits: the token is floor(u * V)"


@pytest.mark.gpu
def test_sampling_update_raises_instead_of_switching_to_torch():
    st = _state(3, 1000, "cuda:0", eos=(2, 3, 4, 5, 6))
    logits = torch.randn(3, 1000, device="cuda:0")
    with pytest.raises(RuntimeError, match="sample_step.hip"):
        st.advance(logits)
    st.allow_torch = True
    st.advance(logits)
    assert int(st.cur) == 1
    g = load_golden("decode_tiny_llama")                                    # fp32 / head_dim 16: not a model the decode kernels serve
    m = _model(g, "cuda:0")
    with pytest.raises(RuntimeError, match="HIP decode kernels"):
        m.generate(g["inputs_embeds"].to("cuda:0"), attention_mask=g["attention_mask"].to("cuda:0"), do_sample=True, max_new_tokens=4)
