"""no_repeat_ngram_size for report decoding (generate(no_repeat_ngram_size=n), greedy / beam search / sampled): the torch contract
against HF itself (tests/golden/decode_tiny_llama_ngram.npz, made by tests/golden/make_golden_ngram.py), `ngram_banned` and the two
restatements against HF's NoRepeatNGramLogitsProcessor on crafted histories, validation and the host side of the ABI on the CPU;
csrc/beam_step.hip and csrc/sample_step.hip against the restatements on histories written into the state, and the end-to-end graph
path on the GPU (-m gpu)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from medical_image_analysis_amd import _abi
from medical_image_analysis_amd.report_decoder import _BeamState, _SampleState, ngram_banned, sample_uniform
from test_report_decoder import HD64_BEAM, HD64_GEN, KEYED, _model, _model_hd64, _model_keyed

NINF = -float("inf")


def _golden():
    data = np.load(os.path.join(GOLDEN, "decode_tiny_llama_ngram.npz"))
    return int(data["seed"]), json.loads(str(data["cases"])), {k[7:]: torch.from_numpy(data[k]) for k in data.files if k.startswith("tokens_")}


# ---- 1. token-exact against HF ----------------------------------------------------------------------------------------------------
def test_generate_with_ngram_ban_equals_hf_golden():
    """Every stored case (n in {1, 2, 3} x greedy / beam 3 / sampled; the generator asserted that each differs from its unflagged
    decode), all rows, integer comparison."""
    seed, cases, streams = _golden()
    assert set(cases) == set(streams) and len(cases) >= 9
    for kind in ("greedy", "beam3", "sample"):
        assert {kw["no_repeat_ngram_size"] for name, kw in cases.items() if name.startswith(kind)} == {1, 2, 3}, kind
    g = load_golden("decode_tiny_llama")
    m = _model(g, "cpu")
    for name, kw in cases.items():
        extra = dict(seed=seed) if kw.get("do_sample") else dict(do_sample=False)
        out = m.generate(g["inputs_embeds"], attention_mask=g["attention_mask"], pad_token_id=0, eos_token_id=2, **extra, **kw)
        assert out.shape == streams[name].shape and torch.equal(out, streams[name]), \
            f"{name}: tokens differ\n got {out.tolist()}\nwant {streams[name].tolist()}"


# ---- 2. the restatements against HF's class ---------------------------------------------------------------------------------------
V0, MAXNEW = 48, 16


def _crafted(n):
    """{cur: (rows, cur) histories}: cur + 1 < n; a prefix that occurs three times with two distinct followers (and ends the row, so
    both are banned); a row of distinct tokens (the only occurrence of its suffix is the suffix itself: no ban); small-alphabet random
    rows at every length up to a full history."""
    out = {}
    for cur in range(0, max(n - 1, 1)):                                   # cur + 1 < n (and cur = 0)
        out.setdefault(cur, []).append(list(range(3, 3 + cur)))
    pre = [5, 6, 8][:n - 1]
    rep = pre + [7] + pre + [9] + pre + [7] + pre                          # followers 7, 9, 7 -> {7, 9}; at most 15 tokens
    out.setdefault(len(rep), []).append(rep)
    out[len(rep)].append(list(range(20, 20 + len(rep))))                   # all distinct
    gen = torch.Generator().manual_seed(100 + n)
    for cur in range(0, MAXNEW):
        rows = torch.randint(0, 4, (5, cur), generator=gen) * 13 + 1       # alphabet {1, 14, 27, 40}
        out.setdefault(cur, []).extend(rows.tolist())
    return {cur: torch.tensor(rows, dtype=torch.long).reshape(len(rows), cur) for cur, rows in out.items()}


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_restatements_equal_hf_no_repeat_ngram_processor(n):
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor
    proc = NoRepeatNGramLogitsProcessor(n)
    fired = 0
    for cur, ids in _crafted(n).items():
        rows = ids.shape[0]
        x = torch.randn(rows, V0, generator=torch.Generator().manual_seed(cur))
        want = proc(ids, x.clone()) == NINF
        hist = torch.full((rows, MAXNEW), 45, dtype=torch.long)            # unwritten slots hold a token that must not matter
        hist[:, :cur] = ids
        got = ngram_banned(hist, torch.tensor(cur), n, V0)
        assert torch.equal(got, want), (n, cur, ids.tolist(), got.nonzero().tolist(), want.nonzero().tolist())
        fired += int(want.sum())
        if cur + 1 < n:
            assert not bool(want.any())
        # the sampling restatement: the -inf set of the processed scores, with and without the penalty in front of it
        for pen in (1.0, 2.0):
            st = _SampleState(rows, V0, MAXNEW, 0, [2], 0, pen, 1.0, None, 1.0, "cpu", n)
            st.seq.copy_(hist), st.cur.fill_(cur)
            sc = st.scores_torch(x)[0]
            assert torch.equal(sc == NINF, want), (n, cur, pen)
            off = _SampleState(rows, V0, MAXNEW, 0, [2], 0, pen, 1.0, None, 1.0, "cpu")
            off.seq.copy_(hist), off.cur.fill_(cur)
            assert torch.equal(sc[~want], off.scores_torch(x)[0][~want])   # everything else is what the unflagged state computes
        # the beam restatement: one beam row per history (B = rows, nb = 1 ... nb = 2 keeps `keep` = 4 candidates)
        assert cur < MAXNEW
        bs = _BeamState(rows, 2, V0, MAXNEW, 0, [], 0, 2.0, 1.0, False, "cpu", n)
        bs.run_seq[:, 0].copy_(hist), bs.run_seq[:, 1].copy_(hist), bs.cur.fill_(cur)
        lg = x.repeat_interleave(2, dim=0)
        bs.advance_torch(lg)
        if cur + 1 < MAXNEW:
            assert not bool(want.gather(1, bs.tok.view(rows, 2)).any()), (n, cur, "a banned token was chosen")
            logp = torch.log_softmax(x, -1)
            hit = torch.zeros_like(want).scatter_(1, ids, True) if cur else torch.zeros_like(want)
            logp = torch.where(hit, torch.where(logp < 0, logp * 2.0, logp / 2.0), logp).masked_fill(want, NINF)
            assert torch.equal(bs.tok.view(rows, 2), logp.topk(2, -1)[1]), (n, cur)
    assert fired > 0
    if n == 2:                                                             # the documented case, spelled out
        h = torch.tensor([[5, 7, 5, 9, 5, 7, 11, 5] + [0] * 8])
        assert ngram_banned(h, torch.tensor(8), 2, V0)[0].nonzero().flatten().tolist() == [7, 9]
    assert ngram_banned(torch.tensor([[3, 4, 3, 0]]), torch.tensor(3), 1, V0)[0].nonzero().flatten().tolist() == [3, 4]


# ---- 3. validation and ABI ----------------------------------------------------------------------------------------------------------
def test_argument_validation_names_the_argument():
    g = load_golden("decode_tiny_llama")
    m = _model(g, "cpu")
    kw = dict(attention_mask=g["attention_mask"], pad_token_id=0, eos_token_id=2, max_new_tokens=4)
    for mode in (dict(), dict(num_beams=3), dict(do_sample=True, seed=1)):
        for bad in (True, False, 2.0, "2", None, -1):
            with pytest.raises(ValueError, match="no_repeat_ngram_size"):
                m.generate(g["inputs_embeds"], no_repeat_ngram_size=bad, **mode, **kw)
    assert not m.__dict__.get("_beam_states") and not m.__dict__.get("_sample_states")        # refused before anything was built
    a = m.generate(g["inputs_embeds"], num_beams=3, **kw)
    assert torch.equal(a, m.generate(g["inputs_embeds"], num_beams=3, no_repeat_ngram_size=0, **kw))
    assert len(m._beam_states) == 1                                        # 0 is the default: one cached state
    m.generate(g["inputs_embeds"], num_beams=3, no_repeat_ngram_size=2, **kw)
    assert len(m._beam_states) == 2                                        # the value is part of the search-state key


def test_descriptor_word_keeps_its_place_and_negative_values_are_refused():
    """The former `reserved0` of both descriptors: same offset, same struct sizes as on the parent commit (184 and 160 bytes: 10 x 4
    bytes of scalars, 17 pointers + one int64 / one int64 + 11 pointers + one int64 + 2 pointers), ABI 13; a negative value is
    MXVL_ERR_SHAPE from both entries before any launch (fake pointers, no GPU)."""
    assert _abi.ABI_VERSION == 13
    assert ctypes.sizeof(_abi.BeamDesc) == 184 and ctypes.sizeof(_abi.SampleDesc) == 160
    for cls, before in ((_abi.BeamDesc, "repetition_penalty"), (_abi.SampleDesc, "top_p")):
        names = [f[0] for f in cls._fields_]
        assert "reserved0" not in names and names.index("no_repeat_ngram_size") == names.index(before) + 1
        f = cls.no_repeat_ngram_size
        assert f.offset == 36 and f.size == 4 and getattr(cls, before).offset == 32
    lib = _abi.load()
    SHAPE = -3
    s = _abi.SampleDesc()
    s.rows, s.vocab, s.max_new, s.min_new, s.n_eos, s.top_k = 6, 32000, 12, 0, 1, 0
    s.repetition_penalty, s.temperature, s.top_p = 1.0, 1.0, 1.0
    for f in ("logits", "seq", "alive", "tok", "cur", "eos", "seed", "unfinished", "scratch", "workspace"):
        setattr(s, f, 64)                                   # fake non-null pointers, never dereferenced: nothing is launched
    s.workspace_bytes = 4 * 6 * 32000
    b = _abi.BeamDesc()
    b.batch, b.beams, b.vocab, b.max_new, b.min_new, b.n_eos, b.early_stopping, b.keep = 2, 3, 32000, 12, 0, 1, 0, 6
    b.repetition_penalty = 2.0
    for f in ("logits", "run_seq", "fin_seq", "run_score", "fin_score", "fin_done", "heur_open", "cur", "eos", "len_tab", "hyp_tab",
              "tok", "beam_src", "unfinished"):
        setattr(b, f, 64)
    for bad in (-1, -2 ** 31):
        s.no_repeat_ngram_size = b.no_repeat_ngram_size = bad
        assert lib.mxvl_sample_step(ctypes.byref(s), None) == SHAPE
        assert lib.mxvl_beam_step(ctypes.byref(b), None) == SHAPE


# ---- GPU: the kernels against the restatements ---------------------------------------------------------------------------------------
STEPS = 12          # max_new of the kernel tests: single updates at cur = 0 .. 11 (the update at cur = 11 reads a history of 11 tokens
#                     and writes the 12th: the full history)
EOS = 2


def _alphabet(V):
    """History tokens: EOS, tokens on both sides of the bitmap tile edges (8192 in the slice kernel, 32 768 in the one-workgroup
    kernel), the last word of the row."""
    return [EOS, 5, V - 1] + ([7, 31, 47 % V] if V < 8192 else [8191, 8192, 32767 % V, 32768 % V, (V // 2) | 1])


def _histories(rows, cur, V, gen):
    """(rows, STEPS) with [:, :cur] drawn from 3 of the alphabet's tokens per row (so n-grams repeat from the third token on); the rest
    holds another token that must not matter.  Row 0 repeats one token: the longest runs."""
    alpha = torch.tensor(_alphabet(V))
    pick = torch.stack([alpha[torch.randperm(alpha.numel(), generator=gen)[:3]] for _ in range(rows)])      # (rows, 3)
    h = torch.gather(pick, 1, torch.randint(0, 3, (rows, STEPS), generator=gen))
    h[0] = pick[0, 0]
    h[:, cur:] = 9
    return h, pick


def _logits(rows, V, pick, gen, dev):
    """Random logits with the row's history tokens on top (the banned ones among them would win: a banned token that is the arg-max,
    and every banned token is in the penalty history), distinct boosts so that no decision is a tie."""
    x = 3.0 * torch.randn(rows, V, generator=gen, device=dev)
    boost = 14.0 + 2.0 * torch.rand(rows, 3, generator=gen, device=dev) + torch.tensor([4.0, 2.0, 0.0], device=dev)
    x.scatter_add_(1, pick.to(dev), boost)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False], ids=["split", "one_wg"])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 6, 16])
@pytest.mark.parametrize("nb", [3, 5])
@pytest.mark.parametrize("V", [48, 32000, 151936])
def test_beam_step_kernel_with_ngram_ban_equals_restatement(V, nb, B, n, split):
    """csrc/beam_step.hip, both layouts, against _BeamState.advance_torch: single updates at every cur from histories written into the
    state (comparison rules and tolerances of test_beam_step_kernel_equals_torch_restatement).  min_new = 6: EOS is banned AND masked
    at cur < 6 wherever it is in a row's history."""
    dev, R = "cuda:0", B * nb
    mk = lambda: _BeamState(B, nb, V, STEPS, 0, [EOS], 6, 2.0, 2.0, False, dev, n)
    hip, ref = mk(), mk()
    hip.split_vocab, ref.use_hip = split, False
    cpu, gg = torch.Generator().manual_seed(V + 100 * nb + B + n), torch.Generator(device=dev).manual_seed(V + nb + B + n)
    fired = 0
    for cur in range(STEPS):
        h, pick = _histories(R, cur, V, cpu)
        score = -(torch.rand(B, nb, generator=cpu) * 3.0 + cur)
        for st in (hip, ref):
            st.reset()
            st.run_seq.copy_(h.view(B, nb, STEPS)), st.run_score.copy_(score), st.cur.fill_(cur)
        banned = ngram_banned(h.to(dev), ref.cur, n, V)
        fired += int(banned.sum())
        lg = _logits(R, V, pick, gg, dev)
        hip.advance(lg.clone())
        ref.advance(lg.clone())
        torch.cuda.synchronize()
        ctx = (V, nb, B, n, split, cur)
        assert int(hip.cur) == int(ref.cur) == cur + 1 and bool(hip.unfinished) == bool(ref.unfinished), ctx
        assert int(hip.ticket) == 0, ctx
        if bool(ref.unfinished):   # once every candidate has stopped the "live" beams are exact -1e9 ties: their order is arbitrary
            assert torch.equal(hip.tok, ref.tok) and torch.equal(hip.beam_src, ref.beam_src), (ctx, hip.tok.tolist(), ref.tok.tolist())
            assert torch.equal(hip.run_seq[:, :, :cur + 1], ref.run_seq[:, :, :cur + 1]), ctx
            assert torch.allclose(hip.run_score, ref.run_score, rtol=2e-6, atol=2e-5), ctx
            live = hip.run_score.view(-1) > -1e8                            # a row that continues a parent with a real token
            assert not bool((banned[hip.beam_src, hip.tok] & live).any()), (ctx, "a banned token was chosen")
        assert torch.equal(hip.fin_done, ref.fin_done) and torch.equal(hip.heur_open, ref.heur_open), ctx
        done = ref.fin_done
        assert torch.allclose(hip.fin_score[done], ref.fin_score[done], rtol=2e-6, atol=2e-5), ctx
        assert torch.equal(hip.fin_seq[done], ref.fin_seq[done]), ctx
        # a finished hypothesis ends in the token its parent row was allowed to emit
        if bool(done.any()):
            fs = hip.fin_seq[done]
            assert bool((fs[:, cur] == EOS).all()) or cur + 1 == STEPS, ctx
    assert fired > 0, "no ban fired: the histories pin nothing"


SAMPLE_SETS = {"k8_rep": dict(top_k=8, temperature=0.7, repetition_penalty=2.0), "plain": dict()}
EPS = 2.0 ** -19    # mass comparisons: as derived in tests/test_sample_decode.py (fixed-point masses, fp32 exponential)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SAMPLE_SETS))
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("rows", [1, 6, 80])
@pytest.mark.parametrize("V", [48, 32000, 151936])
def test_sample_step_kernel_with_ngram_ban_vs_restatement(V, rows, n, name):
    """csrc/sample_step.hip against _SampleState.scores_torch / advance_torch (comparison rules of
    test_sample_step_kernel_vs_restatement, top_p = 1: smallest kept score and kept count are the restatement's exactly; the token lies
    in the kept set and in the interval of the uniform).  Two EOS ids, min_new = 6: a banned EOS while cur < min_new."""
    dev, kw = "cuda:0", SAMPLE_SETS[name]
    mk = lambda: _SampleState(rows, V, STEPS, 0, [EOS, 5], 6, kw.get("repetition_penalty", 1.0), kw.get("temperature", 1.0),
                              kw.get("top_k"), 1.0, dev, n)
    hip, ref = mk(), mk()
    ref.use_hip = False
    cpu, gg = torch.Generator().manual_seed(V + rows + n), torch.Generator(device=dev).manual_seed(V + rows + n)
    fired = 0
    for cur in range(STEPS):
        h, pick = _histories(rows, cur, V, cpu)
        for st in (hip, ref):
            st.reset()
            st.seq.copy_(h), st.cur.fill_(cur), st.seed.fill_(20240607 + (3 << 35))
            if rows > 1 and cur % 4 == 3:
                st.alive[rows // 2] = False                                 # a stopped row emits `fill`
        alive0 = ref.alive.clone()
        banned = ngram_banned(h.to(dev), ref.cur, n, V)
        fired += int(banned.sum())
        lg = _logits(rows, V, pick, gg, dev)
        sc, keep_ref, thr_ref, kept_ref = ref.scores_torch(lg)
        assert bool((sc[banned] == NINF).all())
        hip.advance(lg)
        ref.advance_torch(lg)
        torch.cuda.synchronize()
        ctx = (V, rows, n, name, cur)
        assert torch.equal(hip.out_thresh, thr_ref) and torch.equal(hip.out_kept.long(), kept_ref), \
            (ctx, hip.out_thresh.tolist()[:4], thr_ref.tolist()[:4], hip.out_kept.tolist()[:4], kept_ref.tolist()[:4])
        tok = hip.tok
        assert bool((tok[~alive0] == hip.fill).all()), ctx
        t = torch.where(alive0, tok, torch.zeros_like(tok))
        assert bool(((t >= 0) & (t < V)).all()), ctx
        assert not bool((banned.gather(1, t[:, None])[:, 0] & alive0).any()), (ctx, "a banned token was drawn")
        assert bool((keep_ref.gather(1, t[:, None])[:, 0] | ~alive0).all()), (ctx, "token outside the kept set")
        mass = torch.where(keep_ref, (sc.double() - sc.max(-1, keepdim=True)[0].double()).exp(), torch.zeros_like(sc, dtype=torch.double))
        c = torch.cumsum(mass, dim=-1)
        Z = c[:, -1]
        hi = c.gather(1, t[:, None])[:, 0] / Z
        lo = torch.where(t > 0, c.gather(1, (t - 1).clamp(min=0)[:, None])[:, 0], torch.zeros_like(Z)) / Z
        u = sample_uniform(hip.seed, rows, cur, device=dev)
        assert bool((((lo - EPS <= u) & (u <= hi + EPS)) | ~alive0).all()), (ctx, lo.tolist()[:4], u.tolist()[:4], hi.tolist()[:4])
        alive1 = alive0 & ~torch.isin(tok, hip.eos_t)
        unf = bool(alive1.any()) and cur + 1 < STEPS
        assert torch.equal(hip.alive, alive1) and torch.equal(hip.seq[:, cur], tok) and int(hip.cur) == cur + 1, ctx
        assert torch.equal(hip.seq[:, :cur], h[:, :cur].to(dev)), ctx
        assert bool(hip.unfinished) == unf and bool(hip.unf_log[cur]) == unf and int(hip.ticket) == 0, ctx
    assert fired > 0, "no ban fired: the histories pin nothing"


# ---- GPU: end to end on the kernel stepper ---------------------------------------------------------------------------------------------
def _e2e_model(which, dev="cuda:0"):
    if which == "hd64":
        g = load_golden("decode_llama_hd64")
        return g, _model_hd64(g, dev, torch.bfloat16)
    g = load_golden(KEYED[0])
    return g, _model_keyed(g, dev, torch.bfloat16)


def _repeated_bigrams(out, eos=EOS):
    """Rows (token lists up to and including the first EOS; what follows is padding) that hold some bigram twice."""
    bad = []
    for r, row in enumerate(out.tolist()):
        row = row[:row.index(eos) + 1] if eos in row else row
        grams = list(zip(row, row[1:]))
        if len(grams) != len(set(grams)):
            bad.append((r, row))
    return bad


class _Launches:
    """Records the names that go through _abi.launch (the package's one launch path) while active."""

    def __enter__(self):
        self.names, self.real = [], _abi.launch
        _abi.launch = lambda name, *a, **k: (self.names.append(name), self.real(name, *a, **k))[1]
        return self

    def __exit__(self, *exc):
        _abi.launch = self.real


LONG = dict(max_new_tokens=24, min_new_tokens=20, pad_token_id=0, eos_token_id=2)      # no repetition penalty: the tiny models repeat


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["hd64", "hd128"])
def test_generate_beam3_with_ngram_ban_on_the_kernel_stepper(which):
    """generate(num_beams=3, no_repeat_ngram_size=2) runs on the kernels: the first call captures the step, the second replays it --
    its only host-side launch is the prefill's mxvl_beam_step, every later update (ban included) is inside the graph replay, one per
    token; no row repeats a bigram; a call without the flag still reproduces HF's golden tokens."""
    from medical_image_analysis_amd.report_decoder import _KernelStepper
    g, m = _e2e_model(which)
    emb, att = g["inputs_embeds"].to("cuda:0").bfloat16(), g["attention_mask"].to("cuda:0")
    kw = dict(attention_mask=att, num_beams=3, do_sample=False, length_penalty=2.0, no_repeat_ngram_size=2, **LONG)
    a = m.generate(emb, **kw)
    with _Launches() as rec:
        b = m.generate(emb, **kw)
    # (the prompt prefill launches its own kernels; nothing of the decode step or the search update is launched outside the replay)
    assert [x for x in rec.names if x.startswith("mxvl_decode") or x.endswith("_step")] == ["mxvl_beam_step"], rec.names
    assert torch.equal(a, b) and a.shape[1] >= 20
    assert len(m._steppers) == 1 and type(next(iter(m._steppers.values()))) is _KernelStepper and len(m._beam_states) == 1
    state = next(iter(m._beam_states.values()))
    assert state.no_repeat == 2 and a.shape[1] <= int(state.cur) <= 24, "one update per generated token"
    assert _repeated_bigrams(a) == [], _repeated_bigrams(a)
    plain = m.generate(emb, **dict(kw, no_repeat_ngram_size=0))
    assert len(m._beam_states) == 2
    if _repeated_bigrams(plain):
        assert not torch.equal(a, plain)
    # the torch update on the kernel stepper's logits: identical tokens
    stepper = next(iter(m._steppers.values()))
    state.use_hip, stepper.sgraph = False, None
    try:
        t = m.generate(emb, use_graph=True, **kw)
    finally:
        state.use_hip, stepper.sgraph = True, None
    assert torch.equal(a, t), f"kernel update {a.tolist()} vs torch update {t.tolist()}"
    # same arguments as the golden but for the flag, then without it: the cached state does not leak the flag
    m.generate(emb, attention_mask=att, use_graph=True, no_repeat_ngram_size=2, **HD64_BEAM, **HD64_GEN)
    out = m.generate(emb, attention_mask=att, use_graph=True, no_repeat_ngram_size=0, **HD64_BEAM, **HD64_GEN)
    assert torch.equal(out.cpu(), g["beam3"]), f"{out.cpu().tolist()} vs HF {g['beam3'].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["hd64", "hd128"])
def test_generate_sampled_with_ngram_ban_on_the_kernel_stepper(which):
    """generate(do_sample=True, no_repeat_ngram_size=2): as above with mxvl_sample_step; the unflagged call before and after the
    flagged ones gives the same tokens for one seed."""
    from medical_image_analysis_amd.report_decoder import _KernelStepper
    g, m = _e2e_model(which)
    emb, att = g["inputs_embeds"].to("cuda:0").bfloat16(), g["attention_mask"].to("cuda:0")
    kw = dict(attention_mask=att, do_sample=True, seed=4242, temperature=0.5, top_k=4, **LONG)
    before = m.generate(emb, **kw)
    a = m.generate(emb, no_repeat_ngram_size=2, **kw)
    with _Launches() as rec:
        b = m.generate(emb, no_repeat_ngram_size=2, **kw)
    # (the prompt prefill launches its own kernels; nothing of the decode step or the search update is launched outside the replay)
    assert [x for x in rec.names if x.startswith("mxvl_decode") or x.endswith("_step")] == ["mxvl_sample_step"], rec.names
    assert torch.equal(a, b) and a.shape[1] >= 20
    assert len(m._steppers) == 1 and type(next(iter(m._steppers.values()))) is _KernelStepper and len(m._sample_states) == 2
    state = [s for s in m._sample_states.values() if s.no_repeat == 2][0]
    assert int(state.cur) == a.shape[1], "one update per generated token"
    assert _repeated_bigrams(a) == [], _repeated_bigrams(a)
    if _repeated_bigrams(before):
        assert not torch.equal(a, before)
    after = m.generate(emb, **kw)
    assert torch.equal(before, after), "the unflagged decode changed after a flagged one"
    stepper = next(iter(m._steppers.values()))
    state.use_hip, stepper.sgraph = False, None
    try:
        t = m.generate(emb, no_repeat_ngram_size=2, use_graph=True, **kw)
    finally:
        state.use_hip, stepper.sgraph = True, None
    assert torch.equal(a, t), f"kernel update {a.tolist()} vs torch update {t.tolist()}"
