"""Report decoder: decoder-only LM built from the hybrid decoder layers + the autoregressive generation loop.

Replaces, for the MambaXray-VL report path, what the reference delegates to HF transformers:
  CXPMRG_Bench_MambaXray_VL/models/MambaXrayVL_DownStream.py:292-301, 389-398
      self.llama_model.generate(inputs_embeds=[bos, prompt, img(197), prompt], num_beams=beam_size(3), do_sample=False,
                                min_new_tokens=80, max_new_tokens=120, repetition_penalty=2.0, length_penalty=2.0, ...)
`ReportDecoder` has HF Llama-2 / Qwen2 parameter names (`model.embed_tokens`, `model.layers.{i}.self_attn.{q,k,v,o}_proj`,
`mlp.{gate,up,down}_proj`, `input_layernorm`, `post_attention_layernorm`, `model.norm`, `lm_head`), so an HF
state_dict loads directly (absent q/k/v biases = 0, i.e. Llama).  Llama-3.x (`rope_scaling` of type "llama3") and Qwen3 (`head_dim`
apart from hidden_size / heads, `qk_norm`: `self_attn.q_norm` / `k_norm`) are constructor arguments.  Layers listed in `hybrid_layers` are
`Qwen2HybridDecoderLayer`s with the gated image cross-attention enabled (EMRRG installer,
MambaXrayVL_DownStream.py:176-208); `condition_vis_x` / `clear_vis_x` fan out to them.

`generate` restates the beam search of the transformers release installed next to the reference
(GenerationMixin._beam_search, vectorised top-K formulation): K = 2*num_beams candidates per step,
length-penalised finished-hypothesis pool, the early-stop heuristic of `early_stopping=False`,
RepetitionPenalty and MinNewTokens processors applied to log-probabilities, prompt given as embeddings (so the
penalties see generated tokens only).  The third-party implementation is not vendored in the reference ->
parity is pinned by token streams generated here with tiny random Llama configs (tests/golden/decode_*.npz).
KV cache: one (k, v) pair per layer, re-ordered by beam index after every step; the prompt is prefilled ONCE per
sample and its cache replicated over the beams (HF prefills batch*beams identical rows).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Iterable, Optional

import gc
import math

import torch
import torch.nn as nn

from . import _abi
from .hybrid_decoder_layer import Qwen2HybridDecoderLayer, Qwen2RMSNorm, Qwen2RotaryEmbedding
from .fp8_linear import Fp8Linear
from .int4_linear import Int4GroupLinear, check_gptq_config
from .int8_linear import Int8Linear
from .mxfp4_linear import MxFp4Linear
from .quant_linear import DequantScratch, QuantLinear
from .weight_formats import WEIGHT_FORMATS


# ---- kv_cache_dtype="fp8": the quantisation contract of the E4M3 KV cache (include/mxvl.h MXVL_KV_FP8), restated with torch ops ----
# Per layer and per tensor (K after RoPE, V) one power-of-two scale s = 2^j and OCP float8_e4m3fn codes:
#   j = ceil(log2(amax / 224)), amax over the whole prompt (224 = 448 / 2: a factor two for the generated positions), clamped so
#   that every code times s is exact in the cache's 16-bit dtype, 0 for amax = 0 or non-finite;
#   code = rne_e4m3(clamp(x / s, -448, 448));   x^ = float(code) * s   (exact in the model dtype: no second rounding).
# The caches below store and return x^ ("fake-quantised"), which makes the eager loop, the torch-module stepper and the CPU the
# oracle of the fp8 kernels, and the prompt prefill on a HIP device what those kernels continue.
KV_FP8_MAX, KV_FP8_TARGET = 448.0, 224.0
KV_FP8_EXP_RANGE = {torch.float16: (-15, 7)}      # every finite code x 2^j survives fp16 there; bf16 / fp32: (-100, 100)


def kv_fp8_scale(x):
    """The power-of-two scale of a tensor as a 0-dim fp32 tensor on its device (no host read)."""
    amax = x.detach().float().abs().amax()
    m, e = torch.frexp(amax)                     # amax = m * 2^e, m in [0.5, 1); 224 = 0.875 * 2^8: the ceil without a log
    j = e - 8 + (m > 0.875).to(e.dtype)
    lo, hi = KV_FP8_EXP_RANGE.get(x.dtype, (-100, 100))
    j = torch.where(torch.isfinite(amax) & (amax > 0), j, torch.zeros_like(j)).clamp(lo, hi)
    return torch.ldexp(torch.ones_like(amax), j)


def kv_fp8_encode(x, s):
    """E4M3 codes of x under scale s.  The clamp is explicit: torch's cast alone gives NaN above 448."""
    return (x.float() / s).clamp(-KV_FP8_MAX, KV_FP8_MAX).to(torch.float8_e4m3fn)


def kv_fp8_fake_quant(x, s):
    return (kv_fp8_encode(x, s).float() * s).to(x.dtype)


def _kv_mode(kv_dtype):
    if kv_dtype is None or (isinstance(kv_dtype, str) and kv_dtype in ("auto", "fp8")):
        return "fp8" if kv_dtype == "fp8" else None
    raise ValueError(f"`kv_cache_dtype` (={kv_dtype!r}) has to be None, \"auto\" (the model's 16-bit dtype) or \"fp8\"")


class KVCache:
    """Minimal per-layer key/value store with the `update` signature the attention module expects.
    kv_dtype="fp8": stores and returns fake-quantised values; a layer's scales are fixed by its first `update` (the prompt)."""

    def __init__(self, kv_dtype=None):
        self.k, self.v = {}, {}
        self.fp8 = _kv_mode(kv_dtype) == "fp8"
        self.scale = {}                  # fp8: layer -> (2,) fp32, the K and the V scale

    def get_seq_length(self, layer_idx=0):
        return 0 if layer_idx not in self.k else self.k[layer_idx].shape[-2]

    def update(self, k, v, layer_idx, cache_kwargs=None):
        if self.fp8:
            if layer_idx not in self.scale:
                self.scale[layer_idx] = torch.stack([kv_fp8_scale(k), kv_fp8_scale(v)])
            sk, sv = self.scale[layer_idx]
            k, v = kv_fp8_fake_quant(k, sk), kv_fp8_fake_quant(v, sv)
        if layer_idx in self.k:
            k = torch.cat([self.k[layer_idx], k], dim=-2)
            v = torch.cat([self.v[layer_idx], v], dim=-2)
        self.k[layer_idx], self.v[layer_idx] = k, v
        return k, v

    def reorder(self, beam_idx):
        for i in self.k:
            self.k[i] = self.k[i].index_select(0, beam_idx)
            self.v[i] = self.v[i].index_select(0, beam_idx)

    def expand(self, n):
        for i in self.k:
            self.k[i] = self.k[i].repeat_interleave(n, dim=0)
            self.v[i] = self.v[i].repeat_interleave(n, dim=0)


class StaticKVCache:
    """Pre-allocated (rows, Hkv, max_len, D) buffers per layer, written in place at `cache_position` -- fixed
    addresses and shapes, which is what lets one decode step be captured in a hipGraph and replayed.
    kv_dtype="fp8": fake-quantised like `KVCache`; the scales are the prompt's (`load_prefix`), held in one (n_layers, 2) tensor."""

    def __init__(self, n_layers, rows, kv_heads, max_len, head_dim, dtype, device, kv_dtype=None):
        self.fp8 = _kv_mode(kv_dtype) == "fp8"
        self.scale = torch.ones(n_layers, 2, dtype=torch.float32, device=device) if self.fp8 else None
        self.k = [torch.zeros(rows, kv_heads, max_len, head_dim, dtype=dtype, device=device) for _ in range(n_layers)]
        self.v = [torch.zeros(rows, kv_heads, max_len, head_dim, dtype=dtype, device=device) for _ in range(n_layers)]
        self.filled = 0

    def get_seq_length(self, layer_idx=0):
        return self.filled

    def load_prefix(self, dyn: "KVCache", repeat):
        for i in range(len(self.k)):
            n = dyn.k[i].shape[-2]
            self.k[i][:, :, :n] = dyn.k[i].repeat_interleave(repeat, dim=0)
            self.v[i][:, :, :n] = dyn.v[i].repeat_interleave(repeat, dim=0)
        if self.fp8:
            self.scale.copy_(torch.stack([dyn.scale[i] for i in range(len(self.k))]))
        self.filled = dyn.get_seq_length()

    def update(self, k, v, layer_idx, cache_kwargs=None):
        pos = cache_kwargs["cache_position"]
        if self.fp8:
            k, v = kv_fp8_fake_quant(k, self.scale[layer_idx, 0]), kv_fp8_fake_quant(v, self.scale[layer_idx, 1])
        self.k[layer_idx].index_copy_(2, pos, k)
        self.v[layer_idx].index_copy_(2, pos, v)
        return self.k[layer_idx], self.v[layer_idx]

    def reorder_(self, beam_idx):
        for i in range(len(self.k)):
            self.k[i].copy_(self.k[i].index_select(0, beam_idx))
            self.v[i].copy_(self.v[i].index_select(0, beam_idx))


class _Stepper:
    """What the two steppers share: the prompt-mask reset, the one hipGraph capture site, and step_search() -- decoder step +
    search update (`_SearchState.advance`) as ONE captured hipGraph per token; the host only reads the 1-byte `unfinished`
    flag between replays."""
    graph = None         # step(): the decoder step alone
    sgraph = None        # step_search(): the decoder step + the update of search state `sstate`
    sstate = None

    def _load_prompt_mask(self, prompt_mask):
        self.mask.zero_()
        self.mask[:, :self.P] = prompt_mask.repeat_interleave(self.mask.shape[0] // prompt_mask.shape[0], dim=0)
        self.n_real.copy_(self.mask[:, :self.P].sum(-1, keepdim=True))          # RoPE position of the first new token

    def _replay(self, slot, body, *args):
        """Replay the graph held in attribute `slot`.  Without one: run `body(*args)` eagerly (this is also the warm-up capture needs),
        then record the same body once; recording executes nothing, so the state (cache, mask, search state) is advanced
        exactly once per token.  Returns a clone of what the eager run returned (None on a replay)."""
        graph = getattr(self, slot)
        if graph is not None:
            graph.replay()
            return None
        out = body(*args)
        out = out if out is None else out.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # No cyclic garbage collection inside the capture: a dead model <-> stepper cycle (model._steppers / stepper.model) owns
        # CUDAGraphs, and destroying a graph is not a call a capturing stream allows -- the collector running at that moment aborts
        # the process.  torch.cuda.graph() used to collect on entry; torch 2.10 does so only under torch.compiler.config.force_cudagraph_gc,
        # so it is done here, and the collector stays off until the capture has ended.
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                body(*args)
        finally:
            if gc_was_on:
                gc.enable()
        setattr(self, slot, graph)
        return out

    def step_search(self, state):
        if self.sstate is not state:
            self.sgraph, self.sstate = None, state
        self._replay("sgraph", self._search_body, state)


class _GraphStepper(_Stepper):
    """One decode step (beam re-order of the cache + one-token forward) captured ONCE in a hipGraph and replayed per
    token: a 32-layer decoder is ~1400 kernel launches per token in eager mode -- launch-bound at batch 1-3."""

    def __init__(self, model: "ReportDecoder", rows, prompt_mask, dyn_cache, max_new, dtype, kv_dtype=None):
        dev = prompt_mask.device
        cfg = model.config
        self.model = model
        self.P = prompt_mask.shape[1]
        self.max_len = self.P + max_new
        self.cache = StaticKVCache(cfg.num_hidden_layers, rows, cfg.num_key_value_heads, self.max_len,
                                   cfg.head_dim, dtype, dev, kv_dtype)
        self.mask = torch.zeros(rows, self.max_len, dtype=torch.long, device=dev)
        self.n_real = torch.zeros(rows, 1, dtype=torch.long, device=dev)
        self.tok = torch.zeros(rows, dtype=torch.long, device=dev)
        self.beam = torch.arange(rows, device=dev)
        self.pos = torch.zeros(1, dtype=torch.long, device=dev)          # cache slot of the token being fed
        self.step_no = torch.zeros(1, dtype=torch.long, device=dev)
        self.logits = None
        self.dtype = dtype
        self.reset(prompt_mask, dyn_cache)

    def reset(self, prompt_mask, dyn_cache):
        self.cache.load_prefix(dyn_cache, self.mask.shape[0] // prompt_mask.shape[0])
        self._load_prompt_mask(prompt_mask)

    def _body(self):
        self.cache.reorder_(self.beam)
        self.mask.index_fill_(1, self.pos, 1)
        emb = self.model.model.embed_tokens(self.tok)[:, None, :].to(self.dtype)
        position_ids = self.n_real + self.step_no
        pos_emb = self.model.model.rotary_emb(emb, position_ids)
        h = emb
        for layer in self.model.model.layers:
            h = layer(h, attention_mask=self.mask, position_ids=position_ids, past_key_value=self.cache, use_cache=True,
                      cache_position=self.pos, position_embeddings=pos_emb)[0]
        return self.model.lm_head(self.model.model.norm(h))[:, -1]

    def _step_body(self):
        self.logits = self._body()          # (the recorded call leaves the graph's own output buffer here)
        return self.logits

    def _search_body(self, state):
        self.tok.copy_(state.tok)
        self.beam.copy_(state.beam_src)
        self.step_no.copy_((state.cur - 1).view(1))
        self.pos.copy_((state.cur + (self.P - 1)).view(1))
        state.advance(self._body())

    def step(self, tok, beam_idx, k):
        """k-th new token (k >= 0): feed `tok` (rows,), re-order the cache by `beam_idx`, return next logits."""
        self.tok.copy_(tok)
        self.beam.copy_(beam_idx)
        self.pos.fill_(self.P + k)
        self.step_no.fill_(k)
        out = self._replay("graph", self._step_body)
        return self.logits if out is None else out


def ngram_banned(hist, cur, n, vocab):
    """HF NoRepeatNGramLogitsProcessor as a static-shape mask.  hist (rows, L): the generated tokens of every row, [:, :cur] written;
    cur: the step index (0-dim int64 tensor); n = no_repeat_ngram_size > 0.  Returns (rows, vocab) bool: token w of a row is banned iff
    some window start i <= cur - n has hist[i : i+n-1] == hist[cur-n+1 : cur] and hist[i+n-1] == w -- nothing while cur + 1 < n (and
    nothing at cur + 1 == n: no window start exists yet); n == 1 bans every generated token.  One comparison per window position and
    per token of the n - 1 wide suffix, all rows at once: no host read of `cur`, so it runs inside a captured step."""
    rows, L = hist.shape
    W = L - n + 1                                                               # window starts that fit into the row
    banned = torch.zeros(rows, vocab + 1, dtype=torch.bool, device=hist.device)  # column `vocab` collects what is not banned
    if W <= 0:
        return banned[:, :vocab]
    ok = (torch.arange(W, device=hist.device) <= cur - n)[None, :].expand(rows, W)
    for j in range(n - 1):                                                      # token j of the window == token j of the current suffix
        suffix = hist.index_select(1, (cur - n + 1 + j).clamp(min=0).view(1))
        ok = ok & (hist[:, j:j + W] == suffix)
    follower = hist[:, n - 1:n - 1 + W]
    ok = ok & (follower >= 0) & (follower < vocab)                              # (a fill id outside the vocabulary has no score)
    banned.scatter_(1, torch.where(ok, follower, torch.full_like(follower, vocab)), True)
    return banned[:, :vocab]


class _SearchState:
    """One search (beam search, sampling) as ONE static-shape update per generated token -- the protocol the steppers and the token
    loop (`ReportDecoder._search`) drive: `advance(logits)` consumes the (rows, V) logits of step `cur` and leaves the next tokens in
    .tok, the parent row of every live row in .beam_src and whether decoding goes on in .unfinished.  Every tensor has a fixed shape
    and the step index `cur` is a device scalar, so the same code runs eagerly (CPU tests, torch restatement) and inside the captured
    hipGraph of the decode step.  A subclass adds its own tensors and supplies `_hip_supported`, `_advance_hip` (its kernel),
    `advance_torch` (the restatement the kernel is held against), `_serves` (for the error) and `result`."""
    nb = 1           # rows per sample: the token loop expands / re-orders the cache for a search that has more

    def __init__(self, rows, vocab, max_new, fill, eos, min_new, rep_pen, dev, no_repeat_ngram_size=0):
        self.V, self.max_new, self.fill, self.min_new, self.rep_pen = vocab, max_new, fill, min_new, rep_pen
        self.no_repeat = int(no_repeat_ngram_size)          # NoRepeatNGramLogitsProcessor, 0 = off
        self.use_hip = True      # tests flip this to compare the HIP kernel with the torch restatement
        self.allow_torch = False  # generate(use_graph="torch" / False) sets it: the torch restatement as an EXPLICIT request only
        self.eos_t = torch.tensor(eos, device=dev, dtype=torch.long)
        self.ar = torch.arange(max_new, device=dev)
        self.cur = torch.zeros((), dtype=torch.long, device=dev)
        self.tok = torch.zeros(rows, dtype=torch.long, device=dev)
        self.beam_src = torch.arange(rows, device=dev)                   # identity until a search re-orders its rows
        self.unfinished = torch.ones((), dtype=torch.bool, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)      # arrival word of the multi-workgroup kernels
        self.workspace = None
        # *unfinished of the step that ran at cur = c, at [c], where the HOST can read it (pinned, device-mapped): the look-ahead
        # token loop polls this instead of enqueueing a device-to-host copy between two replays (a 4 us copy kernel + a 5 us gap
        # per token in the round-4 timeline)
        self.unf_log = torch.zeros(max_new, dtype=torch.uint8).pin_memory() if torch.device(dev).type == "cuda" else None

    def reset(self):
        self.cur.zero_()
        self.unfinished.fill_(True)

    def advance(self, logits):
        if self.use_hip and logits.is_cuda:
            lg = logits if (logits.dtype == torch.float32 and logits.is_contiguous()) else logits.float().contiguous()
            if self._hip_supported(lg):
                return self._advance_hip(lg)
            if not self.allow_torch:
                # ONE search update on a HIP device, as for the decoder step: the kernel, or an error naming what it cannot serve
                what, served = self._serves()
                raise RuntimeError(f"{what} update on {logits.device}: {served}; pass use_graph=\"torch\" (or False) to generate() "
                                   f"for the torch restatement")
        return self.advance_torch(logits)


class _BeamState(_SearchState):
    """HF beam search (transformers generation/utils.py `_beam_search`, the vectorised form).
    Processors: RepetitionPenalty -> NoRepeatNGram -> MinNewTokensLength on the log-probabilities; criteria: MaxLength + EosToken."""

    def __init__(self, B, nb, vocab, max_new, fill, eos, min_new, rep_pen, len_pen, early_stopping, dev, no_repeat_ngram_size=0):
        super().__init__(B * nb, vocab, max_new, fill, eos, min_new, rep_pen, dev, no_repeat_ngram_size)
        self.B, self.nb, self.early = B, nb, early_stopping
        self.keep = max(2, 1 + len(eos)) * nb
        self.top_mask = torch.zeros(self.keep, dtype=torch.bool, device=dev)
        self.top_mask[:nb] = True
        self.row0 = torch.arange(B, device=dev)[:, None] * nb
        # (cur+1)**length_penalty and the early-stop heuristic's hypothesis length, as fp32 tables indexed by cur
        steps = torch.arange(1, max_new + 1, dtype=torch.float64)
        self.len_tab = steps.pow(len_pen).to(torch.float32).to(dev)
        hyp = torch.full_like(steps, float(max_new)) if (early_stopping == "never" and len_pen > 0.0) else steps
        self.hyp_tab = hyp.pow(len_pen).to(torch.float32).to(dev)
        self.run_seq = torch.empty(B, nb, max_new, dtype=torch.long, device=dev)
        self.fin_seq = torch.empty_like(self.run_seq)
        self.run_score = torch.empty(B, nb, device=dev)
        self.fin_score = torch.empty(B, nb, device=dev)
        self.fin_done = torch.empty(B, nb, dtype=torch.bool, device=dev)
        self.heur_open = torch.empty(B, 1, dtype=torch.bool, device=dev)
        self.split_vocab = True          # (tests switch it off to run the one-workgroup-per-sample sweeps)
        self.reset()

    def reset(self):
        self.run_seq.fill_(self.fill)
        self.fin_seq.fill_(self.fill)
        self.run_score.fill_(-1e9)
        self.run_score[:, 0] = 0.0
        self.fin_score.fill_(-1e9)
        self.fin_done.fill_(False)
        self.heur_open.fill_(True)
        super().reset()

    def _serves(self):
        return "beam-search", (f"csrc/beam_step.hip serves num_beams <= 8, <= 4 EOS ids and num_beams * vocab < 2^31 "
                               f"(got num_beams={self.nb}, eos ids={self.eos_t.numel()}, vocab={self.V})")

    def result(self):
        """The best finished hypothesis of every sample, trimmed to the longest returned one (HF trims by the recorded beam indices)."""
        out = self.fin_seq[:, 0].clone()
        lens = []
        for b in range(self.B):
            n = self.max_new
            if self.eos_t.numel():
                e = torch.isin(out[b], self.eos_t).nonzero()
                if len(e):
                    n = int(e[0]) + 1
            lens.append(n)
        return out[:, :max(lens)]

    def _hip_supported(self, logits):
        """What csrc/beam_step.hip serves: beams <= 8, keep <= 16, <= 4 EOS ids, beams * vocab < 2^31 -- any vocabulary size (the
        history bitmap is tiled since round 5: Qwen1.5's 151 936 tokens at beam 5 take the same kernels as Llama's 32 000)."""
        # LDS of the one-workgroup kernel: the old sequences; with an n-gram ban also its bitmap of a 32 768-word tile and the followers
        ban_lds = (4 * self.nb * ((min(self.V, 32768) + 31) // 32) + 4 * self.nb * self.max_new) if self.no_repeat else 0
        return (logits.is_cuda and self.nb <= 8 and self.keep <= 16 and self.eos_t.numel() <= 4 and self.nb * self.V < 2 ** 31
                and 16 * self.nb * self.max_new + ban_lds <= 128 * 1024 and logits.dtype == torch.float32 and logits.is_contiguous())

    def _advance_hip(self, logits):
        """csrc/beam_step.hip: the whole update below as one kernel (capturable in the decode step's hipGraph)."""
        lib = _abi.load()
        d = _abi.BeamDesc()
        d.batch, d.beams, d.vocab, d.max_new, d.min_new = self.B, self.nb, self.V, self.max_new, self.min_new
        d.n_eos, d.early_stopping, d.keep, d.repetition_penalty = self.eos_t.numel(), int(self.early is True), self.keep, self.rep_pen
        d.no_repeat_ngram_size = self.no_repeat
        d.logits, d.run_seq, d.fin_seq = logits.data_ptr(), self.run_seq.data_ptr(), self.fin_seq.data_ptr()
        d.run_score, d.fin_score, d.fin_done = self.run_score.data_ptr(), self.fin_score.data_ptr(), self.fin_done.data_ptr()
        d.heur_open, d.cur, d.eos = self.heur_open.data_ptr(), self.cur.data_ptr(), _abi.ptr(self.eos_t if self.eos_t.numel() else None)
        d.len_tab, d.hyp_tab = self.len_tab.data_ptr(), self.hyp_tab.data_ptr()
        d.tok, d.beam_src, d.unfinished = self.tok.data_ptr(), self.beam_src.data_ptr(), self.unfinished.data_ptr()
        d.scratch = self.ticket.data_ptr() if self.B > 1 else None        # one workgroup per sample
        d.unfinished_log = _abi.ptr(self.unf_log)
        if self.split_vocab:              # the vocabulary sweeps of a sample over 16 / 32 workgroups (csrc/beam_step.hip)
            if self.workspace is None:
                self.workspace = torch.empty(max(int(lib.mxvl_beam_workspace_bytes(self.B, self.nb, self.keep)), 4), dtype=torch.uint8, device=logits.device)
            d.workspace, d.workspace_bytes = self.workspace.data_ptr(), self.workspace.numel()
        _abi.launch("mxvl_beam_step", d, device=logits.device)

    def advance_torch(self, logits):
        B, nb, V, keep, cur = self.B, self.nb, self.V, self.keep, self.cur
        has_eos = self.eos_t.numel() > 0
        logp = torch.log_softmax(logits.float(), dim=-1)
        if self.rep_pen != 1.0:                                                 # RepetitionPenaltyLogitsProcessor
            flat = self.run_seq.view(B * nb, -1)
            idx = torch.where(self.ar[None, :] < cur, flat, flat[:, :1])        # unwritten slots alias token 0 of the row
            sc = torch.gather(logp, 1, idx)
            pen = torch.where(sc < 0, sc * self.rep_pen, sc / self.rep_pen)
            logp = logp.scatter(1, idx, torch.where(cur > 0, pen, sc))
        if self.no_repeat > 0:                                                  # NoRepeatNGramLogitsProcessor: after the penalty, a ban wins
            logp = logp.masked_fill(ngram_banned(self.run_seq.view(B * nb, -1), cur, self.no_repeat, V), -float("inf"))
        if has_eos and self.min_new > 0:                                        # MinNewTokensLengthLogitsProcessor
            col = logp.index_select(1, self.eos_t)
            logp.index_copy_(1, self.eos_t, torch.where(cur < self.min_new, torch.full_like(col, -float("inf")), col))
        acc = (logp.view(B, nb, V) + self.run_score[:, :, None]).view(B, nb * V)
        top_lp, top_ix = torch.topk(acc, k=keep)
        src_beam = top_ix // V
        new_tok = top_ix % V
        top_seq = torch.take_along_dim(self.run_seq, src_beam[:, :, None], dim=1)
        top_seq.scatter_(2, cur.view(1, 1, 1).expand(B, keep, 1), new_tok[:, :, None])
        hits = (cur + 1 >= self.max_new).expand(B, keep)                         # MaxLengthCriteria
        if has_eos:
            hits = hits | (new_tok[:, :, None] == self.eos_t).any(-1)            # EosTokenCriteria
        # live beams for the next step: best nb candidates that did not stop
        live_lp = top_lp + hits.float() * -1e9
        nxt = torch.topk(live_lp, k=nb)[1]
        run_seq = torch.take_along_dim(top_seq, nxt[:, :, None], dim=1)
        run_score = torch.take_along_dim(live_lp, nxt, dim=1)
        beam_src = torch.take_along_dim(src_beam, nxt, dim=1) + self.row0
        # finished pool: candidates among the top nb that just stopped, scored with the length penalty
        just = hits & self.top_mask[None, :]
        cand = top_lp / self.len_tab.index_select(0, cur.view(1))
        if self.early is True:
            cand = cand + self.fin_done.all(-1, keepdim=True).float() * -1e9
        cand = cand + (~self.heur_open).float() * -1e9 + (~just).float() * -1e9
        m_seq = torch.cat([self.fin_seq, top_seq], dim=1)
        m_score = torch.cat([self.fin_score, cand], dim=1)
        m_done = torch.cat([self.fin_done, just], dim=1)
        best = torch.topk(m_score, k=nb)[1]
        fin_seq = torch.take_along_dim(m_seq, best[:, :, None], dim=1)
        fin_score = torch.take_along_dim(m_score, best, dim=1)
        fin_done = torch.take_along_dim(m_done, best, dim=1)
        # early-stop heuristic of early_stopping=False: best live score at the CURRENT length vs worst finished
        best_live = run_score[:, :1] / self.hyp_tab.index_select(0, cur.view(1))
        worst_fin = torch.where(fin_done, fin_score.min(dim=1, keepdim=True)[0], torch.full_like(fin_score, -1e9))
        heur_open = self.heur_open & (best_live > worst_fin).any(dim=-1, keepdim=True)
        unfinished = heur_open.any() & ~hits.all()
        if self.early is True:
            unfinished = unfinished & ~fin_done.all()
        self.tok.copy_(torch.take_along_dim(new_tok, nxt, dim=1).reshape(-1))
        self.beam_src.copy_(beam_src.reshape(-1))
        self.run_seq.copy_(run_seq)
        self.run_score.copy_(run_score)
        self.fin_seq.copy_(fin_seq)
        self.fin_score.copy_(fin_score)
        self.fin_done.copy_(fin_done)
        self.heur_open.copy_(heur_open)
        self.unfinished.copy_(unfinished)
        self.cur.add_(1)


def sample_uniform(seed, rows, step, device="cpu"):
    """The uniform of the sampled decode for (seed, row, step): a 24-bit value in [0, 1), u = (hash >> 8) * 2^-24, a pure function
    of its arguments -- the host restatement of csrc/sample_step.hip sample_hash (the mixer of csrc/attn.hip attn_drop_hash, see
    flash_attention.dropout_keep_mask, over (low seed word, row, step, high seed word)) in int64 arithmetic.  `seed` and `step` are
    ints or int64 tensors (the state's device seed and step counter); returns (rows,) float64."""
    M = 0xFFFFFFFF
    seed = torch.as_tensor(seed, dtype=torch.int64, device=device).reshape(-1)[:1]
    step = torch.as_tensor(step, dtype=torch.int64, device=device).reshape(-1)[:1]
    row = torch.arange(rows, dtype=torch.int64, device=device)
    lo, hi = seed & M, (seed >> 32) & M
    x = lo ^ ((row * 0x9E3779B1) & M)
    x = ((x ^ ((step * 0x85EBCA77) & M)) * 0xC2B2AE3D) & M
    x = x ^ ((hi * 0x27D4EB2F) & M)
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & M
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & M
    x = x ^ (x >> 16)
    return (x >> 8).double() * 2.0 ** -24


class _SampleState(_SearchState):
    """HF `_sample` with do_sample=True (num_beams = 1): RepetitionPenalty -> NoRepeatNGram -> MinNewTokens -> Temperature -> TopK -> TopP on the fp32
    logits (HF's order, generation/utils.py `_get_logits_processor`), then an inverse-CDF draw in vocabulary order fed by
    `sample_uniform(seed, row, cur)`; the drawn tokens also land in .seq[:, cur].
    The seed lives in DEVICE memory and the step counter is the device scalar `cur`: a captured step replays with a fresh number per
    token and per call.  Top-p keeps token i iff the softmax mass of the strictly greater scores is < top_p: HF's rule with the ties
    at the cut kept together (HF's own outcome on ties follows an unstable sort; include/mxvl.h records the deviation)."""

    def __init__(self, B, vocab, max_new, fill, eos, min_new, rep_pen, temperature, top_k, top_p, dev, no_repeat_ngram_size=0):
        super().__init__(B, vocab, max_new, fill, eos, min_new, float(rep_pen), dev, no_repeat_ngram_size)
        self.B = B
        self.temperature, self.top_p = float(temperature), float(top_p)
        self.top_k = min(int(top_k), vocab) if top_k else 0           # 0 = off (HF: None or 0)
        # divisors as fp32 DEVICE scalars: torch divides by a host scalar on a HIP device as a multiplication by its reciprocal, which
        # is not the IEEE division HF's processors perform on the CPU (and csrc/sample_step.hip on the device)
        self.temp_t = torch.tensor(self.temperature, dtype=torch.float32, device=dev)
        self.pen_t = torch.tensor(self.rep_pen, dtype=torch.float32, device=dev)
        self.seq = torch.empty(B, max_new, dtype=torch.long, device=dev)
        self.alive = torch.empty(B, dtype=torch.bool, device=dev)
        self.seed = torch.zeros(1, dtype=torch.long, device=dev)        # device memory, never a kernel scalar
        self.out_thresh = torch.zeros(B, dtype=torch.float32, device=dev)   # smallest kept score / kept tokens of the last step
        self.out_kept = torch.zeros(B, dtype=torch.int32, device=dev)
        self.reset()

    def reset(self):
        self.seq.fill_(self.fill)
        self.alive.fill_(True)
        super().reset()

    def _serves(self):
        return "sampling", (f"csrc/sample_step.hip serves <= 80 rows, <= 4 EOS ids and rows * vocab < 2^31 "
                            f"(got rows={self.B}, eos ids={self.eos_t.numel()}, vocab={self.V})")

    def result(self):
        return self.seq[:, :int(self.cur)].clone()

    def _hip_supported(self, logits):
        """What csrc/sample_step.hip serves: <= 80 rows (the kernel stepper's bound), <= 4 EOS ids, rows * vocab < 2^31."""
        return (logits.is_cuda and self.B <= 80 and self.eos_t.numel() <= 4 and self.B * self.V < 2 ** 31
                and logits.dtype == torch.float32 and logits.is_contiguous())

    def _advance_hip(self, logits):
        """csrc/sample_step.hip: the whole update below as one kernel (capturable in the decode step's hipGraph)."""
        lib = _abi.load()
        if self.workspace is None:
            self.workspace = torch.empty(int(lib.mxvl_sample_workspace_bytes(self.B, self.V)), dtype=torch.uint8, device=logits.device)
        d = _abi.SampleDesc()
        d.rows, d.vocab, d.max_new, d.min_new, d.n_eos, d.top_k = self.B, self.V, self.max_new, self.min_new, self.eos_t.numel(), self.top_k
        d.repetition_penalty, d.temperature, d.top_p, d.fill = self.rep_pen, self.temperature, self.top_p, self.fill
        d.no_repeat_ngram_size = self.no_repeat
        d.logits, d.seq, d.alive, d.tok, d.cur = logits.data_ptr(), self.seq.data_ptr(), self.alive.data_ptr(), self.tok.data_ptr(), self.cur.data_ptr()
        d.eos, d.seed = _abi.ptr(self.eos_t if self.eos_t.numel() else None), self.seed.data_ptr()
        d.unfinished, d.unfinished_log, d.scratch = self.unfinished.data_ptr(), _abi.ptr(self.unf_log), self.ticket.data_ptr()
        d.workspace, d.workspace_bytes = self.workspace.data_ptr(), self.workspace.numel()
        d.out_thresh, d.out_kept = self.out_thresh.data_ptr(), self.out_kept.data_ptr()
        _abi.launch("mxvl_sample_step", d, device=logits.device)

    def scores_torch(self, logits):
        """Steps 1-5: the processed fp32 scores, the kept mask, the smallest kept score and the kept count of every row."""
        cur = self.cur
        sc = logits.float().clone()
        if self.rep_pen != 1.0:                                                 # RepetitionPenaltyLogitsProcessor, generated tokens only
            idx = torch.where(self.ar[None, :] < cur, self.seq, self.seq[:, :1])  # unwritten slots alias token 0 of the row
            g = torch.gather(sc, 1, idx)
            pen = torch.where(g < 0, g * self.pen_t, g / self.pen_t)
            sc = sc.scatter(1, idx, torch.where(cur > 0, pen, g))
        if self.no_repeat > 0:                                                  # NoRepeatNGramLogitsProcessor: after the penalty, a ban wins
            sc = sc.masked_fill(ngram_banned(self.seq, cur, self.no_repeat, self.V), -float("inf"))
        if self.eos_t.numel() > 0 and self.min_new > 0:                         # MinNewTokensLengthLogitsProcessor
            col = sc.index_select(1, self.eos_t)
            sc.index_copy_(1, self.eos_t, torch.where(cur < self.min_new, torch.full_like(col, -float("inf")), col))
        if self.temperature != 1.0:                                             # TemperatureLogitsWarper: a true fp32 division
            sc = sc / self.temp_t
        keep = torch.ones_like(sc, dtype=torch.bool)
        if self.top_k > 0:                                                      # TopKLogitsWarper: ties with the k-th value stay
            kth = torch.topk(sc, self.top_k)[0][:, -1:]
            keep = sc >= kth
        if self.top_p < 1.0:                                                    # TopPLogitsWarper, ties at the cut kept together
            vals = torch.sort(torch.where(keep, sc, torch.full_like(sc, -float("inf"))), dim=-1, descending=True)[0]
            p = torch.softmax(vals.double(), dim=-1)
            above = torch.cumsum(p, dim=-1) - p                                 # mass in front of every sorted position
            first = torch.ones_like(keep)
            first[:, 1:] = vals[:, 1:] != vals[:, :-1]
            s_gt = torch.cummax(torch.where(first, above, torch.full_like(above, -1.0)), dim=-1)[0]   # ... of the strictly greater scores
            cut = torch.where(s_gt < self.top_p, vals, torch.full_like(vals, float("inf"))).min(dim=-1, keepdim=True)[0]
            keep = keep & (sc >= cut)
        thresh = torch.where(keep, sc, torch.full_like(sc, float("inf"))).min(dim=-1)[0]
        return sc, keep, thresh, keep.sum(-1)

    def advance_torch(self, logits):
        B, cur = self.B, self.cur
        sc, keep, thresh, kept = self.scores_torch(logits)
        p = torch.softmax(torch.where(keep, sc, torch.full_like(sc, -float("inf"))), dim=-1)      # fp32, as HF's `probs`
        c = p.double().cumsum(-1)
        u = sample_uniform(self.seed, B, cur, device=logits.device)
        tok = (c <= (u[:, None] * c[:, -1:])).sum(-1)
        last = (keep * torch.arange(1, self.V + 1, device=logits.device)).max(-1)[0] - 1           # the last kept index
        tok = torch.minimum(tok, last)
        tok = torch.where(self.alive, tok, torch.full_like(tok, self.fill))
        self.seq.scatter_(1, cur.view(1, 1).expand(B, 1), tok[:, None])
        if self.eos_t.numel() > 0:
            self.alive.copy_(self.alive & ~torch.isin(tok, self.eos_t))
        self.tok.copy_(tok)
        self.out_thresh.copy_(thresh)
        self.out_kept.copy_(kept)
        self.cur.add_(1)
        self.unfinished.copy_(self.alive.any() & (self.cur < self.max_new))


class _KernelStepper(_Stepper):
    """One decode step on the hand-written HIP kernels (csrc/decode.hip): per layer a fused RMSNorm+QKV GEMV, the
    RoPE/cache-append/attention kernel, o_proj GEMV (+residual), fused RMSNorm + gate/up GEMV + SwiGLU, down GEMV
    (+residual); then RMSNorm + lm_head.  161 launches per token for 32 layers, captured once in a hipGraph.
    Beam re-ordering permutes a (rows, max_len) int32 slot table; cache lines never move.
    Hybrid layers conditioned on image tokens (`condition_vis_x`, "vanilla" cross-attention: every token attends,
    hybrid_decoder_layer.py:653-697) add one launch: the image K / V are projected once per generation and
    mxvl_decode_cross_attn adds the gated single-query attention to the self-attention output before o_proj."""

    @staticmethod
    def _cond_layers(model):
        return [i for i in model.hybrid_layers if model.model.layers[i].vis_x is not None]

    @staticmethod
    def cond_signature(model):
        """Shapes the captured graph depends on: part of the stepper cache key."""
        return tuple((i, tuple(model.model.layers[i].vis_x.shape), model.model.layers[i].cross_attn_mask is not None)
                     for i in _KernelStepper._cond_layers(model))

    @staticmethod
    def supported(model, rows, dtype, device, kv_dtype=None):
        if torch.device(device).type == "cuda":
            _abi.load()          # a missing libmxvl.so is an error on a GPU box, never a silent torch path
        cfg = model.config
        D = cfg.head_dim
        if _kv_mode(kv_dtype) == "fp8" and D == 256:
            return False         # the fp8-cache attention kernels (MXVL_KV_FP8) are built for head_dim 64 and 128
        for i in _KernelStepper._cond_layers(model):
            lay = model.model.layers[i]
            at = lay.self_attn
            # the decode step of the reference is only defined for the all-token ("vanilla") cross-attention with a
            # scalar gate projection; anything else stays on the module path (which raises where the reference does)
            if not (at.cross_attention_implementation.startswith("vanilla") and hasattr(at, "cross_attn_gate_proj")
                    and lay.media_locations is not None and lay.vis_x.dim() == 3 and rows % lay.vis_x.shape[0] == 0):
                return False
            # a gating type that names the warm-up gate without ending in it has no such parameter: the module path raises
            # there (as the reference does, hybrid_decoder_layer.py:631-640) -- the kernel path must not decode without the gate
            if "warmup" in at.gating_type and not hasattr(at, "cross_attn_warm_up_gate"):
                return False
        # rows <= 8: GEMV kernels with the activations of all rows in LDS; 9..80 rows (the reference's decode batches: 6 x 3,
        # 8 x 3, 16 x 3, 16 x 5 -- launch/*.sh, configs/config.py:11-12,50): MFMA projections (csrc/decode_gemm.h)
        # (rows <= 8 on the MFMA kernels as well wherever every K is a multiple of 64: no LDS bound on the activations there)
        HD = cfg.num_attention_heads * D          # o_proj's K (= hidden_size unless head_dim is given)
        mfma8 = cfg.hidden_size % 64 == 0 and cfg.intermediate_size % 64 == 0 and HD % 64 == 0 and cfg.hidden_size <= 16384
        fits = (mfma8 or rows * max(cfg.hidden_size, cfg.intermediate_size, HD) * 2 <= 150 * 1024) if rows <= 8 else \
            (rows <= 80 and min(cfg.hidden_size, cfg.intermediate_size, HD) >= 32 and cfg.hidden_size <= 16384)
        fmt = model.weight_format()
        if fmt is not None and any(k % fmt.K_MULTIPLE for k in (cfg.hidden_size, cfg.intermediate_size, HD)):
            return False         # a quantised format (WEIGHT_FORMATS) has one kernel: every projection width in whole K_MULTIPLE columns
        # bf16, or fp16 -- the dtype the reference loads its LLM in (MambaXrayVL_DownStream.py:72,85,92); csrc/decode_elt.h
        return (torch.device(device).type == "cuda" and dtype in (torch.bfloat16, torch.float16) and D in (64, 128, 256)
                and cfg.hidden_size % 8 == 0 and cfg.intermediate_size % 8 == 0 and fits)

    def __init__(self, model, rows, prompt_mask, dyn_cache, max_new, dtype, kv_dtype=None):
        dev = prompt_mask.device
        cfg = model.config
        self.model, self.rows = model, rows
        self.kv8 = _kv_mode(kv_dtype) == "fp8"
        self.H, self.Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
        self.D = cfg.head_dim
        self.qk_norm = bool(cfg.qk_norm)          # Qwen3: mxvl_decode_attn normalises the new q / k heads (MXVL_QK_NORM) -- in place in self.qkv
        self.hidden, self.inter, self.V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
        self.P = prompt_mask.shape[1]
        self.max_len = self.P + max_new
        model.fuse_qkv_()
        if model.lm_head.weight.dtype != dtype:
            raise RuntimeError(f"decode kernels: weights are {model.lm_head.weight.dtype}, activations {dtype}; cast the decoder first")
        self.dt = _abi.dtype_code(dtype)
        bf = dict(dtype=dtype, device=dev)
        L = cfg.num_hidden_layers
        # kv_cache_dtype="fp8": one byte per element (E4M3 codes, code 0 = 0.0) and the layers' (K, V) scales, refilled by reset()
        cbf = dict(dtype=torch.uint8, device=dev) if self.kv8 else bf
        self.kc = [torch.zeros(rows, self.Hkv, self.max_len, self.D, **cbf) for _ in range(L)]
        self.vc = [torch.zeros(rows, self.Hkv, self.max_len, self.D, **cbf) for _ in range(L)]
        self.kv_scale = torch.ones(L, 2, dtype=torch.float32, device=dev) if self.kv8 else None
        self.x = torch.zeros(rows, self.hidden, **bf)
        self.x2 = torch.zeros(rows, self.hidden, **bf)
        # rows > 8 need the matrix-core projections; below that they are still ~3 % faster per token than the GEMV kernels wherever
        # their LDS-DMA form applies (K % 64 == 0: every real decoder width) -- 5.2-6.2 TB/s against 4.4-5 of the weight stream
        self.batched = rows > 8 or (self.hidden % 64 == 0 and self.inter % 64 == 0 and (self.H * self.D) % 64 == 0)
        # layer projections in a quantised format (WEIGHT_FORMATS, ReportDecoder.quantize_): the matrix-core kernel at every row count with
        # the format's W_FLAG, explicit norm launches ("split" mode) -- there is no quantised form of the fused RMSNorm; lm_head and the
        # embedding stay 16-bit
        self.wfmt = model.weight_format()                # None or a class of WEIGHT_FORMATS
        self.quantised = self.wfmt is not None
        # rows <= 8: RMSNorm fused into the MFMA projection that consumes the rows (csrc/decode_gemm.h NORM, K % 64 == 0): no
        # mxvl_decode_rmsnorm launches (65 of a token's 229), o_proj / down_proj add their residual in their own epilogue instead of
        # splitting K.  Measured in one call (profiles/r05_decode_norm_ab.txt): batch 1 x beam 3 332.7 -> 361.1 tok/s, Qwen-1.8B 1 x 5
        # 755.7 -> 809.6; at 18 / 48 / 80 rows the unsplit o_proj / down_proj (256 workgroups of ONE 16-column tile: activation
        # re-reads = rows / 16 x the weight bytes) cost more than the launches save (1638 -> 1575, 2894 -> 2656, 2212 -> 1852
        # tok/s): those keep the K-split sums folded by an explicit norm launch ("split"; norm_mode is the A/B switch of bench.py)
        self.fused_norm = self.batched and not self.quantised and self.norm_mode == "fused" and rows <= 8 and self.hidden % 64 == 0 and self.hidden >= 256 \
            and self.inter % 64 == 0 and self.inter >= 256 and (self.H * self.D) % 64 == 0 and self.H * self.D >= 256
        # fp16 only (bf16 has fp32's exponent range): a power-of-two scale per RMSNorm gain, 2^-ceil(log2 max|g|), so that the fused
        # projection's dtype(g * s * x) can neither overflow nor sink into subnormals where the modules' dtype(dtype(x * rstd) * g) --
        # normalised in fp32 first -- would not (mxvl_gemv_desc.norm_gain_scale, ABI v9).  Keyed by the gain's storage and version;
        # taken once here, outside any graph capture (one host read for all gains)
        self._gain_scale = {}
        if self.fused_norm and dtype == torch.float16:
            norms = [ln.weight for layer in model.model.layers for ln in (layer.input_layernorm, layer.post_attention_layernorm)] + [model.model.norm.weight]
            with torch.no_grad():
                peaks = torch.stack([w.detach().float().abs().max() for w in norms]).cpu().tolist()
            for w, pk in zip(norms, peaks):
                self._gain_scale[(w.data_ptr(), w._version)] = 2.0 ** -math.ceil(math.log2(pk)) if (pk > 0.0 and math.isfinite(pk)) else 1.0
        self.xn = torch.zeros(rows, self.hidden, **bf) if self.batched else None      # RMSNorm output ahead of an MFMA projection
        # fp32 partial sums of the K-split o_proj / down_proj, one plane per split (written whole by the projection, added in a
        # fixed order by the folding norm: deterministic -- round 4 added into one plane with fp32 atomics)
        self.acc = torch.zeros(8, rows, self.hidden, dtype=torch.float32, device=dev) if self.batched else None
        self.qkv = torch.zeros(rows, (self.H + 2 * self.Hkv) * self.D, **bf)
        self.att = torch.zeros(rows, self.H * self.D, **bf)
        self.att2 = torch.zeros(rows, self.H * self.D, **bf)      # self-attention output + gated image context
        self.q_rope = torch.zeros(rows, self.H * self.D, **bf)    # rotated query of the current layer
        self.cond = {}                                            # layer -> image K / V, masks, gate flags (filled by reset)
        self.act = torch.zeros(rows, self.inter, **bf)
        self.logits = torch.zeros(rows, self.V, dtype=torch.float32, device=dev)
        self.cos = torch.zeros(rows, self.D, dtype=torch.float32, device=dev)
        self.sin = torch.zeros(rows, self.D, dtype=torch.float32, device=dev)
        self.slot = torch.zeros(rows, self.max_len, dtype=torch.int32, device=dev)
        self.own = torch.arange(rows, dtype=torch.int32, device=dev)[:, None]
        self.mask = torch.zeros(rows, self.max_len, dtype=torch.long, device=dev)
        self.n_real = torch.zeros(rows, 1, dtype=torch.long, device=dev)
        self.tok = torch.zeros(rows, dtype=torch.long, device=dev)
        self.beam = torch.arange(rows, device=dev)
        self.pos = torch.zeros(1, dtype=torch.long, device=dev)
        self.cur = torch.zeros(1, dtype=torch.long, device=dev)
        # RoPE rows of every position a generation can reach, from the model's own rotary module (so they are its bits)
        with torch.no_grad():
            ct, st = model.model.rotary_emb(self.cos, torch.arange(self.max_len + 1, device=dev)[None])
        self.cos_table, self.sin_table = ct[0].float().contiguous(), st[0].float().contiguous()
        self.reset(prompt_mask, dyn_cache)

    def reset(self, prompt_mask, dyn_cache):
        rep = self.rows // prompt_mask.shape[0]
        if self.kv8:
            if not getattr(dyn_cache, "fp8", False):
                raise RuntimeError("an fp8 KV cache continues a prompt cache built with kv_dtype=\"fp8\" (its values are on the grid already)")
            self.kv_scale.copy_(torch.stack([dyn_cache.scale[i] for i in range(len(self.kc))]))
        for i in range(len(self.kc)):
            n = dyn_cache.k[i].shape[-2]
            k, v = dyn_cache.k[i], dyn_cache.v[i]
            if self.kv8:             # on-grid values back to their codes: exact
                k = kv_fp8_encode(k, self.kv_scale[i, 0]).view(torch.uint8)
                v = kv_fp8_encode(v, self.kv_scale[i, 1]).view(torch.uint8)
            self.kc[i][:, :, :n] = k.repeat_interleave(rep, dim=0)
            self.vc[i][:, :, :n] = v.repeat_interleave(rep, dim=0)
        self._load_prompt_mask(prompt_mask)
        self.slot.copy_(self.own.expand(-1, self.max_len))
        # the beams of a sample continue the SAME prompt: their prompt positions name one physical copy (the sample's first row), so
        # the other beams' attention reads of it are L2 hits (same head -> same XCD) instead of HBM reads of identical bytes --
        # at 6 x 3 rows and a 230-token prompt that is half of the cache traffic of a step
        self.slot[:, :self.P] = (self.own // rep) * rep
        self.beams = rep
        self._project_image_tokens()

    @torch.no_grad()
    def _project_image_tokens(self):
        """K_img / V_img of every conditioned hybrid layer: `cross_attn_kv_proj(input_layernorm(vis_x))`, constant over the
        generation (hybrid_decoder_layer.py:1428, :683).  Written into persistent buffers so a captured graph stays valid."""
        for i in self._cond_layers(self.model):
            lay = self.model.model.layers[i]
            at = lay.self_attn
            k, v = at._vision_kv(lay.input_layernorm(lay.vis_x.to(self.x.dtype)))           # (Bv, Hkv, Lv, D) views
            km = lay.cross_attn_mask
            on = (lay.media_locations == 3).sum(dim=-1).bool()
            flags = _abi.GATE_TANH if any(isinstance(mod, nn.Tanh) for mod in at.cross_attn_gate_proj) else 0
            lin = at.cross_attn_gate_proj[0]
            c = self.cond.get(i)
            if c is None or c["k"].shape != k.shape:
                c = dict(k=torch.empty(k.shape, dtype=self.x.dtype, device=self.x.device),
                         v=torch.empty(v.shape, dtype=self.x.dtype, device=self.x.device),
                         km=None if km is None else torch.empty(km.shape, dtype=torch.uint8, device=self.x.device),
                         on=torch.empty(on.shape, dtype=torch.uint8, device=self.x.device))
                self.cond[i] = c
                self.graph = None                       # new buffers: a captured graph no longer describes this step
            c["k"].copy_(k)
            c["v"].copy_(v)
            if km is not None:
                c["km"].copy_(km.to(torch.uint8))
            c["on"].copy_(on.to(torch.uint8))
            c["flags"] = flags
            c["gate_w"], c["gate_b"] = lin.weight.reshape(-1), lin.bias
            c["warm"] = getattr(at, "cross_attn_warm_up_gate", None) if "warmup" in at.gating_type else None
            c["div"] = self.rows // k.shape[0]
        for i in [i for i in self.cond if i not in self._cond_layers(self.model)]:
            del self.cond[i]
            self.graph = None

    def _cross_attn(self, i):
        c = self.cond[i]
        d = _abi.DecodeCrossAttnDesc()
        d.rows, d.n_heads, d.n_kv_heads, d.head_dim, d.n_keys = self.rows, self.H, self.Hkv, self.D, c["k"].shape[2]
        d.kv_rows_div, d.gate_flags, d.scale, d.dtype = c["div"], c["flags"], self.D ** -0.5, self.dt
        d.q_rope, d.k, d.v = self.q_rope.data_ptr(), c["k"].data_ptr(), c["v"].data_ptr()
        d.key_mask, d.row_on = _abi.ptr(c["km"]), c["on"].data_ptr()
        d.text_state, d.out = self.att.data_ptr(), self.att2.data_ptr()
        d.gate_weight, d.gate_bias, d.warm_up_gate = c["gate_w"].data_ptr(), c["gate_b"].data_ptr(), _abi.ptr(c["warm"])
        _abi.launch("mxvl_decode_cross_attn", d, device=self.x.device)

    int8 = property(lambda self: self.wfmt is Int8Linear)
    mxfp4 = property(lambda self: self.wfmt is MxFp4Linear)
    fp8 = property(lambda self: self.wfmt is Fp8Linear)
    int4 = property(lambda self: self.wfmt is Int4GroupLinear)

    def _rmsnorm(self, x, norm, eps, K, fold_res=None, x_out=None, splits=1):
        """rows > 8: RMSNorm ahead of an MFMA projection (the GEMV kernel, rows <= 8, normalises in its own prologue).  With
        fold_res the row is first completed from the split projection's fp32 sums: x_out = bf16(acc) + fold_res; acc is cleared."""
        n = _abi.RmsNormDesc()
        n.rows, n.K, n.eps, n.dtype = self.rows, K, eps, self.dt
        n.x, n.weight, n.y = _abi.ptr(x), norm.data_ptr(), self.xn.data_ptr()
        if fold_res is not None:
            n.acc, n.residual, n.x_out, n.acc_splits = self.acc.data_ptr(), fold_res.data_ptr(), x_out.data_ptr(), splits
        _abi.launch("mxvl_decode_rmsnorm", n, device=self.x.device)
        return self.xn

    def _gemv(self, x, W, y, K, N, norm=None, eps=0.0, W2=None, bias=None, res=None, out_f32=False, split=0, scale=None, scale2=None):
        d = _abi.GemvDesc()
        d.rows, d.K, d.N, d.dtype = self.rows, K, N, self.dt
        if scale is not None:                   # W / W2 are the codes of a quantised format (WEIGHT_FORMATS), scale / scale2 its scales
            d.dtype |= self.wfmt.W_FLAG
            d.w_scale, d.w2_scale = scale.data_ptr(), _abi.ptr(scale2)
        d.swiglu, d.out_f32, d.eps = int(W2 is not None), int(out_f32), eps
        d.x, d.norm_weight, d.W = x.data_ptr(), _abi.ptr(norm), W.data_ptr()
        if norm is not None and self._gain_scale:
            d.norm_gain_scale = self._gain_scale.get((norm.data_ptr(), norm._version), 1.0)
        d.W2, d.bias, d.residual, d.y = _abi.ptr(W2), _abi.ptr(bias), _abi.ptr(res), _abi.ptr(y)
        if split:
            d.split_acc, d.k_splits = self.acc.data_ptr(), split
        elif self.batched:
            d.k_splits = 1
        _abi.launch("mxvl_decode_gemv", d, device=x.device)

    @staticmethod
    def _k_splits(N, K, rows=0):
        """Workgroups of 64 columns: split K until ~256 of them exist (o_proj / down_proj: N = hidden), a wave keeping >= 4 chunks of 64.
        (33..80 rows with 8 splits of 128-column workgroups -- two column tiles per wave on the wide kernel -- measured the same within
        noise: 2739 / 2719 vs 2756 / 2745 tok/s at 16 x 5, one call; not adopted.)"""
        s = max(1, min(8, 256 // max(1, -(-N // 64))))
        while s > 1 and K // 64 < 4 * 4 * s:
            s //= 2
        return s

    norm_mode = "fused"

    def _prologue(self, tok, beam, cur):
        """slot-table re-ordering, new position's slot / mask bit, token embeddings, RoPE rows: ONE launch (mxvl_decode_prologue)
        instead of 22 small torch kernels per token."""
        d = _abi.DecodePrologueDesc()
        d.rows, d.hidden, d.max_len, d.head_dim = self.rows, self.hidden, self.max_len, self.D
        d.prompt_len, d.table_len = self.P, self.cos_table.shape[0]
        d.tok, d.beam_src, d.cur, d.n_real = tok.data_ptr(), beam.data_ptr(), cur.data_ptr(), self.n_real.data_ptr()
        d.embed = self.model.model.embed_tokens.weight.data_ptr()
        d.cos_table, d.sin_table = self.cos_table.data_ptr(), self.sin_table.data_ptr()
        d.slot_table, d.mask, d.x = self.slot.data_ptr(), self.mask.data_ptr(), self.x.data_ptr()
        d.cos, d.sin, d.pos = self.cos.data_ptr(), self.sin.data_ptr(), self.pos.data_ptr()
        _abi.launch("mxvl_decode_prologue", d, device=self.x.device)

    def _beams_attn_fits(self):
        """what mxvl_decode_attn checks before it runs the beams of a sample in one workgroup (csrc/decode.hip): 32-bit cache offsets
        and the 4-wave shape's LDS (two K / V tile stages per wave + the rotated queries + the nb x max_len slot table) within 160 KB --
        a long table takes the workgroup-per-row kernel instead of an error"""
        nb, D, T = self.beams, self.D, self.max_len
        lds = 4 * 2 * (2 * 16 * D * 2) + 16 * D * 2 + 4 * (3 * nb * D + 2 * nb * 5 + nb * T)
        return self.rows * self.Hkv * T * D < 2 ** 31 and lds <= 160 * 1024

    def _body(self, tok, beam, cur):
        m = self.model
        self._prologue(tok, beam, cur)
        # Qwen3 (config.qk_norm): the descriptor heads the longer one that carries the layer's q_norm / k_norm gains
        aq = _abi.DecodeAttnQkNormDesc() if self.qk_norm else None
        a = aq.attn if self.qk_norm else _abi.DecodeAttnDesc()
        a.rows, a.n_heads, a.n_kv_heads, a.head_dim, a.max_len = self.rows, self.H, self.Hkv, self.D, self.max_len
        a.scale, a.dtype = self.D ** -0.5, self.dt | (_abi.MXVL_KV_FP8 if self.kv8 else 0) | (_abi.MXVL_QK_NORM if self.qk_norm else 0)
        # the beams of a sample share a workgroup (and the cache lines they have in common) once head x sample workgroups fill the
        # chip; below that a workgroup per (head, row) keeps more requests in flight (batch 1 x beam 3: 9 vs 15 us per layer)
        a.beams = self.beams if (2 <= self.beams <= 5 and self.H * (self.rows // self.beams) >= 128 and self._beams_attn_fits()) else 0
        a.qkv, a.cos, a.sin = self.qkv.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr()
        a.slot_table, a.pos, a.mask, a.out = self.slot.data_ptr(), self.pos.data_ptr(), self.mask.data_ptr(), self.att.data_ptr()
        batched = self.batched and not self.fused_norm   # MFMA projections with explicit RMSNorm launches; o_proj / down_proj split K and are folded by the next norm
        so, sd = (self._k_splits(self.hidden, self.H * self.D, self.rows), self._k_splits(self.hidden, self.inter, self.rows)) if batched else (0, 0)
        for i, layer in enumerate(m.model.layers):
            at = layer.self_attn
            ln1, ln2 = layer.input_layernorm, layer.post_attention_layernorm
            if batched:
                xin = self._rmsnorm(self.x, ln1.weight, ln1.variance_epsilon, self.hidden,
                                    fold_res=self.x2 if i else None, x_out=self.x, splits=sd)      # layer i - 1's down_proj sums + residual
                self._gemv(xin, at.qkv_weight, self.qkv, self.hidden, self.qkv.shape[1], bias=at.qkv_bias, scale=getattr(at, "qkv_scale", None))
            else:
                self._gemv(self.x, at.qkv_weight, self.qkv, self.hidden, self.qkv.shape[1], norm=ln1.weight, eps=ln1.variance_epsilon,
                           bias=at.qkv_bias)
            a.k_cache, a.v_cache = self.kc[i].data_ptr(), self.vc[i].data_ptr()
            a.kv_scale = self.kv_scale[i].data_ptr() if self.kv8 else None
            a.q_rope = self.q_rope.data_ptr() if i in self.cond else None
            if self.qk_norm:
                aq.q_norm_weight, aq.k_norm_weight, aq.qk_norm_eps = at.q_norm.weight.data_ptr(), at.k_norm.weight.data_ptr(), at.q_norm.variance_epsilon
            _abi.launch("mxvl_decode_attn", aq if self.qk_norm else a, device=self.x.device)
            att = self.att
            if i in self.cond:                       # gated image cross-attention on the rotated query, before o_proj
                self._cross_attn(i)
                att = self.att2
            if batched:
                self._gemv(att, _codes(at.o_proj), None, self.H * self.D, self.hidden, split=so, scale=_scales(at.o_proj))
                xin = self._rmsnorm(None, ln2.weight, ln2.variance_epsilon, self.hidden, fold_res=self.x, x_out=self.x2, splits=so)
                self._gemv(xin, _codes(layer.mlp.gate_proj), self.act, self.hidden, self.inter, W2=_codes(layer.mlp.up_proj),
                           scale=_scales(layer.mlp.gate_proj), scale2=_scales(layer.mlp.up_proj))
                self._gemv(self.act, _codes(layer.mlp.down_proj), None, self.inter, self.hidden, split=sd, scale=_scales(layer.mlp.down_proj))
            else:
                self._gemv(att, at.o_proj.weight, self.x2, self.H * self.D, self.hidden, res=self.x)
                self._gemv(self.x2, layer.mlp.gate_proj.weight, self.act, self.hidden, self.inter,
                           norm=ln2.weight, eps=ln2.variance_epsilon, W2=layer.mlp.up_proj.weight)
                self._gemv(self.act, layer.mlp.down_proj.weight, self.x, self.inter, self.hidden, res=self.x2)
        if batched:
            xin = self._rmsnorm(None, m.model.norm.weight, m.model.norm.variance_epsilon, self.hidden, fold_res=self.x2, x_out=self.x, splits=sd)
            self._gemv(xin, m.lm_head.weight, self.logits, self.hidden, self.V, out_f32=True)
        else:
            self._gemv(self.x, m.lm_head.weight, self.logits, self.hidden, self.V, norm=m.model.norm.weight,
                       eps=m.model.norm.variance_epsilon, out_f32=True)
        return self.logits

    def _search_body(self, state):
        state.advance(self._body(state.tok, state.beam_src, state.cur))      # the prologue kernel reads the search state's tensors itself

    def step(self, tok, beam_idx, k):
        self.tok.copy_(tok)
        self.beam.copy_(beam_idx)
        self.cur.fill_(k + 1)               # the prologue kernel derives the position and the RoPE step from it
        out = self._replay("graph", self._body, self.tok, self.beam, self.cur)
        return self.logits if out is None else out


def _codes(lin):
    """the weight bytes a decode projection reads: an nn.Linear's `weight`, a QuantLinear's codes"""
    return lin.codes if isinstance(lin, QuantLinear) else lin.weight


def _scales(lin):
    return lin.scales if isinstance(lin, QuantLinear) else None


class _Stack(nn.Module):
    def __init__(self, cfg, hybrid_layers, impl, gating):
        super().__init__()
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.layers = nn.ModuleList([
            Qwen2HybridDecoderLayer(cfg, i, is_hyper_enabled=(i in hybrid_layers), cross_attn_implementation=impl,
                                    cross_attn_gating_type=gating) for i in range(cfg.num_hidden_layers)])
        self.norm = Qwen2RMSNorm(cfg.hidden_size, eps=cfg.rms_norm_eps)
        self.rotary_emb = Qwen2RotaryEmbedding(config=cfg)


class ReportDecoder(nn.Module):
    _tuned_gemms_checked = False
    autocast_shadows = True        # forward_frozen_autocast keeps casted copies (bench.py --llm-shadows off: the A/B switch)

    def __init__(self, vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads,
                 num_key_value_heads=None, rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=4096,
                 hybrid_layers: Iterable[int] = (), cross_attn_implementation="vanilla",
                 cross_attn_gating_type="whole-dynamic-tanh-warmup", head_dim=None, qk_norm=False, rope_scaling=None):
        """head_dim: None = hidden_size // num_attention_heads (Llama, Qwen2); Qwen3 publishes 128 at every size.  qk_norm: Qwen3's
        per-head RMSNorm of q and k ahead of the rotation (`self_attn.q_norm` / `k_norm`).  rope_scaling: None or an HF dict
        (`rope_type` "default" / "llama3" with its four parameters); every other type raises NotImplementedError."""
        super().__init__()
        self.config = SimpleNamespace(
            vocab_size=vocab_size, hidden_size=hidden_size, intermediate_size=intermediate_size,
            num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
            num_key_value_heads=num_key_value_heads or num_attention_heads, rms_norm_eps=rms_norm_eps,
            rope_theta=rope_theta, max_position_embeddings=max_position_embeddings, attention_dropout=0.0,
            rope_scaling=None if rope_scaling is None else dict(rope_scaling), hidden_act="silu", _attn_implementation="sdpa",
            head_dim=int(head_dim) if head_dim is not None else hidden_size // num_attention_heads, qk_norm=bool(qk_norm))
        if head_dim is None and self.config.head_dim * num_attention_heads != hidden_size:
            raise ValueError(f"hidden_size must be divisible by num_heads (got `hidden_size`: {hidden_size} and `num_heads`: {num_attention_heads}).")
        self.hybrid_layers = tuple(hybrid_layers)
        self.model = _Stack(self.config, set(self.hybrid_layers), cross_attn_implementation, cross_attn_gating_type)
        self.lm_head = nn.Linear(hidden_size, vocab_size, bias=False)

    # ---- weights -------------------------------------------------------------------------------------------
    def load_hf_state_dict(self, sd):
        """HF LlamaForCausalLM / Qwen2ForCausalLM state_dict; Llama has no q/k/v biases -> zero them."""
        missing, unexpected = self.load_state_dict(sd, strict=False)
        with torch.no_grad():
            for name in missing:
                if name.endswith(("q_proj.bias", "k_proj.bias", "v_proj.bias")):
                    owner = self.get_submodule(name.rsplit(".", 1)[0])         # (a quantised projection keeps its bias as a buffer)
                    (self.get_buffer if isinstance(owner, QuantLinear) else self.get_parameter)(name).zero_()
        bad = [m for m in missing if not (m.endswith("_proj.bias") or "cross_attn" in m)]
        if bad or unexpected:
            raise RuntimeError(f"state_dict mismatch: missing {bad}, unexpected {list(unexpected)}")

    def fuse_qkv_(self):
        """Re-home q/k/v weights (and biases) of every layer in ONE (H+2Hkv)*D x hidden buffer; the nn.Linear
        parameters become views of it, so state_dict keys and the torch path are unchanged and no memory is added."""
        for layer in self.model.layers:
            at = layer.self_attn
            W = getattr(at, "qkv_weight", None)
            qkv = (at.q_proj, at.k_proj, at.v_proj)
            w0 = _codes(at.q_proj)
            if W is not None and W.data_ptr() == w0.data_ptr() and W.dtype == w0.dtype:
                continue        # still fused (a later .to(device/dtype) re-creates the parameters and un-fuses them)
            with torch.no_grad():
                W = torch.cat([_codes(lin) for lin in qkv], dim=0).contiguous()
                b = torch.cat([at.q_proj.bias, at.k_proj.bias, at.v_proj.bias], dim=0).contiguous()
                nq, nk = w0.shape[0], _codes(at.k_proj).shape[0]
                if isinstance(at.q_proj, QuantLinear):
                    # a quantised format (WEIGHT_FORMATS): the codes' rows and the per-row (per-block, per-group) scales concatenate exactly; the buffers become views of
                    # the fused ones (assigned, not .data: the unfused storage is released, no second copy of the bytes)
                    S = torch.cat([lin.scales for lin in qkv], dim=0).contiguous()
                    for lin, lo, hi in ((at.q_proj, 0, nq), (at.k_proj, nq, nq + nk), (at.v_proj, nq + nk, W.shape[0])):
                        lin.set_quantized(W[lo:hi], S[lo:hi]); lin.bias = b[lo:hi]
                    at.qkv_scale = S
                else:
                    at.q_proj.weight.data, at.k_proj.weight.data, at.v_proj.weight.data = W[:nq], W[nq:nq + nk], W[nq + nk:]
                    at.q_proj.bias.data, at.k_proj.bias.data, at.v_proj.bias.data = b[:nq], b[nq:nq + nk], b[nq + nk:]
                    at.qkv_scale = None
            at.qkv_weight, at.qkv_bias = W, b

    _INT8_TARGETS = (("self_attn", ("q_proj", "k_proj", "v_proj", "o_proj")), ("mlp", ("gate_proj", "up_proj", "down_proj")))

    def weight_format(self):
        """None (16-bit) or a class of WEIGHT_FORMATS: the class of the layer projections"""
        cls = type(self.model.layers[0].mlp.down_proj)
        return cls if issubclass(cls, QuantLinear) else None

    def _refuse_other_format(self, cls):
        """Formats do not mix on one decoder: a quantised decoder's 16-bit weights are gone, and codes are not re-quantised."""
        cur = self.weight_format()
        if cur is not None and cur is not cls:
            raise RuntimeError(f"quantize_{cls.NAME}_() on an {cur.NAME} decoder: quantise the 16-bit weights, not their {cur.NAME} codes")

    def _swap_projections(self, cls, make):
        """The one walk over the layer projections: each that is not a `cls` yet becomes make(lin, scratch).  Returns them all."""
        self._refuse_other_format(cls)
        scratch, done = DequantScratch(), []
        for layer in self.model.layers:
            at = layer.self_attn
            at.qkv_weight = at.qkv_bias = at.qkv_scale = None           # a fused 16-bit buffer would keep the old bytes alive
            for owner, names in self._INT8_TARGETS:
                mod = getattr(layer, owner)
                for name in names:
                    lin = getattr(mod, name)
                    if not isinstance(lin, cls):
                        lin = make(lin, scratch)
                        setattr(mod, name, lin)
                    scratch.reserve(lin.in_features * lin.out_features)        # the buffer is sized once, for the largest weight
                    done.append(lin)
        self.__dict__.pop("_steppers", None)                            # captured steps name the old weights
        self.__dict__.pop("_autocast_shadows", None)
        return done

    def quantize_(self, fmt):
        """`low_resource`: q/k/v/o_proj and gate/up/down_proj of every layer become WEIGHT_FORMATS[fmt] modules (the reference's
        load_in_8bit=True is int8: row-wise absmax, bitsandbytes' Int8Params storage) and their 16-bit storage is released; lm_head
        (HF's 8-bit loader skips it too), embed_tokens, the norms and the hybrid layers' cross-attention projections stay 16-bit.  The
        layers share one dequantisation scratch buffer for the multi-token paths; the decode step reads the codes directly.  A
        decoder in another quantised format is refused; what the format itself refuses -- an in_features that is no multiple of its
        block, an fp16 weight outside its exact range -- raises from its quantiser (<fmt>_linear.py)."""
        cls = WEIGHT_FORMATS[fmt]
        self._swap_projections(cls, cls.from_linear)
        return self

    def quantize_int8_(self):
        return self.quantize_(Int8Linear.NAME)

    def quantize_mxfp4_(self):
        return self.quantize_(MxFp4Linear.NAME)

    def quantize_fp8_(self):
        return self.quantize_(Fp8Linear.NAME)

    def quantize_int4_(self):
        return self.quantize_(Int4GroupLinear.NAME)

    def is_int8(self):
        return self.weight_format() is Int8Linear

    def is_mxfp4(self):
        return self.weight_format() is MxFp4Linear

    def is_fp8(self):
        return self.weight_format() is Fp8Linear

    def is_int4(self):
        return self.weight_format() is Int4GroupLinear

    def prepare_int4_(self, quantization_config=None):
        """Ahead of loading a GPTQ state dict: the projections quantize_ covers become EMPTY Int4GroupLinear modules (zero codes,
        their 16-bit weights are dropped unread) that repack `qweight` / `qzeros` / `scales` / `g_idx` on load, read by the
        checkpoint's `quantization_config` (checkpoint_format "gptq" when absent; bits != 4, group_size != 128 and desc_act raise a
        ValueError here).  lm_head, the embedding, the norms and the cross-attention projections stay 16-bit, as in the checkpoints."""
        self._refuse_other_format(Int4GroupLinear)
        check_gptq_config(quantization_config)
        qc = dict(quantization_config or {})
        for owner, names in self._INT8_TARGETS:                         # (before anything is swapped: a width the format refuses raises here)
            for name in names:
                Int4GroupLinear.buffers(1, getattr(getattr(self.model.layers[0], owner), name).in_features)

        def empty(lin, scratch):
            w = lin.weight
            return Int4GroupLinear(lin.in_features, lin.out_features, bias=lin.bias is not None, dtype=w.dtype, device=w.device, scratch=scratch)
        for lin in self._swap_projections(Int4GroupLinear, empty):
            lin.gptq_config = qc
        return self

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def condition_vis_x(self, vis_x, cross_attn_mask=None, token_type=None):
        for i in self.hybrid_layers:
            self.model.layers[i].condition_vis_x(vis_x, cross_attn_mask, token_type)

    def clear_vis_x(self):
        for i in self.hybrid_layers:
            self.model.layers[i].clear_vis_x()

    # ---- forward -------------------------------------------------------------------------------------------
    def forward(self, inputs_embeds, attention_mask=None, position_ids=None, past_key_values: Optional[KVCache] = None):
        """inputs_embeds (B, T, hidden); attention_mask (B, past+T) 1 = real token.  Returns logits (B, T, vocab)."""
        B, T, _ = inputs_embeds.shape
        past = past_key_values.get_seq_length() if past_key_values is not None else 0
        if position_ids is None:
            if attention_mask is not None:   # HF: positions count real tokens (left padding gets position 0..)
                position_ids = (attention_mask.long().cumsum(-1) - 1).clamp(min=0)[:, past:past + T]
            else:
                position_ids = torch.arange(past, past + T, device=inputs_embeds.device)[None].expand(B, -1)
        pos_emb = self.model.rotary_emb(inputs_embeds, position_ids)
        h = inputs_embeds
        for layer in self.model.layers:
            h = layer(h, attention_mask=attention_mask, position_ids=position_ids, past_key_value=past_key_values,
                      use_cache=past_key_values is not None, position_embeddings=pos_emb)[0]
        return self.lm_head(self.model.norm(h))

    def forward_frozen_autocast(self, inputs_embeds, attention_mask=None, position_ids=None):
        """forward() for a FROZEN decoder under an autocast context whose dtype is not the weights' -- the reference's stage-3 / R2GenCSR
        training step: an LLM loaded with torch_dtype=torch.float16 (MambaXrayVL_DownStream.py:72-92, R2GenCSR.py) under Lightning's
        bf16-mixed precision (configs/config.py:67).  autocast re-casts every nn.Linear weight on every call (13 GB read + 13 GB written
        per forward of a 7B model; its cast cache only covers parameters that require grad); here ONE casted copy of every projection
        matrix is kept (refreshed when a weight's storage or version changes) and the call runs on those copies through
        torch.func.functional_call -- the same values autocast would produce, the same kernels, no per-step cast traffic.  The copies
        cost the weights' size in HBM once (13.5 GB for Llama-2-7B)."""
        dev_type = inputs_embeds.device.type
        if not torch.is_autocast_enabled(dev_type) or not ReportDecoder.autocast_shadows:
            self.free_autocast_shadows()       # autocast off (or the switch): nothing reads the copies
            return self.forward(inputs_embeds, attention_mask=attention_mask, position_ids=position_ids)
        dt = torch.get_autocast_dtype(dev_type)
        cache = self.__dict__.setdefault("_autocast_shadows", {})
        shadows = {}
        for name, w in self.named_parameters():
            if w.requires_grad or w.dim() != 2 or w.dtype == dt or "embed_tokens" in name or not w.is_floating_point():
                cache.pop(name, None)          # unfrozen / re-typed since the copy was made: the copy (2 bytes per weight) is released
                continue
            key = (w._version, w.data_ptr(), w.dtype, dt, w.device)
            hit = cache.get(name)
            if hit is None or hit[0] != key:
                hit = (key, w.detach().to(dt))
                cache[name] = hit
            shadows[name] = hit[1]
        for name in [n for n in cache if n not in shadows]:
            del cache[name]
        if not shadows:
            return self.forward(inputs_embeds, attention_mask=attention_mask, position_ids=position_ids)
        return torch.func.functional_call(self, shadows, (inputs_embeds,), dict(attention_mask=attention_mask, position_ids=position_ids))

    def free_autocast_shadows(self) -> int:
        """Release the casted weight copies of forward_frozen_autocast (13.5 GB for a 7B decoder); the next call under autocast makes
        them again.  Returns the bytes released.  (The copies are also dropped, per weight, as soon as a call finds the weight
        unfrozen, re-typed, moved or re-allocated, and all of them when a call runs outside autocast.)"""
        cache = self.__dict__.pop("_autocast_shadows", None) or {}
        return sum(t.numel() * t.element_size() for _, t in cache.values())

    # ---- generation ------------------------------------------------------------------------------------------
    def _greedy(self, logits, cache, attn, dtype, eos_t, fill, min_new, max_new, rep_pen, stepper=None, no_repeat=0):
        """num_beams = 1 (HF `_sample` with do_sample=False): the processors act on the raw LOGITS here (on
        log-probabilities in beam search), finished rows keep emitting the pad token."""
        B, dev = logits.shape[0], logits.device
        seq = torch.empty(B, 0, dtype=torch.long, device=dev)
        alive = torch.ones(B, dtype=torch.bool, device=dev)
        has_eos = eos_t.numel() > 0
        while True:
            sc = logits.float().clone()
            if rep_pen != 1.0 and seq.shape[1] > 0:
                g = torch.gather(sc, 1, seq)
                sc = sc.scatter(1, seq, torch.where(g < 0, g * rep_pen, g / rep_pen))
            if no_repeat > 0:                                                   # NoRepeatNGramLogitsProcessor (pad tokens of stopped rows count, as in HF)
                sc = sc.masked_fill(ngram_banned(seq, torch.tensor(seq.shape[1], device=dev), no_repeat, sc.shape[1]), -float("inf"))
            if has_eos and seq.shape[1] < min_new:
                sc[:, eos_t] = -float("inf")
            tok = sc.argmax(-1)
            if has_eos:
                tok = torch.where(alive, tok, torch.full_like(tok, fill))
            seq = torch.cat([seq, tok[:, None]], dim=1)
            if has_eos:
                alive = alive & ~torch.isin(tok, eos_t)
            if seq.shape[1] >= max_new or not bool(alive.any()):
                return seq
            if stepper is not None:
                logits = stepper.step(tok, torch.arange(B, device=dev), seq.shape[1] - 1)
                continue
            attn = torch.cat([attn, torch.ones(B, 1, dtype=attn.dtype, device=dev)], dim=1)
            emb = self.model.embed_tokens(tok)[:, None, :].to(dtype)
            logits = self.forward(emb, attention_mask=attn, past_key_values=cache)[:, -1]

    def _search_state(self, store, cls, *args):
        """The search state of an argument set (the cache key), built once -- its tensors, workspace and pinned log keep their
        addresses, so a captured step stays valid over calls -- and reset for every call."""
        states = self.__dict__.setdefault(store, {})
        state = states.get(args)
        if state is None:
            state = states[args] = cls(*args)
        else:
            state.reset()
        return state

    def _search(self, state, logits, cache, attn, dtype, stepper, use_graph):
        """The token loop of every `_SearchState`: with a stepper, decoder step + search update in ONE hipGraph replay per token and
        no host round trip (`_search_lookahead`); without one, the eager forward on the dynamic cache.  `logits` (B, V): the prefill's."""
        nb = state.nb
        if nb > 1:
            logits = logits.repeat_interleave(nb, dim=0)
        state.allow_torch = use_graph == "torch" or use_graph is False
        state.advance(logits)                                    # step 0: the prefill logits
        if stepper is None and nb > 1:
            cache.expand(nb)
            attn = attn.repeat_interleave(nb, dim=0)
        if isinstance(stepper, _KernelStepper) and state.use_hip and state._hip_supported(stepper.logits):
            self._search_lookahead(stepper, state)
        while bool(state.unfinished):
            if stepper is not None:
                stepper.step_search(state)                       # decoder step + search update, one hipGraph replay
                continue
            if nb > 1:
                cache.reorder(state.beam_src)
            attn = torch.cat([attn, torch.ones(attn.shape[0], 1, dtype=attn.dtype, device=attn.device)], dim=1)
            emb = self.model.embed_tokens(state.tok)[:, None, :].to(dtype)
            state.advance(self.forward(emb, attention_mask=attn, past_key_values=cache)[:, -1])
        return state.result()

    def _sample(self, seed, state_args, *loop_args):
        """num_beams = 1, do_sample=True (HF `_sample`): a `_SampleState` on the token loop of the beam path."""
        if seed is None:
            # a generator of the decoder's own (seeded once from torch's initial seed): a call must not shift the global CPU stream
            # that samplers and augmentation draw from
            gen = self.__dict__.get("_sample_gen")
            if gen is None:
                gen = self.__dict__["_sample_gen"] = torch.Generator().manual_seed(torch.initial_seed() & (2 ** 63 - 1))
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=gen, dtype=torch.int64))
        state = self._search_state("_sample_states", _SampleState, *state_args)
        state.seed.copy_(torch.tensor([seed & (2 ** 63 - 1)], dtype=torch.long))       # device memory: never baked into a capture
        return self._search(state, *loop_args)

    @staticmethod
    def _search_lookahead(stepper, state):
        """Token loop without a host round trip per token: replay k + 1 is enqueued BEFORE the host has seen `unfinished` of replay k
        (the beam kernel leaves it in pinned memory).  If k was the last token, replay k + 1 is a no-op for the search state -- mxvl_beam_step
        returns at once when *unfinished is already 0 -- so the result is what the synchronous loop returns; the ~45 us the
        device idled per token while the host read one byte are gone."""
        if not bool(state.unfinished):
            return
        if getattr(state, "_look", None) is None:          # events live with the (cached) search state
            state._look = [torch.cuda.Event() for _ in range(2)]
        events, log = state._look, state.unf_log.numpy()   # the kernel stores the flag of the step at cur = c in log[c] (pinned)
        c = int(state.cur)                                 # one read per report; from here the host counts the steps itself
        stepper.step_search(state)                         # (the first call runs eagerly and captures the graph)
        k = 0
        events[0].record()
        while True:
            stepper.step_search(state)                     # speculative: a no-op if the previous step finished the search
            events[1 - k].record()
            events[k].synchronize()
            if not log[c]:
                break
            c += 1
            k = 1 - k
        torch.cuda.current_stream().synchronize()

    @torch.no_grad()
    def generate(self, inputs_embeds, *args, **kwargs):
        """Greedy (num_beams=1) / beam search / sampling (num_beams=1, do_sample=True with temperature, top_k, top_p, seed) over a
        prompt given as embeddings.  Returns (B, <= max_new_tokens) ids.
        no_repeat_ngram_size = n > 0 (HF's keyword; 0 = off): no n-gram of generated tokens occurs twice in a row's output, in all
        three modes; on a HIP device the ban is part of the beam / sampling kernel of the captured step.
        use_graph (default: on for HIP devices): static KV cache + one hipGraph replay per generated token.
        A decoder held in a 16-bit dtype decodes IN that dtype, prompt prefill included: an enclosing autocast context (the
        reference's validation_step runs under Lightning's bf16-mixed one, configs/config.py:67, around an LLM loaded with
        torch_dtype=torch.float16, MambaXrayVL_DownStream.py:72-92) is suspended for the call -- the decode kernels never see it,
        and a prefill that autocast re-cast per nn.Linear would fill the KV cache in another dtype than the steps that extend it."""
        wdt = self.lm_head.weight.dtype
        if wdt in (torch.bfloat16, torch.float16):
            with torch.autocast(device_type=inputs_embeds.device.type, enabled=False):
                return self._generate(inputs_embeds.to(wdt), *args, **kwargs)
        return self._generate(inputs_embeds, *args, **kwargs)

    def _generate(self, inputs_embeds, attention_mask=None, num_beams=1, do_sample=False, min_new_tokens=0,
                  max_new_tokens=20, repetition_penalty=1.0, length_penalty=1.0, eos_token_id=None, pad_token_id=None,
                  early_stopping=False, temperature=None, use_graph=None, top_k=None, top_p=1.0, seed=None, no_repeat_ngram_size=0,
                  kv_cache_dtype=None):
        kv_dtype = _kv_mode(kv_cache_dtype)          # None / "auto": the model's dtype; "fp8": E4M3.  Checked before anything is enqueued
        # HF: a strictly positive integer or unset; 0 (the default here) switches the processor off.  Checked before anything is enqueued
        if isinstance(no_repeat_ngram_size, bool) or not isinstance(no_repeat_ngram_size, int) or no_repeat_ngram_size < 0:
            raise ValueError(f"`no_repeat_ngram_size` (={no_repeat_ngram_size}) has to be a non-negative integer (0 = off)")
        if do_sample:
            # HF validates these before it generates (GenerationConfig.validate, the warpers' constructors): so do we, before
            # anything is enqueued.  With do_sample=False they stay ignored (the reference's default --temperature 0 keeps working)
            if num_beams != 1:
                raise NotImplementedError("beam-sample (num_beams > 1 with do_sample=True) is not built: sample with num_beams=1")
            temperature = 1.0 if temperature is None else temperature
            if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not (0.0 < float(temperature) < float("inf")):
                raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive finite float with do_sample=True")
            top_p = 1.0 if top_p is None else top_p
            if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not (0.0 < float(top_p) <= 1.0):
                raise ValueError(f"`top_p` (={top_p}) has to be a float > 0 and <= 1")
            if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0):
                raise ValueError(f"`top_k` (={top_k}) has to be a non-negative integer or None")
            if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
                raise ValueError(f"`seed` (={seed}) has to be an integer or None")
        dev = inputs_embeds.device
        B = inputs_embeds.shape[0]
        nb = num_beams
        eos = [] if eos_token_id is None else ([eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id))
        eos_t = torch.tensor(eos, device=dev, dtype=torch.long)
        # beam search pads with `pad_token_id or eos[0]` in HF (a falsy pad id 0 falls through to EOS); greedy pads with pad
        fill = (pad_token_id or (eos[0] if eos else -1)) if nb > 1 else (pad_token_id if pad_token_id is not None else (eos[0] if eos else -1))
        if attention_mask is None:
            attention_mask = torch.ones(inputs_embeds.shape[:2], dtype=torch.long, device=dev)

        if inputs_embeds.is_cuda and not ReportDecoder._tuned_gemms_checked:
            # the prompt prefill is library GEMMs (M = batch x prompt tokens): use the per-shape solutions picked offline on an
            # MI355X (tuned/tunableop_gfx950.csv, read-only; e.g. gate / up at 6 x 230 tokens run in three tile rounds by default)
            from .pretrain_engine import enable_tuned_gemms
            ReportDecoder._tuned_gemms_checked = True
            enable_tuned_gemms()
        cache = KVCache(kv_dtype)
        logits = self.forward(inputs_embeds, attention_mask=attention_mask, past_key_values=cache)[:, -1]   # (B, V)
        if use_graph is None:
            use_graph = inputs_embeds.is_cuda
        stepper = None
        if use_graph:
            # the captured graph is reused by later calls with the same shapes (capture costs ~a hundred ms for 32 layers)
            # A captured graph bakes in weight addresses and the (un)conditioned layer structure: a later .to()/.half()
            # (new parameter storage) or condition_vis_x() must not replay it.  The weight identity is part of the cache
            # (stale steppers are dropped), the conditioning state is part of the key.
            conditioned = any(self.model.layers[i].vis_x is not None for i in self.hybrid_layers)
            last = self.model.layers[-1].mlp.down_proj
            ident = tuple((w.data_ptr(), w.dtype) for w in (self.lm_head.weight, self.model.embed_tokens.weight,
                                                            _codes(last)))
            if self.__dict__.get("_stepper_weights") != ident:
                self.__dict__["_steppers"] = {}
                self.__dict__["_stepper_weights"] = ident
            key = (B * nb, nb, attention_mask.shape[1], max_new_tokens, inputs_embeds.dtype, str(dev), str(use_graph), conditioned,
                   _KernelStepper.cond_signature(self), kv_dtype)
            stepper = getattr(self, "_steppers", {}).get(key)
            if stepper is None:
                cls = _GraphStepper
                if use_graph != "torch":
                    # ONE decode path on a HIP device: the kernels, or an error naming what they cannot serve -- the torch-module
                    # stepper is an explicit request (use_graph="torch": CPU-parity experiments), never a silent substitute
                    if not _KernelStepper.supported(self, B * nb, inputs_embeds.dtype, dev, kv_dtype):
                        raise RuntimeError(
                            f"report decoding on {dev}: the HIP decode kernels serve bf16 / fp16 models with head_dim 64/128/256 "
                            f"(64/128 with kv_cache_dtype=\"fp8\") and "
                            f"batch * beams <= 80 (got rows={B * nb}, dtype={inputs_embeds.dtype}, head_dim="
                            f"{self.config.head_dim}, kv_cache_dtype={kv_cache_dtype!r}); pass use_graph=\"torch\" for the "
                            f"torch-module stepper or use_graph=False for the eager loop")
                    cls = _KernelStepper
                stepper = cls(self, B * nb, attention_mask, cache, max_new_tokens, inputs_embeds.dtype, kv_dtype)
                self.__dict__.setdefault("_steppers", {})[key] = stepper
            else:
                stepper.reset(attention_mask, cache)
        if nb == 1 and not do_sample:
            return self._greedy(logits, cache, attention_mask, inputs_embeds.dtype, eos_t, fill, min_new_tokens,
                                max_new_tokens, repetition_penalty, stepper, no_repeat_ngram_size)
        vocab = logits.shape[-1]
        loop_args = (logits, cache, attention_mask, inputs_embeds.dtype, stepper, use_graph)
        if do_sample:
            return self._sample(seed, (B, vocab, max_new_tokens, fill, tuple(eos), min_new_tokens, repetition_penalty, float(temperature),
                                       top_k or 0, float(top_p), str(dev), no_repeat_ngram_size), *loop_args)
        state = self._search_state("_beam_states", _BeamState, B, nb, vocab, max_new_tokens, fill, tuple(eos), min_new_tokens,
                                   repetition_penalty, length_penalty, early_stopping, str(dev), no_repeat_ngram_size)
        return self._search(state, *loop_args)
