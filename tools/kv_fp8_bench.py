"""Dev tool: report decoding with an E4M3 KV cache (ReportDecoder.generate(kv_cache_dtype="fp8"), mxvl_decode_attn with MXVL_KV_FP8)
against the 16-bit cache, on the same model.

    python tools/kv_fp8_bench.py [--out profiles/kv_fp8_bench.txt] [--new 128] [--weights w16,mxfp4]

One process, one box: the two cache formats are two steppers of ONE decoder and their generate() calls alternate.  Shape:
decode_llama7b_128 at batch x beams 1 x 3, 6 x 3 and 16 x 5, with 16-bit weights and with low_resource="mxfp4" weights
(ReportDecoder.quantize_mxfp4_).  One JSON line per leg, printed and appended to --out:
  tok_per_s         median of 3 alternating repeats after the capturing call, both arms, and their ratio;
  first_step_dev    the first decode step on the kernel stepper (same prompt, same token fed): max |logits_fp8 - logits_16| over the
                    row's max |logits_16|, worst row;
  greedy_agree      of the first 64 greedy tokens (num_beams = 1 at the leg's batch): equal positions and the common prefix, per-row mean;
  kv_bytes          bytes of the steppers' K / V caches."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from medical_image_analysis_amd.report_decoder import KVCache, ReportDecoder, _KernelStepper  # noqa: E402

dev = "cuda:0"
ARMS = {"kv16": None, "fp8": "fp8"}


@torch.no_grad()
def first_step_logits(m, emb, rows, kv):
    """Prefill into a cache of the arm's format, then ONE step of the kernel stepper (eager, no graph) on the 16-bit arm's first token."""
    B, P = emb.shape[:2]
    mask = torch.ones(B, P, dtype=torch.long, device=dev)
    tok16 = m.forward(emb, attention_mask=mask, past_key_values=KVCache())[:, -1].argmax(-1)
    cache = KVCache(kv)
    m.forward(emb, attention_mask=mask, past_key_values=cache)
    st = _KernelStepper(m, rows, mask, cache, 8, emb.dtype, kv)
    tok = tok16.repeat_interleave(rows // B)
    return st._body(tok, torch.arange(rows, device=dev), torch.ones(1, dtype=torch.long, device=dev)).float().clone()


def bench_leg(m, weights, B, nb, plen, hidden, new):
    emb = (0.02 * torch.randn(B, plen, hidden, generator=torch.Generator().manual_seed(1000))).to(dev, torch.bfloat16)
    kw = dict(num_beams=nb, min_new_tokens=new, max_new_tokens=new, repetition_penalty=2.0, length_penalty=2.0, eos_token_id=2, pad_token_id=0)
    times = {k: [] for k in ARMS}
    for k, kv in ARMS.items():
        m.generate(emb, kv_cache_dtype=kv, **kw)                 # prefill + capture
    for _ in range(3):                                           # alternating rounds
        for k, kv in ARMS.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.generate(emb, kv_cache_dtype=kv, **kw)
            torch.cuda.synchronize()
            times[k].append(B * out.shape[1] / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in times.items()}
    kv_bytes = {("fp8" if s.kv8 else "kv16"): sum(t.numel() * t.element_size() for t in s.kc + s.vc)
                for s in m._steppers.values() if isinstance(s, _KernelStepper)}
    m.__dict__.pop("_steppers", None)
    l16, l8 = (first_step_logits(m, emb, B * nb, kv) for kv in ARMS.values())
    dev_rows = (l8 - l16).abs().amax(-1) / l16.abs().amax(-1)
    gkw = dict(num_beams=1, min_new_tokens=64, max_new_tokens=64, eos_token_id=2, pad_token_id=0)
    g16, g8 = (m.generate(emb, kv_cache_dtype=kv, **gkw) for kv in ARMS.values())
    same = (g16 == g8)
    prefix = same.long().cumprod(-1).sum(-1).float()
    m.__dict__.pop("_steppers", None)
    torch.cuda.empty_cache()
    return dict(bench="kv_fp8", shape="decode_llama7b_128", weights=weights, batch=B, beams=nb, rows=B * nb, prompt=plen, new_tokens=new,
                tok_per_s={k: round(v, 1) for k, v in med.items()}, fp8_over_kv16=round(med["fp8"] / med["kv16"], 4),
                first_step_dev=round(float(dev_rows.max()), 5), first_step_argmax_agree=float((l16.argmax(-1) == l8.argmax(-1)).float().mean()),
                greedy_agree=dict(equal_of_64=round(float(same.sum(-1).float().mean()), 2), common_prefix=round(float(prefix.mean()), 2)),
                kv_bytes=kv_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_fp8_bench.txt"))
    ap.add_argument("--new", type=int, default=None)
    ap.add_argument("--weights", default="w16,mxfp4")
    ap.add_argument("--cases", default="1x3,6x3,16x5")
    args = ap.parse_args()
    from bench import DECODE_WORKLOADS
    vocab, hidden, inter, layers, heads, kvh, plen, wl_new, _, _, _ = DECODE_WORKLOADS["decode_llama7b_128"]
    cases = [tuple(int(v) for v in c.split("x")) for c in args.cases.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for weights in args.weights.split(","):
        torch.manual_seed(0)
        with torch.device(dev):
            m = ReportDecoder(vocab, hidden, inter, layers, heads, kvh).to(torch.bfloat16).eval()
        if weights == "mxfp4":
            m.quantize_mxfp4_()
        m.fuse_qkv_()
        for B, nb in cases:
            line = json.dumps(bench_leg(m, weights, B, nb, plen, hidden, args.new or wl_new))
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
