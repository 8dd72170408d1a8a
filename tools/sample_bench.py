"""Dev tool: the sampling update (mxvl_sample_step) against its torch restatement, and a sampled token against a greedy one.

    python tools/sample_bench.py update      # rows {1, 6, 16, 80} x V {32 000, 151 936} x {no filter, top_k 50, top_p 0.9, both}
    python tools/sample_bench.py token       # generate(do_sample=True) vs greedy, decode_llama7b_128-shaped decoder, 16 rows x 128 tokens

One process, one box: both arms of every comparison run interleaved on the same device.  One JSON line per shape.  `update`: 200 timed
calls after 20 warm-ups, HIP events around every call, median; the state is reset every 100 calls (max_new 128)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medical_image_analysis_amd.report_decoder import ReportDecoder, _SampleState  # noqa: E402

dev = "cuda:0"
FILTERS = {"none": dict(top_k=None, top_p=1.0), "top_k50": dict(top_k=50, top_p=1.0), "top_p0.9": dict(top_k=None, top_p=0.9),
           "both": dict(top_k=50, top_p=0.9)}


def _time_calls(fn, state, n=200, warm=20):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i in range(warm + n):
        if i % 100 == 0:
            state.reset()
        if i >= warm:
            ev[i - warm][0].record()
        fn()
        if i >= warm:
            ev[i - warm][1].record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def bench_update():
    for V in (32000, 151936):
        for rows in (1, 6, 16, 80):
            logits = torch.randn(rows, V, device=dev) * 4
            for name, f in FILTERS.items():
                st = _SampleState(rows, V, 128, 0, [2], 128, 2.0, 0.8, f["top_k"], f["top_p"], dev)
                st.seed.fill_(1234)
                assert st._hip_supported(logits)
                hip = _time_calls(lambda: st._advance_hip(logits), st)
                tor = _time_calls(lambda: st.advance_torch(logits), st)
                print(json.dumps(dict(bench="sample_update", vocab=V, rows=rows, filters=name, hip_us=round(hip, 1), torch_us=round(tor, 1),
                                      torch_over_hip=round(tor / hip, 2))), flush=True)


def bench_token():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import DECODE_WORKLOADS
    vocab, hidden, inter, layers, heads, kvh, plen, new, _, _, _ = DECODE_WORKLOADS["decode_llama7b_128"]
    B = 16
    torch.manual_seed(0)
    with torch.device(dev):
        m = ReportDecoder(vocab, hidden, inter, layers, heads, kvh).to(torch.bfloat16).eval()
    emb = (0.02 * torch.randn(B, plen, hidden, generator=torch.Generator().manual_seed(1000))).to(dev, torch.bfloat16)
    common = dict(num_beams=1, min_new_tokens=new, max_new_tokens=new, repetition_penalty=2.0, eos_token_id=2, pad_token_id=0)
    arms = {"greedy": dict(do_sample=False), "sample": dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9),
            "sample_nofilter": dict(do_sample=True)}
    times = {k: [] for k in arms}
    for k, kw in arms.items():
        m.generate(emb, **common, **kw)                      # capture
    for _ in range(5):                                       # interleaved
        for k, kw in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.generate(emb, **common, **kw)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / out.shape[1] * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps(dict(bench="sample_token", shape="decode_llama7b_128", rows=B, new_tokens=new,
                          ms_per_token={k: round(v, 4) for k, v in med.items()},
                          sample_over_greedy=round(med["sample"] / med["greedy"], 4),
                          sample_nofilter_over_greedy=round(med["sample_nofilter"] / med["greedy"], 4))), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "update"
    {"update": bench_update, "token": bench_token}[what]()
