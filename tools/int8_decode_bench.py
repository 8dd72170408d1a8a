"""Dev tool: report decoding with int8 layer projections (ReportDecoder.quantize_int8_, mxvl_decode_gemv with MXVL_W_INT8) against
the 16-bit decoder.

    python tools/int8_decode_bench.py [llama|qwen|all]

One process, one box: the 16-bit and the int8 decoder of a shape live side by side and their generate() calls alternate.  Shapes:
decode_llama7b_128 at batch x beams 1 x 3, 6 x 3, 16 x 3, 16 x 5 and Qwen-1.8B at 16 x 5 (the reference's decode batches).  One JSON
line per case: tokens/s of both arms (median of 3 alternating repeats after the capturing call), their ratio, and the bytes the
decoder's parameters + buffers hold (`decoder_bytes`, what low_resource is for) with the peak allocated while quantising and decoding."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medical_image_analysis_amd.report_decoder import ReportDecoder  # noqa: E402

dev = "cuda:0"


def _bytes(m):
    seen, total = set(), 0
    for t in list(m.parameters()) + list(m.buffers()):
        st = t.untyped_storage()
        if st.data_ptr() not in seen:
            seen.add(st.data_ptr())
            total += st.nbytes()
    return total


def bench_shape(name, cases, new=None):
    from bench import DECODE_WORKLOADS
    vocab, hidden, inter, layers, heads, kvh, plen, wl_new, _, _, _ = DECODE_WORKLOADS[name]
    new = new or wl_new
    arms, mem = {}, {}
    for arm in ("w16", "int8"):
        torch.manual_seed(0)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.device(dev):
            m = ReportDecoder(vocab, hidden, inter, layers, heads, kvh).to(torch.bfloat16).eval()
        if arm == "int8":
            m.quantize_int8_()
        m.fuse_qkv_()
        torch.cuda.synchronize()
        arms[arm] = m
        mem[arm] = dict(decoder_bytes=_bytes(m), allocated_after_load=torch.cuda.memory_allocated() - base,
                        peak_while_loading=torch.cuda.max_memory_allocated() - base)
    for B, nb in cases:
        emb = (0.02 * torch.randn(B, plen, hidden, generator=torch.Generator().manual_seed(1000))).to(dev, torch.bfloat16)
        kw = dict(num_beams=nb, min_new_tokens=new, max_new_tokens=new, repetition_penalty=2.0, length_penalty=2.0, eos_token_id=2, pad_token_id=0)
        times = {k: [] for k in arms}
        for k, m in arms.items():
            m.generate(emb, **kw)                                # prefill + capture
        for _ in range(3):                                       # interleaved
            for k, m in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = m.generate(emb, **kw)
                torch.cuda.synchronize()
                times[k].append(B * out.shape[1] / (time.perf_counter() - t0))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps(dict(bench="int8_decode", shape=name, batch=B, beams=nb, rows=B * nb, new_tokens=new,
                              tok_per_s={k: round(v, 1) for k, v in med.items()}, int8_over_w16=round(med["int8"] / med["w16"], 4),
                              decoder_bytes={k: v["decoder_bytes"] for k, v in mem.items()},
                              decoder_bytes_ratio=round(mem["int8"]["decoder_bytes"] / mem["w16"]["decoder_bytes"], 4),
                              load=mem)), flush=True)
        for m in arms.values():
            m.__dict__.pop("_steppers", None)                    # the next case's buffers, not both cases'
    del arms
    torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("llama", "all"):
        bench_shape("decode_llama7b_128", [(1, 3), (6, 3), (16, 3), (16, 5)])
    if what in ("qwen", "all"):
        bench_shape("decode_qwen1p8b_b16x5", [(16, 5)])
