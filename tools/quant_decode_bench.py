"""Dev tool: what the quantised storages of the layer weights (weight_formats.WEIGHT_FORMATS: ReportDecoder.quantize_(name), mxvl_decode_gemv
with the format's W_FLAG) gain or lose against the 16-bit one and against each other.  Separate from bench.py; nothing routes on its
numbers.  (It folds the per-format tools int8_decode_bench.py, w4_bench.py, fp8_decode_bench.py and int4_decode_bench.py into one.)

    python tools/quant_decode_bench.py [--arms bf16,int8,fp8,mxfp4,int4]                    every step below, each in a fresh child process
                                                     under its own time limit; stops at the first step that fails or runs out of time
    python tools/quant_decode_bench.py [--arms ...] proj|llama|qwen                         one step, in this process

An arm is "bf16" or a name of WEIGHT_FORMATS; the default is all of them.
proj (a): one projection launch per arm at the Llama-7B and Qwen-1.8B widths, rows 1, 3, 18, 48 and 80, with the descriptors of the kernel
stepper's split-norm step (qkv + bias; o_proj and down_proj as K-split planes, k_splits as the stepper picks them; gate / up with the
SwiGLU epilogue), the arms interleaved in one process.  Every launch reads another copy of the weights (enough copies to exceed the
256 MB of last-level cache several times), as a decode step walks through the layers.  One JSON line per (model, projection, rows):
microseconds per launch, median of 3 repeats after a dropped warm-up one, and GB/s of weight bytes (codes + scales).
llama / qwen (b): generate() tokens/s of decode_llama7b_128 (random weights, 230-embedding prompt, 128 new tokens) at batch x beams 1 x 3,
6 x 3, 16 x 3, 16 x 5 and of the Qwen-1.8B shape at 16 x 5; the arms' decoders of a shape live side by side and their calls alternate;
median of 3 after the capturing call; plus the bytes each decoder's parameters + buffers hold (`decoder_bytes`).
Ratios (`<arm>_over_bf16`) are speed-ups: above 1 the arm is faster than the 16-bit one."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

STEPS = (("proj", 600), ("llama", 900), ("qwen", 420))          # (step, seconds it may take)

ap = argparse.ArgumentParser()
ap.add_argument("--arms", default=None, help="comma-separated: bf16 and names of WEIGHT_FORMATS (default: all)")
ap.add_argument("step", nargs="?", choices=[s for s, _ in STEPS])
args = ap.parse_args() if __name__ == "__main__" else ap.parse_args([])


def main_driver():
    for step, limit in STEPS:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + (["--arms", args.arms] if args.arms else []) + [step], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(bench="quant_decode", step=step, failed=True, rc=rc)), flush=True)
            return rc
    return 0


if __name__ == "__main__" and args.step is None:
    sys.exit(main_driver())                                      # (before torch is imported: the driver never opens the GPU)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from medical_image_analysis_amd import _abi  # noqa: E402
from medical_image_analysis_amd.report_decoder import ReportDecoder, _KernelStepper  # noqa: E402
from medical_image_analysis_amd.weight_formats import WEIGHT_FORMATS  # noqa: E402

dev = torch.device("cuda:0")
ARMS = tuple(args.arms.split(",")) if args.arms else ("bf16",) + tuple(WEIGHT_FORMATS)
WIDTHS = {"llama7b": (4096, 11008, 4096 * 3), "qwen1p8b": (2048, 5504, 2048 * 3)}       # hidden, intermediate, fused qkv rows
ROWS = (1, 3, 18, 48, 80)
COPY_BYTES = 768 << 20


def _flag(arm):
    return WEIGHT_FORMATS[arm].W_FLAG if arm in WEIGHT_FORMATS else 0


def _weights(arm, N, K):
    """(weight, scale) of one random (N, K) projection in the storage of `arm`: the format's own quantiser on a random weight"""
    W = (torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16)
    return WEIGHT_FORMATS[arm].quantize(W) if arm in WEIGHT_FORMATS else (W, None)


def _nbytes(ws):
    return sum(t.numel() * t.element_size() for t in ws if t is not None)


def _desc(arm, x, w, s, y=None, w2=None, s2=None, bias=None, acc=None, splits=1):
    d = _abi.GemvDesc()
    d.rows, d.K, d.N = x.shape[0], x.shape[1], y.shape[1] if y is not None else acc.shape[2]
    d.dtype = _abi.MXVL_BF16 | _flag(arm)
    d.x, d.W, d.y, d.bias = x.data_ptr(), w.data_ptr(), _abi.ptr(y), _abi.ptr(bias)
    d.W2, d.swiglu = _abi.ptr(w2), int(w2 is not None)
    d.w_scale, d.w2_scale = _abi.ptr(s), _abi.ptr(s2)
    d.split_acc, d.k_splits = _abi.ptr(acc), splits
    return d


def _ratios(v, faster_is_smaller):
    """<arm>_over_bf16 of the per-arm medians `v`"""
    if "bf16" not in v:
        return {}
    return {f"{a}_over_bf16": round(v["bf16"] / v[a] if faster_is_smaller else v[a] / v["bf16"], 4) for a in v if a != "bf16"}


def bench_proj():
    for model, (hidden, inter, nqkv) in WIDTHS.items():
        projs = (("qkv", nqkv, hidden, "bias"), ("o_proj", hidden, hidden, "split"), ("gate_up", inter, hidden, "swiglu"),
                 ("down_proj", hidden, inter, "split"))
        for pname, N, K, epi in projs:
            sets = {}
            for arm in ARMS:                     # one quantised pair per arm, copied: the time of a launch does not depend on the values
                first = (_weights(arm, N, K), _weights(arm, N, K) if epi == "swiglu" else None)
                nbytes = _nbytes(first[0]) + (_nbytes(first[1]) if first[1] else 0)
                clone = lambda ws: None if ws is None else tuple(None if t is None else t.clone() for t in ws)  # noqa: E731
                sets[arm] = ([first] + [(clone(first[0]), clone(first[1])) for _ in range(max(2, -(-COPY_BYTES // nbytes)) - 1)], nbytes)
            for rows in ROWS:
                x = torch.randn(rows, K, device=dev).to(torch.bfloat16)
                y = torch.empty(rows, N, device=dev, dtype=torch.bfloat16)
                bias = torch.zeros(N, device=dev, dtype=torch.bfloat16)
                splits = _KernelStepper._k_splits(N, K, rows) if epi == "split" else 1
                acc = torch.empty(splits, rows, N, device=dev) if epi == "split" else None
                descs, plans = {}, {}
                for arm in ARMS:
                    descs[arm] = [_desc(arm, x, a[0], a[1], y=None if acc is not None else y, w2=b[0] if b else None, s2=b[1] if b else None,
                                        bias=bias if epi == "bias" else None, acc=acc, splits=splits) for a, b in sets[arm][0]]
                    out = (ctypes.c_int32 * 5)()
                    _abi.load().mxvl_decode_gemm_plan(ctypes.byref(descs[arm][0]), out)
                    plans[arm] = list(out)
                times = {arm: [] for arm in ARMS}
                for rep in range(4):                                         # the first repeat warms up and is dropped
                    for arm in ARMS:
                        ds = descs[arm]
                        iters = max(24, len(ds) * 2)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(iters):
                            _abi.launch("mxvl_decode_gemv", ds[i % len(ds)], device=dev)
                        e1.record()
                        e1.synchronize()
                        if rep:
                            times[arm].append(e0.elapsed_time(e1) * 1e3 / iters)
                us = {arm: statistics.median(v) for arm, v in times.items()}
                print(json.dumps(dict(bench="quant_proj", model=model, proj=pname, N=N, K=K, rows=rows, epi=epi, k_splits=splits,
                                      us={a: round(v, 2) for a, v in us.items()},
                                      all_runs={a: [round(t, 2) for t in v] for a, v in times.items()},
                                      weight_GBps={a: round(sets[a][1] / us[a] / 1e3, 1) for a in ARMS},
                                      **_ratios(us, True), plan=plans)), flush=True)
            del sets
            torch.cuda.empty_cache()


def _bytes(m):
    seen, total = set(), 0
    for t in list(m.parameters()) + list(m.buffers()):
        st = t.untyped_storage()
        if st.data_ptr() not in seen:
            seen.add(st.data_ptr())
            total += st.nbytes()
    return total


def bench_generate(name, cases):
    from bench import DECODE_WORKLOADS
    vocab, hidden, inter, layers, heads, kvh, plen, new, _, _, _ = DECODE_WORKLOADS[name]
    arms = {}
    for arm in ARMS:
        torch.manual_seed(0)
        with torch.device(dev):
            m = ReportDecoder(vocab, hidden, inter, layers, heads, kvh).to(torch.bfloat16).eval()
        if arm in WEIGHT_FORMATS:
            m.quantize_(arm)
        m.fuse_qkv_()
        arms[arm] = m
    torch.cuda.empty_cache()
    nbytes = {k: _bytes(m) for k, m in arms.items()}
    for B, nb in cases:
        emb = (0.02 * torch.randn(B, plen, hidden, generator=torch.Generator().manual_seed(1000))).to(dev, torch.bfloat16)
        kw = dict(num_beams=nb, min_new_tokens=new, max_new_tokens=new, repetition_penalty=2.0, length_penalty=2.0, eos_token_id=2, pad_token_id=0)
        times = {k: [] for k in arms}
        for m in arms.values():
            m.generate(emb, **kw)                                    # prefill + capture
        for _ in range(3):                                           # interleaved
            for k, m in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = m.generate(emb, **kw)
                torch.cuda.synchronize()
                times[k].append(B * out.shape[1] / (time.perf_counter() - t0))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps(dict(bench="quant_generate", shape=name, batch=B, beams=nb, rows=B * nb, new_tokens=new,
                              tok_per_s={k: round(v, 1) for k, v in med.items()}, all_runs={k: [round(t, 1) for t in v] for k, v in times.items()},
                              **_ratios(med, False), decoder_bytes=nbytes)), flush=True)
        for m in arms.values():
            m.__dict__.pop("_steppers", None)                        # the next case's buffers, not both cases'


if __name__ == "__main__":
    bad = [a for a in ARMS if a != "bf16" and a not in WEIGHT_FORMATS]
    if bad:
        sys.exit(f"unknown arm(s) {bad}: bf16 or one of {list(WEIGHT_FORMATS)}")
    if args.step == "proj":
        bench_proj()
    elif args.step == "llama":
        bench_generate("decode_llama7b_128", [(1, 3), (6, 3), (16, 3), (16, 5)])
    else:
        bench_generate("decode_qwen1p8b_b16x5", [(16, 5)])
