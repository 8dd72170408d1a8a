"""The stage-2 loss beyond 89 rows (dev tool; bench.py is the contract): mxvl_clip_loss's multi-workgroup path against the eager fp32
torch forward + backward it replaces on a HIP device, at n = 96, 384, 1024, 4096 global studies with 512 features (the reference's
projection width).  Both are timed in ONE process in alternating rounds, so clock and box noise hit both alike; HIP events around
every single call, one warm-up round, median of 20.  Nothing gates on these numbers.
usage: python tools/clip_loss_bench.py [--dim 512] [--calls 20]"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from medical_image_analysis_amd.mambaxray_vl import clip_contrastive_loss

DEV = torch.device("cuda:0")


def _eager(img, txt, ls):
    a, b = F.normalize(img, dim=1), F.normalize(txt, dim=1)
    logits = ls.exp() * a @ b.t()
    labels = torch.arange(logits.shape[0], device=logits.device)
    return (F.cross_entropy(logits, labels) + F.cross_entropy(logits.t(), labels)) / 2


def _once(loss_fn, img, txt, ls):
    """forward + backward of one loss, in microseconds between two HIP events"""
    for t in (img, txt, ls):
        t.grad = None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    loss_fn(img, txt, ls).backward()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def bench(n, dim, calls):
    g = torch.Generator().manual_seed(n)
    img, txt = (torch.randn(n, dim, generator=g).to(DEV).requires_grad_(True) for _ in range(2))
    ls = torch.tensor(math.log(1 / 0.07), device=DEV, requires_grad=True)
    paths = {"kernel": clip_contrastive_loss, "eager": _eager}
    t = {k: [] for k in paths}
    for rnd in range(calls + 1):                       # round 0 warms both up
        for k, fn in paths.items():
            us = _once(fn, img, txt, ls)
            if rnd:
                t[k].append(us)
    ker, eag = statistics.median(t["kernel"]), statistics.median(t["eager"])
    print(f"n {n:5d} dim {dim}: mxvl_clip_loss median {ker:9.1f} us (min {min(t['kernel']):9.1f}) | eager fp32 median {eag:9.1f} us "
          f"(min {min(t['eager']):9.1f}) | kernel / eager x{ker / eag:.2f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    for n in (96, 384, 1024, 4096):
        bench(n, args.dim, args.calls)
