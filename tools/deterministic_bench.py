"""What deterministic mode costs (dev tool; bench.py is the contract): mxvl_scan_bwd and mxvl_conv1d_bwd at the north-star shape
(B8 L4096 D1536 N16 bf16) and at the ARM-large pre-training step's shape (B16 L4080 D2048), and the default bench.py model's training step,
mode off and on interleaved in one process so that clock and box noise hit both alike.
usage: python tools/deterministic_bench.py [--no-step] [--steps K]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import medical_image_analysis_amd as pkg
from medical_image_analysis_amd import _abi
from medical_image_analysis_amd import causal_conv1d as cc
from medical_image_analysis_amd import selective_scan_interface as ssi

DEV = torch.device("cuda:0")


def _time(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _ab(what, fn, iters=10, rounds=5):
    """`fn` timed with the mode off and on in interleaved rounds -> one line with min / median of both and their ratio"""
    t = {False: [], True: []}
    try:
        for _ in range(rounds):
            for on in (False, True):
                pkg.set_deterministic(on)
                t[on].append(_time(fn, iters))
    finally:
        pkg.set_deterministic(None)
    off, on = min(t[False]), min(t[True])
    print(f"{what:44s} default min {off:9.1f} us med {statistics.median(t[False]):9.1f} us | deterministic min {on:9.1f} us "
          f"med {statistics.median(t[True]):9.1f} us | x{on / off:.3f}", flush=True)


def scan_bwd(B, D, L, N, dtype):
    g = torch.Generator(device="cpu").manual_seed(0)
    A = (-0.5 * torch.rand(D, N, generator=g)).to(DEV)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV, dtype)
    u, z, Bm, Cm, dout = mk(B, D, L), mk(B, D, L), mk(B, 1, N, L), mk(B, 1, N, L), mk(B, D, L)
    delta = (0.5 * torch.rand(B, D, L, generator=g)).to(DEV, dtype)
    Dv, bias = torch.randn(D, generator=g).to(DEV), (0.5 * torch.rand(D, generator=g)).to(DEV)
    _, _, ckpt = ssi.scan_fwd_raw(u, delta, A, Bm, Cm, Dv, z, bias, True, want_ckpt=True)
    pkg.set_deterministic(True)
    ws = _abi.det_workspace_bytes("mxvl_scan_bwd_workspace_bytes", _fwd_desc(u, delta, A, Bm, Cm, Dv, z, bias, ckpt))
    pkg.set_deterministic(None)
    _ab(f"scan_bwd B{B} D{D} L{L} N{N} {str(dtype)[6:]} (ws {ws / 2 ** 20:.0f} MiB)",
        lambda: ssi.scan_bwd_raw(u, delta, A, Bm, Cm, Dv, z, bias, True, ckpt, dout))


def _fwd_desc(u, delta, A, Bm, Cm, Dv, z, bias, ckpt):
    d = _abi.ScanDesc()
    ssi._fill_fwd(d, u, delta, A, Bm, Cm, Dv, z, bias, True, None, None, ckpt, False, ckpt is not None and ckpt.dim() == 3)
    return d


def conv_bwd(B, D, L, dtype):
    g = torch.Generator(device="cpu").manual_seed(1)
    x, dy = torch.randn(B, D, L, generator=g).to(DEV, dtype), torch.randn(B, D, L, generator=g).to(DEV, dtype)
    w, b = torch.randn(D, 4, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV)
    _ab(f"conv1d_bwd B{B} D{D} L{L} W4 {str(dtype)[6:]}", lambda: cc.conv1d_bwd_raw(x, w, b, 1, dy))


def step(steps):
    """the default bench.py workload (arm_pretrain_large_1024: VisionMamba 1024 x 24 at 1024 x 1024, batch 16, bf16 autocast)"""
    from medical_image_analysis_amd.models_pretrain import VisionMamba
    from medical_image_analysis_amd.pretrain_engine import PretrainEngine
    torch.manual_seed(0)
    model = VisionMamba(img_size=1024, patch_size=16, stride=16, embed_dim=1024, depth=24, dec_embed_dim=512, rms_norm=True,
                        residual_in_fp32=True, fused_add_norm=True, if_abs_pos_embed=True, bimamba_type="None").to(DEV)
    eng = PretrainEngine(model, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(1000)
    batches = [torch.randn(16, 3, 1024, 1024, generator=g).to(DEV) for _ in range(2)]
    it = [0]

    def one():
        eng.step(batches[it[0] % 2])
        it[0] += 1

    _ab("training step arm_pretrain_large_1024 (eager)", one, iters=steps, rounds=3)
    print(f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--steps", type=int, default=4, help="training steps per timed round")
    args = ap.parse_args()
    for shape in ((8, 1536, 4096, 16), (16, 2048, 4080, 16)):
        scan_bwd(*shape, torch.bfloat16)
    for B, D, L, _ in ((8, 1536, 4096, 16), (16, 2048, 4080, 16)):
        conv_bwd(B, D, L, torch.bfloat16)
    if not args.no_step:
        step(args.steps)
