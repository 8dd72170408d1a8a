"""-m gpu: the multi-workgroup path of mxvl_clip_loss (90 <= batch <= 4096, csrc/clip_loss.hip) against a float64 evaluation of
MambaXrayVL_CLIP.py:133-148 on the same fp32 inputs, its guard bands and scratch, reproducibility, the seam at 89 | 90 rows, graph
capture, the routing of MambaXrayVLCLIP.forward, and the global batch (gather_with_grad, args.global_batch) under two ranks on cuda:0.

The bound is not guessed: at every shape the eager fp32 torch expression -- the reference's own statement -- is run on the same
inputs on the same device, its error against float64 is measured per output (max over the elements), and the kernel is allowed 4 x
that (its tile-ordered sums reassociate differently from rocBLAS's) plus fp64_bounds.FLOOR."""
import functools
import math
import os
import socket
import sys
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fp64_bounds import FLOOR, GUARD, _Buf, _ratio, _report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = {"t0.07": math.log(1 / 0.07), "clamp100": 4.6}       # the initial value; the reference clamps the multiplier to 100
SHAPES = [(90, 16), (97, 24), (130, 64), (256, 512), (1024, 100), (4096, 64)]
OUTPUTS = ("loss", "d_image", "d_text", "d_logit_scale")


def _expression(img, txt, ls):
    img, txt = F.normalize(img, dim=1), F.normalize(txt, dim=1)
    logits = ls.exp() * img @ txt.t()
    labels = torch.arange(logits.shape[0], device=logits.device)
    return (F.cross_entropy(logits, labels) + F.cross_entropy(logits.t(), labels)) / 2


def _evaluate(img, txt, ls, dtype):
    """-> (loss, d_image, d_text, d_logit_scale) of the torch expression in `dtype`, as float64 CPU tensors"""
    a, b, c = (t.detach().to(dtype).requires_grad_(True) for t in (img, txt, ls))
    loss = _expression(a, b, c)
    loss.backward()
    return tuple(t.detach().double().cpu() for t in (loss, a.grad, b.grad, c.grad))


def _inputs(n, P, scale, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + n + P)
    return torch.randn(n, P, generator=g).to(DEV), torch.randn(n, P, generator=g).to(DEV), torch.tensor(SCALES[scale], device=DEV)


def _launch(img, txt, ls):
    """one mxvl_clip_loss call; every output a view into a NaN-patterned buffer with GUARD elements on each side"""
    from medical_image_analysis_amd import _abi
    n, P = img.shape
    bufs = {"loss": _Buf.flat((1,), torch.float32, DEV), "d_image": _Buf.flat((n, P), torch.float32, DEV),
            "d_text": _Buf.flat((n, P), torch.float32, DEV), "d_logit_scale": _Buf.flat((1,), torch.float32, DEV)}
    _abi.launch("mxvl_clip_loss", img.data_ptr(), txt.data_ptr(), ls.reshape(1).data_ptr(), n, P, *(bufs[k].view.data_ptr() for k in OUTPUTS),
                device=img.device)
    torch.cuda.synchronize()
    return bufs


@functools.lru_cache(maxsize=None)
def _case(n, P, scale):
    """reference, bound and one kernel run per case, computed once and shared by the tests below (none of them writes to it)"""
    img, txt, ls = _inputs(n, P, scale)
    ref = _evaluate(img, txt, ls, torch.float64)
    eager = _evaluate(img, txt, ls, torch.float32)
    eager_err = [float((e - r).abs().max()) for e, r in zip(eager, ref)]
    bufs = _launch(img, txt, ls)
    return types.SimpleNamespace(img=img, txt=txt, ls=ls, ref=dict(zip(OUTPUTS, ref)), eager=dict(zip(OUTPUTS, eager)),
                                 tol={k: 4.0 * e + FLOOR for k, e in zip(OUTPUTS, eager_err)}, eager_err=dict(zip(OUTPUTS, eager_err)), bufs=bufs)


def _check(what, c, bufs=None):
    bufs = bufs or c.bufs
    got = {k: bufs[k].view.reshape(c.ref[k].shape) for k in OUTPUTS}
    err = {k: float(torch.nan_to_num((got[k].double().cpu() - c.ref[k]).abs(), nan=float("inf")).max()) for k in OUTPUTS}
    print(f"{what}: max |err| against float64, eager fp32 / kernel: " + " ".join(f"{k} {c.eager_err[k]:.3e} / {err[k]:.3e}" for k in OUTPUTS))
    _report(f"{what} eager fp32", **{k: _ratio(c.eager[k], c.ref[k], c.tol[k]) for k in OUTPUTS})
    _report(f"{what} kernel", **{k: _ratio(got[k], c.ref[k], c.tol[k]) for k in OUTPUTS})


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("n,P", SHAPES)
def test_kernel_against_float64(n, P, scale):
    """Measured on an MI355X, max |err| against float64 per output (eager fp32 torch / kernel): see DESIGN.md, "Stage-2 loss beyond
    89 rows"."""
    _check(f"clip_loss n={n} P={P} {scale}", _case(n, P, scale))


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("n,P", SHAPES)
def test_guards_intact_and_no_scratch_value_survives(n, P, scale):
    c = _case(n, P, scale)
    for k in OUTPUTS:
        assert c.bufs[k].guard_intact(), f"store outside {k}"
        assert c.bufs[k].written(), f"{k}: a NaN pattern survived"
    # the 8 n scratch floats at the head of d_image were overwritten by gradient rows, not left as norms / log-sum-exps: the head
    # rows meet the same bound as every other row
    R0 = -(-8 * n // P)
    assert _ratio(c.bufs["d_image"].view[:R0], c.ref["d_image"][:R0], c.tol["d_image"]) <= 1.0


@pytest.mark.parametrize("n,P", [(130, 64), (1024, 100)])
def test_same_bits_on_every_run_and_in_deterministic_mode(n, P):
    import medical_image_analysis_amd as pkg
    c = _case(n, P, "t0.07")
    try:
        pkg.set_deterministic(False)
        again = _launch(c.img, c.txt, c.ls)
        pkg.set_deterministic(True)
        det = _launch(c.img, c.txt, c.ls)
    finally:
        pkg.set_deterministic(None)
    for k in OUTPUTS:
        assert torch.equal(again[k].raw, c.bufs[k].raw), f"{k}: two calls differ"
        assert torch.equal(det[k].raw, c.bufs[k].raw), f"{k}: deterministic mode changes the bits"


def test_seam_89_and_90_rows():
    """89 rows: the single-workgroup kernel, 90: the first size of the multi-workgroup path; both within their own measured bound, and
    the old kernel's result bit-equal between two calls."""
    for n in (89, 90):
        _check(f"clip_loss seam n={n} P=64", _case(n, 64, "t0.07"))
    c = _case(89, 64, "t0.07")
    again = _launch(c.img, c.txt, c.ls)
    for k in OUTPUTS:
        assert torch.equal(again[k].raw, c.bufs[k].raw), k


def test_graph_capture_and_replay():
    """the call is a fixed sequence of launches on the caller's stream: captured once, replayed on new contents of the static inputs"""
    from medical_image_analysis_amd.mambaxray_vl import clip_contrastive_loss
    img, txt, ls = _inputs(128, 64, "t0.07")
    ls.requires_grad_(True)
    s_img, s_txt = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        clip_contrastive_loss(s_img, s_txt, ls)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = clip_contrastive_loss(s_img, s_txt, ls)
    new_img, new_txt, _ = _inputs(128, 64, "t0.07", seed=1)
    with torch.no_grad():
        s_img.copy_(new_img)
        s_txt.copy_(new_txt)
    graph.replay()
    torch.cuda.synchronize()
    want = clip_contrastive_loss(new_img.requires_grad_(True), new_txt.requires_grad_(True), ls)
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), want.detach())
    got_saved, want_saved = loss.grad_fn.saved_tensors, want.grad_fn.saved_tensors
    assert len(got_saved) == 3
    for a, b in zip(got_saved, want_saved):
        assert torch.equal(a, b)


# ---- the module ---------------------------------------------------------------------------------------------------------------------
TEXTS = ["heart size is normal . lungs are clear .", "no acute cardiopulmonary process .", "mild left lower lobe opacity .",
         "stable cardiomegaly . no pleural effusion ."]


class TextEnc(nn.Module):
    config = types.SimpleNamespace(hidden_size=32)

    def __init__(self):
        super().__init__()
        self.emb = nn.Embedding(256, 32)

    def forward(self, ids, attention_mask=None):
        return {"last_hidden_state": self.emb(ids)}


class PatchEnc(nn.Module):
    """(B, 3, 224, 224) -> (B, 49, 768): one trainable layer in place of the 12-layer ARM encoder.  The two-rank comparison is about
    the gather and its gradient; a frozen random-init ARM under bf16 autocast feeds the loss features whose rounding noise (a
    different GEMM tiling at 46 and at 92 images, twelve layers deep) moves a contrastive loss in its third digit."""
    num_features = 768

    def __init__(self):
        super().__init__()
        self.proj = nn.Linear(3 * 32 * 32, 768)

    def forward(self, x):
        p = x.unfold(2, 32, 32).unfold(3, 32, 32).permute(0, 2, 3, 1, 4, 5).reshape(x.shape[0], 49, 3 * 32 * 32)
        return torch.tanh(self.proj(p))


def _build_clip(global_batch, tiny=False):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_mambaxray_vl import WordTokenizer
    from medical_image_analysis_amd import mambaxray_vl as mx
    torch.manual_seed(0)
    args = mx.default_args(type="base", projection_dim=64, global_batch=global_batch)      # freeze_vm: the encoder only runs forward
    m = mx.MambaXrayVLCLIP(args, tokenizer=WordTokenizer(), text_encoder=TextEnc())
    if tiny:
        m.visual_encoder = PatchEnc()
    return m.to(DEV)


def _studies(first, count, step=0):
    g = torch.Generator().manual_seed(100 * step + first)
    return {"id": [f"s{step}i{first + i}" for i in range(count)], "image": [torch.randn(count, 3, 224, 224, generator=g).to(DEV)],
            "input_text": [f"{TEXTS[(first + i) % 4]} study {first + i} of step {step}" for i in range(count)]}


def test_module_routes_96_studies_to_the_kernel():
    m = _build_clip(False)
    seen = {}
    enc_i, enc_t = m.encode_img, m.encode_txt
    m.encode_img = lambda images: seen.setdefault("img", enc_i(images))
    m.encode_txt = lambda toks: seen.setdefault("txt", enc_t(toks))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = m(_studies(0, 96))["loss"]
    assert type(loss.grad_fn).__name__ == "_ClipLossBackward", f"batch 96 on a HIP device left the kernel: {loss.grad_fn}"
    img, txt, ls = seen["img"].detach().float(), seen["txt"].detach().float(), m.logit_scale.detach()
    assert img.shape == (96, 64)
    ref, eager = _evaluate(img, txt, ls, torch.float64)[0], _evaluate(img, txt, ls, torch.float32)[0]
    tol = 4.0 * float((eager - ref).abs()) + FLOOR
    print(f"module loss {float(loss.detach()):.7f} float64 {float(ref):.7f} eager fp32 error {float((eager - ref).abs()):.3e}")
    _report("MambaXrayVLCLIP batch 96", loss=_ratio(loss, ref, tol))
    loss.backward()
    assert m.logit_scale.grad is not None and torch.isfinite(m.vision_proj.weight.grad).all()


# ---- two ranks on cuda:0 over gloo --------------------------------------------------------------------------------------------------
PER_RANK = 46


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _grads(model):
    return {k: p.grad.detach().float().cpu().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from medical_image_analysis_amd.pretrain_engine import init_distributed, wrap_ddp
    torch.cuda.set_device(0)
    init_distributed("gloo")
    try:
        for global_batch in (True, False):
            model = _build_clip(global_batch, tiny=True)
            net = wrap_ddp(model, DEV, bucket_cap_mb=1)
            opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, fused=True)
            grads, losses, nodes = None, [], set()
            for step in range(3):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = net(_studies(PER_RANK * rank, PER_RANK, step))["loss"]
                nodes.add(type(loss.grad_fn).__name__)
                loss.backward()
                if step == 0:
                    grads = _grads(model)
                opt.step()
                opt.zero_grad(set_to_none=True)
                losses.append(float(loss.detach()))
            torch.cuda.synchronize()
            sd = {k: v.detach().float().cpu().numpy().copy() for k, v in model.state_dict().items()
                  if v.is_floating_point() and not k.startswith("visual_encoder.")}
            out.put((rank, global_batch, losses, sd, grads, sorted(nodes)))
    except Exception as e:      # noqa: BLE001 -- reported to the parent, which fails the test with the message
        out.put((rank, None, f"{type(e).__name__}: {str(e)[:400]}", None, None, None))
    dist.barrier()
    dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _two_ranks():
    """ONE spawn of two ranks; each runs three steps with global_batch on, then three with it off.  Ends on the first child that dies."""
    import queue
    import time
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results, deadline = [], time.monotonic() + 600
    try:
        while len(results) < 2 * world:
            try:
                results.append(q.get(timeout=1))
            except queue.Empty:
                pass
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not dead, f"a rank ended with status {dead[0]}"
            assert not (results and isinstance(results[-1][2], str)), results[-1][2]
            assert time.monotonic() < deadline, "the two ranks did not finish"
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return {(r[0], r[1]): r for r in results}


def _l2(t):
    return float((t.astype("float64") ** 2).sum())


def test_two_ranks_global_batch_equals_one_process_on_the_92_studies():
    res = _two_ranks()
    (_, _, l0, sd0, g0, nodes0), (_, _, l1, sd1, g1, nodes1) = res[(0, True)], res[(1, True)]
    assert nodes0 == nodes1 == ["_ClipLossBackward"], "92 global studies run on the multi-workgroup kernel"
    assert l0 == l1 and all(x == x for x in l0), "every rank evaluates the same global loss"
    for k in sd0:
        assert (sd0[k] == sd1[k]).all(), f"replicas diverged at {k}"
    for k in g0:
        assert (g0[k] == g1[k]).all(), f"ranks hold different averaged gradients at {k}"
    # one process on the concatenated batch, twice: the second pass measures how well the batch repeats itself (bf16 autocast encoder,
    # batch-dependent kernel choices); the check is test_ddp_finetune_gpu.py's -- as close as a repetition is to itself (x 4), 5e-2 at least
    model = _build_clip(False, tiny=True)
    both = [_studies(PER_RANK * r, PER_RANK, 0) for r in range(2)]
    batch = {"id": both[0]["id"] + both[1]["id"], "image": [torch.cat([both[0]["image"][0], both[1]["image"][0]])],
             "input_text": both[0]["input_text"] + both[1]["input_text"]}
    passes = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(batch)["loss"]
        loss.backward()
        lv = float(loss.detach())
        assert abs(lv - l0[0]) <= 2e-3 * max(1.0, abs(lv)), (lv, l0[0])
        passes.append(_grads(model))
    wants, again = passes
    assert sorted(wants) == sorted(g0) and "logit_scale" in g0
    total = sum(_l2(w) for w in wants.values())
    floor_all = (sum(_l2(again[k] - wants[k]) for k in g0) / total) ** 0.5
    num, worst = 0.0, 0.0
    for k, got in g0.items():
        e2, w2 = _l2(got - wants[k]), _l2(wants[k])
        num += e2
        if w2 > 1e-6 * total:
            rel, floor = (e2 / w2) ** 0.5, (_l2(again[k] - wants[k]) / w2) ** 0.5
            worst = max(worst, rel)
            assert rel <= max(5e-2, 4.0 * floor), f"grad {k}: relative L2 difference {rel} (repeatability: {floor})"
    assert (num / total) ** 0.5 <= max(5e-2, 4.0 * floor_all)
    print(f"global batch, 2 ranks x {PER_RANK} vs one process x {2 * PER_RANK}: worst per-tensor relative L2 difference {worst:.2e}, "
          f"all gradients {(num / total) ** 0.5:.2e}; repeatability {floor_all:.2e}")


def test_two_ranks_without_global_batch_keep_the_per_rank_loss():
    res = _two_ranks()
    (_, _, l0, sd0, _, nodes0), (_, _, l1, sd1, _, nodes1) = res[(0, False)], res[(1, False)]
    assert nodes0 == nodes1 == ["_ClipLossBackward"]
    for k in sd0:
        assert (sd0[k] == sd1[k]).all(), f"replicas diverged at {k}"
    model = _build_clip(False, tiny=True)
    for rank, got in ((0, l0[0]), (1, l1[0])):
        with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
            want = float(model(_studies(PER_RANK * rank, PER_RANK, 0))["loss"])
        assert abs(want - got) <= 2e-3 * max(1.0, abs(want)), (rank, want, got)
    assert l0[0] != l1[0], "each rank contrasts its own 46 studies"
