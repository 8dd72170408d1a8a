"""Dev helper (GPU box, one process, one MI355X): what the device-side pre-training augmentation costs per batch, next to the
CPU pipeline it replaces.
    PYTHONPATH=. python tools/augment_bench.py [--out profiles/r09_augment.txt] [--batch 16] [--height 2544 --width 3056]

Two recipes on one batch of synthetic radiographs:
    arm : RandomResizedCrop -> flip -> ToTensor -> Normalize(ImageNet)      -> (B, 3, 1024, 1024)   (main_pretrain.py:116-120)
    mae : RandomResizedCrop -> Grayscale -> flip -> ToTensor -> Normalize(.5) -> (B, 1, 1280, 1280)   (HD_Xray_Pretrain_MAE main.py:136-141)
A pool of `--sets` parameter sets (one random box + flip per image, seeded) is drawn BEFORE any timing; iteration k of every arm uses
set k mod sets, so all arms do the same work and no iteration repeats its predecessor's boxes.  The crop paths compute their
resample coefficients on the host for every box of every call (no cache is involved), so that cost is inside every device arm; it
is also timed alone.  Arms, all in this process, each timed as `--repeats` windows (median [min .. max] of the window means):
    batched, resident : one preprocess_batch call on images already on the device -- host clock to a device synchronise (the
                        call's host work -- coefficients, packing, one pinned upload -- is serial with its launch), and device events
    batched, from host: the same call on the host arrays (uploads the rows each crop reads; bytes and rate printed)
    16 singles        : preprocess_image per image with crop / flip / gray, resident; each call computes and uploads its own tables
                        (one pinned copy), so this is the per-image API, not a tuned baseline
    coefficients      : the host-side table computation of one batch alone (2 tables per image)
    Pillow            : crop -> resize(BICUBIC) -> [convert("L")] -> transpose -> ToTensor / Normalize arithmetic in torch, one
                        image after the other on the CPU -- host clock; the CPU model and the thread counts are printed
The outputs of the three device arms are compared bit for bit with the Pillow arm on set 0 before anything is timed.  No GPU: the tool fails."""
import argparse
import os
import time

import numpy as np
import torch

from medical_image_analysis_amd import augment, image_processing as ip


def radiograph(h, w, seed):
    """Smooth anatomy-like gradients, sharp edges and sensor noise; grey replicated to RGB with small channel offsets."""
    rs = np.random.RandomState(seed)
    y = np.arange(h, dtype=np.float32)[:, None]
    x = np.arange(w, dtype=np.float32)[None, :]
    base = 120 + 90 * np.sin(x / (0.11 * w + 3)) * np.cos(y / (0.07 * h + 5)) + 40 * ((x / w - 0.5) ** 2 + (y / h - 0.5) ** 2 < 0.09)
    base = base + 60 * (np.abs(x - 0.3 * w) < 2) - 50 * (np.abs(y - 0.6 * h) < 1)
    img = base[:, :, None] + np.array([0, 3, -4], np.float32)[None, None, :] + rs.randint(-25, 26, size=(h, w, 3)).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def pillow_batch(imgs, params, size, gray, table):
    from PIL import Image
    out = []
    for im, (i, j, h, w, flip) in zip(imgs, params):
        pil = Image.fromarray(im).crop((j, i, j + w, i + h)).resize((size, size), resample=Image.BICUBIC)
        if gray:
            pil = pil.convert("L")
        if flip:
            pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
        t = torch.from_numpy(np.array(pil).reshape(size, size, -1)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)   # ToTensor
        mean, std = (torch.tensor(v, dtype=torch.float32).view(-1, 1, 1) for v in table)
        out.append(t.sub_(mean).div_(std))                                                                                   # Normalize
    return torch.stack(out, 0)


def windows(fn, warmup, iters, repeats, clock):
    """`repeats` windows of `iters` calls fn(k) after `warmup` calls; ms per call of each window.  clock: "device" (events around
    the window), "sync" (host clock, device synchronise at both ends) or "host" (host clock, no device work)."""
    k = 0
    for _ in range(warmup):
        fn(k)
        k += 1
    out = []
    for _ in range(repeats):
        if clock != "host":
            torch.cuda.synchronize()
        if clock == "device":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn(k)
            k += 1
        if clock == "device":
            e1.record()
        if clock != "host":
            torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters if clock == "device" else (time.perf_counter() - t0) / iters * 1e3)
    return out


def fmt(ws):
    return f"{float(np.median(ws)):8.3f} ms [{min(ws):.3f} .. {max(ws):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r09_augment.txt"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=2544)       # a MIMIC-CXR-sized radiograph
    ap.add_argument("--width", type=int, default=3056)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=600, help="calls per window of the batched resident arm (the others: a third)")
    ap.add_argument("--cpu-iters", type=int, default=1, help="batches per window of the Pillow arm")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs an MI355X: nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    imgs = [radiograph(a.height, a.width, 100 + n) for n in range(a.batch)]
    resident = [torch.from_numpy(im).to(dev) for im in imgs]
    n3 = max(1, a.iters // 3)
    lines = [f"augment_bench: batch {a.batch} of {a.height} x {a.width} x 3 uint8 radiographs, bicubic, {torch.cuda.get_device_name(0)}",
             f"{a.sets} seeded parameter sets drawn before timing, iteration k uses set k mod {a.sets}; every figure is the median "
             f"[min .. max] over {a.repeats} windows, per batch",
             f"CPU arm: {cpu_model()}, one Python thread (images one after the other), torch intra-op threads {torch.get_num_threads()}, "
             f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}; Pillow resamples single-threaded"]
    for name, make, size, stats in (("arm 1024^2 rgb", augment.arm_pretrain_augment, 1024, (ip.IMAGENET_DEFAULT_MEAN, ip.IMAGENET_DEFAULT_STD)),
                                    ("mae 1280^2 gray", augment.mae_pretrain_augment, 1280, ((0.5,), (0.5,)))):
        aug = make(size, device=dev, generator=torch.Generator().manual_seed(0))
        pool = [[aug.draw(a.height, a.width) for _ in imgs] for _ in range(a.sets)]
        at = lambda k: pool[k % a.sets]
        table = aug.byte_table.to(dev)
        gray = aug.grayscale
        singles = lambda k: [ip.preprocess_image(t, size, size, ip.BICUBIC, table, crop=p[:4], flip=p[4], gray=gray)
                             for t, p in zip(resident, at(k))]
        coeffs = lambda k: [(ip._coeffs_uncached(p[3], size, ip.BICUBIC), ip._coeffs_uncached(p[2], size, ip.BICUBIC)) for p in at(k)]
        want = pillow_batch(imgs, pool[0], size, gray, stats)
        same = [bool(torch.equal(aug(resident, params=pool[0]).cpu(), want)), bool(torch.equal(aug(imgs, params=pool[0]).cpu(), want)),
                bool(torch.equal(torch.stack(singles(0), 0).cpu(), want))]
        w_res = windows(lambda k: aug(resident, params=at(k)), 5, a.iters, a.repeats, "sync")
        w_dev = windows(lambda k: aug(resident, params=at(k)), 5, a.iters, a.repeats, "device")
        w_host = windows(lambda k: aug(imgs, params=at(k)), 3, n3, a.repeats, "sync")
        w_one = windows(singles, 3, n3, a.repeats, "sync")
        w_coef = windows(coeffs, 3, a.iters, a.repeats, "host")
        w_cpu = windows(lambda k: pillow_batch(imgs, at(k), size, gray, stats), 1, a.cpu_iters, a.repeats, "host")
        crop_px = float(np.mean([p[2] * p[3] for ps in pool for p in ps]))
        up = float(np.mean([sum(p[2] * a.width * 3 for p in ps) for ps in pool]))       # rows [i, i+h) of every image, full width
        extra = float(np.median(w_host)) - float(np.median(w_res))
        lines += [f"[{name}] mean crop {crop_px / 1e6:.2f} Mpixel of {a.height * a.width / 1e6:.2f}; set 0, device outputs == Pillow arm bit for bit: "
                  f"batched resident {same[0]}, batched from host {same[1]}, singles {same[2]}",
                  f"[{name}] batched, resident   : {fmt(w_res)}  host clock to a synchronise, {a.iters} calls / window",
                  f"[{name}]   same, device events: {fmt(w_dev)}  {a.iters} calls / window",
                  f"[{name}] batched, from host  : {fmt(w_host)}  host clock to a synchronise, {n3} calls / window; uploads {up / 1e6:.1f} MB / batch "
                  f"(pageable), {up / 1e6 / max(extra, 1e-9):.1f} GB/s over the {extra:.3f} ms it adds to the resident arm",
                  f"[{name}] {a.batch} singles, resident : {fmt(w_one)}  host clock to a synchronise, {n3} batches / window",
                  f"[{name}] coefficients alone  : {fmt(w_coef)}  host clock, {2 * a.batch} tables / batch, inside every device arm above",
                  f"[{name}] Pillow on the CPU   : {fmt(w_cpu)}  host clock, {a.cpu_iters} batch / window"]
        if not all(same):
            lines.append(f"[{name}] MISMATCH: the timings above are of wrong results")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
