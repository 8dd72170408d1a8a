"""Pre-training augmentation on the GPU: RandomResizedCrop -> [Grayscale] -> RandomHorizontalFlip -> ToTensor -> Normalize.

Mirror of the transform both pre-training scripts build per radiograph on the CPU:

    CXPMRG_Bench_MambaXray_VL/pretrain/main_pretrain.py:116-120          HD_Xray_Pretrain_MAE/pretrain/main.py:136-141
        RandomResizedCrop(input_size, scale=(0.2, 1.0), interpolation=3)     RandomResizedCrop(input_size, scale=(0.2, 1.0), interpolation=3)
        RandomHorizontalFlip()                                               Grayscale()
        ToTensor()                                                           RandomHorizontalFlip()
        Normalize(ImageNet mean / std)                                       ToTensor(); Normalize([0.5], [0.5])

The random DRAWS stay on the host (a CPU `torch.Generator`, a handful of scalars per image); the PIXELS never do: one batched
`mxvl_image_preprocess` call crops by pointer + pitch, resamples with Pillow's 8-bit arithmetic, mirrors, takes Pillow's luma
and looks every byte up in the ToTensor / Normalize table -- bit for bit what `Image.crop(box).resize(size, BICUBIC)`
[`.convert("L")`] `.transpose(FLIP_LEFT_RIGHT)` and the two tensor transforms give.  `random_resized_crop_params` restates
torchvision's `RandomResizedCrop.get_params` (same draws, same order); torchvision is not a dependency, and no parity of the
random STREAM with it is claimed.  There is no CPU path: the augmenter raises without a GPU.
"""
from __future__ import annotations

import math

import torch

from .image_processing import BICUBIC, BILINEAR, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, preprocess_batch


def random_resized_crop_params(height: int, width: int, scale=(0.2, 1.0), ratio=(3 / 4, 4 / 3), generator=None):
    """(i, j, h, w) of torchvision's RandomResizedCrop.get_params for a height x width image: ten tries of
    {area fraction ~ U(scale), aspect ratio ~ logU(ratio), w = round(sqrt(area * ar)), h = round(sqrt(area / ar))}, the first
    that fits the image gets a uniform top-left corner; otherwise the central crop clamped to the ratio range."""
    area = height * width
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,), generator=generator).item()
            j = torch.randint(0, width - w + 1, size=(1,), generator=generator).item()
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def to_tensor_normalize_table(mean, std) -> torch.Tensor:
    """(C, 256) float32: what byte v of channel c becomes under ToTensor (`.to(float32).div(255)`) and Normalize
    (`.sub_(mean).div_(std)` with float32 statistics) -- the torch expressions themselves, so a lookup IS those transforms."""
    if len(mean) != len(std) or len(mean) not in (1, 3):
        raise ValueError("mean / std must have 1 (grey) or 3 (RGB) entries")
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return torch.stack([v.sub(torch.tensor(m, dtype=torch.float32)).div(torch.tensor(s, dtype=torch.float32))
                        for m, s in zip(mean, std)], 0).contiguous()


class PretrainAugment:
    """Callable: a list of (H, W, 3) uint8 images (numpy arrays or tensors, any sizes) -> (B, 3 or 1, S, S) on the device,
    every image through its own random resized crop and flip.  `params` = [(i, j, h, w, flip), ...] replaces the draws;
    `last_params` holds what the last call used."""

    def __init__(self, input_size, scale=(0.2, 1.0), ratio=(3 / 4, 4 / 3), resample=BICUBIC, hflip=0.5, grayscale=False,
                 mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, device=None, dtype=torch.float32, generator=None):
        self.input_size, self.scale, self.ratio = int(input_size), tuple(scale), tuple(ratio)
        self.resample, self.hflip, self.grayscale = int(resample), float(hflip), bool(grayscale)
        if self.resample not in (BILINEAR, BICUBIC):
            raise ValueError(f"resample {resample}: only PIL BILINEAR (2) and BICUBIC (3) have a kernel")
        self.mean, self.std = tuple(mean), tuple(std)
        if len(self.mean) != (1 if self.grayscale else 3) or len(self.std) != len(self.mean):
            raise ValueError("mean / std need one entry per output channel (1 with grayscale, 3 without)")
        self.device = torch.device(device) if device is not None else None
        self.dtype, self.generator = dtype, generator
        self.byte_table = to_tensor_normalize_table(self.mean, self.std)
        self._table = None
        self.last_params = None

    def _device(self):
        if self.device is not None:
            if self.device.type != "cuda":
                raise RuntimeError("PretrainAugment needs an MI355X (no CPU path exists)")
            if self.device.index is None:       # "cuda" never equals a tensor's "cuda:0": pin the index once, keep the table
                self.device = torch.device("cuda", torch.cuda.current_device())
            return self.device
        if not torch.cuda.is_available():
            raise RuntimeError("PretrainAugment needs an MI355X (no CPU path exists)")
        return torch.device("cuda", torch.cuda.current_device())

    def draw(self, height: int, width: int):
        """One image's (i, j, h, w, flip): the crop's draws, then the flip's `torch.rand(1) < p`, as the transform chain runs them."""
        i, j, h, w = random_resized_crop_params(height, width, self.scale, self.ratio, self.generator)
        return i, j, h, w, bool(torch.rand(1, generator=self.generator) < self.hflip)

    def __call__(self, images, params=None):
        dev = self._device()
        images = list(images)
        if params is None:
            params = [self.draw(int(im.shape[0]), int(im.shape[1])) for im in images]
        params = [(int(i), int(j), int(h), int(w), bool(f)) for i, j, h, w, f in params]
        if len(params) != len(images):
            raise ValueError("params needs one (i, j, h, w, flip) per image")
        if self._table is None or self._table.device != dev:
            self._table = self.byte_table.to(dev)
        self.last_params = params
        return preprocess_batch(images, [p[:4] for p in params], [p[4] for p in params], self.input_size, self.resample,
                                self._table, gray=self.grayscale, dtype=self.dtype)


def arm_pretrain_augment(input_size, **kw) -> PretrainAugment:
    """The transform of CXPMRG_Bench_MambaXray_VL/pretrain/main_pretrain.py:116-120 (ARM pre-training, 3 channels)."""
    return PretrainAugment(input_size, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, grayscale=False, **kw)


def mae_pretrain_augment(input_size, **kw) -> PretrainAugment:
    """The transform of HD_Xray_Pretrain_MAE/pretrain/main.py:136-141 (MAE pre-training, `Grayscale()` -> 1 channel)."""
    return PretrainAugment(input_size, mean=(0.5,), std=(0.5,), grayscale=True, **kw)
