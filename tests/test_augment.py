"""Pre-training augmentation on the device (RandomResizedCrop -> [Grayscale] -> RandomHorizontalFlip -> ToTensor -> Normalize of
CXPMRG_Bench_MambaXray_VL/pretrain/main_pretrain.py:116-120 and HD_Xray_Pretrain_MAE/pretrain/main.py:136-141) through the crop /
flip / grey / batch fields of mxvl_image_desc.  Everything is bit-exact against ONE test-local reference:
    oracle.image_ref.resize_u8 on the cropped array, then Pillow's luma formula, then the mirror, then the byte table
  CPU : that reference against live Pillow (crop -> resize -> [convert("L")] -> transpose); the crop-parameter rule against an
        independent restatement and a hand-derived fallback; the byte table against the torch ToTensor / Normalize expressions; the
        new ABI fields and their argument checks (fake pointers, nothing launched).
  GPU : single calls with a row pitch at every alignment, flips, grey, half outputs, one batched call against the single calls, and
        the seeded augmenter end to end."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, synthetic_xray


# ---------------------------------------------------------------------------------------------------------------------
# the test-local reference
# ---------------------------------------------------------------------------------------------------------------------
def ref_bytes(img, crop, out_h, out_w, kind, flip=False, gray=False):
    """(out_h, out_w, 3 or 1) uint8: crop, THEN resize (taps clamp at the crop's border), luma on the bytes, mirror."""
    from oracle import image_ref as ir
    i, j, h, w = crop
    r = ir.resize_u8(np.ascontiguousarray(img[i:i + h, j:j + w]), out_h, out_w, kind)
    if gray:
        r32 = r.astype(np.int64)
        r = ((19595 * r32[..., 0] + 38470 * r32[..., 1] + 7471 * r32[..., 2] + 0x8000) >> 16).astype(np.uint8)[..., None]
    if flip:
        r = r[:, ::-1]
    return np.ascontiguousarray(r)


def ref_values(img, crop, out_h, out_w, kind, table, flip=False, gray=False):
    """(C, out_h, out_w) float32 through a (C, 256) float32 numpy table."""
    r = ref_bytes(img, crop, out_h, out_w, kind, flip, gray)
    return np.stack([table[c][r[:, :, c]] for c in range(r.shape[2])], 0)


def _table(mean, std):
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return torch.stack([v.sub(torch.tensor(m, dtype=torch.float32)).div(torch.tensor(s, dtype=torch.float32)) for m, s in zip(mean, std)], 0)


IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
RGB_TABLE = _table(*IMAGENET)
GRAY_TABLE = _table((0.5,), (0.5,))


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def _restated_params(height, width, scale, ratio, g):
    """torchvision's published get_params rule, written a second time for the draw-order check."""
    lo, hi = torch.log(torch.tensor(ratio))
    for _ in range(10):
        frac = torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
        ar = torch.exp(torch.empty(1).uniform_(lo, hi, generator=g)).item()
        w, h = int(round(math.sqrt(height * width * frac * ar))), int(round(math.sqrt(height * width * frac / ar)))
        if 0 < w <= width and 0 < h <= height:
            i = int(torch.randint(0, height - h + 1, (1,), generator=g))
            return i, int(torch.randint(0, width - w + 1, (1,), generator=g)), h, w
    if width / height < min(ratio):
        w, h = width, int(round(width / min(ratio)))
    elif width / height > max(ratio):
        h, w = height, int(round(height * max(ratio)))
    else:
        h, w = height, width
    return (height - h) // 2, (width - w) // 2, h, w


def test_crop_params_rule():
    from medical_image_analysis_amd.augment import PretrainAugment, random_resized_crop_params as rrc
    shapes = [(97, 83), (1024, 1024), (2544, 3056), (7, 300), (300, 7), (1, 1), (50, 1000)]
    for seed, (H, W) in enumerate(shapes):
        g1, g2, g3 = (torch.Generator().manual_seed(seed) for _ in range(3))
        a = [rrc(H, W, generator=g1) for _ in range(20)]
        assert a == [rrc(H, W, generator=g2) for _ in range(20)]                            # same seed, same parameters
        assert a == [_restated_params(H, W, (0.2, 1.0), (3 / 4, 4 / 3), g3) for _ in range(20)]   # same draws in the same order
        assert len(set(a)) > 1 or not 3 / 4 <= W / H <= 4 / 3 or (H, W) == (1, 1)   # elongated images mostly take the fallback
        for i, j, h, w in a:
            assert 0 <= i and 0 <= j and 0 < h and 0 < w and i + h <= H and j + w <= W, (H, W, i, j, h, w)
    # other scale / ratio arguments take the same path
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    assert [rrc(200, 300, (0.5, 0.6), (1.0, 2.0), g1) for _ in range(10)] == \
        [_restated_params(200, 300, (0.5, 0.6), (1.0, 2.0), g2) for _ in range(10)]
    # fallback, derived by hand: area 2000 and ratio >= 3/4 need w >= sqrt(1500) = 38.7 > 10, so no try is accepted; width/height =
    # 0.05 < 3/4 -> w = 10, h = round(10 / 0.75) = 13, centred: i = (200 - 13) // 2 = 93, j = 0
    assert rrc(200, 10, scale=(1, 1), generator=torch.Generator().manual_seed(0)) == (93, 0, 13, 10)
    assert rrc(10, 200, scale=(1, 1), generator=torch.Generator().manual_seed(0)) == (0, 93, 10, 13)   # h = 10, w = round(13.33)
    # the augmenter draws the crop, then the flip (`torch.rand(1) < p`), image after image
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    aug = PretrainAugment(32, generator=g1)
    want = []
    for _ in range(6):
        box = _restated_params(120, 90, (0.2, 1.0), (3 / 4, 4 / 3), g2)
        want.append(box + (bool(torch.rand(1, generator=g2) < 0.5),))
    got = [aug.draw(120, 90) for _ in range(6)]
    assert got == want and {p[4] for p in got} == {True, False}


def test_byte_table_is_the_torch_to_tensor_normalize_expression():
    from medical_image_analysis_amd import augment
    arm, mae = augment.arm_pretrain_augment(64), augment.mae_pretrain_augment(64)
    assert arm.byte_table.shape == (3, 256) and arm.byte_table.dtype == torch.float32 and not arm.grayscale
    assert mae.byte_table.shape == (1, 256) and mae.byte_table.dtype == torch.float32 and mae.grayscale
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)               # ToTensor
    for aug, (mean, std) in ((arm, IMAGENET), (mae, ((0.5,), (0.5,)))):
        for c, (m, s) in enumerate(zip(mean, std)):
            want = v.clone().sub_(torch.as_tensor(m, dtype=torch.float32)).div_(torch.as_tensor(s, dtype=torch.float32))   # Normalize
            assert torch.equal(aug.byte_table[c], want), c


def test_reference_equals_live_pillow():
    """crop -> resize -> [convert("L")] -> transpose(FLIP_LEFT_RIGHT) with the Pillow that is installed; and resize(box=...) is a
    DIFFERENT operation (it reads pixels outside the box), which is why the contract is crop, then resize."""
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(4)
    differs = 0
    for n in range(12):
        H, W = (int(v) for v in rs.randint(8, 120, size=2))
        h, w = int(rs.randint(1, H + 1)), int(rs.randint(1, W + 1))
        i, j = int(rs.randint(0, H - h + 1)), int(rs.randint(0, W - w + 1))
        oh, ow = (int(v) for v in rs.randint(1, 70, size=2))
        kind, flip, gray = (2, 3)[n % 2], bool(n & 2), bool(n & 4)
        img = rs.randint(0, 256, (H, W, 3), dtype=np.uint8)
        pil = Image.fromarray(img).crop((j, i, j + w, i + h)).resize((ow, oh), resample=kind)
        if gray:
            pil = pil.convert("L")
        if flip:
            pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
        want = np.array(pil).reshape(oh, ow, -1)
        assert np.array_equal(ref_bytes(img, (i, j, h, w), oh, ow, kind, flip, gray), want), (n, H, W, i, j, h, w, oh, ow)
        if (h, w) != (H, W):
            boxed = np.array(Image.fromarray(img).resize((ow, oh), resample=kind, box=(j, i, j + w, i + h)))
            differs += not np.array_equal(boxed, ref_bytes(img, (i, j, h, w), oh, ow, kind))
    assert differs > 0


def _header():
    return open(os.path.join(ROOT, "include", "mxvl.h")).read()


def _struct_fields(name):
    m = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", _header(), re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            decl = re.sub(r"^(const\s+)?(void|int32_t|int64_t)\s*", "", decl)
            names += [n.strip().lstrip("*").strip() for n in decl.split(",")]
    return names


def test_abi_carries_the_new_fields_inside_the_old_surface():
    from medical_image_analysis_amd import _abi
    desc = _struct_fields("mxvl_image_desc")
    assert desc == [f[0] for f in _abi.ImageDesc._fields_]
    assert desc[7] == "flags" and desc[-4:] == ["src_pitch", "batch", "reserved1", "items"] and "reserved0" not in desc
    assert _struct_fields("mxvl_image_item") == [f[0] for f in _abi.ImageItem._fields_]
    assert ctypes.sizeof(_abi.ImageItem) == 80 and ctypes.sizeof(_abi.ImageDesc) == 120
    assert _abi.ImageDesc.src_pitch.offset == 96 and _abi.ImageDesc.batch.offset == 104 and _abi.ImageDesc.items.offset == 112
    assert re.search(r"MXVL_IMG_FLIP_H\s*=\s*1\b", _header()) and re.search(r"MXVL_IMG_GRAY\s*=\s*2\b", _header())
    assert (_abi.MXVL_IMG_FLIP_H, _abi.MXVL_IMG_GRAY) == (1, 2)
    # no new export, no version bump
    assert _abi.ABI_VERSION == 13 and _abi.load().mxvl_abi_version() == 13
    assert len(set(re.findall(r"\b(mxvl_\w+)\s*\([^)]*\bvoid\s*\*\s*hip_stream\s*\)\s*;", _header()))) == 43


def _fake_desc():
    """Every check passes up to the launch -- so each test below breaks exactly one thing and never sends this one."""
    from medical_image_analysis_amd import _abi
    d = _abi.ImageDesc()
    d.in_h, d.in_w, d.out_h, d.out_w, d.ksize_h, d.ksize_v, d.out_dtype = 8, 8, 4, 4, 5, 5, _abi.MXVL_F32
    d.src = d.bounds_h = d.kk_h = d.bounds_v = d.kk_v = d.lut = d.tmp = d.out = 64      # fake non-null pointers, never dereferenced
    return d


def test_new_fields_are_checked_before_any_launch():
    from medical_image_analysis_amd import _abi
    call = lambda d: _abi.load().mxvl_image_preprocess(ctypes.byref(d), None)
    NULL, SHAPE, STRIDE, UNSUPPORTED = -1, -3, -5, -7
    assert (_abi.STATUS[NULL], _abi.STATUS[SHAPE], _abi.STATUS[STRIDE], _abi.STATUS[UNSUPPORTED]) == \
        ("MXVL_ERR_NULL", "MXVL_ERR_SHAPE", "MXVL_ERR_STRIDE", "MXVL_ERR_UNSUPPORTED")
    for bad in (4, 8, 1 | 4, 1 << 30, -1):
        d = _fake_desc()
        d.flags = bad
        assert call(d) == UNSUPPORTED, bad
    for pitch in (23, 1, -24):                          # a row of 8 pixels is 24 bytes
        d = _fake_desc()
        d.src_pitch = pitch
        assert call(d) == STRIDE, pitch
    d = _fake_desc()
    d.batch = -1
    assert call(d) == SHAPE
    d = _fake_desc()
    d.batch = 3                                         # items NULL
    assert call(d) == NULL
    d = _fake_desc()
    d.batch, d.items, d.lut = 3, 64, None
    assert call(d) == NULL
    d = _fake_desc()
    d.batch, d.items, d.in_w = 3, 64, 30000             # the LDS row limit holds for the widest crop of a batch
    assert call(d) == UNSUPPORTED
    d = _fake_desc()
    d.src = None                                        # and the old checks are where they were
    assert call(d) == NULL


def test_augmenter_has_no_cpu_path(monkeypatch):
    from medical_image_analysis_amd import augment, image_processing as ip
    img = synthetic_xray(20, 24, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        augment.arm_pretrain_augment(8, device="cpu")([img])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        augment.mae_pretrain_augment(8)([img])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ip.preprocess_batch([img], [None], [False], 8, 3, RGB_TABLE)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ip.preprocess_image(torch.from_numpy(img), 8, 8, 3, RGB_TABLE, crop=(0, 0, 4, 4))


def test_raw_image_folder_and_collate(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from medical_image_analysis_amd.data_pipeline import RawImageFolder, collate_images
    a, b = synthetic_xray(20, 30, 1), synthetic_xray(25, 17, 2)
    (tmp_path / "sub").mkdir()
    Image.fromarray(a).save(tmp_path / "b.png")
    Image.fromarray(b[:, :, 0]).save(tmp_path / "sub" / "a.png")           # a grey file comes back as RGB
    (tmp_path / "notes.txt").write_text("x")
    ds = RawImageFolder(str(tmp_path))
    assert len(ds) == 2 and np.array_equal(ds[0], a) and np.array_equal(ds[1], np.repeat(b[:, :, :1], 3, 2))
    batch = collate_images([ds[0], ds[1]])
    assert isinstance(batch, list) and [x.shape for x in batch] == [(20, 30, 3), (25, 17, 3)]
    with pytest.raises(FileNotFoundError):
        RawImageFolder(str(tmp_path / "sub" / "none"))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
SRC_H, SRC_W = 97, 83


def _source():
    return np.random.RandomState(7).randint(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8)      # R != G != B everywhere that matters


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("S", [7, 32, 33])
def test_single_image_with_pitch(S, kind):
    from medical_image_analysis_amd import image_processing as ip
    dev = torch.device("cuda:0")
    img = _source()
    t, table = torch.from_numpy(img).to(dev), RGB_TABLE.to(dev)
    lut = RGB_TABLE.numpy()
    crops = [(0, 0, SRC_H, SRC_W), (5, 0, 1, SRC_W), (2, 3, 90, 80)]                        # full image, one row, the downscale for S = 7
    for j in range(4):                                                                      # every alignment of the crop's first byte
        crops += [(3 + j, j, 1, 1), (0, j, SRC_H, 1), (40, j, 5, 9), (10 + j, j, S, 20 + j), (96, 82 - j, 1, 1 + j)]
    for crop in crops:
        got = ip.preprocess_image(t, S, S, kind, table, crop=crop)
        assert got.shape == (3, S, S) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), ref_values(img, crop, S, S, kind, lut)), (crop, S, kind)
    # crop=None is the old call; the full-image crop computes the same through the pitch path
    assert torch.equal(ip.preprocess_image(t, S, S, kind, table), ip.preprocess_image(t, S, S, kind, table, crop=(0, 0, SRC_H, SRC_W)))
    with pytest.raises(ValueError):
        ip.preprocess_image(t, S, S, kind, table, crop=(90, 0, 8, 8))


@pytest.mark.gpu
def test_flip_at_odd_and_even_width():
    from medical_image_analysis_amd import image_processing as ip
    dev = torch.device("cuda:0")
    img = _source()
    t, table = torch.from_numpy(img).to(dev), RGB_TABLE.to(dev)
    for oh, ow, crop in [(7, 33, (1, 2, 60, 50)), (9, 32, (0, 1, 97, 40)), (5, 1, (3, 3, 20, 20)), (4, 2, None), (33, 300, (0, 0, 97, 83))]:
        box = crop or (0, 0, SRC_H, SRC_W)
        got = ip.preprocess_image(t, oh, ow, 3, table, crop=crop, flip=True).cpu().numpy()
        assert np.array_equal(got, ref_values(img, box, oh, ow, 3, RGB_TABLE.numpy(), flip=True)), (oh, ow, crop)
        plain = ip.preprocess_image(t, oh, ow, 3, table, crop=crop).cpu().numpy()
        assert np.array_equal(got, plain[:, :, ::-1])


@pytest.mark.gpu
def test_gray_and_half_outputs():
    from medical_image_analysis_amd import image_processing as ip
    dev = torch.device("cuda:0")
    img = _source()
    t, table = torch.from_numpy(img).to(dev), GRAY_TABLE.to(dev)           # a (1, 256) table: only row 0 may be read
    for S, crop, flip in [(32, (4, 1, 70, 61), False), (33, (0, 2, 97, 30), True), (7, None, False)]:
        box = crop or (0, 0, SRC_H, SRC_W)
        ref = ref_values(img, box, S, S, 3, GRAY_TABLE.numpy(), flip=flip, gray=True)
        got = ip.preprocess_image(t, S, S, 3, table, crop=crop, flip=flip, gray=True)
        assert got.shape == (1, S, S) and np.array_equal(got.cpu().numpy(), ref)
        for dtype in (torch.float16, torch.bfloat16):
            half = ip.preprocess_image(t, S, S, 3, table, crop=crop, flip=flip, gray=True, dtype=dtype)
            assert half.dtype == dtype and torch.equal(half.cpu(), torch.from_numpy(ref).to(dtype))     # = casting the fp32 result
    for dtype in (torch.float16, torch.bfloat16):                          # the RGB path with a crop, too
        ref = ref_values(img, (4, 1, 70, 61), 32, 32, 2, RGB_TABLE.numpy(), flip=True)
        half = ip.preprocess_image(t, 32, 32, 2, RGB_TABLE.to(dev), crop=(4, 1, 70, 61), flip=True, dtype=dtype)
        assert torch.equal(half.cpu(), torch.from_numpy(ref).to(dtype))
    with pytest.raises(RuntimeError):
        ip.preprocess_image(t, 8, 8, 3, table)                             # a one-row table cannot serve three channels


BATCH_SHAPES = [(97, 83), (40, 120), (131, 31), (64, 64), (9, 300)]
BATCH_CROPS = [(10, 3, 50, 41), None, (0, 1, 131, 30), (16, 16, 33, 33), (2, 250, 5, 49)]
BATCH_FLIPS = [True, False, True, False, True]


@pytest.mark.gpu
@pytest.mark.parametrize("gray", [False, True])
def test_batched_call_equals_single_calls_and_reference(gray):
    from medical_image_analysis_amd import image_processing as ip
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(11)
    imgs = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in BATCH_SHAPES]
    cpu_table = GRAY_TABLE if gray else RGB_TABLE
    table, S, C = cpu_table.to(dev), 33, (1 if gray else 3)
    boxes = [c or (0, 0, im.shape[0], im.shape[1]) for c, im in zip(BATCH_CROPS, imgs)]
    ref = np.stack([ref_values(im, b, S, S, 3, cpu_table.numpy(), flip=f, gray=gray) for im, b, f in zip(imgs, boxes, BATCH_FLIPS)], 0)
    # host arrays (only the crop's rows are uploaded), device tensors (read in place), and a mixture
    mixed = [torch.from_numpy(im).to(dev) if n % 2 else (torch.from_numpy(im) if n == 2 else im) for n, im in enumerate(imgs)]
    for images in (imgs, [torch.from_numpy(im).to(dev) for im in imgs], mixed):
        got = ip.preprocess_batch(images, BATCH_CROPS, BATCH_FLIPS, S, 3, table, gray=gray)
        assert got.shape == (5, C, S, S) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), ref)
    singles = torch.stack([ip.preprocess_image(torch.from_numpy(im).to(dev), S, S, 3, table, crop=c, flip=f, gray=gray)
                           for im, c, f in zip(imgs, BATCH_CROPS, BATCH_FLIPS)], 0)
    assert torch.equal(got, singles)
    for n in (0, 4):                                                        # a batch of one, rectangular output, bilinear, bf16
        one = ip.preprocess_batch([imgs[n]], [BATCH_CROPS[n]], [BATCH_FLIPS[n]], (7, 32), 2, table, gray=gray, dtype=torch.bfloat16)
        want = ref_values(imgs[n], boxes[n], 7, 32, 2, cpu_table.numpy(), flip=BATCH_FLIPS[n], gray=gray)
        assert one.shape == (1, C, 7, 32) and torch.equal(one.cpu()[0], torch.from_numpy(want).to(torch.bfloat16))
    with pytest.raises(ValueError):
        ip.preprocess_batch(imgs, BATCH_CROPS[:4], BATCH_FLIPS, S, 3, table, gray=gray)
    with pytest.raises(ValueError):
        ip.preprocess_batch(imgs[:1], [(0, 0, 98, 83)], [False], S, 3, table, gray=gray)


@pytest.mark.gpu
def test_row_limit_is_the_crops_not_the_sources():
    from medical_image_analysis_amd import image_processing as ip
    dev = torch.device("cuda:0")
    wide = np.random.RandomState(2).randint(0, 256, (4, 30000, 3), dtype=np.uint8)
    table = RGB_TABLE.to(dev)
    crop = (1, 29899, 3, 100)
    ref = ref_values(wide, crop, 7, 33, 3, RGB_TABLE.numpy(), flip=True)
    t = torch.from_numpy(wide).to(dev)
    assert np.array_equal(ip.preprocess_image(t, 7, 33, 3, table, crop=crop, flip=True).cpu().numpy(), ref)
    small = synthetic_xray(20, 24, 3)
    got = ip.preprocess_batch([wide, small, t], [crop, None, crop], [True, False, True], (7, 33), 3, table)
    assert np.array_equal(got[0].cpu().numpy(), ref) and np.array_equal(got[2].cpu().numpy(), ref)
    assert np.array_equal(got[1].cpu().numpy(), ref_values(small, (0, 0, 20, 24), 7, 33, 3, RGB_TABLE.numpy()))
    with pytest.raises(RuntimeError, match="MXVL_ERR_UNSUPPORTED"):
        ip.preprocess_image(t, 7, 33, 3, table)                             # the dense 30 000-pixel row still has no kernel
    with pytest.raises(RuntimeError, match="MXVL_ERR_UNSUPPORTED"):
        ip.preprocess_batch([wide, small], [None, None], [False, False], (7, 33), 3, table)


@pytest.mark.gpu
@pytest.mark.parametrize("factory", ["arm_pretrain_augment", "mae_pretrain_augment"])
def test_augmenter_end_to_end(factory):
    from medical_image_analysis_amd import augment
    make = getattr(augment, factory)
    gray = factory.startswith("mae")
    imgs = [synthetic_xray(h, w, 20 + n) for n, (h, w) in enumerate([(97, 83), (64, 150), (200, 120), (33, 33), (90, 91), (128, 70)])]
    imgs[1], imgs[4] = torch.from_numpy(imgs[1]), torch.from_numpy(imgs[4]).to("cuda:0")     # arrays and tensors, host and device
    arrays = [im.cpu().numpy() if isinstance(im, torch.Tensor) else im for im in imgs]
    S = 32
    aug = make(S, generator=torch.Generator().manual_seed(5))
    out = aug(imgs)
    params = list(aug.last_params)
    assert out.is_cuda and out.shape == (6, 1 if gray else 3, S, S) and out.dtype == torch.float32 and len(params) == 6
    table = aug.byte_table.numpy()
    ref = np.stack([ref_values(a, p[:4], S, S, 3, table, flip=p[4], gray=gray) for a, p in zip(arrays, params)], 0)
    assert np.array_equal(out.cpu().numpy(), ref)
    again = make(S, generator=torch.Generator().manual_seed(5))
    assert torch.equal(again(imgs), out) and again.last_params == params                     # the same seed repeats
    other = make(S, generator=torch.Generator().manual_seed(6))
    assert not torch.equal(other(imgs), out) and other.last_params != params                 # another seed differs
    # random boxes do not come back: they leave the host coefficient cache alone; and a device given without an index keeps its table
    from medical_image_analysis_amd import image_processing as ip
    cached = ip._coeffs_host.cache_info().currsize
    loose = make(S, device="cuda", generator=torch.Generator().manual_seed(5))
    assert torch.equal(loose(imgs), out)
    table_on_device = loose._table
    assert torch.equal(loose(imgs, params=params), out) and loose._table is table_on_device
    assert ip._coeffs_host.cache_info().currsize == cached
    forced = [(0, 0, a.shape[0], a.shape[1], n % 2 == 0) for n, a in enumerate(arrays)]      # params override the draws
    got = make(S, dtype=torch.float16)(imgs, params=forced)
    want = np.stack([ref_values(a, p[:4], S, S, 3, table, flip=p[4], gray=gray) for a, p in zip(arrays, forced)], 0)
    assert torch.equal(got.cpu(), torch.from_numpy(want).to(torch.float16))
