"""csrc/cross_scan.hip, bit for bit: every launch path launch_cross() can choose (several planes per workgroup with and without a ragged
last group, V = 4 / V = 1 by shape and by an unaligned base, the d == 1 arms of cross_div, the 32 x 32 tiles with ragged edges), scan
and merge, in fp32 / bf16 / fp16.

Both entries are index work plus, in the merge, the reference's three tensor adds in the io dtype, so the reference is exact: the scan is
flatten, transpose-flatten and two flips, the merge is (ys0 + flip(ys2)) + transpose(ys1 + flip(ys3)) as torch adds on the CPU, and every
comparison is of bit patterns.  No tolerance appears in this file.

Every tensor a kernel touches is a view into a larger buffer pre-filled with a NaN bit pattern (fp64_bounds._Buf): a store outside the
view changes the pattern, a load outside it reaches an output as NaN, and an element the kernel never wrote stays NaN.  Launches go
through _abi.launch with the test's own pointers.  The CPU tests (no `gpu` mark) restate cross_planes_per_wg(), the flat / V / tiles
choice and cross_div(), prove that the case list reaches every configuration it names and that the magic-number quotient equals integer
division over every index a case can form, and hold the reference against the oracle.

Out of scope: the `plane += gridDim.y` loop of the two tile kernels.  It takes a second trip only with more than 65 535 planes on the tile
path, i.e. planes too large for the LDS (more than 15 360 fp32 elements each): at least 4 GB of input."""
import zlib

import pytest
import torch

from fp64_bounds import _assert_buffers, _Buf, _ptr
from medical_image_analysis_amd import _abi
from oracle import oracle as orc

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALF = DTYPES[1:]
_DT = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
_ESZ = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}
gpu = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------------
def _scan_ref(x):
    """(B, C, H, W) -> (B, 4, C, H W): row-major, column-major and their reversals"""
    a, t = x.flatten(2), x.transpose(2, 3).flatten(2)
    return torch.stack([a, t, a.flip(-1), t.flip(-1)], 1)


def _merge_ref(ys, H, W):
    """(B, 4, C, H W) -> (B, C, H W): three tensor adds, each rounded to ys.dtype"""
    B, _, C, L = ys.shape
    a = ys[:, 0] + ys[:, 2].flip(-1)
    t = ys[:, 1] + ys[:, 3].flip(-1)
    return a + t.reshape(B, C, W, H).transpose(2, 3).reshape(B, C, L)


# ---- 2. cross_planes_per_wg(), launch_cross() and cross_div() restated -------------------------------------------------------------------
def _planes_per_wg(merge, B, C, L, esz):
    plane = L * esz * (4 if merge else 1)
    if plane > 60 * 1024:
        return 0
    P = min(max((48 if merge else 16) * 1024 // plane, 1), 16)
    while P > 1 and B * -(-C // P) < 1024:
        P -= 1
    return P


def _geometry(merge, B, C, H, W, esz, aligned=True):
    """-> (path, P, V, workgroups per batch element, planes of the last one); P = V = 0 on the tiles"""
    L = H * W
    P = _planes_per_wg(merge, B, C, L, esz)
    if P > 0 and B <= 65535 and P * L * L < 1 << 32:
        groups = -(-C // P)
        return "flat", P, 4 if L % 4 == 0 and aligned else 1, groups, C - (groups - 1) * P
    return "tiles", 0, 0, (-(-W // 32)) * (-(-H // 32)), 0


def _cross_div(n, d):
    """cross_div(n, d, floor(2^32 / d) + 1): the high word of the 32 x 32-bit product; d == 1 has no such 32-bit word and returns n"""
    if d == 1:
        return n
    mag = (1 << 32) // d + 1
    assert mag < 1 << 32
    return (n * mag) >> 32


def _aligned(dtype, shift):
    return shift * _ESZ[dtype] % 16 == 0


class Case:
    def __init__(self, B, C, H, W, dtypes=DTYPES, shifts=()):
        self.shape, self.dtypes, self.shifts = (B, C, H, W), dtypes, shifts
        self.id = f"B{B}C{C}H{H}W{W}"


CASES = [
    Case(4, 4099, 7, 7),                                          # P 16, V 1, last group of 3
    Case(2, 1031, 14, 14, shifts=(1, 2)),                         # P 2, V 4, last group of 1; shifted: V 1 by alignment at P 2
    Case(2, 3000, 14, 14),                                        # P 5, V 4, no ragged group
    Case(3, 1366, 2, 2),                                          # P 4, LV 1: the d == 1 arm of the plane quotient, last group of 2
    Case(2, 2050, 1, 1),                                          # P 4, L 1: all three d == 1 arms
    Case(1, 2051, 1, 6), Case(1, 2051, 5, 1),                     # H 1 / W 1 at P 2, ragged
    Case(3, 700, 28, 28),                                         # P 2 at a real stage size
    Case(8, 256, 56, 56, dtypes=HALF),                            # 16-bit: P 2 scan, P 1 merge
    Case(1, 2, 123, 125),                                         # fp32: tiles, ragged both ways; 16-bit: flat V 1 scan, tiles merge
    Case(1, 1, 200, 200),                                         # tiles for every dtype, ragged last tile
    Case(1, 2, 128, 96),                                          # flat V 4 scan at P 1, tiles merge
]
RUNS = [(c, dt, 0) for c in CASES for dt in c.dtypes] + [(c, dt, s) for c in CASES for dt in c.dtypes for s in c.shifts]

# what the case list has to contain: name -> (dtypes it is wanted in, predicate over (shape, shift, scan geometry, merge geometry))
_both = lambda s, m, **kw: all(all(dict(zip(("path", "P", "V", "groups", "last"), g))[k] == v for k, v in kw.items()) for g in (s, m))
NEED = {
    "P 16, V 1, last group of 3": (DTYPES, lambda sh, sf, s, m: sf == 0 and _both(s, m, path="flat", P=16, V=1, last=3)),
    "P 2, V 4, last group of 1": (DTYPES, lambda sh, sf, s, m: sf == 0 and _both(s, m, path="flat", P=2, V=4, last=1)),
    "P 5, V 4, no ragged group": (DTYPES, lambda sh, sf, s, m: _both(s, m, path="flat", P=5, V=4, last=5)),
    "P 4, LV 1, ragged": (DTYPES, lambda sh, sf, s, m: sh[2] * sh[3] == 4 and _both(s, m, path="flat", P=4, V=4) and s[4] < 4),
    "P 4, L 1": (DTYPES, lambda sh, sf, s, m: sh[2] * sh[3] == 1 and _both(s, m, path="flat", P=4, V=1)),
    "H 1, P 2, ragged": (DTYPES, lambda sh, sf, s, m: sh[2] == 1 and sh[3] > 1 and _both(s, m, path="flat", P=2, last=1)),
    "W 1, P 2, ragged": (DTYPES, lambda sh, sf, s, m: sh[3] == 1 and sh[2] > 1 and _both(s, m, path="flat", P=2, last=1)),
    "P 2 at 28 x 28": (DTYPES, lambda sh, sf, s, m: sh[2:] == (28, 28) and _both(s, m, path="flat", P=2, V=4)),
    "P 2 scan, P 1 merge": (HALF, lambda sh, sf, s, m: s[:2] == ("flat", 2) and m[:2] == ("flat", 1)),
    "tiles, ragged both ways, H != W": (DTYPES[:1], lambda sh, sf, s, m: _both(s, m, path="tiles") and sh[2] != sh[3] and sh[2] % 32 and sh[3] % 32),
    "flat V 1 scan, tiles merge": (HALF, lambda sh, sf, s, m: s[:3] == ("flat", 1, 1) and m[0] == "tiles"),
    "tiles in every dtype, ragged last tile": (DTYPES, lambda sh, sf, s, m: _both(s, m, path="tiles") and sh[2] == sh[3] and sh[2] % 32),
    "flat V 4 scan, tiles merge": (DTYPES, lambda sh, sf, s, m: s[:3] == ("flat", 1, 4) and m[0] == "tiles"),
    "V 1 by a base 1 element off, P 2": (DTYPES, lambda sh, sf, s, m: sf == 1 and sh[2] * sh[3] % 4 == 0 and _both(s, m, path="flat", P=2, V=1)),
    "V 1 by a base 2 elements off, P 2": (DTYPES, lambda sh, sf, s, m: sf == 2 and sh[2] * sh[3] % 4 == 0 and _both(s, m, path="flat", P=2, V=1)),
}


def _missing(runs):
    """the configurations of NEED that `runs` does not reach, as 'name (dtype)'"""
    seen = {k: set() for k in NEED}
    for c, dt, shift in runs:
        s, m = (_geometry(merge, *c.shape, _ESZ[dt], _aligned(dt, shift)) for merge in (False, True))
        for k, (_, pred) in NEED.items():
            if pred(c.shape, shift, s, m):
                seen[k].add(dt)
    return [f"{k} ({_DT[dt]})" for k, (dts, _) in NEED.items() for dt in dts if dt not in seen[k]]


# ---- CPU: the case list reaches what it says it reaches --------------------------------------------------------------------------------
def test_cases_cover_every_launch_path():
    assert _missing(RUNS) == [], "not reached"
    for c in CASES:                                               # and every row is needed: without it something is named
        rest = [r for r in RUNS if r[0] is not c]
        assert _missing(rest), f"{c.id} reaches nothing of its own"
    for s in CASES[1].shifts:
        assert _missing([r for r in RUNS if r[2] != s]) == [f"V 1 by a base {s} element{'s' * (s > 1)} off, P 2 ({_DT[dt]})" for dt in DTYPES]
    # the rows of the table, as the launcher sees them: (path, P, V, workgroups, planes of the last workgroup)
    for esz in (4, 2):
        for merge in (False, True):
            geo = lambda *shape, aligned=True: _geometry(merge, *shape, esz, aligned)
            assert geo(4, 4099, 7, 7) == ("flat", 16, 1, 257, 3)
            assert geo(2, 1031, 14, 14) == ("flat", 2, 4, 516, 1) and geo(2, 1031, 14, 14, aligned=False) == ("flat", 2, 1, 516, 1)
            assert geo(2, 3000, 14, 14) == ("flat", 5, 4, 600, 5)
            assert geo(3, 1366, 2, 2) == ("flat", 4, 4, 342, 2)
            assert geo(2, 2050, 1, 1) == ("flat", 4, 1, 513, 2)
            assert geo(1, 2051, 1, 6) == geo(1, 2051, 5, 1) == ("flat", 2, 1, 1026, 1)
            assert geo(3, 700, 28, 28) == ("flat", 2, 4, 350, 2)
            assert geo(1, 1, 200, 200) == ("tiles", 0, 0, 49, 0)
    assert _geometry(False, 8, 256, 56, 56, 2) == ("flat", 2, 4, 128, 2) and _geometry(True, 8, 256, 56, 56, 2) == ("flat", 1, 4, 256, 1)
    assert _geometry(False, 8, 256, 56, 56, 4)[1] == 1, "in fp32 the same shape keeps one plane per workgroup"
    assert _geometry(False, 1, 2, 123, 125, 4)[0] == _geometry(True, 1, 2, 123, 125, 4)[0] == _geometry(True, 1, 2, 123, 125, 2)[0] == "tiles"
    assert _geometry(False, 1, 2, 123, 125, 2) == ("flat", 1, 1, 2, 1)
    assert _geometry(False, 1, 2, 128, 96, 4) == _geometry(False, 1, 2, 128, 96, 2) == ("flat", 1, 4, 2, 1)
    assert _geometry(True, 1, 2, 128, 96, 4)[0] == _geometry(True, 1, 2, 128, 96, 2)[0] == "tiles"
    # the shapes of test_vmamba_gpu.py all stay at one plane per workgroup
    for shape in [(2, 96, 56, 56), (3, 7, 33, 65), (1, 5, 1, 70), (2, 4, 31, 1), (1, 2, 128, 96), (3, 70, 14, 14), (2, 37, 7, 7), (2, 19, 28, 28),
                  (1, 3, 12, 20), (1, 1030, 14, 14), (8, 256, 56, 56), (2, 64, 128, 128)]:
        assert all(_geometry(merge, *shape, esz)[1] <= 1 for merge in (False, True) for esz in (4,) + ((2,) if shape[0] != 8 else ()))


def test_cross_div_equals_integer_division():
    """for every flat launch of every case: n // d for all n < P L and d in {LV, H, W}, where the kernels form quotients"""
    checked = set()
    for c, dt, shift in RUNS:
        B, C, H, W = c.shape
        for merge in (False, True):
            path, P, V, _, _ = _geometry(merge, B, C, H, W, _ESZ[dt], _aligned(dt, shift))
            if path != "flat":
                continue
            L = H * W
            n = torch.arange(P * L, dtype=torch.int64)
            for d in (L // V, H, W):
                if (P * L, d) in checked:
                    continue
                checked.add((P * L, d))
                assert P * L * d < 1 << 32, "the range the magic number is exact on"
                assert torch.equal(_cross_div(n, d), n // d), (c.id, d)
    assert any(d == 1 for _, d in checked) and any(d > 1 for _, d in checked)


# ---- CPU: the restated reference against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 1, 6), (1, 2, 5, 1), (2, 2, 1, 1), (1, 3, 2, 2), (1, 1, 33, 34)])
def test_ref_equals_oracle(shape, dtype):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, ys = torch.randn(B, C, H, W, generator=g).to(dtype), torch.randn(B, 4, C, H * W, generator=g).to(dtype)
    assert torch.equal(_bits(_scan_ref(x)), _bits(orc.cross_scan_ref(x)))
    assert torch.equal(_bits(_merge_ref(ys, H, W)), _bits(orc.cross_merge_ref(ys, H, W).to(dtype)))


# ---- GPU: the two entries on guarded buffers -------------------------------------------------------------------------------------------
def _launch(merge, shape, dtype, data, shift=0):
    """mxvl_cross_scan / mxvl_cross_merge on views into NaN-patterned buffers -> the output view, after the buffer checks"""
    B, C, H, W = shape
    src = _Buf.flat(data.shape, dtype, DEV, data, shift)
    dst = _Buf.flat((B, C, H * W) if merge else (B, 4, C, H * W), dtype, DEV, None, shift)
    for buf in (src, dst):
        assert (_ptr(buf) % 16 == 0) == _aligned(dtype, shift) and buf.view.is_contiguous()
    name = "mxvl_cross_merge" if merge else "mxvl_cross_scan"
    _abi.launch(name, _ptr(src), _ptr(dst), B, C, H, W, _abi.dtype_code(dtype), device=src.view.device)
    torch.cuda.synchronize()
    _assert_buffers(f"{name} {shape} {_DT[dtype]} base + {shift}", inputs=[("in", src)], outputs=[("out", dst)])
    return dst.view


def _data(case, dtype):
    B, C, H, W = case.shape
    g = torch.Generator().manual_seed(zlib.crc32(f"cross {case.id} {_DT[dtype]}".encode()))
    return torch.randn(B, C, H, W, generator=g).to(dtype), torch.randn(B, 4, C, H * W, generator=g).to(dtype)


def _check(case, dtype, shift):
    H, W = case.shape[2:]
    x, ys = _data(case, dtype)
    assert torch.equal(_bits(_launch(False, case.shape, dtype, x, shift).cpu()), _bits(_scan_ref(x))), "scan"
    assert torch.equal(_bits(_launch(True, case.shape, dtype, ys, shift).cpu()), _bits(_merge_ref(ys, H, W))), "merge"


@gpu
@pytest.mark.parametrize("case,dtype", [pytest.param(c, dt, id=f"{c.id}-{_DT[dt]}") for c in CASES for dt in c.dtypes])
def test_cross_scan_merge_bit_exact(case, dtype):
    _check(case, dtype, 0)


@gpu
@pytest.mark.parametrize("case,dtype", [pytest.param(c, dt, id=f"{c.id}-{_DT[dt]}") for c in CASES if c.shifts for dt in c.dtypes])
def test_cross_scan_merge_unaligned_base(case, dtype):
    """input and output one and two elements past a 16-byte boundary: launch_cross has to choose V = 1, nothing else changes"""
    for shift in case.shifts:
        assert all(_geometry(merge, *case.shape, _ESZ[dtype], _aligned(dtype, shift))[1:3] == (2, 1) for merge in (False, True))
        _check(case, dtype, shift)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
def test_roundtrip_is_four_x(dtype):
    """merge(scan(x)) == 4 x with several planes per workgroup: x + x and 2 x + 2 x are exact in all three dtypes"""
    case = CASES[1]
    assert _geometry(False, *case.shape, _ESZ[dtype])[1] > 1 and _geometry(True, *case.shape, _ESZ[dtype])[1] > 1
    x, _ = _data(case, dtype)
    xs = _launch(False, case.shape, dtype, x)
    assert torch.equal(_bits(_launch(True, case.shape, dtype, xs).cpu()), _bits((4 * x).flatten(2)))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_DT.get)
def test_autograd_pair_is_each_others_backward(dtype):
    """vmamba.CrossScan's backward is the merge and vmamba.CrossMerge's backward is the scan, with several planes per workgroup"""
    from medical_image_analysis_amd import vmamba as vm
    case = CASES[1]
    B, C, H, W = case.shape
    x, ys = _data(case, dtype)
    xd = x.to(DEV).requires_grad_(True)
    vm.CrossScan.apply(xd).backward(ys.to(DEV))
    assert torch.equal(_bits(xd.grad.cpu()), _bits(_merge_ref(ys, H, W).view(B, C, H, W)))
    yd = ys.to(DEV).view(B, 4, C, H, W).requires_grad_(True)
    vm.CrossMerge.apply(yd).backward(x.to(DEV).flatten(2))
    assert torch.equal(_bits(yd.grad.cpu()), _bits(_scan_ref(x).view(B, 4, C, H, W)))
