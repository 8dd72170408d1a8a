"""What the kernel-against-float64 test files share (test_conv1d_gpu.py, test_dwconv2d_gpu.py, test_norm_act_gpu.py, test_gemm_gpu.py): the rounding model
of the fp32 kernels, the err / tol ratio, and the NaN-patterned buffers with guard bands that every tensor a kernel touches is a view into."""
import torch

U = 2.0 ** -24                     # unit roundoff of fp32
FLOOR = 2.0 ** -100                # the fast exponential flushes denormals: no tolerance below this
_PREC = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}


def _ulp(v, dtype):
    """one unit in the last place of `dtype` at |v| (float64 tensor)"""
    p, emin = _PREC[dtype]
    _, ex = torch.frexp(v.abs().clamp_min(2.0 ** emin))          # |v| in [2^(ex-1), 2^ex)
    return torch.ldexp(torch.ones_like(v), ex - p)


def _rho(v):
    """relative error allowed to sigmoid(v) / exp(v) as the kernels form them: v * log2e rounded once (|v| u in the exponent),
    v_exp_f32 and v_rcp_f32 at one ulp each, one add, one multiply"""
    return (v.abs() + 8.0) * 2.0 ** -23


def _rnd(v, dtype):
    """float64 `v` rounded to `dtype` (nearest even), back in float64"""
    return v.to(dtype).double()


def _near_tie(v, err, dtype):
    """where a value within `err` of `v` can round to another `dtype` number than `v` does: the midpoint between two neighbours of
    v's binade lies ulp / 2 - |v - rnd(v)| away"""
    return (0.5 * _ulp(v, dtype) - (v - _rnd(v, dtype)).abs()) <= err


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product is exact in float64, one rounding to 53 bits and one to 24 follow"""
    return (a.double() * b.double() + c.double()).float()


def _ratio(got, ref, tol):
    """max err / tol over ALL elements; a non-finite result counts as infinitely wrong"""
    r = (got.detach().double().cpu() - ref).abs() / tol
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def _report(what, **ratios):
    """prints max err / tol per output, asserts each <= 1"""
    ratios = {k: v for k, v in ratios.items() if v is not None}
    print(f"{what}: max err / tol " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{what}: outside the bound: {bad}"


GUARD = 64                                                        # elements before and after: keeps 256 / 128-byte alignment
_NAN_BITS = {torch.float32: 0x7FC0DEAD, torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}


class _Buf:
    """a view of `shape` / `strides` at `off` into `n` elements holding the NaN pattern"""

    def __init__(self, n, off, strides, shape, dtype, device, data=None):
        self.pat, self.geom = _NAN_BITS[dtype], (tuple(shape), tuple(strides), off)
        self.raw = torch.full((n,), self.pat, dtype=torch.int32 if dtype == torch.float32 else torch.int16, device=device)
        self.view = self.raw.view(dtype).as_strided(*self.geom)
        assert self.raw.data_ptr() % 256 == 0
        self.before = None
        if data is not None:
            self.view.copy_(data)
            self.before = self.raw.clone()

    @classmethod
    def flat(cls, shape, dtype, device, data=None, shift=0):
        """a contiguous view, `shift` elements past the aligned start that follows the leading guard"""
        t = torch.empty(shape, device="meta")
        return cls(t.numel() + shift + 2 * GUARD, GUARD + shift, t.stride(), shape, dtype, device, data)

    def guard_intact(self):
        snap = self.raw.clone()
        snap.as_strided(*self.geom).fill_(self.pat)
        return bool((snap == self.pat).all())

    def unchanged(self):
        return torch.equal(self.raw, self.before)

    def written(self):
        return not bool(torch.isnan(self.view).any())

    def untouched(self):
        """nothing stored anywhere, the view included: a buffer the kernel was told to leave alone"""
        return bool((self.raw == self.pat).all())


def _ptr(buf):
    return None if buf is None else buf.view.data_ptr()


def _assert_buffers(what, inputs=(), outputs=(), untouched=()):
    """after a launch: guards intact, inputs unchanged, outputs fully written, buffers the kernel must leave alone still all pattern"""
    for name, buf in inputs:
        assert buf is None or buf.unchanged(), f"{what}: input {name} was modified"
    for name, buf in outputs:
        assert buf is None or buf.guard_intact(), f"{what}: store outside {name}"
        assert buf is None or buf.written(), f"{what}: {name} not fully written (or a read outside an input reached it)"
    for name, buf in untouched:
        assert buf is None or buf.untouched(), f"{what}: {name} was written"
