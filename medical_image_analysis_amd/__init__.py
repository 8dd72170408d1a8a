"""medical_image_analysis_amd -- MI355X (gfx950) native hot path of MambaXray-VL.

The package is a thin host-side mirror of the reference's operator / module surface
(`selective_scan_fn`, `causal_conv1d_fn`, `mamba_inner_fn[_no_out_proj]`, `Mamba`, `ARM`,
`VisionMamba` ...) over a C-ABI shared library of hand-written HIP kernels
(csrc/*.hip -> libmxvl.so, declared in include/mxvl.h).  There is NO CPU or PyTorch fallback:
every operator raises if libmxvl.so is missing or the tensors are not on a HIP device.
"""
__version__ = "0.1.0"


def set_deterministic(mode=None):
    """Deterministic mode of libmxvl (include/mxvl.h mxvl_set_deterministic): True / False, or None (the default) to follow
    torch.are_deterministic_algorithms_enabled() at each call.  With it on, every fp32-accumulated gradient the hand-written kernels
    produce is bit-identical from run to run; vendor GEMMs, RCCL and torch's own ops are outside the guarantee.  Under the mode
    mamba_inner_fn_native's backward raises MXVL_ERR_UNSUPPORTED (the composed C entry refuses it); mamba_inner_fn is covered."""
    from . import _abi
    _abi.set_deterministic(mode)


def is_deterministic():
    """The mode the next libmxvl call runs in."""
    from . import _abi
    return _abi.is_deterministic()
