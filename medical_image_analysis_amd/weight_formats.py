"""The quantised weight formats of the frozen report LLM's layer projections, by name: the one table on the Python side of the ABI
(csrc/decode_gemm.hip with_format is the one on the other).  A class carries what differs -- NAME, W_FLAG, K_MULTIPLE, its buffers, its
quantiser (quant_linear.QuantLinear) -- so ReportDecoder.quantize_(name), the stepper and the tools read it here instead of naming
formats themselves."""
from __future__ import annotations

from .fp8_linear import Fp8Linear
from .int4_linear import Int4GroupLinear
from .int8_linear import Int8Linear
from .mxfp4_linear import MxFp4Linear

WEIGHT_FORMATS = {cls.NAME: cls for cls in (Int8Linear, MxFp4Linear, Fp8Linear, Int4GroupLinear)}


def low_resource_format(value):
    """`low_resource` as the models take it -> None (16-bit) or a name of WEIGHT_FORMATS.  The reference's flag is a bool that means
    load_in_8bit=True, so every truthy value that is not a format's name is int8."""
    if not value:
        return None
    return value if isinstance(value, str) and value in WEIGHT_FORMATS else Int8Linear.NAME
