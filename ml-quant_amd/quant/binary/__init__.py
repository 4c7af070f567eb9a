"""Scaled binary quantization: sign/STE, quantizers, quantizer modules, QuantConv2d and QuantLinear."""

from quant.binary.binary_linear import QuantLinear  # noqa: F401
