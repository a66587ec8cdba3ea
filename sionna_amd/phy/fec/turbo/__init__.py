"""Turbo codes - mirror of reference src/sionna/phy/fec/turbo/__init__.py: ``TurboEncoder`` and ``TurboDecoder`` on the HIP
kernels of csrc/turbo.hip, ``TurboTermination``, ``puncture_pattern`` and ``polynomial_selector`` on the host."""
from .encoding import TurboEncoder
from .decoding import TurboDecoder
from .utils import TurboTermination, puncture_pattern, polynomial_selector
