"""Convolutional codes - mirror of reference src/sionna/phy/fec/conv/__init__.py: ``ConvEncoder`` and the ``ViterbiDecoder`` /
``BCJRDecoder`` on the HIP kernels of csrc/conv.hip, ``polynomial_selector`` and ``Trellis`` on the host."""
from .encoding import ConvEncoder
from .decoding import ViterbiDecoder, BCJRDecoder
from .utils import polynomial_selector, Trellis
