"""Filters, windows, resampling and spectrum helpers (mirror of ``sionna.phy.signal``, reference
src/sionna/phy/signal/__init__.py:1-12); filtering runs on ``csrc/signal.hip``."""
from .utils import convolve, fft, ifft, empirical_psd, empirical_aclr, upfirdn
from .window import Window, HannWindow, HammingWindow, BlackmanWindow, CustomWindow
from .filter import Filter, RaisedCosineFilter, RootRaisedCosineFilter, SincFilter, CustomFilter
from .upsampling import Upsampling
from .downsampling import Downsampling
