"""Pulse-shaping filters (reference src/sionna/phy/signal/filter.py:12-713).  The coefficient formulas are the ones of the
class documentation, evaluated in float64 at the float32 sampling times and rounded once; window, normalisation and
conjugation are applied to the taps on the host before the launch of ``csrc/signal.hip``."""
import numpy as np
import torch

from ._block import SignalBlock
from .utils import empirical_aclr, _filter_rows, _padding
from .window import Window, HannWindow, HammingWindow, BlackmanWindow


class Filter(SignalBlock):
    """A filter of ``length`` K = ``span_in_symbols`` * ``samples_per_symbol`` (plus one if that is even) applied to
    ``x`` [..., N] along the last axis by discrete convolution, with an optional ``window`` on the coefficients and
    normalisation to unit energy.  ``call(x, padding="full", conjugate=False)``: "full" returns N + K - 1 samples, "same" N
    (centred on tap (K - 1) / 2), "valid" N - K + 1."""

    def __init__(self, span_in_symbols, samples_per_symbol, window=None, normalize=True, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        assert span_in_symbols > 0, "span_in_symbols must be positive"
        self._span_in_symbols = span_in_symbols
        assert samples_per_symbol > 0, "samples_per_symbol must be positive"
        self._samples_per_symbol = samples_per_symbol
        self.window = window
        assert isinstance(normalize, bool), "normalize must be bool"
        self._normalize = normalize

    @property
    def span_in_symbols(self):
        return self._span_in_symbols

    @property
    def samples_per_symbol(self):
        return self._samples_per_symbol

    @property
    def length(self):
        """filter length in samples, forced odd"""
        n = self._span_in_symbols * self._samples_per_symbol
        return 2 * (n // 2) + 1

    @property
    def window(self):
        return self._window

    @window.setter
    def window(self, value):
        if isinstance(value, str):
            kinds = {"hann": HannWindow, "hamming": HammingWindow, "blackman": BlackmanWindow}
            if value not in kinds:
                raise AssertionError("Invalid window type")
            self._window = kinds[value](precision=self.precision)
        elif isinstance(value, Window) or value is None:
            self._window = value
        else:
            raise AssertionError("Invalid window type")
        if value is not None:
            assert self._window.precision == self._precision, "Window and Filter must have the same precision."
            self._window(torch.ones(self.length, dtype=self.cdtype))      # fixes the window's length (on the host)

    @property
    def normalize(self):
        return self._normalize

    @property
    def coefficients(self):
        """[K] real or complex host tensor: the raw coefficients (before window and normalisation); settable"""
        return self._coefficients

    @coefficients.setter
    def coefficients(self, v):
        from ..block import wrap
        self._coefficients = wrap(self._cast_or_check_precision(v))

    @property
    def sampling_times(self):
        """[K] numpy.float32: the sampling times in multiples of the symbol duration"""
        n_min = -(self.length // 2)
        t = np.arange(n_min, n_min + self.length, dtype=np.float32)
        t /= self.samples_per_symbol
        return t

    def _taps(self):
        """window, then normalisation, of the coefficients (filter.py:269-278), on the host"""
        h = self.coefficients.as_subclass(torch.Tensor)
        if self.window is not None:
            h = self._window(h).as_subclass(torch.Tensor)
        if self.normalize:
            h = h / torch.sqrt(torch.sum(torch.square(torch.abs(h)))).to(h.dtype)
        return h

    def show(self, response="impulse", scale="lin"):
        """Plots the impulse or the magnitude response (DFT of at least 1024 points; ``scale`` "lin" or "db")."""
        import matplotlib.pyplot as plt
        assert response in ["impulse", "magnitude"], "Invalid response"
        h = self._taps().numpy()
        plt.figure(figsize=(12, 6))
        if response == "impulse":
            t = self.sampling_times
            plt.plot(t, np.real(h))
            if np.iscomplexobj(h):
                plt.plot(t, np.imag(h))
                plt.legend(["Real part", "Imaginary part"])
            plt.title("Impulse response")
            plt.xlabel(r"Normalized time $(t/T)$")
            plt.ylabel(r"$h(t)$")
            plt.xlim(t[0], t[-1])
        else:
            assert scale in ["lin", "db"], "Invalid scale"
            fft_size = max(1024, h.shape[-1])
            mag = np.abs(np.fft.fftshift(np.fft.fft(h, fft_size)))
            if scale == "db":
                mag = 10 * np.log10(np.maximum(mag, 1e-10))
                plt.ylabel(r"$|H(f)|$ (dB)")
            else:
                plt.ylabel(r"$|H(f)|$")
            f = np.linspace(-self._samples_per_symbol / 2, self._samples_per_symbol / 2, fft_size)
            plt.plot(f, mag)
            plt.title("Magnitude response")
            plt.xlabel(r"Normalized frequency $(f/W)$")
            plt.xlim(f[0], f[-1])
        plt.grid()

    @property
    def aclr(self):
        """ACLR (linear) of the filter used as pulse shape on i.i.d. symbols, in-band [-0.5, 0.5] (filter.py:238-266):
        the empirical ACLR of the taps zero-padded to 1024 samples"""
        h = self._taps()
        c = torch.cat([h, torch.zeros(1024 - h.shape[-1], dtype=h.dtype)], -1).to(torch.complex64)
        return empirical_aclr(c, oversampling=self._samples_per_symbol, precision=self.precision)

    def call(self, x, padding="full", conjugate=False):
        h = self._taps()
        if x.is_cuda:                                    # the taps travel when they change, not once per call
            cached = getattr(self, "_taps_cache", None)
            if cached is None or cached[0] != x.device or cached[1].dtype != h.dtype or not torch.equal(cached[1], h):
                self._taps_cache = cached = (x.device, h, h.to(x.device))
            h = cached[2]
        start, m = _padding(padding, x.shape[-1], h.shape[0])
        return _filter_rows(x, h, 1, start, 1, m, conjugate)


def _sinc(x):
    return np.sinc(x)                                    # sin(pi x) / (pi x), 1 at 0


class RaisedCosineFilter(Filter):
    r"""h(t) = 1/T sinc(t/T) cos(pi beta t/T) / (1 - (2 beta t/T)^2), and pi/(4T) sinc(1/(2 beta)) at t = +-T/(2 beta); roll-off
    ``beta`` in [0, 1], T = 1.  (``precision`` is honoured; the reference passes it on under a misspelt keyword, filter.py:378.)"""

    def __init__(self, span_in_symbols, samples_per_symbol, beta, window=None, normalize=True, precision=None, **kwargs):
        super().__init__(span_in_symbols, samples_per_symbol, window=window, normalize=normalize, precision=precision, **kwargs)
        assert 0 <= beta <= 1, "beta must be from the intervall [0,1]"
        self._beta = beta
        t = np.abs(self.sampling_times.astype(np.float64))
        h = np.empty_like(t)
        for i, tt in enumerate(t):
            if beta > 0 and tt == 1 / (2 * beta):
                h[i] = np.pi / 4 * _sinc(1 / (2 * beta))
            else:
                h[i] = _sinc(tt) * np.cos(np.pi * beta * tt) / (1 - (2 * beta * tt) ** 2)
        self.coefficients = h.astype(np.float32)

    @property
    def beta(self):
        return self._beta


class RootRaisedCosineFilter(Filter):
    r"""h(0) = 1/T (1 + beta (4/pi - 1)); h(+-T/(4 beta)) = beta/(T sqrt 2) [(1 + 2/pi) sin(pi/(4 beta)) + (1 - 2/pi) cos(pi/(4 beta))];
    otherwise h(t) = 1/T [sin(pi t/T (1 - beta)) + 4 beta t/T cos(pi t/T (1 + beta))] / [pi t/T (1 - (4 beta t/T)^2)]; T = 1."""

    def __init__(self, span_in_symbols, samples_per_symbol, beta, window=None, normalize=True, precision=None, **kwargs):
        super().__init__(span_in_symbols, samples_per_symbol, window=window, normalize=normalize, precision=precision, **kwargs)
        assert 0 <= beta <= 1, "beta must be from the intervall [0,1]"
        self._beta = beta
        t = np.abs(self.sampling_times.astype(np.float64))
        h = np.empty_like(t)
        for i, tt in enumerate(t):
            if tt == 0:
                h[i] = 1 + beta * (4 / np.pi - 1)
            elif beta > 0 and tt == 1 / (4 * beta):
                h[i] = beta / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * beta)))
            else:
                h[i] = (np.sin(np.pi * tt * (1 - beta)) + 4 * beta * tt * np.cos(np.pi * tt * (1 + beta))) \
                    / (np.pi * tt * (1 - (4 * beta * tt) ** 2))
        self.coefficients = h.astype(np.float32)

    @property
    def beta(self):
        return self._beta


class SincFilter(Filter):
    r"""h(t) = 1/T sinc(t/T), T = 1."""

    def __init__(self, span_in_symbols, samples_per_symbol, window=None, normalize=True, precision=None, **kwargs):
        super().__init__(span_in_symbols, samples_per_symbol, window=window, normalize=normalize, precision=precision, **kwargs)
        self.coefficients = _sinc(self.sampling_times.astype(np.float64)).astype(np.float32)


class CustomFilter(Filter):
    """A filter of given ``coefficients`` [K], K odd."""

    def __init__(self, samples_per_symbol, coefficients, window=None, normalize=True, precision=None, **kwargs):
        assert samples_per_symbol > 0, "samples_per_symbol must be positive"
        n = coefficients.shape[-1]
        assert n % 2 == 1, "The number of coefficients must be odd"
        super().__init__(n // samples_per_symbol, samples_per_symbol, window=window, normalize=normalize, precision=precision,
                         **kwargs)
        self.coefficients = coefficients
        assert self.length == n, f"`coefficients` must have length {self.length}"
