"""Window functions (reference src/sionna/phy/signal/window.py:12-373), multiplied onto the last axis."""
import numpy as np
import torch

from ._block import SignalBlock


class Window(SignalBlock):
    """A real window of N coefficients, applied by element-wise multiplication along the last axis; ``normalize`` scales
    it to unit mean square.  The output has the dtype of the input."""

    def __init__(self, normalize=False, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        assert isinstance(normalize, bool), "normalize must be bool"
        self._normalize = normalize

    @property
    def coefficients(self):
        """[N] real tensor: the raw window coefficients (before normalisation); settable"""
        return self._coefficients

    @coefficients.setter
    def coefficients(self, v):
        self._coefficients = self._cast_or_check_precision(v)

    @property
    def length(self):
        return self.coefficients.shape[0]

    @property
    def normalize(self):
        return self._normalize

    def _normalized(self):
        w = self.coefficients
        if self.normalize:
            w = w / torch.sqrt(torch.mean(torch.square(w)))
        return w

    def show(self, samples_per_symbol, domain="time", scale="lin"):
        """Plots the window in the time or the frequency domain (DFT of at least 1024 points)."""
        import matplotlib.pyplot as plt
        assert domain in ["time", "frequency"], "Invalid domain"
        w = self._normalized().numpy()
        n_min = -(self.length // 2)
        t = np.arange(n_min, n_min + self.length, dtype=np.float32) / np.float32(samples_per_symbol)
        plt.figure(figsize=(12, 6))
        if domain == "time":
            plt.plot(t, w)
            plt.title("Time domain")
            plt.xlabel(r"Normalized time $(t/T)$")
            plt.ylabel(r"$w(t)$")
            plt.xlim(t[0], t[-1])
        else:
            assert scale in ["lin", "db"], "Invalid scale"
            fft_size = max(1024, w.shape[-1])
            h = np.abs(np.fft.fftshift(np.fft.fft(w, fft_size)))
            if scale == "db":
                h = 10 * np.log10(np.maximum(h, 1e-10))
                plt.ylabel(r"$|W(f)|$ (dB)")
            else:
                plt.ylabel(r"$|W(f)|$")
            f = np.linspace(-samples_per_symbol / 2, samples_per_symbol / 2, fft_size)
            plt.plot(f, h)
            plt.title("Frequency domain")
            plt.xlabel(r"Normalized frequency $(f/W)$")
            plt.xlim(f[0], f[-1])
        plt.grid()

    def call(self, x):
        w = self._normalized().to(x.device)
        return x * w


class CustomWindow(Window):
    """A window of given ``coefficients`` [N]."""

    def __init__(self, coefficients, normalize=False, precision=None, **kwargs):
        super().__init__(normalize=normalize, precision=precision, **kwargs)
        self.coefficients = coefficients


class HannWindow(Window):
    r"""w_n = sin^2(pi n / N), 0 <= n <= N - 1, N the length of the last axis of the first input."""

    def build(self, input_shape):
        n = np.arange(input_shape[-1])
        self.coefficients = np.sin(np.pi * n / input_shape[-1]) ** 2


class HammingWindow(Window):
    r"""w_n = a_0 - (1 - a_0) cos(2 pi n / N), a_0 = 25 / 46."""

    def build(self, input_shape):
        n = np.arange(input_shape[-1])
        a0 = 25. / 46.
        self.coefficients = a0 - (1. - a0) * np.cos(2. * np.pi * n / input_shape[-1])


class BlackmanWindow(Window):
    r"""w_n = a_0 - a_1 cos(2 pi n / N) + a_2 cos(4 pi n / N), a_0 = 7938 / 18608, a_1 = 9240 / 18608, a_2 = 1430 / 18608."""

    def build(self, input_shape):
        n = np.arange(input_shape[-1])
        a0, a1, a2 = 7938. / 18608., 9240. / 18608., 1430. / 18608.
        self.coefficients = a0 - a1 * np.cos(2. * np.pi * n / input_shape[-1]) + a2 * np.cos(4. * np.pi * n / input_shape[-1])
