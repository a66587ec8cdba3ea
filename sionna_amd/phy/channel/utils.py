"""Channel utilities of the hot path - mirror of reference src/sionna/phy/channel/utils.py
(``subcarrier_frequencies`` :15-66, ``cir_to_ofdm_channel`` :180-253, ``time_to_ofdm_channel`` :352-457)."""
import numpy as np
import torch

from ... import _ffi
from ..block import wrap
from ..config import config, dtypes


def subcarrier_frequencies(num_subcarriers, subcarrier_spacing, precision=None):
    """Baseband frequencies of the subcarriers, DC at index num_subcarriers//2 (utils.py:15-66)."""
    p = config.precision if precision is None else precision
    f = dtypes[p]["np"]["rdtype"]
    start = -(num_subcarriers // 2)
    limit = num_subcarriers // 2 + (num_subcarriers % 2)
    return (np.arange(start, limit, dtype=f) * f(subcarrier_spacing)).astype(f)


def time_frequency_vector(num_samples, sample_duration, precision=None):
    """Time and frequency vector of ``num_samples`` samples of ``sample_duration`` (normalised time), both ascending with
    the zero at index num_samples // 2 (utils.py:66-120): t = k sample_duration, f = k / (sample_duration num_samples),
    k = -(num_samples // 2) ... (num_samples - 1) // 2, each product rounded once in the precision's real type."""
    p = config.precision if precision is None else precision
    r = dtypes[p]["np"]["rdtype"]
    num_samples = int(num_samples)
    k = np.arange(-(num_samples // 2), (num_samples + 1) // 2, dtype=np.int32).astype(r)
    df = r(r(1.0 / sample_duration) / r(num_samples))
    return (k * r(sample_duration)).astype(r), (k * df).astype(r)


def cir_to_ofdm_channel(frequencies, a, tau, normalize=False):
    """h_f[b,rx,ra,tx,ta,t,f] = sum_p a[b,rx,ra,tx,ta,p,t] exp(-j 2 pi f tau[b,rx,tx,p])
    (+ optional normalisation to unit mean energy per (b,rx,tx)) - utils.py:180-253."""
    # the precision follows the coefficients like in the reference (real_dtype = tau.dtype, utils.py:228): complex128 taps
    # run the float64 kernel (csrc/f64_ofdm.hip)
    dbl = str(getattr(a, "dtype", "")).endswith("complex128")
    cdt, rdt = (torch.complex128, torch.float64) if dbl else (torch.complex64, torch.float32)
    a = _ffi.to_device(a, cdt)
    tau = _ffi.to_device(tau, rdt)
    fr = _ffi.to_device(np.asarray(frequencies.cpu() if isinstance(frequencies, torch.Tensor) else frequencies,
                                   np.float64 if dbl else np.float32), rdt)
    if tau.dim() != 4:
        raise NotImplementedError("cir_to_ofdm_channel: per-antenna delays (rank-6 tau) are outside the hot path")
    b, rx, ra, tx, ta, p, t = a.shape
    assert tuple(tau.shape) == (b, rx, tx, p), "tau must have shape [batch, num_rx, num_tx, num_paths]"
    h = torch.empty((b, rx, ra, tx, ta, t, fr.numel()), dtype=cdt, device=a.device)
    fn = _ffi.lib().samd_cir_to_ofdm_c128 if dbl else _ffi.lib().samd_cir_to_ofdm_c64
    _ffi.check(fn(_ffi.ptr(a), _ffi.ptr(tau), _ffi.ptr(fr), b, rx, ra, tx, ta, p, t, fr.numel(), int(bool(normalize)),
                  _ffi.ptr(h), _ffi.stream()), "cir_to_ofdm_channel")
    return wrap(h)


def time_to_ofdm_channel(h_t, rg, l_min):
    """Channel frequency response per OFDM symbol from the discrete complex-baseband impulse response
    (utils.py:352-457): h_t [..., num_time_steps, l_max - l_min + 1] -> [..., num_ofdm_symbols, fft_size].  The taps at the
    first sample after every cyclic prefix, zero-padded to fft_size, rolled by l_min so that the response starts with lag 0,
    FFT, zero subcarrier moved to the centre.  Library-shaped work: ``torch.fft`` on the device the tensor lives on (rocFFT
    for device tensors), in the tensor's own precision."""
    h = h_t if isinstance(h_t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(h_t)))
    h = h.as_subclass(torch.Tensor)
    assert h.is_complex() and h.dim() >= 2, "h_t must be complex with shape [..., num_time_steps, l_max - l_min + 1]"
    assert h.shape[-1] <= rg.fft_size, "the impulse response is longer than fft_size"
    h = h[..., rg.cyclic_prefix_length:rg.num_time_samples:rg.fft_size + rg.cyclic_prefix_length, :]
    h = torch.nn.functional.pad(h, (0, rg.fft_size - h.shape[-1]))
    h = torch.roll(h, int(l_min), dims=-1)
    return wrap(torch.fft.fftshift(torch.fft.fft(h, dim=-1), dim=-1).contiguous())
