"""``convolve``, ``fft`` / ``ifft``, ``empirical_psd`` / ``empirical_aclr`` (reference src/sionna/phy/signal/utils.py:13-370)
and ``upfirdn``, an addition: upsampling, filtering and downsampling in one launch of ``csrc/signal.hip``.

Device tensors are filtered by the HIP kernel (``samd_upfirdn_*``), host tensors by the same arithmetic written in torch on
the CPU (``_host_upfirdn``; tests/signal_f32.py states it in NumPy): every real sum starts at +0 and adds ``h[k] * x`` in
ascending ``k``; a complex output is ``(rr - ii) + j (ri + ir)`` (utils.py:122-151).  No gradients flow through either."""
import numpy as np
import torch

from ..config import config, dtypes

MAX_TAPS = 1025          # SAMD_UPFIRDN_MAX_TAPS of include/sionna_amd.h: the most taps the kernel takes


def _types(precision):
    if precision is None:
        precision = config.precision
    if precision not in ("single", "double"):
        raise ValueError("'precision' must be 'single' or 'double'")
    return dtypes[precision]["torch"]["rdtype"], dtypes[precision]["torch"]["cdtype"]


def _as_tensor(v, rdtype, cdtype):
    """utils.py:76-83: floating inputs are cast to the real dtype, complex ones to the complex dtype; tensors stay on
    their device, arrays stay on the host"""
    if not isinstance(v, torch.Tensor):
        v = torch.from_numpy(np.ascontiguousarray(v))
    v = v.detach().as_subclass(torch.Tensor)
    if v.dtype.is_complex:
        return v.to(cdtype)
    return v.to(rdtype)


def _padding(padding, length, k):
    """(start, M) of a padding mode for an (upsampled) input of ``length`` samples and ``k`` taps (utils.py:23-33, 101-120)"""
    padding = padding.lower()
    assert padding in ("valid", "same", "full"), "Invalid padding method"
    if padding == "full":
        return 0, length + k - 1
    if padding == "same":
        return (k - 1) // 2, length
    return k - 1, length - k + 1


def _host_upfirdn(x, h, n_up, start, down, m):
    """the specification arithmetic on host tensors: x [B, N], h [K] -> [B, m]"""
    b, n = x.shape
    k = h.shape[0]
    xc, hc = x.dtype.is_complex, h.dtype.is_complex
    rd = x.real.dtype
    # zero-stuffed row with K - 1 zeros to its left and zeros to its right: a product with one of them is +-0 and leaves a
    # sum that started at +0 as it is
    last = start + (m - 1) * down
    width = max(last + 1, n * n_up) + k
    xu = torch.zeros((b, width), dtype=x.dtype)
    xu[:, k - 1:k - 1 + n * n_up:n_up] = x
    pos = start + down * torch.arange(m) + (k - 1)
    xr, xi = (xu.real, xu.imag) if xc else (xu, None)
    hr, hi = (h.real, h.imag) if hc else (h, None)
    rr, ii, ri, ir = (torch.zeros((b, m), dtype=rd) for _ in range(4))
    for t in range(k):
        idx = pos - t
        rr += hr[t] * xr[:, idx]
        if xc:
            ir += hr[t] * xi[:, idx]
        if hc:
            ri += hi[t] * xr[:, idx]
        if xc and hc:
            ii += hi[t] * xi[:, idx]
    if xc or hc:
        return torch.complex(rr - ii, ri + ir)
    return rr


def _device_upfirdn(x, h, n_up, start, down, m, conjugate):
    """x [B, N] contiguous device tensor, h [K] tensor (any device) -> [B, m] through samd_upfirdn_*"""
    from ... import _ffi
    b, n = x.shape
    k = h.shape[0]
    if k > MAX_TAPS:
        raise ValueError(f"the filter kernel takes at most {MAX_TAPS} taps, got {k}")
    xc, hc = x.dtype.is_complex, h.dtype.is_complex
    rd = x.real.dtype
    h = h.to(x.device)
    h_re = (h.real if hc else h).contiguous()
    h_im = h.imag.contiguous() if hc else None
    out = torch.empty((b, m), dtype=(torch.complex64 if rd == torch.float32 else torch.complex128) if (xc or hc) else rd,
                      device=x.device)
    if b == 0 or m == 0:
        return out
    name = "samd_upfirdn_" + (("c64" if xc else "f32") if rd == torch.float32 else ("c128" if xc else "f64"))
    xv = torch.view_as_real(x) if xc else x
    ov = torch.view_as_real(out) if out.dtype.is_complex else out
    _ffi.check(getattr(_ffi.lib(), name)(_ffi.ptr(xv), _ffi.ptr(h_re), _ffi.ptr(h_im), b, n, k, n_up, start, down, m,
                                         int(bool(conjugate)), _ffi.ptr(ov), _ffi.stream()), name)
    return out


def _filter_rows(x, h, n_up, start, down, m, conjugate):
    """rows of x [..., N] -> [..., m]"""
    batch, n = x.shape[:-1], x.shape[-1]
    if m < 0:
        raise ValueError("the kernel is longer than the input: 'valid' padding has no output")
    x2 = x.reshape(-1, n)
    if x2.is_cuda:
        y = _device_upfirdn(x2.contiguous(), h, n_up, start, down, m, conjugate)
    else:
        if conjugate and h.dtype.is_complex:
            h = torch.conj_physical(h)
        y = _host_upfirdn(x2, h.cpu(), n_up, start, down, m)
    return y.reshape(*batch, m)


def convolve(inp, ker, padding="full", axis=-1, precision=None):
    """utils.py:13-159: filters ``inp`` [..., N] along ``axis`` with the kernel ``ker`` [K].  The output is real only if
    both are real.  "full": M = N + K - 1; "same": M = N, centred on tap (K - 1) // 2; "valid": M = N - K + 1."""
    from ..block import wrap
    rdtype, cdtype = _types(precision)
    inp, ker = _as_tensor(inp, rdtype, cdtype), _as_tensor(ker, rdtype, cdtype)
    x = torch.swapaxes(inp, axis, -1)
    start, m = _padding(padding, x.shape[-1], ker.shape[0])
    y = _filter_rows(x, ker, 1, start, 1, m, False)
    return wrap(torch.swapaxes(y, axis, -1))


def upfirdn(x, h, up=1, down=1, offset=0, num_symbols=None, padding="full", conjugate=False, precision=None):
    """Upsampling, filtering and downsampling of the last axis in one launch (not in the reference):
    ``Downsampling(down, offset, num_symbols)(convolve(Upsampling(up)(x), h, padding))`` with the same bits, without the
    zero-stuffed and the oversampled tensors.  ``up`` = samples per symbol is a pulse-shaping transmitter, ``down`` =
    samples per symbol a matched-filter receiver.  ``conjugate`` applies the complex conjugate of complex taps."""
    from ..block import wrap
    rdtype, cdtype = _types(precision)
    x, h = _as_tensor(x, rdtype, cdtype), _as_tensor(h, rdtype, cdtype)
    up, down, offset = int(up), int(down), int(offset)
    if up < 1 or down < 1 or offset < 0:
        raise ValueError("up and down must be positive, offset non-negative")
    start, mc = _padding(padding, x.shape[-1] * up, h.shape[0])
    if mc < 0:
        raise ValueError("the kernel is longer than the upsampled input: 'valid' padding has no output")
    m = max(0, -((offset - mc) // down))                   # len(range(offset, mc, down))
    if num_symbols is not None:
        m = min(m, int(num_symbols))
    return wrap(_filter_rows(x, h, up, start + offset, down, m, conjugate))


def fft(tensor, axis=-1, precision=None):
    """utils.py:161-204: the normalised DFT, 1 / sqrt(N) * fft"""
    from ..block import wrap
    _, cdtype = _types(precision)
    t = _as_tensor(tensor, cdtype, cdtype).to(cdtype)
    n = t.shape[axis]
    return wrap(torch.fft.fft(t, dim=axis) * (1 / np.sqrt(n)))


def ifft(tensor, axis=-1, precision=None):
    """utils.py:206-249: the normalised IDFT, sqrt(N) * ifft"""
    from ..block import wrap
    _, cdtype = _types(precision)
    t = _as_tensor(tensor, cdtype, cdtype).to(cdtype)
    n = t.shape[axis]
    return wrap(torch.fft.ifft(t, dim=axis) * np.sqrt(n))


def empirical_psd(x, show=True, oversampling=1.0, ylim=(-30, 3), precision=None):
    """utils.py:251-315: the squared magnitude of the normalised DFT along the last axis, averaged over all other axes and
    centred; returns (normalised frequencies [N], psd [N]) on the device of ``x``"""
    from ..block import wrap
    rdtype, cdtype = _types(precision)
    x = _as_tensor(x, cdtype, cdtype).to(cdtype)
    psd = torch.abs(fft(x, precision=precision).as_subclass(torch.Tensor)) ** 2
    if psd.dim() > 1:
        psd = psd.mean(dim=tuple(range(psd.dim() - 1)))
    psd = torch.fft.fftshift(psd)
    f_min = -0.5 * oversampling
    freqs = torch.linspace(f_min, -f_min, psd.shape[0], dtype=torch.float64, device=psd.device).to(rdtype)
    if show:
        import matplotlib.pyplot as plt
        f, p = freqs.cpu().numpy(), psd.cpu().numpy()
        plt.figure()
        plt.plot(f, 10 * np.log10(p))
        plt.title("Power Spectral Density")
        plt.xlabel("Normalized Frequency")
        plt.xlim([f[0], f[-1]])
        plt.ylabel(r"$\mathbb{E}\left[|X(f)|^2\right]$ (dB)")
        plt.ylim(ylim)
        plt.grid(True, which="both")
    return wrap(freqs), wrap(psd)


def empirical_aclr(x, oversampling=1.0, f_min=-0.5, f_max=0.5, precision=None):
    """utils.py:317-370: out-of-band over in-band power of the empirical PSD; the in-band is (f_min, f_max)"""
    from ..block import wrap
    freqs, psd = empirical_psd(x, show=False, oversampling=oversampling, precision=precision)
    freqs, psd = freqs.as_subclass(torch.Tensor), psd.as_subclass(torch.Tensor)
    out = (freqs < f_min) | (freqs > f_max)
    inside = (freqs > f_min) & (freqs < f_max)
    return wrap(psd[out].sum() / psd[inside].sum())
