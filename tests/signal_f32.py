"""Specification of the filter kernel (csrc/signal.hip) in NumPy, float32 and float64.

    y[b, m] = sum_{k = 0..K-1} h[k] * xu[b, start + m * down - k],   xu[b, j] = x[b, j / up] if up | j and 0 <= j / up < N, else 0

Every real accumulator starts at +0 and adds ``h[k] * x[...]`` in ascending k - one multiplication, one addition, both rounded
to ``dtype`` - over those k whose sample exists (not an inserted zero, not out of range).  A complex output keeps the four real
sums the reference forms (signal/utils.py:122-151): rr, ii, ri (input real x tap imag), ir, and is (rr - ii) + j (ri + ir);
real taps use rr and ir only, a real input rr and ri only.  Conjugation negates the taps' imaginary part first.

``three_step`` is the composition ``upfirdn`` of the package must equal: zero insertion, convolution, decimation."""
import numpy as np


def padding_params(padding, length, k):
    """(start, M) for a (zero-stuffed) input of ``length`` samples: "same" is centred on tap (K - 1) // 2"""
    padding = padding.lower()
    if padding == "full":
        return 0, length + k - 1
    if padding == "same":
        return (k - 1) // 2, length
    assert padding == "valid"
    return k - 1, length - k + 1


def upfirdn(x, h, up=1, start=0, down=1, m=None, conjugate=False, dtype=np.float32):
    """x [..., N] real or complex, h [K] real or complex -> [..., m] in ``dtype`` (or its complex twin)"""
    x, h = np.asarray(x), np.asarray(h)
    xc, hc = np.iscomplexobj(x), np.iscomplexobj(h)
    batch, n, k = x.shape[:-1], x.shape[-1], h.shape[0]
    if m is None:
        m = n * up + k - 1 - start
    x2 = x.reshape(-1, n)
    xr, xi = x2.real.astype(dtype), (x2.imag.astype(dtype) if xc else None)
    hr, hi = h.real.astype(dtype), (h.imag.astype(dtype) if hc else None)
    if hc and conjugate:
        hi = -hi
    rr, ii, ri, ir = (np.zeros((x2.shape[0], m), dtype) for _ in range(4))
    p = start + down * np.arange(m, dtype=np.int64)
    for t in range(k):
        j = p - t
        ok = (j % up == 0) & (j >= 0) & (j // up < n)
        src = (j // up)[ok]
        rr[:, ok] = rr[:, ok] + hr[t] * xr[:, src]
        if xc:
            ir[:, ok] = ir[:, ok] + hr[t] * xi[:, src]
        if hc:
            ri[:, ok] = ri[:, ok] + hi[t] * xr[:, src]
        if xc and hc:
            ii[:, ok] = ii[:, ok] + hi[t] * xi[:, src]
    assert rr.dtype == dtype
    if xc or hc:
        y = np.empty(rr.shape, np.complex64 if dtype == np.float32 else np.complex128)
        y.real, y.imag = rr - ii, ri + ir
    else:
        y = rr
    return y.reshape(*batch, m)


def convolve(x, h, padding="full", dtype=np.float32):
    start, m = padding_params(padding, np.asarray(x).shape[-1], np.asarray(h).shape[0])
    return upfirdn(x, h, 1, start, 1, m, False, dtype)


def upsample(x, up):
    x = np.asarray(x)
    y = np.zeros(x.shape + (up,), x.dtype)
    y[..., 0] = x
    return y.reshape(*x.shape[:-1], -1)


def three_step(x, h, up=1, down=1, offset=0, num_symbols=None, padding="full", conjugate=False, dtype=np.float32):
    """Downsampling(down, offset, num_symbols)(convolve(Upsampling(up)(x), h, padding)), each step on its own"""
    h = np.asarray(h)
    if conjugate and np.iscomplexobj(h):
        h = np.conj(h)
    y = convolve(upsample(x, up), h, padding, dtype)[..., offset::down]
    return y if num_symbols is None else y[..., :num_symbols]


def fused(x, h, up=1, down=1, offset=0, num_symbols=None, padding="full", conjugate=False, dtype=np.float32):
    """the same through ONE evaluation of the formula: what ``sionna_amd.phy.signal.upfirdn`` launches"""
    start, mc = padding_params(padding, np.asarray(x).shape[-1] * up, np.asarray(h).shape[0])
    m = len(range(offset, mc, down))
    if num_symbols is not None:
        m = min(m, num_symbols)
    return upfirdn(x, h, up, start + offset, down, m, conjugate, dtype)


def running_sum_bound(x, h, padding, unit):
    """(K + 3) * unit * sum_k |h[k]| |x[n - k]| per output (float64): K roundings of the running sum, one of the products,
    one of the final difference of two sums, one of the fixture's own cast"""
    k = np.asarray(h).shape[0]
    return (k + 3) * unit * convolve(np.abs(x).astype(np.float64), np.abs(h).astype(np.float64), padding, np.float64)
