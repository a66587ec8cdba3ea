"""The filter kernel (csrc/signal.hip) against its specification tests/signal_f32.py, bit for bit, in float32 and float64,
and ``sionna_amd.phy.signal`` on the device.  T = 1024 is the tile of the up = down = 1 path (256 lanes x 4 outputs), 8192 the
most workgroups of a launch, MAX_TAPS = 1025 the most taps."""
import ctypes

import numpy as np
import pytest
import torch

import signal_f32 as spec

pytestmark = pytest.mark.gpu

T, GRID_CAP = 1024, 256 * 32
DTYPES = [(np.float32, np.complex64, "single"), (np.float64, np.complex128, "double")]


@pytest.fixture(scope="module")
def sig():
    from sionna_amd import _ffi
    from sionna_amd.phy import signal
    _ffi.device()
    assert signal.utils.MAX_TAPS == 1025
    return signal


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rand(rng, shape, dtype):
    if np.dtype(dtype).kind == "c":
        return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype)
    return rng.normal(size=shape).astype(dtype)


@pytest.mark.parametrize("k", [1, 2, 4, 5, 33, 129, 1025])
@pytest.mark.parametrize("rd,cd,prec", DTYPES)
def test_convolve_equals_the_specification(sig, k, rd, cd, prec):
    """N = K (one "valid" output), T - 1, T, T + 1, 2 T + 3 (a halo across tiles); the three paddings; complex x complex"""
    rng = np.random.default_rng(k)
    h = rand(rng, k, cd)
    for n in sorted({k} | {n for n in (T - 1, T, T + 1, 2 * T + 3) if n >= k}):
        x = rand(rng, (2, n), cd)
        for pad in ("full", "same", "valid"):
            got = sig.convolve(dev(x), dev(h), pad, precision=prec)
            ref = spec.convolve(x, h, pad, rd)
            assert got.is_cuda and tuple(got.shape) == ref.shape == (2, {"full": n + k - 1, "same": n, "valid": n - k + 1}[pad])
            assert got.dtype == torch.from_numpy(ref).dtype
            assert np.array_equal(got.cpu().numpy(), ref), (n, pad)


@pytest.mark.parametrize("rd,cd,prec", DTYPES)
def test_real_and_complex_combinations_and_conjugate(sig, rd, cd, prec):
    """the output is real only if input and taps are; the conjugate flag negates the taps' imaginary part (and does nothing
    to real taps); odd and even K"""
    rng = np.random.default_rng(7)
    for k in (5, 4):
        for xd in (rd, cd):
            for hd in (rd, cd):
                x, h = rand(rng, (3, T + 1), xd), rand(rng, k, hd)
                for pad in ("full", "same", "valid"):
                    for conj in (False, True):
                        got = sig.upfirdn(dev(x), dev(h), padding=pad, conjugate=conj, precision=prec)
                        ref = spec.fused(x, h, padding=pad, conjugate=conj, dtype=rd)
                        assert got.dtype == (torch.from_numpy(np.zeros(1, rd if xd == hd == rd else cd)).dtype)
                        assert np.array_equal(got.cpu().numpy(), ref), (k, xd, hd, pad, conj)
                        if conj and hd == cd:
                            assert np.array_equal(ref, spec.convolve(x, np.conj(h), pad, rd))


def test_more_taps_than_the_kernel_takes_are_refused(sig):
    from sionna_amd import _ffi
    x, h = torch.zeros(2, 2000, device="cuda"), torch.ones(1026, device="cuda")
    with pytest.raises(ValueError):
        sig.convolve(x, h)
    with pytest.raises(ValueError):
        sig.upfirdn(x, h, up=2)
    out = torch.zeros(2, 3025, device="cuda")
    rc = _ffi.lib().samd_upfirdn_f32(_ffi.ptr(x), _ffi.ptr(h), None, 2, 2000, 1026, 1, 0, 1, 3025, 0, _ffi.ptr(out), _ffi.stream())
    assert rc == _ffi.ERR_INVALID and b"1025" in _ffi.lib().samd_last_error()
    with pytest.raises(ValueError):                       # the input samples of 256 decimated outputs exceed the LDS budget
        sig.upfirdn(torch.zeros(1, 100000, dtype=torch.complex128, device="cuda"), torch.ones(5, dtype=torch.float64), down=64,
                    precision="double")
    with pytest.raises(ValueError):
        sig.convolve(torch.zeros(2, 3, device="cuda"), torch.ones(5), "valid")


@pytest.mark.parametrize("rd,cd,prec", DTYPES)
def test_rows_one_none_and_past_one_grid_trip(sig, rd, cd, prec):
    rng = np.random.default_rng(11)
    h = rand(rng, 5, cd)
    for rows in (1, GRID_CAP + 1, 2 * GRID_CAP + 37):
        x = rand(rng, (rows, 40), rd)
        got = sig.convolve(dev(x), dev(h), "same", precision=prec)
        assert np.array_equal(got.cpu().numpy(), spec.convolve(x, h, "same", rd))
    empty = sig.convolve(torch.zeros(0, 40, dtype=torch.from_numpy(np.zeros(1, cd)).dtype, device="cuda"), dev(h), precision=prec)
    assert tuple(empty.shape) == (0, 44) and empty.is_cuda
    # two tiles per row and more work items than workgroups: rows x tiles past the cap
    x = rand(rng, (GRID_CAP // 2 + 3, T + 9), rd)
    hr = rand(rng, 4, rd)
    got = sig.convolve(dev(x), dev(hr), "full", precision=prec)
    assert got.dtype == torch.from_numpy(np.zeros(1, rd)).dtype and np.array_equal(got.cpu().numpy(), spec.convolve(x, hr, "full", rd))


def test_axes_and_a_view(sig):
    rng = np.random.default_rng(13)
    x = rand(rng, (37, 50, 3), np.complex64)
    h = rand(rng, 5, np.float32)
    for axis in (0, 1):
        got = sig.convolve(dev(x), dev(h), "same", axis=axis).cpu().numpy()
        ref = np.swapaxes(spec.convolve(np.swapaxes(x, axis, -1), h, "same"), axis, -1)
        assert got.shape == x.shape and np.array_equal(got, ref), axis
    view = dev(x)[:, ::2, 1]
    assert not view.is_contiguous()
    assert np.array_equal(sig.convolve(view, dev(h), "full").cpu().numpy(), spec.convolve(x[:, ::2, 1], h, "full"))


@pytest.mark.parametrize("up,down", [(4, 1), (1, 4), (3, 2), (2, 3)])
@pytest.mark.parametrize("rd,cd,prec", DTYPES)
def test_upfirdn_equals_the_three_blocks(sig, up, down, rd, cd, prec):
    """identical to Upsampling, convolve, Downsampling run one after the other on the device, and to the specification;
    more outputs than one tile holds"""
    rng = np.random.default_rng(100 * up + down)
    n = 1300 * down // up + 57
    x, h = rand(rng, (2, n), cd), rand(rng, 33, cd)
    xd, hd = dev(x), dev(h)
    for offset in (0, 1, down + 2):
        for num in (None, 1100):
            for pad, conj in (("full", False), ("same", True), ("valid", False)):
                got = sig.upfirdn(xd, hd, up, down, offset, num, pad, conj, precision=prec)
                hh = torch.conj_physical(hd) if conj else hd
                steps = sig.Downsampling(down, offset, num, precision=prec)(
                    sig.convolve(sig.Upsampling(up, precision=prec)(xd), hh, pad, precision=prec))
                assert got.shape[-1] > T and torch.equal(got, steps), (offset, num, pad)
                assert np.array_equal(got.cpu().numpy(), spec.fused(x, h, up, down, offset, num, pad, conj, rd))


def test_pulse_shaping_link_of_the_tutorial(sig):
    """QPSK -> Upsampling(4) -> root-raised cosine (span 32, 4 samples per symbol, beta 0.22) -> matched filter ->
    Downsampling(4, offset = length - 1, num_symbols): the symbols come back within the inter-symbol interference the
    truncated pulse leaves, |g_0 - 1| + sum_{i != 0} |g_{4 i}| of the float64 pulse g = h * h, times the symbol modulus
    (float32 rounding is five orders below); two upfirdn calls give identical bits"""
    rng = np.random.default_rng(17)
    num, sps = 500, 4
    x = ((2 * rng.integers(0, 2, (3, num)) - 1) + 1j * (2 * rng.integers(0, 2, (3, num)) - 1)).astype(np.complex64) / np.float32(np.sqrt(2))
    rrc = sig.RootRaisedCosineFilter(32, sps, 0.22)
    assert rrc.length == 129
    xd = dev(x)
    x_us = sig.Upsampling(sps)(xd)
    x_rrc = rrc(x_us)
    x_mf = rrc(x_rrc)
    x_hat = sig.Downsampling(sps, rrc.length - 1, num)(x_mf)
    assert tuple(x_rrc.shape) == (3, num * sps + 128) and tuple(x_hat.shape) == (3, num)
    h64 = sig.RootRaisedCosineFilter(32, sps, 0.22, precision="double")._taps().numpy()
    g = np.convolve(h64, h64)[128 % sps::sps]
    centre = 128 // sps
    floor = abs(g[centre] - 1) + np.abs(np.delete(g, centre)).sum()
    err = np.abs(x_hat.cpu().numpy() - x).max()
    print("max symbol error", err, "interference floor", floor)
    assert floor < 0.05 and err <= floor + 1e-5
    h = rrc._taps()
    tx = sig.upfirdn(xd, h, up=sps)
    assert torch.equal(tx, x_rrc)
    rx = sig.upfirdn(tx, h, down=sps, offset=rrc.length - 1, num_symbols=num)
    assert torch.equal(rx, x_hat)


def test_every_filter_class_with_a_window(sig):
    rng = np.random.default_rng(19)
    x = rand(rng, (2, 300), np.complex64)
    custom = rand(rng, 17, np.complex64)
    filters = [sig.RaisedCosineFilter(8, 4, 0.35, window="hann", normalize=False),
               sig.RootRaisedCosineFilter(8, 4, 0.35, window="hann", normalize=False),
               sig.SincFilter(8, 4, window="hann", normalize=False),
               sig.CustomFilter(4, custom, window="hann", normalize=False)]
    for f in filters:
        y = f(x, "same", conjugate=True)                  # an array goes to the device like in every other block
        taps = f._taps().numpy()
        assert y.is_cuda and len(taps) == f.length and f.window.length == f.length
        assert np.array_equal(y.cpu().numpy(), spec.convolve(x, np.conj(taps), "same")), type(f).__name__
    w = sig.HammingWindow()
    assert np.array_equal(w(dev(x)).cpu().numpy(), x * w.coefficients.numpy())
    f, p = sig.empirical_psd(dev(x), show=False, oversampling=2.0)
    assert f.is_cuda and p.is_cuda and abs(float(p.mean()) - float(np.mean(np.abs(x) ** 2))) < 1e-4
    assert abs(float(sig.empirical_aclr(dev(x), oversampling=2.0)) - 1) < 0.3
