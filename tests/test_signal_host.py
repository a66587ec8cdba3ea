"""``sionna_amd.phy.signal`` on the CPU against the reference-executed fixture (tests/golden/signal_ref_golden.npz,
tools/gen_signal_ref_golden.py): coefficients and windows, resampling, the specification tests/signal_f32.py of the filter
kernel, the host path of ``convolve`` / ``upfirdn``, aclr and the empirical spectrum, the signatures.

Bars: coefficients and windows within 2^-24 max|h_ref| (both sides round a float64 formula once; absolute, because the
sinc's zero crossings are rounding noise); resampling array_equal; the float32 / float64 specification of convolve per
output (each real component) within (K + 3) u sum_k |h[k]| |x[n - k]|, u = 2^-24 / 2^-53 (signal_f32.running_sum_bound);
aclr, empirical_psd, empirical_aclr 1e-5 relative."""
import json
import os

import numpy as np
import pytest
import torch

import signal_f32 as spec
from sionna_amd.phy import signal as sig

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "signal_ref_golden.npz"))
FILTERS = [str(n) for n in G["filter_names"]]
WINDOWS = [str(n) for n in G["window_names"]]
U32, U53 = 2.0 ** -24, 2.0 ** -53


def make_filter(name, **kw):
    kind, span, sps = name.split("_")[:3]
    span, sps = int(span[1:]), int(sps[1:])
    if kind == "sinc":
        return sig.SincFilter(span, sps, **kw)
    beta = float(name.split("_b")[1])
    return (sig.RaisedCosineFilter if kind == "rc" else sig.RootRaisedCosineFilter)(span, sps, beta, **kw)


def test_fixture_covers_the_singular_branches():
    """sps 4 with beta 0.25 and 0.5 puts a sampling time on t = T / (2 beta) (raised cosine) and t = T / (4 beta) (root)"""
    for name, t0 in (("rc_s8_o4_b0.25", 2.0), ("rc_s8_o4_b0.5", 1.0), ("rrc_s8_o4_b0.25", 1.0), ("rrc_s8_o4_b0.5", 0.5)):
        assert t0 in G[f"filter/{name}/sampling_times"], name
    assert {"rc_s8_o4_b0.0", "rc_s8_o4_b1.0", "rrc_s8_o4_b0.0", "rrc_s8_o4_b1.0"} <= set(FILTERS)
    assert os.path.getsize(os.path.join(GOLD, "signal_ref_golden.npz")) < 512 * 1024


@pytest.mark.parametrize("name", FILTERS)
def test_coefficients(name):
    f = make_filter(name)
    ref = G[f"filter/{name}/coefficients"]
    got = f.coefficients.numpy()
    assert got.dtype == np.float32 and f.length == len(ref) and f.length % 2 == 1
    assert np.array_equal(f.sampling_times, G[f"filter/{name}/sampling_times"]) and f.sampling_times.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref).max()
    print(name, "max |h - h_ref| =", err, "bar", U32 * np.abs(ref).max())
    assert err <= U32 * np.abs(ref).max()


@pytest.mark.parametrize("name", FILTERS)
def test_taps_after_window_and_normalisation(name):
    """the taps the launch receives (``Filter._taps``): normalised, and Hann-windowed without normalisation; the fixture
    read them back through an impulse.  Bars from the roundings: both sides normalise by a float32 sum of K squares
    (relative error (K + 1) u at most, halved by the root), a root, a division, on coefficients one u apart: (K + 7) u in
    all; the window is a product of two factors each one u apart, rounded once on either side: 3 u of the raw peak."""
    for kw, key in (({}, "taps"), ({"window": "hann", "normalize": False}, "taps_hann_raw")):
        ref = G[f"filter/{name}/{key}"]
        got = make_filter(name, **kw)._taps().numpy()
        assert got.dtype == np.float32
        bar = (len(ref) + 7) * U32 * np.abs(ref).max() if not kw else 3 * U32 * np.abs(G[f"filter/{name}/coefficients"]).max()
        err = np.abs(got.astype(np.float64) - ref).max()
        print(name, key, err, bar)
        assert err <= bar
    assert abs(float(np.sum(make_filter(name)._taps().numpy().astype(np.float64) ** 2)) - 1) < 1e-6


@pytest.mark.parametrize("name", FILTERS)
def test_aclr(name):
    for kw, key in (({}, "aclr"), ({"window": "hann", "normalize": False}, "aclr_hann_raw")):
        got, ref = float(make_filter(name, **kw).aclr), float(G[f"filter/{name}/{key}"])
        print(name, key, got, ref)
        assert abs(got - ref) <= 1e-5 * abs(ref)


@pytest.mark.parametrize("name", WINDOWS)
def test_windows(name):
    kind, n, norm = name.split("_")
    cls = {"hann": sig.HannWindow, "hamming": sig.HammingWindow, "blackman": sig.BlackmanWindow}[kind]
    w = cls(normalize=norm == "norm")
    got = w(torch.ones(int(n))).numpy()
    ref = G[f"window/{name}"]
    assert got.dtype == np.float32 and w.length == int(n) and w.normalize == (norm == "norm")
    bar = (int(n) + 7 if norm == "norm" else 1) * U32 * np.abs(ref).max()   # normalised: a float32 mean of n squares, root, division
    assert np.abs(got.astype(np.float64) - ref).max() <= bar
    if norm == "raw":
        assert np.abs(w.coefficients.numpy().astype(np.float64) - G[f"window/{name}/coefficients"]).max() <= U32 * np.abs(ref).max()
    else:
        assert abs(np.mean(got.astype(np.float64) ** 2) - 1) < 1e-6


def test_custom_window_on_complex_input_and_length():
    w = sig.CustomWindow(np.linspace(0.5, 1.5, 9).astype(np.float32), normalize=True)
    y = w(torch.from_numpy(G["window/custom_x"])).numpy()
    ref = G["window/custom_y"]
    assert y.dtype == np.complex64 and np.abs(y - ref).max() <= (9 + 7 + 2) * U32 * np.abs(ref).max()
    assert sig.CustomWindow(np.ones(5), precision="double").coefficients.dtype == torch.float64


def test_resampling_is_exact():
    x = torch.from_numpy(G["resample/x"])
    cases = [("up3_last", sig.Upsampling(3)), ("up2_axis1", sig.Upsampling(2, axis=1)), ("down4", sig.Downsampling(4)),
             ("down4_off2", sig.Downsampling(4, offset=2)), ("down3_off5_num4", sig.Downsampling(3, offset=5, num_symbols=4)),
             ("down2_off1_num100_axis1", sig.Downsampling(2, offset=1, num_symbols=100, axis=1))]
    for key, block in cases:
        got = block(x).numpy()
        assert got.dtype == np.complex64 and np.array_equal(got, G["resample/" + key]), key
    assert np.array_equal(spec.upsample(G["resample/x"], 3), G["resample/up3_last"])


CONV = [(prec, xn, hn, k, pad) for prec in ("single", "double") for xn in ("real", "complex") for hn in ("real", "complex")
        for k in (5, 4, 33) for pad in ("full", "same", "valid")]


@pytest.mark.parametrize("prec,xn,hn,k,pad", CONV)
def test_convolve_specification_and_host_path(prec, xn, hn, k, pad):
    """the NumPy specification against the fixture within the running-sum bound, per real component; the package's host
    path (torch on the CPU) equals the specification bit for bit; the output is real only if both inputs are"""
    rd, unit = (np.float32, U32) if prec == "single" else (np.float64, U53)
    x, h = G[f"conv/{prec}/x_{xn}"], G[f"conv/{prec}/h_{hn}_{k}"]
    ref = G[f"conv/{prec}/y_{xn}_{hn}_{k}_{pad}"]
    got = spec.convolve(x, h, pad, rd)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert np.iscomplexobj(got) == (xn == "complex" or hn == "complex")
    bound = spec.running_sum_bound(x, h, pad, unit)
    d = got.astype(np.complex128) - ref
    worst = max((np.abs(d.real) / bound).max(), (np.abs(d.imag) / bound).max())
    print(prec, xn, hn, k, pad, "max error / bound =", worst)
    assert worst <= 1
    host = sig.convolve(torch.from_numpy(x), torch.from_numpy(h), padding=pad.upper(), precision=prec)
    assert not host.is_cuda and np.array_equal(host.numpy(), got)


@pytest.mark.parametrize("prec", ["single", "double"])
def test_convolve_inner_axis(prec):
    rd, unit = (np.float32, U32) if prec == "single" else (np.float64, U53)
    x, h = G[f"conv/{prec}/x_axis"], G[f"conv/{prec}/h_axis"]
    for axis, xin, pad, key in ((1, x, "same", "y_axis1_same"), (0, np.swapaxes(x, 0, 1), "full", "y_axis0_full")):
        ref = G[f"conv/{prec}/{key}"]
        got = sig.convolve(torch.from_numpy(np.ascontiguousarray(xin)), torch.from_numpy(h), pad, axis=axis, precision=prec).numpy()
        assert got.shape == ref.shape and got.dtype == ref.dtype
        moved = np.swapaxes(xin, axis, -1)
        assert np.array_equal(np.swapaxes(got, axis, -1), spec.convolve(moved, h, pad, rd))
        bound = np.swapaxes(spec.running_sum_bound(moved, h, pad, unit), axis, -1)
        d = got.astype(np.complex128) - ref
        assert (np.abs(d.real) <= bound).all() and (np.abs(d.imag) <= bound).all()


UPFIRDN = [(4, 1), (1, 4), (3, 2), (2, 3)]


@pytest.mark.parametrize("up,down", UPFIRDN)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_upfirdn_equals_the_three_steps(up, down, dtype):
    """one evaluation of the formula = zero insertion, convolution, decimation, bit for bit, in the specification and on the
    package's host path; offsets 0, 1 and one >= down, num_symbols set and unset, the three paddings, conjugated taps"""
    rng = np.random.default_rng(up * 10 + down)
    prec = "single" if dtype == np.float32 else "double"
    x = (rng.normal(size=(2, 37)) + 1j * rng.normal(size=(2, 37)))
    for k, hc in ((9, True), (4, False)):
        h = rng.normal(size=k) + (1j * rng.normal(size=k) if hc else 0)
        for offset in (0, 1, down + 2):
            for num in (None, 5):
                for pad in ("full", "same", "valid"):
                    for conj in (False, True):
                        ref = spec.three_step(x, h, up, down, offset, num, pad, conj, dtype)
                        got = spec.fused(x, h, up, down, offset, num, pad, conj, dtype)
                        assert got.shape == ref.shape and np.array_equal(got, ref), (k, offset, num, pad, conj)
                        cd = np.complex64 if dtype == np.float32 else np.complex128
                        host = sig.upfirdn(torch.from_numpy(x.astype(cd)), torch.from_numpy(h.astype(cd if hc else dtype)), up, down,
                                           offset, num, pad, conj, precision=prec)
                        assert np.array_equal(host.numpy(), ref)


def test_filter_blocks_on_the_host_equal_convolve():
    rng = np.random.default_rng(3)
    x = torch.from_numpy((rng.normal(size=(2, 50)) + 1j * rng.normal(size=(2, 50))).astype(np.complex64))
    f = sig.RootRaisedCosineFilter(4, 4, 0.3)
    for pad in ("full", "same", "valid"):
        y = f(x, pad)
        assert np.array_equal(y.numpy(), spec.convolve(x.numpy(), f._taps().numpy(), pad))
    c = sig.CustomFilter(2, (rng.normal(size=5) + 1j * rng.normal(size=5)).astype(np.complex64), normalize=False)
    assert c.coefficients.dtype == torch.complex64 and c.span_in_symbols == 2
    assert np.array_equal(c(x, "same", conjugate=True).numpy(), spec.convolve(x.numpy(), np.conj(c.coefficients.numpy()), "same"))
    with pytest.raises(AssertionError):
        sig.CustomFilter(2, np.ones(4, np.float32))
    with pytest.raises(AssertionError):
        sig.SincFilter(4, 4, window="kaiser")
    with pytest.raises(AssertionError):
        sig.SincFilter(4, 4, window=sig.HannWindow(precision="double"))
    with pytest.raises(AssertionError):
        sig.convolve(x, torch.ones(3), padding="circular")


def test_raised_cosine_honours_precision():
    """deliberate difference: the reference passes ``precision`` under a misspelt keyword"""
    f = sig.RaisedCosineFilter(4, 4, 0.3, precision="double")
    assert f.precision == "double" and f.coefficients.dtype == torch.float64
    y = f(torch.ones(20, dtype=torch.complex64))
    assert y.dtype == torch.complex128


def test_empirical_spectrum():
    x = torch.from_numpy(G["psd/x"])
    freqs, psd = sig.empirical_psd(x, show=False, oversampling=4.0)
    assert freqs.dtype == torch.float32 and psd.dtype == torch.float32
    assert np.abs(freqs.numpy() - G["psd/freqs"]).max() <= 1e-5 * np.abs(G["psd/freqs"]).max()
    assert (np.abs(psd.numpy() - G["psd/psd"]) <= 1e-5 * G["psd/psd"].max()).all()
    for kw, key in (({}, "aclr"), ({"f_min": -0.7, "f_max": 0.6}, "aclr_band")):
        got = float(sig.empirical_aclr(x, oversampling=4.0, **kw))
        assert abs(got - float(G["psd/" + key])) <= 1e-5 * float(G["psd/" + key])
    xf = torch.from_numpy(G["fft/x"])
    assert np.abs(sig.fft(xf).numpy() - G["fft/fft"]).max() <= 1e-5 * np.abs(G["fft/fft"]).max()
    assert np.abs(sig.ifft(xf, axis=0).numpy() - G["fft/ifft_axis0"]).max() <= 1e-5 * np.abs(G["fft/ifft_axis0"]).max()


def test_signatures_match_the_reference():
    from test_api_signatures import _check
    with open(os.path.join(GOLD, "signal_api_signatures.json")) as f:
        table = json.load(f)["signatures"]
    assert len(table) == 17
    for name, ref in table.items():
        obj = getattr(sig, name.split(".")[1])
        if ref["kind"] == "function":
            _check(ref["params"], obj, name)
            continue
        _check(ref["__init__"], obj.__init__, name + ".__init__")
        if "call" in ref:
            _check(ref["call"], obj.call, name + ".call")
        for attr, kind, prm in ref["public"]:
            assert hasattr(obj, attr), f"{name}.{attr}"
            if kind == "property":
                assert isinstance(getattr(obj, attr), property), f"{name}.{attr}"
            else:
                _check(prm, getattr(obj, attr), f"{name}.{attr}")
    assert "signal.upfirdn" not in table and callable(sig.upfirdn)


def test_matplotlib_is_imported_only_to_plot():
    import subprocess
    import sys
    code = ("import sys, torch; from sionna_amd.phy import signal as s; f = s.RootRaisedCosineFilter(4, 4, 0.3, window='hann'); "
            "f.aclr; s.empirical_psd(torch.ones(8, dtype=torch.complex64), show=False); assert 'matplotlib' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.join(os.path.dirname(__file__), ".."))


def test_import_path_under_install_as_sionna():
    import sionna_amd
    sionna_amd.install_as_sionna()
    from sionna.phy.signal import RootRaisedCosineFilter, Upsampling, convolve
    assert RootRaisedCosineFilter is sig.RootRaisedCosineFilter and Upsampling is sig.Upsampling and convolve is sig.convolve
