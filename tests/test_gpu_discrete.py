"""Discrete channels on the MI355X (csrc/discrete.hip) against the specification tests/discrete_f32.py at the same
(seed, call): np.array_equal everywhere (NaN = NaN where pb = 1 makes log(1 - 1 - eps) undefined), except memoryless LLRs
in float64, which use the device log and are held within 2^-52 (|log a| + |log b|) + 2^-53 |llr| - two ulp per log.

Shapes are the smallest at which the kernel can go wrong: the 4-element block and its tail (n = 0, 1, 3, 4, 5, 1023, 1025),
an unaligned view (the element-by-element path), a non-contiguous x, and one element past a whole number of grid trips
(the grid cap is 8192 blocks of 256 lanes of 4 elements: 2^23 elements a trip)."""
import itertools

import numpy as np
import pytest
import torch

import discrete_f32 as spec
import sionna_amd.phy as phy
from sionna_amd import _ffi
from sionna_amd.phy.channel import (BinaryErasureChannel, BinaryMemorylessChannel, BinarySymmetricChannel, BinaryZChannel)

pytestmark = pytest.mark.gpu

CLASSES = {"bmc": BinaryMemorylessChannel, "bsc": BinarySymmetricChannel, "z": BinaryZChannel, "bec": BinaryErasureChannel}
SEED = 77
TRIP = 8192 * 256 * 4
TORCH = {"float32": torch.float32, "float64": torch.float64, "int8": torch.int8, "uint8": torch.uint8, "int16": torch.int16,
         "int32": torch.int32, "int64": torch.int64}


def _bits(shape, bipolar, dtype, seed=5):
    b = np.random.default_rng(seed).integers(0, 2, shape)
    return ((2 * b - 1) if bipolar else b).astype(dtype)


def _split(channel, pb):
    """pb as the block takes it -> (pb0, pb1) for the specification"""
    if channel == "bmc":
        if isinstance(pb, tuple):
            return np.asarray(pb[0]), np.asarray(pb[1])
        pb = np.asarray(pb)
        return pb[..., 0], pb[..., 1]
    pb = np.asarray(pb.cpu() if isinstance(pb, torch.Tensor) else pb)
    return (pb if channel == "bsc" else None), pb


def _expected(channel, x, pb, call, bipolar, llrs, llr_max):
    pb0, pb1 = _split(channel, pb)
    kind = spec.ERASURE if channel == "bec" else spec.MEMORYLESS
    return spec.channel(x, pb0, pb1, SEED, call, kind, bipolar, llrs, llr_max), pb0, pb1


def _run(channel, x, pb, bipolar=False, llrs=False, llr_max=100.0, xt=None):
    """one call of a fresh block at call id 0 of SEED against the specification"""
    precision = "double" if x.dtype == np.float64 else "single"
    phy.config.seed = SEED
    ch = CLASSES[channel](return_llrs=llrs, bipolar_input=bipolar, llr_max=llr_max, precision=precision)
    got = ch(torch.from_numpy(x) if xt is None else xt, pb)
    assert got.dtype == TORCH[x.dtype.name] and tuple(got.shape) == x.shape
    got = got.cpu().numpy()
    want, pb0, pb1 = _expected(channel, x, pb, 0, bipolar, llrs, llr_max)
    if llrs and channel != "bec" and x.dtype == np.float64:
        hard = spec.channel(x, pb0, pb1, SEED, 0, spec.MEMORYLESS, bipolar, False)
        b1 = spec.per_element(x.shape, np.asarray(pb1, np.float64))
        b0 = np.zeros_like(b1) if pb0 is None else spec.per_element(x.shape, np.asarray(pb0, np.float64))
        terms = spec.llr_log_terms(b0, b1, hard.reshape(-1) == 1, np.float64).reshape(x.shape)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        bar = 2.0 ** -52 * terms + 2.0 ** -53 * np.abs(want)
        d = np.abs(got - want)[~nan]
        if d.size:
            print(f"float64 LLR deviation: {d.max():.3e} = {float(np.max(d / bar[~nan])):.3f} of the bar")
        assert np.all(d <= bar[~nan]), (d.max(), channel, bipolar)
    else:
        assert np.array_equal(got, want, equal_nan=x.dtype.kind == "f"), (channel, x.dtype, bipolar, llrs)
    return got


# ------------------------------------------------------------------------------------------------ sizes and launch paths
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1025])
def test_block_and_tail(n):
    for channel, bipolar, llrs in (("bsc", False, False), ("bmc", True, True), ("bec", False, True), ("z", False, False)):
        pb = (0.3, 0.6) if channel == "bmc" else 0.4
        _run(channel, _bits((n,), bipolar, np.float32), pb, bipolar, llrs)
    _run("bsc", _bits((n,), False, np.float64), 0.4, False, True)
    _run("bsc", _bits((n,), False, np.int8), 0.4)
    _run("bmc", _bits((n,), False, np.int64), np.float32([0.2, 0.9]))


@pytest.mark.parametrize("dtype", sorted(TORCH))
def test_unaligned_view_and_non_contiguous_input(dtype):
    """a view starting one element into a buffer is contiguous but not 16-byte aligned: the element-by-element path; a
    strided view is copied on the host"""
    bipolar = dtype != "uint8"
    base = _bits((1030,), bipolar, dtype)
    buf = torch.from_numpy(base).to(_ffi.device())
    view = buf[1:1027]
    assert view.data_ptr() % 16 != 0
    _run("bsc", base[1:1027], 0.3, bipolar, xt=view)
    pb = np.linspace(0, 1, 13, dtype=np.float32)
    grid = _bits((26, 13), bipolar, dtype)
    xt = torch.from_numpy(grid).to(_ffi.device())[::2]
    assert not xt.is_contiguous()
    _run("z", np.ascontiguousarray(grid[::2]), pb, bipolar, xt=xt)


@pytest.mark.parametrize("channel,dtype,llrs", [("bsc", "float32", False), ("bmc", "float32", True), ("bec", "int8", False)])
def test_one_element_past_a_whole_number_of_grid_trips(channel, dtype, llrs):
    n = TRIP + 1
    x = _bits((n,), False, dtype)
    pb = np.float32([[0.1, 0.2], [0.5, 0.01], [0.0, 1.0]]) if channel == "bmc" else np.float32([0.25, 0.0, 0.75])
    # a per-position pb whose period (3) does not divide the trip: the position in the period carries across trips
    assert n % 3 == 0
    got = _run(channel, x.reshape(-1, 3), pb, False, llrs)
    assert got.size == TRIP + 1


# ------------------------------------------------------------------------------------------------ every mode
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("channel", sorted(CLASSES))
def test_all_modes_float(channel, dtype):
    """binary / bipolar, hard / LLR, llr_max 0, 20 and 100 (the clip at pb = 0), pb values 0, 1, NaN and 1e-10 (threshold 1)
    among per-position values"""
    B, C, n = 3, 2, 37
    vals = np.array([0, 1, np.nan, 1e-10, 0.5, 1e-7, 0.99, 0.01, 0.3, 2.0, -1.0], dtype)
    rng = np.random.default_rng(11)
    for bipolar, llrs in itertools.product((False, True), repeat=2):
        x = _bits((B, C, n), bipolar, dtype)
        for llr_max in ((0.0, 20.0, 100.0) if llrs else (100.0,)):
            pb = rng.choice(vals, (n, 2) if channel == "bmc" else (n,))
            _run(channel, x, pb, bipolar, llrs, llr_max)


@pytest.mark.parametrize("dtype", ["int8", "uint8", "int16", "int32", "int64"])
@pytest.mark.parametrize("channel", sorted(CLASSES))
def test_all_modes_integer(channel, dtype):
    for bipolar in (False, True):
        if dtype == "uint8" and (bipolar or channel == "bec"):
            continue
        x = _bits((5, 41), bipolar, dtype)
        pb = np.float32([[0.2, 0.7]] * 41) if channel == "bmc" else np.linspace(0, 1, 41, dtype=np.float32)
        _run(channel, x, pb, bipolar)


@pytest.mark.parametrize("value", [0.0, 1.0, float("nan"), 1e-10])
def test_scalar_pb_edges(value):
    n = 4099
    x = _bits((n,), False, np.float32)
    y = _run("bsc", x, value)
    flips = int((y != x).sum())
    assert flips == (n if value == 1.0 else 0)          # 1e-10: threshold 1, P(e) = 2^-32
    _run("bec", x, value, llrs=True)
    _run("bmc", x, (value, 0.5), llrs=True, llr_max=20.0)
    _run("z", x.astype(np.float64), value, llrs=True)


def test_pb_forms():
    B, C, n = 4, 3, 29
    rng = np.random.default_rng(2)
    x = _bits((B, C, n), False, np.float32)
    f = lambda *s: rng.random(s).astype(np.float32)
    for channel in ("bsc", "z", "bec"):
        for pb in (0.3, torch.tensor(0.3), f(n), f(C, n), f(B, C, n), f(B, 1, n), f(C, 1), f(1, 1, 1)):
            _run(channel, x, pb)
    for pb in ((0.2, 0.6), np.float32([0.2, 0.6]), f(n, 2), f(C, n, 2), f(B, C, n, 2), f(B, 1, n, 2), (f(n), f(n)), (0.3, f(C, n))):
        _run("bmc", x, pb, llrs=True)
    x64 = x.astype(np.float64)
    _run("bmc", x64, rng.random((B, 1, n, 2)), llrs=True)
    _run("bec", x64, rng.random((C, n)))


def test_float_input_of_the_other_precision_keeps_its_dtype():
    x = _bits((3, 50), False, np.float64)
    phy.config.seed = SEED
    y = BinarySymmetricChannel(return_llrs=True)(torch.from_numpy(x), 0.2)            # computed in float32
    assert y.dtype == torch.float64
    want = spec.channel(x.astype(np.float32), 0.2, 0.2, SEED, 0, return_llrs=True)
    assert np.array_equal(y.cpu().numpy(), want.astype(np.float64))
    phy.config.seed = SEED
    y = BinaryErasureChannel(precision="double")(torch.from_numpy(x.astype(np.float32)), 0.2)
    assert y.dtype == torch.float32
    assert np.array_equal(y.cpu().numpy(), spec.channel(x, None, 0.2, SEED, 0, kind=spec.ERASURE).astype(np.float32))
    phy.config.seed = SEED
    y = BinaryZChannel()(x.astype(np.int32), 0.6)                                     # NumPy input
    assert y.dtype == torch.int32 and np.array_equal(y.cpu().numpy(), spec.channel(x.astype(np.int32), None, 0.6, SEED, 0))


def test_consecutive_calls_differ_and_reproduce():
    x = _bits((2000,), False, np.float32)
    xt = torch.from_numpy(x)
    phy.config.seed = SEED
    ch = BinarySymmetricChannel()
    a, b = ch(xt, 0.5).cpu().numpy(), ch(xt, 0.5).cpu().numpy()
    assert not np.array_equal(a, b)
    assert np.array_equal(a, spec.channel(x, 0.5, 0.5, SEED, 0)) and np.array_equal(b, spec.channel(x, 0.5, 0.5, SEED, 1))
    phy.config.seed = SEED
    assert np.array_equal(ch(xt, 0.5).cpu().numpy(), a) and np.array_equal(ch(xt, 0.5).cpu().numpy(), b)


def test_in_place_entry_and_c_level_refusals():
    """y may be x; the argument checks of the C entries"""
    lib = _ffi.lib()
    x = torch.from_numpy(_bits((1025,), False, np.float32)).to(_ffi.device())
    pb = torch.tensor([0.3], device=x.device)
    want = spec.channel(x.cpu().numpy(), 0.3, 0.3, 9, 4)
    args = lambda **k: [k.get("x", x.data_ptr()), pb.data_ptr(), pb.data_ptr(), k.get("stride", 1), k.get("plen", 1), k.get("kind", 0),
                        k.get("bipolar", 0), k.get("llrs", 0), k.get("llr_max", 100.0), 9, 4, k.get("n", x.numel()), x.data_ptr(), _ffi.stream()]
    for bad in (dict(x=None), dict(stride=0), dict(plen=0), dict(kind=2), dict(llr_max=-1.0), dict(llr_max=float("nan")), dict(n=-1)):
        assert lib.samd_discrete_channel_f32(*args(**bad)) == _ffi.ERR_INVALID, bad
    u = torch.zeros(8, dtype=torch.uint8, device=x.device)
    for bad in (dict(llrs=1), dict(bipolar=1), dict(kind=1)):
        a = args(**bad)
        a[0] = a[12] = u.data_ptr()
        a[11] = 8
        assert lib.samd_discrete_channel_u8(*a) == _ffi.ERR_INVALID, bad
    assert lib.samd_discrete_channel_f32(*args(n=0)) == _ffi.OK
    assert lib.samd_discrete_channel_f32(*args()) == _ffi.OK
    assert np.array_equal(x.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ refusals at the block
def test_block_refusals():
    x = torch.zeros(8)
    with pytest.raises(ValueError, match="Last dim of pb must be of length 2"):
        BinaryMemorylessChannel()(x, 0.1)
    with pytest.raises(ValueError, match="Last dim of pb must be of length 2"):
        BinaryMemorylessChannel()(x, (0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match="Last dim of pb must be of length 2"):
        BinaryMemorylessChannel()(x, torch.zeros(8, 3))
    with pytest.raises(ValueError, match="does not broadcast"):
        BinarySymmetricChannel()(x, torch.zeros(5))
    with pytest.raises(ValueError, match="Input must be binary"):
        BinarySymmetricChannel()(torch.tensor([0., 1., 2.]), 0.1)
    with pytest.raises(ValueError, match="Input must be binary"):
        BinarySymmetricChannel(bipolar_input=True)(torch.tensor([0., 1., -1.]), 0.1)
    ch = BinaryErasureChannel()
    ch(torch.tensor([0., 1.]), 0.1)
    ch(torch.tensor([0., 3.]), 0.1)                 # discrete_channel.py:148-149: the check runs on the first call only
    with pytest.raises(ValueError, match="LLR outputs require"):
        BinaryZChannel(return_llrs=True)(torch.zeros(4, dtype=torch.int32), 0.1)


# ------------------------------------------------------------------------------------------------ one link with a closed form
def test_hamming_over_bsc_with_ml_decoding_meets_the_closed_form():
    """Hamming (7,4) over BinarySymmetricChannel(return_llrs=True) into OSDecoder at t = 4 (exhaustive = maximum
    likelihood; the code is perfect, so no ties): a block fails iff it has two or more flips.  2e4 blocks at pb = 0.05,
    the count within 4 binomial standard deviations of N (1 - (1-p)^7 - 7 p (1-p)^6); the seed was checked with the
    specification and a brute-force decoder on the CPU."""
    from sionna_amd.phy.fec.linear import OSDecoder
    gm = np.array([[1, 0, 0, 0, 1, 1, 0], [0, 1, 0, 0, 1, 0, 1], [0, 0, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], np.float32)
    N, p = 20000, 0.05
    u = np.random.default_rng(1).integers(0, 2, (N, 4))
    c = ((u @ gm.astype(np.int64)) % 2).astype(np.float32)
    phy.config.seed = 4242
    llr = BinarySymmetricChannel(return_llrs=True)(torch.from_numpy(c), p)
    want = spec.channel(c, p, p, 4242, 0, return_llrs=True)
    assert np.array_equal(llr.cpu().numpy(), want)
    c_hat = OSDecoder(gm, t=4)(llr).cpu().numpy()
    errors = int((c_hat != c).any(axis=1).sum())
    flips = ((want > 0) != (c > 0)).sum(axis=1)
    assert errors == int((flips >= 2).sum())
    pe = 1 - (1 - p) ** 7 - 7 * p * (1 - p) ** 6
    print(f"block errors {errors}, expected {N * pe:.1f} +- {np.sqrt(N * pe * (1 - pe)):.1f}")
    assert abs(errors - N * pe) <= 4 * np.sqrt(N * pe * (1 - pe))
