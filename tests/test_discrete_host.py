"""Discrete channels on the CPU: the specification tests/discrete_f32.py against the reference-executed fixture
(tests/golden/discrete_ref_golden.npz, tools/gen_discrete_ref_golden.py), the statistics of its draw and of the reference's
recorded draw against the law, the index rule of pb, the signatures and the refusals.

Bars.  Hard outputs and erasure LLRs: equality.  Memoryless float32 LLRs: the reference's own single-precision result
against its own double-precision result on the same float32 probabilities, e32 = max |ref32 - ref64| over the case, times
2, plus one float32 ulp at the element's |LLR| (the convention of test_turbo_host.py).  Float64: 2^-52 (|log a| + |log b|)
of the two logs an LLR is the difference of.  Statistics: |k - N P(e)| <= 5 sqrt(N P(e) (1 - P(e))) + 1, P(e) =
ceil(p 2^32) / 2^32 for the specification and the reference's (pb + 1e-9) / (1 + 2e-9) for its recorded counts."""
import json
import os

import numpy as np
import pytest
import torch

import discrete_f32 as spec
from sionna_amd.phy.channel import (BinaryErasureChannel, BinaryMemorylessChannel, BinarySymmetricChannel, BinaryZChannel)
from sionna_amd.phy.channel.discrete_channel import _trailing_block

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "discrete_ref_golden.npz"))
META = json.loads(str(G["meta"]))
BITS, PATTERN = G["bits"].astype(np.int64), G["pattern"]
CLASSES = {"bmc": BinaryMemorylessChannel, "bsc": BinarySymmetricChannel, "z": BinaryZChannel, "bec": BinaryErasureChannel}
SEED = 20261020
N = 200000


def _pb01(channel, pb, x):
    """pb0 / pb1 per element of x in the compute dtype, from pb as the block was given it"""
    P = spec.compute_dtype(x.dtype)
    pb = np.asarray(pb, P)
    if channel == "bmc":
        return spec.per_element(x.shape, pb[..., 0]), spec.per_element(x.shape, pb[..., 1])
    b1 = spec.per_element(x.shape, pb)
    return (b1 if channel == "bsc" else np.zeros_like(b1)), b1


def _spec_on_pattern(m, dtype):
    x = ((2 * BITS - 1) if m["bipolar"] else BITS).astype(dtype)
    b0, b1 = _pb01(m["channel"], G[m["key"] + "/pb"], x)
    kind = spec.ERASURE if m["channel"] == "bec" else spec.MEMORYLESS
    y, e = spec.apply(x, b0, b1, PATTERN, kind, m["bipolar"], m["llrs"], m["llr_max"], pattern=True)
    assert np.array_equal(e, PATTERN != 0) and y.dtype == np.dtype(dtype) and y.shape == x.shape
    return x, b0, b1, y


def test_fixture_covers_what_it_should():
    seen = {(m["channel"], m["bipolar"], m["llrs"]) for m in META if m["dtype"] == "float"}
    assert seen == {(c, b, l) for c in CLASSES for b in (False, True) for l in (False, True)}
    assert {m["llr_max"] for m in META if m["llrs"]} == {20.0, 100.0}
    assert {m["dtype"] for m in META} == {"float", "int8", "uint8", "int16", "int32", "int64"}
    forms = {m["form"] for m in META}
    assert forms >= {"scalar0", "position", "full", "pair0", "position2", "full2", "int"}
    scal = {float(G[m["key"] + "/pb"]) for m in META if m["form"].startswith("scalar")}
    assert scal == {float(np.float32(v)) for v in (0, 1, 0.5, 1e-7, 0.99)}
    assert any(np.array_equal(G[m["key"] + "/pb"], np.float32([0.01, 0.99])) for m in META)
    assert 0.3 < PATTERN.mean() < 0.7


@pytest.mark.parametrize("m", [m for m in META if not m["llrs"] or m["channel"] == "bec"], ids=lambda m: m["key"])
def test_hard_outputs_and_erasure_llrs_equal_the_reference(m):
    for dtype, key in ((("float32", "/y32"), ("float64", "/y64")) if m["dtype"] == "float" else ((m["dtype"], "/y"),)):
        ref = G[m["key"] + key]
        _, _, _, y = _spec_on_pattern(m, dtype)
        assert ref.dtype == y.dtype and np.array_equal(y, ref), (m, dtype)


@pytest.mark.parametrize("m", [m for m in META if m["llrs"] and m["channel"] != "bec"], ids=lambda m: m["key"])
def test_memoryless_llrs_within_the_reference_s_own_error(m):
    r32, r64 = G[m["key"] + "/y32"], G[m["key"] + "/y64"]
    nan = np.isnan(r64)
    assert np.array_equal(np.isnan(r32), nan)                      # pb = 1: log(1 - 1 - eps) in either precision
    # float32
    _, _, _, y = _spec_on_pattern(m, np.float32)
    assert np.array_equal(np.isnan(y), nan)
    ok = ~nan
    e32 = np.max(np.abs(r32[ok].astype(np.float64) - r64[ok])) if ok.any() else 0.0
    bar = 2 * e32 + np.spacing(np.abs(r64[ok]).astype(np.float32)).astype(np.float64)
    d = np.abs(y[ok].astype(np.float64) - r64[ok])
    print(m["key"], m["channel"], m["form"], f"e32 {e32:.3e} spec32 - ref64 {d.max() if d.size else 0:.3e}")
    assert np.all(d <= bar), (m, d.max(), bar.min())
    # float64
    x, b0, b1, y = _spec_on_pattern(m, np.float64)
    assert np.array_equal(np.isnan(y), nan)
    received_one = (x.reshape(-1) * (1 - 2 * (PATTERN.reshape(-1) != 0)) == 1) if m["bipolar"] else \
        (np.abs(x.reshape(-1) - (PATTERN.reshape(-1) != 0)) == 1)
    bar = 2.0 ** -52 * spec.llr_log_terms(b0, b1, received_one, np.float64).reshape(y.shape)
    d = np.abs(y - r64)
    assert np.all(d[ok] <= bar[ok]), (m, d[ok].max())
    assert np.all(np.abs(y[ok]) <= m["llr_max"])


def test_clip_reaches_llr_max_at_pb_zero():
    """pb = 0: log((1 - eps) / eps) = 20.72 is cut at llr_max = 20 and passes at 100"""
    x = BITS.astype(np.float32)
    z = np.zeros(x.size, np.float32)
    y20, _ = spec.apply(x, z, z, PATTERN * 0, return_llrs=True, llr_max=20.0, pattern=True)
    y100, _ = spec.apply(x, z, z, PATTERN * 0, return_llrs=True, llr_max=100.0, pattern=True)
    assert np.array_equal(y20, 20 * (2 * x - 1))
    assert np.all(np.abs(np.abs(y100) - 20.7232658) < 1e-5) and np.array_equal(np.sign(y100), 2 * x - 1)
    y0, _ = spec.apply(x, z, z, PATTERN * 0, return_llrs=True, llr_max=0.0, pattern=True)
    assert not y0.any()


# ------------------------------------------------------------------------------------------------ the law
def _bound(n, p):
    return 5 * np.sqrt(n * p * (1 - p)) + 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_spec_draw_follows_the_law_scalar(dtype):
    x = np.zeros(N, dtype)
    for call, pb in enumerate(G["law_pb"]):
        y = spec.channel(x, pb, pb, SEED, call)
        k, p = int((y != x).sum()), float(spec.event_probability(pb, dtype))
        print(f"pb {pb}: {k} events, N P(e) = {N * p:.1f}, bound {_bound(N, p):.1f}")
        assert abs(k - N * p) <= _bound(N, p)
        if pb == 0:
            assert k == 0
        if pb == 1:
            assert k == N


def test_reference_counts_follow_the_law():
    n = int(G["law_n"])
    assert n == N and list(G["law_pb"]) == [0, 1e-3, 0.1, 0.5, 0.95, 1]
    for pb, k in zip(G["law_pb"], G["law_counts"]):
        p = (pb + 1e-9) / (1 + 2e-9)                # two Gumbel variables at log(pb + eps) and log(1 - pb + eps)
        assert abs(k - n * p) <= _bound(n, p), (pb, k)
    assert G["law_counts"][0] == 0 and G["law_counts"][-1] == n


PB_TUPLES = [(0.2, 0.4), (0.95, 0.2), (1.0, 0.0), ((0.1, 0.1, 0.1, 0.8), (0.4, 0.2, 0.3, 0.8)),
             (((0.2, 0.7, 0.0, 0.5), (0.02, 0.4, 0.9, 0.3)), ((0.2, 0.3, 0.1, 0.0), (0.2, 0.7, 0.2, 0.3)))]


@pytest.mark.parametrize("bipolar", [False, True])
@pytest.mark.parametrize("idx", range(len(PB_TUPLES)))
def test_spec_draw_follows_the_law_per_position(idx, bipolar):
    """the pb tuples of the reference's test_pb (test_discrete_channel.py:162-206) on x of shape [N, 2, 4]: all-neutral
    input counts the pb0 events, all-one input the pb1 events, per position"""
    pb0, pb1 = (np.asarray(v, np.float32) for v in PB_TUPLES[idx])
    for call, (value, pb) in enumerate((((-1 if bipolar else 0), pb0), (1, pb1))):
        x = np.full((N, 2, 4), value, np.float32)
        y = spec.channel(x, pb0, pb1, SEED + idx, call, bipolar=bipolar)
        assert set(np.unique(y)) <= {-1.0 if bipolar else 0.0, 1.0}
        k = (y != x).sum(axis=0)
        p = np.broadcast_to(spec.event_probability(pb), (2, 4))
        assert np.all(np.abs(k - N * p) <= _bound(N, p)), (k, N * p)
        assert np.all(k[p == 0] == 0) and np.all(k[p == 1] == N)


def test_threshold_edges():
    f = np.float32
    assert list(spec.threshold(spec.unit_clip(f([0, 1, np.nan, -0.5, 2, 1e-10, 0.5])))) == [0, 2 ** 32, 0, 0, 2 ** 32, 1, 2 ** 31]
    assert list(spec.threshold(spec.unit_clip(np.float64([0, 1, np.nan, 1e-10, 2.0 ** -33])))) == [0, 2 ** 32, 0, 1, 1]
    p = f(0.1)
    assert p <= spec.event_probability(p) < float(p) + 2.0 ** -32
    # the erasure channel rounds pb to float32 in double precision too
    x = np.zeros(4096, np.float64)
    pb = np.full(4096, 0.3)
    a = spec.channel(x, None, pb, 5, 0, kind=spec.ERASURE)
    b = spec.channel(x.astype(np.float32), None, pb.astype(np.float32), 5, 0, kind=spec.ERASURE)
    assert np.array_equal(a, b) and set(np.unique(a)) == {-1.0, 0.0}


# ------------------------------------------------------------------------------------------------ pb indexing
@pytest.mark.parametrize("x_shape,pb_shape,plen", [
    ((2, 3, 5), (), 1), ((2, 3, 5), (1,), 1), ((2, 3, 5), (1, 1, 1), 1), ((2, 3, 5), (5,), 5), ((2, 3, 5), (3, 5), 15),
    ((2, 3, 5), (2, 3, 5), 30), ((2, 3, 5), (2, 1, 5), 30), ((2, 3, 5), (1, 3, 1), 15), ((2, 3, 5), (3, 1), 15),
    ((2, 3, 5), (1, 1, 5), 5), ((7,), (7,), 7), ((1025,), (), 1)])
def test_index_rule_is_broadcasting(x_shape, pb_shape, plen):
    pb = np.random.default_rng(3).random(pb_shape).astype(np.float32)
    assert spec.pb_period(x_shape, pb_shape)[1] == plen
    assert np.array_equal(spec.per_element(x_shape, pb), np.broadcast_to(pb, x_shape).reshape(-1))
    s, block = _trailing_block(x_shape, pb_shape)                     # the block's own version of the rule
    assert int(np.prod(block, dtype=np.int64)) == plen and block == spec.pb_period(x_shape, pb_shape)[0]


def test_pb_that_does_not_broadcast_is_refused():
    for x_shape, pb_shape in (((2, 3, 5), (4,)), ((2, 3, 5), (2, 5)), ((5,), (1, 5))):
        with pytest.raises(ValueError):
            _trailing_block(x_shape, pb_shape)
        with pytest.raises(ValueError):
            spec.pb_period(x_shape, pb_shape)


# ------------------------------------------------------------------------------------------------ interface
def test_signatures_match_the_reference():
    from test_api_signatures import _check
    with open(os.path.join(GOLD, "discrete_api_signatures.json")) as f:
        sig = json.load(f)["signatures"]
    assert set(sig) == {"channel." + c.__name__ for c in CLASSES.values()}
    for cls in CLASSES.values():
        ref = sig["channel." + cls.__name__]
        _check(ref["__init__"], cls.__init__, cls.__name__ + ".__init__")
        _check(ref["call"], cls.call, cls.__name__ + ".call")
    assert [a for a, _, _ in sig["channel.BinaryMemorylessChannel"]["public"]] == ["llr_max", "temperature"]
    for cls in CLASSES.values():
        for attr in ("llr_max", "temperature"):
            assert isinstance(getattr(cls, attr), property) and getattr(cls, attr).fset is not None


def test_properties_round_to_the_precision():
    ch = BinarySymmetricChannel(llr_max=20.1)
    assert ch.llr_max == float(np.float32(20.1)) and ch.temperature == float(np.float32(0.1))
    ch.llr_max, ch.temperature = 7, 0.5
    assert ch.llr_max == 7.0 and ch.temperature == 0.5
    assert BinaryErasureChannel(llr_max=20.1, precision="double").llr_max == 20.1


@pytest.mark.parametrize("cls", CLASSES.values())
def test_negative_llr_max_is_refused(cls):
    with pytest.raises(AssertionError):
        cls(llr_max=-1.0)
    ch = cls()
    with pytest.raises(AssertionError):
        ch.llr_max = -0.5


def test_negative_temperature_is_refused():
    with pytest.raises(AssertionError):
        BinaryZChannel().temperature = -1


def test_flags_must_be_bool():
    with pytest.raises(AssertionError):
        BinarySymmetricChannel(return_llrs=1)
    with pytest.raises(AssertionError):
        BinarySymmetricChannel(bipolar_input="yes")


def test_precision_is_checked():
    with pytest.raises(ValueError):
        BinarySymmetricChannel(precision="half")


@pytest.mark.parametrize("cls", CLASSES.values())
@pytest.mark.parametrize("dtype", [torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64])
def test_llrs_need_a_float_dtype(cls, dtype):
    with pytest.raises(ValueError, match="LLR outputs require non-integer dtypes|Only signed"):
        cls(return_llrs=True)(torch.zeros(4, dtype=dtype), 0.1)


@pytest.mark.parametrize("cls", CLASSES.values())
def test_bipolar_input_needs_a_signed_dtype(cls):
    with pytest.raises(ValueError, match="signed"):
        cls(bipolar_input=True)(torch.ones(4, dtype=torch.uint8), 0.1)


def test_erasure_channel_takes_no_unsigned_dtype():
    with pytest.raises(ValueError, match="Only signed dtypes supported"):
        BinaryErasureChannel()(torch.zeros(4, dtype=torch.uint8), 0.1)


@pytest.mark.parametrize("cls", CLASSES.values())
@pytest.mark.parametrize("x", [torch.zeros(4, dtype=torch.bool), np.zeros(4, np.uint16), np.zeros(4, np.uint32),
                               np.zeros(4, np.uint64), np.zeros(4, bool), torch.zeros(4, dtype=torch.complex64),
                               torch.zeros(4, dtype=torch.float16)], ids=lambda x: str(x.dtype))
def test_uncarried_dtypes_are_refused_by_name(cls, x):
    with pytest.raises(ValueError, match=str(x.dtype).replace("torch.", "")):
        cls()(x, 0.1)


def test_memoryless_build_needs_a_last_dimension_of_two():
    """discrete_channel.py:224-236"""
    for shape in ((), (3,), (4, 3)):
        with pytest.raises(ValueError, match="Last dim of pb must be of length 2"):
            BinaryMemorylessChannel().build((4,), shape)
    BinaryMemorylessChannel().build((4,), (2,))
    BinaryMemorylessChannel().build((4,), (4, 2))
    for cls in (BinarySymmetricChannel, BinaryZChannel, BinaryErasureChannel):
        cls().build((4,), (3,))
