"""Every kernel variant of ``cir_to_ofdm_channel`` (csrc/ofdm.hip: two-pass, register-staged, pass and fused kernels) against
the float64 anchor of tests/channel_f32.py, on EVERY output, within the bound derived there from the kernels' arithmetic.

The shapes (tests/channel_cases.py) are the smallest that reach each family and each path of the host dispatcher: path-count
class edges, grouped and ungrouped row ownership, one row group, divisors of 1 in the multiply-high divisions, spare lanes,
padded rows, F at and past the block size.  ``kernel_models.c2o_dispatch`` restates the dispatcher; the family of every row is
asserted with it so that a later change of the dispatcher cannot silently move a case (CPU: tests/test_kernel_models.py, which
also shows that the bound is neither too tight nor too loose on these very inputs).

Every table test prints its max |h - anchor| / bound (run with -s).  On an MI355X with ROCm's device library, over the table
and normalize off / on: pass kernel 0.018 ... 0.53, register-staged kernel 0.025 ... 0.09 (0.54 when forced onto the pass
rows), two-pass kernel 0.008 ... 0.55, wide band 0.72.  The large ratios are the rows with few paths and many subcarriers,
where the argument and sin / cos terms are most of the bound; nothing is above 1 and the bound is not idle."""
import types

import numpy as np
import pytest
import torch

import channel_cases as chc
import channel_f32 as chf
import kernel_models as km

pytestmark = pytest.mark.gpu

PASS_SHAPES = [s for s, fam, _ in chc.TABLE if fam == "pass"]
EDGE_SHAPES = [(1, 1, 4, 2, 300), (2, 3, 8, 3, 12)]


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as p
    from sionna_amd import _ffi
    _ffi.device()
    return p


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def case():
    """inputs, anchor and bound of a table row, computed once and shared (read-only)"""
    cache = {}

    def get(shape, normalize):
        key = (shape, normalize)
        if key not in cache:
            fr, a, tau = chc.make(shape)
            ref, bd = chf.anchor(fr, a, tau, normalize), chf.bound(fr, a, tau, normalize)
            for x in (fr, a, tau, ref, bd):
                x.setflags(write=False)
            cache[key] = (fr, a, tau, ref, bd)
        return cache[key]
    return get


def _hold(h, ref, bd, what):
    """|h - anchor| <= bound on every output; returns the largest ratio"""
    h = np.asarray(h)
    assert h.shape == ref.shape and h.dtype == np.complex64, (h.shape, h.dtype)
    assert np.all(np.isfinite(h.view(np.float32))), what
    err = np.abs(h.astype(np.complex128) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = float(np.max(np.where(err == 0, 0.0, err / bd)))
    print(f"c2o {what}: max |h - anchor| / bound = {q:.4f}")
    bad = err > bd
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outputs outside the bound, worst ratio {q:.3f}"
    return q


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape,family,props", chc.TABLE, ids=[chc.sid(s) for s in chc.SHAPES])
def test_table_holds_the_bound(phy, case, shape, family, props, normalize):
    d = km.c2o_dispatch(*shape)
    assert d["family"] == family and all(d[k] == v for k, v in props.items()), d
    fr, a, tau, ref, bd = case(shape, normalize)
    h = _np(phy.channel.cir_to_ofdm_channel(fr, a, tau, normalize=normalize))
    _hold(h, ref, bd, f"{family} {chc.sid(shape)} normalize={normalize}")


def test_wide_band_needs_the_argument_term(phy):
    """F = 512 at 120 kHz, tau up to 5 us: |theta| ~ 1e3 and the rounding of the argument dominates.  The bound holds; the same
    bound with |theta| = 0 is violated, so the term is not decoration."""
    shape = (1, 1, 4, 2, 512)
    assert km.c2o_dispatch(*shape)["family"] == "pass"
    fr, a, tau = chc.make(shape, seed=1, tau_max=5e-6, spacing=120e3)
    assert float(np.max(np.abs(2 * np.pi * fr.astype(np.float64)[:, None] * tau.reshape(1, -1)))) > 900
    for normalize in (False, True):
        h = _np(phy.channel.cir_to_ofdm_channel(fr, a, tau, normalize=normalize))
        ref = chf.anchor(fr, a, tau, normalize)
        _hold(h, ref, chf.bound(fr, a, tau, normalize), f"wide band normalize={normalize}")
        err = np.abs(h.astype(np.complex128) - ref)
        assert np.any(err > chf.bound(fr, a, tau, normalize, theta_scale=0.0))


@pytest.mark.parametrize("shape", PASS_SHAPES, ids=chc.sid)
def test_development_variants(phy, case, shape):
    """SAMD_C2O_PASS = 2 and 8 walk the same chain as the default passes of 4: equal bits.  0 is none of the pass widths: the
    register-staged kernel runs (its own order: within the bound); so does the two-pass kernel under SAMD_C2O_TWO_PASS."""
    from sionna_amd import _ffi
    assert km.c2o_dispatch(*shape, pass_width=0)["family"] == "reg" and km.c2o_dispatch(*shape, two_pass=True)["family"] == "two_pass"
    for normalize in (False, True):
        fr, a, tau, ref, bd = case(shape, normalize)
        h = _np(phy.channel.cir_to_ofdm_channel(fr, a, tau, normalize=normalize))
        for v in (2, 8):
            with _ffi.option("SAMD_C2O_PASS", v):
                hv = _np(phy.channel.cir_to_ofdm_channel(fr, a, tau, normalize=normalize))
            assert np.array_equal(hv.view(np.uint32), h.view(np.uint32)), (v, normalize)
        with _ffi.option("SAMD_C2O_PASS", 0):
            h0 = _np(phy.channel.cir_to_ofdm_channel(fr, a, tau, normalize=normalize))
        _hold(h0, ref, bd, f"reg (SAMD_C2O_PASS=0) {chc.sid(shape)} normalize={normalize}")
        with _ffi.option("SAMD_C2O_TWO_PASS"):
            h2 = _np(phy.channel.cir_to_ofdm_channel(fr, a, tau, normalize=normalize))
        _hold(h2, ref, bd, f"two_pass (SAMD_C2O_TWO_PASS) {chc.sid(shape)} normalize={normalize}")


class _FixedCir:
    """channel-model stub: hands out the given taps and delays"""

    def __init__(self, a, tau):
        self.a, self.tau = a, tau

    def __call__(self, batch_size, num_time_steps, sampling_frequency=None):
        assert batch_size == self.a.shape[0] and num_time_steps == self.a.shape[-1]
        return self.a, self.tau


FUSED_ROWS = [s for s in chc.SHAPES if km.c2o_dispatch(*s)["fused"]]


def _fused_vs_separate(phy, shape):
    ra, ta, p, t, f = shape
    fr, a, tau = chc.make(shape, seed=2, num_tx=1)
    rng = np.random.default_rng(3)
    x = (rng.normal(size=(chc.BATCH, 1, ta, t, f)) + 1j * rng.normal(size=(chc.BATCH, 1, ta, t, f))).astype(np.complex64)
    dev = torch.device("cuda")
    a_t, tau_t, x_t = (torch.from_numpy(v).to(dev) for v in (a, tau, x))
    rg = types.SimpleNamespace(num_ofdm_symbols=t, fft_size=f, subcarrier_spacing=chc.SPACING, ofdm_symbol_duration=1 / chc.SPACING)
    for normalize in (False, True):
        ch = phy.channel.OFDMChannel(_FixedCir(a_t, tau_t), rg, normalize_channel=normalize, return_channel=False)
        y = _np(ch(x_t))
        h = phy.channel.cir_to_ofdm_channel(fr, a_t, tau_t, normalize=normalize)
        y_ref = _np(phy.channel.ApplyOFDMChannel()(x_t, h))
        assert y.shape == (chc.BATCH, chc.NUM_RX, ra, t, f)
        assert np.array_equal(y.view(np.uint32), y_ref.view(np.uint32)), (shape, normalize)
        # and the channel itself is held to the bound with one transmitter too
        _hold(_np(h), chf.anchor(fr, a, tau, normalize), chf.bound(fr, a, tau, normalize), f"one transmitter {chc.sid(shape)}")


@pytest.mark.parametrize("shape", FUSED_ROWS + [(2, 3, 8, 3, 12)], ids=chc.sid)
def test_fused_launch_equals_the_separate_blocks(phy, shape):
    """OFDMChannel(return_channel=False) with one transmitter: ApplyOFDMChannel on the staged registers gives the bits of
    ApplyOFDMChannel on the stored cir_to_ofdm_channel output.  (2, 3, 8, 3, 12) is refused by the fused entry (RPT 8 is no
    multiple of TA 3): the block falls back to the separate entries and still agrees."""
    d = km.c2o_dispatch(*shape)
    assert d["fused"] == (shape != (2, 3, 8, 3, 12)) and d["family"] == "pass"
    _fused_vs_separate(phy, shape)


def test_fused_launch_where_the_separate_entry_leaves_the_pass_kernel(phy):
    """(2, 1, 24, 16, 300): the tables of the pass kernel fit the 64 KB of LDS, the register-staged kernel's do not, so
    samd_cir_to_ofdm_c64 runs the two-pass kernel (another order of the energy sum).  The fused entry took this shape and
    its normalised output differed from the separate blocks in the last bits; it refuses the shape now and the block falls
    back."""
    shape = (2, 1, 24, 16, 300)
    d = km.c2o_dispatch(*shape)
    assert d["family"] == "two_pass" and not d["fused"]
    _fused_vs_separate(phy, shape)


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=chc.sid)
def test_edge_inputs(phy, shape):
    fr, a, tau = chc.make(shape, seed=4)
    run = phy.channel.cir_to_ofdm_channel
    # a link without energy under normalisation: exactly 0, no NaN, the other links keep their bits
    a0 = a.copy()
    a0[1, 0, :, 1] = 0
    h, h0 = _np(run(fr, a, tau, normalize=True)), _np(run(fr, a0, tau, normalize=True))
    assert np.all(np.isfinite(h0.view(np.float32))) and np.all(h0[1, 0, :, 1] == 0)
    keep = np.ones(h.shape, bool)
    keep[1, 0, :, 1] = False
    assert np.array_equal(h0[keep].view(np.uint32), h[keep].view(np.uint32))
    _hold(h0, chf.anchor(fr, a0, tau, True), chf.bound(fr, a0, tau, True), f"zero link {chc.sid(shape)}")
    # one path only
    a1, tau1 = np.ascontiguousarray(a[..., :1, :]), np.ascontiguousarray(tau[..., :1])
    for normalize in (False, True):
        _hold(_np(run(fr, a1, tau1, normalize=normalize)), chf.anchor(fr, a1, tau1, normalize), chf.bound(fr, a1, tau1, normalize),
              f"one path {chc.sid(shape)} normalize={normalize}")
    # tau = 0: cos 0 = 1 and sin 0 = 0 are exact in any library, the output is the plain sum of the taps up to the
    # accumulation term sqrt(2) gamma(2 P + 2) sum |a_p| alone
    tz = np.zeros_like(tau)
    hz = _np(run(fr, a, tz, normalize=False))
    plain = a.astype(np.complex128).sum(axis=5)[..., None]
    acc = np.sqrt(2) * chf._gamma(2 * shape[2] + 2) * np.abs(a.astype(np.complex128)).sum(axis=5)[..., None]
    assert np.all(np.abs(hz.astype(np.complex128) - plain) <= acc)
    _hold(_np(run(fr, a, tz, normalize=True)), chf.anchor(fr, a, tz, True), chf.bound(fr, a, tz, True), f"tau 0 {chc.sid(shape)}")
    # a non-contiguous view of the taps: every second time step of a tensor twice as long
    t = shape[3]
    wide = np.zeros(a.shape[:-1] + (2 * t,), np.complex64)
    wide[..., ::2] = a
    wide[..., 1::2] = 7.0                                              # what a kernel reading the storage as it lies would pick up
    view = torch.from_numpy(wide).cuda()[..., ::2]
    assert not view.is_contiguous()
    for normalize in (False, True):
        hv = _np(run(fr, view, tau, normalize=normalize))
        assert np.array_equal(hv.view(np.uint32), _np(run(fr, a, tau, normalize=normalize)).view(np.uint32))


@pytest.mark.parametrize("shape", chc.SHAPES, ids=chc.sid)
def test_table_in_double_precision(phy, shape):
    """complex128 taps run samd_cir_to_ofdm_c128: the same table against the anchor at the bar of test_gpu_double.py"""
    fr, a, tau = chc.make(shape)
    fr64, a64, tau64 = fr.astype(np.float64), a.astype(np.complex128), tau.astype(np.float64)
    for normalize in (False, True):
        h = phy.channel.cir_to_ofdm_channel(fr64, a64, tau64, normalize=normalize)
        assert h.dtype == torch.complex128
        got, ref = _np(h), chf.anchor(fr, a, tau, normalize)
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert np.allclose(got, ref, rtol=1e-9, atol=1e-9), float(np.max(np.abs(got - ref)))
