"""GPU parity tests of the OFDM / MIMO part of the hot path (north-star config C4) against
oracle/ofdm.py on the same inputs and the same Philox streams.

The reference pins these blocks only statistically or through invariants (SURVEY.md section 4:
LMMSE error statistics, whitening -> identity covariance, TDL power-delay profile, "ber == 0" at
high SNR); the same invariants are asserted here next to the value-level comparison with the
oracle (complex64 arithmetic: rtol 1e-4 / atol 1e-5 unless stated)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ofdm as o, mapping as omap, utils as outil, mimo_f32 as of32
import channel_f32 as chf


def _same_f32(got, ref):
    """Bit-for-bit equality of float32 / complex64 arrays (the sign of a zero is not distinguished)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    if not np.array_equal(got, ref):
        bad = got != ref
        raise AssertionError(f"{bad.mean():.3e} of the entries differ, max |diff| {np.max(np.abs(got[bad] - ref[bad])):.3e} "
                             f"at magnitude {np.max(np.abs(ref[bad])):.3e}")
    return True


def _llr_close(got, ref64):
    """north-star LLR bar (1e-5 relative) with the absolute floor of test_demapper_vs_oracle."""
    return np.allclose(got, ref64, rtol=1e-5, atol=1e-4 * max(1.0, float(np.max(np.abs(ref64))) * 1e-2))


@pytest.fixture(scope="module")
def phy():
    import sionna_amd.phy as p
    from sionna_amd import _ffi
    _ffi.device()
    return p


def _np(t):
    return t.detach().cpu().numpy()


def _grids(phy, num_tx=1, ns=2, fft=76, guards=(5, 6), dc=True, pilots=(2, 11)):
    kw = dict(num_tx=num_tx, num_streams_per_tx=ns, cyclic_prefix_length=6, num_guard_carriers=list(guards),
              dc_null=dc, pilot_pattern="kronecker", pilot_ofdm_symbol_indices=list(pilots))
    return phy.ofdm.ResourceGrid(14, fft, 15e3, **kw), o.ResourceGrid(14, fft, 15e3, **kw)


def _tdl_params(phy, model="A", ds=300e-9):
    t = phy.channel.tr38901.TDL(model, ds, 2.6e9, min_speed=10., num_rx_ant=4, num_tx_ant=2)
    return t


def test_resource_grid_tables_match_oracle(phy):
    for kw in (dict(), dict(num_tx=2, ns=1), dict(fft=64, guards=(0, 0), dc=False, pilots=(0,)), dict(num_tx=2, ns=2, fft=72, guards=(3, 4))):
        rg, org = _grids(phy, **kw)
        assert np.array_equal(rg.build_type_grid(), org.build_type_grid())
        assert np.array_equal(rg.effective_subcarrier_ind, org.effective_subcarrier_ind)
        assert np.allclose(rg.pilot_pattern.pilots, org.pilot_pattern.pilots)
        assert (rg.num_data_symbols, rg.num_pilot_symbols, rg.dc_ind) == (org.num_data_symbols, org.num_pilot_symbols, org.dc_ind)
        assert np.array_equal(phy.ofdm.NearestNeighborInterpolator(rg.pilot_pattern).gather_ind, o.nn_gather_ind(org.pilot_pattern))


def test_rg_mapper_demapper_roundtrip(phy):
    rg, org = _grids(phy, num_tx=2, ns=2, fft=72, guards=(3, 4))
    sm = phy.mimo.StreamManagement([[1, 0], [0, 1]], 2)
    rng = np.random.default_rng(0)
    x = (rng.normal(size=(5, 2, 2, rg.num_data_symbols)) + 1j * rng.normal(size=(5, 2, 2, rg.num_data_symbols))).astype(np.complex64)
    grid = _np(phy.ofdm.ResourceGridMapper(rg)(x))
    assert np.array_equal(grid, o.rg_map(org, x))
    assert np.array_equal(_np(phy.ofdm.RemoveNulledSubcarriers(rg)(grid)), o.remove_nulled(org, grid))
    # [b, rx, streams_per_rx, T, fft] with identity association -> back to the data symbols
    back = _np(phy.ofdm.ResourceGridDemapper(rg, sm)(grid))
    assert np.array_equal(back, x)


@pytest.mark.parametrize("model", ["A", "C", "D"])
def test_tdl_matches_oracle_and_statistics(phy, model):
    phy.config.seed = 11
    tdl = phy.channel.tr38901.TDL(model, 300e-9, 2.6e9, min_speed=3., max_speed=30., num_rx_ant=4, num_tx_ant=2)
    fs = 1 / 71.4e-6
    a, tau = tdl(64, 14, fs)
    ref_a, ref_tau = o.tdl_cir(11, 0, 64, 14, fs, tdl.delays, tdl._mean_powers, tdl._min_doppler, tdl._max_doppler, 4, 2, 20,
                               los_power=tdl._los_power if tdl.los else None)
    assert a.shape == (64, 1, 4, 1, 2, tdl.num_clusters, 14) and tau.shape == (64, 1, 1, tdl.num_clusters)
    assert np.allclose(_np(a), ref_a, rtol=1e-3, atol=2e-4)          # f32 sincos of arguments up to ~1e2
    assert np.allclose(_np(tau), ref_tau)
    # power delay profile (test_3gpp_channel_tdl.py:156-263): mean tap powers, unit total power
    a2, _ = tdl(4096, 1, fs)
    p = np.mean(np.abs(_np(a2)) ** 2, axis=(0, 1, 2, 3, 4, 6))
    assert np.allclose(p, tdl.mean_powers, rtol=0.12, atol=2e-3)
    assert abs(p.sum() - 1) < 0.03


def test_cir_to_ofdm_large_links(phy):
    """Links whose taps do not fit in LDS beside the phase table (64 x 1 antennas, 23 clusters, 14 symbols = 165 KB; a
    32 x 4 link) and more than 64 paths run on the global-tap / LDS-phase variants of the same kernel instead of failing
    (round-2 advisor finding), with the same products in the same order."""
    rng = np.random.default_rng(11)
    fr = phy.channel.subcarrier_frequencies(48, 30e3)
    for (ra, ta, p_, t) in ((64, 1, 23, 14), (32, 4, 23, 14), (2, 2, 80, 3), (16, 2, 70, 14)):
        a = ((rng.normal(size=(2, 1, ra, 2, ta, p_, t)) + 1j * rng.normal(size=(2, 1, ra, 2, ta, p_, t))) / np.sqrt(2 * p_)).astype(np.complex64)
        tau = (rng.uniform(0, 2e-6, size=(2, 1, 2, p_))).astype(np.float32)
        for norm in (False, True):
            h = _np(phy.channel.cir_to_ofdm_channel(fr, a, tau, normalize=norm))
            ref = o.cir_to_ofdm_channel(fr, a, tau, normalize=norm)
            assert np.allclose(h, ref, rtol=2e-4, atol=5e-5), (ra, ta, p_, t, norm)
            # and on every output within the bound derived from the kernels' arithmetic (tests/channel_f32.py)
            assert chf.ratio(h, fr, a, tau, norm) <= 1.0, (ra, ta, p_, t, norm)
    # a link that fits is bit-identical whether its taps come from LDS or from global memory is not observable from
    # here; the small case of test_cir_to_ofdm_and_apply_channel pins the LDS variant against the same oracle


def test_cir_to_ofdm_and_apply_channel(phy):
    rg, org = _grids(phy)
    phy.config.seed = 5
    tdl = _tdl_params(phy)
    a, tau = tdl(8, 14, 1 / rg.ofdm_symbol_duration)
    fr = phy.channel.subcarrier_frequencies(76, 15e3)
    assert np.array_equal(fr, o.subcarrier_frequencies(76, 15e3))
    for norm in (False, True):
        h = _np(phy.channel.cir_to_ofdm_channel(fr, a, tau, normalize=norm))
        ref = o.cir_to_ofdm_channel(fr, _np(a), _np(tau), normalize=norm)
        assert np.allclose(h, ref, rtol=1e-4, atol=2e-5)
    assert abs(np.mean(np.abs(h) ** 2) - 1) < 1e-4                   # unit energy after normalisation
    rng = np.random.default_rng(1)
    x = (rng.normal(size=(8, 1, 2, 14, 76)) + 1j * rng.normal(size=(8, 1, 2, 14, 76))).astype(np.complex64)
    y = _np(phy.channel.ApplyOFDMChannel()(x, h))
    assert np.allclose(y, o.apply_ofdm_channel(x, h), rtol=1e-4, atol=1e-5)   # test_apply_channel.py:62-104 uses 1e-5


def test_ofdm_channel_block_and_rayleigh(phy):
    rg, _ = _grids(phy)
    phy.config.seed = 6
    ch = phy.channel.OFDMChannel(_tdl_params(phy), rg, normalize_channel=True, return_channel=True, add_awgn=True)
    x = torch.zeros((16, 1, 2, 14, 76), dtype=torch.complex64).cuda() + 1
    y, h = ch(x, 0.0)
    assert y.shape == (16, 1, 4, 14, 76) and h.shape == (16, 1, 4, 1, 2, 14, 76)
    assert np.allclose(_np(y), _np(h).sum(axis=(3, 4)), rtol=1e-4, atol=1e-5)
    ray = phy.channel.RayleighBlockFading(1, 4, 1, 2)
    a, tau = ray(20000, 3)
    assert a.shape == (20000, 1, 4, 1, 2, 1, 3) and float(tau.abs().max()) == 0
    an = _np(a)
    assert abs(np.mean(np.abs(an) ** 2) - 1) < 0.02 and np.array_equal(an[..., 0], an[..., 2])


@pytest.mark.parametrize("model", ["tdl", "rayleigh"])
@pytest.mark.parametrize("no", [None, 0.3])
def test_ofdm_channel_fused_launch_equals_the_separate_blocks(phy, model, no):
    """Round 6 (verdict next #5): OFDMChannel with one transmitter runs cir_to_ofdm_channel + ApplyOFDMChannel + AWGN as ONE
    launch (samd_ofdm_channel_fused_c64) and DEFERS the returned h_freq - the same bits as GenerateOFDMChannel ->
    ApplyOFDMChannel (-> AWGN) on the same random streams (reference channel/ofdm_channel.py:109-115, utils.py:237-251)."""
    from sionna_amd import _ffi
    from sionna_amd.phy.block import pending_of
    rg, _ = _grids(phy)
    rng = np.random.default_rng(5)
    x = torch.from_numpy((rng.normal(size=(37, 1, 2, 14, 76)) + 1j * rng.normal(size=(37, 1, 2, 14, 76))).astype(np.complex64)).cuda()

    def cm():
        return _tdl_params(phy) if model == "tdl" else phy.channel.RayleighBlockFading(1, 4, 1, 2)
    phy.config.seed = 31
    h_ref = phy.channel.GenerateOFDMChannel(cm(), rg, normalize_channel=True)(37)
    y_ref = phy.channel.ApplyOFDMChannel()(x, h_ref, no)
    phy.config.seed = 31
    y, h = phy.channel.OFDMChannel(cm(), rg, normalize_channel=True, return_channel=True)(x, no)
    assert pending_of(h) is not None, "h_freq was written although nobody read it"
    assert np.array_equal(_np(y), _np(y_ref))
    assert np.array_equal(_np(h), _np(h_ref)) and pending_of(h) is None          # filled on first use, the same channel
    phy.config.seed = 31
    y2 = phy.channel.OFDMChannel(cm(), rg, normalize_channel=True, return_channel=False)(x, no)
    assert np.array_equal(_np(y2), _np(y_ref))
    with _ffi.option("SAMD_NO_FUSED_CHANNEL"):                                   # the fall-back inside the block: same streams
        phy.config.seed = 31
        y3, h3 = phy.channel.OFDMChannel(cm(), rg, normalize_channel=True, return_channel=True)(x, no)
        assert np.array_equal(_np(y3), _np(y_ref)) and np.array_equal(_np(h3), _np(h_ref))
    if no is not None:                                                           # the noise is there and has the asked variance
        phy.config.seed = 31
        y0 = phy.channel.OFDMChannel(cm(), rg, normalize_channel=True)(x, None)
        d = _np(y) - _np(y0)
        assert abs(np.mean(np.abs(d) ** 2) / no - 1) < 0.02


def test_ls_estimator_matches_oracle(phy):
    rg, org = _grids(phy, num_tx=2, ns=1)
    rng = np.random.default_rng(2)
    y = (rng.normal(size=(6, 1, 4, 14, 76)) + 1j * rng.normal(size=(6, 1, 4, 14, 76))).astype(np.complex64)
    for interp in ("nn", None):
        h_hat, ev = phy.ofdm.LSChannelEstimator(rg, interpolation_type=interp)(y, 0.07)
        rh, rev = o.ls_estimate(org, y, 0.07, interp)
        assert h_hat.shape == rh.shape
        assert np.allclose(_np(h_hat), rh, rtol=1e-5, atol=1e-6)
        assert np.allclose(_np(ev), rev, rtol=1e-6) and np.broadcast_shapes(tuple(ev.shape), rh.shape) == rh.shape
    # per-batch noise variance
    no_b = rng.uniform(0.01, 1, size=(6,)).astype(np.float32)
    _, ev = phy.ofdm.LSChannelEstimator(rg)(y, no_b)
    assert ev.shape[0] == 6 and np.allclose(_np(ev)[3], o.ls_estimate(org, y, no_b[3])[1][0], rtol=1e-6)


@pytest.mark.parametrize("m,k", [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 2), (8, 4)])
@pytest.mark.parametrize("whiten", [True, False])
def test_lmmse_equalizer_vs_oracle(phy, m, k, whiten):
    rng = np.random.default_rng(m * 10 + k)
    n = 500
    h = (rng.normal(size=(n, m, k)) + 1j * rng.normal(size=(n, m, k))).astype(np.complex64) / np.sqrt(2)
    q = (rng.normal(size=(n, m, m)) + 1j * rng.normal(size=(n, m, m))).astype(np.complex64)
    s = (0.1 * q @ np.conj(np.swapaxes(q, -1, -2)) + 0.05 * np.eye(m)).astype(np.complex64)   # coloured noise
    x = omap.qam(4)[rng.integers(0, 16, (n, k))]
    y = ((h @ x[..., None])[..., 0] + 0.1 * (rng.normal(size=(n, m)) + 1j * rng.normal(size=(n, m)))).astype(np.complex64)
    xh, ne = phy.mimo.lmmse_equalizer(y, h, s, whiten)
    # float32 oracle with the defined operation order (oracle/mimo_f32.py): bit for bit
    fx, fn = of32.lmmse_equalizer(y, h, s, whiten)
    _same_f32(_np(xh), fx) and _same_f32(_np(ne), fn)
    # second witness: the complex128 restatement, at float32 conditioning (tests/test_oracle_mimo_f32.py has the bound)
    rx, rn = o.lmmse_equalizer(y, h, s, whiten)
    assert np.allclose(_np(xh), rx, rtol=3e-4, atol=3e-5)
    assert np.allclose(_np(ne), rn, rtol=3e-4)
    assert np.all(_np(ne) > 0)


@pytest.mark.parametrize("m,k", [(16, 4), (3, 2), (5, 5), (12, 1), (32, 8), (4, 2), (8, 4)])
@pytest.mark.parametrize("whiten", [True, False])
def test_lmmse_equalizer_any_shape(phy, m, k, whiten):
    """Shapes outside the unrolled list run the LDS-resident any-shape kernel (csrc/mimo.hip lmmse_items_any_kernel): the
    float32 spec's operation order, so bit-exact against oracle/mimo_f32.py and - for listed shapes, forced through it with
    SAMD_LMMSE_ANY - against the unrolled kernel.  Plus the reference-EXECUTED 16 x 4 outputs (phy_ref_golden.npz)."""
    from sionna_amd import _ffi
    rng = np.random.default_rng(m * 100 + k)
    n = 257
    h = (rng.normal(size=(n, m, k)) + 1j * rng.normal(size=(n, m, k))).astype(np.complex64) / np.sqrt(2)
    q = (rng.normal(size=(n, m, m)) + 1j * rng.normal(size=(n, m, m))).astype(np.complex64)
    s = (0.1 * q @ np.conj(np.swapaxes(q, -1, -2)) / m + 0.05 * np.eye(m)).astype(np.complex64)
    x = omap.qam(4)[rng.integers(0, 16, (n, k))]
    y = ((h @ x[..., None])[..., 0] + 0.1 * (rng.normal(size=(n, m)) + 1j * rng.normal(size=(n, m)))).astype(np.complex64)
    with _ffi.option("SAMD_LMMSE_ANY"):
        xh, ne = phy.mimo.lmmse_equalizer(y, h, s, whiten)
        xh, ne = _np(xh), _np(ne)
    fx, fn = of32.lmmse_equalizer(y, h, s, whiten)
    _same_f32(xh, fx) and _same_f32(ne, fn)
    if (m, k) in ((4, 2), (8, 4)):
        xu, nu = phy.mimo.lmmse_equalizer(y, h, s, whiten)
        assert np.array_equal(xh.view(np.float32), _np(xu).view(np.float32)) and np.array_equal(ne, _np(nu))
    rx, rn = o.lmmse_equalizer(y, h, s, whiten)
    assert np.allclose(xh, rx, rtol=1e-3, atol=1e-4) and np.allclose(ne, rn, rtol=1e-3)
    if (m, k) == (16, 4):
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "phy_ref_golden.npz"))
        for tag in ("col", "wht"):
            p_ = f"mimo16x4_{tag}_"
            gx, gn = phy.mimo.lmmse_equalizer(g[p_ + "y"], g[p_ + "h"], g[p_ + "s"], whiten)
            assert np.allclose(_np(gx), g[p_ + f"lmmse_w{int(whiten)}_x"], rtol=2e-3, atol=2e-4)
            assert np.allclose(_np(gn), g[p_ + f"lmmse_w{int(whiten)}_no"], rtol=2e-3, atol=1e-5)


def test_lmmse_error_statistics(phy):
    # test_mimo_equalizers.py:55-102: unbiased estimate, error variance == no_eff
    rng = np.random.default_rng(3)
    n, m, k = 200000, 8, 4
    h = ((rng.normal(size=(n, m, k)) + 1j * rng.normal(size=(n, m, k))) / np.sqrt(2)).astype(np.complex64)
    x = omap.qam(2)[rng.integers(0, 4, (n, k))]
    no = 0.3
    w = np.sqrt(no / 2) * (rng.normal(size=(n, m)) + 1j * rng.normal(size=(n, m)))
    y = ((h @ x[..., None])[..., 0] + w).astype(np.complex64)
    s = (no * np.eye(m)).astype(np.complex64)
    xh, ne = phy.mimo.lmmse_equalizer(y, h, np.broadcast_to(s, (n, m, m)).copy())
    err = _np(xh) - x
    assert abs(np.mean(err)) < 5e-3
    assert abs(np.mean(np.abs(err) ** 2) - np.mean(_np(ne))) / np.mean(_np(ne)) < 1e-2


@pytest.mark.parametrize("cfg", ["c4", "two_tx_interference", "two_rx"])
def test_fused_ofdm_lmmse_vs_oracle(phy, cfg):
    if cfg == "c4":
        (rg, org), assoc, ns, nra, nta = _grids(phy), [[1]], 2, 4, 2
    elif cfg == "two_tx_interference":      # one receiver detects tx 0, tx 1 is an interferer... both detected here
        (rg, org), assoc, ns, nra, nta = _grids(phy, num_tx=2, ns=1), [[1, 1]], 1, 4, 1
    else:                                   # two receivers, each detects its own transmitter, the other interferes
        (rg, org), assoc, ns, nra, nta = _grids(phy, num_tx=2, ns=2, fft=72, guards=(3, 4)), [[1, 0], [0, 1]], 2, 4, 2
    sm, osm = phy.mimo.StreamManagement(assoc, ns), o.StreamManagement(assoc, ns)
    nrx, ntx = len(assoc), len(assoc[0])
    rng = np.random.default_rng(4)
    B = 5
    x = omap.qam(2)[rng.integers(0, 4, (B, ntx, ns, rg.num_data_symbols))]
    grid = o.rg_map(org, x)
    h = ((rng.normal(size=(B, nrx, nra, ntx, nta, 14, rg.fft_size)) + 1j * rng.normal(size=(B, nrx, nra, ntx, nta, 14, rg.fft_size))) / np.sqrt(2)).astype(np.complex64)
    no = 0.05
    y = o.apply_ofdm_channel(grid, h)
    y = (y + np.sqrt(no / 2) * (rng.normal(size=y.shape) + 1j * rng.normal(size=y.shape))).astype(np.complex64)
    assert nta == ns
    h_perf = o.remove_nulled(org, h)                       # streams = tx antennas (no precoding)
    # perfect CSI, err_var = 0
    xh, ne = phy.ofdm.LMMSEEqualizer(rg, sm)(y, h_perf, 0., no)
    fxh, fne = of32.ofdm_equalize(org, osm, y, h_perf, np.zeros((1,) * 7, np.float32), no)
    _same_f32(_np(xh), fxh) and _same_f32(_np(ne), fne)                      # float32 order-defined oracle: bit for bit
    rxh, rne = o.ofdm_lmmse_equalize(org, osm, y, h_perf, np.zeros((1,) * 7, np.float32), no)
    assert np.allclose(_np(xh), rxh, rtol=3e-4, atol=3e-5) and np.allclose(_np(ne), rne, rtol=3e-4)   # complex128 witness
    # without undesired streams the covariance is diagonal and a leaner kernel runs; it performs the general
    # kernel's operations minus products with exact zeros
    from sionna_amd import _ffi
    with _ffi.option("SAMD_LMMSE_GENERAL"):
        xg, ng = phy.ofdm.LMMSEEqualizer(rg, sm)(y, h_perf, 0., no)
    assert np.array_equal(_np(xh), _np(xg)) and np.array_equal(_np(ne), _np(ng))
    # LS + nearest neighbour with its error variance table; per-batch noise
    no_b = rng.uniform(0.02, 0.1, size=(B,)).astype(np.float32)
    h_hat, ev = phy.ofdm.LSChannelEstimator(rg)(y, no_b)
    xh2, ne2 = phy.ofdm.LMMSEEqualizer(rg, sm, whiten_interference=False)(y, h_hat, ev, no_b)
    rh, rev = o.ls_estimate(org, y, 1.0)
    rev = rev * no_b.reshape(B, 1, 1, 1, 1, 1, 1)
    fxh2, fne2 = of32.ofdm_equalize(org, osm, y, _np(h_hat), _np(ev), no_b, "lmmse", whiten_interference=False)
    _same_f32(_np(xh2), fxh2) and _same_f32(_np(ne2), fne2)
    xh3, ne3 = phy.ofdm.LMMSEEqualizer(rg, sm)(y, h_hat, ev, no_b)          # whitened, with the error-variance table
    fxh3, fne3 = of32.ofdm_equalize(org, osm, y, _np(h_hat), _np(ev), no_b, "lmmse")
    _same_f32(_np(xh3), fxh3) and _same_f32(_np(ne3), fne3)
    rxh2, rne2 = o.ofdm_lmmse_equalize(org, osm, y, rh, rev, no_b, whiten_interference=False)
    assert np.allclose(_np(xh2), rxh2, rtol=3e-4, atol=3e-5) and np.allclose(_np(ne2), rne2, rtol=3e-4)
    # detector = equaliser + demapper
    det = phy.ofdm.LinearDetector("lmmse", "bit", "maxlog", rg, sm, "qam", 2)
    llr = det(y, h_perf, 0., no)
    assert llr.shape == (B, ntx, ns, rg.num_data_symbols * 2)
    for method in ("maxlog", "app"):                           # detector LLRs at the north-star bar (1e-5 relative)
        llr = phy.ofdm.LinearDetector("lmmse", "bit", method, rg, sm, "qam", 2)(y, h_perf, 0., no)
        ref_llr = omap.demapper(fxh.astype(np.complex128), fne.astype(np.float64), omap.qam(2).astype(np.complex128), method)
        assert _llr_close(_np(llr), ref_llr), np.max(np.abs(_np(llr) - ref_llr))


@pytest.mark.parametrize("cfg", ["c4_4x2", "siso", "two_tx_4x1", "cdl_8x4"])
def test_fused_ls_nn_lmmse_demap_is_bit_identical_to_the_separate_blocks(phy, cfg):
    """``LSChannelEstimator("nn")`` returns h_hat DEFERRED (block.py Pending); LMMSEEqualizer / LinearDetector then run
    samd_ofdm_lsnn_lmmse_c64 - estimate, equalise (and demap) in one launch, h_hat never written.  Same bits as the three
    separate launches (estimator with defer=False), for equaliser and LLR outputs, scalar and per-antenna noise variance;
    the deferred tensors still behave like tensors afterwards; everything the recipe does not cover takes the general path."""
    from sionna_amd.phy.block import pending_of
    nra, ns, num_tx, fft, guards = {"c4_4x2": (4, 2, 1, 76, (5, 6)), "siso": (1, 1, 1, 76, (5, 6)), "two_tx_4x1": (4, 1, 2, 76, (5, 6)),
                                    "cdl_8x4": (8, 4, 1, 72, (5, 6))}[cfg]
    rg, org = _grids(phy, num_tx=num_tx, ns=ns, fft=fft, guards=guards)
    sm = phy.mimo.StreamManagement([[1] * num_tx], ns)
    rng = np.random.default_rng(7)
    B = 37
    for m in (2, 4, 6):
        x = omap.qam(m)[rng.integers(0, 2 ** m, (B, num_tx, ns, rg.num_data_symbols))]
        grid = o.rg_map(org, x)
        h = ((rng.normal(size=(B, 1, nra, num_tx, ns, 14, rg.fft_size)) + 1j * rng.normal(size=(B, 1, nra, num_tx, ns, 14, rg.fft_size))) / np.sqrt(2)).astype(np.complex64)
        y = o.apply_ofdm_channel(grid, h)
        no_s = 0.03
        y = (y + np.sqrt(no_s / 2) * (rng.normal(size=y.shape) + 1j * rng.normal(size=y.shape))).astype(np.complex64)
        for no in (no_s, (no_s * (0.5 + rng.random((B, 1, nra)))).astype(np.float32), (no_s * (0.5 + rng.random(B))).astype(np.float32)):
            est_l, est_e = phy.ofdm.LSChannelEstimator(rg, "nn"), phy.ofdm.LSChannelEstimator(rg, "nn", defer=False)
            eq = phy.ofdm.LMMSEEqualizer(rg, sm)
            hh_e, ev_e = est_e(y, no)
            assert pending_of(hh_e) is None
            xe, ne = eq(y, hh_e, ev_e, no)
            hh_l, ev_l = est_l(y, no)
            assert pending_of(hh_l) is not None and tuple(hh_l.shape) == tuple(hh_e.shape) and hh_l.dtype == hh_e.dtype
            xl, nl = eq(y, hh_l, ev_l, no)
            assert pending_of(hh_l) is not None, "the fused launch must not fill h_hat"
            _same_f32(_np(xl), _np(xe)) and _same_f32(_np(nl), _np(ne))
            for meth in ("app", "maxlog"):
                for hard in (False, True):
                    det = phy.ofdm.LinearDetector("lmmse", "bit", meth, rg, sm, constellation_type="qam", num_bits_per_symbol=m, hard_out=hard)
                    ref = _np(det(y, hh_e, ev_e, no))
                    got = det(y, hh_l, ev_l, no)
                    assert pending_of(hh_l) is not None
                    _same_f32(_np(got), ref)
            # the deferred tensors are ordinary tensors for everybody else
            assert np.array_equal(_np(ev_l), _np(ev_e))
            assert np.array_equal(_np(hh_l + 0), _np(hh_e)) and pending_of(hh_l) is None
    # outside the recipe: a different err_var, ZF equaliser, another resource grid -> general path, still correct
    hh_l, ev_l = phy.ofdm.LSChannelEstimator(rg, "nn")(y, no_s)
    x0, n0 = phy.ofdm.LMMSEEqualizer(rg, sm)(y, hh_l, 0., no_s)
    assert pending_of(hh_l) is None
    xr, nr = phy.ofdm.LMMSEEqualizer(rg, sm)(y, hh_e if np.isscalar(no) else est_e(y, no_s)[0], 0., no_s)
    _same_f32(_np(x0), _np(xr)) and _same_f32(_np(n0), _np(nr))
    hh_l, ev_l = phy.ofdm.LSChannelEstimator(rg, "nn")(y, no_s)
    xz, _ = phy.ofdm.ZFEqualizer(rg, sm)(y, hh_l, ev_l, no_s)
    assert pending_of(hh_l) is None and np.isfinite(_np(xz)).all()


def test_c4_chain_high_snr_is_error_free(phy):
    """Config C4 end to end (TDL-A 300 ns, 4x2, LS-NN + LMMSE + LDPC) at 25 dB: BER == 0
    (the reference's own bar for this chain, test_mimo_ofdm_estimation_detection.py:183-195)."""
    rg, _ = _grids(phy)
    sm = phy.mimo.StreamManagement([[1]], 2)
    k, n, m = 768, 1536, 2
    assert rg.num_data_symbols * m == n
    enc = phy.fec.ldpc.LDPC5GEncoder(k, n)
    dec = phy.fec.ldpc.LDPC5GDecoder(enc, cn_update="minsum", num_iter=20)
    src, mapper, rgm = phy.mapping.BinarySource(), phy.mapping.Mapper("qam", m), phy.ofdm.ResourceGridMapper(rg)
    ch = phy.channel.OFDMChannel(_tdl_params(phy), rg, normalize_channel=True, return_channel=True)
    est, eq, demap = phy.ofdm.LSChannelEstimator(rg), phy.ofdm.LMMSEEqualizer(rg, sm), phy.mapping.Demapper("app", "qam", m)
    remove = phy.ofdm.RemoveNulledSubcarriers(rg)

    def mc_fun(batch_size, ebno_db, perfect_csi=False):
        no = phy.utils.ebnodb2no(ebno_db, m, k / n, rg)
        b = src([batch_size, 1, 2, k])
        x_rg = rgm(mapper(enc(b)))
        y, h = ch(x_rg, no)
        if perfect_csi:
            h_hat, ev = remove(h), 0.
        else:
            h_hat, ev = est(y, no)
        x_hat, no_eff = eq(y, h_hat, ev, no)
        return b, dec(demap(x_hat, no_eff))

    phy.config.seed = 8
    for perfect in (True, False):
        b, b_hat = mc_fun(64, 25.0, perfect)
        assert b_hat.shape == b.shape == (64, 1, 2, k)
        assert float((b != b_hat).float().mean()) == 0.0
    ber, bler = phy.utils.sim_ber(mc_fun, [-5.0, 25.0], batch_size=32, max_mc_iter=2, verbose=False)
    assert ber.numpy()[0] > 0.05 and ber.numpy()[1] == 0


@pytest.mark.parametrize("perfect_csi", [False, True])
def test_c4_chain_matches_oracle_on_same_noise(phy, perfect_csi):
    """BASELINE config 4 (OFDM 14 x 76, TDL-A 300 ns, 4x2 MIMO, LS-NN + LMMSE + QPSK demapper + 5G LDPC min-sum 20)
    on the GPU against the oracle chain on the SAME Philox streams (bits: call 0, TDL draws: calls 1-4, AWGN: call 5),
    like test_c1_chain_matches_oracle_on_same_noise does for C1.

    Two comparisons.  (1) end to end from the seed: every intermediate tensor at its stage tolerance (the TDL taps
    carry the float32 sincos error of arguments ~1e2, which everything downstream inherits) and identical bit
    decisions up to LLR near-ties.  (2) stage by stage on the GPU's own intermediate tensors, where nothing is
    inherited: LS estimate 1e-5, LMMSE bit for bit against the float32 order-defined oracle, LLRs at 1e-5 relative,
    min-sum decoder bit for bit."""
    from oracle.ldpc5g import LDPC5GCode
    from oracle import ldpc_bp as obp, cbind
    rg, org = _grids(phy)
    sm, osm = phy.mimo.StreamManagement([[1]], 2), o.StreamManagement([[1]], 2)
    k, n, m, B = 768, 1536, 2, 48
    enc = phy.fec.ldpc.LDPC5GEncoder(k, n)
    dec = phy.fec.ldpc.LDPC5GDecoder(enc, cn_update="minsum", num_iter=20)
    dec_soft = phy.fec.ldpc.LDPC5GDecoder(enc, cn_update="minsum", num_iter=20, hard_out=False)
    src, mapper, rgm = phy.mapping.BinarySource(), phy.mapping.Mapper("qam", m), phy.ofdm.ResourceGridMapper(rg)
    tdl = _tdl_params(phy)
    ch = phy.channel.OFDMChannel(tdl, rg, normalize_channel=True, return_channel=True)
    est, eq, demap = phy.ofdm.LSChannelEstimator(rg), phy.ofdm.LMMSEEqualizer(rg, sm), phy.mapping.Demapper("app", "qam", m)
    remove = phy.ofdm.RemoveNulledSubcarriers(rg)
    code = LDPC5GCode(k, n)
    odec = obp.LDPC5GDecoder(code, cn_update="minsum", num_iter=20, hard_out=False)
    pts = omap.qam(m)
    fr = o.subcarrier_frequencies(76, 15e3)
    total_bits = mism_bits = 0
    for seed, ebno in ((31, -4.0), (32, -1.0), (33, 2.0)):
        phy.config.seed = seed
        no = phy.utils.ebnodb2no(ebno, m, k / n, rg)
        assert np.isclose(float(no), float(outil.ebnodb2no(ebno, m, k / n, org)), rtol=1e-6)
        b = src([B, 1, 2, k])
        x_rg = rgm(mapper(enc(b)))
        y, h = ch(x_rg, no)
        h_hat, ev = (remove(h), 0.) if perfect_csi else est(y, no)
        x_hat, no_eff = eq(y, h_hat, ev, no)
        llr = demap(x_hat, no_eff)
        b_hat, soft = dec(llr), dec_soft(llr)

        # ---- (1) oracle chain from the seed
        bo = outil.random_bits(seed, 0, B * 2 * k).reshape(B, 1, 2, k)
        assert np.array_equal(_np(b), bo)
        xo = o.rg_map(org, omap.mapper(code.encode(bo.reshape(-1, k)).reshape(B, 1, 2, n), pts))
        assert np.array_equal(_np(x_rg), xo)
        ao, tauo = o.tdl_cir(seed, 1, B, 14, 1 / org.ofdm_symbol_duration, tdl.delays, tdl._mean_powers, tdl._min_doppler,
                             tdl._max_doppler, 4, 2, 20)
        ho = o.cir_to_ofdm_channel(fr, ao, tauo, normalize=True)
        assert np.allclose(_np(h), ho, rtol=1e-3, atol=1e-3)
        no_o = outil.ebnodb2no(ebno, m, k / n, org)
        yo = outil.awgn(o.apply_ofdm_channel(xo, ho), no_o, seed, 5)
        assert np.allclose(_np(y), yo, rtol=1e-3, atol=2e-3)
        if perfect_csi:
            hho, evo = o.remove_nulled(org, ho), np.zeros((1,) * 7, np.float32)
        else:
            hho, evo = o.ls_estimate(org, yo, no_o)
        xho, neo = of32.ofdm_equalize(org, osm, yo, hho, evo, no_o)
        llro = omap.demapper(xho, neo, pts, "app")
        ref_soft = cbind.bp_decode(odec, odec.rate_recover(llro.reshape(B * 2, n)))[:, :k].reshape(B, 1, 2, k)
        ref = (ref_soft > 0).astype(np.float32)
        got = _np(b_hat)
        # identical decisions; only a word that min-sum fails to decode may amplify the inherited 1e-3 input
        # difference (20 iterations of a non-converging decoder are chaotic), so codewords are compared by status
        ok_ref, ok_got = np.all(ref == bo, axis=-1), np.all(got == bo, axis=-1)
        differ = got != ref
        total_bits += differ.size
        mism_bits += int(differ.sum())
        assert np.mean(ok_ref != ok_got) <= 0.03, f"seed {seed}: block status differs on {np.mean(ok_ref != ok_got)}"
        assert not differ[ok_ref & ok_got].any()
        assert abs(np.mean(got != bo) - np.mean(ref != bo)) < 1e-2, (np.mean(got != bo), np.mean(ref != bo))

        # ---- (2) stage by stage on the GPU's own tensors
        yg, hg = _np(y), _np(h)
        if perfect_csi:
            hh_g, ev_g = o.remove_nulled(org, hg), np.zeros((1,) * 7, np.float32)
            assert np.array_equal(_np(h_hat), hh_g)
        else:
            hh_ref, ev_ref = o.ls_estimate(org, yg, float(no))
            assert np.allclose(_np(h_hat), hh_ref, rtol=1e-5, atol=1e-6) and np.allclose(_np(ev), ev_ref, rtol=1e-6)
            hh_g, ev_g = _np(h_hat), _np(ev)
        fx, fne = of32.ofdm_equalize(org, osm, yg, hh_g, ev_g, np.float32(float(no)))
        _same_f32(_np(x_hat), fx) and _same_f32(_np(no_eff), fne)
        llr_ref = omap.demapper(fx.astype(np.complex128), fne.astype(np.float64), pts.astype(np.complex128), "app")
        assert _llr_close(_np(llr), llr_ref), np.max(np.abs(_np(llr) - llr_ref))
        soft_ref = cbind.bp_decode(odec, odec.rate_recover(_np(llr).reshape(B * 2, n)))[:, :k].reshape(B, 1, 2, k)
        _same_f32(_np(soft), soft_ref)
        assert np.array_equal(got, (soft_ref > 0).astype(np.float32))
    # (measured on MI355X: 2.4 % of all bits differ with LS estimation, all of them inside words neither side decodes at
    # -4 / -1 dB; 0 with perfect CSI at 2 dB)
    assert mism_bits <= 5e-2 * total_bits, mism_bits / total_bits


def test_c4_full_batch_properties(phy):
    """Config C4 at BASELINE.json's full batch (8192): size-independent properties - BER falls with the SNR,
    perfect CSI is never worse than LS estimation, noiseless transmission is error free."""
    rg, _ = _grids(phy)
    sm = phy.mimo.StreamManagement([[1]], 2)
    k, n, m, B = 768, 1536, 2, 8192
    enc = phy.fec.ldpc.LDPC5GEncoder(k, n)
    dec = phy.fec.ldpc.LDPC5GDecoder(enc, cn_update="minsum", num_iter=20)
    src, mapper, rgm = phy.mapping.BinarySource(), phy.mapping.Mapper("qam", m), phy.ofdm.ResourceGridMapper(rg)
    ch = phy.channel.OFDMChannel(_tdl_params(phy), rg, normalize_channel=True, return_channel=True)
    est, eq, demap = phy.ofdm.LSChannelEstimator(rg), phy.ofdm.LMMSEEqualizer(rg, sm), phy.mapping.Demapper("app", "qam", m)
    remove = phy.ofdm.RemoveNulledSubcarriers(rg)
    phy.config.seed = 21

    def ber(ebno_db, perfect):
        no = phy.utils.ebnodb2no(ebno_db, m, k / n, rg)
        b = src([B, 1, 2, k])
        y, h = ch(rgm(mapper(enc(b))), no)
        h_hat, ev = (remove(h), 0.) if perfect else est(y, no)
        x_hat, no_eff = eq(y, h_hat, ev, no)
        return float((b != dec(demap(x_hat, no_eff))).float().mean())

    ls = [ber(e, False) for e in (-6.0, -3.0, 0.0)]
    pc = [ber(e, True) for e in (-6.0, -3.0, 0.0)]
    assert ls[0] > ls[1] > ls[2] and pc[0] > pc[1] > pc[2]
    assert all(p <= l for p, l in zip(pc, ls))
    assert ber(40.0, True) == 0.0 and ber(40.0, False) == 0.0


# ------------------------------------------------------------------ time-domain variant (rocFFT)
def _cplx(rng, shape):
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)


@pytest.mark.parametrize("cp", [0, 1, 6, 12, 72])
def test_ofdm_modulator_demodulator_vs_oracle(phy, cp):
    rng = np.random.default_rng(cp)
    x = _cplx(rng, (16, 2, 14, 72))
    xt = _np(phy.ofdm.OFDMModulator(cp)(x))
    ref = o.ofdm_modulate(x, cp)
    assert xt.shape == ref.shape
    assert np.allclose(xt, ref, rtol=1e-4, atol=2e-5)
    sym = xt.reshape(16, 2, 14, -1)
    if cp:   # reference test_cyclic_prefixes: prefix is a bit copy of the tail
        assert np.array_equal(sym[..., :cp], sym[..., -cp:])
    for l_min in (0, -3):
        xh = _np(phy.ofdm.OFDMDemodulator(72, l_min, cp)(ref))
        assert np.allclose(xh, o.ofdm_demodulate(ref, 72, l_min, cp), rtol=1e-4, atol=2e-5)
    # round trip + trailing samples ignored (reference test_overlapping_input)
    x_time = np.concatenate([xt, xt[..., :10]], axis=-1)
    assert np.max(np.abs(_np(phy.ofdm.OFDMDemodulator(72, 0, cp)(x_time)) - x)) < 1e-5 * 4


def test_ofdm_modulator_variable_cp_and_errors(phy):
    rng = np.random.default_rng(5)
    cps = np.arange(72)
    x = _cplx(rng, (3, 72, 72))
    xt = _np(phy.ofdm.OFDMModulator(cps)(x))
    assert np.allclose(xt, o.ofdm_modulate(x, cps), rtol=1e-4, atol=2e-5)
    xh = _np(phy.ofdm.OFDMDemodulator(72, 0, cps)(xt))
    assert np.max(np.abs(xh - x)) < 4e-5
    with pytest.raises(ValueError):
        phy.ofdm.OFDMModulator(73)(x)
    with pytest.raises(ValueError):
        phy.ofdm.OFDMModulator(-1)
    # other transform sizes (power of two, odd, large)
    for n in (64, 75, 1024, 4096):
        x = _cplx(rng, (2, 3, n))
        xt = _np(phy.ofdm.OFDMModulator(7)(x))
        assert np.allclose(xt, o.ofdm_modulate(x, 7), rtol=1e-4, atol=1e-4)
        assert np.max(np.abs(_np(phy.ofdm.OFDMDemodulator(n, 0, 7)(xt)) - x)) < 1e-4


@pytest.mark.parametrize("tn,l_tot", [(1, 1), (5, 3), (32, 8), (128, 16), (300, 27)])
def test_apply_time_channel_vs_oracle(phy, tn, l_tot):
    rng = np.random.default_rng(tn)
    B, rx, ra, tx, ta = 5, 2, 4, 2, 2
    x = _cplx(rng, (B, tx, ta, tn))
    h = _cplx(rng, (B, rx, ra, tx, ta, tn + l_tot - 1, l_tot))
    y = _np(phy.channel.ApplyTimeChannel(tn, l_tot)(x, h))
    assert y.shape == (B, rx, ra, tn + l_tot - 1)
    assert np.allclose(y, o.apply_time_channel(x, h), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("normalize", [False, True])
def test_cir_to_time_channel_vs_oracle(phy, normalize):
    tdl = phy.channel.tr38901.TDL("C", 300e-9, 3.5e9, min_speed=3., max_speed=30., num_rx_ant=2, num_tx_ant=2)
    bw = 76 * 30e3
    l_min, l_max = phy.channel.time_lag_discrete_time_channel(bw)
    assert (l_min, l_max) == o.time_lag_discrete_time_channel(bw)
    a, tau = tdl(6, 200, bw)
    h = _np(phy.channel.cir_to_time_channel(bw, a, tau, l_min, l_max, normalize))
    ref = o.cir_to_time_channel(bw, _np(a), _np(tau), l_min, l_max, normalize)
    assert h.shape == ref.shape == (6, 1, 2, 1, 2, 200, l_max - l_min + 1)
    assert np.allclose(h, ref, rtol=1e-4, atol=2e-5)
    if normalize:
        e = np.mean(np.sum(np.abs(h) ** 2, axis=6), axis=(2, 4, 5))
        assert np.allclose(e, 1.0, atol=1e-4)


@pytest.mark.parametrize("tag", ["cp2", "cp20", "c4", "small"])
def test_time_domain_kernels_match_reference_execution(phy, tag):
    """The HIP kernels against outputs of the reference's OWN modulator / cir_to_time_channel / ApplyTimeChannel /
    demodulator / cir_to_ofdm_channel code (tests/golden/ofdm_time_ref_golden.npz, tools/gen_ofdm_time_ref_golden.py),
    including the fft 72, l_min -6 ... l_max 10, cyclic prefix 2 configuration (the ISI regime)."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ofdm_time_ref_golden.npz"))
    fft, nsym, cp, l_min, l_max, B, nrx, nra, ntx, nta, P = (int(v) for v in g[f"{tag}_meta"])
    bw = fft * float(g[f"{tag}_scs"])
    assert phy.channel.time_lag_discrete_time_channel(bw) == (l_min, l_max)
    close = lambda a, b, tol=1e-5: np.abs(a - b).max() <= 4 * tol * np.abs(b).max()
    x, a, tau = g[f"{tag}_x"], g[f"{tag}_a"], g[f"{tag}_tau"]
    xt = phy.ofdm.OFDMModulator(cp)(x)
    assert close(_np(xt), g[f"{tag}_x_time"])
    for norm in (True, False):
        h = phy.channel.cir_to_time_channel(bw, a, tau, l_min, l_max, normalize=norm)
        assert close(_np(h), g[f"{tag}_h_time_n{int(norm)}"]), norm
    N = nsym * (fft + cp)
    y = phy.channel.ApplyTimeChannel(N, l_max - l_min + 1)(g[f"{tag}_x_time"].reshape(B, ntx, nta, -1), g[f"{tag}_h_time_n1"])
    assert close(_np(y), g[f"{tag}_y_time"])
    assert close(_np(phy.ofdm.OFDMDemodulator(fft, l_min, cp)(g[f"{tag}_y_time"])), g[f"{tag}_y_rg"])
    f = phy.channel.subcarrier_frequencies(fft, float(g[f"{tag}_scs"]))
    assert np.array_equal(np.asarray(f.cpu() if hasattr(f, "cpu") else f, np.float32), g[f"{tag}_freqs"])
    a_f = np.ascontiguousarray(a[..., cp:-1:(fft + cp)][..., :nsym])
    for norm in (True, False):
        hf = phy.channel.cir_to_ofdm_channel(f, a_f, tau, normalize=norm)
        assert close(_np(hf), g[f"{tag}_h_freq_n{int(norm)}"], 2e-5), norm


def test_time_domain_chain_matches_frequency_response(phy):
    """Reference test_channel_utils.py:83-135 restated: mod -> TimeChannel (static TDL-A) -> demod
    equals H[k] x[k] with H the DFT of the taps, for taps inside the cyclic prefix."""
    cp, n, nsym, B = 10, 128, 5, 8
    rg = phy.ofdm.ResourceGrid(nsym, n, 15e3, cyclic_prefix_length=cp)
    l_min, l_max = -4, 6
    tdl = phy.channel.tr38901.TDL("A", 100e-9, 3.5e9, min_speed=0., max_speed=0.)
    ch = phy.channel.TimeChannel(tdl, rg.bandwidth, rg.num_time_samples, l_min=l_min, l_max=l_max,
                                 normalize_channel=True, return_channel=True)
    rng = np.random.default_rng(2)
    x = _cplx(rng, (B, 1, 1, nsym, n))
    xt = phy.ofdm.OFDMModulator(cp)(x)
    y, h_time = ch(xt)
    yf = _np(phy.ofdm.OFDMDemodulator(n, l_min, cp)(y))
    taps = _np(h_time)[:, 0, 0, 0, 0, 0, :].astype(np.complex128)
    k = np.arange(n) - n // 2
    H = (taps[:, None, :] * np.exp(-2j * np.pi * k[None, :, None] * np.arange(l_min, l_max + 1)[None, None, :] / n)).sum(-1)
    assert np.allclose(yf[:, 0, 0], H[:, None, :] * x[:, 0, 0], atol=1e-4)
    # and the whole chain against the oracle on the same taps
    ref = o.ofdm_demodulate(o.apply_time_channel(o.ofdm_modulate(x, cp), _np(h_time)), n, l_min, cp)
    assert np.allclose(yf, ref, rtol=1e-4, atol=1e-4)


def test_time_channel_deferred_normalisation_is_identical(phy):
    """Without return_channel the normalisation factor of h_time is applied while the channel is applied (no second
    pass over h_time): the received signal equals the one of the two-pass path bit for bit."""
    rg = phy.ofdm.ResourceGrid(3, 64, 30e3, cyclic_prefix_length=8)
    mk = lambda ret: phy.channel.TimeChannel(
        phy.channel.tr38901.TDL("C", 300e-9, 3.5e9, min_speed=3., max_speed=30., num_rx_ant=2, num_tx_ant=2),
        rg.bandwidth, rg.num_time_samples, normalize_channel=True, return_channel=ret)
    x = _cplx(np.random.default_rng(5), (7, 1, 2, rg.num_time_samples))
    phy.config.seed = 21
    y1 = _np(mk(False)(x))
    phy.config.seed = 21
    y2, h = mk(True)(x)
    assert np.array_equal(y1, _np(y2))
    e = np.mean(np.sum(np.abs(_np(h)) ** 2, axis=6), axis=(2, 4, 5))
    assert np.allclose(e, 1.0, atol=1e-4)


# ------------------------------------------------------------------ linear interpolation ("lin", "lin_time_avg")
from test_oracle_ofdm_time import LIN_PATTERNS


@pytest.mark.parametrize("name", sorted(LIN_PATTERNS))
@pytest.mark.parametrize("time_avg", [False, True])
def test_linear_interpolator_vs_oracle(phy, name, time_avg):
    opp = LIN_PATTERNS[name]()
    pp = phy.ofdm.PilotPattern(opp.mask, opp.pilots)
    rng = np.random.default_rng(len(name))
    ntx, ns, T, F = opp.mask.shape
    h_p = _cplx(rng, (3, 2, ntx, ns, opp.pilots.shape[-1])) * (np.abs(opp.pilots) > 0)
    ev_p = rng.uniform(0.1, 1.0, h_p.shape).astype(np.float32) * (np.abs(opp.pilots) > 0)
    h, ev = phy.ofdm.LinearInterpolator(pp, time_avg)(h_p, ev_p)
    h_ref, ev_ref = o.LinearInterpolator(opp, time_avg)(h_p, ev_p)
    assert tuple(h.shape) == h_ref.shape == (3, 2, ntx, ns, T, F)
    assert np.allclose(_np(h), h_ref, rtol=1e-4, atol=1e-5) and np.allclose(_np(ev), ev_ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("itype", ["lin", "lin_time_avg"])
def test_ls_estimator_linear_vs_oracle(phy, itype):
    rg, org = _grids(phy, num_tx=2, ns=2, fft=72, guards=(3, 4))
    rng = np.random.default_rng(7)
    y = _cplx(rng, (6, 1, 4, 14, 72))
    h, ev = phy.ofdm.LSChannelEstimator(rg, interpolation_type=itype)(y, 0.05)
    h_ref, ev_ref = o.ls_estimate_lin(org, y, 0.05, time_avg=itype == "lin_time_avg")
    assert np.allclose(_np(h), h_ref, rtol=1e-4, atol=1e-5)
    assert np.allclose(np.broadcast_to(_np(ev), h_ref.shape), np.broadcast_to(ev_ref, h_ref.shape), rtol=1e-4, atol=1e-6)
    # an explicit interpolator object is accepted like in the reference
    h2, _ = phy.ofdm.LSChannelEstimator(rg, interpolator=phy.ofdm.LinearInterpolator(rg.pilot_pattern, itype == "lin_time_avg"))(y, 0.05)
    assert np.array_equal(_np(h2), _np(h))


def test_ls_estimator_custom_interpolator(phy):
    """``interpolator=`` any object with BaseChannelInterpolator's call interface (channel_estimation.py:160-167, 287-321):
    it receives the LS estimates / error variances at the pilots and returns them for the whole grid."""
    rg, org = _grids(phy, num_tx=2, ns=2, fft=72, guards=(3, 4))
    y = _cplx(np.random.default_rng(9), (4, 1, 4, 14, 72))
    lin = phy.ofdm.LinearInterpolator(rg.pilot_pattern)
    seen = {}

    class Mine:                                                        # delegates, through NumPy on the way out
        def __call__(self, h_hat, err_var):
            seen["shapes"] = (tuple(h_hat.shape), tuple(err_var.shape))
            h, ev = lin(h_hat, err_var)
            return _np(h), _np(ev)

    h, ev = phy.ofdm.LSChannelEstimator(rg, interpolator=Mine())(y, 0.05)
    h_ref, ev_ref = phy.ofdm.LSChannelEstimator(rg, interpolation_type="lin")(y, 0.05)
    npil = rg.pilot_pattern.num_pilot_symbols
    assert seen["shapes"] == ((4, 1, 4, 2, 2, npil),) * 2
    assert np.array_equal(_np(h), _np(h_ref)) and np.array_equal(_np(ev), np.broadcast_to(_np(ev_ref), ev.shape))
    assert float(_np(ev).min()) >= 0.0


def test_time_domain_chain_ls_lin_recovers_frequency_response(phy):
    """Reference test_channel_utils.py:83-135: static TDL channel through modulator -> ApplyTimeChannel ->
    demodulator; the noise-free LS estimate with linear interpolation equals the DFT of the taps."""
    cp, n, nsym, B = 10, 128, 5, 8
    l_min, l_max = -3, 5
    rg = phy.ofdm.ResourceGrid(nsym, n, 15e3, pilot_pattern="kronecker", pilot_ofdm_symbol_indices=[0, 2, 4],
                               cyclic_prefix_length=cp)
    l_tot = l_max - l_min + 1
    tdl = phy.channel.tr38901.TDL("A", 100e-9, 3.5e9, min_speed=0., max_speed=0.)
    a, tau = tdl(B, rg.num_time_samples + l_tot - 1, rg.bandwidth)
    h_time = phy.channel.cir_to_time_channel(rg.bandwidth, a, tau, l_min, l_max, normalize=True)
    rng = np.random.default_rng(4)
    x = (np.sign(rng.normal(size=(B, 1, 1, rg.num_data_symbols))) + 1j * np.sign(rng.normal(size=(B, 1, 1, rg.num_data_symbols)))).astype(np.complex64) / np.sqrt(2)
    x_time = phy.ofdm.OFDMModulator(cp)(phy.ofdm.ResourceGridMapper(rg)(x))
    y_time = phy.channel.ApplyTimeChannel(rg.num_time_samples, l_tot)(x_time, h_time)
    y_freq = phy.ofdm.OFDMDemodulator(n, l_min, cp)(y_time)
    h_hat, _ = phy.ofdm.LSChannelEstimator(rg, interpolation_type="lin")(y_freq, 1e-4)
    taps = _np(h_time)[:, 0, 0, 0, 0, 0, :].astype(np.complex128)
    k = np.arange(n) - n // 2
    H = (taps[:, None, :] * np.exp(-2j * np.pi * k[None, :, None] * np.arange(l_min, l_max + 1)[None, None, :] / n)).sum(-1)
    assert np.allclose(_np(h_hat)[:, 0, 0, 0, 0], np.broadcast_to(H[:, None, :], (B, nsym, n)), atol=1e-4)


# ------------------------------------------------------------------ MMSE-PIC detector
@pytest.mark.parametrize("m,k,nb", [(4, 2, 2), (4, 2, 4), (2, 2, 2), (8, 4, 4), (4, 1, 6), (1, 1, 2)])
@pytest.mark.parametrize("method", ["app", "maxlog"])
def test_mimo_mmse_pic_vs_oracle(phy, m, k, nb, method):
    rng = np.random.default_rng(m * 10 + k + nb)
    n = 300
    pts = omap.qam(nb)
    bits = rng.integers(0, 2, (n, k, nb))
    x = pts[(bits * (2 ** np.arange(nb - 1, -1, -1))).sum(-1)]
    h = _cplx(rng, (n, m, k)) / np.sqrt(2)
    no = 0.15
    y = ((h @ x[..., None])[..., 0] + np.sqrt(no / 2) * _cplx(rng, (n, m))).astype(np.complex64)
    a = _cplx(rng, (n, m, m)) * 0.2
    s = (a @ np.conj(np.swapaxes(a, -1, -2)) + no * np.eye(m)).astype(np.complex64)          # coloured noise covariance
    prior = (rng.normal(size=(n, k, nb)) * 2).astype(np.float32)
    for num_iter in (1, 3):
        det = phy.mimo.MMSEPICDetector("bit", method, num_iter=num_iter, constellation_type="qam", num_bits_per_symbol=nb)
        got = _np(det(y, h, s, prior))
        ref = o.mmse_pic(y, h, s, prior, pts, method, num_iter)
        assert got.shape == ref.shape == (n, k, nb)
        assert np.mean(np.isclose(got, ref, rtol=2e-3, atol=2e-3)) > 0.995, np.max(np.abs(got - ref))
    # zero prior, one iteration == LMMSE equaliser + demapper (x_hat = 0, unit variance: [CST2011] reduces to LMMSE)
    det = phy.mimo.MMSEPICDetector("bit", method, num_iter=1, constellation_type="qam", num_bits_per_symbol=nb)
    got = _np(det(y, h, s, np.zeros_like(prior)))
    lin = _np(phy.mimo.LinearDetector("lmmse", "bit", method, constellation_type="qam", num_bits_per_symbol=nb)(y, h, s))
    assert np.mean(np.isclose(got, lin, rtol=2e-3, atol=2e-3)) > 0.995
    hard = _np(phy.mimo.MMSEPICDetector("bit", method, num_iter=2, constellation_type="qam", num_bits_per_symbol=nb,
                                        hard_out=True)(y, h, s, prior))
    assert set(np.unique(hard)) <= {0.0, 1.0}
    # output="symbol" (logits on the points as priors and as result): tests/test_gpu_symbol.py
    assert phy.mimo.MMSEPICDetector("symbol", method, constellation_type="qam", num_bits_per_symbol=nb)._output == "symbol"


@pytest.mark.parametrize("num_tx,ns,assoc", [(1, 2, [[1]]), (2, 1, [[1, 1]]), (2, 2, [[1, 0], [0, 1]])])
def test_ofdm_mmse_pic_vs_oracle(phy, num_tx, ns, assoc):
    rg, org = _grids(phy, num_tx=num_tx, ns=ns, fft=72, guards=(3, 4))
    sm, osm = phy.mimo.StreamManagement(np.array(assoc), ns), o.StreamManagement(np.array(assoc), ns)
    rng = np.random.default_rng(num_tx + ns)
    B, nb = 3, 2
    pts = omap.qam(nb)
    nrx = len(assoc)
    y = _cplx(rng, (B, nrx, 4, 14, 72))
    h_hat = _cplx(rng, (B, nrx, 4, num_tx, ns, 14, rg.num_effective_subcarriers))
    err_var = rng.uniform(0.0, 0.05, (1, 1, 1, num_tx, ns, 14, rg.num_effective_subcarriers)).astype(np.float32)
    prior = (rng.normal(size=(B, num_tx, ns, rg.num_data_symbols * nb)) * 1.5).astype(np.float32)
    for method, it in (("maxlog", 1), ("app", 2)):
        det = phy.ofdm.MMSEPICDetector("bit", method, rg, sm, num_iter=it, constellation_type="qam", num_bits_per_symbol=nb)
        got = _np(det(y, h_hat, prior, err_var, 0.3))
        ref = o.ofdm_mmse_pic(org, osm, y, h_hat, prior, err_var, 0.3, pts, method, it)
        assert got.shape == ref.shape
        assert np.mean(np.isclose(got, ref, rtol=2e-3, atol=2e-3)) > 0.995, np.max(np.abs(got - ref))
    # zero prior + one iteration == the linear LMMSE detector of the same grid
    det = phy.ofdm.MMSEPICDetector("bit", "app", rg, sm, num_iter=1, constellation_type="qam", num_bits_per_symbol=nb)
    lin = phy.ofdm.LinearDetector("lmmse", "bit", "app", rg, sm, constellation_type="qam", num_bits_per_symbol=nb)
    a, b = _np(det(y, h_hat, np.zeros_like(prior), err_var, 0.3)), _np(lin(y, h_hat, err_var, 0.3))
    assert np.mean(np.isclose(a, b, rtol=2e-3, atol=2e-3)) > 0.995


# ------------------------------------------------------------------ EP detector
@pytest.mark.parametrize("m,k,nb", [(4, 4, 4), (4, 2, 2), (8, 4, 6), (2, 2, 4), (1, 1, 2)])
def test_mimo_ep_detector_vs_oracle(phy, m, k, nb):
    rng = np.random.default_rng(m + k + nb)
    n = 400
    pts = omap.qam(nb)
    bits = rng.integers(0, 2, (n, k, nb))
    x = pts[(bits * (2 ** np.arange(nb - 1, -1, -1))).sum(-1)]
    h = _cplx(rng, (n, m, k)) / np.sqrt(2)
    no = 0.05
    y = ((h @ x[..., None])[..., 0] + np.sqrt(no / 2) * _cplx(rng, (n, m))).astype(np.complex64)
    a = _cplx(rng, (n, m, m)) * 0.1
    s = (a @ np.conj(np.swapaxes(a, -1, -2)) + no * np.eye(m)).astype(np.complex64)
    for l, beta in ((1, 0.9), (10, 0.9), (5, 0.5)):
        got = _np(phy.mimo.EPDetector("bit", nb, l=l, beta=beta)(y, h, s))
        ref = o.ep_detector(y, h, s, nb, l=l, beta=beta)
        assert got.shape == ref.shape == (n, k, nb)
        # EP iterates a fixed-point map with 1e-6 floors: compare on the scale of the LLRs
        tol = 2e-2 * (1 + np.abs(ref))
        assert np.mean(np.abs(got - ref) <= tol) > 0.99, np.max(np.abs(got - ref))
        assert np.mean((got > 0) == (ref > 0)) > 0.998
    hard = _np(phy.mimo.EPDetector("bit", nb, hard_out=True)(y, h, s))
    assert set(np.unique(hard)) <= {0.0, 1.0}
    if m == k == 4:            # EP beats the linear detector on a square 16-QAM system
        lin = _np(phy.mimo.LinearDetector("lmmse", "bit", "maxlog", constellation_type="qam", num_bits_per_symbol=nb)(y, h, s))
        got = _np(phy.mimo.EPDetector("bit", nb)(y, h, s))
        assert np.mean((got > 0) != bits) < 0.7 * np.mean((lin > 0) != bits)
    assert phy.mimo.EPDetector("symbol", nb)._output == "symbol"          # its outputs: tests/test_gpu_symbol.py


def test_ofdm_ep_detector_vs_oracle(phy):
    rg, org = _grids(phy, num_tx=2, ns=2, fft=72, guards=(3, 4))
    assoc = [[1, 0], [0, 1]]
    sm, osm = phy.mimo.StreamManagement(np.array(assoc), 2), o.StreamManagement(np.array(assoc), 2)
    rng = np.random.default_rng(3)
    B, nb = 3, 4
    y = _cplx(rng, (B, 2, 4, 14, 72))
    h_hat = _cplx(rng, (B, 2, 4, 2, 2, 14, rg.num_effective_subcarriers))
    err_var = rng.uniform(0.0, 0.05, (1, 1, 1, 2, 2, 14, rg.num_effective_subcarriers)).astype(np.float32)
    got = _np(phy.ofdm.EPDetector("bit", rg, sm, nb, l=6)(y, h_hat, err_var, 0.3))
    ref = o.ofdm_ep_detector(org, osm, y, h_hat, err_var, 0.3, nb, l=6)
    assert got.shape == ref.shape
    assert np.mean(np.abs(got - ref) <= 2e-2 * (1 + np.abs(ref))) > 0.99, np.max(np.abs(got - ref))


# ------------------------------------------------------------------ K-Best detector
@pytest.mark.parametrize("m,k,nb,paths", [(2, 2, 2, 16), (4, 4, 2, 8), (4, 2, 4, 16), (8, 4, 4, 32), (4, 4, 4, 64), (1, 1, 6, 5)])
def test_mimo_kbest_vs_oracle(phy, m, k, nb, paths):
    rng = np.random.default_rng(m + k + nb + paths)
    n = 300
    pts = omap.qam(nb)
    bits = rng.integers(0, 2, (n, k, nb))
    x = pts[(bits * (2 ** np.arange(nb - 1, -1, -1))).sum(-1)]
    h = _cplx(rng, (n, m, k)) / np.sqrt(2)
    no = 0.1
    y = ((h @ x[..., None])[..., 0] + np.sqrt(no / 2) * _cplx(rng, (n, m))).astype(np.complex64)
    a = _cplx(rng, (n, m, m)) * 0.1
    s = (a @ np.conj(np.swapaxes(a, -1, -2)) + no * np.eye(m)).astype(np.complex64)
    det = phy.mimo.KBestDetector("bit", k, paths, constellation_type="qam", num_bits_per_symbol=nb)
    got = _np(det(y, h, s))
    ref = o.kbest_detector(y, h, s, pts, paths)
    assert got.shape == ref.shape == (n, k, nb)
    # identical surviving lists except for float32 near-ties in the partial distances
    ok = np.all(np.isclose(got, ref, rtol=1e-3, atol=2e-3), axis=(1, 2))
    assert ok.mean() > 0.97, (1 - ok.mean(), np.max(np.abs(got - ref)))
    hard = _np(phy.mimo.KBestDetector("bit", k, paths, constellation_type="qam", num_bits_per_symbol=nb, hard_out=True)(y, h, s))
    ref_h = o.kbest_detector(y, h, s, pts, paths, hard_out=True)
    assert np.mean(np.all(hard == ref_h, axis=(1, 2))) > 0.99
    if (m, k, nb, paths) == (2, 2, 2, 16):       # full enumeration == max-log ML: more bits right than the linear detector
        lin = _np(phy.mimo.LinearDetector("lmmse", "bit", "maxlog", constellation_type="qam", num_bits_per_symbol=nb)(y, h, s))
        assert np.mean((got > 0) != bits) <= np.mean((lin > 0) != bits)
    with pytest.raises(NotImplementedError):                                   # custom list-to-LLR callables: no HIP path
        phy.mimo.KBestDetector("bit", k, paths, constellation_type="qam", num_bits_per_symbol=nb, list2llr=lambda *a: None)


def test_ofdm_kbest_vs_oracle(phy):
    rg, org = _grids(phy, num_tx=1, ns=2, fft=72, guards=(3, 4))
    sm, osm = phy.mimo.StreamManagement(np.array([[1]]), 2), o.StreamManagement(np.array([[1]]), 2)
    rng = np.random.default_rng(8)
    B, nb = 3, 2
    pts = omap.qam(nb)
    y = _cplx(rng, (B, 1, 4, 14, 72))
    h_hat = _cplx(rng, (B, 1, 4, 1, 2, 14, rg.num_effective_subcarriers))
    got = _np(phy.ofdm.KBestDetector("bit", 2, 8, rg, sm, constellation_type="qam", num_bits_per_symbol=nb)(y, h_hat, 0.0, 0.4))
    ref = o.ofdm_kbest_detector(org, osm, y, h_hat, np.zeros(1, np.float32), 0.4, pts, 8)
    assert got.shape == ref.shape
    assert np.mean(np.isclose(got, ref, rtol=1e-3, atol=2e-3)) > 0.99


# ------------------------------------------------------------------ ZF / MF equalisers
@pytest.mark.parametrize("m,k", [(4, 2), (4, 4), (8, 4), (2, 1), (1, 1)])
def test_zf_mf_equalizers_vs_oracle(phy, m, k):
    rng = np.random.default_rng(m * 3 + k)
    n = 200
    y, h = _cplx(rng, (n, m)), _cplx(rng, (n, m, k))
    a = _cplx(rng, (n, m, m)) * 0.3
    s = (a @ np.conj(np.swapaxes(a, -1, -2)) + 0.2 * np.eye(m)).astype(np.complex64)
    for fn, ref_fn, f32_fn in ((phy.mimo.zf_equalizer, o.zf_equalizer, of32.zf_equalizer),
                               (phy.mimo.mf_equalizer, o.mf_equalizer, of32.mf_equalizer)):
        x, ne = fn(y, h, s)
        fx, fne = f32_fn(y, h, s)
        _same_f32(_np(x), fx) and _same_f32(_np(ne), fne)                   # float32 order-defined oracle: bit for bit
        xr, nr = ref_fn(y, h, s)                                            # complex128 witness (ZF: cond(H^H H) * eps)
        assert np.allclose(_np(x), xr, rtol=2e-3, atol=2e-3 * np.abs(xr).max()) and np.allclose(_np(ne), nr, rtol=2e-3, atol=1e-4 * nr.max())
    # zero forcing removes the interference exactly in the noise-free case
    x0 = _cplx(rng, (n, k))
    xz, _ = phy.mimo.zf_equalizer((h @ x0[..., None])[..., 0], h, s)
    assert np.allclose(_np(xz), x0, rtol=1e-2, atol=1e-2)
    det = phy.mimo.LinearDetector("zf", "bit", "app", constellation_type="qam", num_bits_per_symbol=2)
    assert tuple(det(y, h, s).shape) == (n, k, 2)


@pytest.mark.parametrize("kind", ["zf", "mf"])
def test_ofdm_zf_mf_vs_oracle(phy, kind):
    rg, org = _grids(phy, num_tx=2, ns=1, fft=72, guards=(3, 4))
    sm, osm = phy.mimo.StreamManagement(np.array([[1, 1]]), 1), o.StreamManagement(np.array([[1, 1]]), 1)
    rng = np.random.default_rng(2)
    y = _cplx(rng, (4, 1, 4, 14, 72))
    h_hat = _cplx(rng, (4, 1, 4, 2, 1, 14, rg.num_effective_subcarriers))
    err_var = rng.uniform(0.0, 0.05, (1, 1, 1, 2, 1, 14, rg.num_effective_subcarriers)).astype(np.float32)
    cls = {"zf": phy.ofdm.ZFEqualizer, "mf": phy.ofdm.MFEqualizer}[kind]
    x, ne = cls(rg, sm)(y, h_hat, err_var, 0.2)
    fx, fne = of32.ofdm_equalize(org, osm, y, h_hat, err_var, 0.2, kind)
    _same_f32(_np(x), fx) and _same_f32(_np(ne), fne)
    xr, nr = o.ofdm_linear_equalize(org, osm, y, h_hat, err_var, 0.2, kind)
    assert np.allclose(_np(x), xr, rtol=2e-3, atol=2e-3 * np.abs(xr).max()) and np.allclose(_np(ne), nr, rtol=2e-3, atol=1e-4 * nr.max())
    llr = phy.ofdm.LinearDetector(kind, "bit", "maxlog", rg, sm, constellation_type="qam", num_bits_per_symbol=2)(y, h_hat, err_var, 0.2)
    assert tuple(llr.shape) == (4, 2, 1, rg.num_data_symbols * 2)


def test_flat_fading_channel(phy):
    phy.config.seed = 9
    ch = phy.channel.FlatFadingChannel(3, 4, return_channel=True)
    rng = np.random.default_rng(1)
    x = _cplx(rng, (5000, 3))
    y, h = ch(x)
    assert tuple(h.shape) == (5000, 4, 3) and tuple(y.shape) == (5000, 4)
    assert np.allclose(_np(y), (_np(h) @ x[..., None])[..., 0], rtol=1e-4, atol=1e-5)
    assert abs(np.mean(np.abs(_np(h)) ** 2) - 1.0) < 0.03 and abs(np.mean(_np(h))) < 0.02
    y2, h2 = ch(x, 0.5)
    nvar = np.mean(np.abs(_np(y2) - (_np(h2) @ x[..., None])[..., 0]) ** 2)
    assert abs(nvar - 0.5) < 0.03
    h3 = phy.channel.GenerateFlatFadingChannel(2, 2)(7)
    assert tuple(phy.channel.ApplyFlatFadingChannel()(x[:7, :2], h3).shape) == (7, 2)
    with pytest.raises(TypeError):
        phy.channel.FlatFadingChannel(2, 2, spatial_corr=object())


def test_spatial_correlation_models_match_reference_execution(phy):
    """KroneckerModel / PerColumnModel on the device (one samd_spatial_corr_c64 launch) against the reference's own models
    executed under the NumPy stand-in (tests/golden/spatial_corr_ref_golden.npz), and through FlatFadingChannel: the sample
    covariance of 40000 correlated 16 x 4 channels is R_rx (x) conj... of Simple_MIMO_Simulation.ipynb cell 44."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "spatial_corr_ref_golden.npz"))
    ch = phy.channel
    close = lambda a, b: np.abs(_np(a) - b).max() <= 1e-5 * max(1.0, np.abs(b).max())
    assert close(ch.KroneckerModel(g["exp_04_4"], g["exp_07_16"])(g["h_16x4"]), g["kron_16x4"])
    assert close(ch.KroneckerModel(None, g["exp_07_16"])(g["h_16x4"]), g["kron_rx_only"])
    assert close(ch.KroneckerModel(g["exp_04_4"], None)(g["h_16x4"]), g["kron_tx_only"])
    assert close(ch.KroneckerModel(g["r_tx3"], g["exp_c_5"])(g["h_5x3"]), g["kron_5x3"])
    assert close(ch.PerColumnModel(g["r_cols"])(g["h_5x3"]), g["percol_5x3"])
    phy.config.seed = 5
    r_tx, r_rx = ch.exp_corr_mat(0.4, 4), ch.exp_corr_mat(0.7, 16)
    fc = ch.FlatFadingChannel(4, 16, spatial_corr=ch.KroneckerModel(r_tx, r_rx), return_channel=True)
    x = np.ones((40000, 4), np.complex64)
    y, h = fc(x)
    h = _np(h)
    assert tuple(h.shape) == (40000, 16, 4) and np.allclose(_np(y), h.sum(-1), rtol=1e-4, atol=1e-4)
    cov_rx = np.einsum("bik,bjk->ij", h, h.conj()) / (40000 * 4)                    # E[h h^H] / K = R_rx
    cov_tx = np.einsum("bmi,bmj->ij", h.conj(), h) / (40000 * 16)                    # E[h^H h] / M = conj-free R_tx (real here)
    assert np.abs(cov_rx - r_rx).max() < 0.02 and np.abs(cov_tx - r_tx).max() < 0.02
    fc.spatial_corr = None
    assert fc.spatial_corr is None and tuple(fc(x)[1].shape) == (40000, 16, 4)


# ------------------------------------------------------------------ symbol output (SymbolDemapper, LinearDetector(output="symbol"))
@pytest.mark.parametrize("m", [2, 4, 6])
def test_symbol_demapper_vs_oracle(phy, m):
    rng = np.random.default_rng(m)
    pts = omap.qam(m)
    idx = rng.integers(0, 2 ** m, (6, 120))
    y = (pts[idx] + 0.2 * _cplx(rng, (6, 120))).astype(np.complex64)
    for no in (np.float32(0.3), rng.uniform(0.05, 2.0, (6, 120)).astype(np.float32)):
        got = _np(phy.mapping.SymbolDemapper("qam", m)(y, no))
        ref = omap.symbol_demapper(y, no, pts)
        assert got.shape == (6, 120, 2 ** m)
        # logits reach -|y - c|^2 / no ~ -1e3: float32 carries ~1e-7 of the largest exponent of a symbol
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 + 2e-6 * np.abs(ref).max())
        assert np.allclose(np.exp(got.astype(np.float64)).sum(-1), 1.0, atol=1e-5)          # normalised log-probabilities
        hard = _np(phy.mapping.SymbolDemapper("qam", m, hard_out=True)(y, no))
        assert hard.dtype == np.int32 and np.array_equal(hard, omap.symbol_demapper(y, no, pts, hard_out=True))
    prior = rng.normal(size=(2 ** m,)).astype(np.float32)
    assert np.allclose(_np(phy.mapping.SymbolDemapper("qam", m)(y, 0.3, prior)), omap.symbol_demapper(y, np.float32(0.3), pts, prior),
                       rtol=1e-5, atol=2e-3)
    assert np.array_equal(_np(phy.mapping.SymbolDemapper("qam", m, hard_out=True)(pts[idx], 0.05)), idx)   # noise-free: the sent point


@pytest.mark.parametrize("eq", ["lmmse", "zf", "mf"])
def test_linear_detector_symbol_output(phy, eq):
    """mimo.LinearDetector / ofdm.LinearDetector with output="symbol" (detection.py:24-143, ofdm/detection.py:740-847):
    equaliser (bit for bit the float32 oracle) followed by the symbol demapper (float64 oracle at 1e-5)."""
    rng = np.random.default_rng(5)
    n, m_ant, k, nb = 300, 4, 2, 4
    pts = omap.qam(nb)
    xi = rng.integers(0, 16, (n, k))
    h = (_cplx(rng, (n, m_ant, k)) / np.sqrt(2)).astype(np.complex64)
    y = ((h @ pts[xi][..., None])[..., 0] + 0.05 * _cplx(rng, (n, m_ant))).astype(np.complex64)
    s = (0.01 * np.eye(m_ant)).astype(np.complex64)
    f32 = {"lmmse": of32.lmmse_equalizer, "zf": of32.zf_equalizer, "mf": of32.mf_equalizer}[eq]
    xh, ne = f32(y, h, np.broadcast_to(s, (n, m_ant, m_ant)))
    det = phy.mimo.LinearDetector(eq, "symbol", "app", constellation_type="qam", num_bits_per_symbol=nb)
    logits = _np(det(y, h, s))
    ref = omap.symbol_demapper(xh, ne, pts)
    assert logits.shape == (n, k, 16) and np.allclose(logits, ref, rtol=1e-5, atol=1e-5 + 2e-6 * np.abs(ref).max())
    hard = _np(phy.mimo.LinearDetector(eq, "symbol", "app", constellation_type="qam", num_bits_per_symbol=nb, hard_out=True)(y, h, s))
    assert hard.shape == (n, k) and np.array_equal(hard, omap.symbol_demapper(xh, ne, pts, hard_out=True))
    if eq != "mf":
        assert np.mean(hard == xi) > 0.95
    # OFDM variant
    rg, org = _grids(phy)
    sm, osm = phy.mimo.StreamManagement([[1]], 2), o.StreamManagement([[1]], 2)
    B = 3
    x = omap.qam(2)[rng.integers(0, 4, (B, 1, 2, rg.num_data_symbols))]
    hf = (_cplx(rng, (B, 1, 4, 1, 2, 14, rg.fft_size)) / np.sqrt(2)).astype(np.complex64)
    yf = o.apply_ofdm_channel(o.rg_map(org, x), hf)
    yf = (yf + 0.05 * _cplx(rng, yf.shape)).astype(np.complex64)
    h_perf = o.remove_nulled(org, hf)
    odet = phy.ofdm.LinearDetector(eq, "symbol", "maxlog", rg, sm, "qam", 2, hard_out=True)
    ind = _np(odet(yf, h_perf, 0., 0.005))
    fx, fne = of32.ofdm_equalize(org, osm, yf, h_perf, np.zeros((1,) * 7, np.float32), np.float32(0.005), eq)
    assert ind.shape == (B, 1, 2, rg.num_data_symbols) and np.array_equal(ind, omap.symbol_demapper(fx, fne, omap.qam(2), hard_out=True))
    soft = _np(phy.ofdm.LinearDetector(eq, "symbol", "maxlog", rg, sm, "qam", 2)(yf, h_perf, 0., 0.005))
    assert soft.shape == (B, 1, 2, rg.num_data_symbols, 4)


def test_tdl_spatial_correlation(phy):
    """TDL(..., spatial_corr_mat / rx_corr_mat / tx_corr_mat) (tdl.py:173-190, 474-492): the correlated taps equal the
    matrix square root applied to the uncorrelated taps of the same stream, and their covariance over the batch is R."""
    ra, ta = 4, 2
    rng = np.random.default_rng(3)
    expc = lambda n, rho: rho ** np.abs(np.subtract.outer(np.arange(n), np.arange(n))) * np.exp(1j * 0.3 * np.subtract.outer(np.arange(n), np.arange(n)))
    r_rx, r_tx = expc(ra, 0.7), expc(ta, 0.5)
    sqrtm = lambda r: (lambda w, v: (v * np.sqrt(w)) @ v.conj().T)(*np.linalg.eigh(r))
    mk = lambda **kw: phy.channel.tr38901.TDL("A", 300e-9, 3.5e9, min_speed=3., num_rx_ant=ra, num_tx_ant=ta, **kw)
    phy.config.seed = 9
    a0, _ = mk()(256, 5, 1e4)
    a0 = _np(a0)                                                               # [B,1,ra,1,ta,P,T]
    phy.config.seed = 9
    a1, tau = mk(rx_corr_mat=r_rx, tx_corr_mat=r_tx)(256, 5, 1e4)
    ref = np.einsum("ij,bjkpt,lk->bilpt", sqrtm(r_rx), a0[:, 0, :, 0], sqrtm(r_tx).conj())   # sqrt(Rrx) H sqrt(Rtx)^H
    assert a1.shape == a0.shape and np.allclose(_np(a1)[:, 0, :, 0], ref, rtol=1e-4, atol=1e-5)
    phy.config.seed = 9
    r_full = np.kron(r_rx, r_tx.conj())      # covariance of vec_rx-major(sqrt(Rrx) H sqrt(Rtx)^H) for i.i.d. unit-variance H
    a2, _ = mk(spatial_corr_mat=r_full)(256, 5, 1e4)
    ref2 = np.einsum("ij,bjpt->bipt", sqrtm(r_full), a0[:, 0, :, 0].reshape(256, ra * ta, a0.shape[5], 5))
    assert np.allclose(_np(a2)[:, 0, :, 0].reshape(256, ra * ta, a0.shape[5], 5), ref2, rtol=1e-4, atol=1e-5)
    # statistics: covariance of the antenna-pair vector of the strongest tap, normalised by its power
    phy.config.seed = 10
    a3, _ = mk(rx_corr_mat=r_rx, tx_corr_mat=r_tx)(20000, 1, 1e4)
    v = _np(a3)[:, 0, :, 0, :, 0, 0].reshape(20000, ra * ta)
    cov = (v.T @ v.conj()) / 20000
    cov = cov / np.real(np.trace(cov)) * (ra * ta)
    assert np.allclose(cov, r_full, atol=0.06)


@pytest.mark.parametrize("name", ["c4", "cdl", "c4b"])
def test_receiver_front_end_matches_reference_execution(phy, name):
    """The HIP blocks against outputs of the reference's OWN ResourceGridMapper / RemoveNulledSubcarriers /
    LSChannelEstimator ("nn", "lin", "lin_time_avg") / LMMSE, ZF, MF equalizers / LinearDetector / MMSEPICDetector /
    KBestDetector / EPDetector code with ESTIMATED channel state (tests/golden/ofdm_rx_ref_golden.npz,
    tools/gen_ofdm_rx_ref_golden.py): guard carriers, DC null, error variance > 0, per-example noise variance.  Bars as
    in tests/test_oracle_ref_exec_ofdm_rx.py (the oracle's twin of this test)."""
    # "c4b": BASELINE config C4's grid itself (1 transmitter x 2 streams, guards [5, 6], 4 receive antennas, QPSK;
    # tools/gen_ofdm_rx_ref_golden.py --baseline)
    L = {"c4": dict(fft=76, guards=(3, 4), num_tx=2, spt=1, m=4, kbest=16), "cdl": dict(fft=72, guards=(5, 6), num_tx=1, spt=4, m=2, kbest=32),
         "c4b": dict(fft=76, guards=(5, 6), num_tx=1, spt=2, m=2, kbest=16)}[name]
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "ofdm_rx_ref_golden_c4.npz" if name == "c4b" else "ofdm_rx_ref_golden.npz"))
    g = {k.split("/", 1)[1]: gold[k] for k in gold.files if k.startswith(name + "/")}
    rg = phy.ofdm.ResourceGrid(14, L["fft"], 15e3, num_tx=L["num_tx"], num_streams_per_tx=L["spt"], cyclic_prefix_length=6,
                               num_guard_carriers=list(L["guards"]), dc_null=True, pilot_pattern="kronecker", pilot_ofdm_symbol_indices=[2, 11])
    assert np.array_equal(rg.pilot_pattern.mask, g["mask"].astype(bool))
    rg.pilot_pattern.pilots = g["pilots"]
    sm = phy.mimo.StreamManagement(np.ones([1, L["num_tx"]]), L["spt"])
    m = L["m"]

    def close(a, b, tol=1e-5):
        a = _np(a) if isinstance(a, torch.Tensor) else np.asarray(a)
        a, b = np.broadcast_arrays(a, b) if a.ndim == b.ndim else (a.reshape(b.shape), b)
        return np.abs(a - b).max() <= 4 * tol * np.abs(b).max()

    def rel(a, b, floor):
        a = _np(a).reshape(b.shape)
        return np.abs(a - b) / np.maximum(np.abs(b), floor)

    x = phy.mapping.Mapper("qam", m)(g["b"].astype(np.float32))
    assert np.array_equal(_np(phy.ofdm.ResourceGridMapper(rg)(x)), g["x_rg"])
    y, no = g["y"], g["no"]
    assert np.array_equal(_np(phy.ofdm.RemoveNulledSubcarriers(rg)(y)), g["removed"])
    for it in ("nn", "lin", "lin_time_avg"):
        h, ev = phy.ofdm.LSChannelEstimator(rg, interpolation_type=it)(y, no)
        assert close(h, g[f"h_hat_{it}"]) and close(ev, g[f"err_var_{it}"]), it
    if name == "c4b":
        # the bench's receiver on its own grid: LS (nearest neighbour, DEFERRED h_hat) -> LMMSE: the fused kernel
        # (samd_ofdm_lsnn_lmmse_c64) and, through LinearDetector, the fused kernel with the app demapper
        h_d, ev_d = phy.ofdm.LSChannelEstimator(rg)(y, no)
        xh, ne = phy.ofdm.LMMSEEqualizer(rg, sm)(y, h_d, ev_d, no)
        assert close(xh, g["x_hat_lmmse_nn"], 2e-5) and close(ne, g["no_eff_lmmse_nn"], 2e-5)
        h_d, ev_d = phy.ofdm.LSChannelEstimator(rg)(y, no)
        det = phy.ofdm.LinearDetector("lmmse", "bit", "app", rg, sm, constellation_type="qam", num_bits_per_symbol=m, hard_out=False)
        assert close(det(y, h_d, ev_d, no), g["llr_lmmse_nn_app"], 4e-5)
    hh, ev = g["h_hat_lin"], g["err_var_lin"]
    for kind, cls in (("lmmse", phy.ofdm.LMMSEEqualizer), ("mf", phy.ofdm.MFEqualizer)):
        xh, ne = cls(rg, sm)(y, hh, ev, no)
        assert close(xh, g[f"x_hat_{kind}"], 2e-5) and close(ne, g[f"no_eff_{kind}"], 2e-5), kind
    xh, ne = phy.ofdm.ZFEqualizer(rg, sm)(y, hh, ev, no)                    # (conditioning: see the oracle's twin)
    for a, b in ((xh, g["x_hat_zf"]), (ne, g["no_eff_zf"])):
        r = rel(a, b, 1e-3 * np.abs(b).max())
        assert r.max() < 1.5e-2 and np.quantile(r, 0.99) < 2e-4, (r.max(), np.quantile(r, 0.99))   # (measured 5.5e-3 / 6.8e-5)
    kw = dict(constellation_type="qam", num_bits_per_symbol=m, hard_out=False)
    for meth in ("app", "maxlog"):
        assert close(phy.ofdm.LinearDetector("lmmse", "bit", meth, rg, sm, **kw)(y, hh, ev, no), g[f"llr_lmmse_{meth}"], 4e-5), meth
    r = rel(phy.ofdm.LinearDetector("zf", "bit", "maxlog", rg, sm, **kw)(y, hh, ev, no), g["llr_zf_maxlog"], 1e-2 * np.abs(g["llr_zf_maxlog"]).max())
    assert r.max() < 1e-2 and np.quantile(r, 0.99) < 4e-4, (r.max(), np.quantile(r, 0.99))
    for meth in ("app", "maxlog"):
        pic = phy.ofdm.MMSEPICDetector(output="bit", demapping_method=meth, resource_grid=rg, stream_management=sm, num_iter=2,
                                       constellation_type="qam", num_bits_per_symbol=m, hard_out=False)
        assert close(pic(y, hh, g["prior"], ev, no), g[f"llr_pic_{meth}"], 1e-4), meth
    kb = _np(phy.ofdm.KBestDetector("bit", L["num_tx"] * L["spt"], L["kbest"], rg, sm, **kw)(y, hh, ev, no))
    assert np.mean(np.isclose(kb.reshape(g["llr_kbest"].shape), g["llr_kbest"], rtol=1e-4, atol=1e-3)) > 0.99
    r = rel(phy.ofdm.EPDetector("bit", rg, sm, m, l=6, hard_out=False)(y, hh, ev, no), g["llr_ep"], 1.0)
    assert r.max() < 6e-2 and np.quantile(r, 0.5) < 2e-3, (r.max(), np.quantile(r, 0.5))   # (measured 2.9e-2 / 4.4e-7 and 4.5e-3 / 3.7e-4)


def test_estimate_at_pilot_locations(phy):
    """LSChannelEstimator.estimate_at_pilot_locations (channel_estimation.py:257-285): y at the pilots / pilots with
    divide_no_nan, err_var = no / |pilots|^2 - against the NumPy formula and consistent with the block's own call."""
    rg, org = _grids(phy, num_tx=1, ns=4, fft=72)
    pp = rg.pilot_pattern
    rng = np.random.default_rng(3)
    B = 3
    yp = _cplx(rng, (B, 1, 4) + tuple(pp.mask.shape[:2]) + (pp.num_pilot_symbols,))
    no = np.array([0.1, 0.2, 0.4], np.float32)
    h, ev = phy.ofdm.LSChannelEstimator(rg).estimate_at_pilot_locations(yp, no)
    pil = np.asarray(pp.pilots)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = np.where(pil != 0, yp / np.where(pil != 0, pil, 1), 0).astype(np.complex64)
        ref_ev = np.where(pil != 0, no[:, None, None, None, None, None] / np.where(pil != 0, np.abs(pil) ** 2, 1), 0)
    assert np.allclose(_np(h), ref, rtol=1e-6, atol=1e-7) and np.allclose(np.broadcast_to(_np(ev), ref_ev.shape), ref_ev, rtol=1e-6)
    assert phy.mimo.KBestDetector("bit", 2, 4, "qam", 2).list2llr is None
