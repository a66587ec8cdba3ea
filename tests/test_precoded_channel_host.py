"""Host side of the precoded channels and the post-equalisation SINR (no GPU needed): the specification of
tests/precoded_channel_f32.py against the reference-executed fixture within the bars measured from the reference itself,
the closed forms of the reference's own tests, the reference's signatures, and the refusals that are raised before anything
reaches the device."""
import json
import os

import numpy as np
import pytest

import precoded_channel_f32 as spec

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
FIX = np.load(os.path.join(GOLD, "precoded_channel_ref_golden.npz"))
CASES = [str(c) for c in FIX["cases"]]


def case(name):
    from sionna_amd.phy.mimo import StreamManagement
    g = {k.split("/", 1)[1]: FIX[k] for k in FIX.files if k.startswith(name + "/")}
    return g, StreamManagement(g["rx_tx_association"], int(g["num_streams_per_tx"]))


def families(name):
    return ["eye"] if name == "eye" else ["rzf", "cbf"]


def test_the_bars_are_the_ones_the_generator_measured():
    """E32 of the specification module is the table the generator printed (three digits)"""
    assert set(spec.E32) == {k.split("/", 1)[1] for k in FIX.files if k.startswith("e32/")}
    for fam, e in spec.E32.items():
        assert abs(e - float(FIX[f"e32/{fam}"])) <= 1e-3 * float(FIX[f"e32/{fam}"]), fam
    # the fixture states what it measures: the reference's single result against its own double result
    e = {}
    for name in CASES:
        g, _ = case(name)
        for fam in families(name):
            e[fam] = max(e.get(fam, 0.0), spec.rel_dev(g[f"h_eff_{fam}32"], g[f"h_eff_{fam}64"]))
        for tag, fam in (("w", "sinr_whitened"), ("u", "sinr_unwhitened")):
            for hat in ("", "hat_"):
                if f"sinr_{hat}{tag}32" in g:
                    e[fam] = max(e.get(fam, 0.0), spec.rel_dev(g[f"sinr_{hat}{tag}32"], g[f"sinr_{hat}{tag}64"]))
    for fam in spec.E32:
        assert e[fam] == float(FIX[f"e32/{fam}"]), fam


def test_fixture_inputs_are_float32_representable_and_well_conditioned():
    for name in CASES:
        g, _ = case(name)
        assert g["h"].dtype == np.complex64 and g["tx_power"].dtype == np.float32 and g["no"].dtype == np.float32
        assert np.all(g["no"] >= 0.01) and np.all(g["tx_power"] >= 0)
        if "alpha" in g and np.any(g["alpha"] == 0):
            assert int(g["num_streams_per_tx"]) < g["h"].shape[4], name          # alpha = 0 only where K < M


@pytest.mark.parametrize("name", CASES)
def test_precoded_channel_spec_within_the_measured_bars(name):
    g, sm = case(name)
    for fam in families(name):
        for dtype, cd, bar in ((np.float32, np.complex64, spec.bar32(fam)), (np.float64, np.complex128, spec.bar64(fam))):
            he = spec.precoded_channel(g["h"], g["tx_power"], sm.precoding_ind, g["effective_subcarrier_ind"], fam,
                                       h_hat=g.get("h_hat"), alpha=g.get("alpha", 0.), dtype=dtype)
            assert he.dtype == cd
            dev = spec.rel_dev(he, g[f"h_eff_{fam}64"])
            print(name, fam, dtype.__name__, f"deviation {dev:.3e} bar {bar:.3e}")
            assert dev <= bar, (name, fam, dtype.__name__, dev, bar)
    if name == "mu8":                                                            # the stream without power
        assert np.all(spec.precoded_channel(g["h"], g["tx_power"], sm.precoding_ind, g["effective_subcarrier_ind"], "rzf",
                                            alpha=g["alpha"])[:, :, :, :, 2] == 0)


@pytest.mark.parametrize("whitening", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_sinr_spec_within_the_measured_bars(name, whitening):
    g, sm = case(name)
    fam, tag = ("sinr_whitened", "w") if whitening else ("sinr_unwhitened", "u")
    h_eff = g[f"h_eff_{families(name)[0]}32"]
    for hat in ("", "hat_"):
        if f"sinr_{hat}{tag}64" not in g:
            continue
        for dtype, bar in ((np.float32, spec.bar32(fam)), (np.float64, spec.bar64(fam))):
            s = spec.lmmse_post_eq_sinr(g["h_eff_hat"] if hat else h_eff, g["no"], sm.detection_desired_ind,
                                        sm.detection_undesired_ind, whitening, dtype=dtype)
            assert s.dtype == dtype
            dev = spec.rel_dev(s, g[f"sinr_{hat}{tag}64"])
            print(name, fam, hat, dtype.__name__, f"deviation {dev:.3e} bar {bar:.3e}")
            assert dev <= bar, (name, fam, hat, dtype.__name__, dev, bar)
    if name == "mu8":
        s = spec.lmmse_post_eq_sinr(h_eff, g["no"], sm.detection_desired_ind, sm.detection_undesired_ind, whitening)
        assert np.all(s[:, :, :, 2, 0] == 0) and np.all(s[:, :, :, 0, 0] > 0)      # no power: exactly 0


def _cn(rng, shape):
    return ((rng.normal(size=shape) + 1j * rng.normal(size=shape)) / np.sqrt(2)).astype(np.complex64)


def test_closed_form_siso():
    """the reference's test_siso (test/unit/ofdm/test_post_eq_sinr.py:128-179): one antenna each side, SINR = |h|^2 p / no,
    with tx_power, alpha and no given by their first dims; relative 1e-6 in double precision as there"""
    from sionna_amd.phy.mimo import StreamManagement
    rng = np.random.default_rng(1)
    B, T, F = 4, 3, 16
    sm = StreamManagement(np.array([[1]]), 1)
    h = _cn(rng, (B, 1, 1, 1, 1, T, F))
    p, alpha, no = rng.random((B, 1, 1, T)).astype(np.float32), rng.random((B, 1)).astype(np.float32), \
        (0.01 + rng.random((B, 1, 1))).astype(np.float32)
    he = spec.precoded_channel(h, p, sm.precoding_ind, np.arange(F), "rzf", alpha=alpha, dtype=np.float64)
    s = spec.lmmse_post_eq_sinr(he, no, sm.detection_desired_ind, sm.detection_undesired_ind, True, dtype=np.float64)
    theo = np.abs(h[:, 0, 0, 0, 0].astype(np.complex128)) ** 2 * p[:, 0, 0, :, None].astype(np.float64) / no[:, 0, 0, None, None]
    assert np.max(np.abs(theo - s[..., 0, 0]) / s[..., 0, 0]) < 1e-6


def test_closed_form_single_antenna_uplink():
    """the reference's test_single_antenna_uplink (:181-244): 8 single-antenna transmitters towards one 16-antenna receiver,
    identity precoder; SINR from the LMMSE matrix of the power-scaled, noise-whitened channel in complex128"""
    from sionna_amd.phy.mimo import StreamManagement
    rng = np.random.default_rng(2)
    B, T, F, RA, NTX = 3, 2, 8, 16, 8
    sm = StreamManagement(np.ones((1, NTX), int), 1)
    h = _cn(rng, (B, 1, RA, NTX, 1, T, F))
    p, no = rng.random((B, NTX, 1, T)).astype(np.float32), (0.01 + rng.random((B, 1, RA))).astype(np.float32)
    he = spec.precoded_channel(h, p, sm.precoding_ind, np.arange(F), "eye", dtype=np.float64)
    s = spec.lmmse_post_eq_sinr(he, no, sm.detection_desired_ind, sm.detection_undesired_ind, True, dtype=np.float64)[:, :, :, 0]
    h_e = np.transpose(h[:, 0, :, :, 0].astype(np.complex128), [0, 3, 4, 1, 2])                  # [B, T, F, RA, NTX]
    h_e = h_e * np.sqrt(np.transpose(p[:, :, 0].astype(np.float64), [0, 2, 1]))[:, :, None, None, :]
    h_e = h_e / np.sqrt(no[:, 0].astype(np.float64))[:, None, None, :, None]
    hh = np.conj(np.swapaxes(h_e, -1, -2))
    f = np.linalg.solve(hh @ h_e + np.eye(NTX), hh)
    fh = np.abs(f @ h_e) ** 2
    signal = np.einsum("...ii->...i", fh)
    theo = signal / (fh.sum(-1) - signal + (np.abs(f) ** 2).sum(-1))
    assert np.max(np.abs(s - theo) / np.abs(s)) < 1e-6


def test_signatures_match_the_reference():
    from test_api_signatures import _check
    with open(os.path.join(GOLD, "precoded_channel_api_signatures.json")) as f:
        sig = json.load(f)["signatures"]
    assert set(sig) == {"ofdm.PrecodedChannel", "ofdm.RZFPrecodedChannel", "ofdm.CBFPrecodedChannel", "ofdm.EyePrecodedChannel",
                        "ofdm.PostEqualizationSINR", "ofdm.LMMSEPostEqualizationSINR"}
    from sionna_amd.phy import ofdm
    for name, ref in sig.items():
        cls = getattr(ofdm, name.rsplit(".", 1)[1])
        assert cls is getattr(ofdm.precoding if "Precoded" in name else ofdm.equalization, cls.__name__)
        if ref.get("__init__"):
            _check(ref["__init__"], cls.__init__, name + ".__init__")
        _check(ref["call"], cls.call, name + ".call")
        for base in ref["bases"]:
            assert base in [b.__name__ for b in cls.__mro__], (name, base)
        for attr, _, params in ref["public"]:
            _check(params, getattr(cls, attr), f"{name}.{attr}")
    for helper in ("get_desired_channels", "compute_effective_channel", "apply_tx_power"):
        assert helper in vars(ofdm.PrecodedChannel)
    for helper in ("get_per_rx_channels", "compute_interference_covariance_matrix", "compute_desired_signal_power",
                   "compute_total_power", "compute_noise_power", "compute_sinr"):
        assert helper in vars(ofdm.PostEqualizationSINR)


def _grid(num_tx=1, streams=4):
    from sionna_amd.phy import ofdm
    return ofdm.ResourceGrid(num_ofdm_symbols=2, fft_size=16, subcarrier_spacing=15e3, num_tx=num_tx, num_streams_per_tx=streams,
                             cyclic_prefix_length=2, num_guard_carriers=[2, 1], dc_null=True, pilot_pattern=None)


def _z(*s):
    return np.zeros(s, np.complex64)


def _blocks(streams=4, assoc=((1,),)):
    from sionna_amd.phy import mimo, ofdm
    rg, sm = _grid(len(assoc[0]), streams), mimo.StreamManagement(np.array(assoc), streams)
    return ofdm, rg, sm


def test_refusal_h_of_another_grid():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="h must have shape"):
        ofdm.RZFPrecodedChannel(rg, sm)(_z(2, 1, 4, 1, 8, 2, 12), 1.0)


def test_refusal_h_hat_of_another_shape():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="h_hat must have the shape of h"):
        ofdm.CBFPrecodedChannel(rg, sm)(_z(2, 1, 4, 1, 8, 2, 16), 1.0, h_hat=_z(2, 1, 4, 1, 4, 2, 16))


def test_refusal_channel_rows_do_not_match_the_streams():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="channel rows"):
        ofdm.RZFPrecodedChannel(rg, sm)(_z(2, 1, 2, 1, 8, 2, 16), 1.0)


def test_refusal_more_streams_than_antennas():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="K <= M"):
        ofdm.CBFPrecodedChannel(rg, sm)(_z(2, 1, 4, 1, 2, 2, 16), 1.0)


def test_refusal_sizes_beyond_the_kernel():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="M = 32"):
        ofdm.RZFPrecodedChannel(rg, sm)(_z(1, 1, 4, 1, 40, 2, 16), 1.0)
    ofdm, rg, sm = _blocks(streams=17)
    with pytest.raises(ValueError, match="K = 16"):
        ofdm.RZFPrecodedChannel(rg, sm)(_z(1, 1, 17, 1, 20, 2, 16), 1.0)


def test_refusal_identity_precoder_needs_k_equal_m():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="K == M"):
        ofdm.EyePrecodedChannel(rg, sm)(_z(2, 1, 4, 1, 8, 2, 16), 1.0)


def test_refusal_tx_power_shape():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="tx_power must have shape"):
        ofdm.RZFPrecodedChannel(rg, sm)(_z(2, 1, 4, 1, 8, 2, 16), np.ones((2, 1, 3), np.float32))


def test_refusal_alpha_shape():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="alpha must have shape"):
        ofdm.RZFPrecodedChannel(rg, sm)(_z(2, 1, 4, 1, 8, 2, 16), 1.0, alpha=np.ones((16,), np.float32))


def test_refusal_grid_and_stream_management_disagree():
    from sionna_amd.phy import mimo, ofdm
    with pytest.raises(ValueError, match="disagree"):
        ofdm.RZFPrecodedChannel(_grid(streams=2), mimo.StreamManagement(np.array([[1]]), 4))(_z(1, 1, 4, 1, 8, 2, 16), 1.0)


def test_refusal_sinr_h_eff_shape():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="h_eff must have shape"):
        ofdm.LMMSEPostEqualizationSINR(rg, sm)(_z(2, 1, 4, 1, 3, 2, 12), 0.1)


def test_refusal_sinr_h_eff_hat_shape():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="h_eff_hat must have the shape"):
        ofdm.LMMSEPostEqualizationSINR(rg, sm)(_z(2, 1, 4, 1, 4, 2, 12), 0.1, h_eff_hat=_z(2, 1, 4, 1, 4, 2, 11))


def test_refusal_sinr_no_shape():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="no must have shape"):
        ofdm.LMMSEPostEqualizationSINR(rg, sm)(_z(2, 1, 4, 1, 4, 2, 12), np.ones((3,), np.float32))


def test_refusal_sinr_sizes_beyond_the_kernel():
    ofdm, rg, sm = _blocks()
    with pytest.raises(ValueError, match="16 receive antennas"):
        ofdm.LMMSEPostEqualizationSINR(rg, sm)(_z(1, 1, 17, 1, 4, 2, 12), 0.1)
    ofdm, rg, sm = _blocks(streams=17)
    with pytest.raises(ValueError, match="16 streams per receiver"):
        ofdm.LMMSEPostEqualizationSINR(rg, sm)(_z(1, 1, 4, 1, 17, 2, 12), 0.1)


def test_abstract_bases_cannot_be_called():
    ofdm, rg, sm = _blocks()
    with pytest.raises(TypeError):
        ofdm.PrecodedChannel(rg, sm)
    with pytest.raises(TypeError):
        ofdm.PostEqualizationSINR(rg, sm)


def test_no_cpu_fallback_without_gpu(monkeypatch):
    import torch
    from sionna_amd import _ffi
    monkeypatch.setattr(_ffi, "_device", None)                                   # as in a process that sees no device
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ofdm, rg, sm = _blocks()
    h = np.ones((1, 1, 4, 1, 8, 2, 16), np.complex64)
    for cls in (ofdm.RZFPrecodedChannel, ofdm.CBFPrecodedChannel):
        with pytest.raises(RuntimeError):
            cls(rg, sm)(h, 1.0)
    with pytest.raises(RuntimeError):
        ofdm.LMMSEPostEqualizationSINR(rg, sm)(np.ones((1, 1, 4, 1, 4, 2, 12), np.complex64), 0.1)
