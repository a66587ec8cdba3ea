"""The NR PUSCH receiver on the host: the specification of the DMRS least-squares kernel (tests/pusch_rx_f32.py) against the
reference's own PUSCHLSChannelEstimator executed under the NumPy stand-in (tests/golden/pusch_rx_ref_golden.npz, made by
tools/gen_pusch_rx_ref_golden.py), the reference's noiseless criterion, the error variance, ``time_to_ofdm_channel`` on host
tensors, the signatures and the refusals.  None of this needs a device."""
import json
import os
import types

import numpy as np
import pytest
import torch

import pusch_rx_f32 as spec
from pusch_rx_cases import CONFIGS, G, GOLD, NO, bound, configs, estimator_of, grid_of, inside, specification
from sionna_amd.phy import nr
from sionna_amd.phy.channel import time_to_ofdm_channel


@pytest.fixture(scope="module")
def built():
    """per fixture configuration: parameters, resource grid and a nearest-neighbour estimator, built once on the host"""
    out = {}
    for name, specs in CONFIGS.items():
        par, rg = grid_of(configs(specs))
        out[name] = (par, rg, estimator_of(par, rg, "nn"))
    return out


def test_the_fixture_covers_the_reference_loops_and_stays_small():
    seen = {k: set() for k in ("layers", "ports", "length", "add", "type", "cdm", "codebook", "tx")}
    for specs in CONFIGS.values():
        p, d = specs[0]["pusch"], specs[0]["dmrs"]
        seen["layers"].add(p["num_layers"]), seen["ports"].add(p["num_antenna_ports"]), seen["length"].add(d["length"])
        seen["add"].add((d["length"], d["additional_position"])), seen["type"].add((d["config_type"], d["num_cdm_groups_without_data"]))
        seen["codebook"].add((p["precoding"], p.get("tpmi"), p["num_layers"] < p["num_antenna_ports"])), seen["tx"].add(len(specs))
        assert 1 <= p["n_size_bwp"] <= 4
    assert seen["layers"] >= {1, 2, 4} and seen["ports"] == {1, 2, 4} and seen["length"] == {1, 2} and seen["tx"] == {1, 3}
    assert seen["add"] == {(1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1)}
    assert seen["type"] == {(1, 1), (1, 2), (2, 1), (2, 2), (2, 3)}
    assert ("codebook", 2, True) in seen["codebook"] and ("non-codebook", None, False) in seen["codebook"]
    assert [s["pusch"]["tpmi"] for s in CONFIGS["three_tx"]] == [2, 11, 16]
    assert [s["dmrs"]["dmrs_port_set"] for s in CONFIGS["three_tx"]] == [[0, 1], [2, 3], [4, 5]]
    assert os.path.getsize(os.path.join(GOLD, "pusch_rx_ref_golden.npz")) < 1 << 20
    assert G[f"{next(iter(CONFIGS))}/y"].shape[:3] == (2, 1, 2)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_tables_match_the_reference_pattern(built, name):
    par, rg, est = built[name]
    t = est._host_tables()
    assert np.array_equal(t["pilots"].reshape(G[f"{name}/pilots"].shape), G[f"{name}/pilots"])
    assert np.array_equal(t["coef"], spec.reciprocal_table(t["pilots"])) and t["coef"].dtype == np.complex64
    assert t["src"].min() >= 0 and t["src"].max() < rg.num_ofdm_symbols * rg.fft_size
    assert t["gather"].min() >= 0 and t["gather"].max() < t["src"].shape[1]
    assert est._run == 2 * par["num_cdm_groups_without_data"] and est._num_pilots_per_dmrs_sym % est._run == 0
    assert est._num_dmrs_syms == par["dmrs_length"] * (par["dmrs_additional_position"] + 1)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_specification_against_the_reference(built, name):
    """at the pilots and through the nearest-neighbour table, float32; inside (2 n + 11) u W of pusch_rx_f32.error_bound, and the
    zero pattern (masked pilots of the other CDM ports) is the same"""
    par, rg, est = built[name]
    y = G[f"{name}/y"]
    t = est._host_tables()
    y_pilots_rows = y.reshape(-1, y.shape[-2] * y.shape[-1])
    at_pilots = specification(est, y, nn=False)
    ref = G[f"{name}/h_pilots"]
    assert at_pilots.shape == ref.shape and at_pilots.dtype == ref.dtype == np.complex64
    worst, ok = inside(at_pilots, ref, bound(est, y, nn=False))
    print(f"{name}: at the pilots, max error / bound = {worst:.3f}")
    assert ok and np.array_equal(at_pilots == 0, ref == 0) and (ref == 0).any() == (t["coef"] == 0).any()
    grid = specification(est, y, nn=True)
    ref = G[f"{name}/h_hat_nn"]
    worst, ok = inside(grid, ref, bound(est, y, nn=True))
    print(f"{name}: nearest neighbour, max error / bound = {worst:.3f}")
    assert grid.shape == ref.shape and ok and not (ref == 0).any()
    # float64: the same evaluation, against the float32 fixture within the float32 bound
    est64 = estimator_of(*grid_of(configs(CONFIGS[name]), "double"), "nn", "double")
    wide = specification(est64, y.astype(np.complex128), nn=True, dtype=np.float64)
    assert wide.dtype == np.complex128 and inside(wide, ref, bound(est, y, nn=True))[1]
    assert y_pilots_rows.shape[0] == 4


@pytest.mark.parametrize("name", list(CONFIGS))
def test_noiseless_block_fading_gives_the_precoded_channel(built, name):
    """the reference's own criterion (test/unit/nr/test_channel_estimation.py:57-61): without noise the nearest-neighbour
    estimate equals the true effective channel under np.allclose(atol=1e-6); the effective channel h W is the fixture's
    recording of the reference receiver's perfect-CSI branch"""
    par, rg, est = built[name]
    h_hat = specification(est, G[f"{name}/y_clean"], nn=True)
    h_eff = G[f"{name}/h_eff"]
    assert h_eff.shape[:5] == h_hat.shape[:5] and h_eff.shape[5:] == (1, 1)
    assert np.allclose(np.broadcast_to(h_eff, h_hat.shape), h_hat, atol=1e-6)
    if par["precoding"] == "codebook":
        w = np.stack(par["precoding_matrices"])
        mine = np.einsum("brmta,tal->brmtl", G[f"{name}/h"].astype(np.complex128), w)
        assert np.allclose(mine, h_eff[..., 0, 0], atol=1e-6)
    else:
        assert np.array_equal(h_eff[..., 0, 0], G[f"{name}/h"])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_error_variance_equals_the_reference(built, name):
    par, rg, est = built[name]
    t = est._host_tables()
    shape = np.asarray(rg.pilot_pattern.mask).shape[:2] + (-1,)
    no_b = G[f"{name}/no_batch"]
    got = spec.error_variance(no_b.reshape(-1, 1, 1, 1, 1, 1), t["pilots"].reshape(shape), par["dmrs_length"])
    ref = G[f"{name}/err_var_pilots"]
    assert got.dtype == ref.dtype == np.float32 and np.array_equal(np.broadcast_to(got, ref.shape), ref)
    # the estimator's table is the same numbers as one division: no / (|pilot|^2 * 2 [* 2])
    live = t["den"] != 0
    table = np.where(live, np.float32(NO) / np.where(live, t["den"], np.float32(1)), np.float32(0))
    assert np.array_equal(table.reshape(shape), spec.error_variance(np.float32(NO), t["pilots"].reshape(shape), par["dmrs_length"]))
    nn = np.take_along_axis(table, t["gather"], axis=1).reshape(np.asarray(rg.pilot_pattern.mask).shape)
    assert np.array_equal(nn[None, None, None], G[f"{name}/err_var_nn"])


@pytest.mark.parametrize("j", [0, 1])
def test_time_to_ofdm_channel_on_host_tensors(j):
    fft, cp, nsym, l_min, l_max = (int(v) for v in G[f"t2f/{j}/params"])
    rg = types.SimpleNamespace(fft_size=fft, cyclic_prefix_length=cp, num_time_samples=(fft + cp) * nsym)
    h_t, ref = G[f"t2f/{j}/h_t"], G[f"t2f/{j}/h_f"]
    got = time_to_ofdm_channel(torch.from_numpy(h_t), rg, l_min)
    assert got.device.type == "cpu" and tuple(got.shape) == ref.shape == h_t.shape[:-2] + (nsym, fft)
    assert got.numpy().dtype == ref.dtype == h_t.dtype
    assert np.abs(got.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    # the definition (channel/utils.py:366): lag k of the symbol's first sample after the prefix rotates by exp(-2 pi j k n / N)
    k, n = np.arange(l_min, l_max + 1), np.arange(fft) - fft // 2
    direct = np.einsum("...sk,kn->...sn", h_t[..., cp::fft + cp, :][..., :nsym, :].astype(np.complex128), np.exp(-2j * np.pi * np.outer(k, n) / fft))
    assert np.abs(got.numpy() - direct).max() <= 1e-5 * np.abs(direct).max()
    assert np.array_equal(time_to_ofdm_channel(h_t, rg, l_min).numpy(), got.numpy())


def test_signatures_match_the_reference():
    from test_api_signatures import _check
    from sionna_amd.phy import channel
    with open(os.path.join(GOLD, "pusch_rx_api_signatures.json")) as f:
        table = json.load(f)["signatures"]
    assert sorted(table) == ["channel.time_to_ofdm_channel", "nr.PUSCHLSChannelEstimator", "nr.PUSCHReceiver"]
    _check(table["channel.time_to_ofdm_channel"]["params"], channel.time_to_ofdm_channel, "time_to_ofdm_channel")
    for name in ("PUSCHLSChannelEstimator", "PUSCHReceiver"):
        ref, obj = table["nr." + name], getattr(nr, name)
        _check(ref["__init__"], obj.__init__, name + ".__init__")
        if "call" in ref:                                            # the estimator inherits LSChannelEstimator.call
            _check(ref["call"], obj.call, name + ".call")
        for attr, kind, prm in ref["public"]:
            if kind == "property":
                assert isinstance(getattr(obj, attr), property), f"{name}.{attr}"
            else:
                _check(prm, getattr(obj, attr), f"{name}.{attr}")
    from sionna_amd.phy.ofdm import LSChannelEstimator
    assert issubclass(nr.PUSCHLSChannelEstimator, LSChannelEstimator)
    assert "call" in table["nr.PUSCHReceiver"] and [p[0] for p in table["nr.PUSCHReceiver"]["public"]] == ["resource_grid"]
    assert [p[0] for p in table["nr.PUSCHLSChannelEstimator"]["public"]] == ["estimate_at_pilot_locations"]


class _Transmitter(types.SimpleNamespace):
    """what PUSCHReceiver reads of a transmitter before it builds a device block"""


def _stub():
    par, rg = grid_of(configs(CONFIGS["nc1_len1_add0_type1_cdm1"]))
    return _Transmitter(resource_grid=rg, _num_subcarriers=12, _cyclic_prefix_length=0)


def test_a_bad_input_domain_is_refused():
    with pytest.raises(AssertionError, match="input_domain must be 'time' or 'freq'"):
        nr.PUSCHReceiver(_stub(), input_domain="frequency")


def test_the_time_domain_needs_l_min():
    with pytest.raises(AssertionError, match="l_min must be provided"):
        nr.PUSCHReceiver(_stub(), input_domain="time")


def test_perfect_csi_needs_h():
    pcs = configs(CONFIGS["nc1_len1_add0_type1_cdm1"])
    par, rg = grid_of(pcs)
    tx = _Transmitter(resource_grid=rg, _precoding="non-codebook", _num_tx=1, _num_layers=1, _layer_mapper=nr.LayerMapper(1),
                      _num_bits_per_symbol=2)
    rx = nr.PUSCHReceiver(tx, channel_estimator="perfect", mimo_detector=lambda *a: None, tb_decoder=lambda llr: (llr, None))
    with pytest.raises(AssertionError, match="h must be provided"):
        rx.call(np.zeros((1, 1, 1, 14, 12), np.complex64), 0.1)


def test_estimator_refusals():
    par, rg = grid_of(configs(CONFIGS["nc1_len1_add0_type1_cdm1"]))
    with pytest.raises(AssertionError, match="Unsupported `interpolation_type`"):
        nr.PUSCHLSChannelEstimator(rg, 1, 0, 1, interpolation_type="cubic")
    with pytest.raises(AssertionError, match="whole runs"):
        nr.PUSCHLSChannelEstimator(rg, 1, 0, 2)                      # 6 pilots per DMRS symbol are no runs of 4
    with pytest.raises(AssertionError, match="dmrs_length"):
        nr.PUSCHLSChannelEstimator(rg, 3, 0, 1)
