"""The PUSCH DMRS least-squares kernel (csrc/pusch_rx.hip) against its specification tests/pusch_rx_f32.py, bit for bit, in
complex64 and complex128; ``PUSCHLSChannelEstimator`` against the reference's executed outputs (tests/golden/
pusch_rx_ref_golden.npz); ``PUSCHReceiver`` end to end on the reference's own link tests (test/unit/nr/test_pusch_receiver.py).
A workgroup covers 256 output positions of one stream; ROW_CAP = 1024 rows ride blockIdx.z, more take further trips of the
grid-stride loop."""
import numpy as np
import pytest
import torch

import pusch_rx_f32 as spec
from pusch_rx_cases import CONFIGS, G, KINDS, LLR_CONFIGS, NO, bound, configs, estimator_of, grid_of, inside, specification

pytestmark = pytest.mark.gpu

ROW_CAP = 1024                                           # kPuschRxRowCap of csrc/pusch_rx.hip
PRECISIONS = [("single", np.float32, np.complex64), ("double", np.float64, np.complex128)]


def _dmrs(length=1, additional_position=0, config_type=1, cdm=1, **more):
    return dict(length=length, additional_position=additional_position, config_type=config_type, num_cdm_groups_without_data=cdm, **more)


# name -> one specification per transmitter.  12 subcarriers (below one wavefront) and 84 (no multiple of 64); runs of 2, 4
# and 6 pilots; DMRS length 1 and 2; additional position 0 and 3; an allocation that starts at symbol 2; 1 to 4 layers; two
# and three transmitters.
CASES = {
    "one_prb_one_layer": [{"pusch": {"n_size_bwp": 1}, "dmrs": _dmrs(cdm=1)}],
    "seven_prbs_two_layers_pairs": [{"pusch": {"n_size_bwp": 7, "num_layers": 2, "num_antenna_ports": 2}, "dmrs": _dmrs(2, 0, 1, 2)}],
    "late_start_three_layers": [{"pusch": {"n_size_bwp": 7, "num_layers": 3, "num_antenna_ports": 4, "precoding": "codebook", "tpmi": 1,
                                           "mapping_type": "B", "symbol_allocation": [2, 10]}, "dmrs": _dmrs(2, 1, 2, 3)}],
    "four_layers_four_dmrs_symbols": [{"pusch": {"n_size_bwp": 1, "num_layers": 4, "num_antenna_ports": 4}, "dmrs": _dmrs(1, 3, 1, 2)}],
    "two_transmitters": [{"pusch": {"n_size_bwp": 7, "num_layers": 2, "num_antenna_ports": 2}, "dmrs": _dmrs(1, 1, 2, 2, dmrs_port_set=ports)}
                         for ports in ([0, 2], [1, 3])],
    "three_transmitters": CONFIGS["three_tx"],
}


@pytest.fixture(scope="module")
def dev():
    from sionna_amd import _ffi
    _ffi.device()
    return _ffi


def received(shape, cd, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(cd)


def built(name, kind, prec="single", table=CASES):
    par, rg = grid_of(configs(table[name]), prec)
    return par, rg, estimator_of(par, rg, kind, prec)


def test_the_cases_take_the_paths_they_name(dev):
    seen = {k: set() for k in ("sc", "run", "length", "add", "start", "layers", "tx")}
    for name in CASES:
        pcs = configs(CASES[name])
        par, rg, est = built(name, "nn")
        seen["sc"].add(rg.fft_size), seen["run"].add(est._run), seen["length"].add(est._dmrs_length)
        seen["add"].add(par["dmrs_additional_position"]), seen["start"].add(pcs[0].symbol_allocation[0])
        seen["layers"].add(par["num_layers"]), seen["tx"].add(len(pcs))
        t = est._host_tables()
        assert (t["coef"] == 0).any() or est._run == 2                     # masked pilots of the other CDM ports
    assert seen["sc"] == {12, 84} and 84 % 64 and seen["run"] == {2, 4, 6} and seen["length"] == {1, 2}
    assert {0, 3} <= seen["add"] and seen["start"] == {0, 2} and seen["layers"] == {1, 2, 3, 4} and seen["tx"] == {1, 2, 3}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("prec,rd,cd", PRECISIONS)
def test_kernel_equals_the_specification(dev, name, prec, rd, cd):
    """random received grids, batch 3, 2 antennas; at the pilots (no interpolation) and with the nearest-neighbour table"""
    for nn, kind in ((False, None), (True, "nn")):
        par, rg, est = built(name, kind, prec)
        y = received((3, 1, 2, rg.num_ofdm_symbols, rg.fft_size), cd, len(name))
        h_hat, err_var = est(torch.from_numpy(y).cuda(), NO)
        ref = specification(est, y, nn, rd)
        assert h_hat.is_cuda and tuple(h_hat.shape) == ref.shape and h_hat.dtype == torch.from_numpy(ref).dtype
        assert np.array_equal(h_hat.cpu().numpy(), ref), (name, nn)
        assert (ref == 0).any() == (not nn and (est._host_tables()["coef"] == 0).any())


@pytest.mark.parametrize("prec,rd,cd", PRECISIONS)
def test_rows_none_one_and_past_one_grid_trip(dev, prec, rd, cd):
    par, rg, est = built("four_layers_four_dmrs_symbols", "nn", prec)
    empty, _ = est(torch.zeros((0, 1, 2, 14, 12), dtype=torch.from_numpy(np.zeros(1, cd)).dtype, device="cuda"), NO)
    assert tuple(empty.shape) == (0, 1, 2, 1, 4, 14, 12) and empty.is_cuda
    one = received((1, 1, 1, 14, 12), cd, 1)
    assert np.array_equal(est(torch.from_numpy(one).cuda(), NO)[0].cpu().numpy(), specification(est, one, True, rd))
    # past the cap the same lanes take a second trip: every row distinct, compared in full
    many = received((ROW_CAP + 37, 1, 1, 14, 12), cd, 2)
    assert np.array_equal(est(torch.from_numpy(many).cuda(), NO)[0].cpu().numpy(), specification(est, many, True, rd))


def test_a_view_of_the_received_grid(dev):
    par, rg, est = built("two_transmitters", "nn")
    wide = received((4, 1, 2, 14, 2 * 84 + 1), np.complex64, 3)
    view = torch.from_numpy(wide).cuda()[::2, :, :, :, 1::2]
    assert not view.is_contiguous() and view.shape[-1] == 84
    assert np.array_equal(est(view, NO)[0].cpu().numpy(), specification(est, wide[::2, :, :, :, 1::2], True))
    with pytest.raises(AssertionError):
        est(torch.from_numpy(wide).cuda(), NO)


@pytest.mark.parametrize("name", ["seven_prbs_two_layers_pairs", "one_prb_one_layer"])
def test_a_zero_sample_at_a_live_pilot_is_masked(dev, name):
    """cond = |h_hat| > 0 depends on the data: where the time-averaged estimate is exactly zero the output is zero, while the
    other pilots of the run still see the (changed) sum"""
    par, rg, est = built(name, None)
    t = est._host_tables()
    y = received((2, 1, 1, rg.num_ofdm_symbols, rg.fft_size), np.complex64, 4)
    p = int(np.flatnonzero(t["coef"][0] != 0)[2])
    res = [int(t["src"][0, p])]
    if est._dmrs_length == 2:                                               # both symbols of the pair, or the mean is not zero
        res.append(int(t["src"][0, p + est._num_pilots_per_dmrs_sym]))
    flat = y.reshape(2, -1)
    flat[0, res] = 0
    got = est(torch.from_numpy(y).cuda(), NO)[0].cpu().numpy()
    ref = specification(est, y, False)
    assert np.array_equal(got, ref)
    first = (p // est._run) * est._run
    run = got[0, 0, 0, 0, 0, first:first + est._run]
    assert run[p - first] == 0 and (run != 0).sum() == (t["coef"][0, first:first + est._run] != 0).sum() - 1
    assert got[1, 0, 0, 0, 0, p] != 0


@pytest.mark.parametrize("prec,rd,cd", PRECISIONS)
@pytest.mark.parametrize("shape", [(), (3,), (3, 1, 2)])
def test_error_variance_by_the_shape_of_no(dev, shape, prec, rd, cd):
    """the device forms one division no / (|pilot|^2 * 2 [* 2]); the specification halves after the division, which is the
    same number, so the two may differ by the rounding of the device's division only: one unit in the last place"""
    for kind in (None, "nn"):
        par, rg, est = built("late_start_three_layers", kind, prec)
        t = est._host_tables()
        no = (0.01 * (1 + np.arange(int(np.prod(shape, dtype=int))))).reshape(shape).astype(rd)
        y = received((3, 1, 2, rg.num_ofdm_symbols, rg.fft_size), cd, 5)
        _, err_var = est(torch.from_numpy(y).cuda(), torch.from_numpy(no).cuda() if shape else float(no))
        mask_shape = np.asarray(rg.pilot_pattern.mask).shape
        table = spec.error_variance(no.reshape(shape + (1,) * (3 - len(shape)) + (1, 1)), t["pilots"], est._dmrs_length, rd)
        if kind == "nn":
            table = np.take_along_axis(table, np.broadcast_to(t["gather"], table.shape[:-1] + t["gather"].shape[-1:]), axis=-1)
        ref = table.reshape(table.shape[:3] + (mask_shape if kind == "nn" else mask_shape[:2] + (-1,)))
        got = err_var.cpu().numpy()
        assert got.dtype == rd and got.shape == ref.shape and np.array_equal(got == 0, ref == 0)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= np.spacing(ref))


@pytest.fixture(scope="module")
def fixture_estimates(dev):
    """every fixture configuration through the estimator once per interpolation type, and at the pilots"""
    out = {}
    for name in CONFIGS:
        y = G[f"{name}/y"]
        for kind in KINDS:
            par, rg, est = built(name, kind, table=CONFIGS)
            h_hat, err_var = est(y, NO)
            assert h_hat.is_cuda and err_var.is_cuda
            out[name, kind] = (est, h_hat.cpu().numpy(), err_var.cpu().numpy())
        est = out[name, "nn"][0]
        t = est._host_tables()
        y_pilots = np.take(y.reshape(y.shape[:3] + (-1,)), t["src"], axis=-1).reshape(G[f"{name}/h_pilots"].shape)
        hp, evp = est.estimate_at_pilot_locations(y_pilots, G[f"{name}/no_batch"])
        out[name, "pilots"] = (est, hp.cpu().numpy(), evp.cpu().numpy())
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_estimator_against_the_reference(fixture_estimates, name):
    """nearest neighbour and at the pilots: inside the derived bound of pusch_rx_f32.error_bound.  Linear interpolation: the bar
    of the existing interpolation tests, 1e-5 of the peak, for the estimates and the error variances."""
    y = G[f"{name}/y"]
    est, h_hat, err_var = fixture_estimates[name, "nn"]
    worst, ok = inside(h_hat, G[f"{name}/h_hat_nn"], bound(est, y, True))
    print(f"{name}: nn max error / bound = {worst:.3f}")
    assert ok and h_hat.shape == G[f"{name}/h_hat_nn"].shape
    ref = G[f"{name}/err_var_nn"]
    assert np.all(np.abs(np.broadcast_to(err_var, ref.shape).astype(np.float64) - ref) <= np.spacing(ref))
    est, hp, evp = fixture_estimates[name, "pilots"]
    worst, ok = inside(hp, G[f"{name}/h_pilots"], bound(est, y, False))
    print(f"{name}: at the pilots max error / bound = {worst:.3f}")
    assert ok and np.array_equal(hp == 0, G[f"{name}/h_pilots"] == 0)
    ref = G[f"{name}/err_var_pilots"]
    assert np.all(np.abs(np.broadcast_to(evp, ref.shape).astype(np.float64) - ref) <= np.spacing(ref))
    for kind in ("lin", "lin_time_avg"):
        _, h_hat, err_var = fixture_estimates[name, kind]
        ref = G[f"{name}/h_hat_{kind}"]
        assert h_hat.shape == ref.shape and np.abs(h_hat - ref).max() <= 1e-5 * np.abs(ref).max(), kind
        ref = G[f"{name}/err_var_{kind}"]
        assert np.abs(np.broadcast_to(err_var, ref.shape) - ref).max() <= 1e-5 * np.abs(ref).max(), kind


def test_the_generic_estimator_fails_where_two_ports_share_a_cdm_group(dev):
    """the check that the fixture bites: LSChannelEstimator on the same grids misses the reference by far more than the bound"""
    from sionna_amd.phy.ofdm import LSChannelEstimator
    name = "nc2_len1_add2_type2_cdm1"
    par, rg, est = built(name, "nn", table=CONFIGS)
    plain = LSChannelEstimator(rg, "nn")(G[f"{name}/y"], NO)[0].cpu().numpy()
    assert not inside(plain, G[f"{name}/h_hat_nn"], bound(est, G[f"{name}/y"], True))[1]
    assert np.abs(plain - G[f"{name}/h_hat_nn"]).max() > 0.1


def test_a_custom_interpolator(dev):
    from sionna_amd.phy import nr
    from sionna_amd.phy.ofdm import NearestNeighborInterpolator
    name = "three_tx"
    par, rg = grid_of(configs(CONFIGS[name]))
    inner, seen = NearestNeighborInterpolator(rg.pilot_pattern), {}

    def interpolator(h_hat, err_var):
        seen["h"], seen["e"] = tuple(h_hat.shape), tuple(err_var.shape)
        assert h_hat.is_cuda and err_var.is_cuda
        return inner(h_hat, err_var)
    est = nr.PUSCHLSChannelEstimator(rg, par["dmrs_length"], par["dmrs_additional_position"], par["num_cdm_groups_without_data"],
                                     interpolation_type="lin", interpolator=interpolator)
    h_hat, err_var = est(G[f"{name}/y"], NO)
    assert seen["h"] == seen["e"] == G[f"{name}/h_pilots"].shape
    direct = estimator_of(par, rg, "nn")(G[f"{name}/y"], NO)
    assert torch.equal(h_hat, direct[0]) and torch.equal(err_var, torch.broadcast_to(direct[1], err_var.shape))


# ---- end to end: test/unit/nr/test_pusch_receiver.py, cases 01, 02, 03, 05, 06, 07
def _link(ports, layers, precoding, bwp=4, tpmi=None, tb=None, pusch=None, **dmrs):
    p = dict(pusch or {}, n_size_bwp=bwp, num_antenna_ports=ports, num_layers=layers, precoding=precoding)
    if tpmi is not None:
        p["tpmi"] = tpmi
    return {"pusch": p, "dmrs": dmrs, "tb": tb or {}}


def _two(first, second_ports):
    second = {"pusch": dict(first["pusch"]), "dmrs": dict(first["dmrs"], dmrs_port_set=second_ports), "tb": dict(first["tb"])}
    return [first, second]


_C06 = _link(4, 2, "codebook", tpmi=2, tb={"mcs_index": 10}, config_type=1, length=2, additional_position=1,
             num_cdm_groups_without_data=2, dmrs_port_set=[2, 3])
LINKS = {
    "01": ([_link(4, 2, "codebook", config_type=1, num_cdm_groups_without_data=1, dmrs_port_set=[0, 1])], "single"),
    "02": (_two(_link(4, 2, "codebook", config_type=2, num_cdm_groups_without_data=2, dmrs_port_set=[0, 2], additional_position=1), [1, 3]), "single"),
    "03": (_two(_link(2, 2, "non-codebook", config_type=2, num_cdm_groups_without_data=2, dmrs_port_set=[0, 2], additional_position=1), [1, 3]), "single"),
    "05": ([_link(1, 1, "non-codebook", bwp=1, tb={"mcs_index": 10}, pusch={"mapping_type": "B", "symbol_allocation": [5, 2]}, config_type=1,
                  additional_position=0, num_cdm_groups_without_data=2, dmrs_port_set=[0])], "single"),
    "06": (_two(_C06, [0, 1]), "single"),             # the reference sets [2, 3] on the first and leaves [0, 1] on the clone
    "07": (_two(_C06, [0, 1]), "double"),
}
# case 04 ("very large transport block") with n_size_bwp cut from 273 to 2: the smallest with more than one code block
LARGE = [_link(4, 4, "codebook", bwp=2, tb={"mcs_index": 26, "mcs_table": 2}, config_type=2, length=2, num_cdm_groups_without_data=1,
               dmrs_port_set=[0, 1, 6, 7], additional_position=0)]


def run_link(specs, channel_estimator, domain, precision="single", batch_size=16, num_rx_ant=8, **receiver):
    """run_test of test_pusch_receiver.py:15-76 -> (ber, outputs of the receiver, bits)"""
    from sionna_amd.phy import nr
    from sionna_amd.phy.channel import OFDMChannel, RayleighBlockFading, TimeChannel
    from sionna_amd.phy.utils import compute_ber
    pcs = configs(specs)
    l_min, l_max = -1, 3
    tx = nr.PUSCHTransmitter(pcs, output_domain=domain, precision=precision)
    rx = nr.PUSCHReceiver(tx, input_domain=domain, l_min=l_min, channel_estimator=channel_estimator, precision=precision, **receiver)
    rayleigh = RayleighBlockFading(num_rx=1, num_rx_ant=num_rx_ant, num_tx=len(pcs), num_tx_ant=pcs[0].num_antenna_ports, precision=precision)
    if domain == "freq":
        channel = OFDMChannel(rayleigh, tx.resource_grid, normalize_channel=True, return_channel=True, precision=precision)
    else:
        channel = TimeChannel(rayleigh, tx.resource_grid.bandwidth, tx.resource_grid.num_time_samples, l_min=l_min, l_max=l_max,
                              normalize_channel=True, return_channel=True, precision=precision)
    x, b = tx(batch_size)
    y, h = channel(x)
    out = rx(y, 0.001, h) if channel_estimator == "perfect" else rx(y, 0.001)
    b_hat = out[0] if isinstance(out, tuple) else out
    assert b_hat.is_cuda and tuple(b_hat.shape) == tuple(b.shape)
    return float(compute_ber(b, b_hat)), out, tx


@pytest.mark.parametrize("case", list(LINKS))
@pytest.mark.parametrize("domain", ["freq", "time"])
@pytest.mark.parametrize("csi", ["perfect", None])
def test_link_has_no_bit_errors(dev, case, domain, csi):
    """no = 0.001, 8 receive antennas, RayleighBlockFading, l_min, l_max = -1, 3, batch 16: BER exactly 0, the reference's own
    assertion"""
    specs, precision = LINKS[case]
    ber, out, tx = run_link(specs, csi, domain, precision)
    assert ber == 0.0


def test_large_transport_block_and_crc_status(dev):
    from sionna_amd.phy import nr
    smaller = [dict(LARGE[0], pusch=dict(LARGE[0]["pusch"], n_size_bwp=1))]
    assert nr.PUSCHTransmitter(configs(smaller))._tb_encoder.num_cbs == 1
    ber, (b_hat, status), tx = run_link(LARGE, None, "freq", batch_size=2, return_tb_crc_status=True)
    assert tx._tb_encoder.num_cbs > 1 and ber == 0.0
    assert status.dtype == torch.bool and tuple(status.shape) == (2, 1) and bool(status.all())


@pytest.mark.parametrize("domain,csi", [("freq", None), ("time", "perfect")])
def test_crc_status_is_true_on_these_links(dev, domain, csi):
    ber, (b_hat, status), tx = run_link(LINKS["02"][0], csi, domain, return_tb_crc_status=True)
    assert ber == 0.0 and tuple(status.shape) == (16, 2) and status.dtype == torch.bool and bool(status.all())


@pytest.mark.parametrize("name", LLR_CONFIGS)
def test_llrs_after_the_layer_demapper(dev, name):
    """the receiver's chain up to the transport-block decoder on the fixture's grids: default estimator ("lin"), default
    LinearDetector, LayerDemapper; LinearDetector's existing bar, max |err| <= 4e-5 max(1, max |ref|)"""
    from sionna_amd.phy import nr
    tx = nr.PUSCHTransmitter(configs(CONFIGS[name]))
    seen = {}

    def decoder(llr):
        seen["llr"] = llr
        return llr, None
    rx = nr.PUSCHReceiver(tx, tb_decoder=decoder)
    rx(G[f"{name}/y"], NO)
    got, ref = seen["llr"].cpu().numpy(), G[f"{name}/llr"]
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 4e-5 * max(1.0, float(np.abs(ref).max()))


def test_a_user_supplied_detector_and_stream_management(dev):
    from sionna_amd.phy.mimo import StreamManagement
    from sionna_amd.phy.ofdm import KBestDetector
    from sionna_amd.phy import nr
    specs = LINKS["03"][0]
    pcs = configs(specs)
    probe = nr.PUSCHTransmitter(pcs)
    sm = StreamManagement(np.ones([1, 2], bool), 2)
    det = KBestDetector("bit", 4, 16, probe.resource_grid, sm, "qam", probe._num_bits_per_symbol)
    ber, out, tx = run_link(specs, None, "freq", mimo_detector=det, stream_management=sm)
    assert ber == 0.0


def test_perfect_csi_effective_channel_against_the_reference(dev):
    """the recorded h W of the reference receiver's perfect-CSI branch, and time_to_ofdm_channel on the device"""
    from sionna_amd.phy import nr
    from sionna_amd.phy.channel import time_to_ofdm_channel
    import types
    name = "three_tx"
    tx = nr.PUSCHTransmitter(configs(CONFIGS[name]))
    seen = {}

    def detector(y, h_hat, err_var, no):
        seen["h"], seen["e"] = h_hat, err_var
        return torch.zeros((2, 3, 2, tx.resource_grid.num_data_symbols * int(tx._num_bits_per_symbol)), device="cuda")
    rx = nr.PUSCHReceiver(tx, channel_estimator="perfect", mimo_detector=detector, tb_decoder=lambda llr: (llr, None))
    h = G[f"{name}/h"]
    rx(G[f"{name}/y"], NO, np.broadcast_to(h[..., None, None], h.shape + (14, 12)))
    ref = np.broadcast_to(G[f"{name}/h_eff"], tuple(seen["h"].shape))
    assert seen["e"] == 0.0 and seen["h"].is_cuda and np.allclose(seen["h"].cpu().numpy(), ref, atol=1e-6)
    for j in (0, 1):
        fft, cp, nsym, l_min, l_max = (int(v) for v in G[f"t2f/{j}/params"])
        rg = types.SimpleNamespace(fft_size=fft, cyclic_prefix_length=cp, num_time_samples=(fft + cp) * nsym)
        got = time_to_ofdm_channel(torch.from_numpy(G[f"t2f/{j}/h_t"]).cuda(), rg, l_min)
        ref = G[f"t2f/{j}/h_f"]
        assert got.is_cuda and np.abs(got.cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
