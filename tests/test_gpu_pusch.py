"""The fused PUSCH grid kernel (csrc/pusch.hip) against its specification tests/pusch_f32.py, bit for bit, in complex64 and
complex128, and ``PUSCHTransmitter`` on the device against the shipped vectors and against its own separate blocks.
A workgroup covers 256 resource elements of one transmitter; BATCH_CAP = 1024 batch entries ride blockIdx.z, more take
further trips of the grid-stride loop."""
import json
import os

import numpy as np
import pytest
import torch

import pusch_f32 as spec

pytestmark = pytest.mark.gpu

BATCH_CAP = 1024
GOLD = os.path.join(os.path.dirname(__file__), "golden")
V = np.load(os.path.join(GOLD, "pusch_ref_vectors.npz"))
G = np.load(os.path.join(GOLD, "pusch_ref_golden.npz"))
IDS = [int(i) for i in V["ids"]]
PRECISIONS = [("single", np.float32), ("double", np.float64)]

QPSK, QAM256 = {"mcs_index": 3}, {"mcs_index": 22, "mcs_table": 2}
# name -> one specification per transmitter.  Between them: 12 subcarriers (below one wavefront) and 84 (no multiple of 64);
# 1, 2, 3 and 4 layers; 2 and 4 ports with codebook matrices that hold zeros (TPMI 0 / 1 / 3) and without codebook; DMRS
# length 1 and 2, configuration type 1 and 2, 1, 2 and 3 CDM groups without data (empty resource elements wherever a port
# leaves a masked subcarrier unused); an allocation that starts at symbol 2; QPSK, 16-QAM and 256-QAM; two transmitters
# with different DMRS ports, with and without codebook.
CASES = {
    "one_prb_qpsk": [{"pusch": {"n_size_bwp": 1}, "dmrs": {"num_cdm_groups_without_data": 1}, "tb": QPSK}],
    "four_layers_codebook_late_start": [{"pusch": {"n_size_bwp": 7, "num_layers": 4, "num_antenna_ports": 4, "precoding": "codebook",
                                                   "tpmi": 1, "mapping_type": "B", "symbol_allocation": [2, 10]},
                                         "dmrs": {"length": 2, "config_type": 2, "num_cdm_groups_without_data": 3,
                                                  "additional_position": 1}, "tb": QAM256}],
    "one_layer_two_ports": [{"pusch": {"n_size_bwp": 3, "num_antenna_ports": 2, "precoding": "codebook", "tpmi": 0}}],
    "two_layers_four_ports": [{"pusch": {"n_size_bwp": 2, "num_layers": 2, "num_antenna_ports": 4, "precoding": "codebook", "tpmi": 3},
                               "dmrs": {"config_type": 2, "additional_position": 1}, "tb": QAM256}],
    "three_layers_four_ports": [{"pusch": {"n_size_bwp": 1, "num_layers": 3, "num_antenna_ports": 4, "precoding": "codebook", "tpmi": 1},
                                 "dmrs": {"length": 2}, "tb": QPSK}],
    "four_layers_no_codebook": [{"pusch": {"n_size_bwp": 6, "num_layers": 4, "num_antenna_ports": 4}, "tb": QPSK}],
    "two_users_no_codebook": [{"pusch": {"n_size_bwp": 2, "num_layers": 2, "num_antenna_ports": 2, "n_rnti": 7},
                               "dmrs": {"dmrs_port_set": [0, 1]}},
                              {"pusch": {"n_size_bwp": 2, "num_layers": 2, "num_antenna_ports": 2, "n_rnti": 9},
                               "dmrs": {"dmrs_port_set": [2, 3]}}],
    "two_users_codebook": [{"pusch": {"n_size_bwp": 7, "num_antenna_ports": 4, "precoding": "codebook", "tpmi": 2},
                            "dmrs": {"dmrs_port_set": [0], "config_type": 2, "num_cdm_groups_without_data": 3}, "tb": QAM256},
                           {"pusch": {"n_size_bwp": 7, "num_antenna_ports": 4, "precoding": "codebook", "tpmi": 9},
                            "dmrs": {"dmrs_port_set": [4], "config_type": 2, "num_cdm_groups_without_data": 3}, "tb": QAM256}],
}


@pytest.fixture(scope="module")
def nr():
    from sionna_amd import _ffi
    from sionna_amd.phy import nr as module
    _ffi.device()
    return module


def configs(nr, specs):
    return [nr.PUSCHConfig(nr.CarrierConfig(**s.get("carrier", {})), nr.PUSCHDMRSConfig(**s.get("dmrs", {})),
                           nr.TBConfig(**s.get("tb", {})), **s.get("pusch", {})) for s in specs]


def from_shipped(nr, cfg):
    pc = nr.PUSCHConfig()
    pc.carrier.n_cell_id, pc.carrier.slot_number = cfg["carrier"]["n_cell_id"], cfg["carrier"]["slot_number"]
    p = cfg["pusch"]
    for k in ("n_size_bwp", "symbol_allocation", "n_rnti", "num_antenna_ports", "num_layers", "precoding"):
        setattr(pc, k, p[k])
    if pc.precoding == "codebook":
        pc.tpmi = p["tpmi"]
    for k in ("length", "config_type", "additional_position", "num_cdm_groups_without_data", "dmrs_port_set", "n_scid", "n_id"):
        setattr(pc.dmrs, k, p["dmrs"][k])
    pc.tb.mcs_index, pc.tb.mcs_table = p["tb"]["mcs_index"], p["tb"]["mcs_table"]
    return pc


def specification(tx, c, rd):
    t = tx._host_tables()
    x = spec.pusch_grid(c, t["points"], t["pilots"], t["data_pos"], t["pilot_pos"], t["w"], tx._num_layers, rd)
    rg = tx.resource_grid
    return x.reshape(x.shape[:3] + (rg.num_ofdm_symbols, rg.fft_size))


def test_the_cases_take_the_paths_they_name(nr):
    seen = {"sc": set(), "layers": set(), "ports": set(), "length": set(), "type": set(), "cdm": set(), "m": set(), "empty": 0, "zero_w": 0}
    for specs in CASES.values():
        tx = nr.PUSCHTransmitter(configs(nr, specs), return_bits=False)
        t, pc = tx._host_tables(), tx._pusch_configs[0]
        seen["sc"].add(pc.num_subcarriers), seen["layers"].add(pc.num_layers), seen["length"].add(pc.dmrs.length)
        seen["type"].add(pc.dmrs.config_type), seen["cdm"].add(pc.dmrs.num_cdm_groups_without_data), seen["m"].add(int(pc.tb.num_bits_per_symbol))
        if t["w"] is not None:
            seen["ports"].add(pc.num_antenna_ports)
            seen["zero_w"] += int((t["w"] == 0).any())
        masked = (t["data_pos"] < 0) & (t["pilot_pos"] >= 0)
        seen["empty"] += int((t["pilots"][np.nonzero(masked)[0], t["pilot_pos"][masked]] == 0).any())
        assert masked.any() and pc.symbol_allocation[0] in (0, 2)
    assert {12, 84} <= seen["sc"] and 84 % 64 and seen["layers"] == {1, 2, 3, 4} and {2, 4} <= seen["ports"]
    assert seen["length"] == {1, 2} and seen["type"] == {1, 2} and seen["cdm"] == {1, 2, 3} and {2, 8} <= seen["m"]
    assert seen["empty"] >= 4 and seen["zero_w"] >= 4


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("prec,rd", PRECISIONS)
def test_fused_kernel_equals_the_specification(nr, name, prec, rd):
    """random coded bits, batch 3; the whole slot including pilots and empty resource elements, bit for bit; the fused
    evaluation equals the four passes of the specification"""
    tx = nr.PUSCHTransmitter(configs(nr, CASES[name]), return_bits=False, precision=prec)
    rng = np.random.default_rng(len(name))
    c = rng.integers(0, 2, (3, len(CASES[name]), tx._num_coded_bits)).astype(np.float32)
    got = tx._grid(torch.from_numpy(c).cuda())
    ref = specification(tx, c, rd)
    assert got.is_cuda and got.dtype == torch.from_numpy(ref).dtype and tuple(got.shape) == ref.shape
    assert ref.shape[2] == tx._pusch_configs[0].num_antenna_ports
    assert np.array_equal(got.cpu().numpy(), ref)
    t = tx._host_tables()
    four = spec.separate_blocks(c, t["points"], t["pilots"], t["data_pos"], t["pilot_pos"], t["w"], tx._num_layers, rd)
    assert np.array_equal(four.reshape(ref.shape), ref)


@pytest.mark.parametrize("prec,rd", PRECISIONS)
def test_batch_none_one_and_past_one_grid_trip(nr, prec, rd):
    tx = nr.PUSCHTransmitter(configs(nr, CASES["one_layer_two_ports"]), return_bits=False, precision=prec)
    n = tx._num_coded_bits
    rng = np.random.default_rng(5)
    empty = tx._grid(torch.zeros(0, 1, n, device="cuda"))
    assert tuple(empty.shape) == (0, 1, 2, 14, 36) and empty.is_cuda
    one = rng.integers(0, 2, (1, 1, n)).astype(np.float32)
    assert np.array_equal(tx._grid(torch.from_numpy(one).cuda()).cpu().numpy(), specification(tx, one, rd))
    # past the cap the same lanes take a second trip: every batch entry distinct, compared in full
    batch = BATCH_CAP + 37
    many = rng.integers(0, 2, (batch, 1, n)).astype(np.float32)
    assert np.array_equal(tx._grid(torch.from_numpy(many).cuda()).cpu().numpy(), specification(tx, many, rd))


def test_a_view_and_an_odd_offset(nr):
    tx = nr.PUSCHTransmitter(configs(nr, CASES["two_users_no_codebook"]), return_bits=False)
    n = tx._num_coded_bits
    rng = np.random.default_rng(9)
    wide = rng.integers(0, 2, (4, 2, 2 * n + 1)).astype(np.float32)
    dev = torch.from_numpy(wide).cuda()
    view = dev[::2, :, 1::2]
    assert not view.is_contiguous() and view.shape[-1] == n
    assert np.array_equal(tx._grid(view).cpu().numpy(), specification(tx, wide[::2, :, 1::2], np.float32))
    flat = torch.from_numpy(np.concatenate([[0.], wide[:1, :, :n].reshape(-1)]).astype(np.float32)).cuda()
    shifted = flat[1:].reshape(1, 2, n)                            # contiguous, four bytes off the 8-byte grid
    assert shifted.is_contiguous() and shifted.data_ptr() % 8 == 4
    assert np.array_equal(tx._grid(shifted).cpu().numpy(), specification(tx, wide[:1, :, :n], np.float32))
    with pytest.raises(AssertionError):
        tx._grid(dev[:, :, :n - 2])


def test_the_entry_point_refuses_what_the_kernel_does_not_take(nr):
    from sionna_amd import _ffi
    tx = nr.PUSCHTransmitter(configs(nr, CASES["one_prb_qpsk"]), return_bits=False)
    tx._grid(torch.zeros(1, 1, tx._num_coded_bits, device="cuda"))
    d, lib = tx._dev, _ffi.lib()
    out = torch.zeros(1, 1, 8, 14, 12, dtype=torch.complex64, device="cuda")
    c = torch.zeros(1, 1, tx._num_coded_bits, device="cuda")

    def call(layers=1, ports=1, m=2, w=None):
        return lib.samd_pusch_grid_c64(_ffi.ptr(c), _ffi.ptr(d["points"]), _ffi.ptr(d["pilots"]), _ffi.ptr(d["data_pos"]),
                                       _ffi.ptr(d["pilot_pos"]), w, 1, 1, layers, ports, 168, tx.resource_grid.num_data_symbols,
                                       d["pilots"].shape[1], m, _ffi.ptr(out), _ffi.stream())
    assert call() == _ffi.OK
    assert call(layers=5, ports=5) == _ffi.ERR_INVALID and call(ports=2) == _ffi.ERR_INVALID      # no matrices: ports = layers
    assert call(m=3) == _ffi.ERR_INVALID and call(m=12) == _ffi.ERR_INVALID and call(ports=8, w=_ffi.ptr(out)) == _ffi.ERR_INVALID


@pytest.fixture(scope="module")
def shipped_on_device(nr):
    """every shipped case through PUSCHTransmitter once: (configuration, transmitter, bits, output on the host)"""
    cases = {}
    for i in IDS:
        pc = from_shipped(nr, json.loads(str(V[f"test_{i}/config"])))
        tx = nr.PUSCHTransmitter(pc, return_bits=False)
        b = np.unpackbits(V[f"test_{i}/bits"])[:int(V[f"test_{i}/num_bits"])].astype(np.float32).reshape(1, 1, -1)
        x = tx(b)
        assert x.is_cuda and x.dtype == torch.complex64
        cases[i] = (pc, tx, b, x.cpu().numpy())
    return cases


@pytest.mark.parametrize("i", IDS)
def test_transmitter_equals_the_shipped_vectors(nr, shipped_on_device, i):
    """the reference's criterion (np.allclose, test_pusch_transmitter.py:51-52) and the derived bound of pusch_f32.error_bound"""
    pc, tx, b, x = shipped_on_device[i]
    ref = V[f"test_{i}/grid"]
    got = np.squeeze(np.transpose(x[0, 0], [2, 1, 0]))
    assert got.shape == ref.shape and np.allclose(got, ref)
    c = tx._tb_encoder(b).cpu().numpy()
    tx64 = nr.PUSCHTransmitter(pc, return_bits=False, precision="double")
    t, t64 = tx._host_tables(), tx64._host_tables()
    bound = spec.error_bound(t64["points"], t64["pilots"], t["data_pos"], t["pilot_pos"], t64["w"], c, tx._num_layers)
    bound = np.squeeze(np.transpose(bound.reshape(x.shape)[0, 0], [2, 1, 0]))
    d = got.astype(np.complex128) - ref
    floor = np.maximum(bound, 1e-300)                              # an empty resource element: error and bound both zero
    print(f"case {i}: max error / bound = {max((np.abs(d.real) / floor).max(), (np.abs(d.imag) / floor).max()):.3f}")
    assert np.all(np.abs(d.real) <= bound) and np.all(np.abs(d.imag) <= bound)


@pytest.mark.parametrize("name", ["four_layers_codebook_late_start", "two_users_no_codebook", "two_users_codebook", "one_prb_qpsk"])
@pytest.mark.parametrize("prec,rd", PRECISIONS)
def test_transmitter_equals_its_separate_blocks(nr, name, prec, rd):
    """TBEncoder, Mapper, LayerMapper, ResourceGridMapper, PUSCHPrecoder run one after the other on the device"""
    from sionna_amd.phy.mapping import Mapper
    from sionna_amd.phy.ofdm import ResourceGridMapper
    pcs = configs(nr, CASES[name])
    tx = nr.PUSCHTransmitter(pcs, return_bits=False, precision=prec)
    par = nr.check_pusch_configs(pcs)
    rng = np.random.default_rng(3)
    b = torch.from_numpy(rng.integers(0, 2, (5, len(pcs), par["tb_size"])).astype(np.float32)).cuda()
    x = tx(b)
    enc = nr.TBEncoder(par["tb_size"], par["num_coded_bits"], par["target_coderate"], par["num_bits_per_symbol"], par["num_layers"],
                       par["n_rnti"], par["n_id"], precision=prec)
    y = ResourceGridMapper(tx.resource_grid, precision=prec)(
        nr.LayerMapper(par["num_layers"], precision=prec)(Mapper("qam", par["num_bits_per_symbol"], precision=prec)(enc(b))))
    if par["precoding"] == "codebook":
        y = nr.PUSCHPrecoder(par["precoding_matrices"], precision=prec)(y)
    assert y.is_cuda and x.dtype == y.dtype == (torch.complex64 if prec == "single" else torch.complex128)
    assert tuple(x.shape) == (5, len(pcs), par["num_antenna_ports"], par["num_ofdm_symbols"], par["num_subcarriers"])
    assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert np.array_equal(x.cpu().numpy(), specification(tx, enc(b).cpu().numpy(), rd))


@pytest.mark.parametrize("prec", ["single", "double"])
def test_time_domain_and_return_bits(nr, prec):
    from sionna_amd.phy.ofdm import OFDMModulator
    pcs = configs(nr, CASES["two_users_codebook"])
    freq = nr.PUSCHTransmitter(pcs, return_bits=True, precision=prec)
    x, b = freq(4)
    assert tuple(b.shape) == (4, 2, pcs[0].tb_size) and tuple(x.shape) == (4, 2, 4, 14, 84)
    assert set(np.unique(b.cpu().numpy())) <= {0, 1}
    again = nr.PUSCHTransmitter(pcs, return_bits=False, precision=prec)(b)          # the returned bits re-encode to the same grid
    assert torch.equal(again, x)
    time = nr.PUSCHTransmitter(pcs, return_bits=False, output_domain="time", precision=prec)
    xt = time(b)
    cp = int(freq.resource_grid.cyclic_prefix_length)
    assert cp == 7 and tuple(xt.shape) == (4, 2, 4, 14 * (84 + cp)) == (4, 2, 4, freq.resource_grid.num_time_samples)
    assert torch.equal(xt, OFDMModulator(cp, precision=prec)(x))
    assert freq.pilot_pattern is freq.resource_grid.pilot_pattern and freq.pilot_pattern.num_tx == 2


def test_two_users_against_the_reference_executed_blocks(nr):
    """tests/golden/pusch_ref_golden.npz: the reference's own Mapper, LayerMapper, ResourceGridMapper, PUSCHPrecoder and
    OFDMModulator on random coded bits; its matrix product and FFT order differ, so np.allclose (time: 1e-5 of the peak)"""
    from sionna_amd.phy.ofdm import OFDMModulator
    for name, specs in json.loads(str(G["two_user"])):
        pcs = configs(nr, specs)
        tx = nr.PUSCHTransmitter(pcs, return_bits=False)
        shape = tuple(G[f"tx/{name}/c_shape"])
        c = np.unpackbits(G[f"tx/{name}/c"])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
        x = tx._grid(torch.from_numpy(c).cuda())
        assert np.allclose(x.cpu().numpy(), G[f"tx/{name}/x_freq"]), name
        xt = OFDMModulator(int(tx.resource_grid.cyclic_prefix_length))(x).cpu().numpy()
        ref = G[f"tx/{name}/x_time"]
        assert xt.shape == ref.shape and np.abs(xt - ref).max() <= 1e-5 * np.abs(ref).max(), name


def test_show_and_a_host_tensor_is_refused(nr, capsys):
    tx = nr.PUSCHTransmitter(configs(nr, CASES["two_users_no_codebook"]))
    tx.show()
    text = capsys.readouterr().out
    assert "---- UE 0 ----" in text and "---- UE 1 ----" in text and text.count("PUSCH DMRS Configuration") == 2
    x, b = tx(2)
    assert x.is_cuda and b.is_cuda
    with pytest.raises(AssertionError):
        nr.PUSCHTransmitter(nr.PUSCHConfig(), output_domain="frequency")
    with pytest.raises(AssertionError):
        nr.PUSCHTransmitter(nr.PUSCHConfig(), return_bits=1)
