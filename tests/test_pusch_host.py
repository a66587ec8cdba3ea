"""The NR PUSCH transmitter's host side on the CPU (``sionna_amd.phy.nr``): the configuration objects against the
reference-executed fixture tests/golden/pusch_ref_golden.npz, the DMRS against the vectors the reference ships
(tests/golden/pusch_ref_vectors.npz, both by tools/gen_pusch_ref_golden.py), the layer mapping, the kernel's specification
tests/pusch_f32.py against the shipped slot grids, the refusals, the signatures.

Bars: every recorded property equal, floating-point arrays within one unit in the last place of the recorded dtype; the
DMRS and the slot grids under the reference's own criterion, np.allclose with its defaults (test/unit/nr/
test_pusch_config.py, test_pusch_transmitter.py); the slot grids also per real component within
pusch_f32.error_bound = (L + 3) 2^-24 sum_l |w_l| |x_l| + sum_l |w_l| |fl(c_l) - c_l| (derivation there)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import pusch_f32 as spec
from sionna_amd.phy import nr
from sionna_amd.phy.mapping import qam
from sionna_amd.phy.ofdm import ResourceGrid

ROOT = os.path.join(os.path.dirname(__file__), "..")
sys.path.insert(0, ROOT)
from oracle import nr_tb  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "pusch_ref_golden.npz"))
V = np.load(os.path.join(GOLD, "pusch_ref_vectors.npz"))
IDS = [int(i) for i in V["ids"]]
EXTRA = json.loads(str(G["extra"]))
NAMES = [str(n) for n in G["config_names"]]
COVERED = ("num_layers", "num_antenna_ports", "precoding", "dmrs.length", "dmrs.config_type", "dmrs.additional_position",
           "dmrs.num_cdm_groups_without_data")


def from_shipped(cfg):
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


def from_spec(s):
    return nr.PUSCHConfig(nr.CarrierConfig(**s.get("carrier", {})), nr.PUSCHDMRSConfig(**s.get("dmrs", {})),
                          nr.TBConfig(**s.get("tb", {})), **s.get("pusch", {}))


def config_of(name):
    kind, i = name.split("_")
    return from_shipped(json.loads(str(V[f"test_{i}/config"]))) if kind == "shipped" else from_spec(EXTRA[int(i)])


def same(got, ref, what):
    """equal; a floating-point array within one unit in the last place of the recorded dtype"""
    got = np.asarray("None" if got is None else got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.dtype.kind in "fc":
        assert got.dtype.kind == ref.dtype.kind, (what, got.dtype, ref.dtype)
        real = ref.real.dtype
        for a, b in ((got.real, ref.real), (got.imag, ref.imag)):
            a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
            ulp = np.spacing(np.abs(b).astype(real)).astype(np.float64)
            assert np.all(np.abs(a - b) <= ulp), (what, float(np.abs(a - b).max()))
    else:
        assert got.dtype.kind == ref.dtype.kind or {got.dtype.kind, ref.dtype.kind} <= {"i", "u"}, (what, got.dtype, ref.dtype)
        assert np.array_equal(got, ref), (what, got, ref)


def test_fixture_selection_covers_every_shipped_value_and_stays_small():
    everything = {tuple(e) for e in json.loads(str(V["covered"]))}
    seen = set()
    for i in IDS:
        p = json.loads(str(V[f"test_{i}/config"]))["pusch"]
        flat = {"num_layers": p["num_layers"], "num_antenna_ports": p["num_antenna_ports"], "precoding": p["precoding"],
                **{"dmrs." + k: p["dmrs"][k] for k in ("length", "config_type", "additional_position", "num_cdm_groups_without_data")}}
        seen |= {(k, flat[k]) for k in COVERED}
    assert seen == everything and {k for k, _ in everything} == set(COVERED)
    sizes = [os.path.getsize(os.path.join(GOLD, f)) for f in ("pusch_ref_vectors.npz", "pusch_ref_golden.npz", "pusch_api_signatures.json")]
    largest_before = os.path.getsize(os.path.join(GOLD, "ldpc_bp_ref_golden.npz"))
    assert sum(sizes) < 2 * 1024 * 1024 and max(sizes) <= largest_before and max(sizes) < 1024 * 1024
    for key in ["reference_dmrs_1", "reference_dmrs_2"] + [f"pusch_dmrs_precoded_{l}_layer_{p}_ports"
                                                            for l, p in ((1, 2), (1, 4), (2, 2), (2, 4), (3, 4), (4, 4))]:
        assert key in V.files
    assert all(V[k].dtype != object for k in V.files) and all(G[k].dtype != object for k in G.files)


@pytest.mark.parametrize("name", NAMES)
def test_config_properties_equal_the_reference(name):
    pc = config_of(name)
    checked = 0
    for part, obj in (("pusch", pc), ("dmrs", pc.dmrs), ("tb", pc.tb), ("carrier", pc.carrier)):
        prefix = f"config/{name}/{part}/"
        recorded = [k[len(prefix):] for k in G.files if k.startswith(prefix)]
        assert len(recorded) >= {"pusch": 29, "dmrs": 14, "tb": 8, "carrier": 17}[part], (part, recorded)
        for prop in recorded:
            assert isinstance(getattr(type(obj), prop), property), (part, prop)
            same(getattr(obj, prop), G[prefix + prop], f"{name} {part}.{prop}")
            checked += 1
    assert checked >= 68
    pattern = nr.PUSCHPilotPattern(pc)
    mask = G[f"config/{name}/pattern_mask"]                    # the reference's pattern keeps it as int32
    assert pattern.mask.dtype == bool and np.array_equal(pattern.mask, mask) and set(np.unique(mask)) <= {0, 1}
    ref = G[f"config/{name}/pattern_pilots"]
    same(pattern.pilots.astype(np.complex128), ref.astype(np.complex64).astype(np.complex128), "pilots")
    assert pattern.pilots.dtype == np.complex64 and pattern.num_pilot_symbols == ref.shape[-1]


def test_decode_mcs_index_against_the_shipped_configurations_and_its_refusals():
    for i in IDS:
        tb = json.loads(str(V[f"test_{i}/config"]))["pusch"]["tb"]
        m, r = nr.decode_mcs_index(tb["mcs_index"], tb["mcs_table"])
        assert m == tb["num_bits_per_symbol"] and r == np.float32(tb["target_code_rate"]) and r.dtype == np.float32
    m, r = nr.decode_mcs_index([0, 1, 5], [1, 2, 2], True, True, [True, False, True])
    assert list(m) == [1, 2, 1] and list(r) == [240 / 1024, 40 / 1024, 198 / 1024]
    assert nr.decode_mcs_index(27, 4, is_pusch=False, check_index_validity=False)[0] == -1
    for args in ((28, 2), (27, 4), (28, 1, True, True)):
        with pytest.raises(ValueError):
            nr.decode_mcs_index(*args)
    for args in ((29,), (-1,), (3, 5), (3, 0)):
        with pytest.raises(AssertionError):
            nr.decode_mcs_index(*args)


@pytest.mark.parametrize("which,n_size_grid", [(1, 1), (2, 4)])
def test_dmrs_grid_against_the_shipped_sequences(which, n_size_grid):
    """test/unit/nr/test_pusch_config.py:17-64: a type-2 double-symbol DMRS over cell identities, slots and ports"""
    ref = V[f"reference_dmrs_{which}"]
    pc = nr.PUSCHConfig()
    pc.carrier.n_size_grid = n_size_grid
    pc.dmrs.config_type, pc.dmrs.num_cdm_groups_without_data, pc.dmrs.additional_position, pc.dmrs.length = 2, 3, 1, 2
    pc.dmrs.n_id = [4, 4]
    cols = []
    for n_cell_id in (0, 1, 10, 24, 99, 1006):
        for slot_number in (0, 1, 5, 9):
            for port in (0, 3, 4, 9, 11):
                pc.carrier.n_cell_id, pc.carrier.slot_number, pc.dmrs.dmrs_port_set = n_cell_id, slot_number, [port]
                a = pc.dmrs_grid
                pilots = np.concatenate([a[0, :, 2], a[0, :, 3], a[0, :, 10], a[0, :, 11]])
                cols.append(pilots[np.where(pilots)] / np.sqrt(3))
    got = np.transpose(np.array(cols))
    assert got.shape == ref.shape == (16 * n_size_grid, 120)
    assert np.allclose(got, ref)


def test_precoded_dmrs_against_the_shipped_arrays():
    """test/unit/nr/test_pusch_config.py:169-228: every TPMI of every (layers, ports) table"""
    pc = nr.PUSCHConfig()
    pc.carrier.n_size_grid, pc.carrier.slot_number = 1, 1
    pc.dmrs.additional_position, pc.dmrs.config_type, pc.dmrs.num_cdm_groups_without_data, pc.dmrs.length = 0, 2, 3, 2
    pc.dmrs.n_id = [8, 8]
    pc.precoding = "codebook"
    checked = 0
    for layers, ports, num_tpmi in ((1, 2, 6), (1, 4, 28), (2, 2, 3), (2, 4, 22), (3, 4, 7), (4, 4, 5)):
        ref = V[f"pusch_dmrs_precoded_{layers}_layer_{ports}_ports"]
        assert len(ref) == num_tpmi
        pc.tpmi = 0
        pc.num_layers, pc.num_antenna_ports = layers, ports
        for tpmi in range(num_tpmi):
            pc.tpmi = tpmi
            assert pc.precoding_matrix.shape == (ports, layers)
            assert np.allclose(pc.dmrs_grid_precoded / np.sqrt(3), ref[tpmi]), (layers, ports, tpmi)
            checked += 1
    assert checked == 71
    pc.tpmi, pc.precoding = 0, "non-codebook"
    assert pc.dmrs_grid_precoded is None and pc.precoding_matrix is None


@pytest.mark.parametrize("layers", range(1, 9))
def test_layer_mapping_is_exact_and_inverts(layers):
    lm = nr.LayerMapper(num_layers=layers)
    assert lm.num_layers == layers and lm.num_codewords == (1 if layers < 5 else 2)
    ref = G[f"layer/{layers}/y"]
    if layers < 5:
        x = torch.from_numpy(G[f"layer/{layers}/x"])
        y = lm(x)
        assert (lm.num_layers0, lm.num_layers1) == (layers, 0)
        back = nr.LayerDemapper(lm)(y)
        assert torch.equal(back, x)
    else:
        x0, x1 = torch.from_numpy(G[f"layer/{layers}/x0"]), torch.from_numpy(G[f"layer/{layers}/x1"])
        y = lm([x0, x1])
        assert lm.num_layers0 + lm.num_layers1 == layers and 0 <= lm.num_layers1 - lm.num_layers0 <= 1
        back = nr.LayerDemapper(lm)(y)
        assert torch.equal(back[0], x0) and torch.equal(back[1], x1)
    assert not y.is_cuda and y.dtype == torch.complex64 and y.is_contiguous() and np.array_equal(y.numpy(), ref)
    assert np.array_equal(spec.layer_mapper(G[f"layer/{layers}/x"], layers), ref) if layers < 5 else True
    for m in (1, 4):
        llr = torch.from_numpy(G[f"layer/{layers}/llr_m{m}"])
        z = nr.LayerDemapper(lm, num_bits_per_symbol=m)(llr)
        if layers < 5:
            assert z.dtype == torch.float32 and np.array_equal(z.numpy(), G[f"layer/{layers}/demapped_m{m}"])
        else:
            assert np.array_equal(z[0].numpy(), G[f"layer/{layers}/demapped0_m{m}"])
            assert np.array_equal(z[1].numpy(), G[f"layer/{layers}/demapped1_m{m}"])
    if layers > 1:
        with pytest.raises(AssertionError):
            nr.LayerMapper(num_layers=layers)(torch.zeros(2, 7 * layers + 1, dtype=torch.complex64) if layers < 5 else torch.zeros(2, 8))
    with pytest.raises(AssertionError):
        nr.LayerDemapper(lm)(torch.zeros(2, layers + 1, 8))


def test_layer_mapper_refusals():
    for bad in (0, 9):
        with pytest.raises(AssertionError):
            nr.LayerMapper(num_layers=bad)
    with pytest.raises(AssertionError):
        nr.LayerMapper(verbose=1)
    with pytest.raises(AssertionError):
        nr.LayerDemapper("mapper")
    with pytest.raises(AssertionError):
        nr.LayerMapper(num_layers=5)([torch.zeros(2, 4), torch.zeros(2, 9)])           # 2 : 3 is 4 : 6
    with pytest.raises(AssertionError):
        nr.LayerDemapper(nr.LayerMapper(2), num_bits_per_symbol=4)(torch.zeros(2, 2, 6))


def host_tables(pcs, precision="single"):
    """what PUSCHTransmitter hands the fused launch, built without the transport-block encoder (no device)"""
    par = nr.check_pusch_configs(pcs)
    pattern = nr.PUSCHPilotPattern(pcs, precision=precision)
    rg = ResourceGrid(par["num_ofdm_symbols"], par["num_subcarriers"], par["subcarrier_spacing"], len(pcs), par["num_layers"],
                      par["cyclic_prefix_length"], pilot_pattern=pattern, precision=precision)
    dp, pp = rg._positions()
    w = np.stack(par["precoding_matrices"]) if par["precoding"] == "codebook" else None
    return par, rg, pattern.pilots.reshape(dp.shape[0], -1), dp, pp, w


@pytest.fixture(scope="module")
def shipped_cases():
    """per shipped case: the coded bits of the oracle's transport-block encoder and the tables, computed once"""
    cases = {}
    for i in IDS:
        pc = from_shipped(json.loads(str(V[f"test_{i}/config"])))
        par, rg, pilots, dp, pp, w = host_tables([pc])
        b = np.unpackbits(V[f"test_{i}/bits"])[:int(V[f"test_{i}/num_bits"])].astype(np.float32)
        assert len(b) == par["tb_size"] == pc.tb_size
        enc = nr_tb.TBEncoder(par["tb_size"], par["num_coded_bits"], float(par["target_coderate"]), int(par["num_bits_per_symbol"]),
                              par["num_layers"], par["n_rnti"], par["n_id"])
        cases[i] = (pc, par, enc.encode(b.reshape(1, 1, -1)), pilots, dp, pp, w)
    return cases


def as_shipped(x, par):
    """[1, 1, ports, symbols, subcarriers] -> [subcarriers, symbols, ports] squeezed (test_pusch_transmitter.py:51-52)"""
    return np.squeeze(np.transpose(x[0, 0], [2, 1, 0]))


@pytest.mark.parametrize("i", IDS)
def test_specification_against_the_shipped_grids(shipped_cases, i):
    pc, par, c, pilots, dp, pp, w = shipped_cases[i]
    m, layers = int(par["num_bits_per_symbol"]), par["num_layers"]
    got = spec.pusch_grid(c, qam(m), pilots, dp, pp, w, layers)
    ports = par["num_antenna_ports"]
    assert got.dtype == np.complex64 and got.shape == (1, 1, ports, par["num_ofdm_symbols"] * par["num_subcarriers"])
    assert np.array_equal(got, spec.separate_blocks(c, qam(m), pilots, dp, pp, w, layers))
    got = got.reshape(1, 1, ports, par["num_ofdm_symbols"], par["num_subcarriers"])
    ref = V[f"test_{i}/grid"]
    assert np.allclose(as_shipped(got, par), ref)                               # the reference's criterion
    par64, _, pilots64, _, _, w64 = host_tables([pc], "double")
    bound = spec.error_bound(qam(m, precision="double"), pilots64, dp, pp, w64, c, layers)
    bound = as_shipped(bound.reshape(got.shape), par)
    d = as_shipped(got, par).astype(np.complex128) - ref
    worst = max((np.abs(d.real) / np.maximum(bound, 1e-300)).max(), (np.abs(d.imag) / np.maximum(bound, 1e-300)).max())
    print(f"case {i}: max error / bound = {worst:.3f}, max error {np.abs(d).max():.3e}")
    assert np.all(np.abs(d.real) <= bound) and np.all(np.abs(d.imag) <= bound)


def test_specification_in_float64_and_two_users_against_the_reference_blocks():
    """the reference's Mapper, LayerMapper, ResourceGridMapper, PUSCHPrecoder executed on random coded bits (two users with
    different DMRS ports): complex64, so equal up to the reference's own matmul order - np.allclose; the host PUSCHPrecoder
    equals the specification bit for bit"""
    for name, specs in json.loads(str(G["two_user"])):
        pcs = [from_spec(s) for s in specs]
        par, rg, pilots, dp, pp, w = host_tables(pcs)
        shape = tuple(G[f"tx/{name}/c_shape"])
        c = np.unpackbits(G[f"tx/{name}/c"])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
        m, layers = int(par["num_bits_per_symbol"]), par["num_layers"]
        got = spec.pusch_grid(c, qam(m), pilots, dp, pp, w, layers)
        ref = G[f"tx/{name}/x_freq"]
        assert np.allclose(got.reshape(ref.shape), ref), name
        got64 = spec.pusch_grid(c, qam(m, precision="double"), host_tables(pcs, "double")[2], dp, pp, w, layers, np.float64)
        assert got64.dtype == np.complex128 and np.abs(got64 - got).max() < 1e-6
        if w is not None:
            layer_grid = spec.pusch_grid(c, qam(m), pilots, dp, pp, None, layers).reshape(shape[0], 2, layers, rg.num_ofdm_symbols, -1)
            y = nr.PUSCHPrecoder(par["precoding_matrices"])(torch.from_numpy(layer_grid))
            assert not y.is_cuda and np.array_equal(y.numpy().reshape(got.shape), got)


REFUSED = [
    ("carrier", {"n_cell_id": 1008}), ("carrier", {"cyclic_prefix": "long"}), ("carrier", {"subcarrier_spacing": 45}),
    ("carrier", {"n_size_grid": 276}), ("carrier", {"n_start_grid": 2200}), ("carrier", {"slot_number": 10}),
    ("carrier", {"frame_number": 1024}), ("carrier", {"cyclic_prefix": "extended"}),
    ("dmrs", {"config_type": 3}), ("dmrs", {"type_a_position": 1}), ("dmrs", {"additional_position": 4}), ("dmrs", {"length": 3}),
    ("dmrs", {"n_id": 65536}), ("dmrs", {"n_id": [1, 2, 3]}), ("dmrs", {"n_scid": 2}), ("dmrs", {"num_cdm_groups_without_data": 4}),
    ("dmrs", {"length": 2, "additional_position": 2}), ("dmrs", {"dmrs_port_set": [4]}),
    ("dmrs", {"num_cdm_groups_without_data": 1, "dmrs_port_set": [2]}), ("dmrs", {"config_type": 1, "num_cdm_groups_without_data": 3}),
    ("tb", {"mcs_index": 29}), ("tb", {"mcs_table": 5}), ("tb", {"channel_type": "PUCCH"}), ("tb", {"n_id": 1024}),
    ("pusch", {"n_size_bwp": 0}), ("pusch", {"n_start_bwp": 2474}), ("pusch", {"num_layers": 5}), ("pusch", {"num_antenna_ports": 3}),
    ("pusch", {"mapping_type": "C"}), ("pusch", {"symbol_allocation": [0, 14, 1]}), ("pusch", {"n_rnti": 65536}),
    ("pusch", {"precoding": "svd"}), ("pusch", {"transform_precoding": 1}), ("pusch", {"tpmi": 28}),
    ("pusch", {"num_layers": 2}),                                                          # non-codebook: ports must equal layers
    ("pusch", {"precoding": "codebook"}),                                                  # one antenna port
    ("pusch", {"precoding": "codebook", "num_layers": 4, "num_antenna_ports": 2}),
    ("pusch", {"precoding": "codebook", "num_antenna_ports": 2, "tpmi": 6}),
    ("pusch", {"precoding": "codebook", "num_antenna_ports": 2, "num_layers": 2, "tpmi": 3}),
    ("pusch", {"precoding": "codebook", "num_antenna_ports": 4, "num_layers": 2, "tpmi": 22}),
    ("pusch", {"precoding": "codebook", "num_antenna_ports": 4, "num_layers": 3, "tpmi": 7}),
    ("pusch", {"precoding": "codebook", "num_antenna_ports": 4, "num_layers": 4, "tpmi": 5}),
    ("pusch", {"symbol_allocation": [0, 3]}), ("pusch", {"symbol_allocation": [1, 10]}), ("pusch", {"symbol_allocation": [0, 15]}),
    ("pusch", {"mapping_type": "B", "symbol_allocation": [14, 1]}), ("pusch", {"mapping_type": "B", "symbol_allocation": [5, 10]}),
    ("pusch", {"mapping_type": "B", "symbol_allocation": [0, 0]}),
]


@pytest.mark.parametrize("part,settings", REFUSED, ids=[f"{p}-{'-'.join(f'{k}={v}' for k, v in s.items())}" for p, s in REFUSED])
def test_refused_settings_raise(part, settings):
    cls = {"carrier": nr.CarrierConfig, "dmrs": nr.PUSCHDMRSConfig, "tb": nr.TBConfig, "pusch": nr.PUSCHConfig}[part]
    with pytest.raises(AssertionError):
        cls(**settings)


def test_refusals_that_need_two_objects():
    with pytest.raises(AssertionError):                        # double-symbol DMRS, mapping type B, four symbols
        nr.PUSCHConfig(pusch_dmrs_config=nr.PUSCHDMRSConfig(length=2), mapping_type="B", symbol_allocation=[0, 4])
    with pytest.raises(AssertionError):
        nr.PUSCHConfig(pusch_dmrs_config=nr.PUSCHDMRSConfig(additional_position=3, type_a_position=3))
    with pytest.raises(AssertionError):                        # as many DMRS ports as layers
        nr.PUSCHConfig(pusch_dmrs_config=nr.PUSCHDMRSConfig(dmrs_port_set=[0, 1]))
    with pytest.raises(AssertionError):
        nr.PUSCHConfig(tb_config=nr.TBConfig(channel_type="PDSCH"))
    with pytest.raises(AssertionError):
        nr.PUSCHConfig(carrier_config="carrier")
    with pytest.raises(AssertionError):
        nr.PUSCHConfig(nr.CarrierConfig(subcarrier_spacing=60, cyclic_prefix="extended"), symbol_allocation=[0, 13])
    with pytest.raises(ValueError):
        nr.PUSCHDMRSConfig(dmrs_port_set=1.5)
    pc = nr.PUSCHConfig()
    pc.dmrs.length = 2
    pc.dmrs.additional_position = 1
    pc.symbol_allocation = [0, 14]
    assert pc.check_config()
    pc.dmrs._additional_position = 2                            # past the setter's own check
    with pytest.raises(AssertionError):
        pc.check_config()
    with pytest.raises(AssertionError):
        nr.check_pusch_configs(pc)
    with pytest.raises(AssertionError):
        nr.check_pusch_configs(["config"])
    a, b = nr.PUSCHConfig(), nr.PUSCHConfig(num_layers=2, num_antenna_ports=2)
    with pytest.raises(AssertionError):
        nr.PUSCHPilotPattern([a, b])
    with pytest.raises(AssertionError):
        nr.PUSCHPilotPattern([a, nr.PUSCHConfig(n_size_bwp=5)])
    with pytest.raises(AssertionError):
        nr.PUSCHPilotPattern([a, nr.PUSCHConfig(mapping_type="B", symbol_allocation=[0, 10])])
    with pytest.raises(ValueError):
        nr.PUSCHPilotPattern(3)
    with pytest.warns(UserWarning, match="DMRS port 0 used by multiple transmitters"):
        nr.PUSCHPilotPattern([nr.PUSCHConfig(pusch_dmrs_config=nr.PUSCHDMRSConfig(dmrs_port_set=[0])),
                              nr.PUSCHConfig(pusch_dmrs_config=nr.PUSCHDMRSConfig(dmrs_port_set=[0]))])
    with pytest.raises(AssertionError):
        nr.PUSCHPrecoder([np.ones((2, 1)), np.ones((4, 1))])
    with pytest.raises(AssertionError):
        nr.PUSCHPrecoder([np.ones((2, 1), complex)])(torch.zeros(1, 2, 1, 14, 12, dtype=torch.complex64))
    with pytest.raises(AssertionError):
        nr.PUSCHPrecoder([np.ones((2, 1), complex)])(torch.zeros(1, 1, 2, 14, 12, dtype=torch.complex64))


def test_clone_show_and_defaults(capsys):
    pc = nr.PUSCHConfig(mapping_type="B")
    pc.dmrs.config_type = 2
    pc.carrier.subcarrier_spacing = 30
    deep, shallow = pc.clone(), pc.clone(deep=False)
    deep.dmrs.config_type = 1
    assert pc.dmrs.config_type == 2 and shallow.dmrs is pc.dmrs and deep.carrier.subcarrier_spacing == 30
    pc.show()
    text = capsys.readouterr().out
    for title in ("Carrier Configuration", "PUSCH Configuration", "PUSCH DMRS Configuration", "Transport Block Configuration"):
        assert title in text and "=" * len(title) in text
    assert "dmrs_grid : shape (1, 48, 14)" in text and "mapping_type : B" in text and "show :" not in text
    d = nr.PUSCHConfig()
    assert (d.num_coded_bits, d.tb_size, d.num_resource_blocks, d.dmrs_symbol_indices, d.tb.mcs_index) == (2496, 1352, 4, [2], 14)
    assert nr.PUSCHConfig(unknown_keyword=3).num_layers == 1 and isinstance(d, nr.Config)


def test_signatures_match_the_reference():
    from test_api_signatures import _check
    with open(os.path.join(GOLD, "pusch_api_signatures.json")) as f:
        table = json.load(f)["signatures"]
    assert len(table) == 12
    for name, ref in table.items():
        obj = getattr(nr, name.split(".")[1])
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
        for attr in ref.get("settable", []):
            assert getattr(obj, attr).fset is not None, f"{name}.{attr} has no setter"
        assert [b.__name__ for b in obj.__mro__ if b.__name__ in ref["bases"]] or not ref["bases"] or ref["bases"] == ["Block"], name


def test_import_path_under_install_as_sionna():
    import sionna_amd
    sionna_amd.install_as_sionna()
    from sionna.phy.nr import PUSCHConfig, PUSCHTransmitter, LayerMapper, decode_mcs_index
    assert PUSCHConfig is nr.PUSCHConfig and PUSCHTransmitter is nr.PUSCHTransmitter and LayerMapper is nr.LayerMapper
    assert decode_mcs_index is nr.decode_mcs_index
