#!/usr/bin/env python3
"""Generates the fixtures of the NR PUSCH transmitter (``sionna_amd.phy.nr``):
  tests/golden/pusch_ref_vectors.npz    a selection of the known-answer vectors the reference SHIPS (test/unit/nr/
                                        pusch_test_configs/test_*.json + .npy: transport-block bits and the slot grid of an
                                        independent generator; reference_dmrs_{1,2}.npy; pusch_dmrs_precoded_*.npy), repacked
                                        without pickled objects: bits packed, grids complex128, configurations as JSON strings
  tests/golden/pusch_ref_golden.npz     outputs of the reference's OWN classes, executed here: every public property of
                                        PUSCHConfig, PUSCHDMRSConfig, TBConfig and CarrierConfig (nr/pusch_config.py :12-1010,
                                        pusch_dmrs_config.py :11-351, tb_config.py :9-409, carrier_config.py :8-277; plain
                                        NumPy on nr/utils.py :16-304, :473-805 under the stand-in tools/ref_exec) for the chosen
                                        configurations, the mask and pilots of PUSCHPilotPattern (pusch_pilot_pattern.py
                                        :12-94), LayerMapper / LayerDemapper (layer_mapping.py :11-291) for 1 to 8 layers, and
                                        the transmitter's passes after the transport-block encoder (pusch_transmitter.py
                                        :217-236: Mapper, LayerMapper, ResourceGridMapper, PUSCHPrecoder, OFDMModulator) on
                                        random coded bits for two-user configurations, frequency and time domain
  tests/golden/pusch_api_signatures.json  constructors, ``call`` signatures and public attributes, read with ast
Then ALL shipped configurations go once through the host path (the configuration objects of ``sionna_amd.phy.nr``, the
transport-block oracle oracle/nr_tb.py and the kernel's specification tests/pusch_f32.py) and the number that meet the
reference's criterion (np.allclose) is printed: the count COVERAGE.md quotes.
Run here (needs /root/reference); the fixtures travel."""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_TESTS = "/root/reference/test/unit/nr"
NUM_SHIPPED = 83
COVERED = ("num_layers", "num_antenna_ports", "precoding", "dmrs.length", "dmrs.config_type", "dmrs.additional_position",
           "dmrs.num_cdm_groups_without_data")
# configurations built by hand for the properties: what the shipped ones do not reach (mapping type B, a late start, extended
# cyclic prefix, type_a_position 3, every MCS table, n_scid 1, an explicit n_id of the transport block)
EXTRA = [
    {"pusch": {"mapping_type": "B", "symbol_allocation": [3, 9], "n_size_bwp": 3}, "dmrs": {"additional_position": 2}},
    {"pusch": {"mapping_type": "B", "symbol_allocation": [2, 10], "n_size_bwp": 2}, "dmrs": {"length": 2, "additional_position": 1,
                                                                                             "config_type": 2, "num_cdm_groups_without_data": 3}},
    {"carrier": {"subcarrier_spacing": 60, "cyclic_prefix": "extended", "slot_number": 7}, "pusch": {"symbol_allocation": [0, 12]},
     "dmrs": {"type_a_position": 3, "additional_position": 1}, "tb": {"mcs_table": 3, "mcs_index": 27}},
    {"carrier": {"subcarrier_spacing": 30, "n_size_grid": 7, "slot_number": 14, "n_cell_id": 1007},
     "pusch": {"num_layers": 2, "num_antenna_ports": 4, "precoding": "codebook", "tpmi": 17, "n_rnti": 65535},
     "dmrs": {"n_scid": 1, "n_id": [3, 40000], "dmrs_port_set": [1, 2]}, "tb": {"mcs_table": 2, "mcs_index": 27, "n_id": 1023}},
    {"pusch": {"symbol_allocation": [0, 4], "n_size_bwp": 1}, "dmrs": {"additional_position": 3}, "tb": {"mcs_table": 4, "mcs_index": 26}},
    {"pusch": {"num_layers": 3, "num_antenna_ports": 4, "precoding": "codebook", "tpmi": 6, "symbol_allocation": [0, 13]},
     "dmrs": {"additional_position": 3}, "tb": {"mcs_index": 0}},
]


def tensor_unpickling():
    """the shipped .npy hold the bits as a pickled TensorFlow tensor, which unpickles through
    ``tensorflow.python.framework.ops.convert_to_tensor(ndarray)``: give the stand-in that one name"""
    import types
    from tools.ref_exec.loader import reference
    reference()
    for name in ("tensorflow.python", "tensorflow.python.framework", "tensorflow.python.framework.ops"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].__path__ = []
    sys.modules["tensorflow.python.framework.ops"].convert_to_tensor = np.asarray


def shipped(i):
    tensor_unpickling()
    with open(f"{REF_TESTS}/pusch_test_configs/test_{i}.json") as f:
        cfg = json.load(f)
    b, grid = np.load(f"{REF_TESTS}/pusch_test_configs/test_{i}.npy", allow_pickle=True)
    return cfg, np.asarray(b), np.asarray(grid)


def flat(cfg):
    p = cfg["pusch"]
    return {"num_layers": p["num_layers"], "num_antenna_ports": p["num_antenna_ports"], "precoding": p["precoding"],
            **{"dmrs." + k: p["dmrs"][k] for k in ("length", "config_type", "additional_position", "num_cdm_groups_without_data")}}


def select():
    """the smallest shipped cases first, then greedily the smallest case that adds a value not seen yet"""
    sizes = {i: os.path.getsize(f"{REF_TESTS}/pusch_test_configs/test_{i}.npy") for i in range(NUM_SHIPPED)}
    values = {i: flat(shipped(i)[0]) for i in range(NUM_SHIPPED)}
    everything = {(k, v[k]) for v in values.values() for k in COVERED}
    order = sorted(sizes, key=lambda i: (sizes[i], i))
    chosen = [i for i in order if sizes[i] < 130000]
    seen = {(k, values[i][k]) for i in chosen for k in COVERED}
    for i in order:
        new = {(k, values[i][k]) for k in COVERED} - seen
        if new:
            chosen.append(i)
            seen |= new
    assert seen == everything, everything - seen
    return sorted(chosen), sorted(everything)


def apply_shipped(cls_pusch, cfg):
    """the reference's own way of turning a shipped JSON into a PUSCHConfig (test/unit/nr/test_pusch_transmitter.py:22-46)"""
    pc = cls_pusch()
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


def apply_extra(classes, spec):
    carrier, dmrs, tb, pusch = classes
    return pusch(carrier(**spec.get("carrier", {})), dmrs(**spec.get("dmrs", {})), tb(**spec.get("tb", {})), **spec.get("pusch", {}))


def public_properties(obj):
    names = [n for n in dir(type(obj)) if not n.startswith("_") and isinstance(getattr(type(obj), n), property)]
    return [n for n in names if n not in ("carrier", "dmrs", "tb")]


def record(out, prefix, obj):
    for name in public_properties(obj):
        v = getattr(obj, name)
        if v is None:
            v = "None"
        out[f"{prefix}/{name}"] = np.asarray(v)
        assert out[f"{prefix}/{name}"].dtype != object, (prefix, name)


def load_ref():
    from tools.ref_exec.loader import reference
    import types
    ref = reference()
    ref.load_utils()
    ref.load_signal()
    if "sionna.phy.nr" not in sys.modules:
        m = types.ModuleType("sionna.phy.nr")
        m.__path__, m.__package__ = [], "sionna.phy.nr"
        sys.modules["sionna.phy.nr"] = m
        sys.modules["sionna.phy"].nr = m
    nr = sys.modules["sionna.phy.nr"]
    mapping = ref.load("sionna.phy.mapping")
    ch = sys.modules["sionna.phy.channel"]
    if not hasattr(ch, "AWGN"):
        ch.AWGN = object                                     # nr/utils.py imports it for a class that is not used here
    ofdm = sys.modules["sionna.phy.ofdm"]
    pp = ref.load("sionna.phy.ofdm.pilot_pattern")
    rg = ref.load("sionna.phy.ofdm.resource_grid")
    mod = ref.load("sionna.phy.ofdm.modulator")
    ofdm.PilotPattern, ofdm.ResourceGrid, ofdm.ResourceGridMapper = pp.PilotPattern, rg.ResourceGrid, rg.ResourceGridMapper
    ofdm.OFDMModulator = mod.OFDMModulator
    for sub in ("utils", "config", "carrier_config", "pusch_dmrs_config", "tb_config", "pusch_config", "pusch_pilot_pattern",
                "layer_mapping", "pusch_precoder"):
        m = ref.load("sionna.phy.nr." + sub)
        for k, v in vars(m).items():
            if not k.startswith("_") and isinstance(v, type) or k in ("decode_mcs_index", "generate_prng_seq", "calculate_tb_size"):
                setattr(nr, k, v)
    nr.Mapper, nr.ResourceGrid, nr.ResourceGridMapper, nr.OFDMModulator = mapping.Mapper, rg.ResourceGrid, rg.ResourceGridMapper, mod.OFDMModulator
    return nr


def numpy1_products(nr):
    """The reference pins numpy < 2.0 (pyproject.toml), where a float32 scalar times a Python float is float64: the product
    ``target_coderate * tb_scaling * n_re * ...`` of PUSCHConfig.tb_size (pusch_config.py:846-847) is formed in float64.
    Under NumPy 2 it would stay in float32 until the int32 factor and round.  The reference's TBConfig is therefore asked
    for its code rate as the float64 of the same float32 value, which restores the arithmetic of the NumPy it supports and
    changes nothing else (the recorded ``target_coderate`` property is the unchanged float32)."""
    class TBConfig64(nr.TBConfig):
        wide = False

        @property
        def target_coderate(self):
            r = nr.TBConfig.target_coderate.fget(self)
            return np.float64(r) if TBConfig64.wide else r
    return TBConfig64


def signatures():
    from tools.gen_api_signatures import params
    table = {}
    wanted = {"config": ["Config"], "carrier_config": ["CarrierConfig"], "pusch_dmrs_config": ["PUSCHDMRSConfig"],
              "tb_config": ["TBConfig"], "pusch_config": ["PUSCHConfig", "check_pusch_configs"],
              "pusch_pilot_pattern": ["PUSCHPilotPattern"], "layer_mapping": ["LayerMapper", "LayerDemapper"],
              "pusch_precoder": ["PUSCHPrecoder"], "pusch_transmitter": ["PUSCHTransmitter"], "utils": ["decode_mcs_index"]}
    for rel, names in wanted.items():
        path = f"nr/{rel}.py"
        tree = ast.parse(open(os.path.join("/root/reference/src/sionna/phy", path)).read())
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and node.name in names:
                table["nr." + node.name] = {"kind": "function", "params": params(node), "file": path}
            if isinstance(node, ast.ClassDef) and node.name in names:
                entry = {"kind": "class", "public": [], "bases": [b.id for b in node.bases if isinstance(b, ast.Name)]}
                for item in node.body:
                    if not isinstance(item, ast.FunctionDef):
                        continue
                    if item.name in ("__init__", "call"):
                        entry[item.name] = params(item)
                    decos = [d.id if isinstance(d, ast.Name) else getattr(d, "attr", "") for d in item.decorator_list]
                    if not item.name.startswith("_") and item.name not in ("call", "build") and "setter" not in decos:
                        is_prop = "property" in decos
                        entry["public"].append([item.name, "property" if is_prop else "method", None if is_prop else params(item)])
                    if "setter" in decos:
                        entry.setdefault("settable", []).append(item.name)
                table["nr." + node.name] = dict(entry, file=path)
    return table


def host_grid(cfg, b):
    """a shipped configuration through the host path: [num_subcarriers, 14, ports] like the shipped grid"""
    import pusch_f32 as spec
    from oracle import nr_tb
    from sionna_amd.phy import nr as mine
    from sionna_amd.phy.mapping import qam
    from sionna_amd.phy.ofdm import ResourceGrid
    pc = apply_shipped(mine.PUSCHConfig, cfg)
    par = mine.check_pusch_configs([pc])
    enc = nr_tb.TBEncoder(par["tb_size"], par["num_coded_bits"], float(par["target_coderate"]), int(par["num_bits_per_symbol"]),
                          par["num_layers"], par["n_rnti"], par["n_id"])
    c = enc.encode(np.asarray(b, np.float32).reshape(1, 1, -1))
    pattern = mine.PUSCHPilotPattern([pc])
    rg = ResourceGrid(par["num_ofdm_symbols"], par["num_subcarriers"], par["subcarrier_spacing"], 1, par["num_layers"],
                      par["cyclic_prefix_length"], pilot_pattern=pattern)
    dp, pp = rg._positions()
    w = np.stack(par["precoding_matrices"]) if par["precoding"] == "codebook" else None
    x = spec.pusch_grid(c, qam(int(par["num_bits_per_symbol"])), pattern.pilots.reshape(dp.shape[0], -1), dp, pp, w, par["num_layers"])
    return x[0, 0].reshape(x.shape[2], par["num_ofdm_symbols"], par["num_subcarriers"]).transpose(2, 1, 0)


def main():
    chosen, everything = select()
    # ---- 1. the shipped vectors, repacked
    vec = {"ids": np.array(chosen), "covered": np.array(json.dumps(everything))}
    for i in chosen:
        cfg, b, grid = shipped(i)
        assert set(np.unique(b)) <= {0, 1}
        vec[f"test_{i}/config"] = np.array(json.dumps(cfg))
        vec[f"test_{i}/bits"], vec[f"test_{i}/num_bits"] = np.packbits(b.astype(np.uint8)), np.int64(b.size)
        vec[f"test_{i}/grid"] = np.asarray(grid, np.complex128)
    for n in (1, 2):
        vec[f"reference_dmrs_{n}"] = np.load(f"{REF_TESTS}/reference_dmrs_{n}.npy")
    for layers, ports in ((1, 2), (1, 4), (2, 2), (2, 4), (3, 4), (4, 4)):
        a = np.load(f"{REF_TESTS}/pusch_dmrs_precoded_{layers}_layer_{ports}_ports.npy", allow_pickle=True)
        vec[f"pusch_dmrs_precoded_{layers}_layer_{ports}_ports"] = np.stack([np.asarray(t, np.complex128) for t in a])
    path = os.path.join(GOLD, "pusch_ref_vectors.npz")
    np.savez_compressed(path, **vec)
    print("wrote", path, os.path.getsize(path), "bytes; shipped cases", chosen)

    # ---- 2. the reference's own classes, executed
    nr = load_ref()
    tb64 = numpy1_products(nr)
    out = {"shipped_ids": np.array(chosen), "extra": np.array(json.dumps(EXTRA))}
    configs = [(f"shipped_{i}", apply_shipped(lambda: nr.PUSCHConfig(tb_config=tb64()), shipped(i)[0])) for i in chosen]
    configs += [(f"extra_{j}", apply_extra((nr.CarrierConfig, nr.PUSCHDMRSConfig, tb64, nr.PUSCHConfig), s)) for j, s in enumerate(EXTRA)]
    for name, pc in configs:
        tb64.wide = False
        record(out, f"config/{name}/pusch", pc)
        record(out, f"config/{name}/dmrs", pc.dmrs)
        record(out, f"config/{name}/tb", pc.tb)
        record(out, f"config/{name}/carrier", pc.carrier)
        tb64.wide = True
        out[f"config/{name}/pusch/tb_size"] = np.asarray(pc.tb_size)
        tb64.wide = False
        pat = nr.PUSCHPilotPattern([pc])
        out[f"config/{name}/pattern_mask"], out[f"config/{name}/pattern_pilots"] = np.asarray(pat.mask), np.asarray(pat.pilots)
    out["config_names"] = np.array([n for n, _ in configs])
    rng = np.random.default_rng(20261020)
    # ---- layer mapping, 1 to 8 layers, symbols and LLRs
    for layers in range(1, 9):
        lm = nr.LayerMapper(num_layers=layers)
        n_per = 12
        if layers < 5:
            x = (rng.normal(size=(2, 3, n_per * layers)) + 1j * rng.normal(size=(2, 3, n_per * layers))).astype(np.complex64)
            y = np.asarray(lm(x))
            out[f"layer/{layers}/x"], out[f"layer/{layers}/y"] = x, y
        else:
            x0 = (rng.normal(size=(2, n_per * lm.num_layers0)) + 1j * rng.normal(size=(2, n_per * lm.num_layers0))).astype(np.complex64)
            x1 = (rng.normal(size=(2, n_per * lm.num_layers1)) + 1j * rng.normal(size=(2, n_per * lm.num_layers1))).astype(np.complex64)
            from tools.ref_exec import tf_numpy
            y = np.asarray(lm.call([x0.view(tf_numpy.Tensor), x1.view(tf_numpy.Tensor)]))
            out[f"layer/{layers}/x0"], out[f"layer/{layers}/x1"], out[f"layer/{layers}/y"] = x0, x1, y
        for m in (1, 4):
            llr = rng.normal(size=(2, layers, n_per * m)).astype(np.float32)
            z = nr.LayerDemapper(lm, num_bits_per_symbol=m)(llr)
            out[f"layer/{layers}/llr_m{m}"] = llr
            if layers < 5:
                out[f"layer/{layers}/demapped_m{m}"] = np.asarray(z)
            else:
                out[f"layer/{layers}/demapped0_m{m}"], out[f"layer/{layers}/demapped1_m{m}"] = np.asarray(z[0]), np.asarray(z[1])
    # ---- the transmitter's passes after the encoder, two users
    two_user = [
        ("nc_2layers", [{"pusch": {"num_layers": 2, "num_antenna_ports": 2, "n_size_bwp": 2}, "dmrs": {"dmrs_port_set": [0, 1]}},
                        {"pusch": {"num_layers": 2, "num_antenna_ports": 2, "n_size_bwp": 2}, "dmrs": {"dmrs_port_set": [2, 3]}}]),
        ("cb_2layers_4ports", [{"pusch": {"num_layers": 2, "num_antenna_ports": 4, "precoding": "codebook", "tpmi": 7, "n_size_bwp": 3},
                                "dmrs": {"dmrs_port_set": [0, 1], "additional_position": 1}, "tb": {"mcs_index": 20, "mcs_table": 2}},
                               {"pusch": {"num_layers": 2, "num_antenna_ports": 4, "precoding": "codebook", "tpmi": 20, "n_size_bwp": 3},
                                "dmrs": {"dmrs_port_set": [2, 3], "additional_position": 1}, "tb": {"mcs_index": 20, "mcs_table": 2}}]),
    ]
    out["two_user"] = np.array(json.dumps(two_user))
    for name, specs in two_user:
        pcs = [apply_extra((nr.CarrierConfig, nr.PUSCHDMRSConfig, nr.TBConfig, nr.PUSCHConfig), s) for s in specs]
        par = sys.modules["sionna.phy.nr.pusch_config"].check_pusch_configs(pcs)
        m, layers = int(par["num_bits_per_symbol"]), par["num_layers"]
        pattern = nr.PUSCHPilotPattern(pcs)
        rg = nr.ResourceGrid(num_ofdm_symbols=par["num_ofdm_symbols"], fft_size=par["num_subcarriers"],
                             subcarrier_spacing=par["subcarrier_spacing"], num_tx=2, num_streams_per_tx=layers,
                             cyclic_prefix_length=par["cyclic_prefix_length"], pilot_pattern=pattern)
        c = rng.integers(0, 2, (3, 2, par["num_coded_bits"])).astype(np.float32)
        x = nr.ResourceGridMapper(rg)(nr.LayerMapper(num_layers=layers)(nr.Mapper("qam", m)(c)))
        if par["precoding"] == "codebook":
            x = nr.PUSCHPrecoder(par["precoding_matrices"])(x)
        out[f"tx/{name}/c"], out[f"tx/{name}/x_freq"] = np.packbits(c.astype(np.uint8)), np.asarray(x)
        out[f"tx/{name}/c_shape"] = np.array(c.shape)
        out[f"tx/{name}/x_time"] = np.asarray(nr.OFDMModulator(par["cyclic_prefix_length"])(x))
    path = os.path.join(GOLD, "pusch_ref_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
    path = os.path.join(GOLD, "pusch_api_signatures.json")
    with open(path, "w") as f:
        json.dump({"_comment": "reference signatures of the PUSCH transmitter's files under nr/ by ast (tools/gen_pusch_ref_golden.py); "
                               "defaults as source text", "signatures": signatures()}, f, indent=1)
    print("wrote", path)

    # ---- 3. every shipped configuration through the host path
    good = 0
    for i in range(NUM_SHIPPED):
        cfg, b, grid = shipped(i)
        ok = bool(np.allclose(np.squeeze(host_grid(cfg, b)), grid))
        good += ok
        if not ok:
            print("shipped configuration", i, "does NOT match")
    print(f"{good} of {NUM_SHIPPED} shipped configurations match through the host path (np.allclose)")


if __name__ == "__main__":
    main()
