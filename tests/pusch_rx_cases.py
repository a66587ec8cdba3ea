"""What the host and the device tests of the PUSCH receiver share: the fixture tests/golden/pusch_rx_ref_golden.npz
(tools/gen_pusch_rx_ref_golden.py) and the way from a recorded configuration to a resource grid and an estimator."""
import json
import os

import numpy as np

import pusch_rx_f32 as spec

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "pusch_rx_ref_golden.npz"))
CONFIGS = json.loads(str(G["configs"]))
LLR_CONFIGS = json.loads(str(G["llr_configs"]))
NO = float(G["no"])
KINDS = ("nn", "lin", "lin_time_avg")


def configs(specs):
    from sionna_amd.phy import nr
    return [nr.PUSCHConfig(nr.CarrierConfig(**s.get("carrier", {})), nr.PUSCHDMRSConfig(**s.get("dmrs", {})),
                           nr.TBConfig(**s.get("tb", {})), **s.get("pusch", {})) for s in specs]


def grid_of(pcs, precision="single"):
    """parameters and the resource grid with the DMRS pilot pattern, built on the host (no transport-block encoder)"""
    from sionna_amd.phy import nr
    from sionna_amd.phy.ofdm import ResourceGrid
    par = nr.check_pusch_configs(pcs)
    pattern = nr.PUSCHPilotPattern(pcs, precision=precision)
    rg = ResourceGrid(par["num_ofdm_symbols"], par["num_subcarriers"], par["subcarrier_spacing"], len(pcs), par["num_layers"],
                      par["cyclic_prefix_length"], pilot_pattern=pattern, precision=precision)
    return par, rg


def estimator_of(par, rg, kind="nn", precision="single", **kwargs):
    from sionna_amd.phy import nr
    return nr.PUSCHLSChannelEstimator(rg, par["dmrs_length"], par["dmrs_additional_position"], par["num_cdm_groups_without_data"],
                                      interpolation_type=kind, precision=precision, **kwargs)


def specification(est, y, nn, dtype=np.float32):
    """the estimator's own tables through the specification: y [batch, num_rx, num_rx_ant, T, fft_size] -> the estimates at the
    pilots [batch, num_rx, num_rx_ant, num_tx, S, num_pilots], or over the grid with the nearest-neighbour table"""
    t = est._host_tables()
    y = np.asarray(y)
    out = spec.pusch_ls(y.reshape(-1, y.shape[-2] * y.shape[-1]), t["src"], t["coef"], est._num_pilots_per_dmrs_sym, est._run,
                        est._dmrs_length, t["gather"] if nn else None, dtype)
    mask = np.asarray(est._pilot_pattern.mask)
    return out.reshape(y.shape[:3] + (mask.shape if nn else mask.shape[:2] + (-1,)))


def bound(est, y, nn, unit=2.0 ** -24):
    t = est._host_tables()
    y = np.asarray(y)
    b = spec.error_bound(y.reshape(-1, y.shape[-2] * y.shape[-1]), t["src"], t["pilots"], est._num_pilots_per_dmrs_sym, est._run,
                         est._dmrs_length, t["gather"] if nn else None, unit)
    mask = np.asarray(est._pilot_pattern.mask)
    return b.reshape(y.shape[:3] + (mask.shape if nn else mask.shape[:2] + (-1,)))


def inside(got, ref, b):
    d = np.asarray(got).astype(np.complex128) - np.asarray(ref).astype(np.complex128)
    floor = np.maximum(b, 1e-300)
    worst = max(float((np.abs(d.real) / floor).max()), float((np.abs(d.imag) / floor).max()))
    return worst, bool(np.all(np.abs(d.real) <= b) and np.all(np.abs(d.imag) <= b))
