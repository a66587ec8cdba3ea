#!/usr/bin/env python3
"""Time of the fused PUSCH DMRS least-squares launch (csrc/pusch_rx.hip) with HIP events: one slot size, 4 layers, DMRS
configuration type 1 with 2 CDM groups without data, length 2, one additional position, 273 PRBs (3276 subcarriers x 14
symbols), batch 16, 8 receive antennas, complex64.
  nn         PUSCHLSChannelEstimator(interpolation_type="nn"): one launch from the received grid to h_hat over the whole grid
  pilots     interpolation_type=None: one launch to the de-spread estimates at the pilots
  lin        interpolation_type="lin": the launch at the pilots, then the linear interpolator's launches
One JSON line: microseconds per call of each, the compulsory HBM bytes of the nn launch (the DMRS symbols of the received grid
read once, 8 B per stream and resource element written) and the fraction of 8 TB/s it reaches.  There is no earlier
implementation to compare with.  ``--out FILE`` also writes the line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8.0e12
BATCH, RX_ANT, PRBS, LAYERS = 16, 8, 273, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tools.signal_rate import timed
    from sionna_amd import _ffi
    from sionna_amd.phy import nr
    from sionna_amd.phy.ofdm import ResourceGrid
    _ffi.device()
    pc = nr.PUSCHConfig(n_size_bwp=PRBS, num_layers=LAYERS, num_antenna_ports=LAYERS)
    pc.dmrs.length, pc.dmrs.additional_position, pc.dmrs.num_cdm_groups_without_data = 2, 1, 2
    par = nr.check_pusch_configs([pc])
    rg = ResourceGrid(par["num_ofdm_symbols"], par["num_subcarriers"], par["subcarrier_spacing"], 1, LAYERS,
                      par["cyclic_prefix_length"], pilot_pattern=nr.PUSCHPilotPattern([pc]))
    est = {kind: nr.PUSCHLSChannelEstimator(rg, 2, 1, 2, interpolation_type=kind) for kind in ("nn", None, "lin")}
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.view_as_complex(torch.randn((BATCH, 1, RX_ANT, rg.num_ofdm_symbols, rg.fft_size, 2), device="cuda", generator=g))
    no = 0.01
    times = {str(kind): timed(lambda e=e: e(y, no), a.iters, a.warmup) for kind, e in est.items()}
    rows, dmrs_symbols = BATCH * RX_ANT, 4
    hbm = rows * 8 * (dmrs_symbols * rg.fft_size + LAYERS * rg.num_ofdm_symbols * rg.fft_size)
    rec = {"batch": BATCH, "rx_antennas": RX_ANT, "prbs": PRBS, "layers": LAYERS, "dmrs_length": 2, "run": 4,
           "nn_us": round(times["nn"] * 1e6, 1), "pilots_us": round(times["None"] * 1e6, 1), "lin_us": round(times["lin"] * 1e6, 1),
           "nn_hbm_bytes": hbm, "nn_fraction_of_8TBps": round(hbm / times["nn"] / PEAK_BYTES, 3)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
