#!/usr/bin/env python3
"""Rate of RZFPrecoder(return_effective_channel=True) (csrc/precoding.hip) with HIP events: the notebook's downlink shape
(MIMO_OFDM_Transmissions_over_CDL.ipynb: 8 transmit antennas, 4 streams to one 4-antenna receiver, 14 x 72 grid, guards
[5, 6], DC null) at B = 2048, and a multi-user shape (16 transmit antennas serving 4 receivers x 2 antennas, K = 8).
Prints one line per shape: microseconds per call, compulsory bytes (h and x read once, x_precoded and h_eff written once)
and the fraction of the 8 TB/s HBM peak they represent."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


def measure(B, num_rx, num_rx_ant, num_tx_ant, iters, warmup):
    import numpy as np
    import torch
    import sionna_amd.phy as phy
    streams = num_rx * num_rx_ant
    rg = phy.ofdm.ResourceGrid(num_ofdm_symbols=14, fft_size=72, subcarrier_spacing=15e3, num_tx=1, num_streams_per_tx=streams,
                               cyclic_prefix_length=6, num_guard_carriers=[5, 6], dc_null=True, pilot_pattern=None)
    sm = phy.mimo.StreamManagement(np.ones((num_rx, 1), int), streams)
    pre = phy.ofdm.RZFPrecoder(rg, sm, return_effective_channel=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((B, 1, streams, 14, 72), dtype=torch.complex64, device="cuda", generator=g)
    h = torch.randn((B, num_rx, num_rx_ant, 1, num_tx_ant, 14, 72), dtype=torch.complex64, device="cuda", generator=g)
    for _ in range(warmup):
        pre(x, h)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        xp, he = pre(x, h)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / iters
    nbytes = 8 * (h.numel() + x.numel() + xp.numel() + he.numel())
    return {"shape": f"B={B} rx={num_rx}x{num_rx_ant} tx_ant={num_tx_ant} K={streams} 14x72", "us": round(us, 1),
            "compulsory_bytes": int(nbytes), "bytes_per_re": round(nbytes / (B * 14 * 72), 1),
            "tb_per_s": round(nbytes / us * 1e-6, 3), "fraction_of_8tbs": round(nbytes / us * 1e6 / PEAK, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for shape in ((2048, 1, 4, 8), (512, 4, 2, 16)):
        print(json.dumps(measure(*shape, a.iters, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
