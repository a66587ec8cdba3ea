#!/usr/bin/env python3
"""Generates tests/golden/precoding_mu_ref_golden.npz by EXECUTING the reference's own ``rzf_precoder`` /
``cbf_precoding_matrix`` (mimo/precoding.py:12-244) and ``RZFPrecoder`` with its effective channel (ofdm/precoding.py:15-177)
under the NumPy stand-in for TensorFlow, for the multi-user cases the single-link fixture (precoding_ref_golden.npz) does
not cover:
  mu1  one transmitter with 8 antennas serving 2 receivers x 2 antennas (4 streams), guard carriers and a DC null,
       a per-resource-element alpha [B, TX, T, F];
  mu2  two transmitters with 4 antennas, each serving one of two 2-antenna receivers, both receivers hearing both
       transmitters: h_eff carries the non-intended (interference) entries; scalar alpha;
  cbf  cbf_precoding_matrix on [n, K, M] batches; plus rzf_precoder at one per-item alpha.
Run here (needs /root/reference); the fixture travels."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "precoding_mu_ref_golden.npz")


def cn(rng, shape):
    return ((rng.normal(size=shape) + 1j * rng.normal(size=shape)) / np.sqrt(2)).astype(np.complex64)


def main():
    from tools.gen_ofdm_rx_ref_golden import load
    from tools.ref_exec.loader import reference
    mp, mimo, ofdm, od, ce, eq = load()
    ref = reference()
    pm = ref.load("sionna.phy.mimo.precoding")
    for k, v in vars(pm).items():
        if not k.startswith("_"):
            setattr(mimo, k, v)
    po = ref.load("sionna.phy.ofdm.precoding")
    rng = np.random.default_rng(4242)
    out = {}

    def grid(num_tx, streams, fft, guards, dc):
        return ofdm.ResourceGrid(num_ofdm_symbols=4, fft_size=fft, subcarrier_spacing=15e3, num_tx=num_tx,
                                 num_streams_per_tx=streams, cyclic_prefix_length=4, num_guard_carriers=guards, dc_null=dc,
                                 pilot_pattern="kronecker", pilot_ofdm_symbol_indices=[1])

    # mu1: 1 tx (8 antennas) -> 2 receivers x 2 antennas, per-RE alpha
    rg = grid(1, 4, 26, [2, 3], True)
    sm = mimo.StreamManagement(np.array([[1], [1]]), 4)
    B = 3
    x, h = cn(rng, (B, 1, 4, 4, 26)), cn(rng, (B, 2, 2, 1, 8, 4, 26))
    alpha = (0.05 + 0.5 * rng.random((B, 1, 4, 26))).astype(np.float32)
    xp, heff = po.RZFPrecoder(rg, sm, return_effective_channel=True)(x, h, alpha=alpha)
    out.update({"mu1/x": x, "mu1/h": h, "mu1/alpha": alpha, "mu1/x_precoded": np.asarray(xp), "mu1/h_eff": np.asarray(heff),
                "mu1/rx_tx_association": np.array([[1], [1]], np.int32), "mu1/num_streams_per_tx": np.int32(4),
                "mu1/precoding_ind": np.asarray(sm.precoding_ind).astype(np.int32),
                "mu1/effective_subcarrier_ind": np.asarray(rg.effective_subcarrier_ind).astype(np.int32)})
    # mu2: 2 tx (4 antennas each), receiver i served by transmitter i, both receivers hear both
    rg = grid(2, 2, 21, [2, 2], True)
    assoc = np.array([[1, 0], [0, 1]])
    sm = mimo.StreamManagement(assoc, 2)
    x, h = cn(rng, (B, 2, 2, 4, 21)), cn(rng, (B, 2, 2, 2, 4, 4, 21))
    xp, heff = po.RZFPrecoder(rg, sm, return_effective_channel=True)(x, h, alpha=np.float32(0.1))
    out.update({"mu2/x": x, "mu2/h": h, "mu2/alpha": np.float32(0.1), "mu2/x_precoded": np.asarray(xp),
                "mu2/h_eff": np.asarray(heff), "mu2/rx_tx_association": assoc.astype(np.int32),
                "mu2/num_streams_per_tx": np.int32(2), "mu2/precoding_ind": np.asarray(sm.precoding_ind).astype(np.int32),
                "mu2/effective_subcarrier_ind": np.asarray(rg.effective_subcarrier_ind).astype(np.int32)})
    # conjugate beamforming and RZF at the matrix level
    for i, (K, M) in enumerate([(2, 4), (4, 8), (3, 5)]):
        h = cn(rng, (5, 2, K, M))
        out[f"cbf{i}/h"], out[f"cbf{i}/g"] = h, np.asarray(pm.cbf_precoding_matrix(h))
    h, x = cn(rng, (5, 2, 3, 6)), cn(rng, (5, 2, 3))
    al = (0.2 * rng.random((5, 2))).astype(np.float32)
    xp, g = pm.rzf_precoder(x, h, alpha=al, return_precoding_matrix=True)
    out.update({"rzf/h": h, "rzf/x": x, "rzf/alpha": al, "rzf/x_precoded": np.asarray(xp), "rzf/g": np.asarray(g)})
    for k, v in out.items():
        print(k, np.asarray(v).shape, np.asarray(v).dtype)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
