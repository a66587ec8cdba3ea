#!/usr/bin/env python3
"""Time of the fused PUSCH grid launch (csrc/pusch.hip) against the separate blocks it replaces, with HIP events: one slot
size, 4 layers, 4 antenna ports, codebook TPMI 3, 273 PRBs (3276 subcarriers x 14 symbols), 256-QAM, batch 64, complex64.
Both start from the same scrambled coded bits on the device:
  fused      PUSCHTransmitter._grid: one launch
  separate   Mapper, LayerMapper, ResourceGridMapper, PUSCHPrecoder one after the other
One JSON line: microseconds per call of each, the compulsory HBM bytes of the fused launch (4 B per coded bit read, 8 B per
antenna port and resource element written) and the fraction of 8 TB/s it reaches.  ``--out FILE`` also writes the line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8.0e12
BATCH, PRBS, LAYERS, PORTS, TPMI = 64, 273, 4, 4, 3


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
    _ffi.device()
    pc = nr.PUSCHConfig(tb_config=nr.TBConfig(mcs_index=22, mcs_table=2), n_size_bwp=PRBS, num_layers=LAYERS,
                        num_antenna_ports=PORTS, precoding="codebook", tpmi=TPMI)
    tx = nr.PUSCHTransmitter(pc, return_bits=False)
    n = pc.num_coded_bits
    g = torch.Generator(device="cuda").manual_seed(0)
    c = torch.randint(0, 2, (BATCH, 1, n), device="cuda", generator=g).to(torch.float32)

    def separate():
        return tx._precoder(tx._resource_grid_mapper(tx._layer_mapper(tx._mapper(c))))

    assert torch.equal(tx._grid(c), separate())
    fused_s, separate_s = timed(lambda: tx._grid(c), a.iters, a.warmup), timed(separate, a.iters, a.warmup)
    hbm = BATCH * (4 * n + 8 * PORTS * 14 * 12 * PRBS)
    rec = {"batch": BATCH, "prbs": PRBS, "layers": LAYERS, "ports": PORTS, "num_bits_per_symbol": int(pc.tb.num_bits_per_symbol),
           "coded_bits_per_slot": n, "fused_us": round(fused_s * 1e6, 1), "separate_blocks_us": round(separate_s * 1e6, 1),
           "fused_hbm_bytes": hbm, "fused_fraction_of_8TBps": round(hbm / fused_s / PEAK_BYTES, 3)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
