#!/usr/bin/env python3
"""Rate of the convolutional-code decoders (csrc/conv.hip) with HIP events, at the notebook shapes:
  Viterbi K = 8, k = 64, n = 128 (5G_Channel_Coding_Polar_vs_LDPC_Codes.ipynb cell 8)
  Viterbi K = 5, k = 512, n = 1024 (Evolution_of_FEC.ipynb cell 5)
  BCJR map K = 4, k = 512, n = 1024 (the constituent code of the LTE turbo code)
Prints one JSON line per shape: decodes/s, and the two bounds:
  - compulsory HBM bytes (n LLRs read, k outputs written, float32) at 8 TB/s;
  - vector-instruction issue: with ``--counters CSV`` (a rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES counter_collection.csv
    of ``conv_rate.py --pmc-pass``), the vector instructions per codeword at one wave-instruction per SIMD per 2 cycles,
    256 CUs x 4 SIMDs at 2.4 GHz;
and the measured fraction of the smaller one."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8.0e12
VALU_ISSUE = 256 * 4 * 2.4e9 / 2          # wave-instructions per second, chip-wide
SHAPES = [("viterbi", 8, 64, 65536, "conv_viterbi_kernel"), ("viterbi", 5, 512, 16384, "conv_viterbi_kernel"),
          ("bcjr_map", 4, 512, 16384, "conv_bcjr_kernel")]


def block(kind, K):
    import sionna_amd.phy as phy
    c = phy.fec.conv
    if kind == "viterbi":
        return c.ViterbiDecoder(rate=1/2, constraint_length=K)
    return c.BCJRDecoder(rate=1/2, constraint_length=K, algorithm="map")


def measure(kind, K, k, B, iters, warmup):
    import torch
    dec = block(kind, K)
    g = torch.Generator(device="cuda").manual_seed(0)
    llr = 2.0 * torch.randn((B, 2 * k), device="cuda", generator=g) + 1.0
    for _ in range(warmup):
        dec(llr)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        dec(llr)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / iters


def valu_per_codeword(path):
    """kernel name -> (SQ_INSTS_VALU, SQ_WAVES) summed over dispatches; instructions per wave"""
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            for key in ("conv_viterbi_kernel<float, 2>", "conv_viterbi_kernel<float, 1>", "conv_bcjr_kernel<float, 0, 1>"):
                if key in name:
                    d = tot.setdefault(key, {})
                    d[row["Counter_Name"]] = d.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    return {k: v["SQ_INSTS_VALU"] / v["SQ_WAVES"] for k, v in tot.items() if v.get("SQ_WAVES")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pmc-pass", action="store_true", help="one call per shape (run under rocprofv3 --pmc)")
    ap.add_argument("--counters", default=None, help="rocprofv3 counter_collection.csv of a --pmc-pass run")
    a = ap.parse_args()
    if a.pmc_pass:
        for kind, K, k, B, _ in SHAPES:
            measure(kind, K, k, B, 1, 0)
        return
    per_wave = valu_per_codeword(a.counters) if a.counters else {}
    for kind, K, k, B, kern in SHAPES:
        s = measure(kind, K, k, B, a.iters, a.warmup)
        ns = 1 << (K - 1)
        per_cw_waves = 1.0 if ns >= 64 else 1.0 / (64 // ns)               # waves per codeword (one wave for 128 states)
        rate = B / s
        nbytes = 4 * (2 * k + k)
        out = {"decoder": kind, "K": K, "k": k, "n": 2 * k, "batch": B, "us_per_call": round(s * 1e6, 1),
               "decodes_per_s": round(rate), "hbm_bound_decodes_per_s": round(PEAK_BYTES / nbytes)}
        key = f"{kern}<float, {'0, ' if kind != 'viterbi' else ''}{2 if ns > 64 else 1}>"
        if key in per_wave:
            per_cw = per_wave[key] * per_cw_waves
            out["valu_instructions_per_codeword"] = round(per_cw)
            out["valu_bound_decodes_per_s"] = round(VALU_ISSUE / per_cw)
        bound = min(out["hbm_bound_decodes_per_s"], out.get("valu_bound_decodes_per_s", float("inf")))
        out["fraction_of_bound"] = round(rate / bound, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
