#!/usr/bin/env python3
"""Rate of the ordered-statistics decoder (csrc/osd.hip) with HIP events:
  (128,64) random code, t = 1..4 (5G_Channel_Coding_Polar_vs_LDPC_Codes.ipynb cell 17 runs t = 4), and BCH (63,45), t = 2.
Prints one JSON line per configuration: codewords/s and candidates/s, the time of the MRB stage and of the search stage,
and each stage's vector-issue bound with the measured fraction of it.
  - Stages: a decode at order t launches the binomial table, the MRB kernel, the search kernel and the final kernel; at
    t = 0 it launches everything but the search.  MRB stage = the time of the same batch at t = 0, search stage = the
    time at order t minus that.
  - Search bound: the loop body of osd_search_kernel<1, 8> per candidate (one parity word, byte tables), counted in the
    gfx950 disassembly: 46 vector instructions and 10 ds_read_b64 (the row, the row's cost, 8 table entries) per lane
    and candidate, i.e. per wave-instruction 64 candidates.  Vector issue at one wave-instruction per SIMD per 2 cycles,
    256 CUs x 4 SIMDs at 2.4 GHz (as tools/conv_rate.py); the LDS figure is 10 reads of 512 B per 64 candidates at
    128 B per cycle and CU without bank conflicts.
  - MRB bound: an ESTIMATE from the source, not a count of the disassembly: per codeword (one wave) the rank loop is n
    iterations of about 6 vector instructions for each of ceil(n / 64) columns per lane, the column gather 64 iterations
    of about 8 for each of ceil(k W / 64) words per lane, the parity extraction the same over k P words, and the
    elimination k steps of about 4 + W + 3 W ceil(k / 64) instructions (pivot search, test and XOR of each lane's rows)."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_ISSUE = 256 * 4 * 2.4e9 / 2          # wave-instructions per second, chip-wide
LDS_CYCLES = 256 * 2.4e9                  # LDS cycles per second, chip-wide (128 B per cycle and CU)
VALU_PER_CANDIDATE = 46                   # osd_search_kernel<1, 8> loop body, per lane = per candidate
LDS_READS_PER_CANDIDATE = 10              # ds_read_b64 per lane and candidate; 4 cycles per wave-instruction


def code(n, k):
    from sionna_amd.phy.fec.utils import load_parity_check_examples, make_systematic, pcm2gm
    if (n, k) == (63, 45):
        return pcm2gm(load_parity_check_examples(1)[0])
    rng = np.random.default_rng(n * 1000 + k)
    while True:
        g = rng.integers(0, 2, (k, n)).astype(np.float32)
        try:
            make_systematic(g)
            return g
        except ValueError:
            continue


def measure(gm, t, llr, iters, warmup):
    import torch
    from sionna_amd.phy.fec.linear import OSDecoder
    dec = OSDecoder(gm, t=t)
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


def mrb_valu_per_codeword(n, k):
    W, P, cols, rows = -(-n // 64), -(-(n - k) // 64), -(-n // 64), -(-k // 64)
    rank = cols * n * 6
    gather = (-(-(k * W) // 64) + -(-(k * P) // 64)) * 64 * 8
    elim = k * (4 + W + 3 * W * rows)
    return rank + gather + elim


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for n, k, t, B in ((128, 64, 1, 65536), (128, 64, 2, 65536), (128, 64, 3, 8192), (128, 64, 4, 1024), (63, 45, 2, 65536)):
        gm = code(n, k)
        g = torch.Generator(device="cuda").manual_seed(0)
        llr = 2.0 * torch.randn((B, n), device="cuda", generator=g) + 1.0
        s_mrb = measure(gm, 0, llr, a.iters, a.warmup)
        s_all = measure(gm, t, llr, a.iters, a.warmup)
        s_search = max(s_all - s_mrb, 1e-12)
        cand = sum(math.comb(k, i) for i in range(1, t + 1))
        cand_rate = B * cand / s_search
        valu_bound = VALU_ISSUE * 64 / VALU_PER_CANDIDATE
        lds_bound = LDS_CYCLES * 64 / (LDS_READS_PER_CANDIDATE * 4)
        mrb_bound = VALU_ISSUE / mrb_valu_per_codeword(n, k)
        print(json.dumps({
            "n": n, "k": k, "t": t, "batch": B, "candidates_per_codeword": cand, "us_per_call": round(s_all * 1e6, 1),
            "codewords_per_s": round(B / s_all), "mrb_stage_us": round(s_mrb * 1e6, 1), "search_stage_us": round(s_search * 1e6, 1),
            "mrb_codewords_per_s": round(B / s_mrb), "mrb_valu_bound_codewords_per_s_estimate": round(mrb_bound),
            "mrb_fraction_of_bound": round(B / s_mrb / mrb_bound, 3),
            "search_candidates_per_s": round(cand_rate), "search_valu_bound_candidates_per_s": round(valu_bound),
            "search_lds_bound_candidates_per_s": round(lds_bound),
            "search_fraction_of_valu_bound": round(cand_rate / valu_bound, 3)}), flush=True)


if __name__ == "__main__":
    main()
