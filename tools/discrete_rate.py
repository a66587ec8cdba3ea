#!/usr/bin/env python3
"""Rate of the discrete-channel kernel (csrc/discrete.hip) with HIP events, float32 at 2^26 elements after warm-up:
  BinarySymmetricChannel, hard output                    scalar pb
  BinarySymmetricChannel, LLR output                     scalar pb, two correctly rounded logs per element
  BinaryMemorylessChannel, hard output                   per-position pb [n, 2] against x [B, n]
and two comparisons of the same size in the same run:
  y.copy_(x)                                             the floor of a streaming kernel (reads x, writes y)
  (torch.rand_like(x) < pb) XOR x                        the torch composition of the hard symmetric channel
Prints one JSON line per measurement - the time per call and the bytes of x + y over that time - and a last line that says
for each kernel configuration how far it sits from the copy: within 15 % of it the kernel is on the HBM bound, beyond that
on its own arithmetic (Philox, and for LLR output the two logs per element)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / iters


def main():
    import torch
    import sionna_amd.phy as phy
    from sionna_amd import _ffi
    from sionna_amd.phy.channel import BinaryMemorylessChannel, BinarySymmetricChannel
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n, row = 1 << a.log2n, 1024
    dev = _ffi.device()
    phy.config.seed = 1
    x = phy.mapping.BinarySource()([n // row, row])
    x = x.as_subclass(torch.Tensor) if type(x) is not torch.Tensor else x
    y = torch.empty_like(x)
    pb2 = torch.rand(row, 2, device=dev) * 0.2
    bsc, bsc_llr, bmc = BinarySymmetricChannel(), BinarySymmetricChannel(return_llrs=True), BinaryMemorylessChannel()
    nbytes = 2 * x.numel() * x.element_size()
    runs = [("bsc_hard", lambda: bsc(x, 0.1)), ("bsc_llr", lambda: bsc_llr(x, 0.1)), ("bmc_hard_per_position_pb", lambda: bmc(x, pb2)),
            ("copy", lambda: y.copy_(x)),
            ("torch_rand_like_lt_pb_xor", lambda: torch.logical_xor(torch.rand_like(x) < 0.1, x > 0).to(x.dtype))]
    res = {}
    for name, fn in runs:
        s = timed(fn, a.iters, a.warmup)
        res[name] = s
        print(json.dumps({"case": name, "elements": n, "dtype": "float32", "us_per_call": round(s * 1e6, 1),
                          "x_plus_y_GB_per_s": round(nbytes / s * 1e-9, 1)}), flush=True)
    verdict = {k: {"times_the_copy": round(res[k] / res["copy"], 2), "bound": "HBM" if res[k] <= 1.15 * res["copy"] else "arithmetic"}
               for k in ("bsc_hard", "bsc_llr", "bmc_hard_per_position_pb")}
    verdict["torch_composition_times_bsc_hard"] = round(res["torch_rand_like_lt_pb_xor"] / res["bsc_hard"], 2)
    print(json.dumps(verdict), flush=True)


if __name__ == "__main__":
    main()
