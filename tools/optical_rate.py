#!/usr/bin/env python3
"""Rate of the SSFM fibre (csrc/optical.hip) with HIP events after warm-up: n = 4096, rows = 256, 200 steps, complex64,
against the same steps written with torch.fft and torch pointwise operations on the same device (half D, 199 x [N, D],
N, half D; dispersion, attenuation and nonlinearity, no window, no noise).  Writes both rates (steps x samples per
second) and their ratio to profiles/optical_rate.json and prints the same JSON line."""
import argparse
import json
import math
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
    import numpy as np
    import torch
    from sionna_amd import _ffi
    from sionna_amd.phy.channel import SSFM
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = _ffi.device()
    par = dict(alpha=0.046, beta_2=-21.67, gamma=1.27, length=80.0, sample_duration=1.0)
    t = (torch.arange(a.n, device=dev) - a.n // 2) / (a.n / 16)
    x = (math.sqrt(0.01) * torch.exp(-t * t / 2)).to(torch.complex64).repeat(a.rows, 1).contiguous()
    ssfm = SSFM(n_ssfm=a.steps, **par)

    dz = par["length"] / a.steps
    k = np.arange(a.n)
    f = (((k - a.n // 2) % a.n) - a.n // 2) / (par["sample_duration"] * a.n)
    c2 = -par["beta_2"] / 2.0 * (2 * np.pi * f) ** 2
    tf = lambda d: torch.from_numpy((np.exp(1j * c2 * d) * np.exp(-par["alpha"] / 2 * d)).astype(np.complex64)).to(dev)
    tf_full, tf_half = tf(dz), tf(dz / 2)

    def torch_steps():
        q = torch.fft.ifft(torch.fft.fft(x) * tf_half)
        for s in range(a.steps):
            q = q * torch.exp(-1j * par["gamma"] * dz * (q.real * q.real + q.imag * q.imag))
            q = torch.fft.ifft(torch.fft.fft(q) * (tf_half if s == a.steps - 1 else tf_full))
        return q

    err = float((ssfm(x).as_subclass(torch.Tensor) - torch_steps()).abs().max())
    s_hip, s_torch = timed(lambda: ssfm(x), a.iters, a.warmup), timed(torch_steps, a.iters, a.warmup)
    work = a.steps * a.rows * a.n
    res = {"n": a.n, "rows": a.rows, "steps": a.steps, "dtype": "complex64", "ssfm_ms": round(s_hip * 1e3, 3),
           "torch_ms": round(s_torch * 1e3, 3), "ssfm_step_samples_per_s": round(work / s_hip), "torch_step_samples_per_s": round(work / s_torch),
           "torch_over_ssfm": round(s_torch / s_hip, 2), "max_abs_difference": err}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = os.environ.get("OPTICAL_RATE_OUT") or os.path.join(ROOT, "profiles", "optical_rate.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
