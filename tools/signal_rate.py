#!/usr/bin/env python3
"""Output-sample rate of the filter kernel (csrc/signal.hip) with HIP events, complex64 input, real root-raised-cosine taps,
K = 129 (span 32, 4 samples per symbol), rows x samples = 4096 x 4096 at the oversampled rate:
  (a) convolve "same"                       4096 x 4096 in, 4096 x 4096 out
  (b) upfirdn(up = 4), "full"               4096 x 1024 symbols in, 4096 x 4224 samples out
  (c) upfirdn(down = 4), offset K - 1       4096 x 4224 samples in, 4096 x 1024 symbols out
One JSON line per case: output samples per second and the two counted bounds
  - compulsory HBM bytes per output (8 B written, 8 / 2 / 32 B read) at 8 TB/s;
  - vector multiply / add issue: a complex sample times a real tap is 2 multiplications and 2 additions, over the taps that
    meet a sample (129, 129 / 4, 129), at one wave-instruction (64 lanes) per SIMD per 2 cycles, 256 CUs x 4 SIMDs, 2.4 GHz;
and the measured fraction of the smaller one.  For orientation only: torch.nn.functional.conv1d on the same shapes (real and
imaginary rows as a batch, zero-stuffed input for (b), stride 4 for (c)) and the three-block composition
Downsampling(convolve(Upsampling(x))).  ``--out FILE`` also writes the lines to FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8.0e12
VALU_LANE_OPS = 256 * 4 * 2.4e9 / 2 * 64       # lane-operations per second, chip-wide
ROWS, SAMPLES, SPS, SPAN, BETA = 4096, 4096, 4, 32, 0.22


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from sionna_amd import _ffi
    from sionna_amd.phy import signal as sig
    _ffi.device()
    rrc = sig.RootRaisedCosineFilter(SPAN, SPS, BETA)
    h = rrc._taps().cuda()
    k = h.shape[0]
    g = torch.Generator(device="cuda").manual_seed(0)
    symbols = torch.randn((ROWS, SAMPLES // SPS, 2), device="cuda", generator=g)
    samples = torch.randn((ROWS, SAMPLES, 2), device="cuda", generator=g)
    x_sym, x_smp = torch.view_as_complex(symbols), torch.view_as_complex(samples)
    x_full = torch.view_as_complex(torch.randn((ROWS, SAMPLES + k - 1, 2), device="cuda", generator=g))
    w = h.flip(0).reshape(1, 1, k)
    up, down = sig.Upsampling(SPS), sig.Downsampling(SPS, k - 1, SAMPLES // SPS)

    def planar(x):
        return torch.view_as_real(x).permute(0, 2, 1).reshape(-1, 1, x.shape[-1])

    cases = [
        ("convolve_same", lambda: sig.convolve(x_smp, h, "same"), ROWS * SAMPLES, 8 + 8, k,
         lambda: F.conv1d(planar(x_smp), w, padding=k // 2), lambda: sig.convolve(x_smp, h, "same")),
        ("upfirdn_up4", lambda: sig.upfirdn(x_sym, h, up=SPS), ROWS * (SAMPLES + k - 1), 8 + 8 / SPS, k / SPS,
         lambda: F.conv1d(planar(up(x_sym)), w, padding=k - 1), lambda: sig.convolve(up(x_sym), h)),
        ("upfirdn_down4", lambda: sig.upfirdn(x_full, h, down=SPS, offset=k - 1, num_symbols=SAMPLES // SPS), ROWS * SAMPLES // SPS,
         8 + 8 * SPS, k, lambda: F.conv1d(planar(x_full), w, stride=SPS), lambda: down(sig.convolve(x_full, h))),
    ]
    lines = []
    for name, fn, outputs, bytes_per_out, taps, torch_fn, blocks_fn in cases:
        s = timed(fn, a.iters, a.warmup)
        rate = outputs / s
        hbm, valu = PEAK_BYTES / bytes_per_out, VALU_LANE_OPS / (4 * taps)
        rec = {"case": name, "K": k, "rows": ROWS, "outputs": outputs, "us_per_call": round(s * 1e6, 1),
               "outputs_per_s": round(rate), "hbm_bytes_per_output": round(bytes_per_out, 2), "hbm_bound_outputs_per_s": round(hbm),
               "valu_ops_per_output": round(4 * taps, 1), "valu_bound_outputs_per_s": round(valu),
               "fraction_of_bound": round(rate / min(hbm, valu), 3),
               "torch_conv1d_us": round(timed(torch_fn, a.iters, a.warmup) * 1e6, 1),
               "three_blocks_us": round(timed(blocks_fn, a.iters, a.warmup) * 1e6, 1)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
