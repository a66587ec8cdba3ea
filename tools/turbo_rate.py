#!/usr/bin/env python3
"""Rate of the turbo decoder (csrc/turbo.hip) with HIP events: LTE code (constraint length 4, terminated), rate 1/3,
k = 512 and k = 6144, 8 iterations, map and maxlog.  Measures in the same run
  fused        TurboDecoder: 2 num_iter launches of samd_turbo_bcjr
  composition  the same decoder put together from the separate public blocks the way the reference's call does it
               (fec/turbo/decoding.py:383-428): the gathers that split the codeword, BCJRDecoder(hard_out=False) with llr_a,
               the interleaver as a gather, torch subtraction, concatenation and clamp
and checks that both give the same bits.  Prints one JSON line per shape and algorithm; ``--out FILE`` also appends them
to FILE (profiles/turbo_rate.txt)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 8192), (6144, 1024)]          # (k, batch)
NUM_ITER = 8


def composition(dec, bcjr, tabs, llr):
    import torch
    k, T = dec.k, tabs["idx1"].shape[0]
    pad = torch.nn.functional.pad(llr, (0, 1))                       # index -1 reads the appended 0
    y1, y2 = pad[:, tabs["idx1"].reshape(-1)], pad[:, tabs["idx2"].reshape(-1)]
    ch1, ch2 = y1[:, 0:2 * k:2], y2[:, 0:2 * k:2]
    B = llr.shape[0]
    llr_1e = torch.zeros((B, T), device=llr.device)
    terminfo = torch.zeros((B, T - k), device=llr.device)
    perm, inv = tabs["perm"], tabs["inv"]
    llr_2i = None
    for _ in range(dec.num_iter):
        llr_1i = bcjr(y1, llr_a=llr_1e)[:, :k]
        llr_extr = llr_1i - ch1 - llr_1e[:, :k]
        llr_2e = torch.clamp(torch.cat([llr_extr[:, perm], terminfo], dim=-1), -20., 20.)
        llr_2i = bcjr(y2, llr_a=llr_2e)[:, :k]
        llr_extr = llr_2i - llr_2e[:, :k] - ch2
        llr_1e = torch.cat([torch.clamp(llr_extr[:, inv], -20., 20.), terminfo], dim=-1)
    return (0.0 < llr_2i[:, inv]).to(llr.dtype)


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import sionna_amd.phy as phy
    lines = []
    for k, B in SHAPES:
        enc = phy.fec.turbo.TurboEncoder(constraint_length=4, rate=1/3, terminate=True)
        g = torch.Generator(device="cuda").manual_seed(0)
        u = (torch.rand((B, k), device="cuda", generator=g) < 0.5).float()
        c = enc(u)
        llr = 2.0 * (2 * c - 1) + 2.0 * torch.randn(c.shape, device="cuda", generator=g)     # Es/N0 = -3 dB
        for alg in ("map", "maxlog"):
            dec = phy.fec.turbo.TurboDecoder(enc, num_iter=NUM_ITER, hard_out=True, algorithm=alg)
            bcjr = phy.fec.conv.BCJRDecoder(gen_poly=enc.gen_poly, rsc=True, terminate=True, hard_out=False, algorithm=alg)
            out = dec(llr)
            tabs = {n: t.long() for n, t in dec._tables.get(k)[1].items()}
            same = bool(torch.equal(out, composition(dec, bcjr, tabs, llr)))
            s_f = timed(lambda: dec(llr), a.iters, a.warmup)
            s_c = timed(lambda: composition(dec, bcjr, tabs, llr), a.iters, a.warmup)
            line = json.dumps({"k": k, "n": int(c.shape[1]), "batch": B, "num_iter": NUM_ITER, "algorithm": alg,
                               "fused_ms": round(s_f * 1e3, 2), "composition_ms": round(s_c * 1e3, 2),
                               "fused_decodes_per_s": round(B / s_f), "composition_decodes_per_s": round(B / s_c),
                               "speedup": round(s_c / s_f, 3), "same_bits": same,
                               "ber": float((out != u).float().mean())})
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
