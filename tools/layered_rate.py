"""Decode rate of cn_schedule="layered", 10 iterations, min-sum: layered_totals "resum" (csrc/ldpc5g_onchip_ly.hip) against
"running" (csrc/ldpc5g_onchip_lyrt.hip) in ONE process on the same pre-generated LLRs, at the codes of BASELINE configs C2,
C4 and C1.  Per code and engine: warm-up, then `--repeats` timed windows of `--calls` decodes each between HIP events, the
two engines alternating window by window; median, minimum, maximum and the spread (max - min) / median of the windows' rates.
Nothing about clocks is assumed: both engines run interleaved in the same minutes on the same device.

  python tools/layered_rate.py [--out profiles/layered_rt_rate.json] [--batch 65536] [--repeats 7] [--calls 3]

A difference between the engines counts only where it exceeds the larger of the two spreads ("faster_beyond_spread").
The tool stops when a decoder did not run the engine its row is named after.  (Until the running-total engine this file held
the flooding-20 / layered-10 / layered-20 comparison for min-sum and boxplus-phi that wrote profiles/r03b/layered_rate_*.txt;
tools/ber_curve_layered.py and bench.py still time flooding against layered.)"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sionna_amd.phy as phy  # noqa: E402

CODES = (("C2", 2816, 8448, "bg1", 6, 4.5), ("C4", 768, 1536, "bg2", 2, 3.0), ("C1", 1024, 2048, "bg1", 2, 3.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layered_rt_rate.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    phy.config.seed = 1
    rows = []
    for name, k, n, bg, m, ebno in CODES:
        enc = phy.fec.ldpc.LDPC5GEncoder(k, n, num_bits_per_symbol=m, bg=bg)
        no = phy.utils.ebnodb2no(ebno, m, k / n)
        u = phy.mapping.BinarySource()([a.batch, k])
        llr = phy.mapping.Demapper("app", "qam", m)(phy.channel.AWGN()(phy.mapping.Mapper("qam", m)(enc(u)), no), no)
        decs, bler, engine = {}, {}, {}
        for tot in ("resum", "running"):
            d = phy.fec.ldpc.LDPC5GDecoder(enc, cn_update="minsum", cn_schedule="layered", num_iter=a.iters)
            d.layered_totals = tot
            for _ in range(2):                                  # warm-up: code objects, tables, workspace
                out = d(llr)
            torch.cuda.synchronize()
            decs[tot], engine[tot] = d, d.layered_engine
            if d.layered_engine != tot:                         # a fallback would make the comparison meaningless
                raise SystemExit(f"{name}: layered_totals={tot!r} ran the {d.layered_engine!r} engine - nothing measured")
            bler[tot] = float((out != u).any(dim=1).float().mean())
        rates = {"resum": [], "running": []}
        for _ in range(a.repeats):
            for tot in ("resum", "running"):                    # alternating windows
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    decs[tot](llr)
                e1.record()
                e1.synchronize()
                rates[tot].append(a.batch * a.calls / (e0.elapsed_time(e1) * 1e-3))
        row = {"config": name, "k": k, "n": n, "bg": bg, "z": enc.z, "batch": a.batch, "num_iter": a.iters, "cn_update": "minsum"}
        for tot in ("resum", "running"):
            r = rates[tot]
            med = statistics.median(r)
            row[tot] = {"engine": engine[tot], "decodes_per_s_median": round(med, 1), "min": round(min(r), 1), "max": round(max(r), 1),
                        "spread": round((max(r) - min(r)) / med, 4), "bler": bler[tot]}
        row["speedup_median"] = round(row["running"]["decodes_per_s_median"] / row["resum"]["decodes_per_s_median"], 3)
        row["faster_beyond_spread"] = bool(row["running"]["min"] > row["resum"]["max"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "tools/layered_rate.py", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_window": a.calls,
           "timing": "HIP events around each window, engines alternating", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
