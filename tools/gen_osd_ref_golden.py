#!/usr/bin/env python3
"""Generates the fixtures of the ordered-statistics decoder by EXECUTING the reference's own fec/linear/decoding.py
(OSDecoder, :14-478) under the NumPy stand-in for TensorFlow (tools/ref_exec):
  tests/golden/osd_ref_golden.npz       random full-rank codes (24,12) t=2 at 2 and 5 dB, (32,16) t=3 at 3 dB, (15,7) t=2
                                        at 6 dB: noisy BPSK LLRs, the reference's decisions in single and in double
                                        precision, and for every codeword the float64 relative gap between the two
                                        smallest candidate distances (read from the reference's own _get_dist in double
                                        precision); and per code the structured inputs (all-zero LLRs, noiseless +-4,
                                        |llr| = 1000 noiseless, every position +-100 with one sign flipped, noisy LLRs
                                        scaled past the float32 overflow of exp) with the reference's decisions
  tests/golden/osd_api_signatures.json  the OSDecoder signature read with ast as tools/gen_api_signatures.py does
Prints, per case, how many codewords fall under the gaps 1e-5 and 1e-4 and on how many the float32 and float64 decisions
of the reference differ.  Run here (needs /root/reference); the fixtures travel."""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

CASES = [("n24k12t2_2dB", 24, 12, 2, 2.0), ("n24k12t2_5dB", 24, 12, 2, 5.0), ("n32k16t3_3dB", 32, 16, 3, 3.0),
         ("n15k7t2_6dB", 15, 7, 2, 6.0)]
B = 250
STRUCT = ("zero", "noiseless4", "noiseless1000", "sat_flip", "sat_mixed")


def load_ref():
    from tools.ref_exec.loader import reference
    ref = reference()
    ref.load_utils()
    ref.load("sionna.phy.fec.ldpc.codes", package_dir=True)
    ref.load("sionna.phy.fec.utils")
    return ref.load("sionna.phy.fec.linear.decoding")


def random_code(rng, k, n):
    from sionna_amd.phy.fec.utils import make_systematic
    while True:
        g = rng.integers(0, 2, (k, n)).astype(np.float32)
        try:
            make_systematic(g)
            return g
        except ValueError:
            continue


def structured(rng, gm, llr_noisy):
    k, n = gm.shape
    u = rng.integers(0, 2, (len(STRUCT), k))
    c = (u @ gm.astype(np.int64)) % 2
    x = np.zeros((len(STRUCT), n), np.float32)
    x[1] = 4.0 * (2 * c[1] - 1)
    x[2] = 1000.0 * (2 * c[2] - 1)
    x[3] = 100.0 * (2 * c[3] - 1)
    x[3, n // 2] *= -1
    x[4] = llr_noisy[0] * 30.0
    return x


def run(ld, gm, t, llr, precision):
    """the reference's decisions and every distance it computed (order 0 first, then the orders), [bs, 1 + candidates]"""
    dec = ld.OSDecoder(gm, t=t, precision=precision)
    seen = []
    inner = dec._get_dist

    def spy(l, c_hat):
        d = inner(l, c_hat)
        seen.append(np.asarray(d))
        return d
    dec._get_dist = spy
    with np.errstate(over="ignore"):
        out = np.asarray(dec(llr.astype(np.float32 if precision == "single" else np.float64)))
    return out, np.concatenate(seen, axis=1)


def signatures():
    from tools.gen_api_signatures import params
    rel = "fec/linear/decoding.py"
    tree = ast.parse(open(os.path.join("/root/reference/src/sionna/phy", rel)).read())
    table = {}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == "OSDecoder":
            entry = {"kind": "class", "public": []}
            for item in node.body:
                if isinstance(item, ast.FunctionDef) and item.name in ("__init__", "call", "__call__"):
                    entry[item.name] = params(item)
                if isinstance(item, ast.FunctionDef) and not item.name.startswith("_") and item.name not in ("call", "build"):
                    is_prop = any(isinstance(d, ast.Name) and d.id == "property" for d in item.decorator_list)
                    entry["public"].append([item.name, "property" if is_prop else "method", None if is_prop else params(item)])
            table["fec.linear.OSDecoder"] = dict(entry, file=rel)
    return table


def main():
    import osd_f32 as spec
    with np.errstate(over="ignore"):
        assert np.isfinite(np.exp(spec.SAT32)) and np.isinf(np.exp(np.nextafter(spec.SAT32, np.float32(np.inf))))
    ld = load_ref()
    rng = np.random.default_rng(20261018)
    out = {"cases": np.array([c[0] for c in CASES]), "struct": np.array(STRUCT)}
    for name, n, k, t, ebno in CASES:
        gm = random_code(rng, k, n)
        u = rng.integers(0, 2, (B, k))
        c = (u @ gm.astype(np.int64)) % 2
        no = 1 / (10 ** (ebno / 10) * k / n)                              # BPSK: llr = 4 y / no, y = (2c - 1) + w
        y = (2 * c - 1) + rng.normal(size=c.shape) * np.sqrt(no / 2)
        llr = (4 * y / no).astype(np.float32)
        r32, _ = run(ld, gm, t, llr, "single")
        r64, d64 = run(ld, gm, t, llr, "double")
        two = np.sort(d64, axis=1)[:, :2]
        gap = (two[:, 1] - two[:, 0]) / two[:, 0]
        xs = structured(rng, gm, llr)
        s32, _ = run(ld, gm, t, xs, "single")
        s64, _ = run(ld, gm, t, xs, "double")
        p = name + "/"
        out.update({p + "gm": gm.astype(np.uint8), p + "t": np.int32(t), p + "llr": llr, p + "ref32": r32.astype(np.uint8),
                    p + "ref64": r64.astype(np.uint8), p + "gap": gap, p + "struct_llr": xs,
                    p + "struct_ref32": s32.astype(np.uint8), p + "struct_ref64": s64.astype(np.uint8)})
        print(f"{name}: {B} codewords, gap < 1e-5 on {int((gap < 1e-5).sum())}, gap < 1e-4 on {int((gap < 1e-4).sum())}, "
              f"float32 and float64 decisions differ on {int((r32 != r64).any(axis=1).sum())}, "
              f"block errors {int((r64 != c).any(axis=1).sum())}")
        for dt, r, s in ((np.float32, r32, s32), (np.float64, r64, s64)):
            got = spec.decode(llr.astype(dt), gm, t, dt)
            bad = (got != r).any(axis=1)
            print(f"   spec {dt.__name__}: differs from the reference on {int(bad.sum())} codewords "
                  f"({int((bad & (gap >= 1e-5)).sum())} of them at gap >= 1e-5); structured: "
                  f"{int((spec.decode(xs.astype(dt), gm, t, dt) != s).any(axis=1).sum())} differ")
    path = os.path.join(GOLD, "osd_ref_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    path = os.path.join(GOLD, "osd_api_signatures.json")
    with open(path, "w") as f:
        json.dump({"_comment": "reference signature of fec/linear OSDecoder by ast (tools/gen_osd_ref_golden.py); defaults as source text",
                   "signatures": signatures()}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
