#!/usr/bin/env python3
"""Generates the fixtures of the convolutional codes by EXECUTING the reference's own fec/conv/*.py (ConvEncoder,
ViterbiDecoder, BCJRDecoder; encoding.py:10-292, decoding.py:13-943, utils.py:10-190) under the NumPy stand-in for
TensorFlow (tools/ref_exec):
  tests/golden/conv_ref_golden.npz      every polynomial_selector code (rate 1/2 and 1/3, K = 3..8), feed-forward and RSC,
                                        terminated and not, plus a custom gen_poly: codewords of random bits, and noisy
                                        LLRs decoded by Viterbi (soft_llr and hard, return_info_bits True / False) and
                                        by BCJR (map / log / maxlog, hard_out=False, with and without llr_a)
  tests/golden/conv_ref_vectors.npz     the reference's own test vectors test/codes/conv/conv_rate_*_ref_{u,y,uhat}.npy
                                        (bits as uint8), used by its test_ref_implementation
  tests/golden/conv_api_signatures.json the conv signatures read with ast as tools/gen_api_signatures.py does
Run here (needs /root/reference); the fixtures travel."""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
REF_TEST = "/root/reference/test/codes/conv"

CASES = []          # (name, gen_poly or None, rate, K, rsc, terminate)
for _rate, _tag in ((1/2, "r2"), (1/3, "r3")):
    for _K in range(3, 9):
        for _rsc in (False, True):
            for _term in (False, True):
                CASES.append((f"{_tag}K{_K}{'rsc' if _rsc else 'ff'}{'T' if _term else 'U'}", None, _rate, _K, _rsc, _term))
CASES.append(("customT", ("1101", "1011", "0111"), None, None, False, True))
CASES.append(("customU", ("10011", "11101"), None, None, False, False))


def load_ref():
    from tools.ref_exec.loader import reference
    ref = reference()
    ref.load_utils()
    ref.load("sionna.phy.fec.ldpc.codes", package_dir=True)
    ref.load("sionna.phy.fec.utils")
    mods = [ref.load(f"sionna.phy.fec.conv.{m}") for m in ("utils", "encoding", "decoding")]
    return mods


def signatures():
    from tools.gen_api_signatures import params
    table = {}
    for rel, mod, names in (("fec/conv/utils.py", "fec.conv", ["polynomial_selector", "Trellis"]),
                            ("fec/conv/encoding.py", "fec.conv", ["ConvEncoder"]),
                            ("fec/conv/decoding.py", "fec.conv", ["ViterbiDecoder", "BCJRDecoder"])):
        tree = ast.parse(open(os.path.join("/root/reference/src/sionna/phy", rel)).read())
        for node in tree.body:
            if isinstance(node, ast.ClassDef) and node.name in names:
                entry = {"kind": "class", "public": []}
                for item in node.body:
                    if isinstance(item, ast.FunctionDef) and item.name in ("__init__", "call", "__call__"):
                        entry[item.name] = params(item)
                    if isinstance(item, ast.FunctionDef) and not item.name.startswith("_") and item.name not in ("call", "build"):
                        is_prop = any(isinstance(d, ast.Name) and d.id == "property" for d in item.decorator_list)
                        entry["public"].append([item.name, "property" if is_prop else "method", None if is_prop else params(item)])
                table[f"{mod}.{node.name}"] = dict(entry, file=rel)
            elif isinstance(node, ast.FunctionDef) and node.name in names:
                table[f"{mod}.{node.name}"] = {"kind": "function", "params": params(node), "file": rel}
    return table


def main():
    cu, ce, cd = load_ref()
    rng = np.random.default_rng(20261016)
    out = {}
    B, k = 4, 24
    for name, gp, rate, K, rsc, term in CASES:
        kw = dict(gen_poly=gp) if gp is not None else dict(rate=rate, constraint_length=K)
        enc = ce.ConvEncoder(rsc=rsc, terminate=term, **kw)
        u = rng.integers(0, 2, (B, k)).astype(np.float32)
        c = np.asarray(enc(u))
        llr = ((2 * c - 1) * 2.0 + rng.normal(size=c.shape) * 1.6).astype(np.float32)
        la = (rng.normal(size=(B, c.shape[1] // len(enc.gen_poly))) * 1.5).astype(np.float32)
        p = name + "/"
        out.update({p + "gen_poly": np.array(enc.gen_poly), p + "rsc": np.bool_(rsc), p + "terminate": np.bool_(term),
                    p + "u": u.astype(np.uint8), p + "c": c.astype(np.uint8), p + "llr": llr, p + "llr_a": la})
        for a in ("to_nodes", "from_nodes", "op_mat", "op_by_tonode", "ip_by_tonode", "op_by_fromnode"):
            out[p + "trellis_" + a] = np.asarray(getattr(enc.trellis, a)).astype(np.int16)
        for method in ("soft_llr", "hard"):
            x = llr if method == "soft_llr" else (llr > 0).astype(np.float32)
            dec = cd.ViterbiDecoder(encoder=enc, method=method)
            out[p + f"vit_{method}"] = np.asarray(dec(x)).astype(np.uint8)
            # return_info_bits=False: the reference reshapes the [B, T] path symbols to [-1, n] (decoding.py:446-451),
            # which only works for B a multiple of conv_n: run it on the first conv_n codewords
            cn = len(enc.gen_poly)
            dec = cd.ViterbiDecoder(encoder=enc, method=method, return_info_bits=False)
            out[p + f"vit_{method}_cw"] = np.asarray(dec(x[:cn])).astype(np.int16)
        for alg in ("map", "log", "maxlog"):
            dec = cd.BCJRDecoder(encoder=enc, algorithm=alg, hard_out=False)
            out[p + f"bcjr_{alg}"] = np.asarray(dec(llr)).astype(np.float32)
            dec = cd.BCJRDecoder(encoder=enc, algorithm=alg, hard_out=False)
            out[p + f"bcjr_{alg}_a"] = np.asarray(dec(llr, llr_a=la)).astype(np.float32)
    out["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(GOLD, "conv_ref_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")

    vec = {}
    for tag in ("half_57", "half_6474", "onethird_577", "onefourth_5777"):
        for part in ("u", "y", "uhat"):
            a = np.load(os.path.join(REF_TEST, f"conv_rate_{tag}_ref_{part}.npy"))
            vec[f"{tag}/{part}"] = a.astype(np.uint8) if part != "y" else a
    path = os.path.join(GOLD, "conv_ref_vectors.npz")
    np.savez_compressed(path, **vec)
    print("wrote", path, os.path.getsize(path), "bytes")

    path = os.path.join(GOLD, "conv_api_signatures.json")
    with open(path, "w") as f:
        json.dump({"_comment": "reference signatures of fec/conv by ast (tools/gen_conv_ref_golden.py); defaults as source text",
                   "signatures": signatures()}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
