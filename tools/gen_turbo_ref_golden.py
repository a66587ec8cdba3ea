#!/usr/bin/env python3
"""Generates the fixtures of the turbo codes by EXECUTING the reference's own fec/turbo/*.py and fec/interleaving.py
(TurboEncoder, TurboDecoder, TurboTermination, Turbo3GPPInterleaver; encoding.py:16-421, decoding.py:15-435, utils.py:10-296,
interleaving.py:598-745) under the NumPy stand-in for TensorFlow (tools/ref_exec):
  tests/golden/turbo_ref_golden.npz       per case random bits, their codeword, noisy LLRs and the decoder's soft outputs
                                          for map / log / maxlog in single and in double precision on the same inputs, hard
                                          decisions, the interleaver's permutation; rate 1/3 and 1/2, terminated and not,
                                          constraint lengths 3..6, the 3GPP and the random interleaver; the permutations of
                                          Turbo3GPPInterleaver for K = 40, 41, 48, 512, 1000, 6144 with their table rows; the
                                          TurboTermination round trips
  tests/golden/turbo_api_signatures.json  the signatures read with ast as tools/gen_api_signatures.py does
Run here (needs /root/reference); the fixtures travel."""
import ast
import contextlib
import io
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
B = 20
PERM_SIZES = (40, 41, 48, 512, 1000, 6144)

# (name, K, rate, terminate, interleaver, k, num_iter)
CASES = []
_KS = {3: 40, 4: 48, 5: 41, 6: 64}                                  # 41: pruned from the table's 48
for _rate, _tag in ((1/3, "r3"), (1/2, "r2")):
    for _term in (False, True):
        for _K in (3, 4, 5, 6):
            CASES.append((f"{_tag}K{_K}{'T' if _term else 'U'}", _K, _rate, _term, "3GPP", _KS[_K], 6 if _K == 4 else 3))
CASES.append(("r3K4Trand", 4, 1/3, True, "random", 57, 4))
CASES.append(("r2K5Urand", 5, 1/2, False, "random", 45, 4))          # rate 1/2, k odd: a last incomplete puncturing period
CASES.append(("r2K4Todd", 4, 1/2, True, "3GPP", 43, 4))              # k + 4 rows, odd
CASES.append(("r3K4Uk128", 4, 1/3, False, "3GPP", 128, 8))
DOUBLE_MAXLOG = ("r3K3U", "r2K4T", "r3K6T", "r2K5Urand")
HARD = ("r3K4T", "r2K4U", "r3K4Trand")


def load_ref():
    from tools.ref_exec.loader import reference
    ref = reference()
    for name in ("sionna.phy.fec.conv", "sionna.phy.fec.turbo"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
            setattr(sys.modules["sionna.phy.fec"], name.rpartition(".")[2], m)
    ref.load_utils()
    ref.load("sionna.phy.fec.ldpc.codes", package_dir=True)
    ref.load("sionna.phy.fec.utils")
    for m in ("utils", "encoding", "decoding"):
        ref.load(f"sionna.phy.fec.conv.{m}")
    ref.load("sionna.phy.fec.turbo.coeffs", package_dir=True)
    il = ref.load("sionna.phy.fec.interleaving")
    tu, te, td = [ref.load(f"sionna.phy.fec.turbo.{m}") for m in ("utils", "encoding", "decoding")]
    return il, tu, te, td


def signatures():
    from tools.gen_api_signatures import params
    table = {}
    for rel, mod, names in (("fec/turbo/utils.py", "fec.turbo", ["polynomial_selector", "puncture_pattern", "TurboTermination"]),
                            ("fec/turbo/encoding.py", "fec.turbo", ["TurboEncoder"]),
                            ("fec/turbo/decoding.py", "fec.turbo", ["TurboDecoder"]),
                            ("fec/interleaving.py", "fec.interleaving", ["Turbo3GPPInterleaver"])):
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


def quiet(fn, *a, **k):
    """the reference's TurboDecoder.call prints its input's dtype (decoding.py:366)"""
    with contextlib.redirect_stdout(io.StringIO()):
        return np.asarray(fn(*a, **k))


def main():
    from tools.ref_exec import tf_numpy
    il, tu, te, td = load_ref()
    rng = np.random.default_rng(20261020)
    out = {}
    for name, K, rate, term, itype, k, num_iter in CASES:
        enc = te.TurboEncoder(constraint_length=K, rate=rate, terminate=term, interleaver_type=itype)
        u = rng.integers(0, 2, (B, k)).astype(np.float32)
        c = quiet(enc, u)
        perm = quiet(enc.internal_interleaver, np.arange(k, dtype=np.float32)[None, :])[0].astype(np.int32)
        llr = ((2 * c - 1) * 2.0 + rng.normal(size=c.shape) * 2.0).astype(np.float32)
        p = name + "/"
        out.update({p + "gen_poly": np.array(enc.gen_poly), p + "rate_inv": np.int32(round(1 / rate)), p + "terminate": np.bool_(term),
                    p + "num_iter": np.int32(num_iter), p + "u": u.astype(np.uint8), p + "c": c.astype(np.uint8), p + "llr": llr,
                    p + "perm": perm})
        for alg in ("map", "log", "maxlog"):
            for prec in ("single", "double"):
                if alg == "maxlog" and prec == "double" and name not in DOUBLE_MAXLOG:
                    continue
                dec = td.TurboDecoder(enc, num_iter=num_iter, hard_out=False, algorithm=alg, precision=prec)
                if prec == "double":
                    # the encoder's interleaver is a single-precision block and would round the extrinsic values of a
                    # double-precision decoder to float32 on the way through (block.py:122-131): give the decoder the
                    # same permutation as a block of its own precision, as its constructor does without ``encoder``
                    dec.internal_interleaver = il.Turbo3GPPInterleaver(precision=prec) if itype == "3GPP" else \
                        il.RandomInterleaver(seed=enc.internal_interleaver.seed, keep_batch_constant=True, keep_state=True,
                                             axis=-1, precision=prec)
                r = quiet(dec, llr.astype(np.float64) if prec == "double" else llr)
                assert r.dtype == (np.float64 if prec == "double" else np.float32) and r.shape == (B, k), (r.dtype, r.shape)
                out[p + f"{alg}_{prec}"] = r
            if name in HARD:
                dec = td.TurboDecoder(enc, num_iter=num_iter, hard_out=True, algorithm=alg)
                out[p + f"{alg}_hard"] = quiet(dec, llr).astype(np.uint8)
    out["cases"] = np.array([c[0] for c in CASES])

    qpp = il.Turbo3GPPInterleaver()
    for K in PERM_SIZES:
        x = np.arange(K, dtype=np.float32)[None, :]
        out[f"qpp/perm_{K}"] = quiet(qpp, x)[0].astype(np.int32)
        out[f"qpp/inv_{K}"] = quiet(qpp, x, inverse=True)[0].astype(np.int32)
    sizes = sorted({K if K in qpp.coeffs_dict else min(x for x in qpp.coeffs_dict if x >= K) for K in PERM_SIZES})
    out["qpp/coeff_rows"] = np.array([(K,) + tuple(qpp.coeffs_dict[K]) for K in sizes], np.int32)
    out["qpp/num_rows"] = np.int32(len(qpp.coeffs_dict))

    for K in (3, 4, 5, 6):
        tt = tu.TurboTermination(K)
        mu = K - 1
        t1 = rng.integers(0, 2, (3, 2 * mu)).astype(np.int32)
        t2 = rng.integers(0, 2, (3, 2 * mu)).astype(np.int32)
        merged = np.asarray(tt.termbits_conv2turbo(t1.view(tf_numpy.Tensor), t2.view(tf_numpy.Tensor)))
        b1, b2 = tt.term_bits_turbo2conv(merged.astype(np.float32).view(tf_numpy.Tensor))
        out.update({f"term/K{K}/t1": t1.astype(np.uint8), f"term/K{K}/t2": t2.astype(np.uint8),
                    f"term/K{K}/merged": merged.astype(np.uint8), f"term/K{K}/num_syms": np.int32(tt.get_num_term_syms()),
                    f"term/K{K}/back1": np.asarray(b1).astype(np.uint8), f"term/K{K}/back2": np.asarray(b2).astype(np.uint8)})

    path = os.path.join(GOLD, "turbo_ref_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    path = os.path.join(GOLD, "turbo_api_signatures.json")
    with open(path, "w") as f:
        json.dump({"_comment": "reference signatures of fec/turbo and Turbo3GPPInterleaver by ast (tools/gen_turbo_ref_golden.py); "
                               "defaults as source text", "signatures": signatures()}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
