#!/usr/bin/env python3
"""Generates the fixtures of the optical channels by EXECUTING the reference's own channel/optical/fiber.py and edfa.py
under the NumPy stand-in for TensorFlow (tools/ref_exec), in single AND double precision on the same complex64 input:
  tests/golden/optical_ref_golden.npz   per case of tests/optical_cases.py: e32 = max |single - double| over the
      reference's own two results and ymax = max |double|; the input and both outputs where the input has at most 4096
      elements (the others are regenerated from the case's seed); the window and frequency vectors of a few (n, h); the
      span loop of SSFM + EDFA.  The stand-in's transform runs in the operand's precision: NumPy keeps complex64 through
      numpy.fft (checked below), so e32 of the single run holds the single-precision transform's error.
  tests/golden/optical_ref_vectors.npz  the known answers the reference ships as data inside
      test/unit/channel/test_optical.py (|u| after length 5, for n_ssfm = 2000 and the adaptive scheme alike), the
      Gaussian input they belong to, and the reference's own double-precision results for them.
  tests/golden/optical_api_signatures.json   SSFM, EDFA and time_frequency_vector read with ast.
Run where the reference is present; the fixtures travel."""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_PHY = "/root/reference/src/sionna/phy"
REF_TEST = "/root/reference/test/unit/channel/test_optical.py"


def load_ref():
    import types
    import scipy.constants
    from tools.ref_exec.loader import reference
    ref = reference()
    ref.load_utils()
    const = types.ModuleType("sionna.phy.constants")
    const.H, const.PI = scipy.constants.Planck, scipy.constants.pi
    sys.modules["sionna.phy.constants"] = const
    sys.modules["sionna.phy"].constants = const
    utils = ref.load("sionna.phy.channel.utils")
    sys.modules["sionna.phy.channel.optical"] = types.ModuleType("sionna.phy.channel.optical")
    sys.modules["sionna.phy.channel.optical"].__path__ = []
    return ref.load("sionna.phy.channel.optical.fiber"), ref.load("sionna.phy.channel.optical.edfa"), utils


def run_ssfm(fiber, x, precision, **par):
    block = fiber.SSFM(precision=precision, **par)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(block(x.astype(np.complex64 if precision == "single" else np.complex128)))


def shipped_vectors():
    """the two long string constants of TestOptical.setUp: |u| in time and the spectrum"""
    tree = ast.parse(open(REF_TEST).read())
    long_strings = [n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str) and len(n.value) > 10000]
    assert len(long_strings) == 2
    return [np.array(s.split(","), dtype=np.float64) for s in long_strings]


def signatures():
    from tools.gen_api_signatures import params
    table = {}
    for rel, names in (("channel/optical/fiber.py", ["SSFM"]), ("channel/optical/edfa.py", ["EDFA"]),
                       ("channel/utils.py", ["time_frequency_vector"])):
        tree = ast.parse(open(os.path.join(REF_PHY, rel)).read())
        for node in tree.body:
            if isinstance(node, ast.ClassDef) and node.name in names:
                entry = {"kind": "class", "file": rel}
                for item in node.body:
                    if isinstance(item, ast.FunctionDef) and item.name in ("__init__", "call"):
                        entry[item.name] = params(item)
                table["channel." + node.name] = entry
            if isinstance(node, ast.FunctionDef) and node.name in names:
                table["channel." + node.name] = {"kind": "function", "file": rel, "params": params(node)}
    return table


def main():
    import optical_cases as oc
    assert np.fft.fft(np.ones(8, np.complex64)).dtype == np.complex64, "numpy.fft does not keep complex64: e32 would be a lower bound"
    fiber, edfa, utils = load_ref()
    out, meta = {}, {}
    for name, (shape, _) in oc.CASES.items():
        x = oc.make_input(name)
        par = oc.parameters(name)
        y32, y64 = run_ssfm(fiber, x, "single", **par), run_ssfm(fiber, x, "double", **par)
        assert y32.dtype == np.complex64 and y64.dtype == np.complex128 and y32.shape == tuple(shape)
        e32, ymax = float(np.max(np.abs(y32.astype(np.complex128) - y64))), float(np.max(np.abs(y64)))
        assert np.isfinite(e32) and np.isfinite(ymax), name
        meta[name] = dict(e32=e32, ymax=ymax, stored=bool(x.size <= 4096))
        if x.size <= 4096:
            out[name + "/x"], out[name + "/y32"], out[name + "/y64"] = x, y32, y64
        else:                                                     # a few rows, to pin the regenerated input
            out[name + "/x_head"], out[name + "/y64_head"] = x[:2], y64[:2]
        print(f"{name:24s} e32 {e32:.3e}  max|y| {ymax:.3e}")
    # windows and frequency vectors as the reference forms them
    for n, h in ((64, 0), (64, 1), (64, 8), (64, 32), (15, 3)):
        for prec in ("single", "double"):
            blk = fiber.SSFM(half_window_length=h, precision=prec)
            w = np.concatenate([np.asarray(blk._window[:h]).real, np.ones(n - 2 * h), np.asarray(blk._window[h:]).real])
            t, f = utils.time_frequency_vector(n, 0.5, precision=prec)
            out[f"window/{n}/{h}/{prec}"] = w.astype(np.float32 if prec == "single" else np.float64)
            out[f"tf/{n}/{prec}/t"], out[f"tf/{n}/{prec}/f"] = np.asarray(t), np.asarray(f)
    # the span loop
    sp = oc.SPAN
    res = {}
    for prec in ("single", "double"):
        u = oc.span_input().astype(np.complex64 if prec == "single" else np.complex128)
        span, amp = fiber.SSFM(precision=prec, **sp["ssfm"]), edfa.EDFA(precision=prec, **sp["edfa"])
        for _ in range(sp["n_span"]):
            u = np.asarray(amp(np.asarray(span(u))))
        res[prec] = u
    out["span/y32"], out["span/y64"] = res["single"], res["double"]
    meta["span"] = dict(e32=float(np.max(np.abs(res["single"].astype(np.complex128) - res["double"]))),
                        ymax=float(np.max(np.abs(res["double"]))), stored=True)
    print(f"{'span':24s} e32 {meta['span']['e32']:.3e}  max|y| {meta['span']['ymax']:.3e}")
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(GOLD, "optical_ref_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")

    # the shipped known answers (test_optical.py:25-92, 273-388): T = 100, N = 2^12, Gaussian of unit width and peak power
    u_ref, spectrum_ref = shipped_vectors()
    n, dt = 2 ** 12, 100 / 2 ** 12
    t, _ = utils.time_frequency_vector(n, dt, precision="double")
    u0 = np.exp(-(np.asarray(t) ** 2.0) / 2.0)
    par = dict(alpha=0.0, beta_2=1.0, f_c=193.55e12, gamma=1.0, half_window_length=0, length=5.0, sample_duration=dt,
               with_amplification=False, with_attenuation=False, with_dispersion=True, with_nonlinearity=True, t_norm=1e-12, n_sp=1.0)
    y_fixed = run_ssfm(fiber, u0.astype(np.complex128), "double", n_ssfm=2000, **par)
    y_adaptive = run_ssfm(fiber, u0.astype(np.complex128), "double", n_ssfm="adaptive", phase_inc=1e-3, **par)
    for nm, y in (("fixed", y_fixed), ("adaptive", y_adaptive)):
        print(f"reference double {nm}: mean (|u| - u_ref)^2 = {np.mean((np.abs(y) - u_ref) ** 2):.3e}, max | |u| - u_ref | = {np.max(np.abs(np.abs(y) - u_ref)):.3e}")
    path = os.path.join(GOLD, "optical_ref_vectors.npz")
    np.savez_compressed(path, u0=u0, u_ref=u_ref, spectrum_ref=spectrum_ref, sample_duration=np.float64(dt),
                        y_fixed=y_fixed, y_adaptive=y_adaptive)
    print("wrote", path, os.path.getsize(path), "bytes")
    path = os.path.join(GOLD, "optical_api_signatures.json")
    with open(path, "w") as f:
        json.dump({"_comment": "reference signatures of channel/optical/{fiber,edfa}.py and channel/utils.py time_frequency_vector by ast "
                               "(tools/gen_optical_ref_golden.py); defaults as source text", "signatures": signatures()}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
