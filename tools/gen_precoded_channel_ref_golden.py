#!/usr/bin/env python3
"""Generates tests/golden/precoded_channel_ref_golden.npz by EXECUTING the reference's own ``RZFPrecodedChannel`` /
``CBFPrecodedChannel`` / ``EyePrecodedChannel`` (ofdm/precoding.py:179-566) and ``LMMSEPostEqualizationSINR``
(ofdm/equalization.py:464-839) under the NumPy stand-in for TensorFlow (tools/ref_exec), in single AND double precision, and
tests/golden/precoded_channel_api_signatures.json (the six classes' signatures read with ast, as
tools/gen_conv_ref_golden.py does).

Every case uses a grid of fft_size 16 with guard carriers (2, 1) and a DC null (12 effective subcarriers), 2 OFDM symbols
and batch 3:
  su    1 tx (4 antennas) -> 1 rx x 2 antennas; alpha 0; tx_power and no of rank 0
  mu4   1 tx (4 antennas) -> 4 rx x 1 antenna (square); scalar alpha; tx_power of rank 2, no of rank 1
  mu8   1 tx (8 antennas) -> 4 rx x 1 antenna; alpha [B]; tx_power of rank 3 with one stream at power 0, no of rank 3
  mc    2 tx (8 antennas), each -> 2 of 4 rx x 2 antennas, every receiver hears both (6 interfering streams); alpha,
        tx_power and no of full shape; precoding from a channel estimate h_hat != h; an estimated h_eff for the SINR
  rt    1 tx (5 antennas) -> 3 rx x 1 antenna (sizes without a compiled instantiation); alpha 0
  s3    1 tx (4 antennas) -> 1 rx x 3 antennas (3 streams: the SINR's run-time sizes)
  eye   2 tx x 2 antennas -> 1 rx x 4 antennas, identity precoder; no interfering streams
Inputs are float32-representable, so both precisions see the same data, and well conditioned: i.i.d. CN(0, 1) channels,
no >= 0.01, alpha = 0 only where K < M.  The SINR of either precision is computed from the reference's single-precision
h_eff (stored), so that the families are measured independently.

Prints, per family, e32 = the largest deviation of the reference's single-precision result from its double-precision result
relative to the largest magnitude of the latter - the figure tests/precoded_channel_f32.py states next to its bars.
Run here (needs /root/reference); the fixture travels."""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
B, T, FFT, GUARDS = 3, 2, 16, (2, 1)

#        name  association                       streams/tx  rxa  M
CASES = [("su", [[1]], 2, 2, 4),
         ("mu4", [[1]] * 4, 4, 1, 4),
         ("mu8", [[1]] * 4, 4, 1, 8),
         ("mc", [[1, 0], [1, 0], [0, 1], [0, 1]], 4, 2, 8),
         ("rt", [[1]] * 3, 3, 1, 5),
         ("s3", [[1]], 3, 3, 4),
         ("eye", [[1, 1]], 2, 4, 2)]


def cn(rng, shape):
    return ((rng.normal(size=shape) + 1j * rng.normal(size=shape)) / np.sqrt(2)).astype(np.complex64)


def inputs(name, assoc, K, rxa, M, rng):
    """the arguments of a case: h, h_hat (or None), alpha, tx_power, no"""
    rx, ntx = np.asarray(assoc).shape
    h = cn(rng, (B, rx, rxa, ntx, M, T, FFT))
    u = lambda *s: rng.random(s).astype(np.float32)  # noqa: E731
    h_hat = None
    if name == "su":
        alpha, p, no = np.float32(0.0), np.float32(0.5), np.float32(0.1)
    elif name == "mu4":
        alpha, p, no = np.float32(0.1), 0.25 + u(B, ntx), 0.01 + u(B)
    elif name == "mu8":
        alpha, p, no = 0.05 + u(B), 0.25 + u(B, ntx, K), 0.01 + u(B, rx, rxa)
        p[:, :, 2] = 0.0                                                   # a stream without power
    elif name == "mc":
        alpha, p, no = 0.05 + u(B, ntx, T, FFT), 0.25 + u(B, ntx, K, T, FFT), 0.01 + u(B, rx, rxa, T, FFT - 4)
        h_hat = (h + np.float32(0.1) * cn(rng, h.shape)).astype(np.complex64)
    elif name == "rt":
        alpha, p, no = np.float32(0.0), 0.25 + u(B, ntx), np.float32(0.05)
    elif name == "s3":
        alpha, p, no = np.float32(0.05), np.float32(1.0), 0.01 + u(B)
    else:
        alpha, p, no = None, 0.25 + u(B, ntx, K), 0.01 + u(B, rx)
    return h, h_hat, alpha, p, no


def rel_dev(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def signatures():
    from tools.gen_api_signatures import params
    table = {}
    for rel, names in (("ofdm/precoding.py", ["PrecodedChannel", "RZFPrecodedChannel", "CBFPrecodedChannel", "EyePrecodedChannel"]),
                       ("ofdm/equalization.py", ["PostEqualizationSINR", "LMMSEPostEqualizationSINR"])):
        tree = ast.parse(open(os.path.join("/root/reference/src/sionna/phy", rel)).read())
        for node in tree.body:
            if isinstance(node, ast.ClassDef) and node.name in names:
                entry = {"kind": "class", "bases": [b.id for b in node.bases if isinstance(b, ast.Name)], "public": []}
                for item in node.body:
                    if isinstance(item, ast.FunctionDef) and item.name in ("__init__", "call"):
                        entry[item.name] = params(item)
                    if isinstance(item, ast.FunctionDef) and not item.name.startswith("_") and item.name not in ("call", "build"):
                        entry["public"].append([item.name, "method", params(item)])
                table[f"ofdm.{node.name}"] = dict(entry, file=rel)
    return table


def main():
    from tools.gen_ofdm_rx_ref_golden import load
    from tools.ref_exec.loader import reference
    mp, mimo, ofdm, od, ce, eq = load()
    ref = reference()
    pm = ref.load("sionna.phy.mimo.precoding")
    for k, v in vars(pm).items():
        if not k.startswith("_"):
            setattr(mimo, k, v)
    po = ref.load("sionna.phy.ofdm.precoding")
    rng = np.random.default_rng(20261020)
    out, e32 = {}, {}

    def note(family, single, double):
        e32[family] = max(e32.get(family, 0.0), rel_dev(single, double))

    for name, assoc, K, rxa, M in CASES:
        rx, ntx = np.asarray(assoc).shape
        rg = ofdm.ResourceGrid(num_ofdm_symbols=T, fft_size=FFT, subcarrier_spacing=15e3, num_tx=ntx, num_streams_per_tx=K,
                               cyclic_prefix_length=2, num_guard_carriers=list(GUARDS), dc_null=True, pilot_pattern=None)
        sm = mimo.StreamManagement(np.array(assoc), K)
        h, h_hat, alpha, p, no = inputs(name, assoc, K, rxa, M, rng)
        o = {"rx_tx_association": np.array(assoc, np.int32), "num_streams_per_tx": np.int32(K), "h": h, "tx_power": p, "no": no,
             "effective_subcarrier_ind": np.asarray(rg.effective_subcarrier_ind).astype(np.int32)}
        if alpha is not None:
            o["alpha"] = alpha
        if h_hat is not None:
            o["h_hat"] = h_hat
        res = {}

        def block(cls, prec):
            # PrecodedChannel builds its RemoveNulledSubcarriers without handing its precision on (ofdm/precoding.py:244), so
            # that helper rounds a double-precision h_eff to single unless the GLOBAL precision is double as well: give it the
            # block's precision, which is what config.precision = "double" does
            blk = cls(rg, sm, precision=prec)
            blk._remove_nulled_scs = ofdm.RemoveNulledSubcarriers(rg, precision=prec)
            return blk

        for prec, tag in (("single", "32"), ("double", "64")):
            if name == "eye":
                res["eye" + tag] = np.asarray(block(po.EyePrecodedChannel, prec)(h, p))
            else:
                res["rzf" + tag] = np.asarray(block(po.RZFPrecodedChannel, prec)(h, p, h_hat=h_hat, alpha=alpha))
                res["cbf" + tag] = np.asarray(block(po.CBFPrecodedChannel, prec)(h, p, h_hat=h_hat))
        fams = ["eye"] if name == "eye" else ["rzf", "cbf"]
        for fam in fams:
            assert res[fam + "32"].dtype == np.complex64 and res[fam + "64"].dtype == np.complex128
            note(fam, res[fam + "32"], res[fam + "64"])
            o[f"h_eff_{fam}32"], o[f"h_eff_{fam}64"] = res[fam + "32"], res[fam + "64"]
        h_eff = res[fams[0] + "32"]                                          # float32-representable: both precisions read it
        h_eff_hat = None
        if name == "mc":                                                     # what a receiver that knows h_hat only expects
            h_eff_hat = np.asarray(po.RZFPrecodedChannel(rg, sm)(h_hat, p, alpha=alpha))
            o["h_eff_hat"] = h_eff_hat
        for wh, wtag in ((True, "w"), (False, "u")):
            for prec, tag in (("single", "32"), ("double", "64")):
                blk = eq.LMMSEPostEqualizationSINR(rg, sm, precision=prec)
                o[f"sinr_{wtag}{tag}"] = np.asarray(blk(h_eff, no, interference_whitening=wh))
                if h_eff_hat is not None:
                    o[f"sinr_hat_{wtag}{tag}"] = np.asarray(blk(h_eff, no, h_eff_hat=h_eff_hat, interference_whitening=wh))
            fam = "sinr_whitened" if wh else "sinr_unwhitened"
            assert o[f"sinr_{wtag}32"].dtype == np.float32 and o[f"sinr_{wtag}64"].dtype == np.float64
            note(fam, o[f"sinr_{wtag}32"], o[f"sinr_{wtag}64"])
            if h_eff_hat is not None:
                note(fam, o[f"sinr_hat_{wtag}32"], o[f"sinr_hat_{wtag}64"])
        for k, v in o.items():
            out[f"{name}/{k}"] = v
            print(name, k, np.asarray(v).shape, np.asarray(v).dtype)
    out["cases"] = np.array([c[0] for c in CASES])
    print("\nfamily            e32 (reference single vs its own double)   4 e32 + 2^-23")
    for fam in ("rzf", "cbf", "eye", "sinr_whitened", "sinr_unwhitened"):
        out[f"e32/{fam}"] = np.float64(e32[fam])
        print(f"{fam:17s} {e32[fam]:.3e}                                   {4 * e32[fam] + 2.0 ** -23:.3e}")
    path = os.path.join(GOLD, "precoded_channel_ref_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    path = os.path.join(GOLD, "precoded_channel_api_signatures.json")
    with open(path, "w") as f:
        json.dump({"_comment": "reference signatures of the precoded channels and the post-equalisation SINR by ast "
                               "(tools/gen_precoded_channel_ref_golden.py); defaults as source text",
                   "signatures": signatures()}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
