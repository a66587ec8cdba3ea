#!/usr/bin/env python3
"""Generates the fixtures of the discrete channels by EXECUTING the reference's own channel/discrete_channel.py under the
NumPy stand-in for TensorFlow (tools/ref_exec):
  tests/golden/discrete_ref_golden.npz
    (a) the deterministic part: _sample_errors replaced by a recorded 0/1 pattern (the same pattern as e0 and e1), all
        four channels, binary and bipolar, hard and LLR, single and double precision on the same float32-representable
        pb, pb as scalar / per position / full shape / [..., 2], pb values 0, 1, 0.5, 1e-7, 0.99 and the pair
        (0.01, 0.99), llr_max 20 and 100, and the integer dtypes (hard outputs): x, pb, the pattern and y;
    (b) the law: the reference's own _sample_errors under the stand-in's generator, 2e5 draws per pb in
        {0, 1e-3, 0.1, 0.5, 0.95, 1}: the number of events.
  tests/golden/discrete_api_signatures.json   the four classes' signatures read with ast as tools/gen_api_signatures.py does
Run here (needs /root/reference); the fixtures travel."""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

SHAPE = (2, 3, 8)
CLASSES = {"bmc": "BinaryMemorylessChannel", "bsc": "BinarySymmetricChannel", "z": "BinaryZChannel", "bec": "BinaryErasureChannel"}
VALUES = [0.0, 1.0, 0.5, 1e-7, 0.99]
PAIRS = [(0.01, 0.99), (0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (1e-7, 0.99), (0.1, 0.4), (0.0, 0.5)]
LAW_PB = [0.0, 1e-3, 0.1, 0.5, 0.95, 1.0]
LAW_N = 200000
INT_DTYPES = ("int8", "uint8", "int16", "int32", "int64")


def load_ref():
    from tools.ref_exec.loader import reference
    ref = reference()
    ref.load_utils()
    return ref.load("sionna.phy.channel.discrete_channel")


def pb_forms(rng, channel):
    """(form name, pb as handed to the block) - every value float32-representable, so that the single and the double run of
    the reference see the same probabilities"""
    f32 = lambda a: np.asarray(a, np.float32)
    pool = f32(VALUES + [0.01, 0.1, 0.3, 0.7])
    if channel == "bmc":
        forms = [(f"pair{i}", f32(p)) for i, p in enumerate(PAIRS)]
        forms.append(("position2", rng.choice(pool, SHAPE[-1:] + (2,))))
        forms.append(("full2", rng.choice(pool, SHAPE + (2,))))
        return forms
    forms = [(f"scalar{i}", f32(v)) for i, v in enumerate(VALUES)]
    forms.append(("position", rng.choice(pool, SHAPE[-1:])))
    forms.append(("full", rng.choice(pool, SHAPE)))
    return forms


def run(mod, channel, x, pb, pattern, bipolar, llrs, llr_max, precision):
    ch = getattr(mod, CLASSES[channel])(return_llrs=llrs, bipolar_input=bipolar, llr_max=llr_max, precision=precision)
    ch._built = True           # build() only validates, and reads the stand-in's shape tuples as "a tuple of two scalars"
    ch._sample_errors = lambda pb_, shape: np.array(pattern, np.float32).view(type(mod.tf.constant(0.)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(ch(x, pb))


def signatures():
    from tools.gen_api_signatures import params
    rel = "channel/discrete_channel.py"
    tree = ast.parse(open(os.path.join("/root/reference/src/sionna/phy", rel)).read())
    table = {}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in CLASSES.values():
            entry = {"kind": "class", "public": []}
            for item in node.body:
                if isinstance(item, ast.FunctionDef) and item.name in ("__init__", "call", "__call__"):
                    entry[item.name] = params(item)
                if isinstance(item, ast.FunctionDef) and not item.name.startswith("_") and item.name not in ("call", "build"):
                    is_prop = any(isinstance(d, ast.Name) and d.id == "property" for d in item.decorator_list)
                    if is_prop:
                        entry["public"].append([item.name, "property", None])
            table["channel." + node.name] = dict(entry, file=rel)
    return table


def main():
    mod = load_ref()
    rng = np.random.default_rng(20261020)
    out, meta = {}, []
    bits = rng.integers(0, 2, SHAPE)
    pattern = rng.integers(0, 2, SHAPE).astype(np.uint8)
    out["bits"], out["pattern"] = bits.astype(np.uint8), pattern
    for channel in CLASSES:
        for bipolar in (False, True):
            x = (2 * bits - 1) if bipolar else bits
            for llrs in (False, True):
                for form, pb in pb_forms(rng, channel):
                    for llr_max in (20.0, 100.0):
                        if not llrs and llr_max != 100.0:
                            continue
                        key = f"c{len(meta)}"
                        y32 = run(mod, channel, x.astype(np.float32), pb, pattern, bipolar, llrs, llr_max, "single")
                        y64 = run(mod, channel, x.astype(np.float64), pb.astype(np.float64), pattern, bipolar, llrs, llr_max, "double")
                        assert y32.dtype == np.float32 and y64.dtype == np.float64 and y32.shape == SHAPE
                        out[key + "/pb"], out[key + "/y32"], out[key + "/y64"] = pb, y32, y64
                        meta.append(dict(key=key, channel=channel, bipolar=bipolar, llrs=llrs, llr_max=llr_max, form=form, dtype="float"))
    # integer dtypes: hard outputs; the pattern decides, pb only has to pass the reference's casts
    for channel in CLASSES:
        for bipolar in (False, True):
            for dt in INT_DTYPES:
                if dt == "uint8" and (bipolar or channel == "bec"):
                    continue
                x = ((2 * bits - 1) if bipolar else bits).astype(dt)
                pb = np.asarray((0.5, 0.5) if channel == "bmc" else 0.5, np.float32)
                y = run(mod, channel, x, pb, pattern, bipolar, False, 100.0, "single")
                assert y.dtype == np.dtype(dt), (channel, dt, y.dtype)
                key = f"c{len(meta)}"
                out[key + "/pb"], out[key + "/y"] = pb, y
                meta.append(dict(key=key, channel=channel, bipolar=bipolar, llrs=False, llr_max=100.0, form="int", dtype=dt))
    out["meta"] = np.array(json.dumps(meta))
    # (b) the law of the reference's own sampler
    ch = mod.BinarySymmetricChannel()
    counts = []
    for p in LAW_PB:
        with np.errstate(divide="ignore"):
            e = np.asarray(ch._sample_errors(mod.tf.constant(p, mod.tf.float32), [LAW_N]))
        assert set(np.unique(e)) <= {0.0, 1.0}
        counts.append(int(e.sum()))
        print(f"law pb={p}: {counts[-1]} of {LAW_N}")
    out["law_pb"], out["law_n"], out["law_counts"] = np.array(LAW_PB), np.int64(LAW_N), np.array(counts, np.int64)

    # the specification on the recorded pattern, here as a report (tests/test_discrete_host.py asserts it)
    import discrete_f32 as spec
    worst = 0
    for m in meta:
        k = m["key"]
        kind = spec.ERASURE if m["channel"] == "bec" else spec.MEMORYLESS
        for prec in (("32", "64") if m["dtype"] == "float" else ("",)):
            y = out[k + "/y" + prec]
            x = ((2 * bits - 1) if m["bipolar"] else bits).astype(y.dtype)
            b0, b1 = spec_pb(spec, m["channel"], out[k + "/pb"], x)
            got, _ = spec.apply(x, b0, b1, pattern, kind, m["bipolar"], m["llrs"], m["llr_max"], pattern=True)
            same = np.array_equal(got, y, equal_nan=True)
            worst += not same and not m["llrs"]
    print(f"{len(meta)} cases, hard outputs differing from the specification: {worst}")
    path = os.path.join(GOLD, "discrete_ref_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    path = os.path.join(GOLD, "discrete_api_signatures.json")
    with open(path, "w") as f:
        json.dump({"_comment": "reference signatures of channel/discrete_channel.py by ast (tools/gen_discrete_ref_golden.py); defaults as source text",
                   "signatures": signatures()}, f, indent=1)
    print("wrote", path)


def spec_pb(spec, channel, pb, x):
    """pb0 / pb1 per element of x in the compute dtype, from pb as the block was given it"""
    P = spec.compute_dtype(x.dtype)
    pb = np.asarray(pb, P)
    if channel == "bmc":
        return spec.per_element(x.shape, pb[..., 0]), spec.per_element(x.shape, pb[..., 1])
    b1 = spec.per_element(x.shape, pb)
    return (b1 if channel == "bsc" else np.zeros_like(b1)), b1


if __name__ == "__main__":
    main()
