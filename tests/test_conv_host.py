"""Convolutional codes on the CPU: the specification tests/conv_f32.py against the reference-executed fixture
(tests/golden/conv_ref_golden.npz, tools/gen_conv_ref_golden.py) and the reference's own test vectors
(conv_ref_vectors.npz), the host trellis, the signatures, the argument checks and the import path; and the preconditions of
the anchored bar of tests/test_gpu_conv_edges.py (tests/conv_cases.py) on the inputs that module draws."""
import json
import os

import numpy as np
import pytest

import conv_cases as cc
import conv_f32 as spec
from sionna_amd.phy.fec.conv import BCJRDecoder, ConvEncoder, Trellis, ViterbiDecoder, polynomial_selector

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "conv_ref_golden.npz"))
V = np.load(os.path.join(GOLD, "conv_ref_vectors.npz"))
CASES = [str(c) for c in G["cases"]]
VECTORS = [("half_57", ("101", "111")), ("half_6474", ("1101", "1111")), ("onethird_577", ("101", "111", "111")),
           ("onefourth_5777", ("101", "111", "111", "111"))]


def _case(name):
    p = name + "/"
    return tuple(str(x) for x in G[p + "gen_poly"]), bool(G[p + "rsc"]), bool(G[p + "terminate"]), p


def test_every_selector_code_is_in_the_fixture():
    assert len(CASES) == 2 * 6 * 4 + 2
    for rate in (1/2, 1/3):
        for K in range(3, 9):
            assert len(polynomial_selector(rate, K)) == round(1 / rate)


@pytest.mark.parametrize("name", CASES)
def test_trellis_tables_match_the_reference(name):
    gp, rsc, _, p = _case(name)
    tr = Trellis(gp, rsc=rsc)
    for a in ("to_nodes", "from_nodes", "op_mat", "op_by_tonode", "ip_by_tonode", "op_by_fromnode"):
        assert np.array_equal(getattr(tr, a), G[p + "trellis_" + a]), a


@pytest.mark.parametrize("name", CASES)
def test_encoder_spec_bit_exact(name):
    gp, rsc, term, p = _case(name)
    assert np.array_equal(spec.encode(G[p + "u"], gp, rsc, term), G[p + "c"])


@pytest.mark.parametrize("name", CASES)
def test_viterbi_spec_bit_exact(name):
    gp, rsc, term, p = _case(name)
    llr = G[p + "llr"]
    cn = len(gp)
    for method in ("soft_llr", "hard"):
        x = llr if method == "soft_llr" else (llr > 0).astype(np.float32)
        assert np.array_equal(spec.viterbi(x, gp, rsc, term, method), G[p + f"vit_{method}"]), method
        # the reference returns the path's output symbols reshaped to [-1, n] (decoding.py:446-451); this build returns
        # their bits [.., n]: the same symbols, packed
        cw = spec.viterbi(x[:cn], gp, rsc, term, method, return_info_bits=False).astype(np.int64)
        syms = (cw.reshape(cn, -1, cn) << np.arange(cn - 1, -1, -1)).sum(-1)
        assert np.array_equal(syms.reshape(-1), G[p + f"vit_{method}_cw"].reshape(-1)), method


@pytest.mark.parametrize("name", CASES)
def test_bcjr_spec_against_reference(name):
    gp, rsc, term, p = _case(name)
    llr, la = G[p + "llr"], G[p + "llr_a"]
    for alg in ("map", "log", "maxlog"):
        for suffix, a in (("", None), ("_a", la)):
            got = spec.bcjr(llr, gp, rsc, term, alg, hard_out=False, llr_a=a)
            ref = G[p + f"bcjr_{alg}{suffix}"]
            if alg == "maxlog":
                assert np.array_equal(got, ref), (alg, suffix)
            else:
                bar = spec.llr_bar(llr, a)[:, None]
                assert np.all(np.abs(got - ref) <= bar), (alg, suffix, np.max(np.abs(got - ref)))
                sure = np.abs(ref) > bar
                assert np.array_equal((got > 0)[sure], (ref > 0)[sure])


def _no():
    from sionna_amd.phy.utils import ebnodb2no
    return ebnodb2no(4.95, num_bits_per_symbol=2, coderate=1.)


@pytest.mark.parametrize("tag,gp", VECTORS)
def test_spec_reproduces_the_reference_test_vectors(tag, gp):
    """test_conv_decoding.py::test_ref_implementation of both decoders: 2 y / no for Viterbi, 0.5 (y + 1) for BCJR"""
    y, uhat = V[tag + "/y"], V[tag + "/uhat"]
    assert np.array_equal(spec.encode(V[tag + "/u"], gp), spec.encode(V[tag + "/u"], gp))
    yv = (2 * y / _no()).astype(np.float32)
    assert np.array_equal(spec.viterbi(yv, gp), uhat)
    yb = (0.5 * (y + 1)).astype(np.float32)
    assert np.array_equal(spec.bcjr(yb, gp), uhat)


def test_spec_double_precision_agrees_with_single():
    gp, rsc, term, p = _case("r2K5ffT")
    llr = G[p + "llr"]
    assert np.array_equal(spec.viterbi(llr, gp, rsc, term, dtype=np.float64), G[p + "vit_soft_llr"])
    d = spec.bcjr(llr, gp, rsc, term, "map", hard_out=False, dtype=np.float64)
    assert np.all(np.abs(d - G[p + "bcjr_map"]) <= spec.llr_bar(llr)[:, None])


@pytest.mark.parametrize("alg,factor", [("map", 100.), ("log", 10.)])
@pytest.mark.parametrize("case", cc.SOFT_CASES, ids=cc.case_id)
def test_anchor_of_the_soft_bar_is_far_below_llr_bar(case, alg, factor):
    """the float32 specification lies within llr_bar / 100 (map) and llr_bar / 10 (log) of its float64 instantiation on
    every input of test_gpu_conv_edges.py, so the anchored bar 2 max |ref32 - ref64| + ulp stays below llr_bar"""
    _, _, _, llr, la = cc.inputs(case)
    for with_a, (r32, r64) in cc.refs(case, alg).items():
        assert r32.dtype == np.float32 and r64.dtype == np.float64
        assert np.all(np.isfinite(r32)) and np.all(np.isfinite(r64))
        bar = spec.llr_bar(llr, la if with_a else None)
        err = np.max(np.abs(r32.astype(np.float64) - r64), axis=-1)
        assert np.all(factor * err < bar), (with_a, float(np.max(err / bar)))
        assert np.all(cc.anchored_bar(r32, r64) < bar)


def test_map_strong_amp_is_the_largest_finite_one():
    """float32 map under strong LLRs: exp(bm) leaves the float32 range; MAP_STRONG_AMP is the largest amplitude of
    MAP_AMPS at which the specification is finite on every STRONG case, with and without llr_a"""
    finite = {amp: all(np.all(np.isfinite(r32)) for case in cc.STRONG for r32, _ in cc.refs(case, "map", amp).values())
              for amp in cc.MAP_AMPS + cc.STRONG_AMPS}
    assert max(a for a in cc.MAP_AMPS if finite[a]) == cc.MAP_STRONG_AMP
    assert not any(finite[a] for a in cc.STRONG_AMPS)


@pytest.mark.parametrize("amp", cc.STRONG_AMPS)
def test_log_spec_is_finite_under_strong_llrs(amp):
    for case in cc.STRONG:
        _, _, _, llr, la = cc.inputs(case, amp)
        for with_a, (r32, r64) in cc.refs(case, "log", amp).items():
            assert np.all(np.isfinite(r32)) and np.all(np.isfinite(r64))
            assert np.all(cc.anchored_bar(r32, r64) < spec.llr_bar(llr, la if with_a else None))


def test_spec_of_the_tail_alone():
    """k = 0 with termination: mu zero symbols, decoded to nothing"""
    for rsc in (False, True):
        c = spec.encode(np.zeros((3, 0)), ("1101", "1011"), rsc, True)
        assert c.shape == (3, 6) and not c.any()
        assert spec.viterbi(c.astype(np.float32), ("1101", "1011"), rsc, True).shape == (3, 0)
        assert spec.bcjr(c.astype(np.float32), ("1101", "1011"), rsc, True).shape == (3, 0)


def test_signatures_match_the_reference():
    from test_api_signatures import _check
    with open(os.path.join(GOLD, "conv_api_signatures.json")) as f:
        sig = json.load(f)["signatures"]
    assert set(sig) == {"fec.conv.polynomial_selector", "fec.conv.Trellis", "fec.conv.ConvEncoder",
                        "fec.conv.ViterbiDecoder", "fec.conv.BCJRDecoder"}
    import sionna_amd.phy.fec.conv as conv
    for name, ref in sig.items():
        obj = getattr(conv, name.rsplit(".", 1)[1])
        if ref["kind"] == "function":
            _check(ref["params"], obj, name)
            continue
        _check(ref["__init__"], obj.__init__, name + ".__init__")
        if ref.get("call"):
            _check(ref["call"], obj.call, name + ".call")
        for attr, kind, _ in ref["public"]:
            assert hasattr(obj, attr), (name, attr)


def test_argument_checks_raise_like_the_reference():
    """encoding.py:113-132, decoding.py:113-141, 553-578, utils.py:42-47; nothing touches a device"""
    for cls in (ConvEncoder, ViterbiDecoder, BCJRDecoder):
        with pytest.raises(ValueError):
            cls(constraint_length=9)
        with pytest.raises(ValueError):
            cls(constraint_length=2)
        with pytest.raises(ValueError):
            cls(rate=1/4)
        with pytest.raises(TypeError):
            cls(gen_poly=(101, 111))
        with pytest.raises(ValueError):
            cls(gen_poly=("101", "1111"))
        with pytest.raises(ValueError):
            cls(gen_poly=("102", "111"))
    with pytest.raises(ValueError):
        ViterbiDecoder(method="soft")
    with pytest.raises(ValueError):
        BCJRDecoder(algorithm="max")
    with pytest.raises(TypeError):
        polynomial_selector(1/2, 3.0)
    with pytest.raises(ValueError):
        polynomial_selector(1/4, 3)
    dec = ViterbiDecoder(rate=1/3, constraint_length=4)
    with pytest.raises(ValueError):
        dec.build((5, 10))                                          # n not divisible by conv_n
    dec = BCJRDecoder(rate=1/2, constraint_length=4)
    with pytest.raises(ValueError):
        dec.build((5, 11))


def test_properties_before_and_after_build():
    enc = ConvEncoder(rate=1/2, constraint_length=5, terminate=True)
    assert enc.gen_poly == ("10011", "11011") and enc.terminate and enc.k is None and enc.n is None
    enc.build((3, 100))
    assert enc.k == 100 and enc.n == 208 and abs(enc.coderate - 0.5 * 100 / 104) < 1e-15
    dec = ViterbiDecoder(encoder=enc)
    dec.build((3, 208))
    assert dec.k == 100 and dec.n == 208 and dec.trellis is enc.trellis
    dec = BCJRDecoder(gen_poly=("101", "111"))
    dec.build((3, 40))
    assert dec.k == 20 and dec.coderate == 0.5


def test_import_path_under_install_as_sionna():
    import sionna_amd
    sionna_amd.install_as_sionna()
    from sionna.phy.fec.conv import BCJRDecoder as B, ConvEncoder as C, ViterbiDecoder as V_
    assert (B, C, V_) == (BCJRDecoder, ConvEncoder, ViterbiDecoder)
