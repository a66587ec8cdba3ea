"""Ordered-statistics decoding on the CPU: the specification tests/osd_f32.py against the reference-executed fixture
(tests/golden/osd_ref_golden.npz, tools/gen_osd_ref_golden.py), against brute-force ML, the signatures, the constructor's
argument checks, and the reference's own test_error_patterns / test_input_consistency / test_multi_dimensional
(test/unit/fec/test_linear_decoding.py:74-196) where they need no device."""
import itertools
import json
import math
import os

import numpy as np
import pytest

import osd_f32 as spec
from sionna_amd.phy.fec.linear import OSDecoder
from sionna_amd.phy.fec.utils import load_parity_check_examples, pcm2gm

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "osd_ref_golden.npz"))
CASES = [str(c) for c in G["cases"]]
STRUCT = [str(c) for c in G["struct"]]
GAP = 1e-5

HAMMING = np.array([[1, 0, 0, 0, 1, 1, 0], [0, 1, 0, 0, 1, 0, 1], [0, 0, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], np.float32)


@pytest.mark.parametrize("dtype,key", [(np.float32, "ref32"), (np.float64, "ref64")])
@pytest.mark.parametrize("name", CASES)
def test_spec_decides_like_the_reference(name, dtype, key):
    """identical decisions on every codeword whose two smallest reference distances are a relative 1e-5 apart in
    float64; at most 1 % of a case's codewords may lie under that gap"""
    p = name + "/"
    gm, t, llr, gap = G[p + "gm"], int(G[p + "t"]), G[p + "llr"], G[p + "gap"]
    close = gap < GAP
    print(name, dtype.__name__, "codewords under the gap:", int(close.sum()), "of", len(gap))
    assert close.sum() <= 0.01 * len(gap)
    got = spec.decode(llr.astype(dtype), gm, t, dtype)
    assert got.dtype == dtype
    assert np.array_equal(got[~close], G[p + key][~close].astype(dtype))


@pytest.mark.parametrize("dtype,key", [(np.float32, "struct_ref32"), (np.float64, "struct_ref64")])
@pytest.mark.parametrize("name", CASES)
def test_structured_inputs_match_exactly(name, dtype, key):
    """all-zero LLRs, noiseless +-4, |llr| = 1000 noiseless, +-100 with one sign flipped, LLRs past the float32 overflow
    of exp: the tie rules and the overflow, no exclusion"""
    p = name + "/"
    gm, t, x = G[p + "gm"], int(G[p + "t"]), G[p + "struct_llr"]
    assert len(x) == len(STRUCT) and not x[0].any() and np.all(np.abs(x[3]) == 100) and np.abs(x[4]).max() > 100
    got = spec.decode(x.astype(dtype), gm, t, dtype)
    for i, s in enumerate(STRUCT):
        assert np.array_equal(got[i], G[p + key][i]), s


def test_float32_overflow_changes_the_decision():
    """the inconsistent saturated word: float32 returns order 0 (every distance is infinite), float64 the minimum"""
    differ = 0
    for name in CASES:
        p = name + "/"
        i = STRUCT.index("sat_flip")
        differ += int(not np.array_equal(G[p + "struct_ref32"][i], G[p + "struct_ref64"][i]))
        x = G[p + "struct_llr"][i]
        pr = spec.prepare(x, G[p + "gm"], np.float32)
        key, idx, _ = spec.search(pr, int(G[p + "t"]))
        assert key == spec.INF and idx == 0
    assert differ > 0


def test_order_k_is_maximum_likelihood():
    """Hamming (7,4) with t = k = 4 against brute force over all 2^k codewords (correlation metric, float64)"""
    rng = np.random.default_rng(4)
    words = np.array([(np.array(u) @ HAMMING.astype(np.int64)) % 2 for u in itertools.product((0, 1), repeat=4)])
    llr = rng.normal(size=(200, 7)) * 2.0
    got = spec.decode(llr, HAMMING, 4, np.float64)
    ml = words[np.argmax((2 * words - 1) @ llr.T, axis=0)]
    assert np.array_equal(got, ml)
    d = spec.reference_distances(llr[0], HAMMING, 4)
    assert len(d) == 16 == 1 + spec.num_candidates(4, 4)


def test_dependent_leading_columns():
    """duplicated columns made the most reliable ones: the pivot method skips them without a special case"""
    gm = np.concatenate([HAMMING[:, :1]] * 3 + [HAMMING], axis=1)            # column 0 four times
    llr = np.array([9, -8.5, 8, 7.5, 1, -1.5, 2, -0.5, 0.25, 3], np.float32)
    p = spec.prepare(llr, gm, np.float32)
    assert sorted(p["perm"]) == list(range(10)) and len(set(p["perm"][:4]) & {0, 1, 2, 3}) == 1
    out = spec.decode(llr, gm, 1)
    assert not ((out.astype(np.int64) @ np.asarray(pcm_of(gm)).T) % 2).any()


def pcm_of(gm):
    from sionna_amd.phy.fec.utils import gm2pcm
    return gm2pcm(gm, verify_results=False)


def test_signatures_match_the_reference():
    from test_api_signatures import _check
    with open(os.path.join(GOLD, "osd_api_signatures.json")) as f:
        sig = json.load(f)["signatures"]
    assert set(sig) == {"fec.linear.OSDecoder"}
    ref = sig["fec.linear.OSDecoder"]
    _check(ref["__init__"], OSDecoder.__init__, "OSDecoder.__init__")
    _check(ref["call"], OSDecoder.call, "OSDecoder.call")
    assert [a for a, _, _ in ref["public"]] == ["gm", "n", "k", "t"]
    for attr, kind, _ in ref["public"]:
        assert isinstance(getattr(OSDecoder, attr), property), attr


def test_constructor_errors():
    """decoding.py:103-163"""
    pcm, k, n, _ = load_parity_check_examples(0)
    with pytest.raises(TypeError):
        OSDecoder(pcm, is_pcm=1)
    with pytest.raises(TypeError):
        OSDecoder(pcm, t=1.5, is_pcm=True)
    with pytest.raises(TypeError):
        OSDecoder(pcm.tolist(), is_pcm=True)
    bad = np.array(pcm)
    bad[1, 2] = 2
    with pytest.raises(TypeError):
        OSDecoder(bad)
    with pytest.raises(TypeError):
        OSDecoder(bad, is_pcm=True)
    with pytest.raises(AttributeError):
        OSDecoder()

    class NotBuilt:
        k = None
    with pytest.raises(AttributeError):
        OSDecoder(encoder=NotBuilt())
    deficient = np.array(HAMMING)
    deficient[3] = (deficient[0] + deficient[1]) % 2
    with pytest.raises(ValueError):
        OSDecoder(deficient)
    with pytest.raises(ResourceWarning):
        OSDecoder(pcm2gm(load_parity_check_examples(1)[0]), t=9)
    dec = OSDecoder(pcm, is_pcm=True, t=2)
    assert (dec.k, dec.n, dec.t) == (k, n, 2) and dec.gm.shape == (k, n)
    with pytest.raises(ValueError):
        dec.build((20, n + 1))
    dec.build((20, n))
    assert OSDecoder(pcm2gm(pcm), precision="double").gm.dtype == np.float64


def test_error_patterns():
    """test_linear_decoding.py:74-103"""
    pcm, _, _, _ = load_parity_check_examples(0)
    dec = OSDecoder(pcm, is_pcm=True)
    for n in (10, 45, 100, 250):
        for t in (1, 2, 3, 4, 5):
            if n > 50 and t > 3:
                break
            assert dec._num_error_patterns(n, t) == math.comb(n, t)
            ep = dec._gen_error_patterns(n, t)
            assert len(ep) == math.comb(n, t) and tuple(ep.shape) == (math.comb(n, t), t)
    ep = dec._gen_error_patterns(6, 3).numpy()
    assert np.array_equal(ep, spec.patterns(6, 3))


def test_input_consistency_and_multi_dimensional_on_the_spec():
    """test_linear_decoding.py:127-196 on the specification: the batch dimension is free, only the last axis is decoded"""
    pcm, k, n, _ = load_parity_check_examples(0)
    gm = pcm2gm(pcm)
    assert not spec.decode(np.zeros((3, n), np.float32), gm, 1).any()
    assert spec.decode(np.zeros((4, n), np.float32), gm, 1).shape == (4, n)
    rng = np.random.default_rng(2)
    for shape in ([n], [2, 3, 4, n], [1, 5, n]):
        llr = (rng.normal(size=shape) * 2).astype(np.float32)
        ref = spec.decode(llr.reshape(-1, n), gm, 2).reshape(shape)
        assert np.array_equal(spec.decode(llr, gm, 2), ref)


def test_import_path_under_install_as_sionna():
    import sionna_amd
    sionna_amd.install_as_sionna()
    from sionna.phy.fec.linear import OSDecoder as O
    assert O is OSDecoder
