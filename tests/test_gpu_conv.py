"""The convolutional-code kernels on the MI355X (csrc/conv.hip) against the specification tests/conv_f32.py: the encoder,
Viterbi and BCJR maxlog bit for bit, BCJR map / log within the bar of conv_f32.llr_bar with identical hard decisions
beyond it; every code of polynomial_selector, RSC, termination, a custom gen_poly, all batch-size classes, the workspace
paths, double precision, multi-dimensional inputs, and the reference's own test vectors."""
import os

import numpy as np
import pytest
import torch

import conv_f32 as spec

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V = np.load(os.path.join(GOLD, "conv_ref_vectors.npz"))
CODES = [(r, K) for r in (1/2, 1/3) for K in range(3, 9)]


def conv():
    import sionna_amd.phy.fec.conv as c
    return c


def noisy(rng, c, snr=1.6):
    return ((2 * np.asarray(c, np.float64) - 1) * 2.0 + rng.normal(size=np.shape(c)) * snr).astype(np.float32)


def check_soft(got, ref, llr, la=None):
    bar = spec.llr_bar(llr, la)[:, None]
    assert np.all(np.abs(got - ref) <= bar), float(np.max(np.abs(got - ref)))
    sure = np.abs(ref) > bar
    assert np.array_equal((got > 0)[sure], (ref > 0)[sure])


@pytest.mark.parametrize("rate,K", CODES)
@pytest.mark.parametrize("rsc", [False, True])
@pytest.mark.parametrize("terminate", [False, True])
def test_kernels_match_the_specification(rate, K, rsc, terminate):
    c_ = conv()
    rng = np.random.default_rng(K * 10 + rsc * 2 + terminate)
    B, k = 37, 61                                                   # odd, not a multiple of the codewords per wave
    enc = c_.ConvEncoder(rate=rate, constraint_length=K, rsc=rsc, terminate=terminate)
    u = rng.integers(0, 2, (B, k)).astype(np.float32)
    c = enc(u).cpu().numpy()
    gp = enc.gen_poly
    assert np.array_equal(c, spec.encode(u, gp, rsc, terminate))
    llr = noisy(rng, c)
    for method in ("soft_llr", "hard"):
        x = llr if method == "soft_llr" else (llr > 0).astype(np.float32) + 2 * rng.integers(-1, 2, llr.shape)
        for rib in (True, False):
            dec = c_.ViterbiDecoder(encoder=enc, method=method, return_info_bits=rib)
            got = dec(x).cpu().numpy()
            assert np.array_equal(got, spec.viterbi(x, gp, rsc, terminate, method, rib)), (method, rib)
    la = (rng.normal(size=(B, c.shape[1] // len(gp))) * 1.5).astype(np.float32)
    for alg in ("map", "log", "maxlog"):
        for a in (None, la):
            dec = c_.BCJRDecoder(encoder=enc, algorithm=alg, hard_out=False)
            got = dec(llr, llr_a=a).cpu().numpy()
            ref = spec.bcjr(llr, gp, rsc, terminate, alg, hard_out=False, llr_a=a)
            if alg == "maxlog":
                assert np.array_equal(got, ref), (alg, a is None)
            else:
                check_soft(got, ref, llr, a)
        hard = c_.BCJRDecoder(encoder=enc, algorithm=alg)(llr).cpu().numpy()
        assert set(np.unique(hard)) <= {0.0, 1.0}


def test_custom_gen_poly_and_rate_one_quarter():
    c_ = conv()
    rng = np.random.default_rng(3)
    for gp, term in ((("1101", "1011", "0111"), True), (("101", "111", "111", "111"), False), (("10011", "11101"), False)):
        enc = c_.ConvEncoder(gen_poly=gp, terminate=term)
        u = rng.integers(0, 2, (9, 40)).astype(np.float32)
        c = enc(u).cpu().numpy()
        assert np.array_equal(c, spec.encode(u, gp, False, term))
        llr = noisy(rng, c)
        dec = c_.ViterbiDecoder(gen_poly=gp, terminate=term)
        assert np.array_equal(dec(llr).cpu().numpy(), spec.viterbi(llr, gp, False, term))
        for alg in ("map", "maxlog"):
            got = c_.BCJRDecoder(gen_poly=gp, terminate=term, algorithm=alg, hard_out=False)(llr).cpu().numpy()
            ref = spec.bcjr(llr, gp, False, term, alg, hard_out=False)
            if alg == "maxlog":
                assert np.array_equal(got, ref)
            else:
                check_soft(got, ref, llr)


@pytest.mark.parametrize("K", [3, 5, 7, 8])
@pytest.mark.parametrize("B", [0, 1, 3, 5, 17, 64, 129])
def test_batch_sizes(K, B):
    c_ = conv()
    rng = np.random.default_rng(B + K)
    enc = c_.ConvEncoder(rate=1/2, constraint_length=K)
    u = rng.integers(0, 2, (B, 20)).astype(np.float32)
    c = enc(u).cpu().numpy()
    assert c.shape == (B, 40)
    llr = noisy(rng, c)
    got = c_.ViterbiDecoder(encoder=enc)(llr).cpu().numpy()
    assert got.shape == (B, 20) and np.array_equal(got, spec.viterbi(llr, enc.gen_poly))
    got = c_.BCJRDecoder(encoder=enc, algorithm="maxlog", hard_out=False)(llr).cpu().numpy()
    assert got.shape == (B, 20) and np.array_equal(got, spec.bcjr(llr, enc.gen_poly, algorithm="maxlog", hard_out=False))


@pytest.mark.parametrize("K", [3, 8])
def test_long_codewords_take_the_workspace_path(K):
    """Viterbi keeps the decision bits in LDS up to 32 KB per wave (T <= 4096 steps, 2048 for K = 8), BCJR the alphas
    up to 32 KB (T <= 128 float, 64 for K = 8): these lengths run from the device workspace"""
    c_ = conv()
    from sionna_amd import _ffi
    rng = np.random.default_rng(K)
    k = 5000
    B = 6
    enc = c_.ConvEncoder(rate=1/2, constraint_length=K, terminate=True)
    u = rng.integers(0, 2, (B, k)).astype(np.float32)
    c = enc(u).cpu().numpy()
    T = c.shape[1] // 2
    assert _ffi.lib().samd_conv_workspace_bytes(0, K, T, B, 0) > 0
    assert _ffi.lib().samd_conv_workspace_bytes(1, K, T, B, 0) > 0
    assert _ffi.lib().samd_conv_workspace_bytes(1, K, 20, B, 0) == 0
    llr = noisy(rng, c)
    assert np.array_equal(c_.ViterbiDecoder(encoder=enc)(llr).cpu().numpy(), spec.viterbi(llr, enc.gen_poly, terminate=True))
    for alg in ("map", "maxlog"):
        got = c_.BCJRDecoder(encoder=enc, algorithm=alg, hard_out=False)(llr).cpu().numpy()
        ref = spec.bcjr(llr, enc.gen_poly, terminate=True, algorithm=alg, hard_out=False)
        if alg == "maxlog":
            assert np.array_equal(got, ref)
        else:
            check_soft(got, ref, llr)


def test_double_precision():
    c_ = conv()
    rng = np.random.default_rng(11)
    enc = c_.ConvEncoder(rate=1/3, constraint_length=6, terminate=True, precision="double")
    u = rng.integers(0, 2, (13, 50)).astype(np.float64)
    c = enc(u)
    assert c.dtype == torch.float64
    llr = noisy(rng, c.cpu().numpy()).astype(np.float64)
    gp = enc.gen_poly
    got = c_.ViterbiDecoder(encoder=enc, precision="double")(llr)
    assert got.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), spec.viterbi(llr, gp, terminate=True, dtype=np.float64))
    for alg in ("map", "log", "maxlog"):
        got = c_.BCJRDecoder(encoder=enc, algorithm=alg, hard_out=False, precision="double")(llr).cpu().numpy()
        ref = spec.bcjr(llr, gp, terminate=True, algorithm=alg, hard_out=False, dtype=np.float64)
        if alg == "maxlog":
            assert np.array_equal(got, ref)
        else:
            assert np.all(np.abs(got - ref) <= 1e-9 * (1 + np.abs(llr).sum(-1))[:, None])


def test_multi_dimensional_inputs_and_rebuild():
    c_ = conv()
    rng = np.random.default_rng(5)
    enc = c_.ConvEncoder(rate=1/2, constraint_length=4)
    dec = c_.ViterbiDecoder(encoder=enc)
    bcjr = c_.BCJRDecoder(encoder=enc, algorithm="log")
    u = rng.integers(0, 2, (2, 3, 4, 30)).astype(np.float32)
    c = enc(u)
    assert tuple(c.shape) == (2, 3, 4, 60)
    llr = noisy(rng, c.cpu().numpy())
    flat = llr.reshape(-1, 60)
    assert np.array_equal(dec(llr).cpu().numpy().reshape(-1, 30), spec.viterbi(flat, enc.gen_poly))
    assert np.array_equal(bcjr(llr).cpu().numpy().reshape(-1, 30), spec.bcjr(flat, enc.gen_poly, algorithm="log"))
    u2 = rng.integers(0, 2, (5, 44)).astype(np.float32)             # k changes: the encoder and the decoders rebuild
    c2 = enc(u2)
    assert enc.k == 44 and tuple(c2.shape) == (5, 88)
    assert np.array_equal(dec(-10.0 * (1 - 2 * c2)).cpu().numpy(), u2) and dec.n == 88
    assert np.array_equal(bcjr(-10.0 * (1 - 2 * c2)).cpu().numpy(), u2) and bcjr.k == 44


@pytest.mark.parametrize("rsc", [False, True])
@pytest.mark.parametrize("terminate", [False, True])
def test_noise_free_identity(rsc, terminate):
    c_ = conv()
    rng = np.random.default_rng(7)
    for rate, K in CODES:
        enc = c_.ConvEncoder(rate=rate, constraint_length=K, rsc=rsc, terminate=terminate)
        u = rng.integers(0, 2, (10, 33)).astype(np.float32)
        c = enc(u)
        llr = 20.0 * (2 * c - 1)
        assert np.array_equal(c_.ViterbiDecoder(encoder=enc)(llr).cpu().numpy(), u)
        assert np.array_equal(c_.ViterbiDecoder(encoder=enc, method="hard")(c).cpu().numpy(), u)
        assert np.array_equal(c_.ViterbiDecoder(encoder=enc, return_info_bits=False)(llr).cpu().numpy(), c.cpu().numpy())
        for alg in ("map", "log", "maxlog"):
            assert np.array_equal(c_.BCJRDecoder(encoder=enc, algorithm=alg)(llr).cpu().numpy(), u), alg


@pytest.mark.parametrize("tag,gp", [("half_57", ("101", "111")), ("half_6474", ("1101", "1111")),
                                    ("onethird_577", ("101", "111", "111")), ("onefourth_5777", ("101", "111", "111", "111"))])
def test_reference_vectors_on_the_gpu(tag, gp):
    """the reference's test_ref_implementation of both decoders (test_conv_decoding.py:218-243, 498-524)"""
    c_ = conv()
    from sionna_amd.phy.utils import ebnodb2no
    y, uhat = V[tag + "/y"], V[tag + "/uhat"]
    no = ebnodb2no(4.95, num_bits_per_symbol=2, coderate=1.)
    got = c_.ViterbiDecoder(gen_poly=gp, method="soft_llr")((2 * y / no).astype(np.float32)).cpu().numpy()
    assert np.array_equal(got, uhat)
    got = c_.BCJRDecoder(gen_poly=gp)((0.5 * (y + 1)).astype(np.float32)).cpu().numpy()
    assert np.array_equal(got, uhat)
    c = c_.ConvEncoder(gen_poly=gp)(V[tag + "/u"].astype(np.float32)).cpu().numpy()
    assert np.array_equal(c, spec.encode(V[tag + "/u"], gp))


def test_device_tensors_in_and_out():
    c_ = conv()
    from sionna_amd import _ffi
    enc = c_.ConvEncoder(rate=1/2, constraint_length=5)
    u = torch.randint(0, 2, (8, 100), device=_ffi.device()).float()
    c = enc(u)
    assert c.is_cuda
    out = c_.ViterbiDecoder(encoder=enc)(20.0 * (2 * c - 1))
    assert out.is_cuda and torch.equal(out, u)
