"""The convolutional-code kernels (csrc/conv.hip) where tests/test_gpu_conv.py does not look: BCJR map / log held to a
float64 anchor, hard outputs under noise, the float64 instantiations, the LDS / workspace switch and the staging-chunk
edges, 1 and 8 generator polynomials, the largest dynamic-LDS launches, degenerate and strong inputs.  Specification:
tests/conv_f32.py, in float32 and in its dtype=np.float64 instantiation; inputs and bars: tests/conv_cases.py.

A  anchored soft bar (float32 map / log): per codeword max |got - ref64| <= 2 max |ref32 - ref64| + ulp32(max |ref64|),
   asserted to lie below conv_f32.llr_bar; hard decisions identical wherever |ref64| exceeds that bar.
   Every check prints the ratio max |got - ref64| / max |ref32 - ref64| it sees (lines ANCHOR ..., pytest -rP).  No
   MI355X figure is recorded here yet: this module has not run on one.  On the CPU the float32 specification itself uses
   at most 0.55 of the bar, and a specification with the a priori LLRs scaled by 1 + 2^-16 exceeds it on every case
   with llr_a (up to 125 times for map, 5.7 for log) while staying inside llr_bar.
B  hard_out=True: maxlog array_equal with the specification, map / log equal wherever |ref64| exceeds the bar of A.
C  float64 kernels: K in {3, 5, 7, 8} x rate 1/2, 1/3 x rsc x terminate, Viterbi soft_llr / hard, both outputs, BCJR with
   and without llr_a; both sides of the float64 BCJR switch (T = 64 | 65, K = 8: 32 | 33); Viterbi at T = 2049, K = 8.
D  exact switch lengths (samd_conv_workspace_bytes 0, then positive), T in {1, 31, 32, 33, 64, 65}, k = 1, k = 0 with
   termination, 1 and 8 polynomials, the launches over 64 KB of dynamic LDS, llr_a of length k, one decoder object
   across LDS, workspace, LDS, larger workspace.
E  all-zero LLRs (every compare a tie), strong LLRs amp (2c - 1) with 5 % flipped signs.

Defects these cases caught:
| case                                          | defect                                                                |
| test_the_tail_alone (k = 0, terminate=True)   | encode() returned before the launch on k == 0 and left the mu conv_n  |
|                                               | tail bits uninitialised; ConvEncoder.call could not reshape [.., 0]   |
"""
import numpy as np
import pytest
import torch

import conv_cases as cc
import conv_f32 as spec

pytestmark = pytest.mark.gpu

ALGS = ("map", "log", "maxlog")


def conv():
    import sionna_amd.phy.fec.conv as c
    return c


def ws_bytes(decoder, K, T, B, dbl=0):
    """decoder 0 Viterbi, 1 BCJR: 0 when the survivors / alphas of T steps stay in LDS"""
    from sionna_amd import _ffi
    return _ffi.lib().samd_conv_workspace_bytes(decoder, K, T, B, dbl)


def code(r, K):
    return conv().polynomial_selector(r, K)


def check_anchored(got, r32, r64, llr, la, what):
    """bar A of the module docstring; prints the ratio it measures before it asserts"""
    assert got.dtype == np.float32 and got.shape == r32.shape
    assert np.all(np.isfinite(r32)) and np.all(np.isfinite(r64)), what
    bar = cc.anchored_bar(r32, r64)
    assert np.all(bar < spec.llr_bar(llr, la)), what
    if got.shape[-1] == 0:
        return
    err = np.max(np.abs(got.astype(np.float64) - r64), axis=-1)
    den = np.max(np.abs(r32.astype(np.float64) - r64), axis=-1)
    ratio = float(np.max(err[den > 0] / den[den > 0])) if np.any(den > 0) else 0.0
    print(f"ANCHOR {what}: max |got - ref64| {float(np.max(err)):.3e} ratio {ratio:.4f} bitwise {np.array_equal(got, r32)}")
    assert np.all(err <= bar), (what, float(np.max(err / bar)))
    sure = np.abs(r64) > bar[:, None]
    assert np.array_equal((got > 0)[sure], (r64 > 0)[sure]), what


def check_bcjr(gp, rsc, term, llr, las=(None,), algs=ALGS, what=""):
    """soft outputs of the float32 kernels: maxlog bit for bit, map / log within bar A"""
    for alg in algs:
        dec = conv().BCJRDecoder(gen_poly=gp, rsc=rsc, terminate=term, algorithm=alg, hard_out=False)
        for a in las:
            got = dec(llr, llr_a=a).cpu().numpy()
            r32 = spec.bcjr(llr, gp, rsc, term, alg, hard_out=False, llr_a=a)
            if alg == "maxlog":
                assert np.array_equal(got, r32), (what, alg, a is None)
            else:
                r64 = spec.bcjr(llr, gp, rsc, term, alg, hard_out=False, llr_a=a, dtype=np.float64)
                check_anchored(got, r32, r64, llr, a, f"{alg} {what} a={a is not None}")


def check_bcjr_f64(gp, rsc, term, llr, las=(None,), algs=ALGS, what=""):
    """float64 kernels: maxlog bit for bit, map / log within the bar of test_gpu_conv.py::test_double_precision"""
    for alg in algs:
        dec = conv().BCJRDecoder(gen_poly=gp, rsc=rsc, terminate=term, algorithm=alg, hard_out=False, precision="double")
        for a in las:
            got = dec(llr, llr_a=a)
            assert got.dtype == torch.float64
            got = got.cpu().numpy()
            ref = spec.bcjr(llr, gp, rsc, term, alg, hard_out=False, llr_a=a, dtype=np.float64)
            assert np.all(np.isfinite(ref)) and got.shape == ref.shape
            if alg == "maxlog":
                assert np.array_equal(got, ref), (what, alg, a is None)
            else:
                err = np.abs(got - ref)
                print(f"F64 {alg} {what} a={a is not None}: max error {float(np.max(err)) if err.size else 0.:.3e}")
                assert np.all(err <= 1e-9 * (1 + np.abs(llr).sum(-1))[:, None]), (what, alg, a is None)


def check_viterbi(gp, rsc, term, x, methods=("soft_llr",), precision=None, ribs=(True, False), what=""):
    dt = np.float64 if precision == "double" else np.float32
    for method in methods:
        for rib in ribs:
            dec = conv().ViterbiDecoder(gen_poly=gp, rsc=rsc, terminate=term, method=method, return_info_bits=rib,
                                        precision=precision)
            got = dec(x[method] if isinstance(x, dict) else x).cpu().numpy()
            ref = spec.viterbi(x[method] if isinstance(x, dict) else x, gp, rsc, term, method, rib, dtype=dt)
            assert got.dtype == dt and got.shape == ref.shape and np.array_equal(got, ref), (what, method, rib)


def hard_inputs(rng, llr):
    """0 / 1 decisions moved by even integers and by -2, 0, 2: what int_mod_2 has to fold back"""
    return (llr > 0).astype(llr.dtype) + 2 * rng.integers(-1, 2, llr.shape).astype(llr.dtype)


# ---------------------------------------------------------------- A, B
@pytest.mark.parametrize("alg", ["map", "log"])
@pytest.mark.parametrize("case", cc.SOFT_CASES, ids=cc.case_id)
def test_soft_outputs_within_the_anchored_bar(case, alg):
    r, K, rsc, term, B, k = case
    gp, _, c, llr, la = cc.inputs(case)
    T = c.shape[1] // len(gp)
    assert (ws_bytes(1, K, T, B) > 0) == (T > (64 if K == 8 else 128))      # SHORT: LDS, but for K = 8 terminated (T = 68)
    dec = conv().BCJRDecoder(gen_poly=gp, rsc=rsc, terminate=term, algorithm=alg, hard_out=False)
    for with_a, (r32, r64) in cc.refs(case, alg).items():
        a = la if with_a else None
        check_anchored(dec(llr, llr_a=a).cpu().numpy(), r32, r64, llr, a, f"{alg} {cc.case_id(case)} a={with_a}")


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("case", cc.SOFT_CASES, ids=cc.case_id)
def test_hard_outputs_match_the_specification(case, alg):
    r, K, rsc, term, B, k = case
    gp, _, c, llr, la = cc.inputs(case)
    T = c.shape[1] // len(gp)
    assert (ws_bytes(1, K, T, B) > 0) == (T > (64 if K == 8 else 128))      # SHORT: LDS, but for K = 8 terminated (T = 68)
    dec = conv().BCJRDecoder(gen_poly=gp, rsc=rsc, terminate=term, algorithm=alg)
    for with_a in ((True,) if case in cc.LONG else (False, True)):
        a = la if with_a else None
        got = dec(llr, llr_a=a).cpu().numpy()
        assert got.shape == (B, k) and set(np.unique(got)) <= {0.0, 1.0}
        if alg == "maxlog":
            assert np.array_equal(got, spec.bcjr(llr, gp, rsc, term, alg, hard_out=True, llr_a=a)), with_a
        else:
            r32, r64 = cc.refs(case, alg)[with_a]
            assert np.all(np.isfinite(r32)) and np.all(np.isfinite(r64))
            bar = cc.anchored_bar(r32, r64)
            assert np.all(bar < spec.llr_bar(llr, a))
            sure = np.abs(r64) > bar[:, None]
            assert np.mean(sure) > 0.99                             # the bar leaves next to nothing undecided
            assert np.array_equal(got[sure], (r64 > 0)[sure].astype(np.float32)), with_a


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("K", [3, 5, 7, 8])
@pytest.mark.parametrize("r", [1/2, 1/3], ids=["r2", "r3"])
@pytest.mark.parametrize("rsc", [False, True])
@pytest.mark.parametrize("terminate", [False, True])
def test_double_precision_matrix(K, r, rsc, terminate):
    c_ = conv()
    rng = np.random.default_rng(1000 + 16 * K + 4 * round(1 / r) + 2 * rsc + terminate)
    B, k = 2 * cc.cw_per_wave(K) + 1, 61
    enc = c_.ConvEncoder(rate=r, constraint_length=K, rsc=rsc, terminate=terminate, precision="double")
    gp = enc.gen_poly
    u = rng.integers(0, 2, (B, k)).astype(np.float64)
    c = enc(u)
    assert c.dtype == torch.float64
    c = c.cpu().numpy()
    assert np.array_equal(c, spec.encode(u, gp, rsc, terminate))
    llr = (2 * c - 1) * 2.0 + rng.normal(size=c.shape) * 1.6        # float64 noise: not representable in float32
    la = rng.normal(size=(B, c.shape[1] // len(gp))) * 1.5
    check_viterbi(gp, rsc, terminate, {"soft_llr": llr, "hard": hard_inputs(rng, llr)}, ("soft_llr", "hard"), "double")
    T = c.shape[1] // len(gp)                                       # 61 .. 68: LDS for K = 3, workspace for K = 8
    assert (ws_bytes(1, K, T, B, 1) > 0) == (T > (32 if K == 8 else 64))
    check_bcjr_f64(gp, rsc, terminate, llr, (None, la), what=f"K{K} T{T}")


@pytest.mark.parametrize("K", [3, 5, 7, 8])
def test_double_precision_bcjr_on_both_sides_of_its_switch(K):
    """float64 alphas leave LDS at T > 64 (T > 32 with two states per lane)"""
    rng = np.random.default_rng(2000 + K)
    r, rsc, B, T0 = (1/2 if K in (3, 8) else 1/3), K in (5, 8), 2 * cc.cw_per_wave(K) + 1, 32 if K == 8 else 64
    gp = code(r, K)
    for T, side in ((T0, 0), (T0 + 1, 1)):
        assert (ws_bytes(1, K, T, B, 1) > 0) == bool(side)
        c = spec.encode(rng.integers(0, 2, (B, T - (K - 1))), gp, rsc, True)
        llr = (2. * c - 1) * 2.0 + rng.normal(size=c.shape) * 1.6
        check_bcjr_f64(gp, rsc, True, llr, (None, rng.normal(size=(B, T)) * 1.5), what=f"K{K} T{T}")


def test_double_precision_viterbi_on_the_workspace_path():
    rng = np.random.default_rng(2100)
    gp, B, T = code(1/2, 8), 3, 2049
    assert ws_bytes(0, 8, T - 1, B, 1) == 0 and ws_bytes(0, 8, T, B, 1) > 0
    c = spec.encode(rng.integers(0, 2, (B, T - 7)), gp, False, True)
    llr = (2. * c - 1) * 2.0 + rng.normal(size=c.shape) * 1.6
    check_viterbi(gp, False, True, llr, precision="double")


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("K", [3, 7, 8])
def test_viterbi_at_the_exact_switch_lengths(K):
    """the survivors stay in LDS up to 32 KB per wave: T <= 4096 (2048 with two ballot words per step)"""
    rng = np.random.default_rng(3000 + K)
    gp, B, T0, term = code(1/2, K), cc.cw_per_wave(K) + 1, 2048 if K == 8 else 4096, K == 7
    for T, side in ((T0, 0), (T0 + 1, 1)):
        assert (ws_bytes(0, K, T, B) > 0) == bool(side)
        llr = cc.noisy(rng, spec.encode(rng.integers(0, 2, (B, T - (K - 1) * term)), gp, False, term))
        check_viterbi(gp, False, term, llr, what=f"T{T}")


@pytest.mark.parametrize("K", [3, 7, 8])
def test_bcjr_at_the_exact_switch_lengths(K):
    """the alphas stay in LDS up to 32 KB per wave: T <= 128 (64 with two states per lane)"""
    rng = np.random.default_rng(3100 + K)
    gp, B, T0, term = code(1/3 if K == 7 else 1/2, K), cc.cw_per_wave(K) + 1, 64 if K == 8 else 128, K != 7
    for T, side in ((T0, 0), (T0 + 1, 1)):
        assert (ws_bytes(1, K, T, B) > 0) == bool(side)
        llr = cc.noisy(rng, spec.encode(rng.integers(0, 2, (B, T - (K - 1) * term)), gp, K == 3, term))
        la = (rng.normal(size=(B, T)) * 1.5).astype(np.float32)
        check_bcjr(gp, K == 3, term, llr, (None, la), what=f"K{K} T{T}")


@pytest.mark.parametrize("K", [3, 6, 8])
@pytest.mark.parametrize("rsc", [False, True])
def test_staging_chunk_edges(K, rsc):
    """32 steps are staged at a time: T of one step, one short of a chunk, a chunk, one more, two chunks, one more;
    k = 1 is T = 1 unterminated"""
    c_ = conv()
    rng = np.random.default_rng(3200 + 2 * K + rsc)
    mu, B = K - 1, cc.cw_per_wave(K) + 1
    gp = code(1/3 if K == 6 else 1/2, K)
    for T in (1, 31, 32, 33, 64, 65):
        for term in (False, True):
            k = T - mu * term
            if k < 1:
                continue
            enc = c_.ConvEncoder(gen_poly=gp, rsc=rsc, terminate=term)
            u = rng.integers(0, 2, (B, k)).astype(np.float32)
            c = enc(u).cpu().numpy()
            assert c.shape == (B, T * len(gp)) and np.array_equal(c, spec.encode(u, gp, rsc, term))
            assert ws_bytes(0, K, T, B) == 0 and (ws_bytes(1, K, T, B) > 0) == (K == 8 and T == 65)
            llr = cc.noisy(rng, c)
            check_viterbi(gp, rsc, term, llr, what=f"T{T} term{term}")
            check_bcjr(gp, rsc, term, llr, (None, (rng.normal(size=(B, T)) * 1.5).astype(np.float32)), what=f"K{K} T{T} term{term}")


@pytest.mark.parametrize("K", [3, 6, 8])
@pytest.mark.parametrize("rsc", [False, True])
def test_the_tail_alone(K, rsc):
    """k = 0 with termination: the codeword is the mu conv_n tail bits, all zero; T = mu"""
    c_ = conv()
    from sionna_amd import _ffi
    rng = np.random.default_rng(3300 + 2 * K + rsc)
    mu, B = K - 1, cc.cw_per_wave(K) + 1
    gp = code(1/3 if K == 6 else 1/2, K)
    n = mu * len(gp)
    enc = c_.ConvEncoder(gen_poly=gp, rsc=rsc, terminate=True)
    poison = torch.full((B, n), float("nan"), device=_ffi.device())  # what the allocator hands the encoder's output next
    del poison
    c = enc(np.zeros((B, 0), np.float32))
    assert tuple(c.shape) == (B, n) and enc.k == 0 and enc.n == n
    c = c.cpu().numpy()
    assert np.array_equal(c, np.zeros((B, n), np.float32)) and np.array_equal(c, spec.encode(np.zeros((B, 0)), gp, rsc, True))
    assert tuple(enc(np.zeros((2, 3, 0), np.float32)).shape) == (2, 3, n)
    llr = cc.noisy(rng, c)
    for method in ("soft_llr", "hard"):
        x = llr if method == "soft_llr" else hard_inputs(rng, llr)
        path = c_.ViterbiDecoder(encoder=enc, method=method, return_info_bits=False)(x).cpu().numpy()
        assert np.array_equal(path, spec.viterbi(x, gp, rsc, True, method, return_info_bits=False))
        assert tuple(c_.ViterbiDecoder(encoder=enc, method=method)(x).shape) == (B, 0)
    for alg in ALGS:
        for hard in (False, True):
            assert tuple(c_.BCJRDecoder(encoder=enc, algorithm=alg, hard_out=hard)(llr).shape) == (B, 0)


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("polys", [1, 8])
def test_one_and_eight_polynomials(K, polys):
    c_ = conv()
    rng = np.random.default_rng(3400 + 10 * K + polys)
    gp = (cc.POLY_1 if polys == 1 else cc.POLY_8)[K]
    B, k = 2 * cc.cw_per_wave(K) + 1, 40
    for rsc, term in ((False, True), (True, False)):
        enc = c_.ConvEncoder(gen_poly=gp, rsc=rsc, terminate=term)
        u = rng.integers(0, 2, (B, k)).astype(np.float32)
        c = enc(u).cpu().numpy()
        assert c.shape == (B, polys * (k + (K - 1) * term)) and np.array_equal(c, spec.encode(u, gp, rsc, term))
        # eight LLRs add up per step: a quarter of the amplitude keeps the float32 specification of map finite
        llr = cc.noisy(rng, c) * np.float32(1 if polys == 1 else 0.25)
        check_viterbi(gp, rsc, term, {"soft_llr": llr, "hard": hard_inputs(rng, llr)}, ("soft_llr", "hard"))
        check_bcjr(gp, rsc, term, llr, (None, (rng.normal(size=(B, c.shape[1] // polys)) * 1.5).astype(np.float32)),
                   what=f"K{K} polys{polys} rsc{rsc}")


def test_largest_dynamic_lds():
    """8 polynomials, K = 3 (16 codewords per wave), float64: 32 KB of staged LLRs next to the 32 KB of survivors
    (66,304 B) or alphas (69,632 B) - the only launches of conv.hip above the 64 KB default"""
    rng = np.random.default_rng(3500)
    gp, B = cc.POLY_8[3], 17
    assert ws_bytes(0, 3, 4096, B, 1) == 0 and ws_bytes(1, 3, 64, B, 1) == 0
    c = spec.encode(rng.integers(0, 2, (B, 4096)), gp)
    check_viterbi(gp, False, False, (2. * c - 1) * 2.0 + rng.normal(size=c.shape) * 1.6, precision="double", ribs=(True,))
    c = spec.encode(rng.integers(0, 2, (B, 62)), gp, False, True)
    llr = (2. * c - 1) * 2.0 + rng.normal(size=c.shape) * 1.6
    check_bcjr_f64(gp, False, True, llr, (None, rng.normal(size=(B, 64)) * 1.5), what="8 polys T64")


def test_llr_a_of_length_k_is_zero_padded():
    """llr_a [..., k] on a terminated code: the mu tail steps get a priori 0"""
    rng = np.random.default_rng(3600)
    gp, B, k = code(1/2, 5), 9, 45
    llr = cc.noisy(rng, spec.encode(rng.integers(0, 2, (B, k)), gp, True, True))
    la = (rng.normal(size=(B, k)) * 1.5).astype(np.float32)
    padded = np.concatenate([la, np.zeros((B, 4), np.float32)], axis=1)
    for alg in ALGS:
        dec = conv().BCJRDecoder(gen_poly=gp, rsc=True, terminate=True, algorithm=alg, hard_out=False)
        got = dec(llr, llr_a=la).cpu().numpy()
        assert np.array_equal(got, dec(llr, llr_a=padded).cpu().numpy())
        assert not np.array_equal(got, dec(llr).cpu().numpy())
        r32 = spec.bcjr(llr, gp, True, True, alg, hard_out=False, llr_a=padded)
        if alg == "maxlog":
            assert np.array_equal(got, r32)
        else:
            r64 = spec.bcjr(llr, gp, True, True, alg, hard_out=False, llr_a=padded, dtype=np.float64)
            check_anchored(got, r32, r64, llr, padded, f"{alg} llr_a [B, k]")
    got = dec(llr.reshape(3, 3, -1), llr_a=la.reshape(3, 3, k)).cpu().numpy()
    assert np.array_equal(got.reshape(B, k), r32)


def test_one_decoder_object_across_lds_and_workspace_lengths():
    """short, workspace, short again, the workspace length with a larger batch: the block's cached workspace is taken,
    left alone, and grown"""
    c_ = conv()
    rng = np.random.default_rng(3700)
    gp = code(1/2, 8)
    vit = c_.ViterbiDecoder(gen_poly=gp)
    bcjr = {alg: c_.BCJRDecoder(gen_poly=gp, algorithm=alg, hard_out=False) for alg in ALGS}
    for B, Tv, Tb in ((3, 100, 50), (3, 2049, 65), (3, 100, 50), (7, 2049, 65)):
        assert (ws_bytes(0, 8, Tv, B) > 0) == (Tv == 2049) and (ws_bytes(1, 8, Tb, B) > 0) == (Tb == 65)
        llr = cc.noisy(rng, spec.encode(rng.integers(0, 2, (B, Tv)), gp))
        assert np.array_equal(vit(llr).cpu().numpy(), spec.viterbi(llr, gp)), (B, Tv)
        llr = cc.noisy(rng, spec.encode(rng.integers(0, 2, (B, Tb)), gp))
        la = (rng.normal(size=(B, Tb)) * 1.5).astype(np.float32)
        for alg, dec in bcjr.items():
            got = dec(llr, llr_a=la).cpu().numpy()
            r32 = spec.bcjr(llr, gp, algorithm=alg, hard_out=False, llr_a=la)
            if alg == "maxlog":
                assert np.array_equal(got, r32), (B, Tb)
            else:
                r64 = spec.bcjr(llr, gp, algorithm=alg, hard_out=False, llr_a=la, dtype=np.float64)
                check_anchored(got, r32, r64, llr, la, f"{alg} reuse B{B} T{Tb}")


# ---------------------------------------------------------------- E
@pytest.mark.parametrize("K", [3, 7, 8])
@pytest.mark.parametrize("terminate", [False, True])
def test_all_zero_llrs(K, terminate):
    """every add-compare-select is a tie and so is the final arg-min: the first predecessor, the first state"""
    B, T = cc.cw_per_wave(K) + 1, 40
    for r, rsc in ((1/2, False), (1/3, True)):
        gp = code(r, K)
        llr = np.zeros((B, T * len(gp)), np.float32)
        check_viterbi(gp, rsc, terminate, llr, what="zeros")
        for alg in ALGS:
            got = conv().BCJRDecoder(gen_poly=gp, rsc=rsc, terminate=terminate, algorithm=alg, hard_out=False)(llr).cpu().numpy()
            ref = spec.bcjr(llr, gp, rsc, terminate, alg, hard_out=False)
            assert not ref.any()
            assert np.array_equal(got + np.float32(0), ref + np.float32(0)), (alg, rsc)     # -0 + 0 = +0


@pytest.mark.parametrize("amp", cc.STRONG_AMPS)
@pytest.mark.parametrize("case", cc.STRONG, ids=cc.case_id)
def test_strong_llrs(case, amp):
    """amp (2c - 1) with 5 % of the signs flipped, llr_a ~ N(0, (amp / 4)^2): Viterbi and maxlog bit for bit, log
    within bar A (its float32 specification stays finite; map does not, see test_map_under_strong_llrs)"""
    r, K, rsc, term, B, k = case
    gp, _, _, llr, la = cc.inputs(case, amp)
    check_viterbi(gp, rsc, term, llr, what=f"amp{amp}")
    check_bcjr(gp, rsc, term, llr, (None, la), ("maxlog",), what=f"amp{amp}")
    dec = conv().BCJRDecoder(gen_poly=gp, rsc=rsc, terminate=term, algorithm="log", hard_out=False)
    for with_a, (r32, r64) in cc.refs(case, "log", amp).items():
        a = la if with_a else None
        check_anchored(dec(llr, llr_a=a).cpu().numpy(), r32, r64, llr, a, f"log strong{amp} {cc.case_id(case)} a={with_a}")


@pytest.mark.parametrize("case", cc.STRONG, ids=cc.case_id)
def test_map_under_strong_llrs(case):
    """float32 map overflows at amp = 20 by the reference's own arithmetic; MAP_STRONG_AMP is the largest of {4, 8, 12}
    at which its specification is finite on every case (decided in test_conv_host.py)"""
    assert cc.MAP_STRONG_AMP == 8
    r, K, rsc, term, B, k = case
    gp, _, _, llr, la = cc.inputs(case, cc.MAP_STRONG_AMP)
    dec = conv().BCJRDecoder(gen_poly=gp, rsc=rsc, terminate=term, algorithm="map", hard_out=False)
    for with_a, (r32, r64) in cc.refs(case, "map", cc.MAP_STRONG_AMP).items():
        a = la if with_a else None
        check_anchored(dec(llr, llr_a=a).cpu().numpy(), r32, r64, llr, a, f"map strong {cc.case_id(case)} a={with_a}")
