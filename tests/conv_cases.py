"""Inputs and bars shared by tests/test_gpu_conv_edges.py (the kernels of csrc/conv.hip on the GPU) and tests/test_conv_host.py
(the same inputs on the CPU, so that the bars can be checked without a GPU).

The anchored bar of BCJR map / log.  conv_f32.llr_bar = 1e-5 (1 + sum |llr|) is 30 to 10^5 times what float32 arithmetic
needs.  The anchor is the float32 specification's own distance from its float64 instantiation on the same inputs: per
codeword the kernel must satisfy

    max |got - ref64| <= ANCHOR_C * max |ref32 - ref64| + ulp32(max |ref64|)

ANCHOR_C = 2: the kernel performs the operations of ref32 in the same order; it can differ from ref32 only where a float64
exp / log that is 1 ulp off NumPy's lands on the other side of a float32 rounding boundary, an error of the size ref32
already carries.  The floor, one float32 ulp at the codeword's largest |ref64|, keeps a codeword whose float32
specification happens to be exact from failing for no reason.  The anchor never involves the kernel's output."""
import functools
import zlib

import numpy as np

import conv_f32 as spec
from sionna_amd.phy.fec.conv import polynomial_selector

CODES = [(r, K) for r in (1/2, 1/3) for K in range(3, 9)]
ANCHOR_C = 2.0
POLY_1 = {3: ("111",), 8: ("11100101",)}
POLY_8 = {3: ("101", "111", "110", "011", "111", "100", "101", "001"),
          8: ("11100101", "10011111", "10010101", "11011001", "11110111", "10000001", "01010101", "11111111")}


def cw_per_wave(K):
    """G of conv.hip: codewords that share one wave"""
    return 64 // min(2**(K - 1), 64)


def noisy(rng, c, snr=1.6):
    return ((2 * np.asarray(c, np.float64) - 1) * 2.0 + rng.normal(size=np.shape(c)) * snr).astype(np.float32)


def draw(gp, rsc, terminate, B, k, seed, amp=None, flip=0.05):
    """u [B, k], its codeword c, channel LLRs [B, n] and a priori LLRs [B, T], float32.  amp None: noisy(); otherwise
    the strong LLRs amp (2 c - 1) with the fraction ``flip`` of the signs inverted and llr_a ~ N(0, (amp / 4)^2)."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2, (B, k)).astype(np.float32)
    c = spec.encode(u, gp, rsc, terminate).astype(np.float32)
    T = c.shape[1] // len(gp)
    if amp is None:
        llr = noisy(rng, c)
        la = (rng.normal(size=(B, T)) * 1.5).astype(np.float32)
    else:
        sign = np.where(rng.random(c.shape) < flip, -1.0, 1.0)
        llr = (amp * (2 * c - 1) * sign).astype(np.float32)
        la = (rng.normal(size=(B, T)) * (amp / 4)).astype(np.float32)
    return u, c, llr, la


def anchored_bar(ref32, ref64, c=ANCHOR_C):
    """per codeword [B]: c max |ref32 - ref64| + one float32 ulp at max |ref64|"""
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    if ref64.shape[-1] == 0:
        return np.zeros(ref64.shape[0])
    floor = np.spacing(np.max(np.abs(ref64), axis=-1).astype(np.float32)).astype(np.float64)
    return c * np.max(np.abs(ref32 - ref64), axis=-1) + floor


def _seed(*a):
    return zlib.crc32(repr(a).encode())


# (rate, K, rsc, terminate, B, k): every selector code, k = 61, two full waves and one codeword
SHORT = [(r, K, rsc, term, 2 * cw_per_wave(K) + 1, 61) for r, K in CODES for rsc in (False, True) for term in (False, True)]
# the BCJR workspace path: T one step past the float32 switch (T = 129, 65 at K = 8) ...
JUST_OVER = [(1/2, 3, False, True, 33, 127), (1/3, 3, True, False, 33, 129), (1/2, 8, True, True, 3, 58), (1/3, 8, False, False, 3, 65)]
# ... and far past it
LONG = [(1/2, 3, False, True, 3, 5000), (1/2, 8, False, True, 3, 5000)]
SOFT_CASES = SHORT + JUST_OVER + LONG
# strong LLRs: both lane layouts with several codewords per wave, one and two states per lane
STRONG = [(1/2, K, rsc, term, 2 * cw_per_wave(K) + 1, 61) for K in (3, 7, 8) for rsc, term in ((False, True), (True, False))]
STRONG_AMPS = (20, 40)
MAP_AMPS = (4, 8, 12)
MAP_STRONG_AMP = 8               # the largest of MAP_AMPS at which the float32 specification of map is finite on every
                                 # STRONG case (test_conv_host.py::test_map_strong_amp_is_the_largest_finite_one)


def case_id(case):
    r, K, rsc, term, B, k = case
    return f"r{round(1 / r)}K{K}{'rsc' if rsc else 'ff'}{'T' if term else 'U'}-B{B}k{k}"


@functools.lru_cache(maxsize=None)
def inputs(case, amp=None):
    """gp, u, c, llr, la of one case, drawn once and shared: leave them unchanged"""
    r, K, rsc, term, B, k = case
    gp = polynomial_selector(r, K)
    return (gp,) + draw(gp, rsc, term, B, k, _seed(round(1 / r), K, rsc, term, B, k, amp), amp)


@functools.lru_cache(maxsize=None)
def refs(case, alg, amp=None):
    """specification outputs of BCJR ``alg`` on inputs(case, amp), computed once and shared, leave them unchanged:
    {with_a: (ref32, ref64)}; the far-past-the-switch cases only with llr_a (the specification loops over T in Python)"""
    _, _, rsc, term, _, _ = case
    gp, _, _, llr, la = inputs(case, amp)
    out = {}
    for with_a in ((True,) if case in LONG else (False, True)):
        a = la if with_a else None
        r32 = spec.bcjr(llr, gp, rsc, term, alg, hard_out=False, llr_a=a)
        r64 = spec.bcjr(llr, gp, rsc, term, alg, hard_out=False, llr_a=a, dtype=np.float64)
        out[with_a] = (r32, r64)
    return out
