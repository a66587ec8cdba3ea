"""Inputs and bars shared by tests/test_gpu_turbo.py (the kernels of csrc/turbo.hip on the GPU) and tests/test_turbo_host.py
(the same inputs on the CPU, so that the conditions of the bars can be checked without a GPU).

Channel LLRs are those of BPSK over AWGN, llr = m (2 c - 1) + N(0, 2 m) with m = 2 / sigma^2 = 4 Es/N0; m is chosen per
case so high that (almost) every codeword converges: a codeword that does not converge makes the float32 and the float64
specification drift apart over the iterations, which widens the anchored bar (conv_cases.anchored_bar) and with it the set
of bits whose hard decision cannot be compared.  tests/test_turbo_host.py checks that at most 1 % of the bits of a case are
lost that way."""
import functools
import zlib

import numpy as np

import turbo_f32 as spec
from conv_cases import anchored_bar
from sionna_amd.phy.fec.interleaving import qpp_perm
from sionna_amd.phy.fec.turbo import polynomial_selector

kCh = 32                                                            # steps staged per chunk (csrc/bcjr_core.h)
GEN_POLY_8 = ("10011011", "11100101")                               # constraint length 8: two trellis states per lane
MAX_SKIPPED = 0.01


def cw_per_wave(K):
    return 64 // min(2**(K - 1), 64)


# (id, K or gen_poly, rate, terminate, k, B, num_iter, m)
def _cases():
    c = []
    for K in (3, 4, 5, 6):                                          # 16 .. 2 codewords per wave; batch G + 1
        c.append((f"K{K}", K, 1/3, K % 2 == 0, 40, cw_per_wave(K) + 1, 6, 3.0))
    c.append(("K8", GEN_POLY_8, 1/3, True, 40, 3, 2, 1.5))          # float32 map underflows with 7 memory bits at more confidence
    c.append(("k41pruned", 4, 1/3, True, 41, 7, 6, 3.0))            # batch G - 1
    for k in (kCh - 1, kCh, kCh + 1):
        c.append((f"k{k}", 4, 1/3, False, k, 1, 6, 3.0))
    c.append(("T128", 4, 1/3, True, 125, 3, 6, 3.0))                # the alphas still in LDS in float32 ...
    c.append(("T129", 4, 1/3, True, 126, 3, 6, 3.0))                # ... and in the workspace
    c.append(("T64", 5, 1/2, False, 64, 3, 6, 4.0))                 # the same switch in float64
    c.append(("T65", 5, 1/2, False, 65, 3, 6, 4.0))                 # k odd: a last incomplete puncturing period
    c.append(("r2T", 4, 1/2, True, 43, 9, 6, 4.0))                  # rate 1/2 terminated, an odd number of rows
    c.append(("iter1", 4, 1/3, True, 40, 9, 1, 3.0))
    c.append(("k6144", 4, 1/3, True, 6144, 3, 2, 3.0))
    return c


CASES = _cases()
BY_ID = {c[0]: c for c in CASES}
SOFT_IDS = [c[0] for c in CASES]
# k = 6144 is compared for map (and maxlog) only: the specification loops over the trellis in Python
SOFT_PAIRS = [(c, a) for c in SOFT_IDS for a in ("map", "log") if not (c == "k6144" and a == "log")]
BIG_BATCH = ("grid", 4, 1/3, True, 40, 8 * 2048 + 3, 2, 3.0)         # 2049 waves, several per compute unit


def gen_poly_of(code):
    return polynomial_selector(code) if isinstance(code, int) else code


def draw(case):
    """u [B, k], codeword c [B, n], llr [B, n] float32 and the 3GPP permutation of one case"""
    cid, code, rate, term, k, B, _, m = case
    gp = gen_poly_of(code)
    rng = np.random.default_rng(zlib.crc32(repr((cid, k, B)).encode()))
    perm = qpp_perm(k)
    u = rng.integers(0, 2, (B, k)).astype(np.float32)
    c = spec.encode(u, gp, perm, rate, term).astype(np.float32)
    llr = (m * (2 * c - 1) + rng.normal(size=c.shape) * np.sqrt(2 * m)).astype(np.float32)
    return gp, perm, u, c, llr


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """drawn once and shared: leave them unchanged"""
    return draw(BY_ID[cid] if cid != "grid" else BIG_BATCH)


@functools.lru_cache(maxsize=None)
def refs(cid, alg):
    """(spec32, spec64) soft outputs of the specification, computed once and shared: leave them unchanged"""
    _, _, rate, term, _, _, it, _ = BY_ID[cid]
    gp, perm, _, _, llr = inputs(cid)
    r32 = spec.decode(llr, gp, perm, rate, term, it, False, alg)
    r64 = spec.decode(llr, gp, perm, rate, term, it, False, alg, dtype=np.float64)
    return r32, r64


def bar_and_mask(cid, alg):
    """per codeword bar [B] of the soft outputs against spec64, and the mask [B, k] of the bits whose hard decision can be
    compared (|spec64| above the bar)"""
    r32, r64 = refs(cid, alg)
    bar = anchored_bar(r32, r64)
    return bar, np.abs(r64) > bar[:, None]
