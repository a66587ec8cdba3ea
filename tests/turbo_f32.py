"""Specification of the turbo-code kernels (csrc/turbo.hip): the reference's TurboEncoder.call and TurboDecoder.call
(src/sionna/phy/fec/turbo/encoding.py:365-421, decoding.py:254-435) restated in NumPy float32 / float64, line by line, on top
of the constituent ``encode`` and ``bcjr`` of tests/conv_f32.py.  Nothing here uses the index tables of the package
(sionna_amd/phy/fec/turbo/utils.py: turbo_tables): the codeword is assembled, punctured, depunctured and split the way the
reference does it, with explicit intermediate arrays.

maxlog involves only IEEE add, compare and sign changes: the kernels are bit-identical to this file.  map / log: see
tests/conv_f32.py."""
import math

import numpy as np

import conv_f32 as conv

LLR_MAX = 20.


def punct_mask(rows, rate):
    """[rows * 3] bool: the pattern of utils.py:71-74 tiled over the rows, a last incomplete period included
    (encoding.py:309-334, decoding.py:340-355)"""
    pattern = np.array([[1, 1, 0], [1, 0, 1]], bool) if rate == 1/2 else np.array([[1, 1, 1]], bool)
    reps = rows // pattern.shape[0]
    mask = np.tile(pattern, (reps, 1))
    extra = rows - reps * pattern.shape[0]
    if extra > 0:
        mask = np.concatenate([mask, pattern[:extra]], axis=0)
    return mask.reshape(-1)


def num_term_syms(mu):
    return math.ceil(2 * 2 * mu / 3)                                # utils.py:151-152


def encode(u, gen_poly, perm, rate=1/3, terminate=False):
    """u [B, k] 0/1 -> turbo codeword [B, n] uint8 (encoding.py:365-421)"""
    u = np.asarray(u).astype(np.int64) & 1
    B, k = u.shape
    mu = len(gen_poly[0]) - 1
    msg2 = u[:, perm]                                               # :392
    cw1_ = conv.encode(u, gen_poly, rsc=True, terminate=terminate)  # :394-395
    cw2_ = conv.encode(msg2, gen_poly, rsc=True, terminate=terminate)
    preterm_n = 2 * k
    cw1, term1 = cw1_[:, :preterm_n], cw1_[:, preterm_n:]           # :397-398
    cw2, term2 = cw2_[:, :preterm_n], cw2_[:, preterm_n:]
    cw2_par = cw2[:, 1::2]                                          # :401-402
    cw = np.concatenate([cw1.reshape(B, k, 2), cw2_par.reshape(B, k, 1)], axis=-1)      # :404-408
    if terminate:
        term = np.concatenate([term1, term2], axis=-1)              # utils.py:216-229
        S = num_term_syms(mu)
        term = np.concatenate([term, np.zeros((B, 3 * S - term.shape[1]), term.dtype)], axis=-1)
        cw = np.concatenate([cw, term.reshape(B, S, 3)], axis=-2)   # :411-414
    cw = cw.reshape(B, -1)
    return cw[:, punct_mask(cw.shape[1] // 3, rate)].astype(np.uint8)


def code_dims(n, rate, terminate, mu):
    """k of a codeword of n bits (decoding.py:321-338)"""
    if rate == 1/2 and n % 2:
        raise ValueError("Codeword length should be a multiple of 2")
    term_bits = 3 * num_term_syms(mu) if terminate else 0
    pre = int(n * (rate * 3)) - term_bits
    if pre % 3:
        raise ValueError("Invalid codeword length for a terminated Turbo code")
    return pre // 3


def split(y, gen_poly, perm, rate, terminate):
    """_convenc_cws (decoding.py:271-312): channel values [B, n] -> (y1_cw, y2_cw) [B, 2 T] of the two constituent codes"""
    B, n = y.shape
    mu = len(gen_poly[0]) - 1
    k = code_dims(n, rate, terminate, mu)
    depunct_len = int(3. * rate * n)
    mask = punct_mask(depunct_len // 3, rate)
    y_turbo = np.zeros((B, depunct_len), y.dtype)                   # depuncture :254-269
    y_turbo[:, np.flatnonzero(mask)] = y
    term_bits = 3 * num_term_syms(mu) if terminate else 0
    y_cw, y_term = y_turbo[:, :depunct_len - term_bits], y_turbo[:, depunct_len - term_bits:]
    sys1, par1, par2 = y_cw[:, 0::3], y_cw[:, 1::3], y_cw[:, 2::3]
    y1_cw = np.stack([sys1, par1], axis=-1).reshape(B, 2 * k)       # :292-295
    sys2 = sys1[:, perm]                                            # :298-300
    y2_cw = np.stack([sys2, par2], axis=-1).reshape(B, 2 * k)       # :303-305
    if terminate:                                                   # :308-311, utils.py:289-293
        y1_cw = np.concatenate([y1_cw, y_term[:, :2 * mu]], axis=1)
        y2_cw = np.concatenate([y2_cw, y_term[:, 2 * mu:4 * mu]], axis=1)
    return k, y1_cw, y2_cw


def decode(llr_ch, gen_poly, perm, rate=1/3, terminate=False, num_iter=6, hard_out=True, algorithm="map", dtype=np.float32):
    """llr_ch [B, n] -> [B, k] LLRs log p(1)/p(0) or hard decisions (decoding.py:357-435)"""
    y = np.asarray(llr_ch, dtype)
    B = y.shape[0]
    mu = len(gen_poly[0]) - 1
    perm = np.asarray(perm)
    inv = np.argsort(perm, kind="stable")
    k, y1_cw, y2_cw = split(y, gen_poly, perm, rate, terminate)
    T = k + (mu if terminate else 0)
    ch1 = y1_cw[:, 0:2 * k:2]                                       # :385-389
    ch2 = y2_cw[:, 0:2 * k:2]
    llr_1e = np.zeros((B, T), dtype)                                # :391
    terminfo = np.zeros((B, T - k), dtype)                          # :394-396
    llr_2i = np.zeros((B, k), dtype)                                # :399
    kw = dict(rsc=True, terminate=terminate, algorithm=algorithm, hard_out=False, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(num_iter):
            llr_1i = conv.bcjr(y1_cw, gen_poly, llr_a=llr_1e, **kw)[:, :k]          # :405-406
            llr_extr = llr_1i - ch1 - llr_1e[:, :k]                                # :407
            llr_2e = np.concatenate([llr_extr[:, perm], terminfo], axis=-1)        # :409-410
            llr_2e = np.minimum(np.maximum(llr_2e, dtype(-LLR_MAX)), dtype(LLR_MAX))    # :411-413
            llr_2i = conv.bcjr(y2_cw, gen_poly, llr_a=llr_2e, **kw)[:, :k]          # :415-416
            llr_extr = llr_2i - llr_2e[:, :k] - ch2                                # :417
            llr_1e = llr_extr[:, inv]                                              # :419
            llr_1e = np.minimum(np.maximum(llr_1e, dtype(-LLR_MAX)), dtype(LLR_MAX))    # :421-423
            llr_1e = np.concatenate([llr_1e, terminfo], axis=-1)                   # :425
    out = llr_2i[:, inv]                                            # :428
    if hard_out:
        out = (dtype(0) < out).astype(dtype)                        # :430-432
    return out.astype(dtype)
