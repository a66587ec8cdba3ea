"""NumPy specification of the discrete channels (csrc/discrete.hip, sionna_amd/phy/channel/discrete_channel.py), in
float32 and float64, for all four channels and every integer dtype, on the Philox stream of oracle/utils.py.

The rule (DESIGN.md "Discrete channels"): element i of the flattened input (C order) uses word i % 4 of
philox_block(seed, call, i // 4); the error event is (uint64)word < (uint64)ceil(p * 2^32) with
p = pb > 0 ? (pb < 1 ? pb : 1) : 0.  Everything after the draw follows the reference's channel/discrete_channel.py
(:238-296 memoryless family, :564-596 erasure) operation by operation; the float32 log is the correctly rounded one
(np.log in float64 rounded once - what csrc/accurate_math.h computes), the float64 log is np.log.
"""
import numpy as np

from oracle.utils import philox_block

EPS = 1e-9
MEMORYLESS, ERASURE = 0, 1


def words(seed, call, n):
    """word i % 4 of block i // 4 for elements 0..n-1, uint32[n] (the layout of oracle.utils.random_bits)"""
    if n == 0:
        return np.zeros(0, np.uint32)
    return np.stack(philox_block(seed, call, (n + 3) // 4), axis=1).reshape(-1)[:n]


def unit_clip(pb):
    """pb > 0 ? (pb < 1 ? pb : 1) : 0 in pb's own dtype: NaN gives 0"""
    pb = np.asarray(pb)
    one, zero = pb.dtype.type(1), pb.dtype.type(0)
    with np.errstate(invalid="ignore"):
        return np.where(pb > 0, np.where(pb < 1, pb, one), zero)


def threshold(p):
    """ceil(p * 2^32) as uint64; the product is exact in float32 and in float64"""
    p = np.asarray(p)
    return np.ceil(p * p.dtype.type(4294967296.0)).astype(np.uint64)


def event_probability(pb, dtype=np.float32):
    """P(e) = ceil(p 2^32) / 2^32 of a probability given in ``dtype`` (float64 result, exact)"""
    return threshold(unit_clip(np.asarray(pb, dtype))).astype(np.float64) / 2.0 ** 32


def pb_period(x_shape, pb_shape):
    """How pb reaches the kernel: (block shape, pb_len).  pb_shape, left-padded with ones to the rank of x, is expanded to
    the smallest trailing block of x that contains it; element i of the flattened x reads index i % pb_len of the
    flattened block."""
    x_shape, pb_shape = tuple(x_shape), tuple(pb_shape)
    if len(pb_shape) > len(x_shape):
        raise ValueError("pb has more dimensions than x")
    s = (1,) * (len(x_shape) - len(pb_shape)) + pb_shape
    for a, b in zip(s, x_shape):
        if a != 1 and a != b:
            raise ValueError(f"pb of shape {pb_shape} does not broadcast to x of shape {x_shape}")
    d = 0
    while d < len(s) and s[d] == 1:
        d += 1
    block = x_shape[d:]
    return block, int(np.prod(block, dtype=np.int64)) if block else 1


def pb_flat(x_shape, pb):
    """pb as the kernel indexes it: the flattened trailing block, read at i % pb_len"""
    pb = np.asarray(pb)
    block, _ = pb_period(x_shape, pb.shape)
    if not block:
        return pb.reshape(-1)
    return np.broadcast_to(pb.reshape(pb.shape[pb.ndim - len(block):] if pb.ndim >= len(block) else pb.shape), block).reshape(-1)


def per_element(x_shape, pb):
    """pb per element of the flattened x by the kernel's index rule"""
    flat = pb_flat(x_shape, pb)
    n = int(np.prod(x_shape, dtype=np.int64))
    return flat[np.arange(n, dtype=np.int64) % len(flat)]


def log_def(a):
    """the defined log: float32 correctly rounded (float64 log rounded once), float64 np.log; a < 0 gives NaN"""
    a = np.asarray(a)
    with np.errstate(invalid="ignore", divide="ignore"):
        if a.dtype == np.float32:
            return np.log(a.astype(np.float64)).astype(np.float32)
        return np.log(a)


def sym_clip(v, m):
    with np.errstate(invalid="ignore"):
        return np.where(v < -m, -m, np.where(v > m, m, v))


def compute_dtype(x_dtype):
    return np.float64 if np.dtype(x_dtype) == np.float64 else np.float32


def apply(x, pb0, pb1, words_or_pattern, kind=MEMORYLESS, bipolar=False, return_llrs=False, llr_max=100.0, pattern=False):
    """The channel on the flattened x.  pb0 / pb1: per element of x (any shape broadcastable by the kernel's index rule is
    resolved by the caller with ``per_element``), in the compute dtype - float64 for float64 x, float32 otherwise; pb0 is
    ignored by the erasure channel.  words_or_pattern: the uint32 words of the stream, or with ``pattern=True`` a 0/1 error
    pattern that replaces the draw (then pb enters only the LLRs).  Returns y of x's dtype and shape, and the pattern."""
    x = np.asarray(x)
    T = x.dtype.type
    P = compute_dtype(x.dtype)
    xf = x.reshape(-1)
    n = xf.size
    pb0 = np.broadcast_to(np.asarray(pb0, P), (n,)) if kind == MEMORYLESS else None
    pb1 = np.broadcast_to(np.asarray(pb1, P), (n,))
    if return_llrs and x.dtype.kind != "f":
        raise ValueError("LLR outputs require non-integer dtypes.")
    if x.dtype.kind == "u" and (bipolar or kind == ERASURE):
        raise ValueError("Only signed dtypes are supported.")
    lm = P(llr_max)
    if kind == ERASURE:
        if pattern:
            e = np.asarray(words_or_pattern).reshape(-1) != 0
        else:
            e = words_or_pattern.astype(np.uint64) < threshold(unit_clip(pb1.astype(np.float32)))
        if return_llrs:
            xb = xf if bipolar else T(2) * xf - T(1)
            y = np.where(e, T(0), xb * T(lm))
        else:
            y = np.where(e, T(0) if bipolar else T(-1), xf)
        return y.astype(x.dtype).reshape(x.shape), e.reshape(x.shape)
    p0, p1 = unit_clip(pb0), unit_clip(pb1)
    one = xf != (T(-1) if bipolar else T(0))
    if pattern:
        e = np.asarray(words_or_pattern).reshape(-1) != 0
    else:
        e = words_or_pattern.astype(np.uint64) < threshold(np.where(one, p1, p0))
    if bipolar:
        y = xf * (T(1) - T(2) * e.astype(x.dtype))
    elif x.dtype.kind == "f":
        y = np.abs(xf - e.astype(x.dtype))
    else:
        y = (xf + e.astype(x.dtype)) & T(1)
    y = y.astype(x.dtype)
    if return_llrs:
        eps = P(EPS)
        r1 = (y == T(1)) if bipolar else (T(2) * y - T(1) == T(1))
        v1 = log_def((P(1) - p1) - eps) - log_def(p0 + eps)
        v0 = log_def(p1 + eps) - log_def((P(1) - p0) - eps)
        y = sym_clip(np.where(r1, v1, v0), lm).astype(x.dtype)
    return y.reshape(x.shape), e.reshape(x.shape)


def channel(x, pb0, pb1, seed, call, kind=MEMORYLESS, bipolar=False, return_llrs=False, llr_max=100.0):
    """The channel with its own draw; pb0 / pb1 of any shape the block takes (None for pb0: the Z channel's 0)."""
    x = np.asarray(x)
    P = compute_dtype(x.dtype)
    b1 = per_element(x.shape, np.asarray(pb1, P))
    b0 = np.zeros_like(b1) if pb0 is None else per_element(x.shape, np.asarray(pb0, P))
    return apply(x, b0, b1, words(seed, call, x.size), kind, bipolar, return_llrs, llr_max)[0]


def llr_log_terms(pb0, pb1, received_one, dtype):
    """|log a| + |log b| of the two logs an LLR is the difference of (float64), for the bars of the tests"""
    P = np.dtype(dtype).type
    p0, p1 = unit_clip(np.asarray(pb0, P)), unit_clip(np.asarray(pb1, P))
    eps = P(EPS)
    with np.errstate(invalid="ignore", divide="ignore"):
        a1, b1 = np.log(((P(1) - p1) - eps).astype(np.float64)), np.log((p0 + eps).astype(np.float64))
        a0, b0 = np.log((p1 + eps).astype(np.float64)), np.log(((P(1) - p0) - eps).astype(np.float64))
    return np.where(received_one, np.abs(a1) + np.abs(b1), np.abs(a0) + np.abs(b0))
