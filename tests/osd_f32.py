"""Specification of the ordered-statistics decoder kernels (csrc/osd.hip): the reference's OSDecoder
(src/sionna/phy/fec/linear/decoding.py:14-478) restated in NumPy, for float32 and float64 inputs.

Points the reference leaves implicit, fixed here (and in the kernels):
  - clip: min(max(llr, -100), 100) in the input's dtype;
  - sort: descending |llr|, equal magnitudes in ascending index order (TF's stable kernel);
  - most reliable basis by the reference's pivot method (_find_mrb, :318-402): for row r = 0..k-1 the pivot is the first 1 of
    row r over all n sorted columns, cleared from every other row; final order = pivots in row order, then the other
    positions ascending.  Dependent leading columns need no special case;
  - order 0: u = llr_sort[:k] > 0 (0 gives bit 0), c0 = u G_mrb mod 2;
  - candidates: after order 0 in the order of itertools.combinations(range(k), i), i = 1..t; the winner is the candidate
    of smallest distance, and among equal distances the one met first (argmin within an order, strict < between orders);
  - distance: the reference's mean over n of log(1 + exp(llr (1 - 2c))) differs between two candidates by the sum of
    llr (2 c0 - 1) over the positions where they differ, divided by n (softplus(-a) - softplus(a) = -a).  The
    specification ranks candidates by that difference to c0, with every clipped LLR rounded once to a multiple of 2^-40
    (rint(llr * 2^40) as int64: exact for a float32 LLR of magnitude >= 2^-16) and the terms summed as integers.  The
    sum is exact, so no order of additions has to be fixed and equal distances are equal;
  - float32 overflow: the reference's exp(|llr|) is +inf in float32 for |llr| > SAT32, so a candidate whose bit
    disagrees with the sign of the LLR at such a position has distance +inf there: it never wins a strict <, and when
    every candidate is infinite, order 0 is returned.  In float64 nothing overflows at |llr| <= 100.
"""
import functools
import itertools

import numpy as np

LLR_MAX = 100.0
SCALE = 2.0 ** 40
# largest float32 x with a finite float32 exp(x): log(FLT_MAX) = 88.72283905..., rounded down to float32
SAT32 = np.float32(88.72283172607422)
INF = np.iinfo(np.int64).max


def quantise(llr):
    """clipped LLRs -> int64 multiples of 2^-40 (float64 product by a power of two is exact; rint = ties to even)"""
    return np.rint(llr.astype(np.float64) * SCALE).astype(np.int64)


def sort_order(a):
    """descending, stable"""
    return np.argsort(-a, kind="stable")


def find_mrb(gm_sorted):
    """pivot method on the [k, n] 0/1 matrix whose columns are already in reliability order: the eliminated matrix in its
    final column order and that order"""
    gm = np.array(gm_sorted, dtype=np.uint8)
    k, n = gm.shape
    pivots = np.zeros(k, np.int64)
    for r in range(k):
        p = int(np.argmax(gm[r]))
        pivots[r] = p
        hit = gm[:, p].astype(bool)
        hit[r] = False
        gm[hit] ^= gm[r]
    rest = np.setdiff1d(np.arange(n), pivots)                       # ascending
    idx = np.concatenate([pivots, rest]).astype(np.int64)
    return gm[:, idx], idx


@functools.lru_cache(maxsize=32)
def patterns(k, t):
    """[C(k, t), t] in the order of itertools.combinations"""
    return np.array(list(itertools.combinations(range(k), t)), dtype=np.int64).reshape(-1, t)


def prepare(llr, gm, dtype=np.float32):
    """one codeword: everything up to order 0.  Returns a dict with perm (sorted position -> input position), par [k, n-k]
    (parity part of the MRB), c0 [n], cost [n] (int64 change of the distance when position i of c0 is flipped), sat [n]
    (float32 overflow positions), and dis0 [n] (saturated positions where c0 disagrees with the LLR's sign)"""
    gm = np.asarray(gm).astype(np.uint8)
    k, n = gm.shape
    l = np.minimum(np.maximum(np.asarray(llr, dtype), dtype(-LLR_MAX)), dtype(LLR_MAX))
    order = sort_order(np.abs(l))
    mrb, idx = find_mrb(gm[:, order])
    perm = order[idx]
    ls = l[perm]
    hard = (ls > 0).astype(np.uint8)
    c0 = (hard[:k].astype(np.int64) @ mrb.astype(np.int64) % 2).astype(np.uint8)
    q = quantise(ls)
    cost = np.where(c0 == 1, q, -q)
    sat = (np.abs(ls) > SAT32) if dtype == np.float32 else np.zeros(n, bool)
    return dict(perm=perm, par=mrb[:, k:], c0=c0, cost=cost, sat=sat, dis0=sat & (c0 != hard), k=k, n=n)


def search(p, t):
    """(key, index, codeword in sorted order) of the winner: index 0 is order 0, 1.. the patterns in candidate order"""
    k, n = p["k"], p["n"]
    par, cost, sat, dis0 = p["par"], p["cost"], p["sat"], p["dis0"]
    best_key, best_idx, best_e = (INF if dis0.any() else 0), 0, np.zeros(n, np.uint8)
    base = 1
    for i in range(1, min(t, k) + 1):
        ep = patterns(k, i)
        e = np.zeros((len(ep), n), np.uint8)
        np.put_along_axis(e, ep, 1, axis=1)
        for j in range(i):
            e[:, k:] ^= par[ep[:, j]]
        key = e.astype(np.int64) @ cost
        inf = ((e.astype(bool) & sat) ^ dis0).any(axis=1)
        key[inf] = INF
        m = int(np.argmin(key))
        if key[m] < best_key:
            best_key, best_idx, best_e = int(key[m]), base + m, e[m]
        base += len(ep)
    return best_key, best_idx, p["c0"] ^ best_e


def decode(llr, gm, t, dtype=np.float32):
    """OSDecoder.call: llr [..., n] -> hard decisions [..., n] of the same dtype"""
    llr = np.asarray(llr, dtype)
    n = llr.shape[-1]
    flat = llr.reshape(-1, n)
    out = np.zeros(flat.shape, dtype)
    for b in range(flat.shape[0]):
        p = prepare(flat[b], gm, dtype)
        _, _, c = search(p, t)
        out[b, p["perm"]] = c
    return out.reshape(llr.shape)


def num_candidates(k, t):
    import math
    return sum(math.comb(k, i) for i in range(1, min(t, k) + 1))


def reference_distances(llr, gm, t, dtype=np.float64):
    """NumPy model of the reference's own metric (mean over n of log(1 + exp(llr (1 - 2c))) in ``dtype``) for order 0 and
    every candidate, in candidate order: [1 + num_candidates].  Used by the fixture generator for the gap between the two
    smallest distances; not part of the specification's arithmetic."""
    p = prepare(llr, gm, np.float32 if dtype == np.float32 else np.float64)
    k, n = p["k"], p["n"]
    l = np.minimum(np.maximum(np.asarray(llr, dtype), dtype(-LLR_MAX)), dtype(LLR_MAX))[p["perm"]]
    cands = [p["c0"][None]]
    for i in range(1, min(t, k) + 1):
        ep = patterns(k, i)
        e = np.zeros((len(ep), n), np.uint8)
        np.put_along_axis(e, ep, 1, axis=1)
        for j in range(i):
            e[:, k:] ^= p["par"][ep[:, j]]
        cands.append(p["c0"][None] ^ e)
    c = np.concatenate(cands).astype(dtype)
    with np.errstate(over="ignore"):
        d = np.log(dtype(1) + np.exp(l[None] * (dtype(1) - dtype(2) * c)))
    return np.mean(d, axis=1)
