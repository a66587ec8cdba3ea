"""Float64 anchor and derived float32 bound of the two LLR kernels behind ``Demapper``: ``demap_square_qam_kernel`` (arithmetic:
``square_qam_llr``, csrc/demap_core.h) and the generic ``demap_kernel<M, MAXLOG>`` (csrc/mapping.hip), with and without a prior.

Anchor.  ``anchor(y, no, levels_or_points, method, prior)`` evaluates Demapper.call / SymbolLogits2LLRs.call (reference
mapping.py:664-691, 927-967) in float64 on the float32 values the kernel receives, widened exactly: e_c = -|y - c|^2 / max(no, tiny)
(+ sum_i log_sigmoid(+-prior_i)), LLR_i = R_{c: bit i = 1} e_c - R_{c: bit i = 0} e_c, R = logsumexp ("app") or max ("maxlog").  The
constellation is the float32 table handed to the C entry: 2^m points, or the 2^(m/2) PAM levels of the square path, from which the
points are formed exactly (``points_from_levels``).  It agrees with ``oracle.mapping.demapper`` in float64 to 1e-12 of
|R_1| + |R_0| (tests/test_demap_host.py).

Bound, per output, u = 2^-24, gamma(k) = k u / (1 - k u).  Inputs are exact.

1. Exponents.  Square kernel, per axis and level: d = y - l (1 rounding), d d (1), inv = 1 / max(no, tiny) (1, correctly rounded),
   (d d) inv (1): d enters twice, 5 roundings, |e^ - e| <= gamma(5) |e|.  Generic kernel: dr, di (1 each, each squared), dr dr, di di
   (1), their sum (1), the IEEE division (1): at most 5 on either addend, gamma(5) |e| again (-ffp-contract=off: no fused operation
   removes one).  Underflow of d d or of a product adds at most ETA = 2^-148 (1 + 1 / no).  With a prior the generic kernel adds
   ps = sum_i ls_i (m - 1 roundings from 0, gamma(m - 1) sum |ls_i|) and e = ps + e (u |e|);  ls = -z or q - z with q = -|p|,
   z = log1pf(expf(q)) in (0, ln 2]:  |dz| <= (C_EXPF + C_LOG1P) u z (log1p(w) is increasing with relative slope <= 1) + 2^-125, and
   q - z costs u |ls|.
   A reduction R is monotone in every exponent, so with de the exponents' error bounds
       R(e - de) <= R(e^) <= R(e + de),
   and the LLR's share is  E = max(R_1(e + de) - R_1(e) + R_0(e) - R_0(e - de),  R_1(e) - R_1(e - de) + R_0(e + de) - R_0(e)),
   evaluated in float64.  To first order this is gamma(5) (sum_j w1_j |e_j| + sum_j w0_j |e_j|) with the sets' softmax weights, for
   maxlog gamma(5) (|mx1| + |mx0|); the exact form also holds where the exponents' errors are not small against 1 (|e| of 1e7).
2. maxlog: one subtraction, u |llr|.
3. app, generic kernel, per set b with shift mx_b (its maximum), x_j = e_j - mx_b, s_b = sum_j exp(x_j) in [1, 2^(m-1)]:
   x_j: u |x_j|;  exp_core_f32: f = (t - rint t) + lo rounds once at |f| <= 1 / 2 (ln 2 u / 2 = 0.35 u), the hardware exp2 C_EXP u,
   ldexp exact: (C_EXP + 0.5) u relative (a result below 2^-126 is lost or denormal: < 2^-126 each, against s_b >= 1);  the ascending
   sum of 2^(m-1) positive terms from 0: gamma(2^(m-1) - 1);  log_core_f32: the hardware log2 C_LOG u max(|log2 s|, 1), times ln 2 in
   extended precision with one final rounding: C_LOG ln 2 u max(|log2 s|, 1) + u |ln s|;  ln s + mx_b: u |R_b|.  Then u |llr|.
4. app, square kernel, per axis.  Below the switch (gap = M - min(mx0, mx1) <= T, M the axis maximum) both sets of a position share
   the shift M:  x_j = e_j - M: u |x_j|;  demap_exp: the product x log2(e) is carried exactly, t + lo rounds once: u |t| in the
   argument = u |x_j| relative, the hardware exp2 C_EXP u, constants' representation < 0.05 u: 2 u |x_j| + (C_EXP + 0.05) u;
   members whose exponential falls below 2^-126 are returned as 0: with T = 64 a set's sum is >= e^-64 = 2^-92.3 and the 2^(NB-1)
   <= 16 members lose < 2^-122 together: C_FLUSH u = 2^-29.6 / 2^-24 < 0.03 u of the sum;  bit_reduce adds along a path of at most
   L / 2 - 1 additions: gamma(L / 2 - 1);  r = (log2 s1 - log2 s0) ln2f: C_LOG ln 2 u max(|log2 s_b|, 1) per set, the subtraction and
   the product u |llr| each, float32(ln 2) 0.05 u |llr|: 2.05 u |llr|.
   Above the switch each set is re-evaluated against its own maximum: as in 3 with demap_exp (2 u |x_j| + (C_EXP + 0.05) u), the sum
   of L / 2 terms from 0, log2(a) ln2f: C_LOG ln 2 u max(|log2 a|, 1) + 1.05 u |ln a|, + mx_b: u |R_b|, then u |llr|.
   The kernel decides on its computed gap: within MARGIN = de(M) + de(best) + u gap of T the larger of the two bounds holds.
   The bound grants NOTHING for members lost at a larger gap: a kernel that switches at 80 loses up to e^-7.34 = 6.5e-4 of a set's
   sum at gap 80; at gap 79.5 with the second member 8 further down it leaves the bound by a factor of 8
   (tests/test_demap_host.py ``test_flush_at_threshold_80``; the MI355X gave the same 8.2 before the switch was lowered).
5. Second-order terms: every sum of terms above is multiplied by 1.001.

C_EXP, C_LOG, C_EXPF, C_LOG1P are properties of the device functions: twice the largest error that tools/ubench/exp_log_accuracy.hip
measured on an MI355X (ROCm 7) over EVERY float of the range the kernels use, against float64, in units of u:
    __builtin_amdgcn_exp2f   [-126, 0]         1.4234 u of the result                  C_EXP   = 2.85
    __builtin_amdgcn_logf    [2^-116, 2^10]    1.9991 u of max(|log2 x|, 1)            C_LOG   = 4.00
    expf                     [-87, 0]          1.4108 u of the result                  C_EXPF  = 2.83
    log1pf                   [2^-126, 1]       1.0491 u of the result                  C_LOG1P = 2.10
(the same run: demap_exp 45.5 u at x = -68.5 = 2 u |x| there / 3, exp_core_f32 1.41 u, log_core_f32 2.72 u - inside items 3 and 4).
They were not fitted to the demapper's output."""
import numpy as np

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
C_EXP, C_LOG, C_EXPF, C_LOG1P = 2.85, 4.00, 2.83, 2.10
C_FLUSH = 0.03
THRESHOLD = 64.0          # the switch of square_qam_llr (csrc/demap_core.h)
SECOND_ORDER = 1.001
LN2 = float(np.log(2.0))


def gamma(k):
    return k * U / (1 - k * U)


def label_bits(m):
    """[2^m, m] bits of every label, MSB first"""
    return (np.arange(2 ** m)[:, None] >> np.arange(m - 1, -1, -1)) & 1


def points_from_levels(lev):
    """the 2^(2 NB) points of the square constellation whose axes carry the levels ``lev`` (indexed by the axis label): even label
    bits drive the real axis, odd ones the imaginary axis (reference mapping.py:108-111); exact in complex128"""
    lev = np.asarray(lev, np.float64)
    nb = int(np.log2(len(lev)))
    bits = label_bits(2 * nb)
    w = 1 << np.arange(nb - 1, -1, -1)
    return lev[bits[:, 0::2] @ w] + 1j * lev[bits[:, 1::2] @ w]


def levels_from_points(points):
    """the float32 levels ``Constellation.pam_levels`` hands to the square kernel, or None where the points are no such square"""
    pts = np.asarray(points).astype(np.complex64)
    m = int(np.log2(len(pts)))
    if m % 2:
        return None
    nb = m // 2
    bits = label_bits(m)
    w = 1 << np.arange(nb - 1, -1, -1)
    li, lq = bits[:, 0::2] @ w, bits[:, 1::2] @ w
    lev = np.zeros(2 ** nb, np.float32)
    lev[li] = pts.real
    return lev if np.array_equal(lev[li], pts.real) and np.array_equal(lev[lq], pts.imag) else None


def _as_points(levels_or_points):
    t = np.asarray(levels_or_points)
    return np.asarray(t, np.complex128) if np.iscomplexobj(t) else points_from_levels(t)


def _no64(y, no):
    no = np.asarray(no, np.float64).reshape(-1)
    assert no.size in (1, y.size)
    return np.maximum(np.broadcast_to(no, (y.size,)), TINY)


def _lse(e, axis=-1):
    mx = np.max(e, axis=axis, keepdims=True)
    return (np.log(np.sum(np.exp(e - mx), axis=axis, keepdims=True)) + mx).squeeze(axis)


def _reduce(e, method):
    return _lse(e) if method == "app" else np.max(e, axis=-1)


def _log_sigmoid_terms(prior, n, m):
    """ls [n, m, 2] (value 0 / 1 of the bit) in float64 and the kernel's error bound on each"""
    p = np.broadcast_to(np.asarray(prior, np.float64).reshape(-1, m), (n, m))
    z = np.log1p(np.exp(-np.abs(p)))
    ls = np.stack([np.where(-p < 0, -p - z, -z), np.where(p < 0, p - z, -z)], axis=-1)
    dls = (C_EXPF + C_LOG1P) * U * z[..., None] + U * np.abs(ls) + 2.0 ** -125
    return ls, dls


def exponents(y, no, points, prior=None, with_error=False):
    """e [n, P] in float64 (P points, or L levels of ONE axis where ``y`` and ``points`` are real) and, on request, the bound de on
    the kernel's error in each (item 1)"""
    y = np.asarray(y).reshape(-1)
    pts = np.asarray(points)
    n0 = _no64(y, no)[:, None]
    if np.iscomplexobj(pts):
        y = y.astype(np.complex128)
        dr, di = y.real[:, None] - pts.real[None, :], y.imag[:, None] - pts.imag[None, :]
        ed = -(dr * dr + di * di) / n0
    else:
        d = y.astype(np.float64)[:, None] - pts.astype(np.float64)[None, :]
        ed = -(d * d) / n0
    e, de = ed, None
    if with_error:
        de = gamma(5) * np.abs(ed) + 2.0 ** -148 * (1 + 1 / n0)
    if prior is not None:
        m = int(np.log2(len(pts)))
        ls, dls = _log_sigmoid_terms(prior, y.size, m)
        lab = label_bits(m)                                                   # [P, m]
        idx = np.arange(m)
        ps = ls[:, idx[None, :], lab].sum(-1)                                   # [n, P]
        e = ps + ed
        if with_error:
            de = de + dls[:, idx[None, :], lab].sum(-1) + gamma(max(m - 1, 0)) * np.abs(ls[:, idx[None, :], lab]).sum(-1) + U * np.abs(e)
    return (e, de) if with_error else e


def anchor(y, no, levels_or_points, method, prior=None, parts=False):
    """LLRs [n, m] in float64; ``parts``: also R_1 and R_0"""
    pts = _as_points(levels_or_points)
    m = int(np.log2(len(pts)))
    e = exponents(y, no, pts, prior)
    lab = label_bits(m)
    r1 = np.stack([_reduce(e[:, lab[:, i] == 1], method) for i in range(m)], axis=-1)
    r0 = np.stack([_reduce(e[:, lab[:, i] == 0], method) for i in range(m)], axis=-1)
    return (r1 - r0, r1, r0) if parts else r1 - r0


def _set_terms(e, de, method, exp_arg, c_exp, n_add, own_shift, shift=None):
    """one set of exponents e [n, K]: R, the two one-sided shares of item 1 and the evaluation terms of items 3 / 4 for its
    log-sum-exp (without the last subtraction).  ``shift``: the common shift M of the square kernel below the switch"""
    r = _reduce(e, method)
    up, dn = _reduce(e + de, method) - r, r - _reduce(e - de, method)
    if method != "app":
        return r, up, dn, 0.0
    sh = np.max(e, axis=-1) if shift is None else shift
    x = e - sh[:, None]
    with np.errstate(all="ignore"):               # far above the switch the common shift leaves nothing in float64 either:
        ex = np.exp(x)                            # that branch's bound is inf there, and is not the one that applies
        s = ex.sum(-1)
        w = ex / s[:, None]
        l2 = np.maximum(np.abs(np.log2(s)), 1.0)
        ev = (w * (exp_arg * U * np.abs(x))).sum(-1) + c_exp * U + gamma(n_add) + C_LOG * LN2 * U * l2
        ev = np.where(s > 0, ev, np.inf)
        s = np.where(s > 0, s, 1.0)
    if own_shift is None:                         # generic kernel: extended-precision ln 2, then + mx
        ev = ev + U * np.abs(np.log(s)) + U * np.abs(r)
    elif own_shift:                               # square kernel above the switch
        ev = ev + 1.05 * U * np.abs(np.log(s)) + U * np.abs(r)
    else:                                         # square kernel below the switch: the members lost to the flush
        ev = ev + C_FLUSH * U
    return r, up, dn, ev


def _combine(t1, t0, last):
    r1, up1, dn1, ev1 = t1
    r0, up0, dn0, ev0 = t0
    llr = r1 - r0
    return SECOND_ORDER * (np.maximum(up1 + dn0, dn1 + up0) + ev1 + ev0 + last * U * np.abs(llr))


def bound_generic(y, no, points, method, prior=None):
    """[n, m]: items 1, 2, 3"""
    pts = np.asarray(points, np.complex128)
    m = int(np.log2(len(pts)))
    e, de = exponents(y, no, pts, prior, with_error=True)
    lab = label_bits(m)
    out = []
    for i in range(m):
        t = [_set_terms(e[:, lab[:, i] == b], de[:, lab[:, i] == b], method, 1.0, C_EXP + 0.5, 2 ** (m - 1) - 1, None) for b in (1, 0)]
        out.append(_combine(t[0], t[1], 1.0))
    return np.stack(out, axis=-1)


def bound_square(y, no, levels, method, threshold=THRESHOLD):
    """[n, 2 NB]: items 1, 2, 4.  Output 2 t + ax is bit t (MSB first) of the axis label, axis 0 = real"""
    lev = np.asarray(levels, np.float32)
    nb = int(np.log2(len(lev)))
    L = 1 << nb
    y = np.asarray(y).reshape(-1)
    out = np.zeros((y.size, 2 * nb))
    lab = label_bits(nb)
    for ax in range(2):
        e, de = exponents(y.real if ax == 0 else y.imag, no, lev, with_error=True)
        jm = np.argmax(e, axis=-1)
        rows = np.arange(y.size)
        mall = e[rows, jm]
        for t in range(nb):
            sel = [lab[:, t] == b for b in (1, 0)]
            if method != "app":
                tt = [_set_terms(e[:, s], de[:, s], method, 0, 0, 0, None) for s in sel]
                out[:, 2 * t + ax] = _combine(tt[0], tt[1], 1.0)
                continue
            lo = [_set_terms(e[:, s], de[:, s], method, 2.0, C_EXP + 0.05, max(L // 2 - 1, 0), False, shift=mall) for s in sel]
            hi = [_set_terms(e[:, s], de[:, s], method, 2.0, C_EXP + 0.05, max(L // 2 - 1, 0), True) for s in sel]
            b_lo, b_hi = _combine(lo[0], lo[1], 2.05), _combine(hi[0], hi[1], 1.0)
            jb = [np.argmax(np.where(s[None, :], e, -np.inf), axis=-1) for s in sel]
            worst = np.where(e[rows, jb[0]] < e[rows, jb[1]], jb[0], jb[1])
            gap = mall - e[rows, worst]
            margin = de[rows, jm] + de[rows, worst] + U * gap
            out[:, 2 * t + ax] = np.where(gap > threshold + margin, b_hi, np.where(gap < threshold - margin, b_lo, np.maximum(b_lo, b_hi)))
    return out


def bound(y, no, levels_or_points, method, prior=None):
    """the bound of the kernel that ``Demapper`` runs on this table: real levels - the square kernel, complex points - the generic"""
    if np.iscomplexobj(np.asarray(levels_or_points)):
        return bound_generic(y, no, levels_or_points, method, prior)
    assert prior is None, "the square kernel takes no prior"
    return bound_square(y, no, levels_or_points, method)


def ratio(out, an, bd):
    """max |out - anchor| / bound and its index; a NaN or inf in ``out`` counts as inf"""
    out = np.asarray(out, np.float64).reshape(an.shape)
    q = np.where(np.isfinite(out), np.abs(out - an) / bd, np.inf)
    at = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[at]), tuple(int(i) for i in at)
