"""Float64 anchors and derived float32 bounds of the symbol-domain mapping kernels of csrc/mapping.hip - ``symbol_demap_kernel``
(SymbolDemapper), ``logits2llrs_kernel<M, MAXLOG>`` (SymbolLogits2LLRs), ``llrs2logits_kernel`` (LLRs2SymbolLogits),
``logits2moments_kernel`` (SymbolLogits2Moments), ``pam2qam_logits_kernel`` (PAM2QAM) - and of their float64 twins in
csrc/f64_mapping.hip.  The helpers of tests/demap_f32.py (gamma, label_bits, the set terms of its items 1-3, the measured constants)
are used, not copied.

Anchors.  Each evaluates the reference's formula (mapping.py:776-792, 927-967, 1043-1058, 1125-1138, 1304-1314) on the float32
inputs widened exactly, in ``wide`` = float64 (against the float32 kernels) or the host's long double (against the float64 kernels,
whose own rounding a float64 anchor would share).  Members at -inf follow tf.reduce_logsumexp / tf.nn.log_softmax: a non-finite
maximum is replaced by 0, so a set (or row) whose members are all -inf reduces to -inf, and a -inf member of any other set has
weight 0.  What the reference's own code returns there is recorded in tests/golden/symbol_edges_ref_golden.npz (generator
tools/gen_symbol_ref_golden.py edges) and tests/test_symbol_host.py holds the anchors to it:  a whole set at -inf gives an LLR of
-+inf (both sets: NaN);  LLRs2SymbolLogits maps an LLR of +-inf to logits of -inf and 0 sums;  SymbolDemapper at no = 0 returns NaN on
EVERY output (0 / 0 on a point, -inf - (-inf) off it) - the reference does not clamp no here, unlike Demapper - so no = 0 defines
nothing and the smallest no that is held is finfo(float32).tiny.

Bounds, per output, u = 2^-24, gamma(k) = k u / (1 - k u).  Inputs are exact; -ffp-contract=off: one rounding per operation, and the
build sets no fast-math flag, so hipcc's default (-fhip-fp32-correctly-rounded-divide-sqrt) leaves sqrtf and / correctly rounded.

1. symbol_demap.  Exponent e_c = -(sqrt(dr^2 + di^2))^2 / no (+ prior_c): dr, di (1 rounding each, each squared: 2 on either addend),
   dr dr, di di (1), their sum (1): gamma(4) on s = dr^2 + di^2;  d = sqrtf(s) halves that and adds its own rounding: (gamma(4) / 2 + u);
   d d doubles it and rounds (gamma(4) + 3 u), the IEEE division rounds once more: |e^ - e| <= gamma(8) |e|, + an underflow term
   2^-147 (1 + 1 / no);  with a prior one addition, u |e|.  The three evaluations of e_c in the kernel are the same float32 operations
   and give the same value.  lse = mx + logf(sum_c expf(e_c - mx)) is monotone in every exponent:
   |lse(e^) - lse(e)| <= max(lse(e + de) - lse(e), lse(e) - lse(e - de)), evaluated in float64; its evaluation adds x_c = e_c - mx
   (u |x_c|, weighted by the softmax weight w_c), expf (C_EXPF u; below -87 the result is under 2^-126 against a sum >= 1), the
   ascending sum of P terms from 0 (gamma(P - 1)), logf on [1, P] (C_LOGF u ln sum), mx + log (u |lse|).  The output e_c - lse: the
   error of e_c, that of lse, and u |out|.  The bound therefore scales with u |e_c| + u |lse|, not with the output.
2. logits2llrs.  Items 1 (prior part), 2 and 3 of tests/demap_f32.py carry over with the logits as EXACT exponents: without a prior
   de = 0, with one de = sum_i dls_i + gamma(m - 1) sum_i |ls_i| + u |e|.  ``bound_logits2llrs`` calls ``_set_terms`` / ``_combine`` of
   demap_f32 on them.  Nothing is granted for members lost below the clamp of the exponential's argument at -104: e^-104 < 2^-150.
3. llrs2logits.  Per log_sigmoid (demap_f32 item 1): (C_EXPF + C_LOG1P) u z + u |ls| + 2^-125;  the sum of m terms from 0:
   gamma(m - 1) sum_j |ls_j|.
4. logits2moments.  Weight p_c = expf(z_c - mx) / den:  t_c = z_c - mx (u |t_c| in the argument = relative in the result), expf
   (C_EXPF u), den = ascending sum (gamma(P - 1) + the weighted mean of its terms' errors), the division (u):
   delta_c = u |t_c| + C_EXPF u + sum_k p_k (u |t_k| + C_EXPF u) + gamma(P - 1) + u, + 2^-125 absolute for weights under 2^-126.
   Mean, per component: sum_c delta_c p_c |x_c| + gamma(P) sum_c p_c |x_c| (product and ascending sum).  Variance: every term
   p_c |x_c - mean|^2 carries delta_c + gamma(P + 4) (difference, two squares and their sum, product, ascending sum), and the error
   Dm of the computed mean moves |x_c - mean|^2 by 2 |x_c - mean| |Dm| + |Dm|^2.  Every part scales with the variance's own terms or
   with Dm: a row with one dominant logit has a bound of the order of its (tiny) variance + u^2.
5. pam2qam: one float32 addition - the correctly rounded sum, bit for bit.
6. float64 twins: the same forms with u = 2^-53, i.e. 2^-29 times the float32 bound (the float64 kernel forms |y - c|^2 without the
   square root: fewer roundings; libm's double exp / log / log1p are within 1 ulp, below the float32 constants).
7. Second-order terms: every sum above is multiplied by 1.001.

C_LOGF is a property of the device function: twice the largest error tools/ubench/exp_log_accuracy.hip measured on an MI355X over
every float of [1, 1024], |logf(x) - ln x| / ln x in units of u (and logf(1) = 0 exactly):  2.6977 u (near x = 256.81; 83886081 floats), C_LOGF = 5.40.  The
other constants are those of tests/demap_f32.py.  None was fitted to the output of the kernels under test."""
import numpy as np

import demap_f32 as df
from demap_f32 import C_EXP, C_EXPF, C_LOG1P, SECOND_ORDER, U, gamma, label_bits

C_LOGF = 5.40
F64_SCALE = 2.0 ** -29
WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
_BIG = -1e300                                   # stands in for -inf where a bound needs finite arithmetic: exp gives 0 all the same


def lse_tf(e, axis=-1):
    """tf.reduce_logsumexp: a non-finite maximum is replaced by 0"""
    with np.errstate(all="ignore"):
        mx = np.max(e, axis=axis, keepdims=True)
        mx = np.where(np.isfinite(mx), mx, 0)
        return (np.log(np.sum(np.exp(e - mx), axis=axis, keepdims=True)) + mx).squeeze(axis)


def first_argmax(e):
    return np.argmax(e, axis=-1).astype(np.int32)


def _log_sigmoid(x):
    with np.errstate(all="ignore"):
        z = np.log1p(np.exp(-np.abs(x)))
        return np.where(x < 0, x - z, -z)


# ------------------------------------------------------------------ 1. SymbolDemapper
def sd_exponents(y, no, points, prior=None, wide=np.float64, with_error=False):
    y = np.asarray(y).reshape(-1)
    pts = np.asarray(points).astype(np.complex128)
    cw = np.clongdouble if wide is np.longdouble else np.complex128
    yw, pw = y.astype(cw), pts.astype(cw)
    n0 = np.broadcast_to(np.asarray(no).astype(wide).reshape(-1), (y.size,))[:, None]
    with np.errstate(all="ignore"):
        dr, di = yw.real[:, None] - pw.real[None, :], yw.imag[:, None] - pw.imag[None, :]
        ed = -(dr * dr + di * di) / n0
        e = ed
        if prior is not None:
            e = ed + np.broadcast_to(np.asarray(prior).astype(wide).reshape(-1, len(pts)), ed.shape)
        if not with_error:
            return e
        de = gamma(8) * np.abs(ed) + 2.0 ** -147 * (1 + 1 / n0)
        if prior is not None:
            de = de + U * np.abs(e)
        de = np.where(np.isfinite(e), de, 0.0)
    return e, np.asarray(de, np.float64)


def anchor_symbol_demap(y, no, points, prior=None, hard=False, wide=np.float64):
    e = sd_exponents(y, no, points, prior, wide)
    if hard:
        return first_argmax(e)
    with np.errstate(all="ignore"):
        return e - lse_tf(e)[:, None]


def bound_symbol_demap(y, no, points, prior=None):
    e, de = sd_exponents(y, no, points, prior, with_error=True)
    P = e.shape[1]
    with np.errstate(all="ignore"):
        ef = np.where(np.isfinite(e), e, _BIG)
        L = df._lse(ef)
        shift = np.maximum(df._lse(ef + de) - L, L - df._lse(ef - de))
        mx = ef.max(-1, keepdims=True)
        x = ef - mx
        ex = np.exp(x)
        s = ex.sum(-1)
        w = ex / s[:, None]
        ev = np.where(w > 0, w * U * np.abs(x), 0).sum(-1) + C_EXPF * U + P * 2.0 ** -125 + gamma(P - 1) + C_LOGF * U * np.log(s) + U * np.abs(L)
        out = ef - L[:, None]
        bd = SECOND_ORDER * (de + (shift + ev)[:, None] + U * np.abs(out))
    return np.where(np.isfinite(e), bd, 0.0)


def sure_argmax(e, de):
    """rows whose first maximum survives every admissible error: e_best - de_best > e_c + de_c for every other c"""
    best = np.argmax(e, axis=-1)
    rows = np.arange(e.shape[0])
    with np.errstate(all="ignore"):
        lo = (e - de)[rows, best]
        hi = np.where(np.isfinite(e), e + de, -np.inf)
    hi[rows, best] = -np.inf
    return lo > hi.max(-1) if e.shape[1] > 1 else np.ones(e.shape[0], bool)


# ------------------------------------------------------------------ 2. SymbolLogits2LLRs
def l2l_exponents(z, m, prior=None, wide=np.float64, with_error=False):
    z = np.asarray(z).astype(wide).reshape(-1, 1 << m)
    n = z.shape[0]
    if prior is None:
        return (z, np.zeros(z.shape)) if with_error else z
    lab, idx = label_bits(m), np.arange(m)
    p = np.broadcast_to(np.asarray(prior).astype(wide).reshape(-1, m), (n, m))
    ls = np.stack([_log_sigmoid(-p), _log_sigmoid(p)], axis=-1)                       # [n, m, 2]: bit value 0 / 1
    with np.errstate(all="ignore"):
        e = ls[:, idx[None, :], lab].sum(-1) + z
        if not with_error:
            return e
        _, dls = df._log_sigmoid_terms(np.asarray(prior, np.float64), n, m)
        lsf = np.where(np.isfinite(ls), np.abs(ls), 0).astype(np.float64)
        dls = np.where(np.isfinite(ls), dls, 0)
        de = dls[:, idx[None, :], lab].sum(-1) + gamma(max(m - 1, 0)) * lsf[:, idx[None, :], lab].sum(-1) + U * np.abs(e)
        de = np.where(np.isfinite(e), de, 0.0)
    return e, np.asarray(de, np.float64)


def anchor_logits2llrs(z, m, method, prior=None, wide=np.float64):
    """[n, m]: +-inf where one set is all -inf, NaN where both are (tf.reduce_logsumexp / reduce_max)"""
    e = l2l_exponents(z, m, prior, wide)
    lab = label_bits(m)
    red = lse_tf if method == "app" else (lambda v: np.max(v, axis=-1))
    with np.errstate(all="ignore"):
        return np.stack([red(e[:, lab[:, i] == 1]) - red(e[:, lab[:, i] == 0]) for i in range(m)], axis=-1)


def bound_logits2llrs(z, m, method, prior=None):
    """[n, m]: items 1 (prior part), 2, 3 of tests/demap_f32.py on the logits; 0 where the anchor is not finite"""
    e, de = l2l_exponents(z, m, prior, with_error=True)
    e = np.asarray(e, np.float64)
    lab = label_bits(m)
    out = []
    for i in range(m):
        t = []
        empty = np.zeros(e.shape[0], bool)
        for b in (1, 0):
            es, ds = e[:, lab[:, i] == b], de[:, lab[:, i] == b]
            none = ~np.isfinite(es).any(-1)
            empty |= none
            es = np.where(none[:, None], 0.0, np.where(np.isfinite(es), es, _BIG))
            with np.errstate(all="ignore"):
                t.append(df._set_terms(es, ds, method, 1.0, C_EXP + 0.5, 2 ** (m - 1) - 1, None))
        out.append(np.where(empty, 0.0, df._combine(t[0], t[1], 1.0)))
    return np.stack(out, axis=-1)


# ------------------------------------------------------------------ 3. LLRs2SymbolLogits
def _l2s_terms(llrs, m, wide):
    l = np.asarray(llrs).astype(wide).reshape(-1, m)
    ls = np.stack([_log_sigmoid(-l), _log_sigmoid(l)], axis=-1)
    lab, idx = label_bits(m), np.arange(m)
    return l, ls, lab, idx


def anchor_llrs2logits(llrs, m, hard=False, wide=np.float64):
    _, ls, lab, idx = _l2s_terms(llrs, m, wide)
    out = ls[:, idx[None, :], lab].sum(-1)
    return first_argmax(out) if hard else out


def bound_llrs2logits(llrs, m):
    l, ls, lab, idx = _l2s_terms(llrs, m, np.float64)
    with np.errstate(all="ignore"):
        _, dls = df._log_sigmoid_terms(l, l.shape[0], m)
        fin = np.isfinite(ls)
        dls, lsa = np.where(fin, dls, 0), np.where(fin, np.abs(ls), 0)
        bd = SECOND_ORDER * (dls[:, idx[None, :], lab].sum(-1) + gamma(max(m - 1, 0)) * lsa[:, idx[None, :], lab].sum(-1))
    return np.where(np.isfinite(ls[:, idx[None, :], lab].sum(-1)), bd, 0.0)


# ------------------------------------------------------------------ 4. SymbolLogits2Moments
def anchor_moments(z, points, wide=np.float64):
    pts = np.asarray(points).astype(np.complex128)
    z = np.asarray(z).astype(wide).reshape(-1, len(pts))
    xr, xi = pts.real.astype(wide), pts.imag.astype(wide)
    with np.errstate(all="ignore"):
        mx = np.max(z, axis=-1, keepdims=True) if z.shape[0] else z[:, :1]
        p = np.exp(z - np.where(np.isfinite(mx), mx, 0))               # (softmax as exp(z - max) / sum: no lse of 1e6 is formed)
        p = p / p.sum(-1, keepdims=True)
        mr, mi = (p * xr).sum(-1), (p * xi).sum(-1)
        var = (p * ((xr - mr[:, None]) ** 2 + (xi - mi[:, None]) ** 2)).sum(-1)
    return mr, mi, var


def bound_moments(z, points):
    """(bound on Re mean, on Im mean, on var), each [n]"""
    pts = np.asarray(points).astype(np.complex128)
    P = len(pts)
    z = np.asarray(z, np.float64).reshape(-1, P)
    mr, mi, _ = anchor_moments(z, pts)
    if z.shape[0] == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    with np.errstate(all="ignore"):
        zf = np.where(np.isfinite(z), z, _BIG)
        t = zf - zf.max(-1, keepdims=True)
        p = np.exp(t)
        p = p / p.sum(-1, keepdims=True)
        term = np.where(p > 0, U * np.abs(t) + C_EXPF * U, 0.0)
        delta = term + (p * term).sum(-1, keepdims=True) + gamma(P - 1) + U
        tiny = 2.0 ** -125
        bm = []
        for x in (pts.real, pts.imag):
            ax = np.abs(x)[None, :]
            bm.append(SECOND_ORDER * ((delta * p * ax).sum(-1) + gamma(P) * (p * ax).sum(-1) + P * tiny * ax.max()))
        dm = np.hypot(bm[0], bm[1])
        d2 = (pts.real[None, :] - mr[:, None]) ** 2 + (pts.imag[None, :] - mi[:, None]) ** 2
        bv = SECOND_ORDER * (((delta + gamma(P + 4)) * p * d2).sum(-1) + (p * (2 * np.sqrt(d2) * dm[:, None] + dm[:, None] ** 2)).sum(-1)
                             + P * tiny * d2.max())
    return bm[0], bm[1], bv


# ------------------------------------------------------------------ 5. PAM2QAM (logits)
def pam2qam_table(nbh):
    """t(i, j): the QAM index whose label interleaves the labels of i and j (mapping.py:1278-1291)"""
    lab = label_bits(nbh)
    P = 1 << nbh
    b = np.zeros([P, P, 2 * nbh], np.int64)
    b[:, :, 0::2] = lab[:, None, :]
    b[:, :, 1::2] = lab[None, :, :]
    return np.sum(b * (1 << np.arange(2 * nbh - 1, -1, -1)), -1)


def anchor_pam2qam(pam1, pam2, nbh, dtype=np.float32):
    """the flattened P x P matrix pam1_i + pam2_j GATHERED with the flattened table (mapping.py:1304-1314), each sum rounded once to
    ``dtype``"""
    P = 1 << nbh
    a, b = np.asarray(pam1, np.float64).reshape(-1, P), np.asarray(pam2, np.float64).reshape(-1, P)
    wide = WIDE if dtype == np.float64 else np.float64
    flat = (a.astype(wide)[:, :, None] + b.astype(wide)[:, None, :]).astype(dtype).reshape(-1, P * P)
    return flat[:, pam2qam_table(nbh).reshape(-1)]


# ------------------------------------------------------------------ comparison
def ratio(out, an, bd):
    """max |out - anchor| / bound and its index over the outputs whose anchor is finite.  Where the anchor is +-inf the output must
    equal it, where it is NaN anything goes; a NaN or inf elsewhere counts as inf"""
    out = np.asarray(out, np.float64).reshape(an.shape)
    an64 = np.asarray(an, np.float64)
    fin = np.isfinite(an64)
    with np.errstate(all="ignore"):
        err = np.abs((out.astype(an.dtype) - an).astype(np.float64))
        q = np.where(fin, np.where(np.isfinite(out), err / np.where(bd > 0, bd, 1.0), np.inf), 0.0)
        q = np.where(fin & (bd == 0) & (err == 0), 0.0, q)
        q = np.where(np.isinf(an64), np.where(out == an64, 0.0, np.inf), q)
    if q.size == 0:
        return 0.0, ()
    at = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[at]), tuple(int(i) for i in at)


def worst(outs, ex):
    """largest ratio over the outputs of a case (``ex``: symbol_cases.Expected), and (output, index ...)"""
    q = [ratio(o, a, b) for o, a, b in zip(outs, ex.anchors, ex.bounds)]
    k = int(np.argmax([v[0] for v in q]))
    return q[k][0], (k,) + q[k][1]


def round_trip_ratio(llrs, logits, back, bd_logits, m, scale=1.0):
    """LLRs2SymbolLogits -> SymbolLogits2LLRs("app"): ``back`` against the LLRs themselves, within the second block's bound on the
    first block's output plus the first block's bounds carried through - an LLR is a difference of two reductions over logits, each
    off by at most the row's largest logit bound.  ``scale``: 2^-29 for the float64 kernels (``bd_logits`` already carries it)"""
    an = np.asarray(llrs, np.float64).reshape(-1, m)
    bd = bound_logits2llrs(logits, m, "app") * scale + 2 * bd_logits.max(-1, keepdims=True)
    return ratio(back, an, np.where(np.isfinite(an), bd, 0.0))[0]
