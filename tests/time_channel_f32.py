"""Float64 anchors and derived per-output error bounds of the time-domain channel kernels: ``cir_to_time_channel``
(csrc/ofdm_time.hip ``cir_to_time_kernel``; csrc/f64_time.hip ``cir_to_time128_kernel`` + ``time_normalize128_kernel``) and
``ApplyTimeChannel`` (``apply_time_kernel``, ``apply_time128_kernel``).

    h[b, rx, ra, tx, ta, t, l] = sum_p a[b, rx, ra, tx, ta, p, t] g_pl,   g_pl = sinc(x_pl),   x_pl = l_min + l - tau[b, rx, tx, p] W
    y[b, rx, ra, t]            = sum_{tx, ta} sum_{l = lo}^{hi} h[b, rx, ra, tx, ta, t, l] x[b, tx, ta, t - l]

with sinc(x) = sin(pi x) / (pi x), lo = max(0, t - (Tn - 1)), hi = min(t, L - 1); with ``normalize`` every (b, rx, tx) link of h is
divided by c = sqrt(mean over (ra, ta, t) of sum_l |h|^2), a link without energy mapping to 0.  The kernels take sin from the
device library and are therefore not bit-equal to a host specification; they are held to ``|out - anchor| <= bound`` on every
output.  The bounds read the inputs only - never anything a kernel returned.  One parameter ``u`` makes the same functions serve
the float32 kernels (u = 2^-24) and the float64 kernels (u = 2^-53).

The bandwidth.  The reference multiplies ``tau * bandwidth`` with tau a float32 tensor and the bandwidth a Python number
(channel/utils.py:330): the number is converted to the tensor's dtype first, so the reference's W IS float32(bandwidth) in single
precision; the C entry takes it as a C ``float`` likewise.  The anchor therefore uses W = float32(bandwidth) for u = 2^-24 and
the double as given for u = 2^-53; a, tau and W enter with their stored values exactly.

Notation: u the unit roundoff (a rounding moves x by at most u |x|), gamma(n) = n u / (1 - n u), y = pi x.  The library is built
without contraction (-ffp-contract=off): every product and every sum below is one rounding; a fused form has fewer.

cir_to_time_channel, per weight g_pl:

1. Argument.  ``(float)(l_min + l) - tau W``: l is exact, the product one rounding, the difference one:
   |x^ - x| <= dx = u (|tau W| + |x|) (1 + u).  The error is the cancellation in l - tau W: proportional to |tau W|.
2. ``pi_f * x^``.  |float32(pi) - pi| = 8.75e-8 = 0.47 u pi (the double constant: 0.35 u pi) and one rounding:
   |y^ - y| <= dy = (1.47 u |y| + pi dx)(1 + 2 u).
3. s(y) = sin y / y has |s'(y)| = |cos y / y - sin y / y^2| <= min(1/2, 2 / |y|) (the maximum of |s'| is 0.4362; beyond |y| = 1,
   1/|y| + 1/y^2 <= 2/|y|), taken at |y| - dy to hold on the whole interval: |s(y^) - s(y)| <= lip dy.
4. ``sinf`` is within C_SC ulp of sin y^ and ulp(v) <= 2 u |v|: a relative 2 C_SC u; the quotient is one rounding (the
   toolchain's float32 division is correctly rounded by default).  C_SC = 4 as in tests/channel_f32.py: ROCm's accuracy table
   is not among the documents shipped with the toolchain, so the 4 ulp that the OpenCL full profile requires of sin stand in - a
   property of the library, not of the code under test.  Together
       e_pl = lip dy + (2 C_SC + 1) u (1 + 2 C_SC u)(|g_pl| + lip dy).
   x == 0 exactly (tau W an integer of the lag window, tau = 0 at l = -l_min): the product and the difference are exact, the
   kernel returns the constant 1: e_pl = 0.
5. Accumulation.  A component of an output is sum_p fl(a_p g^_pl) added in ascending p onto 0: a product passes its own
   rounding and at most P additions: gamma(P + 1) sum_p |a_p| |g^_pl| per output in modulus (the weights are real: the two
   components of a path's contribution form a vector of length |a_p| |g^_pl|).
6. The anchor's own float64 evaluation: the same terms with 2^-53: lip dy <= 2^-53 (1.6 |tau W| + 5), sin and quotient 5 more,
   the sum P + 1: 2^-50 (max_p |tau_p W| + P + 2) A with A = sum_p |a_p| covers it.

    B = sum_p |a_p| [ e_pl + gamma(P + 1)(|g_pl| + e_pl) ] + 2^-50 (max_p |tau_p W| + P + 2) A                 (unnormalised)

7. Normalisation, as item 5 of tests/channel_f32.py with this kernel's energy chain.  inv = 1 / sqrtf(E / n), n = RA TA T, E the
   float32 sum of fl(fl(x^2) + fl(y^2)) over the RA TA T L outputs of the link:
   - the energy is that of the COMPUTED outputs: |c(computed) - c64| <= c(computed - h64) <= c(B) (triangle inequality in l2):
     rho_d = c(B) / c64;
   - a term is three roundings old when it has joined a thread's chain, the chain is RA TA ceil(T / 256) L terms long (one lane
     per time step, 256 per block pass), the 256 partial sums meet in a tree of 8 levels: depth = 3 + RA TA ceil(T/256) L + 8.
     The float64 second pass walks ceil(RA TA T L / 256) terms per thread and the same tree: no deeper;
   - E / n: n < 2^24 exact, the division 2.5 ulp (5 u); sqrtf 3 ulp (6 u); 1 / c 2.5 ulp (5 u) - the OpenCL full-profile figures
     that tests/channel_f32.py uses, in either order of division and root:
     rho_f = (gamma(depth) + 5 u) / 2 / (1 - gamma(depth) - 5 u) + 11 u;
   - inv = (1 / c64)(1 + e), |e| <= rho = r / (1 - r), r = rho_d + rho_f                                       (``bound_scale``)
   - the stored value is one more rounding: rho' = rho + u + rho u.

    B_n = B / c64 (1 + rho') + |h64_n| rho'                                                                    (normalised)

   A link whose taps are all zero: every product is an exact zero, E = 0, inv = 0: output, scale and bounds are exactly 0.

ApplyTimeChannel, per output: N = TX TA (hi - lo + 1) complex multiply-adds.  A component is N times two products, their
difference (sum) and the addition onto the accumulator: a product passes at most N + 2 roundings, a fused form at most 2 N;
gamma(2 N + 2) covers every order.  The error vector of the two components is at most sqrt(2) gamma(2 N + 2) S long, S = sum
|h| |x| over the window (Cauchy-Schwarz with 2 |cos sin| <= 1, item 3 of tests/channel_f32.py).  With ``link_scale`` the tap is
fl(h s) - one more rounding on every tap: gamma(2 N + 3), and the anchor multiplies h s exactly.  The anchor's own float64
sum, in whatever order: sqrt(2) gamma_64(2 N + 2) S = 2.9 (N + 1) 2^-53 S <= 2^-50 (N + 1) S.

    B_y = [ sqrt(2) gamma(2 N + 2 [+ 1]) + 2^-50 (N + 1) ] sum_{tx, ta, l} |h| |s| |x|
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
C_SC = 4.0            # ulp of sin: OpenCL full profile (no ROCm accuracy table on the build machine)


def _gamma(n, u):
    return n * u / (1 - n * u)


def _cir_inputs(bandwidth, a, tau, l_min, l_max, u):
    a, tau = np.asarray(a), np.asarray(tau)
    b, rx, ra, tx, ta, p, t = a.shape
    assert tau.shape == (b, rx, tx, p) and l_max >= l_min and u in (U32, U64)
    w = float(np.float32(bandwidth)) if u == U32 else float(bandwidth)
    lags = np.arange(int(l_min), int(l_max) + 1, dtype=np.float64)
    return w, a.astype(np.complex128), tau.astype(np.float64), lags


def _sinc(x):
    y = np.pi * x
    return np.where(x == 0, 1.0, np.sin(y) / np.where(x == 0, 1.0, y))


def _link_c(h):
    """h [b, rx, ra, tx, ta, t, l] -> sqrt(mean over (ra, ta, t) of sum_l |h|^2) per (b, rx, tx), broadcastable to h"""
    return np.sqrt(np.mean(np.sum(np.abs(h) ** 2, axis=6, keepdims=True), axis=(2, 4, 5), keepdims=True))


def anchor_cir(bandwidth, a, tau, l_min, l_max, normalize, u=U32):
    """complex128 [b, rx, ra, tx, ta, t, L] from the inputs as stored; W = float32(bandwidth) for u = 2^-24 (module docstring)"""
    w, a, tau, lags = _cir_inputs(bandwidth, a, tau, l_min, l_max, u)
    g = _sinc(lags - (tau * w)[..., None])                                       # [b, rx, tx, p, L]
    h = np.einsum("brxyzpt,brypl->brxyztl", a, g)
    if normalize:
        c = _link_c(h)
        h = np.where(c > 0, h / np.where(c > 0, c, 1.0), 0.0)
    return h


def _cir_unnormalised(bandwidth, a, tau, l_min, l_max, u):
    w, a, tau, lags = _cir_inputs(bandwidth, a, tau, l_min, l_max, u)
    p = a.shape[5]
    tw = np.abs(tau * w)[..., None]                                              # [b, rx, tx, p, 1]
    x = lags - (tau * w)[..., None]
    ax, y = np.abs(x), np.pi * np.abs(x)
    g = np.abs(_sinc(x))
    dx = u * (tw + ax) * (1 + u)
    dy = (1.47 * u * y + np.pi * dx) * (1 + 2 * u)
    lip = np.minimum(0.5, 2.0 / np.maximum(y - dy, 1e-300))
    e = lip * dy + (2 * C_SC + 1) * u * (1 + 2 * C_SC * u) * (g + lip * dy)
    e = np.where(x == 0, 0.0, e)
    wgt = e + _gamma(p + 1, u) * (g + e)                                         # [b, rx, tx, p, L]
    absa = np.abs(a)
    bu = np.einsum("brxyzpt,brypl->brxyztl", absa, wgt)
    big_a = np.sum(absa, axis=5)[..., None]                                      # [b, rx, ra, tx, ta, t, 1]
    tw_max = np.max(tw, axis=3)[:, :, None, :, None, None, :]                    # [b, rx, 1, tx, 1, 1, 1]
    return bu + 2.0 ** -50 * (tw_max + p + 2) * big_a


def _cir_rho(bandwidth, a, tau, l_min, l_max, u):
    """-> bu, h64 (unnormalised), c64, live, rho (relative error of inv before the last product)"""
    bu = _cir_unnormalised(bandwidth, a, tau, l_min, l_max, u)
    h = anchor_cir(bandwidth, a, tau, l_min, l_max, False, u)
    c = _link_c(h)
    live = c > 0
    cs = np.where(live, c, 1.0)
    b, rx, ra, tx, ta, p, t = np.asarray(a).shape
    depth = 3 + ra * ta * (-(-t // 256)) * h.shape[6] + 8
    gd = _gamma(depth, u) + 5 * u
    rho_f = gd / 2 / (1 - gd) + 11 * u
    r = _link_c(bu) / cs + rho_f
    return bu, h, cs, live, r / (1 - r)


def bound_cir(bandwidth, a, tau, l_min, l_max, normalize, u=U32):
    """float64 [b, rx, ra, tx, ta, t, L]: how far a kernel of unit roundoff ``u`` may be from ``anchor_cir`` in modulus"""
    if not normalize:
        return _cir_unnormalised(bandwidth, a, tau, l_min, l_max, u)
    bu, h, cs, live, rho = _cir_rho(bandwidth, a, tau, l_min, l_max, u)
    rho = rho + u + rho * u
    return np.where(live, bu / cs * (1 + rho) + np.abs(h) / cs * rho, 0.0)


def anchor_scale(bandwidth, a, tau, l_min, l_max, u=U32):
    """float64 [b, rx, tx]: 1 / c64 of the deferred normalisation, 0 for a link without energy"""
    c = _link_c(anchor_cir(bandwidth, a, tau, l_min, l_max, False, u))[:, :, 0, :, 0, 0, 0]
    return np.where(c > 0, 1.0 / np.where(c > 0, c, 1.0), 0.0)


def bound_scale(bandwidth, a, tau, l_min, l_max, u=U32):
    """float64 [b, rx, tx]: how far the factor of the deferred path (``_defer_norm=True``) may be from ``anchor_scale``"""
    _, _, cs, live, rho = _cir_rho(bandwidth, a, tau, l_min, l_max, u)
    return np.where(live, rho / cs, 0.0)[:, :, 0, :, 0, 0, 0]


def _apply_terms(x, h, link_scale):
    x, h = np.asarray(x), np.asarray(h)
    b, rx, ra, tx, ta, tout, l_tot = h.shape
    tn = tout - l_tot + 1
    assert x.shape == (b, tx, ta, tn) and tn >= 1
    x, h = x.astype(np.complex128), h.astype(np.complex128)
    if link_scale is not None:
        s = np.asarray(link_scale).astype(np.float64)
        assert s.shape == (b, rx, tx)
        h = h * s[:, :, None, :, None, None, None]                               # exact: products of two float32 values
    t = np.arange(tout)[:, None]
    l = np.arange(l_tot)[None, :]
    ok = (t - l >= 0) & (t - l < tn)                                             # [tout, L]: lo <= l <= hi
    xs = np.where(ok, x[:, :, :, np.clip(t - l, 0, tn - 1)], 0.0)                # [b, tx, ta, tout, L]
    n = tx * ta * ok.sum(axis=1)                                                 # [tout]
    return h, xs, n


def anchor_apply(x, h, link_scale=None):
    """complex128 [b, rx, ra, tout]; with ``link_scale`` [b, rx, tx] the taps are h s, multiplied exactly"""
    h, xs, _ = _apply_terms(x, h, link_scale)
    return np.einsum("brxyztl,byztl->brxt", h, xs)


def bound_apply(x, h, link_scale=None, u=U32):
    """float64 [b, rx, ra, tout]: how far a kernel of unit roundoff ``u`` may be from ``anchor_apply`` in modulus"""
    h, xs, n = _apply_terms(x, h, link_scale)
    s = np.einsum("brxyztl,byztl->brxt", np.abs(h), np.abs(xs))
    k = 2 * n + 2 + (0 if link_scale is None else 1)
    return (np.sqrt(2.0) * _gamma(k, u) + 2.0 ** -50 * (n + 1)) * s


def ratio(out, ref, bd):
    """max over the outputs of |out - anchor| / bound (0 / 0 counts as 0, x / 0 as inf): what the tests assert to be <= 1"""
    out, ref, bd = np.asarray(out), np.asarray(ref), np.asarray(bd)
    assert out.shape == ref.shape == bd.shape, (out.shape, ref.shape, bd.shape)
    if out.size == 0:
        return 0.0
    err = np.abs(out.astype(ref.dtype) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bd)
    q = np.where(np.isnan(q), np.inf, q)
    return float(np.max(q))
