"""Float64 anchor and derived per-output error bound of the TDL tap generators: ``tdl_cir_kernel`` (csrc/ofdm.hip, float32) and
``tdl_cir128_kernel`` (csrc/f64_ofdm.hip, float64).

    a[b, ra, ta, p, t] = sqrt(P_p / N) sum_n exp(j (d_b t/fs cos(alpha_bpn) + phi_{b,ra,ta,p,n}))
                         [+ sqrt(P_los) exp(j (d_b t/fs cos(aoa) + phi0_b)) at p = 0],     alpha_bpn = 2 pi (n + 1) / N + theta_bpn

The anchor takes the STORED draws (``oracle.ofdm._u``: float32 for u = 2^-24; ``oracle.f64_ofdm._u``, the float64 mapping of the same
24-bit uniforms, for u = 2^-53), fs = float32(sampling_frequency), the float32 ``mean_powers``, ``los_power`` and angle of arrival
(the C entry takes them as ``float``; the doubles as given for u = 2^-53) and evaluates the formula above in float64.  The kernels
take sin / cos from the device library and are not bit-equal to a host specification: they are held to ``|a - anchor| <= bound`` on
every output.  The bound reads the inputs and the draws only - never anything a kernel returned.

Notation: u the unit roundoff, gamma(n) = n u / (1 - n u), D_t = |d t / fs|, A_n = 2 pi (n + 1) / N.  The library is built with
-ffp-contract=off: every product and every sum is one rounding.  Library constants as in tests/time_channel_f32.py (OpenCL full
profile): sin / cos C_SC = 4 ulp (a relative 2 C_SC u), division 2.5 ulp (5 u), sqrt 3 ulp (6 u).

Per sinusoid n of an output at step t = t0 + k (t0 a multiple of 16, k <= 15; the float64 kernel: t0 = t, k = 0):

1. alpha.  ``(2.f * pi / (float)N) * (float)(n + 1) + theta``: float32(pi) is 0.47 u off (the double constant less), the quotient
   5 u, the product u, the sum u |alpha|.  The interval end ``pi / (float)N`` of the theta draw is 5.47 u pi / N from the exact one and the
   anchor's stored float32(pi / N) another u: the two draws ``lo + (hi - lo) u01`` differ by at most three times that plus their two
   roundings:          d_alpha = (6.47 A_n + |alpha|) u + 22.4 u pi / N.
2. ``cosf(alpha)``: |cos'| <= 1 and 2 C_SC u of the library:  d_ca = d_alpha + 2 C_SC u.
3. The direct argument ``d * ((float)t0 / fs) * ca + phi``: quotient 5 u, two products, one sum.  With |ca| <= 1:
       e_0 = D_t0 (d_ca + 7 u) + u (D_t0 + |phi|)        - proportional to |d t| and |phi|.
4. ``sincosf``: each component within 2 C_SC u of itself: a vector of length <= 2 C_SC u.
5. Rotation (float32 kernel only).  w = d (1 / fs) ca carries the same relative error as item 3: |w^ - w| <= W (d_ca + 7 u), W = |d / fs|;
   (cos w^, sin w^) is 2 C_SC u long in error; a packed multiply-add step (two products, one sum per component) adds 2 sqrt(2) u of
   the vector's length.  k steps:   e_rot = k [W (d_ca + 7 u) + (2 C_SC + 2 sqrt 2) u].  D_t0 + k W = D_t: items 3 and 5 together are
       e_n = D_t (d_ca + 7 u) + u (D_t0 + |phi|) + 2 C_SC u + k (2 C_SC + 2 sqrt 2) u.
   The float64 kernel evaluates every step directly: k = 0 (``rotation=False``; the float32 oracle likewise).
6. Accumulation over N in ascending n onto 0: sqrt(2) gamma(N) sum_n (1 + e_n) in modulus.
7. Scale ``amp * (acc * norm)``: two roots (6 u each), a quotient (5 u), two products: gamma(19) of the scaled sum.
8. LoS at p = 0: cos(aoa) 2 C_SC u (+ u |aoa| for the angle's own float32 rounding); argument as item 3; sincos; sqrt(P_los) 6 u; one
   product; the sum onto the tap one rounding of the result:
       e_los = D_t (2 C_SC u + u |aoa| + 7 u) + u (D_t + |phi0|) + (2 C_SC + 7) u.
9. The anchor's own float64 evaluation: 2^-50 (D_t + N + 4) (sqrt(P_p N) + sqrt(P_los)).

    B = sqrt(P_p / N) [ (1 + gamma(19)) (sum_n e_n + sqrt(2) gamma(N) sum_n (1 + e_n)) + gamma(19) |sum_n exp(j arg_n)| ]
        + [p = 0] sqrt(P_los) e_los + u |a| + item 9,   all times (1 + 64 u) for the second-order terms.

10. The same count per COMPONENT (``bound_re``, ``bound_im``; ``ratio_parts``).  The modulus bound B grants every sinusoid a disc of
    2 C_SC u, yet the library's 4 ulp are 4 ulp of each returned value: |d cos| <= 2 C_SC u |cos|.  With c_n + j s_n = exp(j arg_n):
    - an argument error E_n = D_t (d_ca + 7 u) + [D_t0 > 0] u (D_t0 + |phi|) is tangential: |d c_n| <= |s_n| E_n + E_n^2, |d s_n| <= |c_n| E_n
      + E_n^2.  At D_t0 = 0 the product ``d * 0 * ca`` is an exact 0 and ``0 + phi`` is exact: the argument IS the stored phi;
    - ``sincosf`` at a directly evaluated step (k = 0): 2 C_SC u |c_n| resp. |s_n|; behind k > 0 rotations the error vector of the
      chunk's first step has turned with the sinusoid: 2 C_SC u on either component, and k (2 C_SC + 2 sqrt 2) u as in item 5;
    - accumulation gamma(N) sum_n (|c_n| + e_n), scale gamma(19) |Re sum| - both act on a component;
    - LoS: |sin arg0| E_los + (2 C_SC + 7) u |cos arg0| + E_los^2, E_los = D_t (2 C_SC u + u |aoa| + 7 u) + [D_t > 0] u (D_t + |phi0|).
    A tap at t = 0 whose phase lies near a multiple of pi / 2 is thereby held to a few ulp of its SMALL component: a phase that is off
    by one ulp of pi - invisible inside a disc of 8 u - leaves bound_re or bound_im there.

Spatial correlation (``correlate``): out_i = sum_j M_ij a_j, M stored in the block's precision (one u per entry in modulus), a complex
product and ascending sum over n = RA TA terms: sqrt(2) gamma(n + 2) sum_j |M_ij| |a_j| + sum_j |M_ij| B_j (1 + gamma(n + 2)).
"""
import numpy as np

from oracle import f64_ofdm as o64
from oracle import ofdm as o32

U32 = 2.0 ** -24
U64 = 2.0 ** -53
C_SC = 4.0
C_DIV = 5.0           # 2.5 ulp
C_SQRT = 6.0          # 3 ulp
PI = np.pi
K_CHUNK = 16


def _gamma(n, u):
    return n * u / (1 - n * u)


def draws(seed, call, batch, ra, ta, p, n, min_doppler, max_doppler, u=U32):
    """the stored draws as float64: d [B], theta [B, P, N], phi [B, RA, TA, P, N], phi0 [B]"""
    _u = o32._u if u == U32 else o64._u
    d = np.asarray(_u(seed, call, batch, min_doppler, max_doppler), np.float64)
    theta = np.asarray(_u(seed, call + 1, batch * p * n, -PI / n, PI / n), np.float64).reshape(batch, p, n)
    phi = np.asarray(_u(seed, call + 2, batch * ra * ta * p * n, -PI, PI), np.float64).reshape(batch, ra, ta, p, n)
    phi0 = np.asarray(_u(seed, call + 3, batch, -PI, PI), np.float64)
    return d, theta, phi, phi0


def _inputs(fs, mean_powers, los_power, los_aoa, u):
    if u == U32:
        return (float(np.float32(fs)), np.asarray(np.asarray(mean_powers, np.float32), np.float64),
                None if los_power is None else float(np.float32(los_power)), float(np.float32(los_aoa)))
    return float(fs), np.asarray(mean_powers, np.float64), None if los_power is None else float(los_power), float(los_aoa)


def anchor_and_bound(*args, **kw):
    """-> anchor complex128, bound float64 (in modulus), both [B, 1, RA, 1, TA, P, T]; arguments of ``anchor_and_bounds``"""
    return anchor_and_bounds(*args, **kw)[:2]


def anchor_and_bounds(seed, call, batch, num_time_steps, sampling_frequency, mean_powers, min_doppler, max_doppler, num_rx_ant=1,
                      num_tx_ant=1, num_sinusoids=20, los_power=None, los_aoa=PI / 4, u=U32, rotation=None):
    """-> anchor complex128, bound (modulus), bound_re, bound_im float64 (item 10), each [B, 1, RA, 1, TA, P, T].  ``rotation``: the
    chain of item 5 (default: the float32 kernel has it, the float64 kernel not)"""
    assert u in (U32, U64)
    rotation = (u == U32) if rotation is None else rotation
    b, ra, ta, t_, n_ = int(batch), int(num_rx_ant), int(num_tx_ant), int(num_time_steps), int(num_sinusoids)
    fs, mp, plos, aoa = _inputs(sampling_frequency, mean_powers, los_power, los_aoa, u)
    p_ = len(mp)
    d, theta, phi, phi0 = draws(seed, call, b, ra, ta, p_, n_, min_doppler, max_doppler, u)
    tt = np.arange(t_, dtype=np.float64)
    k = (tt % K_CHUNK) if rotation else np.zeros(t_)
    dt = np.abs(d)[:, None] * tt[None, :] / fs                                     # [B, T]
    dt0 = np.abs(d)[:, None] * (tt - k)[None, :] / fs
    big_a = 2 * PI * np.arange(1, n_ + 1) / n_                                      # [N]
    alpha = big_a + theta                                                          # [B, P, N]
    d_ca = (6.47 * big_a + np.abs(alpha)) * u + 22.4 * u * PI / n_ + 2 * C_SC * u   # [B, P, N]
    ca = np.cos(alpha)
    sc = np.sqrt(mp / n_)                                                          # [P]
    anchor = np.zeros((b, ra, ta, p_, t_), np.complex128)
    e_sum = np.zeros((b, ra, ta, p_, t_))
    krot = (k * (2 * C_SC + 2 * np.sqrt(2.0)) * u)[None, None, :]
    live0 = (dt0 > 0)[:, None, :]                                                  # [B, 1, T]: d t0 = 0: product and sum are exact
    s_re, s_im, abs_c, abs_s = (np.zeros((b, ra, ta, p_, t_)) for _ in range(4))
    for n in range(n_):                                                            # [B, RA, TA, P, T] per sinusoid: no N-fold temporary
        arg = (d[:, None, None] * ca[:, :, n, None] * (tt / fs)[None, None, :])[:, None, None] + phi[..., n, None]
        z = np.exp(1j * arg)
        anchor += z
        e_arg = dt[:, None, :] * (d_ca[:, :, n, None] + 7 * u)                     # [B, P, T]
        e_bpt = e_arg + u * dt0[:, None, :] + 2 * C_SC * u + krot
        e_sum += e_bpt[:, None, None] + u * np.abs(phi[..., n, None])
        e_ph = (e_arg + live0 * u * dt0[:, None, :])[:, None, None] + live0[:, None, None] * u * np.abs(phi[..., n, None])
        ac, as_ = np.abs(z.real), np.abs(z.imag)
        s_re += as_ * e_ph + 2 * C_SC * u * np.where(k > 0, 1.0, ac) + krot + e_ph ** 2
        s_im += ac * e_ph + 2 * C_SC * u * np.where(k > 0, 1.0, as_) + krot + e_ph ** 2
        abs_c += ac
        abs_s += as_
    g19 = _gamma(1 + 2 * C_SQRT + C_DIV + 2, u)
    bound = sc[:, None] * ((1 + g19) * (e_sum + np.sqrt(2.0) * _gamma(n_, u) * (n_ + e_sum)) + g19 * np.abs(anchor))
    b_re = sc[:, None] * ((1 + g19) * (s_re + _gamma(n_, u) * (abs_c + e_sum)) + g19 * np.abs(anchor.real))
    b_im = sc[:, None] * ((1 + g19) * (s_im + _gamma(n_, u) * (abs_s + e_sum)) + g19 * np.abs(anchor.imag))
    anchor *= sc[:, None]
    own = (sc * n_)[:, None] * np.ones((b, 1, 1, 1, 1))
    if plos is not None:
        kf = np.sqrt(plos)
        arg0 = d[:, None] * (tt / fs)[None, :] * np.cos(aoa) + phi0[:, None]         # [B, T]
        z0 = np.exp(1j * arg0)
        anchor[:, :, :, 0, :] += (kf * z0)[:, None, None]
        e_los = dt * (2 * C_SC * u + u * abs(aoa) + 7 * u) + u * (dt + np.abs(phi0)[:, None]) + (2 * C_SC + 7) * u
        bound[:, :, :, 0, :] += (kf * e_los)[:, None, None]
        l_ph = dt * (2 * C_SC * u + u * abs(aoa) + 7 * u) + (dt > 0) * u * (dt + np.abs(phi0)[:, None])
        b_re[:, :, :, 0, :] += (kf * (np.abs(z0.imag) * l_ph + (2 * C_SC + 7) * u * np.abs(z0.real) + l_ph ** 2))[:, None, None]
        b_im[:, :, :, 0, :] += (kf * (np.abs(z0.real) * l_ph + (2 * C_SC + 7) * u * np.abs(z0.imag) + l_ph ** 2))[:, None, None]
        own = own + kf * (np.arange(p_) == 0)[:, None]
    own = 2.0 ** -50 * (dt[:, None, None, None, :] + n_ + 4) * own
    bound = (bound + u * np.abs(anchor)) * (1 + 64 * u) + own
    b_re = (b_re + u * np.abs(anchor.real)) * (1 + 64 * u) + own
    b_im = (b_im + u * np.abs(anchor.imag)) * (1 + 64 * u) + own
    return tuple(x[:, None, :, None] for x in (anchor, bound, b_re, b_im))


def ratio_parts(out, ref, b_re, b_im):
    """-> (max over the outputs of max(|Re(out - anchor)| / bound_re, |Im(out - anchor)| / bound_im), its index)"""
    out = np.asarray(out).astype(np.complex128)
    qr, ir = ratio(out.real, np.asarray(ref).real, b_re)
    qi, ii = ratio(out.imag, np.asarray(ref).imag, b_im)
    return (qr, ir) if qr >= qi else (qi, ii)


def correlate(anchor, bound, mat, u=U32):
    """anchor, bound [B, 1, RA, 1, TA, P, T], mat [RA TA, RA TA] complex128 (the float64 square root) -> the same pair behind
    ``samd_spatial_corr``"""
    b, _, ra, _, ta, p, t = anchor.shape
    n = ra * ta
    mat = np.asarray(mat, np.complex128)
    assert mat.shape == (n, n)
    v = anchor.reshape(b, n, p, t)
    am = np.abs(mat)
    g = _gamma(n + 2, u)
    out = np.einsum("ij,bjpt->bipt", mat, v)
    bd = np.sqrt(2.0) * g * np.einsum("ij,bjpt->bipt", am, np.abs(v)) + (1 + g) * np.einsum("ij,bjpt->bipt", am, bound.reshape(b, n, p, t))
    bd = bd + 2.0 ** -50 * (n + 1) * np.einsum("ij,bjpt->bipt", am, np.abs(v))
    return out.reshape(anchor.shape), bd.reshape(anchor.shape)


def ratio(out, ref, bd):
    """-> (max over the outputs of |out - anchor| / bound, its index); 0 / 0 counts as 0, x / 0 as inf"""
    out, ref, bd = np.asarray(out), np.asarray(ref), np.asarray(bd)
    assert out.shape == ref.shape == bd.shape, (out.shape, ref.shape, bd.shape)
    if out.size == 0:
        return 0.0, ()
    err = np.abs(out.astype(ref.dtype) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bd)
    q = np.where(np.isnan(q), np.inf, q)
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[i]), tuple(int(j) for j in i)
