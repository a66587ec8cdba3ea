"""Float64 anchor and derived per-output error bound of ``cir_to_ofdm_channel`` in single precision (csrc/ofdm.hip:
``cir_to_ofdm_kernel``, ``cir_to_ofdm_reg_kernel``, ``cir_to_ofdm_pass_kernel``, ``cir_to_ofdm_fused_kernel``).

    h[b, rx, ra, tx, ta, t, f] = sum_p a[b, rx, ra, tx, ta, p, t] exp(-j 2 pi freqs[f] tau[b, rx, tx, p])

and with ``normalize`` every (b, rx, tx) link is divided by its root mean square over (ra, ta, t, f), a link without energy
mapping to 0.  The four kernels sum the same products in different orders and take sin / cos from the device library, so
they are not bit-equal to a host specification; they are held to ``|h - anchor| <= bound`` on every output instead.  The
bound reads the inputs only - never anything a kernel returned.

Notation: u = 2^-24 (unit roundoff of float32: a rounding moves x by at most u |x|), gamma(n) = n u / (1 - n u),
A = sum_p |a_p| over the paths of one output, theta_p = -2 pi f tau_p the exact phase of path p.

1. Argument.  The kernels form ``fl(fl(c f) tau)`` with c = -2 * float32(pi).  |float32(pi) - pi| = 8.75e-8 = 0.47 u pi, the
   two products are one rounding each: the argument is theta (1 + d), |d| <= (1 + 0.47 u)(1 + u)^2 - 1 < 2.5 u.  Since
   |e^{jx} - e^{jy}| <= |x - y| the phase factor moves by at most 2.5 u |theta_p|.  (tau = 0 or f = 0: exactly 0.)
2. sin / cos.  Each within C_SC ulp of the true value at the rounded argument.  ulp(x) <= 2 u |x|, so the error vector of
   (cos, sin) is at most 2 C_SC u sqrt(cos^2 + sin^2) = 2 C_SC u long.  C_SC = 4: ROCm's accuracy table of the device
   ``sincosf`` is not among the documents shipped with the toolchain this suite builds with, so the 4 ulp that the OpenCL
   full profile requires of sin and cos stand in.  A property of the library, not of the code under test.
   Together the stored phase factor is e^{j theta_p} + d_p with |d_p| <= PHI_p u, PHI_p = 2.5 |theta_p| + 2 C_SC.
3. Accumulation.  A component of an output is a chain of 2 P fused multiply-adds (padded paths add an exact 0 * x): the
   first-order bound of a recursive sum is (number of roundings) u sum |term|.  The register-staged kernel runs two chains of
   P and joins them with one more rounding: P + 1 <= 2 P + 1.  With n = 2 P + 2 (one rounding in hand) a component is off by
   at most gamma(n) sum_p (|Re a_p| |x_p| + |Im a_p| |y_p|) with (x_p, y_p) the stored factor.  The vector of the two
   component sums of path p is at most sqrt(2) |a_p| |stored factor| long (Cauchy-Schwarz with 2 |cos sin| <= 1), so the
   output moves by at most sqrt(2) gamma(2 P + 2) sum_p |a_p| (1 + PHI_p u).
4. The anchor's own float64 evaluation: the same terms with 2^-53 for u; 2^-50 (|theta| + P) A covers it.

    B = sum_p |a_p| [ PHI_p u + sqrt(2) gamma(2 P + 2) (1 + PHI_p u) ] + 2^-50 (max_p |theta_p| + P) A        (unnormalised)

5. Normalisation.  The kernels store fl(h inv), inv = 1 / sqrtf(E / n), E the float32 sum of fl(fl(x^2) + fl(y^2)) over the
   n = rows F outputs of the link (rows = RA TA T).
   - The energy is that of the COMPUTED outputs: |rms(computed) - rms64| <= rms(computed - h64) <= rms(B) (triangle inequality
     in l2): relative rho_d = rms(B) / rms64.
   - Float32 summation of non-negative terms is off by at most gamma(depth) relatively, depth the longest chain of roundings
     a term passes.  Three roundings form a term.  Per thread the terms are added serially: at most
     ceil(rows / G) ceil(F / 256) of them with G = max(1, 256 // F) in the two-pass kernel (the other kernels have at least as
     many row groups and at most 40 rows per thread).  Across threads: a tree over at most 512 slots (9 levels), or 6 wave
     shuffles and a serial sum over at most 8 waves (14).  depth = 3 + chain + 14 covers the worst order of the four kernels.
   - E / n: n < 2^24 is exact, the division 2.5 ulp (5 u); sqrtf 3 ulp (6 u); 1 / c 2.5 ulp (5 u) - the OpenCL full-profile
     figures again.  rho_f = (gamma(depth) + 5 u) / 2 / (1 - gamma(depth) - 5 u) + 11 u.
   - inv = (1 / rms64)(1 + e), |e| <= rho = r / (1 - r), r = rho_d + rho_f; the last product one rounding:
     rho' = rho + u + rho u.

    B_n = B / rms64 (1 + rho') + |h64_n| rho'                                                              (normalised)

   A link whose taps are all zero: every product is an exact zero, E = 0, inv = 0: the output is exactly 0 and B_n = 0.
"""
import numpy as np

U = 2.0 ** -24
C_SC = 4.0            # ulp of sin and cos: OpenCL full profile (no ROCm accuracy table on the build machine)


def _gamma(n):
    return n * U / (1 - n * U)


def _shapes(freqs, a, tau):
    freqs, a, tau = np.asarray(freqs), np.asarray(a), np.asarray(tau)
    b, rx, ra, tx, ta, p, t = a.shape
    assert tau.shape == (b, rx, tx, p) and freqs.ndim == 1
    return freqs.astype(np.float64), a.astype(np.complex128), tau.astype(np.float64)


def _link_rms(h):
    """h [b, rx, ra, tx, ta, t, f] -> root mean square per (b, rx, tx), broadcastable to h"""
    return np.sqrt(np.mean(np.abs(h) ** 2, axis=(2, 4, 5, 6), keepdims=True))


def anchor(freqs, a, tau, normalize):
    """complex128 [b, rx, ra, tx, ta, t, f] from the inputs as given (float32 values taken exactly)"""
    fr, a, tau = _shapes(freqs, a, tau)
    theta = -2.0 * np.pi * tau[..., None] * fr                                   # [b, rx, tx, p, f]
    e = np.exp(1j * theta)
    h = np.einsum("brxyzpt,brypf->brxyztf", a, e)
    if normalize:
        c = _link_rms(h)
        h = np.where(c > 0, h / np.where(c > 0, c, 1.0), 0.0)
    return h


def bound(freqs, a, tau, normalize, theta_scale=1.0):
    """float64 [b, rx, ra, tx, ta, t, f]: how far a single-precision kernel may be from ``anchor`` in modulus (module
    docstring).  ``theta_scale = 0`` leaves the argument term out (a test shows that the term is needed)."""
    fr, a, tau = _shapes(freqs, a, tau)
    b, rx, ra, tx, ta, p, t = a.shape
    f = fr.size
    theta = np.abs(2.0 * np.pi * tau[..., None] * fr) * theta_scale              # [b, rx, tx, p, f]
    phi_u = (2.5 * theta + 2.0 * C_SC) * U
    w = phi_u + np.sqrt(2.0) * _gamma(2 * p + 2) * (1.0 + phi_u)
    absa = np.abs(a)
    bu = np.einsum("brxyzpt,brypf->brxyztf", absa, w)
    big_a = np.sum(absa, axis=5)[..., None]                                      # [b, rx, ra, tx, ta, t, 1]
    th_max = np.max(theta, axis=3)[:, :, None, :, None, None, :]                 # [b, rx, 1, tx, 1, 1, f]
    bu = bu + 2.0 ** -50 * (th_max + p) * big_a
    if not normalize:
        return bu
    h = anchor(freqs, a, tau, False)
    c = _link_rms(h)
    live = c > 0
    cs = np.where(live, c, 1.0)
    rows = ra * ta * t
    g = max(1, 256 // f)
    depth = 3 + (-(-rows // g)) * (-(-f // 256)) + 14
    gd = _gamma(depth) + 5 * U
    rho_f = gd / 2 / (1 - gd) + 11 * U
    r = _link_rms(bu) / cs + rho_f
    rho = r / (1 - r)
    rho = rho + U + rho * U
    return np.where(live, bu / cs * (1 + rho) + np.abs(h) / cs * rho, 0.0)


def ratio(h, freqs, a, tau, normalize):
    """max over the outputs of |h - anchor| / bound (0 / 0 counts as 0, x / 0 as inf): what the tests assert to be <= 1"""
    err = np.abs(np.asarray(h).astype(np.complex128) - anchor(freqs, a, tau, normalize))
    bd = bound(freqs, a, tau, normalize)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bd)
    return float(np.max(q))
