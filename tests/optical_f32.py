"""NumPy specification of the optical channels (csrc/optical.hip) in float32 and float64: the SSFM fibre and the EDFA.

Restates the reference's channel/optical/fiber.py:257-449 and edfa.py:107-170 in the operation order of the kernels:

* the parameters are float64 in either precision; what a kernel receives as a scalar or a table is formed in float64 and
  rounded ONCE to the working type R (float32 / float64);
* time domain, per sample (both polarisations together): f = pre * w[t]; q = q * f; power = sum_p (re^2 + im^2);
  rotation by power * kerr, kerr = -gamma dz (8/9 with Manakov); q += normal * sigma; q = q * post;
* frequency domain: q[k] *= tf[k], tf = exp(j c2[k] dz) exp(half_alpha dz) / n with c2[k] = -beta_2 / 2 (2 pi f_k)^2 and
  f_k in the reference's fft-shifted order (fiber.py:271); the inverse transform is unnormalised;
* fixed step count: half D, (n_ssfm - 1) x [window, N, noise, D], N, noise, half D (fiber.py:425-447); linear operators
  that meet with nothing between them (no nonlinearity and no noise) are applied as one;
* adaptive: per step max |q|^2 over the tensor, dz = min(phase_inc / gamma / max, remaining) in R, then window, D, N,
  noise (fiber.py:335-350); the dispersion phase c2[k] dz, its sine and its cosine are float64, rounded once to R;
* noise: element i of the flattened tensor takes half i & 1 of Philox block i / 2 of the stream (seed, call + step),
  Box-Muller on the stream's 24-bit uniforms (oracle/utils.py), evaluated in R; sigma^2 = p_n_ase dz / length / 2.

``fault`` seeds a deliberate mistake (tests/test_optical_host.py shows that each lands outside the bar)."""
import numpy as np

from oracle.utils import philox_block

H = 6.62607015e-34


def _types(precision):
    return (np.float32, np.complex64) if precision in ("single", "float32", np.float32) else (np.float64, np.complex128)


def time_frequency_vector(n, sample_duration, precision="double"):
    """channel/utils.py:66-120"""
    R, _ = _types(precision)
    k = np.arange(-(n // 2), (n + 1) // 2, dtype=np.int32).astype(R)
    df = R(R(1.0 / sample_duration) / R(n))
    return (k * R(sample_duration)).astype(R), (k * df).astype(R)


def hamming(h, precision="double"):
    """the 2 h taper values, tf.signal.hamming_window(2 h) (periodic): 0.54 - 0.46 cos(2 pi k / (2 h)), float64 rounded once"""
    R, _ = _types(precision)
    k = np.arange(2 * h, dtype=np.float64)
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * k / max(2 * h, 1))).astype(R)


def window(n, h, precision="double", fault=None):
    """fiber.py:391-407: the taper in the first and last h samples, 1 elsewhere"""
    R, _ = _types(precision)
    w = np.ones(n, R)
    t = hamming(h, precision)
    if fault == "taper_in_middle" and h > 0:                   # the 2 h taper values laid over the centre of the signal
        w[n // 2 - h:n // 2 + h] = t
        return w
    if h > 0:
        w[:h], w[n - h:] = t[:h], t[h:]
    return w


def bin_frequency(n, sample_duration):
    """frequency of transform bin k as the reference orders it: np.fft.fftshift of the ascending vector (fiber.py:271)"""
    k = np.arange(n)
    j = (k - n // 2) % n
    return (j - n // 2).astype(np.float64) * (1.0 / sample_duration / n)


def unit_normals(seed, call, total, precision):
    """complex unit normal (variance 1 per real dimension) of every flat element index"""
    R, Cc = _types(precision)
    nb = (total + 1) // 2
    w0, w1, w2, w3 = philox_block(seed, call, nb)
    u = lambda w: (w >> np.uint32(8)).astype(R) * R(2.0 ** -24) + R(2.0 ** -25)
    ua = np.stack([u(w0), u(w2)], axis=1).reshape(-1)[:total]
    ub = np.stack([u(w1), u(w3)], axis=1).reshape(-1)[:total]
    r = np.sqrt(R(-2.0) * np.log(ua))
    t = R(6.283185307179586) * ub
    return (r * np.cos(t)).astype(R), (r * np.sin(t)).astype(R)


def p_n_ase_ssfm(alpha, f_c, length, n_sp, sample_duration, t_norm, with_manakov):
    """fiber.py:236-244"""
    p = H * f_c * alpha * length * n_sp / sample_duration / t_norm
    return p / 2.0 if with_manakov else p


def _time(q, P, w, pre, post, kerr, sigma, nonlin, noise, seed, call, R, manakov_factor_missing=False):
    """q [rows, P, n] complex -> the fused time-domain pass"""
    Cc = q.dtype
    re, im = q.real.astype(R), q.imag.astype(R)
    f = R(pre) * w if w is not None else np.full(q.shape[-1], R(pre), R)
    re, im = re * f, im * f
    if nonlin:
        power = np.zeros(re[:, 0].shape, R)
        for p in range(P):
            power = power + (re[:, p] * re[:, p] + im[:, p] * im[:, p])
        phi = (power * R(kerr))[:, None, :]
        cs, sn = np.cos(phi).astype(R), np.sin(phi).astype(R)
        re, im = re * cs - im * sn, re * sn + im * cs
    if noise:
        nr, ni = unit_normals(seed, call, q.size, R)
        re = re + nr.reshape(q.shape) * R(sigma)
        im = im + ni.reshape(q.shape) * R(sigma)
    out = np.empty(q.shape, Cc)
    out.real, out.imag = re * R(post), im * R(post)
    return out


def _cmul(q, tf):
    re = q.real * tf.real - q.imag * tf.imag
    im = q.real * tf.imag + q.imag * tf.real
    out = np.empty(q.shape, q.dtype)
    out.real, out.imag = re, im
    return out


def ssfm(x, alpha=0.046, beta_2=-21.67, f_c=193.55e12, gamma=1.27, half_window_length=0, length=80, n_ssfm=1, n_sp=1.0,
         sample_duration=1.0, t_norm=1e-12, with_amplification=False, with_attenuation=True, with_dispersion=True,
         with_manakov=False, with_nonlinearity=True, phase_inc=1e-4, precision="double", seed=0, call=0, fault=None):
    """-> (y of the shape of x, number of steps = number of stream calls consumed)"""
    R, Cc = _types(precision)
    x = np.asarray(x).astype(Cc)
    n = x.shape[-1]
    P = 2 if with_manakov else 1
    if x.size == 0:
        return x.copy(), 0
    q = x.reshape(-1, P, n).copy()
    h = int(half_window_length)
    adaptive = n_ssfm == "adaptive"
    p_n = p_n_ase_ssfm(alpha, f_c, length, n_sp, sample_duration, t_norm, with_manakov)
    noise = bool(with_amplification) and p_n > 0.0
    half_alpha = ((1.0 if with_amplification else 0.0) - (1.0 if with_attenuation else 0.0)) * alpha / 2.0
    kerr_unit = -gamma * ((8.0 / 9.0) if (with_manakov and fault != "no_8_9") else 1.0)
    sigma_unit = np.sqrt(p_n / length / 2.0) if noise else 0.0
    w = window(n, h, R, fault) if h > 0 else None
    omega = 2.0 * np.pi * bin_frequency(n, sample_duration)
    c2 = -beta_2 / 2.0 * omega * omega                         # left to right, as the kernel's host table
    inv_n = 1.0 if fault == "no_1_n" else 1.0 / n

    def transfer(dz):
        sc = np.exp(half_alpha * dz) if fault == "no_1_n" else np.exp(half_alpha * dz) / n
        return ((np.cos(c2 * dz) * sc) + 1j * (np.sin(c2 * dz) * sc)).astype(Cc)

    def linear(q, tf):
        return np.fft.ifft(_cmul(np.fft.fft(q, axis=-1).astype(Cc), tf), axis=-1, norm="forward").astype(Cc)

    if not adaptive:
        dz = length / n_ssfm
        last_empty = not with_nonlinearity and not noise
        identity_time = last_empty and (h == 0 or n_ssfm == 1)
        kerr, sigma = kerr_unit * dz, sigma_unit * np.sqrt(dz)
        windowed = n_ssfm - 1
        if with_dispersion:
            if identity_time:
                return linear(q, transfer(length)).reshape(x.shape), n_ssfm
            tf_full, tf_half, tf_join = transfer(dz), transfer(dz / 2.0), transfer(1.5 * dz)
            q = linear(q, tf_half)
            for s in range(windowed):
                q = _time(q, P, w, 1.0, 1.0, kerr, sigma, with_nonlinearity, noise, seed, call + s, R)
                q = linear(q, tf_join if (last_empty and s == windowed - 1) else tf_full)
            if not last_empty:
                q = _time(q, P, None, 1.0, 1.0, kerr, sigma, with_nonlinearity, noise, seed, call + windowed, R)
                q = linear(q, tf_half)
            return q.reshape(x.shape), n_ssfm
        if identity_time:
            return _time(q, P, None, np.exp(half_alpha * length), 1.0, 0.0, 0.0, False, False, seed, call, R).reshape(x.shape), n_ssfm
        a_half, a_full, a_join = np.exp(half_alpha * dz / 2.0), np.exp(half_alpha * dz), np.exp(half_alpha * 1.5 * dz)
        for s in range(n_ssfm):
            last = s == windowed
            if last and last_empty:
                break
            post = a_half if last else (a_join if (last_empty and s == windowed - 1) else a_full)
            q = _time(q, P, None if last else w, a_half if s == 0 else 1.0, post, kerr, sigma, with_nonlinearity, noise, seed,
                      call + s, R)
        return q.reshape(x.shape), n_ssfm

    remaining, steps = R(length), 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while remaining >= R(1e-3):
            maxp = np.max(q.real.astype(R) * q.real.astype(R) + q.imag.astype(R) * q.imag.astype(R))
            want = R(phase_inc) / R(gamma) / R(maxp)
            dz = want if want < remaining else remaining
            remaining = R(remaining - dz)
            scale = R(np.exp(half_alpha * float(dz)))

            def lin(q):
                if not with_dispersion:
                    return _time(q, P, None, scale, 1.0, 0.0, 0.0, False, False, seed, call, R)
                ph = c2 * float(dz)
                f = R(scale) * R(inv_n)
                Q = np.fft.fft(q, axis=-1).astype(Cc)
                cs, sn = np.cos(ph).astype(R), np.sin(ph).astype(R)
                out = np.empty(Q.shape, Cc)
                out.real = (Q.real * cs - Q.imag * sn) * f
                out.imag = (Q.real * sn + Q.imag * cs) * f
                return np.fft.ifft(out, axis=-1, norm="forward").astype(Cc)

            def nl(q):
                return _time(q, P, None, 1.0, 1.0, R(kerr_unit) * dz, R(sigma_unit) * np.sqrt(dz), with_nonlinearity, noise, seed,
                             call + steps, R)

            if w is not None:
                q = _time(q, P, w, 1.0, 1.0, 0.0, 0.0, False, False, seed, call, R)
            q = lin(nl(q)) if fault == "adaptive_order" else nl(lin(q))      # the fault: N before D, the fixed scheme's order
            steps += 1
    return q.reshape(x.shape), steps


def edfa_parameters(g=4.0, f=7.0, f_c=193.55e12, dt=1e-12, with_dual_polarization=False, precision="double"):
    """edfa.py:117-143 -> (sqrt(g), sigma per real dimension, p_n_ase); the parameters are float64 in either precision, the
    two scalars the kernel receives are rounded once to R"""
    R, _ = _types(precision)
    g, f, f_c, dt = float(g), float(f), float(f_c), float(dt)
    n_sp = 0.0 if g == 1.0 else f / 2.0 * g / (g - 1.0)
    p = 2.0 * (n_sp * (g - 1.0) * H * f_c) / dt
    if with_dual_polarization:
        p = p / 2.0
    return float(R(np.sqrt(g))), float(R(np.sqrt(p / 2.0))), p


def edfa(x, g=4.0, f=7.0, f_c=193.55e12, dt=1e-12, with_dual_polarization=False, precision="double", seed=0, call=0):
    R, Cc = _types(precision)
    x = np.asarray(x).astype(Cc)
    sqrt_g, sigma, _ = edfa_parameters(g, f, f_c, dt, with_dual_polarization, precision)
    re, im = x.real.astype(R) * R(sqrt_g), x.imag.astype(R) * R(sqrt_g)
    if sigma != 0.0 and x.size:
        nr, ni = unit_normals(seed, call, x.size, R)
        re = re + nr.reshape(x.shape) * R(sigma)
        im = im + ni.reshape(x.shape) * R(sigma)
    out = np.empty(x.shape, Cc)
    out.real, out.imag = re, im
    return out
