"""Specification of the PUSCH DMRS least-squares kernel (csrc/pusch_rx.hip) in NumPy, float32 and float64, and of the error
variance of ``PUSCHLSChannelEstimator``.

    ls(p)  = y[r, src[s, p]] * coef[s, p]                 coef = 1 / pilot rounded to ``dtype``, 0 for a zero pilot: ls = +0
    t(p)   = (ls(p) + ls(p')) / 2   (dmrs_length 2)       p' the same position of the adjacent DMRS symbol; else t = ls
    h(p)   = (t(g) + ... + t(g + n - 1)) / 2              g the first pilot of p's run of n = 2 * num_cdm_groups_without_data
           = 0 where t(p) = 0 (real and imaginary part)
    out[r, s, j] = h(j), or h(gather[s, j]) with a nearest-neighbour table

Pilots of a stream are numbered row-major, ``pilots_per_symbol`` per DMRS symbol.  Order of operations, each rounded once to
``dtype``: ls re = yr * cr - yi * ci, im = yr * ci + yi * cr (two products, one difference or sum); the pair sum and its
halving; the run's sum starts at +0 and adds t in ascending p; the halving.  Halvings are exact."""
import numpy as np


def _cdtype(dtype):
    return np.complex64 if dtype == np.float32 else np.complex128


def reciprocal_table(pilots, dtype=np.float32):
    """pilots [S, num_pilots] (any complex type) -> 1 / pilot in ``dtype``, 0 where the pilot is 0; the reciprocal is formed
    in complex128 from the pilot as the block stores it and rounded once"""
    pil = np.asarray(pilots).astype(_cdtype(dtype)).astype(np.complex128)
    live = pil != 0
    return np.where(live, 1 / np.where(live, pil, 1), 0).astype(_cdtype(dtype))


def pusch_ls(y, src, coef, pilots_per_symbol, run, dmrs_length, gather=None, dtype=np.float32):
    """y [rows, n_in] complex, src int [S, num_pilots], coef [S, num_pilots] -> [rows, S, num_pilots], or [rows, S, n_out]
    with gather int [S, n_out]"""
    y, coef = np.asarray(y).astype(_cdtype(dtype)), np.asarray(coef).astype(_cdtype(dtype))
    rows, (s_, num_pilots) = y.shape[0], src.shape
    assert num_pilots % pilots_per_symbol == 0 and pilots_per_symbol % run == 0 and dmrs_length in (1, 2)
    num_syms = num_pilots // pilots_per_symbol
    live = (coef != 0) & (src >= 0) & (src < y.shape[1])
    v = y[:, np.where(live, src, 0)]                                       # [rows, S, num_pilots]
    yr, yi, cr, ci = v.real, v.imag, coef.real[None], coef.imag[None]
    zero = np.zeros((), dtype)
    lr = np.where(live[None], yr * cr - yi * ci, zero)
    li = np.where(live[None], yr * ci + yi * cr, zero)
    assert lr.dtype == dtype
    if dmrs_length == 2:
        assert num_syms % 2 == 0
        def pair_mean(a):
            a = a.reshape(rows, s_, num_syms // 2, 2, pilots_per_symbol)
            m = (a[:, :, :, 0] + a[:, :, :, 1]) / dtype(2)
            return np.repeat(m[:, :, :, None], 2, axis=3).reshape(rows, s_, num_pilots)
        lr, li = pair_mean(lr), pair_mean(li)
    def run_sum(a):
        a = a.reshape(rows, s_, num_pilots // run, run)
        acc = np.zeros(a.shape[:-1], dtype)
        for k in range(run):
            acc = acc + a[..., k]
        return np.repeat((acc / dtype(2))[..., None], run, axis=-1).reshape(rows, s_, num_pilots)
    alive = (lr != 0) | (li != 0)
    hr, hi = np.where(alive, run_sum(lr), zero), np.where(alive, run_sum(li), zero)
    assert hr.dtype == dtype
    out = np.empty(hr.shape, _cdtype(dtype))
    out.real, out.imag = hr, hi
    if gather is not None:
        known = (gather >= 0) & (gather < num_pilots)
        out = np.where(known[None], np.take_along_axis(out, np.where(known, gather, 0)[None].repeat(rows, 0), axis=2), 0).astype(out.dtype)
    return out


def error_bound(y, src, pilots, pilots_per_symbol, run, dmrs_length, gather=None, unit=2.0 ** -24):
    """Per output and real component (float64 [rows, S, num_pilots] or [rows, S, n_out]): what ``pusch_ls`` in the precision of
    ``unit`` and the reference's evaluation in the same precision may differ by,
        (2 n + 11) * unit * W,      W = sum over the sources of an output of weight * |y| / |pilot|
    with n = ``run`` and weight = 1/2 (dmrs_length 1) or 1/4 (dmrs_length 2): W bounds every partial sum of the output.
    Both work on the same stored y and pilots and differ from the exact value e = sum weight * y / pilot as follows.
    Specification: the reciprocal rounded once (1 unit of |y| / |pilot|), a real component of y * coef is two products and one
    sum, together at most 2 units of |y| |coef|: 3 units per source; the pair sum one rounding; the run's sum n - 1 roundings
    (the first addition, to +0, is exact), each at most one unit of a partial sum; halvings are exact: (n + 3) units of W.
    Reference: y / pilot is NumPy's complex division (Smith's method): seven roundings d/c, d * (d/c), c + ., 1 / ., b * (d/c),
    a + ., . * scale, each moving a component by at most one unit of |y| / |pilot| to first order, and one unit kept for the
    second-order terms: 8 units per source; the pair sum one rounding; the sum over n terms n - 1 roundings in any order:
    (n + 8) units of W.  A masked output is zero on both sides whenever t(p) is: the mask is compared exactly."""
    y = np.asarray(y).astype(np.complex128)
    pil = np.asarray(pilots).astype(np.complex128)
    live = (pil != 0) & (src >= 0) & (src < y.shape[1])
    a = np.where(live[None], np.abs(y[:, np.where(live, src, 0)]) / np.where(live, np.abs(pil), 1)[None], 0.)
    rows, (s_, num_pilots) = y.shape[0], src.shape
    weight = 0.5
    if dmrs_length == 2:
        a = a.reshape(rows, s_, -1, 2, pilots_per_symbol)
        a = np.repeat((a[:, :, :, :1] + a[:, :, :, 1:]), 2, axis=3).reshape(rows, s_, num_pilots)
        weight = 0.25
    w = a.reshape(rows, s_, -1, run).sum(-1, keepdims=True).repeat(run, -1).reshape(rows, s_, num_pilots) * weight
    bound = (2 * run + 11) * unit * w
    if gather is not None:
        bound = np.take_along_axis(bound, gather[None].repeat(rows, 0), axis=2)
    return bound


def error_variance(no, pilots, dmrs_length, dtype=np.float32):
    """no broadcastable to [..., S, num_pilots] -> no / |pilot|^2 with divide_no_nan, halved for the frequency averaging and
    once more with dmrs_length 2 (nr/pusch_channel_estimation.py:129, 148, 167), in ``dtype``: |pilot| is the modulus of the
    stored pilot in ``dtype``, squared; one division; exact halvings"""
    pil = np.asarray(pilots).astype(_cdtype(dtype))
    den = (np.abs(pil) ** 2).astype(dtype)
    no = np.asarray(no, dtype)
    live = den != 0
    ev = np.where(live, no / np.where(live, den, dtype(1)), dtype(0)).astype(dtype)
    if dmrs_length == 2:
        ev = ev / dtype(2)
    return ev / dtype(2)
