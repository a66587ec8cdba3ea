"""Float64 anchor and derived per-output error bound of the CDL tap generator ``cdl_cir_kernel`` (csrc/cdl.hip; float32 and float64
instantiations) behind the host tables of sionna_amd/phy/channel/tr38901/cdl.py.

    a[b, u, s, n, t] = sum_r c_r exp(j w_r t / fs)   [+ the LoS term at output position 0],
    c_r = amp_n (F_rx^T PM F_tx)_r a_rx,r a_tx,r,        w_r = (2 pi / lambda) r_rx,r . v_b

The anchor evaluates oracle/cdl.py (``field_gcs``, ``unit_vector``, ``rotation_matrix``; the sum of ``CDL._link``, with the ray axis
kept so that the per-ray magnitudes are at hand) in float64 on the STORED draws of the float32 stream (``CDL.draw(...,
precision="single")``: coupling permutations and phases; the three velocity uniforms as stored, the vector itself in float64), with
fs = float32(sampling_frequency); for u = 2^-53 on the float64 mapping of the same 24-bit uniforms and the doubles as given.  The
value is taken before any cast to complex64; ``oracle.cdl.CDL.__call__`` is unchanged.

Notation: u the unit roundoff, gamma(n) = n u / (1 - n u).  -ffp-contract=off: one rounding per operation.  Library constants as in
tests/time_channel_f32.py: sin / cos 4 ulp (a relative 2 C_SC u = 8 u), division 2.5 ulp (5 u).  A complex product of two values
adds 2 sqrt(2) u of its modulus.  Per ray r (cluster n = order[no]):

1. Host tables, rounded to the block's precision on the way to the device: each field entry, amp, xpr_scale and two_pi_over_lambda one u;
   an array response one u in modulus and phase; each component of r_rx one u.
2. Phase matrix: the four draws are the stored ones (the kernel's ``lo + (hi - lo) u01`` is the oracle's, operation for operation);
   each ``sincos`` 8 u.
3. Field chain ``frt * (c0 * ftt + k * c1 * ftp) + frp * (k * c2 * ftt + c3 * ftp)``: a co-polar term passes two table roundings, the
   sincos, two products and two sums: 14 u; a cross-polar term k and one product more: 16 u.  The four terms can cancel, so the error
   is relative to the sum of their moduli, F_abs = sum_ab |F_rx,a| |PM_ab| |F_tx,b| >= |F_rx^T PM F_tx|:  gamma(17) F_abs.
4. ``a_rx a_tx``: two table roundings and a complex product: 5 u.  Times the field (complex product) and amp (table, product): 5 u.
   With m_r = amp_n F_abs,r:   |c^_r - c_r| <= gamma(28) m_r.
5. Velocity: the three draws are the stored ones; four sin / cos (8 u each), two products per component: 18 u of v = |v_b|.
   ``r . v``: table, product, two sums per term: 22 u sum_i |r_i| |v_i| <= 22 u v (Cauchy-Schwarz, |r| = 1) - relative to v, not to
   r . v.  ``w = k0 (r . v)``: 2 u more.  |w^ - w| <= 24 u W,  W = (2 pi / lambda) v >= |w_r|.
6. ``w * ((float)t / fs)``: quotient 5 u, product u: the argument is off by at most 30 u W t / fs - the term that dominates at low
   sampling rates.  ``sincos``: 8 u.  Rotation of c_r (complex product): 2 sqrt(2) u.
7. Accumulation over the 20 rays (21 with the LoS term) per component: sqrt(2) gamma(21) sum_r m_r.
8. LoS (output position 0): ``frt ftt - frp ftp`` 4 u of |frt ftt| + |frp ftp|, the array product 5 u, two products with a table value
   3 u: gamma(12) m_los, m_los = sqrt(K / (K + 1)) (|frt ftt| + |frp ftp|); Doppler and accumulation as for a ray.
9. The anchor's own float64 evaluation and the float64 differences between the product's host tables and the oracle's (the same
   formulas in another order): 2^-44 sum m_r + 2^-48 W t / fs sum m_r.

    B = [gamma(28) + (8 + 2 sqrt 2) u + 30 u W t / fs + sqrt(2) gamma(21)] (1 + 64 u) M + item 9,     M = sum_r m_r [+ m_los]

``anchor_and_bound`` also returns M and M_w = sum_r m_r |w_r t / fs| per output.  tau is compared for equality.
"""
import numpy as np

from oracle import cdl as oc
from oracle import f64_ofdm as o64
from oracle import ofdm as o32

U32 = 2.0 ** -24
U64 = 2.0 ** -53
C_SC = 4.0
PI = np.pi
R = oc.NUM_RAYS


def _gamma(n, u):
    return n * u / (1 - n * u)


def _rays(ref, aoa, aod, zoa, zod, pm):
    """per-ray complex coefficient without amp, its F_abs and the arrival unit vector: angles [..., R], pm [..., R, 2, 2]
    -> c [..., R, U, S], f_abs [..., R, U, S], r_rx [..., R, 3]"""
    frx = oc.field_gcs(ref.rx_array, ref.rx_o, zoa, aoa)[..., ref.rx_array.pol, :]
    ftx = oc.field_gcs(ref.tx_array, ref.tx_o, zod, aod)[..., ref.tx_array.pol, :]
    field = np.einsum("...ua,...ab,...sb->...us", frx, pm, ftx)
    f_abs = np.einsum("...ua,...ab,...sb->...us", np.abs(frx), np.abs(pm), np.abs(ftx))
    r_rx, r_tx = oc.unit_vector(zoa, aoa), oc.unit_vector(zod, aod)
    d_rx = ref.rx_array.ant_pos @ oc.rotation_matrix(ref.rx_o).T
    d_tx = ref.tx_array.ant_pos @ oc.rotation_matrix(ref.tx_o).T
    a_rx = np.exp(2j * PI / ref.lambda_0 * (r_rx @ d_rx.T))
    a_tx = np.exp(2j * PI / ref.lambda_0 * (r_tx @ d_tx.T))
    return field * a_rx[..., :, None] * a_tx[..., None, :], f_abs, r_rx


def velocity(ref, seed, call, batch, u=U32):
    """-> v [B] (speed), vel [B, 3] in float64 from the stored uniforms"""
    _u = o32._u if u == U32 else o64._u
    v_r = np.asarray(_u(seed, call, batch, ref.min_speed, ref.max_speed), np.float64)
    v_phi = np.asarray(_u(seed, call + 1, batch, 0.0, 2 * PI), np.float64)
    v_th = np.asarray(_u(seed, call + 2, batch, 0.0, PI), np.float64)
    return v_r, np.stack([v_r * np.cos(v_phi) * np.sin(v_th), v_r * np.sin(v_phi) * np.sin(v_th), v_r * np.cos(v_th)], axis=-1)


def anchor_and_bound(ref, seed, call, batch, num_time_steps, sampling_frequency, u=U32):
    """ref: an ``oracle.cdl.CDL``.  -> anchor complex128, bound, M, M_w float64, each [B, 1, U, 1, S, N, T], and tau float64 [N]"""
    assert u in (U32, U64)
    n_, b_, t_ = ref.num_clusters, int(batch), int(num_time_steps)
    fs = float(np.float32(sampling_frequency)) if u == U32 else float(sampling_frequency)
    v, vel = velocity(ref, seed, call, b_, u)
    _, perm, phi = ref.draw(seed, call, b_, "single" if u == U32 else "double")
    ts = np.arange(t_, dtype=np.float64) / fs
    ang = {k: np.take_along_axis(np.broadcast_to(ref.rays[k], (b_, n_, R)), perm[k], axis=-1) for k in perm}
    kx = np.sqrt(1 / ref.xpr)
    e = np.exp(1j * phi)
    pm = np.stack([np.stack([e[..., 0], kx * e[..., 1]], -1), np.stack([kx * e[..., 2], e[..., 3]], -1)], -2)
    c, f_abs, r_rx = _rays(ref, ang["aoa"], ang["aod"], ang["zoa"], ang["zod"], pm)                  # [B, N, R, U, S]
    k0 = 2 * PI / ref.lambda_0
    w = k0 * np.sum(r_rx * vel[:, None, None, :], axis=-1)                                            # [B, N, R]
    amp = np.sqrt(ref.powers / R)
    if ref.los:
        amp = amp * np.sqrt(1 / (ref.k_factor + 1))
    dop = np.exp(1j * w[..., None] * ts)                                                              # [B, N, R, T]
    h = np.einsum("bnrus,bnrt->bnust", c, dop, optimize=True) * amp[None, :, None, None, None]
    m = np.sum(f_abs, axis=2) * amp[None, :, None, None]                                              # [B, N, U, S]
    m_w = np.einsum("bnrus,bnrt->bnust", f_abs, np.abs(w)[..., None] * ts, optimize=True) * amp[None, :, None, None, None]
    h, m, m_w = h[:, ref.order], m[:, ref.order], m_w[:, ref.order]
    if ref.los:
        la = {k2: np.full((b_, 1), val) for k2, val in ref.los_ang.items()}
        pm_los = np.broadcast_to(np.array([[1., 0.], [0., -1.]], complex), (b_, 1, 2, 2))
        cl, fl, rl = _rays(ref, la["aoa"], la["aod"], la["zoa"], la["zod"], pm_los)                  # [B, 1, U, S]
        kf = np.sqrt(ref.k_factor / (ref.k_factor + 1))
        wl = k0 * np.sum(rl[:, 0] * vel, axis=-1)                                                     # [B]
        h[:, 0] += kf * cl[:, 0, :, :, None] * np.exp(1j * wl[:, None] * ts)[:, None, None, :]
        m[:, 0] += kf * fl[:, 0]
        m_w[:, 0] += kf * fl[:, 0, :, :, None] * (np.abs(wl)[:, None] * ts)[:, None, None, :]
    wt = (k0 * v)[:, None] * ts                                                                       # [B, T]: W t / fs
    rel = (_gamma(28, u) + (2 * C_SC + 2 * np.sqrt(2.0)) * u + np.sqrt(2.0) * _gamma(21, u)
           + 30 * u * wt[:, None, None, None, :]) * (1 + 64 * u)
    mm = m[..., None]
    bound = rel * mm + 2.0 ** -44 * mm + 2.0 ** -48 * wt[:, None, None, None, :] * mm
    tr = lambda x: np.ascontiguousarray(np.transpose(np.broadcast_to(x, h.shape), [0, 2, 3, 1, 4])[:, None, :, None])
    tau = (ref.delays * ref.delay_spread)[ref.order]
    return tr(h), tr(bound), tr(mm), tr(m_w), tau


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
