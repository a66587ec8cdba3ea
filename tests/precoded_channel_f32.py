"""Specification of the precoded channels and of the post-equalisation SINR (TEST INFRASTRUCTURE): NumPy restatements of
``RZFPrecodedChannel`` / ``CBFPrecodedChannel`` / ``EyePrecodedChannel`` (reference ofdm/precoding.py:179-566) and of
``LMMSEPostEqualizationSINR`` (ofdm/equalization.py:464-839) in float32 AND float64 with a DEFINED order of operations -
the one of ``samd_precoded_channel_*`` (csrc/precoding.hip) and ``samd_lmmse_post_eq_sinr_*`` (csrc/post_eq_sinr.hip),
which follow it bit for bit (tests/test_gpu_precoded_channel.py):

* every sum runs in ascending index order, starting from zero; |z|^2 is re*re + im*im;
* G is the precoding matrix of ``tests/precoding_f32.py`` (``_core``: RZF with alpha, CBF) computed from ``h_hat``, or the
  identity; column k is multiplied by s_k = sqrt(tx_power[b, tx, k, t, f]) as (s_k re, s_k im);
* h_eff[b, r, a, tx, k, t, fe] = sum_m h[b, r, a, tx, m, t, f] G_mk from the TRUE h, at the effective subcarriers only;
* SINR, per receiver and resource element: V_ij = sum_u Hu_iu conj(Hu_ju) (j <= i) over the undesired columns (zero
  without interference whitening), then V_ii.re += no_i; V = L L^H (``oracle.mimo_f32.cholesky``);
  Li_ic = ((i == c) - sum_{c <= q < i} L_iq Li_qc) * (1 / L_ii); Hw_is = sum_{q <= i} Li_iq Hd_qs;
  A_ab = (a == b) + sum_i conj(Hw_ia) Hw_ib (b <= a); A = C C^H; F = C^-H C^-1 Hw^H by forward and then backward
  substitution, each row multiplied by the reciprocal of C_ii; signal_s = |sum_a F_sa Hw_as|^2;
  total_s = sum_c |sum_a F_sa w_ac|^2 over the desired and then the undesired columns, the latter whitened (w = Li hu)
  whether or not they entered V; interference = max(total - signal, 0); noise_s = sum_a |F_sa|^2;
  sinr = signal / (interference + noise), 0 where the denominator is 0.

The float64 form is the same program with every float32 replaced by float64 (``precision``): the helpers of
``oracle/mimo_f32.py`` and ``tests/precoding_f32.py`` take their real type from the module constant ``F``, which
``precision`` sets for the duration of a call.

How far the reference itself is from its own double-precision result on the cases of
tests/golden/precoded_channel_ref_golden.npz (tools/gen_precoded_channel_ref_golden.py prints this table; e32 = largest
relative deviation of its single-precision result from its double-precision one, per family), and the bars that
tests/test_precoded_channel_host.py and tests/test_gpu_precoded_channel.py hold this specification and the kernels to:

    bar32 = 4 e32 + 2^-23 (the factor 4 allows an equally valid summation order), bar64 = bar32 2^-29 (the same
    algorithm on the same data: the error scales with the unit roundoff, 2^-53 / 2^-24)
"""
import contextlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import oracle.mimo_f32 as _m32  # noqa: E402
import precoding_f32 as _p32  # noqa: E402
from oracle.mimo_f32 import C, cholesky  # noqa: E402

# measured by tools/gen_precoded_channel_ref_golden.py (its printed table), per family
E32 = {"rzf": 2.047e-06, "cbf": 1.819e-07, "eye": 7.045e-08, "sinr_whitened": 2.703e-05, "sinr_unwhitened": 2.703e-05}


def bar32(family):
    return 4 * E32[family] + 2.0 ** -23


def bar64(family):
    return bar32(family) * 2.0 ** -29


def rel_dev(a, b):
    """largest deviation of a from b relative to the largest magnitude of b"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return 0.0 if b.size == 0 else float(np.abs(a - b).max() / max(np.abs(b).max(), np.finfo(np.float64).tiny))


@contextlib.contextmanager
def precision(dtype):
    """the real type of ``oracle.mimo_f32`` / ``precoding_f32`` for the duration of the block"""
    old = _m32.F, _p32.F
    _m32.F = _p32.F = np.dtype(dtype).type
    try:
        yield np.dtype(dtype).type
    finally:
        _m32.F, _p32.F = old


def _c(v):
    v = np.asarray(v)
    return C(np.real(v), np.imag(v))


def _pack(z, R):
    cd = np.complex64 if R is np.float32 else np.complex128
    out = np.empty(z.re.shape, cd)
    out.real, out.imag = z.re, z.im
    return out


def _expand(v, shape, R):
    """``[..first n dims]`` -> full shape (expand_to_rank(..., axis=-1) then broadcast)"""
    v = np.asarray(v, R)
    return np.broadcast_to(v.reshape(v.shape + (1,) * (len(shape) - v.ndim)), shape)


def precoded_channel(h, tx_power, precoding_ind, effective_subcarrier_ind, mode, h_hat=None, alpha=0., dtype=np.float32):
    """h, h_hat [B, rx, rxa, tx, M, T, F], tx_power [B, tx, K, T, F] or its first n dims, alpha [B, tx, T, F] or its first
    n dims, mode "rzf" | "cbf" | "eye" -> h_eff [B, rx, rxa, tx, K, T, Fe] (complex64, or complex128 for float64)."""
    with np.errstate(all="ignore"), precision(dtype) as R:
        cd = np.complex64 if R is np.float32 else np.complex128
        sc = np.asarray(effective_subcarrier_ind)
        h = np.asarray(h).astype(cd)[..., sc]                        # a resource element is computed on its own: only the
        B, rx, rxa, ntx, M, T, Fe = h.shape                          # effective subcarriers are evaluated
        n = B * ntx * T * Fe
        if mode == "eye":
            K = M
            one, zero = np.ones(n, R), np.zeros(n, R)
            gt = [[C(one if k == m else zero, zero) for m in range(M)] for k in range(K)]
        else:
            hh = h if h_hat is None else np.asarray(h_hat).astype(cd)[..., sc]
            pind = np.asarray(precoding_ind).reshape(ntx, -1)
            K = pind.shape[1] * rxa
            hd = np.stack([np.stack([hh[:, pind[t, k // rxa], k % rxa, t] for k in range(K)], 1) for t in range(ntx)], 1)
            hd = np.transpose(hd, [0, 1, 4, 5, 2, 3])                # [B, tx, T, Fe, K, M]
            a = np.asarray(alpha, R)
            a = _expand(a[..., sc] if a.ndim == 4 else a, (B, ntx, T, Fe), R)
            gt = _p32._core(hd.reshape(-1, K, M), np.ascontiguousarray(a).reshape(-1), mode)
        p = np.asarray(tx_power, R)
        p = _expand(p[..., sc] if p.ndim == 5 else p, (B, ntx, K, T, Fe), R)
        heff = np.zeros((B, rx, rxa, ntx, K, T, Fe), cd)
        for k in range(K):
            s = np.sqrt(np.ascontiguousarray(p[:, :, k]).reshape(-1))                # [n] over (b, tx, t, fe)
            v = C(np.zeros((B, rx, rxa, ntx, T, Fe), R), np.zeros((B, rx, rxa, ntx, T, Fe), R))
            for m in range(M):
                g = C((gt[k][m].re * s).reshape(B, 1, 1, ntx, T, Fe), (gt[k][m].im * s).reshape(B, 1, 1, ntx, T, Fe))
                v = v + _c(h[:, :, :, :, m]) * g
            heff[:, :, :, :, k] = _pack(v, R)
        return heff


def lmmse_post_eq_sinr(h_eff, no, detection_desired_ind, detection_undesired_ind, interference_whitening=True,
                       dtype=np.float32):
    """h_eff [B, rx, rxa, tx, K, T, Fe] (the estimate when there is one), no [B, rx, rxa, T, Fe] or its first n dims, the
    flat stream indices of StreamManagement -> sinr [B, T, Fe, rx, S] (float32 or float64)."""
    with np.errstate(all="ignore"), precision(dtype) as R:
        cd = np.complex64 if R is np.float32 else np.complex128
        h_eff = np.asarray(h_eff).astype(cd)
        B, RX, RA, ntx, K, T, Fe = h_eff.shape
        no = _expand(no, (B, RX, RA, T, Fe), R)
        des = np.asarray(detection_desired_ind).reshape(RX, -1)
        und = np.asarray(detection_undesired_ind).reshape(RX, -1) if np.size(detection_undesired_ind) else np.zeros((RX, 0), int)
        S, U = des.shape[1], und.shape[1]
        cols = np.transpose(h_eff, [1, 3, 4, 2, 0, 5, 6]).reshape(RX * ntx * K, RA, B * T * Fe)   # [q][a] -> items
        n = B * T * Fe
        zero = lambda: C(np.zeros(n, R), np.zeros(n, R))  # noqa: E731
        abs2 = lambda z: z.re * z.re + z.im * z.im  # noqa: E731
        out = np.zeros((B, T, Fe, RX, S), R)
        for r in range(RX):
            Hd = [[_c(cols[des[r, s], a]) for s in range(S)] for a in range(RA)]
            Hu = [[_c(cols[und[r, u], a]) for a in range(RA)] for u in range(U)]
            V = [[zero() for _ in range(RA)] for _ in range(RA)]
            if interference_whitening:
                for u in range(U):
                    for i in range(RA):
                        for j in range(i + 1):
                            V[i][j] = V[i][j] + Hu[u][i].mulc(Hu[u][j])
            for i in range(RA):
                V[i][i] = C(V[i][i].re + np.ascontiguousarray(no[:, r, i]).reshape(-1), V[i][i].im)
            cholesky(V, RA)
            Li = [[None] * RA for _ in range(RA)]
            for c in range(RA):
                for i in range(c, RA):
                    v = C(np.full(n, 1 if i == c else 0, R), np.zeros(n, R))
                    for q in range(c, i):
                        v = v - V[i][q] * Li[q][c]
                    Li[i][c] = v.scale(R(1) / V[i][i].re)

            def whiten(col):
                w = [None] * RA
                for i in range(RA - 1, -1, -1):
                    v = zero()
                    for q in range(i + 1):
                        v = v + Li[i][q] * col[q]
                    w[i] = v
                return w

            for s in range(S):
                w = whiten([Hd[a][s] for a in range(RA)])
                for a in range(RA):
                    Hd[a][s] = w[a]
            A = [[None] * S for _ in range(S)]
            for a in range(S):
                for c in range(a + 1):
                    v = C(np.full(n, 1 if a == c else 0, R), np.zeros(n, R))
                    for i in range(RA):
                        v = v + Hd[i][c].mulc(Hd[i][a])                          # conj(Hw_ia) Hw_ic
                    A[a][c] = v
            cholesky(A, S)
            G = [[None] * RA for _ in range(S)]
            for i in range(RA):
                for a in range(S):
                    v = Hd[i][a].conj()
                    for q in range(a):
                        v = v - A[a][q] * G[q][i]
                    G[a][i] = v.scale(R(1) / A[a][a].re)
                for a in range(S - 1, -1, -1):
                    v = G[a][i]
                    for q in range(a + 1, S):
                        v = v - G[q][i].mulc(A[q][a])                            # conj(C_qa) G_qi
                    G[a][i] = v.scale(R(1) / A[a][a].re)

            def combine(s, col):
                v = zero()
                for a in range(RA):
                    v = v + G[s][a] * col[a]
                return abs2(v)

            signal = [combine(s, [Hd[a][s] for a in range(RA)]) for s in range(S)]
            total = [np.zeros(n, R) for _ in range(S)]
            for c in range(S):
                for s in range(S):
                    total[s] = total[s] + combine(s, [Hd[a][c] for a in range(RA)])
            for u in range(U):
                w = whiten(Hu[u])
                for s in range(S):
                    total[s] = total[s] + combine(s, w)
            for s in range(S):
                interference = np.maximum(total[s] - signal[s], R(0))
                noise = np.zeros(n, R)
                for a in range(RA):
                    noise = noise + abs2(G[s][a])
                den = interference + noise
                sinr = np.where(den == 0, R(0), signal[s] / np.where(den == 0, R(1), den))
                out[:, :, :, r, s] = sinr.reshape(B, T, Fe)
        return out
