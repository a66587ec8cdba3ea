"""Float32 specification of the precoders (TEST INFRASTRUCTURE): ``rzf_precoding_matrix`` / ``cbf_precoding_matrix`` /
``rzf_precoder`` (reference mimo/precoding.py:12-244) and ``RZFPrecoder`` with its effective channel
(ofdm/precoding.py:81-177) in SINGLE precision with a DEFINED order of operations, built on the complex helpers of
``oracle/mimo_f32.py`` (``C``, ``cholesky``):

* every sum runs in ascending index order, starting from zero;
* |z|^2 is re*re + im*im;
* A = H H^H is the Gram sum A_ij = sum_m H_im conj(H_jm) (j <= i); alpha is then added to the real part of the diagonal;
* A = L L^H is the Cholesky-Banachiewicz factor of ``oracle.mimo_f32.cholesky``; A X = H is solved by forward and then
  backward substitution, each row multiplied by the reciprocal of L_ii;
* G = X^H (RZF) or H^H (CBF); column k is divided by n_k = sqrt(sum_m |G_mk|^2) as two IEEE divisions (real and
  imaginary part), and is zero when n_k == 0 (``divide_no_nan``);
* x_precoded_m = sum_k G_mk x_k; h_eff[r, a, k] = sum_m H_r[a, m] G_mk.

The reference evaluates these formulas through TensorFlow's batched Cholesky solve in complex64, whose internal order is
not part of its contract; its results agree with this order within cond(A) 2^-24 (tests/test_precoding_host.py).  The HIP
kernel csrc/precoding.hip follows this order bit for bit (compiled with -ffp-contract=off; tests/test_gpu_precoding.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle.mimo_f32 import C, F, cholesky  # noqa: E402


def _c(v):
    v = np.asarray(v)
    return C(np.real(v).astype(F), np.imag(v).astype(F))


def _zero(n):
    return C(np.zeros(n, F), np.zeros(n, F))


def _forward(A, X, K, m):
    """column m of X [K][M] <- L^-1 X for the factor ``cholesky`` left in A"""
    for i in range(K):
        v = X[i][m]
        for q in range(i):
            v = v - A[i][q] * X[q][m]
        X[i][m] = v.scale(F(1) / A[i][i].re)


def _backward(A, X, K, m):
    """column m of X [K][M] <- L^-H X"""
    for i in range(K - 1, -1, -1):
        v = X[i][m]
        for q in range(i + 1, K):
            v = v - A[q][i].conj() * X[q][m]
        X[i][m] = v.scale(F(1) / A[i][i].re)


def _core(hf, al, mode):
    """hf [n, K, M] complex64, al [n] float32 -> Gt[k][m] = G_mk as lists of C over the n items."""
    n, K, M = hf.shape
    X = [[_c(hf[:, k, m]) for m in range(M)] for k in range(K)]
    if mode == "rzf":
        A = [[None] * K for _ in range(K)]
        for i in range(K):
            for j in range(i + 1):
                v = _zero(n)
                for m in range(M):
                    v = v + X[i][m].mulc(X[j][m])
                if i == j:
                    v = C(v.re + al, v.im)
                A[i][j] = v
        cholesky(A, K)
        for m in range(M):
            _forward(A, X, K, m)
            _backward(A, X, K, m)
    for k in range(K):
        n2 = np.zeros(n, F)
        for m in range(M):
            n2 = n2 + (X[k][m].re * X[k][m].re + X[k][m].im * X[k][m].im)
        nrm = np.sqrt(n2)
        zero = nrm == 0
        for m in range(M):
            g = X[k][m].conj()
            X[k][m] = C(np.where(zero, F(0), g.re / nrm), np.where(zero, F(0), g.im / nrm))
    return X


def _pack_g(gt, lead):
    K, M = len(gt), len(gt[0])
    g = np.stack([np.stack([gt[k][m].to_np() for k in range(K)], -1) for m in range(M)], -2)      # [n, M, K]
    return g.reshape(tuple(lead) + (M, K))


def _apply(gt, xf):
    """x_precoded [n, M] = G x for x [n, K] complex64."""
    K, M = len(gt), len(gt[0])
    xs = [_c(xf[:, k]) for k in range(K)]
    out = []
    for m in range(M):
        v = _zero(xf.shape[0])
        for k in range(K):
            v = v + gt[k][m] * xs[k]
        out.append(v.to_np())
    return np.stack(out, -1)


def _alpha(alpha, lead, leading_axis=False):
    a = np.asarray(alpha, F)
    pad = (1,) * (len(lead) - a.ndim)
    a = a.reshape(pad + a.shape if leading_axis else a.shape + pad)
    return np.ascontiguousarray(np.broadcast_to(a, tuple(lead))).reshape(-1)


def precoding_matrix(h, alpha=0., mode="rzf"):
    """h [..., K, M] -> G [..., M, K] (complex64)."""
    with np.errstate(all="ignore"):
        h = np.asarray(h, np.complex64)
        lead = h.shape[:-2]
        gt = _core(h.reshape((-1,) + h.shape[-2:]), _alpha(alpha, lead), mode)
        return _pack_g(gt, lead)


def rzf_precoder(x, h, alpha=0.):
    """(x_precoded [..., M], G [..., M, K]) for x [..., K], h [..., K, M]."""
    with np.errstate(all="ignore"):
        h, x = np.asarray(h, np.complex64), np.asarray(x, np.complex64)
        lead = np.broadcast_shapes(h.shape[:-2], x.shape[:-1])
        K, M = h.shape[-2:]
        hf = np.broadcast_to(h, lead + (K, M)).reshape(-1, K, M)
        xf = np.broadcast_to(x, lead + (K,)).reshape(-1, K)
        gt = _core(hf, _alpha(alpha, lead), "rzf")
        return _apply(gt, xf).reshape(lead + (M,)), _pack_g(gt, lead)


def ofdm_rzf_precoder(x, h, precoding_ind, effective_subcarrier_ind, alpha=0., batch=None):
    """RZFPrecoder.call with return_effective_channel=True: x [B, tx, K, T, F], h [B, rx, rxa, tx, M, T, F] ->
    (x_precoded [B', tx, M, T, F], h_eff [B', rx, rxa, tx, K, T, F_eff]), B' = the batch entries ``batch`` (all if None)."""
    with np.errstate(all="ignore"):
        x, h = np.asarray(x, np.complex64), np.asarray(h, np.complex64)
        B, ntx, K, T, Fft = x.shape
        a = _alpha(alpha, (B, ntx, T, Fft), leading_axis=True).reshape(B, ntx, T, Fft)
        if batch is not None:
            x, h, a = x[batch], h[batch], a[batch]
            B = x.shape[0]
        rx, rxa, M = h.shape[1], h.shape[2], h.shape[4]
        pind = np.asarray(precoding_ind).reshape(ntx, -1)
        # intended channels [B, tx, T, F, K, M]: rows k = (receiver pind[tx, k // rxa], antenna k % rxa)
        hd = np.stack([np.stack([h[:, pind[t, k // rxa], k % rxa, t] for k in range(K)], 1) for t in range(ntx)], 1)
        hd = np.transpose(hd, [0, 1, 4, 5, 2, 3])                                   # [B, tx, T, F, K, M]
        gt = _core(hd.reshape(-1, K, M), a.reshape(-1), "rzf")
        xd = np.transpose(x, [0, 1, 3, 4, 2]).reshape(-1, K)
        xp = _apply(gt, xd).reshape(B, ntx, T, Fft, M).transpose(0, 1, 4, 2, 3)
        # effective channel: every receiver, every antenna, at the effective subcarriers
        sc = np.asarray(effective_subcarrier_ind)
        hr = h[..., sc]                                                              # [B, rx, rxa, tx, M, T, Fe]
        Fe = len(sc)
        g_re = [[gt[k][m].re.reshape(B, ntx, T, Fft)[..., sc] for m in range(M)] for k in range(K)]
        g_im = [[gt[k][m].im.reshape(B, ntx, T, Fft)[..., sc] for m in range(M)] for k in range(K)]
        heff = np.zeros((B, rx, rxa, ntx, K, T, Fe), np.complex64)
        for k in range(K):
            v = _zero((B, rx, rxa, ntx, T, Fe))
            for m in range(M):
                g = C(g_re[k][m][:, None, None], g_im[k][m][:, None, None])           # [B, 1, 1, tx, T, Fe]
                v = v + _c(hr[:, :, :, :, m]) * g
            heff[:, :, :, :, k] = v.to_np()
        return xp, heff
