"""Linear precoding - mirror of reference src/sionna/phy/mimo/precoding.py: ``rzf_precoding_matrix`` (:12-88),
``cbf_precoding_matrix`` (:91-155) and ``rzf_precoder`` (:157-244) on the HIP kernel ``samd_precoding_matrix_c64`` /
``_c128`` (csrc/precoding.hip; 1 <= K <= M, K <= 16, M <= 32)."""
import numpy as np
import torch

from ... import _ffi
from ..block import wrap

MODE_RZF, MODE_CBF = 0, 1                   # SAMD_PRECODE_RZF / SAMD_PRECODE_CBF (include/sionna_amd.h)


def _dtypes(precision):
    from ..config import config
    dbl = (precision or config.precision) == "double"
    return dbl, (torch.complex128 if dbl else torch.complex64), (torch.float64 if dbl else torch.float32)


def _host_scalar(a):
    """float value of a host scalar (Python / NumPy number, 0-d or 1-element host array or CPU tensor), else None.
    Device tensors are not inspected (that would synchronise): they are expanded instead."""
    if isinstance(a, (int, float, np.number)):
        return float(a)
    if isinstance(a, np.ndarray) and a.size == 1:
        return float(a.reshape(-1)[0])
    if isinstance(a, torch.Tensor) and a.device.type == "cpu" and a.numel() == 1:
        return float(a.reshape(-1)[0])
    return None


def expand_alpha(alpha, lead, rdt, leading_axis=False):
    """(scalar value, per-item device tensor of shape ``lead`` or None).  The reference expands ``alpha`` with trailing unit
    dimensions (mimo/precoding.py:79, expand_to_rank(..., axis=-1)), RZFPrecoder with leading ones (ofdm/precoding.py:162,
    axis=0) before broadcasting."""
    a0 = _host_scalar(alpha)
    if a0 is not None:
        return a0, None
    a = _ffi.to_device(alpha, rdt)
    if a.dim() > len(lead):
        raise ValueError(f"alpha of shape {tuple(a.shape)} does not broadcast to the batch shape {tuple(lead)}")
    pad = (1,) * (len(lead) - a.dim())
    a = a.reshape(pad + tuple(a.shape) if leading_axis else tuple(a.shape) + pad)
    return 0.0, torch.broadcast_to(a, tuple(lead)).contiguous()


def _shape(v):
    return tuple(v.shape) if hasattr(v, "shape") else tuple(np.shape(v))


def _run(h, x, alpha, mode, want_g, precision, name):
    dbl, cdt, rdt = _dtypes(precision)
    hs = _shape(h)                                      # the arguments are checked before anything touches the device
    if len(hs) < 2:
        raise ValueError(f"{name}: h must have shape [..., K, M]")
    k, m = int(hs[-2]), int(hs[-1])
    if k > m:
        raise ValueError(f"{name}: K = {k} streams exceed M = {m} transmit antennas (K <= M required)")
    if k > 16 or m > 32:
        raise ValueError(f"{name}: supported up to K = 16 streams and M = 32 transmit antennas (got K = {k}, M = {m})")
    lead = hs[:-2]
    if x is not None:
        xs = _shape(x)
        if len(xs) < 1 or int(xs[-1]) != k:
            raise ValueError(f"{name}: x must have shape [..., K] with K = {k}, got {xs}")
        try:
            lead = tuple(torch.broadcast_shapes(lead, xs[:-1]))
        except RuntimeError as e:
            raise ValueError(f"{name}: the batch shapes of x {xs} and h {hs} do not broadcast") from e
        x = torch.broadcast_to(_ffi.to_device(x, cdt), lead + (k,)).contiguous()
    h = torch.broadcast_to(_ffi.to_device(h, cdt), lead + (k, m)).contiguous()
    a0, a = expand_alpha(alpha, lead, rdt) if mode == MODE_RZF else (0.0, None)
    n = h.numel() // (k * m)
    g = torch.empty(lead + (m, k), dtype=cdt, device=h.device) if want_g else None
    xp = torch.empty(lead + (m,), dtype=cdt, device=h.device) if x is not None else None
    fn = _ffi.lib().samd_precoding_matrix_c128 if dbl else _ffi.lib().samd_precoding_matrix_c64
    _ffi.check(fn(_ffi.ptr(h), _ffi.ptr(x), _ffi.ptr(a), a0, n, k, m, mode, _ffi.ptr(g), _ffi.ptr(xp), _ffi.stream()), name)
    return xp, g


def rzf_precoding_matrix(h, alpha=0., precision=None):
    """h [..., K, M] -> G [..., M, K] = V D, V = H^H (H H^H + alpha I)^-1, D = diag(1 / ||v_k||) (precoding.py:12-88)."""
    return wrap(_run(h, None, alpha, MODE_RZF, True, precision, "rzf_precoding_matrix")[1])


def cbf_precoding_matrix(h, precision=None):
    """h [..., K, M] -> G [..., M, K] = H^H D with unit-norm columns (precoding.py:91-155)."""
    return wrap(_run(h, None, 0.0, MODE_CBF, True, precision, "cbf_precoding_matrix")[1])


def rzf_precoder(x, h, alpha=0., return_precoding_matrix=False, precision=None):
    """x [..., K], h [..., K, M] -> x_precoded [..., M] = G x, and G [..., M, K] with ``return_precoding_matrix``
    (precoding.py:157-244)."""
    xp, g = _run(h, x, alpha, MODE_RZF, bool(return_precoding_matrix), precision, "rzf_precoder")
    return (wrap(xp), wrap(g)) if return_precoding_matrix else wrap(xp)
