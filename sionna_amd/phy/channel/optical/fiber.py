"""Split-step Fourier method - mirror of reference src/sionna/phy/channel/optical/fiber.py:15-449.

The step loop runs inside one C-ABI call (csrc/optical.hip): rocFFT for the transforms, one fused time-domain kernel
(window, Kerr rotation, Raman ASE noise) and one fused frequency-domain kernel (dispersion, attenuation / gain and the
transform's 1/n as one factor per bin) between them; the adaptive step width is found on the device (DESIGN.md "Optical
channels").  The parameters enter the kernels' tables as float64 in either precision."""
import ctypes as C

import torch

from .... import _ffi
from ... import constants
from ...block import Block
from ...config import config


class SSFM(Block):
    """``SSFM(alpha, beta_2, f_c, gamma, half_window_length, length, n_ssfm, ...)(x)``: the symmetrised split-step
    solution of the nonlinear Schroedinger equation (the Manakov equation with ``with_manakov``, where axis [-2] of x holds
    the x- and y-polarisation) over ``length``, in ``n_ssfm`` steps or with ``n_ssfm="adaptive"`` in steps of at most
    ``phase_inc`` rad nonlinear phase rotation; optional ideal distributed Raman amplification with its noise, and a
    Hamming window of ``half_window_length`` samples at both ends in every step.  x [..., n] or [..., 2, n], complex; the
    output has the shape of x.  ``swap_memory`` is accepted and ignored."""

    def __init__(self, alpha=0.046, beta_2=-21.67, f_c=193.55e12, gamma=1.27, half_window_length=0, length=80, n_ssfm=1,
                 n_sp=1.0, sample_duration=1.0, t_norm=1e-12, with_amplification=False, with_attenuation=True,
                 with_dispersion=True, with_manakov=False, with_nonlinearity=True, phase_inc=1e-4, swap_memory=True,
                 precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        self._alpha = float(alpha)
        self._beta_2 = float(beta_2)
        self._f_c = float(f_c)
        self._gamma = float(gamma)
        self._half_window_length = int(half_window_length)
        self._length = float(length)
        self._phase_inc = float(phase_inc)
        if n_ssfm == "adaptive":
            self._n_ssfm = -1  # adaptive == -1
        elif isinstance(n_ssfm, int):
            self._n_ssfm = int(n_ssfm)
            if self._n_ssfm <= 0:
                raise ValueError("n_ssfm must be greater than 0.")
        else:
            raise ValueError("Unsupported parameter for n_ssfm. \
                              Either an integer or 'adaptive'.")
        self._dz = self._length / self._n_ssfm       # only used for the constant step width (:221-223)
        self._n_sp = float(n_sp)
        self._swap_memory = swap_memory
        self._t_norm = float(t_norm)
        self._sample_duration = float(sample_duration)
        self._with_amplification = bool(with_amplification)
        self._with_attenuation = bool(with_attenuation)
        self._with_dispersion = bool(with_dispersion)
        self._with_manakov = bool(with_manakov)
        self._with_nonlinearity = bool(with_nonlinearity)
        self._rho_n = constants.H * self._f_c * self._alpha * self._length * self._n_sp      # in (W/Hz)
        self._p_n_ase = self._rho_n / self._sample_duration / self._t_norm                   # noise power, simulation bandwidth
        if self._with_manakov:
            self._p_n_ase = self._p_n_ase / 2.0
        self._ws = _ffi.Workspace()
        self.last_num_steps = None                   # steps of the last call (the adaptive scheme's count)

    def call(self, inputs):
        x = inputs
        if self._with_manakov and (x.dim() < 2 or x.shape[-2] != 2):
            raise ValueError("with_manakov: axis [-2] of the input must have length 2 (x- and y-polarization)")
        if x.dim() < 1:
            raise ValueError("the input must have at least one dimension [..., n]")
        n = int(x.shape[-1])
        if 2 * self._half_window_length > n:
            raise ValueError(f"half_window_length {self._half_window_length} exceeds half of the signal length {n}")
        x = _ffi.to_device(x, self.cdtype)
        y = torch.empty_like(x)
        if x.numel() == 0:
            return y
        rows = x.numel() // n // (2 if self._with_manakov else 1)
        dbl = self.precision == "double"
        ws, ws_bytes = self._ws.get(_ffi.lib().samd_ssfm_workspace_bytes(n, int(dbl)))
        steps = C.c_int64(0)
        fn = _ffi.lib().samd_ssfm_c128 if dbl else _ffi.lib().samd_ssfm_c64
        _ffi.check(fn(_ffi.ptr(x), rows, n, int(self._with_manakov), self._alpha, self._beta_2, self._gamma, self._length,
                      self._sample_duration, self._n_ssfm, self._phase_inc, self._half_window_length, self._p_n_ase,
                      int(self._with_amplification), int(self._with_attenuation), int(self._with_dispersion),
                      int(self._with_nonlinearity), config.rng.seed, config.rng.call, C.byref(steps), _ffi.ptr(ws), ws_bytes,
                      _ffi.ptr(y), _ffi.stream()), "SSFM")
        config.rng.call += steps.value               # every step took a call of the stream of its own
        self.last_num_steps = steps.value
        return y
