"""Erbium-doped fibre amplifier - mirror of reference src/sionna/phy/channel/optical/edfa.py:14-170.

One streaming launch of csrc/optical.hip per call: the gain and the ASE noise of the element-indexed Philox stream
(DESIGN.md "Optical channels")."""
import math

import torch

from .... import _ffi
from ... import constants
from ...block import Block
from ...config import config


class EDFA(Block):
    """``EDFA(g, f, f_c, dt)(x)``: y = sqrt(g) x + n with the ASE noise power 2 n_sp (g - 1) h f_c / dt per polarisation
    (halved with ``with_dual_polarization``, where axis [-2] of x holds the two polarisations), n_sp = f / 2 g / (g - 1)
    and 0 at g = 1."""

    def __init__(self, g=4.0, f=7.0, f_c=193.55e12, dt=1e-12, with_dual_polarization=False, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        # like SSFM, the parameters stay float64 in either precision (the reference rounds them to the block's real type);
        # what the kernel receives - sqrt(g) and the noise's standard deviation - is rounded once to the block's precision
        r = self._np_rdtype
        self._g, self._f, self._f_c, self._dt = float(g), float(f), float(f_c), float(dt)
        assert isinstance(with_dual_polarization, bool), "with_dual_polarization must be bool."
        self._with_dual_polarization = with_dual_polarization
        # Spontaneous emission factor (:126-132)
        self._n_sp = 0.0 if self._g == 1.0 else self._f / 2.0 * self._g / (self._g - 1.0)
        self._rho_n_ase = self._n_sp * (self._g - 1.0) * constants.H * self._f_c     # noise density in (W/Hz)
        self._p_n_ase = 2.0 * self._rho_n_ase / self._dt                              # noise power in (W)
        if self._with_dual_polarization:
            self._p_n_ase = self._p_n_ase / 2.0
        self._sqrt_g = float(r(math.sqrt(self._g)))                                  # (:165)
        self._sigma = float(r(math.sqrt(self._p_n_ase / 2.0)))

    def call(self, inputs):
        x = inputs
        if self._with_dual_polarization and (x.dim() < 2 or x.shape[-2] != 2):
            raise ValueError("with_dual_polarization: axis [-2] of the input must have length 2 (x- and y-polarization)")
        x = _ffi.to_device(x, self.cdtype)
        y = torch.empty_like(x)
        fn = _ffi.lib().samd_edfa_c128 if self.precision == "double" else _ffi.lib().samd_edfa_c64
        # a fresh call of the stream per amplifier call, also for a noiseless amplifier (one rule for every configuration)
        _ffi.check(fn(_ffi.ptr(x), x.numel(), self._sqrt_g, self._sigma, config.rng.seed, config.rng.next_call(), _ffi.ptr(y),
                      _ffi.stream()), "EDFA")
        return y
