"""Convolutional encoding - mirror of reference src/sionna/phy/fec/conv/encoding.py: ``ConvEncoder`` (:10-292) on the HIP
kernels ``samd_conv_encode_f32`` / ``_f64`` (csrc/conv.hip: feed-forward codes one lane per output symbol, recursive
systematic codes one lane per codeword)."""
import math

import torch

from .... import _ffi
from ...block import Block, wrap
from .utils import Trellis, check_gen_poly, kernel_code, select_gen_poly


class ConvEncoder(Block):
    """``ConvEncoder(gen_poly=None, rate=1/2, constraint_length=3, rsc=False, terminate=False)(bits [..., k]) -> [..., n]``
    with n = k / rate, plus conv_n (constraint_length - 1) tail bits when ``terminate`` (encoding.py:96-292)."""

    def __init__(self,
                 gen_poly=None,
                 rate=1/2,
                 constraint_length=3,
                 rsc=False,
                 terminate=False,
                 precision=None,
                 **kwargs):
        super().__init__(precision=precision, **kwargs)
        if gen_poly is not None:
            check_gen_poly(gen_poly, "Each element of gen_poly must be a string.")
            self._gen_poly = gen_poly
        else:
            self._gen_poly = select_gen_poly(rate, constraint_length)
        self._rsc = rsc
        self._terminate = terminate
        self._coderate_desired = 1/len(self.gen_poly)
        self._coderate = self._coderate_desired
        self._trellis = Trellis(self.gen_poly, rsc=self._rsc)
        self._mu = self.trellis._mu
        self._conv_k = self._trellis.conv_k
        self._conv_n = self._trellis.conv_n
        self._ni = 2**self._conv_k
        self._no = 2**self._conv_n
        self._ns = self._trellis.ns
        self._polys, _, self._cl = kernel_code(self._gen_poly)
        self._k = None
        self._n = None

    @property
    def gen_poly(self):
        """Generator polynomial used by the encoder"""
        return self._gen_poly

    @property
    def coderate(self):
        """Rate of the code; with termination k / (k + mu) of the design rate once k is known (encoding.py:186-197)"""
        if self.terminate and self._k is None:
            print("Note that, due to termination, the true coderate is lower "
                  "than the returned design rate. "
                  "The exact true rate is dependent on the value of k and "
                  "hence cannot be computed before the first call().")
        elif self.terminate and self._k is not None:
            term_factor = self._k/(self._k + self._mu)
            self._coderate = self._coderate_desired*term_factor
        return self._coderate

    @property
    def trellis(self):
        """Trellis object used during encoding"""
        return self._trellis

    @property
    def terminate(self):
        """Indicates if the convolutional encoder is terminated"""
        return self._terminate

    @property
    def k(self):
        """Number of information bits per codeword"""
        if self._k is None:
            print("Note: The value of k cannot be computed before the first call().")
        return self._k

    @property
    def n(self):
        """Number of codeword bits"""
        if self._n is None:
            print("Note: The value of n cannot be computed before the first call().")
        return self._n

    def build(self, input_shape):
        """k from the last dimension (encoding.py:226-237); n = conv_n (k + mu) when terminated"""
        self._k = int(input_shape[-1])
        self._n = self._conv_n * (self._k + (self._mu if self._terminate else 0))
        self.num_syms = int(self._k//self._conv_k)

    def call(self, bits, /):
        if bits.shape[-1] != self._k:                               # rebuild when k changes (encoding.py:247-248)
            self.build(bits.shape)
        dbl = self.precision == "double"
        u = _ffi.to_device(bits, torch.float64 if dbl else torch.float32)
        lead = tuple(u.shape[:-1])
        u2 = u.reshape(math.prod(lead), self._k).contiguous()       # not -1: k = 0 (terminated, the tail alone) is allowed
        out = torch.empty((u2.shape[0], self._n), dtype=u.dtype, device=u.device)
        fn = _ffi.lib().samd_conv_encode_f64 if dbl else _ffi.lib().samd_conv_encode_f32
        _ffi.check(fn(_ffi.ptr(u2), u2.shape[0], self._k, self._polys.ctypes.data, self._conv_n, self._cl, int(self._rsc),
                      int(self._terminate), _ffi.ptr(out), _ffi.stream()), "ConvEncoder")
        return wrap(out.reshape(lead + (self._n,)))
