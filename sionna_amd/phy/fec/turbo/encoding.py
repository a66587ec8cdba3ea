"""Turbo encoding - mirror of reference src/sionna/phy/fec/turbo/encoding.py: ``TurboEncoder`` (:16-421) on the HIP kernel
``samd_turbo_encode_f32`` / ``_f64`` (csrc/turbo.hip): one launch, one lane per (codeword, constituent encoder), the
output bits written straight to their punctured positions."""
import math

import torch

from .... import _ffi
from ...block import Block, wrap
from .. import interleaving
from ..conv.utils import Trellis, kernel_code
from .utils import TurboTermination, polynomial_selector, puncture_pattern, turbo_tables


class _Tables:
    """the index tables of ``turbo_tables`` per k, on the host and on the device"""

    def __init__(self, coderate, terminate, mu, interleaver):
        self._args = (coderate, terminate, mu)
        self._interleaver = interleaver
        self._cache = {}

    def host_perm(self, k):
        il = self._interleaver
        if isinstance(il, interleaving.Turbo3GPPInterleaver):
            return il._generate_perm_full(k)
        return il._perm(il.seed, k)[0].cpu().numpy()                # RandomInterleaver: the block's own permutation

    def get(self, k):
        if k not in self._cache:
            if len(self._cache) > 16:
                self._cache.clear()
            host = turbo_tables(k, *self._args, self.host_perm(k))
            dev = {name: _ffi.to_device(host[name], torch.int32) for name in ("idx1", "idx2", "opos", "perm", "inv")}
            self._cache[k] = (host, dev)
        return self._cache[k]


class TurboEncoder(Block):
    """``TurboEncoder(gen_poly=None, constraint_length=3, rate=1/3, terminate=False, interleaver_type='3GPP')(bits
    [..., k]) -> [..., n]``: two identical rate-1/2 recursive systematic encoders, the second fed through the interleaver,
    rate 1/3 or punctured to 1/2; with ``terminate`` ceil(4 mu / 3) / rate more bits (encoding.py:97-175, 365-421).
    ``gen_poly``: two 0/1 strings of constraint length up to 8 (the reach of the BCJR kernel)."""

    def __init__(self,
                 gen_poly=None,
                 constraint_length=3,
                 rate=1/3,
                 terminate=False,
                 interleaver_type='3GPP',
                 precision=None,
                 **kwargs):
        super().__init__(precision=precision, **kwargs)
        if gen_poly is not None:
            if not all(isinstance(poly, str) for poly in gen_poly):
                raise TypeError("Each element of gen_poly must be a string.")
            if not all(len(poly) == len(gen_poly[0]) for poly in gen_poly):
                raise ValueError("Each polynomial must be of same length.")
            if not all(all(char in ['0', '1'] for char in poly) for poly in gen_poly):
                raise ValueError("Each Polynomial must be a string of 0/1 s.")
            if len(gen_poly) != 2:
                raise ValueError("Generator polynomials need to be of rate-1/2")
            self._gen_poly = gen_poly
        else:
            valid_constraint_length = (3, 4, 5, 6)
            if constraint_length not in valid_constraint_length:
                raise ValueError("Constraint length must be between 3 and 6.")
            self._gen_poly = polynomial_selector(constraint_length)
        valid_rates = (1/2, 1/3)
        if rate not in valid_rates:
            raise ValueError("Invalid coderate.")
        if not isinstance(terminate, bool):
            raise TypeError("terminate must be bool.")
        if interleaver_type not in ('3GPP', 'random'):
            raise ValueError("Invalid interleaver_type.")
        self._polys, _, self._cl = kernel_code(self._gen_poly)      # refuses constraint lengths beyond 8
        self._coderate_desired = rate
        self._coderate = self._coderate_desired
        self._terminate = terminate
        self._interleaver_type = interleaver_type
        rsc = True
        self._coderate_conv = 1/len(self.gen_poly)
        self._punct_pattern = puncture_pattern(rate, self._coderate_conv)
        self._trellis = Trellis(self.gen_poly, rsc=rsc)
        self._mu = self.trellis._mu
        self._conv_k = self._trellis.conv_k
        self._conv_n = self._trellis.conv_n
        self._ni = 2**self._conv_k
        self._no = 2**self._conv_n
        self._ns = self._trellis.ns
        self._k = None
        self._n = None
        if self.terminate:
            self.turbo_term = TurboTermination(self._mu+1, conv_n=self._conv_n)
        if self._interleaver_type == '3GPP':
            self.internal_interleaver = interleaving.Turbo3GPPInterleaver()
        else:
            self.internal_interleaver = interleaving.RandomInterleaver(keep_batch_constant=True, keep_state=True, axis=-1)
        if self.punct_pattern is not None:
            self.punct_idx = torch.nonzero(self.punct_pattern)
        self._tables = _Tables(rate, terminate, self._mu, self.internal_interleaver)

    @property
    def gen_poly(self):
        """Generator polynomial used by the encoder"""
        return self._gen_poly

    @property
    def constraint_length(self):
        """Constraint length of the encoder"""
        return self._mu + 1

    @property
    def coderate(self):
        """Rate of the code used in the encoder"""
        if self.terminate and self._k is None:
            print("Note that, due to termination, the true coderate is lower "
                  "than the returned design rate. "
                  "The exact true rate is dependent on the value of k and "
                  "hence cannot be computed before the first call().")
        elif self.terminate and self._k is not None:
            term_factor = 1+math.ceil(4*self._mu/3)/self._k
            self._coderate = self._coderate_desired/term_factor
        return self._coderate

    @property
    def trellis(self):
        """Trellis object used during encoding"""
        return self._trellis

    @property
    def terminate(self):
        """Indicates if the convolutional encoders are terminated"""
        return self._terminate

    @property
    def punct_pattern(self):
        """Puncturing pattern for the Turbo codeword"""
        return self._punct_pattern

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
        """k from the last dimension (encoding.py:347-363)"""
        self._k = int(input_shape[-1])
        self._n = int(self._k/self._coderate_desired)
        if self._interleaver_type == '3GPP':
            if self._k > 6144:
                raise ValueError('3GPP Turbo Codes define Interleavers only upto frame lengths of 6144')
        self.num_syms = int(self._k//self._conv_k)

    def call(self, bits, /):
        if bits.shape[-1] != self._k:
            self.build(bits.shape)
        dbl = self.precision == "double"
        u = _ffi.to_device(bits, torch.float64 if dbl else torch.float32)
        lead = tuple(u.shape[:-1])
        u2 = u.reshape(math.prod(lead), self._k).contiguous()
        host, dev = self._tables.get(self._k)
        n = host["n"]
        out = torch.empty((u2.shape[0], n), dtype=u.dtype, device=u.device)
        fn = _ffi.lib().samd_turbo_encode_f64 if dbl else _ffi.lib().samd_turbo_encode_f32
        _ffi.check(fn(_ffi.ptr(u2), _ffi.ptr(dev["perm"]), _ffi.ptr(dev["opos"]), u2.shape[0], self._k, n,
                      self._polys.ctypes.data, self._cl, int(self._terminate), int(host["zpos"][0]), int(host["zpos"][1]),
                      _ffi.ptr(out), _ffi.stream()), "TurboEncoder")
        return wrap(out.reshape(lead + (n,)))
