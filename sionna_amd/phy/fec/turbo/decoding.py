"""Turbo decoding - mirror of reference src/sionna/phy/fec/turbo/decoding.py: ``TurboDecoder`` (:15-435) on the HIP kernel
``samd_turbo_bcjr_f32`` / ``_f64`` (csrc/turbo.hip).  A call is 2 ``num_iter`` launches of that kernel, one per
half-iteration: the BCJR pass of one constituent code reading the punctured codeword through an index table, with the
extrinsic value, its clipping and the (de)interleaving folded into the backward pass."""
import math

import torch

from .... import _ffi
from ...block import Block, wrap
from .. import interleaving
from ..conv.decoding import _ALGORITHMS
from ..conv.utils import Trellis, kernel_code
from .encoding import _Tables
from .utils import TurboTermination, polynomial_selector, puncture_pattern

_EXT1, _EXT2, _FINAL = 0, 1, 2                                       # SAMD_TURBO_EXT1 / _EXT2 / _FINAL


class TurboDecoder(Block):
    """``TurboDecoder(encoder=None, gen_poly=None, rate=1/3, constraint_length=None, interleaver='3GPP', terminate=False,
    num_iter=6, hard_out=True, algorithm='map')(llr_ch [..., n]) -> [..., k]`` LLRs log p(1)/p(0) of the information bits,
    or hard decisions (decoding.py:101-208, 357-435)."""

    def __init__(self,
                 encoder=None,
                 gen_poly=None,
                 rate=1/3,
                 constraint_length=None,
                 interleaver='3GPP',
                 terminate=False,
                 num_iter=6,
                 hard_out=True,
                 algorithm='map',
                 precision=None,
                 **kwargs):
        super().__init__(precision=precision, **kwargs)
        if encoder is not None:
            self._coderate = encoder._coderate_desired
            self._gen_poly = encoder._gen_poly
            self._terminate = encoder.terminate
            self._trellis = encoder.trellis
            assert self._trellis.rsc is True
            self.rsc = True
            self.internal_interleaver = encoder.internal_interleaver
        else:
            if gen_poly is not None:
                if not all(isinstance(poly, str) for poly in gen_poly):
                    raise TypeError("Each polynomial must be a string.")
                if not all(len(poly) == len(gen_poly[0]) for poly in gen_poly):
                    raise ValueError("Each polynomial must be of same length.")
                if not all(all(char in ['0', '1'] for char in poly) for poly in gen_poly):
                    raise ValueError("Each polynomial must be a string of 0's and 1's.")
                self._gen_poly = gen_poly
            else:
                valid_constraint_length = (3, 4, 5, 6)
                if constraint_length not in valid_constraint_length:
                    raise ValueError("Constraint length must be between 3 and 6.")
                self._gen_poly = polynomial_selector(constraint_length)
            valid_rates = (1/2, 1/3)
            if rate not in valid_rates:
                raise ValueError("rate must be 1/3 or 1/2.")
            self._coderate = rate
            if not isinstance(terminate, bool):
                raise TypeError("terminate must be bool.")
            self._terminate = terminate
            if interleaver not in ('3GPP', 'random'):
                raise ValueError("interleaver must be 3GPP or random.")
            if interleaver == '3GPP':
                self.internal_interleaver = interleaving.Turbo3GPPInterleaver(precision=precision)
            else:
                self.internal_interleaver = interleaving.RandomInterleaver(keep_batch_constant=True, keep_state=True,
                                                                           axis=-1, precision=precision)
            self.rsc = True
            self._trellis = Trellis(self._gen_poly, rsc=self.rsc)
        if not isinstance(hard_out, bool):
            raise TypeError('hard_out must be bool.')
        if algorithm not in _ALGORITHMS:
            raise ValueError("algorithm must be one of map, log or maxlog")
        self._polys, _, self._cl = kernel_code(self._gen_poly)      # refuses constraint lengths beyond 8
        self._coderate_conv = 1/len(self._gen_poly)
        self.punct_pattern = puncture_pattern(self._coderate, self._coderate_conv)
        self._conv_k = self._trellis.conv_k
        self._mu = self._trellis._mu
        self._conv_n = self._trellis.conv_n
        self._ni = 2**self._conv_k
        self._no = 2**self._conv_n
        self._ns = self._trellis.ns
        if self._conv_k != 1:
            raise NotImplementedError("Only single bit stream support.")
        if self._conv_n != 2:
            raise NotImplementedError("Only single bit stream support.")
        self._k = None
        self._n = None
        if self._terminate:
            self.turbo_term = TurboTermination(self._mu+1, conv_n=self._conv_n)
            self._num_term_bits = 3 * self.turbo_term.get_num_term_syms()
        else:
            self._num_term_bits = 0
        self.num_iter = num_iter
        self._hard_out = hard_out
        self._algorithm = algorithm
        self._tables = _Tables(self._coderate, self._terminate, self._mu, self.internal_interleaver)
        self._ws = _ffi.Workspace()

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
        return self._coderate

    @property
    def trellis(self):
        """Trellis object used during encoding"""
        return self._trellis

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

    def depuncture(self, y):
        """``y`` [batch, n] scattered into [batch, 3 rate n], the punctured positions 0 (decoding.py:254-269).  The decoder
        itself reads ``y`` through index tables instead."""
        y = _ffi.to_device(y, self.rdtype)
        if self._n is None or y.shape[-1] != self._n:
            self.build(y.shape)
        rows = self._depunct_len // 3
        mask = self.punct_pattern.repeat(-(-rows // self.punct_pattern.shape[0]), 1)[:rows].reshape(-1)
        out = torch.zeros((y.shape[0], self._depunct_len), dtype=y.dtype, device=y.device)
        out[:, mask.to(y.device)] = y
        return wrap(out)

    def build(self, input_shape):
        """n from the last dimension, k from n (decoding.py:318-338)"""
        n = int(input_shape[-1])
        if self.coderate == 1/2:
            if n % 2 != 0:
                raise ValueError("Codeword length should be a multiple of 2")
        codefactor = self.coderate * 3
        turbo_n = int(n * codefactor)
        turbo_n_preterm = turbo_n - self._num_term_bits
        if turbo_n_preterm % 3 != 0 or turbo_n_preterm < 0:
            raise ValueError("Invalid codeword length for a terminated Turbo code")
        self._n = n
        self._k = int(turbo_n_preterm/3)
        self._convenc_numsyms = self._k
        if self._terminate:
            self._convenc_numsyms += self._mu
        self._depunct_len = int(3. * self._coderate * n)
        if isinstance(self.internal_interleaver, interleaving.Turbo3GPPInterleaver) and self._k > 6144:
            raise ValueError("3GPP Turbo Interleaver is defined for block lengths up to 6144.")

    def call(self, llr_ch, /):
        if llr_ch.shape[-1] != self._n:                             # allow different codeword lengths (decoding.py:371-373)
            self.build(llr_ch.shape)
        dbl = self.precision == "double"
        y = _ffi.to_device(llr_ch, torch.float64 if dbl else torch.float32)
        lead = tuple(y.shape[:-1])
        y = y.reshape(math.prod(lead), self._n).contiguous()
        batch, k, T = y.shape[0], self._k, self._convenc_numsyms
        out = torch.zeros((batch, k), dtype=y.dtype, device=y.device) if self.num_iter < 1 else \
            torch.empty((batch, k), dtype=y.dtype, device=y.device)
        if batch and k and self.num_iter >= 1:
            host, dev = self._tables.get(k)
            if host["n"] != self._n:
                raise ValueError("Invalid codeword length for a terminated Turbo code")
            la = torch.zeros((2, batch, T), dtype=y.dtype, device=y.device)     # a priori of decoder 1 / 2; the mu tail slots stay 0
            nbytes = _ffi.lib().samd_turbo_workspace_bytes(self._cl, T, batch, int(dbl))
            ws, wsb = self._ws.get(nbytes)
            fn = _ffi.lib().samd_turbo_bcjr_f64 if dbl else _ffi.lib().samd_turbo_bcjr_f32
            alg, stream = _ALGORITHMS[self._algorithm], _ffi.stream()

            def half(idx, la_in, scat, mode, dst):
                _ffi.check(fn(_ffi.ptr(y), _ffi.ptr(dev[idx]), _ffi.ptr(la_in), _ffi.ptr(dev[scat]), batch, self._n, k,
                              self._polys.ctypes.data, self._cl, int(self._terminate), alg, mode, int(self._hard_out),
                              _ffi.ptr(dst), _ffi.ptr(ws), wsb, stream), "TurboDecoder")

            for it in range(self.num_iter):
                half("idx1", la[0], "inv", _EXT1, la[1])
                if it + 1 < self.num_iter:
                    half("idx2", la[1], "perm", _EXT2, la[0])
                else:
                    half("idx2", la[1], "perm", _FINAL, out)
        return wrap(out.reshape(lead + (k,)))
