"""Viterbi and BCJR decoding of convolutional codes - mirror of reference src/sionna/phy/fec/conv/decoding.py:
``ViterbiDecoder`` (:13-453) and ``BCJRDecoder`` (:456-943) on the HIP kernels ``samd_conv_viterbi_f32`` / ``_f64`` and
``samd_conv_bcjr_f32`` / ``_f64`` (csrc/conv.hip).  The kernels follow the order of operations of the specification
tests/conv_f32.py."""
import torch

from .... import _ffi
from ...block import Block, wrap
from .utils import Trellis, check_gen_poly, kernel_code, select_gen_poly

_METHODS = {"soft_llr": 0, "hard": 1}
_ALGORITHMS = {"map": 0, "log": 1, "maxlog": 2}              # SAMD_CONV_MAP / _LOG / _MAXLOG


class _ConvDecoderBase(Block):
    """code parameters and the properties both decoders share (decoding.py:105-213, 546-663)"""

    def _init_code(self, encoder, gen_poly, rate, constraint_length, rsc, terminate):
        if encoder is not None:
            self._gen_poly = encoder.gen_poly
            self._trellis = encoder.trellis
            self._terminate = encoder.terminate
        else:
            if gen_poly is not None:
                check_gen_poly(gen_poly, "Each polynomial must be a string.")
                self._gen_poly = gen_poly
            else:
                self._gen_poly = select_gen_poly(rate, constraint_length)
            self._trellis = Trellis(self.gen_poly, rsc=rsc)
            self._terminate = terminate
        self._coderate_desired = 1/len(self.gen_poly)
        self._mu = len(self._gen_poly[0])-1
        self._conv_k = self._trellis.conv_k
        self._conv_n = self._trellis.conv_n
        self._ni = 2**self._conv_k
        self._no = 2**self._conv_n
        self._ns = self._trellis.ns
        self._k = None
        self._n = None
        self._num_syms = None
        self._polys, _, self._cl = kernel_code(self._gen_poly)
        self._ws = _ffi.Workspace()

    @property
    def gen_poly(self):
        """Generator polynomial used by the encoder"""
        return self._gen_poly

    @property
    def coderate(self):
        """Rate of the code; with termination (n rate - mu) / n once n is known"""
        if self.terminate and self._n is None:
            print("Note that, due to termination, the true coderate is lower "
                  "than the returned design rate. "
                  "The exact true rate is dependent on the value of n and "
                  "hence cannot be computed before the first call().")
            self._coderate = self._coderate_desired
        elif self.terminate and self._n is not None:
            k = self._coderate_desired*self._n - self._mu
            self._coderate = k/self._n
        else:
            self._coderate = self._coderate_desired
        return self._coderate

    @property
    def trellis(self):
        """Trellis object used during encoding"""
        return self._trellis

    @property
    def terminate(self):
        """Indicates if the encoder is terminated during codeword generation"""
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

    def build(self, input_shape, **kwargs):
        """n from the last dimension (decoding.py:388-401, 885-897)"""
        n = int(input_shape[-1])
        if n % self._conv_n != 0:
            raise ValueError("Length of codeword should be divisible by number of output bits per symbol.")
        self._n = n
        self._num_syms = n // self._conv_n
        self._num_term_syms = self._mu if self._terminate else 0
        self._k = self._num_syms - self._num_term_syms
        if self._k < 0:
            raise ValueError(f"codeword of {n} bits is shorter than the termination tail")

    def _prepare(self, x):
        """reshape to [batch, n] on the device of the block's precision; rebuild when n changes"""
        if x.shape[-1] != self._n:
            self.build(x.shape)
        dbl = self.precision == "double"
        x = _ffi.to_device(x, torch.float64 if dbl else torch.float32)
        lead = tuple(x.shape[:-1])
        return dbl, lead, x.reshape(-1, self._n).contiguous()

    def _workspace(self, decoder, batch, dbl):
        nbytes = _ffi.lib().samd_conv_workspace_bytes(decoder, self._cl, self._num_syms, batch, int(dbl))
        return self._ws.get(nbytes)


class ViterbiDecoder(_ConvDecoderBase):
    """``ViterbiDecoder(encoder=None, gen_poly=None, rate=1/2, constraint_length=3, rsc=False, terminate=False,
    method='soft_llr', return_info_bits=True)(inputs [..., n]) -> [..., k]`` information bits, or ``[..., n]`` codeword
    bits along the survivor path when ``return_info_bits`` is False.  ``soft_llr``: LLRs log p(1)/p(0); ``hard``: inputs
    quantised to 0/1 (int_mod_2)."""

    def __init__(self,
                 *,
                 encoder=None,
                 gen_poly=None,
                 rate=1/2,
                 constraint_length=3,
                 rsc=False,
                 terminate=False,
                 method='soft_llr',
                 return_info_bits=True,
                 precision=None,
                 **kwargs):
        super().__init__(precision=precision, **kwargs)
        self._init_code(encoder, gen_poly, rate, constraint_length, rsc, terminate)
        if method not in ('soft_llr', 'hard'):
            raise ValueError("method must be `soft_llr` or `hard`.")
        self._method = method
        self._return_info_bits = return_info_bits

    def call(self, inputs, /):
        dbl, lead, y = self._prepare(inputs)
        batch = y.shape[0]
        m = self._k if self._return_info_bits else self._n
        out = torch.empty((batch, m), dtype=y.dtype, device=y.device)
        ws, wsb = self._workspace(0, batch, dbl)
        fn = _ffi.lib().samd_conv_viterbi_f64 if dbl else _ffi.lib().samd_conv_viterbi_f32
        _ffi.check(fn(_ffi.ptr(y), batch, self._n, self._polys.ctypes.data, self._conv_n, self._cl, int(self._trellis.rsc),
                      int(self._terminate), _METHODS[self._method], int(bool(self._return_info_bits)), _ffi.ptr(out),
                      _ffi.ptr(ws), wsb, _ffi.stream()), "ViterbiDecoder")
        return wrap(out.reshape(lead + (m,)))


class BCJRDecoder(_ConvDecoderBase):
    """``BCJRDecoder(encoder=None, gen_poly=None, rate=1/2, constraint_length=3, rsc=False, terminate=False, hard_out=True,
    algorithm='map')(llr_ch [..., n], llr_a=None) -> [..., k]``.  ``llr_a``: a priori LLRs of the information bits,
    [..., T] with T = n / conv_n trellis steps (the reference reshapes it so, decoding.py:917-920) or [..., k] (the tail
    steps then get a priori 0)."""

    def __init__(self,
                 encoder=None,
                 gen_poly=None,
                 rate=1/2,
                 constraint_length=3,
                 rsc=False,
                 terminate=False,
                 hard_out=True,
                 algorithm='map',
                 precision=None,
                 **kwargs):
        super().__init__(precision=precision, **kwargs)
        self._init_code(encoder, gen_poly, rate, constraint_length, rsc, terminate)
        if algorithm not in ['map', 'log', 'maxlog']:
            raise ValueError("algorithm must be one of map, log or maxlog")
        self._hard_out = hard_out
        self._algorithm = algorithm

    def call(self, llr_ch, /, *, llr_a=None):
        dbl, lead, y = self._prepare(llr_ch)
        batch = y.shape[0]
        a = None
        if llr_a is not None:
            a = _ffi.to_device(llr_a, y.dtype)
            T = self._num_syms
            if a.shape[-1] == self._k and self._k != T:
                a = torch.nn.functional.pad(a, (0, T - self._k))
            if a.shape[-1] != T or a.numel() != batch * T:
                raise ValueError(f"llr_a must have shape [..., {T}] matching llr_ch, got {tuple(a.shape)}")
            a = a.reshape(batch, T).contiguous()
        out = torch.empty((batch, self._k), dtype=y.dtype, device=y.device)
        ws, wsb = self._workspace(1, batch, dbl)
        fn = _ffi.lib().samd_conv_bcjr_f64 if dbl else _ffi.lib().samd_conv_bcjr_f32
        _ffi.check(fn(_ffi.ptr(y), _ffi.ptr(a), batch, self._n, self._polys.ctypes.data, self._conv_n, self._cl,
                      int(self._trellis.rsc), int(self._terminate), _ALGORITHMS[self._algorithm], int(bool(self._hard_out)),
                      _ffi.ptr(out), _ffi.ptr(ws), wsb, _ffi.stream()), "BCJRDecoder")
        return wrap(out.reshape(lead + (self._k,)))
