"""``OSDecoder`` - mirror of reference src/sionna/phy/fec/linear/decoding.py:14-478 on the HIP kernels
``samd_osd_decode_f32`` / ``_f64`` (csrc/osd.hip).  The kernels follow the specification tests/osd_f32.py: bit-packed rows,
patterns enumerated on the fly, no ``[bs, num_patterns, n]`` tensor."""
import itertools
import math

import numpy as np
import torch

from .... import _ffi
from ...block import Block, wrap
from ..utils import make_systematic, pcm2gm


class OSDecoder(Block):
    """``OSDecoder(enc_mat=None, t=0, is_pcm=False, encoder=None)(llr_ch [..., n]) -> [..., n]`` hard decisions of all
    codeword bits by ordered-statistics decoding of order ``t`` (LLRs log p(1)/p(0)).  ``enc_mat``: binary generator
    matrix [k, n], or a full-rank parity-check matrix [n-k, n] with ``is_pcm``.  ``encoder``: any encoder block with a
    property ``k``; its generator matrix is read by encoding the identity (``enc_mat`` is then ignored)."""

    def __init__(self,
                 enc_mat=None,
                 t=0,
                 is_pcm=False,
                 encoder=None,
                 precision=None,
                 **kwargs):
        super().__init__(precision=precision, **kwargs)
        if not isinstance(is_pcm, bool):
            raise TypeError('is_pcm must be bool.')
        self._llr_max = 100.                                        # the kernels clip to this value
        if enc_mat is not None:
            if isinstance(enc_mat, np.ndarray):
                data = enc_mat
            elif hasattr(enc_mat, "todense") and hasattr(enc_mat, "data"):      # scipy csr / csc
                data = np.asarray(enc_mat.data)
            else:
                raise TypeError("Unsupported dtype of pcm.")
            if not np.array_equal(data, data.astype(bool)):
                raise TypeError('PC matrix must be binary.')
            if hasattr(enc_mat, "todense"):
                enc_mat = np.asarray(enc_mat.todense())
        if int(t) != t:
            raise TypeError("t must be int.")
        self._t = int(t)
        if encoder is not None:
            if encoder.k is None:
                raise AttributeError("It seems as if the encoder is not "
                                     "initialized or has no attribute k.")
            u = torch.eye(int(encoder.k), dtype=torch.float32).unsqueeze(0)
            gm = np.asarray(encoder(u).squeeze(0).cpu().numpy())
        else:
            if enc_mat is None:
                raise AttributeError("enc_mat cannot be None if no encoder is provided.")
            if is_pcm:
                gm = pcm2gm(enc_mat)
            else:
                make_systematic(enc_mat)                            # raises for a rank-deficient matrix
                gm = enc_mat
        self._gm = np.asarray(gm).astype(self._np_rdtype)
        self._k, self._n = int(self._gm.shape[0]), int(self._gm.shape[1])
        num_symbols = self._num_error_patterns(self._n, self._t) * self._n
        if num_symbols > 1e9:
            print(f"Note: Required memory complexity is large for the "
                  f"given code parameters and t={t}. Please consider small "
                  f"batch-sizes to keep the inference complexity small and "
                  f"activate XLA mode if possible.")
        if num_symbols > 1e11:
            raise ResourceWarning("Due to its high complexity, OSD is not "
                                  "feasible for the selected parameters. "
                                  "Please consider using a smaller value for t.")
        # the kernels' own limits (n - k <= 512, the 64 KB LDS budget, fewer than 2^62 candidates), learnt here rather than
        # at the first call: the size query answers 0 for a code or an order it refuses and leaves the reason
        if _ffi.lib().samd_osd_workspace_bytes(self._k, self._n, self._t, 1) == 0:
            raise ValueError(_ffi.lib().samd_last_error().decode())
        # rows of G packed along n into 64-bit words, LSB = lowest column index
        words = (self._n + 63) // 64
        g = np.zeros((self._k, words * 64), np.uint8)
        g[:, :self._n] = self._gm.astype(np.uint8)
        self._rows = np.packbits(g.reshape(self._k, words, 64), axis=-1, bitorder="little").view(np.int64).reshape(self._k, words)
        self._dev = None
        self._ws = _ffi.Workspace()

    gm = property(lambda self: self._gm, doc="Generator matrix of the code")
    n = property(lambda self: self._n, doc="Codeword length")
    k = property(lambda self: self._k, doc="Number of information bits per codeword")
    t = property(lambda self: self._t, doc="Order of the OSD algorithm")

    def _num_error_patterns(self, n, t):
        """number of error patterns of t errors in n positions"""
        return math.comb(n, t)

    def _gen_error_patterns(self, n, t):
        """[C(n, t), t] int32: all patterns of t errors in n positions, in the order the kernels enumerate them"""
        return torch.tensor(list(itertools.combinations(range(n), t)), dtype=torch.int32).reshape(-1, t)

    def build(self, input_shapes):
        if not input_shapes[-1] == self._n:
            raise ValueError(f" Last dimension must be of size n={self._n}.")

    def call(self, llr_ch, /):
        dbl = self.precision == "double"
        x = _ffi.to_device(llr_ch, torch.float64 if dbl else torch.float32)
        if x.shape[-1] != self._n:
            raise ValueError(f" Last dimension must be of size n={self._n}.")
        if self._dev is None:
            self._dev = _ffi.to_device(self._rows, torch.int64)
        shape = tuple(x.shape)
        x2 = x.reshape(-1, self._n).contiguous()
        batch = x2.shape[0]
        out = torch.empty_like(x2)
        nbytes = _ffi.lib().samd_osd_workspace_bytes(self._k, self._n, self._t, batch)
        ws, wsb = self._ws.get(nbytes)
        fn = _ffi.lib().samd_osd_decode_f64 if dbl else _ffi.lib().samd_osd_decode_f32
        _ffi.check(fn(_ffi.ptr(x2), _ffi.ptr(self._dev), batch, self._k, self._n, self._t, _ffi.ptr(out), _ffi.ptr(ws), wsb,
                      _ffi.stream()), "OSDecoder")
        return wrap(out.reshape(shape))
