"""``RowColumnInterleaver`` and ``Deinterleaver`` - mirrors of reference
src/sionna/phy/fec/interleaving.py:12-195, 500-596 (a gather along one axis through
``samd_gather3``), ``RandomInterleaver`` (:198-497) with one permutation for the whole batch, and
``Turbo3GPPInterleaver`` (:598-745), the quadratic permutation polynomial interleaver of the LTE turbo code."""
import numpy as np
import torch

from ... import _ffi
from ..block import Block, wrap


class RowColumnInterleaver(Block):
    """``RowColumnInterleaver(row_depth, axis=-1, inverse=False)(x, inverse=None)``."""

    def __init__(self, row_depth, axis=-1, inverse=False, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        if not isinstance(axis, int):
            raise TypeError("axis must be int.")
        self._axis = axis
        if not isinstance(row_depth, int):
            raise TypeError("row_depth must be int.")
        self._row_depth = row_depth
        if not isinstance(inverse, bool):
            raise TypeError("inverse must be bool.")
        self._inverse = inverse
        self._keep_state = True
        self._perm_seq = self._perm_seq_inv = None
        self._dev = {}

    axis = property(lambda self: self._axis)
    row_depth = property(lambda self: self._row_depth)
    perm_seq = property(lambda self: self._perm_seq)
    perm_seq_inv = property(lambda self: self._perm_seq_inv)
    keep_state = property(lambda self: True)

    @staticmethod
    def _generate_perm_rc(n_seq, r_depth):
        """interleaving.py:111-144: write row-wise into rows of length ceil-padded n/r_depth ... read
        column-wise, dropping the filler positions."""
        n = int(np.ceil(n_seq / r_depth) * r_depth)
        ind = np.arange(n, dtype=np.int32).reshape(n // r_depth, -1).T.reshape(-1)
        perm = ind[ind < n_seq]
        return perm.astype(np.int32), np.argsort(perm).astype(np.int32)

    def build(self, input_shape, **kwargs):
        if self._axis >= len(input_shape) or self._axis < -len(input_shape):
            raise ValueError("Axis does match input shape")
        self._perm_seq, self._perm_seq_inv = self._generate_perm_rc(int(input_shape[self._axis]), self._row_depth)
        self._dev = {}

    def _device_perm(self, inverse):
        if inverse not in self._dev:
            p = self._perm_seq_inv if inverse else self._perm_seq
            self._dev[inverse] = (_ffi.to_device(p, torch.int32), _ffi.to_device(np.zeros(1, np.int32), torch.int32))
        return self._dev[inverse]

    def call(self, x, /, *, inverse=None, **kwargs):
        x = _ffi.to_device(x, self.rdtype)
        if self._perm_seq is None or x.shape[self._axis] != self._perm_seq.shape[0]:
            self.build(tuple(x.shape))
        inverse = self._inverse if inverse is None else bool(inverse)
        perm, zero = self._device_perm(inverse)
        xm = torch.movedim(x, self._axis, -1).contiguous()          # layout plumbing only
        n = xm.shape[-1]
        rows = xm.numel() // n if n else 0
        out = torch.empty_like(xm)
        if rows:
            _ffi.check(_ffi.lib().samd_gather3(_ffi.ptr(xm), _ffi.ptr(zero), _ffi.ptr(perm), rows, 1, n, 1, n, xm.element_size() // 4,
                                               _ffi.ptr(out), _ffi.stream()), "RowColumnInterleaver")
        return wrap(torch.movedim(out, -1, self._axis).contiguous())


class RandomInterleaver(Block):
    """``RandomInterleaver(seed=None, keep_batch_constant=True, inverse=False, keep_state=True, axis=-1)(x, seed=None,
    inverse=None)`` (interleaving.py:198-497): a pseudo-random permutation along ``axis`` = the argsort of i.i.d.
    draws (:330-366).  ``keep_state=True`` (default): one permutation for the block's lifetime, drawn from the build's
    Philox stream with the block's seed; an explicit ``seed`` in the call draws the permutation of that seed (the way the
    reference pairs an interleaver with its deinterleaver); ``keep_state=False`` without a seed: a fresh one per call.
    One permutation per batch EXAMPLE (``keep_batch_constant=False``) has no HIP path."""

    def __init__(self, seed=None, keep_batch_constant=True, inverse=False, keep_state=True, axis=-1, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        if not isinstance(keep_batch_constant, bool):
            raise TypeError("keep_batch_constant must be bool.")
        if not keep_batch_constant:
            raise NotImplementedError("RandomInterleaver: keep_batch_constant=False has no HIP path")
        if not isinstance(axis, int):
            raise TypeError("axis must be int.")
        if not isinstance(inverse, bool):
            raise TypeError("inverse must be bool.")
        if not isinstance(keep_state, bool):
            raise TypeError("keep_state must be bool.")
        if seed is not None and not isinstance(seed, int):
            raise TypeError("seed must be int.")
        if axis == 0:
            raise ValueError("Cannot permute batch_dim.")
        from ..config import config
        self._seed = int(seed) if seed is not None else int(config.rng.seed) * 7919 + int(config.rng.next_call()) + 1
        self._keep_batch_constant, self._inverse, self._keep_state, self._axis = True, inverse, keep_state, axis
        self._fresh = 0
        self._cache = {}

    seed = property(lambda self: self._seed)
    axis = property(lambda self: self._axis)
    keep_state = property(lambda self: self._keep_state)

    def _perm(self, seed, n):
        """(perm, inverse perm) int32 device tables of the permutation of ``seed`` for length n"""
        key = (int(seed), int(n))
        if key not in self._cache:
            if len(self._cache) > 64:
                self._cache.clear()
            r = torch.zeros(max(n, 1), dtype=torch.complex64, device=_ffi.device())
            one = torch.ones(1, dtype=torch.float32, device=r.device)
            _ffi.check(_ffi.lib().samd_awgn_c64(_ffi.ptr(r), _ffi.ptr(one), 1, key[0] & 0x7FFFFFFFFFFFFFFF, 1, r.numel(), _ffi.ptr(r),
                                                _ffi.stream()), "RandomInterleaver draws")      # CN(0, 1) on the stream (seed, call 1)
            perm = torch.argsort(r.real[:n], stable=True).to(torch.int32)               # (index plumbing)
            inv = torch.argsort(perm, stable=True).to(torch.int32)
            self._cache[key] = (perm.contiguous(), inv.contiguous(), _ffi.to_device(np.zeros(1, np.int32), torch.int32))
        return self._cache[key]

    def find_s_min(self, seed, seq_length, s_min_stop=0):
        """S-parameter of the permutation of ``seed`` (interleaving.py:285-328): the smallest distance between the images
        of any two positions less than S apart (host; analysis helper)."""
        perm = self._perm(seed, seq_length)[0].cpu().numpy().astype(np.int64)
        s_min = seq_length
        for i in range(len(perm)):
            for j in range(-s_min, s_min):
                if j == 0 or not 0 <= i + j < seq_length:
                    continue
                d = abs(perm[i] - perm[i + j])
                if d <= abs(j):
                    s_min = min(s_min, abs(j))
                if d < s_min and abs(j) < s_min:
                    s_min = min(s_min, int(d))
            if s_min <= s_min_stop:
                break
        return int(s_min)

    def call(self, x, /, *, seed=None, inverse=None, **kwargs):
        x = _ffi.to_device(x, self.rdtype)
        if self._axis >= x.dim() or self._axis < -x.dim():
            raise ValueError("Axis does not match input shape")
        if seed is None:
            if self._keep_state:
                seed = self._seed
            else:
                self._fresh += 1
                seed = self._seed + 104729 * self._fresh
        inverse = self._inverse if inverse is None else bool(inverse)
        xm = torch.movedim(x, self._axis, -1).contiguous()
        n = xm.shape[-1]
        perm, inv, zero = self._perm(int(seed), n)
        rows = xm.numel() // n if n else 0
        out = torch.empty_like(xm)
        if rows:
            _ffi.check(_ffi.lib().samd_gather3(_ffi.ptr(xm), _ffi.ptr(zero), _ffi.ptr(inv if inverse else perm), rows, 1, n, 1, n, xm.element_size() // 4,
                                               _ffi.ptr(out), _ffi.stream()), "RandomInterleaver")
        return wrap(torch.movedim(out, -1, self._axis).contiguous())


# 3GPP TS 36.212 Table 5.1.3-3: the coefficients (f1, f2) of the 188 block sizes K_i.  The sizes run 40, 48 .. 512 in
# steps of 8, 528 .. 1024 in steps of 16, 1056 .. 2048 in steps of 32 and 2112 .. 6144 in steps of 64.
_QPP_SIZES = tuple(list(range(40, 513, 8)) + list(range(528, 1025, 16)) + list(range(1056, 2049, 32))
                   + list(range(2112, 6145, 64)))
_QPP_F1_F2 = (
    (3, 10), (7, 12), (19, 42), (7, 16), (7, 18), (11, 20), (5, 22), (11, 24), (7, 26), (41, 84),
    (103, 90), (15, 32), (9, 34), (17, 108), (9, 38), (21, 120), (101, 84), (21, 44), (57, 46), (23, 48),
    (13, 50), (27, 52), (11, 36), (27, 56), (85, 58), (29, 60), (33, 62), (15, 32), (17, 198), (33, 68),
    (103, 210), (19, 36), (19, 74), (37, 76), (19, 78), (21, 120), (21, 82), (115, 84), (193, 86), (21, 44),
    (133, 90), (81, 46), (45, 94), (23, 48), (243, 98), (151, 40), (155, 102), (25, 52), (51, 106), (47, 72),
    (91, 110), (29, 168), (29, 114), (247, 58), (29, 118), (89, 180), (91, 122), (157, 62), (55, 84), (31, 64),
    (17, 66), (35, 68), (227, 420), (65, 96), (19, 74), (37, 76), (41, 234), (39, 80), (185, 82), (43, 252),
    (21, 86), (155, 44), (79, 120), (139, 92), (23, 94), (217, 48), (25, 98), (17, 80), (127, 102), (25, 52),
    (239, 106), (17, 48), (137, 110), (215, 112), (29, 114), (15, 58), (147, 118), (29, 60), (59, 122), (65, 124),
    (55, 84), (31, 64), (17, 66), (171, 204), (67, 140), (35, 72), (19, 74), (39, 76), (19, 78), (199, 240),
    (21, 82), (211, 252), (21, 86), (43, 88), (149, 60), (45, 92), (49, 846), (71, 48), (13, 28), (17, 80),
    (25, 102), (183, 104), (55, 954), (127, 96), (27, 110), (29, 112), (29, 114), (57, 116), (45, 354), (31, 120),
    (59, 610), (185, 124), (113, 420), (31, 64), (17, 66), (171, 136), (209, 420), (253, 216), (367, 444), (265, 456),
    (181, 468), (39, 80), (27, 164), (127, 504), (143, 172), (43, 88), (29, 300), (45, 92), (157, 188), (47, 96),
    (13, 28), (111, 240), (443, 204), (51, 104), (51, 212), (451, 192), (257, 220), (57, 336), (313, 228), (271, 232),
    (179, 236), (331, 120), (363, 244), (375, 248), (127, 168), (31, 64), (33, 130), (43, 264), (33, 134), (477, 408),
    (35, 138), (233, 280), (357, 142), (337, 480), (37, 146), (71, 444), (71, 120), (37, 152), (39, 462), (127, 234),
    (39, 158), (39, 80), (31, 96), (113, 902), (41, 166), (251, 336), (43, 170), (21, 86), (43, 174), (45, 176),
    (45, 178), (161, 120), (89, 182), (323, 184), (47, 186), (23, 94), (47, 190), (263, 480),
)
assert len(_QPP_SIZES) == len(_QPP_F1_F2) == 188
QPP_COEFFS = dict(zip(_QPP_SIZES, _QPP_F1_F2))


def qpp_perm(frame_size):
    """The permutation of ``Turbo3GPPInterleaver`` for ``frame_size`` <= 6144 as int32 (interleaving.py:678-709):
    pi(i) = (f1 i + f2 i^2) mod K; a size outside the table takes the next larger K of the table and drops the
    images >= frame_size (the reference's deviation from the standard, :629-634)."""
    frame_size = int(frame_size)
    if frame_size > _QPP_SIZES[-1]:
        raise ValueError("3GPP Turbo Interleaver is defined for block lengths up to 6144.")
    K = frame_size if frame_size in QPP_COEFFS else next(x for x in _QPP_SIZES if x >= frame_size)
    f1, f2 = QPP_COEFFS[K]
    i = np.arange(K, dtype=np.int64)
    perm = (f1 * i + f2 * i * i) % K
    return perm[perm < frame_size].astype(np.int32)


class Turbo3GPPInterleaver(Block):
    """``Turbo3GPPInterleaver(inverse=False, axis=-1)(x, inverse=None)`` (interleaving.py:598-745): the interleaver of
    the 3GPP turbo code, up to 6144 elements along ``axis``; lengths that the standard does not list are pruned from
    the next larger one.  A gather along ``axis`` through ``samd_gather3``."""

    def __init__(self, inverse=False, axis=-1, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        if not isinstance(axis, int):
            raise TypeError("axis must be int.")
        self._axis = axis
        self._keep_state = True                                     # only required for the deinterleaver
        self.frame_size = None
        if not isinstance(inverse, bool):
            raise TypeError("inverse must be boolean")
        self._inverse = inverse
        self.coeffs_dict = QPP_COEFFS
        self._host = {}
        self._dev = {}

    axis = property(lambda self: self._axis)
    keep_state = property(lambda self: True)

    def _generate_perm_full(self, frame_size, inverse=False):
        """int32 host permutation (or its inverse) of ``frame_size`` elements (interleaving.py:678-709)"""
        key = (int(frame_size), bool(inverse))
        if key not in self._host:
            perm = qpp_perm(frame_size)
            self._host[key] = np.argsort(perm, kind="stable").astype(np.int32) if inverse else perm
        return self._host[key]

    def build(self, input_shape, **kwargs):
        if not self.axis < len(input_shape):
            raise ValueError("Axis does not match input shape.")
        if input_shape[self._axis] >= 6145:
            raise ValueError("3GPP Turbo Interleaver is defined for block lengths up to 6144.")

    def _device_perm(self, frame_size, inverse):
        key = (int(frame_size), bool(inverse))
        if key not in self._dev:
            self._dev[key] = (_ffi.to_device(self._generate_perm_full(frame_size, inverse), torch.int32),
                              _ffi.to_device(np.zeros(1, np.int32), torch.int32))
        return self._dev[key]

    def call(self, x, /, *, inverse=None, **kwargs):                # **kwargs: a seed handed over by a deinterleaver
        x = _ffi.to_device(x, self.rdtype)
        self.build(tuple(x.shape))
        inverse = self._inverse if inverse is None else bool(inverse)
        xm = torch.movedim(x, self._axis, -1).contiguous()          # layout plumbing only
        n = xm.shape[-1]
        rows = xm.numel() // n if n else 0
        out = torch.empty_like(xm)
        if rows:
            perm, zero = self._device_perm(n, inverse)
            _ffi.check(_ffi.lib().samd_gather3(_ffi.ptr(xm), _ffi.ptr(zero), _ffi.ptr(perm), rows, 1, n, 1, n, xm.element_size() // 4,
                                               _ffi.ptr(out), _ffi.stream()), "Turbo3GPPInterleaver")
        return wrap(torch.movedim(out, -1, self._axis).contiguous())


class Deinterleaver(Block):
    """``Deinterleaver(interleaver)(x, seed=None)`` = ``interleaver(x, inverse=True)``."""

    def __init__(self, interleaver, precision=None, **kwargs):
        if not isinstance(interleaver, (RowColumnInterleaver, RandomInterleaver, Turbo3GPPInterleaver)):
            raise ValueError("interleaver is not a valid interleaver instance.")
        self._interleaver = interleaver
        super().__init__(precision=interleaver.precision if precision is None else precision, **kwargs)

    interleaver = property(lambda self: self._interleaver)

    def call(self, x, seed=None):
        return self._interleaver(x, seed=seed, inverse=True)
