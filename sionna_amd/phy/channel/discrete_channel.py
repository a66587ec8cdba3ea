"""Discrete channels - mirror of reference src/sionna/phy/channel/discrete_channel.py:10-596.

One streaming launch of csrc/discrete.hip per call: the draw, the selection of pb0 / pb1 by the input, the flip and the
hard or LLR output.  The error pattern is drawn directly on the element-indexed Philox stream (DESIGN.md "Discrete
channels"): there is no gradient through ``pb``, so ``temperature`` is accepted and stored but has no effect.
"""
import numpy as np
import torch

from ... import _ffi
from ..block import Block
from ..config import config

_ENTRY = {torch.float32: "f32", torch.float64: "f64", torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16",
          torch.int32: "i32", torch.int64: "i64"}
_SIGNED = (torch.float32, torch.float64, torch.int8, torch.int16, torch.int32, torch.int64)
_KIND_MEMORYLESS, _KIND_ERASURE = 0, 1


def _trailing_block(x_shape, pb_shape):
    """Shape of the smallest trailing block of x that contains pb (left-padded with ones): () for a single value."""
    if len(pb_shape) > len(x_shape):
        raise ValueError(f"pb of shape {tuple(pb_shape)} has more dimensions than x of shape {tuple(x_shape)}")
    s = (1,) * (len(x_shape) - len(pb_shape)) + tuple(pb_shape)
    for a, b in zip(s, x_shape):
        if a not in (1, b):
            raise ValueError(f"pb of shape {tuple(pb_shape)} does not broadcast to x of shape {tuple(x_shape)}")
    d = 0
    while d < len(s) and s[d] == 1:
        d += 1
    return s[d:], tuple(x_shape[d:])


class BinaryMemorylessChannel(Block):
    """``BinaryMemorylessChannel()(x, pb)``: x in {0,1} (or {-1,1} with ``bipolar_input``) is flipped with probability
    pb[..., 0] where it is the neutral element and pb[..., 1] elsewhere; ``pb`` is a tuple of two scalars (or of two
    tensors broadcastable to x) or a ``[..., 2]`` tensor.  With ``return_llrs`` the output is
    log((1 - pb1) / pb0) for a received 1 and log(pb1 / (1 - pb0)) for a received 0, clipped to +-``llr_max``."""

    _kind = _KIND_MEMORYLESS
    _allow_uint = True

    def __init__(self, return_llrs=False, bipolar_input=False, llr_max=100., precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        assert isinstance(return_llrs, bool), "return_llrs must be bool."
        self._return_llrs = return_llrs
        assert isinstance(bipolar_input, bool), "bipolar_input must be bool."
        self._bipolar_input = bipolar_input
        assert llr_max >= 0., "llr_max must be a positive scalar value."
        self._llr_max = self._round(llr_max)
        self._check_input = True                    # the binary / bipolar check runs on the first call only (:148-149)
        self._eps = 1e-9
        self._temperature = self._round(0.1)
        self._pairs = {}                            # (pb0, pb1) given as Python scalars -> device tensor [2]

    def _round(self, v):
        return float(self._np_rdtype(v))

    @property
    def llr_max(self):
        """Maximum value used for LLR calculations"""
        return self._llr_max

    @llr_max.setter
    def llr_max(self, value):
        assert value >= 0, "llr_max cannot be negative."
        self._llr_max = self._round(value)

    @property
    def temperature(self):
        """Temperature of the reference's Gumbel-softmax sampler: stored, without effect (no gradient through pb)"""
        return self._temperature

    @temperature.setter
    def temperature(self, value):
        assert value >= 0, "temperature cannot be negative."
        self._temperature = self._round(value)

    # ------------------------------------------------------------------ checks
    def _check_dtype(self, dtype):
        """:151-166; of torch's unsigned types only uint8 is carried"""
        if dtype not in _ENTRY:
            raise ValueError(f"{type(self).__name__}: dtype {dtype} is not supported (float32, float64, uint8, int8, int16, "
                             "int32 and int64 are)")
        if self._return_llrs:
            if not dtype.is_floating_point:
                raise ValueError("LLR outputs require non-integer dtypes.")
        elif self._bipolar_input and dtype not in _SIGNED:
            raise ValueError("Only signed dtypes are supported for bipolar inputs.")
        if not self._allow_uint and dtype not in _SIGNED:
            raise ValueError("Only signed dtypes supported.")

    def _check_inputs(self, x):
        """:134-149: one device reduction and one host read, on the first call only"""
        if self._check_input:
            lo = -1 if self._bipolar_input else 0
            if x.numel() and not bool(((x == lo) | (x == 1)).all().item()):
                raise ValueError("Input must be binary.")
            self._check_input = False

    def build(self, *input_shapes):
        """:224-236"""
        pb_shape = input_shapes[1]
        if self.__dict__.get("_pb_is_pair"):
            if self._pb_pair_len != 2:
                raise ValueError("Last dim of pb must be of length 2.")
        elif len(pb_shape) == 0 or pb_shape[-1] != 2:
            raise ValueError("Last dim of pb must be of length 2.")

    def __call__(self, x, pb):
        # the output has the dtype of x; Block.__call__ casts a float x to the block's precision (:253-254), the result is
        # converted back below (:291)
        if not isinstance(x, torch.Tensor):
            a = np.asarray(x)
            if a.dtype.kind == "b" or a.dtype in (np.uint16, np.uint32, np.uint64):
                raise ValueError(f"{type(self).__name__}: dtype {a.dtype} is not supported")
            x = torch.from_numpy(np.ascontiguousarray(a))
        self._check_dtype(x.dtype)
        self._in_dtype = x.dtype
        self._pb_is_pair = isinstance(pb, (tuple, list))
        self._pb_pair_len = len(pb) if self._pb_is_pair else None
        return super().__call__(x, pb)

    # ------------------------------------------------------------------ pb -> (tensor kept alive, ptr0, ptr1, stride, len)
    def _pb_single(self, pb, x, dtype):
        """scalar or any shape broadcastable to x -> contiguous values of the smallest trailing block that contains it"""
        pb = _ffi.to_device(pb, dtype)
        if pb.numel() == 1:
            return pb.reshape(1), 1
        s, block = _trailing_block(x.shape, pb.shape)
        pb = pb.reshape(s)
        if s != block:                                  # an interior broadcast dimension: expanded to that block only
            pb = pb.expand(block)
        pb = pb.contiguous()
        return pb, pb.numel()

    def _pb_pair(self, pb, x, dtype):
        """tuple of two or [..., 2] -> interleaved values [pb_len, 2]"""
        if isinstance(pb, (tuple, list)):
            if len(pb) != 2:
                raise ValueError("Last dim of pb must be of length 2.")
            if all(isinstance(v, (int, float)) for v in pb):
                key = (float(pb[0]), float(pb[1]), dtype)
                t = self._pairs.get(key)
                if t is None:
                    if len(self._pairs) > 64:
                        self._pairs.clear()
                    t = self._pairs[key] = torch.tensor([key[0], key[1]], dtype=torch.float64).to(dtype).to(_ffi.device())
                return t, 1
            a, b = torch.broadcast_tensors(_ffi.to_device(pb[0], dtype), _ffi.to_device(pb[1], dtype))
            pb = torch.stack((a, b), dim=-1)
        else:
            pb = _ffi.to_device(pb, dtype)
            if pb.dim() == 0 or pb.shape[-1] != 2:
                raise ValueError("Last dim of pb must be of length 2.")
        if pb.numel() == 2:
            return pb.reshape(2), 1
        s, block = _trailing_block(x.shape, pb.shape[:-1])
        pb = pb.reshape(s + (2,))
        if s != block:
            pb = pb.expand(block + (2,))
        pb = pb.contiguous()
        return pb, pb.numel() // 2

    def _pointers(self, x, pb, dtype):
        t, n = self._pb_pair(pb, x, dtype)
        base = t.data_ptr()
        return t, base, base + t.element_size(), 2, n

    # ------------------------------------------------------------------ the launch
    def call(self, x, pb):
        out_dtype = self.__dict__.pop("_in_dtype", x.dtype)
        self._check_dtype(out_dtype)
        x = _ffi.to_device(x, x.dtype if not x.dtype.is_floating_point else self.rdtype)
        pdtype = torch.float64 if x.dtype == torch.float64 else torch.float32
        keep, p0, p1, stride, plen = self._pointers(x, pb, pdtype)
        self._check_inputs(x)
        y = torch.empty_like(x)
        fn = getattr(_ffi.lib(), "samd_discrete_channel_" + _ENTRY[x.dtype])
        _ffi.check(fn(_ffi.ptr(x), p0, p1, stride, plen, self._kind, int(self._bipolar_input), int(self._return_llrs),
                      self._llr_max, config.rng.seed, config.rng.next_call(), x.numel(), _ffi.ptr(y), _ffi.stream()),
                   type(self).__name__)
        del keep
        return y if y.dtype == out_dtype else y.to(out_dtype)


class _SinglePb(BinaryMemorylessChannel):
    """the three channels that take one pb: a scalar or any shape broadcastable to x"""

    def build(self, *input_shapes):
        pass


class BinarySymmetricChannel(_SinglePb):
    """``BinarySymmetricChannel()(x, pb)``: bits are flipped with probability pb (:298-385)."""

    def _pointers(self, x, pb, dtype):
        t, n = self._pb_single(pb, x, dtype)
        return t, t.data_ptr(), t.data_ptr(), 1, n


class BinaryZChannel(_SinglePb):
    """``BinaryZChannel()(x, pb)``: a 1 (the non-neutral element) is flipped with probability pb, a 0 never (:387-478)."""

    def _pointers(self, x, pb, dtype):
        t, n = self._pb_single(pb, x, dtype)
        return t, None, t.data_ptr(), 1, n


class BinaryErasureChannel(_SinglePb):
    """``BinaryErasureChannel()(x, pb)``: an element is erased with probability pb - output -1 (0 for bipolar input), or
    LLR 0; unerased elements pass, as +-llr_max with ``return_llrs`` (:480-596)."""

    _kind = _KIND_ERASURE
    _allow_uint = False

    def _pointers(self, x, pb, dtype):
        t, n = self._pb_single(pb, x, dtype)
        return t, None, t.data_ptr(), 1, n
