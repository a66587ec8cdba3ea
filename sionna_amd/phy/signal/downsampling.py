"""``Downsampling`` (reference src/sionna/phy/signal/downsampling.py:9-72): one sample out of ``samples_per_symbol``."""
import torch

from ._block import SignalBlock


class Downsampling(SignalBlock):
    """Keeps the samples ``offset``, ``offset + samples_per_symbol``, ... of ``axis``, at most ``num_symbols`` of them:
    [..., n, ...] -> [..., min((n - offset) / samples_per_symbol rounded up, num_symbols), ...].  A strided copy; ``upfirdn``
    computes only the kept outputs of a filter."""

    def __init__(self, samples_per_symbol, offset=0, num_symbols=None, axis=-1, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        self._samples_per_symbol = samples_per_symbol
        self._offset = offset
        self._num_symbols = num_symbols
        self._axis = axis

    def call(self, inputs):
        x = torch.swapaxes(inputs, self._axis, -1)
        x = x[..., self._offset::self._samples_per_symbol]
        if self._num_symbols is not None:
            x = x[..., :self._num_symbols]
        return torch.swapaxes(x, -1, self._axis).contiguous()
