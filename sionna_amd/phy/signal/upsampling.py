"""``Upsampling`` (reference src/sionna/phy/signal/upsampling.py:12-65): zeros after every sample of an axis."""
import torch

from ._block import SignalBlock


class Upsampling(SignalBlock):
    """Inserts ``samples_per_symbol`` - 1 zeros after every sample of ``axis``: [..., n, ...] -> [..., n * samples_per_symbol, ...].
    A strided copy; ``upfirdn`` filters without forming this tensor."""

    def __init__(self, samples_per_symbol, axis=-1, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        self._samples_per_symbol = samples_per_symbol
        self._axis = axis

    def call(self, inputs):
        x = torch.swapaxes(inputs, self._axis, -1)
        y = torch.zeros(x.shape + (self._samples_per_symbol,), dtype=x.dtype, device=x.device)
        y[..., 0] = x
        return torch.swapaxes(y.reshape(*x.shape[:-1], -1), -1, self._axis)
