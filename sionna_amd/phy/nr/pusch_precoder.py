"""``PUSCHPrecoder`` - codebook precoding of a batch of resource grids, one matrix per transmitter (mirror of reference
src/sionna/phy/nr/pusch_precoder.py:11-95).  The stand-alone block evaluates the arithmetic of the fused kernel
(csrc/pusch.hip, specification tests/pusch_f32.py) with element-wise tensor operations, one rounding each; inside
``PUSCHTransmitter`` the product is part of the fused launch."""
import numpy as np
import torch

from ..signal._block import SignalBlock as _Block


def precode(x, w):
    """x [batch, num_tx, num_layers, T, F] complex, w [num_tx, num_ports, num_layers] complex -> [batch, num_tx, num_ports,
    T, F]: per port the sum over layers in ascending order from +0 of (wr xr - wi xi) + j (wr xi + wi xr)"""
    xr, xi = x.real, x.imag
    wr, wi = w.real[None, :, :, :, None, None], w.imag[None, :, :, :, None, None]
    shape = (x.shape[0], x.shape[1], w.shape[1]) + tuple(x.shape[3:])
    acc_r, acc_i = torch.zeros(shape, dtype=xr.dtype, device=x.device), torch.zeros(shape, dtype=xr.dtype, device=x.device)
    for l in range(x.shape[2]):
        a, b = xr[:, :, l:l + 1], xi[:, :, l:l + 1]
        acc_r = acc_r + (wr[:, :, :, l] * a - wi[:, :, :, l] * b)
        acc_i = acc_i + (wr[:, :, :, l] * b + wi[:, :, :, l] * a)
    return torch.complex(acc_r, acc_i)


class PUSCHPrecoder(_Block):
    """``PUSCHPrecoder(precoding_matrices)``: [batch, num_tx, num_layers, num_symbols, num_subcarriers] ->
    [batch, num_tx, num_antenna_ports, num_symbols, num_subcarriers]."""

    def __init__(self, precoding_matrices, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        self._num_tx = len(precoding_matrices)
        shape = np.shape(precoding_matrices[0])
        for w in precoding_matrices:
            assert np.shape(w)[0] == shape[0] and np.shape(w)[1] == shape[1], "All precoding matrices must have the same shape"
        self._w = self._cast_or_check_precision(np.stack([np.asarray(w) for w in precoding_matrices]).astype(complex))

    def build(self, input_shape):
        _, num_tx, num_layers, _, _ = input_shape
        assert num_tx == len(self._w), \
            f"The input shape is for {num_tx} transmitters, but you have configured precoding matrices for {len(self._w)}."
        assert num_layers == self._w[0].shape[1], \
            f"You have configured precoding matrices for {self._w[0].shape[1]} layers, but the input provides {num_layers} layers."

    def call(self, inputs):
        if self._w.device != inputs.device:
            self._w = self._w.to(inputs.device)
        return precode(inputs, self._w)
