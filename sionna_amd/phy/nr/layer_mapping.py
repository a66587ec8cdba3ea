"""``LayerMapper`` / ``LayerDemapper`` - 38.211 Sec. 6.3.1.3 and 7.3.1.3 (mirror of reference
src/sionna/phy/nr/layer_mapping.py:11-291): symbol i of a codeword goes to layer i mod num_layers; with more than four
layers two codewords share the layers as Table 7.3.1.3-1 says.  Reshapes and one copy, no kernel: a host tensor stays on
the host, an array goes to the device like in every other block."""
import torch

from ..block import wrap
from ..signal._block import SignalBlock as _Block

# layers of the first and second codeword (Table 7.3.1.3-1)
_TWO_CODEWORDS = {5: (2, 3), 6: (3, 3), 7: (3, 4), 8: (4, 4)}


class LayerMapper(_Block):
    """``LayerMapper(num_layers=1, verbose=False)``: [..., n] -> [..., num_layers, n / num_layers]; for more than four
    layers a list of two inputs [..., n1], [..., n2]."""

    def __init__(self, num_layers=1, verbose=False, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        assert isinstance(verbose, bool), "verbose must be bool"
        assert num_layers in range(1, 9), "num_layers must be between 1 and 8."
        self._verbose, self._num_layers = verbose, num_layers
        self._num_codewords = 1 if num_layers < 5 else 2
        if self._num_codewords == 2:
            self._num_layers0, self._num_layers1 = _TWO_CODEWORDS[num_layers]
        if verbose:
            print("Number of layers: ", self._num_layers)
            if self._num_codewords == 2:
                print("Dual codeword mode active and cw multiplexing as defined in Tab. 7.3.1.3-1 from 38.211 applied.")
                print(f"Length of cw1/cw2: {self._num_layers0}/{self._num_layers1} ")

    num_codewords = property(lambda self: self._num_codewords)
    num_layers = property(lambda self: self._num_layers)
    num_layers0 = property(lambda self: self._num_layers if self._num_codewords == 1 else self._num_layers0)
    num_layers1 = property(lambda self: 0 if self._num_codewords == 1 else self._num_layers1)

    def __call__(self, inputs):
        if isinstance(inputs, (list, tuple)):               # two codewords: convert each like a single argument
            inputs = [self._convert_to_tensor(x) for x in inputs]
            self.build([tuple(x.shape) for x in inputs])
            self._built = True
            return wrap(self.call(inputs))
        return super().__call__(inputs)

    def build(self, input_shapes):
        if self._num_codewords == 1:
            assert not isinstance(input_shapes[0], (list, tuple)), "Only single input codeword expected."
            assert input_shapes[-1] % self._num_layers == 0, \
                "Invalid input dimensions: last dimension must be a multiple of num_layers."
        else:
            assert len(input_shapes) == 2 and all(isinstance(s, (list, tuple)) for s in input_shapes), \
                "List of two inputs streams is expected."
            s0, s1 = input_shapes
            assert s0[-1] % self._num_layers0 == 0, \
                "Invalid input dimensions: last dimension of first input must be a multiple of num_layers0."
            assert s1[-1] % self._num_layers1 == 0, \
                "Invalid input dimensions: last dimension of second input must be a multiple of num_layers1."
            assert s0[-1] / self._num_layers0 == s1[-1] / self._num_layers1, \
                f"Invalid input dimensions: length of first input must be {self._num_layers0 / self._num_layers1:.2f} " \
                "of the length of the second input."

    def call(self, inputs):
        if self._num_codewords == 1:
            y = inputs.reshape(inputs.shape[:-1] + (-1, self._num_layers))
        else:
            x0, x1 = inputs
            y = torch.cat([x0.reshape(x0.shape[:-1] + (-1, self._num_layers0)),
                           x1.reshape(x1.shape[:-1] + (-1, self._num_layers1))], dim=-1)
        return y.transpose(-1, -2).contiguous()


class LayerDemapper(_Block):
    """``LayerDemapper(layer_mapper, num_bits_per_symbol=1)``: [..., num_layers, n / num_layers] -> [..., n] (a list of two
    for two codewords).  ``num_bits_per_symbol`` consecutive values belong to one symbol, so LLRs can be demapped."""

    def __init__(self, layer_mapper, num_bits_per_symbol=1, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        assert isinstance(layer_mapper, LayerMapper), "layer_mapper must be LayerMapper."
        assert num_bits_per_symbol % 1 == 0, "num_bits_per_symbol must be int."
        self._mapper, self._num_bits_per_symbol = layer_mapper, int(num_bits_per_symbol)

    def build(self, input_shapes):
        assert input_shapes[-2] == self._mapper.num_layers, "Invalid input dimension: input shape must be [...,num_layers,n]."
        assert input_shapes[-1] % self._num_bits_per_symbol == 0, \
            "Invalid input dimension: last dimension must be a multiple of num_bits_per_symbol."

    def call(self, inputs):
        m = self._num_bits_per_symbol
        x = inputs.reshape(inputs.shape[:-1] + (-1, m)).transpose(-2, -3)      # [..., symbols, layers, m]
        lead = tuple(x.shape[:-3])
        if self._mapper.num_codewords == 1:
            return x.reshape(lead + (-1,))
        n0 = self._mapper.num_layers0
        return [x[..., :n0, :].reshape(lead + (-1,)), x[..., n0:, :].reshape(lead + (-1,))]
