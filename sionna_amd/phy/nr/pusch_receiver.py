"""``PUSCHReceiver`` - recovers the information bits of batches of 5G NR PUSCH slots sent by a ``PUSCHTransmitter`` (mirror of
reference src/sionna/phy/nr/pusch_receiver.py:19-270): optional OFDM demodulation, channel estimation (or perfect channel
state), MIMO detection, layer demapping and transport-block decoding.  Every stage is a block of this package and runs on
the device; the default estimator is ``PUSCHLSChannelEstimator`` with linear interpolation on the fused DMRS kernel."""
import numpy as np
import torch

from ... import _ffi
from ..block import Block, wrap
from ..channel.utils import time_to_ofdm_channel
from ..mimo import StreamManagement
from ..ofdm import LinearDetector, OFDMDemodulator
from .layer_mapping import LayerDemapper
from .pusch_channel_estimation import PUSCHLSChannelEstimator
from .tb_decoder import TBDecoder


class PUSCHReceiver(Block):
    """``PUSCHReceiver(pusch_transmitter, channel_estimator=None, mimo_detector=None, tb_decoder=None,
    return_tb_crc_status=False, stream_management=None, input_domain="freq", l_min=None)``:
    ``(y, no[, h]) -> b_hat [batch, num_tx, tb_size]`` (and ``tb_crc_status [batch, num_tx]``);
    y [batch, num_rx, num_rx_ant, num_ofdm_symbols, fft_size], or [batch, num_rx, num_rx_ant, num_time_samples + l_max - l_min]
    in the time domain; ``h`` only with ``channel_estimator="perfect"``: [batch, num_rx, num_rx_ant, num_tx, num_tx_ant,
    num_ofdm_symbols, fft_size], or [..., num_time_samples + l_max - l_min, l_max - l_min + 1] in the time domain."""

    def __init__(self, pusch_transmitter, channel_estimator=None, mimo_detector=None, tb_decoder=None,
                 return_tb_crc_status=False, stream_management=None, input_domain="freq", l_min=None, precision=None, **kwargs):
        super().__init__(precision=precision, **kwargs)
        assert input_domain in ["time", "freq"], "input_domain must be 'time' or 'freq'"
        self._input_domain = input_domain
        self._return_tb_crc_status = return_tb_crc_status
        self._resource_grid = pusch_transmitter.resource_grid
        if self._input_domain == "time":
            assert l_min is not None, "l_min must be provided for input_domain==time"
            self._l_min = l_min
            self._ofdm_demodulator = OFDMDemodulator(fft_size=pusch_transmitter._num_subcarriers, l_min=self._l_min,
                                                     cyclic_prefix_length=pusch_transmitter._cyclic_prefix_length,
                                                     precision=self.precision)
        self._perfect_csi = False
        self._w = None
        if channel_estimator is None:
            self._channel_estimator = PUSCHLSChannelEstimator(self.resource_grid, pusch_transmitter._dmrs_length,
                                                              pusch_transmitter._dmrs_additional_position,
                                                              pusch_transmitter._num_cdm_groups_without_data,
                                                              interpolation_type="lin", precision=self.precision)
        elif isinstance(channel_estimator, str) and channel_estimator == "perfect":
            self._perfect_csi = True
            if pusch_transmitter._precoding == "codebook":
                self._w = np.stack(pusch_transmitter._precoding_matrices).astype(self._np_cdtype)    # [num_tx, ports, layers]
        else:
            self._channel_estimator = channel_estimator
        if stream_management is None:
            rx_tx_association = np.ones([1, pusch_transmitter._num_tx], bool)
            self._stream_management = StreamManagement(rx_tx_association, pusch_transmitter._num_layers)
        else:
            self._stream_management = stream_management
        # the default blocks take this block's precision; one without a double path refuses there, nothing is computed in
        # single silently
        what = f"PUSCHReceiver(precision='{self.precision}')"
        if mimo_detector is None:
            self._mimo_detector = self._own(what, LinearDetector, "lmmse", "bit", "maxlog", pusch_transmitter.resource_grid,
                                            self._stream_management, "qam", pusch_transmitter._num_bits_per_symbol,
                                            precision=self.precision)
        else:
            self._mimo_detector = mimo_detector
        self._layer_demapper = LayerDemapper(pusch_transmitter._layer_mapper,
                                             num_bits_per_symbol=pusch_transmitter._num_bits_per_symbol, precision=self.precision)
        if tb_decoder is None:
            self._tb_decoder = self._own(what, TBDecoder, pusch_transmitter._tb_encoder, precision=self.precision)
        else:
            self._tb_decoder = tb_decoder
        self._w_dev = None

    @staticmethod
    def _own(what, cls, *args, **kwargs):
        try:
            return cls(*args, **kwargs)
        except NotImplementedError as e:
            raise NotImplementedError(f"{what}: {cls.__name__} has no path in this precision ({e})") from e

    @property
    def resource_grid(self):
        """OFDM resource grid underlying the PUSCH transmissions"""
        return self._resource_grid

    def _effective_channel(self, h):
        """h [batch, num_rx, num_rx_ant, num_tx, num_tx_ant, T, F] times the transmitters' precoding matrices
        -> [batch, num_rx, num_rx_ant, num_tx, num_layers, T, F] (:238-252), one device einsum"""
        if self._w_dev is None:
            self._w_dev = _ffi.to_device(self._w, self.cdtype)
        return torch.einsum("brmtaof,tal->brmtlof", h.as_subclass(torch.Tensor), self._w_dev).contiguous()

    def call(self, y, no, h=None):
        if self._input_domain == "time":
            y = self._ofdm_demodulator(y)
        if self._perfect_csi:
            assert h is not None, "h must be provided with channel_estimator='perfect'"
            h = _ffi.to_device(h, self.cdtype)
            if self._input_domain == "time":
                h = time_to_ofdm_channel(h, self.resource_grid, self._l_min)
            if self._w is not None:
                h = self._effective_channel(h)
            h_hat, err_var = wrap(h), 0.0
        else:
            h_hat, err_var = self._channel_estimator(y, no)
        llr = self._mimo_detector(y, h_hat, err_var, no)
        llr = self._layer_demapper(llr)
        b_hat, tb_crc_status = self._tb_decoder(llr)
        if self._return_tb_crc_status:
            return b_hat, tb_crc_status
        return b_hat
