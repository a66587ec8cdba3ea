"""``PUSCHTransmitter`` - batches of 5G NR PUSCH slots for one or several transmitters (mirror of reference
src/sionna/phy/nr/pusch_transmitter.py:16-243).  After ``TBEncoder`` the reference runs the mapper, the layer mapper, the
resource-grid mapper and the precoder one after the other (:217-230); here they are ONE launch, ``samd_pusch_grid_c64``
(``_c128`` with ``precision="double"``, csrc/pusch.hip), which reads the scrambled coded bits and writes the precoded
grids.  The separate blocks stay available as attributes, and the fused launch equals their composition bit for bit."""
import numpy as np
import torch

from ... import _ffi
from ..block import Block, wrap
from ..mapping import BinarySource, Mapper
from ..ofdm.modulator import OFDMModulator
from ..ofdm.resource_grid import ResourceGrid, ResourceGridMapper
from .config import Config
from .layer_mapping import LayerMapper
from .pusch_config import PUSCHConfig, check_pusch_configs
from .pusch_pilot_pattern import PUSCHPilotPattern
from .pusch_precoder import PUSCHPrecoder
from .tb_encoder import TBEncoder


class PUSCHTransmitter(Block):
    """``PUSCHTransmitter(pusch_configs, return_bits=True, output_domain="freq", verbose=False)``:
    ``(batch_size) -> x, b`` with ``return_bits``, else ``(b [batch, num_tx, tb_size]) -> x``;
    x [batch, num_tx, num_antenna_ports, num_ofdm_symbols, num_subcarriers], or [..., num_time_samples] in the time domain."""

    def __init__(self, pusch_configs, return_bits=True, output_domain="freq", precision=None, verbose=False, **kwargs):
        super().__init__(precision=precision, **kwargs)
        assert isinstance(return_bits, bool), "return_bits must be bool"
        assert output_domain in ["time", "freq"], "output_domain must be 'time' or 'freq'"
        assert isinstance(verbose, bool), "verbose must be bool"
        self._return_bits, self._output_domain, self._verbose = return_bits, output_domain, verbose
        if isinstance(pusch_configs, PUSCHConfig):
            pusch_configs = [pusch_configs]
        for key, value in check_pusch_configs(pusch_configs).items():
            setattr(self, "_" + key, value)
        self._pusch_configs = pusch_configs
        if return_bits:
            self._binary_source = BinarySource(precision=self.precision)
        self._tb_encoder = TBEncoder(target_tb_size=self._tb_size, num_coded_bits=self._num_coded_bits,
                                     target_coderate=self._target_coderate, num_bits_per_symbol=self._num_bits_per_symbol,
                                     num_layers=self._num_layers, n_rnti=self._n_rnti, n_id=self._n_id, channel_type="PUSCH",
                                     codeword_index=0, use_scrambler=True, verbose=verbose, precision=self.precision)
        self._layer_mapper = LayerMapper(num_layers=self._num_layers, precision=self.precision)
        self._mapper = Mapper("qam", self._num_bits_per_symbol, precision=self.precision)
        self._pilot_pattern = PUSCHPilotPattern(self._pusch_configs, precision=self.precision)
        self._resource_grid = ResourceGrid(num_ofdm_symbols=self._num_ofdm_symbols, fft_size=self._num_subcarriers,
                                           subcarrier_spacing=self._subcarrier_spacing, num_tx=self._num_tx,
                                           num_streams_per_tx=self._num_layers,
                                           cyclic_prefix_length=self._cyclic_prefix_length,
                                           pilot_pattern=self._pilot_pattern, precision=self.precision)
        self._resource_grid_mapper = ResourceGridMapper(self._resource_grid, precision=self.precision)
        if self._precoding == "codebook":
            self._precoder = PUSCHPrecoder(self._precoding_matrices, precision=self.precision)
        if self._output_domain == "time":
            self._ofdm_modulator = OFDMModulator(self._cyclic_prefix_length, precision=self.precision)
        self._dev = None

    resource_grid = property(lambda self: self._resource_grid)
    pilot_pattern = property(lambda self: self._pilot_pattern)

    def show(self):
        """the carrier and PUSCH settings all transmitters share, then DMRS and transport block of each"""
        self._pusch_configs[0].carrier.show()
        Config.show(self._pusch_configs[0])
        for idx, p in enumerate(self._pusch_configs):
            print(f"---- UE {idx} ----")
            p.dmrs.show()
            p.tb.show()

    def _host_tables(self):
        """what the fused launch reads besides the bits, as host arrays: constellation points [2^m], pilots [S, num_pilots],
        data_pos / pilot_pos [S, num_re] (S = num_tx * num_layers, the tables of ``samd_rg_map_c64``) and the precoding
        matrices [num_tx, ports, layers] or None"""
        rg = self._resource_grid
        data_pos, pilot_pos = rg._positions()
        pilots = np.asarray(self._pilot_pattern.pilots).reshape(data_pos.shape[0], -1)
        w = None
        if self._precoding == "codebook":
            w = np.stack(self._precoding_matrices).astype(self._np_cdtype)
        return {"points": self._mapper.constellation.points.astype(self._np_cdtype), "pilots": pilots.astype(self._np_cdtype),
                "data_pos": data_pos, "pilot_pos": pilot_pos, "w": w}

    def _grid(self, c):
        """scrambled coded bits [batch, num_tx, num_coded_bits] -> x [batch, num_tx, ports, num_ofdm_symbols, fft_size]:
        mapper, layer mapper, resource-grid mapper and precoder in one launch"""
        if self._dev is None:
            t = self._host_tables()
            self._dev = {k: None if v is None else _ffi.to_device(v, torch.int32 if v.dtype == np.int32 else self.cdtype)
                         for k, v in t.items()}
        d = self._dev
        c = _ffi.to_device(c, torch.float32)
        if c.data_ptr() % 8:                                # a contiguous view at an odd offset: the kernel loads bit pairs
            c = c.clone()
        rg = self._resource_grid
        assert c.dim() == 3 and tuple(c.shape[1:]) == (self._num_tx, self._num_coded_bits), "unexpected shape of the coded bits"
        assert rg.num_data_symbols * self._num_layers * int(self._num_bits_per_symbol) == self._num_coded_bits
        ports = self._num_antenna_ports if d["w"] is not None else self._num_layers
        x = torch.empty((c.shape[0], self._num_tx, ports, rg.num_ofdm_symbols, rg.fft_size), dtype=self.cdtype, device=c.device)
        fn = _ffi.lib().samd_pusch_grid_c128 if self.precision == "double" else _ffi.lib().samd_pusch_grid_c64
        num_pilots = d["pilots"].shape[1]
        _ffi.check(fn(_ffi.ptr(c), _ffi.ptr(d["points"]), _ffi.ptr(d["pilots"]) if num_pilots else None, _ffi.ptr(d["data_pos"]),
                      _ffi.ptr(d["pilot_pos"]), _ffi.ptr(d["w"]), c.shape[0], self._num_tx, self._num_layers, ports,
                      d["data_pos"].shape[1], rg.num_data_symbols, num_pilots, int(self._num_bits_per_symbol), _ffi.ptr(x),
                      _ffi.stream()), "PUSCHTransmitter")
        return x

    def call(self, inputs):
        if self._return_bits:
            b = self._binary_source([inputs, self._num_tx, self._tb_size])
        else:
            b = inputs
        x = self._grid(self._tb_encoder(b))
        if self._output_domain == "time":
            x = self._ofdm_modulator(x)
        return (wrap(x), b) if self._return_bits else wrap(x)
