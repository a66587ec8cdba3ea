"""``PUSCHPilotPattern`` - the DMRS of one or several ``PUSCHConfig`` as a ``PilotPattern`` over the allocated OFDM
symbols (mirror of reference src/sionna/phy/nr/pusch_pilot_pattern.py:12-94): one transmitter per configuration, one
stream per layer; the masked resource elements of the CDM groups without data that a port does not use carry zeros."""
import warnings
from collections.abc import Sequence

import numpy as np

from ..ofdm.pilot_pattern import PilotPattern
from .pusch_config import PUSCHConfig


class PUSCHPilotPattern(PilotPattern):
    def __init__(self, pusch_configs, precision=None):
        if isinstance(pusch_configs, PUSCHConfig):
            pusch_configs = [pusch_configs]
        elif isinstance(pusch_configs, Sequence):
            for c in pusch_configs:
                assert isinstance(c, PUSCHConfig), "Each element of pusch_configs must be a valide PUSCHConfig"
        else:
            raise ValueError("Invalid value for pusch_configs")
        first = pusch_configs[0]
        num_layers, num_subcarriers, num_symbols = first.num_layers, first.num_subcarriers, first.l_d
        num_pilots = int(np.sum(first.dmrs_mask))
        used_ports = []
        for c in pusch_configs:
            assert c.num_layers == num_layers, "All pusch_configs must have the same number of layers"
            assert c.dmrs_grid[0].shape[0] == num_subcarriers, "All pusch_configs must have the same number of subcarriers"
            assert c.l_d == num_symbols, "All pusch_configs must have the same number of OFDM symbols"
            assert c.precoding == first.precoding, "All pusch_configs must have a the same precoding method"
            assert np.sum(c.dmrs_mask) == num_pilots, "All pusch_configs must have a the same number of masked REs"
            with warnings.catch_warnings():
                warnings.simplefilter("always")
                for port in c.dmrs.dmrs_port_set:
                    if port in used_ports:
                        warnings.warn(f"DMRS port {port} used by multiple transmitters")
            used_ports += c.dmrs.dmrs_port_set
        mask = np.zeros([len(pusch_configs), num_layers, num_symbols, num_subcarriers], bool)
        pilots = np.zeros([len(pusch_configs), num_layers, num_pilots], complex)
        for i, c in enumerate(pusch_configs):
            start, length = c.symbol_allocation
            mask[i] = c.dmrs_mask[:, start:start + length].T
            grid = c.dmrs_grid[:, :, start:start + length]
            for j in range(num_layers):
                pilots[i, j] = grid[j].T[mask[i, j]]
        super().__init__(mask, pilots, normalize=False, precision=precision)
